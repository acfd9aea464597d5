"""Times the TSDF integration (csrc/tsdf.hip): a 256^3 lattice, 36 views at 512^2 of a sphere of radius 0.4 seen from
an orbit at radius 2.2 (analytic ray-parameter depth, the normal as colour).  Not part of bench.py; the recorded run is
profiles/fuse_depth_bench.json.

- ``kernel``: ``ia_tsdf_integrate`` alone through the project's phase timer (``hipops.PROFILE``: device events around the launch),
  without colours and with 3 channels; median, smallest and largest of the timed launches after warm-up.
- ``torch``: a straightforward per-view PyTorch formulation of the same definition on the device (N passes over the volume, a dozen
  temporaries each), device events; its ``tsdf`` must agree with the kernel's to 1e-5 (it contracts nothing on purpose, but PyTorch's
  kernels are free to), else the tool exits non-zero.
- ``floor``: the larger of traffic over 6.3 TB/s (the lattice planes written once, every depth / colour image read once) and arithmetic
  over 157.3 TFLOP/s fp32 (about 40 operations per point and view, counted from the definition: 3 + 15 + 10 + 2 divisions at 1 + the
  square root and the sums), and the kernel's share of it.  Which of the two bounds is recorded.
- ``end_to_end``: ``geometry.fuse_depth`` and ``fused_mesh``, host clock around a synchronise.

Usage: python tools/bench_fuse_depth.py [--out FILE] [--res 256] [--views 36] [--image 512]"""
import json
import os
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_surface_distance import spread, timed                 # noqa: E402

HBM = 6.3e12                 # bytes / s, measured streaming rate of the MI355X
FP32 = 157.3e12              # fp32 vector operations / s
OPS_PER_POINT_VIEW = 40.0
RADIUS = 0.4


def arg(name, default):
    return int(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def scene(n_views, size, device):
    """(cameras [N,25], depth [N,H,W], colors [N,3,H,W]) on the device: the analytic sphere."""
    import numpy as np
    import torch
    from invertavatar_amd.training_avatar_texture.camera_utils import FOV_to_intrinsics, LookAtPoseSampler
    from invertavatar_amd.training_avatar_texture.volumetric_rendering.ray_sampler import RaySampler_zxc
    K = FOV_to_intrinsics(36.0).reshape(1, 9)
    poses = [LookAtPoseSampler.sample(np.pi / 2 + 2 * np.pi * k / n_views, np.pi / 2 + 0.6 * np.sin(1.7 * k), torch.zeros(3), radius=2.2)
             for k in range(n_views)]
    cams = torch.cat([torch.cat([p.reshape(1, 16), K], 1) for p in poses]).to(device)
    with torch.no_grad():
        o, d = RaySampler_zxc()(cams[:, :16].reshape(-1, 4, 4), cams[:, 16:].reshape(-1, 3, 3), size)
    b = (o * d).sum(-1)
    disc = b * b - ((o * o).sum(-1) - RADIUS * RADIUS)
    t = torch.where(disc > 0, -b - disc.clamp(min=0).sqrt(), torch.zeros_like(b))
    normal = (o + t[..., None] * d) / RADIUS
    depth = t.reshape(n_views, size, size).contiguous()
    colors = (normal * 0.5 + 0.5).reshape(n_views, size, size, 3).permute(0, 3, 1, 2).contiguous() * (depth > 0)[:, None]
    return cams, depth, colors.contiguous()


def torch_fuse(depth, views, axes, tau, near):
    """The definition view by view in PyTorch (no colours): (sum, weight, tsdf) [nx,ny,nz]."""
    import torch
    N, H, W = depth.shape
    X, Y, Z = torch.meshgrid(*axes, indexing='ij')
    F, Wt = torch.zeros_like(X), torch.zeros_like(X)
    for n in range(N):
        v = views[n]
        dx, dy, dz = X - v[9], Y - v[10], Z - v[11]
        xx = (v[0] * dx + v[3] * dy) + v[6] * dz
        xy = (v[1] * dx + v[4] * dy) + v[7] * dz
        xz = (v[2] * dx + v[5] * dy) + v[8] * dz
        u = ((v[12] * xx + v[13] * xy) + v[14] * xz) / xz
        w = ((v[15] * xx + v[16] * xy) + v[17] * xz) / xz
        fi, fj = torch.round(u), torch.round(w)
        ok = torch.isfinite(xz) & (xz > near) & torch.isfinite(u) & torch.isfinite(w) & (fi >= 0) & (fi <= W - 1) & (fj >= 0) & (fj <= H - 1)
        q = torch.where(ok, fj * W + fi, torch.zeros_like(fi)).long()
        t = depth[n].reshape(-1)[q]
        s = t - torch.sqrt((dx * dx + dy * dy) + dz * dz)
        ok &= torch.isfinite(t) & (t > 0) & ~(s < -tau)
        F = torch.where(ok, F + torch.clamp(s / tau, max=1.0), F)
        Wt = torch.where(ok, Wt + 1.0, Wt)
    return F, Wt, torch.where(Wt > 0, F / torch.where(Wt > 0, Wt, torch.ones_like(Wt)), torch.ones_like(Wt))


def main():
    import numpy as np
    import torch
    from invertavatar_amd import build as ia_build, geometry, hipops
    if not torch.cuda.is_available():
        raise SystemExit('bench_fuse_depth needs a GPU: nothing is measured without one')
    res_n, n_views, size = arg('--res', 256), arg('--views', 36), arg('--image', 512)
    out_path = sys.argv[sys.argv.index('--out') + 1] if '--out' in sys.argv else None
    dev = torch.device('cuda')
    cams, depth, colors = scene(n_views, size, dev)
    dims, origin = (res_n,) * 3, (-0.6,) * 3
    spacing = (1.2 / (res_n - 1),) * 3
    tau, near = float(np.float32(3 * spacing[0])), 1e-6
    R, o, k = geometry._camera_numpy(cams.cpu().numpy(), size, size, np.float32)
    views = torch.from_numpy(np.concatenate([R.reshape(n_views, 9), o, k], 1).astype(np.float32)).to(dev)
    points = res_n ** 3
    res = {'source_digest': ia_build.source_digest(), 'lattice': list(dims), 'views': n_views, 'image': [size, size], 'truncation': tau}

    def kernel_times(cols):
        run = lambda: hipops.tsdf_integrate(depth, views, dims, origin, spacing, tau, near, colors=cols)
        for _ in range(3):
            run()
        torch.cuda.synchronize()
        hipops.PROFILE = []
        try:
            for _ in range(15):
                run()
            torch.cuda.synchronize()
            ts = [e0.elapsed_time(e1) for fam, _, _, e0, e1, _ in hipops.PROFILE if fam == 'tsdf_integrate']
        finally:
            hipops.PROFILE = None
        return spread(ts)

    for name, cols, c in (('kernel', None, 0), ('kernel_rgb', colors, 3)):
        r = kernel_times(cols)
        planes = 3 + (c + 1 if c else 0)
        traffic = 4.0 * points * planes + 4.0 * n_views * size * size * (1 + c)
        t_mem, t_alu = traffic / HBM, OPS_PER_POINT_VIEW * points * n_views / FP32
        floor_ms = max(t_mem, t_alu) * 1e3
        r.update(floor_ms=round(floor_ms, 4), bound='arithmetic' if t_alu > t_mem else 'traffic', share_of_floor=round(floor_ms / r['ms'], 4),
                 traffic_bytes=traffic, operations=OPS_PER_POINT_VIEW * points * n_views)
        res[name] = r
    axes = [torch.from_numpy(a).to(dev) for a in geometry._lattice_axes(dims, origin, spacing)]
    with torch.no_grad():
        res['torch'] = timed(lambda: torch_fuse(depth, views, axes, tau, near), warmup=1, reps=3)
        ref = torch_fuse(depth, views, axes, tau, near)[2]
    got = hipops.tsdf_integrate(depth, views, dims, origin, spacing, tau, near)['tsdf']
    res['torch']['max_abs_difference'] = float((got - ref).abs().max())
    res['ratio_torch_over_kernel'] = round(res['torch']['ms'] / res['kernel']['ms'], 2)

    def end_to_end():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fusion = geometry.fuse_depth(depth, cams, dims, origin, spacing, colors=colors)
        mesh = geometry.fused_mesh(fusion, with_colors=True)
        torch.cuda.synchronize()
        return fusion, mesh, (time.perf_counter() - t0) * 1e3
    end_to_end()
    runs = [end_to_end() for _ in range(3)]
    fusion, mesh = runs[-1][0], runs[-1][1]
    dist = (mesh[0].double().norm(dim=1) - RADIUS).abs()
    res['end_to_end'] = dict(spread([r[2] for r in runs]), observed=fusion['info']['observed'], band=fusion['info']['band'],
                             vertices=int(mesh[0].shape[0]), faces=int(mesh[1].shape[0]), mean_distance_to_sphere=float(dist.mean()),
                             max_distance_to_sphere=float(dist.max()), spacing=spacing[0])
    line = json.dumps(res)
    print(line)
    if out_path:
        with open(out_path, 'w') as fh:
            fh.write(line + '\n')
    sys.exit(0 if res['torch']['max_abs_difference'] <= 1e-5 else 1)


if __name__ == '__main__':
    main()
