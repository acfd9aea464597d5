"""Kernel times of the surface ray caster (HIP events; one JSON line on stdout).

Full-width generator, B = 1, synthetic weights, level 0 (so that a surface exists), a 256^3 density volume:
- ia_volume_bricks on it;
- one 512^2 view (the generator's ray sampler, frontal camera) with brick skipping and on the dense path;
- a 36-view yaw orbit (512^2 each) in one launch;
- ``volume_normals`` (ia_volume_gradient) at the vertices of the 256^3 marching-cubes mesh.
Usage: python tools/bench_raycast.py [--out FILE]"""
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))

import torch  # noqa: E402

from invertavatar_amd import build as ia_build, geometry, hipops, synthetic  # noqa: E402
from invertavatar_amd.extract_geometry import orbit_cameras  # noqa: E402
from invertavatar_amd.training_avatar_texture.triplane_v20 import TriPlaneGenerator  # noqa: E402


def timed(fn, warmup=2, reps=10):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def main():
    out_path = sys.argv[sys.argv.index('--out') + 1] if '--out' in sys.argv else None
    assert torch.cuda.is_available(), 'bench_raycast needs the GPU'
    g = synthetic.fill_parameters(TriPlaneGenerator(**synthetic.generator_kwargs('full')).eval().requires_grad_(False)).cuda()
    bw = g.rendering_kwargs['box_warp']
    res = {'source_digest': ia_build.source_digest(), 'volume': 256, 'level': 0.0}
    with torch.no_grad():
        ws = g.mapping(synthetic.latent(0, 1).cuda(), synthetic.conditioning_camera().cuda(), truncation_psi=0.7, truncation_cutoff=14)
        mesh = {'uvcoords_image': synthetic.uv_conditions([0]).cuda()}
        planes = geometry.generator_planes(g, ws, mesh, noise_mode='const')
        vol = geometry.density_volume(planes, g.decoder, 256, bw, box_warp=bw)[0].contiguous()
        _, lo, step = geometry.lattice_axis(256, bw, 0.0)
        lo3, step3 = (float(lo),) * 3, (float(step),) * 3
        bricks = hipops.volume_bricks(vol)
        res['bricks'] = dict(ms=round(timed(lambda: hipops.volume_bricks(vol)), 4), grid=list(bricks.shape[:3]),
                             frac_skippable=round(float((bricks[..., 1] <= 0.0).float().mean()), 4))
        cams = orbit_cameras(g, 36, device='cuda')
        o36, d36 = hipops.ray_sampler(cams, 512)
        o36, d36 = o36.reshape(-1, 3).contiguous(), d36.reshape(-1, 3).contiguous()
        n1 = 512 * 512
        o1, d1 = o36[:n1].contiguous(), d36[:n1].contiguous()
        skip = hipops.raycast_volume(vol, 0.0, lo3, step3, o1, d1, 0.0, bricks)
        dense = hipops.raycast_volume(vol, 0.0, lo3, step3, o1, d1, 0.0, None)
        same = all(torch.equal(a, b) for a, b in zip(skip, dense))
        ms_skip = timed(lambda: hipops.raycast_volume(vol, 0.0, lo3, step3, o1, d1, 0.0, bricks))
        ms_dense = timed(lambda: hipops.raycast_volume(vol, 0.0, lo3, step3, o1, d1, 0.0, None))
        res['view_512'] = dict(skip_ms=round(ms_skip, 4), dense_ms=round(ms_dense, 4), dense_over_skip=round(ms_dense / ms_skip, 2),
                               hit_pixels=int(skip[2].sum()), skip_equals_dense=same, mrays_per_s_skip=round(n1 / ms_skip / 1e3, 1))
        ms36 = timed(lambda: hipops.raycast_volume(vol, 0.0, lo3, step3, o36, d36, 0.0, bricks), warmup=1, reps=5)
        hits36 = int(hipops.raycast_volume(vol, 0.0, lo3, step3, o36, d36, 0.0, bricks)[2].sum())
        res['orbit_36x512'] = dict(ms=round(ms36, 3), ms_per_view=round(ms36 / 36, 4), hit_pixels=hits36,
                                   mrays_per_s=round(36 * n1 / ms36 / 1e3, 1))
        verts, faces = geometry.marching_cubes(vol, 0.0, lo3, step3)
        ms_n = timed(lambda: geometry.volume_normals(vol, verts, lo3, step3))
        ms_g = timed(lambda: hipops.volume_gradient(vol, lo3, step3, verts))
        res['volume_normals_256'] = dict(verts=int(verts.shape[0]), ms=round(ms_n, 4), gradient_kernel_ms=round(ms_g, 4))
    line = json.dumps(res)
    print(line)
    if out_path:
        with open(out_path, 'w') as fh:
            fh.write(line + '\n')


if __name__ == '__main__':
    main()
