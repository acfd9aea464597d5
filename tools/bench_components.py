"""Times of the connected-components path on the device (HIP events; one JSON line on stdout).

Full-width generator, B = 1, synthetic weights, level 0 (so that a surface exists), density volumes of 256^3 and 512^3:
- ``ia_density_grid`` at the same resolution, from the same run (what producing the volume costs);
- labelling (``ia_volume_components``, 26- and 6-connectivity), statistics (``ia_component_stats``) and the filter (``ia_volume_keep``);
  K and the largest component's share of the inside points;
- the host route they replace: device-to-host copy + ``scipy.ndimage.label`` + copy of the labels back (or a note that scipy is absent);
- mesh labelling (``ia_mesh_components`` + statistics) of the marching-cubes mesh;
- ``extract_geometry`` end to end with and without ``keep='largest'`` (host clock around a synchronised call, alternating).
Every time is the median of ``REPS`` timed runs after warm-up, with the smallest and largest beside it.
Usage: python tools/bench_components.py [--out FILE]"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from invertavatar_amd import build as ia_build, geometry, hipops, synthetic  # noqa: E402
from invertavatar_amd.training_avatar_texture.triplane_v20 import TriPlaneGenerator  # noqa: E402

REPS = 9


def spread(ts):
    ts = sorted(ts)
    return dict(ms=round(ts[len(ts) // 2], 4), min_ms=round(ts[0], 4), max_ms=round(ts[-1], 4), reps=len(ts))


def timed(fn, warmup=2, reps=REPS):
    """Per-call HIP-event times of ``fn``."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    return spread(ts)


def host_timed(fn, warmup=1, reps=3):
    """Host clock around calls that end synchronised."""
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return spread(ts)


def main():
    out_path = sys.argv[sys.argv.index('--out') + 1] if '--out' in sys.argv else None
    assert torch.cuda.is_available(), 'bench_components needs the GPU'
    g = synthetic.fill_parameters(TriPlaneGenerator(**synthetic.generator_kwargs('full')).eval().requires_grad_(False)).cuda()
    bw = g.rendering_kwargs['box_warp']
    res = {'source_digest': ia_build.source_digest(), 'level': 0.0, 'reps': REPS}
    try:
        from scipy import ndimage
    except ImportError:
        ndimage = None
        res['host_route'] = 'scipy is not installed on this machine: the host route was not measured'
    with torch.no_grad():
        ws = g.mapping(synthetic.latent(0, 1).cuda(), synthetic.conditioning_camera().cuda(), truncation_psi=0.7, truncation_cutoff=14)
        mesh = {'uvcoords_image': synthetic.uv_conditions([0]).cuda()}
        planes = geometry.generator_planes(g, ws, mesh, noise_mode='const')
        for n in (256, 512):
            r = {}
            r['density_grid'] = timed(lambda: geometry.density_volume(planes, g.decoder, n, bw, box_warp=bw), reps=5)
            vol = geometry.density_volume(planes, g.decoder, n, bw, box_warp=bw)[0].contiguous()
            labels, k = hipops.volume_components(vol, 0.0, 26)
            stats = hipops.component_stats(labels, k)
            inside = int(stats[:, 0].sum())
            r.update(K=k, inside_points=inside, largest_share=round(float(stats[:, 0].max()) / max(inside, 1), 6),
                     K_6=hipops.volume_components(vol, 0.0, 6)[1])
            r['label_26'] = timed(lambda: hipops.volume_components(vol, 0.0, 26))          # includes the host read of K
            r['label_6'] = timed(lambda: hipops.volume_components(vol, 0.0, 6))
            r['stats'] = timed(lambda: hipops.component_stats(labels, k))
            flags = torch.zeros(k + 1, dtype=torch.uint8)
            flags[geometry.select_components(stats)] = 1
            flags = flags.cuda()
            out = torch.empty_like(vol)
            r['keep'] = timed(lambda: hipops.volume_keep(vol, labels, flags, 0.0, out=out))
            r['keep_components_total'] = host_timed(lambda: geometry.keep_components(vol, 0.0, 'largest'), reps=5)
            if ndimage is not None:
                def host_route():
                    lab, _ = ndimage.label(vol.cpu().numpy() > np.float32(0.0), structure=np.ones((3, 3, 3)))
                    return torch.from_numpy(lab).cuda()
                r['host_scipy_label_round_trip'] = host_timed(host_route, warmup=1, reps=3 if n == 256 else 2)
            _, lo, step = geometry.lattice_axis(n, bw, 0.0)
            verts, faces = geometry.marching_cubes(out, 0.0, (float(lo),) * 3, (float(step),) * 3)
            v_all, f_all = geometry.marching_cubes(vol, 0.0, (float(lo),) * 3, (float(step),) * 3)
            f32 = f_all.to(torch.int32).contiguous()
            vl, mk = hipops.mesh_components(f32, v_all.shape[0])
            r['mesh'] = dict(verts=int(v_all.shape[0]), faces=int(f_all.shape[0]), K=mk, faces_after_keep_largest=int(faces.shape[0]),
                             label=timed(lambda: hipops.mesh_components(f32, v_all.shape[0])),
                             stats=timed(lambda: hipops.mesh_component_stats(f32, vl, mk)))
            del verts, faces, v_all, f_all, f32, vl, labels, out
            if n == 256:
                kw = dict(resolution=256, level=0.0, with_colors=True, noise_mode='const')
                plain, kept = [], []
                for fn in (lambda: g.extract_geometry(ws, mesh, **kw), lambda: g.extract_geometry(ws, mesh, keep='largest', **kw)):
                    fn()
                for _ in range(REPS):                                                    # alternating, same run
                    for ts, keep in ((plain, None), (kept, 'largest')):
                        torch.cuda.synchronize()
                        t0 = time.perf_counter()
                        g.extract_geometry(ws, mesh, keep=keep, **kw)
                        torch.cuda.synchronize()
                        ts.append((time.perf_counter() - t0) * 1e3)
                r['extract_geometry'] = dict(plain=spread(plain), keep_largest=spread(kept),
                                             ratio=round(spread(kept)['ms'] / spread(plain)['ms'], 3))
            res[f'volume_{n}'] = r
    line = json.dumps(res)
    print(line)
    if out_path:
        with open(out_path, 'w') as fh:
            fh.write(line + '\n')


if __name__ == '__main__':
    main()
