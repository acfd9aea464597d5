"""Times of the mesh rasteriser on the device, per stage (one JSON line on stdout, kept in profiles/mesh_raster_bench.json).

The marching-cubes mesh of an analytic sphere (density = 0.3 - |x| on a ``--volume``^3 lattice over the unit cube, level 0) from 1 and 8
cameras of a yaw orbit at radius 2.7, 512^2: seconds per stage of ``geometry.rasterize_mesh`` (project, raster, resolve; each stage ends in
a device synchronise, ``hipops.MESH_RASTER_TIMES``), the whole call between two device events, and the same with every triangle on the
wave path (``oversize_pixels=0``) and none (``2**30``).  Median and range of ``--reps`` runs after one warm-up.
Usage: python tools/bench_mesh_raster.py [--volume 256] [--res 512] [--reps 5] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')
sys.path.insert(0, ROOT)


def spread(xs):
    return {'ms': round(statistics.median(xs), 4), 'min': round(min(xs), 4), 'max': round(max(xs), 4), 'n': len(xs)}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--volume', type=int, default=256)
    ap.add_argument('--res', type=int, default=512)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'mesh_raster_bench.json'))
    args = ap.parse_args(argv)
    import numpy as np
    import torch
    from invertavatar_amd import build, geometry, hipops
    from invertavatar_amd.training_avatar_texture.camera_utils import FOV_to_intrinsics, LookAtPoseSampler
    dev = 'cuda'
    ax, lo, step = geometry.lattice_axis(args.volume, 1.0, 0.0)
    a = torch.from_numpy(ax).to(dev)
    vol = 0.3 - torch.sqrt(a[:, None, None] ** 2 + a[None, :, None] ** 2 + a[None, None, :] ** 2)
    v, f = geometry.marching_cubes(vol, 0.0, (float(lo),) * 3, (float(step),) * 3)[:2]
    f = f.int().contiguous()
    nrm = torch.nn.functional.normalize(v, dim=1).contiguous()
    K = FOV_to_intrinsics(18.837, device=dev).reshape(1, 9)
    result = {'device': torch.cuda.get_device_name(0), 'source_digest': build.source_digest(), 'volume': args.volume, 'resolution': args.res,
              'verts': int(v.shape[0]), 'faces': int(f.shape[0]), 'views': {}}
    for n in (1, 8):
        cams = torch.cat([torch.cat([LookAtPoseSampler.sample(np.pi / 2 + 2 * np.pi * k / n, np.pi / 2, torch.zeros(3, device=dev), radius=2.7,
                                                              device=dev).reshape(1, 16), K], 1) for k in range(n)]).contiguous()
        r = {}
        for name, kw in (('default', {}), ('all_wave', {'oversize_pixels': 0}), ('none_wave', {'oversize_pixels': 2 ** 30})):
            call = lambda: geometry.rasterize_mesh(v, f, cams, args.res, normals=nrm, attributes=nrm, **kw)
            out = call()
            stages, whole = {}, []
            for _ in range(args.reps):
                hipops.MESH_RASTER_TIMES = {}
                call()
                for k, x in hipops.MESH_RASTER_TIMES.items():
                    stages.setdefault(k, []).append(x * 1e3)
                hipops.MESH_RASTER_TIMES = None
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                call()
                e1.record()
                e1.synchronize()
                whole.append(e0.elapsed_time(e1))
            r[name] = {'stages': {k: spread(x) for k, x in stages.items()}, 'whole_call': spread(whole),
                       'surface_pixels': int(out['mask'].sum()), 'culled': int(out['culled'].sum())}
        result['views'][str(n)] = r
    line = json.dumps(result)
    print(line)
    with open(args.out, 'w') as fh:
        fh.write(line + '\n')


if __name__ == '__main__':
    main()
