"""Times of the winding-number path on the device (HIP events; one JSON line on stdout, ``--out FILE`` to keep it).

Full-width generator, B = 1, synthetic weights, level 0.  Every step runs in a child process of its own under a time limit, one after
the other; the first step that fails, faults or runs out of time ends the run (its name and exit status are recorded).

- ``kernel``: ``ia_winding_number`` (``hipops.winding_number`` on packed triangles) against the 128^3 and the 256^3 mesh, for 1 000 and
  100 000 random points of the box and for the mesh's own vertices: time and point-triangle pairs per second.
- ``volume``: ``mesh_to_volume`` of the 128^3 mesh on lattices of 64 and 128 points along the longest axis, ``sign='regions'`` and
  ``sign='winding'`` (host clock, synchronised), with the evaluation counts of ``info``.  The mesh of a head is open at the neck, so
  ``'regions'`` is forced here to show its cost; its signs are only right for a closed mesh.
- ``signed``: ``signed_distance`` end to end (grid given) for 100 000 points against the 256^3 mesh.
- ``torch``: the yardstick, the same formula through chunked PyTorch device ops (float32 terms, float64 sum), 10 000 points against
  the 128^3 mesh, with its largest difference from the kernel.
Every time is the median of the timed runs after warm-up, with the smallest and largest beside it.
Usage: python tools/bench_winding.py [--out FILE] [--steps kernel,volume,signed,torch]"""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_surface_distance import mesh_at, setup, spread, timed        # noqa: E402

STEPS = {'kernel': 400, 'volume': 400, 'signed': 240, 'torch': 300}       # step -> seconds


def mesh(n):
    from invertavatar_amd import geometry
    g, planes = setup()
    vol, lo, step = mesh_at(g, planes, n)
    return geometry.marching_cubes(vol, 0.0, lo, step)


def box_points(verts, n, seed=0):
    import torch
    gen = torch.Generator().manual_seed(seed)
    lo, hi = verts.amin(0), verts.amax(0)
    return (lo + (hi - lo) * torch.rand(n, 3, generator=gen).to(verts.device)).contiguous()


def with_rate(t, pairs):
    return dict(t, pairs=pairs, gpairs_per_s=round(pairs / (t['ms'] * 1e-3) / 1e9, 3))


def step_kernel():
    from invertavatar_amd import geometry, hipops
    r = {}
    for n in (128, 256):
        v, f = mesh(n)
        grid = geometry.TriangleGrid(v, f, build=False)
        faces = int(f.shape[0])
        row = dict(faces=faces, vertices=int(v.shape[0]))
        for name, pts in (('n1k', box_points(v, 1000)), ('n100k', box_points(v, 100000)), ('vertices', v.contiguous())):
            reps = 3 if pts.shape[0] * faces > 2e10 else 7
            row[name] = with_rate(timed(lambda: hipops.winding_number(pts, grid.tris), warmup=1, reps=reps), int(pts.shape[0]) * faces)
        r[f'mesh{n}'] = row
    return r


def step_volume():
    import torch
    from invertavatar_amd import geometry
    v, f = mesh(128)
    r = dict(faces=int(f.shape[0]))
    for res in (64, 128):
        for sign in ('regions', 'winding'):
            ts = []
            for _ in range(1 + 3):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                out = geometry.mesh_to_volume(v, f, res, sign=sign)
                torch.cuda.synchronize()
                ts.append((time.perf_counter() - t0) * 1e3)
            r[f'res{res}_{sign}'] = dict(end_to_end_host_clock=spread(ts[1:]), lattice=list(out['inside'].shape), info=out['info'],
                                         inside_points=int(out['inside'].sum()))
    return r


def step_signed():
    from invertavatar_amd import geometry
    v, f = mesh(256)
    grid = geometry.TriangleGrid(v, f)
    pts = box_points(v, 100000)
    return dict(points=100000, faces=int(f.shape[0]), signed_distance=timed(lambda: geometry.signed_distance(pts, v, f, grid=grid), warmup=1, reps=5),
                closest_alone=timed(lambda: grid.closest(pts), warmup=1, reps=5))


def torch_winding(pts, tris, pairs=1 << 24):
    """The formula of csrc/winding.hip through PyTorch device ops: float32 terms, a float64 sum per point (torch's own order)."""
    import math
    import torch
    A, B, C = tris[:, 0, :3], tris[:, 1, :3], tris[:, 2, :3]
    use = tris[:, 0, 3] != 0
    A, B, C = A[use], B[use], C[use]
    out = torch.empty(pts.shape[0], dtype=torch.float64, device=pts.device)
    step = max(1, pairs // max(A.shape[0], 1))
    for s in range(0, pts.shape[0], step):
        p = pts[s:s + step, None, :]
        a, b, c = A[None] - p, B[None] - p, C[None] - p
        num = (a * torch.cross(b - a, c - a, dim=-1)).sum(-1)
        la, lb, lc = a.norm(dim=-1), b.norm(dim=-1), c.norm(dim=-1)
        den = la * lb * lc + (a * b).sum(-1) * lc + (b * c).sum(-1) * la + (c * a).sum(-1) * lb
        out[s:s + step] = (2 * torch.atan2(num, den)).sum(-1, dtype=torch.float64) / (4 * math.pi)
    return out


def step_torch():
    from invertavatar_amd import geometry, hipops
    v, f = mesh(128)
    grid = geometry.TriangleGrid(v, f, build=False)
    pts = box_points(v, 10000)
    pairs = 10000 * int(f.shape[0])
    diff = float((torch_winding(pts, grid.tris) - hipops.winding_number(pts, grid.tris)).abs().max())
    return dict(points=10000, faces=int(f.shape[0]), torch_ops=with_rate(timed(lambda: torch_winding(pts, grid.tris), warmup=1, reps=3), pairs),
                kernel=with_rate(timed(lambda: hipops.winding_number(pts, grid.tris), warmup=1, reps=3), pairs), largest_difference=diff)


def main():
    if '--step' in sys.argv:                                                      # child: one step, one JSON line
        name = sys.argv[sys.argv.index('--step') + 1]
        print('RESULT ' + json.dumps({'kernel': step_kernel, 'volume': step_volume, 'signed': step_signed, 'torch': step_torch}[name]()))
        return
    from invertavatar_amd import build as ia_build
    out_path = sys.argv[sys.argv.index('--out') + 1] if '--out' in sys.argv else None
    steps = sys.argv[sys.argv.index('--steps') + 1].split(',') if '--steps' in sys.argv else list(STEPS)
    res = {'source_digest': ia_build.source_digest(), 'level': 0.0}
    for name in steps:
        try:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), '--step', name], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                               timeout=STEPS[name], text=True)
        except subprocess.TimeoutExpired:
            res['stopped_at'] = dict(step=name, reason=f'no result within {STEPS[name]} s')
            break
        lines = [ln for ln in p.stdout.splitlines() if ln.startswith('RESULT ')]
        if p.returncode != 0 or not lines:
            res['stopped_at'] = dict(step=name, returncode=p.returncode, stderr=p.stderr[-600:])
            break
        res[name] = json.loads(lines[-1][len('RESULT '):])
    line = json.dumps(res)
    print(line)
    if out_path:
        with open(out_path, 'w') as fh:
            fh.write(line + '\n')
    sys.exit(1 if 'stopped_at' in res else 0)


if __name__ == '__main__':
    main()
