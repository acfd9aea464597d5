"""Times of the closest-point query on the cluster tree against the uniform grid (HIP events; one JSON line on stdout, ``--out FILE``
to keep it; the recorded run is profiles/closest_tree_bench.json).

Full-width generator, B = 1, synthetic weights, level 0 (the meshes of tools/bench_winding.py).  Every step runs in a child process of
its own under a time limit, one after the other; the first step that fails, faults or runs out of time ends the run.  Every case that
is timed is also compared: tree and grid (and brute, where it runs) must give the same bits, or the step fails.

- ``build``: ``hipops.tree_boxes`` (the box table) of the 128^3 and the 256^3 mesh, beside the build of the tree it sits on.
- ``query``: ``WindingTree.closest`` (with its point sort) against ``TriangleGrid.closest`` (with its own), and the brute mode where it is
  below 1e10 pairs, for the mesh's own vertices, 100 000 and 1 000 random points of the box and, the far case, 1 000 and 100 000
  points on a sphere of 10 times the extent around the middle of the box: times and the mean boxes and pairs per point.  The grid
  walks every cell for a far point: it is run once on the 1 000, and the 100 000 are compared with one run of the brute mode.
- ``callers``: ``signed_distance`` of 100 000 box points against the 256^3 mesh (``method='tree'``), ``mesh_to_volume`` of the 128^3 mesh
  on lattices of 64 and 128 points (``winding='tree'``) and ``align_mesh`` of 20 000 vertices of the 128^3 mesh from a displaced start
  (``init='identity'``, 10 iterations), each with ``search='grid'`` and ``'tree'`` (host clock, synchronised).
Every time is the median of the timed runs after warm-up, with the smallest and largest beside it.
Usage: python tools/bench_closest_tree.py [--out FILE] [--steps build,query,callers]"""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_surface_distance import spread, timed        # noqa: E402
from bench_winding import box_points, mesh              # noqa: E402

STEPS = {'build': 240, 'query': 420, 'callers': 420}     # step -> seconds
BRUTE_PAIRS = 1e10


def same_bits(a, b):
    import torch
    return all(torch.equal(a[k].view(torch.int32) if a[k].dtype == torch.float32 else a[k], b[k].view(torch.int32) if b[k].dtype == torch.float32
                           else b[k]) for k in ('dist', 'face', 'point'))


def shell_points(verts, n, factor=10.0, seed=1):
    """``n`` points on the sphere of ``factor`` times the extent around the middle of the box."""
    import torch
    gen = torch.Generator().manual_seed(seed)
    d = torch.randn(n, 3, generator=gen, dtype=torch.float64)
    d = d / d.norm(dim=1, keepdim=True)
    lo, hi = verts.amin(0).double().cpu(), verts.amax(0).double().cpu()
    extent = float(torch.maximum(lo.abs(), hi.abs()).max())
    return ((lo + hi) / 2 + factor * extent * d).float().to(verts.device).contiguous()


def host_clock(fn, reps=3):
    import torch
    ts = []
    for _ in range(1 + reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return out, spread(ts[1:])


def step_build():
    from invertavatar_amd import geometry, hipops
    r = {}
    for n in (128, 256):
        v, f = mesh(n)
        grid = geometry.TriangleGrid(v, f, build=False)
        tree = geometry.WindingTree.from_grid(grid)
        nodes = int(sum(tree.counts))
        r[f'mesh{n}'] = dict(info=tree.info, boxes=timed(lambda: hipops.tree_boxes(tree.tris, tree.usable, nodes), warmup=1, reps=7),
                             tree=timed(lambda: geometry.WindingTree.from_grid(grid), warmup=1, reps=5),
                             grid=timed(lambda: geometry.TriangleGrid(v, f), warmup=1, reps=5))
    return r


def once(fn):
    """(result, {'ms': ...}) of one run under HIP events: for the runs that are too long to repeat, timed as they are compared."""
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    return out, spread([e0.elapsed_time(e1)])


def step_query():
    from invertavatar_amd import geometry
    r = {}
    for n in (128, 256):
        v, f = mesh(n)
        grid = geometry.TriangleGrid(v, f)
        tree = geometry.WindingTree.from_grid(grid)
        tree.boxes
        faces = int(f.shape[0])
        row = dict(faces=faces, vertices=int(v.shape[0]), grid_cells=list(grid.dims))
        for name, pts in (('vertices', v.contiguous()), ('n100k', box_points(v, 100000)), ('n1k', box_points(v, 1000)),
                          ('far1k', shell_points(v, 1000)), ('far100k', shell_points(v, 100000))):
            by_tree = tree.closest(pts, return_counts=True)
            cnt = by_tree['counts'].double()
            cell = dict(points=int(pts.shape[0]), tree=timed(lambda: tree.closest(pts), warmup=1, reps=7),
                        boxes_per_point=float(cnt[:, 0].mean()), pairs_per_point=float(cnt[:, 1].mean()), most_pairs=int(cnt[:, 1].max()))
            if name == 'far100k':                                                 # (the grid walks every cell for each of them: far1k has it)
                by_brute, cell['brute'] = once(lambda: grid.closest(pts, brute=True))
                if not same_bits(by_tree, by_brute):
                    raise SystemExit(f'mesh{n} {name}: tree and brute differ')
            else:
                by_grid, first = once(lambda: grid.closest(pts))
                if not same_bits(by_tree, by_grid):
                    raise SystemExit(f'mesh{n} {name}: tree and grid differ')
                cell['grid'] = first if name == 'far1k' else timed(lambda: grid.closest(pts), warmup=0, reps=5)
                if pts.shape[0] * faces <= BRUTE_PAIRS:
                    by_brute, first = once(lambda: grid.closest(pts, brute=True))
                    if not same_bits(by_tree, by_brute):
                        raise SystemExit(f'mesh{n} {name}: tree and brute differ')
                    cell['brute'] = first if name == 'far1k' else timed(lambda: grid.closest(pts, brute=True), warmup=0, reps=3)
            row[name] = cell
        r[f'mesh{n}'] = row
    return r


def step_callers():
    import numpy as np
    import torch
    from invertavatar_amd import geometry
    r = {}
    v, f = mesh(256)
    pts = box_points(v, 100000)
    out = {}
    for search in ('grid', 'tree'):
        out[search], t = host_clock(lambda: geometry.signed_distance(pts, v, f, method='tree', search=search))
        r[f'signed_distance_100k_mesh256_{search}'] = dict(end_to_end_host_clock=t, faces=int(f.shape[0]))
    if not (same_bits(out['grid'], out['tree']) and torch.equal(out['grid']['sdf'].view(torch.int32), out['tree']['sdf'].view(torch.int32))):
        raise SystemExit('signed_distance: tree and grid differ')
    del v, f, pts, out
    v, f = mesh(128)
    for res in (64, 128):
        out = {}
        for search in ('grid', 'tree'):
            out[search], t = host_clock(lambda: geometry.mesh_to_volume(v, f, res, winding='tree', search=search))
            r[f'mesh_to_volume_{res}_mesh128_{search}'] = dict(end_to_end_host_clock=t, lattice=list(out[search]['sdf'].shape),
                                                               info=out[search]['info'])
        if not torch.equal(out['grid']['sdf'].view(torch.int32), out['tree']['sdf'].view(torch.int32)):
            raise SystemExit(f'mesh_to_volume {res}: tree and grid differ')
    lo, hi = v.amin(0).double().cpu().numpy(), v.amax(0).double().cpu().numpy()
    T = np.eye(4)
    T[:3, :3] = geometry._rodrigues(np.array([1.0, 2.0, 3.0]) / np.sqrt(14.0) * np.deg2rad(8.0))
    T[:3, 3] = 0.75 * (hi - lo)                                                   # out of the target's box: most of the source starts far
    src = geometry.transform_points(v[::max(int(v.shape[0]) // 20000, 1)].contiguous(), T)
    out = {}
    for search in ('grid', 'tree'):
        out[search], t = host_clock(lambda: geometry.align_mesh(src, v, f, iterations=10, init='identity', search=search), reps=2)
        r[f'align_mesh_displaced_mesh128_{search}'] = dict(end_to_end_host_clock=t, points=int(src.shape[0]), iterations=out[search]['iterations'],
                                                           rms_first=out[search]['rms_history'][0], rms_last=out[search]['rms'])
    if not (np.array_equal(out['grid']['matrix'], out['tree']['matrix']) and out['grid']['rms_history'] == out['tree']['rms_history']):
        raise SystemExit('align_mesh: tree and grid differ')
    return r


def main():
    if '--step' in sys.argv:                                                      # child: one step, one JSON line
        name = sys.argv[sys.argv.index('--step') + 1]
        print('RESULT ' + json.dumps({'build': step_build, 'query': step_query, 'callers': step_callers}[name]()))
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
