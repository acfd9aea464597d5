"""Times of the winding tree on the device against the exact kernel (HIP events; one JSON line on stdout, ``--out FILE`` to keep it;
the recorded run is profiles/winding_tree_bench.json).

Full-width generator, B = 1, synthetic weights, level 0 (the meshes of tools/bench_winding.py).  Every step runs in a child process of
its own under a time limit, one after the other; the first step that fails, faults or runs out of time ends the run.

- ``build``: ``geometry.WindingTree.from_grid`` of the 128^3 and the 256^3 mesh (keys, sort, gather, nodes), with the tree's ``info``.
- ``query``: ``WindingTree.query`` (with its point sort) for beta = 2 and 4 against ``hipops.winding_number``, for 1 000 and 100 000
  random points of the box and for the mesh's own vertices: times, the mean far terms and exact pairs per point, and the largest
  difference to the exact kernel.
- ``volume``: ``mesh_to_volume(sign='winding')`` of the 128^3 mesh on lattices of 64 and 128 points, ``winding='exact'`` and ``'tree'``
  (host clock, synchronised), with the number of lattice points on which the two disagree.
Every time is the median of the timed runs after warm-up, with the smallest and largest beside it.
Usage: python tools/bench_winding_tree.py [--out FILE] [--steps build,query,volume]"""
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

STEPS = {'build': 240, 'query': 420, 'volume': 420}      # step -> seconds
BETAS = (2.0, 4.0)


def step_build():
    from invertavatar_amd import geometry
    r = {}
    for n in (128, 256):
        v, f = mesh(n)
        grid = geometry.TriangleGrid(v, f, build=False)
        tree = geometry.WindingTree.from_grid(grid)
        r[f'mesh{n}'] = dict(info=tree.info, counts=tree.counts, build=timed(lambda: geometry.WindingTree.from_grid(grid), warmup=1, reps=5))
    return r


def step_query():
    from invertavatar_amd import geometry, hipops
    r = {}
    for n in (128, 256):
        v, f = mesh(n)
        grid = geometry.TriangleGrid(v, f, build=False)
        tree = geometry.WindingTree.from_grid(grid)
        faces = int(f.shape[0])
        row = dict(faces=faces, vertices=int(v.shape[0]))
        for name, pts in (('n1k', box_points(v, 1000)), ('n100k', box_points(v, 100000)), ('vertices', v.contiguous())):
            reps = 3 if pts.shape[0] * faces > 2e10 else 7
            exact = hipops.winding_number(pts, grid.tris)
            cell = dict(points=int(pts.shape[0]), exact=timed(lambda: hipops.winding_number(pts, grid.tris), warmup=1, reps=reps))
            for beta in BETAS:
                w, cnt = tree.query(pts, beta, return_counts=True)
                cell[f'beta{beta:g}'] = dict(timed(lambda: tree.query(pts, beta), warmup=1, reps=7),
                                             far_terms_per_point=float(cnt[:, 0].double().mean()),
                                             exact_pairs_per_point=float(cnt[:, 1].double().mean()),
                                             largest_difference=float((w - exact).abs().max()),
                                             sides_changed=int(((w >= 0.5) != (exact >= 0.5)).sum()))
            row[name] = cell
        r[f'mesh{n}'] = row
    return r


def step_volume():
    import torch
    from invertavatar_amd import geometry
    v, f = mesh(128)
    r = dict(faces=int(f.shape[0]))
    for res in (64, 128):
        masks = {}
        for winding in ('exact', 'tree'):
            ts = []
            for _ in range(1 + 3):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                out = geometry.mesh_to_volume(v, f, res, sign='winding', winding=winding)
                torch.cuda.synchronize()
                ts.append((time.perf_counter() - t0) * 1e3)
            masks[winding] = out['inside']
            r[f'res{res}_{winding}'] = dict(end_to_end_host_clock=spread(ts[1:]), lattice=list(out['inside'].shape), info=out['info'],
                                            inside_points=int(out['inside'].sum()))
        r[f'res{res}_points_that_differ'] = int((masks['exact'] != masks['tree']).sum())
    return r


def main():
    if '--step' in sys.argv:                                                      # child: one step, one JSON line
        name = sys.argv[sys.argv.index('--step') + 1]
        print('RESULT ' + json.dumps({'build': step_build, 'query': step_query, 'volume': step_volume}[name]()))
        return
    from invertavatar_amd import build as ia_build
    out_path = sys.argv[sys.argv.index('--out') + 1] if '--out' in sys.argv else None
    steps = sys.argv[sys.argv.index('--steps') + 1].split(',') if '--steps' in sys.argv else list(STEPS)
    res = {'source_digest': ia_build.source_digest(), 'level': 0.0, 'betas': list(BETAS)}
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
