"""Times of the non-rigid fit on the device (HIP events; one JSON line on stdout, ``--out FILE`` to keep it).

Full-width generator, B = 1, synthetic weights, level 0.  Every step runs in a child process of its own under a time limit, one after
the other; the first step that fails, faults or runs out of time ends the run (its name and exit status are recorded).

- ``kernels``: ``ia_nonrigid_terms``, one conjugate-gradient step (the difference of a 101-step and a 1-step solve, over 100; with its
  launches and the algorithmic bytes it moves) and one solve of 100 steps, for templates of about 5 k, 20 k and 100 k vertices
  (``simplify_mesh`` of the 128^3 head) against the 256^3 head.  The solves run without a tolerance, so no step is a no-op.
- ``fit``: ``nonrigid_align`` end to end (host clock, synchronised) for the same templates, via the grid and via the tree.
- ``host``: the yardstick, the same loop on the host with ``scipy.sparse.linalg.cg`` on the assembled matrix and ``cKDTree`` nearest
  VERTICES (a cheaper, inexact pairing), on 16 threads; skipped, and said so, where scipy is not installed.
Every time is the median of the timed runs after warm-up, with the smallest and largest beside it.
Usage: python tools/bench_nonrigid.py [--out FILE] [--steps kernels,fit,host]"""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_surface_distance import mesh_at, setup, spread, timed        # noqa: E402

STEPS = {'kernels': 300, 'fit': 420, 'host': 420}                        # step -> seconds
BUDGETS = (10000, 40000, 200000)                                         # triangles: about 5 k, 20 k and 100 k vertices
SCHEDULE = dict(stiffness=(50.0, 10.0, 2.0, 0.5), iterations=5)


def meshes():
    """The templates (the 128^3 head simplified to each budget) and the target (the 256^3 head)."""
    from invertavatar_amd import geometry
    g, planes = setup()
    vol, lo, step = mesh_at(g, planes, 128)
    va, fa = geometry.marching_cubes(vol, 0.0, lo, step)
    vol, lo, step = mesh_at(g, planes, 256)
    target = geometry.marching_cubes(vol, 0.0, lo, step)
    templates = []
    for budget in BUDGETS:
        if budget >= fa.shape[0]:
            templates.append((va, fa))
        else:
            s = geometry.simplify_mesh(va, fa, target_faces=budget)
            templates.append((s['verts'], s['faces']))
    return templates, target


def step_kernels():
    import torch
    from invertavatar_amd import geometry, hipops
    templates, (vb, fb) = meshes()
    grid = geometry.TriangleGrid(vb, fb)
    r = dict(faces_target=int(fb.shape[0]), launches_per_step=hipops.NONRIGID_LAUNCHES)
    for x, f in templates:
        x = x.contiguous()
        adj = geometry.MeshAdjacency(x, f)
        nv, e = adj.n_verts, adj._state['E']
        pinned = torch.zeros(nv, dtype=torch.bool, device=x.device)
        q = grid.closest(x)
        args = (x, x, q['point'].contiguous(), q['dist'].contiguous(), q['face'].int().contiguous(), pinned)
        c, _, b, _ = hipops.nonrigid_terms(*args)

        def solve(steps):
            return hipops.nonrigid_solve(adj._state, c, b, 10.0, pinned, cg_iterations=steps, cg_tol=0.0)
        one, many = timed(lambda: solve(1), reps=5), timed(lambda: solve(101), reps=5)
        per_step = (many['ms'] - one['ms']) / 100.0
        nbytes = hipops.nonrigid_step_bytes(nv, e)
        r[f'v{nv}'] = dict(vertices=nv, csr_entries=int(e), heavy_vertices=int(adj._state['n_heavy']), terms_point=timed(lambda: hipops.nonrigid_terms(*args)),
                           solve_1_step=one, solve_101_steps=many, solve_100_steps=timed(lambda: solve(100), reps=5),
                           cg_step_ms=round(per_step, 5), cg_step_bytes=int(nbytes),
                           cg_step_gb_per_s=round(nbytes / (per_step * 1e-3) / 1e9, 1) if per_step > 0 else None)
    return r


def step_fit():
    import torch
    from invertavatar_amd import geometry
    templates, (vb, fb) = meshes()
    grid = geometry.TriangleGrid(vb, fb)
    tree = geometry.WindingTree.from_grid(grid)
    r = dict(faces_target=int(fb.shape[0]), schedule=list(SCHEDULE['stiffness']), iterations=SCHEDULE['iterations'])
    for x, f in templates:
        adj = geometry.MeshAdjacency(x, f)
        row = dict(vertices=adj.n_verts)
        for search in ('grid', 'tree'):
            ts = []
            for _ in range(1 + 3):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fit = geometry.nonrigid_align((x, f), vb, fb, adjacency=adj, grid=grid, search=search, tree=tree if search == 'tree' else None,
                                              **SCHEDULE)
                torch.cuda.synchronize()
                ts.append((time.perf_counter() - t0) * 1e3)
            row[search] = dict(end_to_end_host_clock=spread(ts[1:]), pairings=len(fit['rms_history']), rms_before=fit['rms_history'][0],
                               rms_after=fit['rms'], cg_steps=[lvl['cg_steps'] for lvl in fit['levels']], inliers=fit['inliers'])
        row['note'] = 'adjacency, grid and tree are built once outside the timed region'
        r[f'v{adj.n_verts}'] = row
    return r


def step_host():
    import numpy as np
    from invertavatar_amd import geometry
    try:
        import scipy.sparse as sp
        from scipy.sparse.linalg import cg
        from scipy.spatial import cKDTree
    except ImportError:
        return 'scipy is not installed on this machine: the host yardstick is skipped'
    templates, (vb, fb) = meshes()
    b = vb.cpu().numpy().astype(np.float64)
    tree = cKDTree(b)
    r = {}
    for x, f in templates:
        adj = geometry.MeshAdjacency(x.cpu().numpy(), f.cpu().numpy())
        x64 = adj.verts.astype(np.float64)
        nv = adj.n_verts
        off = np.asarray(adj.offsets).astype(np.int64)
        rows = np.repeat(np.arange(nv), np.diff(off))
        lap = sp.diags(np.diff(off).astype(np.float64)) - sp.csr_matrix((np.ones(rows.size), (rows, np.asarray(adj.neighbors))), shape=(nv, nv))
        t0 = time.perf_counter()
        d, hist, steps = np.zeros((nv, 3)), [], 0
        for a in SCHEDULE['stiffness']:
            prev = None
            for k in range(SCHEDULE['iterations']):
                p = (x64 + d).astype(np.float32).astype(np.float64)
                dist, idx = tree.query(p, workers=16)
                rms = float(np.sqrt((dist ** 2).mean()))
                hist.append(rms)
                if prev is not None and abs(prev - rms) <= 1e-4 * prev:
                    break
                prev = rms
                A = sp.identity(nv, format='csr') + a * lap
                rhs = b[idx] - x64
                for col in range(3):
                    count = [0]
                    d[:, col], _ = cg(A, rhs[:, col], x0=d[:, col], maxiter=100, callback=lambda _: count.__setitem__(0, count[0] + 1))
                    steps += count[0]
        r[f'v{nv}'] = dict(vertices=nv, loop_ms=round((time.perf_counter() - t0) * 1e3, 2), pairings=len(hist), cg_steps=steps, rms_before=hist[0],
                           rms_after=hist[-1])
    r['note'] = 'nearest vertex, not nearest surface point: a cheaper, inexact pairing; scipy cg at its default tolerance, one coordinate at a time'
    return r


def main():
    if '--step' in sys.argv:                                                      # child: one step, one JSON line
        name = sys.argv[sys.argv.index('--step') + 1]
        print('RESULT ' + json.dumps({'kernels': step_kernels, 'fit': step_fit, 'host': step_host}[name]()))
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
