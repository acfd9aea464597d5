"""Times of the alignment path on the device (HIP events; one JSON line on stdout, ``--out FILE`` to keep it).

Full-width generator, B = 1, synthetic weights, level 0.  Every step runs in a child process of its own under a time limit, one after
the other; the first step that fails, faults or runs out of time ends the run (its name and exit status are recorded).

- ``kernels``: ``ia_transform_points``, the closest-point query (``TriangleGrid.closest`` against the 256^3 mesh) and ``ia_align_sums``
  in both metrics, at the vertex counts of the 128^3 and the 256^3 mesh.
- ``align``: ``align_mesh`` end to end (host clock, synchronised) for the vertices of the 128^3 mesh, moved by 5 degrees, 2 % and a
  shift of 0.02, against the 256^3 mesh, per metric: steps taken, rms before and after, the error of the matrix.
- ``host``: the yardstick, the same loop on the host with ``scipy.spatial.cKDTree`` nearest VERTICES (a cheaper, inexact pairing; the
  point metric only, a vertex has no face) and NumPy sums, on 16 threads.
Every time is the median of the timed runs after warm-up, with the smallest and largest beside it.
Usage: python tools/bench_align.py [--out FILE] [--steps kernels,align,host]"""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_surface_distance import mesh_at, setup, spread, timed        # noqa: E402

STEPS = {'kernels': 240, 'align': 300, 'host': 300}                      # step -> seconds


def offset():
    import numpy as np
    from invertavatar_amd import geometry
    ax = np.array([1.0, 2.0, 3.0]) / np.sqrt(14.0)
    T = np.eye(4)
    T[:3, :3] = 1.02 * geometry._rodrigues(ax * np.deg2rad(5.0))
    T[:3, 3] = (0.02, -0.01, 0.015)
    return T


def meshes():
    from invertavatar_amd import geometry
    g, planes = setup()
    out = []
    for n in (128, 256):
        vol, lo, step = mesh_at(g, planes, n)
        out.append(geometry.marching_cubes(vol, 0.0, lo, step))
    return out


def moved_source(verts, T):
    import numpy as np
    import torch
    Ti = np.linalg.inv(T)
    x = verts.cpu().numpy().astype(np.float64) @ Ti[:3, :3].T + Ti[:3, 3]
    return torch.from_numpy(x.astype(np.float32)).to(verts.device)


def step_kernels():
    from invertavatar_amd import geometry, hipops
    (va, fa), (vb, fb) = meshes()
    grid = geometry.TriangleGrid(vb, fb)
    normals = geometry.face_normals(grid.verts, grid.faces).float().contiguous()
    centre = [(a + b) / 2 for a, b in zip(grid.lo, grid.hi)]
    M = offset()
    r = dict(faces_256=int(fb.shape[0]))
    for name, pts in (('n128', va), ('n256', vb)):
        pts = pts.contiguous()
        q = grid.closest(hipops.transform_points(pts, M))
        p = hipops.transform_points(pts, M)
        args = (p, q['point'].contiguous(), q['dist'].contiguous(), q['face'].int().contiguous(), centre, float('inf'))
        r[name] = dict(points=int(pts.shape[0]), transform_points=timed(lambda: hipops.transform_points(pts, M)),
                       closest_with_cell_sort=timed(lambda: grid.closest(p), reps=5),
                       align_sums_point=timed(lambda: hipops.align_sums(*args, 'point')),
                       align_sums_plane=timed(lambda: hipops.align_sums(*args, 'plane', normals)))
    return r


def step_align():
    import numpy as np
    import torch
    from invertavatar_amd import geometry
    (va, fa), (vb, fb) = meshes()
    T = offset()
    src = moved_source(va, T)
    grid = geometry.TriangleGrid(vb, fb)
    r = dict(points=int(src.shape[0]), faces=int(fb.shape[0]))
    for metric in ('plane', 'point'):
        ts = []
        for _ in range(1 + 3):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fit = geometry.align_mesh(src, vb, fb, metric=metric, scale=True, iterations=30, grid=grid)
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        r[metric] = dict(end_to_end_host_clock=spread(ts[1:]), steps=fit['iterations'], converged=fit['converged'], rms_before=fit['rms_history'][0],
                         rms_after=fit['rms'], matrix_error=float(np.abs(fit['matrix'] - T).max()),
                         note='the grid is built once outside the timed region; the rms floor is the difference of the two lattices')
    return r


def step_host():
    import numpy as np
    from invertavatar_amd import geometry
    try:
        from scipy.spatial import cKDTree
    except ImportError:
        return 'scipy is not installed on this machine'
    (va, fa), (vb, fb) = meshes()
    T = offset()
    src = moved_source(va, T).cpu().numpy()
    b = vb.cpu().numpy().astype(np.float64)
    centre = (b.min(0) + b.max(0)) / 2
    t0 = time.perf_counter()
    tree = cKDTree(b)
    t1 = time.perf_counter()
    M, hist = np.eye(4), []
    for k in range(31):
        p = geometry._transform_numpy(src, M)
        d, idx = tree.query(p.astype(np.float64), workers=16)
        terms, _ = geometry._align_terms_numpy(p, b[idx], d, idx, None, centre, np.inf, 'point')
        S = np.concatenate([terms.sum(0), [0.0]])
        hist.append(float(np.sqrt(S[18] / S[0])))
        if k == 30 or (k > 0 and abs(hist[k - 1] - hist[k]) <= 1e-6 * hist[k - 1]):
            break
        M = geometry._align_solve(S, 'point', True, centre) @ M
    t2 = time.perf_counter()
    return dict(build_ms=round((t1 - t0) * 1e3, 2), loop_ms=round((t2 - t1) * 1e3, 2), pairings=len(hist), rms_before=hist[0], rms_after=hist[-1],
                matrix_error=float(np.abs(M - T).max()), points=int(src.shape[0]), target_vertices=int(b.shape[0]),
                note='nearest vertex, not nearest surface point: a cheaper, inexact pairing; point metric, plain NumPy sums')


def main():
    if '--step' in sys.argv:                                                      # child: one step, one JSON line
        name = sys.argv[sys.argv.index('--step') + 1]
        print('RESULT ' + json.dumps({'kernels': step_kernels, 'align': step_align, 'host': step_host}[name]()))
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
