"""Times the point-cloud queries (csrc/point_tree.hip) on the vertices of the 128^3 and 256^3 head meshes taken as
clouds.  Not part of bench.py; the recorded run is profiles/point_cloud_bench.json.

Each mesh runs in a child process with a deadline:

- ``build``: ``geometry.PointTree`` (keys, ``torch.sort``, gather, boxes), host clock.
- ``nearest``: ``nearest_points`` at k = 1, 8, 16 for the cloud queried by itself, by 100 000 random box points and by 1 000 points at
  10 extents: the tree, the all-pairs kernel where it stays below ``BRUTE_PAIRS`` pairs, chunked ``torch.cdist`` + ``topk`` on the
  device and ``scipy.spatial.cKDTree`` on the host when scipy imports.  Tree and brute must give the same bits in every timed case,
  else the tool exits non-zero.
- ``normals``: ``estimate_normals(k=16)``;  ``align``: ``align_mesh(faces=None)`` of 20 000 displaced points, both metrics, end to end.

Usage: python tools/bench_point_cloud.py [--out FILE] [--meshes 128,256]"""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_closest_tree import host_clock, once, shell_points     # noqa: E402
from bench_surface_distance import spread, timed                 # noqa: E402
from bench_winding import box_points, mesh                       # noqa: E402

DEADLINE = 540               # seconds per mesh
BRUTE_PAIRS = 2e10
CDIST_ROWS = 4096


def cdist_topk(q, pts, k):
    import torch
    out = []
    for s in range(0, q.shape[0], CDIST_ROWS):
        out.append(torch.cdist(q[s:s + CDIST_ROWS], pts).topk(k, dim=1, largest=False))
    return torch.cat([o.values for o in out]), torch.cat([o.indices for o in out])


def step_mesh(n):
    import numpy as np
    import torch
    from invertavatar_amd import geometry
    pts = mesh(n)[0].contiguous()
    tree, t_build = host_clock(lambda: geometry.PointTree(pts), reps=5)
    r = {'info': tree.info, 'build_host_clock': t_build}
    sets = {'self': pts, 'box100k': box_points(pts, 100000), 'far1k': shell_points(pts, 1000)}
    try:
        from scipy.spatial import cKDTree
        kd = cKDTree(pts.cpu().numpy().astype(np.float64))
    except ImportError:
        kd = None
    for name, q in sets.items():
        for k in (1, 8, 16):
            case = {'queries': int(q.shape[0])}
            case['tree'] = timed(lambda: tree.nearest(q, k), warmup=1, reps=5)
            a = tree.nearest(q, k)
            if float(q.shape[0]) * tree.usable <= BRUTE_PAIRS:
                b, case['brute'] = once(lambda: tree.nearest(q, k, brute=True))
                if not (torch.equal(a['dist'].view(torch.int32), b['dist'].view(torch.int32)) and torch.equal(a['index'], b['index'])):
                    raise SystemExit(f'mesh{n} {name} k={k}: tree and brute differ')
            if float(q.shape[0]) * tree.usable <= BRUTE_PAIRS:
                case['cdist_topk'] = once(lambda: cdist_topk(q, pts, k))[1]
            if kd is not None and q.shape[0] <= 100000:
                qh = q.cpu().numpy().astype(np.float64)
                t0 = time.perf_counter()
                kd.query(qh, k=k)
                case['ckdtree_host'] = spread([(time.perf_counter() - t0) * 1e3])
            r[f'nearest_{name}_k{k}'] = case
    r['normals_k16'] = timed(lambda: geometry.estimate_normals(pts, 16, tree=tree), warmup=1, reps=5)
    normals = geometry.estimate_normals(pts, 16, tree=tree)['normal']
    lo, hi = pts.amin(0).double().cpu().numpy(), pts.amax(0).double().cpu().numpy()
    T = np.eye(4)
    T[:3, :3] = geometry._rodrigues(np.array([1.0, 2.0, 3.0]) / np.sqrt(14.0) * np.deg2rad(8.0))
    T[:3, 3] = 0.02 * (hi - lo)
    src = geometry.transform_points(pts[::max(int(pts.shape[0]) // 20000, 1)].contiguous(), T)
    for metric in ('point', 'plane'):
        fit, t = host_clock(lambda: geometry.align_mesh(src, pts, metric=metric, iterations=10, normals=normals if metric == 'plane' else None),
                            reps=2)
        r[f'align_cloud_{metric}'] = dict(end_to_end_host_clock=t, points=int(src.shape[0]), iterations=fit['iterations'],
                                          rms_first=fit['rms_history'][0], rms_last=fit['rms'])
    return r


def main():
    if '--step' in sys.argv:                                                      # child: one mesh, one JSON line
        print('RESULT ' + json.dumps(step_mesh(int(sys.argv[sys.argv.index('--step') + 1]))))
        return
    from invertavatar_amd import build as ia_build
    out_path = sys.argv[sys.argv.index('--out') + 1] if '--out' in sys.argv else None
    meshes = sys.argv[sys.argv.index('--meshes') + 1].split(',') if '--meshes' in sys.argv else ['128', '256']
    res = {'source_digest': ia_build.source_digest(), 'level': 0.0}
    for n in meshes:
        try:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), '--step', n], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                               timeout=DEADLINE, text=True)
        except subprocess.TimeoutExpired:
            res['stopped_at'] = dict(mesh=n, reason=f'no result within {DEADLINE} s')
            break
        lines = [ln for ln in p.stdout.splitlines() if ln.startswith('RESULT ')]
        if p.returncode != 0 or not lines:
            res['stopped_at'] = dict(mesh=n, returncode=p.returncode, stderr=p.stderr[-600:])
            break
        res[f'mesh{n}'] = json.loads(lines[-1][len('RESULT '):])
    line = json.dumps(res)
    print(line)
    if out_path:
        with open(out_path, 'w') as fh:
            fh.write(line + '\n')
    sys.exit(1 if 'stopped_at' in res else 0)


if __name__ == '__main__':
    main()
