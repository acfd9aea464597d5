"""Times of mesh smoothing and mesh normals on the device (one JSON line on stdout, ``--out FILE`` to keep it).

Full-width generator, B = 1, synthetic weights, level 0, ``keep='largest'``.  Every step runs in a child process of its own under a time
limit, one after the other; the first step that fails, faults or runs out of time ends the run (its name and exit status are recorded).

``mesh256`` / ``mesh512``: on the marching-cubes mesh at that resolution and on its ``simplify_mesh(target_faces=100000)`` version:

- the phases of ``MeshAdjacency`` (key emission, the two ``torch.sort`` calls, the CSR build: each phase ends in a synchronise) and the
  cotangent weights;
- one step: time (device events around 20 steps, uniform and cotangent), the algorithmic bytes of a step (24 V for the positions read
  and written, 4 (V + 1) + V for offsets and pinned flags, 4 E for the neighbours (8 E with weights), 12 E for the gathered positions) and
  the rate they give, with the degree histogram;
- ``smooth_mesh`` end to end for 10 pairs with a prebuilt adjacency and without, and ``mesh_normals``;
- in the same run, alternating with the above: ``torch.sparse.mm`` of the same CSR (row-normalised, float32) on the device per step, the
  host route (copy out, ``scipy.sparse``, 20 steps, copy back; skipped without scipy), and ``marching_cubes`` of the same mesh;
- the signed volume before and after and the Hausdorff distance of the smoothed mesh to its input (``surface_distance``).
Usage: python tools/bench_smooth.py [--out FILE] [--steps mesh256,mesh512]"""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_simplify import host_timed, mesh_at, spread                              # noqa: E402

STEPS = {'mesh256': 420, 'mesh512': 540}                                            # step -> seconds


def event_timed(fn, reps=3):
    import torch
    ts = []
    for _ in range(reps + 1):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return spread(ts[1:])


def measure(v, f, with_host):
    import numpy as np
    import torch
    from invertavatar_amd import geometry, hipops
    r = {'verts': int(v.shape[0]), 'faces': int(f.shape[0])}
    hipops.SMOOTH_TIMES = {}
    adj = geometry.MeshAdjacency(v, f)
    adj.cotangent()
    r['build_phases_ms'], hipops.SMOOTH_TIMES = {k: round(x * 1e3, 3) for k, x in hipops.SMOOTH_TIMES.items()}, None
    r['build'], _ = host_timed(lambda: geometry.MeshAdjacency(v, f), reps=3)
    r['info'] = adj.info
    nv, ne = r['verts'], int(adj.neighbors.numel())
    deg = (adj.offsets[1:] - adj.offsets[:-1]).long()
    r['degree_histogram'] = torch.bincount(deg.clamp(max=16), minlength=17).cpu().tolist()   # (the last bin: 16 and above)
    s = adj._state
    n_steps = 20
    rows = torch.repeat_interleave(torch.arange(nv, device=v.device), deg)
    for weights in ('uniform', 'cotangent'):
        w = adj.cotangent() if weights == 'cotangent' else None
        pinned = hipops.smooth_pinned(s, adj.verts, w, True, None)
        t = event_timed(lambda: hipops.smooth_steps(s, adj.verts, w, pinned, [0.5, -0.53] * (n_steps // 2)))
        nbytes = 24 * nv + 4 * (nv + 1) + nv + (8 if w is not None else 4) * ne + 12 * ne
        per = t['ms'] / n_steps
        r[f'step_{weights}'] = dict(per_step_ms=round(per, 4), of_steps=t, algorithmic_bytes=nbytes, gb_per_s=round(nbytes / per / 1e6, 1))
        # yardstick: the same step as a sparse matrix product (row-normalised weights, float32), alternating with the kernel above
        vals = torch.ones(ne, device=v.device) if w is None else w.clone()
        wsum = torch.zeros(nv, device=v.device).index_add_(0, rows, vals)
        m = torch.sparse_csr_tensor(adj.offsets.long(), adj.neighbors.long(), vals / wsum[rows].clamp_min(1e-30), size=(nv, nv))

        def sparse_steps():
            p = adj.verts
            for k in range(n_steps):
                p = p + (0.5 if k % 2 == 0 else -0.53) * (torch.sparse.mm(m, p) - p)
            return p
        ts = event_timed(sparse_steps)
        r[f'step_{weights}']['torch_sparse_mm_per_step_ms'] = round(ts['ms'] / n_steps, 4)
        del m
    r['smooth_10_pairs_prebuilt'], out = host_timed(lambda: geometry.smooth_mesh(v, f, adjacency=adj), reps=3)
    r['smooth_10_pairs'], _ = host_timed(lambda: geometry.smooth_mesh(v, f), reps=3)
    r['mesh_normals_area'], _ = host_timed(lambda: geometry.mesh_normals(v, f, adjacency=adj), reps=3)
    r['mesh_normals_angle'], _ = host_timed(lambda: geometry.mesh_normals(v, f, weighting='angle', adjacency=adj), reps=3)
    d = geometry.surface_distance(out['verts'], f, v, f, samples=200000)
    r['check'] = dict(volume_before=geometry.signed_volume(v, f), volume_after=geometry.signed_volume(out['verts'], f),
                      smoothed_to_input=d['max_ab'], input_to_smoothed=d['max_ba'], pinned=int(out['pinned'].sum()))
    if with_host:
        try:
            import scipy.sparse as sp
        except ImportError:
            r['host_route'] = 'scipy is not installed'
            return r
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        hv, hf = v.cpu().numpy().astype(np.float64), f.cpu().numpy()
        t1 = time.perf_counter()
        i = np.concatenate([hf[:, 0], hf[:, 1], hf[:, 1], hf[:, 2], hf[:, 2], hf[:, 0]])
        j = np.concatenate([hf[:, 1], hf[:, 0], hf[:, 2], hf[:, 1], hf[:, 0], hf[:, 2]])
        m = sp.coo_matrix((np.ones(len(i)), (i, j)), shape=(nv, nv)).tocsr()
        m.data[:] = 1.0
        inv = 1.0 / np.maximum(np.diff(m.indptr), 1)
        t2 = time.perf_counter()
        p = hv
        for k in range(n_steps):
            p = p + (0.5 if k % 2 == 0 else -0.53) * ((m @ p) * inv[:, None] - p)
        t3 = time.perf_counter()
        back = torch.from_numpy(p.astype(np.float32)).cuda()
        torch.cuda.synchronize()
        t4 = time.perf_counter()
        del back
        r['host_route'] = dict(to_host_ms=round((t1 - t0) * 1e3, 2), scipy_build_ms=round((t2 - t1) * 1e3, 2),
                               steps_ms=round((t3 - t2) * 1e3, 2), to_device_ms=round((t4 - t3) * 1e3, 2), total_ms=round((t4 - t0) * 1e3, 2))
    return r


def step_mesh(n):
    from invertavatar_amd import geometry
    vol, lo, step = mesh_at(n)
    r = {}
    r['marching_cubes'], (v, f) = host_timed(lambda: geometry.marching_cubes(vol, 0.0, lo, step), reps=3)
    del vol
    r['full'] = measure(v, f, with_host=n <= 256)
    simple = geometry.simplify_mesh(v, f, target_faces=100000)
    r['simplified_100000'] = measure(simple['verts'], simple['faces'], with_host=True)
    return r


def main():
    if '--step' in sys.argv:                                                      # child: one step, one JSON line
        print('RESULT ' + json.dumps(step_mesh(int(sys.argv[sys.argv.index('--step') + 1][4:]))))
        return
    from invertavatar_amd import build as ia_build
    out_path = sys.argv[sys.argv.index('--out') + 1] if '--out' in sys.argv else None
    steps = sys.argv[sys.argv.index('--steps') + 1].split(',') if '--steps' in sys.argv else list(STEPS)
    res = {'source_digest': ia_build.source_digest(), 'level': 0.0, 'keep': 'largest'}
    try:
        import torch
        res['device'] = torch.cuda.get_device_name(0)
    except Exception as exc:                                                      # a measurement without a device fails, it does not fall back
        print(json.dumps({'error': f'no device: {exc}'}))
        sys.exit(1)
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
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, 'w') as fh:
            fh.write(line + '\n')
    sys.exit(1 if 'stopped_at' in res else 0)


if __name__ == '__main__':
    main()
