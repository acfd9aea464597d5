"""Times and errors of the surface-distance path on the device (HIP events; one JSON line on stdout, ``--out FILE`` to keep it).

Full-width generator, B = 1, synthetic weights, level 0.  Every step runs in a child process of its own under a time limit, one after
the other; the first step that fails, faults or runs out of time ends the run (its name and exit status are recorded).

- ``mesh256`` / ``mesh512``: the marching-cubes mesh at that resolution (and the 128^3 one): grid build (``TriangleGrid``: pack, count,
  scan, fill, two host reads) and query time with the vertices of the 128^3 mesh as queries and the reverse, ``ia_distance_stats``,
  ``surface_distance`` end to end next to ``ia_density_grid`` and ``marching_cubes`` of the same run, and the host yardstick:
  ``scipy.spatial.cKDTree`` nearest-VERTEX queries on the same data, a cheaper and inexact quantity (the distance to the nearest vertex
  is an upper bound of the distance to the surface), build and query on 16 threads.
- ``brute``: the brute mode of the same kernel on 4096 queries against the 256^3 mesh; pairs per second, and the time all queries would
  take at that rate (an extrapolation, marked as such).
- ``accuracy``: e32 of the float32 restatement and the device's own error against the float64 restatement on the cases of
  tests/test_surface_distance_gpu.py (tolerance = 4 * e32 + eps32 * extent).
Every time is the median of the timed runs after warm-up, with the smallest and largest beside it.
Usage: python tools/bench_surface_distance.py [--out FILE] [--steps mesh256,brute,...]"""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')
sys.path.insert(0, ROOT)

STEPS = {'mesh256': 240, 'mesh512': 420, 'brute': 180, 'accuracy': 420}          # step -> seconds


def spread(ts):
    ts = sorted(ts)
    return dict(ms=round(ts[len(ts) // 2], 4), min_ms=round(ts[0], 4), max_ms=round(ts[-1], 4), reps=len(ts))


def timed(fn, warmup=2, reps=7):
    import torch
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


def setup():
    import torch
    from invertavatar_amd import geometry, synthetic
    from invertavatar_amd.training_avatar_texture.triplane_v20 import TriPlaneGenerator
    g = synthetic.fill_parameters(TriPlaneGenerator(**synthetic.generator_kwargs('full')).eval().requires_grad_(False)).cuda()
    with torch.no_grad():
        ws = g.mapping(synthetic.latent(0, 1).cuda(), synthetic.conditioning_camera().cuda(), truncation_psi=0.7, truncation_cutoff=14)
        mesh = {'uvcoords_image': synthetic.uv_conditions([0]).cuda()}
        planes = geometry.generator_planes(g, ws, mesh, noise_mode='const')
    return g, planes


def mesh_at(g, planes, n):
    import torch
    from invertavatar_amd import geometry
    bw = g.rendering_kwargs['box_warp']
    _, lo, step = geometry.lattice_axis(n, bw, 0.0)
    with torch.no_grad():
        vol = geometry.density_volume(planes, g.decoder, n, bw, box_warp=bw)[0].contiguous()
    return vol, (float(lo),) * 3, (float(step),) * 3


def step_mesh(n):
    import numpy as np
    import torch
    from invertavatar_amd import geometry, hipops
    g, planes = setup()
    bw = g.rendering_kwargs['box_warp']
    r = {}
    with torch.no_grad():
        r['density_grid'] = timed(lambda: geometry.density_volume(planes, g.decoder, n, bw, box_warp=bw), reps=5)
    vol, lo, step = mesh_at(g, planes, n)
    r['marching_cubes'] = timed(lambda: geometry.marching_cubes(vol, 0.0, lo, step), reps=5)
    vb, fb = geometry.marching_cubes(vol, 0.0, lo, step)
    del vol
    v128, lo128, step128 = mesh_at(g, planes, 128)
    va, fa = geometry.marching_cubes(v128, 0.0, lo128, step128)
    r.update(verts=int(vb.shape[0]), faces=int(fb.shape[0]), verts_128=int(va.shape[0]), faces_128=int(fa.shape[0]))
    r['grid_build'] = timed(lambda: geometry.TriangleGrid(vb, fb), reps=5)
    r['grid_build_128'] = timed(lambda: geometry.TriangleGrid(va, fa), reps=5)
    gb, ga = geometry.TriangleGrid(vb, fb), geometry.TriangleGrid(va, fa)
    r['grid'] = dict(dims=list(gb.dims), entries=gb.entries, oversize=gb.n_over)
    # alternating order: the two directions take turns
    q_ab, q_ba = [], []
    for k in range(2 + 7):
        for ts, grid, pts in ((q_ab, gb, va), (q_ba, ga, vb)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out = grid.closest(pts)
            e1.record()
            torch.cuda.synchronize()
            if k >= 2:
                ts.append(e0.elapsed_time(e1))
    r['query_128_vertices_against_this_mesh'] = spread(q_ab)
    r['query_this_mesh_vertices_against_128'] = spread(q_ba)
    pts_sorted = vb
    r['query_kernel_only_this_vertices_against_128'] = timed(lambda: hipops.closest_point(pts_sorted, ga.tris, ga.extent, ga.grid), reps=5)
    dist = out['dist'].contiguous()
    r['distance_stats'] = timed(lambda: hipops.distance_stats(dist, [0.01, 0.02, 0.04]))
    e2e = []
    for _ in range(1 + 3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        sd = geometry.surface_distance(va, fa, vb, fb)
        torch.cuda.synchronize()
        e2e.append((time.perf_counter() - t0) * 1e3)
    r['surface_distance_end_to_end_host_clock'] = spread(e2e[1:])
    r['surface_distance_128_against_this'] = {k: sd[k] for k in ('chamfer', 'hausdorff', 'mean_ab', 'mean_ba', 'max_ab', 'max_ba', 'fscore',
                                                                'thresholds')}
    try:
        from scipy.spatial import cKDTree
        a, b = va.cpu().numpy().astype(np.float64), vb.cpu().numpy().astype(np.float64)
        t0 = time.perf_counter()
        tree = cKDTree(b)
        t1 = time.perf_counter()
        dv, _ = tree.query(a, workers=16)
        t2 = time.perf_counter()
        exact = gb.closest(va)['dist'].cpu().numpy()
        r['host_ckdtree_nearest_VERTEX'] = dict(build_ms=round((t1 - t0) * 1e3, 2), query_ms=round((t2 - t1) * 1e3, 2), queries=int(a.shape[0]),
                                                note='nearest vertex, not nearest surface point: a cheaper, inexact quantity',
                                                mean_vertex_distance=float(dv.mean()), mean_surface_distance=float(exact.mean()))
    except ImportError:
        r['host_ckdtree_nearest_VERTEX'] = 'scipy is not installed on this machine'
    return r


def step_brute():
    import torch
    from invertavatar_amd import geometry, hipops
    g, planes = setup()
    vol, lo, step = mesh_at(g, planes, 256)
    vb, fb = geometry.marching_cubes(vol, 0.0, lo, step)
    v128, lo128, step128 = mesh_at(g, planes, 128)
    va, _ = geometry.marching_cubes(v128, 0.0, lo128, step128)
    grid = geometry.TriangleGrid(vb, fb)
    q = va[:: max(1, va.shape[0] // 4096)][:4096].contiguous()
    t = timed(lambda: hipops.closest_point(q, grid.tris, grid.extent, None), warmup=1, reps=3)
    a, b = grid.closest(q), grid.closest(q, brute=True)
    pairs = q.shape[0] * fb.shape[0]
    rate = pairs / (t['ms'] * 1e-3)
    return dict(queries=int(q.shape[0]), faces=int(fb.shape[0]), brute=t, pairs_per_second=rate,
                extrapolated_ms_for_all_128_vertices=round(va.shape[0] * fb.shape[0] / rate * 1e3, 1),
                note='the last figure is an extrapolation from the pairs per second of the subset, not a measurement',
                grid_equals_brute=bool(torch.equal(a['dist'], b['dist']) and torch.equal(a['face'], b['face'])))


def step_accuracy():
    import numpy as np
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    import test_surface_distance_cpu as cpu
    import test_surface_distance_gpu as gpu
    rs = np.random.RandomState(77)
    out = {}
    for name, n_tris, clustered in (('soup_1000', 1000, False), ('soup_1000_clustered', 1000, True), ('soup_5000', 5000, False)):
        verts, faces = cpu.random_soup(rs, n_tris, clustered=clustered)
        pts = rs.uniform(-1.3, 1.3, (800, 3)).astype(np.float32)
        d64, _, e32 = cpu.restatement_error(pts, verts, faces)
        extent = cpu.extent_of(pts, verts)
        ratio = gpu.check_case(name, pts, verts, faces)
        tol = 4 * e32 + cpu.EPS32 * extent
        out[name] = dict(extent=extent, e32=e32, tolerance=tol, device_error=ratio * tol, device_error_in_eps32_extent=ratio * tol / (cpu.EPS32 * extent))
    return out


def run_step(name):
    if name.startswith('mesh'):
        return step_mesh(int(name[4:]))
    return {'brute': step_brute, 'accuracy': step_accuracy}[name]()


def main():
    if '--step' in sys.argv:                                                      # child: one step, one JSON line
        print('RESULT ' + json.dumps(run_step(sys.argv[sys.argv.index('--step') + 1])))
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
