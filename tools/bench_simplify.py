"""Times and errors of mesh simplification on the device (one JSON line on stdout, ``--out FILE`` to keep it).

Full-width generator, B = 1, synthetic weights, level 0, ``keep='largest'``.  Every step runs in a child process of its own under a time
limit, one after the other; the first step that fails, faults or runs out of time ends the run (its name and exit status are recorded).

- ``mesh256`` / ``mesh512``: on the marching-cubes mesh at that resolution: ``marching_cubes`` of the same run for scale;
  ``simplify_mesh`` end to end (host clock around a device synchronise, median of the timed runs after warm-up with the smallest and
  largest beside it) for ``cells`` in {32, 64, 128, 256} and ``target_faces`` in {20 k, 100 k, 500 k} with the number of count-only
  passes; per-phase times of one run per ``cells`` (keys and clusters, the three ``torch.sort`` calls, accumulate, place, faces: each
  phase then ends in a synchronise, so their sum exceeds the end-to-end time); the host route it replaces (copy to the host, the NumPy
  restatement, copy back) at ``cells`` = 64; ``surface_distance`` of each result against the input.
- ``accuracy``: ``e_ord`` of the float64 restatement, the device's error against it and the tolerance ``4 * e_ord + eps32 * extent`` on the
  256^3 mesh at ``cells`` = 64.
Usage: python tools/bench_simplify.py [--out FILE] [--steps mesh256,mesh512,accuracy]"""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')
sys.path.insert(0, ROOT)

STEPS = {'mesh256': 420, 'mesh512': 540, 'accuracy': 420}                        # step -> seconds


def spread(ts):
    ts = sorted(ts)
    return dict(ms=round(ts[len(ts) // 2], 3), min_ms=round(ts[0], 3), max_ms=round(ts[-1], 3), reps=len(ts))


def host_timed(fn, warmup=1, reps=5):
    import torch
    ts, out = [], None
    for k in range(warmup + reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        if k >= warmup:
            ts.append((time.perf_counter() - t0) * 1e3)
    return spread(ts), out


def mesh_at(n):
    import torch
    from invertavatar_amd import geometry, synthetic
    from invertavatar_amd.training_avatar_texture.triplane_v20 import TriPlaneGenerator
    g = synthetic.fill_parameters(TriPlaneGenerator(**synthetic.generator_kwargs('full')).eval().requires_grad_(False)).cuda()
    with torch.no_grad():
        ws = g.mapping(synthetic.latent(0, 1).cuda(), synthetic.conditioning_camera().cuda(), truncation_psi=0.7, truncation_cutoff=14)
        mesh = {'uvcoords_image': synthetic.uv_conditions([0]).cuda()}
        planes = geometry.generator_planes(g, ws, mesh, noise_mode='const')
        bw = g.rendering_kwargs['box_warp']
        _, lo, step = geometry.lattice_axis(n, bw, 0.0)
        vol = geometry.density_volume(planes, g.decoder, n, bw, box_warp=bw)[0].contiguous()
    vol = geometry.keep_components(vol, 0.0, 'largest')[0]
    return vol, (float(lo),) * 3, (float(step),) * 3


def distance(res, v, f):
    from invertavatar_amd import geometry
    if res['faces'].shape[0] == 0:
        return None
    d = geometry.surface_distance(res['verts'], res['faces'], v, f, samples=200000)
    diag = float(sum(h * h for h in res['cell']) ** 0.5) if res['dims'] is not None else 0.0
    return dict(simplified_to_input=d['max_ab'], input_to_simplified=d['max_ba'], chamfer=d['chamfer'], cell_diagonal=diag)


def step_mesh(n):
    import torch
    from invertavatar_amd import geometry, hipops
    vol, lo, step = mesh_at(n)
    r = {}
    r['marching_cubes'], (v, f) = host_timed(lambda: geometry.marching_cubes(vol, 0.0, lo, step), reps=3)
    del vol
    r.update(verts=int(v.shape[0]), faces=int(f.shape[0]))
    for cells in (32, 64, 128, 256):
        t, res = host_timed(lambda: geometry.simplify_mesh(v, f, cells=cells), reps=3)
        hipops.SIMPLIFY_TIMES = {}
        geometry.simplify_mesh(v, f, cells=cells)
        phases, hipops.SIMPLIFY_TIMES = {k: round(x * 1e3, 3) for k, x in hipops.SIMPLIFY_TIMES.items()}, None
        r[f'cells_{cells}'] = dict(end_to_end=t, phases_ms=phases, dims=res['dims'], verts=int(res['verts'].shape[0]),
                                   faces=int(res['faces'].shape[0]), distance=distance(res, v, f))
    for target in (20000, 100000, 500000):
        t, res = host_timed(lambda: geometry.simplify_mesh(v, f, target_faces=target), warmup=1, reps=3)
        r[f'target_{target}'] = dict(end_to_end=t, count_only_passes=res['steps'], dims=res['dims'], faces=int(res['faces'].shape[0]),
                                     distance=distance(res, v, f))
    if n <= 256:
        ts = []
        for _ in range(1):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            hv, hf = v.cpu().numpy(), f.cpu().numpy()
            t1 = time.perf_counter()
            out = geometry.simplify_mesh(hv, hf, cells=64)
            t2 = time.perf_counter()
            back = [torch.from_numpy(out[k]).cuda() for k in ('verts', 'faces', 'vertex_map', 'cluster_size')]
            torch.cuda.synchronize()
            ts.append(dict(to_host_ms=round((t1 - t0) * 1e3, 2), numpy_ms=round((t2 - t1) * 1e3, 2),
                           to_device_ms=round((time.perf_counter() - t2) * 1e3, 2), total_ms=round((time.perf_counter() - t0) * 1e3, 2)))
            del back
        r['host_route_cells_64'] = ts
    return r


def step_accuracy():
    import numpy as np
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    import test_simplify_cpu as cpu
    from invertavatar_amd import geometry
    vol, lo, step = mesh_at(256)
    v, f = geometry.marching_cubes(vol, 0.0, lo, step)
    hv, hf = v.cpu().numpy(), f.cpu().numpy()
    out = {}
    for cells in (64,):
        got = geometry.simplify_mesh(v, f, cells=cells)
        want = geometry.simplify_mesh(hv, hf, cells=cells)
        ref, e_ord, tol, extent = cpu.reference64(hv, hf, want, 'quadric')
        err = float(np.abs(got['verts'].cpu().numpy().astype(np.float64) - ref['verts']).max())
        ints = all(np.array_equal(got[k].cpu().numpy(), want[k]) for k in ('faces', 'vertex_map', 'cluster_size'))
        out[f'cells_{cells}'] = dict(extent=extent, e_ord=e_ord, tolerance=tol, device_error=err, integer_outputs_equal=bool(ints))
    return out


def run_step(name):
    if name.startswith('mesh'):
        return step_mesh(int(name[4:]))
    return {'accuracy': step_accuracy}[name]()


def main():
    if '--step' in sys.argv:                                                      # child: one step, one JSON line
        print('RESULT ' + json.dumps(run_step(sys.argv[sys.argv.index('--step') + 1])))
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
