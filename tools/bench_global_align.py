"""Times of global registration on the device (HIP events; one JSON line on stdout, ``--out FILE`` to keep it).

Full-width generator, B = 1, synthetic weights, level 0.  Every step runs in a child process of its own under a time limit, one after
the other; the first step that fails, faults or runs out of time ends the run (its name and exit status are recorded).

- ``field``: ``PoseField`` at 32 and 64 points along the longest side against the 128^3 and the 256^3 head mesh.
- ``scores``: ``ia_pose_scores`` for the 4 416 rotations of the 15-degree set with n = 256 / 1 024 / 4 096 points of the 128^3 mesh and
  shifts = 1 / 5, against the 32-point field of the 256^3 mesh: time, lookups per second and the byte rate of the gathers (eight
  float32 reads per lookup).  The step fails unless two runs of the kernel give the same bits.
- ``align``: ``global_align`` end to end (host clock, synchronised) for the vertices of the 128^3 mesh under a known 140-degree
  offset against the 256^3 mesh: the error of the matrix, the winner's place.
- ``torch``: the same definition through chunked PyTorch device operations (index arithmetic + eight gathers): the yardstick.
- ``numpy``: the NumPy restatement on the host, n = 256, shifts = 1.
Every time is the median of the timed runs after warm-up, with the smallest and largest beside it.
Usage: python tools/bench_global_align.py [--out FILE] [--steps field,scores,align,torch,numpy]"""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_align import meshes, moved_source                            # noqa: E402
from bench_surface_distance import spread, timed                        # noqa: E402

STEPS = {'field': 300, 'scores': 300, 'align': 300, 'torch': 300, 'numpy': 300}      # step -> seconds


def offset():
    import numpy as np
    from invertavatar_amd import geometry
    ax = np.array([1.0, 2.0, 3.0]) / np.sqrt(14.0)
    T = np.eye(4)
    T[:3, :3] = geometry._rodrigues(ax * np.deg2rad(140.0))
    T[:3, 3] = (0.3, -0.2, 0.25)
    return T


def subset(verts, n):
    import torch
    idx = (torch.arange(n, dtype=torch.int64, device=verts.device) * verts.shape[0]) // n
    return verts[idx].contiguous()


def score_inputs(n):
    import torch
    from invertavatar_amd import geometry
    (va, fa), (vb, fb) = meshes()
    field = geometry.PoseField(vb, fb, 32)
    x = subset(moved_source(va, offset()), n)
    rot = torch.from_numpy(geometry.pose_candidates(15.0).reshape(-1, 9)).float().cuda()
    return field, x, rot, x.double().mean(0).cpu().numpy()


def step_field():
    from invertavatar_amd import geometry
    r = {}
    for name, (v, f) in zip(('mesh128', 'mesh256'), meshes()):
        for res in (32, 64):
            field = geometry.PoseField(v, f, res)
            r[f'{name}_res{res}'] = dict(faces=int(f.shape[0]), dims=list(field.dims), build=timed(lambda: geometry.PoseField(v, f, res), warmup=1, reps=3))
    return r


def step_scores():
    import torch
    from invertavatar_amd import hipops
    r = {}
    for n in (256, 1024, 4096):
        field, x, rot, c_src = score_inputs(n)
        for shifts in (1, 5):
            run = lambda: hipops.pose_scores(x, field.dist, field.origin, field.spacing, rot, c_src, field.centroid, shifts)      # noqa: E731
            if not torch.equal(run(), run()):
                raise SystemExit(f'ia_pose_scores: two runs differ at n = {n}, shifts = {shifts}')
            t = timed(run)
            lookups = rot.shape[0] * shifts ** 3 * n
            r[f'n{n}_shifts{shifts}'] = dict(time=t, lookups=lookups, lookups_per_s=lookups / (t['ms'] * 1e-3),
                                             gather_gb_per_s=32.0 * lookups / (t['ms'] * 1e-3) / 1e9, bit_equal=True)
    return r


def step_align():
    import numpy as np
    import torch
    from invertavatar_amd import geometry
    (va, fa), (vb, fb) = meshes()
    T = offset()
    src = moved_source(va, T)
    field = geometry.PoseField(vb, fb, 32)
    grid = geometry.TriangleGrid(vb, fb, build=False)
    ts = []
    for _ in range(1 + 3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fit = geometry.global_align(src, vb, fb, field=field, grid=grid)
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return dict(points=int(src.shape[0]), faces=int(fb.shape[0]), end_to_end_host_clock=spread(ts[1:]), rank=fit['rank'], rms=fit['rms'],
                refined_rms=[c['rms'] for c in fit['candidates']], matrix_error=float(np.abs(fit['matrix'] - T).max()),
                note='field and packed triangles are built once outside the timed region; the rms floor is the difference of the two lattices')


def torch_scores(x, dist, origin, h, rot, c_src, c_tgt, chunk=256):
    """The definition in PyTorch device operations, float32 per point and float64 sums, ``chunk`` rotations at a time (shifts = 1)."""
    import torch
    dims = torch.tensor(dist.shape, device=x.device)
    y = x - torch.tensor(c_src, dtype=torch.float32, device=x.device)
    org, ct = (torch.tensor(v, dtype=torch.float32, device=x.device) for v in (origin, c_tgt))
    flat, out = dist.reshape(-1), []
    for r0 in range(0, rot.shape[0], chunk):
        p = torch.einsum('rij,nj->rni', rot[r0:r0 + chunk].reshape(-1, 3, 3), y) + ct
        u = (p - org) / h
        c = torch.minimum(u.clamp_min(0), (dims - 1).float())
        i = torch.minimum(c.floor().long(), dims - 2)
        t = c - i.float()
        acc = 0
        for corner in range(8):
            o = [(corner >> 2) & 1, (corner >> 1) & 1, corner & 1]
            w = torch.ones_like(t[..., 0])
            for a in range(3):
                w = w * (t[..., a] if o[a] else 1 - t[..., a])
            acc = acc + w * flat[((i[..., 0] + o[0]) * dims[1] + i[..., 1] + o[1]) * dims[2] + i[..., 2] + o[2]]
        d = (acc + h * (u - c).norm(dim=-1)).double()
        out.append((d * d).mean(1))
    return torch.cat(out)


def step_torch():
    from invertavatar_amd import hipops
    r = {}
    for n in (256, 1024, 4096):
        field, x, rot, c_src = score_inputs(n)
        ref = hipops.pose_scores(x, field.dist, field.origin, field.spacing, rot, c_src, field.centroid)[:, 0]
        run = lambda: torch_scores(x, field.dist, field.origin, field.spacing, rot, c_src, field.centroid)      # noqa: E731
        r[f'n{n}_shifts1'] = dict(time=timed(run, warmup=1, reps=3), largest_difference=float((run() - ref).abs().max()))
    return r


def step_numpy():
    from invertavatar_amd import geometry
    field, x, rot, c_src = score_inputs(256)
    t0 = time.perf_counter()
    geometry._pose_scores_numpy(x.cpu().numpy(), field.dist.cpu().numpy(), field.origin, field.spacing, rot.cpu().numpy().reshape(-1, 3, 3), c_src,
                                field.centroid)
    return dict(n256_shifts1_ms=round((time.perf_counter() - t0) * 1e3, 2), note='one run, float64, one thread')


def main():
    fns = {'field': step_field, 'scores': step_scores, 'align': step_align, 'torch': step_torch, 'numpy': step_numpy}
    if '--step' in sys.argv:                                                      # child: one step, one JSON line
        print('RESULT ' + json.dumps(fns[sys.argv[sys.argv.index('--step') + 1]]()))
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
