"""Times of the distribution scores on the device (HIP events; one JSON line on stdout, ``--out FILE`` to keep it).

Seeded Gaussian features.  Every step runs in a child process of its own under a time limit, one after the other; the first step that
fails, faults or runs out of time ends the run (its name and exit status are recorded).  A kernel step fails unless two runs give the
same bits.

- ``moments``: ``ia_feature_moments`` over N = 50 000 rows at D = 512 / 2048 in chunks of 64 and 4096 rows: time of the whole pass and
  the achieved fp64 rate (N D (D + 1) floating-point operations: the lower triangle), beside ``cov += x.double().T @ x.double()`` per
  chunk on the device and the NumPy restatement on the host.
- ``kid``: ``ia_kid_subsets`` at S = 100, m = 1000, D = 2048 beside the reference-shaped torch route on the device (per subset: gather,
  three float32 products, cube, sums) and NumPy on the host (4 subsets, scaled to 100: marked).
- ``pr``: ``ia_knn_radius`` and ``ia_manifold_covered`` at N = P = 10 000 and 50 000, D = 512 and 4096, beside the reference-shaped torch
  route on the device (``torch.cdist`` blocks of 10 000 rows, ``kthvalue``, compare) and NumPy on the host at N = P = 2 000 (its size is recorded).
- ``fid``: ``fid()`` end to end from device statistics at D = 512 / 2048 (two ``torch.linalg.eigh``) and from host statistics.
Usage: python tools/bench_distribution.py [--out FILE] [--steps moments,kid,pr,fid]"""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_surface_distance import timed                                # noqa: E402

STEPS = {'moments': 300, 'kid': 300, 'pr': 420, 'fid': 300}             # step -> seconds
N_ROWS = 50000


def features(n, d, seed, device='cuda'):
    import torch
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(n, d, generator=g) * 0.5 + 0.25).to(device)


def host_ms(fn):
    t0 = time.perf_counter()
    fn()
    return round((time.perf_counter() - t0) * 1e3, 3)


def same_bits(a, b):
    import torch
    return torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def step_moments():
    import numpy as np
    import torch
    from invertavatar_amd import hipops
    r = {}
    for d in (512, 2048):
        x = features(N_ROWS, d, d)
        for chunk in (64, 4096):
            def run():
                s = torch.zeros(d, dtype=torch.float64, device='cuda')
                c = torch.zeros(d, d, dtype=torch.float64, device='cuda')
                for lo in range(0, N_ROWS, chunk):
                    hipops.feature_moments(x[lo:lo + chunk], s, c)
                return s, c

            def yard():
                c = torch.zeros(d, d, dtype=torch.float64, device='cuda')
                for lo in range(0, N_ROWS, chunk):
                    xd = x[lo:lo + chunk].double()
                    c += xd.T @ xd
                return c
            (s0, c0), (s1, c1) = run(), run()
            if not (same_bits(s0, s1) and same_bits(c0, c1)):
                raise SystemExit('ia_feature_moments: two runs differ')
            t = timed(run, warmup=1, reps=3)
            ty = timed(yard, warmup=1, reps=3)
            rel = float(((c0 - yard()).abs().max() / c0.abs().max()).item())
            r[f'D{d}_chunk{chunk}'] = dict(kernel=t, fp64_tflops=round(N_ROWS * d * (d + 1.0) / (t['ms'] * 1e-3) / 1e12, 3), torch_double_matmul=ty,
                                           max_rel_difference=rel)
        if d == 512:
            xh = x.cpu().numpy()

            def numpy_pass():
                c = np.zeros((d, d))
                for lo in range(0, N_ROWS, 4096):
                    x64 = xh[lo:lo + 4096].astype(np.float64)
                    c += x64.T @ x64
            r['D512_chunk4096']['numpy_host_ms'] = host_ms(numpy_pass)
    return r


def step_kid():
    import numpy as np
    import torch
    from invertavatar_amd import distribution_metrics as dm, hipops
    s, m, d = 100, 1000, 2048
    gen, real = features(N_ROWS, d, 1), features(N_ROWS, d, 2) * 1.1
    ig, ir = dm.kid_subset_indices(N_ROWS, N_ROWS, s, m, 0)
    a, b = hipops.kid_subsets(gen, real, ig, ir), hipops.kid_subsets(gen, real, ig, ir)
    if not same_bits(a, b):
        raise SystemExit('ia_kid_subsets: two runs differ')
    igd, ird = torch.from_numpy(ig).cuda(), torch.from_numpy(ir).cuda()

    def yard():
        out = torch.empty(s, 3, dtype=torch.float64, device='cuda')
        for k in range(s):
            x, y = gen[igd[k]], real[ird[k]]
            kxx, kyy, kxy = (x @ x.T / d + 1) ** 3, (y @ y.T / d + 1) ** 3, (x @ y.T / d + 1) ** 3
            out[k, 0], out[k, 1], out[k, 2] = kxx.sum() - kxx.diag().sum(), kyy.sum() - kyy.diag().sum(), kxy.sum()
        return out
    t = timed(lambda: hipops.kid_subsets(gen, real, ig, ir), warmup=1, reps=5)
    ty = timed(yard, warmup=1, reps=3)
    rel = float(((a - yard().double()).abs() / a.abs()).max().item())
    gh, rh = gen.cpu().numpy(), real.cpu().numpy()
    four = host_ms(lambda: dm.kid_sums_reference(gh, rh, ig[:4], ir[:4]))
    return dict(S=s, m=m, D=d, kernel=t, fp32_tflops=round(6.0 * s * m * m * d / (t['ms'] * 1e-3) / 1e12, 2), torch_route=ty,
                max_rel_difference_from_torch_float32=rel, numpy_host_ms_scaled_from_4_subsets=round(four * s / 4, 1))


def step_pr():
    import torch
    from invertavatar_amd import distribution_metrics as dm, hipops
    r, k, blk = {}, 3, 10000
    for n in (10000, 50000):
        for d in (512, 4096):
            manifold, probes = features(n, d, 3).half().float(), (features(n, d, 4) * 1.1).half().float()
            r2, r2b = hipops.knn_radius(manifold, k), hipops.knn_radius(manifold, k)
            cov, covb = hipops.manifold_covered(probes, manifold, r2), hipops.manifold_covered(probes, manifold, r2)
            if not (same_bits(r2, r2b) and same_bits(cov, covb)):
                raise SystemExit('ia_knn_radius / ia_manifold_covered: two runs differ')
            reps = 3 if n == 10000 else 1

            def yard_radius():
                return torch.cat([torch.cat([torch.cdist(manifold[lo:lo + blk], manifold[c:c + blk]) for c in range(0, n, blk)], 1)
                                 .kthvalue(k + 1).values for lo in range(0, n, blk)])

            def yard_covered(rad):
                return torch.cat([torch.stack([(torch.cdist(probes[lo:lo + blk], manifold[c:c + blk]) <= rad[c:c + blk]).any(1)
                                               for c in range(0, n, blk)]).any(0) for lo in range(0, n, blk)])
            rad = yard_radius()
            r[f'N{n}_D{d}'] = dict(knn_radius=timed(lambda: hipops.knn_radius(manifold, k), warmup=0, reps=reps),
                                   manifold_covered=timed(lambda: hipops.manifold_covered(probes, manifold, r2), warmup=0, reps=reps),
                                   covered_share=float(cov.float().mean().item()),
                                   torch_cdist_radius=timed(yard_radius, warmup=0, reps=reps),
                                   torch_cdist_covered=timed(lambda: yard_covered(rad), warmup=0, reps=reps),
                                   radius_max_rel_difference=float(((r2.sqrt() - rad).abs() / rad).max().item()),
                                   covered_disagree=int((cov != yard_covered(rad)).sum().item()))
    mh, ph = features(2000, 512, 3, 'cpu').half().float().numpy(), (features(2000, 512, 4, 'cpu') * 1.1).half().float().numpy()
    r['numpy_host_N2000_D512_ms'] = host_ms(lambda: dm.covered_reference(ph, mh, dm.knn_radius_reference(mh, k)))
    return r


def step_fid():
    import torch
    from invertavatar_amd import distribution_metrics as dm
    r = {}
    for d in (512, 2048):
        real, gen = features(N_ROWS, d, 5), features(N_ROWS, d, 6) * 1.1 + 0.1
        dev, host = [], []
        for x in (real, gen):
            s = dm.FeatureStats(capture_mean_cov=True)
            for lo in range(0, N_ROWS, 4096):
                s.append_torch(x[lo:lo + 4096])
            dev.append(s)
            h = dm.FeatureStats(capture_mean_cov=True)
            h.num_items, h.num_features, h.device = s.num_items, d, 'cpu'
            h.raw_mean, h.raw_cov = s.raw_mean.cpu().numpy(), s.raw_cov.cpu().numpy()
            host.append(h)
        torch.cuda.synchronize()
        vd = dm.fid(*dev)
        r[f'D{d}'] = dict(fid_device=vd, device_ms=host_ms(lambda: dm.fid(*dev)), fid_host=dm.fid(*host), host_ms=host_ms(lambda: dm.fid(*host)))
    return r


def main(argv=None):
    import argparse
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--steps', default=','.join(STEPS))
    ap.add_argument('--step', default=None, help='(internal) run one step in this process and print its JSON')
    args = ap.parse_args(argv)
    if args.step:
        print(json.dumps(globals()[f'step_{args.step}']()))
        return 0
    from invertavatar_amd import build as ia_build
    res = {'tool': 'bench_distribution', 'source_digest': ia_build.source_digest(), 'rows': N_ROWS}
    for step in args.steps.split(','):
        try:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), '--step', step], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                               timeout=STEPS[step])
        except subprocess.TimeoutExpired:
            res['stopped'] = dict(step=step, why=f'no result within {STEPS[step]} s')
            break
        if p.returncode != 0:
            res['stopped'] = dict(step=step, exit_status=p.returncode, stderr=p.stderr.decode()[-800:])
            break
        res[step] = json.loads(p.stdout.decode().strip().splitlines()[-1])
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, 'w') as fh:
            fh.write(line + '\n')
    return 1 if 'stopped' in res else 0


if __name__ == '__main__':
    raise SystemExit(main())
