"""Times of the device LPIPS (HIP events; one JSON line on stdout, optionally written to --out).

For both backbones (synthetic weights), 256^2 and 512^2 float32 frames and N = 1, 8, 64 pairs:
(a) ``lpips.compare`` end to end against the same definition through PyTorch device ops in float32 on the same weights (conv2d,
    max_pool2d, elementwise ops, mean): the route a user has without the kernels.  Every shape is warmed; the two sides alternate in
    one process in windows of >= 0.3 s; the median window of each side is reported, also where the yardstick wins.
(b) milliseconds per kernel family inside one call (direct convolutions, MFMA convolutions, activation splits, pools, heads), from
    events around every launch (``hipops.PROFILE``), median of 3 calls.
(c) the largest relative difference between the two routes' per-frame scores.
Usage: python tools/bench_lpips.py [--out FILE] [--nets alex,vgg] [--sizes 256,512] [--batches 1,8,64]"""
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from invertavatar_amd import build as ia_build, hipops, lpips  # noqa: E402

WINDOW_S, ROUNDS = 0.3, 3
FAMILIES = {'conv2d_direct': 'direct_conv_ms', 'conv2d_mfma_k3': 'mfma_conv_ms', 'act_split': 'split_ms', 'maxpool2d': 'pool_ms',
            'lpips_layer': 'head_ms'}


def library_route(x, y, model):
    """The same definition through PyTorch device ops, float32 -> [N] scores."""
    held = model.on(x.device)
    v, n, total, i, taps = lpips._batch(x, y, torch.float32), x.shape[0], 0.0, 0, 0
    for op in model.plan:
        if op[0] == 'pool':
            v = F.max_pool2d(v, op[1], op[2])
            continue
        v = F.relu(F.conv2d(v, held['w'][i], held['b'][i], stride=op[5], padding=op[6]))
        i += 1
        if op[7]:
            f = v / (torch.sqrt((v * v).sum(1, keepdim=True)) + lpips.EPS)
            d = (f[:n] - f[n:]) ** 2
            total = total + (d * held['lin'][taps].reshape(1, -1, 1, 1)).sum(1).mean(dim=(1, 2))
            taps += 1
    return total


def window(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def reps_for(fn):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    return max(2, int(WINDOW_S * 1e3 / max(window(fn, 2), 1e-3)) + 1)


def ab(fn_a, fn_b):
    ra, rb = reps_for(fn_a), reps_for(fn_b)
    ta, tb = [], []
    for _ in range(ROUNDS):
        ta.append(window(fn_a, ra))
        tb.append(window(fn_b, rb))
    return statistics.median(ta), statistics.median(tb), ra, rb


def families(fn):
    runs = []
    for _ in range(3):
        hipops.PROFILE = []
        try:
            fn()
            torch.cuda.synchronize()
            per = {}
            for family, _, _, e0, e1, _ in hipops.PROFILE:
                per[family] = per.get(family, 0.0) + e0.elapsed_time(e1)
        finally:
            hipops.PROFILE = None
        runs.append(per)
    return {FAMILIES.get(k, k): round(statistics.median(r.get(k, 0.0) for r in runs), 4) for k in sorted(set().union(*runs))}


def frames(n, side, seed):
    gen = torch.Generator().manual_seed(seed)
    a = torch.rand(n, 3, side, side, generator=gen) * 2 - 1
    a = (F.avg_pool2d(F.pad(a, (2, 2, 2, 2), mode='reflect'), 5, stride=1) * 2.5).clamp(-1, 1)
    b = (a + 0.05 * torch.randn(n, 3, side, side, generator=gen)).clamp(-1, 1)
    return a.contiguous(), b.contiguous()


def arg(name, default):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


def main():
    out_path = arg('--out', None)
    nets = arg('--nets', 'alex,vgg').split(',')
    sizes = [int(s) for s in arg('--sizes', '256,512').split(',')]
    batches = [int(s) for s in arg('--batches', '1,8,64').split(',')]
    assert torch.cuda.is_available(), 'bench_lpips needs the GPU'
    res = {'source_digest': ia_build.source_digest(), 'device': torch.cuda.get_device_name(0), 'window_s': WINDOW_S, 'rounds': ROUNDS,
           'weights': 'synthetic (seed 1)', 'cases': {}}
    with torch.no_grad():
        for net in nets:
            model = lpips.LPIPS.synthetic(net, 1)
            for side in sizes:
                for n in batches:
                    a, b = (t.cuda() for t in frames(n, side, 5 + n))
                    hip_ms, lib_ms, r_hip, r_lib = ab(lambda: lpips.compare(a, b, model), lambda: library_route(a, b, model))
                    got, lib = lpips.compare(a, b, model)['lpips'].double(), library_route(a, b, model).double()
                    res['cases'][f'{net}_{side}_n{n}'] = dict(
                        net=net, side=side, frames=n, hip_ms=round(hip_ms, 4), library_ms=round(lib_ms, 4),
                        library_over_hip=round(lib_ms / hip_ms, 3), reps_per_window=[r_hip, r_lib], us_per_frame_hip=round(1e3 * hip_ms / n, 2),
                        families=families(lambda: lpips.compare(a, b, model)),
                        max_rel_difference=float(((got - lib).abs() / lib.abs()).max()))
                    del a, b
                    torch.cuda.empty_cache()
    line = json.dumps(res)
    print(line)
    if out_path:
        with open(out_path, 'w') as fh:
            fh.write(line + '\n')


if __name__ == '__main__':
    main()
