"""Times of the device contextual loss (HIP events; one JSON line on stdout, optionally written to --out).

For synthetic VGG19 weights, 256^2 and 512^2 float32 frames of unrelated content and N = 1, 8 pairs:
(a) ``contextual.compare`` end to end against the same definition through PyTorch device ops in float32 on the same weights, with the
    head as the reference writes it (the P x P matrices materialised) and chunked (blocks of 512 whole rows of x, whose minimum, sum and quotient are row-wise).
    Every shape is warmed; the routes alternate in one process in windows of >= 0.3 s; the median window of each is reported, also
    where a yardstick wins, with the peak device memory of one call of each route.
(b) milliseconds per kernel family inside one call (resize, direct convolutions, MFMA convolutions, splits, pools, the head's five
    kernels), from events around every launch (``hipops.PROFILE``), median of 3 calls.
(c) the largest relative difference between the routes' per-frame losses.
Usage: python tools/bench_contextual.py [--out FILE] [--sizes 256,512] [--batches 1,8]"""
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from invertavatar_amd import build as ia_build, contextual, hipops  # noqa: E402

WINDOW_S, ROUNDS, CHUNK = 0.3, 3, 512


def library_features(x, y, model):
    held = model.on(x.device)
    v, i = torch.cat([x, y], 0), 0
    if v.shape[-1] > contextual.FRAME:
        v = F.interpolate(v, (contextual.FRAME, contextual.FRAME), mode='bilinear', align_corners=False)
    for op in model.plan:
        if op[0] == 'pool':
            v = F.max_pool2d(v, op[1], op[2])
        else:
            v = F.relu(F.conv2d(v, held['w'][i], held['b'][i], padding=1))
            i += 1
    return v[:x.shape[0]], v[x.shape[0]:]


def operands(fx, fy):
    n, c = fx.shape[:2]
    mu = fy.mean(dim=(2, 3), keepdim=True)
    return F.normalize(fx - mu, p=2, dim=1).reshape(n, c, -1).transpose(1, 2), F.normalize(fy - mu, p=2, dim=1).reshape(n, c, -1)


def library_materialised(x, y, model):
    """The head as the reference writes it: distance, relative distance, exp and quotient as P x P tensors."""
    xh, yh = operands(*library_features(x, y, model))
    d = 1 - torch.bmm(xh, yh)
    t = torch.clamp(d / (d.min(dim=2, keepdim=True)[0] + 1e-5), min=-10.0, max=10.0)
    w = torch.exp((1 - t) / model.band_width)
    cx = (w / w.sum(dim=2, keepdim=True)).max(dim=1)[0].mean(dim=1)
    return -torch.log(cx + 1e-5)


def library_chunked(x, y, model):
    """The same head in blocks of CHUNK rows of x: one pass, since a block holds whole rows (minimum, sum and quotient are row-wise)."""
    xh, yh = operands(*library_features(x, y, model))
    colmax = None
    for lo in range(0, xh.shape[1], CHUNK):
        d = 1 - torch.bmm(xh[:, lo:lo + CHUNK], yh)
        t = torch.clamp(d / (d.min(dim=2, keepdim=True)[0] + 1e-5), min=-10.0, max=10.0)
        w = torch.exp((1 - t) / model.band_width)
        q = (w / w.sum(dim=2, keepdim=True)).max(dim=1)[0]
        colmax = q if colmax is None else torch.maximum(colmax, q)
    return -torch.log(colmax.mean(dim=1) + 1e-5)


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


def alternate(fns):
    reps = [reps_for(fn) for fn in fns]
    times = [[] for _ in fns]
    for _ in range(ROUNDS):
        for t, fn, r in zip(times, fns, reps):
            t.append(window(fn, r))
    return [statistics.median(t) for t in times], reps


def peak_mb(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return round((torch.cuda.max_memory_allocated() - base) / 2 ** 20, 2)


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
    return {k + '_ms': round(statistics.median(r.get(k, 0.0) for r in runs), 4) for k in sorted(set().union(*runs))}


def frames(n, side, seed):
    gen = torch.Generator().manual_seed(seed)

    def one():
        a = torch.rand(n, 3, side, side, generator=gen) * 2 - 1
        return (F.avg_pool2d(F.pad(a, (2, 2, 2, 2), mode='reflect'), 5, stride=1) * 2.5).clamp(-1, 1).contiguous()
    return one(), one()


def arg(name, default):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


def main():
    out_path = arg('--out', None)
    sizes = [int(s) for s in arg('--sizes', '256,512').split(',')]
    batches = [int(s) for s in arg('--batches', '1,8').split(',')]
    assert torch.cuda.is_available(), 'bench_contextual needs the GPU'
    res = {'source_digest': ia_build.source_digest(), 'device': torch.cuda.get_device_name(0), 'window_s': WINDOW_S, 'rounds': ROUNDS,
           'weights': 'synthetic (seed 1)', 'chunk_rows': CHUNK, 'cases': {}}
    model = contextual.CXScore.synthetic(1)
    with torch.no_grad():
        for side in sizes:
            for n in batches:
                a, b = (t.cuda() for t in frames(n, side, 5 + n))
                fns = [lambda: contextual.compare(a, b, model), lambda: library_materialised(a, b, model), lambda: library_chunked(a, b, model)]
                (hip_ms, mat_ms, chunk_ms), reps = alternate(fns)
                got = contextual.compare(a, b, model)['cx_loss'].double()
                lib = library_materialised(a, b, model).double()
                res['cases'][f'{side}_n{n}'] = dict(
                    side=side, frames=n, hip_ms=round(hip_ms, 4), library_materialised_ms=round(mat_ms, 4), library_chunked_ms=round(chunk_ms, 4),
                    materialised_over_hip=round(mat_ms / hip_ms, 3), chunked_over_hip=round(chunk_ms / hip_ms, 3), reps_per_window=reps,
                    us_per_frame_hip=round(1e3 * hip_ms / n, 2), peak_mb=dict(zip(('hip', 'library_materialised', 'library_chunked'), map(peak_mb, fns))),
                    families=families(fns[0]), max_rel_difference=float(((got - lib).abs() / lib.abs()).max()))
                del a, b
                torch.cuda.empty_cache()
    line = json.dumps(res)
    print(line)
    if out_path:
        with open(out_path, 'w') as fh:
            fh.write(line + '\n')


if __name__ == '__main__':
    main()
