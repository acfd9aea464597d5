"""Times of the device identity similarity (HIP events; one JSON line on stdout, optionally written to --out).

Synthetic weights, 256^2 and 512^2 float32 frames, N = 1, 8, 64 pairs:
(a) ``identity.compare`` end to end against the same network through PyTorch device ops in float32 on the same weights
    (``model_irse.Backbone`` with ``helpers.HIP_TRUNK = False`` and ``layers.HIP_CONVS = False``, torch's adaptive pools in front): the
    route a user has without the kernels.  Every shape is warmed; the two sides alternate in one process in windows of >= 0.3 s; the
    median window of each side is reported, also where the yardstick wins.
(b) milliseconds per kernel family inside one call (front end, input layer, trunk convolutions and splits, the 7^2 convolutions, head,
    dot), from events around every launch (``hipops.PROFILE``; launches without a record, the squeeze-and-excitation gates, are in the
    end-to-end time only), median of 3 calls.
(c) the largest difference between the two routes' per-frame scores.
(d) what scoring identity adds to a ``ClipMetrics.update`` call of 8 frames of 512^2 (the call ``drive_sequence`` makes per group),
    against the plain ``ClipMetrics`` of the parent commit.
Usage: python tools/bench_identity.py [--out FILE] [--sizes 256,512] [--batches 1,8,64]"""
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from invertavatar_amd import build as ia_build, hipops, identity, image_metrics  # noqa: E402
from invertavatar_amd.encoder_inversion.models import helpers, layers  # noqa: E402

WINDOW_S, ROUNDS = 0.3, 3
FAMILIES = {'face_crop_pool': 'front_ms', 'conv2d_mfma_k3': 'mfma_conv_ms', 'conv2d_mfma_k1': 'shortcut_conv_ms', 'act_split': 'split_ms',
            'prelu_channels': 'prelu_ms', 'conv3x3_small': 'small_conv_ms', 'id_head': 'head_ms', 'id_similarity': 'dot_ms'}


def library_route(x, y, model):
    """The same network through PyTorch device ops, float32 -> [N] scores."""
    net = model.on(x.device)['net']
    v, n = torch.cat([x, y], 0), x.shape[0]
    if tuple(v.shape[-2:]) != (identity.FRAME, identity.FRAME):
        v = F.adaptive_avg_pool2d(v, (identity.FRAME, identity.FRAME))
    v = F.adaptive_avg_pool2d(v[:, :, identity.CROP_Y:identity.CROP_Y + identity.CROP, identity.CROP_X:identity.CROP_X + identity.CROP],
                              (identity.SIDE, identity.SIDE))
    trunk, convs = helpers.HIP_TRUNK, layers.HIP_CONVS
    helpers.HIP_TRUNK = layers.HIP_CONVS = False
    try:
        f = net(v)
    finally:
        helpers.HIP_TRUNK, layers.HIP_CONVS = trunk, convs
    return (f[:n] * f[n:]).sum(1)


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
    coarse = torch.randn(n, 3, 12, 12, generator=gen)
    a = torch.tanh(F.interpolate(coarse, size=(side, side), mode='bicubic', align_corners=False))
    b = (a + 0.05 * torch.randn(n, 3, side, side, generator=gen)).clamp(-1, 1)
    return a.contiguous(), b.contiguous()


def arg(name, default):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


def main():
    out_path = arg('--out', None)
    sizes = [int(s) for s in arg('--sizes', '256,512').split(',')]
    batches = [int(s) for s in arg('--batches', '1,8,64').split(',')]
    assert torch.cuda.is_available(), 'bench_identity needs the GPU'
    res = {'source_digest': ia_build.source_digest(), 'device': torch.cuda.get_device_name(0), 'window_s': WINDOW_S, 'rounds': ROUNDS,
           'weights': 'synthetic (seed 1)', 'cases': {}}
    model = identity.IDScore.synthetic(1)
    with torch.no_grad():
        for side in sizes:
            for n in batches:
                a, b = (t.cuda() for t in frames(n, side, 5 + n))
                hip_ms, lib_ms, r_hip, r_lib = ab(lambda: identity.compare(a, b, model), lambda: library_route(a, b, model))
                got, lib = identity.compare(a, b, model)['id_sim'].double(), library_route(a, b, model).double()
                res['cases'][f'{side}_n{n}'] = dict(
                    side=side, pairs=n, hip_ms=round(hip_ms, 4), library_ms=round(lib_ms, 4), library_over_hip=round(lib_ms / hip_ms, 3),
                    reps_per_window=[r_hip, r_lib], us_per_pair_hip=round(1e3 * hip_ms / n, 2),
                    families=families(lambda: identity.compare(a, b, model)), max_difference=float((got - lib).abs().max()))
                del a, b
                torch.cuda.empty_cache()
        a, b = (t.cuda() for t in frames(8, 512, 77))
        plain, with_id = image_metrics.ClipMetrics(), image_metrics.ClipMetrics(identity=model)

        def call(clip):
            clip.reset()
            clip.update(a, b)
        plain_ms, id_ms, _, _ = ab(lambda: call(plain), lambda: call(with_id))
        res['clip_metrics_update_8x512'] = dict(plain_ms=round(plain_ms, 4), with_identity_ms=round(id_ms, 4), added_ms=round(id_ms - plain_ms, 4))
    line = json.dumps(res)
    print(line)
    if out_path:
        with open(out_path, 'w') as fh:
            fh.write(line + '\n')


if __name__ == '__main__':
    main()
