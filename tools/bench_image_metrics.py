"""Times of the device image metrics (HIP events; one JSON line on stdout, optionally written to --out).

(a) ``image_metrics.compare`` on N = 1, 8, 64 pairs of 3 x 512^2 float32 frames and N = 8 uint8 NHWC pairs, against the same definition
    through PyTorch device ops in float32 (grouped conv2d with the 11 x 11 window, elementwise maps, avg_pool2d, mean): the route a
    user has without the kernel.  Every shape is warmed; the two sides alternate in one process in windows of >= 0.5 s; the median
    window of each side is reported.
(b) algorithmic bytes (both images read once at every level, pooled pairs written once) over the call time, as a share of the
    achievable (6.3 TB/s) and peak (8 TB/s) HBM rate, and launches per call.
(c) ``eval_seq.drive_sequence`` on the synthetic full-width network, 64 frames with ground truth, with and without ``metrics``.
(d) the largest distances of the device results from the float64 restatement on N = 8 (float32 and uint8).
Usage: python tools/bench_image_metrics.py [--out FILE] [--skip-drive]"""
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from invertavatar_amd import build as ia_build, image_metrics as im  # noqa: E402

WINDOW_S, ROUNDS = 0.5, 3
HBM_ACHIEVABLE, HBM_PEAK = 6.3e12, 8.0e12


def library_route(a, b, data_range, levels=5):
    """The same definition through PyTorch device ops, float32."""
    if a.dtype == torch.uint8:
        a, b = a.permute(0, 3, 1, 2).float(), b.permute(0, 3, 1, 2).float()
    c = a.shape[1]
    g = im.gaussian_window(torch.float32).to(a.device)
    win = (g[:, None] * g[None, :]).expand(c, 1, im.WINDOW, im.WINDOW).contiguous()
    c1, c2 = (0.01 * data_range) ** 2, (0.03 * data_range) ** 2
    d = a - b
    mse, l1 = (d * d).mean(dim=(1, 2, 3)), d.abs().mean(dim=(1, 2, 3))
    psnr = 10.0 * torch.log10(data_range ** 2 / mse)
    ssims, css = [], []
    for k in range(levels):
        mu1, mu2 = F.conv2d(a, win, groups=c), F.conv2d(b, win, groups=c)
        s1 = F.conv2d(a * a, win, groups=c) - mu1 * mu1
        s2 = F.conv2d(b * b, win, groups=c) - mu2 * mu2
        s12 = F.conv2d(a * b, win, groups=c) - mu1 * mu2
        v1, v2 = 2.0 * s12 + c2, s1 + s2 + c2
        css.append((v1 / v2).mean(dim=(1, 2, 3)))
        ssims.append(((2.0 * mu1 * mu2 + c1) * v1 / ((mu1 * mu1 + mu2 * mu2 + c1) * v2)).mean(dim=(1, 2, 3)))
        if k + 1 < levels:
            a, b = F.avg_pool2d(a, 2), F.avg_pool2d(b, 2)
    w = torch.tensor(im.MS_WEIGHTS, device=a.device)
    ssims, css = torch.stack(ssims, 1), torch.stack(css, 1)
    ms = torch.prod(css[:, :-1] ** w[:-1], dim=1) * ssims[:, -1] ** w[-1]
    return mse, l1, psnr, ssims, css, ms


def window(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def reps_for(fn):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    return max(3, int(WINDOW_S * 1e3 / max(window(fn, 5), 1e-3)) + 1)


def ab(fn_a, fn_b):
    ra, rb = reps_for(fn_a), reps_for(fn_b)
    ta, tb = [], []
    for _ in range(ROUNDS):
        ta.append(window(fn_a, ra))
        tb.append(window(fn_b, rb))
    return statistics.median(ta), statistics.median(tb), ra, rb


def algorithmic_bytes(n, c, h, w, elem, levels=5):
    total = 0
    for k in range(levels):
        total += 2 * n * c * (h >> k) * (w >> k) * (elem if k == 0 else 4)
        if k + 1 < levels:
            total += 2 * n * c * (h >> (k + 1)) * (w >> (k + 1)) * 4
    return total


def frames(n, seed):
    gen = torch.Generator().manual_seed(seed)
    a = torch.rand(n, 3, 512, 512, generator=gen) * 2 - 1
    a = F.avg_pool2d(F.pad(a, (2, 2, 2, 2), mode='reflect'), 5, stride=1) * 2.5 + 0.1 * (torch.rand(n, 3, 512, 512, generator=gen) - 0.5)
    a = a.clamp(-1, 1)
    b = (a + 0.05 * torch.randn(n, 3, 512, 512, generator=gen)).clamp(-1, 1)
    return a.contiguous(), b.contiguous()


def to_u8(t):
    return ((t + 1.0) * 127.5).round().clamp(0, 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous()


def drive_leg():
    from invertavatar_amd import eval_seq, synthetic
    from invertavatar_amd.encoder_inversion.models.uvnet import inversionNet
    from invertavatar_amd.training_avatar_texture.triplane_v20 import TriPlaneGenerator
    g = synthetic.fill_parameters(TriPlaneGenerator(**synthetic.generator_kwargs('full')).eval().requires_grad_(False))
    net = inversionNet(generator=g, encoding_triplane=True, encoding_texture=True).requires_grad_(False)
    synthetic.fill_encoder_parameters(net)
    net = eval_seq.set_eval_seq_modes(net.cuda())
    g = net.generator
    n, nrr = 64, 128
    fr = list(range(n))
    c, uv = synthetic.camera_labels(fr).cuda(), synthetic.uv_conditions(fr).cuda()
    with torch.no_grad():
        ws = g.mapping(synthetic.latent(3, 1).cuda(), synthetic.conditioning_camera().cuda(), truncation_psi=0.7, truncation_cutoff=14)
        res = {'w': ws,
               'texture': g.texture_backbone.synthesis(ws, cond_list=None, return_list=True, update_emas=False, noise_mode='const'),
               'static': g.backbone.synthesis(ws, cond_list=None, return_list=True, update_emas=False, noise_mode='const')}
        images, _ = eval_seq.drive_sequence(net, ws, res, c, uv, neural_rendering_resolution=nrr)          # capture + warm-up
        gt = (images + 0.05 * torch.randn_like(images)).clamp(-1, 1)

        def run(**kw):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            eval_seq.drive_sequence(net, ws, res, c, uv, neural_rendering_resolution=nrr, **kw)
            torch.cuda.synchronize()
            return n / (time.perf_counter() - t0)
        clip = im.ClipMetrics()
        run(gt=gt, metrics=clip)                                                                          # warm the metric shapes
        fps = {'no_gt': [], 'gt': [], 'gt_metrics': []}
        for _ in range(5):
            fps['no_gt'].append(run())
            fps['gt'].append(run(gt=gt))
            clip.reset()
            fps['gt_metrics'].append(run(gt=gt, metrics=clip))
        s = clip.summary()
    med = {k: round(statistics.median(v), 1) for k, v in fps.items()}
    return dict(frames=n, nrr=nrr, network='synthetic full width', frames_per_s=med,
                metrics_cost_percent=round(100.0 * (1.0 - med['gt_metrics'] / med['gt']), 2),
                clip_mean={k: round(v, 5) for k, v in s['mean'].items()},
                note='gt = the mosaics of today (layout_grid per frame) are built in both gt legs; median of 5 alternating runs, wall clock around synchronised calls')


def main():
    out_path = sys.argv[sys.argv.index('--out') + 1] if '--out' in sys.argv else None
    assert torch.cuda.is_available(), 'bench_image_metrics needs the GPU'
    res = {'source_digest': ia_build.source_digest(), 'device': torch.cuda.get_device_name(0), 'window_s': WINDOW_S, 'rounds': ROUNDS, 'compare': {}}
    with torch.no_grad():
        for name, n, u8 in (('f32_n1', 1, False), ('f32_n8', 8, False), ('f32_n64', 64, False), ('u8_n8', 8, True)):
            a, b = frames(n, 5 + n)
            if u8:
                a, b = to_u8(a), to_u8(b)
            a, b = a.cuda(), b.cuda()
            L = 255.0 if u8 else 2.0
            hip_ms, lib_ms, r_hip, r_lib = ab(lambda: im.compare(a, b, L), lambda: library_route(a, b, L))
            nbytes = algorithmic_bytes(n, 3, 512, 512, 1 if u8 else 4)
            res['compare'][name] = dict(frames=n, hip_ms=round(hip_ms, 4), library_ms=round(lib_ms, 4), library_over_hip=round(lib_ms / hip_ms, 2),
                                        reps_per_window=[r_hip, r_lib], us_per_frame_hip=round(1e3 * hip_ms / n, 3),
                                        algorithmic_mb=round(nbytes / 1e6, 3), tb_per_s=round(nbytes / (hip_ms * 1e-3) / 1e12, 3),
                                        share_of_achievable_hbm=round(nbytes / (hip_ms * 1e-3) / HBM_ACHIEVABLE, 3),
                                        share_of_peak_hbm=round(nbytes / (hip_ms * 1e-3) / HBM_PEAK, 3), launches_per_call=6)
            if n == 8:
                want = im.reference_table(a.cpu(), b.cpu(), L, 5)
                got = im.compare(a, b, L)
                lib = library_route(a, b, L)
                res['compare'][name]['max_abs_vs_float64'] = dict(
                    ssim=float((got['ssim_levels'].cpu().double() - want[:, 5:10]).abs().max()),
                    cs=float((got['cs_levels'].cpu().double() - want[:, 10:15]).abs().max()),
                    ms_ssim=float((got['ms_ssim'].cpu().double() - want[:, 4]).abs().max()),
                    mse_rel=float(((got['mse'].cpu().double() - want[:, 0]).abs() / want[:, 0]).max()),
                    library_ssim=float((lib[3].cpu().double() - want[:, 5:10]).abs().max()),
                    library_ms_ssim=float((lib[5].cpu().double() - want[:, 4]).abs().max()))
        if '--skip-drive' not in sys.argv:
            res['drive_sequence'] = drive_leg()
    line = json.dumps(res)
    print(line)
    if out_path:
        with open(out_path, 'w') as fh:
            fh.write(line + '\n')


if __name__ == '__main__':
    main()
