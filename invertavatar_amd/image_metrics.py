"""Per-frame reconstruction scores: PSNR, SSIM and MS-SSIM of rendered frames against ground truth.

The definition is the reference's ``encoder_inversion/criteria/ms_ssim.py`` (the pytorch-msssim formulation its encoders were trained
against) with ``size_average=False`` and no ``normalize``: 11-tap Gaussian window (sigma 1.5), "valid" correlation, per channel,
five levels of 2 x 2 average pooling with the weights (0.0448, 0.2856, 0.3001, 0.2363, 0.1333); see include/ia_hip.h for the formulas.
Images smaller than 11 pixels at the last level are refused (the reference shrinks its window instead).

Device tensors go to the HIP kernel (``hipops.image_metrics``: `levels` + 1 launches for the whole batch) and never fall back; CPU
tensors and NumPy arrays take ``reference_compare``, the same definition restated in torch and computed in float64 -- the yardstick of
the device tests.  Inputs: float32 ``[N,C,H,W]`` (what ``synthesis`` returns; ``data_range`` defaults to 2.0, the generator's [-1, 1])
or uint8 ``[N,H,W,C]`` (what the output side holds; ``data_range`` defaults to 255), ``1 <= C <= 4``.

CLI:  python -m invertavatar_amd.image_metrics --pred P --gt G [--data-range R] [--levels K] [--chunk N] --out metrics.json
where P / G are ``.npy`` stacks or directories of them (sorted order).  ``--lpips alex|vgg --lpips-weights FILE --lpips-lin FILE`` adds
LPIPS (``invertavatar_amd/lpips.py``) per frame; ``--lpips-synthetic SEED`` takes seeded weights instead (smoke runs: meaningless scores).
``--id-weights FILE`` (the ArcFace IR-SE50 state dict) adds the identity similarity ``id_sim`` (``invertavatar_amd/identity.py``) per
frame; ``--id-synthetic SEED`` takes seeded weights instead.  ``--cx-weights FILE`` (a torchvision ``vgg19`` state dict) adds the contextual
score ``cx`` / ``cx_loss`` (``invertavatar_amd/contextual.py``) per frame; ``--cx-synthetic SEED`` takes seeded weights instead and
``--cx-band-width H`` sets the band width (0.5)."""
import json
import math
import os
import sys

import numpy as np
import torch

WINDOW, SIGMA = 11, 1.5
MS_WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)
MAX_LEVELS = len(MS_WEIGHTS)
KEYS = ('mse', 'l1', 'psnr', 'ssim', 'ms_ssim')


def gaussian_window(dtype=torch.float64):
    x = torch.arange(WINDOW, dtype=torch.float64) - WINDOW // 2
    g = torch.exp(-x * x / (2.0 * SIGMA ** 2))
    return (g / g.sum()).to(dtype)


def _checked(a, b, data_range, levels):
    """Validates a pair; returns (a, b, data_range) with NumPy arrays wrapped as CPU tensors."""
    if isinstance(a, np.ndarray):
        a = torch.from_numpy(a)
    if isinstance(b, np.ndarray):
        b = torch.from_numpy(b)
    if not (torch.is_tensor(a) and torch.is_tensor(b)):
        raise ValueError('image metrics take torch tensors or NumPy arrays')
    if a.dtype != b.dtype or a.dtype not in (torch.float32, torch.uint8):
        raise ValueError(f'both images must be float32 [N,C,H,W] or both uint8 [N,H,W,C], got {a.dtype} and {b.dtype}')
    if a.device != b.device:
        raise ValueError(f'images are on different devices: {a.device} and {b.device}')
    if a.dim() != 4 or a.shape != b.shape:
        raise ValueError(f'images must be two 4-D batches of the same shape, got {tuple(a.shape)} and {tuple(b.shape)}')
    if a.dtype == torch.uint8:
        n, h, w, c = a.shape
    else:
        n, c, h, w = a.shape
    if n < 1:
        raise ValueError('empty batch')
    if not 1 <= c <= 4:
        raise ValueError(f'1 to 4 channels are supported, got {c} (float32 is [N,C,H,W], uint8 is [N,H,W,C])')
    if not (isinstance(levels, int) and 1 <= levels <= MAX_LEVELS):
        raise ValueError(f'levels must be an integer in 1..{MAX_LEVELS}, got {levels!r}')
    if (min(h, w) >> (levels - 1)) < WINDOW:
        raise ValueError(f'a {h} x {w} image is too small for {levels} levels: the smaller side >> {levels - 1} must be >= {WINDOW}')
    if data_range is None:
        data_range = 255.0 if a.dtype == torch.uint8 else 2.0
    data_range = float(data_range)
    if not data_range > 0.0:
        raise ValueError(f'data_range must be positive, got {data_range}')
    return a, b, data_range


def _unpack(out, levels):
    res = {k: out[:, i] for i, k in enumerate(KEYS)}
    res['ssim_levels'] = out[:, 5:5 + levels]
    res['cs_levels'] = out[:, 5 + levels:5 + 2 * levels]
    return res


@torch.no_grad()
def reference_table(a, b, data_range, levels):
    """The definition in float64 torch ops on the inputs' device -> float64 [N, 5 + 2 * levels] (columns as ia_image_metrics)."""
    if a.dtype == torch.uint8:
        a, b = a.permute(0, 3, 1, 2), b.permute(0, 3, 1, 2)
    a, b = a.double(), b.double()
    n, c = a.shape[:2]
    L = float(data_range)
    c1, c2 = (0.01 * L) ** 2, (0.03 * L) ** 2
    d = a - b
    mse = (d * d).mean(dim=(1, 2, 3))
    l1 = d.abs().mean(dim=(1, 2, 3))
    psnr = torch.where(mse > 0, 10.0 * torch.log10(L * L / mse.clamp_min(1e-300)), torch.full_like(mse, math.inf))
    g = gaussian_window().to(a.device)
    win = (g[:, None] * g[None, :]).expand(c, 1, WINDOW, WINDOW).contiguous()
    ssims, css = [], []
    for k in range(levels):
        conv = lambda t: torch.nn.functional.conv2d(t, win, groups=c)  # noqa: E731
        mu1, mu2 = conv(a), conv(b)
        s1, s2, s12 = conv(a * a) - mu1 * mu1, conv(b * b) - mu2 * mu2, conv(a * b) - mu1 * mu2
        v1, v2 = 2.0 * s12 + c2, s1 + s2 + c2
        css.append((v1 / v2).mean(dim=(1, 2, 3)))
        ssims.append(((2.0 * mu1 * mu2 + c1) * v1 / ((mu1 * mu1 + mu2 * mu2 + c1) * v2)).mean(dim=(1, 2, 3)))
        if k + 1 < levels:
            a, b = torch.nn.functional.avg_pool2d(a, 2), torch.nn.functional.avg_pool2d(b, 2)
    ssims, css = torch.stack(ssims, 1), torch.stack(css, 1)
    if levels == MAX_LEVELS:
        w = torch.tensor(MS_WEIGHTS, dtype=torch.float64, device=a.device)
        ms = torch.prod(css[:, :-1] ** w[:-1], dim=1) * ssims[:, -1] ** w[-1]
    else:
        ms = torch.full_like(mse, math.nan)              # MS-SSIM is defined on five levels only
    return torch.cat([torch.stack([mse, l1, psnr, ssims[:, 0], ms], 1), ssims, css], 1)


def reference_compare(a, b, data_range=None, levels=MAX_LEVELS):
    """``compare`` through the float64 restatement, wherever the inputs live; results as float32."""
    a, b, data_range = _checked(a, b, data_range, levels)
    return _unpack(reference_table(a, b, data_range, levels).float(), levels)


@torch.no_grad()
def compare(a, b, data_range=None, levels=MAX_LEVELS):
    """Per-frame scores of `a` against `b`: dict of float32 [N] tensors ``mse, l1, psnr, ssim, ms_ssim`` and [N, levels] tensors
    ``ssim_levels, cs_levels`` on the inputs' device.  With ``levels < 5``, ``ms_ssim`` is NaN (MS-SSIM is defined on five levels).
    Device tensors: the HIP kernel, no fallback.  CPU tensors / NumPy arrays: the float64 restatement."""
    a, b, data_range = _checked(a, b, data_range, levels)
    if not a.is_cuda:
        return _unpack(reference_table(a, b, data_range, levels).float(), levels)
    from . import hipops
    return _unpack(hipops.image_metrics(a.contiguous(), b.contiguous(), data_range, levels), levels)


def psnr(a, b, data_range=None):
    return compare(a, b, data_range, levels=1)['psnr']


def ssim(a, b, data_range=None):
    return compare(a, b, data_range, levels=1)['ssim']


def ms_ssim(a, b, data_range=None):
    return compare(a, b, data_range, levels=MAX_LEVELS)['ms_ssim']


class ClipMetrics:
    """Scores of a clip, gathered call by call: ``update`` keeps each call's per-frame results where they were computed (no host
    synchronisation); ``summary`` makes the clip's one device -> host read."""

    def __init__(self, data_range=2.0, levels=MAX_LEVELS, lpips=None, identity=None, contextual=None):
        self.data_range, self.levels, self.lpips = data_range, levels, lpips      # lpips: an lpips.LPIPS model, or None
        self.identity = identity                                                  # an identity.IDScore model, or None
        self.contextual = contextual                                              # a contextual.CXScore model, or None
        self._calls = []

    def update(self, pred, gt):
        res = compare(pred, gt, self.data_range, self.levels)
        if self.lpips is not None:
            from . import lpips as _lpips
            res.update(_lpips.compare(pred, gt, self.lpips, self.data_range))
        if self.identity is not None:
            from . import identity as _identity
            res.update(_identity.compare(pred, gt, self.identity, self.data_range))
        if self.contextual is not None:
            from . import contextual as _contextual
            res.update(_contextual.compare(pred, gt, self.contextual, self.data_range))
        self._calls.append(res)
        return res

    def reset(self):
        self._calls = []

    def per_frame(self):
        """{name: tensor over all frames so far} on the device of the first call."""
        if not self._calls:
            raise ValueError('no frames were scored')
        dev = self._calls[0]['mse'].device
        return {k: torch.cat([c[k].to(dev) for c in self._calls], 0) for k in self._calls[0]}

    def summary(self):
        pf = self.per_frame()
        names = list(pf)
        table = torch.cat([pf[k].reshape(pf[k].shape[0], -1).double() for k in names], 1).cpu()      # the one read
        frames, res, col = table.shape[0], {'frames': table.shape[0], 'data_range': self.data_range, 'levels': self.levels,
                                            'mean': {}, 'min': {}, 'max': {}, 'per_frame': {}}, 0
        for k in names:
            width = 1 if pf[k].dim() == 1 else pf[k].shape[1]
            block = table[:, col:col + width]
            col += width
            if pf[k].dim() == 1:
                vals = [float(v) for v in block[:, 0]]
                res['per_frame'][k] = vals
                res['mean'][k], res['min'][k], res['max'][k] = sum(vals) / frames, min(vals), max(vals)
            else:
                res['per_frame'][k] = [[float(v) for v in row] for row in block]
        return res

    def write_json(self, path):
        res = self.summary()
        with open(path, 'w') as fh:
            json.dump(res, fh)              # (inf / nan are written as Infinity / NaN, which json.load reads back)
            fh.write('\n')
        return res


def _stack_files(path):
    if os.path.isdir(path):
        files = sorted(os.path.join(path, f) for f in os.listdir(path) if f.endswith('.npy'))
        if not files:
            raise ValueError(f'no .npy files in {path}')
        return files
    return [path]


def _frames(files):
    """Yields the arrays of the stacks one after the other, memory-mapped; a 3-D array is one frame."""
    for f in files:
        arr = np.load(f, mmap_mode='r')
        yield arr[None] if arr.ndim == 3 else arr


def score_files(pred, gt, data_range=None, levels=MAX_LEVELS, chunk=16, device=None, lpips=None, identity=None, contextual=None):
    """Scores two ``.npy`` stacks (or directories of them) chunk by chunk -> ClipMetrics (with LPIPS when `lpips` is a model, with the
    identity similarity when `identity` is one, with the contextual score when `contextual` is one)."""
    device = device or ('cuda' if torch.cuda.is_available() else 'cpu')
    p_files, g_files = _stack_files(pred), _stack_files(gt)
    if len(p_files) != len(g_files):
        raise ValueError(f'{len(p_files)} prediction stacks against {len(g_files)} ground-truth stacks')
    clip = None
    for pa, ga in zip(_frames(p_files), _frames(g_files)):
        if pa.shape != ga.shape or pa.dtype != ga.dtype:
            raise ValueError(f'stacks differ: {pa.dtype} {pa.shape} against {ga.dtype} {ga.shape}')
        for lo in range(0, pa.shape[0], chunk):
            a = torch.from_numpy(np.array(pa[lo:lo + chunk])).to(device)
            b = torch.from_numpy(np.array(ga[lo:lo + chunk])).to(device)
            if clip is None:
                clip = ClipMetrics(data_range if data_range is not None else (255.0 if a.dtype == torch.uint8 else 2.0), levels, lpips, identity, contextual)
            clip.update(a, b)
    return clip


def main(argv=None):
    import argparse
    ap = argparse.ArgumentParser(description='PSNR / SSIM / MS-SSIM per frame of two .npy stacks ([F,3,H,W] float32 or [F,H,W,3] uint8)')
    ap.add_argument('--pred', required=True)
    ap.add_argument('--gt', required=True)
    ap.add_argument('--data-range', type=float, default=None, help='default: 2.0 for float32 ([-1, 1]), 255 for uint8')
    ap.add_argument('--levels', type=int, default=MAX_LEVELS)
    ap.add_argument('--chunk', type=int, default=16, help='frames per device call')
    ap.add_argument('--device', default=None)
    ap.add_argument('--out', required=True)
    ap.add_argument('--lpips', choices=('alex', 'vgg'), default=None, help='also score LPIPS with this backbone')
    ap.add_argument('--lpips-weights', default=None, help="the backbone's torchvision state dict (alexnet / vgg16)")
    ap.add_argument('--lpips-lin', default=None, help='the LPIPS v0.1 linear layers of the backbone')
    ap.add_argument('--lpips-synthetic', type=int, default=None, metavar='SEED', help='seeded weights instead of files (smoke runs only)')
    ap.add_argument('--id-weights', default=None, help='also score identity similarity: the ArcFace IR-SE50 state dict (model_ir_se50.pth)')
    ap.add_argument('--id-synthetic', type=int, default=None, metavar='SEED', help='seeded identity weights instead of a file (smoke runs only)')
    ap.add_argument('--cx-weights', default=None, help='also score the contextual loss: a torchvision vgg19 state dict')
    ap.add_argument('--cx-synthetic', type=int, default=None, metavar='SEED', help='seeded VGG19 weights instead of a file (smoke runs only)')
    ap.add_argument('--cx-band-width', type=float, default=None, metavar='H', help='band width of the contextual loss (default 0.5)')
    args = ap.parse_args(argv)
    model = None
    if args.lpips is not None:
        from . import lpips as _lpips
        if args.lpips_synthetic is not None:
            print(f'warning: LPIPS with synthetic weights (seed {args.lpips_synthetic}): the lpips numbers mean nothing', file=sys.stderr)
            model = _lpips.LPIPS.synthetic(args.lpips, args.lpips_synthetic)
        elif args.lpips_weights and args.lpips_lin:
            model = _lpips.LPIPS(args.lpips, args.lpips_weights, args.lpips_lin)
        else:
            ap.error('--lpips needs --lpips-weights and --lpips-lin (or --lpips-synthetic SEED)')
    elif args.lpips_weights or args.lpips_lin or args.lpips_synthetic is not None:
        ap.error('--lpips-weights / --lpips-lin / --lpips-synthetic need --lpips alex|vgg')
    id_model = None
    if args.id_weights is not None and args.id_synthetic is not None:
        ap.error('--id-weights and --id-synthetic exclude each other')
    if args.id_synthetic is not None:
        from . import identity as _identity
        print(f'warning: identity similarity with synthetic weights (seed {args.id_synthetic}): the id_sim numbers mean nothing', file=sys.stderr)
        id_model = _identity.IDScore.synthetic(args.id_synthetic)
    elif args.id_weights is not None:
        from . import identity as _identity
        id_model = _identity.IDScore(args.id_weights)
    cx_model = None
    if args.cx_weights is not None and args.cx_synthetic is not None:
        ap.error('--cx-weights and --cx-synthetic exclude each other')
    if args.cx_band_width is not None and args.cx_weights is None and args.cx_synthetic is None:
        ap.error('--cx-band-width needs --cx-weights FILE or --cx-synthetic SEED')
    if args.cx_synthetic is not None:
        from . import contextual as _contextual
        print(f'warning: contextual loss with synthetic weights (seed {args.cx_synthetic}): the cx numbers mean nothing', file=sys.stderr)
        cx_model = _contextual.CXScore.synthetic(args.cx_synthetic, 0.5 if args.cx_band_width is None else args.cx_band_width)
    elif args.cx_weights is not None:
        from . import contextual as _contextual
        cx_model = _contextual.CXScore(args.cx_weights, 0.5 if args.cx_band_width is None else args.cx_band_width)
    res = score_files(args.pred, args.gt, args.data_range, args.levels, args.chunk, args.device, model, id_model, cx_model).write_json(args.out)
    print(json.dumps({'frames': res['frames'], 'mean': res['mean']}))
    return 0


if __name__ == '__main__':
    raise SystemExit(main())
