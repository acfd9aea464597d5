"""Tensor-level wrappers over the C ABI for the generator's fused HIP stages.

Each function allocates its output with torch (device memory is plumbing), passes raw
pointers to libia_hip.so on torch's current stream and raises on any non-zero status.
None of them has a CPU path: they are only ever called with device tensors."""
import contextlib
import contextvars
import ctypes
import math
import os
import weakref

import torch

from . import _lib

ACT_ID = {'linear': 1, 'lrelu': 3}

# Optional per-launch timing for bench.py's roofline leg: when PROFILE is a list, every fused stage appends
# (kernel family, algorithmic FLOPs, algorithmic HBM bytes, start event, end event, shape note) recorded on the launch stream.
PROFILE = None


class _Timed:
    def __init__(self, family, flops, nbytes, desc=''):
        self.args = (family, float(flops), float(nbytes))
        self.desc = desc

    def __enter__(self):
        if PROFILE is not None:
            self.e0 = torch.cuda.Event(enable_timing=True)
            self.e1 = torch.cuda.Event(enable_timing=True)
            self.e0.record()
        return self

    def __exit__(self, *exc):
        if PROFILE is not None:
            self.e1.record()
            PROFILE.append(self.args + (self.e0, self.e1, self.desc))
        return False


def _p(t):
    return None if t is None else t.data_ptr()


def _f32c(t, what):
    if not (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()):
        raise RuntimeError(f'{what} must be a contiguous float32 device tensor')
    return t


def pack_conv_weight(w):
    """[O, I, kh, kw] -> [kh*kw, I, O] (tap-major, out-channel contiguous): the layout ia_conv2d_mfma reads."""
    o, i, kh, kw = w.shape
    return w.detach().permute(2, 3, 1, 0).reshape(kh * kw, i, o).contiguous()


def pack_conv_weight_h(w):
    """[O, I, kh, kw] -> fp16 [kh*kw, I/8, O, 8] (channel octets innermost): the layout ia_conv2d_mfma_h reads."""
    o, i, kh, kw = w.shape
    if i % 8:
        raise RuntimeError('fp16 packing needs in_channels % 8 == 0')
    return w.detach().permute(2, 3, 1, 0).reshape(kh * kw, i // 8, 8, o).permute(0, 1, 3, 2).contiguous().to(torch.float16)


def pack_conv_weight_split(w):
    """[O, I, kh, kw] -> fp16 [2, kh*kw, I/8, O, 8]: hi = fp16(w * 2^e) and lo = fp16(w * 2^e - hi), the layout ia_conv2d_mfma_s
    reads.  e (returned as the tensor attribute `wk_exp`) is the largest power of two with max|w| * 2^e <= 32768: it keeps the
    low parts, and the high parts times 2^-11, normal fp16 numbers (the MFMA flushes denormals)."""
    w = w.detach().float()
    top = float(w.abs().max())
    e = 0 if not (top > 0.0 and math.isfinite(top)) else max(-14, min(30, math.floor(math.log2(32768.0 / top))))
    ws = w * (2.0 ** e)
    hi = ws.to(torch.float16)
    lo = (ws - hi.float()).to(torch.float16)
    out = torch.stack([pack_conv_weight_h(hi), pack_conv_weight_h(lo)]).contiguous()
    out.wk_exp = int(e)
    return out


def conv_h_supported(i, o, h, w, ksize, transposed):
    """Shapes ia_conv2d_mfma_h covers (see include/ia_hip.h)."""
    if ksize != 3 or i % 8 or o % 4:
        return False
    if transposed:
        return (h + 1) * (w + 1) > 320
    return o >= 128 and h * w >= 1024 and w <= 512


def conv_sx_supported(i, o, h, w, ksize, transposed):
    """Shapes the split-DMA form (ia_conv2d_mfma_sx) covers: the library's own rule (ia_conv2d_sx_supported) -- 3x3 layers from 8^2 up
    (the 4^2 layers stay on the fp32 tiles: no gain measured)."""
    return bool(_lib.load().ia_conv2d_sx_supported(int(i), int(o), int(h), int(w), int(ksize), int(bool(transposed))))


def weight_sq_sum(w):
    """wsq[o, i] = sum over taps of w^2: the static half of the demodulation reduction."""
    return w.detach().float().square().sum(dim=[2, 3]).contiguous()


def modconv_demod(styles, wsq):
    b, i = styles.shape
    o = wsq.shape[0]
    d = torch.empty(b, o, device=styles.device, dtype=torch.float32)
    st = _lib.load().ia_modconv_demod(_p(_f32c(styles, 'styles')), _p(_f32c(wsq, 'wsq')), _p(d), b, i, o, _lib.stream_ptr(styles.device))
    _lib.check(st, 'ia_modconv_demod')
    return d


# Stream-K accumulator slabs (caller-owned memory, as the ABI requires).  Launches on different streams may overlap, so a slab
# is keyed by (device, stream).  A captured graph may be replayed on any stream, concurrently with eager launches or with other
# graphs, so each GraphedSynthesis brings its OWN registry (scratch_owner) for the duration of its capture; the registry dies
# with the graph object.  The default registry serves eager launches.
_default_scratch = {}
_scratch_registry = contextvars.ContextVar('ia_scratch_registry', default=None)


@contextlib.contextmanager
def scratch_owner(registry):
    """Route the scratch allocations of the launches issued inside the block to `registry` (a dict the caller keeps alive)."""
    token = _scratch_registry.set(registry)
    try:
        yield registry
    finally:
        _scratch_registry.reset(token)


def _scratch_buffer(device, nbytes):
    """Grow-only scratch for the stream-K accumulator slabs, one per (device, stream) of the active registry."""
    reg = _scratch_registry.get()
    if reg is None:
        reg = _default_scratch
    key = (device, torch.cuda.current_stream(device).cuda_stream)
    buf = reg.get(key)
    if buf is None or buf.numel() * 4 < nbytes:
        buf = torch.empty((nbytes + 3) // 4, device=device, dtype=torch.float32)
        reg[key] = buf
    return buf


def conv2d_mfma(x, wk, styles=None, demod=None, noise=None, noise_strength=None, bias=None, residual=None,
                ksize=3, transposed=False, act='linear', alpha=0.2, gain=1.0, clamp=None, ksplit=None):
    """One fused StyleGAN2 convolution (see ia_conv2d_mfma in include/ia_hip.h).  A float16 `wk` (pack_conv_weight_h)
    selects the fp16-operand form ia_conv2d_mfma_h."""
    _f32c(x, 'x')
    b, i, h, w = x.shape
    half_ops = wk.dtype == torch.float16
    split = half_ops and wk.dim() == 5
    if half_ops:
        if not (wk.is_cuda and wk.is_contiguous() and wk.dim() in (4, 5) and wk.shape[-1] == 8 and (not split or wk.shape[0] == 2)):
            raise RuntimeError('wk must be a contiguous fp16 [taps, I/8, O, 8] (or [2, taps, I/8, O, 8] hi/lo) device tensor')
        if split and not hasattr(wk, 'wk_exp'):
            raise RuntimeError('hi/lo weights must come from pack_conv_weight_split (they carry their scale as .wk_exp)')
        taps, wi, o = wk.shape[-4], wk.shape[-3] * 8, wk.shape[-2]
    else:
        _f32c(wk, 'wk')
        taps, wi, o = wk.shape
    if taps != ksize * ksize or wi != i:
        raise RuntimeError(f'packed weight {tuple(wk.shape)} does not match ksize {ksize}, in-channels {i}')
    for name, t in (('styles', styles), ('demod', demod), ('noise', noise), ('bias', bias), ('residual', residual)):
        if t is not None:
            _f32c(t, name)
    lib = _lib.load()
    plan_s, plan_bytes = ctypes.c_int(0), ctypes.c_size_t(0)
    form = 2 if split else (1 if half_ops else 0)
    _lib.check(lib.ia_conv2d_plan(b, i, o, h, w, ksize, int(transposed), form, ctypes.byref(plan_s), ctypes.byref(plan_bytes)), 'ia_conv2d_plan')
    nbytes = plan_bytes.value
    if ksplit is None:
        ksplit = plan_s.value
    elif plan_s.value > 0 and ksplit != plan_s.value:   # caller-chosen worker count (tests): scale the slabs with it
        nbytes = nbytes // plan_s.value * max(int(ksplit), 1)
    oh, ow = (2 * h + 1, 2 * w + 1) if transposed else (h, w)
    y = torch.empty(b, o, oh, ow, device=x.device, dtype=torch.float32)
    scratch = None
    if nbytes:
        scratch = _scratch_buffer(x.device, nbytes)
    flops = 2.0 * b * h * w * i * o * ksize * ksize
    traffic = 4.0 * (x.numel() + wk.numel() + y.numel() + (residual.numel() if residual is not None else 0))
    with torch.cuda.device(x.device), _Timed('conv2d_mfma_t' if transposed else f'conv2d_mfma_k{ksize}', flops, traffic,
                                             f'B{b} I{i} O{o} {h}x{w} G{ksplit}' + (' f16x3' if split else (' f16' if half_ops else ''))):
        fn = lib.ia_conv2d_mfma_s if split else (lib.ia_conv2d_mfma_h if half_ops else lib.ia_conv2d_mfma)
        head = (_p(x), _p(wk), int(wk.wk_exp)) if split else (_p(x), _p(wk))
        st = fn(*head, _p(styles), _p(demod), _p(noise), _p(noise_strength), _p(bias), _p(residual),
                                _p(y), _p(scratch), nbytes, b, i, o, h, w, ksize, int(transposed), ACT_ID[act], float(alpha),
                                float(gain), float(-1 if clamp is None else clamp), int(ksplit), _lib.stream_ptr(x.device))
    _lib.check(st, 'ia_conv2d_mfma')
    return y


def conv1x1_supported(i, o, h, w):
    """Shapes ia_conv1x1 covers (see include/ia_hip.h)."""
    return o <= 96 and i % 32 == 0 and (h * w) % 4 == 0


def conv1x1(x, wk, styles=None, bias=None, residual=None, clamp=None):
    """ToRGB layer in one streaming launch (see ia_conv1x1): clamp((wk * styles) (*) x + bias) + residual.  wk [1, I, O] or [I, O]
    (pack_conv_weight of a 1x1 weight)."""
    _f32c(x, 'x')
    _f32c(wk, 'wk')
    b, i, h, w = x.shape
    o = wk.shape[-1]
    if wk.numel() != i * o:
        raise RuntimeError(f'wk has {wk.numel()} elements, expected {i} x {o}')
    for t, name, n in ((styles, 'styles', b * i), (bias, 'bias', o), (residual, 'residual', b * o * h * w)):
        if t is not None and (_f32c(t, name).numel() != n):
            raise RuntimeError(f'{name} has {t.numel()} elements, expected {n}')
    y = torch.empty(b, o, h, w, device=x.device, dtype=torch.float32)
    flops = 2.0 * b * h * w * i * o
    traffic = 4.0 * (x.numel() + wk.numel() + y.numel() + (residual.numel() if residual is not None else 0))
    with torch.cuda.device(x.device), _Timed('conv1x1', flops, traffic, f'B{b} I{i} O{o} {h}x{w}'):
        st = _lib.load().ia_conv1x1(_p(x), _p(wk), _p(styles), _p(bias), _p(residual), _p(y), b, i, o, h, w,
                                    float(-1 if clamp is None else clamp), _lib.stream_ptr(x.device))
    _lib.check(st, 'ia_conv1x1')
    return y


def torgb_supported(i, o, h, w, with_skip=False):
    """Shapes ia_torgb covers (see include/ia_hip.h)."""
    return o <= 96 and i in (128, 256, 512, 1024) and not (with_skip and (h % 2 or w % 2))


def torgb(x, wk, styles=None, bias=None, residual=None, skip=None, skip_filter=None, clamp=None):
    """ToRGB layer + the skip-image branch in one launch (see ia_torgb): clamp((wk * styles) (*) x + bias) + residual, or
    + upsample2d(skip, skip_filter) with skip [B, O, H/2, W/2] and the [4, 4] resample filter."""
    _f32c(x, 'x')
    _f32c(wk, 'wk')
    b, i, h, w = x.shape
    o = wk.shape[-1]
    if wk.numel() != i * o:
        raise RuntimeError(f'wk has {wk.numel()} elements, expected {i} x {o}')
    if residual is not None and skip is not None:
        raise RuntimeError('either a residual image or a skip image, not both')
    for t, name, n in ((styles, 'styles', b * i), (bias, 'bias', o), (residual, 'residual', b * o * h * w),
                       (skip, 'skip', b * o * (h // 2) * (w // 2)), (skip_filter, 'skip_filter', 16)):
        if t is not None and (_f32c(t, name).numel() != n):
            raise RuntimeError(f'{name} has {t.numel()} elements, expected {n}')
    if skip is not None and skip_filter is None:
        raise RuntimeError('skip needs skip_filter (the [4, 4] resample filter)')
    y = torch.empty(b, o, h, w, device=x.device, dtype=torch.float32)
    flops = 2.0 * b * h * w * i * o
    traffic = 4.0 * (x.numel() + wk.numel() + y.numel() + (residual.numel() if residual is not None else 0) + (skip.numel() if skip is not None else 0))
    with torch.cuda.device(x.device), _Timed('conv1x1', flops, traffic, f'B{b} I{i} O{o} {h}x{w} torgb'):
        st = _lib.load().ia_torgb(_p(x), _p(wk), _p(styles), _p(bias), _p(residual), _p(skip), _p(skip_filter), _p(y), b, i, o, h, w,
                                  float(-1 if clamp is None else clamp), _lib.stream_ptr(x.device))
    _lib.check(st, 'ia_torgb')
    return y


# Debug switch: every producer of a SplitAct counts the elements its hi / lo split clamped at +-65504 (ia_split_saturation_count) and
# raises when there are any -- the range contract of the fp16-pair convolutions, otherwise silent (one sync per producer: tests only).
CHECK_SPLIT_RANGE = False


def split_saturation_poll(device=None, reset=True):
    """True when any hi / lo split on `device` since the last reset met a value outside +-65504 (it was clamped): the always-on
    range watch of the fp16-pair convolutions (ia_split_saturation_poll; a device -> host read, not for captured regions)."""
    device = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
    flag = ctypes.c_uint(0)
    with torch.cuda.device(device):
        st = _lib.load().ia_split_saturation_poll(ctypes.byref(flag), int(bool(reset)), _lib.stream_ptr(device))
    _lib.check(st, 'ia_split_saturation_poll')
    return flag.value != 0


def split_saturation_clear(device=None):
    """Clear the range-watch flags of `device` in stream order; no host synchronisation (the top of a clip / an inversion)."""
    device = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
    with torch.cuda.device(device):
        st = _lib.load().ia_split_saturation_poll(None, 1, _lib.stream_ptr(device))
    _lib.check(st, 'ia_split_saturation_poll')


def split_saturation_count(sa):
    """Elements of the SplitAct's hi plane that sit on the fp16 maximum (a device -> host sync)."""
    b, c, h, w = sa.shape
    cnt = torch.zeros(1, device=sa.data.device, dtype=torch.int32)
    with torch.cuda.device(sa.data.device):
        st = _lib.load().ia_split_saturation_count(_p(sa.data), int(sa.planes), b, c, h, w, _p(cnt), _lib.stream_ptr(sa.data.device))
    _lib.check(st, 'ia_split_saturation_count')
    return int(cnt.item())


class SplitAct:
    """An activation stored as fp16 planes [B, planes, C/8, H, W, 8] (the input format of ia_conv2d_mfma_sx, see include/ia_hip.h):
    planes = 2 hi / lo pairs (fp32-equivalent consumers), planes = 1 one rounded fp16 plane (fp16-operand consumers: the
    fp16-storage form); already multiplied by the styles of the layer `consumer` (any object; None = unscaled)."""

    requires_grad = False      # (forward-only: lets the autograd eligibility checks treat it like a detached tensor)

    def __init__(self, data, channels, consumer=None):
        self.data, self.channels, self.consumer = data, channels, consumer
        b, self.planes, c8, h, w, _ = data.shape
        self.shape = (b, channels, h, w)
        self.device, self.dtype = data.device, torch.float32      # stands in for an fp32 activation
        if CHECK_SPLIT_RANGE and not torch.cuda.is_current_stream_capturing():
            n = split_saturation_count(self)
            if n:
                raise OverflowError(f'{n} activations of a {self.shape} split tensor were clamped at +-65504 (fp16 range of the hi plane)')

    def float(self):     # inverse of the split (tests / fallbacks): hi + lo * 2^-11, channel groups unfolded
        v = self.data[:, 0].float()
        if self.planes == 2:
            v = v + self.data[:, 1].float() * (1.0 / 2048.0)
        b, c8, h, w, _ = v.shape
        return v.permute(0, 1, 4, 2, 3).reshape(b, c8 * 8, h, w)


def act_split(x, styles=None, consumer=None, planes=2, shift=None):
    """fp32 NCHW (x styles [B,C] + shift [B,C]) -> SplitAct (see ia_act_split)."""
    _f32c(x, 'x')
    b, c, h, w = x.shape
    if c % 8:
        raise RuntimeError('the split format needs channels % 8 == 0')
    out = torch.empty(b, planes, c // 8, h, w, 8, device=x.device, dtype=torch.float16)
    with torch.cuda.device(x.device), _Timed('act_split', 0.0, (4.0 + 2.0 * planes) * x.numel()):
        st = _lib.load().ia_act_split(_p(x), _p(None if styles is None else _f32c(styles, 'styles')),
                                      _p(None if shift is None else _f32c(shift, 'shift')), _p(out), int(planes), b, c, h, w,
                                      _lib.stream_ptr(x.device))
    _lib.check(st, 'ia_act_split')
    return SplitAct(out, c, consumer)


def bn_train_split(x, weight, bias, running_mean, running_var, num_batches_tracked, eps, momentum, consumer=None, planes=2):
    """ia_bn_train_split: train-mode BatchNorm2d (batch statistics over B, H, W; running statistics moved in place when given) folded
    into the split staging of the convolution that follows it.  Returns the SplitAct of the normalised tensor."""
    _f32c(x, 'x')
    b, c, h, w = x.shape
    if c % 8:
        raise RuntimeError(f'the split format stores channels in groups of 8 (C = {c})')
    for name, t in (('weight', weight), ('bias', bias), ('running_mean', running_mean), ('running_var', running_var)):
        if t is not None and _f32c(t, name).numel() != c:
            raise RuntimeError(f'{name} has {t.numel()} elements, expected {c}')
    if num_batches_tracked is not None and not (num_batches_tracked.is_cuda and num_batches_tracked.dtype == torch.int64 and num_batches_tracked.numel() == 1):
        raise RuntimeError('num_batches_tracked must be a device int64 scalar')
    chunks = max(1, min(256, -(-(b * h * w) // 8192)))
    partials = torch.empty(c * chunks * 2, device=x.device, dtype=torch.float64)
    out = torch.empty(b, planes, c // 8, h, w, 8, device=x.device, dtype=torch.float16)
    with torch.cuda.device(x.device), _Timed('bn_train_split', 3.0 * x.numel(), 4.0 * x.numel() * 2 + 2.0 * out.numel(), f'B{b} C{c} {h}x{w}'):
        st = _lib.load().ia_bn_train_split(_p(x), _p(weight), _p(bias), _p(running_mean), _p(running_var), _p(num_batches_tracked), _p(partials), chunks,
                                           _p(out), int(planes), b, c, h, w, float(eps), float(momentum), _lib.stream_ptr(x.device))
    _lib.check(st, 'ia_bn_train_split')
    for t in (running_mean, running_var, num_batches_tracked):      # written through raw pointers: tell torch (the eval-mode affine caches of
        if t is not None:                                           # trunk_hip._UnitPack are keyed on the version counters)
            torch.autograd.graph.increment_version(t)
    return SplitAct(out, c, consumer)


def conv2d_mfma_sx(xs, wk, demod=None, noise=None, noise_strength=None, bias=None, residual=None, transposed=False, act='linear',
                   alpha=0.2, gain=1.0, clamp=None, want_f32=True, split_for=None, styles_next=None, ksplit=None, split_planes=2, prelu=None,
                   want_split=None):
    """ia_conv2d_mfma_sx: 3x3 convolution of a SplitAct (already multiplied by this layer's styles).  Returns the fp32 result,
    a SplitAct for `split_for` (multiplied by styles_next, `split_planes` planes), or the pair (y, ys) when both are asked for.
    A two-plane input takes weights from pack_conv_weight_split, a one-plane input those of pack_conv_weight_h."""
    if not isinstance(xs, SplitAct):
        raise RuntimeError('xs must be a SplitAct (hipops.act_split or a producing layer)')
    if xs.planes == 2 and not (wk.dtype == torch.float16 and wk.dim() == 5 and wk.shape[0] == 2 and hasattr(wk, 'wk_exp')):
        raise RuntimeError('wk must come from pack_conv_weight_split')
    if xs.planes == 1 and not (wk.dtype == torch.float16 and wk.dim() == 4):
        raise RuntimeError('a one-plane input takes the weights of pack_conv_weight_h')
    b, i, h, w = xs.shape
    o = wk.shape[-2]
    if wk.shape[-4] != 9 or wk.shape[-3] * 8 != i:
        raise RuntimeError(f'packed weight {tuple(wk.shape)} does not match 3x3, in-channels {i}')
    if want_split is None:
        want_split = split_for is not None or styles_next is not None
    if prelu is not None and (_f32c(prelu, 'prelu').numel() != o or act != 'lrelu'):
        raise RuntimeError('prelu: [O] per-channel slopes, with act="lrelu"')
    if transposed and (want_split or not want_f32):
        raise RuntimeError('the transposed form only writes the fp32 image')
    for name, t in (('demod', demod), ('noise', noise), ('bias', bias), ('residual', residual), ('styles_next', styles_next)):
        if t is not None:
            _f32c(t, name)
    lib = _lib.load()
    plan_s, plan_bytes = ctypes.c_int(0), ctypes.c_size_t(0)
    _lib.check(lib.ia_conv2d_plan(b, i, o, h, w, 3, int(transposed), 3, ctypes.byref(plan_s), ctypes.byref(plan_bytes)), 'ia_conv2d_plan')
    nbytes = plan_bytes.value
    if ksplit is None:
        ksplit = plan_s.value
    elif plan_s.value > 0 and ksplit != plan_s.value:
        nbytes = nbytes // plan_s.value * max(int(ksplit), 1)
    oh, ow = (2 * h + 1, 2 * w + 1) if transposed else (h, w)
    dev = xs.data.device
    y = torch.empty(b, o, oh, ow, device=dev, dtype=torch.float32) if want_f32 else None
    ys = torch.empty(b, split_planes, o // 8, oh, ow, 8, device=dev, dtype=torch.float16) if want_split else None
    scratch = _scratch_buffer(dev, nbytes) if nbytes else None
    flops = 2.0 * b * h * w * i * o * 9
    traffic = (2.0 * (xs.data.numel() + wk.numel()) + 4.0 * (y.numel() if want_f32 else 0) + 2.0 * (ys.numel() if want_split else 0)
               + 4.0 * (residual.numel() if residual is not None else 0))
    with torch.cuda.device(dev), _Timed('conv2d_mfma_t' if transposed else 'conv2d_mfma_k3', flops, traffic,
                                        f'B{b} I{i} O{o} {h}x{w} G{ksplit} ' + ('f16x3 dma' if xs.planes == 2 else 'f16 dma')):
        st = lib.ia_conv2d_mfma_sx(_p(xs.data), int(xs.planes), _p(wk), int(getattr(wk, 'wk_exp', 0)), _p(demod), _p(noise), _p(noise_strength),
                                   _p(bias), _p(residual), _p(y), _p(ys), int(split_planes), _p(styles_next), _p(scratch), nbytes, b, i, o, h, w, int(transposed), ACT_ID[act],
                                   float(alpha), _p(prelu), float(gain), float(-1 if clamp is None else clamp), int(ksplit), _lib.stream_ptr(dev))
    _lib.check(st, 'ia_conv2d_mfma_sx')
    out_s = SplitAct(ys, o, split_for) if want_split else None
    if want_f32 and want_split:
        return y, out_s
    return y if want_f32 else out_s


def upsample_bilinear_add(x, addend):
    """ia_upsample_bilinear_add: bilinear resize (align_corners=True) of x [B, C, H, W] to addend's size, plus addend."""
    _f32c(x, 'x')
    _f32c(addend, 'addend')
    b, c, h, w = x.shape
    if addend.shape[:2] != x.shape[:2]:
        raise RuntimeError(f'upsample_bilinear_add: {tuple(x.shape)} onto {tuple(addend.shape)}')
    y = torch.empty_like(addend)
    with torch.cuda.device(x.device):
        st = _lib.load().ia_upsample_bilinear_add(_p(x), _p(addend), _p(y), b * c, h, w, addend.shape[2], addend.shape[3], _lib.stream_ptr(x.device))
    _lib.check(st, 'ia_upsample_bilinear_add')
    return y


def dwconv3x3_tokens(x, w9c, bias, h, w, gelu=False):
    """ia_dwconv3x3_tokens: depth-wise 3x3 convolution of tokens [B, H*W, C] on their H x W grid (+ GELU); w9c [9, C]."""
    _f32c(x, 'x')
    _f32c(w9c, 'w9c')
    b, n, c = x.shape
    if n != h * w or tuple(w9c.shape) != (9, c) or c % 4:
        raise RuntimeError(f'dwconv3x3_tokens: tokens {tuple(x.shape)} on a {h} x {w} grid with weights {tuple(w9c.shape)} (C % 4 == 0)')
    y = torch.empty_like(x)
    with torch.cuda.device(x.device):
        st = _lib.load().ia_dwconv3x3_tokens(_p(x), _p(w9c), _p(None if bias is None else _f32c(bias, 'bias')), _p(y), b, h, w, c, 1 if gelu else 0,
                                             _lib.stream_ptr(x.device))
    _lib.check(st, 'ia_dwconv3x3_tokens')
    return y


def dwconv3x3_tokens_split(x, w9c, bias, h, w, gelu=False):
    """dwconv3x3_tokens with the result written as SplitTokens (the operand of the linear layer behind it; see ia_dwconv3x3_tokens_split)."""
    _f32c(x, 'x')
    _f32c(w9c, 'w9c')
    b, n, c = x.shape
    if n != h * w or tuple(w9c.shape) != (9, c) or c % 16:
        raise RuntimeError(f'dwconv3x3_tokens_split: tokens {tuple(x.shape)} on a {h} x {w} grid with weights {tuple(w9c.shape)} (C % 16 == 0)')
    out = torch.empty(2, c // 8, b * n, 8, device=x.device, dtype=torch.float16)
    with torch.cuda.device(x.device):
        st = _lib.load().ia_dwconv3x3_tokens_split(_p(x), _p(w9c), _p(None if bias is None else _f32c(bias, 'bias')), _p(out), b, h, w, c,
                                                   1 if gelu else 0, _lib.stream_ptr(x.device))
    _lib.check(st, 'ia_dwconv3x3_tokens_split')
    return SplitTokens(out, b * n, c, (b, n))


def conv_tiny_supported(i, o, h, w):
    """Shapes ia_conv3x3_s2_tiny covers (3x3, stride 2, padding 1 on 2^2 / 4^2 / 8^2 images)."""
    return bool(_lib.load().ia_conv3x3_s2_tiny_supported(int(i), int(o), int(h), int(w)))


def conv3x3_s2_tiny(x, w, bias=None, act='linear', alpha=0.2):
    """ia_conv3x3_s2_tiny: [B, I, H, W] (H = W in {2, 4, 8}) -> [B, O, H/2, W/2] with the module's own weight [O, I, 3, 3]."""
    _f32c(x, 'x')
    _f32c(w, 'w')
    b, i, h, wd = x.shape
    o = w.shape[0]
    if tuple(w.shape) != (o, i, 3, 3):
        raise RuntimeError(f'weight {tuple(w.shape)} does not match [O, {i}, 3, 3]')
    if bias is not None and _f32c(bias, 'bias').numel() != o:
        raise RuntimeError(f'bias has {bias.numel()} elements, expected {o}')
    y = torch.empty(b, o, h // 2, wd // 2, device=x.device, dtype=torch.float32)
    with torch.cuda.device(x.device), _Timed('conv3x3_tiny', 2.0 * b * (h // 2) * (wd // 2) * i * o * 9, 4.0 * (x.numel() + w.numel() + y.numel()),
                                             f'B{b} I{i} O{o} {h}x{wd} s2'):
        st = _lib.load().ia_conv3x3_s2_tiny(_p(x), _p(w), _p(bias), _p(y), b, i, o, h, wd, ACT_ID[act], float(alpha), _lib.stream_ptr(x.device))
    _lib.check(st, 'ia_conv3x3_s2_tiny')
    return y


def conv_down_supported(b, i, o, h, w):
    """Shapes ia_conv2d_down_sx covers (3x3, stride 2, padding 1 on an h x w input): asks the library's planner."""
    ks, nbytes = ctypes.c_int(0), ctypes.c_size_t(0)
    return _lib.load().ia_conv2d_down_plan(int(b), int(i), int(o), int(h), int(w), ctypes.byref(ks), ctypes.byref(nbytes)) == 0


def conv2d_down_sx(xs, wk, demod=None, bias=None, residual=None, act='linear', alpha=0.2, gain=1.0, clamp=None, want_f32=True, split_for=None,
                   styles_next=None, split_planes=2, prelu=None, want_split=None):
    """ia_conv2d_down_sx: 3x3 convolution with stride 2 and padding 1 of a SplitAct -> [B, O, (H-1)//2+1, (W-1)//2+1]; results as
    conv2d_mfma_sx returns them."""
    if not isinstance(xs, SplitAct):
        raise RuntimeError('xs must be a SplitAct (hipops.act_split or a producing layer)')
    if xs.planes == 2 and not (wk.dtype == torch.float16 and wk.dim() == 5 and wk.shape[0] == 2 and hasattr(wk, 'wk_exp')):
        raise RuntimeError('wk must come from pack_conv_weight_split')
    if xs.planes == 1 and not (wk.dtype == torch.float16 and wk.dim() == 4):
        raise RuntimeError('a one-plane input takes the weights of pack_conv_weight_h')
    b, i, h, w = xs.shape
    o = wk.shape[-2]
    if wk.shape[-4] != 9 or wk.shape[-3] * 8 != i:
        raise RuntimeError(f'packed weight {tuple(wk.shape)} does not match 3x3, in-channels {i}')
    if want_split is None:
        want_split = split_for is not None or styles_next is not None
    if prelu is not None and (_f32c(prelu, 'prelu').numel() != o or act != 'lrelu'):
        raise RuntimeError('prelu: [O] per-channel slopes, with act="lrelu"')
    for name, t in (('demod', demod), ('bias', bias), ('residual', residual), ('styles_next', styles_next)):
        if t is not None:
            _f32c(t, name)
    lib = _lib.load()
    plan_s, plan_bytes = ctypes.c_int(0), ctypes.c_size_t(0)
    _lib.check(lib.ia_conv2d_down_plan(b, i, o, h, w, ctypes.byref(plan_s), ctypes.byref(plan_bytes)), 'ia_conv2d_down_plan')
    nbytes, ksplit = plan_bytes.value, plan_s.value
    oh, ow = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    dev = xs.data.device
    y = torch.empty(b, o, oh, ow, device=dev, dtype=torch.float32) if want_f32 else None
    ys = torch.empty(b, split_planes, o // 8, oh, ow, 8, device=dev, dtype=torch.float16) if want_split else None
    scratch = _scratch_buffer(dev, nbytes) if nbytes else None
    flops = 2.0 * b * oh * ow * i * o * 9
    traffic = (2.0 * (xs.data.numel() + wk.numel()) + 4.0 * (y.numel() if want_f32 else 0) + 2.0 * (ys.numel() if want_split else 0)
               + 4.0 * (residual.numel() if residual is not None else 0))
    with torch.cuda.device(dev), _Timed('conv2d_mfma_k3', flops, traffic, f'B{b} I{i} O{o} {h}x{w} s2 G{ksplit} ' + ('f16x3 dma' if xs.planes == 2 else 'f16 dma')):
        st = lib.ia_conv2d_down_sx(_p(xs.data), int(xs.planes), _p(wk), int(getattr(wk, 'wk_exp', 0)), _p(demod), _p(bias), _p(residual), _p(y), _p(ys),
                                   int(split_planes), _p(styles_next), _p(scratch), nbytes, b, i, o, h, w, ACT_ID[act], float(alpha), _p(prelu),
                                   float(gain), float(-1 if clamp is None else clamp), int(ksplit), _lib.stream_ptr(dev))
    _lib.check(st, 'ia_conv2d_down_sx')
    out_s = SplitAct(ys, o, split_for) if want_split else None
    if want_f32 and want_split:
        return y, out_s
    return y if want_f32 else out_s


def upconv_rows_supported(b, i, o, h, w):
    """Shapes ia_upconv2d_rows_sx covers (the row-phase form of the transposed 3x3 convolution): asks the library."""
    nbytes = ctypes.c_size_t(0)
    return _lib.load().ia_upconv2d_rows_plan(int(b), int(i), int(o), int(h), int(w), ctypes.byref(nbytes)) == 0


def upconv2d_rows_sx(xs, wk, demod=None):
    """ia_upconv2d_rows_sx: stride-2 transposed 3x3 convolution of a two-plane SplitAct -> the demodulated [B, O, 2H+1, 2W+1] fp32 image
    (what conv2d_mfma_sx(transposed=True) returns), evaluated per output row phase on the stride-1 tile."""
    if not (isinstance(xs, SplitAct) and xs.planes == 2):
        raise RuntimeError('xs must be a two-plane SplitAct')
    if not (wk.dtype == torch.float16 and wk.dim() == 5 and wk.shape[0] == 2 and hasattr(wk, 'wk_exp')):
        raise RuntimeError('wk must come from pack_conv_weight_split')
    b, i, h, w = xs.shape
    o = wk.shape[-2]
    if wk.shape[-4] != 9 or wk.shape[-3] * 8 != i:
        raise RuntimeError(f'packed weight {tuple(wk.shape)} does not match 3x3, in-channels {i}')
    if demod is not None:
        _f32c(demod, 'demod')
    lib = _lib.load()
    plan_bytes = ctypes.c_size_t(0)
    _lib.check(lib.ia_upconv2d_rows_plan(b, i, o, h, w, ctypes.byref(plan_bytes)), 'ia_upconv2d_rows_plan')
    dev = xs.data.device
    y = torch.empty(b, o, 2 * h + 1, 2 * w + 1, device=dev, dtype=torch.float32)
    scratch = _scratch_buffer(dev, plan_bytes.value)
    flops = 2.0 * b * h * w * i * o * 9
    traffic = 2.0 * (xs.data.numel() + wk.numel()) + 4.0 * y.numel()
    with torch.cuda.device(dev), _Timed('conv2d_mfma_t', flops, traffic, f'B{b} I{i} O{o} {h}x{w} rows f16x3 dma'):
        st = lib.ia_upconv2d_rows_sx(_p(xs.data), _p(wk), int(wk.wk_exp), _p(demod), _p(y), _p(scratch), plan_bytes.value, b, i, o, h, w,
                                     _lib.stream_ptr(dev))
    _lib.check(st, 'ia_upconv2d_rows_sx')
    return y


def conv_sx_rgb_supported(b, i, o, h, w):
    """Layers ia_conv2d_mfma_sx_rgb covers: stride-1 layers that run in whole rounds of tiles holding every output channel."""
    if o > 128 or i % 8 or o % 8:
        return False
    plan_s, plan_bytes = ctypes.c_int(0), ctypes.c_size_t(0)
    st = _lib.load().ia_conv2d_plan(b, i, o, h, w, 3, 0, 3, ctypes.byref(plan_s), ctypes.byref(plan_bytes))
    # (whole rounds of the 128-channel x 256-point tile: a layer with fewer of those than CUs runs on the 32-channel tile family or stream-K)
    return st == 0 and plan_s.value == 0 and h * w >= 8192 and b * ((h * w + 255) // 256) >= 256


def conv2d_mfma_sx_rgb(xs, wk, rgb_wk, rgb_styles=None, rgb_bias=None, rgb_residual=None, rgb_clamp=None, demod=None, noise=None,
                       noise_strength=None, bias=None, act='linear', alpha=0.2, gain=1.0, clamp=None, want_f32=False, split_for=None,
                       styles_next=None, split_planes=2):
    """ia_conv2d_mfma_sx_rgb: the stride-1 3x3 convolution of a SplitAct AND the ToRGB layer that reads its result, in one launch.
    rgb_wk = pack_conv_weight of the 1x1 ToRGB weight ([1, O, RC] or [O, RC]).  Returns (y or None, SplitAct or None, rgb)."""
    if not isinstance(xs, SplitAct):
        raise RuntimeError('xs must be a SplitAct (hipops.act_split or a producing layer)')
    b, i, h, w = xs.shape
    o = wk.shape[-2]
    if wk.shape[-4] != 9 or wk.shape[-3] * 8 != i:
        raise RuntimeError(f'packed weight {tuple(wk.shape)} does not match 3x3, in-channels {i}')
    _f32c(rgb_wk, 'rgb_wk')
    rc = rgb_wk.shape[-1]
    if rgb_wk.numel() != o * rc:
        raise RuntimeError(f'rgb_wk has {rgb_wk.numel()} elements, expected {o} x {rc}')
    for name, t, n in (('demod', demod, b * o), ('noise', noise, h * w), ('bias', bias, o), ('styles_next', styles_next, b * o),
                       ('rgb_styles', rgb_styles, b * o), ('rgb_bias', rgb_bias, rc), ('rgb_residual', rgb_residual, b * rc * h * w)):
        if t is not None and _f32c(t, name).numel() != n:
            raise RuntimeError(f'{name} has {t.numel()} elements, expected {n}')
    want_split = split_for is not None or styles_next is not None
    dev = xs.data.device
    y = torch.empty(b, o, h, w, device=dev, dtype=torch.float32) if want_f32 else None
    ys = torch.empty(b, split_planes, o // 8, h, w, 8, device=dev, dtype=torch.float16) if want_split else None
    rgb = torch.empty(b, rc, h, w, device=dev, dtype=torch.float32)
    flops = 2.0 * b * h * w * i * o * 9
    traffic = (2.0 * (xs.data.numel() + wk.numel()) + 4.0 * (y.numel() if want_f32 else 0) + 2.0 * (ys.numel() if want_split else 0)
               + 4.0 * rgb.numel() * (2 if rgb_residual is not None else 1))
    with torch.cuda.device(dev), _Timed('conv2d_mfma_k3', flops, traffic, f'B{b} I{i} O{o} {h}x{w} G0 ' + ('f16x3 dma' if xs.planes == 2 else 'f16 dma') + ' +rgb'):
        st = _lib.load().ia_conv2d_mfma_sx_rgb(_p(xs.data), int(xs.planes), _p(wk), int(getattr(wk, 'wk_exp', 0)), _p(demod), _p(noise),
                                               _p(noise_strength), _p(bias), _p(y), _p(ys), int(split_planes), _p(styles_next), _p(rgb_wk),
                                               _p(rgb_styles), _p(rgb_bias), _p(rgb_residual), _p(rgb), int(rc),
                                               float(-1 if rgb_clamp is None else rgb_clamp), b, i, o, h, w, ACT_ID[act], float(alpha), float(gain),
                                               float(-1 if clamp is None else clamp), _lib.stream_ptr(dev))
    _lib.check(st, 'ia_conv2d_mfma_sx_rgb')
    return y, (SplitAct(ys, o, split_for) if want_split else None), rgb


def upfirdn2d_bias_act(x, f, noise=None, noise_strength=None, bias=None, up=1, pad0=(1, 1), out_hw=None, fir_gain=1.0,
                       act='linear', alpha=0.2, act_gain=1.0, clamp=None, flip=False):
    """FIR + noise + bias + activation in one pass (see ia_upfirdn2d_bias_act)."""
    if not (x.is_cuda and x.is_contiguous() and x.dtype in (torch.float32, torch.float16)):
        raise RuntimeError('x must be a contiguous f32/f16 device tensor')
    n, c, ih, iw = x.shape
    fh, fw = f.shape
    y = torch.empty(n, c, out_hw[0], out_hw[1], device=x.device, dtype=x.dtype)
    with torch.cuda.device(x.device), _Timed('upfirdn2d_bias_act', 2.0 * y.numel() * (fh * fw) / (up * up),
                                             x.element_size() * (x.numel() + y.numel())):
        st = _lib.load().ia_upfirdn2d_bias_act(_p(x), _p(_f32c(f, 'f')), _p(noise), _p(noise_strength), _p(bias), _p(y),
                                               _lib.DTYPE_ID[x.dtype], n, c, ih, iw, fh, fw, out_hw[0], out_hw[1], int(up),
                                               int(pad0[0]), int(pad0[1]), 1 if flip else 0, float(fir_gain), ACT_ID[act],
                                               float(alpha), float(act_gain), float(-1 if clamp is None else clamp),
                                               _lib.stream_ptr(x.device))
    _lib.check(st, 'ia_upfirdn2d_bias_act')
    return y


def fir_tail_split(x, f, noise=None, noise_strength=None, bias=None, styles_next=None, out_hw=None, pad0=(1, 1), fir_gain=1.0, act='linear',
                   alpha=0.2, act_gain=1.0, clamp=None, flip=False, want_f32=False, split_for=None, planes=2):
    """upfirdn2d_bias_act (4x4 filter, up 1) whose result goes out in split format for `split_for` (see ia_fir_tail_split).
    Returns the SplitAct, or (y, SplitAct) with want_f32."""
    _f32c(x, 'x')
    n, c, ih, iw = x.shape
    if tuple(f.shape) != (4, 4) or c % 8:
        raise RuntimeError('fir_tail_split needs the 4x4 filter and channels % 8 == 0')
    oh, ow = out_hw
    ys = torch.empty(n, planes, c // 8, oh, ow, 8, device=x.device, dtype=torch.float16)
    y = torch.empty(n, c, oh, ow, device=x.device, dtype=torch.float32) if want_f32 else None
    with torch.cuda.device(x.device), _Timed('upfirdn2d_bias_act', 2.0 * n * c * oh * ow * 16, 4.0 * (x.numel() + n * c * oh * ow * (2 if want_f32 else 1)),
                                             'split'):
        st = _lib.load().ia_fir_tail_split(_p(x), _p(_f32c(f, 'f')), _p(noise), _p(noise_strength), _p(bias), _p(styles_next), _p(y), _p(ys),
                                           int(planes), n, c, ih, iw, oh, ow, int(pad0[0]), int(pad0[1]), 1 if flip else 0, float(fir_gain), ACT_ID[act],
                                           float(alpha), float(act_gain), float(-1 if clamp is None else clamp), _lib.stream_ptr(x.device))
    _lib.check(st, 'ia_fir_tail_split')
    out = SplitAct(ys, c, split_for)
    return (y, out) if want_f32 else out


def compose_upfir_weight(w, f, gain=4.0):
    """[O, I, 3, 3] weight of an up-sampling layer + its [4, 4] resample filter -> [4*O, I, 3, 3]: per output phase (py, px) the 3x3
    kernel on the INPUT image that equals conv_transpose2d(stride 2) followed by upfirdn2d(f, padding [1,1,1,1], gain)
    (see ia_upconv2d_fir_sx).  Row ((py * O/32 + o // 32) * 2 + px) * 32 + o % 32."""
    w = w.detach().double()
    f = torch.as_tensor(f).double().to(w.device)
    if tuple(f.shape) != (4, 4) or tuple(w.shape[2:]) != (3, 3):
        raise RuntimeError('compose_upfir_weight: 3x3 weight and 4x4 filter')
    F = f.flip([0, 1])                                   # upfirdn2d applies the flipped filter (a true convolution)
    o, i = w.shape[:2]
    out = torch.zeros(4, o, i, 3, 3, dtype=torch.float64, device=w.device)
    for py in range(2):
        for px in range(2):
            for a in range(4):
                for ky in range(3):
                    ny = py + a - 1 - ky
                    if ny % 2:
                        continue
                    for b_ in range(4):
                        for kx in range(3):
                            nx = px + b_ - 1 - kx
                            if nx % 2:
                                continue
                            out[2 * py + px, :, :, ny // 2 + 1, nx // 2 + 1] += gain * F[a, b_] * w[:, :, ky, kx]
    if o % 32:
        raise RuntimeError('compose_upfir_weight: out_channels % 32 == 0')
    # row order (py, block of 32 channels, px, channel in block): the two horizontal phases of a block are neighbours (see the kernel's store)
    out = out.view(2, 2, o // 32, 32, i, 3, 3).permute(0, 2, 1, 3, 4, 5, 6)
    return out.reshape(4 * o, i, 3, 3).float()


def upconv_fir_supported(b, i, o, h, w):
    """Layers ia_upconv2d_fir_sx covers: the composed 4*O-channel stride-1 layer runs in whole tiles that divide O."""
    if i % 8 or o % 128:
        return False
    plan_s, plan_bytes = ctypes.c_int(0), ctypes.c_size_t(0)
    st = _lib.load().ia_conv2d_plan(b, i, 4 * o, h, w, 3, 0, 3, ctypes.byref(plan_s), ctypes.byref(plan_bytes))
    # whole rounds of the 128-channel x 256-point tile (a layer with fewer of those than CUs runs on the 32-channel tiles or stream-K)
    return st == 0 and plan_s.value == 0 and h * w >= 1024 and w <= 512 and b * ((h * w + 255) // 256) * (4 * o // 128) >= 256


def upconv_fir_sx(xs, wk, demod=None, noise=None, noise_strength=None, bias=None, styles_next=None, act='linear', alpha=0.2, gain=1.0,
                  clamp=None, want_f32=False, split_for=None, split_planes=2):
    """ia_upconv2d_fir_sx: an up-sampling layer (transposed convolution + resample FIR + noise + bias + activation) of a SplitAct as one
    stride-1 launch on the COMPOSED weight (pack of compose_upfir_weight).  Returns the SplitAct of the [B, O, 2H, 2W] result for
    `split_for` (multiplied by styles_next), or (y, SplitAct) with want_f32."""
    if not isinstance(xs, SplitAct):
        raise RuntimeError('xs must be a SplitAct')
    b, i, h, w = xs.shape
    o4 = wk.shape[-2]
    if o4 % 4 or wk.shape[-4] != 9 or wk.shape[-3] * 8 != i:
        raise RuntimeError(f'packed composed weight {tuple(wk.shape)} does not match 3x3, in-channels {i}, 4 x O rows')
    o = o4 // 4
    for name, t, n in (('demod', demod, b * o), ('noise', noise, 4 * h * w), ('bias', bias, o), ('styles_next', styles_next, b * o)):
        if t is not None and _f32c(t, name).numel() != n:
            raise RuntimeError(f'{name} has {t.numel()} elements, expected {n}')
    dev = xs.data.device
    y = torch.empty(b, o, 2 * h, 2 * w, device=dev, dtype=torch.float32) if want_f32 else None
    ys = torch.empty(b, split_planes, o // 8, 2 * h, 2 * w, 8, device=dev, dtype=torch.float16)
    flops = 2.0 * b * h * w * i * o * 9          # (algorithmic: the transposed convolution's; 4x of it is executed)
    traffic = 2.0 * (xs.data.numel() + wk.numel()) + 2.0 * ys.numel() + (4.0 * y.numel() if want_f32 else 0.0)
    with torch.cuda.device(dev), _Timed('conv2d_mfma_t', flops, traffic, f'B{b} I{i} O{o} {h}x{w} ' + ('f16x3 dma' if xs.planes == 2 else 'f16 dma') + ' composed up-FIR'):
        st = _lib.load().ia_upconv2d_fir_sx(_p(xs.data), int(xs.planes), _p(wk), int(getattr(wk, 'wk_exp', 0)), _p(demod), _p(noise),
                                            _p(noise_strength), _p(bias), _p(y), _p(ys), int(split_planes), _p(styles_next), b, i, o, h, w,
                                            ACT_ID[act], float(alpha), float(gain), float(-1 if clamp is None else clamp), _lib.stream_ptr(dev))
    _lib.check(st, 'ia_upconv2d_fir_sx')
    out = SplitAct(ys, o, split_for)
    return (y, out) if want_f32 else out


def planes_channels_last(planes):
    """[B, 3, C, H, W] -> [B, 3, H, W, C] contiguous: the layout ia_render_rays gathers from."""
    return planes.permute(0, 1, 3, 4, 2).contiguous()


# ia_render_rays stages the decoder weights as fp16 hi / lo pairs at 2^12 (csrc/render_rays.hip): a staged weight -- layer 1 times its
# gain and log2 e, the colour rows of layer 2 times their gain -- of 65520 / 4096 = 15.996 or more has an infinite high part and the
# launch returns NaN.  The bound below leaves room for the kernel's fp32 rounding of the product.
RENDER_WEIGHT_BOUND = 15.99
_render_weight_checks = {}      # (data_ptr, _version) of w0 and w1 -> (their storages, weakly; max |w0|; max |w1 colour rows|)


def _render_weight_maxima(w0, w1):
    """(max |w0|, max |w1[1:]|) as python floats: one device -> host read."""
    return tuple(torch.stack([w0.abs().max(), w1[1:].abs().max()]).tolist())


def _render_weights_checked(w0, w1, lr_multiplier):
    """Raises if a staged decoder weight leaves the range of the kernel's fp16 pairs.  The maxima are read from the device once per
    version of the two tensors (an in-place update bumps `_version`, a new tensor has another pointer; the entry also holds weak
    references to the two storages, so a new tensor at the address of a freed one is not taken for it); while a stream is capturing
    nothing is read, and nothing is checked unless the version is already known."""
    key = (w0.data_ptr(), w0._version, w1.data_ptr(), w1._version)
    s0, s1 = w0.untyped_storage(), w1.untyped_storage()
    entry = _render_weight_checks.get(key)
    if entry is None or entry[0]() is not s0 or entry[1]() is not s1:
        if torch.cuda.is_current_stream_capturing():
            return
        if len(_render_weight_checks) >= 64:
            _render_weight_checks.clear()
        entry = _render_weight_checks[key] = (weakref.ref(s0), weakref.ref(s1)) + _render_weight_maxima(w0, w1)
    maxima = entry[2:]
    lr = abs(float(lr_multiplier))
    staged = (maxima[0] * lr / math.sqrt(32.0) * math.log2(math.e), maxima[1] * lr / math.sqrt(64.0))
    for name, value, what in (('w0', staged[0], '|w0| * lr_multiplier / sqrt(32) * log2(e)'), ('w1', staged[1], '|w1[1:]| * lr_multiplier / sqrt(64)')):
        if not value < RENDER_WEIGHT_BOUND:
            raise RuntimeError(f'render_rays: {name} is outside the decoder\'s fp16 pair range: max {what} = {value:.4g}, '
                               f'must stay below {RENDER_WEIGHT_BOUND} (the high parts at 2^12 overflow at 16)')


def render_rays(planes_cl, rays_o, rays_d, jitter, dist, w0, b0, w1, b1, lr_multiplier=1.0, box_warp=1.0, white_back=False,
                n_coarse=48, n_importance=48, debug=False, channel_major=False, u_importance=None, split_styles=None, split_planes=0):
    """Fused importance renderer (see ia_render_rays).  Returns (rgb [B,R,32], depth [B,R,1], wsum [B,R,1][, aux]).
    channel_major=True stores rgb as [B,32,R] (the feature image the super-resolution head reads) and returns the [B,R,32] VIEW of
    it: same values and shape, and `rgb.permute(0, 2, 1).reshape(B, 32, nrr, nrr)` is then contiguous without a copy."""
    for name, t in (('planes', planes_cl), ('rays_o', rays_o), ('rays_d', rays_d), ('jitter', jitter), ('dist', dist),
                    ('w0', w0), ('b0', b0), ('w1', w1), ('b1', b1)):
        _f32c(t, name)
    b, three, ph, pw, c = planes_cl.shape
    if three != 3 or c != 32:
        raise RuntimeError(f'planes must be [B,3,H,W,32] channels-last, got {tuple(planes_cl.shape)}')
    r = rays_o.shape[1]
    if dist.numel() not in (1, b):
        raise RuntimeError(f'dist must have 1 or B = {b} elements, got {dist.numel()}')
    dist_per_frame = dist.numel() == b and b > 1
    if tuple(jitter.shape[:3]) != (b, r, n_coarse):
        raise RuntimeError(f'jitter must be [B,R,{n_coarse}(,1)], got {tuple(jitter.shape)}')
    if u_importance is not None and (_f32c(u_importance, 'u_importance').numel() != b * r * n_importance):
        raise RuntimeError(f'u_importance must hold B * R * {n_importance} sorted uniform draws')
    _render_weights_checked(w0, w1, lr_multiplier)
    dev = planes_cl.device
    lib = _lib.load()
    rgb = torch.empty(b, 32, r, device=dev).permute(0, 2, 1) if channel_major else torch.empty(b, r, 32, device=dev)
    depth = torch.empty(b, r, 1, device=dev)
    wsum = torch.empty(b, r, 1, device=dev)
    scratch = torch.empty(2 * lib.ia_render_rays_grid(b, r) * (8 * b if dist_per_frame else 1), device=dev)      # (8 waves per workgroup: include/ia_hip.h)
    # split_planes = 1 | 2: the composited features ALSO in the split format (x split_styles [B,32]) as `rgb.split_data` [B, planes, 4, R, 8]
    split = torch.empty(b, split_planes, 4, r, 8, device=dev, dtype=torch.float16) if split_planes else None
    if split_styles is not None and (_f32c(split_styles, 'split_styles').numel() != b * 32 or not split_planes):
        raise RuntimeError('split_styles: [B,32] styles of the layer that consumes the split copy (with split_planes = 1 or 2)')
    aux = {}
    if debug:
        aux = dict(z_fine=torch.empty(b, r, 48, device=dev), inds=torch.empty(b, r, 48, device=dev, dtype=torch.int32),
                   order=torch.empty(b, r, 96, device=dev, dtype=torch.int32), w_coarse=torch.empty(b, r, 47, device=dev),
                   sigma_coarse=torch.empty(b, r, 48, device=dev))
    # algorithmic work: 2 passes x 48 samples x (32*64 + 64*33) MACs per ray; planes + rays in, 34 floats out
    flops = b * r * 96 * 2.0 * (32 * 64 + 64 * 33)
    traffic = 4.0 * (planes_cl.numel() + 2 * rays_o.numel() + jitter.numel() + b * r * 34)
    with torch.cuda.device(dev), _Timed('render_rays', flops, traffic):
        st = lib.ia_render_rays(_p(planes_cl), _p(rays_o), _p(rays_d), _p(jitter), _p(u_importance), _p(dist), _p(w0), _p(b0), _p(w1), _p(b1),
                                float(lr_multiplier), float(box_warp), int(bool(white_back)) | (2 if channel_major else 0) | (4 if dist_per_frame else 0), b, r, ph, pw,
                                int(n_coarse),
                                int(n_importance), _p(rgb), _p(depth), _p(wsum), _p(scratch), _p(aux.get('z_fine')),
                                _p(aux.get('inds')), _p(aux.get('order')), _p(aux.get('w_coarse')), _p(aux.get('sigma_coarse')),
                                _p(split), _p(split_styles), int(split_planes or 2), _lib.stream_ptr(dev))
    _lib.check(st, 'ia_render_rays')
    if split is not None:
        rgb.split_data = split
    return (rgb, depth, wsum, aux) if debug else (rgb, depth, wsum)


def ray_limits_box(rays_o, rays_d, box_side_length, repair_misses=False):
    """math_utils.get_ray_limits_box on the device (see ia_ray_limits_box) -> limits [..., 2] = (t_near, t_far); repair_misses: with
    ImportanceRenderer.forward's repair of the rays that miss the box (renderer.py:133-136), no host round trip."""
    _f32c(rays_o, 'rays_o'); _f32c(rays_d, 'rays_d')
    n = rays_o.numel() // 3
    lib = _lib.load()
    limits = torch.empty(*rays_o.shape[:-1], 2, device=rays_o.device)
    part = torch.empty(2 * lib.ia_ray_limits_box_parts(n), device=rays_o.device)
    with torch.cuda.device(rays_o.device):
        st = lib.ia_ray_limits_box(_p(rays_o), _p(rays_d), float(box_side_length), n, int(bool(repair_misses)), _p(limits), _p(part),
                                   _lib.stream_ptr(rays_o.device))
    _lib.check(st, 'ia_ray_limits_box')
    return limits


def render_rays_box(planes_cl, rays_o, rays_d, jitter, u_importance, w0, b0, w1, b1, ray_limits=None, ray_start=0.0, ray_end=0.0,
                    flip_z=False, lr_multiplier=1.0, box_warp=1.0, white_back=False, n_coarse=48, n_importance=48, debug=False):
    """ImportanceRenderer.forward as one launch (see ia_render_rays_box): `ray_limits` [B,R,2] (the 'auto' box limits) or the fixed
    [ray_start, ray_end]; `u_importance` [B*R, 48] sorted draws.  Returns (rgb [B,R,32], depth [B,R,1], wsum [B,R,1][, aux])."""
    for name, t in (('planes', planes_cl), ('rays_o', rays_o), ('rays_d', rays_d), ('jitter', jitter), ('u_importance', u_importance),
                    ('w0', w0), ('b0', b0), ('w1', w1), ('b1', b1)):
        _f32c(t, name)
    b, three, ph, pw, c = planes_cl.shape
    if three != 3 or c != 32:
        raise RuntimeError(f'planes must be [B,3,H,W,32] channels-last, got {tuple(planes_cl.shape)}')
    r = rays_o.shape[1]
    if tuple(jitter.shape[:3]) != (b, r, n_coarse):
        raise RuntimeError(f'jitter must be [B,R,{n_coarse}(,1)], got {tuple(jitter.shape)}')
    if u_importance.numel() != b * r * n_importance:
        raise RuntimeError(f'u_importance must hold B * R * {n_importance} sorted uniform draws')
    if ray_limits is not None and _f32c(ray_limits, 'ray_limits').numel() != b * r * 2:
        raise RuntimeError('ray_limits must be [B,R,2]')
    _render_weights_checked(w0, w1, lr_multiplier)
    dev = planes_cl.device
    lib = _lib.load()
    rgb, depth, wsum = torch.empty(b, r, 32, device=dev), torch.empty(b, r, 1, device=dev), torch.empty(b, r, 1, device=dev)
    scratch = torch.empty(2 * lib.ia_render_rays_grid(b, r), device=dev)
    aux = {}
    if debug:
        aux = dict(z_fine=torch.empty(b, r, 48, device=dev), inds=torch.empty(b, r, 48, device=dev, dtype=torch.int32),
                   order=torch.empty(b, r, 96, device=dev, dtype=torch.int32), w_coarse=torch.empty(b, r, 47, device=dev),
                   sigma_coarse=torch.empty(b, r, 48, device=dev))
    flops = b * r * 96 * 2.0 * (32 * 64 + 64 * 33)
    traffic = 4.0 * (planes_cl.numel() + 2 * rays_o.numel() + jitter.numel() + u_importance.numel() + b * r * 36)
    with torch.cuda.device(dev), _Timed('render_rays', flops, traffic, 'box'):
        st = lib.ia_render_rays_box(_p(planes_cl), _p(rays_o), _p(rays_d), _p(jitter), _p(u_importance), _p(ray_limits), float(ray_start), float(ray_end),
                                    _p(w0), _p(b0), _p(w1), _p(b1), float(lr_multiplier), float(box_warp),
                                    int(bool(white_back)) | (8 if flip_z else 0), b, r, ph, pw, int(n_coarse), int(n_importance),
                                    _p(rgb), _p(depth), _p(wsum), _p(scratch), _p(aux.get('z_fine')), _p(aux.get('inds')), _p(aux.get('order')),
                                    _p(aux.get('w_coarse')), _p(aux.get('sigma_coarse')), _lib.stream_ptr(dev))
    _lib.check(st, 'ia_render_rays_box')
    return (rgb, depth, wsum, aux) if debug else (rgb, depth, wsum)


def importance_stage(z_coarse, w_coarse):
    """Importance resampling + merge order from given coarse depths/weights (parity-test entry)."""
    n = z_coarse.shape[0]
    dev = z_coarse.device
    z_fine = torch.empty(n, 48, device=dev)
    inds = torch.empty(n, 48, device=dev, dtype=torch.int32)
    order = torch.empty(n, 96, device=dev, dtype=torch.int32)
    st = _lib.load().ia_importance_stage(_p(_f32c(z_coarse, 'z_coarse')), _p(_f32c(w_coarse, 'w_coarse')), _p(z_fine), _p(inds),
                                         _p(order), n, _lib.stream_ptr(dev))
    _lib.check(st, 'ia_importance_stage')
    return z_fine, inds, order


def fill_mouth(alpha):
    """alpha [B,1,H,W] -> mouth mask [B,1,H,W] (see ia_fill_mouth)."""
    _f32c(alpha, 'alpha')
    b, one, h, w = alpha.shape
    mouth = torch.empty_like(alpha)
    with torch.cuda.device(alpha.device):
        st = _lib.load().ia_fill_mouth(_p(alpha), _p(mouth), b * one, h, w, _lib.stream_ptr(alpha.device))
    _lib.check(st, 'ia_fill_mouth')
    return mouth


def mouth_edge_blur(alpha, mouth):
    """alpha, mouth (= fill_mouth(alpha)) [B,1,H,W] -> the eroded + blurred mouth mask [B,1,H,W] (see ia_mouth_edge_blur)."""
    _f32c(alpha, 'alpha'); _f32c(mouth, 'mouth')
    b, one, h, w = alpha.shape
    out = torch.empty_like(alpha)
    with torch.cuda.device(alpha.device):
        st = _lib.load().ia_mouth_edge_blur(_p(alpha), _p(mouth), _p(out), b * one, h, w, _lib.stream_ptr(alpha.device))
    _lib.check(st, 'ia_mouth_edge_blur')
    return out


def rasterize_level(tex, uvcoords_image, upper_alpha, sta, bbox, res, tex_cl=None):
    """One level of TriPlaneGenerator.rasterize (see ia_rasterize_level).  tex [B,C,Rt,Rt]; sta NCHW (may be a channel
    slice of a wider tensor as long as channels/rows are dense); returns [B, C+1, res, res].  `tex_cl` is the level
    already in channels-last order (channels_last_copy), if the caller made it ahead of time."""
    b, c, rt, _ = tex.shape
    if tex_cl is None:
        tex_cl = channels_last_copy(tex)
    rs = sta.shape[-1]
    if not (sta.stride(3) == 1 and sta.stride(2) == rs and sta.stride(1) == rs * rs and sta.shape[1] >= c):
        sta = sta.contiguous()
    out = torch.empty(b, c + 1, res, res, device=tex.device, dtype=torch.float32)
    y0, y1, x0, x1 = bbox
    with torch.cuda.device(tex.device):
        st = _lib.load().ia_rasterize_level(_p(_f32c(tex_cl, 'tex')), _p(_f32c(uvcoords_image, 'uvcoords_image')),
                                            _p(_f32c(upper_alpha, 'upper_alpha')), sta.data_ptr(), sta.stride(0), _p(out),
                                            b, c, rt, rs, res, y0, y1, x0, x1, _lib.stream_ptr(tex.device))
    _lib.check(st, 'ia_rasterize_level')
    return out


def cond_blend(cond, x):
    """cond[:, :-1] * a + x * (1 - a) with a = cond[:, -1:] in one pass (see ia_cond_blend)."""
    b, c, h, w = x.shape
    y = torch.empty_like(x)
    with torch.cuda.device(x.device):
        st = _lib.load().ia_cond_blend(_p(_f32c(cond, 'cond')), _p(_f32c(x, 'x')), _p(y), b, c, h, w, _lib.stream_ptr(x.device))
    _lib.check(st, 'ia_cond_blend')
    return y


def cond_blend_split(cond, x, styles_next, consumer):
    """cond_blend whose result exists only as the SplitAct `consumer` reads (see ia_cond_blend_split)."""
    b, c, h, w = x.shape
    ys = torch.empty(b, 2, c // 8, h, w, 8, device=x.device, dtype=torch.float16)
    with torch.cuda.device(x.device):
        st = _lib.load().ia_cond_blend_split(_p(_f32c(cond, 'cond')), _p(_f32c(x, 'x')), _p(None if styles_next is None else _f32c(styles_next, 'styles')),
                                             _p(ys), b, c, h, w, _lib.stream_ptr(x.device))
    _lib.check(st, 'ia_cond_blend_split')
    return SplitAct(ys, c, consumer)


def channels_last_copy(t):
    """[B,C,H,W] -> contiguous [B,H,W,C] (the layout ia_rasterize_level gathers from): ia_channels_last for contiguous fp32 device
    tensors (a tiled transpose: 25 -> ~8 us for 256 channels @128^2 against the strided Tensor.copy_), torch otherwise."""
    if t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and t.dim() == 4:
        b, c, h, w = t.shape
        out = torch.empty(b, h, w, c, device=t.device, dtype=torch.float32)
        with torch.cuda.device(t.device):
            st = _lib.load().ia_channels_last(_p(t), _p(out), b, c, h, w, _lib.stream_ptr(t.device))
        _lib.check(st, 'ia_channels_last')
        return out
    return t.permute(0, 2, 3, 1).contiguous()


def blend_planes(stitch, full_alpha, static_planes, bbox):
    """Channels-last blended tri-planes [B,3,256,256,32] (see ia_blend_planes).  static_planes [B,96,256,256]: dense per batch
    element, any batch stride (0 for planes expanded over the batch; the kernel takes the stride)."""
    b = stitch.shape[0]
    if not (static_planes.is_cuda and static_planes.dtype == torch.float32 and tuple(static_planes.stride()[1:]) == (65536, 256, 1)):
        static_planes = _f32c(static_planes, 'static_planes')
    planes_cl = torch.empty(b, 3, 256, 256, 32, device=stitch.device, dtype=torch.float32)
    y0, y1, x0, x1 = bbox
    with torch.cuda.device(stitch.device):
        st = _lib.load().ia_blend_planes(_p(_f32c(stitch, 'stitch')), _p(_f32c(full_alpha, 'full_alpha')),
                                         static_planes.data_ptr(), static_planes.stride(0), _p(planes_cl),
                                         b, y0, y1, x0, x1, _lib.stream_ptr(stitch.device))
    _lib.check(st, 'ia_blend_planes')
    return planes_cl


class StylePlan:
    """Device tables describing every modulated layer of one synthesis network (see ia_styles_demod).

    `layers` is a list of (module, w_index): module has .affine (FullyConnectedLayer), .weight and `demodulate`
    semantics given by `hasattr(module, 'noise_strength') or module is a SynthesisLayer` -> passed explicitly."""

    def __init__(self, entries, device):
        # entries: list of dict(affine=FC module, weight=conv weight param, widx=int, demod=bool)
        self.entries = entries
        self.device = device
        self.key = None
        self._build()

    def _signature(self):
        sig = []
        for e in self.entries:
            sig += [e['affine'].weight.data_ptr(), e['affine'].weight._version, e['weight'].data_ptr(), e['weight']._version]
        return tuple(sig)

    def _build(self):
        rows, soff, doff = [], 0, 0
        table, gains, srl, drl = [], [], [], []
        self.keep = []
        for li, e in enumerate(self.entries):
            fc = e['affine']
            a = fc.weight.detach().float().contiguous()
            bias = fc.bias.detach().float().contiguous() if fc.bias is not None else None
            i_dim = a.shape[0]
            wsq = weight_sq_sum(e['weight']) if e['demod'] else None
            o_dim = e['weight'].shape[0]
            self.keep += [a, bias, wsq]
            table.append([a.data_ptr(), bias.data_ptr() if bias is not None else 0, wsq.data_ptr() if wsq is not None else 0,
                          i_dim, o_dim, e['widx'], soff, doff if e['demod'] else -1])
            gains.append([float(fc.weight_gain), float(fc.bias_gain)])
            srl += [li] * i_dim
            e['soff'], e['I'] = soff, i_dim
            soff += i_dim
            if e['demod']:
                drl += [li] * o_dim
                e['doff'], e['O'] = doff, o_dim
                doff += o_dim
        dev = self.device
        self.table = torch.tensor(table, dtype=torch.int64, device=dev)
        self.gains = torch.tensor(gains, dtype=torch.float32, device=dev)
        self.srl = torch.tensor(srl, dtype=torch.int32, device=dev)
        self.drl = torch.tensor(drl if drl else [0], dtype=torch.int32, device=dev)
        self.srows, self.drows = soff, doff
        self.key = self._signature()

    def run(self, ws):
        """ws [B, num_ws, w_dim] -> list of (styles [B,I], demod [B,O] or None) per entry (views into two buffers)."""
        if self._signature() != self.key:
            self._build()
        ws = _f32c(ws.float().contiguous(), 'ws')
        b, num_ws, w_dim = ws.shape
        styles = torch.empty(b * self.srows, device=ws.device)
        demod = torch.empty(b * max(self.drows, 1), device=ws.device)
        with torch.cuda.device(ws.device):
            st = _lib.load().ia_styles_demod(_p(ws), b, num_ws, w_dim, _p(self.table), _p(self.gains), _p(self.srl), self.srows,
                                             _p(self.drl), self.drows, _p(styles), _p(demod), _lib.stream_ptr(ws.device))
        _lib.check(st, 'ia_styles_demod')
        self.last_buffers = (styles, demod)      # alive until the next run: the per-layer views may be consumed on other streams than this one
        out = []
        for e in self.entries:
            s = styles[b * e['soff']:b * (e['soff'] + e['I'])].view(b, e['I'])
            d = demod[b * e['doff']:b * (e['doff'] + e['O'])].view(b, e['O']) if e['demod'] else None
            out.append((s, d))
        return out


def ray_sampler(cam25, resolution, normalize=True):
    """cam25 [B,25] (cam2world 16 + intrinsics 9) -> rays_o, rays_d [B, res^2, 3] (see ia_ray_sampler)."""
    cam25 = _f32c(cam25.float().contiguous(), 'cam')
    b = cam25.shape[0]
    rays_o = torch.empty(b, resolution * resolution, 3, device=cam25.device)
    rays_d = torch.empty_like(rays_o)
    with torch.cuda.device(cam25.device):
        st = _lib.load().ia_ray_sampler(_p(cam25), cam25.stride(0), _p(rays_o), _p(rays_d), b, int(resolution), int(bool(normalize)),
                                        _lib.stream_ptr(cam25.device))
    _lib.check(st, 'ia_ray_sampler')
    return rays_o, rays_d


def convgru_gates(gates_pre, x, h):
    """cat[x, sigmoid(r_pre) * h] (see ia_convgru_gates)."""
    b, c, hh, w = x.shape
    xrh = torch.empty(b, 2 * c, hh, w, device=x.device, dtype=torch.float32)
    with torch.cuda.device(x.device):
        st = _lib.load().ia_convgru_gates(_p(_f32c(gates_pre, 'gates_pre')), _p(_f32c(x, 'x')), _p(_f32c(h, 'h')), _p(xrh), b, c, hh, w,
                                          _lib.stream_ptr(x.device))
    _lib.check(st, 'ia_convgru_gates')
    return xrh


def convgru_update(gates_pre, cand_pre, h, prelu_weight=None, x_next=None):
    """h' = (1 - z) h + z tanh(c_pre) and, with x_next, cat[x_next, h'] for the next step (see ia_convgru_update)."""
    b, c, hh, w = h.shape
    h_out = torch.empty_like(h)
    xh = torch.empty(b, 2 * c, hh, w, device=h.device, dtype=torch.float32) if x_next is not None else None
    with torch.cuda.device(h.device):
        st = _lib.load().ia_convgru_update(_p(_f32c(gates_pre, 'gates_pre')), _p(_f32c(cand_pre, 'cand_pre')), _p(_f32c(h, 'h')),
                                           _p(None if prelu_weight is None else _f32c(prelu_weight, 'prelu_weight')), _p(h_out),
                                           _p(None if x_next is None else _f32c(x_next, 'x_next')), _p(xh), b, c, hh, w, _lib.stream_ptr(h.device))
    _lib.check(st, 'ia_convgru_update')
    return h_out, xh



def convgru_gates_split(gates_pre, x, h, consumer=None):
    """SplitAct of cat[x, sigmoid(r_pre) * h] (see ia_convgru_gates_split): the input of the cell's second convolution."""
    b, c, hh, w = x.shape
    out = torch.empty(b, 2, 2 * c // 8, hh, w, 8, device=x.device, dtype=torch.float16)
    with torch.cuda.device(x.device):
        st = _lib.load().ia_convgru_gates_split(_p(_f32c(gates_pre, 'gates_pre')), _p(_f32c(x, 'x')), _p(_f32c(h, 'h')), _p(out), b, c, hh, w,
                                                _lib.stream_ptr(x.device))
    _lib.check(st, 'ia_convgru_gates_split')
    return SplitAct(out, 2 * c, consumer)


def convgru_update_split(gates_pre, cand_pre, h, prelu_weight=None, x_next=None, consumer=None):
    """h' (fp32) and, with x_next, the SplitAct of cat[x_next, h'] for the next step's first convolution (see ia_convgru_update_split)."""
    b, c, hh, w = h.shape
    h_out = torch.empty_like(h)
    xh = torch.empty(b, 2, 2 * c // 8, hh, w, 8, device=h.device, dtype=torch.float16) if x_next is not None else None
    with torch.cuda.device(h.device):
        st = _lib.load().ia_convgru_update_split(_p(_f32c(gates_pre, 'gates_pre')), _p(_f32c(cand_pre, 'cand_pre')), _p(_f32c(h, 'h')),
                                                 _p(None if prelu_weight is None else _f32c(prelu_weight, 'prelu_weight')), _p(h_out),
                                                 _p(None if x_next is None else _f32c(x_next, 'x_next')), _p(xh), b, c, hh, w, _lib.stream_ptr(h.device))
    _lib.check(st, 'ia_convgru_update_split')
    return h_out, (SplitAct(xh, 2 * c, consumer) if xh is not None else None)


def stage_inputs(pairs):
    """Copy each (src, dst) pair of same-shaped contiguous device tensors in ONE launch (ia_stage_inputs): the per-frame inputs
    of a captured frame into the graph's static buffers.  Pairs the kernel cannot take (broadcast / strided / other dtype sources)
    fall through to Tensor.copy_."""
    import ctypes
    segs = []
    for src, dst in pairs:
        if (src.is_cuda and src.device == dst.device and src.dtype == dst.dtype and src.shape == dst.shape
                and src.is_contiguous() and dst.is_contiguous() and src.numel() > 0):
            segs.append((src, dst))
        else:
            dst.copy_(src)
    for i in range(0, len(segs), 8):
        part = segs[i:i + 8]
        n = len(part)
        srcs = (ctypes.c_void_p * n)(*[s_.data_ptr() for s_, _ in part])
        dsts = (ctypes.c_void_p * n)(*[d_.data_ptr() for _, d_ in part])
        nbytes = (ctypes.c_int64 * n)(*[s_.numel() * s_.element_size() for s_, _ in part])
        dev = part[0][1].device
        with torch.cuda.device(dev):
            st = _lib.load().ia_stage_inputs(srcs, dsts, nbytes, n, _lib.stream_ptr(dev))
        _lib.check(st, 'ia_stage_inputs')


def attention(q, kv, heads, scale):
    """softmax(Q K^T * scale) V per head in one launch (see ia_attention).  q [B,N,C], kv [B,M,2C] (k = kv[..., :C], v = kv[..., C:]);
    returns [B,N,C]."""
    _f32c(q, 'q')
    _f32c(kv, 'kv')
    b, n, c = q.shape
    m = kv.shape[1]
    if kv.shape[0] != b or kv.shape[2] != 2 * c or c % heads:
        raise RuntimeError(f'attention: q {tuple(q.shape)} / kv {tuple(kv.shape)} / {heads} heads do not fit together')
    out = torch.empty_like(q)
    k, v = kv[..., :c], kv[..., c:]
    with torch.cuda.device(q.device), _Timed('attention', 4.0 * b * n * m * c, 4.0 * (q.numel() + kv.numel() + out.numel()), f'B{b} N{n} M{m} C{c}'):
        st = _lib.load().ia_attention(_p(q), k.data_ptr(), v.data_ptr(), _p(out), b, heads, n, m, c // heads, q.stride(0), q.stride(1),
                                      kv.stride(0), kv.stride(1), kv.stride(0), kv.stride(1), out.stride(0), out.stride(1), float(scale),
                                      _lib.stream_ptr(q.device))
    _lib.check(st, 'ia_attention')
    return out


class SplitTokens:
    """A token matrix [M, K] stored as fp16 hi / lo pairs [2, K/8, M, 8] (ia_tokens_split): the operand of linear_sx."""

    def __init__(self, data, rows, cols, lead_shape):
        self.data, self.rows, self.cols, self.lead_shape = data, rows, cols, tuple(lead_shape)


def linear_supported(in_features):
    return in_features % 16 == 0


def pack_linear_weight_split(w):
    """nn.Linear weight [N, K] -> the convolution weight format of a 1x1 kernel, fp16 [2, 1, K/8, N, 8] with its scale as `.wk_exp`
    (pack_conv_weight_split): the weight operand of linear_sx."""
    n, k = w.shape
    return pack_conv_weight_split(w.detach().reshape(n, k, 1, 1))


def tokens_split(x):
    """fp32 [..., K] (rows contiguous, or a column slice of such a tensor: rows x.stride(-2) apart) -> SplitTokens (see ia_tokens_split).
    One split serves every linear layer that reads x."""
    if not (x.is_cuda and x.dtype == torch.float32 and x.stride(-1) == 1):
        raise RuntimeError('tokens_split: x must be a float32 device tensor with contiguous rows')
    k = x.shape[-1]
    m = x.numel() // k
    ld = k
    if not x.is_contiguous():
        ld = x.stride(-2)
        if x.dim() < 2 or any(x.stride(d) != x.stride(d + 1) * x.shape[d + 1] for d in range(x.dim() - 2)):
            raise RuntimeError('tokens_split: rows must be evenly spaced')
    out = torch.empty(2, k // 8, m, 8, device=x.device, dtype=torch.float16)
    with torch.cuda.device(x.device), _Timed('tokens_split', 0.0, 8.0 * x.numel(), f'M{m} K{k}'):
        st = _lib.load().ia_tokens_split(_p(x), int(ld), _p(out), m, k, _lib.stream_ptr(x.device))
    _lib.check(st, 'ia_tokens_split')
    return SplitTokens(out, m, k, x.shape[:-1])


def layernorm_split_supported(k):
    return k in (512, 1024, 2048)


def layernorm_split(x, norm):
    """nn.LayerNorm `norm` over the last dimension of x [..., K] + tokens_split of the result, one launch (see ia_layernorm_split)."""
    _f32c(x, 'x')
    k = x.shape[-1]
    m = x.numel() // k
    out = torch.empty(2, k // 8, m, 8, device=x.device, dtype=torch.float16)
    with torch.cuda.device(x.device), _Timed('layernorm_split', 8.0 * x.numel(), 8.0 * x.numel(), f'M{m} K{k}'):
        st = _lib.load().ia_layernorm_split(_p(x), _p(_f32c(norm.weight.detach(), 'weight')), _p(_f32c(norm.bias.detach(), 'bias')), float(norm.eps),
                                            _p(out), m, k, _lib.stream_ptr(x.device))
    _lib.check(st, 'ia_layernorm_split')
    return SplitTokens(out, m, k, x.shape[:-1])


ATTENTION_SX_ONE_LAUNCH = True      # head_dim 256: ia_attention_sx (online softmax) instead of matmul / softmax / matmul


def attention_sx_supported(head_dim, n, m):
    return head_dim % 16 == 0 and m % 16 == 0 and m <= 4096


def attention_sx(q, kv, heads, scale):
    """softmax(Q K^T * scale) V per head through the fp16-pair GEMM (see ia_matmul_sx): q [B, N, C], kv [B, M, 2C] (k = kv[..., :C],
    v = kv[..., C:]); returns [B, N, C].  The score matrix [heads, N, M] passes through HBM once (fp32) and once as fp16 pairs."""
    _f32c(q, 'q')
    _f32c(kv, 'kv')
    b, n, c = q.shape
    m = kv.shape[1]
    hd = c // heads
    if kv.shape[0] != b or kv.shape[2] != 2 * c or c % heads or not attention_sx_supported(hd, n, m):
        raise RuntimeError(f'attention_sx: q {tuple(q.shape)} / kv {tuple(kv.shape)} / {heads} heads are not covered')
    lib, dev = _lib.load(), q.device
    out = torch.empty_like(q)
    with torch.cuda.device(dev), _Timed('attention_sx', 4.0 * b * n * m * c, 4.0 * (q.numel() + kv.numel() + out.numel()) + 16.0 * b * heads * n * m,
                                        f'B{b} N{n} M{m} C{c}'):
        s_ = _lib.stream_ptr(dev)
        scores = torch.empty(heads, n, m, device=dev, dtype=torch.float32)
        probs = torch.empty(2, heads, m // 8, n, 8, device=dev, dtype=torch.float16)
        vt = torch.empty(2, m // 8, c, 8, device=dev, dtype=torch.float16)
        for i in range(b):
            qs, ks = tokens_split(q[i]), tokens_split(kv[i, :, :c])
            flash = ATTENTION_SX_ONE_LAUNCH and bool(lib.ia_attention_sx_supported(hd, n, m))
            _lib.check(lib.ia_tokens_split_t(kv[i, :, c:].data_ptr(), kv.stride(1), _p(vt), m, c, int(flash), s_), 'ia_tokens_split_t')
            if flash:        # one launch, no score matrix (head_dim 256)
                _lib.check(lib.ia_attention_sx(_p(qs.data), _p(ks.data), _p(vt), _p(out[i]), heads, n, m, hd, float(scale), s_), 'ia_attention_sx')
                continue
            _lib.check(lib.ia_matmul_sx(_p(qs.data), _p(ks.data), _p(scores), heads, n, m, hd, n, (c // 8) * n * 16, (hd // 8) * n * 16,
                                        m, (c // 8) * m * 16, (hd // 8) * m * 16, n * m, m, float(scale), s_), 'ia_matmul_sx')
            _lib.check(lib.ia_softmax_split(_p(scores), _p(probs), heads, n, m, s_), 'ia_softmax_split')
            _lib.check(lib.ia_matmul_sx(_p(probs), _p(vt), _p(out[i]), heads, n, hd, m, n, heads * (m // 8) * n * 16, (m // 8) * n * 16,
                                        c, (m // 8) * c * 16, hd * 16, hd, c, 1.0, s_), 'ia_matmul_sx')
    return out


def pack_patch_weight_split(w):
    """Conv2d weight [N, C, k, k] -> pack_linear_weight_split of its [N, C*k*k] matrix, columns zero-padded to a multiple of 16: the
    weight operand of linear_sx over im2col_split tokens."""
    n = w.shape[0]
    w2 = w.detach().reshape(n, -1)
    kp = (w2.shape[1] + 15) // 16 * 16
    if kp != w2.shape[1]:
        w2 = torch.nn.functional.pad(w2, (0, kp - w2.shape[1]))
    return pack_linear_weight_split(w2.contiguous())


def im2col_split(x, ksize, stride, pad):
    """NCHW fp32 image -> SplitTokens of its ksize x ksize patches (see ia_im2col_split); lead shape (B, OH * OW)."""
    _f32c(x, 'x')
    b, c, h, w = x.shape
    oh, ow = (h + 2 * pad - ksize) // stride + 1, (w + 2 * pad - ksize) // stride + 1
    kp = (c * ksize * ksize + 15) // 16 * 16
    m = b * oh * ow
    out = torch.empty(2, kp // 8, m, 8, device=x.device, dtype=torch.float16)
    with torch.cuda.device(x.device), _Timed('im2col_split', 0.0, 4.0 * x.numel() + 4.0 * m * kp, f'B{b} C{c} {h}x{w} k{ksize} s{stride}'):
        st = _lib.load().ia_im2col_split(_p(x), _p(out), b, c, h, w, int(ksize), int(stride), int(pad), _lib.stream_ptr(x.device))
    _lib.check(st, 'ia_im2col_split')
    t = SplitTokens(out, m, kp, (b, oh * ow))
    t.grid = (oh, ow)
    return t


def linear_sx_splitk(xs, w_split, bias=None):
    """linear_sx with K cut over the launch when the library's plan says so (few rows, very long K; see ia_linear_sx_splitk)."""
    k8, n = w_split.shape[2], w_split.shape[3]
    ks, nbytes = ctypes.c_int(0), ctypes.c_size_t(0)
    _lib.check(_lib.load().ia_linear_splitk_plan(xs.rows, xs.cols, n, ctypes.byref(ks), ctypes.byref(nbytes)), 'ia_linear_splitk_plan')
    if ks.value <= 1:
        return linear_sx(xs, w_split, bias)
    if k8 * 8 != xs.cols:
        raise RuntimeError(f'linear_sx_splitk: {xs.cols} input features against a weight of {k8 * 8}')
    y = torch.empty(*xs.lead_shape, n, device=xs.data.device, dtype=torch.float32)
    scratch = torch.empty(nbytes.value // 4, device=y.device, dtype=torch.float32)
    with torch.cuda.device(y.device), _Timed('linear_sx', 2.0 * xs.rows * xs.cols * n, 4.0 * (xs.rows * xs.cols + xs.cols * n + y.numel()),
                                             f'M{xs.rows} K{xs.cols} N{n} splitk{ks.value}'):
        st = _lib.load().ia_linear_sx_splitk(_p(xs.data), _p(w_split), int(w_split.wk_exp), _p(None if bias is None else _f32c(bias, 'bias')), _p(y),
                                             xs.rows, xs.cols, n, ks.value, _p(scratch), nbytes.value, _lib.stream_ptr(y.device))
    _lib.check(st, 'ia_linear_sx_splitk')
    return y


def linear_sx(xs, w_split, bias=None, residual=None, gelu=False):
    """act(x @ w^T + bias) + residual on the fp16-pair GEMM (see ia_linear_sx).  xs: SplitTokens; w_split: pack_linear_weight_split(w);
    residual: fp32 [..., N] like the output.  Returns fp32 [*lead, N]."""
    if not (w_split.dtype == torch.float16 and w_split.dim() == 5 and w_split.shape[0] == 2 and w_split.shape[1] == 1 and hasattr(w_split, 'wk_exp')):
        raise RuntimeError('linear_sx: the weight must come from pack_linear_weight_split')
    k8, n = w_split.shape[2], w_split.shape[3]
    if k8 * 8 != xs.cols:
        raise RuntimeError(f'linear_sx: {xs.cols} input features against a weight of {k8 * 8}')
    y = torch.empty(*xs.lead_shape, n, device=xs.data.device, dtype=torch.float32)
    if residual is not None:
        _f32c(residual, 'residual')
        if residual.shape != y.shape:
            raise RuntimeError(f'linear_sx: residual {tuple(residual.shape)} against an output of {tuple(y.shape)}')
    with torch.cuda.device(y.device), _Timed('linear_sx', 2.0 * xs.rows * xs.cols * n, 4.0 * (xs.rows * xs.cols + xs.cols * n + y.numel()),
                                             f'M{xs.rows} K{xs.cols} N{n}'):
        st = _lib.load().ia_linear_sx(_p(xs.data), _p(w_split), int(w_split.wk_exp), _p(None if bias is None else _f32c(bias, 'bias')),
                                      _p(residual), _p(y), xs.rows, xs.cols, n, int(bool(gelu)), _lib.stream_ptr(y.device))
    _lib.check(st, 'ia_linear_sx')
    return y


def se_gate_split(v, shortcut, w1, w2, next_scale=None, next_shift=None, consumer=None):
    """ia_se_gate_split: (out, SplitAct of out * next_scale + next_shift or None).  next_scale / next_shift: [B, C] rows (the eval-mode
    BatchNorm in front of the convolution that reads `out` next) or both None."""
    b, c, h, w = v.shape
    if not (v.is_cuda and v.dtype == torch.float32 and shortcut.dtype == torch.float32 and tuple(shortcut.shape) == (b, c, h, w)):
        raise RuntimeError('se_gate_split: v and shortcut must be float32 device tensors of one shape')
    if (next_scale is None) != (next_shift is None):
        raise RuntimeError('next_scale and next_shift come together')
    r = w1.shape[0]
    _f32c(w1, 'w1'); _f32c(w2, 'w2')
    if next_scale is not None and (_f32c(next_scale, 'next_scale').numel() != b * c or _f32c(next_shift, 'next_shift').numel() != b * c):
        raise RuntimeError(f'next_scale / next_shift must have {b} x {c} elements')
    out = torch.empty(b, c, h, w, device=v.device, dtype=torch.float32)
    pooled = torch.empty(b * c, device=v.device, dtype=torch.float32)
    ys = torch.empty(b, 2, c // 8, h, w, 8, device=v.device, dtype=torch.float16) if next_scale is not None else None
    with torch.cuda.device(v.device):
        st = _lib.load().ia_se_gate_split(v.data_ptr(), _lib.strides64(v), shortcut.data_ptr(), _lib.strides64(shortcut), _p(w1), _p(w2), _p(pooled),
                                          _p(out), _p(next_scale), _p(next_shift), _p(ys), b, c, r, h, w, _lib.stream_ptr(v.device))
    _lib.check(st, 'ia_se_gate_split')
    return out, (SplitAct(ys, c, consumer) if ys is not None else None)


def se_gate(v, shortcut, w1, w2):
    """v * sigmoid(w2 relu(w1 mean_hw(v))) + shortcut (see ia_se_gate).  v, shortcut: fp32 [B,C,H,W] views (any strides);
    w1 [R,C], w2 [C,R]."""
    b, c, h, w = v.shape
    if not (v.is_cuda and v.dtype == torch.float32 and shortcut.dtype == torch.float32 and tuple(shortcut.shape) == (b, c, h, w)):
        raise RuntimeError('se_gate: v and shortcut must be float32 device tensors of one shape')
    r = w1.shape[0]
    _f32c(w1, 'w1'); _f32c(w2, 'w2')
    out = torch.empty(b, c, h, w, device=v.device, dtype=torch.float32)
    pooled = torch.empty(b * c, device=v.device, dtype=torch.float32)
    with torch.cuda.device(v.device):
        st = _lib.load().ia_se_gate(v.data_ptr(), _lib.strides64(v), shortcut.data_ptr(), _lib.strides64(shortcut), _p(w1), _p(w2), _p(pooled),
                                    _p(out), b, c, r, h, w, _lib.stream_ptr(v.device))
    _lib.check(st, 'ia_se_gate')
    return out


# ------------------------------------------------------------------ shared by the geometry wrappers below

def _f3(values):
    return (ctypes.c_float * 3)(*[float(v) for v in values])


def _i3(values):
    return (ctypes.c_int * 3)(*[int(v) for v in values])


def _d3(values):
    return (ctypes.c_double * 3)(*[float(v) for v in values])


def _i32c(t, what):
    if not (t.is_cuda and t.dtype == torch.int32 and t.is_contiguous()):
        raise RuntimeError(f'{what} must be a contiguous int32 device tensor')
    return t


def _volume_checked(volume):
    _f32c(volume, 'volume')
    if volume.dim() != 3:
        raise RuntimeError(f'volume must be [nx,ny,nz], got {tuple(volume.shape)}')
    return tuple(int(n) for n in volume.shape)


def _mesh_checked(verts, faces):
    _f32c(verts, 'verts')
    _i32c(faces, 'faces')
    if verts.dim() != 2 or verts.shape[1] != 3 or faces.dim() != 2 or faces.shape[1] != 3 or faces.device != verts.device:
        raise RuntimeError(f'a mesh is verts [V,3] and faces [F,3] on one device, got {tuple(verts.shape)} and {tuple(faces.shape)}')
    return verts.shape[0], faces.shape[0]


def _scratch(fn_name, *args, dtype, device, extra=0):
    """The scratch buffer that the library's ``fn_name(*args, &bytes)`` asks for, rounded up to whole elements of ``dtype`` (plus
    ``extra`` elements) -> (tensor, its size in bytes)."""
    nbytes = ctypes.c_size_t(0)
    _lib.check(getattr(_lib.load(), fn_name)(*args, ctypes.byref(nbytes)), fn_name)
    t = torch.empty(-(-nbytes.value // dtype.itemsize) + extra, dtype=dtype, device=device)
    return t, t.numel() * dtype.itemsize


SIMPLIFY_TIMES = None        # a dict collects seconds per phase (each phase then ends in a device synchronise): tools/bench_simplify.py
SMOOTH_TIMES = None          # the same for the smoothing wrappers: tools/bench_smooth.py


class _Phase:
    """Adds the seconds of its block to entry ``name`` of the module-level dict named ``times``, while that is not None."""
    def __init__(self, name, dev, times):
        self.name, self.dev, self.times = name, dev, times

    def __enter__(self):
        if globals()[self.times] is not None:
            import time
            torch.cuda.synchronize(self.dev)
            self.t0 = time.perf_counter()
        return self

    def __exit__(self, *exc):
        acc = globals()[self.times]
        if acc is not None:
            import time
            torch.cuda.synchronize(self.dev)
            acc[self.name] = acc.get(self.name, 0.0) + time.perf_counter() - self.t0
        return False


# ------------------------------------------------------------------ avatar geometry (csrc/geometry.hip)

def _decoder_checked(w0, b0, w1, b1):
    for name, t in (('w0', w0), ('b0', b0), ('w1', w1), ('b1', b1)):
        _f32c(t, name)
    if tuple(w0.shape) != (64, 32) or b0.numel() != 64 or tuple(w1.shape) != (33, 64) or b1.numel() != 33:
        raise RuntimeError('decoder weights must be the OSGDecoder shapes w0 [64,32], b0 [64], w1 [33,64], b1 [33]')


def _planes_checked(planes_cl):
    _f32c(planes_cl, 'planes')
    if planes_cl.dim() != 5 or planes_cl.shape[1] != 3 or planes_cl.shape[4] != 32:
        raise RuntimeError(f'planes must be [B,3,H,W,32] channels-last, got {tuple(planes_cl.shape)}')
    return planes_cl.shape[0], planes_cl.shape[2], planes_cl.shape[3]


def query_planes(planes_cl, points, w0, b0, w1, b1, lr_multiplier=1.0, box_warp=1.0, flip_z=False, rgb=True):
    """Decoder output at points (see ia_query_planes): planes [B,3,H,W,32], points [B,M,3] -> (sigma [B,M,1], rgb [B,M,32] or None)."""
    b, ph, pw = _planes_checked(planes_cl)
    _decoder_checked(w0, b0, w1, b1)
    _f32c(points, 'points')
    if points.dim() != 3 or points.shape[0] != b or points.shape[2] != 3:
        raise RuntimeError(f'points must be [B={b},M,3], got {tuple(points.shape)}')
    m = points.shape[1]
    dev = planes_cl.device
    sigma = torch.empty(b, m, 1, device=dev)
    col = torch.empty(b, m, 32, device=dev) if rgb else None
    flops = b * m * 2.0 * (32 * 64 + 64 * (33 if rgb else 1))
    traffic = 4.0 * b * m * (3 + 1 + (32 if rgb else 0)) + 4.0 * planes_cl.numel()
    with torch.cuda.device(dev), _Timed('query_planes', flops, traffic, f'M={m}'):
        st = _lib.load().ia_query_planes(_p(planes_cl), _p(points), _p(w0), _p(b0), _p(w1), _p(b1), float(lr_multiplier), float(box_warp),
                                         1 if flip_z else 0, b, m, ph, pw, _p(sigma), _p(col), _lib.stream_ptr(dev))
    _lib.check(st, 'ia_query_planes')
    return sigma, col


def density_grid(planes_cl, w0, b0, w1, b1, res, cube_length, origin, lr_multiplier=1.0, box_warp=1.0, flip_z=False):
    """Density on the nx x ny x nz lattice of `cube_length` / `origin` (per-axis triples): [B,nx,ny,nz] (see ia_density_grid)."""
    b, ph, pw = _planes_checked(planes_cl)
    _decoder_checked(w0, b0, w1, b1)
    nx, ny, nz = (int(r) for r in res)
    dev = planes_cl.device
    vol = torch.empty(b, nx, ny, nz, device=dev)
    n = b * nx * ny * nz
    with torch.cuda.device(dev), _Timed('density_grid', n * 2.0 * (32 * 64 + 64), 4.0 * (n + planes_cl.numel()), f'{nx}x{ny}x{nz}'):
        st = _lib.load().ia_density_grid(_p(planes_cl), _p(w0), _p(b0), _p(w1), _p(b1), float(lr_multiplier), float(box_warp),
                                         1 if flip_z else 0, b, ph, pw, nx, ny, nz, _f3(cube_length), _f3(origin), _p(vol),
                                         _lib.stream_ptr(dev))
    _lib.check(st, 'ia_density_grid')
    return vol


def marching_cubes(volume, level, origin=(0.0, 0.0, 0.0), spacing=(1.0, 1.0, 1.0)):
    """Mesh of {volume > level} (see ia_mc_count / ia_mc_emit): volume [nx,ny,nz] -> (verts float32 [V,3], faces int32 [F,3]).
    One host synchronisation (the two totals)."""
    nx, ny, nz = _volume_checked(volume)
    lib, dev = _lib.load(), volume.device
    scratch, nbytes = _scratch('ia_mc_scratch_bytes', nx, ny, nz, dtype=torch.uint8, device=dev)
    totals = torch.empty(2, dtype=torch.int32, device=dev)
    stream = _lib.stream_ptr(dev)
    with torch.cuda.device(dev):
        with _Timed('mc_count', 0.0, 4.0 * volume.numel() + nbytes, f'{nx}x{ny}x{nz}'):
            st = lib.ia_mc_count(_p(volume), nx, ny, nz, float(level), _p(scratch), nbytes, _p(totals), stream)
        _lib.check(st, 'ia_mc_count')
        n_verts, n_faces = (int(v) for v in totals.cpu())
        if n_verts < 0 or n_faces < 0:
            raise RuntimeError(f'marching_cubes: more than 2^31 - 1 vertices or triangles in a {nx}x{ny}x{nz} volume')
        verts = torch.empty(n_verts, 3, device=dev)
        faces = torch.empty(n_faces, 3, dtype=torch.int32, device=dev)
        with _Timed('mc_emit', 0.0, 4.0 * volume.numel() + nbytes + 12.0 * (n_verts + n_faces), f'{nx}x{ny}x{nz}'):
            st = lib.ia_mc_emit(_p(volume), nx, ny, nz, float(level), _f3(origin), _f3(spacing), _p(scratch), nbytes,
                                _p(verts), n_verts, _p(faces), n_faces, stream)
        _lib.check(st, 'ia_mc_emit')
    return verts, faces


def _rays_checked(t, what, device):
    _f32c(t, what)
    if t.dim() != 2 or t.shape[1] != 3 or t.device != device:
        raise RuntimeError(f'{what} must be [n,3] on {device}, got {tuple(t.shape)} on {t.device}')
    return t.shape[0]


def volume_bricks(volume):
    """{min, max} per brick of 8^3 cells (see ia_volume_bricks): volume [nx,ny,nz] -> [bx,by,bz,2] float32."""
    nx, ny, nz = _volume_checked(volume)
    dev = volume.device
    bricks, nbytes = _scratch('ia_raycast_scratch_bytes', nx, ny, nz, dtype=torch.float32, device=dev)
    bricks = bricks.view((nx + 6) // 8, (ny + 6) // 8, (nz + 6) // 8, 2)
    with torch.cuda.device(dev), _Timed('volume_bricks', 0.0, 4.0 * volume.numel(), f'{nx}x{ny}x{nz}'):
        st = _lib.load().ia_volume_bricks(_p(volume), nx, ny, nz, _p(bricks), nbytes, _lib.stream_ptr(dev))
    _lib.check(st, 'ia_volume_bricks')
    return bricks


def raycast_volume(volume, level, lo, step, rays_o, rays_d, t_min=0.0, bricks=None):
    """First hit of each ray with {volume > level} (see ia_raycast_volume): rays [n,3] -> (depth [n], normal [n,3], mask bool [n]).
    With ``bricks`` (from ``volume_bricks``) empty bricks are skipped; without, every cell is walked.  The results are the same."""
    nx, ny, nz = _volume_checked(volume)
    dev = volume.device
    n = _rays_checked(rays_o, 'rays_o', dev)
    if _rays_checked(rays_d, 'rays_d', dev) != n:
        raise RuntimeError(f'rays_o and rays_d differ in length: {n} vs {rays_d.shape[0]}')
    if bricks is not None:
        _f32c(bricks, 'bricks')
    depth = torch.empty(n, device=dev)
    normal = torch.empty(n, 3, device=dev)
    mask = torch.empty(n, dtype=torch.uint8, device=dev)
    if n == 0:
        return depth, normal, mask.bool()
    with torch.cuda.device(dev), _Timed('raycast_volume', 0.0, 40.0 * n, f'{nx}x{ny}x{nz} rays={n}'):
        st = _lib.load().ia_raycast_volume(_p(volume), nx, ny, nz, _f3(lo), _f3(step), float(level), _p(bricks),
                                           0 if bricks is None else bricks.numel() * 4, _p(rays_o), _p(rays_d), n, float(t_min),
                                           _p(depth), _p(normal), _p(mask), 1 if bricks is None else 0, _lib.stream_ptr(dev))
    _lib.check(st, 'ia_raycast_volume')
    return depth, normal, mask.view(torch.bool)


def volume_gradient(volume, lo, step, points):
    """Interpolated central-difference gradient of the volume at points [n,3] (see ia_volume_gradient) -> [n,3]."""
    nx, ny, nz = _volume_checked(volume)
    dev = volume.device
    n = _rays_checked(points, 'points', dev)
    grad = torch.empty(n, 3, device=dev)
    with torch.cuda.device(dev), _Timed('volume_gradient', 0.0, 24.0 * n, f'{nx}x{ny}x{nz} points={n}'):
        st = _lib.load().ia_volume_gradient(_p(volume), nx, ny, nz, _f3(lo), _f3(step), _p(points), n, _p(grad), _lib.stream_ptr(dev))
    _lib.check(st, 'ia_volume_gradient')
    return grad


# ------------------------------------------------------------------ connected components (csrc/components.hip)

def volume_components(volume, level, connectivity=26):
    """Components of {volume > level} (see ia_volume_components): volume [nx,ny,nz] -> (labels int32 [nx,ny,nz], K).  One host
    synchronisation (K)."""
    nx, ny, nz = _volume_checked(volume)
    lib, dev = _lib.load(), volume.device
    scratch, nbytes = _scratch('ia_components_scratch_bytes', nx, ny, nz, dtype=torch.int32, device=dev)
    labels = torch.empty(nx, ny, nz, dtype=torch.int32, device=dev)
    count = torch.empty(1, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        with _Timed('volume_components', 0.0, 4.0 * volume.numel() * 8, f'{nx}x{ny}x{nz} c{connectivity}'):
            st = lib.ia_volume_components(_p(volume), nx, ny, nz, float(level), int(connectivity), _p(labels), _p(scratch),
                                          nbytes, _p(count), _lib.stream_ptr(dev))
        _lib.check(st, 'ia_volume_components')
        return labels, int(count.cpu())


def component_stats(labels, k):
    """Per-component statistics (see ia_component_stats): labels int32 [nx,ny,nz], K -> int32 [K,8] = count, smallest linear index,
    imin, jmin, kmin, imax, jmax, kmax."""
    _i32c(labels, 'labels')
    if labels.dim() != 3:
        raise RuntimeError(f'labels must be [nx,ny,nz], got {tuple(labels.shape)}')
    nx, ny, nz = labels.shape
    dev = labels.device
    stats = torch.empty(max(int(k), 0), 8, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev), _Timed('component_stats', 0.0, 4.0 * labels.numel(), f'{nx}x{ny}x{nz} K={k}'):
        st = _lib.load().ia_component_stats(_p(labels), nx, ny, nz, int(k), _p(stats), _lib.stream_ptr(dev))
    _lib.check(st, 'ia_component_stats')
    return stats


def volume_keep(volume, labels, keep_flags, fill, out=None):
    """The filter (see ia_volume_keep): points of components 1..K whose flag is 0 become ``fill``; keep_flags uint8 [K+1] on the device.
    ``out``: where to write (``volume`` itself for in place); default a new tensor."""
    _f32c(volume, 'volume')
    _i32c(labels, 'labels')
    if labels.shape != volume.shape or labels.device != volume.device:
        raise RuntimeError(f'labels {tuple(labels.shape)} on {labels.device} do not match volume {tuple(volume.shape)} on {volume.device}')
    if not (keep_flags.is_cuda and keep_flags.dtype == torch.uint8 and keep_flags.is_contiguous() and keep_flags.dim() == 1
            and keep_flags.numel() >= 1 and keep_flags.device == volume.device):
        raise RuntimeError('keep_flags must be a contiguous uint8 device tensor [K+1] on the volume\'s device')
    if out is None:
        out = torch.empty_like(volume)
    elif not (out.is_cuda and out.dtype == torch.float32 and out.is_contiguous() and out.shape == volume.shape and out.device == volume.device):
        raise RuntimeError('out must be a contiguous float32 tensor of the volume\'s shape and device')
    dev = volume.device
    with torch.cuda.device(dev), _Timed('volume_keep', 0.0, 12.0 * volume.numel(), f'{tuple(volume.shape)}'):
        st = _lib.load().ia_volume_keep(_p(volume), _p(labels), volume.numel(), _p(keep_flags), keep_flags.numel() - 1, float(fill),
                                        _p(out), _lib.stream_ptr(dev))
    _lib.check(st, 'ia_volume_keep')
    return out


def mesh_components(faces, n_verts):
    """Components of a mesh's vertices (see ia_mesh_components): faces int32 [F,3], V -> (vert_labels int32 [V], K).  One host
    synchronisation (K)."""
    _i32c(faces, 'faces')
    if faces.dim() != 2 or faces.shape[1] != 3:
        raise RuntimeError(f'faces must be [F,3], got {tuple(faces.shape)}')
    v, f = int(n_verts), faces.shape[0]
    lib, dev = _lib.load(), faces.device
    scratch, nbytes = _scratch('ia_mesh_components_scratch_bytes', v, dtype=torch.int32, device=dev)
    labels = torch.empty(v, dtype=torch.int32, device=dev)
    count = torch.empty(1, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        with _Timed('mesh_components', 0.0, 12.0 * f + 32.0 * v, f'F={f} V={v}'):
            st = lib.ia_mesh_components(_p(faces), f, v, _p(labels), _p(scratch), nbytes, _p(count), _lib.stream_ptr(dev))
        _lib.check(st, 'ia_mesh_components')
        return labels, int(count.cpu())


def mesh_component_stats(faces, vert_labels, k):
    """int32 [K,3] = vertex count, face count, smallest vertex index per component (see ia_mesh_component_stats)."""
    _i32c(faces, 'faces')
    _i32c(vert_labels, 'vert_labels')
    dev = faces.device
    stats = torch.empty(max(int(k), 0), 3, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev), _Timed('mesh_component_stats', 0.0, 4.0 * (faces.numel() + vert_labels.numel()), f'K={k}'):
        st = _lib.load().ia_mesh_component_stats(_p(faces), faces.shape[0], vert_labels.numel(), _p(vert_labels), int(k), _p(stats),
                                                 _lib.stream_ptr(dev))
    _lib.check(st, 'ia_mesh_component_stats')
    return stats


IMAGE_LAYOUT_F32_NCHW, IMAGE_LAYOUT_U8_NHWC = 0, 1


def image_metrics(a, b, data_range, levels=5):
    """Per-frame mse, l1, psnr, ssim, ms_ssim, ssim_0.., cs_0.. of two image batches (see ia_image_metrics): float32 [N,C,H,W] or
    uint8 [N,H,W,C] contiguous device tensors of the same shape -> float32 [N, 5 + 2 * levels].  `levels` + 1 launches, no atomics."""
    if not (a.is_cuda and b.is_cuda and a.device == b.device and a.is_contiguous() and b.is_contiguous()):
        raise RuntimeError('image_metrics: a and b must be contiguous tensors on the same device')
    if a.dtype != b.dtype or a.dtype not in (torch.float32, torch.uint8) or a.shape != b.shape or a.dim() != 4:
        raise RuntimeError(f'image_metrics: float32 [N,C,H,W] or uint8 [N,H,W,C] pairs, got {a.dtype} {tuple(a.shape)} and {b.dtype} {tuple(b.shape)}')
    if a.dtype == torch.uint8:
        layout, (n, h, w, c) = IMAGE_LAYOUT_U8_NHWC, a.shape
    else:
        layout, (n, c, h, w) = IMAGE_LAYOUT_F32_NCHW, a.shape
    lib, dev = _lib.load(), a.device
    scratch, nbytes = _scratch('ia_image_metrics_scratch_bytes', n, c, h, w, int(levels), dtype=torch.float64, device=dev)
    out = torch.empty(n, 5 + 2 * int(levels), device=dev)
    pixels = float(a.numel())
    with torch.cuda.device(dev), _Timed('image_metrics', 400.0 * pixels, 2.0 * a.element_size() * pixels * (1.0 + 1.0 / 3.0 if levels > 1 else 1.0),
                                        f'{n}x{c}x{h}x{w} levels={levels}'):
        st = lib.ia_image_metrics(_p(a), _p(b), layout, n, c, h, w, float(data_range), int(levels), _p(scratch), nbytes,
                                  _p(out), _lib.stream_ptr(dev))
    _lib.check(st, 'ia_image_metrics')
    return out


# ------------------------------------------------------------------ surface distance (csrc/surface_distance.hip)

def tri_pack(verts, faces):
    """Packed triangles (see ia_tri_pack): verts float32 [V,3], faces int32 [F,3] -> float32 [F,3,4]."""
    _mesh_checked(verts, faces)
    dev = verts.device
    tris = torch.empty(faces.shape[0], 3, 4, device=dev)
    with torch.cuda.device(dev), _Timed('tri_pack', 0.0, 84.0 * faces.shape[0], f'F={faces.shape[0]}'):
        st = _lib.load().ia_tri_pack(_p(verts), verts.shape[0], _p(faces), faces.shape[0], _p(tris), _lib.stream_ptr(dev))
    _lib.check(st, 'ia_tri_pack')
    return tris


def trigrid_plan(n_faces, lo, hi, cells=None):
    """Grid dimensions and inverse cell sizes for a mesh of ``n_faces`` triangles in the box [lo, hi] (host arithmetic, see
    ia_trigrid_plan).  ``cells``: None, an int or a triple fixes the cells per axis."""
    req = (0, 0, 0) if cells is None else ((int(cells),) * 3 if isinstance(cells, int) else tuple(int(c) for c in cells))
    if len(req) != 3 or (cells is not None and min(req) < 1):
        raise ValueError(f'cells must be None, an int >= 1 or three of them, got {cells!r}')
    dims, inv = (ctypes.c_int * 3)(), (ctypes.c_float * 3)()
    _lib.check(_lib.load().ia_trigrid_plan(int(n_faces), _f3(lo), _f3(hi), _i3(req), dims, inv), 'ia_trigrid_plan')
    return tuple(dims), tuple(inv)


def trigrid_build(tris, lo, inv_cell, dims):
    """The CSR cell lists of packed triangles (see ia_trigrid_count / ia_trigrid_fill): -> (cell_start int32 [ncell + 2], cell_tris
    int32 [entries + n_over], entries, n_over).  One host synchronisation (the two totals)."""
    _f32c(tris, 'tris')
    f = tris.shape[0]
    dev = tris.device
    ncell = int(dims[0]) * int(dims[1]) * int(dims[2])
    lib = _lib.load()
    clo, cinv, cdims = _f3(lo), _f3(inv_cell), _i3(dims)
    cell_start = torch.empty(ncell + 2, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        with _Timed('trigrid_count', 0.0, 48.0 * f + 8.0 * ncell, f'F={f} cells={tuple(dims)}'):
            st = lib.ia_trigrid_count(_p(tris), f, clo, cinv, cdims, _p(cell_start), _lib.stream_ptr(dev))
        _lib.check(st, 'ia_trigrid_count')
        entries, n_over = (int(v) for v in cell_start[ncell:].cpu())
        cell_tris = torch.empty(max(entries + n_over, 1), dtype=torch.int32, device=dev)
        scratch = torch.empty(ncell + 1, dtype=torch.int32, device=dev)
        with _Timed('trigrid_fill', 0.0, 48.0 * f + 8.0 * ncell + 4.0 * entries, f'F={f} entries={entries} oversize={n_over}'):
            st = lib.ia_trigrid_fill(_p(tris), f, clo, cinv, cdims, _p(cell_start), entries, n_over, _p(scratch), scratch.numel() * 4,
                                     _p(cell_tris), _lib.stream_ptr(dev))
        _lib.check(st, 'ia_trigrid_fill')
    return cell_start, cell_tris, entries, n_over


def closest_point(points, tris, mesh_extent, grid=None):
    """Closest triangle per point (see ia_closest_point): points float32 [N,3], tris from ``tri_pack`` -> (dist [N], face int32 [N],
    point [N,3]).  ``grid``: (lo, inv_cell, dims, cell_start, cell_tris, entries, n_over), or None for the brute mode."""
    _f32c(points, 'points')
    _f32c(tris, 'tris')
    if points.dim() != 2 or points.shape[1] != 3 or points.device != tris.device:
        raise RuntimeError(f'points must be [N,3] on the device of the triangles, got {tuple(points.shape)} on {points.device}')
    n, f, dev = points.shape[0], tris.shape[0], points.device
    dist = torch.empty(n, device=dev)
    face = torch.empty(n, dtype=torch.int32, device=dev)
    point = torch.empty(n, 3, device=dev)
    lib = _lib.load()
    with torch.cuda.device(dev), _Timed('closest_point', 0.0, 32.0 * n, f'N={n} F={f} {"brute" if grid is None else tuple(grid[2])}'):
        if grid is None:
            st = lib.ia_closest_point(_p(points), n, _p(tris), f, float(mesh_extent), None, None, None, None, None, 0, 0, _p(dist), _p(face),
                                      _p(point), _lib.stream_ptr(dev))
        else:
            lo, inv, dims, cell_start, cell_tris, entries, n_over = grid
            st = lib.ia_closest_point(_p(points), n, _p(tris), f, float(mesh_extent), _f3(lo), _f3(inv), _i3(dims), _p(cell_start),
                                      _p(cell_tris), int(entries), int(n_over), _p(dist), _p(face), _p(point), _lib.stream_ptr(dev))
    _lib.check(st, 'ia_closest_point')
    return dist, face, point


def distance_stats(dist, thresholds=(), face=None, normals_a=None, normals_b=None):
    """Reductions of a distance array (see ia_distance_stats): float64 device tensor [14] = finite count, sum, sum of squares, max,
    sum |n_a . n_b|, non-finite count, counts <= thresholds[k]."""
    _f32c(dist, 'dist')
    thresholds = [float(t) for t in thresholds]
    if len(thresholds) > 8:
        raise ValueError(f'at most 8 thresholds per call, got {len(thresholds)}')
    n, dev = dist.numel(), dist.device
    with_normals = face is not None
    if with_normals:
        _i32c(face, 'face')
        _f32c(normals_a, 'normals_a')
        _f32c(normals_b, 'normals_b')
        if face.numel() != n or tuple(normals_a.shape) != (n, 3) or normals_b.dim() != 2 or normals_b.shape[1] != 3:
            raise RuntimeError('face [N], normals_a [N,3] and normals_b [Fb,3] do not match the distances')
    lib = _lib.load()
    scratch, nbytes = _scratch('ia_distance_stats_scratch_bytes', n, dtype=torch.float64, device=dev)
    out = torch.empty(14, dtype=torch.float64, device=dev)
    thr = (ctypes.c_float * max(len(thresholds), 1))(*thresholds)
    with torch.cuda.device(dev), _Timed('distance_stats', 0.0, (32.0 if with_normals else 4.0) * n, f'N={n}'):
        st = lib.ia_distance_stats(_p(dist), n, thr, len(thresholds), _p(face), _p(normals_a), _p(normals_b),
                                   normals_b.shape[0] if with_normals else 0, _p(scratch), nbytes, _p(out), _lib.stream_ptr(dev))
    _lib.check(st, 'ia_distance_stats')
    return out


# ------------------------------------------------------------------ alignment (csrc/align.hip)

def transform_points(points, matrix):
    """``fp32(M) x`` per point (see ia_transform_points): points float32 [N,3], matrix 4x4 (or 3x4) of floats on the host -> [N,3]."""
    _f32c(points, 'points')
    if points.dim() != 2 or points.shape[1] != 3:
        raise RuntimeError(f'points must be [N,3], got {tuple(points.shape)}')
    m12 = (ctypes.c_double * 12)(*[float(matrix[r][c]) for r in range(3) for c in range(4)])
    n, dev = points.shape[0], points.device
    out = torch.empty_like(points)
    with torch.cuda.device(dev), _Timed('transform_points', 18.0 * n, 24.0 * n, f'N={n}'):
        st = _lib.load().ia_transform_points(_p(points), n, m12, _p(out), _lib.stream_ptr(dev))
    _lib.check(st, 'ia_transform_points')
    return out


ALIGN_MODES = {'point': 0, 'plane': 1}


def align_sums(src, dst, dist, face, centre, max_dist=float('inf'), metric='point', face_normals=None):
    """The sums of one alignment iteration (see ia_align_sums): src, dst float32 [N,3], dist float32 [N], face int32 [N], centre three
    floats, face_normals float32 [Fb,3] for ``metric='plane'`` -> float64 device tensor [20] (point) or [56] (plane)."""
    if metric not in ALIGN_MODES:
        raise ValueError(f"metric must be 'point' or 'plane', got {metric!r}")
    mode = ALIGN_MODES[metric]
    for t, what in ((src, 'src'), (dst, 'dst'), (dist, 'dist')):
        _f32c(t, what)
    _i32c(face, 'face')
    n, dev = dist.numel(), dist.device
    if tuple(src.shape) != (n, 3) or tuple(dst.shape) != (n, 3) or face.numel() != n or not (src.device == dst.device == face.device == dev):
        raise RuntimeError('src [N,3], dst [N,3], dist [N] and face [N] must match and share a device')
    fb = 0
    if mode:
        _f32c(face_normals, 'face_normals')
        if face_normals.dim() != 2 or face_normals.shape[1] != 3 or face_normals.device != dev:
            raise RuntimeError(f'face_normals must be [Fb,3] on the device of the points, got {tuple(face_normals.shape)}')
        fb = face_normals.shape[0]
    scratch, nbytes = _scratch('ia_align_sums_scratch_bytes', n, mode, dtype=torch.float64, device=dev)
    out = torch.empty(56 if mode else 20, dtype=torch.float64, device=dev)
    with torch.cuda.device(dev), _Timed('align_sums', 0.0, (32.0 + 12.0 * mode) * n, f'N={n} {metric}'):
        st = _lib.load().ia_align_sums(_p(src), _p(dst), _p(dist), _p(face), n, _p(face_normals) if mode else None, fb, _d3(centre),
                                       float(max_dist), mode, _p(scratch), nbytes, _p(out), _lib.stream_ptr(dev))
    _lib.check(st, 'ia_align_sums')
    return out


# ------------------------------------------------------------------ pose search (csrc/pose_search.hip)

POSE_MAX_POINTS = 4096       # csrc/pose_search.hip kMaxPoints
POSE_SLAB = 1 << 16          # candidate rotations per launch; a score does not depend on the cut


def pose_scores(points, dist, origin, spacing, rotations, c_src, c_tgt, shifts=1, shift_step=None, scale=1.0, cap=float('inf')):
    """The score of every candidate pose (see ia_pose_scores): points float32 [n,3] (n <= 4096), dist float32 [nx,ny,nz] the distance
    lattice with ``origin`` (three floats) and ``spacing`` (one float), rotations float32 [R,9], ``c_src`` / ``c_tgt`` three floats on
    the host -> float64 device tensor [R, shifts^3].  R is cut into slabs of POSE_SLAB; n = 0 gives NaN (a mean over nothing) and
    R = 0 an empty tensor, both without a launch."""
    _f32c(points, 'points')
    _f32c(rotations, 'rotations')
    nx, ny, nz = _volume_checked(dist)
    if points.dim() != 2 or points.shape[1] != 3:
        raise RuntimeError(f'points must be [n,3], got {tuple(points.shape)}')
    if rotations.dim() != 2 or rotations.shape[1] != 9 or not (rotations.device == dist.device == points.device):
        raise RuntimeError(f'rotations must be [R,9] on the device of the points and the lattice, got {tuple(rotations.shape)}')
    shifts = int(shifts)
    n, r, dev = points.shape[0], rotations.shape[0], points.device
    if n > POSE_MAX_POINTS:
        raise ValueError(f'pose_scores takes at most {POSE_MAX_POINTS} points, got {n}: score a subset (samples=)')
    if shifts < 1 or shifts % 2 == 0:
        raise ValueError(f'shifts must be odd and >= 1, got {shifts}')
    s3 = shifts ** 3
    step = float(spacing) if shift_step is None else float(shift_step)
    if n == 0 or r == 0:
        return torch.full((r, s3), float('nan'), dtype=torch.float64, device=dev)
    out = torch.empty(r, s3, dtype=torch.float64, device=dev)
    org = (ctypes.c_float * 3)(*[float(v) for v in origin])
    lib = _lib.load()
    for r0 in range(0, r, POSE_SLAB):
        rows = min(POSE_SLAB, r - r0)
        lookups = float(rows) * s3 * n
        with torch.cuda.device(dev), _Timed('pose_scores', 40.0 * lookups, 32.0 * lookups, f'R={rows} n={n} shifts={shifts}'):
            st = lib.ia_pose_scores(_p(points), n, _p(dist), nx, ny, nz, org, float(spacing), _p(rotations[r0:r0 + rows]), rows, _d3(c_src),
                                    _d3(c_tgt), shifts, step, float(scale), float(cap), _p(out[r0:r0 + rows]), _lib.stream_ptr(dev))
        _lib.check(st, 'ia_pose_scores')
    return out


# ------------------------------------------------------------------ non-rigid fitting (csrc/nonrigid.hip)

def _f64c(t, what, shape):
    if t is not None and not (t.is_cuda and t.dtype == torch.float64 and t.is_contiguous() and tuple(t.shape) == tuple(shape)):
        raise RuntimeError(f'{what} must be a contiguous float64 device tensor {tuple(shape)}')
    return t


def _pinned_checked(pinned, v):
    if not (pinned.is_cuda and pinned.dtype == torch.bool and pinned.is_contiguous() and tuple(pinned.shape) == (v,)):
        raise RuntimeError(f'pinned must be a contiguous bool device tensor [{v}]')
    return pinned


def nonrigid_terms(x, p, q, dist, face, pinned, max_dist=float('inf'), metric='point', face_normals=None, source_normals=None,
                   normal_cos=None, point_share=0.1, beta=None, land=None):
    """The terms of one pairing of the non-rigid fit (see ia_nonrigid_terms): x, p, q float32 [V,3], dist float32 [V], face int32 [V],
    pinned bool [V], face_normals float32 [Fb,3] (plane metric, normal_cos), source_normals float32 [V,3] (normal_cos), beta float64
    [V] and land float64 [V,3] (landmarks, or None) -> ``(c [V], n [V,3], b [V,3], stats [2])``, float64 device tensors; stats =
    (sum c |p - q|^2, sum c).  No host synchronisation."""
    if metric not in ALIGN_MODES:
        raise ValueError(f"metric must be 'point' or 'plane', got {metric!r}")
    mode, use_cos = ALIGN_MODES[metric], normal_cos is not None
    v, dev = dist.numel(), dist.device
    for t, what in ((x, 'x'), (p, 'p'), (q, 'q')):
        if tuple(_f32c(t, what).shape) != (v, 3) or t.device != dev:
            raise RuntimeError(f'{what} must be [V,3] on the device of dist, got {tuple(t.shape)}')
    _f32c(dist, 'dist')
    if _i32c(face, 'face').numel() != v:
        raise RuntimeError('face must be [V]')
    _pinned_checked(pinned, v)
    fb = 0
    if mode or use_cos:
        _f32c(face_normals, 'face_normals')
        if face_normals.dim() != 2 or face_normals.shape[1] != 3 or face_normals.device != dev:
            raise RuntimeError(f'face_normals must be [Fb,3] on the device of the points, got {tuple(face_normals.shape)}')
        fb = face_normals.shape[0]
    if use_cos and tuple(_f32c(source_normals, 'source_normals').shape) != (v, 3):
        raise RuntimeError('source_normals must be [V,3]')
    _f64c(beta, 'beta', (v,))
    if beta is not None:
        _f64c(land, 'land', (v, 3))
    f64 = dict(dtype=torch.float64, device=dev)
    c, n, b, out = torch.empty(v, **f64), torch.empty(v, 3, **f64), torch.empty(v, 3, **f64), torch.empty(2, **f64)
    scratch, nbytes = _scratch('ia_nonrigid_terms_scratch_bytes', v, dtype=torch.float64, device=dev)
    with torch.cuda.device(dev), _Timed('nonrigid_terms', 0.0, (61.0 + 56.0) * v, f'V={v} {metric}'):
        st = _lib.load().ia_nonrigid_terms(_p(x), _p(p), _p(q), _p(dist), _p(face), v, _p(face_normals) if fb else None, fb,
                                           _p(source_normals) if use_cos else None, float(max_dist), mode, int(use_cos),
                                           float(normal_cos) if use_cos else 0.0, float(point_share), _p(pinned), _p(beta),
                                           _p(land) if beta is not None else None, _p(c), _p(n), _p(b), _p(scratch), nbytes, _p(out),
                                           _lib.stream_ptr(dev))
    _lib.check(st, 'ia_nonrigid_terms')
    return c, n, b, out


def nonrigid_rhs(weight, target_offset, pinned, normals=None, point_share=0.1, beta=None, land=None):
    """float64 [V,3]: the right-hand side ``C t + B l`` of the non-rigid system from given weights and offsets (ia_nonrigid_rhs)."""
    v, dev = weight.numel(), weight.device
    _f64c(weight, 'weight', (v,))
    _f64c(target_offset, 'target_offset', (v, 3))
    _f64c(normals, 'normals', (v, 3))
    _f64c(beta, 'beta', (v,))
    if beta is not None:
        _f64c(land, 'land', (v, 3))
    _pinned_checked(pinned, v)
    b = torch.empty(v, 3, dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        st = _lib.load().ia_nonrigid_rhs(v, _p(weight), _p(target_offset), _p(normals), float(point_share), _p(beta),
                                         _p(land) if beta is not None else None, _p(pinned), _p(b), _lib.stream_ptr(dev))
    _lib.check(st, 'ia_nonrigid_rhs')
    return b


NONRIGID_LAUNCHES = 3        # launches per conjugate-gradient step (apply, update, direction); one more with heavy vertices


def nonrigid_step_bytes(v, e):
    """Algorithmic bytes one conjugate-gradient step moves: apply reads a 24-byte row and a 4-byte index per CSR entry, its own row,
    offset, weight and pin (37) and writes 24; update reads four rows and writes two (144); direction reads two and writes one (72)."""
    return 28.0 * e + (37.0 + 24.0 + 144.0 + 72.0) * v


def nonrigid_solve(s, weight, b, stiffness, pinned, normals=None, point_share=0.1, beta=None, x0=None, cg_iterations=100, cg_tol=1e-6):
    """Conjugate gradients on ``(C + a L + B) x = b`` over the ``mesh_adjacency`` state ``s`` (see ia_nonrigid_solve): weight float64
    [V], b float64 [V,3], pinned bool [V], normals float64 [V,3] (plane metric) or None, beta float64 [V] or None, x0 float64 [V,3] or
    None (zero) -> ``(x [V,3], out [5])``, float64 device tensors; out = (energy at the start, at the end, steps taken, |r| / |b|,
    frozen).  ``x0`` is not written.  Every launch goes to the current stream; there is no host synchronisation."""
    v, dev = s['V'], weight.device
    _f64c(weight, 'weight', (v,))
    _f64c(b, 'b', (v, 3))
    _f64c(normals, 'normals', (v, 3))
    _f64c(beta, 'beta', (v,))
    _pinned_checked(pinned, v)
    if int(cg_iterations) < 1:
        raise ValueError(f'cg_iterations must be >= 1, got {cg_iterations}')
    f64 = dict(dtype=torch.float64, device=dev)
    if x0 is None:
        x = torch.zeros(v, 3, **f64)
    else:
        x = torch.where(pinned[:, None], torch.zeros((), **f64), _f64c(x0, 'x0', (v, 3))).contiguous()
    out = torch.empty(5, **f64)
    scratch, nbytes = _scratch('ia_nonrigid_solve_scratch_bytes', v, dtype=torch.float64, device=dev)
    e = s['E']
    step_bytes = nonrigid_step_bytes(v, e)
    with torch.cuda.device(dev), _Timed('nonrigid_solve', 0.0, step_bytes * int(cg_iterations), f'V={v} E={e} steps={int(cg_iterations)}'):
        st = _lib.load().ia_nonrigid_solve(v, _p(s['offsets']), _p(s['neighbors']) if e else None, e, _p(s['heavy']) if s['n_heavy'] else None,
                                           s['n_heavy'], _p(weight), _p(normals), _p(beta), _p(pinned), _p(b), float(stiffness),
                                           float(point_share), _p(x), int(cg_iterations), float(cg_tol), _p(scratch), nbytes, _p(out),
                                           _lib.stream_ptr(dev))
    _lib.check(st, 'ia_nonrigid_solve')
    return x, out


def nonrigid_apply(x, d, pinned):
    """float32 [V,3]: ``fl32(x + d)``, the input bits where a vertex is pinned or a displacement is 0 (ia_nonrigid_apply)."""
    v, dev = x.shape[0], x.device
    _f32c(x, 'x')
    _f64c(d, 'd', (v, 3))
    _pinned_checked(pinned, v)
    out = torch.empty_like(x)
    with torch.cuda.device(dev), _Timed('nonrigid_apply', 0.0, 49.0 * v, f'V={v}'):
        st = _lib.load().ia_nonrigid_apply(_p(x), _p(d), _p(pinned), v, _p(out), _lib.stream_ptr(dev))
    _lib.check(st, 'ia_nonrigid_apply')
    return out


# ------------------------------------------------------------------ winding number (csrc/winding.hip)

WINDING_TILE = 256           # triangles per LDS tile (csrc/winding.hip kTile)
WINDING_CHUNK = 2048         # faces per partial sum (kChunk): part of the results, geometry._winding_numpy uses the same
WINDING_POINTS = 512         # points per workgroup (kPoints)
WINDING_WORKSPACE = 256 << 20


def winding_layout():
    """(tile, chunk, points per workgroup) as the library reports them (ia_winding_layout; host only)."""
    vals = [ctypes.c_int(0) for _ in range(3)]
    _lib.check(_lib.load().ia_winding_layout(*[ctypes.byref(v) for v in vals]), 'ia_winding_layout')
    return tuple(v.value for v in vals)


def winding_number(points, tris, workspace_bytes=WINDING_WORKSPACE):
    """Generalised winding number per point (see ia_winding_number): points float32 [N,3], tris from ``tri_pack`` -> float64 [N].  The
    partial sums take 8 N ceil(F / WINDING_CHUNK) bytes; the points are cut into slabs so that one call's workspace stays within
    ``workspace_bytes`` (at least one point per slab).  A point's result does not depend on the slab it is in."""
    _f32c(points, 'points')
    _f32c(tris, 'tris')
    if points.dim() != 2 or points.shape[1] != 3 or points.device != tris.device:
        raise RuntimeError(f'points must be [N,3] on the device of the triangles, got {tuple(points.shape)} on {points.device}')
    if tris.dim() != 3 or tuple(tris.shape[1:]) != (3, 4):
        raise RuntimeError(f'tris must be the [F,3,4] tensor of tri_pack, got {tuple(tris.shape)}')
    n, f, dev = points.shape[0], tris.shape[0], points.device
    chunks = -(-f // WINDING_CHUNK)
    slab = n if chunks == 0 else max(1, min(n, int(workspace_bytes) // (8 * chunks)))
    out = torch.empty(n, dtype=torch.float64, device=dev)
    lib = _lib.load()
    scratch = torch.empty(max(slab * chunks, 1), dtype=torch.float64, device=dev)
    with torch.cuda.device(dev), _Timed('winding_number', 75.0 * n * f, 48.0 * f * -(-n // WINDING_POINTS) + 16.0 * n * chunks,
                                        f'N={n} F={f} slab={slab}'):
        for s in range(0, n, max(slab, 1)):
            m = min(slab, n - s)
            st = lib.ia_winding_number(_p(points[s:s + m]), m, _p(tris), f, _p(scratch), scratch.numel() * 8, _p(out[s:s + m]),
                                       _lib.stream_ptr(dev))
            _lib.check(st, 'ia_winding_number')
    return out


# ------------------------------------------------------------------ winding tree (csrc/winding_tree.hip)

WINDING_LEAF = 32            # faces per leaf (csrc/winding_tree.hip kLeaf): part of the results, geometry restates the tree with the same
WINDING_BRANCH = 8           # children per upper node (kBranch): part of the results
WINDING_ROW = 20             # floats per node row (5 float4)
WINDING_MAX_LEVELS = 8
WINDING_NO_KEY = 1 << 30     # Morton key of an unusable triangle or a non-finite point


def winding_tree_layout():
    """(leaf, branch, floats per node row, most levels) as the library reports them (ia_winding_tree_layout; host only)."""
    vals = [ctypes.c_int(0) for _ in range(4)]
    _lib.check(_lib.load().ia_winding_tree_layout(*[ctypes.byref(v) for v in vals]), 'ia_winding_tree_layout')
    return tuple(v.value for v in vals)


def winding_tree_plan(n_usable):
    """(nodes per level, leaves first; total nodes; scratch bytes of the build) for ``n_usable`` faces (ia_winding_tree_plan; host only)."""
    levels, nodes, nbytes = ctypes.c_int(0), ctypes.c_int64(0), ctypes.c_size_t(0)
    counts = (ctypes.c_int * WINDING_MAX_LEVELS)()
    st = _lib.load().ia_winding_tree_plan(int(n_usable), ctypes.byref(levels), counts, ctypes.byref(nodes), ctypes.byref(nbytes))
    _lib.check(st, 'ia_winding_tree_plan')
    return list(counts[:levels.value]), nodes.value, nbytes.value


def _tris_checked(tris):
    _f32c(tris, 'tris')
    if tris.dim() != 3 or tuple(tris.shape[1:]) != (3, 4):
        raise RuntimeError(f'tris must be the [F,3,4] tensor of tri_pack, got {tuple(tris.shape)}')


def winding_tree_point_keys(points, lo, scale):
    """Morton keys int32 [N] of points float32 [N,3] over the cube (lo, scale) (see ia_winding_tree_point_keys)."""
    _f32c(points, 'points')
    if points.dim() != 2 or points.shape[1] != 3:
        raise RuntimeError(f'points must be [N,3], got {tuple(points.shape)}')
    n, dev = points.shape[0], points.device
    keys = torch.empty(n, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev), _Timed('winding_tree_keys', 0.0, 16.0 * n, f'N={n}'):
        st = _lib.load().ia_winding_tree_point_keys(_p(points), n, _f3(lo), float(scale), _p(keys), _lib.stream_ptr(dev))
    _lib.check(st, 'ia_winding_tree_point_keys')
    return keys


def winding_tree_build(tris, lo, scale):
    """The cluster tree of packed triangles (see ia_winding_tree_nodes): tris from ``tri_pack``, (lo, scale) the Morton cube ->
    (order int64 [F]: sorted position -> input face, sorted tris [F,3,4], nodes float32 [n,20], nodes per level, usable faces).  The
    integer keys are sorted by ``torch.sort`` (stable); one host synchronisation (the number of usable faces)."""
    _tris_checked(tris)
    f, dev = tris.shape[0], tris.device
    lib = _lib.load()
    keys = torch.empty(f, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        with _Timed('winding_tree_keys', 0.0, 52.0 * f, f'F={f}'):
            st = lib.ia_winding_tree_face_keys(_p(tris), f, _f3(lo), float(scale), _p(keys), _lib.stream_ptr(dev))
        _lib.check(st, 'ia_winding_tree_face_keys')
        skeys, order = torch.sort(keys, stable=True)
        usable = int((skeys < WINDING_NO_KEY).sum()) if f else 0
        order32 = order.int().contiguous()
        sorted_tris = torch.empty_like(tris)
        with _Timed('winding_tree_gather', 0.0, 100.0 * f, f'F={f}'):
            st = lib.ia_winding_tree_gather(_p(tris), f, _p(order32), _p(sorted_tris), _lib.stream_ptr(dev))
        _lib.check(st, 'ia_winding_tree_gather')
        counts, total, nbytes = winding_tree_plan(usable)
        nodes = torch.empty(total, WINDING_ROW, device=dev)
        scratch = torch.empty(max(nbytes // 8, 1), dtype=torch.float64, device=dev)
        with _Timed('winding_tree_nodes', 0.0, 96.0 * usable + 240.0 * total, f'F={usable} nodes={total}'):
            st = lib.ia_winding_tree_nodes(_p(sorted_tris), usable, _p(scratch), scratch.numel() * 8, _p(nodes), total, _lib.stream_ptr(dev))
        _lib.check(st, 'ia_winding_tree_nodes')
    return order, sorted_tris, nodes, counts, usable


def winding_tree_query(points, sorted_tris, nodes, n_usable, beta=2.0, bound=False, counts=False):
    """Winding numbers through the tree (see ia_winding_tree_query): points float32 [N,3], ``sorted_tris`` / ``nodes`` / ``n_usable``
    from ``winding_tree_build`` -> (w float64 [N], bound float64 [N] or None, counts int32 [N,2] or None)."""
    _f32c(points, 'points')
    _tris_checked(sorted_tris)
    _f32c(nodes, 'nodes')
    if points.dim() != 2 or points.shape[1] != 3 or points.device != sorted_tris.device or nodes.device != points.device:
        raise RuntimeError(f'points must be [N,3] on the device of the tree, got {tuple(points.shape)} on {points.device}')
    if nodes.dim() != 2 or nodes.shape[1] != WINDING_ROW or not 0 <= int(n_usable) <= sorted_tris.shape[0]:
        raise RuntimeError(f'nodes must be [n,{WINDING_ROW}] and n_usable within the triangles, got {tuple(nodes.shape)} and {n_usable}')
    n, dev = points.shape[0], points.device
    out = torch.empty(n, dtype=torch.float64, device=dev)
    bnd = torch.empty(n, dtype=torch.float64, device=dev) if bound else None
    cnt = torch.empty(n, 2, dtype=torch.int32, device=dev) if counts else None
    with torch.cuda.device(dev), _Timed('winding_tree_query', 0.0, 36.0 * n, f'N={n} F={int(n_usable)} beta={beta}'):
        st = _lib.load().ia_winding_tree_query(_p(points), n, _p(sorted_tris), int(n_usable), _p(nodes), nodes.shape[0], float(beta), _p(out),
                                               _p(bnd), _p(cnt), _lib.stream_ptr(dev))
    _lib.check(st, 'ia_winding_tree_query')
    return out, bnd, cnt


# ------------------------------------------------------------------ closest point on the tree (csrc/closest_tree.hip)

TREE_BOX_ROW = 8             # floats per box row: (lo.xyz, 0) (hi.xyz, 0)


def tree_boxes(sorted_tris, n_usable, n_nodes):
    """Bounding boxes float32 [n_nodes, 8] of the nodes of the tree over ``sorted_tris`` (see ia_tree_boxes)."""
    _tris_checked(sorted_tris)
    if not 0 <= int(n_usable) <= sorted_tris.shape[0]:
        raise RuntimeError(f'n_usable must be within the {sorted_tris.shape[0]} triangles, got {n_usable}')
    dev = sorted_tris.device
    boxes = torch.empty(int(n_nodes), TREE_BOX_ROW, device=dev)
    with torch.cuda.device(dev), _Timed('tree_boxes', 0.0, 48.0 * int(n_usable) + 64.0 * int(n_nodes), f'F={int(n_usable)} nodes={int(n_nodes)}'):
        st = _lib.load().ia_tree_boxes(_p(sorted_tris), int(n_usable), _p(boxes), int(n_nodes), _lib.stream_ptr(dev))
    _lib.check(st, 'ia_tree_boxes')
    return boxes


def closest_point_tree(points, sorted_tris, order, boxes, n_usable, mesh_extent, counts=False):
    """Closest triangle per point through the tree (see ia_closest_point_tree): points float32 [N,3], ``sorted_tris`` / ``n_usable``
    from ``winding_tree_build``, ``order`` int32 (sorted position -> input face), ``boxes`` from ``tree_boxes`` -> (dist [N], face
    int32 [N]: input face indices, point [N,3], counts int32 [N,2] or None)."""
    _f32c(points, 'points')
    _tris_checked(sorted_tris)
    _i32c(order, 'order')
    _f32c(boxes, 'boxes')
    dev = points.device
    if points.dim() != 2 or points.shape[1] != 3 or any(t.device != dev for t in (sorted_tris, order, boxes)):
        raise RuntimeError(f'points must be [N,3] on the device of the tree, got {tuple(points.shape)} on {dev}')
    if boxes.dim() != 2 or boxes.shape[1] != TREE_BOX_ROW or not 0 <= int(n_usable) <= min(sorted_tris.shape[0], order.numel()):
        raise RuntimeError(f'boxes must be [n,{TREE_BOX_ROW}] and n_usable within the triangles and the order, got {tuple(boxes.shape)} and '
                           f'{n_usable}')
    n = points.shape[0]
    dist = torch.empty(n, device=dev)
    face = torch.empty(n, dtype=torch.int32, device=dev)
    point = torch.empty(n, 3, device=dev)
    cnt = torch.empty(n, 2, dtype=torch.int32, device=dev) if counts else None
    with torch.cuda.device(dev), _Timed('closest_point_tree', 0.0, 32.0 * n, f'N={n} F={int(n_usable)}'):
        st = _lib.load().ia_closest_point_tree(_p(points), n, _p(sorted_tris), _p(order), int(n_usable), _p(boxes), boxes.shape[0],
                                               float(mesh_extent), _p(dist), _p(face), _p(point), _p(cnt), _lib.stream_ptr(dev))
    _lib.check(st, 'ia_closest_point_tree')
    return dist, face, point, cnt


# ------------------------------------------------------------------ rays against the mesh on the tree (csrc/ray_tree.hip)

def _ray_args(origins, dirs, t_lo, t_hi, sorted_tris, order, n_usable):
    for x, name in ((origins, 'origins'), (dirs, 'dirs'), (t_lo, 't_lo'), (t_hi, 't_hi')):
        _f32c(x, name)
    _tris_checked(sorted_tris)
    _i32c(order, 'order')
    dev, n = origins.device, origins.shape[0]
    if origins.dim() != 2 or origins.shape[1] != 3 or tuple(dirs.shape) != (n, 3) or tuple(t_lo.shape) != (n,) or tuple(t_hi.shape) != (n,):
        raise RuntimeError(f'origins and dirs must be [N,3], t_lo and t_hi [N], got {tuple(origins.shape)}, {tuple(dirs.shape)}, '
                           f'{tuple(t_lo.shape)}, {tuple(t_hi.shape)}')
    if any(t.device != dev for t in (dirs, t_lo, t_hi, sorted_tris, order)):
        raise RuntimeError(f'the rays must be on the device of the tree, got {dev}')
    if not 0 <= int(n_usable) <= min(sorted_tris.shape[0], order.numel()):
        raise RuntimeError(f'n_usable must be within the triangles and the order, got {n_usable}')
    return dev, n


def _ray_outputs(n, dev, any_hit):
    hit = torch.empty(n, dtype=torch.uint8, device=dev)
    if any_hit:
        return hit, None, None, None, None
    return (hit, torch.empty(n, device=dev), torch.empty(n, dtype=torch.int32, device=dev), torch.empty(n, 3, device=dev),
            torch.empty(n, 3, device=dev))


def ray_mesh_brute(origins, dirs, t_lo, t_hi, sorted_tris, order, n_usable, any_hit=False):
    """Every ray against every usable triangle (see ia_ray_mesh_brute): origins, dirs float32 [N,3], t_lo, t_hi float32 [N],
    ``sorted_tris`` / ``n_usable`` from ``winding_tree_build``, ``order`` int32 -> (hit bool [N], t [N], face int32 [N]: input face
    indices, bary [N,3], point [N,3]); with ``any_hit`` everything but ``hit`` is None."""
    dev, n = _ray_args(origins, dirs, t_lo, t_hi, sorted_tris, order, n_usable)
    hit, t, face, bary, point = _ray_outputs(n, dev, any_hit)
    with torch.cuda.device(dev), _Timed('ray_mesh_brute', 0.0, 64.0 * n, f'N={n} F={int(n_usable)} any={int(any_hit)}'):
        st = _lib.load().ia_ray_mesh_brute(_p(origins), _p(dirs), _p(t_lo), _p(t_hi), n, _p(sorted_tris), _p(order), int(n_usable), int(any_hit),
                                           _p(hit), _p(t), _p(face), _p(bary), _p(point), _lib.stream_ptr(dev))
    _lib.check(st, 'ia_ray_mesh_brute')
    return hit.bool(), t, face, bary, point


def ray_mesh_tree(origins, dirs, t_lo, t_hi, sorted_tris, order, boxes, n_usable, mesh_extent, any_hit=False, counts=False):
    """The same through the tree (see ia_ray_mesh_tree): ``boxes`` from ``tree_boxes`` -> (hit, t, face, bary, point, counts int32
    [N,2] or None)."""
    dev, n = _ray_args(origins, dirs, t_lo, t_hi, sorted_tris, order, n_usable)
    _f32c(boxes, 'boxes')
    if boxes.dim() != 2 or boxes.shape[1] != TREE_BOX_ROW or boxes.device != dev:
        raise RuntimeError(f'boxes must be [n,{TREE_BOX_ROW}] on the device of the rays, got {tuple(boxes.shape)} on {boxes.device}')
    hit, t, face, bary, point = _ray_outputs(n, dev, any_hit)
    cnt = torch.empty(n, 2, dtype=torch.int32, device=dev) if counts else None
    with torch.cuda.device(dev), _Timed('ray_mesh_tree', 0.0, 64.0 * n, f'N={n} F={int(n_usable)} any={int(any_hit)}'):
        st = _lib.load().ia_ray_mesh_tree(_p(origins), _p(dirs), _p(t_lo), _p(t_hi), n, _p(sorted_tris), _p(order), int(n_usable), _p(boxes),
                                          boxes.shape[0], float(mesh_extent), int(any_hit), _p(hit), _p(t), _p(face), _p(bary), _p(point),
                                          _p(cnt), _lib.stream_ptr(dev))
    _lib.check(st, 'ia_ray_mesh_tree')
    return hit.bool(), t, face, bary, point, cnt


def ao_rays(verts, normals, table, bias):
    """The rays of the ambient-occlusion estimate (see ia_ao_rays): verts, normals float32 [V,3], table float32 [S,3] -> (origins,
    dirs) float32 [V S, 3], ray v S + s."""
    for x, name in ((verts, 'verts'), (normals, 'normals'), (table, 'table')):
        _f32c(x, name)
    dev, v, s = verts.device, verts.shape[0], table.shape[0]
    if verts.dim() != 2 or verts.shape[1] != 3 or tuple(normals.shape) != (v, 3) or table.dim() != 2 or table.shape[1] != 3:
        raise RuntimeError(f'verts and normals must be [V,3] and table [S,3], got {tuple(verts.shape)}, {tuple(normals.shape)}, {tuple(table.shape)}')
    if normals.device != dev or table.device != dev:
        raise RuntimeError(f'normals and table must be on the device of verts, got {normals.device} and {table.device}')
    origins, dirs = torch.empty(v * s, 3, device=dev), torch.empty(v * s, 3, device=dev)
    with torch.cuda.device(dev), _Timed('ao_rays', 0.0, 24.0 * v + 24.0 * v * s, f'V={v} S={s}'):
        st = _lib.load().ia_ao_rays(_p(verts), _p(normals), v, _p(table), s, float(bias), _p(origins), _p(dirs), _lib.stream_ptr(dev))
    _lib.check(st, 'ia_ao_rays')
    return origins, dirs


# ------------------------------------------------------------------ point clouds on the tree (csrc/point_tree.hip)

NEAREST_MAX_K = 32           # csrc/point_tree.hip kMaxK


def _cloud_checked(points, what='points'):
    _f32c(points, what)
    if points.dim() != 2 or points.shape[1] != 3:
        raise RuntimeError(f'{what} must be [N,3], got {tuple(points.shape)}')


def point_tree_build(points, lo, scale):
    """The cluster tree of a cloud (see ia_point_tree_gather): points float32 [n,3], (lo, scale) the Morton cube -> (order int64 [n]:
    sorted position -> input index, usable points first, sorted float32 [n_usable,4], boxes float32 [nodes,8], nodes per level,
    n_usable).  The keys are sorted by ``torch.sort`` (stable); one host synchronisation (the number of usable points)."""
    _cloud_checked(points)
    n, dev = points.shape[0], points.device
    lib = _lib.load()
    with torch.cuda.device(dev):
        keys = winding_tree_point_keys(points, lo, scale)
        skeys, order = torch.sort(keys, stable=True)
        usable = int((skeys < WINDING_NO_KEY).sum()) if n else 0
        order32 = order.int().contiguous()
        rows = torch.empty(usable, 4, device=dev)
        with _Timed('point_tree_gather', 0.0, 32.0 * usable, f'n={usable}'):
            st = lib.ia_point_tree_gather(_p(points), n, _p(order32), usable, _p(rows), _lib.stream_ptr(dev))
        _lib.check(st, 'ia_point_tree_gather')
        counts, total, _ = winding_tree_plan(usable)
        boxes = torch.empty(total, TREE_BOX_ROW, device=dev)
        with _Timed('point_tree_boxes', 0.0, 16.0 * usable + 64.0 * total, f'n={usable} nodes={total}'):
            st = lib.ia_point_tree_boxes(_p(rows), usable, _p(boxes), total, _lib.stream_ptr(dev))
        _lib.check(st, 'ia_point_tree_boxes')
    return order, rows, boxes, counts, usable


def nearest_points(queries, sorted_points, boxes=None, k=1, max_dist=float('inf'), exclude=None, counts=False):
    """The k nearest points of a cloud per query (see ia_nearest_points_tree; ``boxes=None``: ia_nearest_points_brute): queries float32
    [N,3], ``sorted_points`` / ``boxes`` from ``point_tree_build``, ``exclude`` int32 [N] or None -> (dist float32 [N,k], index int32
    [N,k], counts int32 [N,2] or None)."""
    _cloud_checked(queries, 'queries')
    _f32c(sorted_points, 'sorted_points')
    dev, n = queries.device, queries.shape[0]
    if sorted_points.dim() != 2 or sorted_points.shape[1] != 4 or sorted_points.device != dev:
        raise RuntimeError(f'sorted_points must be [n,4] on the device of the queries, got {tuple(sorted_points.shape)}')
    if boxes is not None:
        _f32c(boxes, 'boxes')
        if boxes.dim() != 2 or boxes.shape[1] != TREE_BOX_ROW or boxes.device != dev:
            raise RuntimeError(f'boxes must be [n,{TREE_BOX_ROW}] on the device of the queries, got {tuple(boxes.shape)}')
    elif counts:
        raise RuntimeError('counts are those of the walk: they need boxes')
    if exclude is not None:
        _i32c(exclude, 'exclude')
        if tuple(exclude.shape) != (n,) or exclude.device != dev:
            raise RuntimeError(f'exclude must be [N] on the device of the queries, got {tuple(exclude.shape)}')
    k = int(k)
    rows = max(min(k, NEAREST_MAX_K), 1)                 # (a k out of range is refused by the library; the buffers stay small)
    dist = torch.empty(n, rows, device=dev)
    index = torch.empty(n, rows, dtype=torch.int32, device=dev)
    cnt = torch.empty(n, 2, dtype=torch.int32, device=dev) if counts else None
    lib, m = _lib.load(), sorted_points.shape[0]
    with torch.cuda.device(dev), _Timed('nearest_points', 0.0, 12.0 * n + 8.0 * n * rows, f'N={n} n={m} k={k} {"brute" if boxes is None else "tree"}'):
        if boxes is None:
            st = lib.ia_nearest_points_brute(_p(queries), n, _p(sorted_points), m, k, float(max_dist), _p(exclude), _p(dist), _p(index),
                                             _lib.stream_ptr(dev))
        else:
            st = lib.ia_nearest_points_tree(_p(queries), n, _p(sorted_points), m, _p(boxes), boxes.shape[0], k, float(max_dist), _p(exclude),
                                            _p(dist), _p(index), _p(cnt), _lib.stream_ptr(dev))
    _lib.check(st, 'ia_nearest_points_brute' if boxes is None else 'ia_nearest_points_tree')
    return dist, index, cnt


def point_normals(points, index):
    """Normals of a cloud from its neighbour table (see ia_point_normals): points float32 [n,3], index int32 [n,k] -> (normal float32
    [n,3], variation float32 [n], eigenvalues float64 [n,3], covariance float64 [n,6])."""
    _cloud_checked(points)
    _i32c(index, 'index')
    n, dev = points.shape[0], points.device
    if index.dim() != 2 or index.shape[0] != n or index.device != dev:
        raise RuntimeError(f'index must be [n,k] on the device of the points, got {tuple(index.shape)}')
    normal, variation = torch.empty(n, 3, device=dev), torch.empty(n, device=dev)
    eig, cov = torch.empty(n, 3, dtype=torch.float64, device=dev), torch.empty(n, 6, dtype=torch.float64, device=dev)
    with torch.cuda.device(dev), _Timed('point_normals', 0.0, (88.0 + 16.0 * index.shape[1]) * n, f'n={n} k={index.shape[1]}'):
        st = _lib.load().ia_point_normals(_p(points), n, _p(index), index.shape[1], _p(normal), _p(variation), _p(eig), _p(cov),
                                          _lib.stream_ptr(dev))
    _lib.check(st, 'ia_point_normals')
    return normal, variation, eig, cov


# ------------------------------------------------------------------ mesh simplification (csrc/simplify.hip)

def simplify_plan(lo, hi, cells=None, cells_long=0, cell_size=0.0):
    """Grid of the clustering (host arithmetic, see ia_simplify_plan): -> (dims, inv_cell, cell)."""
    dims, inv, cell = (ctypes.c_int * 3)(), (ctypes.c_float * 3)(), (ctypes.c_double * 3)()
    st = _lib.load().ia_simplify_plan(_f3(lo), _f3(hi), None if cells is None else _i3(cells), int(cells_long), float(cell_size), dims, inv, cell)
    _lib.check(st, 'ia_simplify_plan')
    return tuple(dims), tuple(inv), tuple(cell)


def simplify_box(verts):
    """(lo, hi) of the finite vertices as lists of floats, or None without a finite vertex (see ia_simplify_box).  One host
    synchronisation."""
    _f32c(verts, 'verts')
    dev = verts.device
    scratch = torch.empty(6 * 1024, device=dev)
    box = torch.empty(6, device=dev)
    with torch.cuda.device(dev), _Phase('keys', dev, 'SIMPLIFY_TIMES'):
        st = _lib.load().ia_simplify_box(_p(verts), verts.shape[0], _p(scratch), scratch.numel() * 4, _p(box), _lib.stream_ptr(dev))
        _lib.check(st, 'ia_simplify_box')
        b = box.cpu().tolist()
    if not all(math.isfinite(x) for x in b):
        return None
    return b[:3], b[3:]


def simplify_keys(verts, lo, inv_cell, dims):
    """int64 [V]: the linear cell index of every vertex, INT64_MAX without a cell (see ia_simplify_keys)."""
    _f32c(verts, 'verts')
    dev = verts.device
    keys = torch.empty(verts.shape[0], dtype=torch.int64, device=dev)
    with torch.cuda.device(dev), _Phase('keys', dev, 'SIMPLIFY_TIMES'):
        st = _lib.load().ia_simplify_keys(_p(verts), verts.shape[0], _f3(lo), _f3(inv_cell), _i3(dims), _p(keys), _lib.stream_ptr(dev))
    _lib.check(st, 'ia_simplify_keys')
    return keys


def simplify_topology(keys, faces, full=True, pairs=False):
    """The integer part of the clustering from per-vertex keys int64 [V] and faces int32 [F,3] (ia_simplify_clusters, _classify,
    _face_heads, _refs; the two key sorts are torch.sort).  Returns a dict of device arrays and the host counts 'K', 'n_valid',
    'usable', 'surviving', 'n_pairs', 'n_faces' (unique surviving faces) and, with ``full``, 'n_verts'.  ``full=False`` is the
    count-only pass.  Two host synchronisations."""
    _i32c(faces, 'faces')
    if not (keys.is_cuda and keys.dtype == torch.int64 and keys.is_contiguous() and keys.device == faces.device):
        raise RuntimeError('keys must be a contiguous int64 tensor on the device of the faces')
    lib, dev = _lib.load(), faces.device
    v, f = keys.numel(), faces.shape[0]
    i32 = dict(dtype=torch.int32, device=dev)
    s = {'V': v, 'F': f}
    with torch.cuda.device(dev):
        stream = _lib.stream_ptr(dev)
        with _Phase('sorts', dev, 'SIMPLIFY_TIMES'):
            skeys, order = torch.sort(keys, stable=True)
        with _Phase('keys', dev, 'SIMPLIFY_TIMES'):
            vcluster, vseg = torch.empty(v, **i32), torch.empty(v, **i32)
            cstart, ckey = torch.empty(v + 1, **i32), torch.empty(max(v, 1), dtype=torch.int64, device=dev)
            scratch, count = torch.empty(v + 1, **i32), torch.empty(2, **i32)
            st = lib.ia_simplify_clusters(_p(skeys), _p(order), v, _p(vcluster), _p(vseg), _p(cstart), _p(ckey), v, _p(scratch),
                                          scratch.numel() * 4, _p(count), stream)
            _lib.check(st, 'ia_simplify_clusters')
            k, n_valid = (int(x) for x in count.cpu())
        with _Phase('faces', dev, 'SIMPLIFY_TIMES'):
            tri, key = torch.empty(max(f, 1), 3, **i32), torch.empty(max(f, 1), dtype=torch.int64, device=dev)
            ref = torch.empty(max(k, 1), **i32) if full else None
            pr = torch.empty(max(3 * f, 1), **i32) if pairs else None
            fcount = torch.empty(3, **i32)
            st = lib.ia_simplify_classify(_p(faces), f, v, _p(vcluster), k, _p(tri), _p(key), _p(ref), _p(pr), _p(fcount), stream)
            _lib.check(st, 'ia_simplify_classify')
        with _Phase('sorts', dev, 'SIMPLIFY_TIMES'):
            perm = torch.sort(key[:f], stable=True)[1]
            if float(k) ** 3 >= 9.0e18:                                   # the key holds (b, c) only: a second, stable sort by a
                perm = perm[torch.sort(tri[:f, 0][perm], stable=True)[1]].contiguous()
        with _Phase('faces', dev, 'SIMPLIFY_TIMES'):
            fpos = torch.empty(f + 1, **i32)
            _lib.check(lib.ia_simplify_face_heads(_p(tri), _p(perm), f, _p(fpos), stream), 'ia_simplify_face_heads')
            outidx = None
            if full:
                outidx = torch.empty(k + 1, **i32)
                _lib.check(lib.ia_simplify_refs(_p(ref), k, _p(outidx), stream), 'ia_simplify_refs')
            tail = torch.cat([fcount, fpos[f:], outidx[k:]] if full else [fcount, fpos[f:]]).cpu().tolist()
    s.update(K=k, n_valid=n_valid, usable=tail[0], surviving=tail[1], n_pairs=tail[2], n_faces=tail[3], n_verts=tail[4] if full else None,
             order=order, vcluster=vcluster, vseg=vseg, cstart=cstart, ckey=ckey, tri=tri, perm=perm, fpos=fpos, ref=ref, outidx=outidx,
             pairs=pr, faces=faces)
    return s


def simplify_outputs(s):
    """faces int64 [F',3], vertex_map int64 [V], cluster_size int64 [V'] and the cluster of every output vertex (int32 [V']) of a full
    ``simplify_topology`` state (ia_simplify_outputs, ia_simplify_faces)."""
    lib, dev = _lib.load(), s['faces'].device
    v, f, k, nv, nf = s['V'], s['F'], s['K'], s['n_verts'], s['n_faces']
    vertex_map = torch.empty(v, dtype=torch.int64, device=dev)
    ocl = torch.empty(nv, dtype=torch.int32, device=dev)
    csize = torch.empty(nv, dtype=torch.int64, device=dev)
    faces_out = torch.empty(nf, 3, dtype=torch.int64, device=dev)
    with torch.cuda.device(dev), _Phase('faces', dev, 'SIMPLIFY_TIMES'):
        stream = _lib.stream_ptr(dev)
        st = lib.ia_simplify_outputs(_p(s['vcluster']), v, _p(s['ref']), _p(s['outidx']), _p(s['cstart']), k, _p(vertex_map), _p(ocl),
                                     _p(csize), nv, stream)
        _lib.check(st, 'ia_simplify_outputs')
        st = lib.ia_simplify_faces(_p(s['tri']), _p(s['perm']), _p(s['fpos']), f, _p(s['outidx']), k, _p(faces_out), nf, stream)
        _lib.check(st, 'ia_simplify_faces')
    return faces_out, vertex_map, csize, ocl


def simplify_vertex_sums(s, cols):
    """float64 [K, C]: per cluster the sums of the columns of ``cols`` (float64 [V,C]) over its vertices, four columns per call of
    ia_simplify_accumulate_verts."""
    if not (cols.is_cuda and cols.dtype == torch.float64 and cols.is_contiguous() and cols.dim() == 2 and cols.shape[0] == s['V']):
        raise RuntimeError(f'cols must be a contiguous float64 [V,C] device tensor, got {cols.dtype} {tuple(cols.shape)}')
    lib, dev = _lib.load(), cols.device
    k, c = s['K'], cols.shape[1]
    out = torch.zeros(k, c, dtype=torch.float64, device=dev)
    if k == 0 or c == 0:
        return out
    scratch, nbytes = _scratch('ia_simplify_accumulate_scratch_bytes', s['n_valid'], 4, dtype=torch.float64, device=dev, extra=1)
    with torch.cuda.device(dev), _Phase('accumulate', dev, 'SIMPLIFY_TIMES'):
        for c0 in range(0, c, 4):
            nc = min(4, c - c0)
            sums = torch.empty(k, 4, dtype=torch.float64, device=dev)
            st = lib.ia_simplify_accumulate_verts(_p(cols), c, c0, nc, _p(s['order']), _p(s['vseg']), s['n_valid'], s['V'], k, _p(sums),
                                                  _p(scratch), nbytes, _lib.stream_ptr(dev))
            _lib.check(st, 'ia_simplify_accumulate_verts')
            out[:, c0:c0 + nc] = sums[:, :nc]
    return out


def simplify_quadric_sums(s, verts, lo, inv_cell, cell, dims):
    """float64 [K,9]: per cluster the summed plane quadrics of its usable faces (ia_simplify_accumulate_faces; the stable sort of the
    (cluster, face) pairs is torch.sort)."""
    _f32c(verts, 'verts')
    lib, dev = _lib.load(), verts.device
    k, f, n = s['K'], s['F'], s['n_pairs']
    sums = torch.zeros(max(k, 1), 9, dtype=torch.float64, device=dev)
    if k == 0:
        return sums
    with torch.cuda.device(dev):
        with _Phase('sorts', dev, 'SIMPLIFY_TIMES'):
            spairs, porder = torch.sort(s['pairs'][:3 * f], stable=True)
        scratch, nbytes = _scratch('ia_simplify_accumulate_scratch_bytes', n, 9, dtype=torch.float64, device=dev, extra=1)
        with _Phase('accumulate', dev, 'SIMPLIFY_TIMES'):
            st = lib.ia_simplify_accumulate_faces(_p(verts), s['V'], _p(s['faces']), f, _p(porder), _p(spairs), n, _p(s['ckey']), k, _f3(lo),
                                                  _f3(inv_cell), _d3(cell), _i3(dims), _p(sums), _p(scratch), nbytes,
                                                  _lib.stream_ptr(dev))
        _lib.check(st, 'ia_simplify_accumulate_faces')
    return sums


def simplify_place(s, ocl, vsum, qsum, lo, inv_cell, cell, dims):
    """float32 [V',3]: the representatives (ia_simplify_place); ``qsum`` None: the cluster means."""
    lib, dev = _lib.load(), ocl.device
    nv = ocl.numel()
    out = torch.empty(nv, 3, device=dev)
    vs = vsum if vsum.shape[1] == 4 else torch.nn.functional.pad(vsum, (0, 4 - vsum.shape[1]))
    with torch.cuda.device(dev), _Phase('place', dev, 'SIMPLIFY_TIMES'):
        st = lib.ia_simplify_place(_p(vs.contiguous()), _p(qsum), _p(ocl), _p(s['cstart']), _p(s['ckey']), s['K'], nv, _f3(lo), _f3(inv_cell),
                                   _d3(cell), _i3(dims), _p(out), nv, _lib.stream_ptr(dev))
    _lib.check(st, 'ia_simplify_place')
    return out


def simplify_means(s, ocl, sums):
    """float64 [V',C]: ``sums`` (float64 [K,C]) over the cluster sizes at the output vertices (ia_simplify_means)."""
    lib, dev = _lib.load(), ocl.device
    nv, c = ocl.numel(), sums.shape[1]
    out = torch.empty(nv, c, dtype=torch.float64, device=dev)
    with torch.cuda.device(dev), _Phase('place', dev, 'SIMPLIFY_TIMES'):
        for c0 in range(0, c, 4):
            nc = min(4, c - c0)
            block = torch.zeros(max(s['K'], 1), 4, dtype=torch.float64, device=dev)
            block[:s['K'], :nc] = sums[:, c0:c0 + nc]
            st = lib.ia_simplify_means(_p(block), _p(ocl), _p(s['cstart']), s['K'], nv, nc, _p(out), c, c0, nv, _lib.stream_ptr(dev))
            _lib.check(st, 'ia_simplify_means')
    return out


# ------------------------------------------------------------------ mesh smoothing and mesh normals (csrc/smooth.hip)

def mesh_adjacency(verts, faces):
    """The neighbourhood structure of a mesh (verts float32 [V,3], faces int32 [F,3]) as a dict of device arrays: 'offsets',
    'neighbors', 'edge_faces', 'boundary', 'face_offsets', 'face_ids' (see geometry.MeshAdjacency), the host dict 'info', the flag
    'out_of_range' and what ``mesh_cotangent`` and ``smooth_steps`` need (ia_mesh_edge_keys, _edge_heads, _csr; the two key sorts are
    torch.sort).  Two host synchronisations."""
    v, f = _mesh_checked(verts, faces)
    lib, dev = _lib.load(), verts.device
    i32 = dict(dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        stream = _lib.stream_ptr(dev)
        count = torch.empty(8, **i32)
        with _Phase('keys', dev, 'SMOOTH_TIMES'):
            ekeys, vkeys = torch.empty(6 * f, dtype=torch.int64, device=dev), torch.empty(3 * f, dtype=torch.int64, device=dev)
            _lib.check(lib.ia_mesh_edge_keys(_p(verts), v, _p(faces), f, _p(ekeys), _p(vkeys), _p(count), stream), 'ia_mesh_edge_keys')
        with _Phase('sorts', dev, 'SMOOTH_TIMES'):
            skeys, order = torch.sort(ekeys, stable=True)
            svkeys, vorder = torch.sort(vkeys, stable=True)
            del ekeys, vkeys
        with _Phase('csr', dev, 'SMOOTH_TIMES'):
            scratch, nbytes = _scratch('ia_mesh_edge_heads_scratch_bytes', f, **i32)
            _lib.check(lib.ia_mesh_edge_heads(_p(skeys), f, _p(scratch), nbytes, _p(count), stream), 'ia_mesh_edge_heads')
            head = count.cpu().tolist()
            usable, oob, e = head[0], bool(head[1]), head[7]
            s = {'V': v, 'F': f, 'E': e, 'out_of_range': oob, 'order': order}
            if oob:
                return s
            offsets, face_offsets = torch.empty(v + 1, **i32), torch.empty(v + 1, **i32)
            neighbors, edge_faces, run_start = torch.empty(e, **i32), torch.empty(e, **i32), torch.empty(e, **i32)
            slot_keys = torch.empty(e, dtype=torch.int64, device=dev)
            boundary = torch.empty(v, dtype=torch.bool, device=dev)
            face_ids, heavy = torch.empty(3 * usable, **i32), torch.empty(max(v, 1), **i32)
            st = lib.ia_mesh_csr(_p(skeys), _p(svkeys), _p(vorder), v, f, usable, e, _p(scratch), _p(offsets), _p(neighbors), _p(edge_faces),
                                 _p(run_start), _p(slot_keys), _p(boundary), _p(face_offsets), _p(face_ids), _p(heavy), _p(count), stream)
            _lib.check(st, 'ia_mesh_csr')
            c = count.cpu().tolist()
    s.update(offsets=offsets, neighbors=neighbors, edge_faces=edge_faces, boundary=boundary, face_offsets=face_offsets, face_ids=face_ids,
             run_start=run_start, slot_keys=slot_keys, heavy=heavy, n_heavy=c[6],
             info={'edges': e // 2, 'boundary_edges': c[2] // 2, 'nonmanifold_edges': c[3] // 2, 'boundary_verts': c[4], 'usable_faces': usable,
                   'max_degree': c[5]})
    return s


def mesh_cotangent(s, verts, faces):
    """float32 [E]: the cotangent weight of every directed edge of a ``mesh_adjacency`` state (ia_mesh_cotangent)."""
    _f32c(verts, 'verts')
    _i32c(faces, 'faces')
    dev = verts.device
    w = torch.empty(s['E'], device=dev)
    with torch.cuda.device(dev), _Phase('cotangent', dev, 'SMOOTH_TIMES'):
        st = _lib.load().ia_mesh_cotangent(_p(verts), s['V'], _p(faces), s['F'], _p(s['order']), _p(s['slot_keys']), _p(s['run_start']),
                                           _p(s['edge_faces']), s['E'], _p(w), _lib.stream_ptr(dev))
    _lib.check(st, 'ia_mesh_cotangent')
    return w


def smooth_pinned(s, verts, weights, fix_boundary, fixed):
    """bool [V]: the vertices that a smoothing step leaves alone (ia_smooth_pinned)."""
    _f32c(verts, 'verts')
    dev = verts.device
    if verts.shape[0] != s['V'] or (weights is not None and (weights.numel() != s['E'] or weights.dtype != torch.float32)):
        raise RuntimeError('verts and weights must match the adjacency')
    if fixed is not None and not (fixed.is_cuda and fixed.dtype == torch.bool and fixed.is_contiguous() and fixed.numel() == s['V']):
        raise RuntimeError('fixed must be a contiguous bool [V] device tensor')
    pinned = torch.empty(s['V'], dtype=torch.bool, device=dev)
    with torch.cuda.device(dev):
        st = _lib.load().ia_smooth_pinned(_p(verts), s['V'], _p(s['offsets']), _p(weights), _p(s['boundary']), int(bool(fix_boundary)), _p(fixed),
                                          _p(pinned), _lib.stream_ptr(dev))
    _lib.check(st, 'ia_smooth_pinned')
    return pinned


def smooth_steps(s, verts, weights, pinned, factors):
    """float32 [V,3]: ``verts`` after one Jacobi step per factor (ia_smooth_steps: every launch on the current stream, no host
    synchronisation).  ``verts`` is not written."""
    _f32c(verts, 'verts')
    dev = verts.device
    a, b = verts.clone(), torch.empty_like(verts)
    n = len(factors)
    if n == 0 or s['V'] == 0:
        return a
    fac = (ctypes.c_double * n)(*[float(x) for x in factors])
    with torch.cuda.device(dev), _Phase('steps', dev, 'SMOOTH_TIMES'):
        st = _lib.load().ia_smooth_steps(_p(a), _p(b), s['V'], _p(s['offsets']), _p(s['neighbors']), _p(weights), _p(pinned), _p(s['heavy']),
                                         s['n_heavy'], fac, n, _lib.stream_ptr(dev))
    _lib.check(st, 'ia_smooth_steps')
    return a if n % 2 == 0 else b


def mesh_normals(s, verts, faces, angle=False):
    """float32 [V,3]: unit vertex normals from the mesh (ia_mesh_normals)."""
    _f32c(verts, 'verts')
    _i32c(faces, 'faces')
    dev = verts.device
    out = torch.empty(s['V'], 3, device=dev)
    with torch.cuda.device(dev), _Phase('normals', dev, 'SMOOTH_TIMES'):
        st = _lib.load().ia_mesh_normals(_p(verts), s['V'], _p(faces), s['F'], _p(s['face_offsets']), _p(s['face_ids']), int(bool(angle)),
                                         _p(out), _lib.stream_ptr(dev))
    _lib.check(st, 'ia_mesh_normals')
    return out


# ------------------------------------------------------------------ mesh rasteriser (csrc/mesh_raster.hip)

MESH_RASTER_TIMES = None     # a dict collects seconds per stage, as SMOOTH_TIMES does: tools/bench_mesh_raster.py


def _views_checked(cams, resolution):
    _f32c(cams, 'cameras')
    if cams.dim() != 2 or cams.shape[1] != 25:
        raise RuntimeError(f'cameras must be [N,25], got {tuple(cams.shape)}')
    h, w = resolution
    return cams.shape[0], int(h), int(w)


def mesh_project(verts, cams, resolution, near=1e-6):
    """int32 [N,V,4]: per view and vertex the snapped screen coordinates U, V (1/256 pixel), the bits of the camera depth z and the
    usable flag (ia_mesh_project; reads the camera labels back once to check K)."""
    _f32c(verts, 'verts')
    n, h, w = _views_checked(cams, resolution)
    dev = verts.device
    proj = torch.empty(n, verts.shape[0], 4, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev), _Phase('project', dev, 'MESH_RASTER_TIMES'):
        st = _lib.load().ia_mesh_project(_p(verts), verts.shape[0], _p(cams), n, h, w, float(near), _p(proj), _lib.stream_ptr(dev))
    _lib.check(st, 'ia_mesh_project')
    return proj


def mesh_raster(proj, faces, resolution, cull_back=False, oversize_pixels=256):
    """(vis int64 [N,H,W] holding the uint64 keys float_bits(z) << 32 | face, all ones on a miss; culled int32 [N]) (ia_mesh_raster)."""
    _i32c(proj, 'proj')
    _i32c(faces, 'faces')
    n, v = proj.shape[:2]
    h, w = (int(r) for r in resolution)
    f, dev = faces.shape[0], proj.device
    vis = torch.empty(n, h, w, dtype=torch.int64, device=dev)
    culled = torch.empty(n, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev), _Phase('raster', dev, 'MESH_RASTER_TIMES'):
        scratch, nbytes = (None, 0)
        if f and oversize_pixels < h * w:
            scratch, nbytes = _scratch('ia_mesh_raster_scratch_bytes', n, f, dtype=torch.int32, device=dev)
        st = _lib.load().ia_mesh_raster(_p(proj), v, _p(faces), f, n, h, w, int(bool(cull_back)), int(oversize_pixels), _p(vis), _p(culled),
                                        _p(scratch), nbytes, _lib.stream_ptr(dev))
    _lib.check(st, 'ia_mesh_raster')
    return vis, culled


def mesh_resolve(vis, proj, verts, faces, cams, normals=None, attributes=None, cull_back=False):
    """dict of 'mask' bool, 'face' int32, 'bary' [..,3], 'depth', 'normal' [..,3], 'attributes' [..,C] or None, leading shape [N,H,W]
    (ia_mesh_resolve)."""
    _f32c(verts, 'verts')
    _i32c(faces, 'faces')
    n, h, w = vis.shape
    _views_checked(cams, (h, w))
    dev = verts.device
    c = 0
    if normals is not None:
        _f32c(normals, 'normals')
    if attributes is not None:
        _f32c(attributes, 'attributes')
        c = attributes.shape[1]
    out = {'mask': torch.empty(n, h, w, dtype=torch.bool, device=dev), 'face': torch.empty(n, h, w, dtype=torch.int32, device=dev),
           'bary': torch.empty(n, h, w, 3, device=dev), 'depth': torch.empty(n, h, w, device=dev), 'normal': torch.empty(n, h, w, 3, device=dev),
           'attributes': torch.empty(n, h, w, c, device=dev) if c else None}
    with torch.cuda.device(dev), _Phase('resolve', dev, 'MESH_RASTER_TIMES'):
        st = _lib.load().ia_mesh_resolve(_p(vis), _p(proj), _p(verts), verts.shape[0], _p(faces), faces.shape[0], _p(cams), n, h, w,
                                         int(bool(cull_back)), _p(normals), _p(attributes), c, _p(out['mask']), _p(out['face']), _p(out['bary']),
                                         _p(out['depth']), _p(out['normal']), _p(out['attributes']), _lib.stream_ptr(dev))
    _lib.check(st, 'ia_mesh_resolve')
    return out


def rasterize_mesh(verts, faces, cams, h, w, normals=None, attributes=None, cull_back=False, near=1e-6, oversize_pixels=256):
    """The three stages of geometry.rasterize_mesh on the current stream; no host read after the camera check of the first."""
    _mesh_checked(verts, faces)
    proj = mesh_project(verts, cams, (h, w), near)
    vis, culled = mesh_raster(proj, faces, (h, w), cull_back, oversize_pixels)
    out = mesh_resolve(vis, proj, verts, faces, cams, normals, attributes, cull_back)
    out['culled'] = culled
    return out


# ------------------------------------------------------------------ TSDF integration (csrc/tsdf.hip)

TSDF_MAX_CHANNELS = 8        # csrc/tsdf.hip kMaxChannels
TSDF_VIEW_ROW = 18           # csrc/tsdf.hip kViewRow


def tsdf_integrate(depth, views, dims, lo, step, truncation, near=1e-6, mask=None, weights=None, colors=None, state=None):
    """Depth maps fused into a lattice (see ia_tsdf_integrate): depth float32 [N,H,W], views float32 [N,18] (rotation, origin, rows 0 and
    1 of K_res), mask bool [N,H,W], weights float32 [N,H,W], colors float32 [N,C,H,W] -> dict of 'sum', 'weight', 'tsdf' [nx,ny,nz] and,
    with colours, 'color_sum' [nx,ny,nz,C] and 'color_weight'.  ``state``: such a dict, whose sums the call goes on from (it is not
    modified)."""
    _f32c(depth, 'depth'), _f32c(views, 'views')
    if depth.dim() != 3 or views.dim() != 2 or tuple(views.shape) != (depth.shape[0], TSDF_VIEW_ROW) or views.device != depth.device:
        raise RuntimeError(f'depth must be [N,H,W] and views [N,{TSDF_VIEW_ROW}] on one device, got {tuple(depth.shape)} and {tuple(views.shape)}')
    n, h, w = depth.shape
    dev = depth.device
    dims = tuple(int(d) for d in dims)
    if len(dims) != 3:
        raise RuntimeError(f'dims must be (nx, ny, nz), got {dims}')
    if mask is not None and not (mask.is_cuda and mask.dtype == torch.bool and mask.is_contiguous() and tuple(mask.shape) == (n, h, w)):
        raise RuntimeError(f'mask must be a contiguous bool device tensor {(n, h, w)}')
    if weights is not None and tuple(_f32c(weights, 'weights').shape) != (n, h, w):
        raise RuntimeError(f'weights must be {(n, h, w)}, got {tuple(weights.shape)}')
    c = 0
    if colors is not None:
        _f32c(colors, 'colors')
        if colors.dim() != 4 or colors.shape[0] != n or tuple(colors.shape[2:]) != (h, w):
            raise RuntimeError(f'colors must be [{n},C,{h},{w}], got {tuple(colors.shape)}')
        c = int(colors.shape[1])
    names = ('sum', 'weight') + (('color_sum', 'color_weight') if c else ())
    shapes = {'color_sum': dims + (c,)}
    if state is None:
        out = {k: torch.empty(shapes.get(k, dims), device=dev) for k in names}
    else:
        for k in names:
            if tuple(_f32c(state[k], f"state['{k}']").shape) != shapes.get(k, dims) or state[k].device != dev:
                raise RuntimeError(f"state['{k}'] must be {shapes.get(k, dims)} on the device of depth, got {tuple(state[k].shape)}")
        out = {k: state[k].clone() for k in names}
    out['tsdf'] = torch.empty(dims, device=dev)
    points = dims[0] * dims[1] * dims[2]
    nbytes = 4.0 * points * (3 + (c + 1 if c else 0)) * (2 if state is not None else 1)
    with torch.cuda.device(dev), _Timed('tsdf_integrate', 40.0 * points * n, nbytes, f'{dims} N={n} {h}x{w} C={c}'):
        st = _lib.load().ia_tsdf_integrate(_p(depth), _p(mask), _p(weights), _p(colors), _p(views), n, c, h, w, *dims, _f3(lo), _f3(step),
                                           float(truncation), float(near), int(state is not None), _p(out['sum']), _p(out['weight']),
                                           _p(out['tsdf']), _p(out.get('color_sum')), _p(out.get('color_weight')), _lib.stream_ptr(dev))
    _lib.check(st, 'ia_tsdf_integrate')
    return out


# ------------------------------------------------------------------ texture atlas (csrc/texture.hip)

TEXTURE_TIMES = None         # a dict collects seconds per stage, as SMOOTH_TIMES does: tools/bench_texture.py


def atlas_points(verts, faces, size, s, normals=None):
    """dict of 'point' [size,size,3], 'face' int32 [size,size], 'bary' [size,size,3], 'normal' [size,size,3] and 'degenerate' int32 [1]
    (a device counter) for the atlas of block side ``s`` (ia_atlas_points)."""
    _mesh_checked(verts, faces)
    if normals is not None:
        _f32c(normals, 'normals')
    dev = verts.device
    out = {'point': torch.empty(size, size, 3, device=dev), 'face': torch.empty(size, size, dtype=torch.int32, device=dev),
           'bary': torch.empty(size, size, 3, device=dev), 'normal': torch.empty(size, size, 3, device=dev),
           'degenerate': torch.empty(1, dtype=torch.int32, device=dev)}
    with torch.cuda.device(dev), _Phase('atlas_points', dev, 'TEXTURE_TIMES'):
        st = _lib.load().ia_atlas_points(_p(verts), verts.shape[0], _p(faces), faces.shape[0], int(size), int(s), _p(normals), _p(out['point']),
                                         _p(out['face']), _p(out['bary']), _p(out['normal']), _p(out['degenerate']), _lib.stream_ptr(dev))
    _lib.check(st, 'ia_atlas_points')
    return out


def texture_project(point, normal, face, images, cams, depth, mask, near, min_cos, power, depth_tol, best=False, fallback=None):
    """dict of 'texture' [..., C], 'weight', 'views' int32 and 'filled' bool with the leading shape of ``face`` (ia_texture_project)."""
    _f32c(point, 'point'), _f32c(normal, 'normal'), _i32c(face, 'face'), _f32c(images, 'images'), _f32c(depth, 'depth')
    n, h, w, c = images.shape
    _views_checked(cams, (h, w))
    if mask.dtype != torch.bool or not mask.is_contiguous() or tuple(mask.shape) != (n, h, w) or tuple(depth.shape) != (n, h, w) or cams.shape[0] != n:
        raise RuntimeError(f'depth and mask must be [N,H,W] = {(n, h, w)} (mask bool) with N cameras')
    lead, dev = tuple(face.shape), point.device
    t = face.numel()
    if tuple(point.shape) != lead + (3,) or tuple(normal.shape) != lead + (3,):
        raise RuntimeError('point and normal must have the shape of face plus [3]')
    if fallback is not None:
        _f32c(fallback, 'fallback')
        if tuple(fallback.shape) != lead + (c,):
            raise RuntimeError(f'fallback must be {lead + (c,)}, got {tuple(fallback.shape)}')
    out = {'texture': torch.empty(lead + (c,), device=dev), 'weight': torch.empty(lead, device=dev),
           'views': torch.empty(lead, dtype=torch.int32, device=dev), 'filled': torch.empty(lead, dtype=torch.bool, device=dev)}
    with torch.cuda.device(dev), _Phase('project', dev, 'TEXTURE_TIMES'):
        st = _lib.load().ia_texture_project(_p(point), _p(normal), _p(face), t, _p(images), _p(cams), n, h, w, c, _p(depth), _p(mask), float(near),
                                            float(min_cos), float(power), float(depth_tol), int(bool(best)), _p(fallback), _p(out['texture']),
                                            _p(out['weight']), _p(out['views']), _p(out['filled']), _lib.stream_ptr(dev))
    _lib.check(st, 'ia_texture_project')
    return out


def texture_sample(texture, s, n_faces, face, bary):
    """float32 ``face.shape + [C]``: the bilinear lookup of ``texture`` [size,size,C] at the barycentrics of the faces (ia_texture_sample)."""
    _f32c(texture, 'texture'), _i32c(face, 'face'), _f32c(bary, 'bary')
    if texture.dim() != 3 or texture.shape[0] != texture.shape[1] or tuple(bary.shape) != tuple(face.shape) + (3,):
        raise RuntimeError(f'texture must be [size,size,C] and bary face.shape + [3], got {tuple(texture.shape)}, {tuple(bary.shape)}')
    dev = texture.device
    out = torch.empty(tuple(face.shape) + (texture.shape[2],), device=dev)
    with torch.cuda.device(dev), _Phase('sample', dev, 'TEXTURE_TIMES'):
        st = _lib.load().ia_texture_sample(_p(texture), texture.shape[0], texture.shape[2], int(s), int(n_faces), _p(face), _p(bary), face.numel(),
                                           _p(out), _lib.stream_ptr(dev))
    _lib.check(st, 'ia_texture_sample')
    return out


# ------------------------------------------------------------------ LPIPS (csrc/lpips.hip)

ACT_RELU = 2     # IA_ACT_RELU


def conv2d_direct(x, w, bias=None, stride=1, padding=0, relu=True):
    """ia_conv2d_direct: fp32 direct convolution + bias (+ ReLU) of x [N,I,H,W] with w [O,I,k,k] (k <= 11, stride 1 or 4, padding < k)."""
    _f32c(x, 'x'), _f32c(w, 'w')
    if x.dim() != 4 or w.dim() != 4 or w.shape[1] != x.shape[1] or w.shape[2] != w.shape[3] or w.device != x.device:
        raise RuntimeError(f'conv2d_direct: x [N,I,H,W] and w [O,I,k,k] on one device, got {tuple(x.shape)} and {tuple(w.shape)}')
    n, i, h, wd = x.shape
    o, k = w.shape[0], w.shape[2]
    if bias is not None and _f32c(bias, 'bias').numel() != o:
        raise RuntimeError(f'conv2d_direct: bias has {bias.numel()} elements, expected {o}')
    stride, padding = int(stride), int(padding)
    if stride < 1 or h + 2 * padding < k or wd + 2 * padding < k:
        raise RuntimeError(f'conv2d_direct: a {h} x {wd} image (padding {padding}) is smaller than the {k} x {k} kernel, or stride < 1')
    oh, ow = (h + 2 * padding - k) // stride + 1, (wd + 2 * padding - k) // stride + 1
    y = torch.empty(n, o, oh, ow, device=x.device, dtype=torch.float32)
    flops = 2.0 * n * oh * ow * i * o * k * k
    with torch.cuda.device(x.device), _Timed('conv2d_direct', flops, 4.0 * (x.numel() + w.numel() + y.numel()), f'N{n} I{i} O{o} {h}x{wd} k{k} s{stride}'):
        st = _lib.load().ia_conv2d_direct(_p(x), _p(w), _p(bias), _p(y), n, i, o, h, wd, k, stride, padding, ACT_RELU if relu else ACT_ID['linear'],
                                          _lib.stream_ptr(x.device))
    _lib.check(st, 'ia_conv2d_direct')
    return y


def maxpool2d(x, kernel_size, stride=2, want_f32=True, want_split=False, split_planes=2, consumer=None):
    """ia_maxpool2d: floor-mode max pool (k3 s2 or k2 s2) of fp32 [N,C,H,W].  Returns the fp32 result, a SplitAct (the operand of a 3x3
    MFMA convolution behind the pool; C % 8 == 0), or the pair (y, ys) when both are asked for."""
    _f32c(x, 'x')
    if x.dim() != 4 or not (want_f32 or want_split):
        raise RuntimeError('maxpool2d: x must be [N,C,H,W], and one of want_f32 / want_split')
    n, c, h, w = x.shape
    k, stride = int(kernel_size), int(stride)
    if k < 1 or stride < 1 or h < k or w < k:
        raise RuntimeError(f'maxpool2d: a {h} x {w} map is smaller than the {k} x {k} window')
    if want_split and c % 8:
        raise RuntimeError(f'the split format stores channels in groups of 8 (C = {c})')
    oh, ow = (h - k) // stride + 1, (w - k) // stride + 1
    y = torch.empty(n, c, oh, ow, device=x.device, dtype=torch.float32) if want_f32 else None
    ys = torch.empty(n, split_planes, c // 8, oh, ow, 8, device=x.device, dtype=torch.float16) if want_split else None
    with torch.cuda.device(x.device), _Timed('maxpool2d', 0.0, 4.0 * x.numel() + 4.0 * n * c * oh * ow * (int(want_f32) + int(want_split)),
                                             f'N{n} C{c} {h}x{w} k{k}'):
        st = _lib.load().ia_maxpool2d(_p(x), _p(y), _p(ys), int(split_planes), n, c, h, w, k, stride, _lib.stream_ptr(x.device))
    _lib.check(st, 'ia_maxpool2d')
    out_s = SplitAct(ys, c, consumer) if want_split else None
    if want_f32 and want_split:
        return y, out_s
    return y if want_f32 else out_s


def lpips_layer(f, lin, out=None):
    """ia_lpips_layer: f fp32 [2N,C,h,w] (maps n and N + n are a pair), lin [C] -> float32 [N], the tap's layer value per pair; `out`:
    a float32 [N] view (any stride) to write into, e.g. a column of the [N,5] table."""
    _f32c(f, 'f'), _f32c(lin, 'lin')
    if f.dim() != 4 or f.shape[0] % 2 or f.shape[0] < 2 or lin.numel() != f.shape[1] or lin.device != f.device:
        raise RuntimeError(f'lpips_layer: f [2N,C,h,w] and lin [C] on one device, got {tuple(f.shape)} and {tuple(lin.shape)}')
    n, c, h, w = f.shape[0] // 2, f.shape[1], f.shape[2], f.shape[3]
    if out is None:
        out = torch.empty(n, device=f.device, dtype=torch.float32)
    if not (out.is_cuda and out.device == f.device and out.dtype == torch.float32 and out.dim() == 1 and out.shape[0] == n
            and (n == 1 or out.stride(0) >= 1)):
        raise RuntimeError('lpips_layer: out must be a float32 [N] device view with a positive stride')
    scratch, nbytes = _scratch('ia_lpips_layer_scratch_bytes', n, h, w, dtype=torch.float64, device=f.device)
    with torch.cuda.device(f.device), _Timed('lpips_layer', 6.0 * f.numel(), 8.0 * f.numel(), f'N{n} C{c} {h}x{w}'):
        st = _lib.load().ia_lpips_layer(_p(f), _p(lin), n, c, h, w, _p(scratch), nbytes, _p(out), max(int(out.stride(0)), 1),
                                        _lib.stream_ptr(f.device))
    _lib.check(st, 'ia_lpips_layer')
    return out


# ------------------------------------------------------------------ identity similarity (csrc/identity.hip)

def face_crop_pool(images):
    """ia_face_crop_pool: float32 [N,3,H,W] or uint8 [N,H,W,3] (H, W >= 256) -> float32 [N,3,112,112], the reference's crop + pool."""
    if not (torch.is_tensor(images) and images.is_cuda and images.is_contiguous() and images.dim() == 4
            and images.dtype in (torch.float32, torch.uint8)):
        raise RuntimeError('face_crop_pool: a contiguous float32 [N,3,H,W] or uint8 [N,H,W,3] device tensor')
    u8 = images.dtype == torch.uint8
    n, c, h, w = (images.shape[0], images.shape[3], images.shape[1], images.shape[2]) if u8 else images.shape
    if c != 3 or n < 1 or h < 256 or w < 256:
        raise RuntimeError(f'face_crop_pool: 3 channels and sides >= 256, got {tuple(images.shape)}')
    y = torch.empty(n, 3, 112, 112, device=images.device, dtype=torch.float32)
    with torch.cuda.device(images.device), _Timed('face_crop_pool', 0.0, float(images.numel() * images.element_size() + 4 * y.numel()), f'N{n} {h}x{w}'):
        st = _lib.load().ia_face_crop_pool(_p(images), 1 if u8 else 0, _p(y), n, h, w, _lib.stream_ptr(images.device))
    _lib.check(st, 'ia_face_crop_pool')
    return y


def prelu_channels(x, slopes, inplace=False):
    """ia_prelu_channels: per-channel PReLU of fp32 [B,C,...]."""
    _f32c(x, 'x'), _f32c(slopes, 'slopes')
    if x.dim() < 2 or slopes.numel() != x.shape[1] or slopes.device != x.device or x.numel() == 0:
        raise RuntimeError(f'prelu_channels: x [B,C,...] and slopes [C] on one device, got {tuple(x.shape)} and {tuple(slopes.shape)}')
    y = x if inplace else torch.empty_like(x)
    b, c = x.shape[0], x.shape[1]
    with torch.cuda.device(x.device), _Timed('prelu_channels', float(x.numel()), 8.0 * x.numel(), f'B{b} C{c}'):
        st = _lib.load().ia_prelu_channels(_p(x), _p(slopes), _p(y), b, c, x.numel() // (b * c), _lib.stream_ptr(x.device))
    _lib.check(st, 'ia_prelu_channels')
    return y


def conv3x3_small(x, wk, in_scale=None, in_shift=None, out_scale=None, out_shift=None, slopes=None):
    """ia_conv3x3_small: 3x3 stride-1 padding-1 convolution of fp32 [B,I,h,w] with h, w < 8; wk = pack_conv_weight(w) [9,I,O].  in_scale /
    in_shift [I]: an affine map per input channel applied before the zero padding; out_scale / out_shift / slopes [O]: the epilogue."""
    _f32c(x, 'x'), _f32c(wk, 'wk')
    if x.dim() != 4 or wk.dim() != 3 or wk.shape[0] != 9 or wk.shape[1] != x.shape[1] or wk.device != x.device:
        raise RuntimeError(f'conv3x3_small: x [B,I,h,w] and wk [9,I,O] on one device, got {tuple(x.shape)} and {tuple(wk.shape)}')
    b, i, h, w = x.shape
    o = wk.shape[2]
    if (in_scale is None) != (in_shift is None):
        raise RuntimeError('conv3x3_small: in_scale and in_shift come together')
    for name, t, n in (('in_scale', in_scale, i), ('in_shift', in_shift, i), ('out_scale', out_scale, o), ('out_shift', out_shift, o),
                       ('slopes', slopes, o)):
        if t is not None and (_f32c(t, name).numel() != n or t.device != x.device):
            raise RuntimeError(f'conv3x3_small: {name} has {t.numel()} elements, expected {n}')
    scratch, nbytes = _scratch('ia_conv3x3_small_scratch_bytes', b, i, o, h, w, dtype=torch.float32, device=x.device)
    y = torch.empty(b, o, h, w, device=x.device, dtype=torch.float32)
    with torch.cuda.device(x.device), _Timed('conv3x3_small', 18.0 * b * h * w * i * o, 4.0 * (x.numel() + wk.numel() + y.numel()), f'B{b} I{i} O{o} {h}x{w}'):
        st = _lib.load().ia_conv3x3_small(_p(x), _p(wk), _p(in_scale), _p(in_shift), _p(out_scale), _p(out_shift), _p(slopes), _p(y), _p(scratch),
                                          nbytes, b, i, o, h, w, _lib.stream_ptr(x.device))
    _lib.check(st, 'ia_conv3x3_small')
    return y


def id_head(x, wt, bias=None, scale=None, shift=None):
    """ia_id_head: x fp32 [B,K] (or [B,C,h,w], flattened), wt [O,K] -> float32 [B,O], ((wt x + bias) * scale + shift) l2-normalised."""
    _f32c(x, 'x'), _f32c(wt, 'wt')
    x2 = x.reshape(x.shape[0], -1)
    if wt.dim() != 2 or wt.shape[1] != x2.shape[1] or wt.device != x.device or x2.shape[0] < 1:
        raise RuntimeError(f'id_head: x [B,K] and wt [O,K] on one device, got {tuple(x.shape)} and {tuple(wt.shape)}')
    b, k = x2.shape
    o = wt.shape[0]
    for name, t in (('bias', bias), ('scale', scale), ('shift', shift)):
        if t is not None and (_f32c(t, name).numel() != o or t.device != x.device):
            raise RuntimeError(f'id_head: {name} has {t.numel()} elements, expected {o}')
    scratch, nbytes = _scratch('ia_id_head_scratch_bytes', b, k, o, dtype=torch.float32, device=x.device)
    out = torch.empty(b, o, device=x.device, dtype=torch.float32)
    with torch.cuda.device(x.device), _Timed('id_head', 2.0 * b * k * o, 4.0 * (x.numel() + wt.numel() + out.numel()), f'B{b} K{k} O{o}'):
        st = _lib.load().ia_id_head(_p(x2), _p(wt), _p(bias), _p(scale), _p(shift), _p(out), _p(scratch), nbytes, b, k, o, _lib.stream_ptr(x.device))
    _lib.check(st, 'ia_id_head')
    return out


def id_similarity(f, out=None):
    """ia_id_similarity: f fp32 [2N,D] -> float32 [N], rows n and N + n dotted; `out`: a float32 [N] view (any positive stride) to write into."""
    _f32c(f, 'f')
    if f.dim() != 2 or f.shape[0] % 2 or f.shape[0] < 2 or f.shape[1] < 1:
        raise RuntimeError(f'id_similarity: f must be [2N,D], got {tuple(f.shape)}')
    n, d = f.shape[0] // 2, f.shape[1]
    if out is None:
        out = torch.empty(n, device=f.device, dtype=torch.float32)
    if not (out.is_cuda and out.device == f.device and out.dtype == torch.float32 and out.dim() == 1 and out.shape[0] == n
            and (n == 1 or out.stride(0) >= 1)):
        raise RuntimeError('id_similarity: out must be a float32 [N] device view with a positive stride')
    with torch.cuda.device(f.device), _Timed('id_similarity', 2.0 * f.numel(), 4.0 * f.numel(), f'N{n} D{d}'):
        st = _lib.load().ia_id_similarity(_p(f), n, d, _p(out), max(int(out.stride(0)), 1), _lib.stream_ptr(f.device))
    _lib.check(st, 'ia_id_similarity')
    return out


# ------------------------------------------------------------------ contextual loss (csrc/contextual.hip)

def resize_bilinear(images, size, general=False):
    """ia_resize_bilinear: float32 [N,C,H,W] or uint8 [N,H,W,C] (read as v / 127.5 - 1) -> float32 [N,C,OH,OW], what
    F.interpolate(mode='bilinear', align_corners=False) gives.  `general`: take the general path where the exact 2 : 1 branch applies."""
    if not (torch.is_tensor(images) and images.is_cuda and images.is_contiguous() and images.dim() == 4
            and images.dtype in (torch.float32, torch.uint8)):
        raise RuntimeError('resize_bilinear: a contiguous float32 [N,C,H,W] or uint8 [N,H,W,C] device tensor')
    u8 = images.dtype == torch.uint8
    n, c, h, w = (images.shape[0], images.shape[3], images.shape[1], images.shape[2]) if u8 else images.shape
    oh, ow = int(size[0]), int(size[1])
    if min(n, c, h, w, oh, ow) < 1:
        raise RuntimeError(f'resize_bilinear: empty input or output ({tuple(images.shape)} -> {oh} x {ow})')
    y = torch.empty(n, c, oh, ow, device=images.device, dtype=torch.float32)
    with torch.cuda.device(images.device), _Timed('resize_bilinear', 7.0 * y.numel(), float(images.numel() * images.element_size() + 4 * y.numel()),
                                                  f'N{n} C{c} {h}x{w}->{oh}x{ow}'):
        st = _lib.load().ia_resize_bilinear(_p(images), 1 if u8 else 0, _p(y), n, c, h, w, oh, ow, int(bool(general)), _lib.stream_ptr(images.device))
    _lib.check(st, 'ia_resize_bilinear')
    return y


def cx_layout():
    """(tile, k_step) of the contextual head: rows / columns per workgroup, and the multiple the channel count is padded to."""
    tile, step = ctypes.c_int(0), ctypes.c_int(0)
    _lib.check(_lib.load().ia_cx_layout(ctypes.byref(tile), ctypes.byref(step)), 'ia_cx_layout')
    return tile.value, step.value


def cx_scratch_bytes(n, c, p):
    nbytes = ctypes.c_size_t(0)
    _lib.check(_lib.load().ia_cx_scratch_bytes(int(n), int(c), int(p), ctypes.byref(nbytes)), 'ia_cx_scratch_bytes')
    return nbytes.value


def cx_head(fx, fy, band_width=0.5, mu='frame', debug=False):
    """The contextual head on fp32 maps fx, fy [N,C,h,w] -> (cx [N], cx_loss [N]) float32: ia_cx_channel_mean, ia_cx_normalize (twice),
    ia_cx_rows, ia_cx_cols, ia_cx_finish.  mu: 'frame' (a frame's own channel means of fy), 'batch' (the batch's), or a float32 [1,C] /
    [N,C] table.  debug: also a dict with mu, the operands xh / yh [N,P,Cpad], m [N,P] float32, s and colmax [N,P] float64."""
    _f32c(fx, 'fx'), _f32c(fy, 'fy')
    if fx.dim() != 4 or fx.shape != fy.shape or fx.device != fy.device or fx.numel() == 0:
        raise RuntimeError(f'cx_head: two float32 [N,C,h,w] maps of one shape on one device, got {tuple(fx.shape)} and {tuple(fy.shape)}')
    n, c, h, w = fx.shape
    p = h * w
    _, step = cx_layout()
    cpad = -(-c // step) * step
    dev = fx.device
    lib, stream = _lib.load(), _lib.stream_ptr(dev)
    scratch = torch.empty(-(-cx_scratch_bytes(n, c, p) // 8), dtype=torch.float64, device=dev)
    mean64, s, colmax = scratch[:n * c], scratch[n * c:n * c + n * p], scratch[n * c + n * p:n * c + 2 * n * p]
    m = scratch[n * c + 2 * n * p:].view(torch.float32)[:n * p]
    xh = torch.empty(n, p, cpad, device=dev, dtype=torch.float32)
    yh = torch.empty(n, p, cpad, device=dev, dtype=torch.float32)
    cx = torch.empty(n, device=dev, dtype=torch.float32)
    loss = torch.empty(n, device=dev, dtype=torch.float32)
    with torch.cuda.device(dev):
        if torch.is_tensor(mu):
            table = _f32c(mu, 'mu')
            if table.dim() != 2 or table.shape[1] != c or table.shape[0] not in (1, n) or table.device != dev:
                raise RuntimeError(f'cx_head: mu must be float32 [1,C] or [N,C] on the maps\' device, got {tuple(table.shape)}')
        elif mu in ('frame', 'batch'):
            frames = torch.empty(n, c, device=dev, dtype=torch.float32)
            batch = torch.empty(1, c, device=dev, dtype=torch.float32) if mu == 'batch' else None
            with _Timed('cx_channel_mean', float(fy.numel()), 4.0 * fy.numel(), f'N{n} C{c} P{p}'):
                st = lib.ia_cx_channel_mean(_p(fy), n, c, p, _p(mean64), _p(frames), _p(batch), stream)
            _lib.check(st, 'ia_cx_channel_mean')
            table = batch if mu == 'batch' else frames
        else:
            raise RuntimeError(f"cx_head: mu must be 'frame', 'batch' or a table, got {mu!r}")
        for src, dst in ((fx, xh), (fy, yh)):
            with _Timed('cx_normalize', 4.0 * src.numel(), 12.0 * src.numel(), f'N{n} C{c} P{p}'):
                st = lib.ia_cx_normalize(_p(src), _p(table), table.shape[0], _p(dst), n, c, p, cpad, stream)
            _lib.check(st, 'ia_cx_normalize')
        with _Timed('cx_rows', 4.0 * n * p * p * cpad, 8.0 * n * p * cpad, f'N{n} C{c} P{p}'):
            st = lib.ia_cx_rows(_p(xh), _p(yh), n, p, cpad, float(band_width), _p(m), _p(s), stream)
        _lib.check(st, 'ia_cx_rows')
        with _Timed('cx_cols', 2.0 * n * p * p * cpad, 8.0 * n * p * cpad, f'N{n} C{c} P{p}'):
            st = lib.ia_cx_cols(_p(xh), _p(yh), _p(m), _p(s), n, p, cpad, float(band_width), _p(colmax), stream)
        _lib.check(st, 'ia_cx_cols')
        with _Timed('cx_finish', float(n * p), 8.0 * n * p, f'N{n} P{p}'):
            st = lib.ia_cx_finish(_p(colmax), n, p, _p(cx), _p(loss), stream)
        _lib.check(st, 'ia_cx_finish')
    if debug:
        return cx, loss, {'mu': table, 'xh': xh, 'yh': yh, 'm': m.reshape(n, p).clone(), 's': s.reshape(n, p).clone(),
                          'colmax': colmax.reshape(n, p).clone()}
    return cx, loss


# ------------------------------------------------------------------ distribution scores (csrc/distribution.hip)

MOMENTS_MAX_D = 4096         # csrc/distribution.hip kMomMaxD
KNN_MAX_K = 15               # csrc/distribution.hip kPrMaxK


def _features_checked(x, what):
    _f32c(x, what)
    if x.dim() != 2 or x.shape[1] < 1:
        raise RuntimeError(f'{what} must be [rows, D] with D >= 1, got {tuple(x.shape)}')
    return x


def feature_moments(x, raw_sum, raw_cov):
    """ia_feature_moments: adds the column sums and the second moments x^T x of the chunk x (float32 [n,D], D <= 4096) into the running
    float64 device tensors raw_sum [D] and raw_cov [D,D], in place."""
    _features_checked(x, 'x')
    n, d = x.shape
    if d > MOMENTS_MAX_D:
        raise ValueError(f'feature_moments takes at most {MOMENTS_MAX_D} features, got {d}')
    _f64c(raw_sum, 'raw_sum', (d,)), _f64c(raw_cov, 'raw_cov', (d, d))
    if not (raw_sum.device == raw_cov.device == x.device):
        raise RuntimeError('feature_moments: x, raw_sum and raw_cov must be on one device')
    if n == 0:
        return
    with torch.cuda.device(x.device), _Timed('feature_moments', float(n) * d * (d + 1), 4.0 * n * d + 16.0 * d * d, f'n={n} D={d}'):
        st = _lib.load().ia_feature_moments(_p(x), n, d, _p(raw_sum), _p(raw_cov), _lib.stream_ptr(x.device))
    _lib.check(st, 'ia_feature_moments')


def kid_subsets(gen, real, idx_gen, idx_real):
    """ia_kid_subsets: gen [Ng,D], real [Nr,D] float32 on the device; idx_gen, idx_real integer [S,m] arrays ON THE HOST (NumPy or CPU
    tensors: they are checked against Ng / Nr here, where that costs no synchronisation) -> float64 device tensor [S,3]."""
    _features_checked(gen, 'gen'), _features_checked(real, 'real')
    if gen.shape[1] != real.shape[1] or gen.device != real.device:
        raise RuntimeError(f'kid_subsets: gen and real must share D and the device, got {tuple(gen.shape)} and {tuple(real.shape)}')
    ig, ir = torch.as_tensor(idx_gen), torch.as_tensor(idx_real)
    if ig.is_cuda or ir.is_cuda or ig.dim() != 2 or ig.shape != ir.shape or ig.is_floating_point() or ir.is_floating_point():
        raise RuntimeError('kid_subsets: idx_gen and idx_real must be host integer arrays of one shape [S,m]')
    s, m = ig.shape
    if m < 1:
        raise ValueError('kid_subsets: a subset needs at least one row')
    out = torch.empty(s, 3, dtype=torch.float64, device=gen.device)
    if s == 0:
        return out
    if int(ig.min()) < 0 or int(ig.max()) >= gen.shape[0] or int(ir.min()) < 0 or int(ir.max()) >= real.shape[0]:
        raise ValueError(f'kid_subsets: an index is outside its set ({gen.shape[0]} generated, {real.shape[0]} real rows)')
    ig = ig.to(torch.int32).contiguous().to(gen.device, non_blocking=True)
    ir = ir.to(torch.int32).contiguous().to(gen.device, non_blocking=True)
    d = gen.shape[1]
    with torch.cuda.device(gen.device), _Timed('kid_subsets', 6.0 * s * m * m * d, 8.0 * s * m * d, f'S={s} m={m} D={d}'):
        st = _lib.load().ia_kid_subsets(_p(gen), _p(real), d, _p(ig), _p(ir), s, m, _p(out), _lib.stream_ptr(gen.device))
    _lib.check(st, 'ia_kid_subsets')
    return out


def knn_radius(feat, k):
    """ia_knn_radius: feat float32 [N,D] -> float32 [N], the squared distance from each row to its (k + 1)-th nearest row, itself included."""
    _features_checked(feat, 'feat')
    n, d = feat.shape
    k = int(k)
    if not 0 <= k <= KNN_MAX_K:
        raise ValueError(f'knn_radius: k must be in [0, {KNN_MAX_K}], got {k}')
    if n <= k:
        raise ValueError(f'knn_radius: {n} rows have no neighbour number {k}')
    r2 = torch.empty(n, dtype=torch.float32, device=feat.device)
    with torch.cuda.device(feat.device), _Timed('knn_radius', 3.0 * n * n * d, 4.0 * n * d, f'N={n} D={d} k={k}'):
        st = _lib.load().ia_knn_radius(_p(feat), n, d, k, _p(r2), _lib.stream_ptr(feat.device))
    _lib.check(st, 'ia_knn_radius')
    return r2


def manifold_covered(probes, manifold, r2):
    """ia_manifold_covered: probes [P,D], manifold [N,D], r2 [N] float32 -> bool [P]: the probe lies within some manifold row's radius."""
    _features_checked(probes, 'probes'), _features_checked(manifold, 'manifold'), _f32c(r2, 'r2')
    if probes.shape[1] != manifold.shape[1] or tuple(r2.shape) != (manifold.shape[0],) or manifold.shape[0] < 1 \
            or not (probes.device == manifold.device == r2.device):
        raise RuntimeError(f'manifold_covered: probes [P,D], manifold [N,D] (N >= 1) and r2 [N] on one device, got {tuple(probes.shape)}, '
                           f'{tuple(manifold.shape)}, {tuple(r2.shape)}')
    p, d = probes.shape
    n = manifold.shape[0]
    covered = torch.zeros(p, dtype=torch.uint8, device=probes.device)
    if p == 0:
        return covered.bool()
    with torch.cuda.device(probes.device), _Timed('manifold_covered', 3.0 * p * n * d, 4.0 * (p + n) * d, f'P={p} N={n} D={d}'):
        st = _lib.load().ia_manifold_covered(_p(probes), p, _p(manifold), _p(r2), n, d, _p(covered), _lib.stream_ptr(probes.device))
    _lib.check(st, 'ia_manifold_covered')
    return covered.bool()
