"""Plain-torch restatements of the resampling family (csrc/upfirdn2d.hip, csrc/filtered_lrelu.hip), the seeded case tables that
tests/test_resample_reference_cpu.py and tests/test_resample_gpu.py share, and a restatement of the dispatch of upfirdn2d.hip
(``expected_form``) that lets the tables be checked for coverage without a device.  No device code.

Every restatement computes in the dtype of its arguments: with float64 tensors it is the reference ``r``, with float32 tensors it is
the yardstick, whose own distance to float64 on the same inputs is ``e32 = max|restatement in float32 - r|``.  The tolerance rule,
per element of a kernel result:

    float32 storage:  |got - r| <= 4 * e32 + 2^-24 * max|r|
    float16 storage:  the same + 2^-11 * |r|      (computed in float32 from the fp16-rounded inputs, rounded once)
    float64 storage:  |got - r| <= 1e-12 * max|r|

The factor 4 covers another, equally valid summation order and fused multiply-adds.  Where two kernels are documented to give the same
bits the tests assert ``torch.equal`` instead.

Restatements take ``wrong=<name>`` (WRONG_FIR, WRONG_TAIL, WRONG_SPLIT, WRONG_FLR): the plausible errors of such kernels, written out
so that the CPU test can show that the tables tell each of them from the right result by at least ten times the tolerance, on every
case the error can show on (``wrong_applies``).

Definitions restated:
  upfirdn2d (header of csrc/upfirdn2d.hip):  U = x with up - 1 zeros after every sample, padded (negative: cropped) by pad;
      out[oy, ox] = gain * sum_k K[ky, kx] * U[oy * down + ky, ox * down + kx];  K = f flipped in both axes unless `flip`
  fused tail (struct Tail):  clamp((lrelu or identity)(FIR + noise[oy, ox] * strength + bias[c]) * gain); the clamp keeps a NaN
  split pair (ia::split_f16):  v = t * styles_next saturated at +-65504;  hi = fp16(v), 0 below 2^-14;  lo = fp16((v - hi) * 2^11)
  filtered_lrelu (header of csrc/filtered_lrelu.hip):  t = upfirdn2d(x + b, fu, up, pad, gain = up^2);
      t = clamp(lrelu(t, slope) * gain);  y = upfirdn2d(t, fd, down)
"""
import itertools
import zlib
from typing import NamedTuple, Optional

import numpy as np
import torch

F64 = torch.float64
EPS32 = 2.0 ** -24
EPS16 = 2.0 ** -11
DTYPES = {'f32': torch.float32, 'f16': torch.float16, 'f64': torch.float64}


# ------------------------------------------------------------------ tolerances

def tolerance(ref, e32, dtype='f32'):
    """Per-element bound of a kernel result stored as `dtype` against the float64 reference `ref` (see the module docstring)."""
    top = float(ref.abs().max())
    if dtype == 'f64':
        return torch.full_like(ref, 1e-12 * top)
    bound = torch.full_like(ref, 4.0 * float(e32) + EPS32 * top)
    return bound + EPS16 * ref.abs() if dtype == 'f16' else bound


def e32_of(fn, ref, *args, **kw):
    """max|fn in float32 - ref| with every floating tensor argument cast to float32."""
    cast = lambda t: t.float() if torch.is_tensor(t) and t.is_floating_point() else t      # noqa: E731
    got = fn(*[cast(a) for a in args], **{k: cast(v) for k, v in kw.items()})
    return float((got.double() - ref).abs().max())


# ------------------------------------------------------------------ upfirdn2d

def _pair(v):
    return (int(v), int(v)) if isinstance(v, int) else (int(v[0]), int(v[1]))


def _pad4(pad):
    if isinstance(pad, int):
        return (pad,) * 4
    return tuple(int(p) for p in pad) if len(pad) == 4 else (int(pad[0]), int(pad[0]), int(pad[1]), int(pad[1]))


def _taps(f, dtype, gain, flip):
    """Correlation taps K [fh, fw] in `dtype`: f (2-D, or 1-D taps applied along both axes) times gain, flipped unless `flip`.  The gain
    meets the float32 taps in float32, as in the kernels and in the reference's definition (sqrt(gain) per pass of a 1-D filter)."""
    if f.ndim == 1:
        k = (f * gain ** 0.5).to(dtype)
        k = k[:, None] * k[None, :]
    else:
        k = (f * gain).to(dtype)
    return k if flip else k.flip(0, 1)


def _canvas(x, up, pad, wrong=None, outside=None):
    """U of the definition, [N, C, H*uy + py0 + py1, W*ux + px0 + px1].  `outside` [C]: the value of samples outside the image (None = 0)."""
    (ux, uy), (px0, px1, py0, py1) = up, pad
    n, c, h, w = x.shape
    hh, ww = h * uy + py0 + py1, w * ux + px0 + px1
    assert hh >= 1 and ww >= 1
    ex, ey = max(abs(px0), abs(px1)) + 2, max(abs(py0), abs(py1)) + 2          # samples added on every side
    xe = x.new_zeros(n, c, h + 2 * ey, w + 2 * ex)
    if outside is not None:
        xe = xe + outside[None, :, None, None]
    xe[:, :, ey:ey + h, ex:ex + w] = x
    if wrong == 'edge_clamp':                           # reads past the right / bottom edge return the edge sample
        xe[:, :, ey:ey + h, ex + w:] = x[:, :, :, -1:]
        xe[:, :, ey + h:, :] = xe[:, :, ey + h - 1:ey + h, :].clone()
    z = x.new_zeros(n, c, (h + 2 * ey) * uy, (w + 2 * ex) * ux)
    z[:, :, (uy - 1 if wrong == 'phase' else 0)::uy, ::ux] = xe          # 'phase': ky0 taken for by + 1
    if wrong == 'pad_order':                            # the pad taken in input samples: applied before the zero insertion
        py0, px0 = py0 * uy, px0 * ux
    y0, x0 = ey * uy - py0, ex * ux - px0
    return z[:, :, y0:y0 + hh, x0:x0 + ww]


def _correlate(u, k, down):
    dx, dy = down
    fh, fw = k.shape
    oh, ow = (u.shape[2] - fh + dy) // dy, (u.shape[3] - fw + dx) // dx
    assert oh >= 1 and ow >= 1
    out = u.new_zeros(u.shape[0], u.shape[1], oh, ow)
    for ky in range(fh):
        for kx in range(fw):
            out = out + k[ky, kx] * u[:, :, ky:ky + (oh - 1) * dy + 1:dy, kx:kx + (ow - 1) * dx + 1:dx]
    return out


def upfirdn2d(x, f, up=1, down=1, pad=0, flip=False, gain=1.0, wrong=None, outside=None):
    """x [N, C, H, W]; f [fh, fw] or [taps]; up, down: int or (x, y); pad: int, (x, y) or (x0, x1, y0, y1)."""
    if wrong == 'no_flip':
        flip = not flip
    return _correlate(_canvas(x, _pair(up), _pad4(pad), wrong, outside), _taps(f, x.dtype, gain, flip), _pair(down))


WRONG_FIR = ('no_flip', 'phase', 'pad_order', 'edge_clamp')


def wrong_applies(wrong, up=(1, 1), pad=(0, 0, 0, 0), tail=None, in_w=None, out_w=None):
    """Whether the error `wrong` can show at all on a case: a phase error needs zeros to insert, the pad order a pad and a rate, the
    clamped edge taps beyond the right or bottom edge, the misplaced lrelu a negative gain (lrelu(t) * g = lrelu(t * g) for g > 0)."""
    (ux, uy), (px0, px1, py0, py1) = _pair(up), _pad4(pad)
    if wrong == 'phase':
        return uy > 1
    if wrong == 'pad_order':
        return (ux > 1 and px0 != 0) or (uy > 1 and py0 != 0)
    if wrong == 'edge_clamp':
        return px1 > 0 or py1 > 0
    if wrong == 'noise_in_width':
        return tail.noise and in_w != out_w
    if wrong == 'lrelu_after_gain':
        return tail.act == 'lrelu' and tail.gain < 0
    return True


# ------------------------------------------------------------------ fused tail, split pair

def implied_pad(in_hw, out_hw, up, pad0, fshape=(4, 4)):
    """(px0, px1, py0, py1) of a call that names its output size and leading pads (pad0 = (px0, py0)), as the fused-tail entries do."""
    (h, w), (oh, ow), (px0, py0), (fh, fw) = in_hw, out_hw, pad0, fshape
    return (px0, ow - w * up - px0 + fw - 1, py0, oh - h * up - py0 + fh - 1)


def fir_tail(x, f, out_hw, up=1, pad0=(1, 1), fir_gain=1.0, noise=None, noise_strength=None, bias=None, act='linear', alpha=0.2,
             act_gain=1.0, clamp=None, flip=False, wrong=None):
    """The FIR, + noise [out_h * out_w] * strength ([1]; None = 1), + bias [C], lrelu or linear, * gain, clamp (which keeps a NaN)."""
    oh, ow = out_hw
    fir_wrong = wrong if wrong in WRONG_FIR else None
    v = upfirdn2d(x, f, up, 1, implied_pad(x.shape[2:], out_hw, up, pad0, tuple(f.shape)), flip, fir_gain, fir_wrong)
    assert tuple(v.shape[2:]) == (oh, ow)
    if noise is not None:
        nz = noise.reshape(-1)
        if wrong == 'noise_in_width':
            idx = (torch.arange(oh)[:, None] * x.shape[3] + torch.arange(ow)[None, :]) % (oh * ow)
            nz = nz[idx.reshape(-1)]
        v = v + nz.reshape(oh, ow) * (1.0 if noise_strength is None else noise_strength.reshape(()))
    if bias is not None:
        v = v + bias[None, :, None, None]
    if wrong == 'lrelu_after_gain':
        v = v * act_gain
    if act == 'lrelu':
        v = torch.where(v > 0, v, v * alpha)
    if wrong != 'lrelu_after_gain':
        v = v * act_gain
    return v if clamp is None else v.clamp(-clamp, clamp)


WRONG_TAIL = WRONG_FIR + ('noise_in_width', 'lrelu_after_gain')


def split_pair(v, styles_next=None, planes=2, wrong=None):
    """The fp16 pair the kernels must store: hi = fp16(t) (0 below the normal range), lo = fp16((t - hi) * 2^11), t = v * styles_next [B, C]
    saturated.  planes = 1: (fp16(t), None), the saturated value rounded once."""
    t = (v if styles_next is None else v * styles_next[:, :, None, None]).clamp(-65504.0, 65504.0)
    if planes == 1:
        return t.half(), None
    hi = torch.where(t.abs() < 6.103515625e-5, torch.zeros_like(t), t).half()
    lo = ((t - hi.float()) * (1024.0 if wrong == 'lo_scale' else 2048.0)).half()
    return hi, lo


WRONG_SPLIT = ('lo_scale',)


def pair_value(hi, lo):
    return hi.double() if lo is None else hi.double() + lo.double() / 2048.0


def split_bound(t):
    """22 mantissa bits: |pair - t| <= 2^-21 |t| + 2^-26."""
    return t.abs() * 2.0 ** -21 + 2.0 ** -26


def act_planes(data):
    """``SplitAct.data`` [b][plane][c/8][h][w][8] -> (hi, lo or None), each fp16 NCHW."""
    b, planes, c8, h, w, e = data.shape
    out = [data[:, p].permute(0, 1, 4, 2, 3).reshape(b, c8 * 8, h, w) for p in range(planes)]
    return out[0], (out[1] if planes == 2 else None)


# ------------------------------------------------------------------ filtered_lrelu

def filtered_lrelu(x, fu=None, fd=None, b=None, up=1, down=1, pad=0, gain=2 ** 0.5, slope=0.2, clamp=None, flip=False, wrong=None):
    one = torch.ones(1, 1)
    fir_wrong = wrong if wrong in WRONG_FIR else None
    outside = b if (wrong == 'bias_outside' and b is not None) else None       # the bias added to the zero padding as well
    t = x if b is None else x + b[None, :, None, None]
    t = upfirdn2d(t, one if fu is None else fu, up, 1, pad, flip, float(up * up), fir_wrong, outside)
    t = torch.where(t > 0, t, t * slope) * gain
    if clamp is not None:
        t = t.clamp(-clamp, clamp)
    return upfirdn2d(t, one if fd is None else fd, 1, down, 0, flip, 1.0, 'no_flip' if wrong == 'no_flip' else None)


WRONG_FLR = ('no_flip', 'phase', 'pad_order', 'edge_clamp', 'bias_outside')


# ------------------------------------------------------------------ seeded inputs

def _rs(*key):
    return np.random.RandomState(zlib.crc32(repr(key).encode()))


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).float()


_cache = {}


def _cached(fn):
    def get(*key):
        k = (fn.__name__,) + key
        if k not in _cache:
            _cache[k] = fn(*key)
        return _cache[k]
    return get


@_cached
def fir_filter(fh, fw=None):
    """float32 taps, all different and none small (0.25 .. 1.25 before the normalisation to sum 1): no symmetry hides a flip or a phase."""
    rs = _rs('filter', fh, fw)
    f = rs.rand(fh, fw) + 0.25 if fw else rs.rand(fh) + 0.25
    return _t(f / f.sum())


@_cached
def image(n, c, h, w, tag=0):
    return _t(_rs('image', n, c, h, w, tag).randn(n, c, h, w))


LAYOUTS = ('contiguous', 'every_second_channel', 'expanded_batch', 'channels_last')


def layout(t, kind):
    """A view with the values of t [N, C, H, W] (on t's device) in one of LAYOUTS; whatever else its storage holds is NaN.
    'expanded_batch' repeats batch element 0 with stride 0: ``layout_values`` gives the values such a view holds."""
    if kind == 'contiguous':
        return t.contiguous()
    if kind == 'channels_last':
        return t.contiguous(memory_format=torch.channels_last)
    if kind == 'expanded_batch':
        return t[:1].contiguous().expand(t.shape[0], -1, -1, -1)
    assert kind == 'every_second_channel'
    big = torch.full((t.shape[0], 2 * t.shape[1], *t.shape[2:]), float('nan'), device=t.device, dtype=t.dtype)
    view = big[:, ::2]
    view.copy_(t)
    return view


def layout_values(t, kind):
    return t[:1].expand_as(t).contiguous() if kind == 'expanded_batch' else t


# ------------------------------------------------------------------ case tables: ia_upfirdn2d

class Fir(NamedTuple):
    """One call of upfirdn2d(x, f, up, down, pad, flip, gain): x = image(*shape) as `dtype` in `layout`, f = fir_filter(*fshape)
    (`f_transposed`: built as [fw, fh] and passed as its .t() view)."""
    name: str
    shape: tuple
    fshape: tuple
    up: tuple = (1, 1)
    down: tuple = (1, 1)
    pad: tuple = (0, 0, 0, 0)
    flip: bool = False
    gain: float = 1.0
    dtype: str = 'f32'
    layout: str = 'contiguous'
    f_transposed: bool = False

    @property
    def out_hw(self):
        (n, c, h, w), (fh, fw), (ux, uy), (dx, dy), (px0, px1, py0, py1) = self.shape, self.fshape, self.up, self.down, self.pad
        return (h * uy + py0 + py1 - fh + dy) // dy, (w * ux + px0 + px1 - fw + dx) // dx


def fir_inputs(case):
    """(x float32 NCHW with the values the call sees -- fp16-rounded for 'f16' --, f float32 [fh, fw] (a .t() view when `f_transposed`))."""
    x = layout_values(image(*case.shape), case.layout)
    if case.dtype == 'f16':
        x = x.half().float()
    f = fir_filter(case.fshape[1], case.fshape[0]).t() if case.f_transposed else fir_filter(*case.fshape)
    return x, f


def fir_reference(case, wrong=None, dtype=F64):
    x, f = fir_inputs(case)
    return upfirdn2d(x.to(dtype), f, case.up, case.down, case.pad, case.flip, case.gain, wrong)


TILE_W, TILE_H, PIPE_TILES = 64, 16, 4
TILED_OUT_W, TILED_OUT_H, TILED_PADS = (1, 63, 64, 65), (1, 15, 16, 17), (-3, 0, 1, 2, 5)


def _sized(out, up, p0, taps=4):
    """(input size, trailing pad) that give `out` outputs behind the leading pad p0, with one or two padded samples at the far edge
    whenever an input of at least one sample allows it."""
    n = max(1, (out + taps - 1 - p0 - 1) // up)
    return n, out + taps - 1 - p0 - n * up


def tiled_case(up, out_h, out_w, px0, py0, flip, dtype='f32', planes=(1, 2)):
    (w, px1), (h, py1) = _sized(out_w, up, px0), _sized(out_h, up, py0)
    return Fir(f'up{up} {out_h}x{out_w} pad0=({px0},{py0}) flip={int(flip)} {dtype}', (*planes, h, w), (4, 4), (up, up), (1, 1), (px0, px1, py0, py1),
               flip, float(up * up), dtype)


def _tiled_table(up, dtype):
    """20 of the 4 x 4 x 25 x 2 combinations: every width, height, pad per axis and flip occurs, px0 != py0 throughout, and every width
    meets every height (i % 4 against i // 4 % 4 over 16 cases; the last four repeat the ragged sizes with the remaining pads)."""
    cases = []
    for i in range(20):
        out_w, out_h = TILED_OUT_W[i % 4], TILED_OUT_H[(i // 4 + (3 if i >= 16 else 0)) % 4]
        px0 = TILED_PADS[i % 5]
        py0 = TILED_PADS[(i + 1 + i // 5) % 5]
        if out_w == 1 and px0 == 5:                     # (one output behind a pad wider than the filter sees no sample)
            px0 = 0 if py0 != 0 else 1
        if out_h == 1 and py0 == 5:
            py0 = 0 if px0 != 0 else 1
        cases.append(tiled_case(up, out_h, out_w, px0, py0, bool((i + i // 4) % 2), dtype))
    return tuple(cases)


TILED_CASES = {(up, dtype): _tiled_table(up, dtype) for up in (1, 2) for dtype in ('f32', 'f16')}

# (out_w, out_h).  The pipelined kernel takes up = 1 calls of at least 64 tiles, a multiple of 4 of them: 65 x 509 is 2 x 32 tiles (every
# workgroup's four tiles span two tile rows), 250 x 256 is 4 x 16, 130 x 380 is 3 x 24 (a workgroup's tiles wrap in the middle of a row).
# 256 x 64 and 130 x 250 have 16 and 48 tiles: several tile rows and columns of the one-tile kernel.
PIPE_OUT_WH = ((65, 509), (250, 256), (130, 380))
MULTI_TILE_OUT_WH = ((256, 64), (130, 250))
PIPE_PADS = ((1, 1), (-3, 2), (5, 0), (2, -3), (0, 5))           # (px0, py0)


def _pipe_table(sizes):
    cases = []
    for i, ((out_w, out_h), dtype) in enumerate(itertools.product(sizes, ('f32', 'f16'))):
        for j in range(2):
            px0, py0 = PIPE_PADS[(i + 2 * j) % 5]
            cases.append(tiled_case(1, out_h, out_w, px0, py0, bool((i + j) % 2), dtype, planes=(1, 2)))
    return tuple(cases)


PIPE_CASES = _pipe_table(PIPE_OUT_WH)
MULTI_TILE_CASES = _pipe_table(MULTI_TILE_OUT_WH)

MIXED = dict(up=(2, 3), down=(3, 2), pad=(2, -1, 0, 3), flip=True, gain=1.5)         # the geometry of golden upfirdn2d/mixed
GENERIC_CASES = (
    Fir('mixed', (2, 3, 10, 9), (3, 5), **MIXED),
    Fir('mixed f16', (2, 3, 10, 9), (3, 5), dtype='f16', **MIXED),
    Fir('mixed f64', (2, 3, 10, 9), (3, 5), dtype='f64', **MIXED),
    Fir('up (3,1) down (1,4)', (1, 2, 9, 14), (5, 3), (3, 1), (1, 4), (1, 2, 3, 0), False, 2.0),
    Fir('filter 1x7', (1, 2, 6, 11), (1, 7), (2, 1), (1, 1), (3, 4, 0, 0), False, 2.0),
    Fir('filter 32x32', (1, 1, 20, 18), (32, 32), (1, 1), (1, 1), (16, 17, 15, 16), False, 1.0),
    Fir('filter 32x32 up 2 flip', (1, 2, 9, 11), (32, 32), (2, 2), (1, 1), (16, 15, 17, 14), True, 4.0),
    Fir('filter 5x3', (2, 2, 8, 7), (5, 3), (1, 2), (2, 1), (1, 1, 2, 3), True, 1.0),
    Fir('transposed filter view', (1, 2, 8, 7), (5, 3), (2, 1), (1, 2), (2, 0, 1, 3), False, 1.0, f_transposed=True),
    Fir('x[:, ::2], tiled-shaped', (2, 3, 7, 9), (4, 4), (2, 2), (1, 1), (2, 1, 2, 1), False, 4.0, layout='every_second_channel'),
    Fir('expanded batch, tiled-shaped', (3, 2, 9, 8), (4, 4), (1, 1), (1, 1), (1, 1, 1, 1), True, 1.0, layout='expanded_batch'),
    Fir('channels-last C = 1', (2, 1, 7, 9), (4, 4), (2, 2), (1, 1), (2, 1, 2, 1), False, 4.0, layout='channels_last'),
    Fir('channels-last C = 5', (2, 5, 7, 9), (4, 4), (2, 2), (1, 1), (2, 1, 2, 1), True, 4.0, layout='channels_last'),
    Fir('channels-last C = 5 f16 down 2', (1, 5, 12, 10), (4, 4), (1, 1), (2, 2), (1, 1, 1, 1), False, 1.0, 'f16', 'channels_last'),
    Fir('output 1x1', (1, 2, 3, 4), (3, 4), (1, 1), (1, 1), (0, 0, 0, 0), False, 1.0),
    Fir('output 1x1 down 5', (2, 1, 1, 1), (4, 4), (2, 2), (5, 5), (1, 1, 1, 1), True, 4.0),
    Fir('grid-stride loop', (1, 2, 520, 520), (3, 3), (1, 1), (1, 1), (0, 0, 0, 0), False, 1.0),          # 2 * 518^2 > 2048 * 256 outputs
    Fir('65537 planes, tiled-shaped', (1, 65537, 2, 3), (4, 4), (2, 2), (1, 1), (2, 1, 2, 1), False, 4.0),
)
GRID_STRIDE_OUTPUTS = 2048 * 256


def expected_form(case, entry='upfirdn2d', want_f32=False):
    """The kernel that csrc/upfirdn2d.hip launches for a call, restated from its dispatch: ``tiled_eligible`` (contiguous NCHW in and
    out, no decimation, one rate of 1 or 2, the 4 x 4 filter, 32-bit storage or narrower, at most 65535 planes), the pipe condition of
    ``launch_tiled`` (up 1, at least 64 tiles and a multiple of 4), the DMA condition of ``ia_fir_tail_split`` (no float32 copy, eight
    channel planes inside one buffer resource).  entry: 'upfirdn2d', 'bias_act' (same kernels with the tail) or 'split'."""
    n, c, h, w = case.shape
    if entry == 'split':
        return 'tail-register' if want_f32 or 8 * h * w * 4 >= 0x7ffffff0 else 'tail-dma'
    tiled = (case.layout == 'contiguous' and case.down == (1, 1) and case.up in ((1, 1), (2, 2)) and case.fshape == (4, 4) and n * c <= 65535
             and case.dtype != 'f64')
    if not tiled:
        return 'generic'
    oh, ow = case.out_hw
    tiles = -(-ow // TILE_W) * -(-oh // TILE_H)
    if case.up == (1, 1) and tiles % PIPE_TILES == 0 and tiles >= 64:
        return 'pipe'
    return f'tiled up{case.up[0]}'


def pipe_workgroup_spans_two_tile_rows(case):
    """Whether some workgroup of the pipelined kernel walks tiles of more than one tile row (tiles 4 g .. 4 g + 3, row = tile // tiles_x)."""
    return -(-case.out_hw[1] // TILE_W) % PIPE_TILES != 0


# ------------------------------------------------------------------ case tables: fused tail and ia_fir_tail_split

class Tail(NamedTuple):
    noise: bool = True
    strength: bool = True
    bias: bool = True
    clamp: Optional[float] = 0.4
    act: str = 'lrelu'
    alpha: float = 0.2
    gain: float = 2 ** 0.5

    def kwargs(self, t):
        """Keyword arguments of the hipops entries and of ``fir_tail`` from the tensors of ``tail_inputs``."""
        return dict(noise=t['noise'] if self.noise else None, noise_strength=t['strength'] if self.noise and self.strength else None,
                    bias=t['bias'] if self.bias else None, act=self.act, alpha=self.alpha, act_gain=self.gain, clamp=self.clamp)


# every combination of noise, bias, clamp and activation; then noise without a strength, another slope, and a negative gain (the one
# setting at which lrelu-then-gain and gain-then-lrelu differ)
TAIL_OPTIONS = tuple(Tail(noise=nz, bias=bi, clamp=cl, act=act) for nz, bi, cl, act in
                     itertools.product((False, True), (False, True), (None, 0.4), ('linear', 'lrelu'))) + (
    Tail(strength=False), Tail(alpha=0.05), Tail(alpha=0.7, clamp=None), Tail(gain=-1.5), Tail(gain=-0.75, clamp=None, noise=False), Tail(gain=-2.0, bias=False))
TAIL_FULL = Tail()


@_cached
def tail_inputs(c, out_h, out_w):
    """float32 {'noise' [out_h * out_w], 'strength' [1], 'bias' [C]}."""
    rs = _rs('tail', c, out_h, out_w)
    return {'noise': _t(rs.randn(out_h * out_w)), 'strength': _t([0.3]), 'bias': _t(rs.randn(c) * 0.5)}


# (up, (out_h, out_w), (px0, py0), flip, dtype) of the fused-tail calls that carry the option table: ragged single tiles and the pipe
FUSED_TAIL_GEOMETRY = ((1, (17, 65), (1, 1), False, 'f32'), (2, (17, 65), (2, 1), True, 'f32'), (1, (15, 63), (0, 2), True, 'f16'),
                       (2, (33, 70), (1, 2), False, 'f16'), (1, (509, 65), (2, 0), False, 'f32'))


def fused_tail_case(up, out_hw, pad0, flip, dtype, planes=(2, 3)):
    return tiled_case(up, out_hw[0], out_hw[1], pad0[0], pad0[1], flip, dtype, planes)


class Split(NamedTuple):
    """One call of hipops.fir_tail_split: out_hw, pad0 = (px0, py0), planes of the pair, channels, batch, the tail's options, whether
    styles_next is passed, and whether channel 1 is scaled to 1e-6 (hi is dropped, the value rides in lo)."""
    out_hw: tuple
    pad0: tuple
    planes: int
    c: int
    b: int
    tail: Tail = TAIL_FULL
    styles: bool = True
    tiny_channel: bool = False

    @property
    def fir(self):
        (oh, ow), (px0, py0) = self.out_hw, self.pad0
        return Fir(f'split {oh}x{ow} pad0={self.pad0}', (self.b, self.c, oh + 2 - py0, ow + 2 - px0), (4, 4), (1, 1), (1, 1), (px0, 1, py0, 1), False, 1.0)


SPLIT_OUT_HW, SPLIT_PAD0 = ((16, 64), (17, 65), (40, 100), (75, 91)), ((1, 1), (0, 2), (2, 0))
# every output size with every pad; planes, channels and batch alternate so that each value meets each size
SPLIT_GEOMETRY = tuple(Split(hw, p0, 1 + (i + j) % 2, (8, 24)[(i + j // 2) % 2], 1 + (i // 2 + j) % 2)
                       for i, hw in enumerate(SPLIT_OUT_HW) for j, p0 in enumerate(SPLIT_PAD0))
SPLIT_OPTIONS = tuple(Split((17, 65), (1, 1), 2, 8, 2, tail) for tail in TAIL_OPTIONS) + (
    Split((17, 65), (1, 1), 2, 8, 2, styles=False), Split((40, 100), (0, 2), 1, 8, 1, styles=False), Split((17, 65), (1, 1), 1, 8, 2, Tail(clamp=None, act='linear')),
    Split((17, 65), (1, 1), 2, 8, 2, Tail(noise=False), tiny_channel=True), Split((40, 100), (2, 0), 2, 24, 1, Tail(noise=False, bias=False, clamp=None, act='linear'), tiny_channel=True))


@_cached
def split_inputs(case):
    """float32 {'x' [B, C, in_h, in_w], 'f' [4, 4], 'noise', 'strength', 'bias', 'styles' [B, C]}.  With `tiny_channel` channel 1 of x and
    of the bias is scaled by 1e-6 (such cases carry no noise, which all channels share): its results lie below the fp16 normal range."""
    assert not (case.tiny_channel and case.tail.noise)
    fir = case.fir
    x = image(*fir.shape).clone()
    t = dict(tail_inputs(case.c, *case.out_hw))
    if case.tiny_channel:
        x[:, 1] *= 1e-6
        t['bias'] = t['bias'].clone()
        t['bias'][1] *= 1e-6
    styles = _t(_rs('styles', case.b, case.c).rand(case.b, case.c) + 0.5)
    return {'x': x, 'f': fir_filter(4, 4), 'styles': styles, **t}


# ------------------------------------------------------------------ case tables: ia_filtered_lrelu

class Flr(NamedTuple):
    name: str
    shape: tuple
    fu: Optional[int]       # taps of the 1-D up filter (None = absent)
    fd: Optional[int]
    up: int
    down: int
    pad: tuple
    slope: float = 0.2
    clamp: Optional[float] = 0.9
    flip: bool = False
    bias: bool = True
    dtype: str = 'f32'


FLR_OUT_W, FLR_OUT_H, FLR_RATES = (31, 32, 33), (7, 8, 9), ((2, 2), (1, 1), (4, 2))


def flr_case(out_w, out_h, up, down, px0, py0, fu=True, fd=True, **kw):
    nu, nd = (4 * up if fu else None), (2 * down + 2 if fd else None)
    size = lambda out, p0: _sized((out - 1) * down + 1 + (nd or 1) - 1, up, p0, nu or 1)      # noqa: E731
    (w, px1), (h, py1) = size(out_w, px0), size(out_h, py0)
    return Flr(f'up{up} down{down} {out_w}x{out_h} pad0=({px0},{py0}) fu={nu} fd={nd} ' + ' '.join(f'{k}={v}' for k, v in kw.items()),
               (1, 2, h, w), nu, nd, up, down, (px0, px1, py0, py1), **kw)


def _flr_table():
    cases = []
    for r, (up, down) in enumerate(FLR_RATES):
        for i, (ow, oh) in enumerate(itertools.product(FLR_OUT_W, FLR_OUT_H)):
            k = i + 3 * r
            kw = {}
            if k % 4 == 1:
                kw['slope'] = 0.0
            if k % 5 == 2:
                kw['dtype'] = 'f16'
            if k % 3 == 0:
                kw['flip'] = True
            if k % 7 == 3:
                kw['clamp'] = None
            # asymmetric pads, every third case a negative one; even ones where no up filter spreads the samples over the phases
            fu = k % 9 not in (4, 6)
            px0, py0 = ((3, -2, 5) if fu else (4, -2, 2))[k % 3], ((1, 4, -3) if fu else (2, 4, -2))[(k // 3) % 3]
            cases.append(flr_case(ow, oh, up, down, px0, py0, fu=fu, fd=k % 9 not in (5, 6), **kw))
    return tuple(cases)


FLR_CASES = _flr_table()


def flr_inputs(case):
    """(x, fu, fd, b): float32 values as the call sees them (x and b fp16-rounded for 'f16'); filters 1-D or None."""
    x = image(*case.shape, 7)
    b = _t(_rs('flr bias', case.shape[1]).randn(case.shape[1]) * 0.5) if case.bias else None
    if case.dtype == 'f16':
        x, b = x.half().float(), (None if b is None else b.half().float())
    return x, (None if case.fu is None else fir_filter(case.fu, None)), (None if case.fd is None else fir_filter(case.fd, None)), b


def flr_reference(case, wrong=None, dtype=F64):
    x, fu, fd, b = flr_inputs(case)
    return filtered_lrelu(x.to(dtype), fu, fd, None if b is None else b.to(dtype), case.up, case.down, case.pad, 2 ** 0.5, case.slope, case.clamp,
                          case.flip, wrong)


# ------------------------------------------------------------------ case tables: adjoint plans

# name -> (x shape, filter shape, keyword arguments of upfirdn2d.upfirdn2d): upsample2d, downsample2d (their paddings written out), the
# pad-1 blur and the mixed geometry
ADJOINT_CASES = {
    'upsample2d': ((2, 3, 9, 7), (4, 4), dict(up=2, down=1, padding=[2, 1, 2, 1], flip_filter=False, gain=4.0)),
    'downsample2d': ((2, 3, 12, 10), (4, 4), dict(up=1, down=2, padding=[1, 1, 1, 1], flip_filter=False, gain=1.0)),
    'blur_pad1': ((1, 2, 19, 67), (4, 4), dict(up=1, down=1, padding=[1, 1, 1, 1], flip_filter=True, gain=4.0)),
    'mixed': ((2, 3, 10, 9), (3, 5), dict(up=[2, 3], down=[3, 2], padding=[2, -1, 0, 3], flip_filter=True, gain=1.5)),
}


def adjoint_reference(name, dtype=F64, double_backward=False):
    """Autograd through the restatement: d/dx sum(y * w) (and, with `double_backward`, d/dw sum(that * v)) for seeded w and v."""
    shape, fshape, kw = ADJOINT_CASES[name]
    x = image(*shape, 3).to(dtype).requires_grad_(True)
    y = upfirdn2d(x, fir_filter(*fshape), kw['up'], kw['down'], kw['padding'], kw['flip_filter'], kw['gain'])
    w = image(*y.shape, 4).to(dtype).requires_grad_(double_backward)
    gx, = torch.autograd.grad((y * w).sum(), x, create_graph=double_backward)
    if not double_backward:
        return y.detach(), gx
    gw, = torch.autograd.grad((gx * image(*shape, 5).to(dtype)).sum(), w)
    return y.detach(), gx.detach(), gw
