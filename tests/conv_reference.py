"""Plain-torch restatement of the 3x3 / 1x1 convolution family (csrc/conv_split.hip, conv_up.hip, conv_small.h, conv_mfma.hip, conv_tiny.hip
and the shared conv_common.h), the seeded case tables that tests/test_conv_reference_cpu.py and tests/test_conv_edges_gpu.py share, and
a restatement of the planner and the dispatch (``expected_route``) that lets the tables be checked for coverage without a device.
No device code.

One layer function (``layer``) computes in the dtype of its arguments: in float64 it is the reference ``r``, in float32 the yardstick
whose distance to float64 on the same inputs is ``e32``.  Its inputs are the operands the kernel sees: the activations rebuilt from the
fp16 hi / lo planes of the split format (``operand``), the fp16 plane of the one-plane form.  The epilogue follows
conv_common.h::epilogue: demodulation, noise[pix] * strength, bias, leaky ReLU (scalar or per-channel slope), gain, clamp, residual
after the clamp.

Tolerance per element of a kernel result (``bound``):

    resample_reference.tolerance(r, e32)  =  4 * e32 + 2^-24 * max|r|
      + 2^-21 * S * |demod| * gain * slope       fp16-pair forms: the packed weights keep 22 bits and lo * lo is dropped
      + 2^-11 * S * |demod| * gain * slope       one-plane fp16 forms: the weights are rounded to fp16 once

with S = sum |x * w| over the receptive field in float64 and `slope` the derivative of the activation at r's pre-activation value (1
where that value is smaller than the term itself: the sign may differ there).  The fp32 forms (ia_conv2d_mfma, ia_conv3x3_s2_tiny) get
the first line alone.  None of these constants is fitted to a kernel.

``layer(..., wrong=<name>)`` (WRONG) writes out the plausible errors of such kernels; the CPU test shows that every table tells each
of them from the right result (ratio > 1) on at least one case.
"""
import itertools
from typing import NamedTuple, Optional

import torch
import torch.nn.functional as F

import resample_reference as R
from resample_reference import _rs, _t, _cached

F64 = torch.float64
NUM_CU = 256                  # ia::kNumCU, compiled in
PATCH_FLOATS = 1024           # kPatchFloats
CHUNK = 8                     # kChunkConv = kChunkTransposed: input channels per K chunk


# ------------------------------------------------------------------ the layer in float64 (or float32)

def raw(x, w, op, fir=None):
    """x [B, I, H, W], w [O, I, k, k] -> the bare sums.  op: 'conv' (stride 1, padding k // 2), 'down' (stride 2, padding 1), 'up'
    (conv_transpose2d, stride 2: (2H+1) x (2W+1)), 'upfir' ('up', then the 4x4 FIR `fir` with padding [1,1,1,1] and gain 4: 2H x 2W)."""
    w = w.to(x.dtype)
    if op == 'conv':
        return F.conv2d(x, w, padding=w.shape[-1] // 2)
    if op == 'down':
        return F.conv2d(x, w, stride=2, padding=1)
    t = F.conv_transpose2d(x, w.transpose(0, 1), stride=2)
    return t if op == 'up' else R.upfirdn2d(t, fir, 1, 1, (1, 1, 1, 1), False, 4.0)


def raw_taps(x, w, op):
    """`raw` for 'conv' / 'down' / 'up' written as a loop over the taps (the definition the kernels implement): the self-consistency test
    holds it against torch.nn.functional."""
    b, i, h, wd = x.shape
    o, k = w.shape[0], w.shape[-1]
    w = w.to(x.dtype)
    if op == 'up':
        out = x.new_zeros(b, o, 2 * h + 1, 2 * wd + 1)
        for ky, kx in itertools.product(range(3), range(3)):
            out[:, :, ky:ky + 2 * h:2, kx:kx + 2 * wd:2] += torch.einsum('oi,bihw->bohw', w[:, :, ky, kx], x)
        return out
    s, p = (2, 1) if op == 'down' else (1, k // 2)
    oh, ow = (h + 2 * p - k) // s + 1, (wd + 2 * p - k) // s + 1
    xp = F.pad(x, [p, p, p, p])
    out = x.new_zeros(b, o, oh, ow)
    for ky, kx in itertools.product(range(k), range(k)):
        out += torch.einsum('oi,bihw->bohw', w[:, :, ky, kx], xp[:, :, ky:ky + (oh - 1) * s + 1:s, kx:kx + (ow - 1) * s + 1:s])
    return out


def point_mask(op, h, w, points):
    """Output-pixel mask [OH, OW] of the points `points` (a slice of the row-major point grid: H x W, (H+1) x (W+1) transposed, the
    OUTPUT grid for stride 2).  A transposed point (r, c) owns pixels (2r + py, 2c + px); a depth-to-space point the same four."""
    gh, gw = {'conv': (h, w), 'down': ((h - 1) // 2 + 1, (w - 1) // 2 + 1), 'up': (h + 1, w + 1), 'upfir': (h, w)}[op]
    m = torch.zeros(gh * gw, dtype=torch.bool)
    m[points] = True
    m = m.view(gh, gw)
    if op in ('conv', 'down'):
        return m
    m = m.repeat_interleave(2, 0).repeat_interleave(2, 1)
    return m[:2 * h + 1, :2 * w + 1] if op == 'up' else m


WRONG = ('border_tap', 'mirror', 'phase_taps', 'noise_grid', 'demod_o4', 'slope_o4', 'residual_first', 'clamp_first', 'last_points',
         'last_quad', 'lo_dropped', 'lo_scale', 'fixup_last_worker', 'odd_tap', 'd2s_swap')


def layer(x, w, op='conv', fir=None, demod=None, noise=None, strength=None, bias=None, slope=None, gain=1.0, clamp=None, residual=None,
          wrong=None, drop=()):
    """The layer: raw sums, then the epilogue in the kernel's order.  slope: None (linear), a float, or [O].  noise [OH * OW].
    drop: ((out-channel slice, point slice, in-channel slice, taps or None), ...): partial sums left out of a region of the output (the
    restatement of a lost stream-K slab / a lost odd tap).  Returns (result, pre-activation value, raw sums)."""
    wm = w
    if wrong == 'mirror':
        wm = w.flip(2, 3)
    elif wrong == 'phase_taps':                      # the one-tap phase (1, 1) of the transposed form takes tap 8 instead of tap 4
        wm = w.clone()
        wm[:, :, 1, 1] = w[:, :, 2, 2]
    acc = raw(x, wm, op, fir)
    b, o, oh, ow = acc.shape
    h, wd = x.shape[2:]
    if wrong == 'border_tap':                        # the centre tap dropped for the first input column (the first output column of a stride-1 layer)
        wc = torch.zeros_like(w)
        wc[:, :, 1, 1] = w[:, :, 1, 1]
        xe = torch.zeros_like(x)
        xe[..., 0] = x[..., 0]
        acc = acc - raw(xe, wc, op, fir)
    for o_sl, p_sl, i_sl, taps in drop:
        wd_ = w[o_sl, i_sl]
        if taps is not None:
            keep = torch.zeros(9, dtype=torch.bool)
            keep[list(taps)] = True
            wd_ = wd_ * keep.view(1, 1, 3, 3).to(w.dtype)
        part = raw(x[:, i_sl], wd_, op, fir)
        acc[:, o_sl] = acc[:, o_sl] - part * point_mask(op, h, wd, p_sl).to(acc.dtype)
    if wrong == 'd2s_swap':                          # depth-to-space phases (py, px) exchanged
        acc = acc.view(b, o, oh // 2, 2, ow // 2, 2).permute(0, 1, 2, 5, 4, 3).reshape(b, o, oh, ow)
    v = acc
    if demod is not None:
        v = v * (demod.roll(4, 1) if wrong == 'demod_o4' else demod)[:, :, None, None]
    if noise is not None:
        nz = noise.view(oh, ow)
        if wrong == 'noise_grid':                    # indexed by the point grid (H x W) instead of the output pixel
            idx = (torch.arange(oh)[:, None] // 2) * (ow // 2) + torch.arange(ow)[None, :] // 2
            nz = noise[idx]
        v = v + nz * (1.0 if strength is None else strength.reshape(()))
    if bias is not None:
        v = v + bias[None, :, None, None]
    pre = v
    if slope is not None:
        sl = slope if not torch.is_tensor(slope) else (slope.roll(4, 0) if wrong == 'slope_o4' else slope)[None, :, None, None]
        v = torch.where(v > 0, v, v * sl)
    if wrong == 'clamp_first' and clamp is not None:
        v = v.clamp(-clamp, clamp)
    v = v * gain
    if wrong == 'residual_first' and residual is not None:
        v = v + residual
    if clamp is not None and wrong != 'clamp_first':
        v = v.clamp(-clamp, clamp)
    if residual is not None and wrong != 'residual_first':
        v = v + residual
    if wrong == 'last_quad':
        v = v.clone()
        v[:, -4:] = 0
    if wrong == 'last_points':                       # the last 32-point fragment of the grid never stored
        n = point_mask(op, h, wd, slice(0, None)).numel() if op in ('conv', 'down') else {'up': (h + 1) * (wd + 1), 'upfir': h * wd}[op]
        v = v * (~point_mask(op, h, wd, slice((n - 1) // 32 * 32, None))).to(v.dtype)
    return v, pre, acc


def torgb(v, rgb_w, rgb_styles, rgb_bias, rgb_clamp, rgb_res):
    """The fused ToRGB epilogue: clamp(sum_o w[o, c] * s[b, o] * v[o] + bias[c]) + residual.  rgb_w [O, C]."""
    ws = rgb_w[None] if rgb_styles is None else rgb_w[None] * rgb_styles[:, :, None]
    out = torch.einsum('boc,bohw->bchw', ws, v)
    if rgb_bias is not None:
        out = out + rgb_bias[None, :, None, None]
    if rgb_clamp is not None:
        out = out.clamp(-rgb_clamp, rgb_clamp)
    return out if rgb_res is None else out + rgb_res


def operand(x, planes):
    """float32 activations -> the value the split-format kernels see (float64): hi + lo / 2^11 of ia_act_split, or the fp16 plane."""
    hi, lo = R.split_pair(x, None, planes)
    return R.pair_value(hi, lo)


# ------------------------------------------------------------------ the planner and the dispatch, restated

def tile_window(p0, p_last, gw, pad, tr, stride=1):
    """conv_common.h::tile_window -> (shape, PW, PSZ); shape: 'single' | 'split' | 'full'."""
    s = 1 if tr else stride
    up, dn, lf, rt = (1, 0, 1, 0) if tr else (pad, pad, pad, pad)
    r_first, r_last = p0 // gw, p_last // gw
    c_first, c_last = p0 - r_first * gw, p_last - r_last * gw
    nrows = up + dn + 1
    if r_first == r_last:
        pw = (s * c_last + rt) - (s * c_first - lf) + 1
        return 'single', pw, nrows * pw
    w0, w1 = (s * (gw - 1) + rt) - (s * c_first - lf) + 1, (s * c_last + rt) + lf + 1
    pw_split, pw_full = max(w0, w1), s * (gw - 1) + 1 + lf + rt
    sz_split, sz_full = 2 * nrows * pw_split, (s * (r_last - r_first) + nrows) * pw_full
    if r_last == r_first + 1 and sz_split < sz_full:
        return 'split', pw_split, sz_split
    return 'full', pw_full, sz_full


def windows(npts, gw, bp, tr, stride=1):
    """[(shape, PSZ, starts mid-row, ends on the last point of the grid)] of the point tiles."""
    out = []
    for q0 in range(0, npts, bp):
        q1 = min(q0 + bp, npts) - 1
        shape, _, psz = tile_window(q0, q1, gw, 0 if tr else 1, tr, stride)
        out.append((shape, psz, q0 % gw != 0, q1 == npts - 1))
    return out


def down_patch_cap(bo):
    return min((160 * 1024 // 2 - 2 * 10 * bo * 16) // (2 * 16) // 64 * 64, 2048)


def tile_dims(o, h, w, ksize, tr, form, stride=1):
    """conv_mfma.hip::tile_dims -> (bo, bp, waves).  (h, w): the input; the OUTPUT grid for stride 2."""
    npts = (h + 1) * (w + 1) if tr else h * w
    sx_small = form == 3 and ksize == 3 and npts >= 64
    worst = lambda: max(p for _, p, _, _ in windows(npts, w, 256, False, stride))      # noqa: E731
    if npts <= 320 and o > 32 and not sx_small:
        return 128, 32, 4
    if tr:
        if form == 3 and 4096 <= npts < 8192:
            return 64, 256, 8
        return 64, (128 if form == 2 and o % 4 == 0 and npts >= 32768 else 64), 4
    if o <= 32:
        return 32, 256, 4
    if ksize == 3 and (o >= 128 or (o >= 64 and form == 3)) and o % 4 == 0 and (npts >= 1024 or sx_small) \
            and worst() <= (PATCH_FLOATS if stride == 1 else down_patch_cap(128)):
        return 128, 256, 8
    if stride == 2 and form == 3 and ksize == 3 and o % 32 == 0 and worst() <= down_patch_cap(32):
        return 32, 256, 8
    return 128, 128, 4


class Plan(NamedTuple):
    bo: int
    bp: int
    waves: int
    T: int
    TO: int
    C: int
    T_dp: int
    G: int
    slab_floats: int


def make_plan(b, i, o, h, w, ksize, tr, form, stride=1):
    """conv_mfma.hip::make_plan."""
    npts = (h + 1) * (w + 1) if tr else h * w
    bo, bp, waves = tile_dims(o, h, w, ksize, tr, form, stride)
    force_whole = stride == 2 and bo == 32 and o > 32
    if form == 3 and not force_whole and not tr and ksize == 3 and waves == 8 and o % 32 == 0:
        t_wide, t_narrow = b * -(-npts // 256) * -(-o // 128), b * -(-npts // 256) * (o // 32)
        if t_wide < NUM_CU and t_narrow >= NUM_CU:
            bo, bp, force_whole = 32, 256, True
    to = -(-o // bo)
    t = -(-npts // bp) * to
    c = -(-i // CHUNK)
    slots = (1 if waves == 8 else 2) * NUM_CU
    gb = max(slots // b, 1)
    rounds = t // gb
    r = t - rounds * gb
    if force_whole or r == 0 or rounds >= 8 or (rounds >= 1 and 4 * r >= 3 * gb):
        t_dp, g = t, 0
    else:
        t_dp = rounds * gb
        ur = r * c
        per = (c // 8 if c >= 8 else 1) if rounds > 0 else 2
        g = min(ur // per, gb)
        if rounds == 0 and npts <= 65 * 65:
            g = min(g, max(t, NUM_CU // 4))
        g = max(g, 1)
    frags = (bo // 32) * (bp // 32) // waves
    return Plan(bo, bp, waves, t, to, c, t_dp, g, (4 if tr else 1) * frags * 16 * waves * 64)


def conv_small_shape(b, i, o, h, w, tr, stride=1):
    """conv_common.h::conv_small_shape (without its experiment overrides)."""
    npts = (h + 1) * (w + 1) if tr else h * w
    wgs = b * -(-npts // 32) * -(-o // 32)
    return stride == 1 and npts <= (17 * 17 if tr else 1024) and wgs <= (384 if npts > 256 else 2 * NUM_CU)


def worker_segments(plan, g):
    """[(worker, local tile, c_lo, c_hi)] of the stream-K launch with g workers: conv_split_kernel's segment loop."""
    u_all = (plan.T - plan.T_dp) * plan.C
    out = []
    for wk in range(g):
        u, u_end = wk * u_all // g, (wk + 1) * u_all // g
        while u < u_end:
            tile, c_lo = divmod(u, plan.C)
            c_hi = min(plan.C, c_lo + u_end - u)
            out.append((wk, tile, c_lo, c_hi))
            u += c_hi - c_lo
    return out


class Route(NamedTuple):
    """What a call takes.  family: 'BOxBP/waves' or a kernel name; mode: 'whole' | 'whole+stream-k' | 'whole+fix-up' | 'stream-k' (every
    tile finished by one worker) | 'fix-up' | 'small' | 'refused' | 'rows' | 'tiny'; windows: the set of window shapes of its tiles;
    jp: patch DMA depth; chunks: 'C=1' | 'even' | 'odd'; parity: the set of {'even', 'odd'} segment lengths of the K loop ('odd' = a last
    chunk without a partner where the PAIR logic runs); flags: further facts of the case (see expected_route)."""
    entry: str
    family: str
    mode: str
    narrow: bool = False
    antiphase: bool = False
    windows: frozenset = frozenset()
    jp: int = 0
    chunks: str = ''
    parity: frozenset = frozenset()
    workers: int = 0
    scratch: int = 0
    flags: frozenset = frozenset()
    why: str = ''


def _chunks(c):
    return 'C=1' if c == 1 else ('even' if c % 2 == 0 else 'odd')


def sx_route(b, i, o, h, w, planes=2, tr=False, stride=1, ksplit=None, rgb=False, d2s=False, epilogue=False, noise=False, entry='sx'):
    """conv_split.hip::conv_sx_impl.  (h, w): the input image; o: the channel count the kernel sees (4 x O for the composed layer)."""
    refuse = lambda why: Route(entry, '', 'refused', why=why)      # noqa: E731
    if stride == 2 and (tr or d2s or rgb or noise):
        return refuse('stride 2: the plain 3x3 convolution')
    if i % 8 or o % 8:
        return refuse('I % 8 == 0 and O % 8 == 0')
    if tr and epilogue:
        return refuse('the transposed form writes the fp32')
    if d2s and (tr or o % 32):
        return refuse('depth-to-space store')
    gh, gw = (h + 1, w + 1) if tr else (((h - 1) // 2 + 1, (w - 1) // 2 + 1) if stride == 2 else (h, w))
    if stride == 2 and min(gh, gw) < 8:
        return refuse('outputs from 8^2 up')
    p = make_plan(b, i, o, gh if stride == 2 else h, gw if stride == 2 else w, 3, tr, 3, stride)
    if not (p.waves == 8 or (tr and p.bo == 64)):
        return refuse('two-stage tiles')
    narrow = p.waves == 8 and p.bp == 256 and (p.bo == 32 or (p.bo == 64 and not tr))
    if narrow and p.T_dp != p.T:
        return refuse('narrow tile families run whole tiles only')
    if rgb and (narrow or tr or p.TO != 1 or p.T_dp != p.T):
        return refuse('fused ToRGB')
    small = p.T_dp < p.T and conv_small_shape(b, i, o, h, w, tr, stride) and not rgb and not d2s
    if d2s and (p.bo != 128 or o % 128 or p.T_dp != p.T):
        return refuse('depth-to-space store: needs whole 128-channel tiles')
    npts = gh * gw
    flags = set()
    if small:
        if i // 8 < 8:
            flags.add('octets<waves')
        if npts % 32:
            flags.add('ragged points')
        if o % 32:
            flags.add('ragged channels')
        return Route(entry, 'small', 'small', chunks=_chunks(p.C), flags=frozenset(flags))
    g, scratch, mode, parity = 0, 0, 'whole', {'even' if p.C % 2 == 0 else 'odd'} if p.T_dp else set()
    if p.T_dp < p.T:
        ur = (p.T - p.T_dp) * p.C
        want = p.G if ksplit is None else ksplit
        if want < 1:
            return refuse('pass the worker count')
        g = min(want, ur)
        if want > ur:
            flags.add('workers clamped to U')
        whole_tiles = ur % g == 0 and (ur // g) % p.C == 0
        scratch = b * g * 2 * p.slab_floats * 4
        segs = worker_segments(p, g)
        parity |= {'even' if (hi - lo) % 2 == 0 else 'odd' for _, _, lo, hi in segs}
        cut = any(hi - lo < p.C for _, _, lo, hi in segs)
        first = {}
        for wk, tile, lo, hi in segs:
            first.setdefault(wk, tile)
            if hi - lo < p.C and tile != first[wk] and lo == 0:
                flags.add('trailing slot')
            if hi - lo == 1 and p.C > 1:
                flags.add('one chunk per worker')
            if lo % 2 == 1:
                flags.add('cut inside a chunk pair')
            elif lo > 0:
                flags.add('cut at a pair boundary')
        mode = ('whole+' if p.T_dp else '') + ('fix-up' if cut else 'stream-k')
        if not whole_tiles and not cut:
            flags.add('fix-up launched, no tile cut')
    win = windows(npts, gw, p.bp, tr, stride)
    worst = max(psz for _, psz, _, _ in win)
    if worst > (PATCH_FLOATS if stride == 1 else 8 * (8 if p.waves == 8 else 4) * 64 // planes):
        return refuse('patch exceeds the LDS budget')
    cap = (worst + 63) & ~63
    per_wave = -(-(planes * cap // 64) // p.waves)
    if planes == 1 and narrow and not (p.bo == 32 and not tr):
        return refuse('one-plane operands: the narrow tile family')
    if any(mid for _, _, mid, _ in win):
        flags.add('tile starts mid-row')
    if win[-1][3] and npts % p.bp == 0:
        flags.add('full last tile')
    if npts % p.bp:
        flags.add('ragged points')
    if o % p.bo:
        flags.add('ragged channels')
    if b > 1:
        flags.add(f'B={b}')
    aph = narrow and planes == 2 and not tr and npts >= 128 * 128
    return Route(entry, f'{p.bo}x{p.bp}/{p.waves}', mode, narrow, aph, frozenset(s for s, _, _, _ in win), 2 if per_wave <= 2 else (4 if per_wave <= 4 else 8),
                 _chunks(p.C), frozenset(parity), g, scratch, frozenset(flags))


def rows_route(b, i, o, h, w):
    """conv_up.hip::plan_up, as far as it does not depend on the window sizes: tile width, rounds, K-split of the long tiles, workers per
    edge tile, scratch bytes.  (The LDS test of plan_up is not restated: the CPU test pins accepted / refused against the library.)"""
    if i % 16 or o % 128 or h < 16 or w < 16 or w > 1024 or h > 1024:
        return Route('rows', '', 'refused', why='row-phase')
    fp = 2 if w >= 256 else 1
    bp, to = 128 * fp, o // 128
    npt = -(-h * w // bp)
    c0 = i // 8
    gpe = min(max(c0 // 16, 2), 4)
    one_round = b * 2 * npt * to <= NUM_CU
    split_long = one_round and i >= 512 and b * 3 * npt * to <= NUM_CU
    interior = b * to * (npt + (npt + 1) // 2)
    edge_tiles = -(-w // bp) + -(-(h + 1) // 64) + -(-h // 64)
    if one_round and not split_long and interior + b * to * edge_tiles <= NUM_CU:
        gpe = 0
    slabs = to * (npt * (2 if split_long else 0) + edge_tiles * gpe)
    flags = {'interior tiles', 'bottom row', 'last column', 'whole edge tiles' if gpe == 0 else 'K-split edge tiles'}
    if split_long:
        flags.add('K-split long tiles')
    if not one_round:
        flags.add('row phases paired')
    if b > 1:
        flags.add(f'B={b}')
    return Route('rows', f'128x{bp}/8', 'rows', workers=gpe, scratch=b * slabs * (2 * 2 * fp * 16) * 512 * 4, flags=frozenset(flags))


def mfma_route(b, i, o, h, w, ksize, tr, form, ksplit=None):
    """conv_mfma.hip::conv2d_entry (forms 0 = fp32, 1 = fp16 operands, 2 = fp16 pairs, staged through registers)."""
    entry = ('mfma', 'mfma_h', 'mfma_s')[form]
    if tr and ksize != 3:
        return Route(entry, '', 'refused', why='transposed form is 3x3')
    p = make_plan(b, i, o, h, w, ksize, tr, form)
    if form and not (ksize == 3 and (p.waves == 8 or (tr and p.bo == 64)) and i % 8 == 0 and o % 4 == 0):
        return Route(entry, '', 'refused', why='fp16-operand form')
    g, mode, flags = 0, 'whole', set()
    if p.T_dp < p.T:
        ur = (p.T - p.T_dp) * p.C
        want = p.G if ksplit is None else ksplit
        g = min(want, ur)
        if want > ur:
            flags.add('workers clamped to U')
        cut = any(hi - lo < p.C for _, _, lo, hi in worker_segments(p, g))
        mode = ('whole+' if p.T_dp else '') + ('fix-up' if cut else 'stream-k')
    if tr:
        flags.add('quad store' if o % 4 == 0 else 'per-element store')
    bo, bp = (32, 256) if (not form and p.bp != 32 and not tr and o <= 32) else (p.bo, p.bp)
    return Route(entry, f'{bo}x{bp}/{p.waves} k{ksize}' + (' transposed' if tr else ''), mode, chunks=_chunks(p.C), workers=g,
                 scratch=b * g * 2 * p.slab_floats * 4, flags=frozenset(flags))


# ------------------------------------------------------------------ cases

class Epi(NamedTuple):
    """Options of the epilogue.  slope: None | 'scalar' | 'prelu'; clamp: None or the quantile of |gain * activation| it sits at."""
    demod: bool = True
    noise: bool = True
    strength: bool = True
    bias: bool = True
    slope: Optional[str] = 'scalar'
    gain: float = 1.3
    clamp: Optional[float] = 0.8
    residual: bool = False
    styles_next: bool = True
    want_f32: bool = True
    split_planes: int = 2


PLAIN = Epi(False, False, False, False, None, 1.0, None, False, False, True, 2)
DEMOD = PLAIN._replace(demod=True)
FULL = Epi()
# every option on and off, every pair of (noise, bias, slope kind, clamp, residual, second output) in both states somewhere
EPI_OPTIONS = (
    FULL, PLAIN, DEMOD,
    Epi(residual=True, slope='prelu'),
    Epi(noise=True, strength=False, bias=False, clamp=None, split_planes=1),
    Epi(demod=False, noise=False, slope='prelu', gain=1.0, residual=True, styles_next=False),
    Epi(noise=False, bias=True, slope=None, clamp=0.6, residual=True, want_f32=False),
    Epi(demod=True, noise=True, bias=False, slope=None, gain=2.0 ** 0.5, clamp=None, residual=False, styles_next=True, want_f32=False, split_planes=1),
    Epi(bias=False, slope='scalar', clamp=0.5, residual=True, styles_next=False),
)


class Case(NamedTuple):
    """entry: 'sx' (conv2d_mfma_sx) | 'down' (conv2d_down_sx) | 'rows' (upconv2d_rows_sx) | 'upfir' (upconv_fir_sx) | 'rgb' (conv2d_mfma_sx_rgb) |
    'mfma' (conv2d_mfma; form 0 / 1 / 2) | 'tiny' (conv3x3_s2_tiny)."""
    name: str
    entry: str
    b: int
    i: int
    o: int
    h: int
    w: int
    planes: int = 2
    tr: bool = False
    epi: Epi = FULL
    ksplit: Optional[int] = None
    form: int = 3
    ksize: int = 3
    rgb_n: int = 0

    @property
    def op(self):
        return {'sx': 'up' if self.tr else 'conv', 'down': 'down', 'rows': 'up', 'upfir': 'upfir', 'rgb': 'conv', 'mfma': 'up' if self.tr else 'conv',
                'tiny': 'down'}[self.entry]

    @property
    def out_hw(self):
        h, w = self.h, self.w
        return {'conv': (h, w), 'down': ((h - 1) // 2 + 1, (w - 1) // 2 + 1), 'up': (2 * h + 1, 2 * w + 1), 'upfir': (2 * h, 2 * w)}[self.op]


def expected_route(case):
    c = case
    e = c.epi
    epilogue = e.noise or e.bias or e.residual or e.slope is not None or e.styles_next or not e.want_f32
    if c.entry in ('sx', 'rgb'):
        return sx_route(c.b, c.i, c.o, c.h, c.w, c.planes, c.tr, 1, c.ksplit, rgb=c.entry == 'rgb', epilogue=epilogue, noise=e.noise, entry=c.entry)
    if c.entry == 'down':
        return sx_route(c.b, c.i, c.o, c.h, c.w, c.planes, False, 2, None, noise=e.noise, entry='down')
    if c.entry == 'upfir':
        return sx_route(c.b, c.i, 4 * c.o, c.h, c.w, c.planes, d2s=True, entry='upfir')
    if c.entry == 'rows':
        return rows_route(c.b, c.i, c.o, c.h, c.w)
    if c.entry == 'mfma':
        return mfma_route(c.b, c.i, c.o, c.h, c.w, c.ksize, c.tr, c.form, c.ksplit)
    ok = c.h == c.w and c.h in (2, 4, 8) and c.i <= 512
    return Route('tiny', 'one wave per channel', 'tiny' if ok else 'refused')


def _sx(name, b, i, o, h, w, planes=2, tr=False, epi=None, ksplit=None):
    return Case(name, 'sx', b, i, o, h, w, planes, tr, (DEMOD if tr else FULL) if epi is None else epi, ksplit)


# stride 1, conv2d_mfma_sx.  The stream-K shape is 33 x 33 (1089 points: five 256-point tiles, the last one ragged) with I = 40 (C = 5).
SX_CASES = (
    _sx('wide, whole rounds, B=4', 4, 8, 128, 128, 128),
    _sx('wide, one whole round + a stream-K tile cut in two', 4, 16, 128, 128, 130, epi=EPI_OPTIONS[3]),
    _sx('narrow 32x256 antiphase', 1, 8, 128, 128, 128, epi=EPI_OPTIONS[4]),
    _sx('narrow 32x256, C even', 1, 16, 256, 64, 128),
    _sx('narrow 32x256, one plane, C odd', 1, 24, 256, 64, 128, planes=1, epi=EPI_OPTIONS[7]),
    _sx('stream-K default workers, C odd', 1, 40, 128, 33, 33),
    _sx('stream-K, every tile by one worker', 1, 40, 128, 33, 33, ksplit=5, epi=EPI_OPTIONS[3]),
    _sx('stream-K, one chunk per worker', 1, 40, 128, 33, 33, ksplit=25, epi=EPI_OPTIONS[5]),
    _sx('stream-K, more workers than units', 1, 40, 128, 33, 33, ksplit=100, epi=EPI_OPTIONS[6]),
    _sx('stream-K, cuts at pair boundaries, C even', 1, 32, 72, 33, 33, ksplit=10, epi=EPI_OPTIONS[8]),
    _sx('stream-K B=2, O=136', 2, 40, 136, 33, 33),
    _sx('stream-K B=3, one plane', 3, 24, 128, 33, 35, planes=1, epi=EPI_OPTIONS[4]),
    _sx('windows full and split, W=200', 1, 8, 64, 17, 200, epi=EPI_OPTIONS[6]),
    _sx('window single, W=256', 1, 8, 128, 5, 256, epi=EPI_OPTIONS[5]),
    _sx('window single, W=512, C=1', 1, 8, 72, 3, 512, epi=EPI_OPTIONS[1]),
) + tuple(_sx(f'options {n}', 1, 16, 72, 33, 34, epi=e) for n, e in enumerate(EPI_OPTIONS)) + (
    _sx('narrow 32x256, window single, W=512', 1, 8, 256, 16, 512, epi=EPI_OPTIONS[5]),
    _sx('narrow 32x256, windows full and split, W=200', 1, 8, 640, 17, 200, epi=EPI_OPTIONS[6]),
)

SMALL_CASES = (
    _sx('small 8x8', 1, 24, 128, 8, 8, epi=EPI_OPTIONS[3]),
    _sx('small 9x9 B=2, O=72', 2, 40, 72, 9, 9),
    _sx('small 12x10, O=136, three octets', 1, 24, 136, 12, 10, epi=EPI_OPTIONS[5]),
    _sx('small 32x32, one plane', 1, 64, 128, 32, 32, planes=1, epi=EPI_OPTIONS[4]),
    _sx('small 16x16 B=3, eight octets', 3, 64, 200, 16, 16, epi=EPI_OPTIONS[6]),
    _sx('small transposed 8x8', 1, 24, 72, 8, 8, tr=True),
    _sx('small transposed 16x15 B=2, O=8', 2, 16, 8, 16, 15, tr=True),
    _sx('small transposed 16x16, one plane', 1, 64, 64, 16, 16, planes=1, tr=True, epi=PLAIN),
)

TR_CASES = (
    _sx('transposed 64x64, stream-K, odd image, O=8', 1, 24, 8, 21, 19, tr=True),
    _sx('transposed 64x64, stream-K B=2, O=72', 2, 40, 72, 20, 20, tr=True, epi=PLAIN),
    _sx('transposed 64x64, one chunk per worker', 1, 24, 8, 21, 19, tr=True, ksplit=21),
    _sx('transposed 64x64, whole rounds B=16', 16, 8, 64, 31, 63, tr=True),
    _sx('transposed 64x64, one plane', 1, 16, 24, 23, 18, planes=1, tr=True),
    _sx('transposed 64x256, fix-up launched, no tile cut', 1, 8, 64, 64, 64, tr=True),
    _sx('transposed 64x256, stream-K whole tiles', 1, 16, 64, 64, 64, tr=True, epi=PLAIN),
    _sx('transposed 64x256, whole rounds B=8', 8, 8, 128, 63, 63, tr=True),
    _sx('transposed 64x256, one plane, tiles cut', 1, 24, 72, 70, 60, planes=1, tr=True),
    _sx('transposed 64x64, window split, W=99', 1, 8, 16, 8, 99, tr=True),
    _sx('transposed 64x256, window split, W=199', 1, 8, 64, 24, 199, tr=True, epi=PLAIN),
)

_DOWN = Epi(noise=False, strength=False)
DOWN_CASES = (
    Case('stride 2 wide, one tile', 'down', 1, 16, 64, 32, 32, epi=_DOWN._replace(slope='prelu', residual=True)),
    Case('stride 2 wide, odd image, B=2', 'down', 2, 24, 136, 33, 47, epi=_DOWN),
    Case('stride 2 wide, one plane', 'down', 1, 16, 64, 31, 34, planes=1, epi=_DOWN._replace(split_planes=1, clamp=None)),
    Case('stride 2 narrow, whole tiles', 'down', 1, 8, 64, 22, 112, epi=_DOWN._replace(residual=True, want_f32=False)),
    Case('stride 2 narrow, B=3, plain', 'down', 3, 16, 96, 21, 111, epi=PLAIN),
)

ROWS_CASES = (
    Case('rows 16x16', 'rows', 1, 16, 128, 16, 16, epi=DEMOD),
    Case('rows 17x33 B=3, O=256', 'rows', 3, 32, 256, 17, 33, epi=DEMOD),
    Case('rows 16x256 (two point fragments)', 'rows', 1, 16, 128, 16, 256, epi=PLAIN),
    Case('rows 130x128 (K-split edge tiles)', 'rows', 1, 16, 128, 130, 128, epi=DEMOD),
    Case('rows 16x16, I=512 (K-split long tiles)', 'rows', 1, 512, 128, 16, 16, epi=DEMOD),
)

_UPFIR = FULL._replace(residual=False, slope='scalar')
UPFIR_CASES = (
    Case('composed up-FIR B=4 128x128', 'upfir', 4, 8, 32, 128, 128, epi=_UPFIR),
    Case('composed up-FIR B=16 64x64, one plane', 'upfir', 16, 8, 32, 64, 64, planes=1, epi=_UPFIR._replace(split_planes=1, clamp=None, strength=False)),
    Case('composed up-FIR B=8 64x128, O=64, pair only', 'upfir', 8, 16, 64, 64, 128, epi=_UPFIR._replace(want_f32=False, noise=False)),
)

_RGB = FULL._replace(styles_next=False)
RGB_CASES = (
    Case('fused ToRGB, 3 colours', 'rgb', 4, 8, 128, 128, 128, epi=_RGB, rgb_n=3),
    Case('fused ToRGB, 1 colour, one plane', 'rgb', 16, 16, 72, 64, 64, planes=1, epi=_RGB._replace(clamp=None, noise=False), rgb_n=1),
)


def _mfma(name, b, i, o, h, w, form=0, ksize=3, tr=False, ksplit=None, epi=None):
    e = (DEMOD if tr else FULL._replace(styles_next=False, residual=True)) if epi is None else epi
    return Case(name, 'mfma', b, i, o, h, w, {0: 0, 1: 1, 2: 2}[form], tr, e, ksplit, form, ksize)


MFMA_CASES = (
    _mfma('fp32 128x32 small-image tile', 2, 24, 40, 8, 8),
    _mfma('fp32 128x32 small-image tile 1x1', 1, 16, 40, 9, 8, ksize=1),
    _mfma('fp32 O <= 32 tile', 1, 16, 32, 12, 13),
    _mfma('fp32 O <= 32 tile 1x1, O=3', 2, 48, 3, 16, 16, ksize=1),
    _mfma('fp32 128x128', 1, 8, 72, 20, 21),
    _mfma('fp32 128x128 1x1', 1, 16, 96, 20, 20, ksize=1),
    _mfma('fp32 wide', 1, 8, 136, 33, 33),
    _mfma('fp32 workers 1', 1, 64, 48, 16, 16, ksplit=1),
    _mfma('fp32 workers 3', 1, 64, 48, 16, 16, ksplit=3),
    _mfma('fp32 workers > units', 1, 64, 48, 16, 16, ksplit=1000),
    _mfma('fp32 transposed O=10 (per-element store)', 1, 16, 10, 9, 7, tr=True),
    _mfma('fp32 transposed O=6 B=2', 2, 8, 6, 11, 5, tr=True, epi=PLAIN),
    _mfma('fp32 transposed O=8 (quad store)', 1, 16, 8, 8, 9, tr=True),
    _mfma('fp32 transposed O=12', 1, 8, 12, 7, 7, tr=True),
    _mfma('fp32 transposed 128x32 tile', 1, 8, 40, 8, 8, tr=True),
    _mfma('fp16 operands wide', 1, 16, 128, 33, 33, form=1),
    _mfma('fp16 operands transposed, O=12', 1, 8, 12, 20, 20, form=1, tr=True),
    _mfma('fp16 pairs wide', 1, 16, 128, 33, 33, form=2),
    _mfma('fp16 pairs transposed 64x64, O=8', 1, 8, 8, 20, 21, form=2, tr=True),
    _mfma('fp16 pairs transposed 64x128', 1, 8, 8, 181, 180, form=2, tr=True),
)

_TINY = PLAIN._replace(bias=True, slope='scalar')
TINY_CASES = (
    Case('tiny 8x8 B=3', 'tiny', 3, 70, 10, 8, 8, planes=0, epi=_TINY),
    Case('tiny 4x4', 'tiny', 1, 16, 7, 4, 4, planes=0, epi=_TINY._replace(slope=None)),
    Case('tiny 2x2 B=2', 'tiny', 2, 8, 5, 2, 2, planes=0, epi=_TINY),
)

TABLES = {'sx': SX_CASES, 'small': SMALL_CASES, 'transposed': TR_CASES, 'down': DOWN_CASES, 'rows': ROWS_CASES, 'upfir': UPFIR_CASES, 'rgb': RGB_CASES,
          'mfma': MFMA_CASES, 'tiny': TINY_CASES}

# Calls the entries must refuse without launching: (case, words of the message).  (Stride 2 with noise is not among them: ia_conv2d_down_sx
# has no noise argument, so no caller reaches that IA_REQUIRE.)
REFUSALS = (
    (_sx('I = 12', 1, 12, 128, 33, 33), 'I % 8'),
    (_sx('O = 132', 1, 16, 132, 33, 33), 'O % 8'),
    (_sx('transposed with an epilogue', 1, 16, 64, 20, 20, tr=True, epi=FULL._replace(styles_next=False)), 'transposed form writes'),
    (Case('depth-to-space on the narrow tiles', 'upfir', 1, 8, 32, 128, 128, epi=_UPFIR), 'depth-to-space'),
    (Case('fused ToRGB on a narrow layer', 'rgb', 1, 8, 128, 128, 128, epi=_RGB, rgb_n=3), 'fused ToRGB'),
    (Case('fused ToRGB on two channel tiles', 'rgb', 4, 8, 256, 128, 128, epi=_RGB, rgb_n=3), 'fused ToRGB'),
    (_sx('W = 257: the 256-point windows pass the patch', 1, 8, 128, 5, 257), 'two-stage tiles'),
)


# ------------------------------------------------------------------ seeded inputs and references

FIR = lambda: R.fir_filter(4, 4)      # noqa: E731  (no symmetry: a flipped or mirrored tap shows)


@_cached
def inputs(case):
    """float32 CPU tensors of a case.  The activations spread over four decades per channel and channel 1 lies below the fp16 normal range
    (it rides in the low plane); demodulation, slopes and styles differ from channel to channel."""
    c = case
    rs = _rs('conv', c.entry, c.b, c.i, c.o, c.h, c.w, c.tr, c.ksize)
    oh, ow = c.out_hw
    mag = 10.0 ** rs.uniform(-3.0, 0.5, size=(1, c.i, 1, 1))
    mag[0, 1 % c.i] = 1.5e-5
    x = _t(rs.randn(c.b, c.i, c.h, c.w) * mag)
    w = _t(rs.randn(c.o, c.i, c.ksize, c.ksize) * (3.0 / (c.ksize * c.ksize * c.i) ** 0.5))
    if c.form == 1:                               # (ia_conv2d_mfma_h rounds its fp32 activations itself: fp16 numbers go through unchanged.  The
        x = x.half().float()                      # weights of every one-plane form stay float32: their rounding to fp16 is what the 2^-11 term is for)
    t = {'x': x, 'w': w,
         'demod': _t(rs.uniform(0.5, 1.5, size=(c.b, c.o))), 'noise': _t(rs.randn(oh * ow)), 'strength': _t([0.3]),
         'bias': _t(rs.randn(c.o) * 0.3), 'prelu': _t(rs.uniform(0.05, 0.55, size=c.o)), 'residual': _t(rs.randn(c.b, c.o, oh, ow)),
         'styles_next': _t(rs.uniform(0.5, 1.5, size=(c.b, c.o)))}
    if c.rgb_n:
        t.update(rgb_w=_t(rs.randn(c.o, c.rgb_n) / c.o ** 0.5), rgb_styles=_t(rs.uniform(0.5, 1.5, size=(c.b, c.o))), rgb_bias=_t(rs.randn(c.rgb_n) * 0.3),
                 rgb_res=_t(rs.randn(c.b, c.rgb_n, oh, ow)))
    return t


RGB_CLAMP = 0.7
ALPHA = 0.2


def seen(case, wrong=None):
    """float64 activations as the kernel of the case sees them."""
    x = inputs(case)['x']
    if case.entry == 'tiny' or case.form == 0:
        return x.double()
    if wrong == 'lo_dropped':
        return R.split_pair(x, None, 2)[0].double()
    return operand(x, 1 if (case.form == 1 or case.planes == 1) else 2)


def epi_args(case, t, dtype, clamp):
    e = case.epi
    g = lambda k: t[k].to(dtype)      # noqa: E731
    return dict(demod=g('demod') if e.demod else None, noise=g('noise') if e.noise else None, strength=g('strength') if e.noise and e.strength else None,
                bias=g('bias') if e.bias else None, slope=None if e.slope is None else (g('prelu') if e.slope == 'prelu' else ALPHA), gain=e.gain,
                clamp=clamp, residual=g('residual') if e.residual else None)


class Ref(NamedTuple):
    y: torch.Tensor                 # float64 result
    tol: torch.Tensor               # per-element bound of the fp32 result
    base: float = 0.0               # its part 4 * e32 + 2^-24 * max|r| (the rest is the weight term)
    clamp: Optional[float] = None   # the clamp the case passes (a float32 number)
    rgb: Optional[torch.Tensor] = None
    rgb_tol: Optional[torch.Tensor] = None


def weight_term(case):
    return 0.0 if (case.entry == 'tiny' or case.form == 0) else (2.0 ** -11 if (case.form == 1 or case.planes == 1) else 2.0 ** -21)


def run(case, dtype=F64, wrong=None, clamp='auto', drop=()):
    """(result, pre-activation, raw sums, clamp) of the case's layer in `dtype`."""
    t = inputs(case)
    x = seen(case, wrong).to(dtype)
    fir = FIR() if case.op == 'upfir' else None
    if clamp == 'auto':
        clamp = reference(case).clamp
    y, pre, acc = layer(x, t['w'].to(dtype), case.op, fir, wrong=wrong, drop=drop, **epi_args(case, t, dtype, clamp))
    return y, pre, acc, clamp


_refs = {}


def reference(case):
    """The float64 result of a case with its per-element bound (computed once, shared, never written to)."""
    if case in _refs:
        return _refs[case]
    t, e = inputs(case), case.epi
    clamp = None
    if e.clamp is not None:         # the clamp sits inside the distribution: at the e.clamp quantile of the unclamped magnitudes
        y0, _, _, _ = run(case, F64, clamp=None)
        v = (y0 - (t['residual'].double() if e.residual else 0.0)).abs().flatten()
        clamp = float(torch.tensor(float(v.kthvalue(max(1, int(e.clamp * v.numel()))).values)).float())
    y, pre, _, _ = run(case, F64, clamp=clamp)
    y32 = run(case, torch.float32, clamp=clamp)[0]
    e32 = float((y32.double() - y).abs().max())
    tol = R.tolerance(y, e32)
    wt = weight_term(case)
    if wt:
        x, w = seen(case).abs(), t['w'].double().abs()
        s = raw(x, w, case.op, FIR().abs() if case.op == 'upfir' else None)
        term = wt * s * e.gain * (t['demod'].double()[:, :, None, None] if e.demod else 1.0)
        if e.slope is not None:
            sl = t['prelu'].double()[None, :, None, None] if e.slope == 'prelu' else ALPHA
            term = term * torch.where((pre < 0) & (pre.abs() > term), torch.as_tensor(sl, dtype=F64).expand_as(pre), torch.ones_like(pre))
        tol = tol + term
    rgb = rgb_tol = None
    if case.rgb_n:
        args = lambda dt, v: (v.to(dt), t['rgb_w'].to(dt), t['rgb_styles'].to(dt), t['rgb_bias'].to(dt), RGB_CLAMP, t['rgb_res'].to(dt))      # noqa: E731
        rgb = torgb(*args(F64, y))
        e32r = float((torgb(*args(torch.float32, y32)).double() - rgb).abs().max())
        ws = (t['rgb_w'].double()[None] * t['rgb_styles'].double()[:, :, None]).abs()
        rgb_tol = R.tolerance(rgb, e32r) + torch.einsum('boc,bohw->bchw', ws, tol - R.tolerance(y, e32) + 2.0 ** -24 * y.abs())
    _refs[case] = Ref(y, tol, 4.0 * e32 + R.EPS32 * float(y.abs().max()), clamp, rgb, rgb_tol)
    return _refs[case]


def ratio(got, ref, tol):
    return float(((got.double() - ref).abs() / tol.clamp_min(1e-300)).max())


def worst_element(got, ref):
    """(ratio, index, bound there, share of 4 * e32 + 2^-24 * max|r| in that bound) of the element of `got` that comes closest to its bound."""
    r = (got.double() - ref.y).abs() / ref.tol.clamp_min(1e-300)
    at = int(r.argmax())
    idx = tuple(int(v) for v in torch.unravel_index(torch.tensor(at), r.shape))
    return float(r.flatten()[at]), idx, float(ref.tol.flatten()[at]), ref.base / float(ref.tol.flatten()[at])


def second_output(case, y):
    """(hi, lo or None) the kernel must store for the float32 result y."""
    e, t = case.epi, inputs(case)
    return R.split_pair(y, t['styles_next'].to(y.device) if e.styles_next else None, e.split_planes)


def pair_ratio(case, hi, lo):
    """The stored pair against the float64 reference times styles_next: the layer's bound times |styles_next| + the pair's own 22 (11) bits."""
    e, t, ref = case.epi, inputs(case), reference(case)
    sn = t['styles_next'].double()[:, :, None, None] if e.styles_next else 1.0
    want = (ref.y * sn).clamp(-65504.0, 65504.0)
    own = R.split_bound(want) if e.split_planes == 2 else want.abs() * 2.0 ** -11 + 2.0 ** -25
    return ratio(R.pair_value(hi, lo), want, ref.tol * sn + own)


# ------------------------------------------------------------------ wrong restatements: where each can show

def wrong_drop(case, wrong):
    """The partial sums a lost slab / a lost odd tap leaves out: `drop` of ``layer``; () where the error cannot occur on this route."""
    r = expected_route(case)
    if r.mode in ('refused', 'small', 'rows', 'tiny') or case.entry not in ('sx', 'down', 'upfir', 'rgb'):
        return ()
    o_k = 4 * case.o if case.entry == 'upfir' else case.o
    p = make_plan(case.b, case.i, o_k, *((case.out_hw) if case.entry == 'down' else (case.h, case.w)), 3, case.tr, 3, 2 if case.entry == 'down' else 1)
    bo, bp = (32, 256) if r.narrow else (p.bo, p.bp)
    out = []
    if wrong == 'odd_tap' and not case.tr and case.entry != 'upfir':
        if p.T_dp and p.C % 2:                       # whole tiles: the last chunk has no partner
            out.append((slice(0, None), slice(0, p.T_dp // p.TO * bp), slice(8 * (p.C - 1), None), (8,)))
        for _, tile, lo, hi in (worker_segments(p, r.workers) if r.workers else ()):
            if (hi - lo) % 2:
                tl = p.T_dp + tile
                out.append((slice(tl % p.TO * bo, tl % p.TO * bo + bo), slice(tl // p.TO * bp, tl // p.TO * bp + bp), slice(8 * (hi - 1), 8 * hi), (8,)))
    if wrong == 'fixup_last_worker' and 'fix-up' in r.mode and case.entry != 'upfir':
        segs = worker_segments(p, r.workers)
        for tile in {tl for _, tl, lo, hi in segs if hi - lo < p.C}:
            lo, hi = max((lo, hi) for _, tl, lo, hi in segs if tl == tile)
            tl = p.T_dp + tile
            out.append((slice(tl % p.TO * bo, tl % p.TO * bo + bo), slice(tl // p.TO * bp, tl // p.TO * bp + bp), slice(8 * lo, 8 * hi), None))
    return tuple(out)


def wrong_applies(wrong, case):
    e, c = case.epi, case
    if wrong == 'phase_taps':
        return c.op in ('up', 'upfir')
    if wrong in ('noise_grid', 'd2s_swap'):
        return c.op == 'upfir' and (e.noise or wrong == 'd2s_swap')
    if wrong == 'demod_o4':
        return e.demod
    if wrong == 'slope_o4':
        return e.slope == 'prelu'
    if wrong == 'residual_first':
        return e.residual and e.clamp is not None
    if wrong == 'clamp_first':
        return e.clamp is not None and e.gain != 1.0
    if wrong == 'lo_dropped':
        return c.planes == 2 and c.entry != 'tiny'
    if wrong == 'lo_scale':
        return e.split_planes == 2 and c.entry in ('sx', 'down', 'upfir') and not c.tr and c.entry != 'rows'
    if wrong in ('odd_tap', 'fixup_last_worker'):
        return bool(wrong_drop(c, wrong))
    if wrong in ('mirror', 'border_tap'):
        return c.ksize == 3
    return True


def wrong_ratio(case, wrong):
    """Worst ratio of the wrong restatement (float64) against the case's bound."""
    ref = reference(case)
    if wrong == 'lo_scale':
        return pair_ratio(case, *R.split_pair(ref.y.float(), inputs(case)['styles_next'] if case.epi.styles_next else None, 2, wrong='lo_scale'))
    y = run(case, F64, wrong=wrong, drop=wrong_drop(case, wrong))[0]
    return ratio(y, ref.y, ref.tol)
