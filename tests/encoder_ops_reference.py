"""Plain-torch restatements of the inversion encoder's small fused kernels, and the seeded inputs that tests/test_encoder_ops_cpu.py
and tests/test_encoder_ops_gpu.py share.  No device code.

Every restatement computes in the dtype of its arguments: with float64 tensors it is the reference, with float32 tensors it is "the
same operation written with ATen ops in float32 on the CPU", whose own distance to float64 (``e32``) is the yardstick of every
comparison of a float32 kernel result with float64:

    |kernel - fp64| <= 4 * max(e32) + floor            (``max_tol``; floors below)

The factor 4 covers another, equally valid summation order and expf / tanhf implementations a few ulp apart.  The ConvGRU halves are
compared per element, because ``(1 - z)`` cancels as z -> 1 and nothing relative to the result can hold:

    gates :  |err| <= 8 * 2^-24 * |h|
    update:  |err| <= 4 * e32_elem + 8 * 2^-24 * (|h| + |cand|)

A value stored as an fp16 hi / lo pair carries 22 mantissa bits: ``|pair - v| <= 2^-21 |v| + 2^-26`` (``split_bound``).

Restatements take ``wrong=<name>``: the plausible index and gate errors of such kernels, written out so that the CPU test can show
that the chosen inputs tell each of them from the right result by at least ten times the tolerance.

Definitions restated:
  ConvGRU (csrc/convgru.hip header; unet_encoders.ConvGRU):  r, z = sigmoid(gates_pre).split(C);  xrh = cat[x, r * h];
      c = tanh(cand_pre) or PReLU(cand_pre);  h' = (1 - z) * h + z * c;  xh_next = cat[x_next, h']
  SE tail (csrc/se_gate.hip; helpers.SEModule + the add of bottleneck_IR_SE):  v * sigmoid(w2 relu(w1 mean_hw v)) + shortcut
  bilinear add (csrc/resize.hip):  F.interpolate(x, size, mode='bilinear', align_corners=True) + y
  token convolution (csrc/dwconv.hip; mix_transformer.DWConv):  depth-wise 3x3, zero padding, on tokens [B, H*W, C]; optional erf GELU
  attention (csrc/attention.hip; mix_transformer.Attention):  softmax(q k^T * scale) v per head, k = kv[..., :C], v = kv[..., C:]
"""
import math

import numpy as np
import torch

F64 = torch.float64
EPS32 = 2.0 ** -24


# ------------------------------------------------------------------ tolerances

def max_tol(e32, floor):
    return 4.0 * float(e32.max()) + floor


def rel_floor(ref):
    """The project's bar of the SE tail, the bilinear add, the token convolution and attention_sx."""
    return 2e-6 * max(1.0, float(ref.abs().max()))


ATTENTION_FLOOR = 5e-6          # the project's bar of ia_attention


def split_bound(v):
    return v.abs() * 2.0 ** -21 + 2.0 ** -26


def gates_bound(h):
    return 8.0 * EPS32 * h.abs()


def update_bound(e32, h, cand):
    return 4.0 * e32 + 8.0 * EPS32 * (h.abs() + cand.abs())


def f64(*tensors):
    return tuple(None if t is None else t.detach().cpu().to(F64) for t in tensors)


def f32(*tensors):
    return tuple(None if t is None else t.detach().cpu().float() for t in tensors)


# ------------------------------------------------------------------ split format

def split_planes(v):
    """The fp16 pair that ``ia::split_f16`` stores for float32 values v: hi = fp16(v) (0 below 2^-14), lo = fp16((v - hi) * 2^11), v
    saturated at +-65504."""
    assert v.dtype == torch.float32
    v = v.clamp(-65504.0, 65504.0)
    hi = torch.where(v.abs() < 6.103515625e-5, torch.zeros_like(v), v).half()
    lo = ((v - hi.float()) * 2048.0).half()
    return hi, lo


def act_planes(data):
    """``SplitAct.data`` [b][plane][c/8][h][w][8] -> (hi, lo), each fp16 NCHW."""
    b, planes, c8, h, w, e = data.shape
    assert planes == 2 and e == 8
    hi, lo = (data[:, p].permute(0, 1, 4, 2, 3).reshape(b, c8 * 8, h, w) for p in (0, 1))
    return hi, lo


def token_planes(data):
    """``SplitTokens.data`` [2][K/8][M][8] -> (hi, lo), each fp16 [M, K]."""
    planes, k8, m, e = data.shape
    assert planes == 2 and e == 8
    hi, lo = (data[p].permute(1, 0, 2).reshape(m, k8 * 8) for p in (0, 1))
    return hi, lo


def pair_value(hi, lo):
    return hi.double() + lo.double() / 2048.0


# ------------------------------------------------------------------ ConvGRU

def _gru_pre(gates_pre, c, wrong):
    r_pre, z_pre = gates_pre[:, :c], gates_pre[:, c:]
    if wrong == 'rz':                                   # r and z read from each other's half
        r_pre, z_pre = z_pre, r_pre
    if wrong == 'batch0':                               # batch 0's gate for every batch
        r_pre, z_pre = r_pre[:1].expand_as(r_pre), z_pre[:1].expand_as(z_pre)
    return r_pre, z_pre


def gru_gates(gates_pre, x, h, wrong=None):
    """cat[x, sigmoid(r_pre) * h]."""
    r_pre, _ = _gru_pre(gates_pre, x.shape[1], wrong)
    return torch.cat([x, torch.sigmoid(r_pre) * h], 1)


def gru_candidate(cand_pre, prelu_w=None, wrong=None):
    if prelu_w is None:
        return torch.tanh(cand_pre)
    if wrong == 'slope':                                # the slope of channel c - 1 for channel c
        prelu_w = torch.roll(prelu_w, 1)
    return torch.where(cand_pre >= 0, cand_pre, cand_pre * prelu_w[None, :, None, None])


def gru_update(gates_pre, cand_pre, h, prelu_w=None, x_next=None, wrong=None):
    """(h', cat[x_next, h'] or None)."""
    _, z_pre = _gru_pre(gates_pre, h.shape[1], wrong)
    z, cand = torch.sigmoid(z_pre), gru_candidate(cand_pre, prelu_w, wrong)
    if wrong == 'keep_take':                            # (1 - z) and z exchanged
        z = 1 - z
    h_new = (1 - z) * h + z * cand
    return h_new, (None if x_next is None else torch.cat([x_next, h_new], 1))


# ------------------------------------------------------------------ squeeze-and-excitation tail

def se_parts(v, w1, w2, wrong=None):
    """{'pooled' [B,C], 'hidden' [B,R], 'pre' [B,C] gate pre-activations, 'gate' [B,C]}."""
    b, c, h, w = v.shape
    r = w1.shape[0]
    pooled = v.sum((2, 3)) / (-(-h * w // 256) * 256 if wrong == 'mean256' else h * w)      # H * W rounded up to the 256 threads
    w1_used = w1
    if wrong == 'lanes':                                # the partial 64-lane pass of the squeeze dropped
        w1_used = w1.clone()
        w1_used[:, c // 64 * 64:] = 0
    hidden = torch.relu(pooled @ w1_used.T)
    if wrong == 'waves':                                # the ragged end of the round-robin over the 4 waves dropped
        hidden = hidden.clone()
        hidden[:, r // 4 * 4:] = 0
    pre = hidden @ w2.T
    gate = torch.sigmoid(pre)
    if wrong == 'batch0':
        gate = gate[:1].expand_as(gate)
    return {'pooled': pooled, 'hidden': hidden, 'pre': pre, 'gate': gate}


def se_tail(v, shortcut, w1, w2, wrong=None):
    """v * sigmoid(w2 relu(w1 mean_hw v)) + shortcut."""
    return v * se_parts(v, w1, w2, wrong)['gate'][:, :, None, None] + shortcut


def se_next(out, next_scale, next_shift, wrong=None):
    """out * next_scale[b][c] + next_shift[b][c]: the value ``ia_se_gate_split`` stores as fp16 pairs."""
    if wrong == 'batch0':
        next_scale = next_scale[:1].expand_as(next_scale)
    return out * next_scale[:, :, None, None] + next_shift[:, :, None, None]


# ------------------------------------------------------------------ bilinear upsample-add

def _axis_taps(n_in, n_out, dtype, wrong=None):
    dst = torch.arange(n_out, dtype=dtype)
    if wrong == 'half_pixel':                           # the source index of align_corners=False
        src = ((dst + 0.5) * (n_in / n_out) - 0.5).clamp(min=0)
    else:
        src = dst * ((n_in - 1) / (n_out - 1) if n_out > 1 else 0.0)
    i0 = src.floor().clamp(max=n_in - 1)
    frac = src - i0
    i0 = i0.long()
    return i0, (i0 + 1).clamp(max=n_in - 1), frac


def upsample_add(x, y, wrong=None):
    """Bilinear resize of x [B,C,H,W] to y's size with align_corners=True, plus y; explicit indexing."""
    y0, y1, fy = _axis_taps(x.shape[2], y.shape[2], x.dtype, wrong)
    x0, x1, fx = _axis_taps(x.shape[3], y.shape[3], x.dtype, wrong)
    fy = fy[:, None]
    top = x[:, :, y0][:, :, :, x0] * (1 - fx) + x[:, :, y0][:, :, :, x1] * fx
    bottom = x[:, :, y1][:, :, :, x0] * (1 - fx) + x[:, :, y1][:, :, :, x1] * fx
    return top * (1 - fy) + bottom * fy + y


def upsample_add_aten(x, y):
    return torch.nn.functional.interpolate(x, size=y.shape[2:], mode='bilinear', align_corners=True) + y


# ------------------------------------------------------------------ depth-wise token convolution

def dwconv_tokens(x, w9c, bias, h, w, gelu=False, wrong=None):
    """x [B, h*w, C], w9c [9, C] (tap ky * 3 + kx), bias [C] or None -> [B, h*w, C]; taps outside the grid count as 0."""
    b, n, c = x.shape
    assert n == h * w and tuple(w9c.shape) == (9, c)
    taps = w9c.reshape(3, 3, c)
    if wrong == 'transposed':                           # ky <-> kx
        taps = taps.transpose(0, 1)
    padded = torch.zeros(b, h + 2, w + 2, c, dtype=x.dtype)
    padded[:, 1:h + 1, 1:w + 1] = x.reshape(b, h, w, c)
    out = torch.zeros(b, h, w, c, dtype=x.dtype) if bias is None else bias.expand(b, h, w, c).clone()
    for ky in range(3):
        for kx in range(3):
            out = out + padded[:, ky:ky + h, kx:kx + w] * taps[ky, kx]
    if gelu:
        out = 0.5 * out * (1 + torch.erf(out * math.sqrt(0.5)))
    return out.reshape(b, n, c)


def dwconv_tokens_aten(x, w9c, bias, h, w, gelu=False):
    b, n, c = x.shape
    y = torch.nn.functional.conv2d(x.transpose(1, 2).reshape(b, c, h, w), w9c.t().reshape(c, 1, 3, 3), bias, padding=1, groups=c)
    y = y.flatten(2).transpose(1, 2)
    return torch.nn.functional.gelu(y) if gelu else y


# ------------------------------------------------------------------ attention

def attention_logits(q, kv, heads, scale):
    """[B, heads, N, M]."""
    b, n, c = q.shape
    m, hd = kv.shape[1], c // heads
    qh = q.reshape(b, n, heads, hd).permute(0, 2, 1, 3)
    kh = kv[..., :c].reshape(b, m, heads, hd).permute(0, 2, 1, 3)
    return (qh @ kh.transpose(-2, -1)) * scale


def attention(q, kv, heads, scale, wrong=None):
    """softmax(q k^T * scale) v per head: q [B,N,C], kv [B,M,2C] -> [B,N,C]."""
    b, n, c = q.shape
    if wrong == 'key_m_included':                       # the mask one key too long: a zero-filled key with a zero value takes part
        kv = torch.cat([kv, torch.zeros_like(kv[:, :1])], 1)
    if wrong == 'last_key_dropped':                     # the mask one key too short
        kv = kv[:, :-1]
    m, hd = kv.shape[1], c // heads
    vh = kv[..., c:].reshape(b, m, heads, hd).permute(0, 2, 1, 3)
    s = attention_logits(q, kv, heads, scale)
    if wrong == 'no_rescale':
        return attention_online(s, vh, rescale=False).transpose(1, 2).reshape(b, n, c)
    return (s.softmax(-1) @ vh).transpose(1, 2).reshape(b, n, c)


def attention_online(s, vh, tile=32, rescale=True):
    """The online softmax over key tiles, as the one-launch kernels walk them: logits s [B,heads,N,M], values vh [B,heads,M,hd] ->
    [B,heads,N,hd].  ``rescale=False`` leaves out the factor exp(m_old - m_new) on the running sum and accumulator."""
    m_run = torch.full(s.shape[:-1], -math.inf, dtype=s.dtype)
    l_run = torch.zeros(s.shape[:-1], dtype=s.dtype)
    acc = torch.zeros(*s.shape[:-1], vh.shape[-1], dtype=s.dtype)
    for k0 in range(0, s.shape[-1], tile):
        st = s[..., k0:k0 + tile]
        m_new = torch.maximum(m_run, st.max(-1).values)
        fac = torch.exp(m_run - m_new) if rescale else torch.ones_like(m_new)
        p = torch.exp(st - m_new[..., None])
        l_run = l_run * fac + p.sum(-1)
        acc = acc * fac[..., None] + p @ vh[:, :, k0:k0 + tile]
        m_run = m_new
    return acc / l_run[..., None]


# ------------------------------------------------------------------ seeded inputs

def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).float()


GRU_SHAPES = ((1, 8, 2, 2), (3, 24, 6, 10), (2, 40, 5, 12), (1, 8, 36, 36))       # (B, C, H, W)
GRU_PLANTED = (0.0, 20.0, -20.0, 90.0, -90.0, 104.0, -104.0)

_cache = {}


def _cached(fn):
    def get(*key):
        k = (fn.__name__,) + key
        if k not in _cache:
            _cache[k] = fn(*key)
        return _cache[k]
    return get


def gru_planted_positions(c, h, w):
    """Flat positions inside a C*H*W half of ``gates_pre`` that hold GRU_PLANTED: (r half, z half)."""
    n = c * h * w
    pos = np.arange(len(GRU_PLANTED)) * (n // len(GRU_PLANTED))
    return pos + 1, pos + 2


@_cached
def gru_inputs(b, c, h, w):
    """float32 {'gates_pre' [B,2C,H,W], 'cand_pre', 'x', 'h', 'x_next' [B,C,H,W], 'prelu_w' [C]}.  Pre-activations randn * 6 with
    GRU_PLANTED in both halves of every batch element; candidates randn * 4 with +-20 planted; x, h, x_next N(0,1) scaled per channel
    by logspace(-6, 2); slopes all different, of both signs, one exactly 0."""
    rs = np.random.RandomState(7000 + 131 * b + 17 * c + h * w)
    n = c * h * w
    scale = np.logspace(-6, 2, c)[None, :, None, None]
    x, hh, x_next = (rs.randn(b, c, h, w) * scale for _ in range(3))
    g = rs.randn(b, 2, n) * 6.0
    for half, pos in enumerate(gru_planted_positions(c, h, w)):
        g[:, half, pos] = GRU_PLANTED
    cand = rs.randn(b, n) * 4.0
    cand[:, 3], cand[:, n - 5] = 20.0, -20.0
    slopes = np.linspace(-0.5, 0.9, c)
    slopes[1] = 0.0
    return {'gates_pre': _t(g.reshape(b, 2 * c, h, w)), 'cand_pre': _t(cand.reshape(b, c, h, w)), 'x': _t(x), 'h': _t(hh), 'x_next': _t(x_next),
            'prelu_w': _t(slopes)}


SE_SHAPES = ((1, 16, 1, 1, 1), (3, 24, 3, 5, 7), (2, 200, 12, 9, 14), (1, 64, 64, 4, 4), (1, 8, 2, 132, 128), (2, 8, 2, 128, 128))   # (B, C, R, H, W)
SE_LAYOUTS = ('contiguous', 'every_second_pixel', 'channel_slice')


@_cached
def se_inputs(b, c, r, h, w):
    """float32 {'v', 'shortcut' [B,C,H,W], 'w1' [R,C], 'w2' [C,R], 'next_scale', 'next_shift' [B,C]}.  v = randn + 3 cos(c); w1 ~
    N(0, 1/sqrt(C)), negated if the ReLU would zero more than half of the hidden units; w2 scaled so that the gate pre-activations have
    a standard deviation of 4."""
    rs = np.random.RandomState(8000 + 131 * b + 17 * c + 5 * r + h * w)
    v = _t(rs.randn(b, c, h, w) + 3.0 * np.cos(np.arange(c))[None, :, None, None])
    shortcut = _t(rs.randn(b, c, h, w))
    w1 = _t(rs.randn(r, c) / np.sqrt(c))
    w2 = _t(rs.randn(c, r))
    if float((se_parts(v.double(), w1.double(), w2.double())['hidden'] <= 0).double().mean()) > 0.5:
        w1 = -w1
    pre = se_parts(v.double(), w1.double(), w2.double())['pre']
    w2 = (w2.double() * (4.0 / float(pre.std()))).float()
    return {'v': v, 'shortcut': shortcut, 'w1': w1, 'w2': w2, 'next_scale': _t(0.5 + rs.rand(b, c)), 'next_shift': _t(rs.randn(b, c))}


def se_layout(t, layout):
    """A view with the values of t [B,C,H,W] (on t's device) in one of SE_LAYOUTS; whatever else its storage holds is NaN.
    'every_second_pixel': [:, :, ::2, ::2] of a tensor twice the size; 'channel_slice': channels 3 .. 3+C of a channels-last tensor
    with C + 5 channels, so that the batch stride is not C * H * W."""
    b, c, h, w = t.shape
    if layout == 'contiguous':
        return t.contiguous()
    if layout == 'every_second_pixel':
        big = torch.full((b, c, 2 * h, 2 * w), float('nan'), device=t.device)
        view = big[:, :, ::2, ::2]
    else:
        assert layout == 'channel_slice'
        big = torch.full((b, h, w, c + 5), float('nan'), device=t.device)
        view = big.permute(0, 3, 1, 2)[:, 3:3 + c]
    view.copy_(t)
    return view


UPSAMPLE_SHAPES = (((1, 3), 1, 1, 5, 4), ((2, 1), 1, 9, 7, 9), ((1, 5), 7, 9, 7, 9), ((3, 1), 7, 3, 100, 97), ((1, 2), 33, 2, 34, 64))   # ((B, C), H, W, OH, OW)


@_cached
def upsample_inputs(bc, h, w, oh, ow):
    rs = np.random.RandomState(9000 + 31 * h + w + 7 * oh)
    return _t(rs.randn(*bc, h, w)), _t(rs.randn(*bc, oh, ow))


DWCONV_SHAPES = ((2, 5, 7, 144), (1, 1, 9, 16), (3, 4, 1, 48))          # (B, H, W, C)


@_cached
def dwconv_inputs(b, h, w, c):
    """(x [B, H*W, C], w9c [9, C], bias [C]) float32; the taps are random, so not symmetric in ky <-> kx."""
    rs = np.random.RandomState(9500 + 31 * h + w + c)
    return _t(rs.randn(b, h * w, c)), _t(rs.randn(9, c) * 0.3), _t(rs.randn(c))


ATT_HEADS, ATT_HEAD_DIM = 4, 256
ATT_SCALE = ATT_HEAD_DIM ** -0.5
ATT_SHAPES = ((1, 1, 1), (2, 33, 33), (1, 40, 63), (1, 64, 97))          # (B, N, M)
ATT_SX_SHAPES = ((2, 33, 48), (1, 40, 64), (1, 64, 96))                  # key counts ia_attention_sx takes (multiples of 16)
ATT_ORDERS = ('random', 'rising', 'falling')


@_cached
def attention_inputs(b, n, m, order):
    """(q [B,N,C], kv [B,M,2C]) float32, C = 4 heads x 256.  'random': q, k = randn * 1.7 (logits about N(0, 2.9^2), the running maximum
    moves up every few keys).  'rising' / 'falling': k_j = a_j d + 0.1 randn, q = d + 0.3 randn with d = +-1 per component and a_j
    monotone over -2.5 .. 2.5, so that every query's logits run monotonically over about +-40.  v_j = randn * logspace(-2, 2)[j]."""
    c = ATT_HEADS * ATT_HEAD_DIM
    rs = np.random.RandomState(9900 + 131 * b + 17 * n + m + 1000 * ATT_ORDERS.index(order))
    v = rs.randn(b, m, c) * np.logspace(-2, 2, m)[None, :, None]
    if order == 'random':
        q, k = rs.randn(b, n, c) * 1.7, rs.randn(b, m, c) * 1.7
    else:
        d = np.where(rs.rand(c) < 0.5, -1.0, 1.0)
        a = np.linspace(-2.5, 2.5, m) if order == 'rising' else np.linspace(2.5, -2.5, m)
        k = a[None, :, None] * d + 0.1 * rs.randn(b, m, c)
        q = d + 0.3 * rs.randn(b, n, c)
    return _t(q), _t(np.concatenate([k, v], -1))
