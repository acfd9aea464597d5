"""Plain torch / numpy restatements of the kernels between the backbones and the renderer (csrc/rasterize.hip, csrc/fill_mouth.hip,
csrc/ray_sampler.hip, csrc/styles.hip, layout_grid_u8 of csrc/output.hip), the seeded case tables that
tests/test_frame_glue_reference_cpu.py and tests/test_frame_glue_gpu.py share, and a restatement of the per-workgroup decisions of
``rasterize_level_kernel`` (``rasterize_forms``) that lets the tables be checked for coverage without a device.  No device code.

Every restatement computes in the dtype of its arguments: with float64 tensors it is the reference ``r``, with float32 tensors the
yardstick whose own distance to float64 on the same inputs is ``e32``.  The tolerance rule, per element of a float32 kernel result:

    |got - r| <= 4 * e32 + 2^-24 * max|r|                       (``tolerance``)
    merged form of the rasteriser:  + 4 * n_src * 2^-40 * max|tex|      (``FIXED_POINT``; see ``rasterize_tolerance``)

Where a kernel is documented to give the same bits as an expression (copies, cond_blend, the split pairs, layout_grid, fill_mouth,
mouth_edge_blur) the tests assert ``torch.equal``.

Restatements take ``wrong=<name>``: the plausible errors of such kernels, written out so that the CPU test can show that the tables tell
each of them from the right result by at least ten times the tolerance on every case the error can show on.

Definitions restated:
  rasterize_level (header of csrc/rasterize.hip):  rend = AA(grid_sample(tex, uv; bilinear, zeros, align_corners=False), 256 -> res);
      a = AA(alpha); s = AA(sta[:, :C, crop], crop -> res);  out[:, :C] = rend * a + s * (1 - a);  out[:, C] = AA(upper).
      A bilinear tap outside the texture adds nothing, and so does every tap of a pixel whose UV is not finite (the kernel's clamps
      send NaN, +-inf and +-1e9 into the zero padding).
  AA: aten's separable anti-aliased triangle filter (_upsample_bilinear2d_aa): taps [int(c - s + .5), int(c + s + .5)) clipped,
      c = scale (o + .5), s = max(scale, 1), weights max(0, 1 - |(j - c + .5) / s|) normalised over the taps kept.
  blend_planes:  plane 0 inside the bbox = AA(stitch, 256 -> n) * AA(alpha) + static * (1 - AA(alpha)); the rest a copy; channels-last.
  fill_mouth:  4-connected breadth-first fill from (0, 0) over the pixels with seed <= fl32(a * 255) <= seed + 254;
      mouth = (255 - a * 255) / 255 off the filled region, 0 on it.
"""
import collections
import zlib
from typing import NamedTuple, Optional

import numpy as np
import torch

from invertavatar_amd import synthetic
from resample_reference import split_pair                 # noqa: F401  (the split pair is defined once, there)
from test_generator_cpu import _soft_mouth_by_loops as mouth_edge_blur_by_loops      # noqa: F401  (the restatement pinned there)

F64 = torch.float64
EPS32 = 2.0 ** -24
FIXED_POINT = 2.0 ** -40
KSRC = 256                           # the UV / alpha maps are 256 x 256
BBOX_256 = (57, 185, 64, 192)


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


# ------------------------------------------------------------------ tolerances

def tolerance(ref, e32, extra=0.0):
    """Per-element bound of a float32 kernel result against the float64 reference `ref`."""
    return torch.full_like(ref, 4.0 * float(e32) + EPS32 * float(ref.abs().max()) + float(extra))


def e32_of(ref32, ref):
    return float((ref32.double() - ref).abs().max())


def rasterize_tolerance(ref, e32, n_src, tex_max):
    """The merged form sums (AA weight x bilinear weight) products per texel as 2^40 fixed point: every product is truncated to a
    multiple of 2^-40 (error < 2^-40), an output pixel takes 4 bilinear taps of each of the n_src source pixels of its footprint, and
    each of those products multiplies a texel of magnitude <= max|tex|: at most 4 * n_src * 2^-40 * max|tex| (6e-10 * max|tex| for the
    widest footprint, 640 pixels; the conversion of a sum back to float32 is an ordinary rounding, inside the factor 4 of e32)."""
    return tolerance(ref, e32, 4.0 * n_src * FIXED_POINT * tex_max)


# ------------------------------------------------------------------ anti-aliased resize, grid_sample

def aa_taps(o, n_in, n_out, ft=np.float32, shift=0.5):
    """(lo, hi, weights [hi - lo] not yet normalised, their sequential sum) of output o, every operation in `ft`, as aten and the kernels."""
    scale = ft(n_in) / ft(n_out)
    support = scale if scale >= 1 else ft(1)
    inv = ft(1) / scale if scale >= 1 else ft(1)
    center = ft(scale * ft(ft(o) + ft(shift)))
    lo, hi = max(int(ft(center - support) + ft(0.5)), 0), min(int(ft(center + support) + ft(0.5)), n_in)
    j = np.arange(lo, hi).astype(ft)
    w = np.maximum(ft(0), ft(1) - np.abs((j - center + ft(0.5)) * inv)).astype(ft)
    total = ft(0)
    for v in w:
        total = ft(total + v)
    return lo, hi, w, total, support


@_cached
def _aa_matrix(n_in, n_out, f64, wrong):
    ft = np.float64 if f64 else np.float32
    m = np.zeros((n_out, n_in), ft)
    for o in range(n_out):
        lo, hi, w, total, support = aa_taps(o, n_in, n_out, ft, 0.0 if wrong == 'aa_shift' else 0.5)
        m[o, lo:hi] = w / (support if wrong == 'aa_unnormalised' else total)
    return torch.from_numpy(m)


def aa_resize(x, size, wrong=None):
    """F.interpolate(x, size, mode='bilinear', antialias=True): the horizontal pass, then the vertical one.
    wrong: 'aa_shift' (centre scale * o), 'aa_unnormalised' (weights divided by the support, not by the sum of the taps kept)."""
    wrong = wrong if wrong in ('aa_shift', 'aa_unnormalised') else None
    f64 = x.dtype == F64
    y = torch.einsum('pw,nchw->nchp', _aa_matrix(x.shape[3], size[1], f64, wrong), x)
    return torch.einsum('oh,nchp->ncop', _aa_matrix(x.shape[2], size[0], f64, wrong), y)


def grid_sample(img, grid, wrong=None):
    """F.grid_sample(img, grid, bilinear, zeros, align_corners=False), an explicit 4-tap gather; grid [N, Ho, Wo, 2] (x to width).
    A tap outside the image and every tap of a non-finite location add exactly nothing.
    wrong: 'align_corners', 'border' (edge value instead of zero), 'wrap' (an outside tap wraps into the texture)."""
    n, c, h, w = img.shape
    gx, gy = grid[..., 0].to(img.dtype), grid[..., 1].to(img.dtype)
    if wrong == 'align_corners':
        px, py = (gx + 1) * ((w - 1) / 2), (gy + 1) * ((h - 1) / 2)
    else:
        px, py = (gx + 1) * (w / 2) - 0.5, (gy + 1) * (h / 2) - 0.5
    finite = torch.isfinite(px) & torch.isfinite(py)
    px = torch.where(finite, px, torch.full_like(px, -4.0)).clamp(-4.0, w + 4.0)
    py = torch.where(finite, py, torch.full_like(py, -4.0)).clamp(-4.0, h + 4.0)
    x0, y0 = torch.floor(px), torch.floor(py)
    fx, fy = px - x0, py - y0
    x0, y0 = x0.long(), y0.long()
    out = img.new_zeros(n, c, *gx.shape[1:])
    flat = img.reshape(n, c, h * w)
    for dy, wy in ((0, 1 - fy), (1, fy)):
        for dx, wx in ((0, 1 - fx), (1, fx)):
            xi, yi = x0 + dx, y0 + dy
            ok = (xi >= 0) & (xi < w) & (yi >= 0) & (yi < h)
            if wrong == 'wrap':
                xi, yi, ok = xi % w, yi % h, finite
            elif wrong == 'border':
                ok = finite
            idx = (yi.clamp(0, h - 1) * w + xi.clamp(0, w - 1)).reshape(n, 1, -1).expand(-1, c, -1)
            tap = torch.gather(flat, 2, idx).reshape(n, c, *gx.shape[1:])
            out = out + tap * torch.where(ok, wx * wy, torch.zeros_like(wx)).unsqueeze(1)
    return out


WRONG_RASTERIZE = ('align_corners', 'aa_shift', 'aa_unnormalised', 'alpha_after_blend', 'one_minus_a_on_render', 'crop_origin', 'border', 'wrap',
                   'upper_unresized')


def rasterize_level(tex, uv, upper, sta, crop, res, wrong=None):
    """tex [B, C, Rt, Rt]; uv [B, 256, 256, 3] (u, v, alpha); upper [B, 256, 256]; sta [B, >= C, Rs, Rs]; crop (y0, y1, x0, x1) of sta
    -> [B, C + 1, res, res].  Computes in tex.dtype."""
    dt, c = tex.dtype, tex.shape[1]
    grid, alpha = uv[..., :2], uv[..., 2][:, None].to(dt)
    y0, y1, x0, x1 = crop
    if wrong == 'crop_origin':
        y0, y1, x0, x1 = 0, y1 - y0, 0, x1 - x0
    a = aa_resize(alpha, (res, res), wrong)
    s = aa_resize(sta[:, :c, y0:y1, x0:x1].to(dt), (res, res), wrong)
    step = KSRC // res
    up = upper[:, None, step // 2::step, step // 2::step].to(dt) if wrong == 'upper_unresized' else aa_resize(upper[:, None].to(dt), (res, res), wrong)
    parts = []
    for c0 in range(0, c, 64):                           # (the 256^2 x C sampled image is never held whole)
        g = grid_sample(tex[:, c0:c0 + 64], grid, wrong)
        sc = s[:, c0:c0 + 64]
        if wrong == 'alpha_after_blend':
            parts.append(aa_resize(g * alpha, (res, res)) + sc * (1 - a))
        elif wrong == 'one_minus_a_on_render':
            parts.append(aa_resize(g, (res, res)) * (1 - a) + sc * a)
        else:
            parts.append(aa_resize(g, (res, res), wrong) * a + sc * (1 - a))
    return torch.cat(parts + [up], 1)


WRONG_BLEND = ('aa_shift', 'aa_unnormalised', 'bbox_swapped')


def blend_planes(stitch, full_alpha, static_planes, bbox, wrong=None):
    """stitch [B, 32, 256, 256], full_alpha [B, 1, 256, 256], static_planes [B, 96, 256, 256], bbox (y0, y1, x0, x1) -> [B, 3, 256, 256, 32]."""
    y0, y1, x0, x1 = bbox
    n = y1 - y0
    if wrong == 'bbox_swapped':
        y0, y1, x0, x1 = x0, x1, y0, y1
    planes = static_planes.reshape(-1, 3, 32, KSRC, KSRC).clone()
    s, a = aa_resize(stitch, (n, n), wrong), aa_resize(full_alpha, (n, n), wrong)
    planes[:, 0, :, y0:y1, x0:x1] = s * a + planes[:, 0, :, y0:y1, x0:x1] * (1 - a)
    return planes.permute(0, 1, 3, 4, 2).contiguous()


def cond_blend(cond, x):
    """networks_stylegan2_new.py:537-540: four elementwise operations, in this order."""
    a = cond[:, -1:]
    return cond[:, :-1] * a + x * (1 - a)


def channels_last(t):
    return t.permute(0, 2, 3, 1).contiguous()


# ------------------------------------------------------------------ path classifier of rasterize_level_kernel

WIN_W, WIN_H, CHUNK, PXB = 16, 8, 128, 4
_BIG = 1 << 20


def _windows(t, s, fill):
    """[B, 256, 256] -> [B, res, res / 4, 2 s * 5 s]: the AA footprint of every workgroup (rows [s y - s/2, s y + 3 s/2), columns
    [4 s xt - s/2, 4 s xt + 9 s/2), clipped to the map: `fill` outside)."""
    p = torch.nn.functional.pad(t, (s // 2, s // 2, s // 2, s // 2), value=fill)
    w = p.unfold(1, 2 * s, s).unfold(2, 5 * s, 4 * s)
    return w.reshape(*w.shape[:3], -1)


def rasterize_forms(uv, tex_res, res, C, crop):
    """The decisions of rasterize_level_kernel per workgroup (4 adjacent output pixels of one row), restated from the kernel in its
    own float32 arithmetic.  Returns a dict: 'form' [B, res, res/4] of 'none' / 'one' / 'two' / 'direct' (as 0..3, see FORMS), 'n_src'
    (footprint pixels), 'passes' (128-pixel passes of the direct form, 0 otherwise), 'a_w', 'a_h' (extent of the bounding box of all
    bilinear cells: window A holds it when a_w <= 16 and a_h <= 8), 'b_w', 'b_h' (extent of the box of the cells A leaves; 0 if none),
    and the scalars 'CV', 'lanes', 'threads', 'nsplit', 'channel_passes', 'crop_tabulated' [res, res/4] (False = the looped resize)."""
    s, rt = KSRC // res, int(tex_res)
    g = uv[..., :2].float().numpy()
    half = np.float32(0.5) * np.float32(rt)
    with np.errstate(invalid='ignore', over='ignore'):
        ix = (g[..., 0] + np.float32(1)) * half - np.float32(0.5)
        iy = (g[..., 1] + np.float32(1)) * half - np.float32(0.5)
        # fminf(fmaxf(floorf(i), -2), Rt + 1): fmaxf returns the other operand for a NaN
        x0 = np.where(np.isnan(ix), -2, np.clip(np.floor(ix), -2, rt + 1)).astype(np.int64)
        y0 = np.where(np.isnan(iy), -2, np.clip(np.floor(iy), -2, rt + 1)).astype(np.int64)
    x0, y0 = torch.from_numpy(x0), torch.from_numpy(y0)
    lx, hx, ly, hy = x0.clamp_min(0), (x0 + 1).clamp_max(rt - 1), y0.clamp_min(0), (y0 + 1).clamp_max(rt - 1)
    valid = (lx <= hx) & (ly <= hy)
    inside = _windows(torch.ones_like(valid), s, False)                           # footprint pixels inside the map
    vw = _windows(valid, s, False)
    lo = lambda t, keep: torch.where(keep, _windows(t, s, 0), torch.full((), _BIG)).amin(-1)      # noqa: E731
    hi = lambda t, keep: torch.where(keep, _windows(t, s, 0), torch.full((), -_BIG)).amax(-1)     # noqa: E731
    ax0, ay0, ax1, ay1 = lo(lx, vw), lo(ly, vw), hi(hx, vw), hi(hy, vw)
    none = ~vw.any(-1)
    one = none | ((ax1 - ax0 < WIN_W) & (ay1 - ay0 < WIN_H))
    in_a = ~vw | ((_windows(hx, s, 0) - ax0[..., None] < WIN_W) & (_windows(hy, s, 0) - ay0[..., None] < WIN_H))
    left = inside & ~in_a & ~one[..., None]
    bx0, by0, bx1, by1 = lo(lx, left), lo(ly, left), hi(hx, left), hi(hy, left)
    has_b = left.any(-1)
    merged = one | ((bx1 - bx0 < WIN_W) & (by1 - by0 < WIN_H))
    form = torch.where(none, 0, torch.where(one, 1, torch.where(merged, 2, 3)))
    n_src = inside.sum(-1)
    zero = torch.zeros_like(ax0)
    cv = 4 if C % 4 == 0 else 1
    ncq = (C + cv - 1) // cv
    threads = 64 if ncq <= 64 else 128 if ncq <= 128 else 256
    lanes = min(ncq, threads)
    y0c, y1c, x0c, x1c = crop
    rows = [aa_taps(o, y1c - y0c, res)[:2] for o in range(res)]
    cols = [aa_taps(o, x1c - x0c, res)[:2] for o in range(res)]
    tab = torch.tensor([[rows[y][1] - rows[y][0] <= 3 and 0 < cols[xt + 3][1] - cols[xt][0] <= 6 for xt in range(0, res, PXB)] for y in range(res)])
    return {'form': form, 'n_src': n_src, 'passes': torch.where(form == 3, (n_src + CHUNK - 1) // CHUNK, zero),
            'a_w': torch.where(none, zero, ax1 - ax0 + 1), 'a_h': torch.where(none, zero, ay1 - ay0 + 1),
            'b_w': torch.where(has_b, bx1 - bx0 + 1, zero), 'b_h': torch.where(has_b, by1 - by0 + 1, zero),
            'CV': cv, 'lanes': lanes, 'threads': threads, 'nsplit': min(8, threads // lanes), 'channel_passes': -(-ncq // lanes), 'crop_tabulated': tab}


FORMS = ('none', 'one', 'two', 'direct')


# ------------------------------------------------------------------ ray sampler, styles, layout_grid

WRONG_RAYS = ('transposed_adjugate', 'scale_all_rows')


def ray_sampler(cam25, res, normalize=True, wrong=None):
    """RaySampler_zxc: K' = K with rows 0-1 scaled by res; d = normalize(R K'^-1 [i, j, 1]) (F.normalize: / max(|d|, 1e-12)); o = t.
    cam25 [B, 25] -> (rays_o, rays_d) [B, res^2, 3], x fastest.  The inverse is torch.linalg.inv in cam25.dtype."""
    c2w, k = cam25[:, :16].reshape(-1, 4, 4), cam25[:, 16:25].reshape(-1, 3, 3).clone()
    if wrong == 'scale_all_rows':
        k = k * res
    else:
        k[:, :2] = k[:, :2] * res
    kinv = torch.linalg.inv(k)
    if wrong == 'transposed_adjugate':
        kinv = kinv.transpose(1, 2)
    pix = torch.arange(res, dtype=cam25.dtype)
    jj, ii = torch.meshgrid(pix, pix, indexing='ij')
    homog = torch.stack([ii, jj, torch.ones_like(ii)], -1).reshape(-1, 3)
    d = (homog @ kinv.transpose(1, 2)) @ c2w[:, :3, :3].transpose(1, 2)
    if normalize:
        d = d / d.norm(dim=-1, keepdim=True).clamp_min(1e-12)
    return c2w[:, :3, 3][:, None].expand_as(d).contiguous(), d


def cameras(kind):
    """[B, 25] float32.  'skewed': three different cameras whose intrinsics have skew, an off-centre principal point and a non-zero bottom
    row (every cofactor of the inverse multiplies something); 'zero_rotation': camera 1 has a zero rotation block, so its directions
    have length 0 and normalisation divides by the eps."""
    cams = synthetic.camera_labels([3, 70, 160]).clone()
    rs = _rs('cameras')
    for b in range(3):
        cams[b, 16:25] = _t(np.array([[4.2 + 0.3 * b, 0.37 - 0.2 * b, 0.43 + 0.05 * b], [-0.21 + 0.1 * b, 3.9 - 0.25 * b, 0.58 - 0.04 * b],
                                      [0.013 * (b + 1), -0.021, 1.0 + 0.02 * b]]).reshape(-1))
        cams[b, [3, 7, 11]] += _t(rs.randn(3) * 0.1)
    if kind == 'zero_rotation':
        cams[1, :16].reshape(4, 4)[:3, :3] = 0
    return cams


WRONG_STYLES = ('no_bias_gain', 'no_eps')


def styles_demod(ws, layers, wrong=None):
    """ws [B, num_ws, w_dim]; layers: dicts of A [I, w_dim], bias [I] or None, wgain, bgain, widx, wsq [O, I] or None
    -> [(styles [B, I], demod [B, O] or None)]:  styles = ws[:, widx] @ (A wgain)^T + bias bgain;  demod = rsqrt(sum_i styles^2 wsq + 1e-8)."""
    out = []
    for l in layers:
        s = ws[:, l['widx']] @ (l['A'].to(ws.dtype) * l['wgain']).t()
        if l['bias'] is not None:
            s = s + l['bias'].to(ws.dtype) * (1.0 if wrong == 'no_bias_gain' else l['bgain'])
        d = None
        if l['wsq'] is not None:
            d = (s.square() @ l['wsq'].to(ws.dtype).t() + (0.0 if wrong == 'no_eps' else 1e-8)).rsqrt()
        out.append((s, d))
    return out


class Style(NamedTuple):
    """One modulated layer of a hand-made plan: affine [I, w_dim] (+ bias unless `bias` is False) with lr multiplier `lr`, conv weight
    [O, I, 3, 3] scaled by `wscale`, which ws row it reads, whether it demodulates."""
    I: int
    O: int
    widx: int
    demod: bool = True
    bias: bool = True
    lr: float = 1.0
    wscale: float = 1.0


# (w_dim, B, num_ws, layers).  I at the edges of the 64-lane loop of the demodulation, w_dim at the edges of the 64-lane x 4 loop of the
# styles; layers with and without demodulation mixed, one without a bias, lr multipliers != 1 (bias_gain), widx on the last ws row, and
# one demodulated layer with tiny weights (the sum under the rsqrt is of the order of the 1e-8).
STYLE_PLANS = (
    (4, 1, 2, (Style(1, 1, 0), Style(63, 5, 1, lr=0.5), Style(64, 1, 1, demod=False), Style(65, 5, 0, bias=False))),
    (252, 3, 3, (Style(65, 1, 2, lr=2.0), Style(1, 5, 0, demod=False), Style(64, 5, 2), Style(63, 1, 1, wscale=1e-4))),
    (256, 1, 2, (Style(64, 5, 1, bias=False, demod=False), Style(65, 5, 1, lr=0.25), Style(1, 1, 0, wscale=1e-4))),
    (260, 3, 4, (Style(63, 5, 3), Style(64, 1, 0, lr=0.5, wscale=1e-4), Style(65, 1, 3, demod=False, lr=3.0))),
    (512, 3, 2, (Style(64, 5, 1, lr=0.01), Style(65, 1, 0, bias=False), Style(1, 5, 1, demod=False), Style(63, 5, 1, wscale=1e-4))),
)


def style_inputs(plan):
    """(ws [B, num_ws, w_dim], per layer (affine weight [I, w_dim], bias [I] or None, conv weight [O, I, 3, 3])), float32."""
    w_dim, b, num_ws, layers = plan
    rs = _rs('styles', w_dim, b, num_ws)
    ws = _t(rs.randn(b, num_ws, w_dim))
    params = [(_t(rs.randn(l.I, w_dim) / l.lr), _t(1.0 + 0.3 * rs.randn(l.I)) if l.bias else None, _t(rs.randn(l.O, l.I, 3, 3) * l.wscale / (3.0 * l.I ** 0.5)))
              for l in layers]
    return ws, params


def style_layers(plan, dtype=F64):
    """The `layers` argument of ``styles_demod`` for a plan, with FullyConnectedLayer's gains (lr / sqrt(w_dim), lr)."""
    w_dim, _, _, layers = plan
    _, params = style_inputs(plan)
    return [dict(A=a.to(dtype), bias=None if bias is None else bias.to(dtype), wgain=l.lr / np.sqrt(w_dim), bgain=l.lr, widx=l.widx,
                 wsq=w.to(dtype).square().sum(dim=[2, 3]) if l.demod else None) for l, (a, bias, w) in zip(layers, params)]


def layout_grid(img, grid_w, grid_h, chw_to_hwc=True, wrong=None):
    """(img * 127.5 + 128).clamp(0, 255).to(uint8) in float32, a NaN giving 0; tiled grid_h x grid_w; CHW or HWC."""
    b, c, h, w = img.shape
    t = (img * 127.5 + 128).clamp(0, 255)
    if wrong == 'round':
        t = t.round()
    t = torch.where(t.isnan(), torch.zeros_like(t), t).to(torch.uint8)
    out = t.reshape(grid_h, grid_w, c, h, w).permute(2, 0, 3, 1, 4).reshape(c, grid_h * h, grid_w * w)
    return out.permute(1, 2, 0).contiguous() if chw_to_hwc else out.contiguous()


@_cached
def u8_edge_values():
    """float32 values v whose fl(fl(v * 127.5) + 128) lands on and on either side of every integer 0 .. 255: for each k the neighbours
    of (k - 128) / 127.5 that are the last to give less than k, the first and the last to give exactly k, and the first to give more.  Then values below 0 and above 255, +-inf and NaN."""
    vals = []
    for k in range(257):
        v0 = np.float32((k - 128.0) / 127.5)
        # candidates: the nextafter neighbours of v0, and steps of a quarter of the spacing of float32 at k (in units of v) to two spacings:
        # near v = 0 one step of v is far finer than one step of v * 127.5 + 128
        step = float(np.spacing(np.float32(max(k, 1)))) / 127.5 / 4
        c = np.unique(np.array([np.nextafter(v0, np.float32(-9)), np.nextafter(v0, np.float32(9))] + [v0 + j * step for j in range(-8, 9)], np.float32))
        t = (c * np.float32(127.5)).astype(np.float32) + np.float32(128)
        on = np.nonzero(t == k)[0]
        assert len(on) and (t < k).any() and (t > k).any(), k
        vals += [c[np.nonzero(t < k)[0][-1]], c[on[0]], c[on[-1]], c[np.nonzero(t > k)[0][0]]]
    special = np.array([-1.5, -1.0039216, -100.0, 1e30, -1e30, 1.5, 3.0, np.inf, -np.inf, np.nan, 0.0, -0.0], np.float32)
    return np.concatenate([np.array(vals, np.float32), special])


# (B, C, H, W, grid_w, grid_h)
LAYOUT_CASES = ((6, 3, 7, 12, 3, 2), (5, 1, 65, 4, 5, 1), (5, 4, 17, 4, 1, 5), (6, 4, 5, 12, 2, 3), (3, 3, 37, 4, 1, 3), (2, 1, 55, 12, 2, 1))


def layout_image(case, k):
    b, c, h, w = case[:4]
    vals = u8_edge_values()
    assert b * c * h * w >= len(vals)
    return torch.from_numpy(np.resize(np.roll(vals, 7 * k), (b, c, h, w)).copy())


# ------------------------------------------------------------------ fill_mouth

def passable_of(alpha):
    """[H, W] float32 array -> (passable, v): seed <= fl32(a * 255) <= fl32(seed + 254)."""
    v = np.asarray(alpha, np.float32) * np.float32(255)
    seed = v[0, 0]
    return (v >= seed) & (v <= np.float32(seed + np.float32(254))), v


def breadth_first(passable, eight=False):
    h, w = passable.shape
    seen = np.zeros((h, w), bool)
    seen[0, 0] = True
    queue = collections.deque([(0, 0)])
    steps = ((-1, 0), (1, 0), (0, -1), (0, 1)) + (((-1, -1), (-1, 1), (1, -1), (1, 1)) if eight else ())
    while queue:
        y, x = queue.popleft()
        for dy, dx in steps:
            yy, xx = y + dy, x + dx
            if 0 <= yy < h and 0 <= xx < w and passable[yy, xx] and not seen[yy, xx]:
                seen[yy, xx] = True
                queue.append((yy, xx))
    return seen


def sweep_fill(passable, max_rounds=None):
    """The kernels' propagation: a round = every row swept both ways (a reached pixel fills its whole horizontal run of passable pixels),
    then every column.  Returns (reached, rounds that reached a new pixel); stops after `max_rounds` rounds like a capped loop."""
    h, w = passable.shape
    row_id = np.cumsum(~passable, 1) + np.arange(h)[:, None] * (w + 1)
    col_id = np.cumsum(~passable, 0) + np.arange(w)[None, :] * (h + 1)
    reached = np.zeros((h, w), bool)
    reached[0, 0] = True
    rounds = 0
    while max_rounds is None or rounds < max_rounds:
        before = int(reached.sum())
        for ids in (row_id, col_id):
            hit = np.zeros(int(ids.max()) + 1, bool)
            hit[ids[reached]] = True
            reached = passable & hit[ids]
        if int(reached.sum()) == before:
            break
        rounds += 1
    return reached, rounds


WRONG_FILL = ('eight_connected', 'round_cap')


def fill_mouth(alpha, wrong=None):
    """alpha [H, W] float32 tensor -> mouth [H, W] float32.  wrong: 'eight_connected'; 'round_cap' (propagation stopped after H + W rounds,
    2 * 256 at 256 x 256)."""
    a = alpha.numpy().astype(np.float32)
    passable, v = passable_of(a)
    if wrong == 'round_cap':
        reached, _ = sweep_fill(passable, 512 if a.shape == (256, 256) else a.shape[0] + a.shape[1])
    else:
        reached = breadth_first(passable, wrong == 'eight_connected')
    return torch.from_numpy(np.where(reached, np.float32(0), (np.float32(255) - v) / np.float32(255)).astype(np.float32))


@_cached
def maze(h, w, seed=1):
    """alpha [h, w]: a depth-first maze, cells on the even pixels (alpha 0), walls alpha 1, entered at (0, 0): a corridor that turns at
    almost every step, which is the worst case of line sweeps."""
    ch, cw = (h + 1) // 2, (w + 1) // 2
    rs = np.random.RandomState(seed)
    open_ = np.zeros((h, w), bool)
    seen = np.zeros((ch, cw), bool)
    seen[0, 0] = open_[0, 0] = True
    stack = [(0, 0)]
    while stack:
        y, x = stack[-1]
        nxt = [(yy, xx) for yy, xx in ((y - 1, x), (y + 1, x), (y, x - 1), (y, x + 1)) if 0 <= yy < ch and 0 <= xx < cw and not seen[yy, xx]]
        if not nxt:
            stack.pop()
            continue
        yy, xx = nxt[rs.randint(len(nxt))]
        seen[yy, xx] = True
        open_[2 * yy, 2 * xx] = open_[y + yy, x + xx] = True
        stack.append((yy, xx))
    return _t(np.where(open_, 0.0, 1.0))


MAZES = ((64, 64), (45, 77), (256, 256))
FILL_LDS_BYTES = 150 * 1024
FILL_LARGEST, FILL_TOO_LARGE = (300, 508), (300, 509)            # H * (W + 4) = 153600 = the limit, and 153900


def _blobs(h, w, tag, lo=0.0, hi=1.0):
    """Smooth-ish random alpha in [lo, hi]: random values on a coarse lattice, repeated (blocks of 1 .. 3 pixels)."""
    rs = _rs('blobs', h, w, tag)
    k = 1 + rs.randint(3)
    coarse = rs.rand(-(-h // k), -(-w // k)) * (hi - lo) + lo
    return np.repeat(np.repeat(coarse, k, 0), k, 1)[:h, :w].astype(np.float32)


@_cached
def fill_case(name):
    """Named alpha masks [H, W] float32 of the fill_mouth table."""
    if name.startswith('maze'):
        return maze(*[int(v) for v in name.split()[1:]])
    h, w, kind = int(name.split()[0]), int(name.split()[1]), name.split()[2]
    rs = _rs('fill', name)
    if kind == 'face':              # alpha 0 outside, 1 on a disc, holes of 0 inside it (the mouth), and a few fractional pixels
        yy, xx = np.mgrid[0:h, 0:w]
        a = ((((yy - h / 2) / (0.4 * h + 0.5)) ** 2 + ((xx - w / 2) / (0.4 * w + 0.5)) ** 2) < 1).astype(np.float32)
        a[int(0.55 * h):int(0.7 * h) + 1, int(0.4 * w):int(0.6 * w) + 1] = 0
        a[int(0.3 * h), int(0.3 * w):int(0.45 * w) + 1] = 0.5
        if min(h, w) >= 9:
            a[0, w // 2], a[h - 1, w // 3], a[h // 2, 0], a[h // 3, w - 1] = 1, 1, 1, 1            # walls on the border itself
    elif kind == 'seed0.3':         # seed alpha 0.3: lower alphas are walls as well
        a = np.where(_blobs(h, w, 1) < 0.55, np.float32(0.3), _blobs(h, w, 2)).astype(np.float32)
        a[0, 0] = 0.3
    elif kind == 'seed1':           # seed alpha 1: only alphas >= 1 are passable
        a = np.where(_blobs(h, w, 3) < 0.6, np.float32(1.0), _blobs(h, w, 4)).astype(np.float32)
        a[0, 0] = 1.0
    elif kind == 'wide':            # alphas in [-0.5, 2]: the upper limit seed + 254 is reached, and pixels sit exactly on both limits
        a = _blobs(h, w, 5, -0.5, 2.0)
        a[0, 0] = -0.25
        lo = np.float32(-0.25)
        hi = np.float32(np.float32(lo * np.float32(255)) + np.float32(254)) / np.float32(255)
        flat = a.reshape(-1)
        picks = rs.permutation(h * w - 1)[:min(24, h * w - 1)] + 1
        for i, p in enumerate(picks):
            base = lo if i % 2 == 0 else hi
            flat[p] = (base, np.nextafter(base, np.float32(-9)), np.nextafter(base, np.float32(9)))[(i // 2) % 3]
    else:
        raise KeyError(name)
    return _t(a)


FILL_CASES = ('1 1 face', '1 9 face', '9 1 face', '3 3 face', '1 9 wide', '9 1 seed0.3', '3 3 wide', '255 256 face', '256 255 seed0.3', '257 256 wide',
              '256 256 face', '256 256 seed0.3', '256 256 seed1', '256 256 wide', '40 52 seed1', '40 52 wide', '40 52 seed0.3',
              f'{FILL_LARGEST[0]} {FILL_LARGEST[1]} face') + tuple(f'maze {h} {w}' for h, w in MAZES)

# (H, W) of the mouth_edge_blur table: below, at and across the 32-pixel tile
EDGE_BLUR_SIZES = ((3, 3), (4, 5), (7, 7), (32, 32), (33, 31), (64, 65))


@_cached
def edge_blur_case(h, w):
    """alpha [H, W]: ones with holes (0 and fractional) within 5 pixels of each border and of the tile seam at 32."""
    rs = _rs('edge blur', h, w)
    a = np.ones((h, w), np.float32)
    spots = [(1, 1), (0, w - 2), (h - 2, 0), (h - 1, w - 1), (h // 2, w // 2), (min(h - 1, 3), min(w - 1, 4))]
    if h > 32:
        spots += [(31, w // 3), (min(h - 1, 33), 2 * w // 3), (min(h - 1, 36), 3)]
    if w > 32:
        spots += [(h // 3, 30), (2 * h // 3, min(w - 1, 32)), (2, min(w - 1, 35))]
    for i, (y, x) in enumerate(spots):
        a[y, x] = 0 if i % 2 == 0 else np.float32(0.1 + 0.2 * rs.rand())
    if h >= 32 and w >= 31:
        a[10:14, 27:31] = 0
    return _t(a)


# ------------------------------------------------------------------ rasteriser case table

class Rast(NamedTuple):
    """One call of hipops.rasterize_level.  uv: kind of map (``uv_map``); tex_res None = res; crop 'half' (the product's bbox), or
    (y0, y1, x0, x1); sta_res None = res; sta_extra: channels of the wider tensor that `sta` is a slice of; alpha: 'mask' (the map's
    own), 'zero', 'one' or 'frac'."""
    name: str
    uv: str
    res: int
    C: int
    B: int = 1
    tex_res: Optional[int] = None
    crop: object = 'half'
    sta_res: Optional[int] = None
    sta_extra: int = 0
    alpha: str = 'mask'

    @property
    def rt(self):
        return self.res if self.tex_res is None else self.tex_res

    @property
    def rs(self):
        return self.res if self.sta_res is None else self.sta_res

    @property
    def bbox(self):
        return tuple(round(i * self.res / 256) for i in BBOX_256) if self.crop == 'half' else tuple(self.crop)


def _texel_grid(rt, offset):
    """u (= v) [256] whose un-normalised coordinate is exactly k + offset - 0.5 for texel k = floor(X rt / 256) (rt a power of two)."""
    k = (np.arange(KSRC) * rt) // KSRC
    return (2.0 * (k + offset) / rt - 1.0).astype(np.float32)


@_cached
def uv_map(kind, b, rt):
    """uvcoords_image [b, 256, 256, 3] float32 over the synthetic.uv_conditions base (u = x, v = y, disc mask with a mouth hole)."""
    uv = synthetic.uv_conditions([5, 60, 100][:b]).clone()
    u, v, m = uv[..., 0], uv[..., 1], uv[..., 2]
    lin = torch.linspace(-1, 1, KSRC)
    X = torch.arange(KSRC)
    kind, _, arg = kind.partition(':')
    if kind == 'face':
        pass
    elif kind == 'affine':                           # u = su x + ou, v = sv y + ov
        su, sv, ou, ov = [float(t) for t in arg.split(',')]
        u[:], v[:] = (lin * su + ou)[None, None, :], (lin * sv + ov)[None, :, None]
    elif kind == 'silhouette':                       # a constant background UV far from the face's texels
        bg = m < 0.5
        u[bg], v[bg] = -0.93, 0.91
    elif kind == 'seam':                             # three clusters, every third column its own: no two windows hold them
        off = torch.tensor([float(t) for t in arg.split(',')] if arg else [-0.8, 0.0, 0.8])[(X // 3) % 3]
        u[:], v[:] = (lin * (0.08 if arg else 0.15) + off)[None, None, :], (lin[:, None] * 0.15 + off[None, :] * 0.9)[None]
    elif kind == 'padding':                          # whole tiles in the zero padding; the right quarter back on the face
        u[:, :, :192] = -3.0
    elif kind == 'edges':                            # u = -1 and u = +1 exactly: half of every cell is in the padding
        u[:, :, :128], u[:, :, 128:] = -1.0, 1.0
        v[:, :64], v[:, 192:] = -1.0, 1.0
    elif kind == 'centres':                          # fx = fy = 0: the second tap of each axis has weight 0 (and is outside at the far edge)
        g = torch.from_numpy(_texel_grid(rt, 0.5))
        u[:], v[:] = g[None, None, :], g[None, :, None]
    elif kind == 'half_texel':                       # fx = fy = 0.5, the last cell half outside
        g = torch.from_numpy(_texel_grid(rt, 1.0))
        u[:], v[:] = g[None, None, :], g[None, :, None]
    elif kind in ('huge', 'nan'):
        vals = (1e9, -1e9, float('inf'), float('-inf')) if kind == 'huge' else (float('nan'),) * 4
        u[:, 100:120, 60:80], u[:, 100:120, 170:190], v[:, 60:80, 100:120], u[:, 125:140, 120:135] = vals
        if kind == 'nan':
            v[:, 125:140, 120:135] = float('nan')
    else:
        raise KeyError(kind)
    return uv.contiguous()


def rast_inputs(case):
    """float32 {'tex' [B, C, Rt, Rt], 'uv' [B, 256, 256, 3], 'upper' [B, 256, 256], 'sta_wide' [B, C + extra, Rs, Rs]} ('sta' of the call is
    sta_wide[:, extra:] when extra > 0: a channel slice that does not start at the tensor's first element)."""
    key = ('rast', case)
    if key not in _cache:
        rs = _rs('rast', case.name)
        uv = uv_map(case.uv, case.B, case.rt).clone()
        if case.alpha == 'zero':
            uv[..., 2] = 0
        elif case.alpha == 'one':
            uv[..., 2] = 1
        elif case.alpha == 'frac':
            uv[..., 2] = _t(rs.rand(case.B, KSRC, KSRC))
        _cache[key] = {'tex': _t(rs.randn(case.B, case.C, case.rt, case.rt)), 'uv': uv, 'upper': _t(rs.rand(case.B, KSRC, KSRC)),
                       'sta_wide': _t(rs.randn(case.B, case.C + case.sta_extra, case.rs, case.rs))}
    return _cache[key]


def rast_reference(case, dtype=F64, wrong=None):
    i = rast_inputs(case)
    return rasterize_level(i['tex'].to(dtype), i['uv'], i['upper'], i['sta_wide'][:, case.sta_extra:].to(dtype), case.bbox, case.res, wrong)


def rast_forms(case):
    key = ('forms', case)
    if key not in _cache:
        _cache[key] = rasterize_forms(rast_inputs(case)['uv'], case.rt, case.res, case.C, case.bbox)
    return _cache[key]


# Affine scales: a footprint is 1280 / res source pixels wide and 512 / res tall, i.e. 5.02 su x 2.01 sv texels when tex_res = res, plus
# the second texel of the last cell.  su = 3.0 puts the box of all cells at 16 and 17 texels (window A holds 16), sv = 3.3 at 8 and 9
# rows; su = 7.3 / sv = 7.1 put what A leaves at 16 / 17 columns and 8 / 9 rows (window B just fits, or the direct form).  The scales were
# chosen with ``rasterize_forms``; tests/test_frame_glue_reference_cpu.py asserts what they reach.
RAST_CASES = (
    # UV content
    Rast('face 32', 'face', 32, 8, B=3),
    Rast('face 64', 'face', 64, 36),
    Rast('face 128', 'face', 128, 4),
    Rast('A 16|17 wide', 'affine:3.0,1,0.1,0', 32, 5),
    Rast('A 16|17 wide 128', 'affine:3.0,1,-0.2,0.05', 128, 3),
    Rast('A 8|9 tall', 'affine:1,3.3,0,0.1', 64, 3),
    Rast('B 16|17 wide', 'affine:7.3,1,0.05,0', 128, 4),
    Rast('B 8|9 tall', 'affine:1,7.1,0,0.02', 32, 1),
    Rast('B 8 tall 64', 'affine:1,7.3,0,0.02', 64, 4),
    Rast('silhouette 32', 'silhouette', 32, 8, B=3),
    Rast('silhouette 64', 'silhouette', 64, 4),
    Rast('silhouette 128', 'silhouette', 128, 3),
    Rast('seam 32', 'seam', 32, 4),
    Rast('seam 64', 'seam', 64, 5),
    Rast('seam 128', 'seam:-0.9,-0.7,-0.5', 128, 8),
    Rast('seam 32 B=3', 'seam', 32, 1, B=3),
    Rast('padding', 'padding', 32, 4),
    Rast('padding 64', 'padding', 64, 3),
    Rast('padding 128', 'padding', 128, 8),
    Rast('u = -1 | +1', 'edges', 64, 4),
    Rast('u = -1 | +1, 7 texels', 'edges', 32, 4, tex_res=7),
    Rast('texel centres', 'centres', 32, 3),
    Rast('texel centres 128', 'centres', 128, 4, tex_res=64),
    Rast('half-texel edges', 'half_texel', 64, 8),
    Rast('|u| = 1e9, inf', 'huge', 32, 4),
    Rast('NaN uv', 'nan', 32, 4),
    # texture resolution
    Rast('tex 1', 'face', 32, 4, tex_res=1),
    Rast('tex 7', 'silhouette', 64, 4, tex_res=7),
    Rast('tex 2 res', 'face', 64, 8, tex_res=128),
    Rast('tex 2 res, seam', 'seam', 32, 4, tex_res=64),
    Rast('tex 300', 'silhouette', 64, 3, tex_res=300),
    Rast('tex 300 at 32', 'face', 32, 5, tex_res=300),
    # channels
    Rast('C = 260', 'silhouette', 32, 260),
    Rast('C = 261', 'face', 32, 261),
    Rast('C = 1028', 'silhouette', 32, 1028),
    Rast('C = 36, seam', 'seam', 64, 36),
    # static crop
    Rast('crop res', 'face', 32, 4, crop=(3, 35, 5, 37), sta_res=40),
    Rast('crop 2 res', 'face', 32, 8, crop=(7, 71, 2, 66), sta_res=80),
    Rast('crop 2 res at 64', 'silhouette', 64, 3, crop=(0, 128, 0, 128), sta_res=128),
    Rast('crop 17', 'face', 32, 4, crop=(4, 21, 9, 26)),
    Rast('crop 45', 'face', 64, 5, crop=(1, 46, 10, 55)),
    Rast('crop 45 at 32', 'silhouette', 32, 4, crop=(2, 47, 0, 45), sta_res=48),
    Rast('crop 1 x 1', 'face', 32, 4, crop=(13, 14, 30, 31)),
    Rast('crop 20 x 33', 'face', 64, 3, crop=(5, 25, 8, 41)),
    Rast('crop 70 x 9', 'face', 32, 4, crop=(10, 80, 3, 12), sta_res=80),
    Rast('crop to the last row and column', 'face', 32, 4, crop=(16, 48, 20, 48), sta_res=48),
    Rast('sta a channel slice', 'silhouette', 32, 8, B=3, sta_extra=3),
    Rast('sta_res 100', 'face', 64, 4, B=3, crop=(30, 62, 68, 100), sta_res=100),
    # alpha
    Rast('alpha 0', 'face', 32, 4, alpha='zero'),
    Rast('alpha 1', 'silhouette', 64, 3, alpha='one'),
    Rast('alpha fractional', 'silhouette', 32, 8, B=3, alpha='frac'),
    Rast('alpha fractional 128', 'seam:-0.9,-0.7,-0.5', 128, 4, alpha='frac'),
)


def rast_wrong_applies(wrong, case):
    """Whether the error `wrong` can show on a case at all."""
    i = rast_inputs(case)
    alpha = i['uv'][..., 2]
    if wrong == 'alpha_after_blend':                  # AA(g a) = AA(g) AA(a) for a constant alpha
        return case.alpha == 'mask' or case.alpha == 'frac'
    if wrong == 'crop_origin':                        # (under alpha 1 the static crop has weight 0)
        return (case.bbox[0] != 0 or case.bbox[2] != 0) and case.alpha != 'one'
    if wrong in ('border', 'wrap'):                   # needs a tap outside the texture, of a pixel that is finite
        return _touches_padding(i['uv'], case.rt)
    if wrong == 'align_corners':                      # (a one-texel texture has no second texel to shift towards)
        return case.rt > 1 and bool((alpha > 0).any())
    return True


def _touches_padding(uv, rt):
    g = uv[..., :2].double()
    p = (g + 1) * (rt / 2) - 0.5
    fin = torch.isfinite(p).all(-1) & (uv[..., 2] > 0)
    return bool((((p < 0) | (p > rt - 1)).any(-1) & fin).any())


# ------------------------------------------------------------------ blend_planes, cond_blend, channels_last tables

# (B, bbox (y0, y1, x0, x1), static planes expanded over the batch)
BLEND_CASES = ((1, BBOX_256, False), (2, (0, 256, 0, 256), True), (1, (0, 64, 0, 64), False), (1, (192, 256, 156, 220), True), (3, (156, 256, 0, 100), True),
               (1, (3, 103, 156, 256), False), (1, (128, 256, 128, 256), False), (1, (70, 134, 5, 69), True))


def blend_inputs(k):
    b, bbox, expanded = BLEND_CASES[k]
    key = ('blend', k)
    if key not in _cache:
        rs = _rs('blend', k)
        _cache[key] = {'stitch': _t(rs.randn(b, 32, KSRC, KSRC)), 'alpha': _t(rs.rand(b, 1, KSRC, KSRC)),
                       'static': _t(rs.randn(1 if expanded else b, 96, KSRC, KSRC))}
    return _cache[key]


def blend_reference(k, dtype=F64, wrong=None):
    b, bbox, expanded = BLEND_CASES[k]
    i = blend_inputs(k)
    return blend_planes(i['stitch'].to(dtype), i['alpha'].to(dtype), i['static'].to(dtype).expand(b, -1, -1, -1), bbox, wrong)


COND_BLEND_SHAPES = ((1, 1, 2, 2), (3, 1, 2, 2), (3, 5, 6, 10), (2, 8, 1, 4), (1, 3, 33, 36))       # (B, C, H, W), H W % 4 == 0
COND_SPLIT_SHAPES = ((1, 8, 2, 2), (3, 16, 8, 12), (2, 8, 5, 7), (1, 24, 1, 1), (3, 8, 33, 36))     # the second form at H W % 4 != 0
CHANNELS_LAST_C, CHANNELS_LAST_HW = (1, 63, 64, 65), ((1, 1), (7, 9), (5, 13), (17, 241))           # H W = 1, 63, 65, 4097


@_cached
def cond_inputs(b, c, h, w, nonfinite=False):
    rs = _rs('cond', b, c, h, w)
    cond, x = _t(rs.randn(b, c + 1, h, w)), _t(rs.randn(b, c, h, w))
    cond[:, -1] = _t(rs.rand(b, h, w))
    if nonfinite:
        flat_c, flat_x = cond.reshape(-1), x.reshape(-1)
        flat_c[0], flat_x[1 % flat_x.numel()], flat_c[2 % flat_c.numel()] = float('inf'), float('-inf'), float('nan')
        cond[-1, -1, -1, -1] = float('nan')
    return cond, x, _t(rs.rand(b, c) + 0.5)
