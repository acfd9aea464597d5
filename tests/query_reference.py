"""float64 restatement of the tri-plane point query (``renderer.sample_from_planes`` + ``OSGDecoder``), written out with explicit
indexing (no ``grid_sample``), and the seeded inputs that tests/test_query_planes_cpu.py and tests/test_query_planes_gpu.py share.

Definition restated (volumetric_rendering/renderer.py and triplane_v20.py:OSGDecoder):

1. optionally negate z, scale the point by ``2 / box_warp``;
2. plane p sees the first two components of ``point @ inv(A_p)`` with the three axis matrices ``A_p`` of ``generate_planes()``; the first
   component runs along the plane's width, the second along its height;
3. bilinear sample, ``align_corners=False`` (texel centre i at ``(2 i + 1) / P - 1``, i.e. ``index = ((g + 1) * P - 1) / 2``), taps
   outside the plane count as 0;
4. mean over the three planes;
5. ``h = softplus(f @ (w0 * lr / sqrt(32)).T + b0 * lr)`` (beta 1, threshold 20), ``o = h @ (w1 * lr / sqrt(64)).T + b1 * lr``;
6. ``sigma = o[0]``, ``rgb = sigmoid(o[1:33]) * 1.002 - 0.001``.
"""
import numpy as np
import torch

F64 = torch.float64

# generate_planes() of the renderer, before the inversion (tests/test_query_planes_cpu.py checks that the two agree)
PLANE_AXES = (((1, 0, 0), (0, 1, 0), (0, 0, 1)),
              ((1, 0, 0), (0, 0, 1), (0, 1, 0)),
              ((0, 0, 1), (1, 0, 0), (0, 1, 0)))

RGB_BAR = 5e-5                  # the project's fp32 bars (tests/test_geometry_gpu.py): rgb, and sigma per unit of max(1, max|sigma|)
SIGMA_BAR = 2e-4


def _taps(g, size):
    """Bilinear taps of normalised coordinates g (float64, any shape) on an axis of ``size`` texels: [(index, weight), (index, weight)]
    with the index clamped into the axis and the weight 0 where the tap lies outside it."""
    pos = ((g + 1.0) * size - 1.0) / 2.0
    lo = torch.floor(pos)
    frac = pos - lo
    out = []
    for tap, w in ((lo, 1.0 - frac), (lo + 1.0, frac)):
        inside = (tap >= 0) & (tap <= size - 1)
        out.append((tap.clamp(0, size - 1).long(), torch.where(inside, w, torch.zeros_like(w))))
    return out


def plane_features_fp64(planes, points, box_warp, flip_z=False):
    """Steps 1-4: planes [B,3,C,H,W], points [B,M,3] -> the averaged features [B,M,C] in float64."""
    planes, pts = planes.detach().cpu().to(F64), points.detach().cpu().to(F64).clone()
    b, n_planes, c, h, w = planes.shape
    assert n_planes == 3 and pts.shape[0] == b and pts.shape[2] == 3
    if flip_z:
        pts[..., 2] = -pts[..., 2]
    pts = pts * (2.0 / float(box_warp))
    inv = torch.linalg.inv(torch.tensor(PLANE_AXES, dtype=F64))
    batch = torch.arange(b)[:, None]
    feats = torch.zeros(b, pts.shape[1], c, dtype=F64)
    for p in range(3):
        proj = pts @ inv[p]                                          # [B,M,3]; the plane sees components 0 (width) and 1 (height)
        plane = planes[:, p].permute(0, 2, 3, 1)                      # [B,H,W,C]
        for iy, wy in _taps(proj[..., 1], h):
            for ix, wx in _taps(proj[..., 0], w):
                feats += plane[batch, iy, ix] * (wy * wx)[..., None]
    return feats / 3.0


def decoder_fp64(feats, w0, b0, w1, b1, lr_multiplier=1.0):
    """Steps 5-6 on features [..., 32]: {'pre' [..., 64] hidden pre-activations, 'hidden' [..., 64], 'out' [..., 33] layer-2 outputs
    (row 0 = sigma, rows 1..32 = rgb logits), 'sigma' [..., 1], 'rgb' [..., 32]}, all float64."""
    w0, b0, w1, b1 = (t.detach().cpu().to(F64) for t in (w0, b0, w1, b1))
    lr = float(lr_multiplier)
    pre = feats.to(F64) @ (w0 * (lr / np.sqrt(32.0))).T + b0 * lr
    hidden = torch.where(pre > 20.0, pre, torch.log1p(torch.exp(pre.clamp(max=20.0))))
    out = hidden @ (w1 * (lr / np.sqrt(64.0))).T + b1 * lr
    rgb = 1.0 / (1.0 + torch.exp(-out[..., 1:])) * 1.002 - 0.001
    return {'pre': pre, 'hidden': hidden, 'out': out, 'sigma': out[..., 0:1], 'rgb': rgb}


def query_parts_fp64(planes, w0, b0, w1, b1, points, box_warp, lr_multiplier=1.0, flip_z=False):
    """``decoder_fp64`` of ``plane_features_fp64``, with the features under 'feats'."""
    feats = plane_features_fp64(planes, points, box_warp, flip_z)
    return dict(decoder_fp64(feats, w0, b0, w1, b1, lr_multiplier), feats=feats)


def query_fp64(planes, w0, b0, w1, b1, points, box_warp, lr_multiplier=1.0, flip_z=False):
    """(sigma [B,M,1], rgb [B,M,32]) in float64: planes [B,3,32,H,W], points [B,M,3] in world coordinates."""
    q = query_parts_fp64(planes, w0, b0, w1, b1, points, box_warp, lr_multiplier, flip_z)
    return q['sigma'], q['rgb']


def propagated_magnitude(planes, w0, b0, w1, b1, points, box_warp, lr_multiplier=1.0, flip_z=False):
    """For reporting only: the sums of absolute terms of both layers, ``(|f| . |W0 g0| + |b0 lr| [B,M,64], |h| . |W1 g1| + |b1 lr|
    [B,M,33])``.  A float32 dot product carries a rounding error of a few eps32 times these."""
    q = query_parts_fp64(planes, w0, b0, w1, b1, points, box_warp, lr_multiplier, flip_z)
    w0, b0, w1, b1 = (t.detach().cpu().to(F64).abs() for t in (w0, b0, w1, b1))
    lr = abs(float(lr_multiplier))
    return (q['feats'].abs() @ (w0 * (lr / np.sqrt(32.0))).T + b0 * lr, q['hidden'].abs() @ (w1 * (lr / np.sqrt(64.0))).T + b1 * lr)


def bars(sigma_ref):
    """The caps on any measured tolerance: (sigma, rgb)."""
    return SIGMA_BAR * max(1.0, float(sigma_ref.abs().max())) if sigma_ref.numel() else SIGMA_BAR, RGB_BAR


# ------------------------------------------------------------------ seeded inputs

PLANE_H, PLANE_W = 24, 40
HOT_CASES = ((1.0, 18.0), (0.5, 72.0))    # (lr_multiplier, factor on w0): hidden pre-activations beyond +-25, colour logits beyond +-20
SQUARE_CASES = ((8, 1.0), (256, 0.25))    # (plane size, amplitude): the float32 rounding of the texel position grows with the size


def quantise_colors(rgb):
    """``geometry.vertex_colors`` on float64 colours [V,32]: uint8 [V,3]."""
    return (rgb[:, :3].clamp(0, 1) * 255).round().to(torch.uint8)


def make_planes(seed, batch, h=PLANE_H, w=PLANE_W, amplitude=1.0):
    """Random planes [batch,3,32,h,w] with another scale and offset on every plane of every batch element, so that a plane, axis or H/W
    mix-up is an O(1) error.  Element b depends on (seed, b) alone: a larger batch extends a smaller one."""
    out = torch.empty(batch, 3, 32, h, w)
    for b in range(batch):
        rs = np.random.RandomState(seed + 1000 * b)
        v = rs.randn(3, 32, h, w)
        scale = amplitude * np.array([0.6, 1.0, 1.4])[rs.permutation(3)]
        offset = amplitude * np.array([-0.5, 0.2, 0.7])[rs.permutation(3)]
        out[b] = torch.from_numpy(v * scale[:, None, None, None] + offset[:, None, None, None]).float()
    return out


def make_decoder_weights(seed, w0_factor=1.0):
    """(w0 [64,32], b0 [64], w1 [33,64], b1 [33]) float32: randn weights (the FullyConnectedLayer initialisation), small biases."""
    rs = np.random.RandomState(seed)
    w0, b0 = rs.randn(64, 32) * w0_factor, rs.randn(64) * 0.1
    w1, b1 = rs.randn(33, 64), rs.randn(33) * 0.1
    return tuple(torch.from_numpy(a).float() for a in (w0, b0, w1, b1))


def make_decoder(weights, lr_multiplier=1.0):
    """The project's OSGDecoder module holding ``weights``."""
    from invertavatar_amd.training_avatar_texture.triplane_v20 import OSGDecoder
    dec = OSGDecoder(32, {'decoder_lr_mul': lr_multiplier, 'decoder_output_dim': 32}).eval().requires_grad_(False)
    dec.load_state_dict(dict(zip(('net.0.weight', 'net.0.bias', 'net.2.weight', 'net.2.bias'), weights)))
    return dec


def edge_points(seed, batch, m, box_warp, h=PLANE_H, w=PLANE_W):
    """World points [batch,m,3] float32.  Every coordinate of every point is drawn on its own from one of four populations, in
    normalised plane coordinates g (texel index ``(g + 1) P / 2 - 1/2`` with P = h or w at random, since every world axis meets both):
      interior (40 %)            |g| < 0.95;
      border, inside (25 %)      the last half texel before a border, where one tap is outside;
      border, outside (25 %)     up to one texel beyond a border: the first half still has one tap inside, the second has none;
      far (10 %)                 +-10 box_warp in world units.
    A few coordinates are then put exactly on a border (g = +-1) and on the centre of the first or last texel."""
    rs = np.random.RandomState(seed)
    shape = (batch, m, 3)
    size = np.where(rs.rand(*shape) < 0.5, float(h), float(w))
    side = np.where(rs.rand(*shape) < 0.5, -1.0, 1.0)
    u = rs.rand(*shape)
    pop = rs.choice(4, size=shape, p=[0.4, 0.25, 0.25, 0.1])
    g = np.select([pop == 0, pop == 1, pop == 2], [side * 0.95 * u, side * (1.0 - u / size), side * (1.0 + 2.0 * u / size)], side * 20.0)
    exact = rs.rand(*shape)
    g = np.where(exact < 0.02, side, np.where(exact < 0.04, side * (1.0 - 1.0 / size), g))
    return torch.from_numpy(g * (box_warp / 2.0)).float()


def outside_points(box_warp, h=PLANE_H, w=PLANE_W):
    """Points [1,8,3] that no tap of any plane reaches: every plane has a coordinate more than one texel beyond a border."""
    far = 1.0 + 2.5 / min(h, w)
    g = [(far, far, far), (-far, -far, -far), (far, -2.0, 3.0), (0.1, far, -far), (-far, 0.2, 0.3), (5.0, 5.0, 5.0), (-20.0, 20.0, 20.0),
         (far, 0.0, far)]
    return (torch.tensor(g, dtype=torch.float64) * (box_warp / 2.0)).float()[None]
