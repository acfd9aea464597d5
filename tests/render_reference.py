"""float64 restatement of the ray pipeline (``ImportanceRenderer_bsMotion.forward`` / ``ImportanceRenderer.forward``: decode the coarse
samples, march, decode the importance samples, merge, march), built on the float64 point query of tests/query_reference.py, and the
seeded scenes that tests/test_render_reference_cpu.py and tests/test_renderer_edges_gpu.py share.

What is NOT restated: the coarse depths (``oracle.renderer.coarse_depths``: an fp32 bit rule by definition) and the importance
resampling.  ``render_fp64`` takes ``z_fine`` as an argument, so the reference never decides a ``searchsorted`` bin itself and a
one-bin flip cannot register as an O(1) "error"; the resampling has its own bit-level reference, ``oracle.renderer.sample_importance``.

Error budget of a device decoder that forms its products from fp16 hi / lo pairs (three products, lo x lo dropped, the split rounded
towards zero): at most 2^-22 of the product each, doubled: ``EPS_PAIR = 2^-20`` times the sum of absolute terms of a layer.
``propagated`` carries that through the pipeline with these first-order bounds (L = longest ray, the intervals of a ray add up to it):

  sigma        P_s  = sum|terms of the density row| + sum_k |W1 g1|[0,k] * sum|terms of hidden unit k|    (softplus has slope <= 1)
  colour       P_c  = 0.2505 * (the same for the worst colour row)                                        (1.002 * sigmoid' <= 0.2505)
  w_i, wsum    L * P_s      (d w_i / d d_i <= delta_i, d w_i / d d_j = -w_i delta_j for j < i, d = softplus(mean sigma - 1): slope <= 1)
  rgb          2 * (1.001 * 2 L P_s + P_c)         (rgb = 2 sum w_i c_i - 1, sum_i |dw_i| <= 2 L P_s, |c| <= 1.001, sum w_i <= 1)
  depth        4 L P_s * z_max / min wsum          (depth = sum w z / sum w; rays without weight are clamped, not divided)
"""
import numpy as np
import torch

from oracle import renderer as OR
from invertavatar_amd import synthetic
import query_reference as QR

F64 = torch.float64
N = 48
EPS_PAIR = 2.0 ** -20
FEATURE_CLAMP = 65000.0 / 256.0     # where ia_render_rays saturates a mean plane feature
BARS = {'sigma': 5e-5, 'w_coarse': 2e-5, 'rgb': 1e-4, 'depth': 1e-4, 'wsum': 1e-4}      # tests/test_renderer_gpu.py (sigma per max(1, max|sigma|))

coarse_depths = OR.coarse_depths


def march_fp64(colors, sigmas, depths, white_back=False, per_frame=False):
    """MipRayMarcher2 (ray_marcher.py:25-57) in float64: colors [B,R,S,C], sigmas and depths [B,R,S,1] ->
    (rgb [B,R,C], depth [B,R,1], wsum [B,R,1], weights [B,R,S-1,1]).  The depth is clamped to [min, max] of ``depths``: of the whole
    call, or of each batch element with ``per_frame``."""
    colors, sigmas, depths = colors.to(F64), sigmas.to(F64), depths.to(F64)
    deltas = depths[:, :, 1:] - depths[:, :, :-1]
    c_mid = (colors[:, :, :-1] + colors[:, :, 1:]) / 2
    d_mid = (sigmas[:, :, :-1] + sigmas[:, :, 1:]) / 2 - 1
    z_mid = (depths[:, :, :-1] + depths[:, :, 1:]) / 2
    d_mid = torch.where(d_mid > 20.0, d_mid, torch.log1p(torch.exp(d_mid.clamp(max=20.0))))
    alpha = 1 - torch.exp(-d_mid * deltas)
    shifted = torch.cat([torch.ones_like(alpha[:, :, :1]), 1 - alpha + 1e-10], 2)
    weights = alpha * torch.cumprod(shifted, 2)[:, :, :-1]
    wsum = weights.sum(2)
    rgb = (weights * c_mid).sum(2)
    depth = (weights * z_mid).sum(2) / wsum
    depth = torch.where(torch.isnan(depth), torch.full_like(depth, float('inf')), depth)
    flat = depths.reshape(depths.shape[0], -1)
    lo, hi = (flat.min(1).values, flat.max(1).values) if per_frame else (flat.min().expand(flat.shape[0]), flat.max().expand(flat.shape[0]))
    depth = torch.minimum(torch.maximum(depth, lo[:, None, None]), hi[:, None, None])
    if white_back:
        rgb = rgb + 1 - wsum
    return rgb * 2 - 1, depth, wsum, weights


def decode_fp64(planes, weights, lr, ro, rd, z, box_warp=1.0, flip_z=False, feature_clamp=None):
    """The point query at ``ro + z * rd``: z [B,R,S,1] -> ``QR.decoder_fp64``'s dict reshaped to [B,R,S,.], with 'feats' (after the
    optional saturation of the mean features at +-feature_clamp), 'feats_raw' (before it) and 'points' [B,R*S,3]."""
    b, r, s, _ = z.shape
    pts = (ro.to(F64)[:, :, None] + z.to(F64) * rd.to(F64)[:, :, None]).reshape(b, r * s, 3)
    raw = feats = QR.plane_features_fp64(planes, pts, box_warp, flip_z)
    if feature_clamp is not None:
        feats = feats.clamp(-feature_clamp, feature_clamp)
    out = dict(QR.decoder_fp64(feats, *weights, lr), feats=feats, feats_raw=raw)
    out = {k: v.reshape(b, r, s, -1) for k, v in out.items()}
    out['points'] = pts
    return out


def render_fp64(planes, weights, lr, ro, rd, z_coarse, z_fine, box_warp=1.0, white_back=False, flip_z=False, per_frame=False,
                feature_clamp=None):
    """All 96 depths decoded in float64, sorted stably with the coarse samples first, marched.  Returns a dict: 'rgb' [B,R,32], 'depth',
    'wsum' [B,R,1], 'den_coarse' [B,R,48,1], 'w_coarse' [B,R,47,1], 'order' [B,R,96,1], and the decoder's parts of all samples under
    'parts' (coarse first)."""
    z_all = torch.cat([z_coarse, z_fine], 2).to(F64)
    parts = decode_fp64(planes, weights, lr, ro, rd, z_all, box_warp, flip_z, feature_clamp)
    n_c = z_coarse.shape[2]
    _, _, _, w_c = march_fp64(parts['rgb'][:, :, :n_c], parts['sigma'][:, :, :n_c], z_all[:, :, :n_c], white_back, per_frame)
    order = torch.sort(z_all, dim=2, stable=True).indices
    rgb, depth, wsum, _ = march_fp64(torch.gather(parts['rgb'], 2, order.expand(-1, -1, -1, 32)), torch.gather(parts['sigma'], 2, order),
                                     torch.gather(z_all, 2, order), white_back, per_frame)
    return dict(rgb=rgb, depth=depth, wsum=wsum, den_coarse=parts['sigma'][:, :, :n_c], w_coarse=w_c, order=order, parts=parts)


def propagated(parts, weights, lr, z_all, wsum):
    """The propagated magnitudes of the module docstring, from the float64 parts of all samples: {'sigma', 'w_coarse', 'wsum', 'rgb',
    'depth'}; multiply by EPS_PAIR."""
    w0, b0, w1, b1 = (t.detach().cpu().to(F64).abs() for t in weights)
    lr = abs(float(lr))
    g0, g1 = w0 * (lr / np.sqrt(32.0)), w1 * (lr / np.sqrt(64.0))
    mag1 = parts['feats'].abs() @ g0.T + b0 * lr
    mag2 = parts['hidden'].abs() @ g1.T + b1 * lr + mag1 @ g1.T
    p_s, p_c = float(mag2[..., 0].max()), 0.2505 * float(mag2[..., 1:].max())
    z = z_all.to(F64)
    length = float((z.amax(2) - z.amin(2)).max())
    hit = wsum[wsum > 0]
    depth = 4 * length * p_s * float(z.max()) / float(hit.min()) if hit.numel() else 0.0
    return dict(sigma=p_s, w_coarse=length * p_s, wsum=length * p_s, rgb=2 * (1.001 * 2 * length * p_s + p_c), depth=depth)


# ------------------------------------------------------------------ seeded inputs

def make_rays(frames, nrr):
    """(rays_o, rays_d) [B, nrr^2, 3] of ``synthetic.camera_labels(frames)``."""
    cams = synthetic.camera_labels(frames)
    return OR.ray_sampler_zxc(cams[:, :16].view(-1, 4, 4), cams[:, 16:25].view(-1, 3, 3), nrr)


def tile_rays(ro, rd, r):
    """The first ``r`` of each frame's rays repeated cyclically: any ray count from an nrr^2 set, each copy nudged in direction so that
    no two rays are the same."""
    n = ro.shape[1]
    idx = torch.arange(r) % n
    turn = (torch.arange(r) // n).float()[None, :, None] * torch.tensor([0.003, -0.002, 0.0])
    rd2 = torch.nn.functional.normalize(rd[:, idx] + turn, dim=-1)
    return ro[:, idx].contiguous(), rd2.contiguous()


def scaled_weight_max(w, lr, fan_in, base2=False):
    """max |w * lr / sqrt(fan_in)| (x log2 e with ``base2``): the weight as ia_render_rays stages it."""
    return float(w.to(F64).abs().max()) * abs(float(lr)) / np.sqrt(float(fan_in)) * (np.log2(np.e) if base2 else 1.0)


class Scene:
    """One render call's inputs on the host, its fp32 oracle run (cached) and its float64 references.

    ``box``: None for ``ia_render_rays`` (one ``dist`` for the call, or one per frame with ``per_frame``), or
    dict(u=[B*R,48] SORTED draws, flip_z=bool) for ``ia_ray_limits_box(repair_misses=True)`` + ``ia_render_rays_box``."""

    def __init__(self, planes, weights, ro, rd, jitter, lr=1.0, box_warp=1.0, white_back=False, per_frame=False, box=None,
                 feature_clamp=None):
        self.planes, self.weights, self.ro, self.rd, self.jitter, self.lr = planes, tuple(weights), ro, rd, jitter, float(lr)
        self.box_warp, self.white_back, self.per_frame, self.box, self.feature_clamp = float(box_warp), white_back, per_frame, box, feature_clamp
        self.flip_z = bool(box and box['flip_z'])
        self._oracle = self._ref = self._tol = None

    @property
    def dec(self):
        return dict(zip(('net.0.weight', 'net.0.bias', 'net.2.weight', 'net.2.bias'), self.weights), lr_mul=self.lr)

    def frame(self, k):
        box = None if self.box is None else dict(self.box, u=self.box['u'].reshape(self.ro.shape[0], -1, N)[k].contiguous())
        return Scene(self.planes[k:k + 1], self.weights, self.ro[k:k + 1], self.rd[k:k + 1], self.jitter[k:k + 1], self.lr, self.box_warp,
                     self.white_back, False, box, self.feature_clamp)

    def dists(self):
        d = torch.norm(self.ro, dim=-1)
        return d.mean(dim=1) if self.per_frame else d.mean().reshape(1)

    def z_coarse(self):
        if self.box is not None:
            return OR.coarse_depths_eg3d(self.ro, self.rd, 'auto', 'auto', N, self.jitter, self.box_warp)
        if self.per_frame:
            return torch.cat([OR.coarse_depths(self.ro[k:k + 1], N, self.jitter[k:k + 1])[0] for k in range(self.ro.shape[0])], 0)
        return OR.coarse_depths(self.ro, N, self.jitter)[0]

    def oracle(self):
        """The CPU fp32 oracle on these inputs: dict(rgb, depth, wsum, den_coarse [B,R,48,1], w_coarse [B,R,47,1], z_coarse, z_fine)."""
        if self._oracle is None:
            if self.box is not None:
                rgb, depth, wsum, aux = OR.render_eg3d(self.planes, self.dec, self.ro, self.rd, self.jitter, self.box['u'], flip_z=self.flip_z,
                                                       box_warp=self.box_warp, return_aux=True)
                z_c = aux['z_coarse']
                aux['z_fine'] = OR.sample_importance(z_c, aux['w_coarse'], N, u=self.box['u'])[0]
                xyz = (self.ro.unsqueeze(-2) + z_c * self.rd.unsqueeze(-2)).reshape(z_c.shape[0], -1, 3) * torch.tensor([1.0, 1.0, -1.0 if self.flip_z else 1.0])
                aux['den_coarse'] = OR.osg_decoder(self.dec, OR.sample_from_planes(self.planes, xyz, self.box_warp))[1].reshape(z_c.shape)
                runs = [(rgb, depth, wsum, aux)]
            elif self.per_frame:
                runs = [OR.render(self.planes[k:k + 1], self.dec, self.ro[k:k + 1], self.rd[k:k + 1], self.jitter[k:k + 1], box_warp=self.box_warp,
                                  white_back=self.white_back, return_aux=True) for k in range(self.ro.shape[0])]
            else:
                runs = [OR.render(self.planes, self.dec, self.ro, self.rd, self.jitter, box_warp=self.box_warp, white_back=self.white_back,
                                  return_aux=True)]
            cat = lambda pick: torch.cat([pick(run) for run in runs], 0)
            self._oracle = dict(rgb=cat(lambda t: t[0]), depth=cat(lambda t: t[1]), wsum=cat(lambda t: t[2]),
                                **{k: cat(lambda t: t[3][k]) for k in ('den_coarse', 'w_coarse', 'z_coarse', 'z_fine')})
        return self._oracle

    def reference(self):
        """``fp64`` fed the oracle's own depths (cached)."""
        if self._ref is None:
            o = self.oracle()
            self._ref = self.fp64(o['z_fine'], o['z_coarse'])
        return self._ref

    def fp64(self, z_fine, z_coarse=None):
        return render_fp64(self.planes, self.weights, self.lr, self.ro, self.rd, self.z_coarse() if z_coarse is None else z_coarse, z_fine,
                           self.box_warp, self.white_back, self.flip_z, self.per_frame, self.feature_clamp)

    def sample_importance(self, w_coarse):
        """``oracle.renderer.sample_importance`` of this scene's coarse depths and the GIVEN fp32 coarse weights [B,R,47(,1)]:
        (z_fine [B,R,48,1], inds [B*R,48])."""
        z_c = self.z_coarse()
        b, r = z_c.shape[:2]
        z_f, ibuf = OR.sample_importance(z_c, w_coarse.reshape(b, r, N - 1, 1).float(), N, u=None if self.box is None else self.box['u'])
        return z_f, ibuf['inds']

    def tolerances(self):
        """Per quantity ``min(bar, 4 * max|CPU fp32 oracle - fp64| + EPS_PAIR * propagated magnitude)`` with the reference fed the oracle's
        own z_fine: {name: (tol, CPU deviation, bar)}.  Raises if the oracle itself is outside a bar on these inputs."""
        if self._tol is not None:
            return self._tol
        o, ref = self.oracle(), self.reference()
        mags = propagated(ref['parts'], self.weights, self.lr, torch.cat([o['z_coarse'], o['z_fine']], 2), ref['wsum'])
        out = {}
        for name, got, want in (('sigma', o['den_coarse'], ref['den_coarse']), ('w_coarse', o['w_coarse'], ref['w_coarse']),
                                ('rgb', o['rgb'], ref['rgb']), ('depth', o['depth'], ref['depth']), ('wsum', o['wsum'], ref['wsum'])):
            bar = BARS[name] * (max(1.0, float(ref['den_coarse'].abs().max())) if name == 'sigma' else 1.0)
            dev = float((got.to(F64) - want).abs().max())
            assert dev <= bar, f'the inputs must keep the CPU oracle inside the bar: {name} {dev:.2e} > {bar:.2e}'
            out[name] = (min(bar, 4.0 * dev + EPS_PAIR * mags[name]), dev, bar)
        self._tol = out
        return out


def scene(seed, frames, nrr=8, size=(16, 16), amplitude=1.0, rays=None, **kw):
    """Seeded ordinary scene: ``QR.make_planes`` / ``QR.make_decoder_weights``, the frames' camera rays (``rays``: that many per frame by
    ``tile_rays``), ``synthetic.jitter``."""
    ro, rd = make_rays(frames, nrr)
    if rays is not None:
        ro, rd = tile_rays(ro, rd, rays)
    planes = QR.make_planes(seed, len(frames), size[0], size[1], amplitude)
    return Scene(planes, QR.make_decoder_weights(seed + 1), ro, rd, synthetic.jitter(frames, ro.shape[1]), **kw)


def measures(sc):
    """float64 quantities of a scene over all 96 samples (the oracle's own z_fine): dict(feat = max |mean feature| before any saturation, pre = max hidden
    pre-activation, abs_pre = max |.|, sigma_max, logit_max = max |colour logit|, padded = share of samples with at least one zero-padded
    tap, on_border = number of plane coordinates exactly on g = +-1)."""
    ref = sc.reference()
    p = ref['parts']
    g = p['points'] * (2.0 / sc.box_warp)
    h, w = sc.planes.shape[-2:]
    padded = torch.zeros(g.shape[:2], dtype=torch.bool)
    for c0, c1 in ((0, 1), (0, 2), (2, 0)):          # (width, height) coordinate of planes 0, 1, 2
        for c, size in ((c0, w), (c1, h)):
            pos = ((g[..., c] + 1.0) * size - 1.0) / 2.0
            padded |= (torch.floor(pos) < 0) | (torch.floor(pos) + 1 > size - 1)
    return dict(feat=float(p['feats_raw'].abs().max()), pre=float(p['pre'].max()), abs_pre=float(p['pre'].abs().max()),
                sigma_max=float(p['sigma'].max()), sigma_min=float(p['sigma'].min()), logit_max=float(p['out'][..., 1:].abs().max()),
                padded=float(padded.double().mean()), on_border=int((g.abs() == 1.0).sum()), ref=ref)


def reach(build, key, target, rel=1e-3, max_iter=16):
    """``build(s) -> Scene`` scales some input by s; fixed-point iteration on s until ``measures(scene)[key]`` is within ``rel`` of
    ``target`` (the quantity moves with s directly and, slightly, through the importance samples).  Returns (scene, measures)."""
    s = 1.0
    for _ in range(max_iter):
        sc = build(s)
        m = measures(sc)
        if abs(m[key] / target - 1.0) <= rel:
            return sc, m
        s *= target / m[key]
    raise AssertionError(f'{key} did not reach {target}: {m[key]}')


FRAMES = [7, 8]
SIZES = ((16, 16), (24, 40))
DOMAIN_CASES = ('ordinary', 'feature_edge', 'hidden_edge', 'w0_edge_lr1', 'w0_edge_lr0.5', 'w1_edge_lr1', 'w1_edge_lr0.5', 'tiny', 'saturated',
                'leaving')
_cases = {}


def _with(sc, planes=None, weights=None, **kw):
    args = dict(lr=sc.lr, box_warp=sc.box_warp, white_back=sc.white_back, per_frame=sc.per_frame, box=sc.box, feature_clamp=sc.feature_clamp)
    args.update(kw)
    return Scene(sc.planes if planes is None else planes, sc.weights if weights is None else weights, sc.ro, sc.rd, sc.jitter, **args)


def border_rays(sc, box_warp, count=6):
    """Replaces the first ``count`` rays of every frame by rays parallel to the z axis whose x (even rays) or y (odd rays) is exactly
    +-box_warp / 2: that plane coordinate is g = +-1 at every sample (box_warp a power of two: the scaling is exact)."""
    ro, rd = sc.ro.clone(), sc.rd.clone()
    dist = float(torch.norm(ro, dim=-1).mean())
    for k in range(count):
        side = box_warp / 2 * (1 if k % 4 < 2 else -1)
        other = 0.05 * (k - count / 2) * box_warp
        ro[:, k] = torch.tensor([side, other, -dist] if k % 2 == 0 else [other, side, -dist])
        rd[:, k] = torch.tensor([0.0, 0.0, 1.0])
    return Scene(sc.planes, sc.weights, ro, rd, sc.jitter, sc.lr, box_warp, sc.white_back, sc.per_frame, sc.box, sc.feature_clamp)


def domain_case(name, size):
    """(scene, measures) of a domain case of tests/test_renderer_edges_gpu.py on a plane of ``size``; B = 2, 64 rays per frame.  Cached:
    the scene's oracle run and tolerances are computed once per session."""
    key = (name, tuple(size))
    if key in _cases:
        return _cases[key]
    base = scene(40 + size[1], FRAMES, 8, size)
    w0, b0, w1, b1 = base.weights
    if name == 'ordinary':
        out = base, measures(base)
    elif name in ('feature_edge', 'feature_over'):
        # planes x s, w0 / s: the pre-activations (and with them the importance samples) stay, the features reach the target
        k = min(1.0, 19.0 / measures(base)['abs_pre'])
        target = 240.0 if name == 'feature_edge' else 255.9
        out = reach(lambda s: _with(base, planes=(base.planes.to(F64) * s).float(), weights=((w0.to(F64) * (k / s)).float(), b0 * k, w1, b1),
                                    feature_clamp=None if name == 'feature_edge' else FEATURE_CLAMP), 'feat', target, rel=2e-4)
    elif name in ('hidden_edge', 'hidden_over'):
        # planes x 100 (features of about 230: inside their range), the rest of the way through w0 (staged weights of about 1)
        hot = (base.planes.to(F64) * 100.0).float()
        out = reach(lambda s: _with(base, planes=hot, weights=((w0.to(F64) * s).float(), b0, w1, b1)), 'pre', 170.0 if name == 'hidden_edge' else 400.0)
    elif name.startswith('w0_edge'):
        lr = float(name.split('lr')[1])
        s = 15.5 / scaled_weight_max(w0, lr, 32, base2=True)
        out = _with(base, planes=(base.planes.to(F64) / (s * lr)).float(), weights=((w0.to(F64) * s).float(), b0 / lr, w1 / lr, b1 / lr), lr=lr)
        out = out, measures(out)
    elif name.startswith('w1_edge'):
        # colour rows x s; the hidden units shrink by about as much (bias - ln s - 2), so that the colour logits stay off saturation
        lr = float(name.split('lr')[1])
        s = 15.5 / scaled_weight_max(w1[1:], lr, 64)
        w1s = torch.cat([w1[:1] / lr, (w1[1:].to(F64) * s).float()], 0)
        out = _with(base, weights=(w0 / lr, (b0 - np.log(s * lr) - 2.0) / lr, w1s, b1 / lr), lr=lr)
        out = out, measures(out)
    elif name == 'tiny':
        out = _with(base, planes=base.planes * 1e-4, weights=(w0, torch.zeros_like(b0), w1, torch.zeros_like(b1)))
        out = out, measures(out)
    elif name == 'saturated':
        # a density so high that exp(-density * delta) is 0 in fp32 (argument beyond -104) on the SHORTEST coarse interval of the scene
        # (the jitter makes some intervals a hundredth of the mean): alpha = 1 everywhere, the first interval takes all the weight and
        # interval k is left with the 1e-10 floor of the transmittance to the power k
        z = base.z_coarse()
        shortest = float((z[:, :, 1:] - z[:, :, :-1]).min())
        b1s = b1.clone()
        b1s[0] = float(np.ceil(120.0 / shortest / 1e4) * 1e4)
        out = _with(base, weights=(w0, b0, w1 * 0.25, b1s))
        out = out, measures(out)
    elif name == 'leaving':
        out = border_rays(base, 0.5)
        out = out, measures(out)
    else:
        raise KeyError(name)
    _cases[key] = out
    return out


def check_targets(name, sc, m):
    """Asserts that a domain case is what its name says (``m = measures(sc)``)."""
    w0, _, w1, _ = sc.weights
    near = lambda got, want, rel=1e-3: abs(got / want - 1.0) <= rel
    # every case stays inside the other two ranges of the fp16 pair decoder
    assert scaled_weight_max(w0, sc.lr, 32, base2=True) <= 15.5 * (1 + 1e-6) and scaled_weight_max(w1[1:], sc.lr, 64) <= 15.5 * (1 + 1e-6)
    assert m['feat'] < FEATURE_CLAMP or name == 'feature_over'
    assert m['pre'] / np.log(2.0) < 255 or name == 'hidden_over'
    if name == 'ordinary':
        assert m['feat'] < 10 and m['abs_pre'] < 20
    elif name == 'feature_edge':
        assert near(m['feat'], 240.0) and m['feat'] < FEATURE_CLAMP and m['abs_pre'] <= 20
    elif name == 'feature_over':
        assert FEATURE_CLAMP < m['feat'] <= 256.0 and near(m['feat'], 255.9, 3e-4) and m['abs_pre'] <= 20
    elif name == 'hidden_edge':
        assert near(m['pre'], 170.0) and m['pre'] / np.log(2.0) < 255 and max(m['sigma_max'], -m['sigma_min']) > 20 and m['logit_max'] > 20
    elif name == 'hidden_over':
        assert near(m['pre'], 400.0)
    elif name.startswith('w0_edge'):
        assert near(scaled_weight_max(w0, sc.lr, 32, base2=True), 15.5, 1e-6) and m['abs_pre'] < 20
    elif name.startswith('w1_edge'):
        assert near(scaled_weight_max(w1[1:], sc.lr, 64), 15.5, 1e-6) and m['logit_max'] < 10
    elif name == 'tiny':
        assert m['feat'] < 3e-4 and float(sc.weights[1].abs().max()) == 0 and float(sc.weights[3].abs().max()) == 0
    elif name == 'saturated':
        z, w = sc.z_coarse().to(F64), m['ref']['w_coarse']
        d_mid = (m['ref']['den_coarse'][:, :, 1:] + m['ref']['den_coarse'][:, :, :-1]) / 2 - 1
        arg = -(d_mid * (z[:, :, 1:] - z[:, :, :-1])).float()
        assert float(arg.max()) < -104 and float(torch.exp(arg).max()) == 0                    # fp32 exp: alpha == 1 in every interval
        assert float((w[:, :, 0] - 1).abs().max()) < 1e-12
        for k in (1, 2, 3):                                                                    # the floor, to the power k
            assert float((w[:, :, k] / 1e-10 ** k - 1).abs().max()) < 1e-9
        assert float(w[:, :, -1].max()) < 1e-300 and float((m['ref']['wsum'] - 1).abs().max()) < 1e-9
    elif name == 'leaving':
        assert m['padded'] >= 0.3 and m['on_border'] >= 48
    else:
        raise KeyError(name)
