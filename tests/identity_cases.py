"""Inputs shared by the identity-similarity tests and tests/golden/make_identity_golden.py: seeded, smooth frames in [-1, 1] (a coarse
random field, bicubically enlarged, through tanh), as three pairs -- identical, near (the frame plus a tenth of another field) and
far (an unrelated field) -- and the synthetic network they are scored with."""
import torch
import torch.nn.functional as F

SEED = 31            # of the frames
MODEL_SEED = 2       # of IDScore.synthetic
PAIRS = ('identical', 'near', 'far')
EPS32 = 2.0 ** -23


def field(seed, n, h, w, cells=12):
    g = torch.Generator().manual_seed(seed)
    coarse = torch.randn(n, 3, cells, cells, generator=g, dtype=torch.float64)
    return F.interpolate(coarse, size=(h, w), mode='bicubic', align_corners=False)


def frames(seed=SEED, h=256, w=256):
    """(x, y): float32 [3,3,h,w] each; pair 0 identical, pair 1 near, pair 2 far."""
    a, b = field(seed, 3, h, w), field(seed + 1, 3, h, w)
    x = torch.tanh(a)
    y = torch.stack([x[0], torch.tanh(a[1] + 0.1 * b[1]), torch.tanh(b[2])])
    return x.float().contiguous(), y.float().contiguous()


def to_uint8(x):
    """float [N,3,H,W] in [-1, 1] -> uint8 [N,H,W,3]."""
    return ((x.permute(0, 2, 3, 1).double() + 1.0) * 127.5).round().clamp(0, 255).to(torch.uint8).contiguous()


def check(name, got, ref64, ref32, multiple=4):
    """The project's bound: |got - float64| <= multiple * e32 + eps32 * scale, e32 the float32 statement's own distance from float64."""
    e32 = (ref32.double() - ref64).abs().max().item()
    err = (got.double().cpu() - ref64).abs().max().item()
    scale = ref64.abs().max().item()
    bound = multiple * e32 + EPS32 * scale
    print(f'{name}: err {err:.3e}  e32 {e32:.3e}  err/e32 {err / max(e32, 1e-300):.2f}  scale {scale:.3e}  bound {bound:.3e}')
    assert err <= bound, f'{name}: {err:.3e} > {bound:.3e}'
    return err, e32
