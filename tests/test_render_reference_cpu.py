"""The float64 restatement of the ray pipeline (tests/render_reference.py) against the project's fp32 oracle renderer and the
reference's recorded fixture, hand cases of the marcher, and the seeded edge scenes that tests/test_renderer_edges_gpu.py holds the
kernels to: every scene reaches the quantity it is named after, and keeps the CPU oracle inside the project's bars."""
import numpy as np
import pytest
import torch

from oracle import renderer as OR
from invertavatar_amd import synthetic
from conftest import rnd, max_abs
import render_reference as RR

F64 = torch.float64


def _compare(what, got, ref):
    """The bars of test_fused_renderer_vs_reference_fixture: 5e-5 density, 2e-5 coarse weights, 1e-4 rgb / depth / wsum."""
    devs = {k: max_abs(got[k].to(F64), ref[k]) for k in ('den_coarse', 'w_coarse', 'rgb', 'depth', 'wsum')}
    print(f'{what}: fp32 oracle vs fp64: ' + ', '.join(f'{k} {v:.2e}' for k, v in devs.items()))
    assert devs['den_coarse'] <= 5e-5 and devs['w_coarse'] <= 2e-5 and devs['rgb'] <= 1e-4 and devs['depth'] <= 1e-4 and devs['wsum'] <= 1e-4


@pytest.mark.parametrize('size', RR.SIZES)
@pytest.mark.parametrize('white_back', [False, True])
def test_fp64_pipeline_matches_the_oracle(size, white_back):
    sc = RR.scene(60, [3, 4], 8, size, white_back=white_back)
    o = sc.oracle()
    assert torch.equal(o['z_coarse'], RR.coarse_depths(sc.ro, 48, sc.jitter)[0])
    ref = sc.fp64(o['z_fine'])
    _compare(f'{size} white_back={white_back}', o, ref)
    assert torch.equal(ref['order'], torch.sort(torch.cat([o['z_coarse'], o['z_fine']], 2), dim=2, stable=True).indices)
    if white_back:
        assert max_abs(ref['rgb'], RR.scene(60, [3, 4], 8, size).fp64(o['z_fine'])['rgb']) > 0.1


def test_fp64_pipeline_per_frame_and_box_routes():
    """One ``dist`` per frame is one oracle call per frame (the depth clamp is the frame's own range); the box route is
    ``render_eg3d`` with rays that miss the cube, with and without the z flip."""
    sc = RR.scene(61, [0, 3], 8, per_frame=True)
    sc.ro[1] *= 1.03
    o = sc.oracle()
    _compare('per frame', o, sc.fp64(o['z_fine']))
    assert float(o['z_coarse'][1].min() - o['z_coarse'][0].min()) > 0.05
    for flip in (False, True):
        u = torch.from_numpy(np.random.RandomState(5).rand(2 * 64, 48).astype(np.float32)).sort(dim=-1).values
        bx = RR.scene(62, [0, 3], 8, box=dict(u=u, flip_z=flip))
        o = bx.oracle()
        _compare(f'box flip_z={flip}', o, bx.fp64(o['z_fine']))
    assert max_abs(RR.scene(62, [0, 3], 8, box=dict(u=u, flip_z=False)).oracle()['rgb'], o['rgb']) > 1e-2


def test_fp64_pipeline_matches_the_recorded_fixture(golden):
    g = golden('renderer.npz')
    frames, nrr = g['frames'].tolist(), g['nrr']
    sd = {k: torch.empty(s) for k, s in (('net.0.weight', (64, 32)), ('net.0.bias', (64,)), ('net.2.weight', (33, 64)), ('net.2.bias', (33,)))}
    sd = synthetic.fill_parameters(sd, salt=5)
    weights = tuple(sd[k] for k in ('net.0.weight', 'net.0.bias', 'net.2.weight', 'net.2.bias'))
    sub = slice(0, None, 7)                 # every 7th recorded ray
    ref = RR.render_fp64(rnd(20, 2, 3, 32, 64, 64), weights, 1.0, g['rays_o'][:, sub], g['rays_d'][:, sub], g['z_coarse'][:, sub], g['z_fine'][:, sub])
    got = dict(den_coarse=g['den_coarse'][:, sub], w_coarse=g['w_coarse'][:, sub], rgb=g['rgb'][:, sub], depth=g['depth'][:, sub], wsum=g['wsum'][:, sub])
    # the fixture's depth is clamped to the range of ALL its rays
    z = torch.cat([g['z_coarse'], g['z_fine']], 2).to(F64)
    ref['depth'] = ref['depth'].clamp(z.min(), z.max())
    got['depth'] = got['depth'].to(F64).clamp(z.min(), z.max())
    _compare('renderer.npz', got, ref)


def test_march_hand_cases():
    z = torch.linspace(2.0, 3.0, 5, dtype=F64).reshape(1, 1, 5, 1)
    col = torch.rand(1, 1, 5, 3, dtype=F64, generator=torch.Generator().manual_seed(1))
    # empty: no weight anywhere, depth NaN -> +inf -> clamped to the largest depth; rgb = -1, or +1 on a white background
    empty = torch.full((1, 1, 5, 1), -1e4, dtype=F64)
    rgb, depth, wsum, w = RR.march_fp64(col, empty, z)
    assert float(wsum) == 0 and float(depth) == 3.0 and torch.equal(rgb, torch.full_like(rgb, -1.0)) and float(w.abs().max()) == 0
    rgb, _, _, _ = RR.march_fp64(col, empty, z, white_back=True)
    assert torch.equal(rgb, torch.ones_like(rgb))
    # one opaque interval (samples 1 and 2): depth = its midpoint, weight -> 1, colour = the mean of its two ends
    # (the marcher averages neighbouring densities: the samples around the interval are low enough to keep its neighbours empty; the
    # transmittance in front of it is the 1 + 1e-10 of one empty interval)
    sig = torch.full((1, 1, 5, 1), -3e4, dtype=F64)
    sig[0, 0, 1:3] = 1e4
    rgb, depth, wsum, w = RR.march_fp64(col, sig, z)
    assert abs(float(wsum) - 1) < 1e-9 and abs(float(depth) - 2.375) < 1e-12 and abs(float(w[0, 0, 1]) - 1) < 1e-9
    assert float(w[0, 0, 0]) == 0 and float(w[0, 0, 2]) == 0 and float(w[0, 0, 3]) == 0
    assert max_abs(rgb, (col[:, :, 1] + col[:, :, 2]) - 1) < 1e-9
    # an opaque wall in front: what lies behind it keeps the 1e-10 floor of the transmittance, not more
    sig = torch.full((1, 1, 5, 1), 1e4, dtype=F64)
    _, _, _, w = RR.march_fp64(col, sig, z)
    assert abs(float(w[0, 0, 0]) - 1) < 1e-12 and abs(float(w[0, 0, 1]) - 1e-10) < 1e-20 and abs(float(w[0, 0, 3]) - 1e-30) < 1e-40
    # per-frame clamp: each batch element's own depth range
    z2 = torch.cat([z, z + 1.0], 0)
    _, depth, _, _ = RR.march_fp64(col.expand(2, -1, -1, -1), empty.expand(2, -1, -1, -1), z2, per_frame=True)
    assert depth.flatten().tolist() == [3.0, 4.0]
    _, depth, _, _ = RR.march_fp64(col.expand(2, -1, -1, -1), empty.expand(2, -1, -1, -1), z2)
    assert depth.flatten().tolist() == [4.0, 4.0]


@pytest.mark.parametrize('size', RR.SIZES)
def test_edge_scenes_reach_their_targets(size):
    """The scaling helper on the reference alone, and the condition the GPU tests rely on: the CPU oracle is inside the bars on every
    in-domain scene (``Scene.tolerances`` raises otherwise)."""
    for name in RR.DOMAIN_CASES:
        sc, m = RR.domain_case(name, size)
        RR.check_targets(name, sc, m)
        tol = sc.tolerances()
        print(f'{size} {name}: ' + ', '.join(f'{k} CPU {v[1]:.2e} / tol {v[0]:.2e} / bar {v[2]:.2e}' for k, v in tol.items()))
        assert all(0 < v[0] <= v[2] for v in tol.values())
    for name in ('feature_over', 'hidden_over'):
        sc, m = RR.domain_case(name, size)
        RR.check_targets(name, sc, m)
