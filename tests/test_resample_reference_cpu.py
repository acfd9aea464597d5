"""tests/resample_reference.py against the reference's recorded outputs and the project's own torch routes in float64, the coverage
of its case tables (checked against a restatement of the dispatch of csrc/upfirdn2d.hip), and the proof that those tables tell a wrong
kernel from a right one: every plausible error, written as a ``wrong=`` variant of a restatement, moves the result by at least ten
times the tolerance that tests/test_resample_gpu.py applies to the same case, on every case the error can show on."""
import collections

import pytest
import torch

from invertavatar_amd.torch_utils.ops import filtered_lrelu as flr, upfirdn2d as ufd
from conftest import max_abs, rnd
import resample_reference as R
from test_filtered_lrelu import CASES as FLR_GOLDEN, _case as _flr_golden

F64 = torch.float64


def _same(a, b, what=''):
    d, bar = max_abs(a, b), 1e-12 * max(1.0, float(b.abs().max()))
    assert a.shape == b.shape and d <= bar, f'{what}: {d:.2e} > {bar:.2e}'


# ------------------------------------------------------------------ a) the restatements are the operations

def test_upfirdn2d_restatement_reproduces_the_golden_outputs(golden):
    g = golden('ops.npz')
    f, x = ufd.setup_filter([1, 3, 3, 1]), rnd(4, 2, 5, 13, 11).double()
    assert max_abs(R.upfirdn2d(x, f, pad=1, gain=4.0), g['upfirdn2d/blur_pad1']) <= 2e-6
    assert max_abs(R.upfirdn2d(x, f, up=2, pad=(2, 1, 2, 1), gain=4.0), g['upfirdn2d/up2']) <= 2e-6
    assert max_abs(R.upfirdn2d(x, f, down=2, pad=1), g['upfirdn2d/down2']) <= 2e-6
    assert max_abs(R.upfirdn2d(x, rnd(5, 3, 5).abs(), **{**R.MIXED, 'pad': R.MIXED['pad']}), g['upfirdn2d/mixed']) <= 2e-6
    assert max_abs(R.upfirdn2d(x, torch.tensor([1., 3., 3., 1.]) / 8, up=2, pad=(2, 1, 2, 1), gain=4.0), g['upfirdn2d/sep']) <= 2e-6


@pytest.mark.parametrize('name', list(FLR_GOLDEN))
def test_filtered_lrelu_restatement_reproduces_the_golden_outputs(golden, name):
    x, y, kw = _flr_golden(golden('filtered_lrelu.npz'), name)
    d = lambda t: None if t is None else t.double()      # noqa: E731
    got = R.filtered_lrelu(x.double(), kw['fu'], kw['fd'], d(kw['b']), kw['up'], kw['down'], kw['padding'], kw['gain'], kw['slope'], kw['clamp'],
                           kw['flip_filter'])
    assert got.shape == y.shape and max_abs(got, y) <= 2e-6


@pytest.mark.parametrize('case', R.GENERIC_CASES[:-2] + R.TILED_CASES[1, 'f32'][:6] + R.TILED_CASES[2, 'f16'][6:12] + R.PIPE_CASES[:1],
                         ids=lambda c: c.name)
def test_upfirdn2d_restatement_is_the_torch_route(case):
    x, f = R.fir_inputs(case)
    want = ufd._upfirdn2d_ref(x.double(), f, up=list(case.up), down=list(case.down), padding=list(case.pad), flip_filter=case.flip, gain=case.gain)
    _same(R.fir_reference(case), want, case.name)
    assert tuple(want.shape[2:]) == case.out_hw


def test_one_dimensional_filter_restated_as_its_outer_product():
    x, f = R.image(2, 2, 9, 8).double(), R.fir_filter(5, None)
    kw = dict(up=[2, 1], down=[1, 2], padding=[3, 1, 2, 2], flip_filter=True, gain=2.5)
    _same(R.upfirdn2d(x, f, (2, 1), (1, 2), (3, 1, 2, 2), True, 2.5), ufd._upfirdn2d_ref(x, f, **kw), '1-D')
    k1 = (f * 2.5 ** 0.5).double()                      # (the gain meets the float32 taps in float32, half of it per pass)
    _same(R.upfirdn2d(x, f, (2, 1), (1, 2), (3, 1, 2, 2), True, 2.5), R.upfirdn2d(x, torch.outer(k1, k1), (2, 1), (1, 2), (3, 1, 2, 2), True, 1.0), 'outer')


@pytest.mark.parametrize('case', R.FLR_CASES[::4], ids=lambda c: c.name)
def test_filtered_lrelu_restatement_is_the_torch_route(case):
    x, fu, fd, b = R.flr_inputs(case)
    want = flr._filtered_lrelu_ref(x.double(), fu, fd, None if b is None else b.double(), up=case.up, down=case.down, padding=list(case.pad),
                                   gain=2 ** 0.5, slope=case.slope, clamp=case.clamp, flip_filter=case.flip)
    _same(R.flr_reference(case), want, case.name)


def test_fir_tail_restatement_is_upfirdn2d_then_bias_act():
    from invertavatar_amd.torch_utils.ops import bias_act
    for up, out_hw, pad0, flip, _ in R.FUSED_TAIL_GEOMETRY[:4]:
        case = R.fused_tail_case(up, out_hw, pad0, flip, 'f32')
        x, f = R.fir_inputs(case)
        t = {k: v.double() for k, v in R.tail_inputs(case.shape[1], *out_hw).items()}
        for tail in R.TAIL_OPTIONS:
            kw = tail.kwargs(t)
            got = R.fir_tail(x.double(), f, out_hw, up, pad0, case.gain, flip=flip, **kw)
            v = ufd._upfirdn2d_ref(x.double(), f, up=up, padding=list(case.pad), flip_filter=flip, gain=case.gain)
            if tail.noise:
                v = v + t['noise'].reshape(out_hw) * (t['strength'] if tail.strength else 1.0)
            want = bias_act._bias_act_ref(v, kw['bias'], act=tail.act, alpha=tail.alpha, gain=tail.gain, clamp=tail.clamp)
            _same(got, want, f'{case.name} {tail}')


def test_clamps_of_the_restatements_keep_a_nan_and_bound_an_infinity():
    x = torch.zeros(1, 1, 6, 6, dtype=F64)
    x[0, 0, 2, 2], f = float('nan'), R.fir_filter(4, 4)
    y = R.fir_tail(x, f, (5, 5), pad0=(1, 1), clamp=2.0)
    assert y.isnan().sum() == 16 and (y[~y.isnan()] == 0).all()
    x[0, 0, 2, 2] = float('inf')
    assert (R.fir_tail(x, f, (5, 5), pad0=(1, 1), clamp=2.0) == 2.0).sum() == 16


def test_split_pair_carries_22_bits_and_drops_a_denormal_high_part():
    v = torch.cat([R.image(2, 8, 5, 7) * torch.logspace(-7, 4, 8)[None, :, None, None], torch.tensor([1e6, -1e6]).expand(2, 8, 5, 2)], 3)
    s = torch.rand(2, 8, generator=torch.Generator().manual_seed(1)) + 0.5
    hi, lo = R.split_pair(v, s)
    t = (v * s[:, :, None, None]).clamp(-65504, 65504)
    assert ((R.pair_value(hi, lo) - t.double()).abs() <= R.split_bound(t.double())).all()
    assert (hi[t.abs() < 2.0 ** -14] == 0).all() and (hi[..., -2:].abs() == 65504).all()
    one, none = R.split_pair(v, s, planes=1)
    assert none is None and torch.equal(one, t.half())


# ------------------------------------------------------------------ b) the tables reach every form and every edge

def _all_fir_cases():
    cases = [c for table in R.TILED_CASES.values() for c in table] + list(R.PIPE_CASES) + list(R.MULTI_TILE_CASES) + list(R.GENERIC_CASES)
    return [(c, R.expected_form(c)) for c in cases]


def test_tables_reach_every_form_at_least_three_times():
    count = collections.Counter(form for _, form in _all_fir_cases())
    for g in R.FUSED_TAIL_GEOMETRY:
        count[R.expected_form(R.fused_tail_case(*g), 'bias_act')] += 1
    for s in R.SPLIT_GEOMETRY + R.SPLIT_OPTIONS:
        count[R.expected_form(s.fir, 'split', want_f32=True)] += 1
        count[R.expected_form(s.fir, 'split', want_f32=False)] += 1
    print(dict(count))
    for form in ('generic', 'tiled up1', 'tiled up2', 'pipe', 'tail-register', 'tail-dma'):
        assert count[form] >= 3, form
    assert all(R.expected_form(c) == 'pipe' for c in R.PIPE_CASES)
    assert all(R.expected_form(c) == 'tiled up1' for c in R.MULTI_TILE_CASES)
    assert all(R.expected_form(c) == 'generic' for c in R.GENERIC_CASES)
    assert all(R.expected_form(c) == f'tiled up{up}' for (up, _), table in R.TILED_CASES.items() for c in table)


def test_pipe_cases_have_ragged_tiles_and_workgroups_across_tile_rows():
    pipe = [c for c, form in _all_fir_cases() if form == 'pipe']
    assert any(c.out_hw[1] % 64 for c in pipe) and any(c.out_hw[0] % 16 for c in pipe)
    assert any(R.pipe_workgroup_spans_two_tile_rows(c) for c in pipe)
    assert {c.dtype for c in pipe} == {'f32', 'f16'} and {c.flip for c in pipe} == {False, True}
    assert {(c.pad[0], c.pad[2]) for c in pipe} == set(R.PIPE_PADS)
    assert R.expected_form(R.fused_tail_case(*R.FUSED_TAIL_GEOMETRY[-1]), 'bias_act') == 'pipe'


@pytest.mark.parametrize('key', list(R.TILED_CASES))
def test_tiled_table_covers_sizes_pads_and_flips(key):
    table = R.TILED_CASES[key]
    assert {c.out_hw[1] for c in table} == set(R.TILED_OUT_W) and {c.out_hw[0] for c in table} == set(R.TILED_OUT_H)
    assert {c.out_hw for c in table} >= {(h, w) for h in R.TILED_OUT_H for w in R.TILED_OUT_W}
    assert {c.pad[0] for c in table} == set(R.TILED_PADS) and {c.pad[2] for c in table} == set(R.TILED_PADS)
    assert all(c.pad[0] != c.pad[2] for c in table) and {c.flip for c in table} == {False, True}
    assert all(c.shape[2] >= 1 and c.shape[3] >= 1 for c in table)


def test_generic_table_covers_the_listed_rows():
    g = {c.name: c for c in R.GENERIC_CASES}
    assert {c.dtype for c in R.GENERIC_CASES} == {'f32', 'f16', 'f64'} and {c.layout for c in R.GENERIC_CASES} == set(R.LAYOUTS)
    assert {(1, 7), (32, 32), (5, 3)} <= {c.fshape for c in R.GENERIC_CASES} and any(c.f_transposed for c in R.GENERIC_CASES)
    assert g['up (3,1) down (1,4)'].up == (3, 1) and g['up (3,1) down (1,4)'].down == (1, 4)
    assert g['output 1x1'].out_hw == (1, 1) and g['output 1x1 down 5'].out_hw == (1, 1)
    big = g['grid-stride loop']
    assert big.shape[0] * big.shape[1] * big.out_hw[0] * big.out_hw[1] > R.GRID_STRIDE_OUTPUTS
    many = g['65537 planes, tiled-shaped']
    assert many.shape == (1, 65537, 2, 3) and R.expected_form(many._replace(shape=(1, 65535, 2, 3))) == 'tiled up2'
    assert {c.shape[1] for c in R.GENERIC_CASES if c.layout == 'channels_last'} >= {1, 5}


def test_split_tables_cover_geometry_and_options():
    geo = R.SPLIT_GEOMETRY
    assert {(s.out_hw, s.pad0) for s in geo} == {(hw, p) for hw in R.SPLIT_OUT_HW for p in R.SPLIT_PAD0}
    for hw in R.SPLIT_OUT_HW:
        mine = [s for s in geo if s.out_hw == hw]
        assert {s.planes for s in mine} == {1, 2} and {s.c for s in mine} == {8, 24} and {s.b for s in mine} == {1, 2}
    tails = {s.tail for s in R.SPLIT_OPTIONS}
    assert tails >= set(R.TAIL_OPTIONS)
    assert any(not s.styles for s in R.SPLIT_OPTIONS) and any(s.tiny_channel for s in R.SPLIT_OPTIONS) and any(s.planes == 1 for s in R.SPLIT_OPTIONS)
    combos = {(t.noise, t.bias, t.clamp is not None, t.act) for t in R.TAIL_OPTIONS}
    assert len(combos) == 16 and any(t.noise and not t.strength for t in R.TAIL_OPTIONS) and any(t.alpha != 0.2 for t in R.TAIL_OPTIONS)


def test_filtered_lrelu_table_covers_the_tile_edge_and_the_options():
    t = R.FLR_CASES
    sizes = {(c.up, c.down): set() for c in t}
    for c in t:
        ref = R.flr_reference(c, dtype=torch.float32)
        sizes[c.up, c.down].add((ref.shape[3], ref.shape[2]))
    want = {(w, h) for w in R.FLR_OUT_W for h in R.FLR_OUT_H}
    assert set(sizes) == set(R.FLR_RATES) and all(s == want for s in sizes.values()), sizes
    assert any(c.fu is None and c.fd is not None for c in t) and any(c.fd is None and c.fu is not None for c in t) and any(c.fu is None and c.fd is None for c in t)
    assert any(c.slope == 0 for c in t) and any(c.dtype == 'f16' for c in t) and any(c.clamp is None for c in t) and any(c.flip for c in t)
    assert any(min(c.pad) < 0 for c in t) and all(c.pad[0] != c.pad[1] or c.pad[2] != c.pad[3] for c in t)


# ------------------------------------------------------------------ c) the tables tell a wrong kernel from a right one

def _moves(ref, wrong, tol):
    return float(((wrong - ref).abs() / tol).max())


def _discriminates(what, ref, tol, variants):
    """variants: {name: tensor or None (does not apply)}; every one that applies must move the result by 10 x its tolerance."""
    for name, w in variants.items():
        if w is not None:
            m = _moves(ref, w, tol)
            assert m >= 10, f'{what}: wrong={name} moves the result by only {m:.2f} x the tolerance'


@pytest.mark.parametrize('table', ['tiled up1 f32', 'tiled up1 f16', 'tiled up2 f32', 'tiled up2 f16', 'pipe', 'multi-tile', 'generic'])
def test_fir_tables_discriminate_every_wrong_variant(table):
    cases = {'pipe': R.PIPE_CASES, 'multi-tile': R.MULTI_TILE_CASES, 'generic': R.GENERIC_CASES}.get(table)
    if cases is None:
        _, up, dtype = table.split()
        cases = R.TILED_CASES[int(up[2:]), dtype]
    applied = collections.Counter()
    for c in cases:
        if c.shape[1] > 1000 or c.shape[2] > 400 and table == 'generic':
            continue                    # the many-plane and grid-stride cases repeat small geometries for their size alone
        ref = R.fir_reference(c)
        tol = R.tolerance(ref, float((R.fir_reference(c, dtype=torch.float32).double() - ref).abs().max()), c.dtype)
        variants = {w: (R.fir_reference(c, w) if R.wrong_applies(w, c.up, c.pad) else None) for w in R.WRONG_FIR}
        applied.update(w for w, v in variants.items() if v is not None)
        _discriminates(c.name, ref, tol, variants)
    need = {'no_flip', 'edge_clamp'} | ({'phase', 'pad_order'} if 'up1' not in table and table not in ('pipe', 'multi-tile') else set())
    assert all(applied[w] >= 3 for w in need), applied


def test_fused_tail_table_discriminates_every_wrong_variant():
    applied = collections.Counter()
    for g in R.FUSED_TAIL_GEOMETRY[:4]:
        up, out_hw, pad0, flip, dtype = g
        case = R.fused_tail_case(*g)
        x, f = R.fir_inputs(case)
        t = R.tail_inputs(case.shape[1], *out_hw)
        if dtype == 'f16':
            t = {**t, 'bias': t['bias'].half().float()}
        for tail in R.TAIL_OPTIONS:
            run = lambda dt, wrong=None: R.fir_tail(x.to(dt), f, out_hw, up, pad0, case.gain, flip=flip, wrong=wrong,      # noqa: E731
                                                    **tail.kwargs({k: v.to(dt) for k, v in t.items()}))
            ref = run(F64)
            tol = R.tolerance(ref, float((run(torch.float32).double() - ref).abs().max()), dtype)
            variants = {w: (run(F64, w) if R.wrong_applies(w, case.up, case.pad, tail, case.shape[3], out_hw[1]) else None) for w in R.WRONG_TAIL}
            applied.update(w for w, v in variants.items() if v is not None)
            _discriminates(f'{case.name} {tail}', ref, tol, variants)
    assert all(applied[w] >= 3 for w in R.WRONG_TAIL), applied


def test_split_tables_discriminate_every_wrong_variant():
    applied = collections.Counter()
    for s in R.SPLIT_GEOMETRY + R.SPLIT_OPTIONS:
        i, fir = R.split_inputs(s), s.fir
        run = lambda dt, wrong=None: R.fir_tail(i['x'].to(dt), i['f'], s.out_hw, 1, s.pad0, 1.0, wrong=wrong,      # noqa: E731
                                                **s.tail.kwargs({k: v.to(dt) for k, v in i.items()}))
        ref = run(F64)
        tol = R.tolerance(ref, float((run(torch.float32).double() - ref).abs().max()))
        variants = {w: (run(F64, w) if R.wrong_applies(w, fir.up, fir.pad, s.tail, fir.shape[3], s.out_hw[1]) else None) for w in R.WRONG_TAIL}
        applied.update(w for w, v in variants.items() if v is not None)
        _discriminates(f'{s}', ref, tol, variants)
        if s.planes == 2:
            y = run(torch.float32)
            sn = i['styles'] if s.styles else None
            hi, lo = R.split_pair(y, sn)
            bad = R.split_pair(y, sn, wrong='lo_scale')
            assert not torch.equal(lo, bad[1]) and torch.equal(hi, bad[0])
            t = (y if sn is None else y * sn[:, :, None, None]).double()
            assert float(((R.pair_value(*bad) - t).abs() / R.split_bound(t)).max()) >= 10
            if s.tiny_channel:
                assert (hi[:, 1] == 0).all() and (lo[:, 1] != 0).any()
    assert all(applied[w] >= 3 for w in set(R.WRONG_TAIL) - {'phase', 'pad_order'}), applied


def test_filtered_lrelu_table_discriminates_every_wrong_variant():
    applied = collections.Counter()
    for c in R.FLR_CASES:
        ref = R.flr_reference(c)
        tol = R.tolerance(ref, float((R.flr_reference(c, dtype=torch.float32).double() - ref).abs().max()), c.dtype)
        up = (c.up, c.up)
        variants = {w: (R.flr_reference(c, w) if R.wrong_applies(w, up, c.pad) else None) for w in R.WRONG_FLR}
        if c.fu is None and c.fd is None:
            variants['no_flip'] = None                        # nothing to flip
        applied.update(w for w, v in variants.items() if v is not None)
        _discriminates(c.name, ref, tol, variants)
    assert all(applied[w] >= 3 for w in R.WRONG_FLR), applied
