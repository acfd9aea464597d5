"""tests/conv_reference.py without a device: the float64 layer against torch.nn.functional and against the packed product of
hipops.compose_upfir_weight; the restated planner against the library's own plan entries (host code: they run without a GPU); the
coverage of the case tables, asserted as sets of routes so that a planner change that moves a case off its route fails here; and the
power of the tables to tell each wrong restatement (conv_reference.WRONG) from the right one."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

from invertavatar_amd import _lib, hipops
import conv_reference as C
import resample_reference as R

F64 = torch.float64
ALL = [c for t in C.TABLES.values() for c in t]
ROUTES = {c: C.expected_route(c) for c in ALL}


# ------------------------------------------------------------------ self-consistency

@pytest.mark.parametrize('op', ['conv', 'down', 'up'])
def test_layer_sums_are_the_library_convolutions_and_the_tap_loop(op):
    x, w = R.image(2, 5, 9, 7, 21).double(), R.image(6, 5, 3, 3, 22).double()
    want = {'conv': lambda: F.conv2d(x, w, padding=1), 'down': lambda: F.conv2d(x, w, stride=2, padding=1),
            'up': lambda: F.conv_transpose2d(x, w.transpose(0, 1), stride=2)}[op]()
    assert torch.equal(C.raw(x, w, op), want)
    assert (C.raw_taps(x, w, op) - want).abs().max() <= 1e-13 * want.abs().max()
    assert want.shape[2:] == {'conv': (9, 7), 'down': (5, 4), 'up': (19, 15)}[op]


def test_composed_upfir_from_its_factors_equals_the_packed_product():
    """Transposed convolution then the 4x4 FIR (padding [1,1,1,1], gain 4) = the stride-1 convolution with compose_upfir_weight's rows
    ((py * O/32 + o // 32) * 2 + px) * 32 + o % 32, stored depth-to-space."""
    b, i, o, h, w = 2, 3, 32, 6, 5
    x, wt, f = R.image(b, i, h, w, 23).double(), R.image(o, i, 3, 3, 24).double(), C.FIR()
    want = C.raw(x, wt, 'upfir', f)
    wc = hipops.compose_upfir_weight(wt, f).double()
    y = F.conv2d(x, wc, padding=1).view(b, 2, o // 32, 2, 32, h, w)            # [b, py, block, px, channel, r, c]
    got = y.permute(0, 2, 4, 5, 1, 6, 3).reshape(b, o, 2 * h, 2 * w)
    # (the product is returned as float32: each of its weights is within 2^-24 of the factors' product, so each sum within 2^-24 sum |x * w|)
    assert want.shape == got.shape
    slack = F.conv2d(x.abs(), wc.abs(), padding=1).view(b, 2, o // 32, 2, 32, h, w).permute(0, 2, 4, 5, 1, 6, 3).reshape(b, o, 2 * h, 2 * w)
    assert ((got - want).abs() <= 2.0 ** -24 * slack + 1e-12 * want.abs().max()).all()


def test_epilogue_order():
    x, w = R.image(1, 8, 4, 4, 25).double(), R.image(8, 8, 3, 3, 26).double()
    d, nz, bi, sl, res = (R.image(1, 8, 1, 1, 27).double().view(1, 8) + 2, R.image(1, 1, 4, 4, 28).double().view(16), R.image(1, 8, 1, 1, 29).double().view(8),
                          R.image(1, 8, 1, 1, 30).double().view(8).abs() * 0.3, R.image(1, 8, 4, 4, 31).double())
    y, pre, acc = C.layer(x, w, 'conv', None, d, nz, torch.tensor([0.5], dtype=F64), bi, sl, 1.5, 0.7, res)
    v = F.conv2d(x, w, padding=1) * d[:, :, None, None] + nz.view(4, 4) * 0.5 + bi[None, :, None, None]
    assert torch.equal(pre, v)
    v = (torch.where(v > 0, v, v * sl[None, :, None, None]) * 1.5).clamp(-0.7, 0.7) + res
    assert torch.equal(y, v)


# ------------------------------------------------------------------ the restated planner against the library

def _plan(fn, *args):
    ks, nbytes = ctypes.c_int(-1), ctypes.c_size_t(0)
    st = fn(*args, ctypes.byref(ks), ctypes.byref(nbytes))
    return st, ks.value, nbytes.value


@pytest.mark.parametrize('case', [c for c in ALL if c.entry != 'tiny'], ids=lambda c: c.name)
def test_expected_route_agrees_with_the_library_plan(case):
    lib, c, r = _lib.load(), case, ROUTES[case]
    default = C.expected_route(c._replace(ksplit=None))
    if c.entry in ('sx', 'rgb', 'upfir', 'mfma'):
        st, ks, nbytes = _plan(lib.ia_conv2d_plan, c.b, c.i, 4 * c.o if c.entry == 'upfir' else c.o, c.h, c.w, c.ksize, int(c.tr), c.form)
        assert (st, ks, nbytes) == (0, default.workers, default.scratch)
        if default.workers:         # scratch = B * G * 2 slabs of bo * bp (x 4 phases) floats: the tile itself is pinned wherever slabs exist
            bo, bp = (int(v) for v in default.family.split('/')[0].split(' ')[0].split('x'))
            assert nbytes == c.b * ks * 2 * bo * bp * (4 if c.tr else 1) * 4
    elif c.entry == 'down':
        assert _plan(lib.ia_conv2d_down_plan, c.b, c.i, c.o, c.h, c.w) == (0, r.workers, r.scratch)
    else:
        nbytes = ctypes.c_size_t(0)
        assert lib.ia_upconv2d_rows_plan(c.b, c.i, c.o, c.h, c.w, ctypes.byref(nbytes)) == 0 and nbytes.value == r.scratch


def test_plan_entries_refuse_what_the_restatement_refuses():
    lib = _lib.load()
    nbytes = ctypes.c_size_t(0)
    for shape in ((1, 24, 128, 64, 64), (1, 32, 64, 64, 64), (1, 32, 128, 8, 8)):
        assert C.rows_route(*shape).mode == 'refused' and lib.ia_upconv2d_rows_plan(*shape, ctypes.byref(nbytes)) != 0
    for shape in ((1, 64, 32, 64, 64), (1, 512, 512, 8, 8), (1, 60, 64, 64, 64)):
        assert C.sx_route(*shape, stride=2, entry='down').mode == 'refused' and _plan(lib.ia_conv2d_down_plan, *shape)[0] != 0
    for i, o, h, w in ((16, 70, 7, 7), (1024, 8, 8, 8), (8, 8, 16, 16), (8, 8, 8, 4)):
        assert lib.ia_conv3x3_s2_tiny_supported(i, o, h, w) == (C.expected_route(C.Case('', 'tiny', 1, i, o, h, w)).mode == 'tiny')
    for case, _ in C.REFUSALS:
        assert C.expected_route(case).mode == 'refused', case.name
    # Widths whose 256-point windows pass kPatchFloats fall off the two-stage tiles: the dispatcher refuses them (ia_conv2d_sx_supported
    # does not know: it answers by W <= 512 alone)
    for w in (255, 257, 300):
        assert C.sx_route(1, 8, 128, 5, w).mode == 'refused'
    # ... and ia_conv2d_sx_supported says what the dispatcher will do, width by width
    for h, w in ((8, 200), (17, 200), (8, 254), (8, 255), (8, 256), (8, 257), (9, 300), (8, 384), (8, 511), (8, 512), (8, 513), (33, 33), (64, 129)):
        for tr in (False, True):
            accepted = C.sx_route(1, 8, 128, h, w, tr=tr).mode != 'refused' and (tr or w <= 512)
            assert lib.ia_conv2d_sx_supported(8, 128, h, w, 3, int(tr)) == int(accepted), (h, w, tr)


# ------------------------------------------------------------------ coverage

def _routes(table, **want):
    return [r for r in (ROUTES[c] for c in C.TABLES[table]) if all(getattr(r, k) == v for k, v in want.items())]


def test_tables_reach_every_route():
    """The routes are those of the restatement.  What pins the restatement to the library: worker counts and scratch bytes of every case
    (test_expected_route_agrees_with_the_library_plan), which give the tile (bo x bp) wherever a layer has slabs.  A layer that runs in whole
    rounds has neither workers nor slabs, so which whole-tile family it takes (wide, narrow, antiphase; the rule is B-dependent and the narrow
    families never have slabs) is NOT visible through the plan entries: there the restatement of tile_dims / make_plan stands alone, and a
    planner change that moves such a case is seen only by whoever updates the restatement."""
    fam = lambda table: {(r.family, r.narrow, r.antiphase, r.mode.replace('whole+', '')) for r in _routes(table)}      # noqa: E731
    # conv_sx_impl, stride 1.  The 64 x 256 stride-1 narrow family of the dispatcher is not in this set: no plan of make_plan yields it
    # (tile_dims never returns 64 channels for a stride-1 layer), so no caller can reach launch_sx<2, false, 1, 2, 2, 4, true>.
    assert fam('sx') == {('128x256/8', False, False, 'whole'), ('128x256/8', False, False, 'stream-k'), ('128x256/8', False, False, 'fix-up'),
                         ('32x256/8', True, False, 'whole'), ('32x256/8', True, True, 'whole')}
    assert {r.mode for r in _routes('sx')} >= {'whole', 'whole+fix-up', 'stream-k', 'fix-up'}
    # transposed.  The 64 x 128 tile belongs to the register-staged pair form alone (tile_dims: form 2); it is reached in the 'mfma' table.
    assert fam('transposed') == {('64x64/4', False, False, m) for m in ('whole', 'stream-k', 'fix-up')} | {('64x256/8', False, False, m) for m in ('whole', 'stream-k', 'fix-up')}
    assert fam('down') == {('128x256/8', False, False, 'stream-k'), ('128x256/8', False, False, 'fix-up'), ('32x256/8', True, False, 'whole')}
    assert fam('upfir') == fam('rgb') == {('128x256/8', False, False, 'whole')}
    assert {r.mode for r in _routes('small')} == {'small'}
    for table in ('sx', 'small', 'transposed', 'down', 'upfir', 'rgb'):
        assert {c.planes for c in C.TABLES[table]} == {1, 2}, table
    # windows, DMA depth, chunk counts and parities
    every = {'single', 'split', 'full'}
    assert set().union(*(r.windows for r in _routes('sx', narrow=False))) == every
    assert set().union(*(r.windows for r in _routes('sx', narrow=True))) == every
    assert set().union(*(r.windows for r in _routes('transposed', family='64x64/4'))) == every
    assert set().union(*(r.windows for r in _routes('transposed', family='64x256/8'))) == every
    assert set().union(*(r.windows for r in _routes('down', narrow=False))) == {'single', 'full'} and {'full'} == set().union(*(r.windows for r in _routes('down', narrow=True)))
    assert {r.jp for r in _routes('sx')} | {r.jp for r in _routes('down')} == {2, 4, 8}
    for table in ('sx', 'small', 'transposed'):
        assert {r.chunks for r in _routes(table)} == {'C=1', 'even', 'odd'} or table == 'small', table
    assert {r.chunks for r in _routes('small')} == {'even', 'odd'}
    assert set().union(*(r.parity for r in _routes('sx'))) == {'even', 'odd'}
    flags = lambda table: set().union(*(r.flags for r in _routes(table)))      # noqa: E731
    assert flags('sx') >= {'cut inside a chunk pair', 'cut at a pair boundary', 'one chunk per worker', 'workers clamped to U', 'trailing slot', 'B=2', 'B=3',
                           'tile starts mid-row', 'full last tile', 'ragged points', 'ragged channels', 'fix-up launched, no tile cut'}
    assert flags('transposed') >= {'trailing slot', 'B=2', 'one chunk per worker', 'fix-up launched, no tile cut', 'ragged channels', 'ragged points'}
    assert flags('small') >= {'octets<waves', 'ragged points', 'ragged channels'}
    assert {c.tr for c in C.SMALL_CASES} == {False, True}
    assert flags('rows') >= {'interior tiles', 'bottom row', 'last column', 'whole edge tiles', 'K-split edge tiles', 'K-split long tiles', 'row phases paired', 'B=3'}
    assert {r.family for r in _routes('rows')} == {'128x128/8', '128x256/8'}
    assert {c.rgb_n for c in C.RGB_CASES} == {1, 3}
    # register-staged forms
    got = {(r.entry, r.family) for r in _routes('mfma')}
    assert got >= {('mfma', f) for f in ('128x32/4 k3', '128x32/4 k1', '32x256/4 k3', '32x256/4 k1', '128x128/4 k3', '128x128/4 k1', '128x256/8 k3',
                                        '64x64/4 k3 transposed', '128x32/4 k3 transposed')}
    assert got >= {('mfma_h', '128x256/8 k3'), ('mfma_h', '64x64/4 k3 transposed'), ('mfma_s', '128x256/8 k3'), ('mfma_s', '64x64/4 k3 transposed'),
                   ('mfma_s', '64x128/4 k3 transposed')}
    assert flags('mfma') >= {'quad store', 'per-element store', 'workers clamped to U'}
    assert {r.mode for r in _routes('mfma')} >= {'stream-k', 'fix-up'}
    assert {r.mode for r in _routes('tiny')} == {'tiny'} and {c.h for c in C.TINY_CASES} == {2, 4, 8}
    # channel counts and image shapes at the rules' edges
    sx_all = [c for t in ('sx', 'small', 'transposed', 'down') for c in C.TABLES[t]]
    assert any(c.i % 8 == 0 and c.i % 16 for c in sx_all) and any(c.o % 8 == 0 and c.o % 32 and c.o % 128 for c in sx_all) and any(c.o == 8 for c in sx_all)
    assert {c.o % 4 == 0 for c in C.MFMA_CASES if c.tr and c.form == 0} == {True, False}
    assert any(c.h != c.w for c in sx_all) and any(c.tr and c.h % 2 and c.w % 2 for c in sx_all)
    assert {c.w for c in sx_all} >= {8, 9, 200, 256, 512}
    # every option of the epilogue on and off
    opts = [c.epi for c in ALL]
    for field in ('demod', 'noise', 'strength', 'bias', 'residual', 'styles_next', 'want_f32'):
        assert {getattr(e, field) for e in opts} == {True, False}, field
    assert {e.slope for e in opts} == {None, 'scalar', 'prelu'} and {e.split_planes for e in opts} == {1, 2}
    assert {e.clamp is None for e in opts} == {True, False} and {e.gain == 1.0 for e in opts} == {True, False}


# ------------------------------------------------------------------ discriminating power

def test_float32_restatement_stays_within_the_bound_and_the_clamp_bites():
    for case in ALL:
        ref = C.reference(case)
        got = C.run(case, torch.float32)[0]
        assert C.ratio(got, ref.y, ref.tol) <= 1, case.name
        if ref.clamp is not None:
            v = ref.y - (C.inputs(case)['residual'].double() if case.epi.residual else 0)
            share = float((v.abs() >= ref.clamp * (1 - 1e-12)).double().mean())
            assert 0.05 <= share <= 0.6, (case.name, share)


@pytest.mark.parametrize('wrong', C.WRONG)
def test_every_table_tells_a_wrong_restatement_from_the_right_one(wrong):
    seen = 0
    for table, cases in C.TABLES.items():
        applies = sorted((c for c in cases if C.wrong_applies(wrong, c)), key=lambda c: c.b * c.i * c.o * c.h * c.w)
        if not applies:
            continue
        seen += 1
        assert any(C.wrong_ratio(c, wrong) > 1 for c in applies), (wrong, table)
    assert seen >= 1, wrong
