"""ia_rasterize_level on the levels that run the tiled kernel (64^2, 128^2), through hipops, against the float64 restatement and with the
tolerance of tests/test_frame_glue_gpu.py, over tests/rasterize_tiles_cases.py (whose coverage of the kernel's paths
tests/test_rasterize_tiles_reference_cpu.py establishes; asserted here again so that this file cannot pass on one path alone)."""
import pytest
import torch

from invertavatar_amd import hipops
import frame_glue_reference as R
import rasterize_tiles_cases as T

pytestmark = pytest.mark.gpu


def _on_device(case):
    i = R.rast_inputs(case)
    return hipops.rasterize_level(i['tex'].cuda(), i['uv'].cuda(), i['upper'].cuda(), i['sta_wide'].cuda(), case.bbox, case.res)


@pytest.mark.parametrize('case', T.CASES, ids=lambda c: c.name)
def test_rasterize_tiles(case):
    got = _on_device(case)
    ref, forms = R.rast_reference(case), R.rast_forms(case)
    e32 = R.e32_of(R.rast_reference(case, torch.float32), ref)
    tol = R.rasterize_tolerance(ref, e32, int(forms['n_src'].max()), float(R.rast_inputs(case)['tex'].abs().max()))
    err = (got.cpu().double() - ref).abs()
    assert tuple(got.shape) == tuple(ref.shape) and torch.isfinite(err).all()
    per_group = (err / tol).amax(1).reshape(case.B, case.res, case.res // 4, 4).amax(-1)
    worst = 0.0
    for k, form in enumerate(R.FORMS):
        sel = forms['form'] == k
        if sel.any():
            r = float(per_group[sel].max())
            print(f'RATIO rasterize tiles {form} ({int(sel.sum())} groups) {case.name}: {r:.3f}')
            worst = max(worst, r)
    assert worst <= 1


def test_rasterize_tiles_reach_every_path():
    seen, _ = T.coverage()
    for key in ('none', 'one', 'two', 'direct', 'tile direct + merged', 'tile one + two', 'crop tabulated', 'crop looped'):
        assert seen[key] > 0, (key, seen)


def test_rasterize_tiles_run_to_run_identical():
    assert torch.equal(_on_device(T.DETERMINISM_CASE), _on_device(T.DETERMINISM_CASE))
