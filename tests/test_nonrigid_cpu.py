"""The definition of the non-rigid fit (geometry.nonrigid_align / nonrigid_solve, NumPy restatement): the solve against a dense solve,
its conjugate-gradient properties, the fit on a sphere -> bumped ellipsoid pair, pins, landmarks, normal rejection, arguments, CLI."""
import json
import os
import sys

import numpy as np
import pytest
import torch

from invertavatar_amd import geometry, geometry_metrics

sys.path.insert(0, os.path.dirname(__file__))
import nonrigid_cases as NC  # noqa: E402

F32 = np.float32


def bits(a):
    return np.ascontiguousarray(a).view(np.int32 if a.dtype == F32 else np.int64)


@pytest.fixture(scope='module')
def pair642():
    """Source sphere, target bumped ellipsoid (642 vertices each), the default-metric fit and the best similarity, computed once."""
    sv, sf = NC.sphere(3)
    tv, tf = NC.bumped_ellipsoid(3)
    fit = geometry.nonrigid_align((sv, sf), tv, tf, stiffness=(10.0, 1.0), iterations=3, search='tree')
    sim = geometry.align_mesh((sv, sf), tv, tf, scale=True, search='tree')
    return {'sv': sv, 'sf': sf, 'tv': tv, 'tf': tf, 'fit': fit, 'sim': sim}


@pytest.mark.parametrize('level', [1, 2])
@pytest.mark.parametrize('metric', ['point', 'plane'])
def test_solve_against_dense_solve(level, metric):
    """3V steps of conjugate gradients without a tolerance agree with np.linalg.solve of the matrix written out from the definition
    within 100 cond(A) eps64 max|x|, on the 42- and 162-vertex spheres with weights in {0, 1}, unit normals, pins and landmarks."""
    v, f = NC.sphere(level)
    adj = geometry.MeshAdjacency(v, f)
    s = NC.system(v, f, metric, 11 + level)
    A, b = NC.dense(adj, s)
    want = np.linalg.solve(A, b).reshape(-1, 3)
    got = NC.solve(adj, s, 3 * v.shape[0], 0.0)
    bound = 100 * np.linalg.cond(A) * NC.EPS64 * np.abs(want).max()
    err = np.abs(got['x'] - want).max()
    print(f'V={v.shape[0]} {metric}: |cg - dense| = {err:.3e}, bound {bound:.3e}, steps {got["cg_steps"]}')
    assert err <= bound
    assert got['energy_end'] <= got['energy_start']
    assert not got['x'][s['pinned']].any()


@pytest.mark.parametrize('stiffness', [0.5, 50.0])
def test_known_answer_constant_offset(stiffness):
    """All weights 1 and the same offset t everywhere: the solution is t (L t = 0), within the bound of the dense test."""
    v, f = NC.sphere(2)
    adj = geometry.MeshAdjacency(v, f)
    nv = v.shape[0]
    t = np.array([0.3, -1.25, 0.7])
    s = {'c': np.ones(nv), 't': np.tile(t, (nv, 1)), 'n': None, 'pinned': np.zeros(nv, dtype=bool), 'landmarks': None, 'stiffness': stiffness,
         'share': 0.1}
    A, _ = NC.dense(adj, s)
    got = geometry.nonrigid_solve(adj, s['c'], s['t'], stiffness, cg_iterations=3 * nv, cg_tol=0.0)
    bound = 100 * np.linalg.cond(A) * NC.EPS64 * np.abs(t).max()
    assert np.abs(got['x'] - t).max() <= bound
    assert got['energy_end'] <= got['energy_start']


def test_zero_case_returns_the_input_bits():
    v, f = NC.sphere(2)
    v = v.copy()
    v[3, 0] = -0.0
    r = geometry.nonrigid_align((v, f), v, f, stiffness=(1.0,), search='tree')
    assert np.array_equal(bits(r['verts']), bits(v))
    assert not r['displacement'].any() and r['rms'] == 0.0 and r['inliers'] == v.shape[0]
    assert r['levels'][0]['pairings'] == 1 and r['levels'][0]['cg_steps'] == []


@pytest.mark.parametrize('metric', ['point', 'plane'])
@pytest.mark.parametrize('steps', [1, 2, 7, 40])
def test_energy_never_rises(metric, steps):
    v, f = NC.sphere(2)
    adj = geometry.MeshAdjacency(v, f)
    s = NC.system(v, f, metric, 5, stiffness=3.0)
    got = NC.solve(adj, s, steps, 1e-12)
    assert got['energy_end'] <= got['energy_start']
    assert got['cg_steps'] == steps


@pytest.mark.parametrize('metric', ['point', 'plane'])
def test_freeze_rule(metric):
    """Once frozen the result does not change: the same bits for cg_iterations = k and k + 10, and the step is reported."""
    v, f = NC.sphere(2)
    adj = geometry.MeshAdjacency(v, f)
    s = NC.system(v, f, metric, 9)
    trace = []
    NC.restated(adj, s, 80, 0.0, trace=trace)
    tol, k = NC.safe_tolerance(trace)
    a, b = NC.solve(adj, s, k, tol), NC.solve(adj, s, k + 10, tol)
    assert a['cg_steps'] == b['cg_steps'] == k
    assert np.array_equal(bits(a['x']), bits(b['x']))
    assert NC.solve(adj, s, max(k - 1, 1), 0.0)['cg_steps'] == max(k - 1, 1)
    zero = geometry.nonrigid_solve(adj, np.zeros(v.shape[0]), s['t'], 1.0, cg_iterations=5)              # b = 0: frozen at once
    assert zero['cg_steps'] == 0 and not zero['x'].any()


def test_fit_beats_the_best_similarity(pair642):
    p = pair642
    fit, hist = p['fit'], p['fit']['rms_history']
    at = 0
    for lvl in fit['levels']:
        assert hist[at + lvl['pairings'] - 1] <= hist[at], (lvl, hist)
        assert len(lvl['cg_steps']) == len(lvl['cg_residual']) <= lvl['pairings']
        at += lvl['pairings']
    assert at + 1 == len(hist) and fit['rms'] == hist[-1]
    print(f'rms {hist[0]:.6g} -> {fit["rms"]:.6g}; similarity {p["sim"]["rms"]:.6g}; levels {fit["levels"]}')
    assert fit['rms'] < p['sim']['rms']
    before = geometry.surface_distance(p['sv'], p['sf'], p['tv'], p['tf'], search='tree')['mean_ab']
    after = geometry.surface_distance(fit['verts'], p['sf'], p['tv'], p['tf'], search='tree')['mean_ab']
    assert after < before
    assert fit['verts'].dtype == F32 and fit['displacement'].dtype == np.float64 and fit['inliers'] == 642
    moved = (p['sv'].astype(np.float64) + fit['displacement']).astype(F32)
    assert np.array_equal(bits(fit['verts']), bits(moved))


def test_plane_metric_fits_too(pair642):
    p = pair642
    fit = geometry.nonrigid_align((p['sv'], p['sf']), p['tv'], p['tf'], metric='plane', stiffness=(10.0, 1.0), iterations=2, search='tree')
    assert fit['rms'] < p['sim']['rms']


def test_stiff_schedule_moves_rigidly(pair642):
    """Stiffness 1e8 and one pairing: the displacement is a translation up to what the system itself allows.  The spread
    max_i |d_i - mean d| stays within 1e-6 max|d| of the spread of the dense solve of the same system."""
    p = pair642
    r = geometry.nonrigid_align((p['sv'], p['sf']), p['tv'], p['tf'], stiffness=(1e8,), iterations=1, search='tree')
    d = r['displacement']
    q = geometry._closest_tree_numpy(p['sv'], geometry.WindingTree(p['tv'], p['tf']))[2]
    s = {'c': np.ones(642), 't': q.astype(np.float64) - p['sv'].astype(np.float64), 'n': None, 'pinned': np.zeros(642, dtype=bool),
         'landmarks': None, 'stiffness': 1e8, 'share': 0.1}
    A, b = NC.dense(r['adjacency'], s)
    x = np.linalg.solve(A, b).reshape(-1, 3)

    def spread(u):
        return np.linalg.norm(u - u.mean(0), axis=1).max()
    largest = np.linalg.norm(d, axis=1).max()
    print(f'spread {spread(d):.6e}, dense {spread(x):.6e}, max|d| {largest:.6e}')
    assert largest > 0 and spread(d) <= spread(x) + 1e-6 * largest


def test_pins_and_landmarks(pair642):
    p = pair642
    sv, sf = p['sv'].copy(), p['sf']
    sv[17] = np.nan                                                       # pinned by itself
    fixed = np.zeros(642, dtype=bool)
    fixed[100:140] = True
    kw = dict(stiffness=(5.0,), iterations=2, search='tree')
    r = geometry.nonrigid_align((sv, sf), p['tv'], p['tf'], fixed=fixed, **kw)
    pinned = r['pinned']
    assert pinned[17] and pinned[100:140].all() and pinned.sum() == 41
    assert np.array_equal(bits(r['verts'][pinned]), bits(sv[pinned])) and not r['displacement'][pinned].any()
    assert (r['verts'][~pinned] != sv[~pinned]).any()
    idx = np.array([5, 300, 600])
    goal = p['sv'][idx].astype(np.float64) * 1.5
    gaps = []
    for w in (0.0, 1.0, 10.0, 100.0):
        m = geometry.nonrigid_align((p['sv'], sf), p['tv'], p['tf'], landmarks=(idx, goal, w), **kw)
        gaps.append(np.linalg.norm(m['verts'][idx].astype(np.float64) - goal, axis=1))
    gaps = np.array(gaps)
    assert (np.diff(gaps, axis=0) < 0).all(), gaps
    free = geometry.nonrigid_align((p['sv'], sf), p['tv'], p['tf'], **kw)
    zero = geometry.nonrigid_align((p['sv'], sf), p['tv'], p['tf'], landmarks=(idx, goal, 0.0), **kw)
    assert np.array_equal(bits(free['verts']), bits(zero['verts']))


def test_normal_cos_rejects_an_inward_target():
    sv, sf = NC.sphere(2)
    tv, tf = (sv * F32(1.3)).astype(F32), sf[:, ::-1].copy()              # larger, wound inwards
    kw = dict(stiffness=(2.0,), iterations=2, search='tree')
    held = geometry.nonrigid_align((sv, sf), tv, tf, normal_cos=0.0, **kw)
    assert held['inliers'] == 0 and not held['displacement'].any() and np.array_equal(bits(held['verts']), bits(sv))
    moved = geometry.nonrigid_align((sv, sf), tv, tf, **kw)
    assert moved['inliers'] == sv.shape[0] and np.abs(moved['displacement']).max() > 0.1
    outward = geometry.nonrigid_align((sv, sf), tv, sf, normal_cos=0.0, **kw)
    assert outward['inliers'] == sv.shape[0] and np.abs(outward['displacement']).max() > 0.1      # compatible normals all count


def test_source_without_faces_goes_to_the_closest_points():
    sv, _ = NC.sphere(1)
    tv, tf = NC.bumped_ellipsoid(2)
    r = geometry.nonrigid_align((sv, np.zeros((0, 3), dtype=np.int64)), tv, tf, stiffness=(1.0,), iterations=2, cg_tol=1e-12, search='tree')
    q = geometry._closest_tree_numpy(sv, geometry.WindingTree(tv, tf))[2]
    assert np.abs(r['verts'].astype(np.float64) - q).max() <= 4 * NC.EPS32 * np.abs(tv).max()


def test_torch_cpu_tensors_keep_their_container(pair642):
    p = pair642
    r = geometry.nonrigid_align((torch.from_numpy(p['sv']), torch.from_numpy(p['sf'])), torch.from_numpy(p['tv']), torch.from_numpy(p['tf']),
                                stiffness=(10.0, 1.0), iterations=3, search='tree')
    assert isinstance(r['verts'], torch.Tensor) and r['displacement'].dtype == torch.float64
    assert np.array_equal(bits(r['verts'].numpy()), bits(p['fit']['verts']))


def test_arguments():
    sv, sf = NC.sphere(1)
    tv, tf = NC.bumped_ellipsoid(1)
    ok = dict(stiffness=(1.0,), iterations=1, search='tree')
    empty_f, empty_v = np.zeros((0, 3), dtype=np.int64), np.zeros((0, 3), dtype=F32)
    bad = [dict(verts=tv, faces=empty_f), dict(verts=empty_v, faces=empty_f), dict(stiffness=()), dict(stiffness=(1.0, 0.0)),
           dict(stiffness=(-2.0,)), dict(cg_iterations=0), dict(metric='plane', point_share=0.0), dict(metric='plane', point_share=-1.0),
           dict(fixed=np.zeros(5, dtype=bool)), dict(landmarks=(np.array([1, 2]), np.zeros((3, 3)), 1.0)),
           dict(landmarks=(np.array([1, 2]), np.zeros((2, 3)), np.ones(3))), dict(landmarks=(np.array([1, 1]), np.zeros((2, 3)), 1.0)),
           dict(landmarks=(np.array([1, 99]), np.zeros((2, 3)), 1.0)), dict(adjacency=geometry.MeshAdjacency(*NC.sphere(2))),
           dict(metric='line'), dict(trim=0.0), dict(search='octree')]
    for case in bad:
        kw = {**ok, **case}
        target = (kw.pop('verts', tv), kw.pop('faces', tf))
        with pytest.raises(ValueError):
            geometry.nonrigid_align((sv, sf), *target, **kw)
    adj = geometry.MeshAdjacency(sv, sf)
    nv = sv.shape[0]
    for case in (dict(cg_iterations=0), dict(normals=np.ones((nv, 3)), point_share=0.0), dict(pinned=np.zeros(3, dtype=bool)),
                 dict(landmarks=(np.array([0, 0]), np.zeros((2, 3)), 1.0)), dict(x0=np.zeros((nv, 2)))):
        with pytest.raises(ValueError):
            geometry.nonrigid_solve(adj, np.ones(nv), np.zeros((nv, 3)), 1.0, **case)
    with pytest.raises(ValueError):
        geometry.nonrigid_solve(adj, np.ones(nv + 1), np.zeros((nv, 3)), 1.0)


def test_cli_fit_nonrigid(tmp_path):
    sv, sf = NC.sphere(2)
    tv, tf = NC.bumped_ellipsoid(2)
    pred, gt = str(tmp_path / 'pred.ply'), str(tmp_path / 'gt.ply')
    geometry.write_ply(pred, sv, sf)
    geometry.write_ply(gt, tv, tf)
    base = ['--pred', pred, '--gt', gt, '--device', 'cpu', '--search', 'tree']
    plain = geometry_metrics.main(base + ['--out', str(tmp_path / 'plain.json')])
    fitted_ply = str(tmp_path / 'fitted.ply')
    res = geometry_metrics.main(base + ['--out', str(tmp_path / 'fit.json'), '--fit-nonrigid', '--fit-stiffness', '10,1', '--fit-iterations', '2',
                                        '--save-fitted', fitted_ply])
    with open(tmp_path / 'plain.json') as fh:
        plain_json = json.load(fh)
    with open(tmp_path / 'fit.json') as fh:
        fit_json = json.load(fh)
    assert 'nonrigid' not in plain_json and set(plain_json) == set(plain) and set(fit_json) == set(plain_json) | {'nonrigid'}
    block = fit_json['nonrigid']
    assert block['rms_after'] < block['rms_before'] and block['inliers'] == sv.shape[0] and block['max_displacement'] > 0
    assert [lvl['stiffness'] for lvl in block['levels']] == [10.0, 1.0]
    assert res['mean_ab'] < plain['mean_ab']                              # the fitted mesh is the one that is scored
    fv, ff, _ = geometry.read_ply(fitted_ply)
    assert np.array_equal(ff, sf) and fv.shape == sv.shape and (fv != sv).any()
    with pytest.raises(SystemExit):
        geometry_metrics.main(base + ['--out', str(tmp_path / 'x.json'), '--save-fitted', fitted_ply])


def test_cli_fit_template(tmp_path):
    """extract_geometry --fit-template writes the template's faces on the avatar's shape; without the flag nothing changes."""
    from invertavatar_amd import extract_geometry
    sv, sf = NC.sphere(2)
    template = str(tmp_path / 'template.ply')
    geometry.write_ply(template, (sv * F32(0.3)).astype(F32), sf)
    base = ['--seeds', '0', '--width', 'small', '--res', '24', '--level', '0', '--device', 'cpu', '--search', 'tree']
    (plain, _), = extract_geometry.main(base + ['--outdir', str(tmp_path / 'plain')])
    (path, out), = extract_geometry.main(base + ['--outdir', str(tmp_path / 'fit'), '--fit-template', template, '--fit-align', 'similarity',
                                                 '--fit-stiffness', '10,1', '--fit-iterations', '2'])
    assert sorted(os.listdir(tmp_path / 'plain')) == ['seed0000.ply']
    assert sorted(os.listdir(tmp_path / 'fit')) == ['seed0000.ply', 'seed0000_geometry.json', 'seed0000_template.ply']
    with open(plain, 'rb') as a, open(path, 'rb') as b:
        assert a.read() == b.read()
    v, f, colors = geometry.read_ply(str(tmp_path / 'fit' / 'seed0000_template.ply'))
    assert np.array_equal(f, sf) and v.shape == sv.shape and colors is not None
    with open(tmp_path / 'fit' / 'seed0000_geometry.json') as fh:
        block = json.load(fh)['template']
    assert block['rms_after'] < block['rms_before'] and 'alignment' in block and len(block['levels']) == 2
    assert out['template']['fit']['rms'] == block['rms_after']
