"""The device path of the non-rigid fit (csrc/nonrigid.hip) against its definition, the NumPy restatement in geometry.py."""
import os
import sys

import numpy as np
import pytest
import torch

from invertavatar_amd import extract_geometry, geometry, hipops

sys.path.insert(0, os.path.dirname(__file__))
import nonrigid_cases as NC  # noqa: E402

pytestmark = pytest.mark.gpu
F32 = np.float32
DEV = 'cuda'
SOLVER_MESHES = ['v1', 'v2', 'strip63', 'strip64', 'strip65', 'strip257', 'sphere642', 'fan', 'isolated', 'nonfinite']
SCHEDULE = dict(stiffness=(10.0, 1.0), iterations=2)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int64)


def device_solve(adj, s, cg_iterations, cg_tol):
    return geometry.nonrigid_solve(adj, dev(s['c']), dev(s['t']), s['stiffness'], normals=None if s['n'] is None else dev(s['n']),
                                   point_share=s['share'], pinned=dev(s['pinned']), x0=dev(s['x0']), landmarks=s['landmarks'],
                                   cg_iterations=cg_iterations, cg_tol=cg_tol)


@pytest.mark.parametrize('metric', ['point', 'plane'])
@pytest.mark.parametrize('name', SOLVER_MESHES)
def test_solver_against_the_restatement(name, metric):
    """hipops.nonrigid_solve within 4 e_ord + eps64 max|x| of the restatement, e_ord the restatement's own deviation with its neighbour
    sums and dot products in the reverse order; the same number of steps.  Two runs per case.  (a) 60 steps without a tolerance on a
    well-conditioned system (stiffness 1, point_share 0.5): every order has converged, so e_ord is the rounding of the result and not
    where an unfinished iteration happens to stand.  (b) The system of the dense test (stiffness 0.05, point_share 0.1) with a
    tolerance at which the restatement freezes within its first five steps with a margin of 4 in |r|^2 / |b|^2 on both sides (another
    seed if there is no such step).  A late freeze on an ill-conditioned system is left out on purpose: there the restatement's own
    orders differ by more than 4 e_ord from each other (a third order, pairwise sums, missed the bound on the host), so the yardstick
    measures nothing."""
    v, f = NC.mesh(name)
    host = geometry.MeshAdjacency(v, f)
    adj = geometry.MeshAdjacency(dev(v), dev(f))
    assert (adj.info['max_degree'] > 64) == (name == 'fan')
    for seed in range(7, 40):
        s = NC.system(v, f, metric, seed)
        trace = []
        NC.restated(host, s, 8, 0.0, trace=trace)
        safe = NC.early_tolerance(trace)
        if safe is not None:
            break
    else:
        pytest.fail('no seed gives a freeze step with a margin of 4 on both sides')
    tol, k = safe
    assert min(trace[:k]) >= 4 * tol ** 2 and trace[k] <= tol ** 2 / 4
    mild = NC.system(v, f, metric, seed, stiffness=1.0, share=0.5)
    for s, steps, cg_tol, expect in ((mild, 60, 0.0, None), (s, k + 6, tol, k)):
        want, n_want = NC.restated(host, s, steps, cg_tol)
        e_ord = float(np.abs(NC.restated(host, s, steps, cg_tol, reverse=True)[0] - want).max())
        got = device_solve(adj, s, steps, cg_tol)
        err = float(np.abs(got['x'].cpu().numpy() - want).max())
        bound = 4 * e_ord + NC.EPS64 * float(np.abs(want).max())
        print(f'{name} {metric} seed {seed} steps {steps} tol {cg_tol:.3g}: device {err:.3e}, e_ord {e_ord:.3e}, ratio '
              f'{err / e_ord if e_ord else float("nan"):.3g}, bound {bound:.3e}, cg_steps {got["cg_steps"]} / {n_want}')
        assert got['cg_steps'] == n_want and (expect is None or n_want == expect)
        assert err <= bound
        assert got['energy_end'] <= got['energy_start']
        assert not bool(got['x'][dev(s['pinned'])].any())


def test_bit_repeatability():
    v, f = NC.sphere(3)
    adj = geometry.MeshAdjacency(dev(v), dev(f))
    s = NC.system(v, f, 'plane', 3)
    a, b = device_solve(adj, s, 40, 1e-9), device_solve(adj, s, 40, 1e-9)
    assert torch.equal(bits(a['x']), bits(b['x'])) and a['cg_steps'] == b['cg_steps'] and a['energy_end'] == b['energy_end']
    tv, tf = NC.bumped_ellipsoid(3)
    runs = [geometry.nonrigid_align((dev(v), dev(f)), dev(tv), dev(tf), metric='plane', **SCHEDULE) for _ in range(2)]
    assert torch.equal(bits(runs[0]['verts']), bits(runs[1]['verts'])) and torch.equal(bits(runs[0]['displacement']), bits(runs[1]['displacement']))
    assert runs[0]['rms_history'] == runs[1]['rms_history'] and runs[0]['levels'] == runs[1]['levels']


def terms_inputs():
    """One pairing's inputs on the host: x, p (moved off the sphere), the closest points of a target with one face without area."""
    x, sf = NC.sphere(3)
    tv, tf = NC.bumped_ellipsoid(3)
    tf = tf.copy()
    tf[40] = [tf[40, 0], tf[40, 0], tf[40, 1]]                             # a face without a normal
    rng = np.random.RandomState(2)
    p = (x + 0.02 * rng.randn(*x.shape)).astype(F32)
    dist, face, q = geometry._closest_tree_numpy(p, geometry.WindingTree(tv, tf))[:3]
    dist, face, q = np.round(dist.astype(F32), 2), face.astype(np.int32), q.astype(F32)      # rounded: many tied distances
    face[:12] = 40                                                        # pairs on the face without area
    dist[20], face[21], dist[22] = np.inf, -1, np.nan
    pinned = np.zeros(x.shape[0], dtype=bool)
    pinned[[3, 50, 333]] = True
    adj = geometry.MeshAdjacency(p, sf)
    return {'x': x, 'p': p, 'q': q, 'dist': dist, 'face': face, 'pinned': pinned, 'fnormals': geometry.face_normals(tv, tf).astype(F32),
            'snormals': geometry._mesh_normals_numpy(p, adj.faces, adj._state, 'area'), 'extent': float(np.abs(tv).max())}


@pytest.mark.parametrize('case', ['max_dist', 'trim', 'normal_cos', 'plane', 'landmarks'])
def test_terms_against_the_restatement(case):
    t = terms_inputs()
    nv = t['x'].shape[0]
    thr, metric, cos, beta, land = np.inf, 'point', None, None, None
    if case == 'max_dist':
        thr = float(np.median(t['dist'][np.isfinite(t['dist'])]))
    if case == 'trim':
        thr = geometry._trim_threshold_numpy(t['dist'], t['face'], None, 0.7)
        assert np.count_nonzero(t['dist'] == F32(thr)) > 1                 # the threshold falls on tied distances: they stay in
    if case == 'normal_cos':
        cos = 0.995
    if case in ('plane', 'landmarks'):
        metric = 'plane'
    if case == 'landmarks':
        rng = np.random.RandomState(5)
        beta, land = np.zeros(nv), np.zeros((nv, 3))
        at = np.array([3, 7, 100, 640])                                   # vertex 3 is pinned
        beta[at], land[at] = [2.0, 0.5, 1.0, 4.0], rng.randn(4, 3)
    c, n, b, sq, cnt = geometry._nonrigid_terms_numpy(t['x'], t['p'], t['q'], t['dist'], t['face'], t['pinned'], thr, metric, t['fnormals'],
                                                      t['snormals'], cos, 0.1, beta, land)
    gc, gn, gb, stats = hipops.nonrigid_terms(dev(t['x']), dev(t['p']), dev(t['q']), dev(t['dist']), dev(t['face']), dev(t['pinned']), thr, metric,
                                              dev(t['fnormals']), dev(t['snormals']) if cos is not None else None, cos, 0.1,
                                              None if beta is None else dev(beta), None if land is None else dev(land))
    gsq, gcnt = stats.cpu().tolist()
    assert 0 < cnt < nv - 5 and np.array_equal(gc.cpu().numpy(), c) and int(gcnt) == cnt
    if metric == 'plane':
        assert np.array_equal(gn.cpu().numpy(), n) and not c[:12].any()
    else:
        assert not bool(gn.any())
    err = float(np.abs(gb.cpu().numpy() - b).max())
    print(f'{case}: {cnt} of {nv} pairs count, |b - b_ref| = {err:.3e}, sum {gsq!r} against {sq!r}')
    assert err <= NC.EPS32 * t['extent']
    assert abs(gsq - sq) <= nv * NC.EPS64 * sq
    if case == 'landmarks':
        assert not gb.cpu().numpy()[3].any() and gb.cpu().numpy()[640].any()


@pytest.fixture(scope='module')
def restatement():
    """The float64 restatement of the end-to-end fit and its own float32-search run, per metric, computed once."""
    sv, sf = NC.sphere(3)
    tv, tf = NC.bumped_ellipsoid(3)
    adj = geometry.MeshAdjacency(sv, sf)
    pinned = np.zeros(sv.shape[0], dtype=bool)
    out = {}
    for metric in ('point', 'plane'):
        runs = []
        for dtype in (np.float64, np.float32):
            d, hist, levels, n = geometry._nonrigid_numpy(sv, adj, tv, tf, pinned, metric, [10.0, 1.0], 2, 1e-4, 100, 1e-6, 0.1, None, 1.0, None,
                                                          None, None, 'tree', dtype)
            runs.append((geometry._moved_numpy(sv, d, pinned).astype(np.float64), hist, levels))
        out[metric] = runs
    return out


@pytest.mark.parametrize('metric', ['point', 'plane'])
def test_end_to_end_against_the_restatement(metric, restatement, monkeypatch):
    """verts within 4 e32 + eps32 extent of the float64 restatement (e32: its own float32-search run); the tree gives the grid's bits;
    no library solver is called."""
    def no_library(*a, **k):
        raise AssertionError('the non-rigid fit called a library solver')
    for name in ('solve', 'lstsq', 'cholesky', 'cholesky_ex', 'lu_factor', 'inv', 'pinv'):
        monkeypatch.setattr(torch.linalg, name, no_library)
    for name in ('mm', 'addmm', 'spsolve') if hasattr(torch.sparse, 'spsolve') else ('mm', 'addmm'):
        monkeypatch.setattr(torch.sparse, name, no_library)
    for name in ('sparse_coo_tensor', 'sparse_csr_tensor'):
        monkeypatch.setattr(torch, name, no_library)
    for name in ('to_sparse', 'to_sparse_csr'):
        monkeypatch.setattr(torch.Tensor, name, no_library)
    monkeypatch.setattr(np.linalg, 'solve', no_library)
    monkeypatch.setattr(np.linalg, 'lstsq', no_library)
    sv, sf = NC.sphere(3)
    tv, tf = NC.bumped_ellipsoid(3)
    (want, hist, levels), (want32, _, _) = restatement[metric]
    e32 = float(np.abs(want - want32).max())
    extent = float(np.abs(tv).max())
    grid = geometry.nonrigid_align((dev(sv), dev(sf)), dev(tv), dev(tf), metric=metric, **SCHEDULE)
    tree = geometry.nonrigid_align((dev(sv), dev(sf)), dev(tv), dev(tf), metric=metric, search='tree', **SCHEDULE)
    err = float(np.abs(grid['verts'].cpu().numpy().astype(np.float64) - want).max())
    print(f'{metric}: |device - restatement| = {err:.3e}, e32 {e32:.3e}, bound {4 * e32 + NC.EPS32 * extent:.3e}; rms {grid["rms_history"]}; '
          f'levels {grid["levels"]}')
    assert err <= 4 * e32 + NC.EPS32 * extent
    assert torch.equal(bits(grid['verts']), bits(tree['verts'])) and grid['rms_history'] == tree['rms_history']
    assert len(grid['rms_history']) == len(hist) and [lvl['pairings'] for lvl in grid['levels']] == [lvl['pairings'] for lvl in levels]
    assert grid['rms'] < grid['rms_history'][0] and grid['inliers'] == sv.shape[0]
    assert grid['verts'].is_cuda and grid['displacement'].dtype == torch.float64 and not bool(grid['pinned'].any())


@pytest.mark.parametrize('trim', [1.0, 0.8])
def test_one_host_synchronisation_per_pairing(trim, monkeypatch):
    """With the adjacency and the grid built beforehand, the fit reads the device once per pairing (the rms), once more for tau when
    trimming, and never inside a solve."""
    sv, sf = NC.sphere(3)
    tv, tf = NC.bumped_ellipsoid(3)
    source, target = (dev(sv), dev(sf)), (dev(tv), dev(tf))
    adj, grid = geometry.MeshAdjacency(*source), geometry.TriangleGrid(*target)
    geometry.nonrigid_align(source, *target, adjacency=adj, grid=grid, trim=trim, **SCHEDULE)             # (everything is loaded and built)
    reads = []

    def counted(owner, name):
        orig = getattr(owner, name)

        def wrap(*a, **k):
            if owner is not torch.Tensor or a[0].is_cuda:
                reads.append(name)
            return orig(*a, **k)
        monkeypatch.setattr(owner, name, wrap)
    for name in ('cpu', 'item', 'tolist', 'numpy', '__float__', '__int__', '__bool__'):
        counted(torch.Tensor, name)
    counted(torch.cuda, 'synchronize')
    r = geometry.nonrigid_align(source, *target, adjacency=adj, grid=grid, trim=trim, **SCHEDULE)
    monkeypatch.undo()
    pairings = len(r['rms_history'])
    assert sum(len(lvl['cg_steps']) for lvl in r['levels']) >= 2
    assert len(reads) == pairings * (2 if trim < 1.0 else 1), reads
    if trim < 1.0:
        assert r['inliers'] < sv.shape[0]


def test_cli_fit_template(tmp_path):
    sv, sf = NC.sphere(3)
    template = str(tmp_path / 'template.ply')
    geometry.write_ply(template, (sv * F32(0.3)).astype(F32), sf)
    base = ['--seeds', '0', '--width', 'small', '--level', '0', '--res', '64', '--device', DEV]
    (plain, _), = extract_geometry.main(base + ['--outdir', str(tmp_path / 'plain')])
    (path, out), = extract_geometry.main(base + ['--outdir', str(tmp_path / 'fit'), '--fit-template', template, '--fit-align', 'similarity',
                                                 '--fit-stiffness', '10,1', '--fit-iterations', '2'])
    assert sorted(os.listdir(tmp_path / 'plain')) == ['seed0000.ply']
    assert sorted(os.listdir(tmp_path / 'fit')) == ['seed0000.ply', 'seed0000_geometry.json', 'seed0000_template.ply']
    with open(plain, 'rb') as a, open(path, 'rb') as b:
        assert a.read() == b.read()
    v, f, colors = geometry.read_ply(str(tmp_path / 'fit' / 'seed0000_template.ply'))
    assert np.array_equal(f, sf) and v.shape == sv.shape and colors is not None and colors.shape == sv.shape
    fit = out['template']['fit']
    assert fit['rms'] < fit['rms_history'][0] and np.array_equal(out['template']['verts'].cpu().numpy(), v)
