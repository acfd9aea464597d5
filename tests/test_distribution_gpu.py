"""The kernels of csrc/distribution.hip against the float64 NumPy restatement of distribution_metrics.py.

  ia_feature_moments   products of float32 values are exact in double, so an entry is held to the reordering error of a float64 sum of
                       n terms, n eps64 sum|x_i x_j|; cov is symmetric bit for bit and two runs give the same bits.
  ia_kid_subsets       4 e32 + eps32 scale per sum (e32: the restatement's own float32-dot run against its float64 run on the same
                       inputs, never the kernel; scale: the sum of |k| over the block); a subset's row is the same bits alone and in a batch.
  ia_knn_radius /      features on a dyadic grid (multiples of 1/8, |x| <= 4): every squared distance is exact in fp32, so radii and
  ia_manifold_covered  coverage must EQUAL the restatement; one Gaussian case compares decisions outside the fp32 rounding margin.
  fid / kid / precision_recall on device tensors against the recorded reference values with the bounds of test_distribution_cpu.py, and
  DistributionMetrics end to end with the identity extractor."""
import ctypes

import numpy as np
import pytest
import torch

from invertavatar_amd import _lib, distribution_metrics as dm, hipops
from test_distribution_cpu import CASES, CHUNK, GOLD, MARGIN, case_features, fid_bound

pytestmark = pytest.mark.gpu

EPS32, EPS64 = float(np.finfo(np.float32).eps), float(np.finfo(np.float64).eps)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def bits(t):
    return t.contiguous().view(torch.int64 if t.dtype == torch.float64 else torch.int32)


# ------------------------------------------------------------------ ia_feature_moments

def moments(chunks, d):
    s = torch.zeros(d, dtype=torch.float64, device='cuda')
    c = torch.zeros(d, d, dtype=torch.float64, device='cuda')
    for x in chunks:
        hipops.feature_moments(dev(x), s, c)
    return s, c


@pytest.mark.parametrize('d', [1, 17, 48, 130])
def test_feature_moments_against_float64(d):
    rs = np.random.RandomState(100 + d)
    worst = 0.0
    for n in (0, 1, 3, 70):
        x = (rs.standard_normal((n, d)) * np.exp(rs.uniform(-3, 3, size=(1, d)))).astype(np.float32)     # asymmetric: columns of many scales
        y = rs.standard_normal((5, d)).astype(np.float32)
        for chunks in ([x], [x, y]):                                         # the second call accumulates onto the first
            s, c = moments(chunks, d)
            s2, c2 = moments(chunks, d)
            assert torch.equal(bits(s), bits(s2)) and torch.equal(bits(c), bits(c2))          # two runs, the same bits
            assert torch.equal(bits(c), bits(c.T.contiguous()))                               # exactly symmetric
            x64 = np.concatenate(chunks).astype(np.float64)
            rows = x64.shape[0]
            want_s, want_c = x64.sum(0), x64.T @ x64
            bound_s = rows * EPS64 * np.abs(x64).sum(0)
            bound_c = rows * EPS64 * (np.abs(x64).T @ np.abs(x64))
            err_s, err_c = np.abs(s.cpu().numpy() - want_s), np.abs(c.cpu().numpy() - want_c)
            assert (err_s <= bound_s).all() and (err_c <= bound_c).all(), (d, n, len(chunks))
            if rows:
                worst = max(worst, float((err_c / np.maximum(bound_c, 1e-300)).max()))
    print(f'D={d}: largest error / bound {worst:.3f}')


def test_feature_moments_refuses_bad_inputs():
    x = torch.zeros(4, 6, device='cuda')
    s, c = torch.zeros(6, dtype=torch.float64, device='cuda'), torch.zeros(6, 6, dtype=torch.float64, device='cuda')
    with pytest.raises(RuntimeError, match='contiguous float32'):
        hipops.feature_moments(torch.zeros(6, 4, device='cuda').T, s, c)
    with pytest.raises(RuntimeError, match='contiguous float32'):
        hipops.feature_moments(x.double(), s, c)
    with pytest.raises(RuntimeError, match='float64'):
        hipops.feature_moments(x, s.float(), c)
    with pytest.raises(RuntimeError, match='float64'):
        hipops.feature_moments(x, s, c[:, :5])
    with pytest.raises(ValueError, match='at most 4096'):
        hipops.feature_moments(torch.zeros(1, 4097, device='cuda'), s, c)
    lib = _lib.load()
    stream = _lib.stream_ptr(x.device)
    assert lib.ia_feature_moments(x.data_ptr(), 4, 0, s.data_ptr(), c.data_ptr(), stream) == -1 and 'D must be in' in _lib.last_error()
    assert lib.ia_feature_moments(x.data_ptr(), -1, 6, s.data_ptr(), c.data_ptr(), stream) == -1 and 'n must be' in _lib.last_error()
    host = (ctypes.c_double * 36)()
    assert lib.ia_feature_moments(x.data_ptr(), 4, 6, s.data_ptr(), ctypes.addressof(host), stream) == -1 and 'device pointers' in _lib.last_error()
    assert lib.ia_feature_moments(None, 0, 6, None, None, stream) == 0                         # n = 0: nothing is read
    torch.cuda.synchronize()
    assert not c.any() and not s.any()


# ------------------------------------------------------------------ ia_kid_subsets

def kid_bound(gen, real, ig, ir):
    """4 e32 + eps32 scale per sum, [S,3]: e32 and scale from the restatement alone."""
    f64 = dm.kid_sums_reference(gen, real, ig, ir)
    f32 = dm.kid_sums_reference(gen, real, ig, ir, dot_dtype=np.float32)
    scale = np.zeros_like(f64)
    n = float(gen.shape[1])
    for s in range(len(ig)):
        x, y = gen[ig[s]].astype(np.float64), real[ir[s]].astype(np.float64)
        for col, (a, b) in enumerate(((x, x), (y, y), (x, y))):
            scale[s, col] = (np.abs(a @ b.T / n + 1.0) ** 3).sum()
    return f64, MARGIN * np.abs(f32 - f64) + EPS32 * scale


@pytest.mark.parametrize('m', [2, 33, 65, 130])
def test_kid_subsets_against_float64(m):
    rs = np.random.RandomState(200 + m)
    worst = 0.0
    for d in (1, 7, 64, 130):
        gen = (rs.standard_normal((m + 9, d)) * 1.1 + 0.6).astype(np.float32)
        real = (rs.standard_normal((m + 4, d)) + 0.5).astype(np.float32)
        for s in (1, 5):
            ig = np.stack([rs.choice(m + 9, m, replace=False) for _ in range(s)])
            ir = np.stack([rs.choice(m + 4, m, replace=False) for _ in range(s)])
            if s == 5:
                ig[3], ir[3] = ig[0], ir[0]                                   # a subset repeated inside the batch
                ig[4, 1] = ig[4, 0]                                           # and a row repeated inside a subset
            got = hipops.kid_subsets(dev(gen), dev(real), ig, ir)
            want, bound = kid_bound(gen, real, ig, ir)
            err = np.abs(got.cpu().numpy() - want)
            assert (err <= bound).all(), (m, d, s, (err / bound).max())
            worst = max(worst, float((err / bound).max()))
            # a subset's three numbers are the same bits alone, elsewhere in the batch, and from run to run
            alone = hipops.kid_subsets(dev(gen), dev(real), ig[:1], ir[:1])
            assert torch.equal(bits(alone[0]), bits(got[0]))
            if s == 5:
                assert torch.equal(bits(got[3]), bits(got[0]))
                last = hipops.kid_subsets(dev(gen), dev(real), ig[4:], ir[4:])
                assert torch.equal(bits(last[0]), bits(got[4]))
            assert torch.equal(bits(hipops.kid_subsets(dev(gen), dev(real), ig, ir)), bits(got))
    print(f'm={m}: largest error / bound {worst:.3f}')


def test_kid_subsets_excludes_the_diagonal_by_position():
    # all rows equal: every k is (|x|^2 / D + 1)^3 = 8 exactly, so the sums count the terms: m (m - 1), m (m - 1), m^2
    for m in (2, 33, 129):
        x = np.ones((m, 4), np.float32)
        idx = np.arange(m)[None]
        got = hipops.kid_subsets(dev(x), dev(x), idx, idx).cpu().numpy()
        assert got.tolist() == [[8.0 * m * (m - 1), 8.0 * m * (m - 1), 8.0 * m * m]]
    with pytest.raises(ValueError, match='outside its set'):
        hipops.kid_subsets(dev(x), dev(x), idx + 1, idx)
    with pytest.raises(RuntimeError, match='host integer arrays'):
        hipops.kid_subsets(dev(x), dev(x), dev(idx), idx)
    with pytest.raises(RuntimeError, match='share D'):
        hipops.kid_subsets(dev(x), dev(x[:, :3]), idx, idx)


# ------------------------------------------------------------------ ia_knn_radius / ia_manifold_covered

def dyadic(rs, n, d):
    return (rs.randint(-32, 33, size=(n, d)) / 8.0).astype(np.float32)


@pytest.mark.parametrize('n,k', [(5, 3), (64, 3), (65, 1), (257, 15)])
def test_knn_radius_and_coverage_equal_the_restatement_on_a_dyadic_grid(n, k):
    rs = np.random.RandomState(300 + n)
    for d in (1, 3, 64, 130):
        manifold = dyadic(rs, n, d)
        manifold[n // 2] = manifold[0]                                       # exact duplicates
        manifold[n - 1] = manifold[0]
        r2 = hipops.knn_radius(dev(manifold), k)
        want_r2 = dm.knn_radius_reference(manifold, k)
        assert r2.dtype == torch.float32 and np.array_equal(r2.cpu().numpy().astype(np.float64), want_r2), (n, k, d)
        for p in (1, 130):
            probes = dyadic(rs, p, d)
            probes[0] = manifold[1]                                          # a probe that is a manifold point: covered at distance 0
            far = probes.copy()
            far[max(1, p // 2):] += 16.0                                     # and some far away (sums stay below 2^24 / 64: still exact)
            for pr in (probes, far):
                got = hipops.manifold_covered(dev(pr), dev(manifold), r2)
                want = dm.covered_reference(pr, manifold, want_r2)
                assert got.dtype == torch.bool and np.array_equal(got.cpu().numpy(), want), (n, k, d, p)
                assert bool(got[0])
    assert torch.equal(hipops.knn_radius(dev(manifold), k), r2)


def test_coverage_on_gaussian_features_outside_the_rounding_margin():
    rs = np.random.RandomState(7)
    n, p, d, k = 257, 130, 64, 3
    manifold, probes = rs.standard_normal((n, d)).astype(np.float32), (rs.standard_normal((p, d)) * 0.9).astype(np.float32)
    d2 = dm.sqdist64(manifold, manifold)
    want_r2 = np.partition(d2, k, axis=1)[:, k]
    r2 = hipops.knn_radius(dev(manifold), k)
    assert (np.abs(r2.cpu().numpy() - want_r2) <= d * EPS32 * want_r2).all()
    # decisions: compared with the float64 ones where some pair decides clearly, i.e. outside D eps32 (d2 + r2) of the radius
    pd2 = dm.sqdist64(probes, manifold)
    r2_64 = r2.cpu().numpy().astype(np.float64)                              # the radii the kernel is given
    margin = d * EPS32 * (pd2 + r2_64[None])
    surely_in = (pd2 <= r2_64[None] - margin).any(1)
    surely_out = (pd2 > r2_64[None] + margin).all(1)
    clear = surely_in | surely_out
    excluded = 1.0 - clear.mean()
    print(f'excluded share {excluded:.4f}')
    assert excluded < 0.01
    got = hipops.manifold_covered(dev(probes), dev(manifold), r2).cpu().numpy()
    assert np.array_equal(got[clear], surely_in[clear])
    assert 0.05 < got.mean() < 0.95                                          # the case decides both ways


def test_precision_recall_argument_checks():
    x = torch.zeros(8, 4, device='cuda')
    with pytest.raises(ValueError, match=r'k must be in \[0, 15\]'):
        hipops.knn_radius(x, 16)
    with pytest.raises(ValueError, match='no neighbour'):
        hipops.knn_radius(x[:3].contiguous(), 3)
    with pytest.raises(RuntimeError, match='contiguous float32'):
        hipops.knn_radius(x.half(), 3)
    with pytest.raises(RuntimeError, match='manifold_covered'):
        hipops.manifold_covered(x, x, torch.zeros(7, device='cuda'))
    lib, stream = _lib.load(), _lib.stream_ptr(x.device)
    r2 = torch.zeros(8, device='cuda')
    assert lib.ia_knn_radius(x.data_ptr(), 3, 4, 3, r2.data_ptr(), stream) == -1 and 'N must be in' in _lib.last_error()
    assert lib.ia_knn_radius(x.data_ptr(), 8, 0, 3, r2.data_ptr(), stream) == -1 and 'D must be' in _lib.last_error()
    host = (ctypes.c_float * 8)()
    assert lib.ia_knn_radius(x.data_ptr(), 8, 4, 3, ctypes.addressof(host), stream) == -1 and 'device pointers' in _lib.last_error()
    assert lib.ia_manifold_covered(x.data_ptr(), 8, x.data_ptr(), r2.data_ptr(), 0, 4, r2.data_ptr(), stream) == -1 and 'N in [1' in _lib.last_error()
    assert lib.ia_kid_subsets(x.data_ptr(), x.data_ptr(), 4, r2.data_ptr(), r2.data_ptr(), 1, 0, r2.data_ptr(), stream) == -1
    assert 'm in [1' in _lib.last_error()
    with pytest.raises(ValueError, match='nhood_size = 9'):
        dm.precision_recall(x, x, nhood_size=9)
    with pytest.raises(ValueError, match='both feature sets'):
        dm.precision_recall(x, x.cpu())


# ------------------------------------------------------------------ the public functions on device tensors, recorded reference values

@pytest.mark.parametrize('name', sorted(CASES))
def test_device_scores_against_the_reference(name):
    real, gen = case_features(*CASES[name])
    stats = []
    for x in (real, gen):
        s = dm.FeatureStats(capture_all=True, capture_mean_cov=True)
        for lo in range(0, x.shape[0], CHUNK):
            s.append_torch(dev(x[lo:lo + CHUNK]))
        assert s.raw_cov.is_cuda and s.raw_cov.dtype == torch.float64 and s.get_all_torch().is_cuda
        assert np.array_equal(s.get_all(), x)
        stats.append(s)
    want, e_ref = float(GOLD[f'{name}_fid']), float(GOLD['e_ref_fid'])
    got = dm.fid(*stats)
    print(f'{name}: fid {got!r} reference {want!r} |d| {abs(got - want):.3e} bound {fid_bound(want, e_ref):.3e}')
    assert abs(got - want) <= fid_bound(want, e_ref)
    assert abs(dm.fid(stats[0], stats[0])) <= fid_bound(0.0, e_ref)
    ig, ir = GOLD[f'{name}_kid_idx_gen'], GOLD[f'{name}_kid_idx_real']
    res = dm.kid(dev(real), dev(gen), subsets=(ig, ir))
    want, e_ref = float(GOLD[f'{name}_kid']), float(GOLD['e_ref_kid'])
    print(f"{name}: kid {res['kid']!r} reference {want!r} |d| {abs(res['kid'] - want):.3e} bound {MARGIN * e_ref:.3e}")
    assert res['per_subset'].is_cuda and abs(res['kid'] - want) <= MARGIN * e_ref
    pr = dm.precision_recall(dev(real), dev(gen), nhood_size=3, feature_dtype='float16')
    (p_ref, r_ref), flips = GOLD[f'{name}_pr'], GOLD[f'{name}_pr_flips']
    for got, ref, probes, allowed in ((pr['precision'], p_ref, gen.shape[0], flips[0]), (pr['recall'], r_ref, real.shape[0], flips[1])):
        differ = round(abs(got - ref) * probes)
        print(f'{name}: {got!r} reference {ref!r}: {differ} probes differ, recorded {allowed}')
        assert abs(abs(got - ref) * probes - differ) <= 1e-3 and differ <= allowed and allowed <= 0.01 * probes


# ------------------------------------------------------------------ end to end

def unclear(probes, manifold, k):
    """Probes whose decision lies within 2 D eps32 (d2 + r2) of some radius (the rounding of a distance and of a radius), float64."""
    r2 = dm.knn_radius_reference(manifold, k)
    d2 = dm.sqdist64(probes, manifold)
    margin = 2 * probes.shape[1] * EPS32 * (d2 + r2[None])
    return int((~((d2 <= r2[None] - margin).any(1) | (d2 > r2[None] + margin).all(1))).sum())


def test_distribution_metrics_end_to_end_with_the_identity_extractor():
    from invertavatar_amd import identity
    model = identity.IDScore.synthetic(0)
    g = torch.Generator().manual_seed(5)
    real = [(torch.rand(8, 3, 256, 256, generator=g) * 2 - 1).cuda() for _ in range(2)]
    gen = [(r * 0.8 + 0.1 * torch.rand(8, 3, 256, 256, generator=g).cuda()).contiguous() for r in real]
    coll = dm.DistributionMetrics(extractor=model, kid_subsets=4, kid_subset_size=12, seed=1)
    coll.update(real=real[0], gen=gen[0])                                    # (the first call uploads the weights)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')                                  # a host synchronisation inside update raises
    try:
        coll.update(real=real[1], gen=gen[1])
    finally:
        torch.cuda.set_sync_debug_mode('default')
    s = coll.summary()
    assert (s['num_real'], s['num_gen'], s['num_features'], s['kid_subset_size']) == (16, 16, 512, 12)
    fr, fg = coll.real.get_all(), coll.gen.get_all()
    assert np.array_equal(fr[:8], identity.embed(real[0], model).cpu().numpy())
    host = dm.DistributionMetrics(kid_subsets=4, kid_subset_size=12, seed=1)
    host.update(real=fr[:8], gen=fg[:8])
    host.update(real=fr[8:], gen=fg[8:])
    h = host.summary()
    # moments: the reordering bound of ia_feature_moments
    x64 = fr.astype(np.float64)
    assert (np.abs(coll.real.raw_cov.cpu().numpy() - host.real.raw_cov) <= 16 * EPS64 * (np.abs(x64).T @ np.abs(x64))).all()
    # fid: 16 rows in 512 dimensions leave both covariances singular.  An eigenvalue that is 0 is computed to about eps64 |M| and its
    # square root to sqrt(eps64 |M|), with |M| = |H Sb H| <= tr(Sa) tr(Sb); D of them bound the difference of two evaluations.
    (_, ca), (_, cb) = host.real.get_mean_cov(), host.gen.get_mean_cov()
    bound = 512 * np.sqrt(EPS64 * np.trace(ca) * np.trace(cb)) + 1e-9 * abs(h['fid'])
    print(f"fid {s['fid']!r} host {h['fid']!r} |d| {abs(s['fid'] - h['fid']):.3e} bound {bound:.3e}")
    assert abs(s['fid'] - h['fid']) <= bound
    ig, ir = dm.kid_subset_indices(16, 16, 4, 12, 1)
    want, kb = kid_bound(fg, fr, ig, ir)
    per_bound = (kb[:, 0] + kb[:, 1]) / 11 + 2 * kb[:, 2] / 12
    assert abs(s['kid'] - h['kid']) <= per_bound.sum() / 4 / 12
    # precision / recall: decisions may differ only for probes inside the fp32 rounding margin of the distances and of the radii
    r16, g16 = fr.astype(np.float16).astype(np.float32), fg.astype(np.float16).astype(np.float32)
    assert abs(s['precision'] - h['precision']) * 16 <= unclear(g16, r16, 3) + 1e-6
    assert abs(s['recall'] - h['recall']) * 16 <= unclear(r16, g16, 3) + 1e-6
