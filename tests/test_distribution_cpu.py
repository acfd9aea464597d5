"""distribution_metrics on the host: the NumPy restatement (the definition) against the recorded results of the reference's metrics/
package (tests/golden/distribution.npz, written by tests/golden/make_distribution_golden.py) and against brute force written here."""
import json
import os
import sys

import numpy as np
import pytest
import torch

from invertavatar_amd import distribution_metrics as dm

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, 'golden'))
from make_distribution_golden import CASES, CHUNK, KID_SUBSET_SIZE, KID_SUBSETS, RANK_CASE, case_features  # noqa: E402

GOLD = np.load(os.path.join(HERE, 'golden', 'distribution.npz'))
MARGIN = 4.0                                     # the project's usual factor over the reference's own error


def stats_of(x, chunk=CHUNK, **kwargs):
    s = dm.FeatureStats(**kwargs)
    for lo in range(0, x.shape[0], chunk):
        s.append(x[lo:lo + chunk])
    return s


def both_stats(name):
    real, gen = case_features(*CASES[name])
    return stats_of(real, capture_mean_cov=True), stats_of(gen, capture_mean_cov=True)


# ------------------------------------------------------------------ FeatureStats

@pytest.mark.parametrize('name', sorted(CASES))
def test_feature_stats_match_the_reference_bits(name):
    """The same chunking gives the reference's float64 arrays bit for bit (the same x64.sum(0) and x64.T @ x64, in the same order)."""
    sr, sg = both_stats(name)
    for s, tag in ((sr, 'real'), (sg, 'gen')):
        mean, cov = s.get_mean_cov()
        assert mean.dtype == cov.dtype == np.float64
        assert np.array_equal(mean, GOLD[f'{name}_mean_{tag}']) and np.array_equal(cov, GOLD[f'{name}_cov_{tag}'])
        mt, ct = s.get_mean_cov_torch()
        assert np.array_equal(mt.numpy(), mean) and np.array_equal(ct.numpy(), cov)


def test_feature_stats_other_chunking_within_float64_rounding():
    real, _ = case_features(*CASES['a'])
    x64 = real.astype(np.float64)
    mean, cov = stats_of(real, chunk=41, capture_mean_cov=True).get_mean_cov()
    n = real.shape[0]
    bound_mean = n * np.finfo(np.float64).eps * np.abs(x64).sum(0) / n
    bound_cov = n * np.finfo(np.float64).eps * (np.abs(x64).T @ np.abs(x64)) / n + 4 * np.finfo(np.float64).eps * np.abs(np.outer(mean, mean))
    assert (np.abs(mean - GOLD['a_mean_real']) <= bound_mean).all()
    assert (np.abs(cov - GOLD['a_cov_real']) <= bound_cov).all()


def test_feature_stats_max_items_capture_all_and_inputs():
    real, _ = case_features(*CASES['b'])
    s = dm.FeatureStats(capture_all=True, capture_mean_cov=True, max_items=150)
    assert not s.is_full() and s.num_items == 0 and s.num_features is None
    for lo in range(0, real.shape[0], 64):
        chunk = real[lo:lo + 64]
        s.append_torch(torch.from_numpy(chunk)) if (lo // 64) % 2 else s.append(chunk)
    assert s.is_full() and s.num_items == 150 and s.num_features == real.shape[1]
    assert np.array_equal(s.get_all(), real[:150]) and s.get_all().dtype == np.float32           # truncated, in call order
    assert torch.equal(s.get_all_torch(), torch.from_numpy(real[:150]))
    want = dm.FeatureStats(capture_mean_cov=True)
    for lo, hi in ((0, 64), (64, 128), (128, 150)):
        want.append(real[lo:hi])
    assert np.array_equal(s.raw_cov, want.raw_cov) and np.array_equal(s.raw_mean, want.raw_mean)
    s.append(real[:5])                                                                         # full: ignored
    assert s.num_items == 150
    with pytest.raises(ValueError, match='columns'):
        stats_of(real, capture_all=True).append(real[:, :3])
    with pytest.raises(ValueError, match=r'\[N, D\]'):
        dm.FeatureStats().append(real[0])
    with pytest.raises(ValueError, match='capture_all=False'):
        stats_of(real, capture_mean_cov=True).get_all()
    with pytest.raises(ValueError, match='capture_mean_cov=False'):
        stats_of(real, capture_all=True).get_mean_cov()
    with pytest.raises(ValueError, match='num_gpus'):
        dm.FeatureStats().append_torch(torch.zeros(2, 2), num_gpus=2)


def test_feature_stats_save_load_round_trip(tmp_path):
    real, _ = case_features(*CASES['b'])
    s = stats_of(real, capture_all=True, capture_mean_cov=True, max_items=280)
    path = str(tmp_path / 'stats.npz')
    s.save(path)
    with np.load(path, allow_pickle=False) as z:                                                # arrays only: no pickle inside
        assert set(z.files) >= {'raw_mean', 'raw_cov', 'all_features', 'num_items'}
    t = dm.FeatureStats.load(path)
    assert (t.capture_all, t.capture_mean_cov, t.max_items, t.num_items, t.num_features) == (True, True, 280, 280, real.shape[1])
    assert np.array_equal(t.get_all(), s.get_all())
    assert all(np.array_equal(a, b) for a, b in zip(t.get_mean_cov(), s.get_mean_cov()))
    empty = str(tmp_path / 'empty.npz')
    dm.FeatureStats(capture_mean_cov=True).save(empty)
    assert dm.FeatureStats.load(empty).num_items == 0


# ------------------------------------------------------------------ FID

def fid_bound(value, e_ref):
    return MARGIN * e_ref + 1e-9 * abs(value)


@pytest.mark.parametrize('name', sorted(CASES))
def test_fid_against_the_reference(name):
    sr, sg = both_stats(name)
    want, e_ref = float(GOLD[f'{name}_fid']), float(GOLD['e_ref_fid'])
    got = dm.fid(sr, sg)
    print(f'{name}: fid {got!r} reference {want!r} |d| {abs(got - want):.3e} bound {fid_bound(want, e_ref):.3e}')
    assert abs(got - want) <= fid_bound(want, e_ref)
    assert abs(dm.fid(sg, sr) - got) <= fid_bound(want, e_ref)                                  # symmetric in its arguments
    assert abs(dm.fid(sr, sr)) <= fid_bound(0.0, e_ref) and abs(dm.fid(sg, sg)) <= fid_bound(0.0, e_ref)
    mu, cov = sr.get_mean_cov()
    assert dm.frechet_distance(torch.from_numpy(mu), torch.from_numpy(cov), *sg.get_mean_cov()) == dm.frechet_distance(mu, cov, *sg.get_mean_cov())


def test_fid_rank_deficient_case():
    real, gen = case_features(*RANK_CASE)
    got = dm.fid(stats_of(real, capture_mean_cov=True), stats_of(gen, capture_mean_cov=True))
    want, e_ref = float(GOLD['rank_fid']), float(GOLD['rank_e_ref'])
    print(f'rank-deficient: fid {got!r} reference {want!r} |d| {abs(got - want):.3e} bound {fid_bound(want, e_ref):.3e}')
    assert abs(got - want) <= fid_bound(want, e_ref)


def test_frechet_distance_closed_form_and_checks():
    # commuting covariances: tr sqrt(Sa Sb) = sum sqrt(a_i b_i)
    a, b = np.array([4.0, 1.0, 0.0]), np.array([9.0, 16.0, 2.0])
    want = 3.0 + a.sum() + b.sum() - 2.0 * np.sqrt(a * b).sum()
    assert abs(dm.frechet_distance(np.ones(3), np.diag(a), np.zeros(3), np.diag(b)) - want) <= 1e-13
    with pytest.raises(ValueError, match='means'):
        dm.frechet_distance(np.ones(3), np.eye(2), np.ones(3), np.eye(3))


# ------------------------------------------------------------------ KID

@pytest.mark.parametrize('name', sorted(CASES))
def test_kid_explicit_subsets_against_the_reference(name):
    real, gen = case_features(*CASES[name])
    ig, ir = GOLD[f'{name}_kid_idx_gen'], GOLD[f'{name}_kid_idx_real']
    res = dm.kid(real, gen, subsets=(ig, ir))
    want, e_ref = float(GOLD[f'{name}_kid']), float(GOLD['e_ref_kid'])
    print(f"{name}: kid {res['kid']!r} reference {want!r} |d| {abs(res['kid'] - want):.3e} bound {MARGIN * e_ref:.3e}")
    assert abs(res['kid'] - want) <= MARGIN * e_ref
    assert res['m'] == min(real.shape[0], gen.shape[0], KID_SUBSET_SIZE) and res['per_subset'].shape == (KID_SUBSETS,)
    assert res['per_subset'].dtype == np.float64
    # the float64 restatement is the definition: brute force over one subset
    x, y = gen[ig[0]].astype(np.float64), real[ir[0]].astype(np.float64)
    n, m = real.shape[1], res['m']
    kxx, kyy, kxy = (x @ x.T / n + 1) ** 3, (y @ y.T / n + 1) ** 3, (x @ y.T / n + 1) ** 3
    brute = (kxx.sum() - np.trace(kxx) + kyy.sum() - np.trace(kyy)) / (m - 1) - 2 * kxy.sum() / m
    assert abs(res['per_subset'][0] - brute) <= 1e-12 * abs(kxy.sum())
    assert res['kid'] == float(res['per_subset'].sum() / KID_SUBSETS / m)


def test_kid_seeded_subsets_and_clamping():
    real, gen = case_features(*CASES['b'])
    a, b = dm.kid(real, gen, num_subsets=4, max_subset_size=1000, seed=3), dm.kid(real, gen, num_subsets=4, max_subset_size=1000, seed=3)
    assert a['kid'] == b['kid'] and np.array_equal(a['per_subset'], b['per_subset'])
    assert a['m'] == 257                                                                       # min(300, 257, 1000), as the reference clamps
    assert dm.kid(real, gen, num_subsets=4, max_subset_size=50, seed=3)['m'] == 50
    assert dm.kid(real, gen, num_subsets=4, seed=4)['kid'] != a['kid']
    ig, ir = dm.kid_subset_indices(300, 257, 4, 1000, seed=3)
    assert ig.shape == ir.shape == (4, 257) and all(len(set(r)) == 257 for r in ig) and ir.max() < 300 and ig.max() < 257
    assert dm.kid(real, gen, subsets=(ig, ir))['kid'] == a['kid']
    assert dm.kid(torch.from_numpy(real), torch.from_numpy(gen), subsets=(torch.from_numpy(ig), ir))['kid'] == a['kid']
    with pytest.raises(ValueError, match='outside'):
        dm.kid(real, gen, subsets=(ig + 1, ir))
    with pytest.raises(ValueError, match='at least two'):
        dm.kid(real[:1], gen)
    with pytest.raises(ValueError, match='features'):
        dm.kid(real[:, :5], gen)
    with pytest.raises(ValueError, match='integer arrays'):
        dm.kid(real, gen, subsets=(ig.astype(np.float32), ir))


# ------------------------------------------------------------------ precision / recall

def brute_pr(manifold, probes, k):
    """Kynkaanniemi's estimator from its definition, float64, one pair at a time."""
    m64, p64 = manifold.astype(np.float64), probes.astype(np.float64)
    radii = np.array([np.sort(((m64 - row) ** 2).sum(1))[k] for row in m64])
    return np.array([(((m64 - row) ** 2).sum(1) <= radii).any() for row in p64]), radii


@pytest.mark.parametrize('name', sorted(CASES))
def test_precision_recall_against_the_reference(name):
    real, gen = case_features(*CASES[name])
    res = dm.precision_recall(real, gen, nhood_size=3, feature_dtype='float16')
    (p_ref, r_ref), flips = GOLD[f'{name}_pr'], GOLD[f'{name}_pr_flips']
    for got, want, probes, allowed in ((res['precision'], p_ref, gen.shape[0], flips[0]), (res['recall'], r_ref, real.shape[0], flips[1])):
        # the reference's mean is float32: its count of covered probes is want * probes up to 2^-24 * probes, far below one probe
        differ = round(abs(got - want) * probes)
        print(f'{name}: {got!r} reference {want!r}: {differ} probes differ, recorded {allowed}')
        assert abs(abs(got - want) * probes - differ) <= 1e-3 and differ <= allowed and allowed <= 0.01 * probes


@pytest.mark.parametrize('dtype', ['float16', 'float32'])
def test_precision_recall_equals_brute_force(dtype):
    real, gen = case_features(*CASES['b'])
    real, gen = real[:90], gen[:75]
    res = dm.precision_recall(real, gen, nhood_size=3, feature_dtype=dtype)
    rr, gg = (real.astype(np.float16).astype(np.float32), gen.astype(np.float16).astype(np.float32)) if dtype == 'float16' else (real, gen)
    cov_gen, r2_real = brute_pr(rr, gg, 3)
    cov_real, r2_gen = brute_pr(gg, rr, 3)
    assert np.array_equal(res['covered_gen'], cov_gen) and np.array_equal(res['covered_real'], cov_real)
    # the brute force adds the D squares in another order than the package (the decisions above still agree); the radii are held to that
    # reordering of a float64 sum, D eps64
    rtol = real.shape[1] * np.finfo(np.float64).eps
    assert (np.abs(res['radii_real'] - np.sqrt(r2_real)) <= rtol * np.sqrt(r2_real)).all()
    assert (np.abs(res['radii_gen'] - np.sqrt(r2_gen)) <= rtol * np.sqrt(r2_gen)).all()
    assert res['precision'] == cov_gen.mean() and res['recall'] == cov_real.mean()


def test_precision_recall_duplicates_and_small_sets():
    rng = np.random.default_rng(0)
    base = (rng.integers(-32, 33, (6, 5)) / 8.0).astype(np.float32)
    manifold = np.concatenate([base, base[:2], base[:1]])                    # row 0 three times, row 1 twice
    res = dm.precision_recall(manifold, base + 100.0, nhood_size=2)
    assert res['radii_real'][0] == 0.0 and res['radii_real'][6] == 0.0 and res['radii_real'][8] == 0.0   # duplicates are separate points
    assert res['radii_real'][1] > 0.0                                        # two copies only: the third neighbour is elsewhere
    assert res['precision'] == 0.0 and res['recall'] == 0.0
    same = dm.precision_recall(manifold, manifold.copy(), nhood_size=2)
    assert same['precision'] == 1.0 and same['recall'] == 1.0                # a probe that is a manifold point is covered at distance 0
    with pytest.raises(ValueError, match='nhood_size = 9'):
        dm.precision_recall(manifold, manifold, nhood_size=9)                # nhood_size >= N
    with pytest.raises(ValueError, match='nhood_size must be'):
        dm.precision_recall(manifold, manifold, nhood_size=0)
    with pytest.raises(ValueError, match='feature_dtype'):
        dm.precision_recall(manifold, manifold, feature_dtype='bfloat16')
    with pytest.raises(ValueError, match='features'):
        dm.precision_recall(manifold, manifold[:, :3])


# ------------------------------------------------------------------ collector and CLI

def test_distribution_metrics_collects_features():
    real, gen = case_features(*CASES['b'])
    coll = dm.DistributionMetrics(kid_subsets=5, kid_subset_size=100, seed=2)
    for lo in range(0, 300, CHUNK):
        coll.update(real=real[lo:lo + CHUNK], gen=gen[lo:lo + CHUNK] if lo < gen.shape[0] else None)
    s = coll.summary()
    assert (s['num_real'], s['num_gen'], s['num_features'], s['kid_subset_size']) == (300, 257, 32, 100)
    assert s['fid'] == dm.fid(stats_of(real, capture_mean_cov=True), stats_of(gen, capture_mean_cov=True))
    assert s['kid'] == dm.kid(real, gen, 5, 100, 2)['kid']
    pr = dm.precision_recall(real, gen)
    assert (s['precision'], s['recall']) == (pr['precision'], pr['recall'])
    doubled = dm.DistributionMetrics(extractor=lambda x: np.asarray(x) * 2.0, kid_subsets=5, kid_subset_size=100, seed=2)
    doubled.update(real=real, gen=gen)
    assert abs(doubled.summary()['fid'] - 4.0 * s['fid']) <= 1e-9 * s['fid'] + 1e-9
    with pytest.raises(ValueError, match='real=, gen='):
        coll.update()
    with pytest.raises(ValueError, match='both sets'):
        dm.DistributionMetrics().summary()
    with pytest.raises(ValueError, match='extractor must be'):
        dm.DistributionMetrics(extractor=3)


KEYS = {'num_real', 'num_gen', 'num_features', 'fid', 'kid', 'kid_subsets', 'kid_subset_size', 'seed', 'precision', 'recall', 'nhood_size',
        'feature_dtype'}


def test_cli_on_feature_files(tmp_path, capsys):
    real, gen = case_features(*CASES['b'])
    rp, gp = str(tmp_path / 'real.npy'), str(tmp_path / 'gen.npy')
    np.save(rp, real), np.save(gp, gen)
    out1, out2, out3 = (str(tmp_path / f'm{i}.json') for i in range(3))
    assert dm.main(['--real', rp, '--gen', gp, '--out', out1, '--device', 'cpu']) == 0
    res = json.load(open(out1))
    assert set(res) == KEYS and json.loads(capsys.readouterr().out) == res
    assert (res['kid_subsets'], res['kid_subset_size'], res['seed'], res['nhood_size']) == (100, 257, 0, 3)
    want = dm.DistributionMetrics()
    want.update(real=real, gen=gen)
    assert res == want.summary()
    # the optional flags at their defaults change nothing, byte for byte
    assert dm.main(['--real', rp, '--gen', gp, '--out', out2, '--device', 'cpu', '--features', 'none', '--kid-subsets', '100',
                    '--kid-subset-size', '1000', '--seed', '0', '--nhood', '3']) == 0
    assert open(out1, 'rb').read() == open(out2, 'rb').read()
    assert dm.main(['--real', rp, '--gen', gp, '--out', out3, '--device', 'cpu', '--kid-subsets', '7', '--kid-subset-size', '64', '--seed', '5',
                    '--nhood', '5']) == 0
    other = json.load(open(out3))
    assert (other['kid_subsets'], other['kid_subset_size'], other['seed'], other['nhood_size']) == (7, 64, 5, 5)
    assert other['fid'] == res['fid'] and other['kid'] != res['kid']
    for bad in (['--id-synthetic', '0'], ['--features', 'identity'], ['--features', 'contextual'], ['--cx-weights', 'x.pt']):
        with pytest.raises(SystemExit):
            dm.main(['--real', rp, '--gen', gp, '--out', out3, '--device', 'cpu'] + bad)
    frames = str(tmp_path / 'frames.npy')
    np.save(frames, np.zeros((2, 3, 8, 8), np.float32))
    with pytest.raises(ValueError, match='feature stack'):
        dm.main(['--real', frames, '--gen', gp, '--out', out3, '--device', 'cpu'])
