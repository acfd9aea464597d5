"""Records tests/golden/distribution.npz: results of the reference's metrics/ package (frechet_inception_distance.compute_fid,
kernel_inception_distance.compute_kid, precision_recall.compute_pr) on seed-generated feature sets.

Runs only where the reference checkout is present (as make_image_metrics_golden.py): this script imports the reference's modules at
generation time and stores seeds' results only, never its text.  The three functions fetch their features through
``metric_utils.compute_feature_stats_for_dataset`` / ``_for_generator``; both attributes are replaced at run time by functions that fill a
reference ``FeatureStats`` from the seeded arrays of ``case_features`` (below), appended in chunks of CHUNK rows, and the functions are
called with ``opts = EasyDict(rank=0, num_gpus=1, device=cpu)``.

Per case <c> in CASES (seeded Gaussians through a random D x D mixing matrix; the generated set has scale 1.1 and offset 0.6, the real
set scale 1.0 and offset 0.5):
  <c>_fid                          compute_fid (scipy.linalg.sqrtm)
  <c>_mean_real, <c>_cov_real, <c>_mean_gen, <c>_cov_gen     the reference FeatureStats.get_mean_cov() (float64)
  <c>_kid                          compute_kid(num_subsets=10, max_subset_size=200) with np.random.seed(KID_SEED) set just before
  <c>_kid_idx_gen, <c>_kid_idx_real   [10, m] the same np.random.choice sequence replayed: kid(subsets=...) gets the identical subsets
  <c>_pr                           (precision, recall) of compute_pr(nhood_size=3, row_batch_size=128, col_batch_size=100)
  <c>_pr_flips                     (n_gen_probes, n_real_probes) on which the reference's fp16 route and this package's exact definition
                                   disagree, bounded by |p - p_ref| P (asserted <= 1 % of the probes)
rank_fid, rank_e_ref               the rank-deficient FID case (D = 64, 40 real and 48 generated rows) and its distance from frechet_distance
e_ref_fid, e_ref_kid               the largest distance of the reference's results from this package's float64 restatement over the
                                   full-rank cases: the reference's own rounding, the unit of the tests' bounds.
Usage: python tests/golden/make_distribution_golden.py --ref <reference checkout>"""
import argparse
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.abspath(os.path.join(HERE, '..', '..'))
sys.path.insert(0, REPO)

CASES = {'a': (64, 600, 500, 11), 'b': (32, 300, 257, 12), 'c': (128, 1000, 900, 13)}      # name: (D, N_real, N_gen, seed)
RANK_CASE = (64, 40, 48, 14)
CHUNK = 97
KID_SEED, KID_SUBSETS, KID_SUBSET_SIZE = 5, 10, 200


def case_features(d, n_real, n_gen, seed):
    """(real [n_real, d], gen [n_gen, d]) float32."""
    rng = np.random.default_rng(seed)
    mix = rng.standard_normal((d, d)) / np.sqrt(d)
    real = (rng.standard_normal((n_real, d)) @ mix) * 1.0 + 0.5
    gen = (rng.standard_normal((n_gen, d)) @ mix) * 1.1 + 0.6
    return real.astype(np.float32), gen.astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--ref', required=True, help='root of the reference checkout')
    ap.add_argument('--out', default=os.path.join(HERE, 'distribution.npz'))
    args = ap.parse_args()
    sys.path.insert(0, args.ref)
    import dnnlib                                            # the reference's packages, imported, never copied
    from metrics import frechet_inception_distance as ref_fid, kernel_inception_distance as ref_kid, metric_utils, precision_recall as ref_pr
    from invertavatar_amd import distribution_metrics as dm

    opts = dnnlib.EasyDict(rank=0, num_gpus=1, device=torch.device('cpu'))
    current = {}

    def fill(which):
        def fn(opts, capture_all=False, capture_mean_cov=False, max_items=None, **_):
            stats = metric_utils.FeatureStats(capture_all=capture_all, capture_mean_cov=capture_mean_cov, max_items=max_items)
            x = current[which]
            for lo in range(0, x.shape[0], CHUNK):
                stats.append(x[lo:lo + CHUNK])
            current[which + '_stats'] = stats
            return stats
        return fn

    metric_utils.compute_feature_stats_for_dataset = fill('real')
    metric_utils.compute_feature_stats_for_generator = fill('gen')

    out, e_fid, e_kid = {}, 0.0, 0.0
    for name, (d, n_real, n_gen, seed) in list(CASES.items()) + [('rank', RANK_CASE)]:
        real, gen = case_features(d, n_real, n_gen, seed)
        current['real'], current['gen'] = real, gen
        fid_ref = ref_fid.compute_fid(opts, max_real=None, num_gen=None)
        mu_r, cov_r = current['real_stats'].get_mean_cov()
        mu_g, cov_g = current['gen_stats'].get_mean_cov()
        ours = dm.frechet_distance(mu_g, cov_g, mu_r, cov_r)
        if name == 'rank':
            out['rank_fid'], out['rank_e_ref'] = np.float64(fid_ref), np.float64(abs(fid_ref - ours))
            print(f'rank-deficient: fid {fid_ref:.6f}, |sqrtm - eigh| {abs(fid_ref - ours):.3e}')
            continue
        e_fid = max(e_fid, abs(fid_ref - ours))
        out[f'{name}_fid'] = np.float64(fid_ref)
        out[f'{name}_mean_real'], out[f'{name}_cov_real'], out[f'{name}_mean_gen'], out[f'{name}_cov_gen'] = mu_r, cov_r, mu_g, cov_g

        np.random.seed(KID_SEED)
        kid_ref = ref_kid.compute_kid(opts, max_real=None, num_gen=None, num_subsets=KID_SUBSETS, max_subset_size=KID_SUBSET_SIZE)
        np.random.seed(KID_SEED)                             # the same draws, replayed in the order compute_kid makes them
        m = min(n_real, n_gen, KID_SUBSET_SIZE)
        ig, ir = [], []
        for _ in range(KID_SUBSETS):
            ig.append(np.random.choice(n_gen, m, replace=False))
            ir.append(np.random.choice(n_real, m, replace=False))
        ig, ir = np.stack(ig).astype(np.int32), np.stack(ir).astype(np.int32)
        kid_ours = dm.kid(real, gen, subsets=(ig, ir))['kid']
        e_kid = max(e_kid, abs(kid_ref - kid_ours))
        out[f'{name}_kid'], out[f'{name}_kid_idx_gen'], out[f'{name}_kid_idx_real'] = np.float64(kid_ref), ig, ir

        p_ref, r_ref = ref_pr.compute_pr(opts, max_real=None, num_gen=None, nhood_size=3, row_batch_size=128, col_batch_size=100)
        pr = dm.precision_recall(real, gen, nhood_size=3, feature_dtype='float16')
        flips = (int(round(abs(pr['precision'] - p_ref) * n_gen)), int(round(abs(pr['recall'] - r_ref) * n_real)))
        assert flips[0] <= 0.01 * n_gen and flips[1] <= 0.01 * n_real, f'{name}: {flips} probes flip: choose other inputs'
        out[f'{name}_pr'], out[f'{name}_pr_flips'] = np.array([p_ref, r_ref], np.float64), np.array(flips, np.int64)
        print(f'{name}: fid {fid_ref:.6f} (ours {ours:.6f}), kid {kid_ref:.6e} (ours {kid_ours:.6e}), p/r {p_ref:.4f} {r_ref:.4f} '
              f'(ours {pr["precision"]:.4f} {pr["recall"]:.4f}, flips {flips})')
    out['e_ref_fid'], out['e_ref_kid'] = np.float64(e_fid), np.float64(e_kid)
    print(f'e_ref: fid {e_fid:.3e}, kid {e_kid:.3e}')
    np.savez(args.out, **out)


if __name__ == '__main__':
    main()
