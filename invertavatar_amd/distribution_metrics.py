"""Scores of a SET of frames as a distribution: Frechet distance (FID), kernel distance (KID) and precision / recall.

The per-frame scores (image_metrics, lpips, identity, contextual) compare a frame with its own ground truth; these compare the set of
generated frames with the set of real ones.  The definitions are the reference's ``metrics/`` package (``frechet_inception_distance.py``,
``kernel_inception_distance.py``, ``precision_recall.py`` on ``metric_utils.FeatureStats``), restated on feature sets ``[N, D]``:

  fid   |mu_a - mu_b|^2 + tr(Sa) + tr(Sb) - 2 tr sqrt(Sa Sb) from the sets' means and covariances (``FeatureStats``).
  kid   the mean over subsets of the unbiased MMD^2 estimate with k(u, v) = (u . v / D + 1)^3, divided by the subset size m as the
        reference divides it.
  p / r Kynkaanniemi's estimator: a probe is covered iff it lies within the radius of some manifold point, the radius of a point being
        the distance to its ``nhood_size``-th nearest other point.

This is NOT an Inception port: the reference runs TorchScript detectors that are not part of this package, so features come from arrays
or ``.npy`` files, from a callable, or from the two extractors of this package (``identity.embed``, 512-d; ``contextual.features`` pooled
over space, 256-d).  Only features of the reference's detectors (Inception-v3 pool3 for FID / KID, VGG16 fc for P/R) give numbers that
can be compared with published ones.

Device tensors go to the HIP kernels of csrc/distribution.hip (``hipops.feature_moments``, ``kid_subsets``, ``knn_radius``,
``manifold_covered``) and never fall back; CPU tensors and NumPy arrays take the NumPy restatement in float64, which is the definition
and the yardstick of the device tests.  Two deliberate differences from the reference: KID subsets come from
``numpy.random.default_rng(seed)`` (the reference draws from the unseeded global ``np.random``) or are given explicitly, and P/R compares
exact squared distances of the fp16-rounded features (the reference also rounds its distances and radii to fp16, which flips a handful
of borderline probes).

CLI:  python -m invertavatar_amd.distribution_metrics --real R --gen G --out m.json [--features identity|contextual|none]
          [--kid-subsets S --kid-subset-size M --seed K] [--nhood K] [--chunk N] [--device D]
R / G are ``.npy`` feature stacks ``[N,D]`` or, with ``--features identity|contextual``, frame stacks or directories of them as in
``image_metrics``.  ``--id-weights FILE`` / ``--id-synthetic SEED`` and ``--cx-weights FILE`` / ``--cx-synthetic SEED`` give the
extractor's weights; the synthetic switches are for smoke runs and their numbers mean nothing."""
import json
import sys

import numpy as np
import torch


def _is_device(x):
    return torch.is_tensor(x) and x.is_cuda


def _host32(x):
    """Array or CPU tensor -> float32 NumPy [N,D]."""
    if torch.is_tensor(x):
        x = x.detach().cpu().numpy()
    x = np.asarray(x, dtype=np.float32)
    if x.ndim != 2:
        raise ValueError(f'features must be [N, D], got {x.shape}')
    return x


def _device32(x):
    if x.dim() != 2:
        raise ValueError(f'features must be [N, D], got {tuple(x.shape)}')
    return x.detach().float().contiguous()


# ------------------------------------------------------------------ FeatureStats

class FeatureStats:
    """The reference's ``metric_utils.FeatureStats``: same constructor, attributes and methods.  ``append`` / ``append_torch`` of a device
    tensor keep everything on that device: ``raw_mean`` [D] and ``raw_cov`` [D,D] are float64 device tensors filled by
    ``ia_feature_moments``, the rows are kept as float32 when ``capture_all``, and nothing waits for the device.  CPU tensors and NumPy
    arrays take the reference's arithmetic (float64 ``x64.sum(0)`` and ``x64.T @ x64`` per appended chunk, added in call order).  One
    object takes one kind of input.  ``save`` / ``load`` write ``.npz``, not a pickle."""

    def __init__(self, capture_all=False, capture_mean_cov=False, max_items=None):
        self.capture_all = capture_all
        self.capture_mean_cov = capture_mean_cov
        self.max_items = max_items
        self.num_items = 0
        self.num_features = None
        self.all_features = None
        self.raw_mean = None
        self.raw_cov = None
        self.device = None                       # None until the first append; then 'cpu' or the torch device of the features

    def set_num_features(self, num_features, device='cpu'):
        if self.num_features is not None:
            if num_features != self.num_features:
                raise ValueError(f'features have {num_features} columns, the earlier ones {self.num_features}')
            if str(device) != str(self.device):
                raise ValueError(f'features on {device} appended to statistics on {self.device}')
            return
        self.num_features = num_features
        self.device = device
        self.all_features = []
        if device == 'cpu':
            self.raw_mean = np.zeros([num_features], dtype=np.float64)
            self.raw_cov = np.zeros([num_features, num_features], dtype=np.float64)
        elif self.capture_mean_cov:
            self.raw_mean = torch.zeros(num_features, dtype=torch.float64, device=device)
            self.raw_cov = torch.zeros(num_features, num_features, dtype=torch.float64, device=device)

    def is_full(self):
        return (self.max_items is not None) and (self.num_items >= self.max_items)

    def append(self, x):
        dev = _is_device(x)
        x = _device32(x) if dev else _host32(x)
        if (self.max_items is not None) and (self.num_items + x.shape[0] > self.max_items):
            if self.num_items >= self.max_items:
                return
            x = x[:self.max_items - self.num_items]
        self.set_num_features(x.shape[1], x.device if dev else 'cpu')
        self.num_items += x.shape[0]
        if self.capture_all:
            self.all_features.append(x)
        if self.capture_mean_cov:
            if dev:
                from . import hipops
                hipops.feature_moments(x.contiguous(), self.raw_mean, self.raw_cov)
            else:
                x64 = x.astype(np.float64)
                self.raw_mean += x64.sum(axis=0)
                self.raw_cov += x64.T @ x64

    def append_torch(self, x, num_gpus=1, rank=0):
        if not (torch.is_tensor(x) and x.dim() == 2):
            raise ValueError('append_torch takes a 2-D tensor')
        if num_gpus != 1 or rank != 0:
            raise ValueError('one process, one device: num_gpus must be 1 and rank 0')
        self.append(x)

    def get_all(self):
        """Every row, in the order appended -> float32 NumPy [N,D] (one device -> host read for device statistics)."""
        return self.get_all_torch().cpu().numpy() if self.device not in (None, 'cpu') else self._all_host()

    def _all_host(self):
        if not self.capture_all:
            raise ValueError('these statistics were built with capture_all=False')
        if not self.all_features:
            raise ValueError('no features were appended')
        return np.concatenate(self.all_features, axis=0)

    def get_all_torch(self):
        """Every row as a float32 tensor, on the device for device statistics."""
        if self.device in (None, 'cpu'):
            return torch.from_numpy(self._all_host())
        if not self.capture_all:
            raise ValueError('these statistics were built with capture_all=False')
        return torch.cat(self.all_features, 0)

    def get_mean_cov_torch(self):
        """(mean [D], cov [D,D]) as float64 tensors where the statistics live; the population covariance, as the reference's."""
        if not self.capture_mean_cov:
            raise ValueError('these statistics were built with capture_mean_cov=False')
        if self.num_items < 1:
            raise ValueError('no features were appended')
        raw_mean, raw_cov = (torch.from_numpy(self.raw_mean), torch.from_numpy(self.raw_cov)) if self.device == 'cpu' else (self.raw_mean, self.raw_cov)
        mean = raw_mean / self.num_items
        cov = raw_cov / self.num_items
        return mean, cov - torch.outer(mean, mean)

    def get_mean_cov(self):
        """(mean, cov) as float64 NumPy arrays, the reference's arithmetic (one device -> host read for device statistics)."""
        if self.device in (None, 'cpu'):
            if not self.capture_mean_cov:
                raise ValueError('these statistics were built with capture_mean_cov=False')
            if self.num_items < 1:
                raise ValueError('no features were appended')
            mean = self.raw_mean / self.num_items
            cov = self.raw_cov / self.num_items
            return mean, cov - np.outer(mean, mean)
        mean, cov = self.get_mean_cov_torch()
        return mean.cpu().numpy(), cov.cpu().numpy()

    def save(self, npz_file):
        """Writes a ``.npz`` (arrays only; device statistics are read back once)."""
        data = {'capture_all': np.bool_(self.capture_all), 'capture_mean_cov': np.bool_(self.capture_mean_cov),
                'max_items': np.int64(-1 if self.max_items is None else self.max_items), 'num_items': np.int64(self.num_items),
                'num_features': np.int64(-1 if self.num_features is None else self.num_features)}
        if self.num_features is not None:
            if self.capture_mean_cov:
                on_host = self.device == 'cpu'
                data['raw_mean'] = self.raw_mean if on_host else self.raw_mean.cpu().numpy()
                data['raw_cov'] = self.raw_cov if on_host else self.raw_cov.cpu().numpy()
            if self.capture_all:
                data['all_features'] = self.get_all()
        with open(npz_file, 'wb') as fh:
            np.savez(fh, **data)

    @staticmethod
    def load(npz_file):
        """Statistics from ``save``, on the host."""
        with np.load(npz_file, allow_pickle=False) as z:
            obj = FeatureStats(bool(z['capture_all']), bool(z['capture_mean_cov']), None if int(z['max_items']) < 0 else int(z['max_items']))
            if int(z['num_features']) >= 0:
                obj.set_num_features(int(z['num_features']))
                obj.num_items = int(z['num_items'])
                if obj.capture_mean_cov:
                    obj.raw_mean, obj.raw_cov = z['raw_mean'].astype(np.float64), z['raw_cov'].astype(np.float64)
                if obj.capture_all:
                    obj.all_features = [z['all_features'].astype(np.float32)]
        return obj


# ------------------------------------------------------------------ Frechet distance

def frechet_distance(mu_a, sigma_a, mu_b, sigma_b):
    """|mu_a - mu_b|^2 + tr(Sa) + tr(Sb) - 2 tr sqrt(Sa Sb) in float64 -> float.

    The last term is the sum of sqrt(max(l, 0)) over the eigenvalues l of the symmetric matrix H Sb H with H = sqrt(Sa) from one
    symmetric eigendecomposition (eigenvalues clamped at 0): Sa Sb is similar to H Sb H wherever Sa is invertible, and the limit holds
    where it is not.  Two ``eigh`` calls: ``numpy.linalg`` for arrays and CPU tensors, ``torch.linalg`` on the device for device tensors.
    The reference calls ``scipy.linalg.sqrtm`` on the unsymmetric product instead.  On full-rank covariances the two agree to the
    rounding of either (3e-12 on 64-d covariances of 500-600 samples); with fewer samples than dimensions the product is singular and
    it is ``sqrtm`` that is inexact there (1e-7 on 64 dimensions from 40 and 48 samples): its Schur recurrence divides by sums of
    square roots of eigenvalues that are zero up to rounding."""
    if any(_is_device(t) for t in (mu_a, sigma_a, mu_b, sigma_b)):
        if not all(_is_device(t) for t in (mu_a, sigma_a, mu_b, sigma_b)):
            raise ValueError('frechet_distance: all four on the device, or none')
        mu_a, sigma_a, mu_b, sigma_b = (t.double() for t in (mu_a, sigma_a, mu_b, sigma_b))
        _check_moments(mu_a.shape, sigma_a.shape, mu_b.shape, sigma_b.shape)
        w, v = torch.linalg.eigh(sigma_a)
        h = (v * w.clamp_min(0.0).sqrt()) @ v.T
        mid = h @ sigma_b @ h
        lam = torch.linalg.eigvalsh((mid + mid.T) * 0.5)
        d = mu_a - mu_b
        return float((d * d).sum() + torch.trace(sigma_a) + torch.trace(sigma_b) - 2.0 * lam.clamp_min(0.0).sqrt().sum())
    mu_a, sigma_a, mu_b, sigma_b = (np.asarray(t.numpy() if torch.is_tensor(t) else t, dtype=np.float64) for t in (mu_a, sigma_a, mu_b, sigma_b))
    _check_moments(mu_a.shape, sigma_a.shape, mu_b.shape, sigma_b.shape)
    w, v = np.linalg.eigh(sigma_a)
    h = (v * np.sqrt(np.maximum(w, 0.0))) @ v.T
    mid = h @ sigma_b @ h
    lam = np.linalg.eigvalsh((mid + mid.T) * 0.5)
    d = mu_a - mu_b
    return float((d * d).sum() + np.trace(sigma_a) + np.trace(sigma_b) - 2.0 * np.sqrt(np.maximum(lam, 0.0)).sum())


def _check_moments(ma, sa, mb, sb):
    if len(ma) != 1 or tuple(ma) != tuple(mb) or tuple(sa) != (ma[0], ma[0]) or tuple(sb) != tuple(sa):
        raise ValueError(f'frechet_distance takes means [D] and covariances [D,D], got {tuple(ma)}, {tuple(sa)}, {tuple(mb)}, {tuple(sb)}')


def fid(stats_real, stats_gen):
    """Frechet distance of two ``FeatureStats`` (``capture_mean_cov=True``) -> float; on the device when both live there."""
    if stats_real.device not in (None, 'cpu') and stats_gen.device not in (None, 'cpu'):
        return frechet_distance(*stats_gen.get_mean_cov_torch(), *stats_real.get_mean_cov_torch())
    return frechet_distance(*stats_gen.get_mean_cov(), *stats_real.get_mean_cov())


# ------------------------------------------------------------------ kernel distance

def kid_subset_indices(n_real, n_gen, num_subsets=100, max_subset_size=1000, seed=0):
    """(idx_gen [S,m], idx_real [S,m]) int64 from ``numpy.random.default_rng(seed)``: per subset m rows of the generated set without
    replacement, then m rows of the real set, the reference's order of draws.  m = min(n_real, n_gen, max_subset_size)."""
    m = min(int(n_real), int(n_gen), int(max_subset_size))
    if m < 2:
        raise ValueError(f'KID needs subsets of at least two rows, got m = {m}')
    rng = np.random.default_rng(seed)
    ig, ir = np.empty((num_subsets, m), np.int64), np.empty((num_subsets, m), np.int64)
    for s in range(num_subsets):
        ig[s] = rng.choice(int(n_gen), m, replace=False)
        ir[s] = rng.choice(int(n_real), m, replace=False)
    return ig, ir


def kid_sums_reference(gen, real, idx_gen, idx_real, dot_dtype=np.float64):
    """The three sums of ``ia_kid_subsets`` per subset, restated in NumPy -> float64 [S,3].  ``dot_dtype=np.float32`` forms the dot
    products in float32 as the kernel does (the restatement's own float32 run, the unit of the device tests' bounds); the cube and the
    sums are float64 either way."""
    gen, real = _host32(gen), _host32(real)
    n = float(gen.shape[1])
    out = np.zeros((len(idx_gen), 3), np.float64)
    for s, (ig, ir) in enumerate(zip(idx_gen, idx_real)):
        x, y = gen[ig].astype(dot_dtype), real[ir].astype(dot_dtype)
        for col, (a, b) in enumerate(((x, x), (y, y), (x, y))):
            t = (a @ b.T).astype(np.float64) / n + 1.0
            t = (t * t) * t
            out[s, col] = t.sum() - (np.trace(t) if col < 2 else 0.0)
    return out


def kid(real, gen, num_subsets=100, max_subset_size=1000, seed=0, subsets=None):
    """The reference's KID estimator on feature sets ``real`` [Nr,D] and ``gen`` [Ng,D]: with n = D, m = min(Nr, Ng, max_subset_size)
    and k(u, v) = (u . v / n + 1)^3, a subset's value is (sum_{i != j} k(x_i, x_j) + sum_{i != j} k(y_i, y_j)) / (m - 1) -
    2 sum_{ij} k(x_i, y_j) / m; the values are summed and divided by num_subsets m.  ``subsets=(idx_gen [S,m], idx_real [S,m])`` gives
    the subsets explicitly (then num_subsets, max_subset_size and seed are not used); otherwise they are ``kid_subset_indices``.
    -> ``{'kid': float, 'per_subset': float64 [S] (NumPy; a device tensor for device features), 'm': int}``."""
    dev = _is_device(real)
    if dev != _is_device(gen):
        raise ValueError('kid: both feature sets on the device, or neither')
    real, gen = (_device32(real), _device32(gen)) if dev else (_host32(real), _host32(gen))
    if real.shape[1] != gen.shape[1]:
        raise ValueError(f'kid: the sets have {real.shape[1]} and {gen.shape[1]} features')
    if subsets is None:
        ig, ir = kid_subset_indices(real.shape[0], gen.shape[0], num_subsets, max_subset_size, seed)
    else:
        ig, ir = (np.asarray(t.cpu() if torch.is_tensor(t) else t) for t in subsets)
        if ig.ndim != 2 or ig.shape != ir.shape or ig.shape[1] < 2 or ig.dtype.kind not in 'iu' or ir.dtype.kind not in 'iu':
            raise ValueError('kid: subsets must be two integer arrays of one shape [S, m] with m >= 2')
        if ig.size and (ig.min() < 0 or ig.max() >= gen.shape[0] or ir.min() < 0 or ir.max() >= real.shape[0]):
            raise ValueError('kid: a subset index is outside its set')
    s, m = ig.shape
    if dev:
        from . import hipops
        sums = hipops.kid_subsets(gen, real, ig, ir)
    else:
        sums = kid_sums_reference(gen, real, ig, ir)
    per = (sums[:, 0] + sums[:, 1]) / (m - 1) - sums[:, 2] * 2 / m
    return {'kid': float(per.sum() / s / m) if s else float('nan'), 'per_subset': per, 'm': int(m)}


# ------------------------------------------------------------------ precision / recall

def _round_features(x, feature_dtype):
    if feature_dtype not in ('float16', 'float32'):
        raise ValueError(f"feature_dtype must be 'float16' or 'float32', got {feature_dtype!r}")
    if feature_dtype == 'float32':
        return x
    return x.half().float() if torch.is_tensor(x) else x.astype(np.float16).astype(np.float32)


def sqdist64(a, b, block=64):
    """Squared distances of float32 rows a [P,D] against b [N,D] in the difference form, float64 -> [P,N] (the differences of float32
    values are exact in float64)."""
    a64, b64 = np.asarray(a, np.float64), np.asarray(b, np.float64)
    out = np.empty((a64.shape[0], b64.shape[0]), np.float64)
    for i in range(0, a64.shape[0], block):
        for j in range(0, b64.shape[0], 4 * block):
            d = a64[i:i + block, None, :] - b64[None, j:j + 4 * block, :]
            out[i:i + block, j:j + 4 * block] = np.einsum('pnd,pnd->pn', d, d)
    return out


def knn_radius_reference(feat, k):
    """r2[j] = the (k + 1)-th smallest squared distance from row j to the rows of ``feat``, itself included -> float64 [N]."""
    return np.partition(sqdist64(feat, feat), k, axis=1)[:, k]


def covered_reference(probes, manifold, r2):
    return (sqdist64(probes, manifold) <= np.asarray(r2, np.float64)[None, :]).any(axis=1)


def precision_recall(real, gen, nhood_size=3, feature_dtype='float16'):
    """Kynkaanniemi's precision and recall of feature sets ``real`` [Nr,D] and ``gen`` [Ng,D].  The radius of manifold point j is the
    (nhood_size + 1)-th smallest distance from j to the manifold's points, j included and duplicates counted; a probe is covered iff
    d(probe, j) <= radius_j for some j.  Precision: manifold real, probes gen; recall the reverse.  ``feature_dtype='float16'`` rounds the
    features through fp16 first, as the reference does.  Squared distances of those features are compared exactly (float64 on the host;
    fp32 difference form on the device), where the reference also rounds its distances and radii to fp16.
    -> ``{'precision', 'recall'}`` floats, ``'radii_real', 'radii_gen'`` (distances, not squared) and ``'covered_gen', 'covered_real'``
    (bool per probe), NumPy on the host and tensors on the device."""
    dev = _is_device(real)
    if dev != _is_device(gen):
        raise ValueError('precision_recall: both feature sets on the device, or neither')
    real, gen = (_device32(real), _device32(gen)) if dev else (_host32(real), _host32(gen))
    if real.shape[1] != gen.shape[1]:
        raise ValueError(f'precision_recall: the sets have {real.shape[1]} and {gen.shape[1]} features')
    k = int(nhood_size)
    if k < 1:
        raise ValueError(f'nhood_size must be >= 1, got {nhood_size}')
    if min(real.shape[0], gen.shape[0]) <= k:
        raise ValueError(f'nhood_size = {k} needs more than {k} rows in each set, got {real.shape[0]} real and {gen.shape[0]} generated')
    real, gen = _round_features(real, feature_dtype), _round_features(gen, feature_dtype)
    if dev:
        from . import hipops
        real, gen = real.contiguous(), gen.contiguous()
        r2_real, r2_gen = hipops.knn_radius(real, k), hipops.knn_radius(gen, k)
        cov_gen, cov_real = hipops.manifold_covered(gen, real, r2_real), hipops.manifold_covered(real, gen, r2_gen)
        return {'precision': float(cov_gen.float().mean()), 'recall': float(cov_real.float().mean()), 'radii_real': r2_real.sqrt(),
                'radii_gen': r2_gen.sqrt(), 'covered_gen': cov_gen, 'covered_real': cov_real}
    r2_real, r2_gen = knn_radius_reference(real, k), knn_radius_reference(gen, k)
    cov_gen, cov_real = covered_reference(gen, real, r2_real), covered_reference(real, gen, r2_gen)
    return {'precision': float(cov_gen.mean()), 'recall': float(cov_real.mean()), 'radii_real': np.sqrt(r2_real), 'radii_gen': np.sqrt(r2_gen),
            'covered_gen': cov_gen, 'covered_real': cov_real}


# ------------------------------------------------------------------ the collector

def _as_extractor(extractor):
    """None, a callable frames -> [N,D], or one of this package's models (identity.IDScore: 512-d embeddings; contextual.CXScore: the
    256 relu3_4 channels averaged over space)."""
    if extractor is None:
        return None
    from . import contextual as _contextual, identity as _identity
    if isinstance(extractor, _identity.IDScore):
        return lambda frames: _identity.embed(frames, extractor)
    if isinstance(extractor, _contextual.CXScore):
        return lambda frames: _contextual.features(frames, extractor).mean(dim=(2, 3))
    if not callable(extractor):
        raise ValueError('extractor must be None, a callable, an identity.IDScore or a contextual.CXScore')
    return extractor


class DistributionMetrics:
    """The two sets of a run, gathered call by call.  ``update(real=..., gen=...)`` takes frame batches (run through ``extractor``) or,
    with ``extractor=None``, features ``[N,D]``, and appends them to two ``FeatureStats`` where they live: no host synchronisation.
    ``summary`` computes FID, KID and precision / recall once."""

    def __init__(self, extractor=None, kid_subsets=100, kid_subset_size=1000, seed=0, nhood_size=3, feature_dtype='float16', max_items=None):
        self.extractor = _as_extractor(extractor)
        self.kid_subsets, self.kid_subset_size, self.seed = int(kid_subsets), int(kid_subset_size), int(seed)
        self.nhood_size, self.feature_dtype = int(nhood_size), feature_dtype
        _round_features(np.zeros((1, 1), np.float32), feature_dtype)
        self.real = FeatureStats(capture_all=True, capture_mean_cov=True, max_items=max_items)
        self.gen = FeatureStats(capture_all=True, capture_mean_cov=True, max_items=max_items)

    def _features(self, batch):
        if self.extractor is None:
            return batch
        with torch.no_grad():
            f = self.extractor(batch)
        if not (torch.is_tensor(f) or isinstance(f, np.ndarray)) or f.ndim != 2:
            raise ValueError('the extractor must return features [N, D]')
        return f

    def update(self, real=None, gen=None):
        if real is None and gen is None:
            raise ValueError('update needs real=, gen= or both')
        if real is not None:
            self.real.append(self._features(real))
        if gen is not None:
            self.gen.append(self._features(gen))

    def reset(self):
        self.real = FeatureStats(capture_all=True, capture_mean_cov=True, max_items=self.real.max_items)
        self.gen = FeatureStats(capture_all=True, capture_mean_cov=True, max_items=self.gen.max_items)

    def summary(self):
        if self.real.num_items < 1 or self.gen.num_items < 1:
            raise ValueError(f'both sets are needed, got {self.real.num_items} real and {self.gen.num_items} generated rows')
        real, gen = self.real.get_all_torch(), self.gen.get_all_torch()
        if self.real.device == 'cpu' or self.gen.device == 'cpu':
            real, gen = real.cpu().numpy(), gen.cpu().numpy()
        k = kid(real, gen, self.kid_subsets, self.kid_subset_size, self.seed)
        pr = precision_recall(real, gen, self.nhood_size, self.feature_dtype)
        return {'num_real': self.real.num_items, 'num_gen': self.gen.num_items, 'num_features': self.real.num_features,
                'fid': fid(self.real, self.gen), 'kid': k['kid'], 'kid_subsets': self.kid_subsets, 'kid_subset_size': k['m'],
                'seed': self.seed, 'precision': pr['precision'], 'recall': pr['recall'], 'nhood_size': self.nhood_size,
                'feature_dtype': self.feature_dtype}

    def write_json(self, path):
        res = self.summary()
        with open(path, 'w') as fh:
            json.dump(res, fh)
            fh.write('\n')
        return res


# ------------------------------------------------------------------ CLI

def score_files(real, gen, extractor=None, chunk=16, device=None, **kwargs):
    """Two ``.npy`` stacks (or directories of them): feature stacks [N,D] with ``extractor=None``, frame stacks otherwise -> DistributionMetrics."""
    from .image_metrics import _frames, _stack_files
    device = device or ('cuda' if torch.cuda.is_available() else 'cpu')
    dm = DistributionMetrics(extractor, **kwargs)
    for name, path in (('real', real), ('gen', gen)):
        for arr in _frames(_stack_files(path)) if extractor is not None else (np.load(f, mmap_mode='r') for f in _stack_files(path)):
            if extractor is None and arr.ndim != 2:
                raise ValueError(f'{path}: a feature stack must be [N, D], got {arr.shape} (frames need --features identity|contextual)')
            step = chunk if extractor is not None else max(chunk, 4096)
            for lo in range(0, arr.shape[0], step):
                dm.update(**{name: torch.from_numpy(np.array(arr[lo:lo + step])).to(device)})
    return dm


def main(argv=None):
    import argparse
    ap = argparse.ArgumentParser(description='FID / KID / precision and recall of two feature sets (.npy [N,D]) or, through an extractor, two frame stacks')
    ap.add_argument('--real', required=True)
    ap.add_argument('--gen', required=True)
    ap.add_argument('--out', required=True)
    ap.add_argument('--features', choices=('identity', 'contextual', 'none'), default='none', help='extractor for frame stacks; none: R and G hold features')
    ap.add_argument('--kid-subsets', type=int, default=100)
    ap.add_argument('--kid-subset-size', type=int, default=1000)
    ap.add_argument('--seed', type=int, default=0, help='seed of the KID subsets')
    ap.add_argument('--nhood', type=int, default=3, help='neighbourhood size of precision / recall')
    ap.add_argument('--chunk', type=int, default=16, help='frames per extractor call')
    ap.add_argument('--device', default=None)
    ap.add_argument('--id-weights', default=None, help='--features identity: the ArcFace IR-SE50 state dict (model_ir_se50.pth)')
    ap.add_argument('--id-synthetic', type=int, default=None, metavar='SEED', help='seeded identity weights instead of a file (smoke runs only)')
    ap.add_argument('--cx-weights', default=None, help='--features contextual: a torchvision vgg19 state dict')
    ap.add_argument('--cx-synthetic', type=int, default=None, metavar='SEED', help='seeded VGG19 weights instead of a file (smoke runs only)')
    args = ap.parse_args(argv)
    extractor = None
    if args.features != 'identity' and (args.id_weights is not None or args.id_synthetic is not None):
        ap.error('--id-weights / --id-synthetic need --features identity')
    if args.features != 'contextual' and (args.cx_weights is not None or args.cx_synthetic is not None):
        ap.error('--cx-weights / --cx-synthetic need --features contextual')
    if args.features == 'identity':
        from . import identity as _identity
        if args.id_weights is not None and args.id_synthetic is not None:
            ap.error('--id-weights and --id-synthetic exclude each other')
        if args.id_synthetic is not None:
            print(f'warning: identity features with synthetic weights (seed {args.id_synthetic}): the numbers mean nothing', file=sys.stderr)
            extractor = _identity.IDScore.synthetic(args.id_synthetic)
        elif args.id_weights is not None:
            extractor = _identity.IDScore(args.id_weights)
        else:
            ap.error('--features identity needs --id-weights FILE or --id-synthetic SEED')
    elif args.features == 'contextual':
        from . import contextual as _contextual
        if args.cx_weights is not None and args.cx_synthetic is not None:
            ap.error('--cx-weights and --cx-synthetic exclude each other')
        if args.cx_synthetic is not None:
            print(f'warning: contextual features with synthetic weights (seed {args.cx_synthetic}): the numbers mean nothing', file=sys.stderr)
            extractor = _contextual.CXScore.synthetic(args.cx_synthetic)
        elif args.cx_weights is not None:
            extractor = _contextual.CXScore(args.cx_weights)
        else:
            ap.error('--features contextual needs --cx-weights FILE or --cx-synthetic SEED')
    dm = score_files(args.real, args.gen, extractor, args.chunk, args.device, kid_subsets=args.kid_subsets, kid_subset_size=args.kid_subset_size,
                     seed=args.seed, nhood_size=args.nhood)
    res = dm.write_json(args.out)
    print(json.dumps(res))
    return 0


if __name__ == '__main__':
    raise SystemExit(main())
