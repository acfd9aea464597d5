"""Shared inputs of tests/test_point_cloud_cpu.py and tests/test_point_cloud_gpu.py: clouds of the sizes at which the tree changes shape
(one point, a leaf short of / at / past 32, one branch, past one branch, three levels, 20 000), the query sets, the lattice with exact
ties, and the cloud alignment case.  Everything is computed once per process and never modified."""
import functools

import numpy as np

from invertavatar_amd import geometry
from test_align_cpu import bumpy_mesh, moved, similarity
from test_surface_distance_cpu import EPS32, F32, extent_of

CLOUD_SIZES = (1, 31, 32, 33, 256, 257, 2049, 20000)
QUERY_COUNTS = (1, 63, 64, 65, 1000)
KS = (1, 3, 8, 16, 32)
EPS64 = float(np.finfo(np.float64).eps)


@functools.lru_cache(maxsize=None)
def cloud(n, seed=0):
    """n points in general position in the box [-1, 1] x [-0.7, 0.7] x [-0.5, 0.5]."""
    rng = np.random.default_rng(1000 * seed + n)
    pts = (rng.random((n, 3)) * 2 - 1) * np.array([1.0, 0.7, 0.5])
    pts = pts.astype(F32)
    pts.setflags(write=False)
    return pts


@functools.lru_cache(maxsize=None)
def queries(kind, count, n=0):
    """'self': the first ``count`` points of cloud(n); 'box': random points of a box a little larger than the cloud's; 'far': points at
    10 extents."""
    rng = np.random.default_rng(7 + count)
    if kind == 'self':
        q = cloud(n)[:count].copy()
    elif kind == 'box':
        q = ((rng.random((count, 3)) * 2 - 1) * 1.2).astype(F32)
    else:
        d = rng.standard_normal((count, 3))
        q = (10.0 * d / np.linalg.norm(d, axis=1, keepdims=True)).astype(F32)
    q.setflags(write=False)
    return q


@functools.lru_cache(maxsize=None)
def lattice():
    """(points, queries) of the 9^3 integer lattice, in a scrambled order: the queries are the lattice points and the cell centres, so
    that most nearest sets hold many exactly equal distances."""
    ax = np.arange(9, dtype=F32)
    pts = np.stack(np.meshgrid(ax, ax, ax, indexing='ij'), -1).reshape(-1, 3)
    pts = pts[np.random.default_rng(5).permutation(pts.shape[0])]
    half = np.arange(8, dtype=F32) + F32(0.5)
    centres = np.stack(np.meshgrid(half, half, half, indexing='ij'), -1).reshape(-1, 3)
    q = np.concatenate([pts[::3], centres]).astype(F32)
    pts.setflags(write=False)
    q.setflags(write=False)
    return pts, q


@functools.lru_cache(maxsize=None)
def host_tree(n):
    return geometry.PointTree(cloud(n))


@functools.lru_cache(maxsize=None)
def _reference32(kind, count, n):
    q = lattice()[1] if kind == 'lattice' else queries(kind, count, n)
    pts = lattice()[0] if kind == 'lattice' else cloud(n)
    out = geometry._nearest_numpy(q, pts, 32, dtype=np.float32)
    for a in out:
        a.setflags(write=False)
    return out


def reference32(kind, count, n, k):
    """The definition in float32, (dist, index) of ``_nearest_numpy``: computed once with k = 32; the k smallest pairs are the first k of
    the 32 smallest (tests/test_point_cloud_cpu.py checks that on the definition itself)."""
    dist, index = _reference32(kind, count, n)
    return np.ascontiguousarray(dist[:, :k]), np.ascontiguousarray(index[:, :k])


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def unit_sphere(n=2000, seed=2):
    d = np.random.default_rng(seed).standard_normal((n, 3))
    return (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(F32)


def sym3(c6):
    c6 = np.asarray(c6, dtype=np.float64)
    return np.stack([c6[:, [0, 1, 2]], c6[:, [1, 3, 4]], c6[:, [2, 4, 5]]], 1)


def direct_covariance(points, index):
    """The covariance of the neighbours by NumPy's own sums (pairwise, not in neighbour order), float64 [n,6]; needs a full table."""
    nb = np.asarray(points, dtype=np.float64)[np.asarray(index, dtype=np.int64)]
    e = nb - nb.mean(1, keepdims=True)
    c = np.einsum('nki,nkj->nij', e, e) / nb.shape[1]
    return np.stack([c[:, 0, 0], c[:, 0, 1], c[:, 0, 2], c[:, 1, 1], c[:, 1, 2], c[:, 2, 2]], -1)


def angle_to(normal, reference):
    """Angle between unoriented directions [n,3], radians, from the cross product (accurate near 0)."""
    a, b = np.asarray(normal, dtype=np.float64), np.asarray(reference, dtype=np.float64)
    return np.arctan2(np.linalg.norm(np.cross(a, b), axis=1), np.abs((a * b).sum(1)))


class CloudAlignCase:
    """The target: 4 000 surface samples of the 702-vertex shape; the source: 500 of them under the inverse of a 12 degree rotation and a
    0.1 shift, so the true pose is a fixed point with rms 0.  The restatement's float64 and float32 runs per metric give the
    tolerance ``4 e32 + eps32 extent`` (tests/test_align_cpu.py)."""
    def __init__(self):
        verts, faces = bumpy_mesh()
        self.target = np.ascontiguousarray(geometry.sample_surface(verts, faces, 4000, seed=11)[0], dtype=F32)
        self.truth = similarity(1.0, 12.0, (0.1, 0.0, 0.0))
        pick = np.random.default_rng(4).permutation(4000)[:500]
        self.src = moved(self.target[pick], self.truth)
        self.extent = extent_of(self.target)
        self.normals = geometry.estimate_normals(self.target, 16)['normal']
        self.r64, self.e32, self.tol = {}, {}, {}
        for metric in ('point', 'plane'):
            nrm = self.normals if metric == 'plane' else None
            runs = [geometry._align_cloud_numpy(self.src, self.target, nrm, np.eye(4), metric, False, 12, 1e-6, None, 1.0, dtype=dt)
                    for dt in (np.float64, np.float32)]
            self.r64[metric] = runs[0]
            self.e32[metric] = float(np.abs(runs[1]['matrix'] - runs[0]['matrix']).max())
            self.tol[metric] = 4 * self.e32[metric] + EPS32 * self.extent


@functools.lru_cache(maxsize=None)
def align_case():
    return CloudAlignCase()
