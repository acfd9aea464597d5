"""Meshes and linear systems shared by test_nonrigid_cpu.py and test_nonrigid_gpu.py (no tests here)."""
import functools

import numpy as np

from invertavatar_amd import geometry

F32 = np.float32
EPS64 = float(np.finfo(np.float64).eps)
EPS32 = float(np.finfo(np.float32).eps)


@functools.lru_cache(maxsize=None)
def sphere(level):
    """A unit icosahedron subdivided ``level`` times (12, 42, 162, 642 vertices): (verts float32 [V,3], faces int64 [F,3])."""
    t = (1 + 5 ** 0.5) / 2
    v = np.array([[-1, t, 0], [1, t, 0], [-1, -t, 0], [1, -t, 0], [0, -1, t], [0, 1, t], [0, -1, -t], [0, 1, -t], [t, 0, -1], [t, 0, 1],
                  [-t, 0, -1], [-t, 0, 1]], dtype=np.float64)
    f = np.array([[0, 11, 5], [0, 5, 1], [0, 1, 7], [0, 7, 10], [0, 10, 11], [1, 5, 9], [5, 11, 4], [11, 10, 2], [10, 7, 6], [7, 1, 8],
                  [3, 9, 4], [3, 4, 2], [3, 2, 6], [3, 6, 8], [3, 8, 9], [4, 9, 5], [2, 4, 11], [6, 2, 10], [8, 6, 7], [9, 8, 1]])
    v /= np.linalg.norm(v, axis=1)[:, None]
    for _ in range(level):
        rows, new, cache = list(v), [], {}

        def mid(a, b):
            k = (min(a, b), max(a, b))
            if k not in cache:
                m = (rows[a] + rows[b]) / 2
                cache[k] = len(rows)
                rows.append(m / np.linalg.norm(m))
            return cache[k]
        for a, b, c in f:
            ab, bc, ca = mid(a, b), mid(b, c), mid(c, a)
            new += [[a, ab, ca], [b, bc, ab], [c, ca, bc], [ab, bc, ca]]
        v, f = np.array(rows), np.array(new)
    return v.astype(F32), f.astype(np.int64)


def bumped_ellipsoid(level=3):
    """The sphere with radii (1.0, 1.2, 0.85) and a smooth bump around +z: the target of the fit tests."""
    v, f = sphere(level)
    bump = 1.0 + 0.15 * np.exp(-((v.astype(np.float64) - [0.0, 0.0, 1.0]) ** 2).sum(1) / 0.1)
    return (v.astype(np.float64) * [1.0, 1.2, 0.85] * bump[:, None]).astype(F32), f


def strip(n, seed=0):
    """A triangle strip over ``n`` random vertices (n >= 3), every vertex of degree <= 4."""
    v = np.random.RandomState(seed).randn(n, 3).astype(F32)
    f = np.stack([np.arange(n - 2), np.arange(1, n - 1), np.arange(2, n)], 1).astype(np.int64)
    return v, f


def fan(spokes=300, seed=0):
    """A hub (vertex 0) with ``spokes`` neighbours: the heavy-degree path of the operator."""
    v = np.random.RandomState(seed).randn(spokes + 1, 3).astype(F32)
    k = np.arange(spokes)
    f = np.stack([np.zeros(spokes, dtype=np.int64), 1 + k, 1 + (k + 1) % spokes], 1).astype(np.int64)
    return v, f


def mesh(name):
    """The meshes of the solver cases by name -> (verts, faces)."""
    if name == 'v1':
        return np.array([[0.25, -0.5, 1.0]], dtype=F32), np.array([[0, 0, 0]], dtype=np.int64)
    if name == 'v2':
        return np.array([[0.25, -0.5, 1.0], [1.0, 0.0, 0.5]], dtype=F32), np.array([[0, 1, 1]], dtype=np.int64)
    if name.startswith('strip'):
        return strip(int(name[5:]))
    if name == 'sphere642':
        return sphere(3)
    if name == 'fan':
        return fan()
    if name == 'isolated':                                                # vertices 40.. have no face; two faces are unusable
        v, f = strip(40, 3)
        v = np.concatenate([v, np.random.RandomState(4).randn(7, 3).astype(F32)])
        return v, np.concatenate([f, [[1, 1, 5], [2, 9, 2]]]).astype(np.int64)
    if name == 'nonfinite':                                               # vertex 11 is not finite: pinned, its faces unusable
        v, f = sphere(1)
        v = v.copy()
        v[11, 1] = np.nan
        return v, f
    raise KeyError(name)


def system(verts, faces, metric, seed, stiffness=0.05, share=0.1):
    """A random system on the mesh: weights in {0, 1}, random offsets, unit normals (plane), pins and landmarks."""
    rng = np.random.RandomState(seed)
    nv = verts.shape[0]
    c = (rng.rand(nv) < 0.8).astype(np.float64)
    c[0] = 1.0
    t = rng.randn(nv, 3)
    n = None
    if metric == 'plane':
        n = rng.randn(nv, 3)
        n /= np.linalg.norm(n, axis=1)[:, None]
    pinned = ~np.isfinite(verts).all(1)
    if nv > 8:
        pinned[rng.choice(nv, max(nv // 16, 1), replace=False)] = True
    k = min(max(nv // 10, 1), nv)
    idx = rng.choice(nv, k, replace=False)
    return {'c': c, 't': t, 'n': n, 'pinned': pinned, 'landmarks': (idx, rng.randn(k, 3), 0.5 + rng.rand(k)), 'stiffness': float(stiffness),
            'share': float(share), 'x0': 0.1 * rng.randn(nv, 3)}


def dense(adj, s):
    """The 3V x 3V matrix and the right-hand side of ``system`` written out from the definition (a pinned row is the identity)."""
    nv = s['c'].shape[0]
    off, nbr = np.asarray(adj.offsets).astype(np.int64), np.asarray(adj.neighbors).astype(np.int64)
    A, b = np.zeros((3 * nv, 3 * nv)), np.zeros(3 * nv)
    beta, land = np.zeros(nv), np.zeros((nv, 3))
    if s['landmarks'] is not None:
        beta[s['landmarks'][0]] = s['landmarks'][2]
        land[s['landmarks'][0]] = s['landmarks'][1]
    eye = np.eye(3)
    for i in range(nv):
        sl = slice(3 * i, 3 * i + 3)
        if s['pinned'][i]:
            A[sl, sl] = eye
            continue
        C = s['c'][i] * (eye if s['n'] is None else np.outer(s['n'][i], s['n'][i]) + s['share'] * eye)
        js = nbr[off[i]:off[i + 1]]
        A[sl, sl] = C + (s['stiffness'] * js.size + beta[i]) * eye
        for j in js:
            if not s['pinned'][j]:
                A[sl, 3 * j:3 * j + 3] -= s['stiffness'] * eye
        b[sl] = C @ s['t'][i] + beta[i] * land[i]
    return A, b


def solve(adj, s, cg_iterations, cg_tol, **more):
    return geometry.nonrigid_solve(adj, s['c'], s['t'], s['stiffness'], normals=s['n'], point_share=s['share'], pinned=s['pinned'],
                                   landmarks=s['landmarks'], x0=s['x0'], cg_iterations=cg_iterations, cg_tol=cg_tol, **more)


def restated(adj, s, cg_iterations, cg_tol, reverse=False, trace=None):
    """The restatement's solve from its parts (``reverse``: neighbour sums and dot products in the reverse order) -> (x, steps)."""
    nv = s['c'].shape[0]
    beta, land = np.zeros(nv), np.zeros((nv, 3))
    beta[s['landmarks'][0]] = s['landmarks'][2]
    land[s['landmarks'][0]] = s['landmarks'][1]
    b = geometry._nonrigid_rhs_numpy(s['c'], s['t'], s['n'], s['share'], beta, land, s['pinned'])
    op = geometry._nonrigid_operator(adj._state, s['c'], s['n'], s['share'], beta, s['pinned'], s['stiffness'], reverse=reverse)
    x, steps = geometry._nonrigid_cg_numpy(op, b, s['x0'], s['pinned'], cg_iterations, cg_tol, reverse=reverse, trace=trace)[:2]
    return x, steps


def early_tolerance(trace, last=5):
    """``safe_tolerance`` for the first such step among the first ``last``: a freeze a few roundings from the start."""
    for k in range(1, min(last + 1, len(trace))):
        before = min(trace[:k])
        if before > 0 and before >= 16.0 * trace[k]:
            return float(np.sqrt(np.sqrt(before * trace[k]))), k
    return None


def safe_tolerance(trace, floor=1e-24):
    """``(cg_tol, step)``: a tolerance at which the solve freezes after ``step`` steps with a margin of 4 in |r|^2 / |b|^2 on both
    sides (every earlier ratio >= 4 cg_tol^2, the freezing one <= cg_tol^2 / 4), the latest such step whose ratio is above ``floor``
    (where the recurrence still follows the residual), else the first such step at all (a system solved exactly in a step or two), or
    None if the trace has no such step."""
    found = first = None
    for k in range(1, len(trace)):
        before = min(trace[:k])
        if before > 0 and before >= 16.0 * trace[k]:
            first = first or (float(np.sqrt(np.sqrt(before * trace[k]))), k)
            if trace[k] > floor:
                found = (float(np.sqrt(np.sqrt(before * trace[k]))), k)
    return found or first
