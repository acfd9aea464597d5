"""The winding tree on the host: the NumPy restatements that are its definition (geometry._winding_tree_numpy, _winding_tree_query_numpy,
WindingTree on NumPy arrays) against the exact float64 sum (geometry._winding_numpy, pinned by test_winding_cpu.py).  No GPU needed.

Truncation is checked three ways, none of them tuned to what the tree gives: the derived bound (loose at beta = 2), the order of
convergence of one node (d^-4, and d^-3 without Q), and the classification of samples whose exact winding number is farther than 0.25
from the threshold."""
import functools

import numpy as np
import pytest

from invertavatar_amd import geometry
from test_winding_cpu import (CLOSED, EPS32, F32, LATTICES, mc_sphere, open_sphere, pushed_samples, shell, sphere, torus, two_spheres)


@functools.lru_cache(maxsize=None)
def mc48():
    _, _, _, _, v, f = mc_sphere(48, 0.8, (0.01, -0.02, 0.03))
    return v, f


MESHES = {'sphere': lambda: sphere(24, 48), 'torus': torus, 'open_sphere': open_sphere, 'shell': shell, 'two_spheres': two_spheres,
          'mc48': mc48}
CLOSED_MESHES = ('sphere', 'torus', 'shell', 'two_spheres', 'mc48')


@functools.lru_cache(maxsize=None)
def case(name):
    """(verts, faces, pushed samples, the exact float64 winding numbers and their sizes, the tree): computed once, left unchanged."""
    verts, faces = MESHES[name]()
    pts, _ = pushed_samples(verts, faces)
    w64, size = geometry._winding_numpy(pts, verts, faces)
    return verts, faces, pts, w64, size, geometry.WindingTree(verts, faces)


def curved_patch():
    """18 triangles on a lopsided paraboloid: one leaf whatever the sort does, with D, Q and the curvature all non-zero."""
    g = np.linspace(-1.0, 1.0, 4)
    x, y = np.meshgrid(g, g, indexing='ij')
    x, y = x + 0.15 * y * y, y * 0.8 + 0.1
    v = np.stack([x, y, 0.35 * x * x + 0.2 * y * y + 0.1 * x * y + 0.05 * x], -1).reshape(-1, 3)
    at = lambda i, j: i * 4 + j
    f = [t for i in range(3) for j in range(3) for t in ((at(i, j), at(i + 1, j), at(i + 1, j + 1)), (at(i, j), at(i + 1, j + 1), at(i, j + 1)))]
    return v.astype(F32), np.array(f)


# ------------------------------------------------------------------ the tree itself

def test_layout_is_the_kernels():
    from invertavatar_amd import hipops
    assert hipops.winding_tree_layout() == (hipops.WINDING_LEAF, hipops.WINDING_BRANCH, hipops.WINDING_ROW, hipops.WINDING_MAX_LEVELS)
    assert (geometry.WINDING_LEAF, geometry.WINDING_BRANCH) == (hipops.WINDING_LEAF, hipops.WINDING_BRANCH) == (32, 8)
    L, B = geometry.WINDING_LEAF, geometry.WINDING_BRANCH
    for n in (0, 1, L - 1, L, L + 1, L * B, L * B + 1, L * B * B + 3, 13324, 1 << 25):
        counts, total, nbytes = hipops.winding_tree_plan(n)
        assert counts == geometry._winding_levels(n) and total == sum(counts) and nbytes == 8 * hipops.WINDING_ROW * total, n
        assert (not counts and n == 0) or (counts[-1] == 1 and counts[0] == -(-n // L) and len(counts) <= hipops.WINDING_MAX_LEVELS)
    assert geometry._winding_levels(13324) == [417, 53, 7, 1]


def test_host_walk_is_depth_first_in_index_order_and_an_empty_subset_prunes():
    counts, seen = [9, 2, 1], []

    def visit(lvl, j, row, idx):
        seen.append((lvl, j, int(row), idx.tolist()))
        return idx[idx != 1] if (lvl, j) == (1, 0) else idx[:0] if (lvl, j) == (1, 1) else idx

    geometry._tree_walk(counts, np.array([0, 1]), visit)
    assert seen == ([(2, 0, 11, [0, 1]), (1, 0, 9, [0, 1])] + [(0, k, k, [0]) for k in range(8)] + [(1, 1, 10, [0, 1])])
    for nothing in (([], np.array([0])), (counts, np.zeros(0, dtype=np.int64))):
        geometry._tree_walk(*nothing, lambda *a: pytest.fail('nothing to walk'))


def test_order_is_the_stable_morton_sort_with_unusable_faces_last():
    verts, faces = sphere()
    nan_vert = np.concatenate([verts, [[np.nan, 0, 0]]]).astype(F32)
    extra = np.concatenate([[[0, 1, len(verts)]], faces[:5], [[-1, 2, 3]], faces[5:], [[3, 7, 7]], [[0, 1, 999]]])   # 3 unusable, 1 without area
    t = geometry._winding_tree_numpy(nan_vert, extra)
    f = extra.shape[0]
    assert t['usable'] == f - 3 and sorted(t['order'].tolist()) == list(range(f))
    assert t['order'][-3:].tolist() == [0, 6, f - 1]                                        # unusable: last, by face index
    tri = nan_vert[extra[t['order'][:t['usable']]]]
    assert np.array_equal(tri, t['tris'])
    lo, scale = t['lo'], t['scale']
    assert np.array_equal(lo, verts.min(0)) and scale == F32(1024) / (verts.max(0) - verts.min(0)).max()
    cen = ((tri[:, 0] + tri[:, 1]) + tri[:, 2]) * (F32(1) / F32(3))
    cell = np.clip(np.floor((cen - lo) * scale), 0, 1023).astype(np.int64)
    keys = np.zeros(len(cell), dtype=np.int64)
    for b in range(10):                                                                     # bit by bit: x lowest
        for a in range(3):
            keys |= ((cell[:, a] >> b) & 1) << (3 * b + a)
    assert (np.diff(keys) >= 0).all() and keys.max() < 1 << 30
    same = np.flatnonzero(np.diff(keys) == 0)
    assert (t['order'][same] < t['order'][same + 1]).all()                                  # ties by face index
    # a permuted face list gives the same sorted triangles wherever the keys differ: the same multiset per key
    assert geometry._winding_tree_numpy(verts, faces[:0])['counts'] == [] and geometry.WindingTree(verts, faces[:0]).info['nodes'] == 0


@pytest.mark.parametrize('name', ['sphere', 'open_sphere', 'mc48'])
def test_nodes_are_the_moments_of_their_faces(name):
    """Every node against a direct float64 evaluation over ALL the faces under it (the upper nodes are built from their children)."""
    verts, faces, _, _, _, tree = case(name)
    t = tree.tris.astype(np.float64)
    L, B = geometry.WINDING_LEAF, geometry.WINDING_BRANCH
    an = 0.5 * np.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0])
    area, ct = np.linalg.norm(an, axis=1), t.mean(1)
    extent = float(np.abs(verts).max())
    start, span = 0, L
    for lvl, count in enumerate(tree.counts):
        for j in range(count):
            sl = slice(j * span, min((j + 1) * span, tree.usable))
            row = tree.nodes64[start + j]
            A = area[sl].sum()
            c = (ct[sl] * area[sl, None]).sum(0) / A
            assert abs(row[7] - A) <= 1e-12 * A and np.abs(row[:3] - c).max() <= 1e-12 * extent
            assert np.abs(row[4:7] - an[sl].sum(0)).max() <= 1e-12 * A
            r = np.linalg.norm(t[sl].reshape(-1, 3) - c, axis=1).max()
            assert row[3] >= r * (1 - 1e-12) and (lvl > 0 or row[3] <= r * (1 + 1e-12))    # an upper radius is an upper bound
            Q = ((ct[sl] - c)[:, :, None] * an[sl][:, None, :]).sum(0)
            assert np.abs(row[8:17].reshape(3, 3) - Q).max() <= 1e-12 * A * row[3]
        start, span = start + count, span * B
    assert tree.nodes.dtype == np.float32 and np.array_equal(tree.nodes, tree.nodes64.astype(F32))
    assert tree.info == {'faces': faces.shape[0], 'usable': faces.shape[0], 'levels': len(tree.counts), 'nodes': sum(tree.counts), 'leaf': L,
                         'branch': B}


def test_faces_without_area():
    verts = np.array([(0, 0, 0), (1, 0, 0), (2, 0, 0), (0, 1, 0)], dtype=F32)
    tree = geometry.WindingTree(verts, np.array([(0, 1, 2), (1, 1, 1)]))                    # no area at all: the mean of the centroids
    assert tree.counts == [1] and np.array_equal(tree.nodes64[0, :3], [(1 + 1) / 2, 0, 0]) and not tree.nodes64[0, 4:17].any()
    assert tree.nodes64[0, 3] == 1.0
    pts = np.array([(0.3, 0.2, 0.5), (9, 9, 9)], dtype=F32)
    assert np.array_equal(tree.query(pts), np.zeros(2))
    mixed = np.array([(0, 1, 2), (0, 1, 3)])
    w = geometry.winding_number(pts, verts, mixed, method='tree')
    assert np.abs(w - geometry.winding_number(pts, verts, mixed)).max() <= 1e-3 and w[0] != 0


# ------------------------------------------------------------------ truncation

@pytest.mark.parametrize('beta', [2.0, 4.0])
@pytest.mark.parametrize('name', sorted(MESHES))
def test_truncation_is_under_the_derived_bound(name, beta):
    verts, faces, pts, w64, _, tree = case(name)
    w, bound, counts = tree.query(pts, beta, return_bound=True, return_counts=True)
    err = np.abs(w - w64)
    print(f'{name} F = {faces.shape[0]} beta = {beta}: largest error {err.max():.3g}, bound {bound.min():.3g} .. {bound.max():.3g}, '
          f'far terms {counts[:, 0].mean():.1f}, exact pairs {counts[:, 1].mean():.1f} per point')
    assert w.dtype == np.float64 and bound.dtype == np.float64 and (bound >= 0).all()
    assert (err <= bound + 1e-9).all()
    assert ((counts[:, 0] > 0) == (bound > 0)).all() and (counts[:, 1] <= faces.shape[0]).all()


def test_one_node_converges_with_the_fourth_power_of_the_distance():
    """The remainder of the degree-1 expansion is d^-4: the error at d = 8 r, 16 r, 32 r, 64 r falls by 16 per doubling (ratios within
    [12, 20]) and stays under the bound; the same node without Q falls by 8 only and breaks the bound at 64 r."""
    verts, faces = curved_patch()
    assert faces.shape[0] <= geometry.WINDING_LEAF
    tree = geometry.WindingTree(verts, faces)
    assert tree.counts == [1] and np.abs(tree.nodes[0, 8:17]).max() > 1e-3 * tree.nodes[0, 7] * tree.nodes[0, 3]
    c, r = tree.nodes64[0, :3], tree.nodes64[0, 3]
    direction = np.array([0.3, -0.5, 0.8]) / np.linalg.norm([0.3, -0.5, 0.8])
    pts = (c + np.array([8.0, 16.0, 32.0, 64.0])[:, None] * r * direction).astype(F32)
    w64 = geometry._winding_numpy(pts, verts, faces)[0]
    w, bound, _, far, pairs = geometry._winding_tree_query_numpy(pts, tree.tris, tree.nodes, tree.counts, 2.0)
    assert (far == 1).all() and (pairs == 0).all()
    err = np.abs(w - w64)
    ratios = err[:-1] / err[1:]
    dropped = np.abs(geometry._winding_tree_query_numpy(pts, tree.tris, tree.nodes, tree.counts, 2.0, use_q=False)[0] - w64)
    print('error', err, 'bound', bound, 'ratios', ratios, 'without Q', dropped, 'ratios', dropped[:-1] / dropped[1:])
    assert (err <= bound).all()
    assert ((ratios >= 12) & (ratios <= 20)).all()
    assert dropped[-1] > bound[-1]


@pytest.mark.parametrize('name', sorted(MESHES))
def test_beta_inf_is_the_exact_sum_in_another_order(name):
    verts, faces, pts, w64, size, tree = case(name)
    w32 = geometry._winding_numpy(pts, verts, faces, F32)[0]
    e32 = float(np.abs(w32 - w64).max())
    tol = 4 * e32 + EPS32 * np.maximum(1.0, size)
    w, bound, counts = tree.query(pts, np.inf, return_bound=True, return_counts=True)
    assert not bound.any() and not counts[:, 0].any() and (counts[:, 1] == faces.shape[0]).all()
    t32 = geometry._winding_tree_query_numpy(pts, tree.tris, tree.nodes, tree.counts, np.inf, F32)[0]
    print(f'{name}: e32 = {e32:.3g}, float64 terms {np.abs(w - w64).max():.3g}, float32 terms {np.abs(t32 - w64).max():.3g}')
    assert (np.abs(w - w64) <= tol).all() and (np.abs(t32 - w64) <= tol).all()


@pytest.mark.parametrize('name', sorted(MESHES))
def test_classification_at_beta_2_is_the_exact_one(name):
    verts, faces, pts, w64, _, tree = case(name)
    assert (np.abs(w64 - 0.5) > 0.25).all()                                                 # a condition of the inputs
    w = tree.query(pts, 2.0)
    assert np.array_equal(w >= 0.5, w64 >= 0.5)
    assert np.array_equal(geometry.inside(pts, verts, faces, method='tree', tree=tree), w64 >= 0.5)


# ------------------------------------------------------------------ purity, defaults, errors

def test_value_is_a_pure_function_of_point_mesh_and_beta():
    verts, faces, pts, _, _, tree = case('sphere')
    pts = np.concatenate([pts[:150], np.random.default_rng(0).uniform(-1.5, 1.5, (50, 3)).astype(F32), [[np.nan, 0, 0]], [[0, np.inf, 0]]])
    for dtype in (np.float64, F32):
        w, b = geometry._winding_tree_query_numpy(pts, tree.tris, tree.nodes, tree.counts, 2.0, dtype)[:2]
        assert np.isnan(w[-2:]).all() and np.isnan(b[-2:]).all() and np.isfinite(w[:-2]).all()
        perm = np.random.default_rng(1).permutation(pts.shape[0])
        wp, bp = geometry._winding_tree_query_numpy(pts[perm], tree.tris, tree.nodes, tree.counts, 2.0, dtype)[:2]
        assert np.array_equal(wp, w[perm], equal_nan=True) and np.array_equal(bp, b[perm], equal_nan=True)
        sub = np.sort(np.random.default_rng(2).choice(pts.shape[0], 37, replace=False))
        assert np.array_equal(geometry._winding_tree_query_numpy(pts[sub], tree.tris, tree.nodes, tree.counts, 2.0, dtype)[0], w[sub], equal_nan=True)
    a = geometry.winding_number(pts.reshape(2, -1, 3), verts, faces, method='tree')          # builds its own tree: the same bits
    assert a.shape == (2, pts.shape[0] // 2) and np.array_equal(a.reshape(-1), tree.query(pts), equal_nan=True)


def test_defaults_are_the_exact_sum():
    verts, faces, pts, w64, _, tree = case('torus')
    assert np.array_equal(geometry.winding_number(pts, verts, faces), w64)
    assert np.array_equal(geometry.winding_number(pts, verts, faces, method='exact', beta=7.0, tree=tree), w64)
    w, bound = geometry.winding_number(pts, verts, faces, return_bound=True)
    assert np.array_equal(w, w64) and bound.shape == w.shape and not bound.any()
    assert np.array_equal(geometry.inside(pts, verts, faces), w64 >= 0.5)
    r, c = geometry.signed_distance(pts, verts, faces), geometry.closest_point(pts, verts, faces)
    assert np.array_equal(r['winding'], w64) and np.array_equal(r['sdf'], np.where(w64 >= 0.5, -c['dist'], c['dist']))
    t = geometry.signed_distance(pts, verts, faces, method='tree', tree=tree)
    assert np.array_equal(t['winding'], tree.query(pts)) and np.array_equal(t['sdf'], r['sdf']) and np.array_equal(t['dist'], r['dist'])
    import torch
    wt = geometry.winding_number(torch.from_numpy(pts), torch.from_numpy(verts), torch.from_numpy(faces), method='tree')
    assert isinstance(wt, torch.Tensor) and wt.dtype == torch.float64 and np.array_equal(wt.numpy(), tree.query(pts))


def test_argument_errors():
    verts, faces, pts, _, _, tree = case('torus')
    for beta in (1.0, 0.5, -2.0, 0.0, np.nan, -np.inf, 1.0 + 1e-9, None, 'two'):                # (1 + 1e-9 is 1 as float32)
        with pytest.raises(ValueError):
            geometry.winding_number(pts, verts, faces, method='tree', beta=beta)
        with pytest.raises(ValueError):
            tree.query(pts, beta)
        with pytest.raises(ValueError):
            geometry.mesh_to_volume(verts, faces, 8, winding='tree', beta=beta)
    for method in ('fast', None, 'Tree'):
        with pytest.raises(ValueError):
            geometry.winding_number(pts, verts, faces, method=method)
        with pytest.raises(ValueError):
            geometry.signed_distance(pts, verts, faces, method=method)
        with pytest.raises(ValueError):
            geometry.mesh_to_volume(verts, faces, 8, winding=method)
        with pytest.raises(ValueError):
            geometry.surface_distance(verts, faces, verts, faces, winding=method)
    with pytest.raises(ValueError):
        geometry.winding_number(pts, verts, faces, method='tree', tree=(verts, faces))
    with pytest.raises(ValueError):
        geometry.WindingTree(verts[:, :2], faces)
    with pytest.raises(ValueError):
        geometry.volume_iou(verts, faces, verts, faces, resolution=8, winding='octree')
    assert np.isfinite(geometry.winding_number(pts, verts, faces, method='tree', beta=1.5)).all()


# ------------------------------------------------------------------ the functions made of it

@pytest.mark.parametrize('lattice', sorted(LATTICES))
@pytest.mark.parametrize('name', sorted(CLOSED))
def test_mesh_to_volume_with_the_tree_gives_the_same_volume(name, lattice):
    verts, faces = CLOSED[name]()
    kw = dict(LATTICES[lattice])
    if lattice == 'cubic':
        kw['resolution'] = 24
    sign = 'winding' if lattice == 'cubic' else 'regions'                                   # (exact regions = exact winding: test_winding_cpu)
    a = geometry.mesh_to_volume(verts, faces, sign='winding', winding='exact', **kw)
    b = geometry.mesh_to_volume(verts, faces, sign=sign, winding='tree', **kw)
    assert a['info']['winding'] == 'exact' and b['info']['winding'] == 'tree' and b['info']['mode'] == sign
    assert b['info']['evaluations'] == (a['inside'].size if sign == 'winding' else b['info']['regions'] + b['info']['band'])
    assert np.array_equal(a['inside'], b['inside']) and np.array_equal(a['sdf'].view(np.int32), b['sdf'].view(np.int32))


def test_volume_iou_and_surface_distance_with_the_tree():
    big, faces = sphere(12, 16, 1.05)
    unit, _ = sphere(12, 16)
    exact = geometry.volume_iou(big, faces, unit, faces, resolution=16, sign='winding')
    assert geometry.volume_iou(big, faces, unit, faces, resolution=16, sign='winding', winding='tree', beta=2.0) == exact
    plain = geometry.surface_distance(big, faces, unit, faces, signed=True)
    res = geometry.surface_distance(big, faces, unit, faces, signed=True, winding='tree')
    assert res == plain and res['inside_share_ab'] == 0.0 and res['inside_share_ba'] == 1.0
    assert geometry.surface_distance(big, faces, unit, faces, winding='tree') == geometry.surface_distance(big, faces, unit, faces)


def test_cli_takes_the_tree(tmp_path):
    from invertavatar_amd import geometry_metrics
    big, faces = sphere(8, 12, 1.05)
    unit, _ = sphere(8, 12)
    geometry.write_ply(str(tmp_path / 'a.ply'), big, faces)
    geometry.write_ply(str(tmp_path / 'b.ply'), unit, faces)
    base = ['--pred', str(tmp_path / 'a.ply'), '--gt', str(tmp_path / 'b.ply'), '--device', 'cpu', '--signed', '--iou', '16']
    exact = geometry_metrics.main(base + ['--out', str(tmp_path / 'e.json'), '--error-ply', str(tmp_path / 'e.ply')])
    tree = geometry_metrics.main(base + ['--out', str(tmp_path / 't.json'), '--error-ply', str(tmp_path / 't.ply'), '--winding', 'tree',
                                         '--winding-beta', '3'])
    assert 'winding' not in exact and tree.pop('winding') == {'method': 'tree', 'beta': 3.0}
    assert tree == exact
    assert np.array_equal(geometry.read_ply(str(tmp_path / 't.ply'))[2], geometry.read_ply(str(tmp_path / 'e.ply'))[2])
    with pytest.raises(SystemExit):
        geometry_metrics.main(base + ['--out', str(tmp_path / 'x.json'), '--winding', 'octree'])
