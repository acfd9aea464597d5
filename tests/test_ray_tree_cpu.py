"""Rays against the mesh on the cluster tree, on the host: the restatement of the walk ``geometry._ray_tree_numpy``
against the definition ``geometry._ray_mesh_numpy``.  The tree only prunes, so the comparisons are exact; the one tolerance, float32
against float64, is stated where it is used.  The meshes are those of test_closest_tree_cpu.py."""
import functools

import numpy as np
import pytest
import torch

from invertavatar_amd import geometry
from test_closest_tree_cpu import CENTRE, FACE_COUNTS, cut, mc48, same_bits, tree_of
from test_winding_cpu import F32, pushed_samples, torus

L, B = geometry.WINDING_LEAF, geometry.WINDING_BRANCH
INSIDE = (0.31, -0.22, 0.27)                 # an inside point well off the centre of the sphere of radius 0.8 about CENTRE
FIELDS = ('hit', 't', 'face', 'bary', 'point')
INWARD = ('far', 'far50', 'far30', 'far20', 'far10', 'far2')
T32_BOUND = 4 * 2.28e-7                      # test 5: four times the largest |t32 - t64| observed on the host


def _thin(a, most):
    return a[::max(1, -(-a.shape[0] // most))]


@functools.lru_cache(maxsize=None)
def rays(n):
    """(origins, dirs float32 [N,3], t_lo, t_hi float32 [N], families: name -> slice) for the mesh ``cut(n)``."""
    verts, faces = cut(n)
    full_v, full_f = mc48()
    rs = np.random.RandomState(11)
    pushed, _ = pushed_samples(full_v, full_f, 48 if n is None else 12)
    used = faces[(faces >= 0).all(1)]
    own = _thin(verts[np.unique(used)], 240) if used.size else np.zeros((0, 3), dtype=F32)
    tri = _thin(verts[used], 80).astype(np.float64) if used.size else np.zeros((0, 3, 3))
    mids = ((tri + np.roll(tri, 1, axis=1)) * 0.5).reshape(-1, 3).astype(F32)
    targets = np.concatenate([pushed, own, mids]).astype(F32)
    extent = float(np.abs(full_v).max())
    lo, hi = full_v.min(0), full_v.max(0)
    fam, parts = {}, []

    def add(name, o, d, t_lo=0.0, t_hi=np.inf):
        o = np.broadcast_to(np.asarray(o, dtype=F32), np.asarray(d).shape)
        k = o.shape[0]
        at = sum(p[0].shape[0] for p in parts)
        fam[name] = slice(at, at + k)
        parts.append((o, np.asarray(d, dtype=F32), np.broadcast_to(np.asarray(t_lo, dtype=F32), (k,)), np.broadcast_to(np.asarray(t_hi, dtype=F32), (k,))))

    c32, in32 = np.array(CENTRE, dtype=F32), np.array(INSIDE, dtype=F32)
    add('centre', c32, targets - c32)
    add('inside', in32, targets - in32)
    unit = rs.standard_normal((targets.shape[0], 3))
    for k in (100, 50, 30, 20, 10, 2):                                                     # from k extents away, inwards
        far = (k * extent * unit / np.linalg.norm(unit, axis=1, keepdims=True)).astype(F32)
        sub = slice(None) if k == 100 else slice(k % 7, None, 3)
        add('far' if k == 100 else f'far{k}', far[sub], targets[sub] - far[sub])
    # axis-parallel: two components exactly 0; the other two coordinates from the vertices, so that many rays lie in the planes of
    # box faces (a box face sits at a vertex coordinate) and, on this marching-cubes mesh, in the lattice planes its edges lie in
    pick = _thin(full_v, 60)
    ax_o, ax_d = [], []
    for k in range(3):
        for sgn in (1.0, -1.0):
            o = pick.copy()
            o[:, k] = -sgn * 3.0
            d = np.zeros_like(o)
            d[:, k] = sgn
            ax_o.append(o)
            ax_d.append(d)
    planes = np.array([(-3.0, hi[1], lo[2]), (-3.0, lo[1], 0.25), (-3.0, hi[1] + 1e-3, 0.0)], dtype=F32)       # the mesh box's own faces
    ax_o.append(planes)
    ax_d.append(np.tile(np.array([(1.0, 0.0, 0.0)], dtype=F32), (3, 1)))
    add('axis', np.concatenate(ax_o), np.concatenate(ax_d))
    # rays that miss the mesh's box: parallel to a face at a clear distance, and pointing away from it
    out = (np.array(CENTRE) + 3.0 * unit[:40] / np.linalg.norm(unit[:40], axis=1, keepdims=True)).astype(F32)
    add('miss', np.concatenate([out, pick[:40] + np.array([0.0, 0.0, 2.5], dtype=F32)]),
        np.concatenate([out - c32, np.tile(np.array([(1.0, 0.5, 0.0)], dtype=F32), (40, 1))]))
    # origins exactly on a vertex
    if own.shape[0]:
        onv = _thin(own, 60)
        add('on_vertex', np.concatenate([onv, onv]), np.concatenate([onv - c32, c32 - onv]))
    # per-ray intervals on rays through the sphere, d = CENTRE - o (hits near t = 0.73 and t = 1.27 on the full mesh)
    thru = (np.array(CENTRE) + 3.0 * unit[40:100] / np.linalg.norm(unit[40:100], axis=1, keepdims=True)).astype(F32)
    add('second', thru, c32 - thru, 1.0, 2.0)
    add('between', thru, c32 - thru, 0.9, 1.1)
    add('first_only', thru, c32 - thru, 0.0, 1.0)
    add('negative', thru, thru - c32, -np.inf, 0.0)
    add('zero', pick[:8], np.zeros((8, 3), dtype=F32))
    add('bad', np.array([(np.nan, 0.0, 0.0), (0.0, 0.0, 0.0), (0.0, 0.0, 0.0)], dtype=F32),
        np.array([(1.0, 0.0, 0.0), (np.inf, 0.0, 0.0), (1.0, 0.0, 0.0)], dtype=F32), 0.0, np.array([np.inf, np.inf, np.nan], dtype=F32))
    o, d, t_lo, t_hi = (np.ascontiguousarray(np.concatenate([p[i] for p in parts])) for i in range(4))
    return o, d, t_lo, t_hi, fam


@functools.lru_cache(maxsize=None)
def brute(n, dtype):
    o, d, t_lo, t_hi, _ = rays(n)
    return geometry._ray_mesh_numpy(o, d, *cut(n), t_lo, t_hi, dtype)


@functools.lru_cache(maxsize=None)
def by_tree(n, dtype, mode='first'):
    o, d, t_lo, t_hi, _ = rays(n)
    return geometry._ray_tree_numpy(o, d, tree_of(n), t_lo, t_hi, mode, dtype)


def assert_same(got, want, what=''):
    for k, name in enumerate(FIELDS):
        g, w = np.asarray(got[k]), np.asarray(want[k])
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name)
        if g.dtype.kind == 'f':
            assert np.array_equal(np.isnan(g), np.isnan(w)), (what, name, 'NaN pattern')
            assert same_bits(np.where(np.isnan(g), 0, g), np.where(np.isnan(w), 0, w)), (what, name)
        else:
            assert np.array_equal(g, w), (what, name)


# ------------------------------------------------------------------ 1. the walk is the definition

@pytest.mark.parametrize('dtype', [np.float64, np.float32], ids=['f64', 'f32'])
@pytest.mark.parametrize('n', FACE_COUNTS)
def test_tree_equals_brute_exactly(n, dtype):
    o, d, t_lo, t_hi, fam = rays(n)
    got, want = by_tree(n, dtype), brute(n, dtype)
    assert_same(got, want, f'F = {n}')
    hit, t, face, bary, point = want
    assert not hit[fam['bad']].any() and np.isnan(t[fam['bad']]).all() and (face[fam['bad']] == -1).all()
    assert not hit[fam['zero']].any() and np.isinf(t[fam['zero']]).all()                               # d = 0: the definition rejects every triangle
    assert not hit[fam['miss']].any() and not hit[fam['between']].any()
    assert np.isinf(t[~hit & ~np.isnan(t)]).all() and (face[~hit] == -1).all() and np.isnan(bary[~hit]).all() and np.isnan(point[~hit]).all()
    assert (face[hit] >= 0).all() and (t[hit] >= t_lo[hit]).all() and (t[hit] <= t_hi[hit]).all()
    usable = tree_of(n).usable
    if not usable:
        assert not hit.any()
    if n is None:
        for name in fam:
            print(f'{name}: {int(hit[fam[name]].sum())} of {fam[name].stop - fam[name].start} rays hit')
        thru = slice(fam['second'].start, fam['first_only'].stop)
        assert hit[fam['second']].all() and hit[fam['first_only']].all() and hit[fam['negative']].all()   # (through the middle: well inside faces)
        assert (t[fam['second']] > 1.2).all() and (t[fam['first_only']] < 0.8).all() and (t[fam['negative']] < -0.7).all()
        assert hit[thru].sum() == 120
        if 'on_vertex' in fam:
            assert (t[fam['on_vertex']][hit[fam['on_vertex']]] == 0).any()                             # a hit at the origin itself


@pytest.mark.parametrize('n', [L * B + 1, None])
def test_a_rays_result_is_its_own(n):
    o, d, t_lo, t_hi, _ = rays(n)
    sel = np.random.RandomState(5).permutation(o.shape[0])[:300]
    whole = by_tree(n, np.float32)
    part = geometry._ray_tree_numpy(o[sel], d[sel], tree_of(n), t_lo[sel], t_hi[sel], 'first', np.float32)
    for k in range(6):
        assert same_bits(part[k], whole[k][sel])
    empty = geometry._ray_tree_numpy(np.zeros((0, 3), dtype=F32), np.zeros((0, 3), dtype=F32), tree_of(n), dtype=np.float32)
    assert [x.shape for x in empty] == [(0,), (0,), (0,), (0, 3), (0, 3), (0, 2)]


# ------------------------------------------------------------------ 2. ties

def fan():
    """Six coplanar triangles around the vertex (0, 0, 1), input order scrambled."""
    ring = [(np.cos(a), np.sin(a), 1.0) for a in np.arange(6) * np.pi / 3]
    verts = np.array([(0.0, 0.0, 1.0)] + ring, dtype=F32)
    faces = np.array([(0, 1 + k, 1 + (k + 1) % 6) for k in (3, 0, 5, 2, 4, 1)], dtype=np.int64)
    return verts, faces


def test_ties_go_to_the_lowest_input_face():
    verts, faces = fan()
    o = np.array([(0.0, 0.0, 0.0), (0.0, 0.0, 3.0), (0.0, 0.0, 0.0)], dtype=F32)
    d = np.array([(0.0, 0.0, 1.0), (0.0, 0.0, -1.0), (0.5, 0.0, 1.0)], dtype=F32)       # through the hub twice, and along the edge hub - ring 0
    base = geometry._ray_mesh_numpy(o, d, verts, faces, dtype=np.float32)
    assert base[0].all() and (base[2][:2] == 0).all() and np.array_equal(base[1], np.array([1.0, 2.0, 1.0], dtype=F32))
    edge = sorted(i for i, f in enumerate(faces) if 1 in f)                               # the two faces that share the edge
    assert base[2][2] == edge[0]
    for seed in range(4):
        perm = np.random.RandomState(seed).permutation(6)
        got = geometry._ray_mesh_numpy(o, d, verts, faces[perm], dtype=np.float32)
        via = geometry._ray_tree_numpy(o, d, geometry.WindingTree(verts, faces[perm]), dtype=np.float32)
        assert_same(via, got)
        assert (got[2][:2] == 0).all() and got[2][2] == min(int(np.flatnonzero(perm == e)[0]) for e in edge)
        for k in (0, 1, 4):                                                               # hit, t, point: unchanged
            assert same_bits(got[k], base[k])
        hub = np.array([np.flatnonzero(f == 0)[0] for f in faces[perm][got[2]]])          # bary follows the winner's vertex order
        assert (got[3][np.arange(2), hub[:2]] == 1).all()


# ------------------------------------------------------------------ 3. any hit

@pytest.mark.parametrize('dtype', [np.float64, np.float32], ids=['f64', 'f32'])
@pytest.mark.parametrize('n', FACE_COUNTS)
def test_any_is_the_hit_of_first(n, dtype):
    got, first = by_tree(n, dtype, 'any'), brute(n, dtype)
    assert np.array_equal(got[0], first[0])
    assert (got[2] == -1).all() and np.isnan(got[3]).all() and np.isnan(got[4]).all()


# ------------------------------------------------------------------ 4. pruning is real

def test_skipping_cuts_the_pairs():
    """Mean pairs per ray over the centre, inside, axis-parallel and every inward family (2 to 100 extents away) <= F_usable / 4
    (a walk that never skips: F_usable)."""
    _, _, _, _, fam = rays(None)
    usable = tree_of(None).usable
    for mode in ('first', 'any'):
        counts = by_tree(None, np.float32, mode)[5]
        assert not counts[fam['bad']].any() and (counts[:, 1] <= usable).all()
        for name in ('centre', 'inside', 'axis', 'miss') + INWARD:
            c = counts[fam[name]]
            print(f'{mode} {name}: mean boxes {c[:, 0].mean():.1f}, mean pairs {c[:, 1].mean():.1f}, most pairs {c[:, 1].max()} of {usable}')
        for name in ('centre', 'inside', 'axis') + INWARD:
            assert counts[fam[name], 1].mean() <= usable / 4, name
    assert not by_tree(None, np.float32)[5][fam['miss'], 1].any()                          # outside the root's box: no pair at all


def test_every_hit_point_lies_in_its_triangles_grown_box():
    """What the skip test's proof uses: the exact point o + t d of every hit lies within slack / 2 = 2^-13 M of the
    box of the triangle that was hit, on every axis and in every family: ray_tri's last clause, with its rounding."""
    o, d, _, _, fam = rays(None)
    verts, faces = cut(None)
    hit, t, face, _, _ = brute(None, np.float32)
    tree = tree_of(None)
    for name, sl in fam.items():
        h = np.flatnonzero(hit[sl]) + sl.start
        if not h.size:
            continue
        tri = verts[faces[face[h]]].astype(np.float64)
        p = o[h].astype(np.float64) + t[h].astype(np.float64)[:, None] * d[h].astype(np.float64)
        gap = np.maximum(np.maximum(tri.min(1) - p, p - tri.max(1)), 0).max(1)
        big = np.maximum(np.abs(o[h]).max(1).astype(np.float64), tree.extent)
        ratio = gap / (2.0 ** -13 * big)
        print(f'{name}: {h.size} hits, largest gap {gap.max():.3g}, largest gap / (slack / 2) = {ratio.max():.3g}')
        assert ratio.max() <= 1, name


def test_tiny_and_huge_directions():
    """Directions scaled by 2^-120 and 2^+120 (t scales the other way; slab products near the subnormal range are not trusted)."""
    o, d, t_lo, t_hi, fam = rays(L * B * B + 3)
    sel = np.r_[fam['centre'], fam['far10'], fam['axis']][::3]
    tree, (verts, faces) = tree_of(L * B * B + 3), cut(L * B * B + 3)
    for scale in (2.0 ** -120, 2.0 ** 120, 2.0 ** -140):
        dd = (d[sel].astype(np.float64) * scale).astype(F32)
        got = geometry._ray_tree_numpy(o[sel], dd, tree, dtype=np.float32)
        assert_same(got, geometry._ray_mesh_numpy(o[sel], dd, verts, faces, dtype=np.float32), f'scale {scale}')
        print(f'scale {scale:.3g}: {int(got[0].sum())} of {sel.size} rays hit')


# ------------------------------------------------------------------ 5. float32 against float64

def test_float32_is_close_to_float64_on_well_conditioned_rays():
    verts, faces = mc48()
    cen = verts[faces].astype(np.float64).mean(1).astype(F32)[::7]
    c32 = np.array(CENTRE, dtype=F32)
    tree = geometry.WindingTree(verts, faces)
    org = np.broadcast_to(c32, cen.shape)
    r32 = geometry._ray_tree_numpy(org, cen - c32, tree, dtype=np.float32)
    r64 = geometry._ray_tree_numpy(org, cen - c32, tree, dtype=np.float64)
    assert r32[0].all() and r64[0].all() and np.array_equal(r32[2], r64[2])
    err = np.abs(r32[1].astype(np.float64) - r64[1]).max()
    print(f'{cen.shape[0]} rays: largest |t32 - t64| = {err:.3g} (t about 1)')
    assert err <= T32_BOUND


# ------------------------------------------------------------------ 6. the public interface and ambient occlusion

def test_ray_mesh_and_occluded_on_the_host():
    verts, faces = cut(L * B + 1)
    o, d, t_lo, t_hi, fam = rays(L * B + 1)
    want = brute(L * B + 1, np.float64)
    for got in (geometry.ray_mesh(o, d, verts, faces, t_lo, t_hi), geometry.ray_mesh(o, d, verts, faces, t_lo, t_hi, brute=True),
                geometry.ray_mesh(o, d, verts, faces, t_lo, t_hi, tree=tree_of(L * B + 1))):
        assert list(got) == list(FIELDS) and got['hit'].dtype == bool and got['face'].dtype == np.int64 and got['t'].dtype == F32
        for k, name in enumerate(FIELDS):
            assert np.array_equal(got[name], want[k].astype(got[name].dtype), equal_nan=True), name
    only = geometry.ray_mesh(o, d, verts, faces, t_lo, t_hi, mode='any')
    assert list(only) == ['hit'] and np.array_equal(only['hit'], want[0])
    tv, tf = torch.from_numpy(verts), torch.from_numpy(faces)
    k = o.shape[0] // 2 * 2
    got = geometry.ray_mesh(torch.from_numpy(o[:k]).reshape(2, -1, 3), torch.from_numpy(d[:k]).reshape(2, -1, 3), tv, tf,
                            torch.from_numpy(t_lo[:k]).reshape(2, -1), torch.from_numpy(t_hi[:k]).reshape(2, -1))
    assert isinstance(got['t'], torch.Tensor) and tuple(got['point'].shape) == (2, k // 2, 3) and got['hit'].dtype == torch.bool
    assert np.array_equal(got['face'].numpy().reshape(-1), want[2][:k])
    with pytest.raises(ValueError):
        geometry.ray_mesh(o, d, verts, faces, mode='all')
    with pytest.raises(ValueError):
        geometry.ray_mesh(o, d[:-1], verts, faces)
    full_v, full_f = mc48()
    c = np.array(CENTRE, dtype=F32)
    a = np.array([c + (1.5, 0, 0), c + (1.5, 0, 0), c, c + (0.79, 0.0, 0.0)], dtype=F32)
    b = np.array([c - (1.5, 0, 0), c + (1.5, 1.0, 0), c + (0.2, 0.1, 0), c + (0.81, 0.0, 0.0)], dtype=F32)
    tree = geometry.WindingTree(full_v, full_f)
    want = np.array([True, False, False, True])
    assert np.array_equal(geometry.occluded(a, b, full_v, full_f, tree=tree), want)
    assert np.array_equal(geometry.occluded(b, a, full_v, full_f, tree=tree), want)


def plates(h=0.5, half=40.0):
    """A triangle facing up around the origin and a larger parallel one at height h above it (its corners reach ``half`` and beyond)."""
    verts = np.array([(-1.0, -1.0, 0.0), (1.0, -1.0, 0.0), (0.0, 1.5, 0.0),
                      (-2 * half, -half, h), (2 * half, -half, h), (0.0, 3 * half, h)], dtype=F32)
    return verts, np.array([(0, 1, 2), (3, 4, 5)], dtype=np.int64)


def test_ambient_occlusion_on_the_host():
    verts, faces = plates()
    up = np.tile(np.array([(0.0, 0.0, 1.0)], dtype=F32), (3, 1))
    alone = geometry.ambient_occlusion(verts[:3], faces[:1], samples=32, normals=up)
    assert alone['samples'] == 32 and alone['ao'].dtype == F32 and alone['unoccluded'].dtype == np.int32
    assert (alone['ao'] == 1).all() and (alone['unoccluded'] == 32).all()
    computed = geometry.ambient_occlusion(verts[:3], faces[:1], samples=32)               # the normals of mesh_normals: the same
    assert np.array_equal(computed['unoccluded'], alone['unoccluded'])
    up6 = np.tile(up[:1], (6, 1))
    near = geometry.ambient_occlusion(verts, faces, samples=32, radius=0.4, normals=up6)
    assert (near['ao'][:3] == 1).all()                                                     # the cover is farther than the radius
    # under the middle of the cover every direction of the table reaches it: the lowest z against the cover's inscribed circle
    mid = np.concatenate([verts, np.zeros((1, 3), dtype=F32)])
    table = geometry._ao_table(32, 0)
    assert table.dtype == F32 and table.shape == (32, 3) and np.abs(np.linalg.norm(table.astype(np.float64), axis=1) - 1).max() < 1e-6
    reach = 0.5 * np.sqrt(1 - table[:, 2].astype(np.float64) ** 2) / table[:, 2]
    assert table[:, 2].min() > 0 and reach.max() < 30.0                                   # (the inscribed radius of the cover is above 30)
    covered = geometry.ambient_occlusion(mid, faces, samples=32, normals=np.tile(up[:1], (7, 1)))
    assert covered['unoccluded'][6] == 0 and covered['ao'][6] == 0 and (covered['unoccluded'][3:6] == 32).all()
    again = geometry.ambient_occlusion(mid, faces, samples=32, normals=np.tile(up[:1], (7, 1)))
    assert np.array_equal(again['unoccluded'], covered['unoccluded'])
    assert not np.array_equal(geometry._ao_table(32, 1), table) and np.array_equal(geometry._ao_table(32, 0), table)
    # a mesh that occludes itself in part, under a permutation of its faces
    sv, sf = torus()
    nrm = geometry.mesh_normals(sv, sf)
    a = geometry.ambient_occlusion(sv, sf, samples=8, normals=nrm, seed=3)
    perm = np.random.RandomState(2).permutation(sf.shape[0])
    b = geometry.ambient_occlusion(sv, sf[perm], samples=8, normals=nrm, seed=3)
    assert np.array_equal(a['unoccluded'], b['unoccluded']) and 0 <= a['unoccluded'].min() < a['unoccluded'].max() <= 8
    other = geometry.ambient_occlusion(sv, sf, samples=8, normals=nrm, seed=4)
    assert other['unoccluded'].shape == a['unoccluded'].shape
    with pytest.raises(ValueError):
        geometry.ambient_occlusion(sv, sf, samples=0)


def test_ao_rays_restatement():
    rs = np.random.RandomState(0)
    n = rs.standard_normal((50, 3))
    n = (n / np.linalg.norm(n, axis=1, keepdims=True)).astype(F32)
    n[:3] = [(0, 0, 1), (0, 0, -1), (1, 0, 0)]
    n[3] = (np.nan, 0, 1)
    p = rs.standard_normal((50, 3)).astype(F32)
    table = geometry._ao_table(16, 0)
    o, d = geometry._ao_rays_numpy(p, n, table, 0.01)
    assert o.shape == d.shape == (800, 3) and o.dtype == d.dtype == F32
    o, d = o.reshape(50, 16, 3), d.reshape(50, 16, 3)
    assert np.isnan(o[3]).all() and np.isnan(d[3]).all()
    ok = np.arange(50) != 3
    assert np.abs(np.linalg.norm(d[ok].astype(np.float64), axis=2) - 1).max() < 1e-5                    # an orthonormal frame
    assert np.abs((d[ok].astype(np.float64) * n[ok, None, :]).sum(2) - table[None, :, 2]).max() < 1e-5  # z is the normal's share
    assert np.abs(o[ok] - (p[ok] + F32(0.01) * n[ok])[:, None, :]).max() == 0


# ------------------------------------------------------------------ 7. the command line

def test_cli_ao(tmp_path):
    """``--ao 16`` writes the grey mesh and the JSON block; without it the files are those of a run that never heard of the option."""
    import json
    import os
    from invertavatar_amd import extract_geometry
    base = ['--seeds', '0', '--width', 'small', '--res', '16', '--level', '0', '--device', 'cpu', '--keep', 'largest', '--smooth', '2']
    plain, with_ao = tmp_path / 'plain', tmp_path / 'ao'
    (_, rough), = extract_geometry.main(base + ['--outdir', str(plain)])
    (_, out), = extract_geometry.main(base + ['--outdir', str(with_ao), '--ao', '16'])
    assert 'ambient_occlusion' not in rough and '--ao' in extract_geometry.__doc__
    before, after = sorted(os.listdir(plain)), sorted(os.listdir(with_ao))
    assert after == sorted(before + ['seed0000_ao.ply']) and 'seed0000_geometry.json' in before
    for name in before:
        if name != 'seed0000_geometry.json':
            assert (plain / name).read_bytes() == (with_ao / name).read_bytes(), name
    meta, old = json.load(open(with_ao / 'seed0000_geometry.json')), json.load(open(plain / 'seed0000_geometry.json'))
    block = meta.pop('ambient_occlusion')
    assert meta == old and 'ambient_occlusion' not in old
    want = geometry.ambient_occlusion(out['verts'], out['faces'], samples=16)
    assert block['samples'] == 16 and block['ply'] == 'seed0000_ao.ply' and block['mean'] == float(want['ao'].double().mean())
    v, f, c = geometry.read_ply(str(with_ao / 'seed0000_ao.ply'))
    assert np.array_equal(f, out['faces'].numpy()) and np.array_equal(v, out['verts'].numpy())
    assert np.array_equal(c, np.repeat(np.round(want['ao'].numpy().astype(np.float64) * 255).astype(np.uint8)[:, None], 3, axis=1))
    again = tmp_path / 'again'
    extract_geometry.main(base + ['--outdir', str(again)])
    assert all((plain / name).read_bytes() == (again / name).read_bytes() for name in before)
