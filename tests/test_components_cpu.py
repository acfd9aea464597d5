"""Connected components, host side: the NumPy restatement of the labelling (against known answers, a brute-force flood fill and
scipy.ndimage.label where it is installed), the statistics, the selection rules, the filter, the triangle property that ties the
filter to marching cubes, mesh components, and the generator / CLI plumbing."""
import os
from collections import deque

import numpy as np
import pytest
import torch

from invertavatar_amd import geometry, synthetic
from invertavatar_amd.training_avatar_texture.triplane_v20 import TriPlaneGenerator
from test_geometry_cpu import sphere_field, torus_field

F32 = np.float32


# ------------------------------------------------------------------ helpers shared with test_components_gpu.py

def brute_force(vol, level, connectivity):
    """Flood fill in scan order, one point at a time: (labels, stats) by the definitions, nothing vectorised."""
    vol = np.asarray(vol, dtype=F32)
    inside = vol > F32(level)
    nx, ny, nz = vol.shape
    offs = [(dx, dy, dz) for dx in (-1, 0, 1) for dy in (-1, 0, 1) for dz in (-1, 0, 1)
            if (dx, dy, dz) != (0, 0, 0) and (connectivity == 26 or abs(dx) + abs(dy) + abs(dz) == 1)]
    labels = np.zeros(vol.shape, dtype=np.int32)
    stats = []
    for i in range(nx):
        for j in range(ny):
            for k in range(nz):
                if not inside[i, j, k] or labels[i, j, k]:
                    continue
                c = len(stats) + 1
                labels[i, j, k] = c
                pts, todo = [], deque([(i, j, k)])
                while todo:
                    p = todo.popleft()
                    pts.append(p)
                    for d in offs:
                        q = (p[0] + d[0], p[1] + d[1], p[2] + d[2])
                        if 0 <= q[0] < nx and 0 <= q[1] < ny and 0 <= q[2] < nz and inside[q] and not labels[q]:
                            labels[q] = c
                            todo.append(q)
                a = np.array(pts)
                stats.append([len(pts), (i * ny + j) * nz + k, *a.min(0), *a.max(0)])
    return labels, np.array(stats, dtype=np.int32).reshape(-1, 8)


def smooth_field(shape, seed, sigma=2.0):
    """Seeded white noise blurred by a separable Gaussian in NumPy, scaled to unit standard deviation."""
    f = np.random.RandomState(seed).randn(*shape)
    r = int(3 * sigma)
    w = np.exp(-0.5 * (np.arange(-r, r + 1) / sigma) ** 2)
    w /= w.sum()
    for a in range(3):
        f = np.apply_along_axis(lambda v: np.convolve(np.pad(v, r, mode='reflect'), w, mode='valid'), a, f)
    return (f / f.std()).astype(F32)


def serpentine(n):
    """One path through every second row of an n^3 volume.  In each slice x = even the rows y = even run along z and row 2s is joined
    to row 2s + 2 by one point at y = 2s + 1, at z = n-1 for even s and z = 0 for odd s: a path from (y, z) = (0, 0) to the far end of
    the last row.  Consecutive slices are joined by one point at x = odd, alternately at that far end and at (0, 0), so the slices
    are walked back and forth.  Returns (volume, path length)."""
    v = np.zeros((n, n, n), dtype=F32)
    rows = list(range(0, n, 2))
    far = (rows[-1], n - 1 if (len(rows) - 1) % 2 == 0 else 0)
    for si, i in enumerate(range(0, n, 2)):
        for s, j in enumerate(rows):
            v[i, j, :] = 1
            if s + 1 < len(rows):
                v[i, j + 1, n - 1 if s % 2 == 0 else 0] = 1
        if i + 2 < n:
            v[(i + 1,) + (far if si % 2 == 0 else (0, 0))] = 1
    return v, int(v.sum())


def checkerboard(shape):
    i, j, k = np.indices(shape)
    return ((i + j + k) % 2 == 0).astype(F32)


def known_cases():
    """(name, volume, level) of the small known-answer volumes."""
    two = np.zeros((6, 6, 6), dtype=F32)
    two[0:3, 0:3, 0:3] = 1
    two[3:6, 3:6, 3:6] = 1
    nan_plane = np.ones((7, 5, 6), dtype=F32)
    nan_plane[3] = np.nan
    rs = np.random.RandomState(4)
    return [('empty', np.zeros((5, 6, 7), dtype=F32), 0.5), ('full', np.ones((5, 6, 7), dtype=F32), 0.5), ('corner', two, 0.5),
            ('nan_plane', nan_plane, 0.5), ('2x2x2', rs.rand(2, 2, 2).astype(F32), 0.5), ('5x9x17', rs.rand(5, 9, 17).astype(F32), 0.55)]


def same_partition(a, b):
    """Two labellings split the same points into the same sets."""
    a, b = np.asarray(a).reshape(-1), np.asarray(b).reshape(-1)
    if not np.array_equal(a > 0, b > 0):
        return False
    sel = np.flatnonzero(a)
    a, b = a[sel].astype(np.int64), b[sel].astype(np.int64)
    pairs = np.unique(a * (int(b.max(initial=0)) + 1) + b)                 # the distinct (label in a, label in b) pairs
    return pairs.size == np.unique(a).size == np.unique(b).size


def check_numbering_and_stats(labels, stats):
    """Labels are exactly 1..K in increasing order of smallest linear index, and the table agrees with them."""
    labels, stats = np.asarray(labels), np.asarray(stats)
    k = stats.shape[0]
    lin = np.flatnonzero(labels)
    c = labels.reshape(-1)[lin]
    assert labels.dtype == np.int32 and stats.dtype == np.int32 and stats.shape == (k, 8)
    assert (np.unique(c) == np.arange(1, k + 1)).all() if k else lin.size == 0
    if not k:
        return
    first = np.full(k + 1, labels.size, dtype=np.int64)
    np.minimum.at(first, c, lin)
    assert (np.diff(first[1:]) > 0).all()
    assert np.array_equal(stats[:, 0], np.bincount(c, minlength=k + 1)[1:]) and np.array_equal(stats[:, 1], first[1:])
    for a, x in enumerate(np.unravel_index(lin, labels.shape)):
        lo, hi = np.full(k + 1, 1 << 30), np.full(k + 1, -1)
        np.minimum.at(lo, c, x)
        np.maximum.at(hi, c, x)
        assert np.array_equal(stats[:, 2 + a], lo[1:]) and np.array_equal(stats[:, 5 + a], hi[1:])


def triangle_multiset(v, f):
    """Sorted rows of the nine coordinates of every triangle (bit patterns), independent of vertex numbering."""
    t = np.ascontiguousarray(np.asarray(v, dtype=F32)[np.asarray(f)].reshape(-1, 9)).view(np.uint32)
    return t[np.lexsort(t.T[::-1])]


# ------------------------------------------------------------------ labelling

@pytest.mark.parametrize('connectivity', [26, 6])
def test_known_answers(connectivity):
    expect = {'empty': 0, 'full': 1, 'corner': 1 if connectivity == 26 else 2, 'nan_plane': 2}
    for name, vol, level in known_cases():
        labels, stats = geometry.components(vol, level, connectivity)
        bl, bs = brute_force(vol, level, connectivity)
        assert np.array_equal(labels, bl) and np.array_equal(stats, bs), name
        check_numbering_and_stats(labels, stats)
        if name in expect:
            assert stats.shape == (expect[name], 8), name
    labels, stats = geometry.components(np.zeros((5, 6, 7), F32), 0.5)
    assert labels.shape == (5, 6, 7) and not labels.any() and stats.shape == (0, 8)
    lt, st = geometry.components(torch.ones(3, 4, 5), 0.5)
    assert isinstance(lt, torch.Tensor) and lt.dtype == torch.int32 and st.dtype == torch.int32 and st.tolist() == [[60, 0, 0, 0, 0, 2, 3, 4]]
    with pytest.raises(ValueError):
        geometry.components(np.zeros((5, 6, 7), F32), 0.5, connectivity=18)
    with pytest.raises(ValueError):
        geometry.components(np.zeros((1, 6, 7), F32), 0.5)


def test_checkerboard_and_serpentine():
    cb = checkerboard((9, 10, 11))
    labels, stats = geometry.components(cb, 0.5, 26)
    assert stats.shape[0] == 1 and stats[0, 0] == int(cb.sum())
    labels, stats = geometry.components(cb, 0.5, 6)
    n_in = int(cb.sum())
    assert stats.shape[0] == n_in and np.array_equal(labels.reshape(-1)[np.flatnonzero(cb)], np.arange(1, n_in + 1))
    assert (stats[:, 0] == 1).all()
    for n in (8, 13):
        vol, length = serpentine(n)
        for connectivity in (6, 26):
            labels, stats = geometry.components(vol, 0.5, connectivity)
            assert stats.shape[0] == 1 and stats[0, 0] == length, (n, connectivity, stats[:, 0])


@pytest.mark.parametrize('level', [0.8, 1.4])
def test_smooth_random_field_numbering_and_stats(level):
    vol = smooth_field((20, 24, 28), 7)
    for connectivity in (26, 6):
        labels, stats = geometry.components(vol, level, connectivity)
        bl, bs = brute_force(vol, level, connectivity)
        assert stats.shape[0] > 3
        assert np.array_equal(labels, bl) and np.array_equal(stats, bs)
        check_numbering_and_stats(labels, stats)


@pytest.mark.parametrize('level', [0.8, 1.4])
def test_smooth_random_field_partition_equals_scipy(level):
    ndimage = pytest.importorskip('scipy.ndimage')
    vol = smooth_field((40, 40, 40), 11)
    for connectivity, structure in ((26, np.ones((3, 3, 3))), (6, ndimage.generate_binary_structure(3, 1))):
        labels, stats = geometry.components(vol, level, connectivity)
        ref, k = ndimage.label(vol > F32(level), structure=structure)
        assert k == stats.shape[0] and same_partition(labels, ref)


# ------------------------------------------------------------------ selection and the filter

def test_selection_rules():
    stats = np.zeros((5, 8), np.int32)
    stats[:, 0] = [4, 9, 2, 9, 1]
    sel = geometry.select_components
    assert sel(stats) == [2] and sel(stats, 'largest') == [2]              # the tie goes to the lowest label
    assert sel(stats, 3) == [2, 4, 1] and sel(stats, 99) == [2, 4, 1, 3, 5]
    assert sel(stats, [5, 1]) == [5, 1] and sel(stats, np.array([3])) == [3]
    assert sel(stats, 4, min_voxels=4) == [2, 4, 1] and sel(stats, [5, 1], min_voxels=2) == [1] and sel(stats, 'largest', min_voxels=10) == []
    assert sel(torch.from_numpy(stats), 2) == [2, 4]
    assert sel(np.zeros((0, 8), np.int32)) == [] and sel(np.zeros((0, 8), np.int32), 2) == []
    for bad in (0, -1, 'smallest', None, True, [0], [6], [1, 1], [1.5]):
        with pytest.raises(ValueError):
            sel(stats, bad)
    for bad in (-1, 1.5):
        with pytest.raises(ValueError):
            sel(stats, 1, min_voxels=bad)


def test_filter_touches_only_dropped_inside_points():
    vol = smooth_field((24, 24, 24), 3)
    vol[2, 3, 4] = np.nan
    level = 0.8                                                            # a Python float: must act as fp32 0.8
    labels, stats = geometry.components(vol, level)
    assert stats.shape[0] > 2
    # points between fp32(0.8) and the double 0.8 are outside (fp32 compare), as for marching cubes
    vol[5, 5, 5] = F32(0.8)
    labels, stats = geometry.components(vol, level)
    assert labels[5, 5, 5] == 0 and float(F32(0.8)) > 0.8
    for keep in ('largest', 2, [3, 1]):
        out, info = geometry.keep_components(vol, level, keep)
        kept = np.isin(labels, info['kept'])
        dropped = (labels > 0) & ~kept
        assert info['count'] == stats.shape[0] and np.array_equal(info['stats'], stats) and dropped.any()
        assert out.dtype == F32 and np.array_equal(out.view(np.uint32)[~dropped], vol.view(np.uint32)[~dropped])      # NaN included
        assert (out[dropped] == F32(level)).all()
        l2, s2 = geometry.components(out, level)
        assert s2.shape[0] == len(info['kept']) and np.array_equal(l2 > 0, kept)
    out, _ = geometry.keep_components(vol, level, 'largest', fill=-5.0)
    assert (out[(labels > 0) & (labels != geometry.select_components(stats)[0])] == F32(-5)).all()
    out, info = geometry.keep_components(vol, level, 3, min_voxels=int(np.sort(stats[:, 0])[-2]))
    assert len(info['kept']) == 2
    t_out, t_info = geometry.keep_components(torch.from_numpy(vol), level, 'largest')
    assert isinstance(t_out, torch.Tensor) and t_info['kept'] == geometry.select_components(stats)


def test_filtered_mesh_is_a_sub_multiset_of_the_original_triangles():
    vol, level = smooth_field((40, 40, 40), 5), 0.8
    labels, stats = geometry.components(vol, level)
    k = stats.shape[0]
    assert k >= 5
    v_all, f_all = geometry.marching_cubes(vol, level)
    parts = []
    for c in range(1, k + 1):
        out, _ = geometry.keep_components(vol, level, [c])
        v, f = geometry.marching_cubes(out, level)
        parts.append(triangle_multiset(v, f))
    whole = triangle_multiset(v_all, f_all)
    joined = np.concatenate(parts)
    assert sum(len(p) for p in parts) == len(whole)
    assert np.array_equal(joined[np.lexsort(joined.T[::-1])], whole)       # the K meshes partition the triangles, bit for bit
    out, info = geometry.keep_components(vol, level, 'largest')
    assert geometry.components(out, level)[1].shape[0] == 1
    v, f = geometry.marching_cubes(out, level)
    assert np.array_equal(triangle_multiset(v, f), parts[info['kept'][0] - 1])


# ------------------------------------------------------------------ meshes

def two_surface_volume():
    """A sphere and a torus, far apart, in one [48, 64, 96] volume (level 0)."""
    vol = np.full((48, 64, 96), -5.0, dtype=F32)
    vol[:, :, :40] = torus_field((48, 64, 40))
    s, _ = sphere_field(40, 12.0)
    vol[4:44, 12:52, 52:92] = s
    return vol


def test_mesh_components_of_two_surfaces():
    vol = two_surface_volume()
    v, f = geometry.marching_cubes(vol, 0.0)
    v_t, f_t = geometry.marching_cubes(np.where(np.arange(96) < 46, vol, F32(-5)), 0.0)
    v_s, f_s = geometry.marching_cubes(np.where(np.arange(96) >= 46, vol, F32(-5)), 0.0)
    vl, fl, stats = geometry.mesh_components(f, len(v))
    assert vl.dtype == np.int32 and fl.dtype == np.int32 and stats.dtype == np.int32
    assert stats.tolist() == [[len(v_t), len(f_t), 0], [len(v_s), len(f_s), int(np.flatnonzero(vl == 2)[0])]]
    assert np.array_equal(fl, vl[f[:, 0]]) and np.array_equal(fl, vl[f[:, 1]]) and np.array_equal(fl, vl[f[:, 2]])
    # an isolated vertex is a component of its own, numbered by its index
    vl2, fl2, st2 = geometry.mesh_components(f + 1, len(v) + 2)
    assert vl2[0] == 1 and vl2[-1] == 4 and st2[[0, 3]].tolist() == [[1, 0, 0], [1, 0, len(v) + 1]] and np.array_equal(vl2[1:-1], vl + 1)
    e_v, e_f, e_s = geometry.mesh_components(np.zeros((0, 3), np.int64), 3)
    assert e_v.tolist() == [1, 2, 3] and e_f.shape == (0,) and e_s.tolist() == [[1, 0, 0], [1, 0, 1], [1, 0, 2]]
    with pytest.raises(ValueError):
        geometry.mesh_components(np.array([[0, 1, 5]]), 5)
    # keeping the larger surface = the mesh of the filtered volume, up to vertex order
    colors = np.arange(len(v) * 3, dtype=np.uint8).reshape(-1, 3)
    kv, kf, (kc,), info = geometry.keep_mesh_components(v, f, 'largest', extras=(colors,))
    big = int(np.argmax(stats[:, 0])) + 1
    assert info['count'] == 2 and info['kept'] == [big]
    assert kf.dtype == np.int64 and kf.min() == 0 and kf.max() == len(kv) - 1 and len(kv) == stats[big - 1, 0] and len(kf) == stats[big - 1, 1]
    assert np.array_equal(kv, v[vl == big]) and np.array_equal(kc, colors[vl == big])
    out, vinfo = geometry.keep_components(vol, 0.0, 'largest')
    fv, ff = geometry.marching_cubes(out, 0.0)
    assert np.array_equal(triangle_multiset(kv, kf), triangle_multiset(fv, ff))
    tv, tf, (tc,), _ = geometry.keep_mesh_components(torch.from_numpy(v), torch.from_numpy(f), [1, 2], extras=(torch.from_numpy(colors),))
    assert torch.equal(tv, torch.from_numpy(v)) and torch.equal(tf, torch.from_numpy(f)) and torch.equal(tc, torch.from_numpy(colors))


# ------------------------------------------------------------------ generator and CLI

@pytest.fixture(scope='module')
def small_setup():
    g = synthetic.fill_parameters(TriPlaneGenerator(**synthetic.generator_kwargs('small')).eval().requires_grad_(False))
    with torch.no_grad():
        ws = g.mapping(synthetic.latent(3, 1), synthetic.conditioning_camera(), truncation_psi=0.7, truncation_cutoff=14)
    return g, ws, {'uvcoords_image': synthetic.uv_conditions([5])}


def test_generator_methods_with_and_without_keep(small_setup):
    g, ws, mesh = small_setup
    kw = dict(resolution=24, level=0.0, with_colors=True, with_normals=True, noise_mode='const')
    base = g.extract_geometry(ws, mesh, **kw)[0]
    none = g.extract_geometry(ws, mesh, keep=None, **kw)[0]
    assert set(base) == set(none) == {'volume', 'verts', 'faces', 'colors', 'normals'}
    assert all(torch.equal(base[k], none[k]) for k in base)
    kept = g.extract_geometry(ws, mesh, keep='largest', **kw)[0]
    info = kept['components']
    assert info['count'] >= 1 and len(info['kept']) == 1 and info['stats'].shape == (info['count'], 8)
    assert geometry.components(kept['volume'], 0.0)[1].shape[0] == 1
    vl, _, ms = geometry.mesh_components(kept['faces'], kept['verts'].shape[0])
    assert kept['colors'].shape == kept['verts'].shape == kept['normals'].shape
    assert np.array_equal(triangle_multiset(kept['verts'].numpy(), kept['faces'].numpy()),
                          triangle_multiset(*[x.numpy() for x in geometry.marching_cubes(kept['volume'], 0.0, (-0.5,) * 3, (1 / 23,) * 3)]))
    cams = synthetic.camera_labels([0])
    rk = dict(resolution=16, volume_resolution=24, level=0.0, noise_mode='const')
    r0, r1 = g.render_geometry(ws, cams, mesh, **rk), g.render_geometry(ws, cams, mesh, keep=None, **rk)
    assert all(torch.equal(r0[k], r1[k]) for k in r0)
    r2 = g.render_geometry(ws, cams, mesh, keep='largest', **rk)
    assert set(r2) == set(r0) and bool((r2['mask'] <= r0['mask']).all())


def test_cli_keep_flags_reach_the_call(tmp_path, capsys):
    from invertavatar_amd import extract_geometry
    assert extract_geometry.parse_keep('largest') == 'largest' and extract_geometry.parse_keep('3') == 3
    for bad in ('0', 'big', '-2'):
        with pytest.raises(Exception):
            extract_geometry.parse_keep(bad)
    res = extract_geometry.main(['--seeds', '0', '--width', 'small', '--res', '24', '--level', '0', '--outdir', str(tmp_path), '--device', 'cpu',
                                 '--keep', 'largest', '--min-voxels', '2'])
    path, out = res[0]
    assert os.path.exists(path) and len(out['components']['kept']) == 1
    assert geometry.components(out['volume'], 0.0)[1].shape[0] == 1
    assert f"{out['components']['count']} connected components" in capsys.readouterr().out
    res = extract_geometry.main(['--seeds', '0', '--width', 'small', '--res', '24', '--level', '0', '--outdir', str(tmp_path), '--device', 'cpu'])
    assert 'components' not in res[0][1]
