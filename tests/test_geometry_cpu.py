"""Avatar geometry on the CPU: the marching-cubes case table (regenerated and compared with csrc/mc_tables.h; its properties over all 256
cases), the NumPy marching cubes on analytic surfaces, the lattice point query against ``sample_mixed``, PLY output and the CLI."""
import os

import numpy as np
import pytest
import torch

from invertavatar_amd import geometry, mc_table, synthetic
from invertavatar_amd.training_avatar_texture.triplane_v20 import TriPlaneGenerator

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))


# ------------------------------------------------------------------ mesh helpers

def mesh_stats(v, f):
    v, f = np.asarray(v, dtype=np.float64), np.asarray(f, dtype=np.int64)
    directed = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    und, und_count = np.unique(np.sort(directed, 1), axis=0, return_counts=True)
    _, dir_count = np.unique(directed, axis=0, return_counts=True)
    a, b, c = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
    area = 0.5 * np.linalg.norm(np.cross(b - a, c - a), axis=1).sum()
    volume = np.einsum('ij,ij->i', a, np.cross(b, c)).sum() / 6.0
    return dict(V=len(v), E=len(und), F=len(f), chi=len(v) - len(und) + len(f), closed=bool((und_count == 2).all()),
                oriented=bool((dir_count == 1).all()), area=area, volume=volume)


def sphere_field(n=64, r=20.0):
    c = (n - 1) / 2.0
    x = np.arange(n, dtype=np.float64) - c
    X, Y, Z = np.meshgrid(x, x, x, indexing='ij')
    return (r - np.sqrt(X ** 2 + Y ** 2 + Z ** 2)).astype(np.float32), c


def torus_field(shape=(48, 64, 40), R=14.0, r=6.0):
    cs = [(s - 1) / 2.0 for s in shape]
    X, Y, Z = np.meshgrid(*[np.arange(s, dtype=np.float64) - c for s, c in zip(shape, cs)], indexing='ij')
    q = np.sqrt(X ** 2 + Y ** 2) - R
    return (r - np.sqrt(q ** 2 + Z ** 2)).astype(np.float32)


# ------------------------------------------------------------------ table

def test_table_header_is_generated():
    with open(os.path.join(REPO, 'invertavatar_amd', 'csrc', 'mc_tables.h')) as fh:
        assert fh.read() == mc_table.header_text(), 'csrc/mc_tables.h is stale: run python tools/gen_mc_tables.py'
    count, edges, max_tris = mc_table.tables()
    assert max_tris == int(count.max()) and count[0] == 0 and count[255] == 0


def test_table_edges_are_exactly_the_crossing_edges():
    count, edges, _ = mc_table.tables()
    for case in range(256):
        ins = [(case >> c) & 1 for c in range(8)]
        crossing = {e for e in range(12) if ins[mc_table.EDGES[e][0]] != ins[mc_table.EDGES[e][1]]}
        used = edges[case, :3 * count[case]].tolist()
        assert -1 not in used and (edges[case, 3 * count[case]:] == -1).all()
        assert set(used) == crossing, case
        for t in range(count[case]):
            assert len(set(used[3 * t:3 * t + 3])) == 3, case


def test_face_segments_depend_only_on_the_face():
    for a, side, cyc, n in mc_table.faces():
        seen = {}
        for case in range(256):
            ins = [(case >> c) & 1 for c in range(8)]
            key = tuple(ins[c] for c in cyc)
            segs = mc_table.face_segments(cyc, n, ins)
            assert seen.setdefault(key, segs) == segs, (a, side, case)


def test_loops_closed_and_outward():
    count, edges, _ = mc_table.tables()
    corners = mc_table.CORNERS.astype(np.float64)
    for case in range(256):
        ins = [(case >> c) & 1 for c in range(8)]
        for loop in mc_table.case_loops(case):
            assert len(loop) >= 3 and len(set(loop)) == len(loop)
            pts = np.array([0.5 * (corners[mc_table.EDGES[e][0]] + corners[mc_table.EDGES[e][1]]) for e in loop])
            normal = np.zeros(3)
            for k in range(len(pts)):          # Newell normal of the closed loop
                p, q = pts[k], pts[(k + 1) % len(pts)]
                normal += np.cross(p, q)
            # outward: summed over the loop's crossing edges, inside end -> outside end points the normal's way (a single edge of a
            # non-planar loop may lean against it)
            total = 0.0
            for e in loop:
                c0, c1 = mc_table.EDGES[e]
                out_c, in_c = (c0, c1) if not ins[c0] else (c1, c0)
                total += np.dot(normal, corners[out_c] - corners[in_c])
            assert total > 0, (case, loop)
        # triangles: per case, the fan of the loops in order
        tris = [(lp[0], lp[i], lp[i + 1]) for lp in mc_table.case_loops(case) for i in range(1, len(lp) - 1)]
        assert edges[case, :3 * count[case]].reshape(-1, 3).tolist() == [list(t) for t in tris]


# ------------------------------------------------------------------ NumPy marching cubes

def test_sphere_closed_manifold_area_volume():
    r = 20.0
    vol, c = sphere_field(64, r)
    v, f = geometry.marching_cubes(vol, 0.0, origin=(-c, -c, -c), spacing=(1, 1, 1))
    assert v.dtype == np.float32 and f.dtype == np.int64 and f.shape[1] == 3
    s = mesh_stats(v, f)
    assert s['closed'] and s['oriented'] and s['chi'] == 2, s
    assert abs(s['area'] / (4 * np.pi * r * r) - 1) < 0.02, s
    assert s['volume'] > 0 and abs(s['volume'] / (4 / 3 * np.pi * r ** 3) - 1) < 0.01, s
    assert np.abs(np.linalg.norm(v.astype(np.float64), axis=1) - r).max() < 0.05


def test_torus_non_cubic_genus_one():
    vol = torus_field()
    v, f = geometry.marching_cubes(vol, 0.0)
    s = mesh_stats(v, f)
    assert s['closed'] and s['oriented'] and s['chi'] == 0 and s['volume'] > 0, s
    assert v[:, 0].max() <= 47 and v[:, 1].max() <= 63 and v[:, 2].max() <= 39


def test_empty_and_full_volumes():
    for fill in (-1.0, 1.0):
        v, f = geometry.marching_cubes(np.full((5, 6, 7), fill, np.float32), 0.0)
        assert v.shape == (0, 3) and f.shape == (0, 3) and v.dtype == np.float32 and f.dtype == np.int64
    vt, ft = geometry.marching_cubes(torch.zeros(4, 4, 4), 0.5)
    assert isinstance(vt, torch.Tensor) and vt.shape == (0, 3) and ft.shape == (0, 3) and ft.dtype == torch.int64


def test_level_ties_and_nans_follow_the_inside_rule():
    vol = np.zeros((4, 4, 4), np.float32)
    vol[1:3, 1:3, 1:3] = 1.0
    # equal to the level: outside, so the block of 8 points is the same shape as with the level just below 1 ...
    v_eq, f_eq = geometry.marching_cubes(vol, 1.0)
    assert v_eq.shape == (0, 3)
    v_a, f_a = geometry.marching_cubes(vol, 0.0)
    assert mesh_stats(v_a, f_a)['chi'] == 2
    # ... and a NaN point is outside too: the mesh equals that of the volume with the point set below the level
    nanv = vol.copy()
    nanv[1, 1, 1] = np.nan
    low = vol.copy()
    low[1, 1, 1] = -5.0
    v_n, f_n = geometry.marching_cubes(nanv, 0.5)
    v_l, f_l = geometry.marching_cubes(low, 0.5)
    assert np.array_equal(f_n, f_l) and v_n.shape == v_l.shape and np.isfinite(v_n).all()


def test_vertex_set_equals_brute_force():
    rs = np.random.RandomState(5)
    for shape in ((7, 9, 6), (12, 5, 10)):
        vol = rs.randn(*shape).astype(np.float32)
        level = np.float32(0.25)
        org, spc = np.array([0.5, -1.0, 2.0], np.float32), np.array([0.25, 0.5, 1.5], np.float32)
        v, f = geometry.marching_cubes(vol, float(level), org, spc)
        expect = []
        for i in range(shape[0]):
            for j in range(shape[1]):
                for k in range(shape[2]):
                    for a, (di, dj, dk) in enumerate(((1, 0, 0), (0, 1, 0), (0, 0, 1))):
                        i1, j1, k1 = i + di, j + dj, k + dk
                        if i1 >= shape[0] or j1 >= shape[1] or k1 >= shape[2]:
                            continue
                        v0, v1 = vol[i, j, k], vol[i1, j1, k1]
                        if (v0 > level) == (v1 > level):
                            continue
                        t = float(level - v0) / float(v1 - v0)
                        p0 = org.astype(np.float64) + np.array([i, j, k]) * spc
                        p1 = org.astype(np.float64) + np.array([i1, j1, k1]) * spc
                        expect.append(p0 + t * (p1 - p0))
        expect = np.array(expect)
        assert v.shape == expect.shape                           # one vertex per crossing edge, in (owner, axis) order
        assert np.abs(v - expect).max() < 1e-5
        assert f.min() >= 0 and f.max() < len(v) and len(np.unique(f)) == len(v)


# ------------------------------------------------------------------ lattice and query path

def test_lattice_points_formula():
    pts = geometry.lattice_points((3, 4, 5), (1.0, 2.0, 0.5), (0.1, 0.0, -0.2))
    assert pts.shape == (60, 3) and pts.dtype == torch.float32
    g = pts.reshape(3, 4, 5, 3)
    f32 = np.float32
    for a, (n, L, o) in enumerate(zip((3, 4, 5), (1.0, 2.0, 0.5), (0.1, 0.0, -0.2))):
        lo, step = f32(o) - f32(0.5) * f32(L), f32(L) / f32(n - 1)
        ax = g.select(3, a).numpy()
        idx = [slice(0, 1)] * 3
        idx[a] = slice(None)
        assert np.array_equal(ax[tuple(idx)].reshape(-1), (lo + np.arange(n, dtype=f32) * step).astype(f32))
    assert np.allclose(g[0, 0, 0].numpy(), [0.1 - 0.5, -1.0, -0.2 - 0.25]) and np.allclose(g[-1, -1, -1].numpy(), [0.6, 1.0, 0.05])


@pytest.fixture(scope='module')
def small_setup():
    g = synthetic.fill_parameters(TriPlaneGenerator(**synthetic.generator_kwargs('small')).eval().requires_grad_(False))
    with torch.no_grad():
        ws = g.mapping(synthetic.latent(3, 1), synthetic.conditioning_camera(), truncation_psi=0.7, truncation_cutoff=14)
    return g, ws, {'uvcoords_image': synthetic.uv_conditions([5])}


def test_query_points_and_density_volume_match_sample_mixed_on_cpu(small_setup):
    g, ws, mesh = small_setup
    res = (6, 5, 7)
    pts = geometry.lattice_points(res, 1.0)[None]
    dirs = torch.zeros_like(pts)
    with torch.no_grad():
        ref = g.sample_mixed(pts.clone(), dirs, ws, mesh, noise_mode='const')
        q = g.query_points(ws, pts.clone(), mesh, noise_mode='const')
        planes = geometry.generator_planes(g, ws, mesh, noise_mode='const')
        vol = geometry.density_volume(planes, g.decoder, res, 1.0, box_warp=g.rendering_kwargs['box_warp'])
    assert torch.equal(q['sigma'], ref['sigma']) and torch.equal(q['rgb'], ref['rgb'])
    assert vol.shape == (1, *res) and torch.equal(vol.reshape(-1), ref['sigma'].reshape(-1))


def test_extract_geometry_and_ply_round_trip(small_setup, tmp_path):
    g, ws, mesh = small_setup
    out = g.extract_geometry(ws, mesh, resolution=24, level=0.0, with_colors=True, noise_mode='const')
    assert len(out) == 1
    o = out[0]
    assert o['volume'].shape == (24, 24, 24) and o['verts'].dtype == torch.float32 and o['faces'].dtype == torch.int64
    assert o['colors'].dtype == torch.uint8 and o['colors'].shape == o['verts'].shape and o['faces'].shape[0] > 0
    assert o['verts'].abs().max() <= 0.5
    path = str(tmp_path / 'm.ply')
    geometry.write_ply(path, o['verts'], o['faces'], o['colors'])
    v, f, c = geometry.read_ply(path)
    assert np.array_equal(v, o['verts'].numpy()) and np.array_equal(f, o['faces'].numpy()) and np.array_equal(c, o['colors'].numpy())


def test_cli_writes_ply_on_cpu(tmp_path):
    from invertavatar_amd import extract_geometry
    res = extract_geometry.main(['--seeds', '0', '--width', 'small', '--res', '32', '--level', '0', '--outdir', str(tmp_path),
                                 '--save-volume', '--device', 'cpu'])
    path, out = res[0]
    assert os.path.basename(path) == 'seed0000.ply' and os.path.exists(tmp_path / 'seed0000.npy')
    with open(path, 'rb') as fh:
        head = fh.read(512).split(b'end_header')[0].decode('ascii')
    assert f'element vertex {out["verts"].shape[0]}' in head and f'element face {out["faces"].shape[0]}' in head
    assert out['faces'].shape[0] > 0
