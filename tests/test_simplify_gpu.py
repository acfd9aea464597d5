"""geometry.simplify_mesh on the device (csrc/simplify.hip) against the NumPy restatement: integer outputs equal exactly, positions
within ``4 * e_ord + eps32 * extent`` of the float64 restatement (tests/test_simplify_cpu.py explains the tolerance and holds the
meshes and checks used here), bit equality from run to run, the count-only pass, and the full-size path through ``extract_geometry``
and the command line."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from invertavatar_amd import geometry
from test_simplify_cpu import (EPS32, check_distance_bound, check_extras, check_invariants, check_target, closed_meshes, corner_distances,
                               cube_with_satellites, diagonal, flat_square, make_extras, reference64, signed_volume, soups, sphere_mesh,
                               to_np)

pytestmark = pytest.mark.gpu
DEV = 'cuda'
F32 = np.float32


def dev(*arrays):
    return [torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in arrays]


def run_both(v, f, **kw):
    tv, tf = dev(v, f)
    return geometry.simplify_mesh(tv, tf, **kw), geometry.simplify_mesh(v, f, **kw)


def assert_matches(name, v, f, got, want, placement):
    for k in ('faces', 'vertex_map', 'cluster_size'):
        assert np.array_equal(to_np(got[k]), want[k]), (name, k)
    assert got['dims'] == want['dims'] and got['usable_faces'] == want['usable_faces'] and got['input_faces'] == want['input_faces']
    assert got['verts'].dtype == torch.float32 and got['faces'].dtype == torch.int64
    ref, e_ord, tol, _ = reference64(v, f, want, placement)
    err = float(np.abs(to_np(got['verts']).astype(np.float64) - ref['verts']).max()) if len(want['verts']) else 0.0
    print(f'{name} {placement}: V {len(v)} -> {len(want["verts"])}, F {len(f)} -> {len(want["faces"])}, e_ord {e_ord:.3e} device error {err:.3e} tol {tol:.3e}')
    assert err <= tol, (name, err, tol)
    return tol


@pytest.mark.parametrize('placement', ['mean', 'quadric'])
def test_cases_equal_the_restatement(placement):
    rs = np.random.RandomState(3)
    for name, (v, f) in {**closed_meshes(), **soups(), 'square': flat_square()}.items():
        for kw in ({'cells': 1}, {'cells': 3}, {'cells': 8}, {'cells': 16}, {'cells': (5, 9, 2)}, {'cell_size': 0.21}, {'cell_size': 1e-4}):
            got, want = run_both(v, f, placement=placement, **kw)
            check_invariants(v, f, got)
            tol = assert_matches(f'{name} {kw}', v, f, got, want, placement)
            if kw == {'cells': 8}:
                cells = 8
                check_distance_bound(name, cells, v, f, got, device=DEV, samples=1500)
                # order independence on the device
                pv, pf = rs.permutation(len(v)), rs.permutation(len(f))
                inv = np.empty_like(pv)
                inv[pv] = np.arange(len(v))
                tv, tf = dev(v[pv], np.roll(inv[f[pf]], rs.randint(3), axis=1))
                perm = geometry.simplify_mesh(tv, tf, placement=placement, **kw)
                assert np.array_equal(to_np(perm['faces']), want['faces']) and np.array_equal(to_np(perm['cluster_size']), want['cluster_size'])
                assert np.array_equal(to_np(perm['vertex_map'])[inv], want['vertex_map'])
                if len(want['verts']):
                    assert np.abs(to_np(perm['verts']).astype(np.float64) - reference64(v, f, want, placement)[0]['verts']).max() <= tol
            if kw == {'cell_size': 1e-4} and name in closed_meshes():   # identity
                assert got['verts'].shape[0] == len(v) and got['faces'].shape[0] == len(f)
                moved = np.abs(to_np(got['verts'])[to_np(got['vertex_map'])].astype(np.float64) - v).max()
                assert moved == 0 if placement == 'mean' else moved <= tol


def test_empty_and_non_finite():
    v, f = sphere_mesh(17)
    for vv, ff in ((np.zeros((0, 3), F32), np.zeros((0, 3), np.int64)), (v, np.zeros((0, 3), np.int64)),
                   (np.full((5, 3), np.nan, F32), np.array([[0, 1, 2], [2, 3, 4]]))):
        for kw in ({'cells': 4}, {'target_faces': 10}, {'cell_size': 0.1}):
            got, want = run_both(vv, ff, **kw)
            assert got['verts'].shape == (0, 3) and got['faces'].shape == (0, 3) and got['cluster_size'].shape == (0,)
            assert np.array_equal(to_np(got['vertex_map']), want['vertex_map']) and got['usable_faces'] == 0
    w = v.copy()
    w[7, 1] = np.nan
    w[100] = np.inf
    for kw in ({'cells': 9}, {'cell_size': 1e-4}, {'target_faces': 10 ** 6}, {'target_faces': 300}):
        got, want = run_both(w, f, **kw)
        check_invariants(w, f, got)
        assert_matches(f'nan {kw}', w, f, got, want, 'quadric')
    tv, tf = dev(v, np.array([[0, 1, len(v)]]))
    with pytest.raises(ValueError):
        geometry.simplify_mesh(tv, tf, cells=4)


def test_orientation_corners_and_planes():
    for name in ('sphere', 'cube'):
        v, f = closed_meshes()[name]
        vol = signed_volume(v, f)
        for cells in (8, 16, 32):
            got, want = run_both(v, f, cells=cells)
            out, ref = signed_volume(to_np(got['verts']), to_np(got['faces'])), signed_volume(want['verts'], want['faces'])
            print(f'{name} cells={cells}: volume {out:.6f} (restatement {ref:.6f}, input {vol:.6f})')
            assert out > 0 and abs(out - ref) <= 1e-5 * vol
    v, f = cube_with_satellites()
    q, q_ref = run_both(v, f, cell_size=0.25)
    m, m_ref = run_both(v, f, cell_size=0.25, placement='mean')
    tol = reference64(v, f, q_ref, 'quadric')[2]
    dq, dm, dm_ref = corner_distances(v, f, q), corner_distances(v, f, m), corner_distances(v, f, m_ref)
    print(f'corner clusters: quadric {dq.max():.3e} (tol {tol:.3e}), mean {dm.min() / 0.25:.3f} cells (restatement {dm_ref.min() / 0.25:.3f})')
    assert dq.max() <= tol
    assert (dm >= 0.5 * dm_ref).all() and dm_ref.min() > 0
    sv, sf = flat_square()
    for placement in ('quadric', 'mean'):
        got, want = run_both(sv, sf, cells=7, placement=placement)
        assert len(want['faces'])
        assert np.abs(to_np(got['verts'])[:, 2].astype(np.float64) - float(F32(0.3))).max() <= reference64(sv, sf, want, placement)[2]


def test_target_faces_extras_and_count_only_pass():
    v, f = sphere_mesh(31)
    tv, tf = dev(v, f)
    run = lambda **kw: geometry.simplify_mesh(tv, tf, **kw)              # noqa: E731
    for n in (12, 100, 777, 3000):
        got, want = run(target_faces=n), geometry.simplify_mesh(v, f, target_faces=n)
        check_invariants(v, f, got)
        check_target(v, f, n, got, run)
        assert got['dims'] == want['dims'] and got['steps'] == want['steps']
        assert_matches(f'target {n}', v, f, got, want, 'quadric')
    got = run(target_faces=len(f) - 1, max_cells=4)
    assert max(got['dims']) == 4 and got['faces'].shape[0] <= len(f) - 1
    got, want = run(target_faces=len(f)), geometry.simplify_mesh(v, f, target_faces=len(f))
    assert got['dims'] is None and np.array_equal(to_np(got['verts']), v) and np.array_equal(to_np(got['faces']), want['faces'])
    # the count-only pass equals the face count of the full pass
    for cells in (1, 2, 5, 8, 13, 21, 64, 200):
        grid = (lambda d, i, c: (d, list(want['lo']), i, c))(*geometry._simplify_plan(want['lo'], to_np(tv.amax(0)).tolist(), cells, None))
        count = geometry._simplify_device(tv, tf.int(), grid, 'quadric', (), count_only=True)['n_faces']
        assert count == run(cells=cells)['faces'].shape[0] == geometry.simplify_mesh(v, f, cells=cells)['faces'].shape[0]
    extras = make_extras(v, np.random.RandomState(2))
    for kw in ({'cells': 6}, {'cells': 13, 'placement': 'mean'}, {'target_faces': 10 ** 6}):
        got = run(extras=dev(*extras), **kw)
        check_extras(v, f, got, extras)
        want = geometry.simplify_mesh(v, f, extras=extras, **kw)
        assert np.array_equal(to_np(got['extras'][1]), want['extras'][1])          # uint8 colours


def test_bit_equal_runs_and_addresses():
    for v, f in (sphere_mesh(37), soups()['soup_clustered']):
        for kw in ({'cells': 1}, {'cells': 3}, {'cells': 11}, {'target_faces': 500}):
            tv, tf = dev(v, f)
            a = geometry.simplify_mesh(tv, tf, **kw)
            b = geometry.simplify_mesh(tv, tf, **kw)
            pad = torch.empty(12345, device=DEV)                             # the same input at other addresses
            tv2, tf2 = tv.clone(), tf.clone()
            c = geometry.simplify_mesh(tv2, tf2, **kw)
            del pad
            for other in (b, c):
                for k in ('verts', 'faces', 'vertex_map', 'cluster_size'):
                    assert torch.equal(a[k].view(torch.int32) if k == 'verts' else a[k], other[k].view(torch.int32) if k == 'verts' else other[k]), (kw, k)


def test_large_cluster_and_sizes_off_the_chunk(capsys):
    """Sums over clusters from one vertex to the whole mesh, entry counts around the chunk and level sizes of the segmented sum."""
    rs = np.random.RandomState(9)
    for nv in (1, 31, 32, 33, 63, 65, 1023, 1025, 5000):
        v = rs.uniform(-1, 1, (nv, 3)).astype(F32)
        f = rs.randint(0, nv, (2 * nv + 3, 3)).astype(np.int64)
        for kw in ({'cells': 2}, {'cells': 7}):
            got, want = run_both(v, f, **kw)
            check_invariants(v, f, got)
            assert_matches(f'random V={nv} {kw}', v, f, got, want, 'quadric')
    # one cluster holds nearly every vertex: two far outliers and a dense ball in one cell
    v = np.concatenate([rs.normal(0, 0.01, (70001, 3)), [[-9, -9, -9], [9, 9, 9], [9, -9, 9]]]).astype(F32)
    f = np.concatenate([rs.randint(0, 70001, (90000, 3)), [[0, 70001, 70002], [1, 70002, 70003], [70001, 70002, 70003]]]).astype(np.int64)
    got, want = run_both(v, f, cells=3)
    assert want['cluster_size'].max() == 70001
    assert_matches('one big cluster', v, f, got, want, 'quadric')


def test_extract_geometry_full_size():
    from invertavatar_amd import synthetic
    from invertavatar_amd.training_avatar_texture.triplane_v20 import TriPlaneGenerator
    G = synthetic.fill_parameters(TriPlaneGenerator(**synthetic.generator_kwargs('full')).eval().requires_grad_(False)).cuda()
    with torch.no_grad():
        ws = G.mapping(synthetic.latent(7, 1).cuda(), synthetic.conditioning_camera().expand(1, -1).cuda(), truncation_psi=0.7, truncation_cutoff=14)
    cond = {'uvcoords_image': synthetic.uv_conditions([3]).cuda()}
    kw = dict(resolution=256, level=0.0, keep='largest', with_colors=True, with_normals=True, noise_mode='const')
    full = G.extract_geometry(ws, cond, **kw)[0]
    item = G.extract_geometry(ws, cond, simplify=100000, **kw)[0]
    info = item['simplify']
    nf, nv = item['faces'].shape[0], item['verts'].shape[0]
    print('simplify:', info)
    assert nf <= 100000 and info['faces_before'] == full['faces'].shape[0] and info['faces_after'] == nf
    assert item['colors'].shape == (nv, 3) and item['colors'].dtype == torch.uint8 and item['normals'].shape == (nv, 3)
    assert torch.isfinite(item['normals']).all()
    c = max(info['dims'])
    more = geometry.simplify_mesh(full['verts'], full['faces'], cells=c + 1)
    assert more['faces'].shape[0] > 100000
    r = geometry.surface_distance(item['verts'], item['faces'], full['verts'], full['faces'], samples=200000)
    diag = float(np.sqrt(3.0)) * info['cell_size']
    print(f'chamfer {r["chamfer"]:.6f}  simplified->full {r["max_ab"]:.6f}  full->simplified {r["max_ba"]:.6f}  cell diagonal {diag:.6f}')
    assert r['max_ab'] <= diag + 8 * EPS32 * float(full['verts'].abs().max())


def test_cli_writes_a_readable_simplified_ply(tmp_path):
    cmd = [sys.executable, '-m', 'invertavatar_amd.extract_geometry', '--seeds', '0', '--outdir', str(tmp_path), '--res', '192',
           '--level', '0', '--keep', 'largest', '--simplify', '50000', '--simplify-check']
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900, cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    print(r.stdout[-2000:], r.stderr[-2000:])
    assert r.returncode == 0
    ply = [p for p in os.listdir(tmp_path) if p.endswith('.ply')]
    assert len(ply) == 1
    v, f, _ = geometry.read_ply(os.path.join(tmp_path, ply[0]))
    assert 0 < len(f) <= 50000 and f.max() == len(v) - 1
    geometry.write_ply(os.path.join(tmp_path, 'again.ply'), v, f)
    v2, f2, _ = geometry.read_ply(os.path.join(tmp_path, 'again.ply'))
    assert np.array_equal(v, v2) and np.array_equal(f, f2)
    meta = json.load(open(os.path.join(tmp_path, ply[0][:-4] + '_geometry.json')))
    chk = meta['simplify']['check']
    assert chk['simplified_to_full'] <= chk['cell_diagonal'] * (1 + 1e-5) + 1e-5


def test_scan_sizes():
    """The one-workgroup exclusive scan that every compacted count goes through (scan_workgroup in csrc/geom_common.h), called
    directly as ia_simplify_refs: empty input, fewer items than the 1024 threads, one item per thread and one over, a ragged last
    slice and several items per thread.  Exact against an int64 cumsum; nothing is written past out[K]."""
    from invertavatar_amd import _lib
    lib = _lib.load()
    for k in (0, 1, 2, 1023, 1024, 1025, 2047, 2049, 7171, 100003):
        for ref in (np.random.RandomState(k).randint(0, 2, size=k).astype(np.int32), np.ones(k, dtype=np.int32)):
            tref, = dev(ref)
            out = torch.full((k + 2,), -7, dtype=torch.int32, device=DEV)
            _lib.check(lib.ia_simplify_refs(tref.data_ptr(), k, out.data_ptr(), _lib.stream_ptr(out.device)), 'ia_simplify_refs')
            got = to_np(out).astype(np.int64)
            assert np.array_equal(got[:k + 1], np.concatenate([[0], np.cumsum(ref, dtype=np.int64)])), k
            assert got[k + 1] == -7, k
