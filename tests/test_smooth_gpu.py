"""geometry.smooth_mesh, MeshAdjacency and mesh_normals on the device (csrc/smooth.hip) against the NumPy restatement: integer outputs
equal exactly, positions within ``4 * e32 + eps32 * extent`` of the restatement (tests/test_smooth_cpu.py explains the tolerance and
holds the meshes and references used here), cotangent weights and normals in the same form, bit equality from run to run, order
independence, and the whole path through ``extract_geometry`` and the command line."""
import json

import numpy as np
import pytest
import torch

from invertavatar_amd import geometry
from test_simplify_cpu import to_np
from test_smooth_cpu import (all_meshes, bad_sphere, check_adjacency, cotangent_reference, fans, normals_reference, reference, small_meshes,
                             surfaces)

pytestmark = pytest.mark.gpu
DEV = 'cuda'
F32 = np.float32
INTS = ('offsets', 'neighbors', 'edge_faces', 'boundary', 'face_offsets', 'face_ids')


def dev(*arrays):
    return [torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in arrays]


def bits(x):
    return to_np(x).view(np.uint32)


def assert_adjacency_equal(name, got, want):
    for k in INTS:
        g, w = to_np(getattr(got, k)), to_np(getattr(want, k))
        assert g.dtype == w.dtype and np.array_equal(g, w), (name, k)
    assert got.info == want.info, (name, got.info, want.info)


def assert_positions(name, v, f, got, **kw):
    """The device result of ``smooth_mesh(v, f, **kw)`` against the restatement; returns the tolerance."""
    ref, pinned, e32, tol = reference(v, f, **kw)
    out = to_np(got['verts'])
    assert got['verts'].dtype == torch.float32 and got['pinned'].dtype == torch.bool and out.shape == v.shape
    assert np.array_equal(to_np(got['pinned']), pinned), name
    assert np.array_equal(out[pinned].view(np.uint32), v[pinned].view(np.uint32)), name            # pinned vertices keep their bits
    ok = np.isfinite(v).all(1)
    assert np.isfinite(out[ok]).all(), name
    err = float(np.abs(out[ok].astype(np.float64) - ref[ok]).max()) if ok.any() else 0.0
    print(f'{name} {kw}: V {len(v)} F {len(f)} e32 {e32:.3e} device error {err:.3e} tol {tol:.3e}')
    assert err <= tol, (name, err, tol)
    return tol


CASES = ({}, {'iterations': 20}, {'iterations': 7, 'mu': None}, {'boundary': 'free'}, {'weights': 'cotangent', 'boundary': 'free'})


def test_cases_equal_the_restatement():
    for name, (v, f) in all_meshes().items():
        tv, tf = dev(v, f)
        adj, want = geometry.MeshAdjacency(tv, tf), geometry.MeshAdjacency(v, f)
        assert_adjacency_equal(name, adj, want)
        check_adjacency(v, f, adj)
        for kw in CASES:
            if kw.get('weights') == 'cotangent' and name not in surfaces():
                continue
            got = geometry.smooth_mesh(tv, tf, adjacency=adj, **kw)
            assert got['info'] == dict(want.info, steps=got['info']['steps'])
            assert_positions(name, v, f, got, **kw)
            assert np.array_equal(bits(tv), v.view(np.uint32))                                                # the caller's vertices are not written


def test_hubs_and_small_meshes_take_both_step_kernels():
    """Hub degrees 63, 64, 65, 70 and 300 straddle the degree above which a vertex gets a wave of its own."""
    for name, (v, f) in {**fans(), **small_meshes()}.items():
        tv, tf = dev(v, f)
        for kw in ({'boundary': 'free', 'iterations': 10}, {'boundary': 'free', 'iterations': 3, 'mu': None, 'weights': 'cotangent'}, {}):
            got = geometry.smooth_mesh(tv, tf, **kw)
            assert_positions(name, v, f, got, **kw)
        assert got['adjacency'].info['max_degree'] == int(np.diff(geometry.MeshAdjacency(v, f).offsets).max())


def test_cotangent_weights_and_normals():
    for name, (v, f) in surfaces().items():
        tv, tf = dev(v, f)
        adj = geometry.MeshAdjacency(tv, tf)
        w64, e32, tol = cotangent_reference(v, f)
        w = to_np(adj.cotangent())
        err = float(np.abs(w.astype(np.float64) - w64).max())
        print(f'{name} cotangent: E {len(w)} e32 {e32:.3e} device error {err:.3e} tol {tol:.3e}')
        assert w.dtype == F32 and err <= tol, (name, err, tol)
    for name, (v, f) in all_meshes().items():
        tv, tf = dev(v, f)
        adj = geometry.MeshAdjacency(tv, tf)
        for weighting in ('area', 'angle'):
            n64, e32, tol = normals_reference(v, f, weighting)
            n = to_np(geometry.mesh_normals(tv, tf, weighting=weighting, adjacency=adj))
            err = float(np.abs(n.astype(np.float64) - n64).max()) if n.size else 0.0
            print(f'{name} normals {weighting}: e32 {e32:.3e} device error {err:.3e} tol {tol:.3e}')
            assert n.dtype == F32 and n.shape == v.shape and np.isfinite(n).all() and err <= tol, (name, weighting, err, tol)
            assert np.array_equal(bits(geometry.mesh_normals(tv, tf, weighting=weighting)), n.view(np.uint32))     # run to run, own adjacency


def test_same_bits_from_run_to_run_and_with_a_prebuilt_adjacency():
    for name in ('sphere25', 'soup', 'fan300c', 'square'):
        v, f = all_meshes()[name]
        tv, tf = dev(v, f)
        adj = geometry.MeshAdjacency(tv, tf)
        for weights in ('uniform', 'cotangent'):
            a = geometry.smooth_mesh(tv, tf, weights=weights, boundary='free')
            b = geometry.smooth_mesh(tv, tf, weights=weights, boundary='free')
            c = geometry.smooth_mesh(tv, tf, weights=weights, boundary='free', adjacency=adj)
            assert np.array_equal(bits(a['verts']), bits(b['verts'])) and np.array_equal(bits(a['verts']), bits(c['verts'])), (name, weights)
            assert np.array_equal(bits(a['adjacency'].cotangent()), bits(adj.cotangent()))
            assert c['adjacency'] is adj
        # two calls on one adjacency with different weights do not disturb each other
        u1 = geometry.smooth_mesh(tv, tf, adjacency=adj)
        geometry.smooth_mesh(tv, tf, weights='cotangent', adjacency=adj)
        u2 = geometry.smooth_mesh(tv, tf, adjacency=adj)
        fresh = geometry.smooth_mesh(tv, tf)
        assert np.array_equal(bits(u1['verts']), bits(u2['verts'])) and np.array_equal(bits(u1['verts']), bits(fresh['verts']))


def test_permuted_vertices_and_faces():
    rs = np.random.RandomState(11)
    for name in ('sphere17', 'cube', 'square', 'soup', 'fan70c'):
        v, f = all_meshes()[name]
        pv, pf = rs.permutation(len(v)), rs.permutation(len(f))
        inv = np.empty_like(pv)
        inv[pv] = np.arange(len(v))                                                                # old index -> new index
        v2, f2 = v[pv], np.roll(inv[f[pf]], rs.randint(1, 3), axis=1)
        base = geometry.smooth_mesh(*dev(v, f), boundary='free')
        perm = geometry.smooth_mesh(*dev(v2, f2), boundary='free')
        assert_adjacency_equal(name, perm['adjacency'], geometry.MeshAdjacency(v2, f2))
        a, b = base['adjacency'], perm['adjacency']
        assert a.info == b.info
        # the permuted integer outputs: the same directed edges with the same face counts, the same boundary and pinned flags
        def edges(adj, relabel):
            off, nbr, ef = (to_np(getattr(adj, k)).astype(np.int64) for k in ('offsets', 'neighbors', 'edge_faces'))
            row = np.repeat(np.arange(len(v)), np.diff(off))
            keys = relabel[row] * len(v) + relabel[nbr]
            o = np.argsort(keys)
            return keys[o], ef[o]
        ka, ea = edges(a, np.arange(len(v)))
        kb, eb = edges(b, pv)
        assert np.array_equal(ka, kb) and np.array_equal(ea, eb), name
        assert np.array_equal(to_np(b.boundary)[inv], to_np(a.boundary)) and np.array_equal(to_np(perm['pinned'])[inv], to_np(base['pinned']))
        foff_a, foff_b = to_np(a.face_offsets), to_np(b.face_offsets)
        assert np.array_equal(np.diff(foff_b)[inv], np.diff(foff_a))
        tol = assert_positions(name + ' permuted', v2, f2, perm, boundary='free')
        ok = np.isfinite(v).all(1)
        diff = float(np.abs(to_np(perm['verts'])[inv][ok].astype(np.float64) - to_np(base['verts'])[ok]).max())
        print(f'{name}: permuted against unpermuted device run {diff:.3e} tol {tol:.3e}')
        assert diff <= tol


def test_non_finite_empty_and_out_of_range():
    v, f = bad_sphere()
    tv, tf = dev(v, f)
    for kw in ({}, {'weights': 'cotangent'}, {'iterations': 4, 'mu': None}):
        got = geometry.smooth_mesh(tv, tf, **kw)
        out = to_np(got['verts'])
        bad = ~np.isfinite(v).all(1)
        assert bad.sum() == 2 and np.array_equal(out[bad].view(np.uint32), v[bad].view(np.uint32))
        assert np.isfinite(out[~bad]).all()
        if 'weights' not in kw:
            assert_positions('bad sphere', v, f, got, **kw)                                        # their former neighbours included
    n = to_np(geometry.mesh_normals(tv, tf))
    assert np.isfinite(n).all() and not n[bad].any()
    for name in ('no_faces', 'no_verts', 'V1'):
        vv, ff = all_meshes()[name]
        tv, tf = dev(vv, ff)
        got = geometry.smooth_mesh(tv, tf, weights='cotangent')
        adj = got['adjacency']
        assert got['verts'].dtype == torch.float32 and tuple(got['verts'].shape) == vv.shape and np.array_equal(bits(got['verts']), vv.view(np.uint32))
        assert got['pinned'].dtype == torch.bool and tuple(got['pinned'].shape) == (len(vv),) and bool(got['pinned'].all())
        assert adj.neighbors.dtype == torch.int32 and adj.neighbors.numel() == 0 and adj.offsets.numel() == len(vv) + 1 and not adj.offsets.any()
        assert adj.cotangent().dtype == torch.float32 and adj.cotangent().numel() == 0 and adj.face_ids.numel() == 0
        nrm = geometry.mesh_normals(tv, tf, adjacency=adj)
        assert nrm.dtype == torch.float32 and tuple(nrm.shape) == (len(vv), 3) and not nrm.any()
        assert adj.info == geometry.MeshAdjacency(vv, ff).info
    v, f = all_meshes()['sphere17']
    for bad_face in ([0, 1, len(v)], [0, -1, 2]):
        tv, tf = dev(v, np.concatenate([f, [bad_face]]))
        with pytest.raises(ValueError):
            geometry.smooth_mesh(tv, tf)
        with pytest.raises(ValueError):
            geometry.mesh_normals(tv, tf)
    tv, tf = dev(v, f)
    fixed = np.zeros(len(v), bool)
    fixed[::2] = True
    got = geometry.smooth_mesh(tv, tf, fixed=dev(fixed)[0])
    assert_positions('fixed mask', v, f, got, fixed=fixed)
    assert np.array_equal(bits(geometry.smooth_mesh(tv, tf, iterations=0)['verts']), v.view(np.uint32))
    assert np.array_equal(bits(geometry.smooth_mesh(tv, tf, fixed=torch.ones(len(v), dtype=torch.bool, device=DEV))['verts']), v.view(np.uint32))


@pytest.fixture(scope='module')
def small_generator():
    from invertavatar_amd import synthetic
    from invertavatar_amd.training_avatar_texture.triplane_v20 import TriPlaneGenerator
    gen = TriPlaneGenerator(**synthetic.generator_kwargs('small')).eval().requires_grad_(False)
    synthetic.fill_parameters(gen)
    gen = gen.to(DEV)
    with torch.no_grad():
        ws = gen.mapping(synthetic.latent(3, 1).to(DEV), synthetic.conditioning_camera().to(DEV), truncation_psi=0.7, truncation_cutoff=14)
    return gen, ws, {'uvcoords_image': synthetic.uv_conditions([0]).to(DEV)}


def test_whole_path(small_generator, tmp_path):
    gen, ws, mesh = small_generator
    kw = dict(resolution=64, level=0.0, keep='largest', with_normals=True, with_colors=True, noise_mode='const')
    rough = gen.extract_geometry(ws, mesh, **kw)[0]
    out = gen.extract_geometry(ws, mesh, smooth=5, **kw)[0]
    assert torch.equal(out['faces'], rough['faces']) and 'smooth' not in rough and out['smooth']['steps'] == 10
    want = geometry.smooth_mesh(rough['verts'], rough['faces'], iterations=5)
    assert np.array_equal(bits(out['verts']), bits(want['verts']))
    assert np.array_equal(bits(out['normals']), bits(geometry.mesh_normals(out['verts'], out['faces'])))
    # colours are queried at the final vertices (the planes of a second call need not have the same bits: one 8-bit step of slack)
    again = geometry.vertex_colors(geometry.generator_planes(gen, ws, mesh, noise_mode='const'), gen.decoder, out['verts'], gen.rendering_kwargs['box_warp'])
    step = int((out['colors'].int() - again.int()).abs().max())
    moved = int((out['colors'].int() - rough['colors'].int()).abs().max())
    print(f'whole path: colours against a second query {step}, against the colours at the unsmoothed vertices {moved}')
    assert step <= 1 < moved
    laplace = geometry.smooth_mesh(rough['verts'], rough['faces'], iterations=5, mu=None)['verts']
    vol, vt, vl = (geometry.signed_volume(x, rough['faces']) for x in (rough['verts'], out['verts'], laplace))
    print(f'whole path: V {out["verts"].shape[0]} F {out["faces"].shape[0]} volume {vol:.6f} taubin {vt:.6f} laplace {vl:.6f}; {out["smooth"]}')
    assert abs(vt - vol) < abs(vl - vol)
    simple = gen.extract_geometry(ws, mesh, simplify={'cells': 24}, **kw)[0]
    both = gen.extract_geometry(ws, mesh, simplify={'cells': 24}, smooth=5, **kw)[0]
    assert torch.equal(both['faces'], simple['faces']) and both['simplify'] == simple['simplify']
    assert np.array_equal(bits(both['verts']), bits(geometry.smooth_mesh(simple['verts'], simple['faces'], iterations=5)['verts']))


def test_command_line(tmp_path):
    from invertavatar_amd import extract_geometry
    args = ['--seeds', '0', '--width', 'small', '--res', '64', '--level', '0', '--keep', 'largest', '--outdir', str(tmp_path), '--device', DEV]
    (path, out), = extract_geometry.main(args + ['--smooth', '5', '--smooth-check', '--normals'])
    v, f, c, n = geometry.read_ply(path, with_normals=True)
    assert np.array_equal(v, to_np(out['verts'])) and np.array_equal(f, to_np(out['faces'])) and np.array_equal(n, to_np(out['normals']))
    assert np.array_equal(c, to_np(out['colors']))
    meta = json.load(open(str(tmp_path / 'seed0000_geometry.json')))['smooth']
    chk = meta['check']
    assert set(chk) >= {'volume_before', 'volume_after', 'smoothed_to_input', 'input_to_smoothed'} and meta['steps'] == 10
    assert chk['volume_after'] == geometry.signed_volume(out['verts'], out['faces']) and 0 < chk['smoothed_to_input'] < 0.1
    assert meta['boundary_edges'] == out['smooth']['boundary_edges'] and meta['nonmanifold_edges'] == out['smooth']['nonmanifold_edges']
