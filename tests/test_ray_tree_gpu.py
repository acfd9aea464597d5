"""Rays against the mesh on the cluster tree on the device (csrc/ray_tree.hip): ia_ray_mesh_tree against ia_ray_mesh_brute and the
float32 restatement, ia_ao_rays against its restatement, ambient occlusion, occlusion of segments and the error paths.  The tree
only prunes, so every comparison is on bits.  Meshes and ray families are those of tests/test_ray_tree_cpu.py."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from invertavatar_amd import _lib, geometry, hipops
from test_closest_tree_cpu import CENTRE, FACE_COUNTS, cut, mc48, tree_of
from test_ray_tree_cpu import FIELDS, INWARD, brute as host_brute, by_tree as host_tree, plates, rays
from test_winding_cpu import F32

pytestmark = pytest.mark.gpu
DEV = 'cuda'
L = geometry.WINDING_LEAF


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def bits(t):
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t


def same(a, b, rows=None):
    return all(a[k].dtype == b[k].dtype and torch.equal(bits(a[k]), bits(b[k] if rows is None else b[k][rows])) for k in b)


@functools.lru_cache(maxsize=None)
def built(n):
    verts, faces = cut(n)
    v, f = dev(verts), dev(faces)
    return v, f, geometry.WindingTree(v, f)


def as_result(r):
    return {'hit': dev(r[0]), 't': dev(r[1]), 'face': dev(r[2].astype(np.int64)), 'bary': dev(r[3]), 'point': dev(r[4])}


@pytest.mark.parametrize('n', FACE_COUNTS)
def test_tree_is_brute_and_the_restatement_bit_for_bit(n):
    v, f, tree = built(n)
    o, d, t_lo, t_hi = (dev(x) for x in rays(n)[:4])
    want = tree.rays(o, d, t_lo, t_hi, brute=True)
    assert list(want) == list(FIELDS) and want['hit'].dtype == torch.bool and want['face'].dtype == torch.int64
    assert same(want, as_result(host_brute(n, np.float32)))                                            # NaN patterns included: int32 views
    for sort in (True, False):
        assert same(tree.rays(o, d, t_lo, t_hi, sort=sort), want)
        only = tree.rays(o, d, t_lo, t_hi, mode='any', sort=sort)
        assert list(only) == ['hit'] and torch.equal(only['hit'], want['hit'])
    assert torch.equal(tree.rays(o, d, t_lo, t_hi, mode='any', brute=True)['hit'], want['hit'])
    assert same(geometry.ray_mesh(o, d, v, f, t_lo, t_hi, tree=tree), want) and same(geometry.ray_mesh(o, d, v, f, t_lo, t_hi, brute=True), want)
    perm = torch.from_numpy(np.random.RandomState(n or 7).permutation(o.shape[0])).to(DEV)
    for sort in (True, False):
        assert same(tree.rays(o[perm], d[perm], t_lo[perm], t_hi[perm], sort=sort), want, perm)
    for m in (0, 1, 63, 64, 65):
        tail = slice(o.shape[0] - m, o.shape[0])
        part = tree.rays(o[tail], d[tail], t_lo[tail], t_hi[tail])
        assert part['t'].shape == (m,) and same(part, want, tail)
        assert torch.equal(tree.rays(o[tail], d[tail], t_lo[tail], t_hi[tail], mode='any')['hit'], want['hit'][tail])
    assert same(tree.rays(o, d, t_lo, t_hi), want)                                                     # run to run


def test_counts_on_the_full_mesh():
    _, _, tree = built(None)
    o, d, t_lo, t_hi, fam = rays(None)
    for mode in ('first', 'any'):
        res = tree.rays(dev(o), dev(d), dev(t_lo), dev(t_hi), mode=mode, return_counts=True)
        counts = res['counts'].cpu().numpy()
        assert counts.dtype == np.int32 and counts.shape == (o.shape[0], 2)
        ref = host_tree(None, np.float32, mode)[5]
        assert not counts[fam['bad']].any() and (counts[:, 1] <= tree.usable).all()
        for name in ('centre', 'inside', 'axis') + INWARD:
            c, r = counts[fam[name]], ref[fam[name]]
            print(f'{mode} {name}: device mean boxes {c[:, 0].mean():.1f} pairs {c[:, 1].mean():.1f}; restatement mean boxes {r[:, 0].mean():.1f} '
                  f'pairs {r[:, 1].mean():.1f}; of {tree.usable} usable faces; rays whose counts differ: {int((c != r).any(1).sum())}')
        for name in ('centre', 'inside', 'axis') + INWARD:
            assert counts[fam[name], 1].mean() <= tree.usable / 4, name
        unsorted = tree.rays(dev(o), dev(d), dev(t_lo), dev(t_hi), mode=mode, return_counts=True, sort=False)['counts'].cpu().numpy()
        assert np.array_equal(unsorted, counts)                                                        # a ray's counts are its own


def test_ao_rays_and_ambient_occlusion():
    rs = np.random.RandomState(0)
    n = rs.standard_normal((300, 3))
    n = (n / np.linalg.norm(n, axis=1, keepdims=True)).astype(F32)
    n[:3] = [(0, 0, 1), (0, 0, -1), (1, 0, 0)]
    n[3] = (np.nan, 0, 1)
    n[4] = (0, np.inf, 0)
    p = rs.standard_normal((300, 3)).astype(F32)
    table = geometry._ao_table(16, 0)
    o, d = hipops.ao_rays(dev(p), dev(n), dev(table), 0.01)
    ro, rd = geometry._ao_rays_numpy(p, n, table, 0.01)
    assert tuple(o.shape) == (4800, 3) and np.array_equal(np.isnan(ro), np.isnan(o.cpu().numpy())) and np.isnan(ro[48:80]).all()
    assert np.array_equal(o.cpu().numpy().view(np.int32), ro.view(np.int32)) and np.array_equal(d.cpu().numpy().view(np.int32), rd.view(np.int32))
    verts, faces = mc48()
    got = geometry.ambient_occlusion(dev(verts), dev(faces), samples=16)
    want = geometry.ambient_occlusion(verts, faces, samples=16)
    assert got['unoccluded'].dtype == torch.int32 and got['ao'].dtype == torch.float32 and got['samples'] == 16
    assert np.array_equal(got['unoccluded'].cpu().numpy(), want['unoccluded']) and np.array_equal(got['ao'].cpu().numpy(), want['ao'])
    again = geometry.ambient_occlusion(dev(verts), dev(faces), samples=16)
    assert torch.equal(again['unoccluded'], got['unoccluded'])
    inward = geometry.ambient_occlusion(dev(verts), dev(faces), samples=16, normals=-geometry.mesh_normals(dev(verts), dev(faces)))
    host_in = geometry.ambient_occlusion(verts, faces, samples=16, normals=-geometry.mesh_normals(verts, faces))
    print(f'outward: mean ao {float(got["ao"].mean()):.4f}; inward (inside the closed sphere): mean ao {float(inward["ao"].mean()):.4f}')
    assert np.array_equal(inward['unoccluded'].cpu().numpy(), host_in['unoccluded']) and float(inward['ao'].mean()) < 0.01
    pv, pf = plates()
    up = torch.tensor([[0.0, 0.0, 1.0]], device=DEV)
    alone = geometry.ambient_occlusion(dev(pv[:3]), dev(pf[:1]), samples=32, normals=up.repeat(3, 1))
    assert (alone['unoccluded'] == 32).all() and (alone['ao'] == 1).all()
    near = geometry.ambient_occlusion(dev(pv), dev(pf), samples=32, radius=0.4, normals=up.repeat(6, 1))
    assert (near['ao'][:3] == 1).all()
    mid = np.concatenate([pv, np.zeros((1, 3), dtype=F32)])
    covered = geometry.ambient_occlusion(dev(mid), dev(pf), samples=32, normals=up.repeat(7, 1))
    assert covered['unoccluded'][6] == 0 and (covered['unoccluded'][3:6] == 32).all()


def test_occluded():
    verts, faces = mc48()
    v, f, tree = built(None)
    c = np.array(CENTRE, dtype=F32)
    a = np.array([c + (1.5, 0, 0), c + (1.5, 0, 0), c, c + (0.79, 0.0, 0.0)], dtype=F32)
    b = np.array([c - (1.5, 0, 0), c + (1.5, 1.0, 0), c + (0.2, 0.1, 0), c + (0.81, 0.0, 0.0)], dtype=F32)
    want = torch.tensor([True, False, False, True], device=DEV)                # through the sphere; outside on one side; inside; across the surface
    # the ends swapped: the hand-made segments only (b - a and a - b round differently, so on a family an edge-on answer could change)
    assert torch.equal(geometry.occluded(dev(a), dev(b), v, f, tree=tree), want) and torch.equal(geometry.occluded(dev(b), dev(a), v, f, tree=tree), want)
    assert torch.equal(geometry.occluded(dev(a), dev(b), v, f), want)
    assert np.array_equal(geometry.occluded(a, b, verts, faces), want.cpu().numpy())


def test_error_paths():
    v, f, tree = built(L + 1)
    o, d, t_lo, t_hi = (dev(x) for x in rays(L + 1)[:4])
    order = tree.order.int().contiguous()
    boxes = tree.boxes
    lib = _lib.load()
    n = o.shape[0]
    hit, t, face = torch.empty(n, dtype=torch.uint8, device=DEV), torch.empty(n, device=DEV), torch.empty(n, dtype=torch.int32, device=DEV)
    bary, point = torch.empty(n, 3, device=DEV), torch.empty(n, 3, device=DEV)
    p = lambda x: ctypes.c_void_p(x.data_ptr())
    host = ctypes.c_void_p(np.zeros(3 * n, dtype=F32).ctypes.data)

    def tree_call(origins=None, count=n, usable=tree.usable, nodes=boxes.shape[0]):
        return lib.ia_ray_mesh_tree(origins or p(o), p(d), p(t_lo), p(t_hi), count, p(tree.tris), p(order), usable, p(boxes), nodes,
                                    float(tree.extent), 0, p(hit), p(t), p(face), p(bary), p(point), None, None)

    def brute_call(origins=None, count=n, usable=tree.usable):
        return lib.ia_ray_mesh_brute(origins or p(o), p(d), p(t_lo), p(t_hi), count, p(tree.tris), p(order), usable, 0, p(hit), p(t), p(face),
                                     p(bary), p(point), None)

    def refused(status, name):
        assert status == -1 and name in _lib.last_error(), (status, _lib.last_error())

    refused(tree_call(nodes=boxes.shape[0] + 1), 'ia_ray_mesh_tree')
    refused(tree_call(origins=host), 'ia_ray_mesh_tree')
    refused(tree_call(usable=(1 << 25) + 1), 'ia_ray_mesh_tree')
    refused(tree_call(usable=-1), 'ia_ray_mesh_tree')
    refused(tree_call(count=(1 << 31) // 3 + 1), 'ia_ray_mesh_tree')
    refused(brute_call(origins=host), 'ia_ray_mesh_brute')
    refused(brute_call(usable=(1 << 25) + 1), 'ia_ray_mesh_brute')
    refused(brute_call(count=(1 << 31) // 3 + 1), 'ia_ray_mesh_brute')
    assert tree_call(count=0) == 0 and brute_call(count=0) == 0
    assert lib.ia_ray_mesh_tree(p(o), p(d), p(t_lo), p(t_hi), n, None, None, 0, None, 0, 0.0, 0, p(hit), p(t), p(face), p(bary), p(point), None, None) == 0
    assert lib.ia_ray_mesh_brute(p(o), p(d), p(t_lo), p(t_hi), n, None, None, 0, 0, p(hit), p(t), p(face), p(bary), p(point), None) == 0
    torch.cuda.synchronize()
    assert not hit.any() and (face == -1).all()
    table = dev(geometry._ao_table(4, 0))
    nrm = torch.zeros_like(v)
    oo, dd = torch.empty(v.shape[0] * 4, 3, device=DEV), torch.empty(v.shape[0] * 4, 3, device=DEV)
    refused(lib.ia_ao_rays(host, p(nrm), v.shape[0], p(table), 4, 0.0, p(oo), p(dd), None), 'ia_ao_rays')
    refused(lib.ia_ao_rays(p(v), p(nrm), v.shape[0], p(table), 0, 0.0, p(oo), p(dd), None), 'ia_ao_rays')
    refused(lib.ia_ao_rays(p(v), p(nrm), (1 << 31) // 12 + 1, p(table), 4, 0.0, p(oo), p(dd), None), 'ia_ao_rays')
    assert lib.ia_ao_rays(None, None, 0, p(table), 4, 0.0, None, None, None) == 0
    with pytest.raises(RuntimeError):
        hipops.ray_mesh_tree(o, d, t_lo, t_hi, tree.tris, tree.order, boxes, tree.usable, tree.extent)          # int64 order
    with pytest.raises(RuntimeError):
        hipops.ray_mesh_tree(o, d, t_lo, t_hi, tree.tris, order, boxes[:-1].contiguous(), tree.usable, tree.extent)   # a node short
    with pytest.raises(ValueError):
        geometry.ray_mesh(o, d, v, f, tree=tree_of(L + 1))                                                    # a host tree for a device mesh
    torch.cuda.synchronize()
