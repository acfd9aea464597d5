"""geometry.rasterize_mesh, the NumPy restatement that is the definition: the fill rule partitions polygons, the
degenerate cases give hand-written images, pixels sit where ``RaySampler_zxc`` puts them, an independent fp64 ray caster agrees, and the
float32 run stays within a measured distance of the float64 run.  The fixtures here are shared with tests/test_mesh_raster_gpu.py.

Measured on the cases below (the asserted bounds are four times these; DESIGN.md 4.18 records them):
  pixel convention, float64 run, |n.d| >= 0.2: worst |o + depth d - sum bary X| = 5.86e-5, 1.16 z/f 2^-9 (a half-pixel error would be 1.3e-2);
  fp64 Moeller-Trumbore reference: 2.34 % of the pixels lie within 2^-7 px of a projected edge and are excluded (cap 10 %); on the
  others mask and face agree and the worst depth difference is 1.073e-3 (at grazing faces of the silhouette, where a
  lateral shift of the snapped edge is divided by |n.d|);
  float32 against float64 run: depth 2.19 eps32 relative, bary 1.01 eps32 absolute."""
import functools

import numpy as np
import pytest
import torch

from invertavatar_amd import geometry
from invertavatar_amd.training_avatar_texture.camera_utils import FOV_to_intrinsics, LookAtPoseSampler
from invertavatar_amd.training_avatar_texture.volumetric_rendering.ray_sampler import RaySampler_zxc

F32 = np.float32
EPS32 = float(np.finfo(np.float32).eps)
CONVENTION_WORST = 5.86e-5       # measured, see the module docstring
REFERENCE_DEPTH_WORST = 1.073e-3
F32_DEPTH_EPS = 2.19
F32_BARY_EPS = 1.01


# ------------------------------------------------------------------ fixtures

def icosphere(subdivisions=2, radius=0.5):
    """Outward-wound icosphere: 20 * 4^subdivisions faces."""
    t = (1 + 5 ** 0.5) / 2
    v = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t), (t, 0, -1), (t, 0, 1), (-t, 0, -1), (-t, 0, 1)]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    v = [np.array(p, dtype=np.float64) / np.linalg.norm(p) for p in v]
    for _ in range(subdivisions):
        mid, g = {}, []

        def midpoint(a, b):
            key = (min(a, b), max(a, b))
            if key not in mid:
                m = v[a] + v[b]
                v.append(m / np.linalg.norm(m))
                mid[key] = len(v) - 1
            return mid[key]
        for a, b, c in f:
            ab, bc, ca = midpoint(a, b), midpoint(b, c), midpoint(c, a)
            g += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = g
    return (np.array(v) * radius).astype(F32), np.array(f, dtype=np.int64)


def label(cam2world, K):
    return np.concatenate([np.asarray(cam2world, dtype=F32).reshape(-1), np.asarray(K, dtype=F32).reshape(-1)])[None]


@functools.lru_cache(None)
def sphere_case():
    """The 320-face icosphere of radius 0.5 from three cameras at radius 2.7 (field of view 36 degrees: the silhouette is in view), 48^2."""
    v, f = icosphere(2, 0.5)
    K = FOV_to_intrinsics(36.0).numpy()
    poses = [LookAtPoseSampler.sample(h, p, torch.zeros(3), radius=2.7).numpy() for h, p in ((np.pi / 2, np.pi / 2), (0.9, 1.2), (2.4, 1.9))]
    cams = np.concatenate([label(p, K) for p in poses])
    return v, f, cams, 48


PLANE_K = np.array([[0.5, 0, 0.5], [0, 0.5, 0.5], [0, 0, 1]], dtype=F32)      # K_res: focal res / 2, centre res / 2
FRONT = label(np.eye(4), PLANE_K)                                             # at the origin, looking down +z
BACK = label(np.array([[-1, 0, 0, 0], [0, 1, 0, 0], [0, 0, -1, 3], [0, 0, 0, 1]]), PLANE_K)      # at (0, 0, 3), looking down -z


def from_pixels(px, z, H, W):
    """World points that FRONT sees at pixel coordinates ``px`` [n,2] and depth z."""
    px, z = np.asarray(px, dtype=np.float64), np.broadcast_to(np.asarray(z, dtype=np.float64), (len(px),))
    return np.stack([(px[:, 0] - W / 2) / (W / 2) * z, (px[:, 1] - H / 2) / (H / 2) * z, z], 1).astype(F32)


BIG = [(-40, -40), (-40, 80), (80, -40)]                                      # faces FRONT (normal toward -z), covers any small viewport


def degenerate_cases():
    """name -> (verts, faces, cameras, resolution, kwargs, expected face image [N,H,W], expected culled [N]); images written by hand."""
    tri = np.array([[0, 1, 2]], dtype=np.int64)
    miss, hit = np.full((1, 4, 4), -1), np.zeros((1, 4, 4), dtype=np.int64)
    one = miss.copy()
    one[0, 2, 2] = 0
    cases = {
        'larger than the viewport': (from_pixels(BIG, 1, 4, 4), tri, FRONT, 4, {}, hit, [0]),
        'off screen': (from_pixels([(10, 10), (14, 10), (10, 14)], 1, 4, 4), tri, FRONT, 4, {}, miss, [0]),
        'vertex behind the camera': (from_pixels(BIG, [1, 1, -1], 4, 4), tri, FRONT, 4, {}, miss, [1]),
        'zero area': (from_pixels([(0, 0), (1, 1), (3, 3)], 1, 4, 4), tri, FRONT, 4, {}, miss, [0]),
        'below a pixel, no centre': (from_pixels([(1.2, 1.2), (1.8, 1.2), (1.2, 1.8)], 1, 4, 4), tri, FRONT, 4, {}, miss, [0]),
        'below a pixel, one centre': (from_pixels([(1.8, 1.8), (2.3, 1.9), (1.9, 2.3)], 1, 4, 4), tri, FRONT, 4, {}, one, [0]),
        'coincident': (from_pixels(BIG, 1, 4, 4), np.array([[0, 1, 2], [0, 1, 2]]), FRONT, 4, {}, hit, [0]),
        'no faces': (from_pixels(BIG, 1, 4, 4), np.zeros((0, 3), dtype=np.int64), FRONT, 4, {}, miss, [0]),
        'resolution 1': (from_pixels(BIG, 1, 1, 1), tri, FRONT, 1, {}, np.zeros((1, 1, 1), dtype=np.int64), [0]),
    }
    # Right triangle (0,0) (8,0) (0,4) at 5 x 9: its top and left edges own their centres, the hypotenuse i + 2 j = 8 does not.
    rows = [8, 6, 4, 2, 0]
    img = np.array([[[0 if i < n else -1 for i in range(9)] for n in rows]])
    for name, order in (('(H, W) = (5, 9)', [0, 1, 2]), ('(H, W) = (5, 9), other winding', [0, 2, 1])):
        cases[name] = (from_pixels([(0, 0), (8, 0), (0, 4)], 1, 5, 9), np.array([order]), FRONT, (5, 9), {}, img, [0])
    # Two parallel triangles, both wound toward FRONT, at z = 1 (face 0) and z = 2 (face 1), seen from both sides.
    v = np.concatenate([from_pixels(BIG, 1, 4, 4), from_pixels(BIG, 2, 4, 4)])
    f = np.array([[0, 1, 2], [3, 4, 5]])
    both = np.concatenate([FRONT, BACK])
    cases['parallel, cull none'] = (v, f, both, 4, {'cull': 'none'}, np.concatenate([hit, hit + 1]), [0, 0])
    cases['parallel, cull back'] = (v, f, both, 4, {'cull': 'back'}, np.concatenate([hit, miss]), [0, 0])
    return cases


HEPTAGON = [(-6, -6), (0, -8), (6, -6), (8, 0), (6, 6), (-6, 6), (-8, 0)]      # convex, integer, with horizontal, vertical-free and diagonal edges


def polygon_placements(integer, count=40, seed=0):
    """Convex 7-gons in pixel coordinates of a 24^2 viewport: the integer HEPTAGON at integer offsets, or 7 points of a circle of 9 px at
    random angles (gaps >= 0.3 rad) about a random centre."""
    rng = np.random.RandomState(seed)
    out = []
    while len(out) < count:
        if integer:
            out.append(np.array(HEPTAGON, dtype=np.float64) + 12 + rng.randint(-3, 4, size=2))
            continue
        ang = np.sort(rng.uniform(0, 2 * np.pi, 7))
        if np.diff(np.concatenate([ang, ang[:1] + 2 * np.pi])).min() < 0.3:
            continue
        out.append(np.stack([np.cos(ang), np.sin(ang)], 1) * 9 + 12 + rng.uniform(-1, 1, size=2))
    return out


def fan(apex):
    return np.array([[apex, (apex + k) % 7, (apex + k + 1) % 7] for k in range(1, 6)], dtype=np.int64)


def covers(px, faces, H=24, W=24):
    """Per-triangle coverage masks [F,H,W] of the restatement for polygon vertices ``px`` seen by FRONT at z = 1."""
    proj = geometry._project_numpy(from_pixels(px, 1, H, W), FRONT, H, W, 1e-6)
    return geometry._raster_faces_numpy(proj, 0, faces, H, W)[0], proj


# ------------------------------------------------------------------ partition

@pytest.mark.parametrize('integer', [False, True])
def test_fans_partition_the_polygon(integer):
    for px in polygon_placements(integer):
        a, proj = covers(px, fan(0))
        b, _ = covers(px, fan(3))
        assert a.sum(0).max() <= 1 and b.sum(0).max() <= 1                     # no pixel twice
        assert np.array_equal(a.any(0), b.any(0))                              # the same union from either apex
        nxt = np.roll(px, -1, 0)
        area, perimeter = 0.5 * abs((px[:, 0] * nxt[:, 1] - px[:, 1] * nxt[:, 0]).sum()), np.linalg.norm(nxt - px, axis=1).sum()
        assert abs(a.any(0).sum() - area) <= 0.5 * perimeter + 1                  # as many centres as the polygon has area
        if integer:
            assert not (proj['U'] % 256).any() and not (proj['V'] % 256).any()    # centres do lie on edges and vertices
            U, V = proj['U'][0] // 256, proj['V'][0] // 256
            # the top-left rule on the polygon itself: vertex 0 (top-left corner) is in, the bottom edge y = 18 + dy is out
            assert a.any(0)[V[0], U[0]] and not a.any(0)[V[5], U[5] + 3]
            # a centre on the shared diagonal (0) - (3) of the fan: covered exactly once
            assert a.sum(0)[(V[0] + V[3]) // 2, (U[0] + U[3]) // 2] == 1


# ------------------------------------------------------------------ hand-written images

@pytest.mark.parametrize('name', list(degenerate_cases()))
def test_degenerate_cases(name):
    v, f, cams, res, kw, face, culled = degenerate_cases()[name]
    for dtype in (np.float32, np.float64):
        out = geometry.rasterize_mesh(v, f, cams, res, dtype=dtype, **kw)
        assert np.array_equal(out['face'], face), (name, out['face'])
        assert np.array_equal(out['mask'], face >= 0) and out['culled'].tolist() == culled
        assert out['face'].dtype == np.int32 and out['mask'].dtype == bool and out['depth'].dtype == dtype and out['attributes'] is None
        assert not out['depth'][face < 0].any() and not out['normal'][face < 0].any() and not out['bary'][face < 0].any()
        hit = face >= 0
        assert np.allclose(out['bary'][hit].sum(-1), 1, atol=1e-5)
        if name.startswith('parallel'):
            # depth is the ray parameter: 1 or 2 along the axis pixel (2, 2) of the front view, 1 from the back
            assert abs(out['depth'][0, 2, 2] - 1) < 1e-6 and out['normal'][0, 2, 2].tolist() == [0, 0, -1]
            if kw['cull'] == 'none':
                assert abs(out['depth'][1, 2, 2] - 1) < 1e-6 and out['normal'][1, 2, 2].tolist() == [0, 0, -1]


def test_containers_and_arguments():
    v, f, cams, res = sphere_case()
    a = geometry.rasterize_mesh(v, f, cams[:1], (8, 12), attributes=v[:, :2])
    b = geometry.rasterize_mesh(torch.from_numpy(v), torch.from_numpy(f), torch.from_numpy(cams[:1]), (8, 12), attributes=torch.from_numpy(v[:, :2]))
    for k in a:
        assert isinstance(b[k], torch.Tensor) and np.array_equal(a[k], b[k].numpy()), k
    assert a['attributes'].shape == (1, 8, 12, 2) and a['culled'].shape == (1,)
    bad = cams[:1].copy()
    bad[0, 22] = 1e-3                                                          # a projective K
    for kw in (dict(cameras=bad), dict(attributes=np.zeros((len(v), 9), F32)), dict(cull='front'), dict(faces=f + 1), dict(near=-1.0),
               dict(normals=v[:5])):
        with pytest.raises(ValueError):
            geometry.rasterize_mesh(**dict(dict(verts=v, faces=f, cameras=cams[:1], resolution=8), **kw))


# ------------------------------------------------------------------ pixel convention, fp64 reference, fp32 against fp64

@functools.lru_cache(None)
def sphere_runs():
    v, f, cams, res = sphere_case()
    nrm = (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(F32)
    kw = dict(normals=nrm, attributes=np.ascontiguousarray(v * 2 + 1))
    return geometry.rasterize_mesh(v, f, cams, res, dtype=np.float32, **kw), geometry.rasterize_mesh(v, f, cams, res, dtype=np.float64, **kw)


@functools.lru_cache(None)
def sphere_rays():
    v, f, cams, res = sphere_case()
    c = torch.from_numpy(cams)
    o, d = RaySampler_zxc()(c[:, :16].reshape(-1, 4, 4), c[:, 16:].reshape(-1, 3, 3), res)
    return o.numpy().astype(np.float64).reshape(-1, res, res, 3), d.numpy().astype(np.float64).reshape(-1, res, res, 3)


def test_pixels_sit_where_the_ray_sampler_puts_them():
    v, f, cams, res = sphere_case()
    out = sphere_runs()[1]
    o, d = sphere_rays()
    m = out['mask']
    tri = v.astype(np.float64)[f[out['face'][m]]]                             # [hits, 3, 3]
    on_mesh = (out['bary'][m][:, :, None] * tri).sum(1)
    on_ray = o[m] + out['depth'][m][:, None] * d[m]
    n = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    facing = np.abs((n * d[m]).sum(1)) >= 0.2
    worst = float(np.linalg.norm(on_mesh - on_ray, axis=1)[facing].max())
    z_over_f = 2.7 / (float(cams[0, 16]) * res)
    print(f'pixel convention: {int(facing.sum())} of {int(m.sum())} hits, worst {worst:.3e} = {worst / (z_over_f * 2 ** -9):.2f} z/f 2^-9; '
          f'half a pixel is {0.5 * z_over_f:.3e}')
    assert int(facing.sum()) > 0.8 * m.sum() > 1000
    assert worst <= 4 * CONVENTION_WORST < 0.5 * z_over_f / 25


def first_hit_reference(v, f, o, d):
    """Brute-force Moeller-Trumbore in float64, two-sided: (t [rays], face [rays], -1 and inf on a miss)."""
    a, e1, e2 = v[f[:, 0]], v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]]
    p = np.cross(d[:, None], e2[None])
    det = (e1[None] * p).sum(-1)
    with np.errstate(all='ignore'):
        s = o[:, None] - a[None]
        u = (s * p).sum(-1) / det
        q = np.cross(s, e1[None])
        w = (d[:, None] * q).sum(-1) / det
        t = (e2[None] * q).sum(-1) / det
    ok = (det != 0) & (u >= 0) & (w >= 0) & (u + w <= 1) & (t > 0)
    t = np.where(ok, t, np.inf)
    face = t.argmin(1)
    best = t[np.arange(len(t)), face]
    return best, np.where(np.isfinite(best), face, -1)


def edge_distance_px(v, f, cam, res):
    """[res,res]: distance in pixels from every pixel centre to the nearest projected triangle edge (float64, unsnapped)."""
    c = cam.astype(np.float64)
    m, K = c[:16].reshape(4, 4), c[16:].reshape(3, 3) * np.array([[res], [res], [1.0]])
    xc = (v.astype(np.float64) - m[:3, 3]) @ m[:3, :3]
    p = xc @ K.T
    s = p[:, :2] / p[:, 2:]
    ii, jj = np.meshgrid(np.arange(res, dtype=np.float64), np.arange(res, dtype=np.float64))
    q = np.stack([ii, jj], -1).reshape(-1, 1, 2)
    best = np.full(len(q), np.inf)
    for a, b in ((0, 1), (1, 2), (2, 0)):
        A, e = s[f[:, a]][None], (s[f[:, b]] - s[f[:, a]])[None]
        t = np.clip(((q - A) * e).sum(-1) / (e * e).sum(-1), 0, 1)
        best = np.minimum(best, np.linalg.norm(q - (A + t[..., None] * e), axis=-1).min(1))
    return best.reshape(res, res)


def test_against_moeller_trumbore():
    """Excluded: 2.34 % of the pixels (within 2^-7 px of a projected edge); the cap is 10 %."""
    v, f, cams, res = sphere_case()
    out = sphere_runs()[1]
    o, d = sphere_rays()
    v64 = v.astype(np.float64)
    excluded, worst = 0, 0.0
    for n in range(len(cams)):
        t, face = first_hit_reference(v64, f, o[n].reshape(-1, 3), d[n].reshape(-1, 3))
        t, face = t.reshape(res, res), face.reshape(res, res)
        keep = edge_distance_px(v, f, cams[n], res) >= 2.0 ** -7
        excluded += int((~keep).sum())
        assert np.array_equal(out['mask'][n][keep], (face >= 0)[keep])
        assert np.array_equal(out['face'][n][keep], face[keep])
        both = keep & (face >= 0)
        assert both.sum() > 500 and (face < 0).sum() > 100                     # the silhouette is in view
        worst = max(worst, float(np.abs(out['depth'][n][both] - t[both]).max()))
    share = excluded / (len(cams) * res * res)
    print(f'Moeller-Trumbore: excluded {100 * share:.2f} % of the pixels, worst depth difference {worst:.3e}')
    assert share <= 0.10 and worst <= 4 * REFERENCE_DEPTH_WORST


def test_float32_run_against_float64_run():
    v, f, cams, res = sphere_case()
    a, b = sphere_runs()
    assert np.array_equal(a['mask'], b['mask']) and np.array_equal(a['culled'], b['culled'])      # coverage: the same integers
    m = a['mask']
    depth_err = float((np.abs(a['depth'].astype(np.float64) - b['depth'])[m] / b['depth'][m]).max() / EPS32)
    proj = geometry._project_numpy(v, cams, res, res, 1e-6, np.float64)
    for n in range(len(cams)):
        z = np.sort(geometry._raster_faces_numpy(proj, n, f, res, res, 'none', np.float64)[1], axis=0)[:2]
        with np.errstate(invalid='ignore'):
            clear = m[n] & (z[1] - z[0] > 4 * F32_DEPTH_EPS * EPS32 * z[0])
        assert clear.sum() > 0.9 * m[n].sum()
        assert np.array_equal(a['face'][n][clear], b['face'][n][clear])
    same = m & (a['face'] == b['face'])
    bary_err = float(np.abs(a['bary'].astype(np.float64) - b['bary'])[same].max() / EPS32)
    print(f'float32 against float64: depth {depth_err:.2f} eps32 (relative), bary {bary_err:.2f} eps32')
    assert depth_err <= 4 * F32_DEPTH_EPS and bary_err <= 4 * F32_BARY_EPS
    # A mix of three values of magnitude <= A with weights off by at most 4 * F32_BARY_EPS eps32 is off by 3 A * 4.04 eps32 plus three
    # roundings, under 16 A eps32; normalising a unit normal adds a few eps32: 64 eps32 for the normals, 128 eps32 for |a| <= 2.
    assert np.abs(a['normal'].astype(np.float64) - b['normal'])[same].max() <= 64 * EPS32
    assert np.abs(a['attributes'].astype(np.float64) - b['attributes'])[same].max() <= 64 * EPS32 * 2


# ------------------------------------------------------------------ the mesh of a volume against the ray cast of the volume

BAND_PX = 1                      # measured below: every pixel where the two masks differ touches the silhouette
INTERIOR_DEPTH_WORST = 1.227e-3  # measured below (1222 interior pixels; the lattice step is 4.3e-2, a chord of the radius-0.3 sphere sags 8e-4)


@functools.lru_cache(None)
def volume_case():
    """density = 0.3 - |x| on a 24^3 lattice over the unit cube, its marching-cubes mesh (NumPy), two orbit cameras at radius 2.7, 32^2."""
    ax, lo, step = geometry.lattice_axis(24, 1.0, 0.0)
    x, y, z = np.meshgrid(ax, ax, ax, indexing='ij')
    vol = (0.3 - np.sqrt(x * x + y * y + z * z)).astype(F32)
    v, f = geometry.marching_cubes(vol, 0.0, (float(lo),) * 3, (float(step),) * 3)[:2]
    K = FOV_to_intrinsics(18.837).numpy()
    cams = np.concatenate([label(LookAtPoseSampler.sample(h, np.pi / 2, torch.zeros(3), radius=2.7).numpy(), K) for h in (np.pi / 2, 2.0)])
    return vol, (float(lo),) * 3, (float(step),) * 3, np.asarray(v, dtype=F32), np.asarray(f, dtype=np.int64), cams, 32


def grow(mask, px):
    """The mask and every pixel within ``px`` (chessboard distance) of it, per view."""
    out = mask.copy()
    for _ in range(px):
        p = np.pad(out, ((0, 0), (1, 1), (1, 1)))
        out = np.stack([p[:, 1 + a:p.shape[1] - 1 + a, 1 + b:p.shape[2] - 1 + b] for a in (-1, 0, 1) for b in (-1, 0, 1)]).any(0)
    return out


def band_and_interior(mask_mesh, depth_mesh, mask_cast, depth_cast, band):
    """(every differing pixel lies within ``band`` px of the ray cast's silhouette, worst depth difference on the pixels further inside)."""
    edge = grow(mask_cast, band) & grow(~mask_cast, band)
    inside = mask_cast & mask_mesh & ~edge
    return bool((edge | (mask_mesh == mask_cast)).all()), float(np.abs(depth_mesh - depth_cast)[inside].max()), int(inside.sum())


def test_mesh_of_a_volume_against_its_ray_cast():
    vol, lo, step, v, f, cams, res = volume_case()
    c = torch.from_numpy(cams)
    o, d = RaySampler_zxc()(c[:, :16].reshape(-1, 4, 4), c[:, 16:].reshape(-1, 3, 3), res)
    cast = geometry.raycast(vol, 0.0, lo, step, o.numpy(), d.numpy())
    mesh = geometry.rasterize_mesh(v, f, cams, res)
    shape = (len(cams), res, res)
    in_band, worst, n = band_and_interior(mesh['mask'], mesh['depth'], cast['mask'].reshape(shape), cast['depth'].reshape(shape), BAND_PX)
    print(f'mesh of a volume: V {len(v)} F {len(f)}, band {BAND_PX} px, {n} interior pixels, worst depth difference {worst:.3e}')
    assert in_band and n > 800 and worst <= INTERIOR_DEPTH_WORST
