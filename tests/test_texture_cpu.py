"""The texture atlas of geometry.py (TextureAtlas, atlas_points, bake_texture, project_texture, sample_texture, write_obj / read_obj), the
NumPy restatement that is the definition: the layout, affine reproduction through the bilinear lookup, projective
texturing on a sphere and the OBJ round trip.  The fixtures here are shared with tests/test_texture_gpu.py.

Projection: a guard texel (lambda_0 < 0) is extrapolated off the surface and a texel within a pixel of a view's silhouette can find the
mask unset whatever the tolerance, so 'every texel with c > min_cos in some view is filled' is asserted for the texels inside their
triangle at min_cos = 0.5 (30 degrees from the silhouette, where a 32^2 pixel cannot reach it), and at the default min_cos = 0.2 it is
asserted that the depth test with the default tolerance rejects no such texel whose pixel the mesh covers.  Measured with 3 views at
32^2 on the 128^2 atlas: 8123 texel-views inside their triangle face a camera at c > 0.2, 312 of them find the mask unset."""
import functools
import os

import numpy as np
import pytest
import torch

from invertavatar_amd import geometry
from test_mesh_raster_cpu import icosphere, label, sphere_case

F32 = np.float32
EPS32 = float(np.finfo(np.float32).eps)
RES = 32

LAYOUTS = [(1, 16, 4), (2, 16, 4), (3, 16, 4), (7, 16, 4), (99, 50, 6), (320, 64, None), (320, 128, None)]      # F, size, block


def sphere():
    v, f, cams, _ = sphere_case()
    return v, f, cams


def mesh_of(F):
    v, f, _ = sphere()
    return v, f[:F]


@functools.lru_cache(None)
def rasters(n_faces=320):
    v, f, cams = sphere()
    return geometry.rasterize_mesh(v, f[:n_faces], cams, RES)


def affine(p):
    """Three channels, each an affine function of position."""
    A = np.array([[0.7, -0.2, 0.4], [-0.3, 0.5, 0.1], [0.2, 0.6, -0.5]])
    return p @ A.T.astype(p.dtype) + np.array([0.5, 0.4, 0.6]).astype(p.dtype)


@functools.lru_cache(None)
def sphere_images():
    """[3,RES,RES,3]: per pixel the affine function of the raster's hit point, 0 on a miss."""
    v, f, cams = sphere()
    r = rasters()
    hit = (r['bary'][..., None] * v[f[np.maximum(r['face'], 0)]]).sum(-2)
    return np.where(r['mask'][..., None], affine(hit.astype(np.float64)), 0).astype(F32)


def cosines(pts, cams):
    """float64 [N,size,size]: c = n . (o - X) / |o - X| of every texel and view."""
    o = cams[:, :16].reshape(-1, 4, 4)[:, :3, 3].astype(np.float64)
    e = o[:, None, None] - pts['point'].astype(np.float64)[None]
    return (e * pts['normal'].astype(np.float64)[None]).sum(-1) / np.linalg.norm(e, axis=-1)


def pixels(pts, cams, res):
    """int [N,size,size] x 2: the pixel (rint u, rint v) of every texel in every view (float64), clipped into the image, and whether
    the projection lies inside it."""
    X = pts['point'].astype(np.float64)
    out = []
    for c in cams.astype(np.float64):
        M, K = c[:16].reshape(4, 4), c[16:].reshape(3, 3)
        xc = (X - M[:3, 3]) @ M[:3, :3]
        u = (K[0, 0] * res * xc[..., 0] + K[0, 1] * res * xc[..., 1]) / xc[..., 2] + K[0, 2] * res
        w = (K[1, 0] * res * xc[..., 0] + K[1, 1] * res * xc[..., 1]) / xc[..., 2] + K[1, 2] * res
        inside = (u >= 0) & (u <= res - 1) & (w >= 0) & (w <= res - 1) & (xc[..., 2] > 0)
        out.append((np.clip(np.rint(u), 0, res - 1).astype(np.int64), np.clip(np.rint(w), 0, res - 1).astype(np.int64), inside))
    return [np.stack([o[k] for o in out]) for k in range(3)]


# ------------------------------------------------------------------ layout

@pytest.mark.parametrize('F,size,block', LAYOUTS)
def test_layout(F, size, block):
    atlas = geometry.TextureAtlas(F, size, block)
    s, G = atlas.s, atlas.G
    assert s >= 4 and G == size // s and 2 * G * G >= F and (block is None or s == block)
    if block is None:
        assert (size // (s + 1)) ** 2 < -(-F // 2)                              # s is the largest that fits
    face = atlas.texel_face()
    assert face.dtype == np.int32 and face.shape == (size, size)
    j, i = np.meshgrid(np.arange(size), np.arange(size), indexing='ij')
    for b in range(-(-F // 2)):
        blk = face[(b // G) * s:(b // G + 1) * s, (b % G) * s:(b % G + 1) * s]
        assert blk.shape == (s, s)
        lower, upper = (blk == 2 * b).sum(), (blk == 2 * b + 1).sum()
        assert lower == s * (s + 1) // 2                                        # ownership partitions the block
        if 2 * b + 1 < F:
            assert upper == s * (s - 1) // 2 and lower + upper == s * s
        else:
            assert upper == 0 and (blk == -1).sum() == s * (s - 1) // 2           # an odd F leaves the last upper half unowned
    assert (face >= 0).sum() == (F // 2) * s * s + (F % 2) * (s * (s + 1) // 2)
    assert (face[(i >= G * s) | (j >= G * s)] == -1).all() and face.max() == F - 1
    # both charts have positive orientation and the corners are where the definition puts them
    c = atlas.corners()
    d1, d2 = c[:, 1] - c[:, 0], c[:, 2] - c[:, 0]
    assert (d1[:, 0] * d2[:, 1] - d1[:, 1] * d2[:, 0] == (s - 3) ** 2).all()
    assert np.array_equal(atlas.uv, ((c.astype(F32) + F32(0.5)) / F32(size))) and atlas.uv.dtype == F32 and atlas.uv.shape == (F, 3, 2)
    assert np.array_equal(face[c[..., 1], c[..., 0]], np.repeat(np.arange(F)[:, None], 3, 1))
    # the bilinear footprint of points of the uv triangle lies in texels the face owns
    rng = np.random.RandomState(F + size)
    bary = rng.dirichlet((1, 1, 1), (F, 1000))
    fixed = np.array([[1, 0, 0], [0, 1, 0], [0, 0, 1], [.5, .5, 0], [0, .5, .5], [.5, 0, .5]])
    bary = np.concatenate([bary, np.broadcast_to(fixed, (F, 6, 3))], 1)
    xy = np.einsum('fpk,fkc->fpc', bary, c.astype(np.float64))
    xy[:, 1000:] = np.einsum('pk,fkc->fpc', fixed, c.astype(np.float64))          # (exact)
    x0, y0 = np.floor(xy[..., 0]).astype(int), np.floor(xy[..., 1]).astype(int)
    fx, fy = xy[..., 0] - x0, xy[..., 1] - y0
    want = np.arange(F)[:, None]
    for dx, dy in ((0, 0), (1, 0), (0, 1), (1, 1)):
        used = ((fx > 0) | (dx == 0)) & ((fy > 0) | (dy == 0))                   # (a texel of weight 0 is not read: its index is clamped)
        xi, yi = np.minimum(x0 + dx, size - 1), np.minimum(y0 + dy, size - 1)
        assert (face[yi, xi] == want)[used].all(), (dx, dy)
        bx, by = ((want >> 1) % G) * s, ((want >> 1) // G) * s
        assert (((xi >= bx) & (xi < bx + s) & (yi >= by) & (yi < by + s)) | ~used).all()


def test_capacity_errors_name_the_size():
    with pytest.raises(ValueError, match='smallest size that fits is 52'):
        geometry.TextureAtlas(320, 51)
    assert geometry.TextureAtlas(320, 52).s == 4
    with pytest.raises(ValueError, match='smallest size that fits is 78'):
        geometry.TextureAtlas(320, 50, block=6)
    with pytest.raises(ValueError, match='block must be >= 4'):
        geometry.TextureAtlas(2, 16, block=3)
    assert geometry.TextureAtlas(0, 8).texel_face().max() == -1


# ------------------------------------------------------------------ points and the lookup

@pytest.mark.parametrize('F,size,block', LAYOUTS)
def test_atlas_points(F, size, block):
    v, f = mesh_of(F)
    atlas = geometry.TextureAtlas(F, size, block)
    pts = geometry.atlas_points(v, f, atlas)
    face, own = pts['face'], pts['face'] >= 0
    assert np.array_equal(face, atlas.texel_face()) and pts['info'] == {'degenerate': 0}
    assert all(pts[k].dtype == F32 and pts[k].shape == (size, size, 3) for k in ('point', 'bary', 'normal'))
    assert not pts['point'][~own].any() and not pts['bary'][~own].any() and not pts['normal'][~own].any()
    b = pts['bary'][own].astype(np.float64)
    assert np.abs(b.sum(1) - 1).max() <= 4 * EPS32 and b[:, 0].min() < 0 <= b[:, 1:].min()      # guard texels extrapolate
    # the corner texels are the vertices, and every point lies on its face's plane
    c = atlas.corners()
    assert np.array_equal(pts['point'][c[..., 1], c[..., 0]], v[f])
    A = v[f[face[own]]].astype(np.float64)
    n = np.cross(A[:, 1] - A[:, 0], A[:, 2] - A[:, 0])
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    assert np.abs(((pts['point'][own] - A[:, 0]) * n).sum(1)).max() <= 16 * EPS32
    assert np.abs(pts['normal'][own] - n).max() <= 4 * EPS32
    smooth = geometry.atlas_points(v, f, atlas, normals=(v / np.linalg.norm(v, axis=1, keepdims=True)).astype(F32))['normal']
    assert np.abs(np.linalg.norm(smooth[own], axis=1) - 1).max() <= 4 * EPS32 and not np.array_equal(smooth, pts['normal'])
    t = geometry.atlas_points(torch.from_numpy(v), torch.from_numpy(f), atlas)
    assert isinstance(t['point'], torch.Tensor) and np.array_equal(t['point'].numpy(), pts['point']) and t['face'].dtype == torch.int32


def degenerate_mesh():
    """Seven faces: 1 has no area, 4 a non-finite vertex."""
    v, f = mesh_of(7)
    v, f = v.copy(), f.copy()
    f[1] = [f[1, 0], f[1, 1], f[1, 0]]
    v[f[4, 2]] = [np.nan, 1, np.inf]
    return v, f


def test_degenerate_faces_are_counted_not_skipped():
    v, f = degenerate_mesh()
    atlas = geometry.TextureAtlas(7, 16, 4)
    with np.errstate(all='ignore'):
        pts = geometry.atlas_points(v, f, atlas)
    bad = np.isin(f, f[4, 2]).any(1) | (np.arange(7) == 1)
    assert pts['info']['degenerate'] == int(bad.sum()) and bad[4] and bad[1]
    face = pts['face']
    for k in range(7):
        assert bool(pts['normal'][face == k].any()) == (not bad[k]), k
    assert np.array_equal(pts['point'][face == 1][0], v[f[1, 0]])                 # the points the formula gives
    assert not np.isfinite(pts['point'][face == 4]).all()


@pytest.mark.parametrize('F,size,block', [(99, 50, 6), (320, 64, None), (320, 128, None)])
def test_affine_functions_are_reproduced(F, size, block):
    v, f = mesh_of(F)
    atlas = geometry.TextureAtlas(F, size, block)
    baked = geometry.bake_texture(v, f, size, affine, atlas=atlas, chunk=1000)
    assert baked['texture'].shape == (size, size, 3) and baked['texture'].dtype == F32 and np.array_equal(baked['mask'], atlas.texel_face() >= 0)
    rng = np.random.RandomState(size)
    face = rng.randint(0, F, 4000).astype(np.int32)
    bary = rng.dirichlet((1, 1, 1), 4000).astype(F32)
    face[:3], bary[:3] = [0, 1, F - 1], np.eye(3, dtype=F32)                      # corners, among them x = s - 1 exactly
    got = geometry.sample_texture(baked['texture'], atlas, face, bary)
    assert got.dtype == F32 and got.shape == (4000, 3)
    # the same in double: points, function and lookup
    p64 = geometry.atlas_points(v, f, atlas, dtype=np.float64)
    tex64 = np.where((p64['face'] >= 0)[..., None], affine(p64['point']), 0)
    got64 = geometry.sample_texture(tex64, atlas, face, bary, dtype=np.float64)
    want = affine(np.einsum('pk,pkc->pc', bary.astype(np.float64), v[f[face]].astype(np.float64)))
    e64, e32 = np.abs(got64 - want).max(), np.abs(got - got64).max()
    tol = 4 * e32 + EPS32 * np.abs(want).max()
    print(f'affine reproduction, size {size}, s {atlas.s}: double {e64:.3e}, float32 against double {e32:.3e}, float32 against f {np.abs(got - want).max():.3e}, bound {tol:.3e}')
    # no clamping, no bleeding: what is left in double is the float32 rounding of the uv corners (2^-24 of u <= 1 is size 2^-24 texels
    # of a function that changes by less than its range per texel) and of barycentrics that add up to 1 within eps32
    assert e64 <= 8 * EPS32 * np.abs(want).max()
    assert np.abs(got - want).max() <= tol
    assert not geometry.sample_texture(baked['texture'], atlas, np.array([-1, F], dtype=np.int32), bary[:2]).any()


def test_distance_bake():
    v, f = mesh_of(320)
    ref = (v * F32(1.1)).astype(F32)
    out = geometry.bake_texture(v, f, 64, lambda p: geometry.closest_point(p, ref, f, brute=True)['dist'])
    d = out['texture'][out['mask'] & (out['points']['bary'][..., 0] >= 0)]        # on the surface: 0.05 under the reference's facets at most
    assert out['texture'].shape == (64, 64, 1) and 0.04 < d.min() and d.max() < 0.051 and not out['texture'][~out['mask']].any()
    assert (out['texture'] >= 0).all()


# ------------------------------------------------------------------ projection

@functools.lru_cache(None)
def projection_case(size=128):
    v, f, cams = sphere()
    atlas = geometry.TextureAtlas(len(f), size)
    return v, f, cams, atlas, geometry.atlas_points(v, f, atlas)


@pytest.mark.parametrize('size', [64, 128])
def test_projection_fills_what_faces_a_view(size):
    v, f, cams, atlas, pts = projection_case(size)
    r = rasters()
    out = geometry.project_texture(v, f, atlas, sphere_images(), cams, r['depth'], r['mask'])
    again = geometry.project_texture(v, f, atlas, sphere_images(), cams)         # depth and mask computed inside
    assert all(np.array_equal(out[k], again[k]) for k in out)
    assert out['texture'].shape == (size, size, 3) and out['views'].dtype == np.int32 and out['filled'].dtype == bool
    c = cosines(pts, cams)
    own = pts['face'] >= 0
    inside = own & (pts['bary'][..., 0] >= 0)
    pi, pj, in_image = pixels(pts, cams, RES)
    covered = np.stack([r['mask'][n][pj[n], pi[n]] for n in range(len(cams))]) & in_image
    # per view: the restatement's own verdicts (float32) against the float64 cosine, away from the threshold by 1e-5
    tol = geometry.TEXTURE_DEPTH_TOL * 1.0 / RES
    verdict = np.zeros((len(cams), size, size), bool)
    views = geometry._texture_views_numpy(pts['point'][own], pts['normal'][own], cams, r['depth'], r['mask'], RES, RES, 1e-6, 0.2, tol, F32)
    for n, (ok, _, _, _) in enumerate(views):
        verdict[n][own] = ok
    assert np.array_equal(verdict.sum(0), out['views']) and np.array_equal(out['filled'], out['views'] > 0)
    facing = inside[None] & (c > 0.2 + 1e-5)
    print(f'size {size}: {int(facing.sum())} texel-views inside their triangle face a camera, {int((facing & ~covered).sum())} find the mask unset')
    assert not (facing & covered & ~verdict).any()                               # the depth test rejects nothing that faces the camera
    assert not (verdict & (c <= 0.2 - 1e-5)).any() and not verdict[:, ~own].any()
    # every texel (inside its triangle) that faces some view by more than 30 degrees from the silhouette is filled
    steep = geometry.project_texture(v, f, atlas, sphere_images(), cams, r['depth'], r['mask'], min_cos=0.5)
    assert steep['filled'][inside & (c > 0.5 + 1e-5).any(0)].all()
    # no texel on the far side passes any view
    assert not out['filled'][own & (c <= 0).all(0)].any() and (own & (c <= 0).all(0)).sum() > 50
    assert not out['texture'][~out['filled']].any() and not out['weight'][~out['filled']].any()
    # the colours are those of the surface: the images are an affine function of the hit point, which a facet of the sphere and the
    # bilinear read reproduce up to the facets' edges; from views within 45 degrees (a pixel is 0.055 wide, 0.08 along the surface, under
    # which a sphere of radius 0.5 departs from its chord by 0.002) within 2 % of the range
    front = geometry.project_texture(v, f, atlas, sphere_images(), cams, r['depth'], r['mask'], min_cos=0.7)
    sure = inside & front['filled']
    worst = np.abs(front['texture'][sure] - affine(pts['point'][sure].astype(np.float64))).max()
    print(f'size {size}: projected colour against the function at the texel, {int(sure.sum())} texels, worst {worst:.3e}')
    assert worst < 0.02 and sure.sum() > 200


def test_best_view_and_blend():
    v, f, cams, atlas, pts = projection_case()
    r = rasters()
    imgs = np.stack([np.full((RES, RES, 2), k + 1, F32) for k in range(3)])        # the view's number as its colour
    best = geometry.project_texture(v, f, atlas, imgs, cams, r['depth'], r['mask'], mode='best')
    blend = geometry.project_texture(v, f, atlas, imgs, cams, r['depth'], r['mask'], power=3)
    assert np.array_equal(best['views'], blend['views']) and np.array_equal(best['filled'], blend['filled'])
    own = pts['face'] >= 0
    verdict = np.zeros((3,) + own.shape, bool)
    cos32 = np.zeros((3,) + own.shape, F32)
    tol = geometry.TEXTURE_DEPTH_TOL * 1.0 / RES
    for n, (ok, _, _, c) in enumerate(geometry._texture_views_numpy(pts['point'][own], pts['normal'][own], cams, r['depth'], r['mask'], RES, RES, 1e-6, 0.2, tol, F32)):
        verdict[n][own], cos32[n][own] = ok, c
    filled = best['filled']
    pick = np.where(verdict, cos32, -1).argmax(0)                                 # the largest cosine, the lowest view among equals
    assert np.array_equal(best['texture'][filled][:, 0], (pick + 1).astype(F32)[filled]) and (verdict.sum(0) > 1).sum() > 500
    assert np.array_equal(best['weight'][filled], (cos32 * cos32).max(0)[filled])  # power 2: c c
    w = (cos32 * cos32) * cos32                                                     # power 3: (c c) c, float32
    num = sum(np.where(verdict[k], (w[k] * F32(k + 1)).astype(np.float64), 0) for k in range(3))
    den = sum(np.where(verdict[k], w[k].astype(np.float64), 0) for k in range(3))
    assert np.array_equal(blend['texture'][filled][:, 1], (num[filled] / den[filled]).astype(F32))
    assert np.array_equal(blend['weight'][filled], den[filled].astype(F32))
    half = geometry.project_texture(v, f, atlas, imgs[:2], cams[:2], r['depth'][:2], r['mask'][:2], power=0.5)
    assert np.isfinite(half['texture']).all() and half['filled'].sum() > 1000


@functools.lru_cache(None)
def shadow_case():
    """The sphere with a small sphere (radius 0.1) between it and camera 0, 1.9 from the centre."""
    v, f, cams = sphere()
    o = cams[0, :16].reshape(4, 4)[:3, 3]
    sv, sf = icosphere(1, 0.1)
    return np.concatenate([v, sv + (o / np.linalg.norm(o) * 1.9).astype(F32)]), np.concatenate([f, sf + len(v)]), cams


def test_occluder_takes_view_0_from_the_shadowed_texels_and_fallback_fills():
    v, f, cams, atlas, pts = projection_case()
    v2, f2, _ = shadow_case()
    tol = geometry.TEXTURE_DEPTH_TOL * 1.0 / RES                                    # the sphere's own default
    r, r2 = rasters(), geometry.rasterize_mesh(v2, f2, cams, RES)
    free = geometry.project_texture(v, f, atlas, sphere_images(), cams, r['depth'], r['mask'], depth_tol=tol)
    shaded = geometry.project_texture(v, f, atlas, sphere_images(), cams, r2['depth'], r2['mask'], depth_tol=tol)
    own = pts['face'] >= 0
    one = lambda rr: geometry.project_texture(v, f, atlas, sphere_images()[:1], cams[:1], rr['depth'][:1], rr['mask'][:1], depth_tol=tol)['filled']
    pi, pj, _ = pixels(pts, cams, RES)
    behind = r2['face'][0][pj[0], pi[0]] >= len(f)                                 # the occluder covers the texel's pixel in view 0
    lost = one(r) & ~one(r2)
    assert np.array_equal(lost, one(r) & behind) and lost.sum() > 100 and not (one(r2) & ~one(r)).any()
    assert np.array_equal(free['views'] - shaded['views'], lost.astype(np.int32))
    assert (r2['face'][1:] < len(f)).all()                                         # (the other views do not see the occluder on the sphere)
    # fallback fills exactly what no view passes
    fb = np.full((atlas.size, atlas.size, 3), 0.25, F32)
    with_fb = geometry.project_texture(v, f, atlas, sphere_images(), cams, r['depth'], r['mask'], fallback=fb)
    assert np.array_equal(with_fb['filled'], free['filled']) and (with_fb['texture'][~free['filled']] == 0.25).all()
    assert np.array_equal(with_fb['texture'][free['filled']], free['texture'][free['filled']]) and not with_fb['weight'][~free['filled']].any()


def test_argument_errors():
    v, f, cams, atlas, _ = projection_case()
    img = sphere_images()
    for kw in ({'mode': 'mean'}, {'power': -1}, {'depth_tol': -1.0}, {'depth': rasters()['depth']}, {'fallback': np.zeros((4, 4, 3), F32)}):
        with pytest.raises(ValueError):
            geometry.project_texture(v, f, atlas, img, cams, **kw)
    with pytest.raises(ValueError):
        geometry.project_texture(v, f, atlas, np.zeros((3, RES, RES, 9), F32), cams)
    with pytest.raises(ValueError):
        geometry.atlas_points(v, f[:10], atlas)
    with pytest.raises(ValueError):
        geometry.sample_texture(np.zeros((8, 8, 3), F32), atlas, np.zeros(2, np.int32), np.zeros((2, 3), F32))


# ------------------------------------------------------------------ files and the command line

def test_obj_round_trip(tmp_path):
    v, f = mesh_of(99)
    atlas = geometry.TextureAtlas(99, 50, 6)
    tex = np.clip(geometry.bake_texture(v, f, 50, affine, atlas=atlas)['texture'], 0, 1)
    nrm = (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(F32)
    path = str(tmp_path / 'ball.obj')
    geometry.write_obj(path, v, f, atlas.uv, tex, nrm)
    assert all(os.path.exists(str(tmp_path / n)) for n in ('ball.obj', 'ball.mtl', 'ball.png'))
    assert 'map_Kd ball.png' in open(str(tmp_path / 'ball.mtl')).read()
    back = geometry.read_obj(path)
    used = np.unique(f)
    assert np.array_equal(back['verts'], v) and np.array_equal(back['faces'], f) and np.array_equal(back['uv'], atlas.uv)
    assert np.array_equal(back['normals'][used], nrm[used])
    assert back['texture'].shape == tex.shape and np.abs(back['texture'] - tex).max() <= 0.5 / 255 + 1e-6
    text = open(path).read().split('\n')
    assert sum(l.startswith('vt ') for l in text) == 3 * 99 and text[-2].count('/') == 6
    v_of_first = float(next(l for l in text if l.startswith('vt ')).split()[2])
    assert v_of_first == 1.0 - float(atlas.uv[0, 0, 1])                           # OBJ's origin is bottom-left
    geometry.write_obj(str(tmp_path / 'plain.obj'), v, f, atlas.uv, tex[..., 0])
    plain = geometry.read_obj(str(tmp_path / 'plain.obj'))
    assert plain['normals'] is None and plain['texture'].shape == (50, 50, 1)


def test_command_line_without_texture_writes_the_same_bytes(tmp_path):
    from invertavatar_amd import extract_geometry
    args = ['--seeds', '0', '--width', 'small', '--level', '0', '--device', 'cpu', '--res', '12', '--normals']
    a, b = tmp_path / 'a', tmp_path / 'b'
    extract_geometry.main(args + ['--outdir', str(a)])
    (path, out), = extract_geometry.main(args + ['--outdir', str(b), '--texture', '128'])
    assert sorted(os.listdir(str(a))) == ['seed0000.ply']
    assert sorted(os.listdir(str(b))) == ['seed0000.mtl', 'seed0000.obj', 'seed0000.ply', 'seed0000.png']
    assert open(str(a / 'seed0000.ply'), 'rb').read() == open(str(b / 'seed0000.ply'), 'rb').read()
    back = geometry.read_obj(str(b / 'seed0000.obj'))
    assert np.array_equal(back['faces'], out['faces'].numpy()) and back['texture'].shape == (128, 128, 3)
    assert np.array_equal(back['uv'], out['uv']) and out['texture_info']['filled'].sum() > 0
