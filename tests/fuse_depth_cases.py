"""Shared inputs of tests/test_fuse_depth_cpu.py and tests/test_fuse_depth_gpu.py: cameras, analytic depth images of a sphere seeded with
unusable values, the device cases (whose builder asserts on the CPU that every branch of the definition is taken), the float32 references
and the end-to-end sphere.  Everything is computed once per process and never modified."""
import functools

import numpy as np
import torch

from invertavatar_amd import geometry
from invertavatar_amd.training_avatar_texture.camera_utils import FOV_to_intrinsics, LookAtPoseSampler
from test_mesh_raster_cpu import icosphere, label

F32 = np.float32
EPS32 = float(np.finfo(np.float32).eps)
RADIUS = 0.4                     # the sphere of the analytic depth images
SUMS = ('sum', 'weight', 'color_sum', 'color_weight')


def orbit(n, seed, fov=36.0, radius=2.2):
    """n seeded cameras [n,25] on a sphere of ``radius`` that look at the origin; the field of view is narrow enough that the corners of
    a lattice over [-0.6, 0.6]^3 fall outside the image while the sphere is in view."""
    rng = np.random.default_rng(seed)
    K = FOV_to_intrinsics(fov).numpy()
    poses = [LookAtPoseSampler.sample(float(rng.uniform(0, 2 * np.pi)), float(rng.uniform(0.6, 2.5)), torch.zeros(3), radius=radius).numpy()
             for _ in range(n)]
    return np.concatenate([label(p, K) for p in poses])


def inside_camera():
    """A camera inside the lattice, looking down +z from (0.1, 0.05, 0): lattice points behind it have xc_z <= near."""
    m = np.eye(4)
    m[:3, 3] = [0.1, 0.05, 0.0]
    return label(m, FOV_to_intrinsics(60.0).numpy())


def sphere_depth(cams, H, W, radius=RADIUS):
    """float32 [N,H,W]: the ray parameter at which the unit ray of every pixel first meets the sphere of ``radius`` about the origin
    (from inside: where it leaves it), 0 on a miss; computed in float64."""
    R, o, k = geometry._camera_numpy(np.asarray(cams, dtype=F32), H, W, np.float64)
    out = np.zeros((cams.shape[0], H, W))
    jj, ii = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing='ij')
    for n in range(cams.shape[0]):
        xs, ys = ii - k[n, 2], jj - k[n, 5]
        det = k[n, 0] * k[n, 4] - k[n, 1] * k[n, 3]
        d = np.stack([(k[n, 4] * xs - k[n, 1] * ys) / det, (k[n, 0] * ys - k[n, 3] * xs) / det, np.ones_like(xs)], -1)
        d = (d / np.linalg.norm(d, axis=-1, keepdims=True)) @ R[n].T
        b = d @ o[n]
        disc = b * b - (o[n] @ o[n] - radius * radius)
        root = np.sqrt(np.maximum(disc, 0))
        t = np.where(-b - root > 0, -b - root, -b + root)
        out[n] = np.where((disc > 0) & (t > 0), t, 0.0)
    return out.astype(F32)


class Case:
    """One device case: lattice ``dims`` over a box a little larger than the sphere (a spacing of its own per axis), images H x W from
    ``n_views`` cameras (the last one inside the lattice when there are three or more), C colour channels, and optional mask and
    weights.  The depth images are seeded with 0 (the misses), negatives, NaN and inf; the weights with 0, negatives and NaN.  The
    truncation is 0.08, so that behind the surface s < -tau occurs and far in front of it the clamp.  ``hits`` counts what the builder
    asserts."""

    def __init__(self, dims, hw, n_views, channels, optional, seed=0):
        self.dims, (self.H, self.W), self.N, self.C = dims, hw, n_views, channels
        rng = np.random.default_rng(1000 * seed + 7 * n_views + dims[0] + hw[0] + channels)
        lo, hi = np.array([-0.6, -0.55, -0.5]), np.array([0.6, 0.58, 0.52])
        self.origin = tuple(float(x) for x in lo)
        self.spacing = tuple(float((hi[a] - lo[a]) / (dims[a] - 1)) for a in range(3))
        self.tau, self.near = 0.08, 1e-6
        cams = orbit(n_views, seed + n_views)
        if n_views >= 3:
            cams[-1] = inside_camera()[0]
        self.cams = cams
        H, W = hw
        depth = sphere_depth(cams, H, W)
        flat = depth.reshape(-1)
        bad = rng.permutation(flat.shape[0])[:max(flat.shape[0] // 10, 6)]
        flat[bad] = np.resize(np.array([-0.5, np.nan, np.inf, -np.inf, 0.0, -0.0], dtype=F32), bad.shape[0])
        self.depth = depth
        self.mask = (rng.random(depth.shape) < 0.9) if optional else None
        self.weights = None
        if optional:
            w = rng.uniform(0.5, 1.5, depth.shape).astype(F32)
            wf = w.reshape(-1)
            badw = rng.permutation(wf.shape[0])[:max(wf.shape[0] // 12, 4)]
            wf[badw] = np.resize(np.array([0.0, -1.0, np.nan, np.inf], dtype=F32), badw.shape[0])
            self.weights = w
        self.colors = rng.random((n_views, channels, H, W)).astype(F32) if channels else None
        for a in (self.cams, self.depth, self.mask, self.weights, self.colors):
            if a is not None:
                a.setflags(write=False)
        self.axes = geometry._lattice_axes(dims, self.origin, self.spacing)
        dec = []
        sums = geometry._fuse_numpy(self.axes, self.depth, self.cams, self.tau, self.near, self.mask, self.weights, self.colors, None, F32, dec)
        self.code, self.pixel = dec[0]
        self.reference = self.fuse()
        self._check_branches(sums)

    def kwargs(self, views=slice(None)):
        pick = lambda a: None if a is None else a[views]
        return dict(origin=self.origin, spacing=self.spacing, truncation=self.tau, near=self.near, mask=pick(self.mask),
                    weights=pick(self.weights), colors=pick(self.colors))

    def fuse(self, views=slice(None), state=None, to=lambda a: a):
        """``geometry.fuse_depth`` of the views given, on arrays passed through ``to`` (the device tests move them there)."""
        kw = {k: (to(v) if isinstance(v, np.ndarray) else v) for k, v in self.kwargs(views).items()}
        return geometry.fuse_depth(to(self.depth[views]), to(self.cams[views]), self.dims, state=state, **kw)

    def _check_branches(self, sums):
        code, pixel = self.code, self.pixel
        looked = [self.depth[n].reshape(-1)[pixel[n][code[n] == -3]] for n in range(self.N)]
        looked = np.concatenate(looked)
        self.hits = {'added': int((code == 0).sum()), 'outside': int((code == -2).sum()), 'hidden': int((code == -4).sum()),
                     'unusable': int((code == -3).sum()), 'behind': int((code == -1).sum())}
        assert self.hits['added'] and self.hits['outside'], self.hits
        if self.dims[0] * self.dims[1] * self.dims[2] < 10000:                      # (the 315 points of the small lattice cannot take every branch)
            return
        assert self.hits['hidden'] and self.hits['unusable'], self.hits
        if self.N >= 3:
            assert self.hits['behind'], self.hits
            if self.mask is None:                                                  # every kind of unusable depth is looked up
                assert (looked == 0).any() and (looked < 0).any() and np.isnan(looked).any() and np.isinf(looked).any()
        F, Wt, Cs, CW = sums
        assert ((F == Wt) & (Wt > 0)).any()                                        # the clamp f = 1 in every view of a point
        if self.C:
            assert (CW < Wt).any() and (CW > 0).any()                              # colour only where s <= tau


LATTICES = ((9, 7, 5), (40, 33, 31))
IMAGES = ((12, 16), (17, 33))        # (H, W): 16 x 12 and 33 x 17 images
VIEWS = (1, 3, 7)
CHANNELS = (0, 1, 3, 8)


@functools.lru_cache(maxsize=None)
def case(dims, hw, n_views, channels, optional):
    return Case(dims, hw, n_views, channels, optional)


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


# ------------------------------------------------------------------ the end-to-end sphere

class SphereScan:
    """An icosphere (subdivision 3, radius 0.5) through ``rasterize_mesh`` from 8 cameras around it at 64^2, fused at 32^3 over the box
    of the back-projected pixels, with the normal image as colours."""

    def __init__(self):
        self.radius = 0.5
        self.verts, self.faces = icosphere(3, self.radius)
        K = FOV_to_intrinsics(30.0).numpy()
        poses = [LookAtPoseSampler.sample(np.pi / 2 + 2 * np.pi * k / 8, np.pi / 2 + 0.5 * np.sin(2.1 * k), torch.zeros(3), radius=2.7).numpy()
                 for k in range(8)]
        self.cams = np.concatenate([label(p, K) for p in poses])
        r = geometry.rasterize_mesh(self.verts, self.faces, self.cams, 64)
        self.depth, self.mask = r['depth'], r['mask']
        self.colors = np.ascontiguousarray(np.moveaxis(r['normal'], -1, 1) * F32(0.5) + F32(0.5))
        for a in (self.depth, self.mask, self.colors, self.cams):
            a.setflags(write=False)

    def fuse(self, dtype=np.float32, to=lambda a: a):
        return geometry.fuse_depth(to(self.depth), to(self.cams), 32, mask=to(self.mask), colors=to(self.colors), dtype=dtype)


@functools.lru_cache(maxsize=None)
def sphere_scan():
    return SphereScan()


@functools.lru_cache(maxsize=None)
def sphere_fusion(dtype=np.float32):
    return sphere_scan().fuse(dtype)
