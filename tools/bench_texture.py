"""Times of the texture atlas on the device (one JSON line on stdout, kept in profiles/texture_bench.json).

The marching-cubes mesh of an analytic sphere (density = 0.3 - |x| on a ``--volume``^3 lattice over the unit cube, level 0), simplified to
``--faces`` triangles; atlas sizes 2048^2 and 4096^2.  Per size: ``ia_atlas_points``; the decoder bake end to end (``geometry.bake_colors`` on
the planes of the small synthetic generator); projection from 8 views of a yaw orbit at 512^2 (``geometry.project_texture`` with depth and
mask given, random images); a textured 512^2 view (``rasterize_mesh`` + ``sample_texture``, and the lookup alone).  The yardstick is the same
steps through PyTorch device ops: the texel points by index arithmetic and gathers, the projection by a matrix product, ``grid_sample`` of
depth, mask and images per view and a weighted sum, the lookup by ``grid_sample`` of the texture at the uv mix.  Median and range of
``--reps`` runs between two device events after one warm-up.
Usage: python tools/bench_texture.py [--volume 256] [--faces 100000] [--reps 5] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')
sys.path.insert(0, ROOT)


def spread(xs):
    return {'ms': round(statistics.median(xs), 4), 'min': round(min(xs), 4), 'max': round(max(xs), 4), 'n': len(xs)}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--volume', type=int, default=256)
    ap.add_argument('--faces', type=int, default=100000)
    ap.add_argument('--res', type=int, default=512)
    ap.add_argument('--views', type=int, default=8)
    ap.add_argument('--sizes', type=int, nargs='+', default=[2048, 4096])
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'texture_bench.json'))
    args = ap.parse_args(argv)
    import numpy as np
    import torch
    import torch.nn.functional as nnf
    from invertavatar_amd import build, geometry, hipops, synthetic
    from invertavatar_amd.training_avatar_texture.camera_utils import FOV_to_intrinsics, LookAtPoseSampler
    from invertavatar_amd.training_avatar_texture.triplane_v20 import TriPlaneGenerator
    dev = 'cuda'

    def timed(call):
        call()
        ms = []
        for _ in range(args.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            call()
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        return spread(ms)

    ax, lo, step = geometry.lattice_axis(args.volume, 1.0, 0.0)
    a = torch.from_numpy(ax).to(dev)
    vol = 0.3 - torch.sqrt(a[:, None, None] ** 2 + a[None, :, None] ** 2 + a[None, None, :] ** 2)
    v, f = geometry.marching_cubes(vol, 0.0, (float(lo),) * 3, (float(step),) * 3)[:2]
    simple = geometry.simplify_mesh(v, f, target_faces=args.faces)
    v, f = simple['verts'].contiguous(), simple['faces'].int().contiguous()
    F = int(f.shape[0])
    n, res = args.views, args.res
    K = FOV_to_intrinsics(18.837, device=dev).reshape(1, 9)
    cams = torch.cat([torch.cat([LookAtPoseSampler.sample(np.pi / 2 + 2 * np.pi * k / n, np.pi / 2, torch.zeros(3, device=dev), radius=2.7,
                                                          device=dev).reshape(1, 16), K], 1) for k in range(n)]).contiguous()
    images = torch.rand(n, res, res, 3, device=dev)
    raster = geometry.rasterize_mesh(v, f, cams, res)
    gen = TriPlaneGenerator(**synthetic.generator_kwargs('small')).eval().requires_grad_(False)
    synthetic.fill_parameters(gen)
    gen = gen.to(dev)
    with torch.no_grad():
        ws = gen.mapping(synthetic.latent(3, 1).to(dev), synthetic.conditioning_camera().to(dev), truncation_psi=0.7, truncation_cutoff=14)
        planes = geometry.generator_planes(gen, ws, {'uvcoords_image': synthetic.uv_conditions([0]).to(dev)}, noise_mode='const')
    box_warp = gen.rendering_kwargs['box_warp']
    result = {'device': torch.cuda.get_device_name(0), 'source_digest': build.source_digest(), 'volume': args.volume, 'verts': int(v.shape[0]),
              'faces': F, 'views': n, 'resolution': res, 'sizes': {}}
    fl = f.long()
    for size in args.sizes:
        atlas = geometry.TextureAtlas(F, size)
        s, G, L = atlas.s, atlas.G, atlas.s - 3
        uv = torch.from_numpy(atlas.uv).to(dev)

        def torch_points():
            j, i = torch.meshgrid(torch.arange(size, device=dev), torch.arange(size, device=dev), indexing='ij')
            li, lj = i % s, j % s
            up = li + lj >= s
            face = 2 * ((j // s) * G + i // s) + up
            own = (i < G * s) & (j < G * s) & (face < F)
            fi = torch.where(own, face, 0)
            l1 = torch.where(up, s - 1 - li, li).float() / L
            l2 = torch.where(up, s - 1 - lj, lj).float() / L
            l0 = 1 - l1 - l2
            A, B, C = (v[fl[fi, k]] for k in range(3))
            point = (l0[..., None] * A + l1[..., None] * B + l2[..., None] * C) * own[..., None]
            normal = nnf.normalize(torch.cross(B - A, C - A, dim=-1), dim=-1) * own[..., None]
            return point, normal, torch.where(own, face, -1).int()

        pts = geometry.atlas_points(v, f, atlas)
        depth_tol = geometry.TEXTURE_DEPTH_TOL * geometry._mesh_extent(v) / res

        def torch_project():
            X, nr = pts['point'].reshape(-1, 3), pts['normal'].reshape(-1, 3)
            num, den = torch.zeros(X.shape[0], 3, device=dev, dtype=torch.float64), torch.zeros(X.shape[0], device=dev, dtype=torch.float64)
            for k in range(n):
                M, Kk = cams[k, :16].view(4, 4), cams[k, 16:].view(3, 3)
                e = M[:3, 3] - X
                xc = -e @ M[:3, :3]
                u, w = (xc[:, 0] / xc[:, 2]) * Kk[0, 0] * res + Kk[0, 2] * res, (xc[:, 1] / xc[:, 2]) * Kk[1, 1] * res + Kk[1, 2] * res
                t = e.norm(dim=1)
                c = (nr * e).sum(1) / t
                grid = torch.stack([(u + 0.5) / res * 2 - 1, (w + 0.5) / res * 2 - 1], -1).view(1, 1, -1, 2)
                near = lambda x: nnf.grid_sample(x, grid, mode='nearest', align_corners=False).view(x.shape[1], -1)
                d, m = near(raster['depth'][k][None, None]), near(raster['mask'][k][None, None].float())
                col = nnf.grid_sample(images[k].permute(2, 0, 1)[None], grid, mode='bilinear', align_corners=False).view(3, -1).t()
                ok = (c > 0.2) & (m[0] > 0) & ((t - d[0]).abs() <= depth_tol) & (u >= 0) & (u <= res - 1) & (w >= 0) & (w <= res - 1)
                wgt = torch.where(ok, c * c, torch.zeros_like(c))
                num += (wgt[:, None] * col).double()
                den += wgt.double()
            return (num / den[:, None]).float().nan_to_num(0).view(size, size, 3)

        tex = geometry.project_texture(v, f, atlas, images, cams, raster['depth'], raster['mask'])['texture']

        def torch_sample():
            face, b = raster['face'].long().clamp(min=0), raster['bary']
            mix = (b[..., None] * uv[face]).sum(-2)
            out = nnf.grid_sample(tex.permute(2, 0, 1)[None].expand(n, -1, -1, -1), mix * 2 - 1, mode='bilinear', align_corners=False)
            return out * raster['mask'][:, None]

        fn = lambda p: geometry.query_planes(planes, gen.decoder, p[None], box_warp, rgb=True)['rgb'][0, :, :3].clamp(0, 1)

        def torch_bake():
            point, _, face = torch_points()
            own = face >= 0
            t = torch.zeros(size, size, 3, device=dev)
            t[own] = torch.cat([fn(c) for c in point[own].split(1 << 20)])
            return t

        r = {'block': s, 'blocks_per_row': G, 'owned_texels': int((pts['face'] >= 0).sum()),
             'ia_atlas_points': timed(lambda: hipops.atlas_points(v, f, size, s)), 'torch_atlas_points': timed(torch_points),
             'decoder_bake': timed(lambda: geometry.bake_colors(planes, gen.decoder, v, f, size, box_warp, atlas=atlas)), 'torch_decoder_bake': timed(torch_bake),
             'project': timed(lambda: geometry.project_texture(v, f, atlas, images, cams, raster['depth'], raster['mask'])),
             'ia_texture_project': timed(lambda: hipops.texture_project(pts['point'], pts['normal'], pts['face'], images, cams, raster['depth'],
                                                                         raster['mask'], 1e-6, 0.2, 2.0, depth_tol)),
             'torch_project': timed(torch_project),
             'textured_view': timed(lambda: geometry.sample_texture(tex, atlas, *(lambda q: (q['face'], q['bary']))(geometry.rasterize_mesh(v, f, cams[:1], res)))),
             'ia_texture_sample_8_views': timed(lambda: geometry.sample_texture(tex, atlas, raster['face'], raster['bary'])),
             'torch_sample_8_views': timed(torch_sample)}
        result['sizes'][str(size)] = r
        del pts, tex
        torch.cuda.empty_cache()
    line = json.dumps(result)
    print(line)
    with open(args.out, 'w') as fh:
        fh.write(line + '\n')


if __name__ == '__main__':
    main()
