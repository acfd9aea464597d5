"""Avatar shape extraction: ``python -m invertavatar_amd.extract_geometry --seeds 0-1 --res 256 --outdir out``.

For every seed: w = mapping(RandomState(seed).randn) with truncation (as the reenactment script draws it), the tri-planes under one mesh
condition (the first frame of ``--drive_root`` in the reference's on-disk layout, or a synthetic frame), the density volume on a
``--res``^3 lattice over the rendering box, and the marching-cubes mesh of density > ``--level``, written as ``seed%04d.ply`` (binary
PLY with per-vertex colours, and with ``--normals`` vertex normals); ``--save-volume`` also writes the volume as ``seed%04d.npy``.
``--views N --render-res R`` also renders the surface from N cameras of a yaw orbit (``LookAtPoseSampler`` at the rendering kwargs'
camera radius and pivot) and writes the shaded views as 8-bit PNGs ``seed%04d_view%02d.png`` (``--save-depth``: the depth maps as
``seed%04d_depth.npy``, [N,R,R]).  ``--keep largest`` (or ``--keep N``) removes the detached components of {density > level} from the
volume first, so the PLY, the views and the saved depth show the N largest only; ``--min-voxels M`` also drops kept components of fewer
than M lattice points; a line per seed reports how many components there were and the sizes of the kept ones.  ``--compare REF.ply``
prints Chamfer distance, Hausdorff distance and F-score of the extracted mesh against ``REF.ply`` and writes them as
``seed%04d_geometry.json`` (``geometry_metrics.compare_meshes``); ``--error-ply`` also writes ``seed%04d_error.ply``, the mesh coloured by
its distance to the reference; ``--align rigid|similarity`` (with ``--align-metric``, ``--align-iterations``, ``--align-trim``, ``--align-init``,
as in ``geometry_metrics``) first moves the extracted mesh onto ``REF.ply`` with ``geometry.align_mesh``, prints the scale, the rotation angle,
|t| and the rms before and after, and scores, colours and (``--mesh-views``) renders the error of the moved mesh; ``--signed`` and ``--iou RES`` (as in ``geometry_metrics``) add the signed distances (with a
diverging ``--error-ply``) and the volumetric IoU against ``REF.ply``; ``--search tree`` (as there) takes their closest-point queries through the cluster tree.  ``--simplify N`` simplifies the mesh to at most N triangles (``geometry.simplify_mesh``: quadric vertex
clustering; the line per seed then shows the triangle counts before and after), ``--simplify-cells C`` to a grid of C cells along the
longest axis; ``--simplify-check`` scores the simplified mesh against the full one (``geometry.surface_distance``), prints both directed
Hausdorff distances beside the cell diagonal and writes them into ``seed%04d_geometry.json``.  ``--smooth N`` smooths the mesh with N
Taubin pairs (``geometry.smooth_mesh``, after ``--keep`` and ``--simplify``; ``--smooth-lambda``, ``--smooth-mu`` (``none``: plain Laplacian
steps) and ``--smooth-weights`` set its arguments; normals then come from the mesh) and prints the boundary and non-manifold edge counts;
``--smooth-check`` prints the signed volume before and after and both directed Hausdorff distances between the smoothed and the
unsmoothed mesh, and writes them into ``seed%04d_geometry.json``.  ``--ao SAMPLES`` shoots SAMPLES cosine-weighted rays from every vertex of the FINAL mesh
(``geometry.ambient_occlusion``), writes ``seed%04d_ao.ply`` with grey vertex colours ``round(255 ao)``, prints the mean and adds an
``ambient_occlusion`` block to ``seed%04d_geometry.json``.  ``--mesh-views N`` renders the FINAL mesh (after ``--keep``,
``--simplify`` and ``--smooth``) from the same orbit through ``geometry.rasterize_mesh`` and writes the shaded views as
``seed%04d_meshview%02d.png``, the coloured ones as ``seed%04d_meshrgb%02d.png`` (unless ``--no-colors``) and, with ``--compare
--error-ply``, the error-coloured mesh as ``seed%04d_errorview%02d.png``; ``--save-depth`` adds ``seed%04d_meshdepth.npy``; a line per
seed reports the surface pixels and the culled triangles (``--views`` keeps rendering the volume).  ``--texture SIZE`` bakes the colours of
the FINAL mesh into a SIZE^2 texture atlas (``geometry.TextureAtlas``) and writes ``seed%04d.obj``, ``.mtl`` and ``.png`` beside the PLY:
``--texture-source decoder`` (default) queries the decoder at every texel, ``views`` projects ``--texture-views`` rendered images of the
orbit onto the mesh (``--texture-mode blend|best``) with the decoder bake as the fallback; with ``--mesh-views`` the mesh is also rendered
through the texture (``seed%04d_meshtex%02d.png``); a line per seed reports the block side, the share of filled texels and the views per
texel.  ``--fit-template T.ply`` wraps the template mesh ``T.ply`` onto the FINAL mesh of every seed (``geometry.nonrigid_align``;
``--fit-align rigid|similarity`` first moves it there with ``geometry.align_mesh`` from the centroids, or with ``--fit-init global`` from
a pose search (``geometry.global_align``: a template in another coordinate frame); ``--fit-metric``, ``--fit-stiffness``,
``--fit-iterations`` and ``--fit-normal-cos`` as in ``geometry_metrics``) and writes ``seed%04d_template.ply``: the template's own faces on
the avatar's shape, so every seed has the same topology, with colours queried at the fitted vertices unless ``--no-colors``; a line per
seed reports the template's vertices, the rms before and after, the inliers and the largest displacement, and ``seed%04d_geometry.json``
gains a ``template`` block.  ``--fuse-depth`` (with ``--views``) fuses the ray-cast depth maps of the orbit into one surface
(``geometry.fuse_depth`` on the lattice of the density volume, ``geometry.fused_mesh``), writes it as ``seed%04d_fused.ply`` and prints the
two-sided ``surface_distance`` between it and the marching-cubes mesh: whether the depth maps of the views describe the shape that was
meshed.  Runs on the device when there is one."""
import argparse
import json
import os

import numpy as np
import torch

from . import geometry, geometry_metrics, synthetic
from .reenact_avatar_next3d import FolderDrive, build_generator, parse_range, seed_latents
from .training_avatar_texture.camera_utils import FOV_to_intrinsics, LookAtPoseSampler


def mesh_condition(drive_root=None, device='cpu'):
    """{'uvcoords_image': [1,256,256,3]}: frame 0 of a drive directory, or synthetic frame 0."""
    uv = FolderDrive(drive_root)[0]['vert']['uvcoords_image'] if drive_root else synthetic.uv_conditions([0])
    return {'uvcoords_image': uv.to(device).float()}


def orbit_cameras(G, n_views, fov_deg=18.837, device='cpu'):
    """[n_views, 25] camera labels: a full yaw orbit (starting frontal) at the rendering kwargs' average radius about their pivot."""
    pivot = torch.tensor(G.rendering_kwargs.get('avg_camera_pivot', [0, 0, 0]), dtype=torch.float32, device=device)
    radius = G.rendering_kwargs.get('avg_camera_radius', 2.7)
    intr = FOV_to_intrinsics(fov_deg, device=device).reshape(1, 9)
    poses = [LookAtPoseSampler.sample(np.pi / 2 + 2 * np.pi * k / n_views, np.pi / 2, pivot, radius=radius, device=device)
             for k in range(n_views)]
    return torch.cat([torch.cat([p.reshape(1, 16), intr], 1) for p in poses], 0)


def parse_keep(s):
    """'largest' or a positive integer (the number of largest components to keep)."""
    if s == 'largest':
        return s
    try:
        n = int(s)
    except ValueError:
        n = 0
    if n < 1:
        raise argparse.ArgumentTypeError(f"--keep takes 'largest' or an integer >= 1, got {s!r}")
    return n


def parse_mu(s):
    """A float, or 'none' (plain Laplacian smoothing)."""
    if s.lower() == 'none':
        return None
    try:
        return float(s)
    except ValueError:
        raise argparse.ArgumentTypeError(f"--smooth-mu takes a number or 'none', got {s!r}")


def main(argv=None):
    ap = argparse.ArgumentParser(description='Density volumes and meshes of tri-plane avatars')
    ap.add_argument('--seeds', type=parse_range, required=True)
    ap.add_argument('--network', default=None, help='torch-saved state dict; default: synthetic weights')
    ap.add_argument('--width', default='full', choices=['full', 'small'])
    ap.add_argument('--drive_root', default=None, help='drive sequence directory (reference layout); default: a synthetic frame')
    ap.add_argument('--res', type=int, default=256, help='lattice points per axis')
    ap.add_argument('--level', type=float, default=10.0, help='density threshold of the surface')
    ap.add_argument('--trunc', type=float, default=1.0)
    ap.add_argument('--trunc-cutoff', type=int, default=14)
    ap.add_argument('--outdir', required=True)
    ap.add_argument('--save-volume', action='store_true')
    ap.add_argument('--no-colors', action='store_true')
    ap.add_argument('--normals', action='store_true', help='write vertex normals into the PLY')
    ap.add_argument('--views', type=int, default=0, help='also render N shaded views of the surface (yaw orbit) as PNGs')
    ap.add_argument('--mesh-views', type=int, default=0, help='also render N views of the final mesh (rasterised; same orbit) as PNGs')
    ap.add_argument('--render-res', type=int, default=512, help='pixels per side of the rendered views')
    ap.add_argument('--save-depth', action='store_true', help='with --views: also write the depth maps as .npy')
    ap.add_argument('--fuse-depth', action='store_true', help='with --views: fuse the depth maps into one surface; writes _fused.ply')
    ap.add_argument('--keep', type=parse_keep, default=None, help="'largest' or N: keep only the N largest connected components of the shape")
    ap.add_argument('--min-voxels', type=int, default=0, help='with --keep: also drop kept components of fewer lattice points')
    ap.add_argument('--compare', default=None, metavar='REF.ply', help='score the extracted mesh against this mesh (Chamfer, Hausdorff, F-score)')
    ap.add_argument('--error-ply', action='store_true', help='with --compare: also write the mesh coloured by its distance to REF.ply')
    geometry_metrics.add_align_arguments(ap)
    geometry_metrics.add_sign_arguments(ap)
    grp = ap.add_mutually_exclusive_group()
    grp.add_argument('--simplify', type=int, default=None, metavar='N', help='simplify the mesh to at most N triangles')
    grp.add_argument('--simplify-cells', type=int, default=None, metavar='C', help='simplify on a grid of C cells along the longest axis')
    ap.add_argument('--simplify-check', action='store_true', help='with --simplify / --simplify-cells: distance of the simplified mesh to the full one')
    ap.add_argument('--smooth', type=int, default=None, metavar='N', help='smooth the mesh with N Taubin pairs (after --keep and --simplify)')
    ap.add_argument('--smooth-lambda', type=float, default=0.5)
    ap.add_argument('--smooth-mu', type=parse_mu, default=-0.53, help="the negative factor of a pair, or 'none' for plain Laplacian steps")
    ap.add_argument('--smooth-weights', default='uniform', choices=['uniform', 'cotangent'])
    ap.add_argument('--smooth-check', action='store_true', help='with --smooth: signed volume before and after, distance to the unsmoothed mesh')
    ap.add_argument('--ao', type=int, default=None, metavar='SAMPLES', help='ambient occlusion of the final mesh with SAMPLES rays per vertex; writes _ao.ply')
    ap.add_argument('--texture', type=int, default=None, metavar='SIZE', help='bake the colours of the final mesh into a SIZE^2 texture atlas; writes .obj/.mtl/.png')
    ap.add_argument('--texture-source', default='decoder', choices=['decoder', 'views'], help='colours from the decoder, or projected from rendered views')
    ap.add_argument('--texture-views', type=int, default=8, help='with --texture-source views: the number of views of the yaw orbit')
    ap.add_argument('--texture-mode', default='blend', choices=['blend', 'best'], help='with --texture-source views: blend the views or take the best')
    ap.add_argument('--fit-template', default=None, metavar='T.ply', help='wrap this template mesh onto the final mesh; writes _template.ply')
    ap.add_argument('--fit-align', default=None, choices=geometry_metrics.ALIGN_MODES, help='with --fit-template: align the template first (from the centroids)')
    ap.add_argument('--fit-init', default='centroid', choices=['centroid', 'global'],
                    help='with --fit-align: start from the centroids, or from a pose search (a template in another coordinate frame)')
    geometry_metrics.add_fit_arguments(ap, flag=False)
    ap.add_argument('--device', default='cuda' if torch.cuda.is_available() else 'cpu')
    args = ap.parse_args(argv)
    G = build_generator(args.network, args.width, device=args.device)
    mesh = mesh_condition(args.drive_root, args.device)
    os.makedirs(args.outdir, exist_ok=True)
    ws, _ = seed_latents(G, args.seeds, args.trunc, args.trunc_cutoff)
    results = []
    simplify = args.simplify if args.simplify is not None else ({'cells': args.simplify_cells} if args.simplify_cells is not None else None)
    if args.simplify_check and simplify is None:
        ap.error('--simplify-check needs --simplify or --simplify-cells')
    if args.smooth_check and args.smooth is None:
        ap.error('--smooth-check needs --smooth')
    if args.align and not args.compare:
        ap.error('--align needs --compare')
    if args.fuse_depth and args.views < 1:
        ap.error('--fuse-depth needs --views')
    if (args.signed or args.iou is not None) and not args.compare:
        ap.error('--signed and --iou need --compare')
    smooth = None if args.smooth is None else {'iterations': args.smooth, 'lam': args.smooth_lambda, 'mu': args.smooth_mu,
                                               'weights': args.smooth_weights}
    texture = {}
    if args.texture is not None:
        texture = {'texture': {'size': args.texture, 'source': args.texture_source, 'n_views': args.texture_views, 'mode': args.texture_mode}}
    if args.fit_align and not args.fit_template:
        ap.error('--fit-align needs --fit-template')
    if args.fit_template:
        tv, tf, _ = geometry.read_ply(args.fit_template)
        texture['fit_template'] = {'verts': torch.from_numpy(tv).to(args.device), 'faces': torch.from_numpy(tf).to(args.device),
                                   **({'align': args.fit_align} if args.fit_align else {}),
                                   **({'align_init': args.fit_init} if args.fit_init != 'centroid' else {}), **geometry_metrics.fit_options_of(args),
                                   **({'search': args.search} if args.search != 'grid' else {})}
    for seed, w in zip(args.seeds, ws):
        out = G.extract_geometry(w.float(), mesh, resolution=args.res, level=args.level, with_colors=not args.no_colors,
                                 with_normals=args.normals, keep=args.keep, min_voxels=args.min_voxels, simplify=simplify, smooth=smooth, noise_mode='const',
                                 **texture)[0]
        path = os.path.join(args.outdir, f'seed{seed:04d}.ply')
        geometry.write_ply(path, out['verts'], out['faces'], out.get('colors'), out.get('normals'))
        if 'texture' in out:
            obj = os.path.join(args.outdir, f'seed{seed:04d}.obj')
            geometry.write_obj(obj, out['verts'], out['faces'], out['uv'], out['texture'], out.get('normals'))
            info, atlas = out['texture_info'], out['atlas']
            owned = max(int(info['mask'].sum()), 1)
            line = (f'seed {seed}: texture {atlas.size}^2, blocks of side {atlas.s} ({atlas.G} per row), {int(info["filled"].sum()) / owned:.1%} of '
                    f'{owned} owned texels filled')
            if 'views' in info:
                line += f' from views, {float(info["views"][info["mask"]].float().mean()):.2f} views per texel'
            print(f'{line} -> {obj}')
        if args.save_volume:
            np.save(os.path.join(args.outdir, f'seed{seed:04d}.npy'), out['volume'].cpu().numpy())
        print(f'seed {seed}: {out["verts"].shape[0]} vertices, {out["faces"].shape[0]} triangles -> {path}')
        if 'simplify' in out:
            info = out['simplify']
            print(f'seed {seed}: simplified {info["faces_before"]} -> {info["faces_after"]} triangles, {info["verts_before"]} -> '
                  f'{info["verts_after"]} vertices, grid {info["dims"]}, cell {info["cell_size"]:.6g}')
            meta = {'simplify': dict(info)}
            if args.simplify_check:
                full = G.extract_geometry(w.float(), mesh, resolution=args.res, level=args.level, keep=args.keep, min_voxels=args.min_voxels,
                                          noise_mode='const')[0]
                samples = 200000 if out['verts'].is_cuda else 2000                # (the host route is brute force)
                d = geometry.surface_distance(out['verts'], out['faces'], full['verts'], full['faces'], samples=samples)
                diag = float(np.sqrt(3.0) * info['cell_size'])
                meta['simplify']['check'] = {'simplified_to_full': d['max_ab'], 'full_to_simplified': d['max_ba'], 'chamfer': d['chamfer'],
                                             'cell_diagonal': diag}
                print(f'seed {seed}: Hausdorff simplified -> full {d["max_ab"]:.6g}, full -> simplified {d["max_ba"]:.6g}, cell diagonal '
                      f'{diag:.6g}, Chamfer {d["chamfer"]:.6g}')
            out['simplify'] = meta['simplify']
            with open(os.path.join(args.outdir, f'seed{seed:04d}_geometry.json'), 'w') as fh:
                json.dump(meta, fh, indent=1)
        if 'smooth' in out:
            info = out['smooth']
            print(f'seed {seed}: smoothed with {info["steps"]} steps, {info["edges"]} edges, {info["boundary_edges"]} boundary edges, '
                  f'{info["nonmanifold_edges"]} non-manifold edges')
            meta = {'smooth': dict(info)}
            if args.smooth_check:
                rough = G.extract_geometry(w.float(), mesh, resolution=args.res, level=args.level, keep=args.keep, min_voxels=args.min_voxels,
                                           simplify=simplify, noise_mode='const')[0]
                samples = 200000 if out['verts'].is_cuda else 2000                # (the host route is brute force)
                d = geometry.surface_distance(out['verts'], out['faces'], rough['verts'], rough['faces'], samples=samples)
                meta['smooth']['check'] = {'volume_before': geometry.signed_volume(rough['verts'], rough['faces']),
                                           'volume_after': geometry.signed_volume(out['verts'], out['faces']),
                                           'smoothed_to_input': d['max_ab'], 'input_to_smoothed': d['max_ba'], 'chamfer': d['chamfer']}
                chk = meta['smooth']['check']
                print(f'seed {seed}: signed volume {chk["volume_before"]:.6g} -> {chk["volume_after"]:.6g}, Hausdorff smoothed -> input '
                      f'{d["max_ab"]:.6g}, input -> smoothed {d["max_ba"]:.6g}')
            out['smooth'] = meta['smooth']
            gpath = os.path.join(args.outdir, f'seed{seed:04d}_geometry.json')
            if 'simplify' in out and os.path.exists(gpath):
                with open(gpath) as fh:
                    meta = dict(json.load(fh), **meta)
            with open(gpath, 'w') as fh:
                json.dump(meta, fh, indent=1)
        if 'components' in out:
            info = out['components']
            sizes = [int(info['stats'][c - 1, 0]) for c in info['kept']]
            print(f'seed {seed}: {info["count"]} connected components, kept {len(sizes)} of {sizes} lattice points')
        if args.compare:
            rv, rf, _ = geometry.read_ply(args.compare)
            rv, rf = torch.from_numpy(rv).to(out['verts'].device), torch.from_numpy(rf).to(out['verts'].device)
            err = os.path.join(args.outdir, f'seed{seed:04d}_error.ply') if args.error_ply else None
            extra = {}
            if args.align:
                out['aligned'] = {}
                extra = {'align': args.align, 'align_options': geometry_metrics.align_options_of(args), 'aligned': out['aligned']}
            extra.update(geometry_metrics.sign_options_of(args))
            out['metrics'] = geometry_metrics.compare_meshes(out['verts'], out['faces'], rv, rf, error_ply=err, **extra)
            with open(os.path.join(args.outdir, f'seed{seed:04d}_geometry.json'), 'w') as fh:
                json.dump(dict(out['metrics'], **{k: out[k] for k in ('simplify', 'smooth') if k in out}), fh, indent=1)
            if args.align:
                print(f'seed {seed}: {geometry_metrics.alignment_summary(out["metrics"]["alignment"])}')
            print(f'seed {seed}: against {args.compare}: {geometry_metrics.summary(out["metrics"])}')
        if args.ao is not None:
            ao = geometry.ambient_occlusion(out['verts'], out['faces'], samples=args.ao)
            grey = (ao['ao'] * 255.0).round().to(torch.uint8)[:, None].expand(-1, 3).cpu().numpy()
            apath = os.path.join(args.outdir, f'seed{seed:04d}_ao.ply')
            geometry.write_ply(apath, out['verts'].cpu().numpy(), out['faces'].cpu().numpy(), colors=grey)
            out['ambient_occlusion'] = {'samples': ao['samples'], 'seed': 0, 'mean': float(ao['ao'].double().mean()) if ao['ao'].numel() else 0.0,
                                        'min': float(ao['ao'].min()) if ao['ao'].numel() else 0.0, 'ply': os.path.basename(apath)}
            gpath = os.path.join(args.outdir, f'seed{seed:04d}_geometry.json')
            meta = {}
            if os.path.exists(gpath) and any(k in out for k in ('simplify', 'smooth', 'metrics')):
                with open(gpath) as fh:
                    meta = json.load(fh)
            with open(gpath, 'w') as fh:
                json.dump(dict(meta, ambient_occlusion=out['ambient_occlusion']), fh, indent=1)
            print(f'seed {seed}: ambient occlusion with {ao["samples"]} samples per vertex, mean {out["ambient_occlusion"]["mean"]:.4f} -> {apath}')
        if 'template' in out:
            tpl = out['template']
            tpath = os.path.join(args.outdir, f'seed{seed:04d}_template.ply')
            geometry.write_ply(tpath, tpl['verts'], tpl['faces'], tpl.get('colors'))
            block = geometry_metrics.nonrigid_block(tpl['fit'])
            if 'alignment' in tpl:
                block['alignment'] = geometry_metrics.alignment_block(tpl['alignment'])
            gpath = os.path.join(args.outdir, f'seed{seed:04d}_geometry.json')
            meta = {}
            if os.path.exists(gpath) and any(k in out for k in ('simplify', 'smooth', 'metrics', 'ambient_occlusion')):
                with open(gpath) as fh:
                    meta = json.load(fh)
            with open(gpath, 'w') as fh:
                json.dump(dict(meta, template=block), fh, indent=1)
            what = f'template of {tpl["verts"].shape[0]} vertices'
            print(f'seed {seed}: {geometry_metrics.nonrigid_summary(block, what)} -> {tpath}')
        if args.views > 0:
            from PIL import Image
            cams = orbit_cameras(G, args.views, device=args.device)[None]
            views = G.render_geometry(w.float(), cams, mesh, resolution=args.render_res, volume_resolution=args.res, level=args.level,
                                      keep=args.keep, min_voxels=args.min_voxels, noise_mode='const')
            shaded = (views['shaded'][0, :, 0].clamp(0, 1) * 255).round().to(torch.uint8).cpu().numpy()
            for k in range(args.views):
                Image.fromarray(shaded[k], mode='L').save(os.path.join(args.outdir, f'seed{seed:04d}_view{k:02d}.png'))
            if args.save_depth:
                np.save(os.path.join(args.outdir, f'seed{seed:04d}_depth.npy'), views['depth'][0, :, 0].cpu().numpy())
            out['views'] = views
            print(f'seed {seed}: {args.views} views at {args.render_res}^2, {int(views["mask"].sum())} surface pixels')
            if args.fuse_depth:
                _, lo, step = geometry.lattice_axis(args.res, G.rendering_kwargs['box_warp'], 0.0)
                fusion = geometry.fuse_depth(views['depth'][0], cams[0], args.res, origin=(float(lo),) * 3, spacing=(float(step),) * 3,
                                             mask=views['mask'][0])
                fv, ff = geometry.fused_mesh(fusion)
                fpath = os.path.join(args.outdir, f'seed{seed:04d}_fused.ply')
                geometry.write_ply(fpath, fv, ff)
                line = f'seed {seed}: fused {args.views} depth maps: {fusion["info"]["observed"]} lattice points seen, {ff.shape[0]} triangles -> {fpath}'
                if ff.shape[0] and out['faces'].shape[0]:
                    d = geometry.surface_distance(fv, ff, out['verts'], out['faces'], samples=200000 if fv.is_cuda else 2000)
                    out['fused'] = {'verts': fv, 'faces': ff, 'distance': d}
                    line += (f'; fused -> mesh mean {d["mean_ab"]:.6g} max {d["max_ab"]:.6g}, mesh -> fused mean {d["mean_ba"]:.6g} max '
                             f'{d["max_ba"]:.6g}, lattice step {float(step):.6g}')
                print(line)
        if args.mesh_views > 0:
            from PIL import Image
            cams = orbit_cameras(G, args.mesh_views, device=args.device)
            to8 = lambda x: (x.clamp(0, 1) * 255).round().to(torch.uint8).cpu().numpy()
            views = G.render_mesh(out['verts'], out['faces'], cams, resolution=args.render_res, normals=out.get('normals'), colors=out.get('colors'))
            shaded = to8(views['shaded'][:, 0])
            rgb = to8(views['rgb'].permute(0, 2, 3, 1)) if 'rgb' in views else None
            err_rgb = None
            if args.compare and args.error_ply:
                err_cols = torch.from_numpy(geometry.read_ply(os.path.join(args.outdir, f'seed{seed:04d}_error.ply'))[2]).to(out['verts'].device)
                err_verts = out['aligned']['verts'] if args.align else out['verts']
                err_rgb = to8(G.render_mesh(err_verts, out['faces'], cams, resolution=args.render_res, colors=err_cols)['rgb'].permute(0, 2, 3, 1))
            if 'texture' in out:
                tex_rgb = to8(G.render_mesh(out['verts'], out['faces'], cams, resolution=args.render_res, texture=out['texture'],
                                            atlas=out['atlas'])['rgb'].permute(0, 2, 3, 1))
                for k in range(args.mesh_views):
                    Image.fromarray(tex_rgb[k], mode='RGB').save(os.path.join(args.outdir, f'seed{seed:04d}_meshtex{k:02d}.png'))
            for k in range(args.mesh_views):
                Image.fromarray(shaded[k], mode='L').save(os.path.join(args.outdir, f'seed{seed:04d}_meshview{k:02d}.png'))
                if rgb is not None:
                    Image.fromarray(rgb[k], mode='RGB').save(os.path.join(args.outdir, f'seed{seed:04d}_meshrgb{k:02d}.png'))
                if err_rgb is not None:
                    Image.fromarray(err_rgb[k], mode='RGB').save(os.path.join(args.outdir, f'seed{seed:04d}_errorview{k:02d}.png'))
            if args.save_depth:
                np.save(os.path.join(args.outdir, f'seed{seed:04d}_meshdepth.npy'), views['depth'][:, 0].cpu().numpy())
            out['mesh_views'] = views
            print(f'seed {seed}: {args.mesh_views} mesh views at {args.render_res}^2, {int(views["mask"].sum())} surface pixels, '
                  f'{int(views["culled"].sum())} culled triangles')
        results.append((path, out))
    return results


if __name__ == '__main__':
    main()
