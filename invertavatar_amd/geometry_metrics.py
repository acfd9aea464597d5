"""Geometry metrics of two meshes: ``python -m invertavatar_amd.geometry_metrics --pred A.ply --gt B.ply --out m.json``.

Reads two PLY meshes (``geometry.read_ply``), computes ``geometry.surface_distance(pred, gt)`` (Chamfer and Hausdorff distance, F-score
at the thresholds, normal consistency with ``--samples``; definitions in that function's docstring; precision is about the predicted
mesh, recall about the ground truth) and writes the numbers as JSON.  ``--error-ply E.ply`` also writes the predicted mesh coloured by
the distance of its vertices to the ground truth (black = 0, red = the largest threshold or more).  ``--align rigid`` (or
``similarity``) first moves the predicted mesh onto the ground truth with ``geometry.align_mesh`` (``--align-metric``, ``--align-iterations``,
``--align-trim``, ``--align-init centroid`` set its arguments; the source points are the ``--samples`` area-weighted samples of the
prediction when given, else its vertices), scores the moved mesh, adds an ``alignment`` block to the JSON and, with ``--save-aligned
OUT.ply``, writes the moved mesh.  ICP finds the nearest local optimum: a prediction far from the ground truth needs ``--align-init
centroid``, a pose from landmarks (``geometry.fit_transform``) or, for a prediction in another coordinate frame altogether,
``--align-init global`` (``geometry.global_align``: ``--align-angle-step``, ``--align-candidates``, ``--align-shifts``; the ``alignment``
block then also carries ``searched``, ``rank`` and ``candidate_scores``).  ``--signed`` adds the signed numbers of
``surface_distance(signed=True)`` (mean signed distance and inside share per direction: is the prediction inflated or deflated?) and
colours ``--error-ply`` with a diverging map (blue inside the ground truth, red outside, white on it).  ``--iou RES`` adds a
``volume_iou`` block: the volumetric IoU of the two meshes on a lattice of ``RES`` points along the longest axis.  ``--winding tree``
(with ``--winding-beta B``, default 2) makes the winding numbers behind both with ``geometry.WindingTree`` instead of the exact all-pairs
sum: the route for meshes of hundreds of thousands of faces.  ``--search tree`` takes every closest-point query (the distances, the
alignment, the IoU lattice, the colours) through ``geometry.closest_point(search='tree')``: the same numbers bit for bit, for meshes that
lie far apart, where the uniform grid walks every cell; the JSON then records ``search: tree``.  ``--fit-nonrigid`` then (after the
optional rigid alignment) wraps the prediction onto the ground truth with ``geometry.nonrigid_align`` (``--fit-metric``,
``--fit-stiffness 50,10,2,0.5``, ``--fit-iterations``, ``--fit-normal-cos``), scores the FITTED mesh, adds a ``nonrigid`` block (rms before
and after, the levels, inliers, the largest displacement) and, with ``--save-fitted OUT.ply``, writes the fitted mesh: the prediction's own
faces on the ground truth's shape.  ``--target-depth depth.npy --target-cameras cams.npy`` (instead of ``--gt``) takes the ground truth
from depth maps [N,H,W] with camera labels [N,25]: they are fused on a lattice of ``--target-resolution`` points along the longest axis
(``geometry.fuse_depth``) and meshed (``geometry.fused_mesh``), and the result is scored through the mesh route like any ``--gt``; the JSON
then carries a ``target`` block (views, lattice, truncation, triangles).  Without these flags the outputs are what they were.  Runs on
the device when there is one."""
import argparse
import json
import math

import numpy as np
import torch

from . import geometry


def error_colors(dist, scale):
    """uint8 [V,3]: black at distance 0 to red at ``scale`` or more; a non-finite distance is blue."""
    d = np.asarray(dist, dtype=np.float64)
    x = np.clip(np.where(np.isfinite(d), d, 0.0) / max(float(scale), 1e-30), 0.0, 1.0)
    col = np.zeros((d.size, 3), dtype=np.uint8)
    col[:, 0] = np.round(255 * x)
    col[~np.isfinite(d)] = (0, 0, 255)
    return col


def signed_error_colors(sdf, scale):
    """uint8 [V,3], diverging: white at signed distance 0, to red at ``+scale`` or more (outside the reference) and to blue at
    ``-scale`` or less (inside it); a non-finite distance is green."""
    d = np.asarray(sdf, dtype=np.float64)
    x = np.clip(np.where(np.isfinite(d), d, 0.0) / max(float(scale), 1e-30), -1.0, 1.0)
    fade = np.round(255 * (1.0 - np.abs(x)))
    col = np.empty((d.size, 3), dtype=np.uint8)
    col[:, 0] = np.where(x >= 0, 255, fade)
    col[:, 1] = fade
    col[:, 2] = np.where(x <= 0, 255, fade)
    col[~np.isfinite(d)] = (0, 255, 0)
    return col


ALIGN_MODES = ('rigid', 'similarity')


def align_prediction(verts, faces, ref_verts, ref_faces, align, samples=None, seed=0, options=None):
    """Move the mesh onto the reference with ``geometry.align_mesh`` (``align``: 'rigid' or 'similarity'; ``options``: its other
    arguments): ``(moved vertices, align_mesh's result)``.  The source points are ``samples`` area-weighted samples, else the vertices."""
    if align not in ALIGN_MODES:
        raise ValueError(f"align must be None, 'rigid' or 'similarity', got {align!r}")
    source = verts if samples is None else geometry.sample_surface(verts, faces, samples, seed)[0]
    fit = geometry.align_mesh(source, ref_verts, ref_faces, scale=align == 'similarity', **dict(options or {}))
    return geometry.transform_points(verts, fit['matrix']), fit


def alignment_block(fit):
    """The JSON form of an ``align_mesh`` result."""
    cos = min(1.0, max(-1.0, (float(np.trace(fit['rotation'])) - 1.0) / 2.0))
    block = {'matrix': [[float(x) for x in row] for row in fit['matrix']], 'scale': float(fit['scale']), 'angle_deg': math.degrees(math.acos(cos)),
             'shift': float(np.linalg.norm(fit['translation'])), 'rms_before': float(fit['rms_history'][0]), 'rms_after': float(fit['rms']),
             'iterations': int(fit['iterations']), 'converged': bool(fit['converged']), 'inliers': int(fit['inliers'])}
    if 'global' in fit:                                                    # init='global': what the pose search did
        g = fit['global']
        block.update(searched=int(g['searched']), rank=int(g['rank']), candidate_scores=[float(c['score']) for c in g['candidates']])
    return block


def fit_prediction(verts, faces, ref_verts, ref_faces, options=None):
    """Wrap the mesh onto the reference with ``geometry.nonrigid_align`` (``options``: its other arguments): ``(fitted vertices, its
    result)``."""
    fit = geometry.nonrigid_align((verts, faces), ref_verts, ref_faces, **dict(options or {}))
    return fit['verts'], fit


def nonrigid_block(fit):
    """The JSON form of a ``nonrigid_align`` result."""
    d = geometry._np(fit['displacement']).astype(np.float64)
    largest = float(np.sqrt((d * d).sum(1)).max()) if d.size else 0.0
    return {'rms_before': float(fit['rms_history'][0]), 'rms_after': float(fit['rms']), 'inliers': int(fit['inliers']),
            'pairings': len(fit['rms_history']), 'max_displacement': largest, 'pinned': int(geometry._np(fit['pinned']).sum()),
            'levels': [{'stiffness': float(l['stiffness']), 'pairings': int(l['pairings']), 'cg_steps': [int(k) for k in l['cg_steps']],
                        'cg_residual': [float(r) for r in l['cg_residual']]} for l in fit['levels']]}


def compare_meshes(verts, faces, ref_verts, ref_faces, samples=None, seed=0, thresholds=None, error_ply=None, align=None, align_options=None,
                   save_aligned=None, aligned=None, signed=False, iou=None, winding='exact', beta=2.0, search='grid', fit=None,
                   save_fitted=None, fitted=None):
    """``surface_distance(mesh, reference)`` plus the sizes of both meshes; ``error_ply``: also write the mesh coloured by distance.
    ``align``: 'rigid' or 'similarity' moves the mesh onto the reference first (``align_prediction`` with ``align_options``); the moved
    mesh is scored (and coloured), the result gains ``alignment`` (``alignment_block``), ``save_aligned`` is a PLY path for the moved mesh
    and ``aligned``, a dict, receives its ``verts`` and the ``matrix``.  ``signed``: the signed keys of ``surface_distance`` and a
    diverging ``error_ply`` (``signed_error_colors``); ``iou``: a lattice resolution, adds ``volume_iou`` of the (moved) mesh and the
    reference.  ``winding='tree'``: the winding numbers behind ``signed`` and ``iou`` come from ``geometry.WindingTree`` with ``beta``
    (the approximation for large meshes) and the result gains ``winding: {'method', 'beta'}``.  ``search='tree'``: every closest-point
    query goes through the cluster tree (``geometry.closest_point``; the same bits) and the result gains ``search: 'tree'``.  ``fit``: a
    dict of ``nonrigid_align`` arguments (may be empty) wraps the (moved) mesh onto the reference after that; the fitted mesh is scored,
    the result gains ``nonrigid`` (``nonrigid_block``), ``save_fitted`` is a PLY path for it and ``fitted``, a dict, receives its ``verts``."""
    tree = {'winding': winding, 'beta': beta} if winding != 'exact' else {}
    how = {'search': geometry._closest_search(search)} if search != 'grid' else {}
    fit_options = fit
    alignment = None
    if align is not None:
        verts, fit = align_prediction(verts, faces, ref_verts, ref_faces, align, samples, seed, {**dict(align_options or {}), **how})
        alignment = alignment_block(fit)
        if save_aligned:
            geometry.write_ply(save_aligned, verts, faces)
        if aligned is not None:
            aligned.update(verts=verts, matrix=fit['matrix'])
    nonrigid = None
    if fit_options is not None:
        verts, wrapped = fit_prediction(verts, faces, ref_verts, ref_faces, {**dict(fit_options), **how})
        nonrigid = nonrigid_block(wrapped)
        if save_fitted:
            geometry.write_ply(save_fitted, verts, faces)
        if fitted is not None:
            fitted.update(verts=verts)
    res = geometry.surface_distance(verts, faces, ref_verts, ref_faces, samples=samples, seed=seed, thresholds=thresholds,
                                    **({'signed': True, **tree} if signed else {}), **how)
    if tree:
        res['winding'] = {'method': winding, 'beta': float(beta)}
    if how:
        res['search'] = search
    res.update(pred_vertices=int(verts.shape[0]), pred_faces=int(faces.shape[0]), gt_vertices=int(ref_verts.shape[0]),
               gt_faces=int(ref_faces.shape[0]))
    if alignment is not None:
        res['alignment'] = alignment
    if nonrigid is not None:
        res['nonrigid'] = nonrigid
    if iou is not None:
        res['volume_iou'] = geometry.volume_iou(verts, faces, ref_verts, ref_faces, resolution=int(iou), **tree, **how)
    if error_ply:
        scale = res['thresholds'][-1] if res['thresholds'] else 1.0
        if signed:
            sdf = geometry.signed_distance(verts, ref_verts, ref_faces, **({'method': winding, 'beta': beta} if tree else {}), **how)['sdf']
            geometry.write_ply(error_ply, verts, faces, signed_error_colors(geometry._np(sdf), scale))
        else:
            dist = geometry.closest_point(verts, ref_verts, ref_faces, **how)['dist']
            geometry.write_ply(error_ply, verts, faces, error_colors(geometry._np(dist), scale))
    return res


def compare_clouds(verts, faces, ref_verts, ref_faces, samples=None, seed=0, thresholds=None, align=None, align_options=None,
                   normals_k=16, save_aligned=None, search='grid'):
    """``compare_meshes`` when the prediction, the reference or both are point clouds (no faces): ``geometry.surface_distance`` with
    ``faces=None`` on that side (the distance to a cloud is the distance to its nearest point), after ``geometry.align_mesh`` onto the
    reference if asked (against a cloud reference: its ``faces=None`` route, the plane metric with normals from ``normals_k``
    neighbours).  The result gains ``"target": "cloud"``."""
    pf = faces if faces.shape[0] else None
    rf = ref_faces if ref_faces.shape[0] else None
    res = {}
    if align is not None:
        if align not in ALIGN_MODES:
            raise ValueError(f"align must be None, 'rigid' or 'similarity', got {align!r}")
        source = verts if samples is None or pf is None else geometry.sample_surface(verts, pf, samples, seed)[0]
        more = {'normals_k': int(normals_k)} if rf is None else {'search': search}
        fit = geometry.align_mesh(source, ref_verts, rf, scale=align == 'similarity', **dict(align_options or {}), **more)
        verts = geometry.transform_points(verts, fit['matrix'])
        res['alignment'] = alignment_block(fit)
        if save_aligned:
            geometry.write_ply(save_aligned, verts, faces)
    res.update(geometry.surface_distance(verts, pf, ref_verts, rf, samples=samples, seed=seed, thresholds=thresholds, search=search))
    res.update(pred_vertices=int(verts.shape[0]), pred_faces=int(faces.shape[0]), gt_vertices=int(ref_verts.shape[0]),
               gt_faces=int(ref_faces.shape[0]), target='cloud')
    return res


def depth_target(depth_path, cameras_path, resolution=128, device='cpu'):
    """A ground truth given as depth maps (``depth_path``: .npy [N,H,W] or [N,1,H,W], the ray parameter per pixel, 0 / NaN where there
    is none; ``cameras_path``: .npy [N,25]): ``(verts, faces, block)`` of ``geometry.fused_mesh(geometry.fuse_depth(...))`` on ``device``."""
    depth = torch.from_numpy(np.ascontiguousarray(np.load(depth_path), dtype=np.float32)).to(device)
    cams = torch.from_numpy(np.ascontiguousarray(np.load(cameras_path), dtype=np.float32)).to(device)
    fusion = geometry.fuse_depth(depth, cams, int(resolution))
    verts, faces = geometry.fused_mesh(fusion)
    block = {'source': 'depth', 'views': fusion['info']['views'], 'resolution': [int(n) for n in fusion['tsdf'].shape], 'origin': list(fusion['origin']),
             'spacing': list(fusion['spacing']), 'truncation': fusion['truncation'], 'observed': fusion['info']['observed'],
             'vertices': int(verts.shape[0]), 'faces': int(faces.shape[0])}
    return verts, faces, block


def add_sign_arguments(ap):
    """``--signed``, ``--iou``, how their winding numbers are made (``--winding``, ``--winding-beta``) and how closest points are searched
    (``--search``), shared with extract_geometry."""
    ap.add_argument('--signed', action='store_true', help='add signed distances (negative inside the reference); diverging --error-ply')
    ap.add_argument('--iou', type=int, default=None, metavar='RES', help='add the volumetric IoU on a lattice of RES points along the longest axis')
    ap.add_argument('--winding', default='exact', choices=['exact', 'tree'],
                    help="winding numbers of --signed / --iou: the exact sum, or the cluster tree with a far field (large meshes)")
    ap.add_argument('--winding-beta', type=float, default=2.0, metavar='B',
                    help='with --winding tree: a node farther than B times its radius is taken as far (> 1; larger is more accurate)')
    ap.add_argument('--search', default='grid', choices=['grid', 'tree'],
                    help='closest-point queries: the uniform grid, or branch and bound on the cluster tree (the same numbers; meshes far apart)')


def sign_options_of(args):
    """The keyword arguments of ``compare_meshes`` for ``--signed`` / ``--iou`` / ``--winding tree`` / ``--search tree``; empty without them."""
    return {**({'signed': True} if args.signed else {}), **({'iou': args.iou} if args.iou is not None else {}),
            **({'winding': args.winding, 'beta': args.winding_beta} if args.winding != 'exact' else {}),
            **({'search': args.search} if args.search != 'grid' else {})}


def add_align_arguments(ap):
    """The ``--align`` family of flags, shared with extract_geometry."""
    ap.add_argument('--align', default=None, choices=ALIGN_MODES, help='move the predicted mesh onto the reference first (ICP)')
    ap.add_argument('--align-metric', default='plane', choices=['point', 'plane'])
    ap.add_argument('--align-iterations', type=int, default=30)
    ap.add_argument('--align-trim', type=float, default=1.0, help='share of the closest pairs that count (1: all)')
    ap.add_argument('--align-init', default='identity', choices=['identity', 'centroid', 'global'],
                    help='the start of ICP; global: a pose search over the reference\'s distance field (geometry.global_align)')
    ap.add_argument('--align-angle-step', type=float, default=15.0, metavar='DEG', help='with --align-init global: spacing of the candidate rotations')
    ap.add_argument('--align-candidates', type=int, default=8, help='with --align-init global: candidates refined by ICP')
    ap.add_argument('--align-shifts', type=int, default=1, help='with --align-init global: offsets per axis around the centroid (odd; expert option)')
    ap.add_argument('--normals-k', type=int, default=16, metavar='K',
                    help='with --align-metric plane against a reference without faces (a point cloud): neighbours per estimated normal')


def align_options_of(args):
    opts = {'metric': args.align_metric, 'iterations': args.align_iterations, 'trim': args.align_trim, 'init': args.align_init}
    if args.align_init == 'global':
        opts['global_options'] = {'angle_step': args.align_angle_step, 'candidates': args.align_candidates, 'shifts': args.align_shifts}
    return opts


def add_fit_arguments(ap, flag=True):
    """The ``--fit-*`` family of flags of the non-rigid fit, shared with extract_geometry (which has ``--fit-template`` for ``flag``)."""
    if flag:
        ap.add_argument('--fit-nonrigid', action='store_true', help='wrap the predicted mesh onto the reference (non-rigid ICP) and score the fitted mesh')
    ap.add_argument('--fit-metric', default='point', choices=['point', 'plane'])
    ap.add_argument('--fit-stiffness', default='50,10,2,0.5', metavar='A,B,...', help='the stiffness schedule, stiff to soft')
    ap.add_argument('--fit-iterations', type=int, default=5, help='pairings per stiffness level')
    ap.add_argument('--fit-normal-cos', type=float, default=None, metavar='C',
                    help='reject pairs whose template and target normals have a dot product below C')


def fit_options_of(args):
    try:
        schedule = tuple(float(x) for x in str(args.fit_stiffness).split(',') if x.strip())
    except ValueError:
        raise ValueError(f'--fit-stiffness must be numbers separated by commas, got {args.fit_stiffness!r}') from None
    return {'metric': args.fit_metric, 'stiffness': schedule, 'iterations': args.fit_iterations,
            **({'normal_cos': args.fit_normal_cos} if args.fit_normal_cos is not None else {})}


def nonrigid_summary(n, what='fitted'):
    return (f'{what}: rms {n["rms_before"]:.6g} -> {n["rms_after"]:.6g} in {n["pairings"]} pairings, {n["inliers"]} inliers, largest '
            f'displacement {n["max_displacement"]:.6g}')


def alignment_summary(a):
    return (f'aligned: scale {a["scale"]:.6g}, rotation {a["angle_deg"]:.4g} deg, |t| {a["shift"]:.6g}, rms {a["rms_before"]:.6g} -> '
            f'{a["rms_after"]:.6g} in {a["iterations"]} steps{"" if a["converged"] else " (not converged)"}')


def summary(res):
    f = ', '.join(f'F@{t:.4g} = {v:.4f}' for t, v in zip(res['thresholds'], res['fscore']))
    line = f'chamfer {res["chamfer"]:.6g}, hausdorff {res["hausdorff"]:.6g}, {f}'
    if 'mean_signed_ab' in res:
        line += (f', signed mean {res["mean_signed_ab"]:.6g} / {res["mean_signed_ba"]:.6g}, inside share {res["inside_share_ab"]:.4f} / '
                 f'{res["inside_share_ba"]:.4f}')
    if 'volume_iou' in res:
        line += f', volume IoU {res["volume_iou"]["iou"]:.4f} at {res["volume_iou"]["resolution"]}'
    return line


def main(argv=None):
    ap = argparse.ArgumentParser(description='Chamfer distance, Hausdorff distance and F-score of two PLY meshes')
    ap.add_argument('--pred', required=True)
    ap.add_argument('--gt', default=None, help='the ground-truth mesh or cloud (PLY); or give --target-depth and --target-cameras')
    ap.add_argument('--target-depth', default=None, metavar='depth.npy', help='ground truth as depth maps [N,H,W]: fused and meshed, then scored as a mesh')
    ap.add_argument('--target-cameras', default=None, metavar='cams.npy', help='with --target-depth: the camera labels [N,25]')
    ap.add_argument('--target-resolution', type=int, default=128, help='with --target-depth: lattice points along the longest axis')
    ap.add_argument('--samples', type=int, default=None, help='area-weighted samples per mesh; default: the vertices')
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--thresholds', type=float, nargs='+', default=None, help='F-score thresholds (at most 8); default 0.5, 1, 2 %% of the diagonal')
    ap.add_argument('--error-ply', default=None, help='write the predicted mesh coloured by its distance to the ground truth')
    ap.add_argument('--out', required=True, help='JSON file for the numbers')
    add_align_arguments(ap)
    add_sign_arguments(ap)
    ap.add_argument('--save-aligned', default=None, metavar='OUT.ply', help='with --align: write the moved predicted mesh')
    add_fit_arguments(ap)
    ap.add_argument('--save-fitted', default=None, metavar='OUT.ply', help='with --fit-nonrigid: write the fitted predicted mesh')
    ap.add_argument('--device', default='cuda' if torch.cuda.is_available() else 'cpu')
    args = ap.parse_args(argv)
    if (args.gt is None) == (args.target_depth is None) or (args.target_depth is None) != (args.target_cameras is None):
        ap.error('give --gt, or --target-depth together with --target-cameras')
    meshes, target = [], None
    for path in (args.pred, args.gt):
        if path is None:
            tv, tf, target = depth_target(args.target_depth, args.target_cameras, args.target_resolution, args.device)
            if not tf.shape[0]:
                ap.error(f'{args.target_depth}: the fused depth maps have no surface')
            args.gt = args.target_depth
            meshes += [tv, tf]
            continue
        v, f, _ = geometry.read_ply(path)
        meshes += [torch.from_numpy(v).to(args.device), torch.from_numpy(f).to(args.device)]
    if args.save_aligned and not args.align:
        ap.error('--save-aligned needs --align')
    if not meshes[1].shape[0] or not meshes[3].shape[0]:                   # a file without faces: the cloud routes
        for on, flag in ((args.signed, '--signed'), (args.iou is not None, '--iou'), (args.fit_nonrigid, '--fit-nonrigid'),
                         (args.align and args.align_init == 'global', '--align-init global'), (args.error_ply, '--error-ply')):
            if on:
                ap.error(f'{flag} needs a surface on both sides; {args.pred if not meshes[1].shape[0] else args.gt} is a point cloud (no faces)')
        res = compare_clouds(*meshes, samples=args.samples, seed=args.seed, thresholds=args.thresholds, align=args.align,
                             align_options=align_options_of(args) if args.align else None, normals_k=args.normals_k,
                             save_aligned=args.save_aligned, search=args.search)
        with open(args.out, 'w') as fh:
            json.dump(res, fh, indent=1)
        if args.align:
            print(alignment_summary(res['alignment']))
        print(summary(res))
        return res
    extra ={'align': args.align, 'align_options': align_options_of(args), 'save_aligned': args.save_aligned} if args.align else {}
    extra.update(sign_options_of(args))
    if args.save_fitted and not args.fit_nonrigid:
        ap.error('--save-fitted needs --fit-nonrigid')
    if args.fit_nonrigid:
        extra.update(fit=fit_options_of(args), save_fitted=args.save_fitted)
    res = compare_meshes(*meshes, samples=args.samples, seed=args.seed, thresholds=args.thresholds, error_ply=args.error_ply, **extra)
    if target is not None:
        res['target'] = target
        print(f'target: {target["views"]} depth maps fused on {target["resolution"]}, {target["faces"]} triangles')
    with open(args.out, 'w') as fh:
        json.dump(res, fh, indent=1)
    if args.align:
        print(alignment_summary(res['alignment']))
    if args.fit_nonrigid:
        print(nonrigid_summary(res['nonrigid']))
    print(summary(res))
    return res


if __name__ == '__main__':
    main()
