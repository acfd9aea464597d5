"""Geometry metrics of two meshes: ``python -m invertavatar_amd.geometry_metrics --pred A.ply --gt B.ply --out m.json``.

Reads two PLY meshes (``geometry.read_ply``), computes ``geometry.surface_distance(pred, gt)`` (Chamfer and Hausdorff distance, F-score
at the thresholds, normal consistency with ``--samples``; definitions in that function's docstring; precision is about the predicted
mesh, recall about the ground truth) and writes the numbers as JSON.  ``--error-ply E.ply`` also writes the predicted mesh coloured by
the distance of its vertices to the ground truth (black = 0, red = the largest threshold or more).  Runs on the device when there is one."""
import argparse
import json

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


def compare_meshes(verts, faces, ref_verts, ref_faces, samples=None, seed=0, thresholds=None, error_ply=None):
    """``surface_distance(mesh, reference)`` plus the sizes of both meshes; ``error_ply``: also write the mesh coloured by distance."""
    res = geometry.surface_distance(verts, faces, ref_verts, ref_faces, samples=samples, seed=seed, thresholds=thresholds)
    res.update(pred_vertices=int(verts.shape[0]), pred_faces=int(faces.shape[0]), gt_vertices=int(ref_verts.shape[0]),
               gt_faces=int(ref_faces.shape[0]))
    if error_ply:
        dist = geometry.closest_point(verts, ref_verts, ref_faces)['dist']
        scale = res['thresholds'][-1] if res['thresholds'] else 1.0
        geometry.write_ply(error_ply, verts, faces, error_colors(geometry._np(dist), scale))
    return res


def summary(res):
    f = ', '.join(f'F@{t:.4g} = {v:.4f}' for t, v in zip(res['thresholds'], res['fscore']))
    return f'chamfer {res["chamfer"]:.6g}, hausdorff {res["hausdorff"]:.6g}, {f}'


def main(argv=None):
    ap = argparse.ArgumentParser(description='Chamfer distance, Hausdorff distance and F-score of two PLY meshes')
    ap.add_argument('--pred', required=True)
    ap.add_argument('--gt', required=True)
    ap.add_argument('--samples', type=int, default=None, help='area-weighted samples per mesh; default: the vertices')
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--thresholds', type=float, nargs='+', default=None, help='F-score thresholds (at most 8); default 0.5, 1, 2 %% of the diagonal')
    ap.add_argument('--error-ply', default=None, help='write the predicted mesh coloured by its distance to the ground truth')
    ap.add_argument('--out', required=True, help='JSON file for the numbers')
    ap.add_argument('--device', default='cuda' if torch.cuda.is_available() else 'cpu')
    args = ap.parse_args(argv)
    meshes = []
    for path in (args.pred, args.gt):
        v, f, _ = geometry.read_ply(path)
        meshes += [torch.from_numpy(v).to(args.device), torch.from_numpy(f).to(args.device)]
    res = compare_meshes(*meshes, samples=args.samples, seed=args.seed, thresholds=args.thresholds, error_ply=args.error_ply)
    with open(args.out, 'w') as fh:
        json.dump(res, fh, indent=1)
    print(summary(res))
    return res


if __name__ == '__main__':
    main()
