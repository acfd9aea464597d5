"""Avatar shape extraction: ``python -m invertavatar_amd.extract_geometry --seeds 0-1 --res 256 --outdir out``.

For every seed: w = mapping(RandomState(seed).randn) with truncation (as the reenactment script draws it), the tri-planes under one mesh
condition (the first frame of ``--drive_root`` in the reference's on-disk layout, or a synthetic frame), the density volume on a
``--res``^3 lattice over the rendering box, and the marching-cubes mesh of density > ``--level``, written as ``seed%04d.ply`` (binary
PLY with per-vertex colours); ``--save-volume`` also writes the volume as ``seed%04d.npy``.  Runs on the device when there is one."""
import argparse
import os

import numpy as np
import torch

from . import geometry, synthetic
from .reenact_avatar_next3d import FolderDrive, build_generator, parse_range, seed_latents


def mesh_condition(drive_root=None, device='cpu'):
    """{'uvcoords_image': [1,256,256,3]}: frame 0 of a drive directory, or synthetic frame 0."""
    uv = FolderDrive(drive_root)[0]['vert']['uvcoords_image'] if drive_root else synthetic.uv_conditions([0])
    return {'uvcoords_image': uv.to(device).float()}


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
    ap.add_argument('--device', default='cuda' if torch.cuda.is_available() else 'cpu')
    args = ap.parse_args(argv)
    G = build_generator(args.network, args.width, device=args.device)
    mesh = mesh_condition(args.drive_root, args.device)
    os.makedirs(args.outdir, exist_ok=True)
    ws, _ = seed_latents(G, args.seeds, args.trunc, args.trunc_cutoff)
    results = []
    for seed, w in zip(args.seeds, ws):
        out = G.extract_geometry(w.float(), mesh, resolution=args.res, level=args.level, with_colors=not args.no_colors, noise_mode='const')[0]
        path = os.path.join(args.outdir, f'seed{seed:04d}.ply')
        geometry.write_ply(path, out['verts'], out['faces'], out.get('colors'))
        if args.save_volume:
            np.save(os.path.join(args.outdir, f'seed{seed:04d}.npy'), out['volume'].cpu().numpy())
        print(f'seed {seed}: {out["verts"].shape[0]} vertices, {out["faces"].shape[0]} triangles -> {path}')
        results.append((path, out))
    return results


if __name__ == '__main__':
    main()
