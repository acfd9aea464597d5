"""Times of the ray queries on the cluster tree (HIP events; one JSON line on stdout, ``--out FILE`` to keep it; a recorded run belongs
in profiles/ray_tree_bench.json).

Full-width generator, B = 1, synthetic weights, level 0 (the meshes of tools/bench_winding.py: 128^3 and 256^3).  Every step runs in a
child process of its own under a time limit, one after the other; the first step that fails, faults or runs out of time ends the run.
Every timed case where tree and brute both run is also compared: they must give the same bits, or the step fails.

- ``camera``: 512^2 pixel-centre rays of 4 orbit cameras (``extract_geometry.orbit_cameras``), first hit through the tree and, below
  1e11 ray-triangle pairs, the brute kernel; ``rasterize_mesh`` of the same views as a yardstick; mean boxes and pairs per ray.
- ``inside``: 100 000 rays from the middle of the box towards random surface samples, tree against brute, and the share of these
  inside-origin rays that find no triangle (the per-triangle test is not watertight).
- ``ao``: any-hit for the ambient-occlusion rays of all vertices at 64 samples (rays made once, then the query alone, chunked as
  ``ambient_occlusion`` does), and ``ambient_occlusion`` end to end (host clock, synchronised); mean boxes and pairs per ray.
Every time is the median of the timed runs after warm-up, with the smallest and largest beside it.
Usage: python tools/bench_ray_tree.py [--out FILE] [--steps camera,inside,ao]"""
import json
import os
import subprocess
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_closest_tree import host_clock, once          # noqa: E402
from bench_surface_distance import timed                 # noqa: E402
from bench_winding import mesh, setup                     # noqa: E402

STEPS = {'camera': 420, 'inside': 300, 'ao': 420}        # step -> seconds
BRUTE_PAIRS = 1e11
FIELDS = ('hit', 't', 'face', 'bary', 'point')


def same_bits(a, b):
    import torch
    return all(torch.equal(a[k].contiguous().view(torch.int32) if a[k].dtype == torch.float32 else a[k],
                           b[k].contiguous().view(torch.int32) if b[k].dtype == torch.float32 else b[k]) for k in FIELDS if k in a)


def camera_rays(cams, res):
    """Pixel-centre rays of camera labels [N,25] (cam2world, normalised intrinsics): (origins, dirs) float32 [N res^2, 3]."""
    import torch
    n, dev = cams.shape[0], cams.device
    c2w, k = cams[:, :16].reshape(n, 4, 4), cams[:, 16:].reshape(n, 3, 3)
    px = (torch.arange(res, device=dev, dtype=torch.float32) + 0.5) / res
    y, x = torch.meshgrid(px, px, indexing='ij')
    local = torch.stack([(x[None] - k[:, 0, 2, None, None]) / k[:, 0, 0, None, None], (y[None] - k[:, 1, 2, None, None]) / k[:, 1, 1, None, None],
                         torch.ones(n, res, res, device=dev)], -1)
    dirs = torch.einsum('nij,nhwj->nhwi', c2w[:, :3, :3], local)
    origins = c2w[:, None, None, :3, 3].expand_as(dirs)
    return origins.reshape(-1, 3).contiguous(), dirs.reshape(-1, 3).contiguous()


def query_cell(tree, o, d, faces, mode='first', t_max=float('inf')):
    counted = tree.rays(o, d, 0.0, t_max, mode=mode, return_counts=True)
    cnt = counted['counts'].double()
    cell = dict(rays=int(o.shape[0]), hits=int(counted['hit'].sum()), tree=timed(lambda: tree.rays(o, d, 0.0, t_max, mode=mode), warmup=1, reps=5),
                boxes_per_ray=float(cnt[:, 0].mean()), pairs_per_ray=float(cnt[:, 1].mean()), most_pairs=int(cnt[:, 1].max()))
    if o.shape[0] * faces <= BRUTE_PAIRS:
        by_brute, cell['brute'] = once(lambda: tree.rays(o, d, 0.0, t_max, mode=mode, brute=True))
        if not same_bits(counted, by_brute):
            raise SystemExit(f'{mode}: tree and brute differ')
    return cell


def step_camera():
    from invertavatar_amd import geometry
    from invertavatar_amd.extract_geometry import orbit_cameras
    g, _ = setup()
    r = {}
    for n in (128, 256):
        v, f = mesh(n)
        tree = geometry.WindingTree(v, f)
        tree.boxes
        cams = orbit_cameras(g, 4, device=v.device)
        o, d = camera_rays(cams, 512)
        row = dict(faces=int(f.shape[0]), views=4, resolution=512, first=query_cell(tree, o, d, int(f.shape[0])))
        row['rasterize_mesh'] = timed(lambda: geometry.rasterize_mesh(v, f, cams, 512), warmup=1, reps=5)
        r[f'mesh{n}'] = row
    return r


def step_inside():
    import torch
    from invertavatar_amd import geometry
    r = {}
    for n in (128, 256):
        v, f = mesh(n)
        tree = geometry.WindingTree(v, f)
        tree.boxes
        pts, _ = geometry.sample_surface(v, f, 100000, 0)
        mid = (v.amin(0) + v.amax(0)) / 2
        o = mid[None].expand(pts.shape[0], 3).contiguous()
        d = (torch.as_tensor(pts).to(v.device).float() - o).contiguous()
        inside = bool(geometry.inside(mid[None], v, f, method='tree', tree=tree)[0])
        cell = query_cell(tree, o, d, int(f.shape[0]))
        cell.update(origin_is_inside=inside, miss_share=1.0 - cell['hits'] / cell['rays'])
        r[f'mesh{n}'] = cell
    return r


def step_ao():
    import torch
    from invertavatar_amd import geometry, hipops
    r = {}
    for n in (128, 256):
        v, f = mesh(n)
        tree = geometry.WindingTree(v, f)
        tree.boxes
        nrm = geometry.mesh_normals(v, f)
        table = torch.from_numpy(geometry._ao_table(64, 0)).to(v.device)
        bias = 2.0 ** -12 * tree.extent
        step = max(1, geometry._AO_MAX_RAYS // 64)
        chunk = slice(0, min(step, v.shape[0]))
        o, d = hipops.ao_rays(v[chunk].contiguous(), nrm[chunk].contiguous(), table, bias)
        row = dict(faces=int(f.shape[0]), vertices=int(v.shape[0]), samples=64, first_chunk_vertices=int(chunk.stop),
                   any_hit_first_chunk=query_cell(tree, o, d, int(f.shape[0]), mode='any'),
                   rays_first_chunk=timed(lambda: hipops.ao_rays(v[chunk].contiguous(), nrm[chunk].contiguous(), table, bias), warmup=1, reps=5))
        out, row['ambient_occlusion_end_to_end_host_clock'] = host_clock(lambda: geometry.ambient_occlusion(v, f, samples=64, normals=nrm, tree=tree))
        row['mean_ao'] = float(out['ao'].double().mean())
        r[f'mesh{n}'] = row
    return r


def main():
    if '--step' in sys.argv:                                                      # child: one step, one JSON line
        name = sys.argv[sys.argv.index('--step') + 1]
        print('RESULT ' + json.dumps({'camera': step_camera, 'inside': step_inside, 'ao': step_ao}[name]()))
        return
    from invertavatar_amd import build as ia_build
    out_path = sys.argv[sys.argv.index('--out') + 1] if '--out' in sys.argv else None
    steps = sys.argv[sys.argv.index('--steps') + 1].split(',') if '--steps' in sys.argv else list(STEPS)
    res = {'source_digest': ia_build.source_digest(), 'level': 0.0}
    for name in steps:
        try:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), '--step', name], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                               timeout=STEPS[name], text=True)
        except subprocess.TimeoutExpired:
            res['stopped_at'] = dict(step=name, reason=f'no result within {STEPS[name]} s')
            break
        lines = [ln for ln in p.stdout.splitlines() if ln.startswith('RESULT ')]
        if p.returncode != 0 or not lines:
            res['stopped_at'] = dict(step=name, returncode=p.returncode, stderr=p.stderr[-600:])
            break
        res[name] = json.loads(lines[-1][len('RESULT '):])
    line = json.dumps(res)
    print(line)
    if out_path:
        with open(out_path, 'w') as fh:
            fh.write(line + '\n')
    sys.exit(1 if 'stopped_at' in res else 0)


if __name__ == '__main__':
    main()
