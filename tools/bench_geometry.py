"""Kernel times of the avatar-geometry path (HIP events; one JSON line on stdout).

- ia_density_grid at 256^3 and 512^3 on the full-width generator's planes (B = 1);
- the same 256^3 volume through chunked ``sample_mixed`` (2^20 points per call, the way the reference's lattice helper queries it), on the
  same box: the comparison;
- ia_mc_count + ia_mc_emit at 256^3 and 512^3 on the generator's density volumes (level = the volume's median: a surface through the
  whole box, far more triangles than an avatar shell);
- end-to-end ``extract_geometry`` at 256^3 (planes, volume, mesh, vertex colours; host clock around a synchronised call).

Rates are algorithmic: decoder FLOPs (sigma only: 32 x 64 + 64 multiply-adds per point) over kernel time against bench.py's fp32 peak;
gather bytes (12 texels x 128 B per point, served by L2 / MALL) and HBM-side bytes of marching cubes against bench.py's HBM peak.
Usage: python tools/bench_geometry.py [--out FILE]"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))

import torch  # noqa: E402

from invertavatar_amd import build as ia_build, geometry, hipops, synthetic  # noqa: E402
from invertavatar_amd.training_avatar_texture.triplane_v20 import TriPlaneGenerator  # noqa: E402

PEAK_FP32_TFLOPS = 157.3     # bench.py PEAK_FP32_MFMA_TFLOPS
PEAK_HBM_GBS = 8000.0        # bench.py PEAK_HBM_GBS


def timed(fn, warmup=2, reps=5):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def mc_kernel_ms(vol, level, origin, spacing, reps=3):
    """(count ms, emit ms, V, F): per-launch HIP events of the wrapper (hipops.PROFILE), medians over `reps` calls after one warm-up."""
    hipops.marching_cubes(vol, level, origin, spacing)
    counts, emits = [], []
    for _ in range(reps):
        hipops.PROFILE = []
        v, f = hipops.marching_cubes(vol, level, origin, spacing)
        torch.cuda.synchronize()
        prof, hipops.PROFILE = hipops.PROFILE, None
        for fam, _, _, e0, e1, _ in prof:
            (counts if fam == 'mc_count' else emits).append(e0.elapsed_time(e1))
    med = lambda x: sorted(x)[len(x) // 2]    # noqa: E731
    return med(counts), med(emits), v.shape[0], f.shape[0]


def main():
    out_path = sys.argv[sys.argv.index('--out') + 1] if '--out' in sys.argv else None
    assert torch.cuda.is_available(), 'bench_geometry needs the GPU'
    g = synthetic.fill_parameters(TriPlaneGenerator(**synthetic.generator_kwargs('full')).eval().requires_grad_(False)).cuda()
    bw = g.rendering_kwargs['box_warp']
    res = {'source_digest': ia_build.source_digest()}
    with torch.no_grad():
        ws = g.mapping(synthetic.latent(0, 1).cuda(), synthetic.conditioning_camera().cuda(), truncation_psi=0.7, truncation_cutoff=14)
        mesh = {'uvcoords_image': synthetic.uv_conditions([0]).cuda()}
        planes = geometry.generator_planes(g, ws, mesh, noise_mode='const')
        vols = {}
        for n in (256, 512):
            ms = timed(lambda: vols.__setitem__(n, geometry.density_volume(planes, g.decoder, n, bw, box_warp=bw)))
            pts = n ** 3
            flops, gather = pts * 2.0 * (32 * 64 + 64), pts * 12 * 128.0
            res[f'density_grid_{n}'] = dict(ms=round(ms, 3), tflops=round(flops / ms / 1e9, 2), frac_fp32_peak=round(flops / ms / 1e9 / PEAK_FP32_TFLOPS, 4),
                                            gather_gbs=round(gather / ms / 1e6, 1), out_hbm_gbs=round(4.0 * pts / ms / 1e6, 1))
        # the comparison: chunked sample_mixed on the same 256^3 lattice (each call runs the backbones too, as the reference's does)
        pts = geometry.lattice_points(256, bw).cuda()[None]
        dirs = torch.zeros(1, 1 << 20, 3, device='cuda')
        chunk = 1 << 20

        def chunked():
            out = torch.empty(pts.shape[1], device='cuda')
            for s in range(0, pts.shape[1], chunk):
                out[s:s + chunk] = g.sample_mixed(pts[:, s:s + chunk].clone(), dirs, ws, mesh, noise_mode='const')['sigma'].reshape(-1)
            return out
        ref = chunked()
        ms_ref = timed(chunked, warmup=0, reps=2)
        d = (ref.reshape(256, 256, 256) - vols[256][0]).abs().max().item()
        res['sample_mixed_chunked_256'] = dict(ms=round(ms_ref, 2), chunk_points=chunk, max_abs_diff_vs_density_grid=float(f'{d:.3e}'))
        res['density_grid_256_speedup_vs_sample_mixed'] = round(ms_ref / res['density_grid_256']['ms'], 1)
        # marching cubes on the generator volumes
        for n in (256, 512):
            vol = vols[n][0].contiguous()
            level = float(vol.float().median())
            step = bw / (n - 1)
            c_ms, e_ms, nv, nf = mc_kernel_ms(vol, level, (-bw / 2,) * 3, (step,) * 3)
            hbm = 4.0 * n ** 3 * (1 + 2 + 2) + 12.0 * nv + 12.0 * nf + 4.0 * 3 * nf
            res[f'marching_cubes_{n}'] = dict(level=round(level, 4), verts=nv, faces=nf, count_ms=round(c_ms, 3), emit_ms=round(e_ms, 3),
                                              total_ms=round(c_ms + e_ms, 3), hbm_gbs=round(hbm / (c_ms + e_ms) / 1e6, 1),
                                              frac_hbm_peak=round(hbm / (c_ms + e_ms) / 1e6 / PEAK_HBM_GBS, 4))
        # end to end at 256^3
        level = res['marching_cubes_256']['level']
        g.extract_geometry(ws, mesh, resolution=256, level=level, with_colors=True, noise_mode='const')
        torch.cuda.synchronize()
        t = []
        for _ in range(3):
            t0 = time.perf_counter()
            o = g.extract_geometry(ws, mesh, resolution=256, level=level, with_colors=True, noise_mode='const')[0]
            torch.cuda.synchronize()
            t.append((time.perf_counter() - t0) * 1e3)
        res['extract_geometry_256'] = dict(ms=round(sorted(t)[1], 2), verts=o['verts'].shape[0], faces=o['faces'].shape[0], with_colors=True)
    res['peaks'] = dict(fp32_tflops=PEAK_FP32_TFLOPS, hbm_gbs=PEAK_HBM_GBS)
    line = json.dumps(res)
    print(line)
    if out_path:
        with open(out_path, 'w') as fh:
            fh.write(line + '\n')


if __name__ == '__main__':
    main()
