"""Times ia_rasterize_level alone on the four launches of a B = 1 frame of the BASELINE model (texture pyramid 32ch@32, 512@32, 512@64,
256@128) and prints, per launch, the median and the range of 5 x 20 event-timed calls and the achieved GB/s over the bytes the level
has to move: texture level + output ((C + 1) planes) + the static crop (the UV / alpha maps, 1 MB, are not counted).
    python tools/bench_raster.py            (IA_HIP_LIB=<library> times another build of the library)"""
import os
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
import torch

from invertavatar_amd import hipops, synthetic

LEVELS = [(32, 32), (512, 32), (512, 64), (256, 128)]       # (channels, resolution) in launch order


def level_bytes(c, r, bbox):
    return 4 * (c * r * r + (c + 1) * r * r + c * (bbox[1] - bbox[0]) * (bbox[3] - bbox[2]))


def main():
    uv_smooth = synthetic.uv_conditions([3]).cuda().contiguous()
    uv_sil = uv_smooth.clone()             # UV = 0 outside the face, as ia_uv_rasterize writes it: silhouette footprints see two texel clusters
    uv_sil[..., 0][uv_sil[..., 2] < 0.5] = 0.0
    uv_sil[..., 1][uv_sil[..., 2] < 0.5] = 0.0
    for name, uv in (('smooth', uv_smooth), ('silhouette', uv_sil)):
        total = 0.0
        for c, r in LEVELS:
            upper = uv[..., 2].clamp(0, 1).contiguous()
            tex = torch.randn(1, c, r, r, device='cuda')
            sta = torch.randn(1, c, r, r, device='cuda')
            bbox = [round(v * r / 256) for v in (57, 185, 64, 192)]
            tcl = hipops.channels_last_copy(tex)
            fn = lambda: hipops.rasterize_level(tex, uv, upper, sta, bbox, r, tex_cl=tcl)
            for _ in range(3):
                fn()
            torch.cuda.synchronize()
            us = []
            for _ in range(5):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(20):
                    fn()
                e1.record()
                torch.cuda.synchronize()
                us.append(e0.elapsed_time(e1) / 20 * 1e3)
            med = statistics.median(us)
            total += med
            mb = level_bytes(c, r, bbox) / 1e6
            print(f'{name:10s} C={c:4d} res={r:4d}: {med:8.1f} us  (min {min(us):.1f}, max {max(us):.1f})  {mb:6.2f} MB  {mb / med * 1e3:7.1f} GB/s', flush=True)
        print(f'{name:10s} sum of the four launches: {total:8.1f} us', flush=True)


if __name__ == '__main__':
    main()
