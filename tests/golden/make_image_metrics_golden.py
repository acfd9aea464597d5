"""Records tests/golden/image_metrics.npz: results of the reference's encoder_inversion/criteria/ms_ssim.py on seed-generated inputs.

Runs only where the reference checkout is present (as make_golden.py): this script imports ``ssim`` / ``msssim`` from it at generation
time, feeds them the inputs of tests/test_image_metrics_cpu.py (``case_pair``) and stores results only.  Per case (6 frames: the
clean image against its six distortions), all float32:
  <case>_ssim, <case>_cs   [6,5]  ssim(..., size_average=False, full=True, val_range=2) at each of the five levels; the level images
                                  are produced as msssim produces them (F.avg_pool2d(img, (2, 2)) in float32)
  <case>_msssim            [6]    msssim(..., val_range=2), one frame per call
  <case>_msssim_auto       [6]    msssim(..., val_range=None): its range detection must give L = 2 on [-1, 1] inputs
(msssim is called on one-frame batches with size_average=True: with size_average=False its ``mcs ** weights`` broadcasts the batch
axis against the five weights, which is not a per-frame MS-SSIM for any batch size; for one frame the two averages are the same number.)
  e_ref_ssim, e_ref_ms_ssim       the largest distance of those float32 results from image_metrics.reference_table (float64) over
                                  all cases: the reference's own rounding error, the unit of the device tests' bounds.
Usage: python tests/golden/make_image_metrics_golden.py --ref <reference checkout>"""
import argparse
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.abspath(os.path.join(HERE, '..', '..'))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, 'tests'))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--ref', required=True, help='root of the reference checkout')
    ap.add_argument('--out', default=os.path.join(HERE, 'image_metrics.npz'))
    args = ap.parse_args()
    sys.path.insert(0, os.path.join(args.ref, 'encoder_inversion', 'criteria'))
    import ms_ssim as ref                                   # the reference's file, imported, never copied
    from invertavatar_amd import image_metrics as im
    from test_image_metrics_cpu import CASES, case_pair

    out, e_ssim, e_ms = {}, 0.0, 0.0
    with torch.no_grad():
        for name in sorted(CASES):
            a, b = case_pair(name)
            assert a.min() < -0.5 and a.max() <= 1.0          # (the reference's range detection reads img1 = a)
            ssims, css = [], []
            la, lb = a, b
            for _ in range(5):
                s, c = ref.ssim(la, lb, size_average=False, full=True, val_range=2)
                ssims.append(s)
                css.append(c)
                la, lb = torch.nn.functional.avg_pool2d(la, (2, 2)), torch.nn.functional.avg_pool2d(lb, (2, 2))
            ssims, css = torch.stack(ssims, 1), torch.stack(css, 1)
            ms = torch.stack([ref.msssim(a[k:k + 1], b[k:k + 1], val_range=2) for k in range(a.shape[0])])
            ms_auto = torch.stack([ref.msssim(a[k:k + 1], b[k:k + 1], val_range=None) for k in range(a.shape[0])])
            tab = im.reference_table(a, b, 2.0, 5)
            assert (tab[:, 10:15] > 0).all() and (css > 0).all(), f'{name}: a mean cs is not positive: MS-SSIM would be NaN'
            assert torch.isfinite(ms).all() and torch.isfinite(ms_auto).all()
            e_ssim = max(e_ssim, (tab[:, 5:10] - ssims.double()).abs().max().item(), (tab[:, 10:15] - css.double()).abs().max().item())
            e_ms = max(e_ms, (tab[:, 4] - ms.double()).abs().max().item(), (tab[:, 4] - ms_auto.double()).abs().max().item())
            print(f'{name}: smallest mean cs {css.min().item():.3f}, ms_ssim {[round(float(v), 4) for v in ms]}')
            for key, t in (('ssim', ssims), ('cs', css), ('msssim', ms), ('msssim_auto', ms_auto)):
                assert t.dtype == torch.float32
                out[f'{name}_{key}'] = t.numpy()
    out['e_ref_ssim'], out['e_ref_ms_ssim'] = np.float64(e_ssim), np.float64(e_ms)
    print(f'e_ref: ssim / cs {e_ssim:.3e}, ms_ssim {e_ms:.3e}')
    np.savez(args.out, **out)


if __name__ == '__main__':
    main()
