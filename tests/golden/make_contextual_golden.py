"""Records tests/golden/contextual.npz: results of the reference's encoder_inversion/criteria/cx_loss.py (``CXLoss`` and the functions
of its ``contextual_loss``) on seed-generated inputs.

Runs only where the reference checkout is present (as make_golden.py): this script imports the reference's module at generation time;
the file is never copied.  The reference calls ``torchvision.models.vgg.vgg19(pretrained=True)``; no torchvision is needed and nothing
is downloaded: a stub ``torchvision.models.vgg`` is registered in ``sys.modules`` whose ``vgg19`` returns an object whose ``features``
is the 18-layer stack carrying ``CXScore.synthetic(MODEL_SEED)``'s weights.  Stored, all float32 (the reference runs in float32):
``dist`` / ``tilde`` / ``cxm`` [2,35,35] (``compute_cosine_distance``, ``compute_relative_distance``, ``compute_cx``) and ``head_loss``
(``contextual_loss``) on the maps ``relu_maps(FEATURE_SEED, 2, 20, 5, 7)``; ``forward_batch`` (``CXLoss.forward`` on the 2-frame 32 x 32
batch ``images(FRAME_SEED, 2, 32, 32)``), ``forward_each`` [2] (the same frames one at a time), ``forward_wide`` (the 1-frame 40 x 300
pair ``images(FRAME_SEED + 1, 1, 40, 300)``, which takes the resize) and the seeds.  No weights are stored.
Usage: python tests/golden/make_contextual_golden.py --ref <reference checkout>"""
import argparse
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.abspath(os.path.join(HERE, '..', '..'))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--ref', required=True, help='root of the reference checkout')
    ap.add_argument('--out', default=os.path.join(HERE, 'contextual.npz'))
    args = ap.parse_args()
    sys.path.insert(0, REPO)
    sys.path.insert(0, os.path.join(REPO, 'tests'))
    sys.path.insert(0, args.ref)
    from invertavatar_amd import contextual
    import contextual_reference as CR

    sd = contextual.CXScore.synthetic(CR.MODEL_SEED).state_dict()
    vgg = types.ModuleType('torchvision.models.vgg')
    vgg.vgg19 = lambda pretrained=False, **kw: types.SimpleNamespace(features=CR.vgg19_stack(sd, torch.float32))
    models = types.ModuleType('torchvision.models')
    models.vgg = vgg
    tv = types.ModuleType('torchvision')
    tv.models = models
    sys.modules.update({'torchvision': tv, 'torchvision.models': models, 'torchvision.models.vgg': vgg})
    from encoder_inversion.criteria import cx_loss as ref          # the reference's file, imported, never copied

    loss = ref.CXLoss().eval()
    assert len(loss.vgg_model.slice1) == 18
    fx, fy = CR.relu_maps(CR.FEATURE_SEED, 2, 20, 5, 7)
    x, y = CR.images(CR.FRAME_SEED, 2, 32, 32)
    xw, yw = CR.images(CR.FRAME_SEED + 1, 1, 40, 300)
    with torch.no_grad():
        dist = ref.compute_cosine_distance(fx, fy)
        tilde = ref.compute_relative_distance(dist)
        cxm = ref.compute_cx(tilde, 0.5)
        out = {'dist': dist.numpy(), 'tilde': tilde.numpy(), 'cxm': cxm.numpy(), 'head_loss': np.float32(ref.contextual_loss(fx, fy, 0.5)),
               'forward_batch': np.float32(loss(x, y)),
               'forward_each': np.array([float(loss(x[i:i + 1], y[i:i + 1])) for i in range(2)], dtype=np.float32),
               'forward_wide': np.float32(loss(xw, yw))}
    assert all(v.dtype == np.float32 for v in out.values())
    print({k: (v.tolist() if v.size <= 2 else v.shape) for k, v in out.items()})
    out.update(model_seed=np.int64(CR.MODEL_SEED), frame_seed=np.int64(CR.FRAME_SEED), feature_seed=np.int64(CR.FEATURE_SEED))
    np.savez_compressed(args.out, **out)


if __name__ == '__main__':
    main()
