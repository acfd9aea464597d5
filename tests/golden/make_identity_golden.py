"""Records tests/golden/identity.npz and tests/golden/identity_state_names.txt: results of the reference's
encoder_inversion/criteria/id_loss.py (``IDLoss``) on seed-generated inputs.

Runs only where the reference checkout is present (as make_golden.py): this script imports ``IDLoss`` from it at generation time, writes
the synthetic state dict (``IDScore.synthetic``, seed tests/identity_cases.py MODEL_SEED) to a temporary file, constructs the reference's
``IDLoss`` from that file and feeds it the three pairs of tests/identity_cases.py (``frames``).  Stored, all float32 (the reference runs
in float32): ``feats_x`` / ``feats_y`` [3,512] (``extract_feats``), ``forward`` and ``csim_loss`` (scalars), and the two seeds.  No
weights are stored.  The text file lists the keys and shapes of the reference's ``Backbone(112, 50, mode='ir_se')`` state dict.
Usage: python tests/golden/make_identity_golden.py --ref <reference checkout>"""
import argparse
import os
import sys
import tempfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.abspath(os.path.join(HERE, '..', '..'))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--ref', required=True, help='root of the reference checkout')
    ap.add_argument('--out', default=os.path.join(HERE, 'identity.npz'))
    ap.add_argument('--names', default=os.path.join(HERE, 'identity_state_names.txt'))
    args = ap.parse_args()
    sys.path.insert(0, REPO)
    sys.path.insert(0, os.path.join(REPO, 'tests'))
    sys.path.insert(0, args.ref)                            # the reference's own packages (encoder_inversion, torch_utils, dnnlib)
    from encoder_inversion.criteria.id_loss import IDLoss   # the reference's file, imported, never copied
    from invertavatar_amd import identity
    import identity_cases as IC

    model = identity.IDScore.synthetic(IC.MODEL_SEED)
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, 'model_ir_se50.pth')
        torch.save(model.state_dict(), path)
        ref = IDLoss(path).eval()
    with open(args.names, 'w') as fh:
        for k, v in ref.facenet.state_dict().items():
            fh.write(f'{k} {"x".join(str(int(s)) for s in v.shape) or "scalar"}\n')
    x, y = IC.frames()
    with torch.no_grad():
        fx, fy = ref.extract_feats(x), ref.extract_feats(y)
        fwd, csim = ref(x, y), ref.CSIM_loss(x, y)
    out = {'feats_x': fx.numpy(), 'feats_y': fy.numpy(), 'forward': np.float32(fwd), 'csim_loss': np.float32(csim),
           'frame_seed': np.int64(IC.SEED), 'model_seed': np.int64(IC.MODEL_SEED)}
    assert all(v.dtype == np.float32 for k, v in out.items() if not k.endswith('seed'))
    print('similarities', (fx * fy).sum(1).tolist(), 'forward', float(fwd), 'CSIM_loss', float(csim))
    np.savez(args.out, **out)


if __name__ == '__main__':
    main()
