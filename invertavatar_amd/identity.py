"""Identity similarity (CSIM) per frame: the cosine of the ArcFace IR-SE50 embeddings of a rendered frame and its ground truth.

The definition is the reference's ``encoder_inversion/criteria/id_loss.py`` (``IDLoss``): crop ``[35:223, 32:220]`` of a 256^2 frame,
``AdaptiveAvgPool2d(112)``, ``Backbone(112, 50, mode='ir_se')`` (``encoder_inversion/models/model_irse.py``) in eval mode, whose output is
an l2-normalised 512-vector; a pair's score is the dot product of its two vectors.  Frames larger than 256^2 (ours are 512^2) are first
adaptively average-pooled to 256^2, what the reference's callers do with their ``face_pool``; smaller ones are refused.

Device tensors go to the HIP kernels and never fall back: ``hipops.face_crop_pool``, the input layer on the fp32 MFMA convolution with
the BatchNorm in its epilogue + ``hipops.prelu_channels``, units 1 - 22 through ``trunk_hip.unit_forward`` (fp16 hi / lo pairs on the
MFMA tiles), units 23 and 24 (7^2 maps) on ``hipops.conv3x3_small`` + ``hipops.se_gate``, ``hipops.id_head`` and
``hipops.id_similarity``.  Both frames of every pair run as one ``[2N,3,H,W]`` batch, so that every weight is read once.  CPU tensors and
NumPy arrays take ``reference_embed`` / ``reference_compare``, the same definition in float64 torch ops -- the yardstick of the device
tests.

Inputs: float32 ``[N,3,H,W]`` in [-1, 1] or uint8 ``[N,H,W,3]`` (mapped by ``v / 127.5 - 1``), H, W >= 256.  Weights come from a file
the caller supplies -- the published ``model_ir_se50.pth`` state dict; nothing here downloads anything.  ``IDScore.synthetic`` makes
seeded weights for tests and benchmarks (their scores mean nothing).  Not done: face detection / alignment in front of the crop,
gradients, IR-100 / IR-152, ``num_scales > 1``."""
import math
import zlib

import numpy as np
import torch

FRAME, CROP_Y, CROP_X, CROP, SIDE = 256, 35, 32, 188, 112
DIM = 512
BN_EPS = 1e-5
KEYS = ('id_sim',)
STAGE_ENDS = (2, 6, 20, 23)             # index of the last unit of each stage of the 24-unit body
STAGE_NAMES = ('input_layer', 'stage1', 'stage2', 'stage3', 'stage4', 'head', 'embedding')
FIRST_SMALL_UNIT = 22                   # units from here on work on 7^2 maps: hipops.conv3x3_small


def _units():
    """(in_channel, depth, stride) of the 24 units."""
    units = []
    for (i, d), n in zip(((64, 64), (64, 128), (128, 256), (256, 512)), (3, 4, 14, 3)):
        units += [(i, d, 2)] + [(d, d, 1)] * (n - 1)
    return units


def _bn_spec(prefix, c):
    return [(f'{prefix}.weight', (c,)), (f'{prefix}.bias', (c,)), (f'{prefix}.running_mean', (c,)), (f'{prefix}.running_var', (c,)),
            (f'{prefix}.num_batches_tracked', ())]


def state_spec():
    """[(key, shape)] of the state dict of the reference's ``Backbone(input_size=112, num_layers=50, mode='ir_se')``."""
    spec = [('input_layer.0.weight', (64, 3, 3, 3))] + _bn_spec('input_layer.1', 64) + [('input_layer.2.weight', (64,))]
    for n, (i, d, _) in enumerate(_units()):
        p = f'body.{n}'
        if i != d:
            spec += [(f'{p}.shortcut_layer.0.weight', (d, i, 1, 1))] + _bn_spec(f'{p}.shortcut_layer.1', d)
        spec += _bn_spec(f'{p}.res_layer.0', i)
        spec += [(f'{p}.res_layer.1.weight', (d, i, 3, 3)), (f'{p}.res_layer.2.weight', (d,)), (f'{p}.res_layer.3.weight', (d, d, 3, 3))]
        spec += _bn_spec(f'{p}.res_layer.4', d)
        spec += [(f'{p}.res_layer.5.fc1.weight', (d // 16, d, 1, 1)), (f'{p}.res_layer.5.fc2.weight', (d, d // 16, 1, 1))]
    spec += _bn_spec('output_layer.0', DIM) + [('output_layer.3.weight', (DIM, DIM * 49)), ('output_layer.3.bias', (DIM,))]
    spec += _bn_spec('output_layer.4', DIM)
    return spec


def _load(obj):
    if isinstance(obj, dict):
        return obj
    try:
        sd = torch.load(obj, map_location='cpu', weights_only=True)
    except TypeError:                                      # (a torch without weights_only)
        sd = torch.load(obj, map_location='cpu')
    if not isinstance(sd, dict):
        raise ValueError(f'identity weights: {obj!r} does not hold a state dict')
    return sd


class IDScore:
    """Weights of the IR-SE50 embedding network.  ``weights``: the state dict of the reference's ``Backbone(112, 50, mode='ir_se')`` (the
    published ``model_ir_se50.pth``; the same keys under a ``facenet.`` prefix are accepted), a path for ``torch.load`` or a dict."""

    def __init__(self, weights=None):
        if weights is None:
            raise ValueError('IDScore needs the IR-SE50 weights from a file: pass weights= (or use IDScore.synthetic for a smoke run)')
        sd = _load(weights)
        self.sd = {}
        for key, shape in state_spec():
            tracked = key.endswith('num_batches_tracked')
            found = next((n for n in (key, 'facenet.' + key) if n in sd), None)
            if found is None:
                if tracked:
                    self.sd[key] = torch.zeros((), dtype=torch.int64)
                    continue
                raise ValueError(f'identity weights: key {key} is missing (also looked for facenet.{key})')
            t = torch.as_tensor(sd[found]).detach()
            if tuple(t.shape) != tuple(shape):
                raise ValueError(f'identity weights: {found} has shape {tuple(t.shape)}, expected {tuple(shape)}')
            self.sd[key] = t.to(device='cpu', dtype=torch.int64 if tracked else torch.float32).contiguous().clone()
        self._device = {}                                  # device -> the network there (+ packed weights, made on first use)

    @classmethod
    def synthetic(cls, seed=0):
        """Seeded weights that depend only on (seed, key): convolutions and the linear layer with variance 1 / fan-in, BatchNorm scales in
        [0.7, 1.1] with small shifts and running statistics near (0, 1), PReLU slopes around 0.25.  The activations then keep their order
        of magnitude from the image to the embedding (tests/test_identity_cpu.py asserts it)."""
        def rs(name):
            return np.random.RandomState((zlib.crc32(f'identity.{name}'.encode()) + 7919 * int(seed)) & 0x7FFFFFFF)
        sd = {}
        for key, shape in state_spec():
            r = rs(key)
            if key.endswith('num_batches_tracked'):
                sd[key] = torch.zeros((), dtype=torch.int64)
                continue
            if len(shape) >= 2:
                fan_in = int(np.prod(shape[1:]))
                v = r.randn(*shape) * math.sqrt(1.0 / fan_in)
            elif key.endswith('running_mean'):
                v = r.randn(*shape) * 0.05
            elif key.endswith('running_var'):
                v = r.uniform(0.8, 1.25, size=shape)
            elif key.endswith('.bias'):
                v = r.randn(*shape) * 0.05
            elif '.res_layer.2.' in key or key == 'input_layer.2.weight':
                v = r.uniform(0.1, 0.4, size=shape)                 # PReLU slopes
            else:
                v = r.uniform(0.7, 1.1, size=shape)                 # BatchNorm scales
            sd[key] = torch.from_numpy(np.asarray(v, dtype=np.float32))
        return cls(sd)

    def state_dict(self):
        """The weights under the reference's keys (what ``Backbone.load_state_dict`` and ``__init__`` read)."""
        return dict(self.sd)

    def on(self, device):
        """The network on `device` (cached): a float32 eval-mode ``model_irse.Backbone``, whose units carry their packed split weights and
        BatchNorm affine maps (trunk_hip), and the packs of the 7^2 units, the input layer and the head, made on first use."""
        device = torch.device(device)
        if device.type == 'cuda' and device.index is None:
            device = torch.device('cuda', torch.cuda.current_device())
        held = self._device.get(device)
        if held is None:
            from .encoder_inversion.models.model_irse import Backbone
            net = Backbone(SIDE, 50, mode='ir_se', drop_ratio=0.6)
            net.load_state_dict(self.sd)
            held = {'net': net.to(device).eval().requires_grad_(False), 'rows': {}}
            self._device[device] = held
        return held

    def __call__(self, x, y):
        """The reference's ``IDLoss.forward`` scalar for ``num_scales = 1``: the sum of (1 - similarity) over the frames divided by N."""
        sim = compare(x, y, self)['id_sim']
        return (1.0 - sim).sum() / sim.shape[0]


# ------------------------------------------------------------------ input checks

def _as_tensor(x):
    if isinstance(x, np.ndarray):
        x = torch.from_numpy(x)
    if not torch.is_tensor(x):
        raise ValueError('identity scores take torch tensors or NumPy arrays')
    return x


def _checked_images(x, model, data_range=None):
    """Validates one batch of frames; returns it with a NumPy array wrapped as a CPU tensor."""
    if not isinstance(model, IDScore):
        raise ValueError('model must be an identity.IDScore')
    x = _as_tensor(x)
    if x.dtype not in (torch.float32, torch.uint8):
        raise ValueError(f'images must be float32 [N,3,H,W] or uint8 [N,H,W,3], got {x.dtype}')
    if x.dim() != 4:
        raise ValueError(f'images must be a 4-D batch, got {tuple(x.shape)}')
    if x.dtype == torch.uint8:
        n, h, w, c = x.shape
        want = 255.0
    else:
        n, c, h, w = x.shape
        want = 2.0
    if n < 1:
        raise ValueError('empty batch')
    if c != 3:
        raise ValueError(f'identity scores take 3 channels, got {c} (float32 is [N,3,H,W], uint8 is [N,H,W,3])')
    if data_range is not None and float(data_range) != want:
        raise ValueError(f'identity scores are defined on images in [-1, 1] (data_range 2.0) or uint8 (data_range 255), got data_range '
                         f'{data_range} for {x.dtype}')
    if min(h, w) < FRAME:
        raise ValueError(f'a {h} x {w} image is too small: the crop is defined on a {FRAME} x {FRAME} frame, both sides must be >= {FRAME}')
    return x


def _checked(x, y, model, data_range):
    x, y = _as_tensor(x), _as_tensor(y)
    if x.dtype != y.dtype:
        raise ValueError(f'both images must be float32 [N,3,H,W] or both uint8 [N,H,W,3], got {x.dtype} and {y.dtype}')
    if x.device != y.device:
        raise ValueError(f'images are on different devices: {x.device} and {y.device}')
    if x.dim() != 4 or x.shape != y.shape:
        raise ValueError(f'images must be two 4-D batches of the same shape, got {tuple(x.shape)} and {tuple(y.shape)}')
    return _checked_images(x, model, data_range), _checked_images(y, model, data_range)


# ------------------------------------------------------------------ the definition, in torch ops of one dtype

def reference_front(images, dtype=torch.float64):
    """Frames -> [N,3,112,112] of `dtype`: (pool to 256^2) -> crop -> pool to 112^2."""
    F = torch.nn.functional
    v = images.permute(0, 3, 1, 2).to(dtype) / 127.5 - 1.0 if images.dtype == torch.uint8 else images.to(dtype)
    if tuple(v.shape[-2:]) != (FRAME, FRAME):
        v = F.adaptive_avg_pool2d(v, (FRAME, FRAME))
    return F.adaptive_avg_pool2d(v[:, :, CROP_Y:CROP_Y + CROP, CROP_X:CROP_X + CROP], (SIDE, SIDE))


@torch.no_grad()
def reference_stages(images, model, dtype=torch.float64):
    """The network in plain torch ops of `dtype` on the frames' device, written out from the state dict.  Returns the list STAGE_NAMES
    names: the activation after the input layer, after each of the four stages, the head's output in front of the l2 norm, the embedding."""
    F = torch.nn.functional
    dev = images.device
    sd = {k: (v.to(dev) if v.dtype == torch.int64 else v.to(device=dev, dtype=dtype)) for k, v in model.sd.items()}

    def bn(p, v):
        return F.batch_norm(v, sd[f'{p}.running_mean'], sd[f'{p}.running_var'], sd[f'{p}.weight'], sd[f'{p}.bias'], False, 0.0, BN_EPS)

    def prelu(v, a):
        return torch.where(v < 0, v * a.reshape(1, -1, 1, 1), v)

    x = reference_front(images, dtype)
    x = prelu(bn('input_layer.1', F.conv2d(x, sd['input_layer.0.weight'], padding=1)), sd['input_layer.2.weight'])
    out = [x]
    for n, (i, d, s) in enumerate(_units()):
        p = f'body.{n}'
        if i == d:
            short = x[:, :, ::s, ::s]
        else:
            short = bn(f'{p}.shortcut_layer.1', F.conv2d(x, sd[f'{p}.shortcut_layer.0.weight'], stride=s))
        r = F.conv2d(bn(f'{p}.res_layer.0', x), sd[f'{p}.res_layer.1.weight'], padding=1)
        r = prelu(r, sd[f'{p}.res_layer.2.weight'])
        r = bn(f'{p}.res_layer.4', F.conv2d(r, sd[f'{p}.res_layer.3.weight'], stride=s, padding=1))
        g = F.conv2d(torch.relu(F.conv2d(r.mean(dim=(2, 3), keepdim=True), sd[f'{p}.res_layer.5.fc1.weight'])), sd[f'{p}.res_layer.5.fc2.weight'])
        x = r * torch.sigmoid(g) + short
        if n in STAGE_ENDS:
            out.append(x)
    z = F.linear(bn('output_layer.0', x).flatten(1), sd['output_layer.3.weight'], sd['output_layer.3.bias'])
    z = bn('output_layer.4', z)
    out.append(z)
    out.append(torch.div(z, torch.norm(z, 2, 1, True)))
    return out


def reference_embed(images, model, dtype=torch.float64):
    """Embeddings through the restatement -> `dtype` [N,512] on the frames' device."""
    return reference_stages(_checked_images(images, model), model, dtype)[-1]


def reference_compare(x, y, model, data_range=None):
    """``compare`` through the float64 restatement, wherever the inputs live; the result as float32."""
    x, y = _checked(x, y, model, data_range)
    f = reference_embed(torch.cat([x, y], 0), model)
    n = x.shape[0]
    return {'id_sim': (f[:n] * f[n:]).sum(1).float()}


# ------------------------------------------------------------------ the device path

class _Packs:
    """Kernel-side parameters of the layers trunk_hip does not own: the input layer, the 7^2 units and the head."""

    def __init__(self, net):
        from . import hipops
        from .encoder_inversion.models import trunk_hip
        conv, bn, prelu = net.input_layer
        self.in_w = hipops.pack_conv_weight(conv.weight.detach().float())
        self.in_scale, self.in_shift = trunk_hip._affine(bn, bn.running_mean, bn.running_var)
        self.in_slopes = prelu.weight.detach().float().contiguous()
        self.small = []
        for unit in list(net.body)[FIRST_SMALL_UNIT:]:
            bn1, conv1, slopes, conv2, bn2, se = unit.res_layer
            c = conv2.out_channels
            self.small.append({
                'w1': hipops.pack_conv_weight(conv1.weight.detach().float()), 'w2': hipops.pack_conv_weight(conv2.weight.detach().float()),
                'bn1': trunk_hip._affine(bn1, bn1.running_mean, bn1.running_var), 'bn2': trunk_hip._affine(bn2, bn2.running_mean, bn2.running_var),
                'slopes': slopes.weight.detach().float().contiguous(),
                'fc1': se.fc1.weight.detach().float().reshape(-1, c).contiguous(), 'fc2': se.fc2.weight.detach().float().reshape(c, -1).contiguous()})
        # head: BatchNorm2d folded into the linear layer in float64 (no padding between them), BatchNorm1d as the kernel's affine map
        bn0, _, _, lin, bn4 = net.output_layer
        dev = lin.weight.device
        a0 = bn0.weight.detach().double().cpu() / torch.sqrt(bn0.running_var.detach().double().cpu() + bn0.eps)
        c0 = bn0.bias.detach().double().cpu() - bn0.running_mean.detach().double().cpu() * a0
        w = lin.weight.detach().double().cpu()
        per = w.shape[1] // a0.numel()
        self.head_w = (w * a0.repeat_interleave(per)).float().contiguous().to(dev)
        self.head_b = (lin.bias.detach().double().cpu() + w @ c0.repeat_interleave(per)).float().contiguous().to(dev)
        a4 = torch.rsqrt(bn4.running_var.detach().float() + bn4.eps)
        if bn4.affine:
            a4 = bn4.weight.detach().float() * a4
        self.head_scale = a4.contiguous()
        shift = -bn4.running_mean.detach().float() * a4
        self.head_shift = (shift + bn4.bias.detach().float() if bn4.affine else shift).contiguous()


def _packs(held):
    if 'packs' not in held:
        held['packs'] = _Packs(held['net'])
    return held['packs']


@torch.no_grad()
def device_stages(images, model):
    """The network through the HIP kernels -> the list STAGE_NAMES names, float32 on the frames' device."""
    from . import hipops
    from .encoder_inversion.models import trunk_hip
    held = model.on(images.device)
    net, p = held['net'], _packs(held)
    x = hipops.face_crop_pool(images.contiguous())
    b = x.shape[0]
    if b not in held['rows']:
        held['rows'][b] = p.in_scale.unsqueeze(0).expand(b, -1).contiguous()
    x = hipops.conv2d_mfma(x, p.in_w, demod=held['rows'][b], bias=p.in_shift, ksize=3)
    x = hipops.prelu_channels(x, p.in_slopes, inplace=True)
    out = [x]
    units = list(net.body)
    xs = None
    for i, unit in enumerate(units):
        if i < FIRST_SMALL_UNIT:
            if not trunk_hip.unit_supported(unit, x):
                raise RuntimeError(f'identity: unit {i} at {tuple(x.shape)} is not covered by the convolution kernels')
            if i + 1 < FIRST_SMALL_UNIT:
                x, xs = trunk_hip.unit_forward(unit, x, xs=xs, nxt=units[i + 1])
            else:
                x = trunk_hip.unit_forward(unit, x, xs=xs)
        else:
            k = p.small[i - FIRST_SMALL_UNIT]
            u = hipops.conv3x3_small(x, k['w1'], in_scale=k['bn1'][0], in_shift=k['bn1'][1], slopes=k['slopes'])
            v = hipops.conv3x3_small(u, k['w2'], out_scale=k['bn2'][0], out_shift=k['bn2'][1])
            x = hipops.se_gate(v, x, k['fc1'], k['fc2'])
        if i in STAGE_ENDS:
            out.append(x)
    emb = hipops.id_head(x, p.head_w, p.head_b, p.head_scale, p.head_shift)
    out.append(None)                                        # (the head's un-normalised output never leaves the kernel)
    out.append(emb)
    return out


@torch.no_grad()
def embed(images, model):
    """Unit-length embeddings of the frames -> float32 [N,512] on their device.  Device tensors: the HIP kernels, no fallback.  CPU
    tensors / NumPy arrays: the float64 restatement."""
    images = _checked_images(images, model)
    if not images.is_cuda:
        return reference_stages(images, model)[-1].float()
    return device_stages(images, model)[-1]


def similarity(fa, fb):
    """Per-pair dot products of two float32 [N,D] sets of embeddings -> float32 [N]."""
    if not (torch.is_tensor(fa) and torch.is_tensor(fb) and fa.dim() == 2 and fa.shape == fb.shape and fa.dtype == fb.dtype == torch.float32
            and fa.device == fb.device and fa.shape[0] >= 1):
        raise ValueError('similarity takes two float32 [N,D] tensors of one shape on one device')
    if not fa.is_cuda:
        return (fa.double() * fb.double()).sum(1).float()
    from . import hipops
    return hipops.id_similarity(torch.cat([fa, fb], 0).contiguous())


@torch.no_grad()
def compare(x, y, model, data_range=None):
    """Per-frame identity similarity of `x` against `y`: ``{'id_sim': float32 [N]}`` on the inputs' device.
    Device tensors: the HIP kernels, no fallback.  CPU tensors / NumPy arrays: the float64 restatement."""
    x, y = _checked(x, y, model, data_range)
    if not x.is_cuda:
        f = reference_stages(torch.cat([x, y], 0), model)[-1]
        n = x.shape[0]
        return {'id_sim': (f[:n] * f[n:]).sum(1).float()}
    from . import hipops
    f = device_stages(torch.cat([x, y], 0), model)[-1]
    return {'id_sim': hipops.id_similarity(f)}


class IDLoss:
    """The reference's ``IDLoss`` (encoder_inversion/criteria/id_loss.py) for inference: the same constructor and method names."""

    def __init__(self, path_ir_se50, num_scales=1):
        if num_scales != 1:
            raise ValueError(f'IDLoss: num_scales = {num_scales} is not supported (only the single-scale score, num_scales = 1)')
        self.num_scales = 1
        self.model = path_ir_se50 if isinstance(path_ir_se50, IDScore) else IDScore(path_ir_se50)

    def extract_feats(self, x):
        return embed(x, self.model)

    def forward(self, x, y):
        return self.model(x, y)

    __call__ = forward

    def CSIM_loss(self, x, y):
        """``cosine_embedding_loss(x_feats, y_feats, target = 1)``: the mean of 1 - cos, with torch's 1e-12 under each squared norm."""
        x, y = _checked(x, y, self.model, None)
        f = embed(torch.cat([x, y], 0), self.model)
        n = x.shape[0]
        fx, fy = f[:n].double(), f[n:].double()
        cos = (fx * fy).sum(1) / torch.sqrt(((fx * fx).sum(1) + 1e-12) * ((fy * fy).sum(1) + 1e-12))
        return (1.0 - cos).mean().float()
