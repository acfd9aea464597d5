"""LPIPS (Learned Perceptual Image Patch Similarity, v0.1) per frame, with the AlexNet and VGG16 backbones.

The definition is the reference's ``encoder_inversion/criteria/lpips`` (``lpips.py``, ``networks.py``, ``utils.py``): both images are
z-scored per channel, run through the backbone's feature stack, and at each of five taps (after a ReLU) the feature vectors are
unit-normalised per pixel (``f / (sqrt(sum_c f^2) + 1e-10)``), their squared differences weighted by the tap's linear layer and
averaged over the map; a frame's score is the sum of its five layer values.  ``LPIPS.__call__`` returns what the reference's
``forward`` does: the sum over the frames divided by N.

Device tensors go to the HIP kernels (``hipops.conv2d_direct``, ``hipops.maxpool2d``, the 3x3 MFMA convolutions on fp16 hi / lo
pairs where ``ia_conv2d_sx_supported`` takes the layer, ``hipops.lpips_layer``) and never fall back; CPU tensors and NumPy arrays take
``reference_compare``, the same definition in float64 torch ops -- the yardstick of the device tests.  Both images of a pair run as
one ``[2N,3,H,W]`` batch, so that every weight is read once.

Inputs: float32 ``[N,3,H,W]`` in [-1, 1] or uint8 ``[N,H,W,3]`` (mapped by ``v / 127.5 - 1``).  Weights come from files the caller
supplies -- a torchvision ``alexnet`` / ``vgg16`` state dict and the published LPIPS v0.1 linear layers; nothing here downloads
anything.  ``LPIPS.synthetic`` makes seeded weights for tests and benchmarks (their scores mean nothing)."""
import math
import zlib

import numpy as np
import torch

MEAN = (-0.030, -0.088, -0.188)
STD = (0.458, 0.448, 0.450)
EPS = 1e-10
KEYS = ('lpips', 'lpips_layers')


def _alex_plan():
    # (feature index, in, out, kernel, stride, padding, tapped) / ('pool', kernel, stride), in torchvision's alexnet.features order
    return [('conv', 0, 3, 64, 11, 4, 2, True), ('pool', 3, 2),
            ('conv', 3, 64, 192, 5, 1, 2, True), ('pool', 3, 2),
            ('conv', 6, 192, 384, 3, 1, 1, True),
            ('conv', 8, 384, 256, 3, 1, 1, True),
            ('conv', 10, 256, 256, 3, 1, 1, True)]


def _vgg_plan():
    plan, index, cin = [], 0, 3
    blocks = ((64, 64), (128, 128), (256, 256, 256), (512, 512, 512), (512, 512, 512))
    for b, widths in enumerate(blocks):
        for j, cout in enumerate(widths):
            plan.append(('conv', index, cin, cout, 3, 1, 1, j == len(widths) - 1))
            index, cin = index + 2, cout                   # conv, ReLU
        if b + 1 < len(blocks):
            plan.append(('pool', 2, 2))
            index += 1
    return plan


PLANS = {'alex': _alex_plan(), 'vgg': _vgg_plan()}
CHANNELS = {net: tuple(op[3] for op in plan if op[0] == 'conv' and op[7]) for net, plan in PLANS.items()}


def tap_sizes(net, h, w):
    """[(h, w)] of the five tapped maps of an h x w image; a side is 0 or less where the image is too small."""
    sizes = []
    for op in PLANS[net]:
        if op[0] == 'conv':
            _, _, _, _, k, s, p, tap = op
            h, w = (h + 2 * p - k) // s + 1, (w + 2 * p - k) // s + 1
            if tap:
                sizes.append((h, w))
        else:
            h, w = (h - op[1]) // op[2] + 1, (w - op[1]) // op[2] + 1
    return sizes


def min_side(net):
    """The smallest image side at which every tapped map has a pixel (31 for alex, 16 for vgg)."""
    s = 1
    while min(min(t) for t in tap_sizes(net, s, s)) < 1:
        s += 1
    return s


def _load(obj, what):
    if isinstance(obj, dict):
        return obj
    try:
        sd = torch.load(obj, map_location='cpu', weights_only=True)
    except TypeError:                                      # (a torch without weights_only)
        sd = torch.load(obj, map_location='cpu')
    if not isinstance(sd, dict):
        raise ValueError(f'{what}: {obj!r} does not hold a state dict')
    return sd


def _entry(sd, names, shape, what):
    for name in names:
        if name in sd:
            t = torch.as_tensor(sd[name]).detach()
            if tuple(t.shape) != tuple(shape):
                raise ValueError(f'{what}: {name} has shape {tuple(t.shape)}, expected {tuple(shape)}')
            return t.to(device='cpu', dtype=torch.float32).contiguous().clone()
    raise ValueError(f'{what}: key {names[0]} is missing (also looked for {", ".join(names[1:])})')


class LPIPS:
    """Backbone and linear weights of one LPIPS model.  ``weights``: a torchvision ``alexnet`` / ``vgg16`` state dict (``features.0.weight``
    ... or the bare ``0.weight`` ... of its feature stack), ``lin``: the published v0.1 linear layers (``lin0.model.1.weight`` ... or the
    reference's renamed ``0.1.weight`` ...); each a path for ``torch.load`` or a dict already loaded."""

    def __init__(self, net='alex', weights=None, lin=None):
        if net not in PLANS:
            raise ValueError(f"net must be 'alex' or 'vgg', got {net!r} (SqueezeNet is not supported)")
        if weights is None or lin is None:
            raise ValueError('LPIPS needs the backbone weights and the linear layers from files: pass weights= and lin= '
                             '(or use LPIPS.synthetic for a smoke run)')
        self.net, self.plan = net, PLANS[net]
        sd, ld = _load(weights, 'backbone weights'), _load(lin, 'linear layers')
        self.conv_w, self.conv_b, self.lin = [], [], []
        for op in self.plan:
            if op[0] != 'conv':
                continue
            _, idx, cin, cout, k = op[:5]
            self.conv_w.append(_entry(sd, (f'features.{idx}.weight', f'{idx}.weight'), (cout, cin, k, k), f'{net} backbone'))
            self.conv_b.append(_entry(sd, (f'features.{idx}.bias', f'{idx}.bias'), (cout,), f'{net} backbone'))
        for j, c in enumerate(CHANNELS[net]):
            self.lin.append(_entry(ld, (f'lin{j}.model.1.weight', f'{j}.1.weight'), (1, c, 1, 1), f'{net} linear layers').reshape(c))
        self._device = {}                                  # device -> weights there (+ packed fp16 pairs, made on first use)

    @classmethod
    def synthetic(cls, net='alex', seed=0):
        """Seeded weights that depend only on (net, seed, key): He-scaled convolutions, small biases, non-negative linear weights."""
        if net not in PLANS:
            raise ValueError(f"net must be 'alex' or 'vgg', got {net!r}")

        def rs(name):
            return np.random.RandomState((zlib.crc32(f'lpips.{net}.{name}'.encode()) + 7919 * int(seed)) & 0x7FFFFFFF)
        sd, ld = {}, {}
        for op in PLANS[net]:
            if op[0] != 'conv':
                continue
            _, idx, cin, cout, k = op[:5]
            w = rs(f'{idx}.weight').randn(cout, cin, k, k) * math.sqrt(2.0 / (cin * k * k))
            sd[f'features.{idx}.weight'] = torch.from_numpy(w.astype(np.float32))
            sd[f'features.{idx}.bias'] = torch.from_numpy((rs(f'{idx}.bias').randn(cout) * 0.05).astype(np.float32))
        for j, c in enumerate(CHANNELS[net]):
            ld[f'lin{j}.model.1.weight'] = torch.from_numpy(np.abs(rs(f'lin{j}').randn(1, c, 1, 1) * 0.5).astype(np.float32))
        return cls(net, sd, ld)

    def state_dicts(self):
        """(backbone, linear layers) in the key spelling of the files ``__init__`` reads."""
        sd, ld, i = {}, {}, 0
        for op in self.plan:
            if op[0] == 'conv':
                sd[f'features.{op[1]}.weight'], sd[f'features.{op[1]}.bias'] = self.conv_w[i], self.conv_b[i]
                i += 1
        for j, v in enumerate(self.lin):
            ld[f'lin{j}.model.1.weight'] = v.reshape(1, -1, 1, 1)
        return sd, ld

    def on(self, device):
        """The weights on `device` (cached)."""
        device = torch.device(device)
        if device.type == 'cuda' and device.index is None:
            device = torch.device('cuda', torch.cuda.current_device())
        held = self._device.get(device)
        if held is None:
            held = {'w': [t.to(device) for t in self.conv_w], 'b': [t.to(device) for t in self.conv_b],
                    'lin': [t.to(device) for t in self.lin], 'split': {}}
            self._device[device] = held
        return held

    def __call__(self, x, y):
        """The reference's scalar: the sum of the frames' scores divided by N."""
        res = compare(x, y, self)['lpips']
        return res.sum() / res.shape[0]


def _checked(x, y, model, data_range):
    """Validates a pair; returns (x, y) with NumPy arrays wrapped as CPU tensors."""
    if not isinstance(model, LPIPS):
        raise ValueError('model must be an lpips.LPIPS')
    if isinstance(x, np.ndarray):
        x = torch.from_numpy(x)
    if isinstance(y, np.ndarray):
        y = torch.from_numpy(y)
    if not (torch.is_tensor(x) and torch.is_tensor(y)):
        raise ValueError('LPIPS takes torch tensors or NumPy arrays')
    if x.dtype != y.dtype or x.dtype not in (torch.float32, torch.uint8):
        raise ValueError(f'both images must be float32 [N,3,H,W] or both uint8 [N,H,W,3], got {x.dtype} and {y.dtype}')
    if x.device != y.device:
        raise ValueError(f'images are on different devices: {x.device} and {y.device}')
    if x.dim() != 4 or x.shape != y.shape:
        raise ValueError(f'images must be two 4-D batches of the same shape, got {tuple(x.shape)} and {tuple(y.shape)}')
    if x.dtype == torch.uint8:
        n, h, w, c = x.shape
        want = 255.0
    else:
        n, c, h, w = x.shape
        want = 2.0
    if n < 1:
        raise ValueError('empty batch')
    if c != 3:
        raise ValueError(f'LPIPS takes 3 channels, got {c} (float32 is [N,3,H,W], uint8 is [N,H,W,3])')
    if data_range is not None and float(data_range) != want:
        raise ValueError(f'LPIPS is defined on images in [-1, 1] (data_range 2.0) or uint8 (data_range 255), got data_range {data_range} '
                         f'for {x.dtype}')
    if min(min(t) for t in tap_sizes(model.net, h, w)) < 1:
        raise ValueError(f"a {h} x {w} image is too small for the '{model.net}' backbone: the smaller side must be >= {min_side(model.net)}")
    return x, y


def _batch(x, y, dtype):
    """The pair as one z-scored [2N,3,H,W] batch of `dtype`."""
    v = torch.cat([x, y], 0)
    if v.dtype == torch.uint8:
        v = v.permute(0, 3, 1, 2).to(dtype) / 127.5 - 1.0
    else:
        v = v.to(dtype)
    mean = torch.tensor(MEAN, dtype=dtype, device=v.device).reshape(1, 3, 1, 1)
    std = torch.tensor(STD, dtype=dtype, device=v.device).reshape(1, 3, 1, 1)
    return ((v - mean) / std).contiguous()


@torch.no_grad()
def reference_table(x, y, model):
    """The definition in float64 torch ops on the inputs' device -> float64 [N,5], the layer values."""
    F = torch.nn.functional
    held = model.on(x.device)
    v, n, layers, i = _batch(x, y, torch.float64), x.shape[0], [], 0
    for op in model.plan:
        if op[0] == 'pool':
            v = F.max_pool2d(v, op[1], op[2])
            continue
        v = F.relu(F.conv2d(v, held['w'][i].double(), held['b'][i].double(), stride=op[5], padding=op[6]))
        i += 1
        if op[7]:
            f = v / (torch.sqrt((v * v).sum(1, keepdim=True)) + EPS)
            d = (f[:n] - f[n:]) ** 2
            layers.append((d * held['lin'][len(layers)].double().reshape(1, -1, 1, 1)).sum(1).mean(dim=(1, 2)))
    return torch.stack(layers, 1)


def _unpack(layers):
    layers = layers.float()
    total = (((layers[:, 0] + layers[:, 1]) + layers[:, 2]) + layers[:, 3]) + layers[:, 4]
    return {'lpips': total, 'lpips_layers': layers}


def reference_compare(x, y, model, data_range=None):
    """``compare`` through the float64 restatement, wherever the inputs live; results as float32 (the sum of the layers in float64)."""
    x, y = _checked(x, y, model, data_range)
    layers = reference_table(x, y, model)
    return {'lpips': layers.sum(1).float(), 'lpips_layers': layers.float()}


def _route(op, h, w):
    """'mfma' for a 3x3 stride-1 layer the fp16-pair MFMA kernels take at h x w, else 'direct'."""
    from . import hipops
    _, _, cin, cout, k, s, p, _ = op
    return 'mfma' if (k == 3 and s == 1 and p == 1 and hipops.conv_sx_supported(cin, cout, h, w, 3, False)) else 'direct'


def plan_routes(plan, h, w):
    """The route of every convolution of `plan` at the size it runs at for an h x w input (None at the pools)."""
    routes = []
    for op in plan:
        if op[0] == 'conv':
            routes.append(_route(op, h, w))
            h, w = (h + 2 * op[6] - op[4]) // op[5] + 1, (w + 2 * op[6] - op[4]) // op[5] + 1
        else:
            routes.append(None)
            h, w = (h - op[1]) // op[2] + 1, (w - op[1]) // op[2] + 1
    return routes


def run_plan(v, plan, held, on_tap=None):
    """Runs the feature stack `plan` on the fp32 batch `v` through the HIP kernels; held: a model's ``on(device)`` dict ('w', 'b',
    'split').  ``on_tap(map, index)`` is called with every tapped map (fp32).  Returns the last layer's fp32 output."""
    from . import hipops
    vs = None                                              # the activation as fp32 (v) and / or as a SplitAct (vs)
    routes = plan_routes(plan, v.shape[2], v.shape[3])
    i = taps = 0
    for j, op in enumerate(plan):
        nxt = plan[j + 1] if j + 1 < len(plan) else None
        nxt_conv = next((r for r in routes[j + 1:] if r is not None), None)     # route of the next convolution
        if op[0] == 'pool':
            out = hipops.maxpool2d(v, op[1], op[2], want_f32=nxt_conv != 'mfma', want_split=nxt_conv == 'mfma')
            v, vs = (None, out) if nxt_conv == 'mfma' else (out, None)
            continue
        tap = op[7]
        need_f32 = tap or nxt is None or nxt[0] == 'pool' or nxt_conv == 'direct'
        need_split = nxt is not None and nxt[0] == 'conv' and nxt_conv == 'mfma'
        if routes[j] == 'mfma':
            if vs is None:
                vs = hipops.act_split(v)
            wk = held['split'].get(i)
            if wk is None:
                wk = held['split'][i] = hipops.pack_conv_weight_split(held['w'][i])
            out = hipops.conv2d_mfma_sx(vs, wk, bias=held['b'][i], act='lrelu', alpha=0.0, gain=1.0, want_f32=need_f32, want_split=need_split)
            v, vs = out if (need_f32 and need_split) else ((out, None) if need_f32 else (None, out))
        else:
            v = hipops.conv2d_direct(v, held['w'][i], held['b'][i], stride=op[5], padding=op[6], relu=True)
            vs = hipops.act_split(v) if need_split else None
        i += 1
        if tap and on_tap is not None:
            on_tap(v, taps)
            taps += 1
    return v


@torch.no_grad()
def device_table(x, y, model):
    """The layer values through the HIP kernels -> float32 [N,5] on the inputs' device."""
    from . import hipops
    held = model.on(x.device)
    table = torch.empty(x.shape[0], 5, device=x.device, dtype=torch.float32)
    run_plan(_batch(x, y, torch.float32), model.plan, held, lambda f, t: hipops.lpips_layer(f, held['lin'][t], out=table[:, t]))
    return table


@torch.no_grad()
def compare(x, y, model, data_range=None):
    """Per-frame LPIPS of `x` against `y`: ``{'lpips': float32 [N], 'lpips_layers': float32 [N,5]}`` on the inputs' device.
    Device tensors: the HIP kernels, no fallback.  CPU tensors / NumPy arrays: the float64 restatement."""
    x, y = _checked(x, y, model, data_range)
    if not x.is_cuda:
        layers = reference_table(x, y, model)
        return {'lpips': layers.sum(1).float(), 'lpips_layers': layers.float()}
    return _unpack(device_table(x.contiguous(), y.contiguous(), model))
