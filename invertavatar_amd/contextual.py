"""Contextual loss (CX) per frame on VGG19 relu3_4 features: every feature of one frame is matched to its nearest feature of the other
frame, wherever it lies, so the score stays meaningful when a reenacted frame is a few pixels off its ground truth.

The definition is the reference's ``encoder_inversion/criteria/cx_loss.py`` (``CXLoss``, ``contextual_loss`` with the cosine distance):

1. frames whose WIDTH is above 256 are resized to 256 x 256 (``F.interpolate``, bilinear, ``align_corners=False``, no antialiasing); the
   reference tests ``shape[-1]`` only, so a 512 x 200 frame is not resized -- kept as it is there;
2. no input normalisation (the reference has it commented out);
3. ``vgg19().features[:18]``: conv1_1, conv1_2, pool, conv2_1, conv2_2, pool, conv3_1 .. conv3_4, a ReLU behind every convolution ->
   ``[N,256,H/4,W/4]``;
4. with P = h w positions: ``mu`` = the channel means of fy; both maps centred by it and every position divided by ``max(norm, 1e-12)``;
   ``d_ij = 1 - x^_i . y^_j``; ``m_i = min_j d_ij``; ``w_ij = exp((1 - clamp(d_ij / (m_i + 1e-5), -10, 10)) / band_width)``;
   ``cx_ij = w_ij / sum_j w_ij``; ``cx = mean_j max_i cx_ij``; ``loss = -log(cx + 1e-5)``.

In the reference ``mu`` runs over the whole batch, so its scalar for N frames is not the mean of N one-frame calls.  ``compare`` is per
frame and does not depend on the batching (frame n uses the means of its own fy_n: the reference's value at N = 1); ``model(x, y)`` is
the reference's ``CXLoss.forward`` scalar with the batch-wide ``mu``.  Identical frames give ``cx_loss = -log(1 + 1e-5)``, about -1e-5.

Device tensors go to the HIP kernels and never fall back: ``hipops.resize_bilinear``, the trunk through ``lpips.run_plan`` (conv1_1 and
conv1_2 direct, conv2_1 .. conv3_4 on the fp16 hi / lo MFMA kernels where ``ia_conv2d_sx_supported`` takes them, the pools writing the
next layer's split operand, the last layer fp32) and ``hipops.cx_head``, which never stores the P x P matrix.  Both frames of a pair run
as one ``[2N,3,H,W]`` batch.  CPU tensors and NumPy arrays take the float64 torch restatement -- the definition, and the yardstick of the
device tests.

Inputs: float32 ``[N,3,H,W]`` in [-1, 1] or uint8 ``[N,H,W,3]`` (mapped by ``v / 127.5 - 1``), sides >= 4.  Weights come from a file the
caller supplies -- a torchvision ``vgg19`` state dict; nothing here downloads anything.  ``CXScore.synthetic`` makes seeded weights for
tests and benchmarks (their scores mean nothing).  Not done: ``contextual_bilateral_loss`` (CoBi), the l1 / l2 distances of the
``contextual_loss`` package, gradients, other VGG taps, frames whose height alone exceeds 256 (kept as the reference treats them)."""
import math
import zlib

import numpy as np
import torch

from . import lpips as _lpips

FRAME = 256
MIN_SIDE = 4
CHANNELS = 256
KEYS = ('cx', 'cx_loss')


def _plan():
    # torchvision's vgg19.features[:18], in the plan format of lpips.py; only the last layer is tapped
    plan, index, cin = [], 0, 3
    for b, widths in enumerate(((64, 64), (128, 128), (256, 256, 256, 256))):
        if b:
            plan.append(('pool', 2, 2))
            index += 1
        for cout in widths:
            plan.append(('conv', index, cin, cout, 3, 1, 1, False))
            index, cin = index + 2, cout
    plan[-1] = plan[-1][:7] + (True,)
    return plan


PLAN = _plan()


class CXScore:
    """Weights of the VGG19 trunk up to relu3_4.  ``weights``: a torchvision ``vgg19`` state dict (``features.0.weight`` ...
    ``features.16.bias``, or the bare ``0.weight`` ... of its feature stack; later layers are ignored), a path for ``torch.load`` or a
    dict already loaded."""

    def __init__(self, weights=None, band_width=0.5):
        if weights is None:
            raise ValueError('CXScore needs the vgg19 weights from a file: pass weights= (or use CXScore.synthetic for a smoke run)')
        if not float(band_width) > 0.0:
            raise ValueError(f'band_width must be positive, got {band_width}')
        self.band_width, self.plan = float(band_width), PLAN
        sd = _lpips._load(weights, 'vgg19 weights')
        self.conv_w, self.conv_b = [], []
        for op in self.plan:
            if op[0] != 'conv':
                continue
            _, idx, cin, cout, k = op[:5]
            self.conv_w.append(_lpips._entry(sd, (f'features.{idx}.weight', f'{idx}.weight'), (cout, cin, k, k), 'vgg19 weights'))
            self.conv_b.append(_lpips._entry(sd, (f'features.{idx}.bias', f'{idx}.bias'), (cout,), 'vgg19 weights'))
        self._device = {}                                  # device -> weights there (+ packed fp16 pairs, made on first use)

    @classmethod
    def synthetic(cls, seed=0, band_width=0.5):
        """Seeded weights that depend only on (seed, key): He-scaled convolutions and small biases, as ``LPIPS.synthetic`` makes them."""
        def rs(name):
            return np.random.RandomState((zlib.crc32(f'contextual.vgg19.{name}'.encode()) + 7919 * int(seed)) & 0x7FFFFFFF)
        sd = {}
        for op in PLAN:
            if op[0] != 'conv':
                continue
            _, idx, cin, cout, k = op[:5]
            w = rs(f'{idx}.weight').randn(cout, cin, k, k) * math.sqrt(2.0 / (cin * k * k))
            sd[f'features.{idx}.weight'] = torch.from_numpy(w.astype(np.float32))
            sd[f'features.{idx}.bias'] = torch.from_numpy((rs(f'{idx}.bias').randn(cout) * 0.05).astype(np.float32))
        return cls(sd, band_width)

    def state_dict(self):
        """The weights in the key spelling of the file ``__init__`` reads."""
        sd, i = {}, 0
        for op in self.plan:
            if op[0] == 'conv':
                sd[f'features.{op[1]}.weight'], sd[f'features.{op[1]}.bias'] = self.conv_w[i], self.conv_b[i]
                i += 1
        return sd

    def on(self, device):
        """The weights on `device` (cached)."""
        device = torch.device(device)
        if device.type == 'cuda' and device.index is None:
            device = torch.device('cuda', torch.cuda.current_device())
        held = self._device.get(device)
        if held is None:
            held = {'w': [t.to(device) for t in self.conv_w], 'b': [t.to(device) for t in self.conv_b], 'split': {}}
            self._device[device] = held
        return held

    def __call__(self, x, y):
        """The reference's ``CXLoss.forward`` scalar: ``mu`` over the whole batch, the mean of the frames' losses."""
        x, y = _checked(x, y, self, None)
        f = _features(torch.cat([x, y], 0), self)
        n = x.shape[0]
        return contextual_loss(f[:n], f[n:], self.band_width, mu='batch')


# ------------------------------------------------------------------ input checks

def _as_tensor(x):
    if isinstance(x, np.ndarray):
        x = torch.from_numpy(x)
    if not torch.is_tensor(x):
        raise ValueError('contextual scores take torch tensors or NumPy arrays')
    return x


def _checked_images(x, model, data_range=None):
    if not isinstance(model, CXScore):
        raise ValueError('model must be a contextual.CXScore')
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
        raise ValueError(f'contextual scores take 3 channels, got {c} (float32 is [N,3,H,W], uint8 is [N,H,W,3])')
    if data_range is not None and float(data_range) != want:
        raise ValueError(f'contextual scores are defined on images in [-1, 1] (data_range 2.0) or uint8 (data_range 255), got data_range '
                         f'{data_range} for {x.dtype}')
    if min(h, w) < MIN_SIDE:
        raise ValueError(f'a {h} x {w} image is too small: the two pools would leave no feature, both sides must be >= {MIN_SIDE}')
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


def _width(images):
    return images.shape[2] if images.dtype == torch.uint8 else images.shape[3]


# ------------------------------------------------------------------ the definition, in torch ops of one dtype

def reference_front(images, dtype=torch.float64):
    """Frames -> [N,3,H,W] of `dtype`, resized to 256 x 256 where the width is above 256."""
    v = images.permute(0, 3, 1, 2).to(dtype) / 127.5 - 1.0 if images.dtype == torch.uint8 else images.to(dtype)
    if v.shape[-1] > FRAME:
        v = torch.nn.functional.interpolate(v, (FRAME, FRAME), mode='bilinear', align_corners=False)
    return v


@torch.no_grad()
def reference_features(images, model, dtype=torch.float64):
    """The trunk in plain torch ops of `dtype` on the frames' device -> [N,256,h,w]."""
    F = torch.nn.functional
    v, i = reference_front(images, dtype), 0
    for op in model.plan:
        if op[0] == 'pool':
            v = F.max_pool2d(v, op[1], op[2])
        else:
            v = F.relu(F.conv2d(v, model.conv_w[i].to(device=v.device, dtype=dtype), model.conv_b[i].to(device=v.device, dtype=dtype), padding=1))
            i += 1
    return v


@torch.no_grad()
def reference_head(fx, fy, band_width=0.5, mu='batch', debug=False):
    """The head in torch ops of the maps' dtype -> (cx [N], cx_loss [N]); mu: 'batch', 'frame' or a [1,C] / [N,C] table."""
    n, c = fx.shape[:2]
    if torch.is_tensor(mu):
        table = mu.to(fx.dtype).reshape(-1, c, 1, 1)
    elif mu == 'batch':
        table = fy.mean(dim=(0, 2, 3), keepdim=True)
    elif mu == 'frame':
        table = fy.mean(dim=(2, 3), keepdim=True)
    else:
        raise ValueError(f"mu must be 'batch', 'frame' or a table, got {mu!r}")
    xh = torch.nn.functional.normalize(fx - table, p=2, dim=1).reshape(n, c, -1)
    yh = torch.nn.functional.normalize(fy - table, p=2, dim=1).reshape(n, c, -1)
    d = 1 - torch.bmm(xh.transpose(1, 2), yh)
    m = d.min(dim=2, keepdim=True)[0]
    w = torch.exp((1 - torch.clamp(d / (m + 1e-5), min=-10.0, max=10.0)) / band_width)
    s = w.sum(dim=2, keepdim=True)
    colmax = (w / s).max(dim=1)[0]
    cx = colmax.mean(dim=1)
    loss = -torch.log(cx + 1e-5)
    if debug:
        return cx, loss, {'mu': table.reshape(-1, c), 'xh': xh.transpose(1, 2), 'yh': yh.transpose(1, 2), 'm': m[:, :, 0], 's': s[:, :, 0],
                          'colmax': colmax}
    return cx, loss


def reference_compare(x, y, model, data_range=None):
    """``compare`` through the float64 restatement, wherever the inputs live; the results as float32."""
    x, y = _checked(x, y, model, data_range)
    f = reference_features(torch.cat([x, y], 0), model)
    n = x.shape[0]
    cx, loss = reference_head(f[:n], f[n:], model.band_width, 'frame')
    return {'cx': cx.float(), 'cx_loss': loss.float()}


# ------------------------------------------------------------------ the device path

@torch.no_grad()
def device_features(images, model):
    """The trunk through the HIP kernels -> float32 [N,256,h,w] on the frames' device."""
    from . import hipops
    images = images.contiguous()
    if _width(images) > FRAME:
        v = hipops.resize_bilinear(images, (FRAME, FRAME))
    elif images.dtype == torch.uint8:
        v = hipops.resize_bilinear(images, (images.shape[1], images.shape[2]))      # (the identity resize: the uint8 front end)
    else:
        v = images
    return _lpips.run_plan(v, model.plan, model.on(images.device))


def _features(images, model):
    return device_features(images, model) if images.is_cuda else reference_features(images, model)


@torch.no_grad()
def features(images, model):
    """relu3_4 maps of the frames -> float32 [N,256,h,w] on their device.  Device tensors: the HIP kernels, no fallback.  CPU tensors /
    NumPy arrays: the float64 restatement."""
    return _features(_checked_images(images, model), model).float()


@torch.no_grad()
def contextual_loss(fx, fy, band_width=0.5, mu='batch'):
    """The head for any float32 feature maps ``[N,C,h,w]`` (C >= 1, h w >= 1).  mu='batch': the reference's scalar, the mean over the
    frames of -log(cx + 1e-5) with the channel means of the whole of fy; mu='frame': float32 [N], every frame with its own means (what
    the reference gives at N = 1).  Float64 CPU maps are taken as they are (the restatement)."""
    if mu not in ('batch', 'frame'):
        raise ValueError(f"mu must be 'batch' or 'frame', got {mu!r}")
    if not (torch.is_tensor(fx) and torch.is_tensor(fy) and fx.dim() == 4 and fx.shape == fy.shape and fx.device == fy.device
            and fx.dtype == fy.dtype and fx.dtype in (torch.float32, torch.float64) and fx.numel() > 0):
        raise ValueError('contextual_loss takes two float32 [N,C,h,w] tensors of one shape on one device')
    if not float(band_width) > 0.0:
        raise ValueError(f'band_width must be positive, got {band_width}')
    if fx.is_cuda:
        if fx.dtype != torch.float32:
            raise ValueError('contextual_loss on the device takes float32 maps')
        from . import hipops
        loss = hipops.cx_head(fx.contiguous(), fy.contiguous(), band_width, mu)[1]
        if mu == 'frame':
            return loss
        return (loss.double().sum() / loss.shape[0]).float()        # (N numbers: not a hot path)
    loss = reference_head(fx.double(), fy.double(), band_width, mu)[1]
    return loss.float() if mu == 'frame' else loss.mean().float()


@torch.no_grad()
def compare(x, y, model, data_range=None):
    """Per-frame contextual score of `x` against `y`: ``{'cx': float32 [N], 'cx_loss': float32 [N]}`` on the inputs' device.
    Device tensors: the HIP kernels, no fallback.  CPU tensors / NumPy arrays: the float64 restatement."""
    x, y = _checked(x, y, model, data_range)
    n = x.shape[0]
    if not x.is_cuda:
        f = reference_features(torch.cat([x, y], 0), model)
        cx, loss = reference_head(f[:n], f[n:], model.band_width, 'frame')
        return {'cx': cx.float(), 'cx_loss': loss.float()}
    from . import hipops
    f = device_features(torch.cat([x, y], 0), model)
    cx, loss = hipops.cx_head(f[:n], f[n:], model.band_width, 'frame')
    return {'cx': cx, 'cx_loss': loss}


class CXLoss:
    """The reference's ``CXLoss`` (encoder_inversion/criteria/cx_loss.py) for inference: ``forward(x, y)`` is its scalar."""

    def __init__(self, path_vgg19, band_width=0.5):
        self.model = path_vgg19 if isinstance(path_vgg19, CXScore) else CXScore(path_vgg19, band_width)
        self.band_width = self.model.band_width

    def forward(self, x, y):
        return self.model(x, y)

    __call__ = forward
