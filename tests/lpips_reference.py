"""An independent plain-torch statement of the reference's LPIPS criterion (encoder_inversion/criteria/lpips: lpips.py, networks.py,
utils.py), for tests/test_lpips_cpu.py and tests/test_lpips_gpu.py.  Not a test.

The feature stacks are ``nn.Sequential`` in torchvision's index layout (``alexnet().features`` / ``vgg16().features``), the taps are
chosen by the criterion's 1-based ``target_layers``, activations are normalised with the ``+ eps`` outside the square root, the linear
layers are bias-free 1x1 convolutions and ``forward`` returns ``sum / N``.  ``per_frame`` gives the [N,5] layer values the scalar is
the sum of.  Everything runs in the dtype the module was built with (float64: the yardstick; float32: its own rounding error, e32)."""
import torch
import torch.nn as nn

TARGET_LAYERS = {'alex': [2, 5, 8, 10, 12], 'vgg': [4, 9, 16, 23, 30]}
N_CHANNELS = {'alex': [64, 192, 384, 256, 256], 'vgg': [64, 128, 256, 512, 512]}


def alexnet_features():
    return nn.Sequential(
        nn.Conv2d(3, 64, kernel_size=11, stride=4, padding=2), nn.ReLU(inplace=True), nn.MaxPool2d(kernel_size=3, stride=2),
        nn.Conv2d(64, 192, kernel_size=5, padding=2), nn.ReLU(inplace=True), nn.MaxPool2d(kernel_size=3, stride=2),
        nn.Conv2d(192, 384, kernel_size=3, padding=1), nn.ReLU(inplace=True),
        nn.Conv2d(384, 256, kernel_size=3, padding=1), nn.ReLU(inplace=True),
        nn.Conv2d(256, 256, kernel_size=3, padding=1), nn.ReLU(inplace=True), nn.MaxPool2d(kernel_size=3, stride=2))


def vgg16_features():
    layers, cin = [], 3
    for v in [64, 64, 'M', 128, 128, 'M', 256, 256, 256, 'M', 512, 512, 512, 'M', 512, 512, 512, 'M']:
        if v == 'M':
            layers.append(nn.MaxPool2d(kernel_size=2, stride=2))
        else:
            layers += [nn.Conv2d(cin, v, kernel_size=3, padding=1), nn.ReLU(inplace=True)]
            cin = v
    return nn.Sequential(*layers)


def normalize_activation(x, eps=1e-10):
    norm_factor = torch.sqrt(torch.sum(x ** 2, dim=1, keepdim=True))
    return x / (norm_factor + eps)


class ReferenceLPIPS(nn.Module):
    def __init__(self, net, backbone_state, lin_state, dtype=torch.float64):
        super().__init__()
        self.layers = alexnet_features() if net == 'alex' else vgg16_features()
        self.target_layers = TARGET_LAYERS[net]
        self.lin = nn.ModuleList([nn.Sequential(nn.Identity(), nn.Conv2d(nc, 1, 1, 1, 0, bias=False)) for nc in N_CHANNELS[net]])
        self.layers.load_state_dict({k.replace('features.', ''): v for k, v in backbone_state.items()})
        self.lin.load_state_dict({k.replace('lin', '').replace('model.', ''): v for k, v in lin_state.items()})
        self.to(dtype)
        self.register_buffer('mean', torch.tensor([-.030, -.088, -.188], dtype=dtype)[None, :, None, None])
        self.register_buffer('std', torch.tensor([.458, .448, .450], dtype=dtype)[None, :, None, None])
        self.dtype = dtype
        self.requires_grad_(False)

    def features(self, x):
        x = (x - self.mean) / self.std
        output = []
        for i, layer in enumerate(self.layers, 1):
            x = layer(x)
            if i in self.target_layers:
                output.append(normalize_activation(x))
            if len(output) == len(self.target_layers):
                break
        return output

    def per_frame(self, x, y):
        """[N,5]: the spatial mean of every linear layer's map, per frame."""
        feat_x, feat_y = self.features(x.to(self.dtype)), self.features(y.to(self.dtype))
        diff = [(fx - fy) ** 2 for fx, fy in zip(feat_x, feat_y)]
        return torch.cat([l(d).mean((2, 3)) for d, l in zip(diff, self.lin)], 1)

    def forward(self, x, y):
        feat_x, feat_y = self.features(x.to(self.dtype)), self.features(y.to(self.dtype))
        diff = [(fx - fy) ** 2 for fx, fy in zip(feat_x, feat_y)]
        res = [l(d).mean((2, 3), True) for d, l in zip(diff, self.lin)]
        return torch.sum(torch.cat(res, 0)) / x.shape[0]


def images(seed, n, h, w):
    """A seeded pair of float32 [n,3,h,w] batches in [-1, 1]: smooth structure plus noise; the second is a perturbed copy of the first."""
    g = torch.Generator().manual_seed(seed)
    yy, xx = torch.meshgrid(torch.linspace(-1, 1, h), torch.linspace(-1, 1, w), indexing='ij')
    phase = torch.rand(n, 3, 1, 1, generator=g) * 6.28
    base = 0.6 * torch.sin(3.0 * xx[None, None] + phase) * torch.cos(2.0 * yy[None, None] - phase)
    x = (base + 0.3 * torch.randn(n, 3, h, w, generator=g)).clamp(-1, 1)
    y = (x + 0.15 * torch.randn(n, 3, h, w, generator=g)).clamp(-1, 1)
    return x.float().contiguous(), y.float().contiguous()


def to_uint8(x):
    """float [-1, 1] NCHW -> uint8 NHWC."""
    return ((x + 1.0) * 127.5).round().clamp(0, 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous()
