"""ArcFace-style IR / IR-SE face embedding network (reference: encoder_inversion/models/model_irse.py, ``Backbone``), built on the
residual units of ``helpers``.  Module and parameter names follow the reference, so that the published ``model_ir_se50.pth`` loads by
name: ``input_layer.{0,1,2}``, ``body.N.{res_layer,shortcut_layer}``, ``output_layer.{0,3,4}``.

This module is the torch.nn statement of the network (any dtype, any device; its ``Conv2d`` layers take the HIP convolutions on
device tensors like every encoder here).  The scoring path with the 7^2 stage and the head on their own kernels is
``invertavatar_amd/identity.py``."""
from torch.nn import BatchNorm1d, BatchNorm2d, Dropout, Linear, Module, PReLU, Sequential

from . import helpers
from .helpers import Flatten, bottleneck_IR, bottleneck_IR_SE, get_blocks, l2_norm
from .layers import Conv2d

STAGE_ENDS = {50: (2, 6, 20, 23)}       # index of the last unit of each of the four stages


class Backbone(Module):
    def __init__(self, input_size, num_layers, mode='ir', drop_ratio=0.4, affine=True):
        super().__init__()
        if input_size not in (112, 224):
            raise ValueError('input_size should be 112 or 224')
        if mode not in ('ir', 'ir_se'):
            raise ValueError('mode should be ir or ir_se')
        unit = bottleneck_IR if mode == 'ir' else bottleneck_IR_SE
        side = input_size // 16
        self.input_layer = Sequential(Conv2d(3, 64, (3, 3), 1, 1, bias=False), BatchNorm2d(64), PReLU(64))
        self.output_layer = Sequential(BatchNorm2d(512), Dropout(drop_ratio), Flatten(), Linear(512 * side * side, 512),
                                       BatchNorm1d(512, affine=affine))
        self.body = Sequential(*[unit(u.in_channel, u.depth, u.stride) for stage in get_blocks(num_layers) for u in stage])

    def forward(self, x):
        x = self.input_layer(x)
        x, _ = helpers.run_trunk(self.body, x, ())
        return l2_norm(self.output_layer(x))

    def stages(self, x, ends):
        """(activation after the input layer, after each unit index in `ends`, the un-normalised head output, the embedding)."""
        x = self.input_layer(x)
        last, taps = helpers.run_trunk(self.body, x, tuple(ends))
        z = self.output_layer(last)
        return [x] + list(taps) + [z, l2_norm(z)]


def IR_SE_50(input_size):
    return Backbone(input_size, num_layers=50, mode='ir_se', drop_ratio=0.4, affine=False)
