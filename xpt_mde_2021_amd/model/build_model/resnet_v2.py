"""ResNet50V2 encoder behind DepthNetPretrained (reference: model/build_model/pretrained_nets.py:31-101, config-example.py:51-53).

The reference takes `tf.keras.applications.ResNet50V2(include_top=False)` from tensorflow==2.4.1 and taps the five layers
scaled_layers.json lists: conv1_conv / conv2_block3_1_relu / conv3_block4_1_relu / conv4_block6_1_relu / post_relu at 1/2 ... 1/32.
This file restates that published architecture (He et al., "Identity Mappings in Deep Residual Networks"; keras resnet_v2 `block2`
/ `stack2`) as torch modules on the gfx950 kernels:

    conv1_pad ZeroPadding2D(3) -> conv1_conv 7x7/2 (64, bias, valid)  -> pool1_pad ZeroPadding2D(1) -> pool1_pool 3x3/2 max
    stack2(64, 3) -> stack2(128, 4) -> stack2(256, 6) -> stack2(512, 3, stride1=1);  the LAST block of a stack carries the stride
    block2:  preact = relu(BN(x));  shortcut = 0_conv(preact) (first block) | MaxPooling2D(1, stride)(x) | x
             h = relu(BN(1_conv(preact)));  h = relu(BN(2_conv 3x3/stride (ZeroPadding2D(1)(h))));  out = shortcut + 3_conv(h)
    post_bn -> post_relu

A block's `_3_conv`, its shortcut add AND the next block's pre-activation BatchNorm + ReLU are ONE launch (hip.ops.res_join, the
residual junction of csrc/xpt_resnet.hip): a block is six launches forward -- 1x1 GEMM, BN + ReLU, 3x3 implicit GEMM, BN + ReLU,
junction (the first block's `_0_conv` rides in it as a second GEMM).  pool1 is hip.ops.maxpool3s2_zero.

PARITY UNPINNED against TensorFlow itself (no golden activations or ImageNet weights offline).  Pinned: the parameter count equals
Keras' published 23,564,800; the five taps sit at the layer indices and have the sizes scaled_layers.json records; an independent
fp64 restatement in Keras conventions (tests/ref_resnet50v2.py) yields the same taps on the same weights; every Keras variable of
the no-top model lands on exactly one tensor (tests/golden/resnet50v2_manifest.json).  Bug-compatible:
  * the reference imports `preprocess_input` from applications.resnet (NOT resnet_v2): caffe mode, RGB -> BGR and minus
    (103.939, 116.779, 123.68), no scaling -- applied to images already in [-1, 1];
  * the strided 3x3 convolutions pad (1, 1) and run VALID: on an even extent that is not TF SAME, which pads (0, 1);
  * pool1's padding is zeros that take part in the max (the conv1_conv output is signed);
  * BatchNorm runs on its moving statistics (train_val.py:82) with trainable gamma / beta; epsilon is 1.001e-5.
"""
import functools

import torch
import torch.nn as nn
import torch.nn.functional as F

from ...hip import conv as _conv
from ...hip import ops as _ops
from ...hip.lib import half as _half
from ...utils.util_class import WrongInputException
from . import keras_weights as _kw
from .keras_weights import _from_keras  # noqa: F401  (the layout converter stays addressable through this module)
from .pretrained_nets import FrozenBatchNorm, KerasApplicationEncoder, conv1x1

RES_BN_EPS = 1.001e-5                    # keras resnet_v2: BatchNormalization(epsilon=1.001e-5) everywhere
STACKS = ((64, 3, 2), (128, 4, 2), (256, 6, 2), (512, 3, 1))          # (filters, blocks, stride1) of conv2 .. conv5
CAFFE_MEAN_BGR = (103.939, 116.779, 123.68)
TAP_NAMES = ("conv1_conv", "conv2_block3_1_relu", "conv3_block4_1_relu", "conv4_block6_1_relu", "post_relu")


_he = KerasApplicationEncoder.he


class ResBatchNorm(FrozenBatchNorm):
    """FrozenBatchNorm with the resnet_v2 epsilon; every one of them is followed by a ReLU."""

    def forward(self, x):
        if x.is_cuda:
            return _ops.batchnorm_inference(x, self.weight, self.bias, self.running_mean, self.running_var, RES_BN_EPS, slope=0.0)
        return F.relu(F.batch_norm(x, self.running_mean, self.running_var, self.weight, self.bias, False, 0.0, RES_BN_EPS))


class Block2(nn.Module):
    """keras resnet_v2 `block2`.  `preact_bn` is the BatchNorm applied to this block's INPUT: it is evaluated by the junction of
    the block before (or, for conv2_block1, on its own behind pool1)."""

    def __init__(self, name, cin, filters, stride, conv_shortcut):
        super().__init__()
        self.name, self.stride = name, stride
        self.preact_bn = ResBatchNorm(cin)
        self.conv0 = _he(nn.Conv2d(cin, 4 * filters, 1, bias=True)) if conv_shortcut else None
        self.conv1 = _he(nn.Conv2d(cin, filters, 1, bias=False))
        self.bn1 = ResBatchNorm(filters)
        self.conv2 = _he(nn.Conv2d(filters, filters, 3, stride, padding=0, bias=False))
        self.bn2 = ResBatchNorm(filters)
        self.conv3 = _he(nn.Conv2d(filters, 4 * filters, 1, bias=True))

    def forward(self, x, pre, next_bn):
        """x: the block input, pre = relu(preact_bn(x)) -> (out, relu(next_bn(out)), the `_1_relu` activation)."""
        h1 = self.bn1(conv1x1(pre, self.conv1.weight))
        if _conv.usable(h1, self.conv2, 1.0):                         # ZeroPadding2D(1) + valid, no F.pad launch
            h2 = _conv.conv2d_same(h1, self.conv2.weight, None, self.stride, 1.0, pad=1)
        else:
            h2 = F.conv2d(F.pad(h1, (1, 1, 1, 1)), self.conv2.weight, None, self.stride)
        h2 = self.bn2(h2)
        if self.conv0 is not None:
            out, nxt = _ops.res_join(h2, self.conv3.weight, self.conv3.bias, next_bn, RES_BN_EPS, sc_x=pre,
                                     sc_w=self.conv0.weight, sc_b=self.conv0.bias)
        else:
            out, nxt = _ops.res_join(h2, self.conv3.weight, self.conv3.bias, next_bn, RES_BN_EPS, shortcut=x, stride=self.stride)
        return out, nxt, h1


class ResNet50V2Encoder(KerasApplicationEncoder):
    """Keras ResNet50V2(include_top=False) with the five taps of scaled_layers.json.

    forward(image NCHW in [-1,1], H and W multiples of 32) -> [c1 (1/2, 64 ch, the LINEAR conv1_conv output), c2 (1/4, 64),
    c3 (1/8, 128), c4 (1/16, 256), c5 (1/32, 2048)]; c2 .. c5 post-ReLU."""
    TAP_NAMES = TAP_NAMES
    TAP_CHANNELS = (64, 64, 128, 256, 2048)
    net_name = "ResNet50V2"

    def __init__(self):
        super().__init__()
        self._caffe_mean = {}                                         # (device, dtype) -> [1,3,1,1] constant; not a Keras variable
        self.conv1 = _he(nn.Conv2d(3, 64, 7, 2, 0, bias=True))       # conv1_conv
        blocks, taps, cin = [], {}, 64
        for s, (filters, n, stride1) in enumerate(STACKS, start=2):
            for b in range(1, n + 1):
                name = f"conv{s}_block{b}"
                if f"{name}_1_relu" in TAP_NAMES:
                    taps[len(blocks)] = filters
                blocks.append(Block2(name, cin, filters, stride1 if b == n else 1, conv_shortcut=(b == 1)))
                cin = 4 * filters
        self.blocks = nn.ModuleList(blocks)
        self.tap_blocks = tuple(sorted(taps))
        self.post_bn = ResBatchNorm(cin)
        self.out_channels = cin

    def preprocess(self, image):
        """applications.resnet.preprocess_input (caffe mode) on the [-1, 1] image, as the reference applies it."""
        key = (image.device, image.dtype)
        if key not in self._caffe_mean:                               # (first used in an eager step: no upload inside a capture)
            self._caffe_mean[key] = torch.tensor(CAFFE_MEAN_BGR, dtype=image.dtype, device=image.device).view(1, 3, 1, 1)
        return image.flip(1) - self._caffe_mean[key]

    def stem(self, image):
        """conv1_pad + conv1_conv: the first tap, linear."""
        x = self.preprocess(image)
        dtype = torch.get_autocast_dtype("cuda") if torch.is_autocast_enabled() else x.dtype
        if x.is_cuda and dtype == _half() and self.conv1.weight.dtype == torch.float32:
            return self.stem_matrix_core(x, self.conv1, 2, pad=3)
        return F.conv2d(F.pad(x, (3, 3, 3, 3)), self.conv1.weight, self.conv1.bias, 2)

    def forward(self, image, physical_taps=False):
        self.check_image(image)
        c1 = self.stem(image)
        taps = [c1]
        x = _ops.maxpool3s2_zero(c1)                                  # pool1_pad + pool1_pool
        pre = self.blocks[0].preact_bn(x)
        for k, block in enumerate(self.blocks):
            next_bn = self.blocks[k + 1].preact_bn if k + 1 < len(self.blocks) else self.post_bn
            x, pre, h1 = block(x, pre, next_bn)
            if k in self.tap_blocks:
                taps.append(h1)
        taps.append(pre)                                              # post_relu
        return taps


# ------------------------------------------------------------------------------------------ Keras weights
def keras_variable_map(encoder):
    """{keras variable name: (tensor of the encoder, kind)} with kind in {"conv", "vector"}
    (tf.keras.applications.resnet_v2 layer names; layouts as keras_weights._to_keras)."""
    out = {}
    bn, conv = functools.partial(_kw.bn, out), functools.partial(_kw.conv, out)

    conv("conv1_conv", encoder.conv1)
    if len(encoder.blocks) != sum(n for _, n, _ in STACKS):
        raise WrongInputException("keras_variable_map: not the ResNet50V2 block sequence")
    for block in encoder.blocks:
        bn(f"{block.name}_preact_bn", block.preact_bn)
        if block.conv0 is not None:
            conv(f"{block.name}_0_conv", block.conv0)
        conv(f"{block.name}_1_conv", block.conv1)
        bn(f"{block.name}_1_bn", block.bn1)
        conv(f"{block.name}_2_conv", block.conv2)
        bn(f"{block.name}_2_bn", block.bn2)
        conv(f"{block.name}_3_conv", block.conv3)
    bn("post_bn", encoder.post_bn)
    return out


def export_keras_weights(encoder):
    """{keras variable name: float32 array in the keras layout} of the encoder's current weights."""
    return _kw.export_weights(keras_variable_map(encoder))


def load_keras_weights(encoder, weights):
    """Fills the encoder from Keras ResNet50V2(include_top=False) variables (a path or a {name: array} dict).  Strict: a
    missing, unknown or mis-shaped variable raises; nothing is loaded partially."""
    return _kw.load_weights(keras_variable_map(encoder), weights, "ResNet50V2")
