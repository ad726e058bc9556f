"""MobileNetV2 encoder behind DepthNetPretrained (reference: model/build_model/pretrained_nets.py:11-117, config-example.py
RIGID_MOBILE / TEST_PLAN_LOW "vode30_mobile").

The reference takes `tf.keras.applications.MobileNetV2(include_top=False)` from tensorflow==2.4.1 (alpha = 1.0) and taps the five
layers scaled_layers.json lists first: block_1_expand_relu / block_3_expand_relu / block_6_expand_relu / block_13_expand_relu /
out_relu at 1/2 ... 1/32.  This file restates that published architecture (Sandler et al., "MobileNetV2: Inverted Residuals and
Linear Bottlenecks") as torch modules on the gfx950 kernels:

    Conv1 3x3/2 (ZeroPadding2D(correct_pad) + valid = TF SAME) -> bn_Conv1 -> ReLU6
    expanded_conv:  depthwise 3x3 -> BN -> ReLU6 -> project 1x1 (16) -> BN
    block_1..16:    expand 1x1 (6x) -> BN -> ReLU6 -> depthwise 3x3 (stride s) -> BN -> ReLU6 -> project 1x1 -> BN (+ input)
    Conv_1 1x1 (1280) -> Conv_1_bn -> ReLU6

Every BatchNorm that is followed by a ReLU6 and feeds a depthwise stage STORES ITS PRE-ACTIVATION output; the depthwise kernel
clamps on load (hip.ops.dwconv_bn_relu6, act_in) and its data gradient is already the gradient w.r.t. that BatchNorm's output, so
a block is three launches forward (pointwise + BN, depthwise + BN + ReLU6, pointwise + BN [+ residual]) and three backward.  The
five tapped tensors are the post-ReLU6 ones: a plain clamp of the stored pre-activation tensor (five launches per pass).

PARITY UNPINNED against TensorFlow itself (no golden activations or ImageNet weights offline).  Pinned: the parameter count
equals Keras' published 2,257,984; the five taps have the sizes scaled_layers.json records; an independent fp64 restatement in
Keras conventions (tests/ref_mobilenet_v2.py) yields the same taps on the same weights; every Keras variable of the no-top model
lands on exactly one tensor (tests/golden/mobilenet_v2_manifest.json).  Bug-compatible, as the NASNet encoder: `preprocess_input`
(x / 127.5 - 1) is applied to images already in [-1, 1] (pretrained_nets.py:40); BatchNorm runs on its moving statistics
(train_val.py:82) with trainable gamma / beta.  Unlike NASNet the stem convolution is SAME-padded, so nothing is resized.
"""
import functools

import torch.nn as nn
import torch.nn.functional as F

from ...hip import conv as _conv
from ...hip import ops as _ops
from ...utils.util_class import WrongInputException
from . import keras_weights as _kw
from .keras_weights import _from_keras  # noqa: F401  (the layout converter stays addressable through this module)
from .pretrained_nets import BN_EPS, FrozenBatchNorm, KerasApplicationEncoder, conv1x1_bn, correct_pad, zero_pad

# (output channels, stride) of block_1 .. block_16, expansion 6 (keras mobilenet_v2.py, alpha = 1.0)
BLOCKS = ((24, 2), (24, 1), (32, 2), (32, 1), (32, 1), (64, 2), (64, 1), (64, 1), (64, 1), (96, 1), (96, 1), (96, 1),
          (160, 2), (160, 1), (160, 1), (320, 1))
TAP_BLOCKS = (1, 3, 6, 13)                 # block_<k>_expand_relu; the fifth tap is out_relu


_he = KerasApplicationEncoder.he


class InvertedResidual(nn.Module):
    """_inverted_res_block.  expansion 1 (expanded_conv) has no expand layer: its input is the stem BatchNorm's pre-activation
    output."""

    def __init__(self, cin, cout, stride, expansion):
        super().__init__()
        mid = cin * expansion
        self.stride = stride
        self.use_res = stride == 1 and cin == cout
        self.expand = self.expand_bn = None
        if expansion != 1:
            self.expand = _he(nn.Conv2d(cin, mid, 1, bias=False))
            self.expand_bn = FrozenBatchNorm(mid)
        self.depthwise = _he(nn.Conv2d(mid, mid, 3, stride, padding=0 if stride == 2 else 1, groups=mid, bias=False))
        self.depthwise_bn = FrozenBatchNorm(mid)
        self.project = _he(nn.Conv2d(mid, cout, 1, bias=False))
        self.project_bn = FrozenBatchNorm(cout)

    def forward(self, x):
        """-> (block output, pre-activation output of the expand BatchNorm: what `block_k_expand_relu` clamps)."""
        h = x if self.expand is None else conv1x1_bn(x, self.expand.weight, self.expand_bn)
        d = _ops.dwconv_bn_relu6(h, self.depthwise.weight, self.depthwise_bn, self.stride, act_in=True, eps=BN_EPS)
        return conv1x1_bn(d, self.project.weight, self.project_bn, residual=x if self.use_res else None), h


class MobileNetV2Encoder(KerasApplicationEncoder):
    """Keras MobileNetV2(alpha=1.0, include_top=False) with the five taps of scaled_layers.json.

    forward(image NCHW in [-1,1], H and W multiples of 32) -> [c1 (1/2, 96 ch), c2 (1/4, 144), c3 (1/8, 192), c4 (1/16, 576),
    c5 (1/32, 1280)], all post-ReLU6."""
    TAP_NAMES = ("block_1_expand_relu", "block_3_expand_relu", "block_6_expand_relu", "block_13_expand_relu", "out_relu")
    TAP_CHANNELS = (96, 144, 192, 576, 1280)
    net_name = "MobileNetV2"

    def __init__(self):
        super().__init__()
        self.conv1 = _he(nn.Conv2d(3, 32, 3, 2, 0, bias=False))
        self.bn_conv1 = FrozenBatchNorm(32)
        blocks = [InvertedResidual(32, 16, 1, 1)]                   # expanded_conv
        cin = 16
        for cout, stride in BLOCKS:
            blocks.append(InvertedResidual(cin, cout, stride, 6))   # block_1 .. block_16
            cin = cout
        self.blocks = nn.ModuleList(blocks)
        self.conv_last = _he(nn.Conv2d(cin, 1280, 1, bias=False))   # Conv_1
        self.bn_last = FrozenBatchNorm(1280)                        # Conv_1_bn
        self.out_channels = 1280

    def preprocess(self, image):
        """pretrained_nets.py:36-43 without the resize (the stem convolution is SAME-padded)."""
        return image / 127.5 - 1.0

    def stem(self, image):
        """Conv1 + bn_Conv1, pre-activation (its ReLU6 rides in expanded_conv's depthwise loads)."""
        x = self.preprocess(image)
        if _conv.usable(x, self.conv1, 1.0):
            x = self.stem_matrix_core(x, self.conv1, 2)
        else:                                                         # host tensors / fp32: ZeroPadding2D(correct_pad) + valid
            x = F.conv2d(zero_pad(x, correct_pad(x.shape[2], x.shape[3], 3)), self.conv1.weight, None, 2)
        return self.bn_conv1(x)

    def forward(self, image, physical_taps=False):
        self.check_image(image)
        x = self.stem(image)
        taps = []
        for k, block in enumerate(self.blocks):                       # k = 0: expanded_conv, k >= 1: block_k
            x, pre = block(x)
            if k in TAP_BLOCKS:
                taps.append(F.relu6(pre))
        x = conv1x1_bn(x, self.conv_last.weight, self.bn_last)
        taps.append(F.relu6(x))
        return taps


# ------------------------------------------------------------------------------------------ Keras weights
def keras_variable_map(encoder):
    """{keras variable name: (tensor of the encoder, kind)} with kind in {"conv", "depthwise", "vector"}
    (tf.keras.applications.MobileNetV2 layer names; layouts as keras_weights._to_keras)."""
    out = {}
    bn = functools.partial(_kw.bn, out)

    out["Conv1/kernel"] = (encoder.conv1.weight, "conv")
    bn("bn_Conv1", encoder.bn_conv1)
    if len(encoder.blocks) != len(BLOCKS) + 1:
        raise WrongInputException("keras_variable_map: not the MobileNetV2 block sequence")
    for k, block in enumerate(encoder.blocks):
        prefix = "expanded_conv" if k == 0 else f"block_{k}"
        if block.expand is not None:
            out[f"{prefix}_expand/kernel"] = (block.expand.weight, "conv")
            bn(f"{prefix}_expand_BN", block.expand_bn)
        out[f"{prefix}_depthwise/depthwise_kernel"] = (block.depthwise.weight, "depthwise")
        bn(f"{prefix}_depthwise_BN", block.depthwise_bn)
        out[f"{prefix}_project/kernel"] = (block.project.weight, "conv")
        bn(f"{prefix}_project_BN", block.project_bn)
    out["Conv_1/kernel"] = (encoder.conv_last.weight, "conv")
    bn("Conv_1_bn", encoder.bn_last)
    return out


def export_keras_weights(encoder):
    """{keras variable name: float32 array in the keras layout} of the encoder's current weights."""
    return _kw.export_weights(keras_variable_map(encoder))


def load_keras_weights(encoder, weights):
    """Fills the encoder from Keras MobileNetV2(include_top=False) variables (a path or a {name: array} dict).  Strict: a
    missing, unknown or mis-shaped variable raises; nothing is loaded partially."""
    return _kw.load_weights(keras_variable_map(encoder), weights, "MobileNetV2")
