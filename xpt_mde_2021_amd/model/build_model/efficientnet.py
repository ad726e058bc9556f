"""EfficientNet-B0 / B3 / B5 / B7 encoders behind DepthNetPretrained (reference: model/build_model/pretrained_nets.py:11-117;
config-example.py JOINT_NET "depth" default EfficientNetB5, RIGID_EF0 / EF3 / EF5 / EF7, TEST_PLAN "vode30_ef0" ... "vode30_ef7").

The reference takes `tf.keras.applications.EfficientNetB{0,3,5,7}(include_top=False)` from tensorflow==2.4.1 and taps the five
layers scaled_layers.json lists first: block2a / 3a / 4a / 6a_expand_activation and top_activation at 1/2 ... 1/32.  This file
restates that published architecture (Tan & Le, "EfficientNet: Rethinking Model Scaling for Convolutional Neural Networks")
as torch modules on the gfx950 kernels, parametrised by the (width, depth) coefficients:

    rescaling (1/255) -> normalization -> stem_conv 3x3/2 (ZeroPadding2D(correct_pad) + valid = TF SAME) -> stem_bn -> swish
    block<i><a..>:  [expand 1x1 -> BN -> swish] -> depthwise k x k (stride s) -> BN -> swish -> squeeze-and-excite (mean ->
                    1x1 + bias, swish -> 1x1 + bias, sigmoid -> multiply) -> project 1x1 -> BN (+ input)
    top_conv 1x1 (round_filters(1280)) -> top_bn -> swish

Every BatchNorm that is followed by a swish STORES ITS PRE-ACTIVATION output; the depthwise kernel activates on load
(hip.ops.mbconv_se, act_in), so a block is five launches forward: expand + BN, depthwise stage, excite, scale, project + BN
[+ residual].  The five tapped tensors are a plain silu of the stored pre-activation tensor.  The block Dropout (drop-connect)
is the identity: the reference calls the model without a training flag (train_val.py:82).

PARITY UNPINNED against TensorFlow itself (no golden activations or ImageNet weights offline).  Pinned: the parameter counts
equal Keras' published no-top totals (B0 4,049,571; B3 10,783,535; B5 28,513,527; B7 64,097,687); the five taps have the sizes
scaled_layers.json records; an independent fp64 restatement in Keras conventions (tests/ref_efficientnet.py) yields the same taps
on the same weights; every Keras variable of the no-top B0 lands on exactly one tensor
(tests/golden/efficientnet_b0_manifest.json).  Bug-compatible: `efficientnet.preprocess_input` is the identity, so the model's
own Rescaling(1/255) and Normalization layers meet images in [-1, 1]: (x / 255 - mean) / sqrt(var); BatchNorm runs on its moving
statistics with trainable gamma / beta.  B3 / B5 / B7 are pinned on the CPU only: they have not run on hardware.
"""
import functools
import math

import torch
import torch.nn as nn
import torch.nn.functional as F

from ...hip import conv as _conv
from ...hip import ops as _ops
from ...utils.util_class import WrongInputException
from . import keras_weights as _kw
from .keras_weights import _from_keras  # noqa: F401  (the layout converter stays addressable through this module)
from .pretrained_nets import BN_EPS, FrozenBatchNorm, KerasApplicationEncoder, conv1x1_bn, correct_pad, zero_pad

# (kernel, repeats, input filters, output filters, expand ratio, stride) of keras efficientnet.DEFAULT_BLOCKS_ARGS; se_ratio 0.25
BLOCK_ARGS = ((3, 1, 32, 16, 1, 1), (3, 2, 16, 24, 6, 2), (5, 2, 24, 40, 6, 2), (3, 3, 40, 80, 6, 2), (5, 3, 80, 112, 6, 1),
              (5, 4, 112, 192, 6, 2), (3, 1, 192, 320, 6, 1))
COEFFICIENTS = {"EfficientNetB0": (1.0, 1.0), "EfficientNetB3": (1.2, 1.4), "EfficientNetB5": (1.6, 2.2),
                "EfficientNetB7": (2.0, 3.1)}                                          # (width, depth)
TAP_NAMES = ("block2a_expand_activation", "block3a_expand_activation", "block4a_expand_activation", "block6a_expand_activation",
             "top_activation")
SE_RATIO = 0.25


def round_filters(filters, width, divisor=8):
    filters *= width
    new = max(divisor, int(filters + divisor / 2) // divisor * divisor)
    if new < 0.9 * filters:
        new += divisor
    return int(new)


def round_repeats(repeats, depth):
    return int(math.ceil(depth * repeats))


_he = KerasApplicationEncoder.he


class MBConv(nn.Module):
    """keras efficientnet `block`.  expand ratio 1 has no expand layer: its input feeds the depthwise stage directly -- the stem
    BatchNorm's pre-activation output for the very first block (input_activated=False: the swish rides in the depthwise loads),
    a finished block output for its repeats in B3 / B5 / B7."""

    def __init__(self, name, cin, cout, k, stride, expansion, input_activated=True):
        super().__init__()
        mid = cin * expansion
        self.name, self.k, self.stride = name, k, stride
        self.use_res = stride == 1 and cin == cout
        self.act_in = expansion != 1 or not input_activated
        self.expand = self.expand_bn = None
        if expansion != 1:
            self.expand = _he(nn.Conv2d(cin, mid, 1, bias=False))
            self.expand_bn = FrozenBatchNorm(mid)
        self.depthwise = _he(nn.Conv2d(mid, mid, k, stride, padding=0, groups=mid, bias=False))
        self.depthwise_bn = FrozenBatchNorm(mid)
        se = max(1, int(cin * SE_RATIO))
        self.se_reduce = _he(nn.Conv2d(mid, se, 1, bias=True))
        self.se_expand = _he(nn.Conv2d(se, mid, 1, bias=True))
        self.project = _he(nn.Conv2d(mid, cout, 1, bias=False))
        self.project_bn = FrozenBatchNorm(cout)

    def forward(self, x):
        """-> (block output, pre-activation output of the expand BatchNorm: what `<name>_expand_activation` activates)."""
        h = x if self.expand is None else conv1x1_bn(x, self.expand.weight, self.expand_bn)
        z = _ops.mbconv_se(h, self.depthwise.weight, self.depthwise_bn, self.se_reduce.weight, self.se_reduce.bias,
                           self.se_expand.weight, self.se_expand.bias, self.k, self.stride, act_in=self.act_in, eps=BN_EPS)
        return conv1x1_bn(z, self.project.weight, self.project_bn, residual=x if self.use_res else None), h


class EfficientNetEncoder(KerasApplicationEncoder):
    """Keras EfficientNetB<n>(include_top=False) with the five taps of scaled_layers.json.

    forward(image NCHW in [-1,1], H and W multiples of 32) -> [c1 (1/2), c2 (1/4), c3 (1/8), c4 (1/16), c5 (1/32)], all
    post-swish; B0 widths 96 / 144 / 240 / 672 / 1280."""
    TAP_NAMES = TAP_NAMES

    def __init__(self, net_name="EfficientNetB0"):
        super().__init__()
        if net_name not in COEFFICIENTS:
            raise WrongInputException(f"EfficientNet encoder: unknown variant {net_name} (available: {tuple(COEFFICIENTS)})")
        width, depth = COEFFICIENTS[net_name]
        self.net_name = net_name
        self.register_buffer("norm_mean", torch.zeros(3))                 # normalization/mean, /variance, /count: un-adapted
        self.register_buffer("norm_variance", torch.ones(3))
        self.register_buffer("norm_count", torch.zeros(()))
        stem = round_filters(32, width)
        self.stem_conv = _he(nn.Conv2d(3, stem, 3, 2, 0, bias=False))
        self.stem_bn = FrozenBatchNorm(stem)
        blocks, taps = [], {}
        for i, (k, repeats, fin, fout, expand, stride) in enumerate(BLOCK_ARGS):
            fin, fout = round_filters(fin, width), round_filters(fout, width)
            for j in range(round_repeats(repeats, depth)):
                name = f"block{i + 1}{chr(97 + j)}"
                if f"{name}_expand_activation" in TAP_NAMES:
                    taps[len(blocks)] = fin * expand
                blocks.append(MBConv(name, fin, fout, k, stride if j == 0 else 1, expand, input_activated=bool(blocks)))
                fin = fout
        self.blocks = nn.ModuleList(blocks)
        self.tap_blocks = tuple(sorted(taps))
        top = round_filters(1280, width)
        self.top_conv = _he(nn.Conv2d(fin, top, 1, bias=False))
        self.top_bn = FrozenBatchNorm(top)
        self.out_channels = top
        self.TAP_CHANNELS = tuple(taps[b] for b in self.tap_blocks) + (top,)

    def preprocess(self, image):
        """Rescaling(1/255) and Normalization(axis=3) of the Keras model, applied to the [-1, 1] image as the reference does
        (efficientnet.preprocess_input is the identity)."""
        shape = (1, 3, 1, 1)
        return (image / 255.0 - self.norm_mean.view(shape).to(image.dtype)) / self.norm_variance.view(shape).to(image.dtype).sqrt()

    def stem(self, image):
        """stem_conv + stem_bn, pre-activation (its swish rides in block1a's depthwise loads)."""
        x = self.preprocess(image)
        if _conv.usable(x, self.stem_conv, 1.0):
            x = self.stem_matrix_core(x, self.stem_conv, 2)
        else:                                                         # host tensors / fp32: ZeroPadding2D(correct_pad) + valid
            x = F.conv2d(zero_pad(x, correct_pad(x.shape[2], x.shape[3], 3)), self.stem_conv.weight, None, 2)
        return self.stem_bn(x)

    def forward(self, image, physical_taps=False):
        self.check_image(image)
        x = self.stem(image)
        taps = []
        for k, block in enumerate(self.blocks):
            x, pre = block(x)
            if k in self.tap_blocks:
                taps.append(F.silu(pre))
        x = conv1x1_bn(x, self.top_conv.weight, self.top_bn)
        taps.append(F.silu(x))
        return taps


# ------------------------------------------------------------------------------------------ Keras weights
def keras_variable_map(encoder):
    """{keras variable name: (tensor of the encoder, kind)} with kind in {"conv", "depthwise", "vector"}
    (tf.keras.applications.efficientnet layer names; layouts as keras_weights._to_keras)."""
    out = {}
    bn = functools.partial(_kw.bn, out)

    out["normalization/mean"] = (encoder.norm_mean, "vector")
    out["normalization/variance"] = (encoder.norm_variance, "vector")
    out["normalization/count"] = (encoder.norm_count, "vector")
    out["stem_conv/kernel"] = (encoder.stem_conv.weight, "conv")
    bn("stem_bn", encoder.stem_bn)
    for block in encoder.blocks:
        prefix = block.name
        if block.expand is not None:
            out[f"{prefix}_expand_conv/kernel"] = (block.expand.weight, "conv")
            bn(f"{prefix}_expand_bn", block.expand_bn)
        out[f"{prefix}_dwconv/depthwise_kernel"] = (block.depthwise.weight, "depthwise")
        bn(f"{prefix}_bn", block.depthwise_bn)
        out[f"{prefix}_se_reduce/kernel"] = (block.se_reduce.weight, "conv")
        out[f"{prefix}_se_reduce/bias"] = (block.se_reduce.bias, "vector")
        out[f"{prefix}_se_expand/kernel"] = (block.se_expand.weight, "conv")
        out[f"{prefix}_se_expand/bias"] = (block.se_expand.bias, "vector")
        out[f"{prefix}_project_conv/kernel"] = (block.project.weight, "conv")
        bn(f"{prefix}_project_bn", block.project_bn)
    out["top_conv/kernel"] = (encoder.top_conv.weight, "conv")
    bn("top_bn", encoder.top_bn)
    return out


def export_keras_weights(encoder):
    """{keras variable name: float32 array in the keras layout} of the encoder's current weights."""
    return _kw.export_weights(keras_variable_map(encoder))


def load_keras_weights(encoder, weights):
    """Fills the encoder from Keras EfficientNetB<n>(include_top=False) variables (a path or a {name: array} dict).  Strict: a
    missing, unknown or mis-shaped variable raises; nothing is loaded partially."""
    return _kw.load_weights(keras_variable_map(encoder), weights, encoder.net_name)
