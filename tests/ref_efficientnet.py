"""TEST INFRASTRUCTURE ONLY: EfficientNet-B0 / B3 / B5 / B7 (include_top=False), written a second time.

The reference takes these encoders from `tf.keras.applications.EfficientNetB<n>` of tensorflow==2.4.1 (call site
model/build_model/pretrained_nets.py:11-117, taps model/build_model/scaled_layers.json "EfficientNetB0" ...).  This file restates
the PUBLISHED architecture (Tan & Le, "EfficientNet: Rethinking Model Scaling for Convolutional Neural Networks"; Keras layer
naming) in the framework's own conventions -- NHWC tensors, HWIO kernels, depthwise kernels [k, k, C, 1], weights addressed by
their Keras VARIABLE NAMES -- the way tests/ref_mobilenet_v2.py does for MobileNetV2, and shares no code with
xpt_mde_2021_amd/model/build_model/efficientnet.py:

  * `manifest(model)`: every Keras variable (name, shape) in layer-creation order -> tests/golden/efficientnet_b0_manifest.json;
  * `forward(weights, image, model)`: the five tapped activations with plain pad / conv2d calls;
  * `random_weights(seed, model)`: a full weight set with non-trivial BatchNorm statistics and squeeze-excite biases.
"""
import collections
import math

import torch
import torch.nn.functional as F

BN_EPS = 1e-3
TAP_NAMES = ("block2a_expand_activation", "block3a_expand_activation", "block4a_expand_activation", "block6a_expand_activation",
             "top_activation")
SCALING = {"B0": (1.0, 1.0), "B3": (1.2, 1.4), "B5": (1.6, 2.2), "B7": (2.0, 3.1)}        # width, depth coefficient
# DEFAULT_BLOCKS_ARGS: kernel_size, repeats, filters_in, filters_out, expand_ratio, strides (se_ratio 0.25, id_skip everywhere)
STAGES = (dict(kernel_size=3, repeats=1, filters_in=32, filters_out=16, expand_ratio=1, strides=1),
          dict(kernel_size=3, repeats=2, filters_in=16, filters_out=24, expand_ratio=6, strides=2),
          dict(kernel_size=5, repeats=2, filters_in=24, filters_out=40, expand_ratio=6, strides=2),
          dict(kernel_size=3, repeats=3, filters_in=40, filters_out=80, expand_ratio=6, strides=2),
          dict(kernel_size=5, repeats=3, filters_in=80, filters_out=112, expand_ratio=6, strides=1),
          dict(kernel_size=5, repeats=4, filters_in=112, filters_out=192, expand_ratio=6, strides=2),
          dict(kernel_size=3, repeats=1, filters_in=192, filters_out=320, expand_ratio=6, strides=1))


def correct_pad(size_hw, k):
    """imagenet_utils.correct_pad: explicit padding that makes a stride-2 VALID conv behave like SAME."""
    adjust = (1 - size_hw[0] % 2, 1 - size_hw[1] % 2)
    c = k // 2
    return (c - adjust[0], c), (c - adjust[1], c)


def scaled_width(filters, coefficient, divisor=8):
    filters = filters * coefficient
    rounded = max(divisor, int(filters + divisor / 2) // divisor * divisor)
    return int(rounded + divisor) if rounded < 0.9 * filters else int(rounded)


class _Graph:
    """RECORDS variable shapes (weights is None) or EVALUATES the network.  Tensors are NHWC."""

    def __init__(self, weights):
        self.weights = weights
        self.variables = collections.OrderedDict()
        self.taps = {}

    def var(self, name, shape):
        shape = tuple(int(s) for s in shape)
        if name in self.variables:
            raise ValueError(f"variable {name} declared twice")
        self.variables[name] = shape
        if self.weights is None:
            return torch.zeros(shape, dtype=torch.float64)
        w = torch.as_tensor(self.weights[name])
        if tuple(w.shape) != shape:
            raise ValueError(f"{name}: expected shape {shape}, got {tuple(w.shape)}")
        return w

    def conv2d(self, x, filters, k, stride, name, bias=False):
        """Conv2D; padding "same" at stride 1, "valid" (on an explicitly padded input) at stride 2."""
        w = self.var(f"{name}/kernel", (k, k, x.shape[-1], filters)).to(x.dtype)
        b = self.var(f"{name}/bias", (filters,)).to(x.dtype) if bias else None
        if stride == 1:
            x = F.pad(x, (0, 0, k // 2, k // 2, k // 2, k // 2))
        y = F.conv2d(x.permute(0, 3, 1, 2), w.permute(3, 2, 0, 1), stride=stride).permute(0, 2, 3, 1)
        return y if b is None else y + b

    def depthwise(self, x, k, stride, name):
        c = x.shape[-1]
        w = self.var(f"{name}/depthwise_kernel", (k, k, c, 1)).to(x.dtype)
        if stride == 1:
            x = F.pad(x, (0, 0, k // 2, k // 2, k // 2, k // 2))
        return F.conv2d(x.permute(0, 3, 1, 2), w.permute(2, 3, 0, 1), stride=stride, groups=c).permute(0, 2, 3, 1)

    def batchnorm(self, x, name):
        c = x.shape[-1]
        gamma, beta = self.var(f"{name}/gamma", (c,)).to(x.dtype), self.var(f"{name}/beta", (c,)).to(x.dtype)
        mean = self.var(f"{name}/moving_mean", (c,)).to(x.dtype)
        variance = self.var(f"{name}/moving_variance", (c,)).to(x.dtype)
        return (x - mean) / torch.sqrt(variance + BN_EPS) * gamma + beta

    def swish(self, x, name):
        y = x * torch.sigmoid(x)
        if name in TAP_NAMES:
            self.taps[name] = y
        return y

    def zero_pad(self, x, pad_hw):
        (pt, pb), (pl, pr) = pad_hw
        return F.pad(x, (0, 0, pl, pr, pt, pb))

    def block(self, inputs, name, kernel_size, filters_in, filters_out, expand_ratio, strides):
        filters = filters_in * expand_ratio
        x = inputs
        if expand_ratio != 1:
            x = self.conv2d(x, filters, 1, 1, name + "expand_conv")
            x = self.batchnorm(x, name + "expand_bn")
            x = self.swish(x, name + "expand_activation")
        if strides == 2:
            x = self.zero_pad(x, correct_pad(x.shape[1:3], kernel_size))
        x = self.depthwise(x, kernel_size, strides, name + "dwconv")
        x = self.batchnorm(x, name + "bn")
        x = self.swish(x, name + "activation")
        filters_se = max(1, int(filters_in * 0.25))
        se = x.mean(dim=(1, 2), keepdim=True)                                   # se_squeeze + se_reshape
        se = self.swish(self.conv2d(se, filters_se, 1, 1, name + "se_reduce", bias=True), name + "se_reduce_activation")
        se = torch.sigmoid(self.conv2d(se, filters, 1, 1, name + "se_expand", bias=True))
        x = x * se                                                              # se_excite
        x = self.conv2d(x, filters_out, 1, 1, name + "project_conv")
        x = self.batchnorm(x, name + "project_bn")
        if strides == 1 and filters_in == filters_out:
            x = x + inputs                                                      # (drop: identity outside training)
        return x

    def network(self, image, model):
        """image NHWC, as DepthNetPretrained hands it over ([-1, 1]); efficientnet.preprocess_input is the identity, the model's
        own Rescaling and Normalization layers follow."""
        width, depth = SCALING[model]
        x = image * (1.0 / 255.0)
        mean = self.var("normalization/mean", (3,)).to(x.dtype)
        variance = self.var("normalization/variance", (3,)).to(x.dtype)
        self.var("normalization/count", ())
        x = (x - mean) / torch.sqrt(variance)
        x = self.zero_pad(x, correct_pad(x.shape[1:3], 3))
        x = self.conv2d(x, scaled_width(32, width), 3, 2, "stem_conv")
        x = self.batchnorm(x, "stem_bn")
        x = self.swish(x, "stem_activation")
        for i, stage in enumerate(STAGES):
            args = dict(stage)
            repeats = int(math.ceil(depth * args.pop("repeats")))
            args["filters_in"] = scaled_width(args["filters_in"], width)
            args["filters_out"] = scaled_width(args["filters_out"], width)
            for j in range(repeats):
                if j > 0:
                    args["strides"] = 1
                    args["filters_in"] = args["filters_out"]
                x = self.block(x, f"block{i + 1}{chr(j + 97)}_", **args)
        x = self.conv2d(x, scaled_width(1280, width), 1, 1, "top_conv")
        x = self.batchnorm(x, "top_bn")
        x = self.swish(x, "top_activation")
        return [self.taps[name] for name in TAP_NAMES]


def manifest(model="B0"):
    """OrderedDict {keras variable name: shape} of EfficientNet<model>(include_top=False), layer-creation order."""
    g = _Graph(None)
    g.network(torch.zeros(1, 32, 32, 3, dtype=torch.float64), model)
    return g.variables


def forward(weights, image_nhwc, model="B0"):
    """The five taps (NHWC) for an image batch [B,H,W,3]; computed in the image's dtype."""
    return _Graph(weights).network(image_nhwc, model)


def random_weights(seed=0, model="B0", dtype=torch.float64):
    """Kernels of variance 1 / fan_in (depthwise 2 / k k) with BatchNorm gammas in [1, 1.4]: the five taps keep a spread of
    0.4 - 0.8 through the 16 blocks (He scaling grows a thousandfold here: half the 1x1 convolutions read un-activated tensors).
    BatchNorm statistics away from the identity, squeeze-excite biases of order one (gates spread over (0, 1)), and an ADAPTED
    normalization layer (mean / variance of the order of the rescaled image, so a wrong formula there cannot pass)."""
    g = torch.Generator().manual_seed(seed)
    out = {}
    for name, shape in manifest(model).items():
        if name == "normalization/mean":
            out[name] = 0.002 * torch.randn(shape, generator=g, dtype=dtype)
        elif name == "normalization/variance":
            out[name] = (0.002 + 0.002 * torch.rand(shape, generator=g, dtype=dtype)) ** 2
        elif name == "normalization/count":
            out[name] = torch.tensor(1000.0, dtype=dtype)
        elif name.endswith("/kernel"):
            fan_in = shape[0] * shape[1] * shape[2]
            out[name] = torch.randn(shape, generator=g, dtype=dtype) * (1.0 / fan_in) ** 0.5
        elif name.endswith("/depthwise_kernel"):
            out[name] = torch.randn(shape, generator=g, dtype=dtype) * (2.0 / (shape[0] * shape[1])) ** 0.5
        elif name.endswith("/bias"):
            out[name] = torch.randn(shape, generator=g, dtype=dtype)
        elif name.endswith("/gamma"):
            out[name] = 1.0 + 0.4 * torch.rand(shape, generator=g, dtype=dtype)
        elif name.endswith("/moving_variance"):
            out[name] = 0.5 + torch.rand(shape, generator=g, dtype=dtype)
        else:                                           # beta, moving_mean
            out[name] = 0.2 * torch.randn(shape, generator=g, dtype=dtype)
    return out
