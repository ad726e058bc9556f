"""TEST INFRASTRUCTURE ONLY: MobileNetV2 (alpha = 1.0, include_top=False), written a second time.

The reference takes this encoder from `tf.keras.applications.MobileNetV2` of tensorflow==2.4.1 (call site
model/build_model/pretrained_nets.py:31-34, taps model/build_model/scaled_layers.json "MobileNetV2").  This file restates the
PUBLISHED architecture (Sandler et al., "MobileNetV2: Inverted Residuals and Linear Bottlenecks"; Keras layer naming) in the
framework's own conventions -- NHWC tensors, HWIO kernels, depthwise kernels [3, 3, C, 1], weights addressed by their Keras
VARIABLE NAMES -- the way oracle/ref_nasnet.py does for NASNet, and shares no code with
xpt_mde_2021_amd/model/build_model/mobilenet_v2.py:

  * `manifest()`: every Keras variable (name, shape) in layer-creation order -> tests/golden/mobilenet_v2_manifest.json;
  * `forward(weights, image)`: the five tapped activations with plain pad / conv2d calls;
  * `random_weights(seed)`: a full weight set with non-trivial BatchNorm statistics.
"""
import collections

import torch
import torch.nn.functional as F

BN_EPS = 1e-3                    # BatchNormalization(epsilon=1e-3, momentum=0.999) everywhere in keras mobilenet_v2
TAP_NAMES = ("block_1_expand_relu", "block_3_expand_relu", "block_6_expand_relu", "block_13_expand_relu", "out_relu")
# (expansion t, output channels c, repeats n, first stride s) of the paper's table 2, alpha = 1.0
BOTTLENECKS = ((1, 16, 1, 1), (6, 24, 2, 2), (6, 32, 3, 2), (6, 64, 4, 2), (6, 96, 3, 1), (6, 160, 3, 2), (6, 320, 1, 1))


def correct_pad(size_hw, k):
    """imagenet_utils.correct_pad: explicit padding that makes a stride-2 VALID conv behave like SAME."""
    adjust = (1 - size_hw[0] % 2, 1 - size_hw[1] % 2)
    c = k // 2
    return (c - adjust[0], c), (c - adjust[1], c)


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

    def conv2d(self, x, filters, k, stride, name):
        """Conv2D(use_bias=False); padding "same" at stride 1, "valid" (on an explicitly padded input) at stride 2."""
        w = self.var(f"{name}/kernel", (k, k, x.shape[-1], filters)).to(x.dtype)
        if stride == 1:
            x = F.pad(x, (0, 0, k // 2, k // 2, k // 2, k // 2))
        return F.conv2d(x.permute(0, 3, 1, 2), w.permute(3, 2, 0, 1), stride=stride).permute(0, 2, 3, 1)

    def depthwise(self, x, stride, name):
        c = x.shape[-1]
        w = self.var(f"{name}/depthwise_kernel", (3, 3, c, 1)).to(x.dtype)
        if stride == 1:
            x = F.pad(x, (0, 0, 1, 1, 1, 1))
        return F.conv2d(x.permute(0, 3, 1, 2), w.permute(2, 3, 0, 1), stride=stride, groups=c).permute(0, 2, 3, 1)

    def batchnorm(self, x, name):
        c = x.shape[-1]
        gamma, beta = self.var(f"{name}/gamma", (c,)).to(x.dtype), self.var(f"{name}/beta", (c,)).to(x.dtype)
        mean = self.var(f"{name}/moving_mean", (c,)).to(x.dtype)
        variance = self.var(f"{name}/moving_variance", (c,)).to(x.dtype)
        return (x - mean) / torch.sqrt(variance + BN_EPS) * gamma + beta

    def relu6(self, x, name):
        y = torch.clamp(x, 0.0, 6.0)
        if name in TAP_NAMES:
            self.taps[name] = y
        return y

    def zero_pad(self, x, pad_hw):
        (pt, pb), (pl, pr) = pad_hw
        return F.pad(x, (0, 0, pl, pr, pt, pb))

    def inverted_res_block(self, x, expansion, stride, filters, block_id):
        inputs, cin = x, x.shape[-1]
        prefix = f"block_{block_id}_" if block_id else "expanded_conv_"
        if block_id:
            x = self.conv2d(x, expansion * cin, 1, 1, prefix + "expand")
            x = self.batchnorm(x, prefix + "expand_BN")
            x = self.relu6(x, prefix + "expand_relu")
        if stride == 2:
            x = self.zero_pad(x, correct_pad(x.shape[1:3], 3))
        x = self.depthwise(x, stride, prefix + "depthwise")
        x = self.batchnorm(x, prefix + "depthwise_BN")
        x = self.relu6(x, prefix + "depthwise_relu")
        x = self.conv2d(x, filters, 1, 1, prefix + "project")
        x = self.batchnorm(x, prefix + "project_BN")
        return inputs + x if (cin == filters and stride == 1) else x

    def network(self, image):
        """image NHWC, as DepthNetPretrained hands it over ([-1, 1]); preprocess_input is applied once more (bug-compatible)."""
        x = image / 127.5 - 1.0
        x = self.zero_pad(x, correct_pad(x.shape[1:3], 3))
        x = self.conv2d(x, 32, 3, 2, "Conv1")
        x = self.batchnorm(x, "bn_Conv1")
        x = self.relu6(x, "Conv1_relu")
        block_id = 0
        for t, c, n, s in BOTTLENECKS:
            for i in range(n):
                x = self.inverted_res_block(x, t, s if i == 0 else 1, c, block_id)
                block_id += 1
        x = self.conv2d(x, 1280, 1, 1, "Conv_1")
        x = self.batchnorm(x, "Conv_1_bn")
        x = self.relu6(x, "out_relu")
        return [self.taps[name] for name in TAP_NAMES]


def manifest():
    """OrderedDict {keras variable name: shape} of MobileNetV2(include_top=False), layer-creation order."""
    g = _Graph(None)
    g.network(torch.zeros(1, 32, 32, 3, dtype=torch.float64))
    return g.variables


def forward(weights, image_nhwc):
    """The five taps (NHWC) for an image batch [B,H,W,3]; computed in the image's dtype."""
    return _Graph(weights).network(image_nhwc)


def random_weights(seed=0, dtype=torch.float64):
    """He-scaled kernels (so that activations keep their scale through 53 layers and both ReLU6 clamps act), BatchNorm
    statistics away from the identity."""
    g = torch.Generator().manual_seed(seed)
    out = {}
    for name, shape in manifest().items():
        if name.endswith("/kernel"):
            fan_in = shape[0] * shape[1] * shape[2]
            out[name] = torch.randn(shape, generator=g, dtype=dtype) * (2.0 / fan_in) ** 0.5
        elif name.endswith("/depthwise_kernel"):
            out[name] = torch.randn(shape, generator=g, dtype=dtype) * (2.0 / 9.0) ** 0.5
        elif name.endswith("/gamma"):
            out[name] = 0.8 + 0.4 * torch.rand(shape, generator=g, dtype=dtype)
        elif name.endswith("/moving_variance"):
            out[name] = 0.5 + torch.rand(shape, generator=g, dtype=dtype)
        else:                                           # beta, moving_mean
            out[name] = 0.2 * torch.randn(shape, generator=g, dtype=dtype)
    return out
