"""TEST INFRASTRUCTURE ONLY: ResNet50V2 (include_top=False), written a second time.

The reference takes this encoder from `tf.keras.applications.ResNet50V2` of tensorflow==2.4.1 (call site
model/build_model/pretrained_nets.py:31-101, taps model/build_model/scaled_layers.json "ResNet50V2").  This file restates the
PUBLISHED architecture (He et al., "Identity Mappings in Deep Residual Networks"; Keras layer naming) in the framework's own
conventions -- NHWC tensors, HWIO kernels, weights addressed by their Keras VARIABLE NAMES -- the way tests/ref_mobilenet_v2.py does
for MobileNetV2, and shares no code with xpt_mde_2021_amd/model/build_model/resnet_v2.py:

  * `manifest()`: every Keras variable (name, shape), in layer order -> tests/golden/resnet50v2_manifest.json;
  * `layers()`: the layer names in the order of Keras' `model.layers` (what scaled_layers.json indexes: a block's shortcut layer
    -- `_0_conv` or the unnamed MaxPooling2D(1) -- sorts BEHIND its main branch, directly before `_3_conv`);
  * `forward(weights, image)`: the five tapped activations with plain pad / conv2d calls;
  * `random_weights(seed)`: a full weight set with non-trivial BatchNorm statistics.

Pooling tie rule (pool1_pool; shared with the kernels' header): the FIRST maximal tap in row-major window order takes the gradient;
the zero padding of pool1_pad is a candidate like any other (and passes no gradient when it wins).
"""
import collections

import torch
import torch.nn.functional as F

BN_EPS = 1.001e-5                 # BatchNormalization(epsilon=1.001e-5) everywhere in keras resnet_v2
TAP_NAMES = ("conv1_conv", "conv2_block3_1_relu", "conv3_block4_1_relu", "conv4_block6_1_relu", "post_relu")
TAP_LAYER_INDICES = (2, 32, 78, 146, 189)                       # scaled_layers.json "ResNet50V2"
# (filters, blocks, stride1, name) of ResNet50V2's stack_fn
STACK_ARGS = ((64, 3, 2, "conv2"), (128, 4, 2, "conv3"), (256, 6, 2, "conv4"), (512, 3, 1, "conv5"))
IMAGENET_MEAN_BGR = (103.939, 116.779, 123.68)


class _Graph:
    """RECORDS variable shapes and layer names (weights is None) or EVALUATES the network.  Tensors are NHWC."""

    def __init__(self, weights):
        self.weights = weights
        self.variables = collections.OrderedDict()
        self.layer_names = []
        self.shapes = {}
        self.taps = {}

    def layer(self, name, y):
        self.layer_names.append(name)
        self.shapes[name] = tuple(y.shape)
        if name in TAP_NAMES:
            self.taps[name] = y
        return y

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

    def conv2d(self, x, filters, k, stride, name, use_bias):
        """Conv2D(padding="valid"): every padded convolution of resnet_v2 has its own ZeroPadding2D layer in front."""
        w = self.var(f"{name}/kernel", (k, k, x.shape[-1], filters)).to(x.dtype)
        b = self.var(f"{name}/bias", (filters,)).to(x.dtype) if use_bias else None
        y = F.conv2d(x.permute(0, 3, 1, 2), w.permute(3, 2, 0, 1), b, stride=stride).permute(0, 2, 3, 1)
        return self.layer(name, y)

    def batchnorm(self, x, name):
        c = x.shape[-1]
        gamma, beta = self.var(f"{name}/gamma", (c,)).to(x.dtype), self.var(f"{name}/beta", (c,)).to(x.dtype)
        mean = self.var(f"{name}/moving_mean", (c,)).to(x.dtype)
        variance = self.var(f"{name}/moving_variance", (c,)).to(x.dtype)
        return self.layer(name, (x - mean) / torch.sqrt(variance + BN_EPS) * gamma + beta)

    def relu(self, x, name):
        return self.layer(name, torch.clamp(x, min=0.0))

    def zero_pad(self, x, p, name):
        return self.layer(name, F.pad(x, (0, 0, p, p, p, p)))

    def max_pool(self, x, k, stride, name):
        """MaxPooling2D(k, strides=stride), valid.  The first maximal tap of a window (row-major) takes the whole gradient."""
        win = x.unfold(1, k, stride).unfold(2, k, stride)                  # [B, OH, OW, C, k, k]
        win = win.reshape(*win.shape[:4], k * k)
        top = win.amax(dim=-1, keepdim=True)
        hit = (win == top)
        earlier = torch.cumsum(hit.to(torch.int64), dim=-1) - hit.to(torch.int64)
        pick = hit & (earlier == 0)
        return self.layer(name, torch.where(pick, win, torch.zeros_like(win)).sum(-1))

    def block2(self, x, filters, stride, conv_shortcut, name):
        preact = self.batchnorm(x, name + "_preact_bn")
        preact = self.relu(preact, name + "_preact_relu")
        h = self.conv2d(preact, filters, 1, 1, name + "_1_conv", use_bias=False)
        h = self.batchnorm(h, name + "_1_bn")
        h = self.relu(h, name + "_1_relu")
        h = self.zero_pad(h, 1, name + "_2_pad")
        h = self.conv2d(h, filters, 3, stride, name + "_2_conv", use_bias=False)
        h = self.batchnorm(h, name + "_2_bn")
        h = self.relu(h, name + "_2_relu")
        if conv_shortcut:
            shortcut = self.conv2d(preact, 4 * filters, 1, stride, name + "_0_conv", use_bias=True)
        elif stride > 1:
            shortcut = self.max_pool(x, 1, stride, f"max_pooling2d@{name}")
        else:
            shortcut = x
        h = self.conv2d(h, 4 * filters, 1, 1, name + "_3_conv", use_bias=True)
        return self.layer(name + "_out", shortcut + h)

    def network(self, image):
        """image NHWC RGB, as DepthNetPretrained hands it over ([-1, 1]); applications.resnet.preprocess_input (caffe mode: BGR,
        minus the ImageNet channel means, no scaling) is applied to it as the reference does (bug-compatible)."""
        self.layer("input_1", image)
        x = image[..., [2, 1, 0]] - torch.tensor(IMAGENET_MEAN_BGR, dtype=image.dtype)
        x = self.zero_pad(x, 3, "conv1_pad")
        x = self.conv2d(x, 64, 7, 2, "conv1_conv", use_bias=True)
        x = self.zero_pad(x, 1, "pool1_pad")
        x = self.max_pool(x, 3, 2, "pool1_pool")
        for filters, blocks, stride1, name in STACK_ARGS:
            x = self.block2(x, filters, 1, True, f"{name}_block1")
            for i in range(2, blocks):
                x = self.block2(x, filters, 1, False, f"{name}_block{i}")
            x = self.block2(x, filters, stride1, False, f"{name}_block{blocks}")
        x = self.batchnorm(x, "post_bn")
        x = self.relu(x, "post_relu")
        return [self.taps[name] for name in TAP_NAMES]


def _recorded(h=32, w=32):
    g = _Graph(None)
    g.network(torch.zeros(1, h, w, 3, dtype=torch.float64))
    return g


def manifest():
    """OrderedDict {keras variable name: shape} of ResNet50V2(include_top=False), layer order."""
    return _recorded().variables


def layers(h=32, w=32):
    """[(layer name, output shape NHWC)] in the order of Keras' model.layers for an h x w image."""
    g = _recorded(h, w)
    return [(name, g.shapes[name]) for name in g.layer_names]


def forward(weights, image_nhwc):
    """The five taps (NHWC) for an image batch [B,H,W,3]; computed in the image's dtype."""
    return _Graph(weights).network(image_nhwc)


def random_weights(seed=0, dtype=torch.float64):
    """He-scaled kernels; the last convolution of every block at a quarter of that, so that 16 residual additions keep the
    activations' scale; BatchNorm statistics away from the identity; biases of order 0.1.  The stem kernel is drawn with zero
    mean over its window per (input, output) channel pair so that the -104 ... -124 offset of the caffe preprocessing does not
    swamp the image's own contribution."""
    g = torch.Generator().manual_seed(seed)
    out = {}
    for name, shape in manifest().items():
        if name.endswith("/kernel"):
            fan_in = shape[0] * shape[1] * shape[2]
            w = torch.randn(shape, generator=g, dtype=dtype) * (2.0 / fan_in) ** 0.5
            if name == "conv1_conv/kernel":
                w = (w - w.mean(dim=(0, 1), keepdim=True)) * 8.0
            if name.endswith("_3_conv/kernel"):
                w = w * 0.25
            out[name] = w
        elif name.endswith("/gamma"):
            out[name] = 0.8 + 0.4 * torch.rand(shape, generator=g, dtype=dtype)
        elif name.endswith("/moving_variance"):
            out[name] = 0.5 + torch.rand(shape, generator=g, dtype=dtype)
        elif name.endswith("/bias"):
            out[name] = 0.1 * torch.randn(shape, generator=g, dtype=dtype)
        else:                                           # beta, moving_mean
            out[name] = 0.2 * torch.randn(shape, generator=g, dtype=dtype)
    return out
