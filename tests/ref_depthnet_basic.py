"""fp64 restatement of DepthNetBasic / DepthNetNoResize (reference: model/build_model/depth_net.py:10-109), written from the
Keras layer semantics in NHWC / HWIO with the Keras layer names -- independent of the package under test: it imports nothing
from it and evaluates the bilinear resize with its own index arithmetic instead of a framework call.

Layers (CustomConv2D: Conv2D(padding="same") + LeakyReLU(0.1), linear on the prediction heads):
  encoder  dp_conv0b 7x7/1 32, dp_conv1a 7x7/2 32, dp_conv1b 5x5/1 64, dp_conv2a 5x5/2 64, dp_conv2b 3x3/1 128, dp_conv3a /2 128,
           dp_conv3b 256, dp_conv4a /2 256, dp_conv4b 512, dp_conv5a /2 512, dp_conv5b 512, dp_conv6a /2 512, dp_conv6b 512,
           dp_conv7a /2 512
  decoder  dp_up<n>_conv1 (on the 2x up-sampled previous level), [resize to the skip's extent], concat with the skip (and the
           up-sampled previous prediction), dp_up<n>_conv2; n = 6 .. 0
  heads    dp_depth<n>_conv 3x3 -> 1 linear channel on up3 .. up0, the depth activation on it, and the prediction resized
           (tf.image.resize bilinear, half-pixel centres) to the next level's extent."""
import math

import torch
import torch.nn.functional as F

ENCODER = [("dp_conv0b", 7, 1, 32), ("dp_conv1a", 7, 2, 32), ("dp_conv1b", 5, 1, 64), ("dp_conv2a", 5, 2, 64),
           ("dp_conv2b", 3, 1, 128), ("dp_conv3a", 3, 2, 128), ("dp_conv3b", 3, 1, 256), ("dp_conv4a", 3, 2, 256),
           ("dp_conv4b", 3, 1, 512), ("dp_conv5a", 3, 2, 512), ("dp_conv5b", 3, 1, 512), ("dp_conv6a", 3, 2, 512),
           ("dp_conv6b", 3, 1, 512), ("dp_conv7a", 3, 2, 512)]
# (level, channels of the previous level, channels of the skip [+ 1 prediction], output channels)
DECODER = [(6, 512, 512, 512), (5, 512, 512, 512), (4, 512, 512, 256), (3, 256, 256, 128), (2, 128, 128 + 1, 64),
           (1, 64, 64 + 1, 32), (0, 32, 1, 16)]
HEADS = [(3, 128), (2, 64), (1, 32), (0, 16)]


def layer_table():
    """[(layer name, k, cin, cout)] in the reference's order of construction."""
    table, cin = [], 3
    for name, k, _, cout in ENCODER:
        table.append((name, k, cin, cout))
        cin = cout
    heads = dict(HEADS)
    for lvl, prev, skip, cout in DECODER:
        table.append((f"dp_up{lvl}_conv1", 3, prev, cout))
        table.append((f"dp_up{lvl}_conv2", 3, cout + skip, cout))
        if lvl in heads:
            table.append((f"dp_depth{lvl}_conv", 3, heads[lvl], 1))
    return table


def random_weights(seed, bias_scale=0.05):
    """{"<layer>/kernel": HWIO fp64, "<layer>/bias": [O] fp64}; He-scaled kernels keep the activations of order one."""
    g = torch.Generator().manual_seed(seed)
    out = {}
    for name, k, cin, cout in layer_table():
        out[name + "/kernel"] = torch.randn(k, k, cin, cout, generator=g, dtype=torch.float64) * math.sqrt(2.0 / (k * k * cin))
        out[name + "/bias"] = torch.randn(cout, generator=g, dtype=torch.float64) * bias_scale
    return out


def assign(layers, weights):
    """Copy the HWIO / [O] variables into {layer name: module with .conv.weight [O,I,H,W] and .conv.bias}; strict both ways."""
    assert {n + s for n in layers for s in ("/kernel", "/bias")} == set(weights)
    with torch.no_grad():
        for name, layer in layers.items():
            layer.conv.weight.copy_(weights[name + "/kernel"].permute(3, 2, 0, 1))
            layer.conv.bias.copy_(weights[name + "/bias"])


def same_padding(n, k, s):
    out = -(-n // s)
    total = max((out - 1) * s + k - n, 0)
    return total // 2, total - total // 2


def conv2d(w, x, name, stride=1, slope=0.1):
    """Keras Conv2D(padding="same") + LeakyReLU(slope) (slope 1: linear) on NHWC x."""
    kernel, bias = w[name + "/kernel"], w[name + "/bias"]
    k = kernel.shape[0]
    (pt, pb), (pl, pr) = same_padding(x.shape[1], k, stride), same_padding(x.shape[2], k, stride)
    xp = F.pad(x.permute(0, 3, 1, 2), (pl, pr, pt, pb))
    y = F.conv2d(xp, kernel.permute(3, 2, 0, 1).contiguous(), bias, stride).permute(0, 2, 3, 1)
    return torch.where(y > 0, y, y * slope)


def _axis_taps(n_in, n_out):
    """tf.image.resize bilinear, half-pixel centres: source = (dst + 0.5) * in / out - 0.5; lower = max(floor, 0),
    upper = min(ceil, in - 1), weight of `upper` = source - floor(source)."""
    src = (torch.arange(n_out, dtype=torch.float64) + 0.5) * (n_in / n_out) - 0.5
    lo = torch.floor(src)
    frac = src - lo
    upper = torch.ceil(src).clamp(max=n_in - 1).long()
    lower = lo.clamp(min=0).long()
    return lower, upper, frac


def resize_bilinear(x, oh, ow):
    """NHWC x -> [B, oh, ow, C]; the identity when the extents match (layer_ops.py:43-50)."""
    if x.shape[1] == oh and x.shape[2] == ow:
        return x
    lo, up, f = _axis_taps(x.shape[1], oh)
    x = x[:, lo] * (1 - f).view(1, -1, 1, 1) + x[:, up] * f.view(1, -1, 1, 1)
    lo, up, f = _axis_taps(x.shape[2], ow)
    return x[:, :, lo] * (1 - f).view(1, 1, -1, 1) + x[:, :, up] * f.view(1, 1, -1, 1)


def upsample2x(x, interp):
    """UpSampling2D(size=2, interpolation=interp)."""
    if interp == "nearest":
        return x.repeat_interleave(2, dim=1).repeat_interleave(2, dim=2)
    assert interp == "bilinear"
    return resize_bilinear(x, 2 * x.shape[1], 2 * x.shape[2])


def inverse_sigmoid(x):
    return 1.0 / (torch.sigmoid(x) + 0.01)


def exponential(x):
    return torch.exp(torch.sigmoid(x + 1.0) * 10.0 - 5.0)


def forward(w, image5d, resize=True, interp="nearest", activation=inverse_sigmoid, slope=0.1):
    """image5d [B,S,H,W,3] fp64 in [-1, 1] -> dict(depth_ms=[d0, d1, d2, d3] NHWC, debug_out=[upconv0, upconv3] NHWC,
    encoder_extents=[(h, w) of conv1 .. conv7], resized={level: did resize_like change the extent})."""
    x = image5d[:, -1]
    height, width = x.shape[1:3]
    feats = {}
    for name, _, stride, _ in ENCODER:
        x = conv2d(w, x, name, stride, slope)
        feats[name] = x
    skips = [feats[n] for n in ("dp_conv1b", "dp_conv2b", "dp_conv3b", "dp_conv4b", "dp_conv5b", "dp_conv6b", "dp_conv7a")]
    conv1, conv2, conv3, conv4, conv5, conv6, conv7 = skips
    resized = {}

    def upconv(bef, skip, lvl, pred=None):
        up = conv2d(w, upsample2x(bef, interp), f"dp_up{lvl}_conv1", 1, slope)
        if resize:
            resized[lvl] = tuple(up.shape[1:3]) != tuple(skip.shape[1:3])
            up = resize_bilinear(up, skip.shape[1], skip.shape[2])
        parts = [up, skip] if pred is None else [up, skip, pred]
        return conv2d(w, torch.cat(parts, dim=3), f"dp_up{lvl}_conv2", 1, slope)

    def head(src, lvl, dst_h, dst_w):
        pred = conv2d(w, src, f"dp_depth{lvl}_conv", 1, 1.0)
        return activation(pred), resize_bilinear(pred, dst_h, dst_w)

    up6 = upconv(conv7, conv6, 6)
    up5 = upconv(up6, conv5, 5)
    up4 = upconv(up5, conv4, 4)
    up3 = upconv(up4, conv3, 3)
    depth3, pred2_up = head(up3, 3, height // 4, width // 4)
    up2 = upconv(up3, conv2, 2, pred2_up)
    depth2, pred1_up = head(up2, 2, height // 2, width // 2)
    up1 = upconv(up2, conv1, 1, pred1_up)
    depth1, pred0_up = head(up1, 1, height, width)
    up0 = upconv(up1, pred0_up, 0)
    depth0, _ = head(up0, 0, height, width)
    return dict(depth_ms=[depth0, depth1, depth2, depth3], debug_out=[up0, up3],
                encoder_extents=[tuple(t.shape[1:3]) for t in skips], resized=resized)
