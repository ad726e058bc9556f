"""DepthNetPretrained: multi-scale encoder + the reference's U-Net style decoder
(model/build_model/depth_net.py:76-92 upsample / get_scaled_depth, :101-109 NoResize skip block, :137-167 decode);
DepthNetBasic / DepthNetNoResize: the SfMLearner-style encoder-decoder without a backbone (:10-109).
"""
import torch
import torch.nn as nn
from ...hip.lib import half as _half      # torch dtype of the 16-bit activations (bf16 | fp16 build of the library)

import torch.nn.functional as F

from ...hip import conv as _conv
from ...hip import ops as _ops
from ..model_util import layer_ops as lo
from ...utils.util_class import WrongInputException
from .pretrained_nets import PretrainedModel


_BATCHED_HEADS = __import__("os").environ.get("XPT_DEBUG_PER_SCALE_LOSS", "0") != "1"     # A/B: one activation launch per scale


class _ChannelsLastOne(torch.autograd.Function):
    """[B,1,H,W] contiguous -> the same memory with channels_last strides (a view); the gradient passes through as it
    comes (as_strided's own backward would materialise it with a zero fill and a copy)."""

    @staticmethod
    def forward(ctx, x):
        return x.as_strided(x.shape, (x.shape[2] * x.shape[3], 1, x.shape[3], 1))

    @staticmethod
    def backward(ctx, g):
        return g


_FUSED_CONCAT = __import__("os").environ.get("XPT_DEBUG_TORCH_CAT", "0") != "1"     # A/B: torch.cat + cached zero pad
_FUSED_FAN_IN = __import__("os").environ.get("XPT_DEBUG_ATEN_FAN_IN", "0") != "1"    # A/B: autograd's add launches for the decoder's fan-ins
_FUSED_BILINEAR = __import__("os").environ.get("XPT_DEBUG_ATEN_BILINEAR", "0") != "1"  # A/B: F.interpolate in front of conv1 ("bilinear")


class UpconvWithSkip(nn.Module):
    """upconv_with_skip_connection of DepthNetNoResize (depth_net.py:101-109):
    2x up-sampling (nearest | bilinear) -> conv3x3 -> concat([., skip][, up-sampled previous prediction]) -> conv3x3.
    resize=True: DepthNetBasic's block (depth_net.py:76-85), which resizes the first convolution's output to the skip's extent
    (lo.resize_like) in front of the concatenation -- the identity wherever the encoder halved an even extent."""

    def __init__(self, conv2d, cin, skip_channels, out_channels, upsample_interp="nearest", resize=False):
        super().__init__()
        self.interp = upsample_interp
        self.resize = resize
        self.conv1 = conv2d(cin, out_channels, 3)
        self.conv2 = conv2d(out_channels + skip_channels, out_channels, 3)

    def forward(self, bef_layer, skips):
        if self.interp == "nearest":
            up = self.conv1(bef_layer, upsample=True)                             # UpSampling2D(2, "nearest") fused into the conv
        elif (_FUSED_BILINEAR and bef_layer.is_cuda and bef_layer.dtype == _half()
              and _conv.usable(bef_layer, self.conv1.conv, self.conv1.slope) and self._fused_bilinear_wins(bef_layer)):
            up = self.conv1(bef_layer, upsample="bilinear")                       # UpSampling2D(2, "bilinear") as the conv's operand load
        else:                                                                     # host tensors, fp32 / fp64: the framework's resize
            up = self.conv1(F.interpolate(bef_layer, scale_factor=2, mode="bilinear", align_corners=False))
        if self.resize:
            up = lo.resize_like(up, skips[0])
        parts = [up] + [s.to(up.dtype) for s in skips]
        if up.is_cuda and up.dtype == _half() and len(parts) <= 4 and _FUSED_CONCAT:
            # the concatenation and its zero pad channels in one launch (torch.cat's batched copy ran at 0.5 - 0.8 TB/s here)
            return self.conv2(_ops.concat_channels(parts))
        if up.is_cuda:
            # a one-channel map is "contiguous" in both layouts; give it channels_last strides explicitly, or torch.cat
            # sees mixed layouts, answers in NCHW and the convolution below pays a full re-layout copy of the concatenation
            parts = [_ChannelsLastOne.apply(p) if p.shape[1] == 1 and p.is_contiguous() else p for p in parts]
        total = sum(p.shape[1] for p in parts)
        if up.is_cuda and up.dtype == _half() and total % 8:
            # the matrix-core convolution reads 8-channel groups: the concatenation is built with its zero pad channels
            parts.append(self._zeros(up, -total % 8))
        return self.conv2(torch.cat(parts, dim=1))

    @staticmethod
    def _fused_bilinear_wins(x):
        """Measured per layer (tools/bench_conv.py --upsample bilinear, batch 8): the fused mode wins on
        up3 .. up0 (2 - 10x) and loses on up4.conv1 at the bench shape (1,056 -> 256 on 8 x 26: 270 against 227 us -- the
        halo-tile forward walks 33 channel chunks of one round trip each), so a layer that deep AND that large keeps the
        framework's resize; the small maps of the unit-test shapes stay fused."""
        return x.shape[1] <= 256 or x.shape[0] * 4 * x.shape[2] * x.shape[3] < 1024

    def _zeros(self, like, channels):
        key = (like.shape[0], channels, like.shape[2], like.shape[3], like.device)
        cache = self.__dict__.setdefault("_zero_cache", {})
        if key not in cache:                       # allocated by the first eager step, reused (also by captured steps)
            cache[key] = torch.zeros((like.shape[0], channels, like.shape[2], like.shape[3]), dtype=like.dtype,
                                     device=like.device).contiguous(memory_format=torch.channels_last)
        return cache[key]


class ScaledDepthHead(nn.Module):
    """get_scaled_depth (depth_net.py:87-92): 3x3 conv to one LINEAR channel, the depth activation on it, and the
    bilinearly up-sampled raw prediction that feeds the next decoder level.  Runs in fp32 (16..128 -> 1 channels:
    negligible cost) so that the depth handed to the warp kernels is not quantised to bf16."""

    def __init__(self, conv2d, cin, pred_depth):
        super().__init__()
        self.conv = conv2d(cin, 1, 3, activation="linear")
        self.predict_depth = pred_depth

    def forward(self, src, dst_height, dst_width, activate=True, split=False):
        """activate=False: depth is None -- the caller applies the activation to all scales at once
        (predict_depth.with_disparity_multi), the decoder itself only consuming the raw prediction.
        split=True (a feature map that ALSO feeds the next decoder level): a fourth result, `src` as an alias for that other
        consumer -- head and next level become one autograd node and their gradients are added inside the head's backward
        launch; likewise the raw prediction's two consumers (activation, up-sampling) below."""
        src_alias = src
        with torch.autocast(device_type=src.device.type, enabled=False):
            fused_fan_in = _FUSED_FAN_IN and split and torch.is_grad_enabled() and src.requires_grad
            if _conv.head_usable(src, self.conv.conv) and self.conv.slope == 1.0:
                if fused_fan_in:
                    conv, src_alias = _conv.head_conv_split(src, self.conv.conv.weight, self.conv.conv.bias)
                else:
                    conv = _conv.head_conv(src, self.conv.conv.weight, self.conv.conv.bias)     # bf16 features in, fp32 prediction out
            elif src.is_cuda:
                conv = self.conv(src.float())
            else:                       # (CPU: the layer's own dtype -- fp64 for the reference step of oracle/ref_step.py)
                conv = self.conv(src.to(self.conv.conv.weight.dtype))
            if not activate:
                depth, self.last_disp = None, None
            elif hasattr(self.predict_depth, "with_disparity"):
                depth, self.last_disp = self.predict_depth.with_disparity(conv)
            else:
                depth, self.last_disp = self.predict_depth(conv), None
            if (_BATCHED_HEADS and conv.is_cuda and conv.dtype == torch.float32 and conv.is_contiguous()
                    and src.dtype == _half() and (dst_height, dst_width) == (2 * conv.shape[2], 2 * conv.shape[3])):
                # the exact 2x resize and the cast to the decoder's dtype in one launch (one more for the backward)
                if _FUSED_FAN_IN and not activate and torch.is_grad_enabled() and conv.requires_grad:
                    conv, conv_up = _ops.upsample2x_split(conv, _half())
                else:
                    conv_up = _ops.upsample2x(conv, _half())
            else:
                conv_up = lo.resize_image(conv, dst_height, dst_width)
        if split:
            return depth, conv_up, conv, src_alias
        return depth, conv_up, conv


class DepthNetPretrained(nn.Module):
    """depth_net.py:112-167.  forward(image5d [B,S,H,W,3]) -> {"depth_ms": [d0 (1/1), d1 (1/2), d2 (1/4), d3 (1/8)]
    each [B,h,w,1] fp32, "debug_out": [p0, up0, p3, up3]}.  The target frame is the LAST frame (:131)."""

    def __init__(self, total_shape, global_batch, conv2d, pred_depth, upsample_iterp, net_name, use_pt_weight,
                 high_res):
        super().__init__()
        self.total_shape = tuple(total_shape)
        self.high_res = high_res
        self.encoder = PretrainedModel(net_name, use_pt_weight).encoder()
        self.cut_backward = False      # see forward()
        self.cuts = []                 # [(encoder outputs, their detached stand-ins)] of the forward calls of this step
        # taps inside a cell with structurally-zero filters arrive WITH them (no gather launch): the convolution that reads
        # such a skip has zero columns at those input channels -- zero by construction, like the encoder's (pretrained_nets)
        layout = self.encoder.tap_layout() if hasattr(self.encoder, "tap_layout") else [(c, None) for c in self.encoder.TAP_CHANNELS]
        self.physical_taps = any(sel is not None for _, sel in layout)
        (c1, _), (c2, sel2), (c3, _), (c4, _), (c5, _) = layout
        self.up4 = UpconvWithSkip(conv2d, c5, c4, 256, upsample_iterp)            # 1/16
        self.up3 = UpconvWithSkip(conv2d, 256, c3, 128, upsample_iterp)           # 1/8
        self.depth3 = ScaledDepthHead(conv2d, 128, pred_depth)
        self.up2 = UpconvWithSkip(conv2d, 128, c2 + 1, 64, upsample_iterp)        # 1/4
        self.depth2 = ScaledDepthHead(conv2d, 64, pred_depth)
        self.up1 = UpconvWithSkip(conv2d, 64, c1 + 1, 32, upsample_iterp)         # 1/2
        self.depth1 = ScaledDepthHead(conv2d, 32, pred_depth)
        self.up0 = UpconvWithSkip(conv2d, 32, 1, 16, upsample_iterp)              # 1/1: the only skip is p1 up-sampled
        # (hip/conv.py, XPT_WGRAD_DEFER: the decoder's weight gradients as one side-stream branch, issued when up4.conv1 --
        #  the decoder's first layer, last in the backward pass -- has sent its data gradient on to the encoder)
        for up in (self.up4, self.up3, self.up2, self.up1, self.up0):
            for layer in (up.conv1, up.conv2):
                layer.conv.weight.defer_wgrad = True
        self.up4.conv1.conv.weight.flush_wgrads = True
        self.depth0 = ScaledDepthHead(conv2d, 16, pred_depth)
        if any(sel is not None for (_, sel) in (layout[0], layout[2], layout[3], layout[4])):
            raise WrongInputException("structurally-zero channels are handled for the 1/4 tap only")
        self.skip2_zero = None
        if sel2 is not None:                                # input channels of up2.conv2: [64 upconv | c2 skip | 1 prediction]
            keep = torch.zeros(c2, dtype=torch.bool)
            keep[sel2] = True
            self.skip2_zero = 64 + torch.nonzero(~keep).flatten()
            self.apply_structural_zeros()

    def structural_pads(self):
        """[(tensor, out_sel, in_sel)] of the DECODER's own tensors with structurally-zero entries (the encoder lists its own):
        up2.conv2 reads the 1/4 tap with its zero channels, so its logical input channels are all but `skip2_zero`."""
        if self.skip2_zero is None:
            return []
        w = self.up2.conv2.conv.weight
        keep = torch.ones(w.shape[1], dtype=torch.bool)
        keep[self.skip2_zero] = False
        return [(w, None, torch.nonzero(keep).flatten())]

    def apply_structural_zeros(self):
        if self.skip2_zero is not None:
            with torch.no_grad():
                w = self.up2.conv2.conv.weight
                w[:, self.skip2_zero.to(w.device)] = 0

    def forward(self, image5d):
        target = image5d[:, -1].permute(0, 3, 1, 2)                               # [B,3,H,W] view of the NHWC frame
        height, width = target.shape[2:]
        taps = self.encoder(target, physical_taps=True) if self.physical_taps else self.encoder(target)
        if self.cut_backward and torch.is_grad_enabled() and all(t.requires_grad for t in taps):
            # the backward pass is cut between decoder and encoder (train_val.ModelTrainerDistrib: the gradients of
            # everything behind the encoder are all-reduced while the encoder's backward still runs): the decoder reads
            # detached leaves, whose gradients the trainer feeds into the encoder's graph in a second backward call
            leaves = [t.detach().requires_grad_(True) for t in taps]
            self.cuts.append((taps, leaves))
            taps = leaves
        conv1, conv2, conv3, conv4, conv5 = taps
        outputs = self.decode(conv1, conv2, conv3, conv4, conv5, height, width)
        return outputs

    def decode(self, conv1, conv2, conv3, conv4, conv5, height, width):
        heads = (self.depth0, self.depth1, self.depth2, self.depth3)
        # the depth activation of all four scales runs as one launch after the decoder (only the raw predictions feed
        # the next decoder level)
        batched = _BATCHED_HEADS and conv5.is_cuda and hasattr(self.depth0.predict_depth, "with_disparity_multi")
        upconv4 = self.up4(conv5, [conv4])
        upconv3 = self.up3(upconv4, [conv3])
        # (split=True: the level's feature map comes back as an alias for the next level -- its two gradients meet inside the
        #  prediction head's backward launch instead of in an aten add)
        depth3, dpconv2_up, dpconv3, upconv3 = self.depth3(upconv3, height // 4, width // 4, not batched, split=True)
        upconv2 = self.up2(upconv3, [conv2, dpconv2_up])
        depth2, dpconv1_up, dpconv2, upconv2 = self.depth2(upconv2, height // 2, width // 2, not batched, split=True)
        upconv1 = self.up1(upconv2, [conv1, dpconv1_up])
        depth1, dpconv0_up, dpconv1, upconv1 = self.depth1(upconv1, height, width, not batched, split=True)
        upconv0 = self.up0(upconv1, [dpconv0_up])
        depth0, _, dpconv0 = self.depth0(upconv0, height, width, not batched)
        if batched:
            with torch.autocast(device_type=conv5.device.type, enabled=False):
                (depth0, depth1, depth2, depth3), disps = self.depth0.predict_depth.with_disparity_multi(
                    [dpconv0, dpconv1, dpconv2, dpconv3])
            for h, d in zip(heads, disps):
                h.last_disp = d

        def nhwc1(x):      # [B,1,h,w] -> [B,h,w,1]: same memory, the reference's axis order
            return x.contiguous().reshape(x.shape[0], x.shape[2], x.shape[3], 1)

        out = {"depth_ms": [nhwc1(depth0), nhwc1(depth1), nhwc1(depth2), nhwc1(depth3)],
               "debug_out": [dpconv0, upconv0, dpconv3, upconv3]}
        disps = [h.last_disp for h in heads]
        for h in heads:        # hand the tensors over: a module attribute would keep this step's autograd graph (and its
            h.last_disp = None  # AccumulateGrad nodes with their stream) alive into the next step / a hipGraph capture
        if all(d is not None for d in disps):      # model_wrappers.py:48-49 would compute it with four more elementwise ops per scale
            out["disp_ms"] = [nhwc1(d) for d in disps]
        return out


class DepthNetBasic(nn.Module):
    """depth_net.py:10-92, the SfMLearner / GeoNet encoder-decoder (no pretrained backbone): fourteen convolutions down to 1/128
    (7 x 7, 7 x 7, 5 x 5, 5 x 5, then 3 x 3; every second one at stride 2), seven decoder levels up6 .. up0 whose first
    convolution's output is resized to the skip's extent (lo.resize_like: the encoder rounds odd extents UP, the 2x up-sampling
    doubles them), prediction heads on up3 .. up0.
    forward(image5d [B,S,H,W,3], already in [-1, 1]) -> {"depth_ms": [d0 (1/1), d1 (1/2), d2 (1/4), d3 (1/8)] each [B,h,w,1]
    fp32, "disp_ms": likewise, "debug_out": [upconv0, upconv3]}.  The target frame is the LAST frame (:37).

    Every layer is registered under the reference's layer name, the "_" between block and layer written as the module path's
    ".": dp_conv0b, dp_up6.conv1 (= dp_up6_conv1), dp_depth3.conv (= dp_depth3_conv); layer_names() gives the mapping.
    Kernel families at the bench shape: DESIGN.md section 13."""

    RESIZE = True
    # (name, filters, kernel, stride): depth_net.py:39-52
    ENCODER = (("dp_conv0b", 32, 7, 1), ("dp_conv1a", 32, 7, 2), ("dp_conv1b", 64, 5, 1), ("dp_conv2a", 64, 5, 2),
               ("dp_conv2b", 128, 3, 1), ("dp_conv3a", 128, 3, 2), ("dp_conv3b", 256, 3, 1), ("dp_conv4a", 256, 3, 2),
               ("dp_conv4b", 512, 3, 1), ("dp_conv5a", 512, 3, 2), ("dp_conv5b", 512, 3, 1), ("dp_conv6a", 512, 3, 2),
               ("dp_conv6b", 512, 3, 1), ("dp_conv7a", 512, 3, 2))
    TAPS = ("dp_conv1b", "dp_conv2b", "dp_conv3b", "dp_conv4b", "dp_conv5b", "dp_conv6b", "dp_conv7a")     # conv1 .. conv7

    def __init__(self, total_shape, global_batch, conv2d, pred_depth, upsample_iterp, high_res):
        super().__init__()
        self.total_shape = tuple(total_shape)
        self.high_res = high_res
        self.cut_backward = False      # DepthNetPretrained.forward: the cut sits between the encoder's taps and the decoder
        self.cuts = []
        cin = 3
        for name, filters, k, s in self.ENCODER:
            setattr(self, name, conv2d(cin, filters, k, strides=s))
            cin = filters
        up = lambda cin, skip, out: UpconvWithSkip(conv2d, cin, skip, out, upsample_iterp, resize=self.RESIZE)   # noqa: E731
        self.dp_up6 = up(512, 512, 512)            # 1/64
        self.dp_up5 = up(512, 512, 512)            # 1/32
        self.dp_up4 = up(512, 512, 256)            # 1/16
        self.dp_up3 = up(256, 256, 128)            # 1/8
        self.dp_depth3 = ScaledDepthHead(conv2d, 128, pred_depth)
        self.dp_up2 = up(128, 128 + 1, 64)         # 1/4
        self.dp_depth2 = ScaledDepthHead(conv2d, 64, pred_depth)
        self.dp_up1 = up(64, 64 + 1, 32)           # 1/2
        self.dp_depth1 = ScaledDepthHead(conv2d, 32, pred_depth)
        self.dp_up0 = up(32, 1, 16)                # 1/1: the "skip" is the up-sampled 1/2 prediction
        self.dp_depth0 = ScaledDepthHead(conv2d, 16, pred_depth)

    @property
    def encoder(self):
        """The fourteen encoder layers as one module (model_wrappers.set_backward_cut reads encoder.parameters()); a view, not
        a registered child: the state dict keeps the flat layer names."""
        return nn.ModuleList([getattr(self, name) for name, _, _, _ in self.ENCODER])

    def layer_names(self):
        """{reference layer name: its Conv2DSame}, in the reference's order of construction."""
        out = {name: getattr(self, name) for name, _, _, _ in self.ENCODER}
        for lvl in (6, 5, 4, 3):
            out[f"dp_up{lvl}_conv1"], out[f"dp_up{lvl}_conv2"] = getattr(self, f"dp_up{lvl}").conv1, getattr(self, f"dp_up{lvl}").conv2
        for lvl in (2, 1, 0):
            out[f"dp_depth{lvl + 1}_conv"] = getattr(self, f"dp_depth{lvl + 1}").conv
            out[f"dp_up{lvl}_conv1"], out[f"dp_up{lvl}_conv2"] = getattr(self, f"dp_up{lvl}").conv1, getattr(self, f"dp_up{lvl}").conv2
        out["dp_depth0_conv"] = self.dp_depth0.conv
        return out

    def check_extent(self, height, width):
        pass

    def encode(self, image5d):
        x = image5d[:, -1].permute(0, 3, 1, 2)                                    # [B,3,H,W] view of the NHWC frame
        if image5d.dtype == torch.float32 and _conv.usable(x, self.dp_conv0b.conv, self.dp_conv0b.slope):
            # the matrix-core path: the target frame cast to the 16-bit format with its five zero pad channels in one launch
            x = _conv.restack_bf16(image5d[:, -1:], 8)
        taps = []
        for name, _, _, _ in self.ENCODER:
            x = getattr(self, name)(x)
            if name in self.TAPS:
                taps.append(x)
        return taps

    def forward(self, image5d):
        height, width = image5d.shape[2:4]
        self.check_extent(height, width)
        taps = self.encode(image5d)
        if self.cut_backward and torch.is_grad_enabled() and all(t.requires_grad for t in taps):
            leaves = [t.detach().requires_grad_(True) for t in taps]
            self.cuts.append((taps, leaves))
            taps = leaves
        return self.decode(*taps, height, width)

    def decode(self, conv1, conv2, conv3, conv4, conv5, conv6, conv7, height, width):
        heads = (self.dp_depth0, self.dp_depth1, self.dp_depth2, self.dp_depth3)
        batched = _BATCHED_HEADS and conv7.is_cuda and hasattr(self.dp_depth0.predict_depth, "with_disparity_multi")
        upconv6 = self.dp_up6(conv7, [conv6])
        upconv5 = self.dp_up5(upconv6, [conv5])
        upconv4 = self.dp_up4(upconv5, [conv4])
        upconv3 = self.dp_up3(upconv4, [conv3])
        depth3, dpconv2_up, dpconv3, upconv3 = self.dp_depth3(upconv3, height // 4, width // 4, not batched, split=True)
        upconv2 = self.dp_up2(upconv3, [conv2, dpconv2_up])
        depth2, dpconv1_up, dpconv2, upconv2 = self.dp_depth2(upconv2, height // 2, width // 2, not batched, split=True)
        upconv1 = self.dp_up1(upconv2, [conv1, dpconv1_up])
        depth1, dpconv0_up, dpconv1, upconv1 = self.dp_depth1(upconv1, height, width, not batched, split=True)
        upconv0 = self.dp_up0(upconv1, [dpconv0_up])
        depth0, _, dpconv0 = self.dp_depth0(upconv0, height, width, not batched)
        if batched:
            with torch.autocast(device_type=conv7.device.type, enabled=False):
                (depth0, depth1, depth2, depth3), disps = self.dp_depth0.predict_depth.with_disparity_multi(
                    [dpconv0, dpconv1, dpconv2, dpconv3])
            for h, d in zip(heads, disps):
                h.last_disp = d

        def nhwc1(x):      # [B,1,h,w] -> [B,h,w,1]: same memory, the reference's axis order
            return x.contiguous().reshape(x.shape[0], x.shape[2], x.shape[3], 1)

        out = {"depth_ms": [nhwc1(depth0), nhwc1(depth1), nhwc1(depth2), nhwc1(depth3)],
               "debug_out": [upconv0, upconv3]}
        disps = [h.last_disp for h in heads]
        for h in heads:        # (DepthNetPretrained.decode: nothing of this step's graph stays on the module)
            h.last_disp = None
        if all(d is not None for d in disps):
            out["disp_ms"] = [nhwc1(d) for d in disps]
        return out


class DepthNetNoResize(DepthNetBasic):
    """depth_net.py:94-109: DepthNetBasic without the resize in its decoder levels.  Height and width must be multiples of 128
    (the reference's graph does not build otherwise: the concatenation's operands differ in extent)."""

    RESIZE = False

    def __init__(self, total_shape, global_batch, conv2d, pred_depth, upsample_iterp, high_res):
        super().__init__(total_shape, global_batch, conv2d, pred_depth, upsample_iterp, high_res)
        self.check_extent(self.total_shape[2], self.total_shape[3])

    def check_extent(self, height, width):
        if height % 128 or width % 128:
            raise WrongInputException(f"[DepthNetNoResize] height and width must be multiples of 128, got {height} x {width}")
