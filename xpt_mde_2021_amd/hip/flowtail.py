"""PWC-Net's 2-channel layers on own gfx950 kernels (csrc/xpt_flowtail.hip): the Conv2D(2, 3, "same", linear) flow heads and
the Conv2DTranspose(2, 4, 2, "same") up-samplers of model/build_model/flow_net.py, each one launch forward and one backward.

Both read the fp32 master weights directly, in channels-last memory order -- a [2, C, 3, 3] head kernel is [2][3][3][C] in
memory, a [C, 2, 4, 4] transposed kernel [C][4][4][2] -- which is also the order of the weight-gradient rows the backward
launch leaves for the step's finishing launch (hip/ops.py GradSink).  A weight in the other memory order is permuted outside
the kernel and its gradient is returned as a tensor; it is never written permuted into a flat gradient buffer.  Results are
fp32: the flow stays unquantised from the head through the up-sampler to the warp.  Misuse raises XptHipError; nothing falls
through to another path."""
import torch

from . import conv as _conv
from . import lib as _lib
from . import ops as _ops

HEAD_CHANNELS = (16, 32, 64, 128)
UPCONV_CHANNELS_16BIT = (8, 16, 32)


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _channels_last_weight(w):
    """(the weight with channels-last memory order, whether it had that order already)."""
    native = w.permute(0, 2, 3, 1).is_contiguous()
    if not native:
        w = w.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
    return w, native


def _sink_of(weight, bias, native, numel):
    """Flat-gradient destinations (weight, bias or None) when the finishing launch can write the kernel's rows as they are."""
    if not native or not _ops.grad_sink.wants(weight) or weight.flat_grad.numel() != numel or weight.flat_grad.dim() != 1:
        return None
    if bias is not None and not (_ops.grad_sink.wants(bias) and bias.flat_grad.numel() == 2):
        return None
    return weight.flat_grad, None if bias is None else bias.flat_grad


def _partials(ctx, tag, nblk, row, device):
    if ctx.sink is not None:
        return _ops.grad_sink.partials(ctx.sink[0], tag, nblk * row)
    # no deferred destination (a weight outside FlatParameters, or one stored in the other memory order): the rows are summed
    # by the framework, and a framework sum must not enter a captured step
    if torch.cuda.is_current_stream_capturing():
        raise _lib.XptHipError(f"{tag}: weight gradient without a flat-gradient destination inside a graph capture")
    return torch.empty(nblk * row, dtype=torch.float32, device=device)


def _finish(ctx, ws, nblk, row):
    """The partial rows -> (dW as [row - 2] floats in memory order, db) tensors, or (None, None) through the sink."""
    nw = row - 2
    if ctx.sink is not None:
        _ops.grad_sink.add(ctx.sink[0], ws, 0, nw, nblk, row)
        if ctx.sink[1] is not None:
            _ops.grad_sink.add(ctx.sink[1], ws, nw, 2, nblk, row)
        return None, None
    tot = ws[:nblk * row].view(nblk, row).sum(0)
    return tot[:nw], (tot[nw:].clone() if ctx.has_bias else None)


def _check_common(name, x, weight, bias):
    if not (torch.is_tensor(x) and x.is_cuda and x.dim() == 4):
        raise _lib.XptHipError(f"{name}: expected a 4-d CUDA/HIP tensor (no CPU fallback)")
    if not weight.is_cuda or weight.dtype != torch.float32:
        raise _lib.XptHipError(f"{name}: weight must be a float32 CUDA/HIP tensor, got {weight.dtype} on {weight.device}")
    if bias is not None and (not bias.is_cuda or bias.dtype != torch.float32 or tuple(bias.shape) != (2,)):
        raise _lib.XptHipError(f"{name}: bias must be float32 [2] on the GPU or None")


# ------------------------------------------------------------------------------- flow heads: Conv2D(2, 3, "same", linear)
class _FlowHead(torch.autograd.Function):
    """pre [B,2,H,W] fp32 (NHWC storage) = conv3x3_same(x 16-bit, weight [2,C,3,3]) + bias."""

    @staticmethod
    def forward(ctx, x, weight, bias):
        lib = _lib.load()
        _check_common("flow_head", x, weight, bias)
        C = x.shape[1]
        if C not in HEAD_CHANNELS:
            raise _lib.XptHipError(f"flow_head: {C} input channels (served: {HEAD_CHANNELS})")
        if tuple(weight.shape) != (2, C, 3, 3):
            raise _lib.XptHipError(f"flow_head: weight must be float32 [2, {C}, 3, 3], got {tuple(weight.shape)}")
        x, xpitch = _conv.nhwc_view(x)
        B, _, H, W = x.shape
        w, native = _channels_last_weight(weight.detach())
        b_ = None if bias is None else bias.detach().contiguous()
        pre = torch.empty((B, H, W, 2), dtype=torch.float32, device=x.device)
        _lib.check(lib.xpt_flowhead_fwd(x.data_ptr(), xpitch, w.data_ptr(), None if b_ is None else b_.data_ptr(),
                                        pre.data_ptr(), B, H, W, C, _stream()), "xpt_flowhead_fwd")
        ctx.save_for_backward(x, w)
        ctx.geom = (B, C, H, W, xpitch)
        ctx.sink = _sink_of(weight, bias, native, 18 * C)
        ctx.has_bias = bias is not None
        return pre.permute(0, 3, 1, 2)

    @staticmethod
    def backward(ctx, g):
        lib = _lib.load()
        x, w = ctx.saved_tensors
        B, C, H, W, xpitch = ctx.geom
        g = g.float().permute(0, 2, 3, 1).contiguous()                   # [B,H,W,2]: a view for a channels-last cotangent
        dx = torch.empty((B, C, H, W), dtype=_lib.half(), device=g.device, memory_format=torch.channels_last)
        if dx.stride(1) != 1:                                           # [B,C,1,1]: force the NHWC order
            dx = torch.empty((B, H, W, C), dtype=_lib.half(), device=g.device).permute(0, 3, 1, 2)
        nblk = lib.xpt_flowhead_bwd_blocks(B, H, W, C)
        row = 18 * C + 2
        ws = _partials(ctx, "flow_head", nblk, row, g.device)
        _lib.check(lib.xpt_flowhead_bwd(x.data_ptr(), xpitch, w.data_ptr(), g.data_ptr(), dx.data_ptr(), ws.data_ptr(),
                                        ws.numel(), B, H, W, C, _stream()), "xpt_flowhead_bwd")
        dw, db = _finish(ctx, ws, nblk, row)
        if dw is not None:
            dw = dw.view(2, 3, 3, C).permute(0, 3, 1, 2)
        return dx, dw, db


def flow_head(x, weight, bias):
    """Conv2D(2, 3, padding="same", linear) of predict_flow / the context network (flow_net.py:131-163): x [B,C,H,W] in the
    library's 16-bit format (NHWC storage, channel slices in place, C in 16 / 32 / 64 / 128), weight [2,C,3,3] float32, bias [2]
    float32 or None -> [B,2,H,W] float32 (NHWC storage)."""
    return _FlowHead.apply(x, weight, bias)


def flow_head_usable(x, conv):
    """Can this convolution (an nn.Conv2d) run as flow_head on x?  The GPU, 16-bit autocast in the library's format (or a tensor
    already in it), fp32 master weights, 3 x 3, stride 1, no dilation, dense, 2 outputs, a served channel count."""
    if not (torch.is_tensor(x) and x.is_cuda and x.dim() == 4):
        return False
    dtype = torch.get_autocast_dtype("cuda") if torch.is_autocast_enabled() else x.dtype
    return dtype == _lib.half() and conv.weight.dtype == torch.float32 and conv.out_channels == 2 \
        and conv.in_channels in HEAD_CHANNELS and x.shape[1] == conv.in_channels and tuple(conv.kernel_size) == (3, 3) \
        and tuple(conv.stride) == (1, 1) and tuple(conv.dilation) == (1, 1) and conv.groups == 1


# ------------------------------------------------------------------------------- up-samplers: Conv2DTranspose(2, 4, 2, "same")
class _UpConv4x4s2(torch.autograd.Function):
    """y [B,2,2H,2W] fp32 (NHWC storage) = conv_transpose2d(x, weight [C,2,4,4], stride 2, padding 1) + bias; x is the fp32
    2-channel flow or a 16-bit feature map."""

    @staticmethod
    def forward(ctx, x, weight, bias):
        lib = _lib.load()
        _check_common("upconv4x4s2", x, weight, bias)
        C = x.shape[1]
        if x.dtype == torch.float32:
            if C != 2:
                raise _lib.XptHipError(f"upconv4x4s2: a float32 input has 2 channels (the flow), got {C}")
            x = x.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)   # a no-op for NHWC storage
            xpitch, f32 = 2, 1
        elif x.dtype == _lib.half():
            if C not in UPCONV_CHANNELS_16BIT:
                raise _lib.XptHipError(f"upconv4x4s2: {C} input channels in the 16-bit format (served: {UPCONV_CHANNELS_16BIT})")
            x, xpitch = _conv.nhwc_view(x)
            f32 = 0
        else:
            raise _lib.XptHipError(f"upconv4x4s2: input must be float32 or {_lib.half()}, got {x.dtype}")
        if tuple(weight.shape) != (C, 2, 4, 4):
            raise _lib.XptHipError(f"upconv4x4s2: weight must be float32 [{C}, 2, 4, 4], got {tuple(weight.shape)}")
        B, _, H, W = x.shape
        w, native = _channels_last_weight(weight.detach())
        b_ = None if bias is None else bias.detach().contiguous()
        y = torch.empty((B, 2 * H, 2 * W, 2), dtype=torch.float32, device=x.device)
        _lib.check(lib.xpt_upconv4x4s2_fwd(x.data_ptr(), xpitch, f32, w.data_ptr(), None if b_ is None else b_.data_ptr(),
                                           y.data_ptr(), B, H, W, C, _stream()), "xpt_upconv4x4s2_fwd")
        ctx.save_for_backward(x, w)
        ctx.geom = (B, C, H, W, xpitch, f32)
        ctx.sink = _sink_of(weight, bias, native, 32 * C)
        ctx.has_bias = bias is not None
        return y.permute(0, 3, 1, 2)

    @staticmethod
    def backward(ctx, g):
        lib = _lib.load()
        x, w = ctx.saved_tensors
        B, C, H, W, xpitch, f32 = ctx.geom
        g = g.float().permute(0, 2, 3, 1).contiguous()                   # [B,2H,2W,2]
        dx = torch.empty((B, H, W, C), dtype=torch.float32 if f32 else _lib.half(), device=g.device)
        nblk = lib.xpt_upconv4x4s2_bwd_blocks(B, H, W, C, f32)
        row = 32 * C + 2
        ws = _partials(ctx, "upconv4x4s2", nblk, row, g.device)
        _lib.check(lib.xpt_upconv4x4s2_bwd(x.data_ptr(), xpitch, f32, w.data_ptr(), g.data_ptr(), dx.data_ptr(), ws.data_ptr(),
                                           ws.numel(), B, H, W, C, _stream()), "xpt_upconv4x4s2_bwd")
        dw, db = _finish(ctx, ws, nblk, row)
        if dw is not None:
            dw = dw.view(C, 4, 4, 2).permute(0, 3, 1, 2)
        return dx.permute(0, 3, 1, 2), dw, db


def upconv4x4s2(x, weight, bias):
    """Conv2DTranspose(2, 4, strides=2, padding="same") (flow_net.py:145-148) = conv_transpose2d(stride 2, padding 1) + bias:
    x [B,C,H,W] float32 with C = 2 (the flow) or the library's 16-bit format with C in 8 / 16 / 32 (NHWC storage, channel slices
    in place), weight [C,2,4,4] float32, bias [2] float32 or None -> [B,2,2H,2W] float32 (NHWC storage)."""
    return _UpConv4x4s2.apply(x, weight, bias)


def upconv_usable(x, weight):
    """Can upconv4x4s2 serve x with this weight?  The GPU, 16-bit autocast in the library's format, an fp32 [C,2,4,4] master
    weight, and x the fp32 flow (C = 2) or a 16-bit feature map (C in 8 / 16 / 32)."""
    if not (torch.is_tensor(x) and x.is_cuda and x.dim() == 4 and weight.is_cuda and weight.dtype == torch.float32):
        return False
    if not (torch.is_autocast_enabled() and torch.get_autocast_dtype("cuda") == _lib.half()):
        return False
    C = x.shape[1]
    if tuple(weight.shape) != (C, 2, 4, 4):
        return False
    return (x.dtype == torch.float32 and C == 2) or (x.dtype == _lib.half() and C in UPCONV_CHANNELS_16BIT)
