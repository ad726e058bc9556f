"""csrc/xpt_resize.hip through the C ABI of BOTH libraries (bf16, IEEE half) and through ops.resize_bilinear: the bilinear resize
to an arbitrary size (tf.image.resize of TF2: half-pixel centres, no antialiasing) and its adjoint against fp64
F.interpolate(align_corners=False, antialias=False) of the same 16-bit inputs.

Bound (the project's per-kernel bar for 16-bit outputs, tests/test_mbconv_gpu.py): |err| <= 2^-8 |ref| + 1e-4 max|ref| for bf16,
2^-11 for IEEE half -- the output format's rounding plus 1e-4 for fp32 arithmetic against fp64."""
import ctypes
import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

FORMATS = {"bf16": (torch.bfloat16, 2.0 ** -8), "fp16": (torch.float16, 2.0 ** -11)}
# (ih, iw, oh, ow): a non-integer shrink, a non-2x growth, an output of one row, a source of one row, one axis unchanged
SIZES = [(10, 14, 9, 13), (5, 7, 9, 13), (2, 4, 1, 2), (1, 2, 2, 3), (6, 8, 6, 5)]
CHANNELS = [8, 24, 136]
B = 2
NAMES = ("xpt_resize_bilinear_fwd", "xpt_resize_bilinear_adjoint", "xpt_half_format")


@functools.lru_cache(maxsize=None)
def library(fmt):
    from xpt_mde_2021_amd.hip import lib as xl
    lib = ctypes.CDLL(xl.LIB_PATH_F16 if fmt == "fp16" else xl.LIB_PATH)
    for name in NAMES:
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = xl.SIGNATURES[name]
    assert lib.xpt_half_format() == (1 if fmt == "fp16" else 0)
    return lib


@functools.lru_cache(maxsize=None)
def case(size, C, fmt):
    """16-bit inputs (as fp64) and the fp64 references of one case, computed once on the CPU; never modified."""
    ih, iw, oh, ow = size
    dtype, _ = FORMATS[fmt]
    g = torch.Generator().manual_seed(1000 * C + 100 * ih + 10 * ow + oh)
    x = torch.randn(B, C, ih, iw, generator=g, dtype=torch.float64).to(dtype).double()
    gy = torch.randn(B, C, oh, ow, generator=g, dtype=torch.float64).to(dtype).double()
    xr = x.clone().requires_grad_(True)
    y = F.interpolate(xr, size=(oh, ow), mode="bilinear", align_corners=False, antialias=False)
    (y * gy).sum().backward()
    return dict(x=x, gy=gy, y=y.detach(), dx=xr.grad)


def bound_ok(got, ref, rel, what):
    err = (got.double().cpu() - ref).abs()
    allowed = rel * ref.abs() + 1e-4 * ref.abs().max()
    worst = float((err / allowed.clamp_min(1e-300)).max())
    print(f"  {what}: max |err| {float(err.max()):.3e}, worst err / bound {worst:.3f}")
    return bool(torch.isfinite(got).all()) and worst <= 1.0


def nhwc(t, dtype, dev, pitch=None):
    """NCHW fp64 CPU tensor -> NHWC 16-bit device tensor, optionally as the leading channels of a wider (pitch) tensor whose
    other channels hold NaN (a kernel that reads past its slice shows up at once)."""
    t = t.permute(0, 2, 3, 1).contiguous().to(dtype).to(dev)
    if pitch is None:
        return t
    wide = torch.full((*t.shape[:3], pitch), float("nan"), dtype=dtype, device=dev)
    wide[..., :t.shape[3]] = t
    return wide


def ptr(t):
    return ctypes.c_void_p(t.data_ptr())


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def run(lib, dev, fmt, size, C, c, pitch=None):
    ih, iw, oh, ow = size
    dtype, _ = FORMATS[fmt]
    x, gy = nhwc(c["x"], dtype, dev, pitch), nhwc(c["gy"], dtype, dev, pitch)
    sp = pitch or C
    y = torch.zeros((B, oh, ow, C), dtype=dtype, device=dev)
    dx = torch.zeros((B, ih, iw, C), dtype=dtype, device=dev)
    assert lib.xpt_resize_bilinear_fwd(ptr(x), sp, ptr(y), C, B, ih, iw, oh, ow, C, stream()) == 0
    assert lib.xpt_resize_bilinear_adjoint(ptr(gy), sp, ptr(dx), C, B, ih, iw, oh, ow, C, stream()) == 0
    torch.cuda.synchronize()
    return y.permute(0, 3, 1, 2), dx.permute(0, 3, 1, 2)


@pytest.mark.parametrize("fmt", list(FORMATS))
@pytest.mark.parametrize("C", CHANNELS)
@pytest.mark.parametrize("size", SIZES, ids=lambda s: "{}x{}to{}x{}".format(*s))
def test_forward_and_adjoint_against_fp64(gpu_device, size, C, fmt):
    lib, (dtype, rel) = library(fmt), FORMATS[fmt]
    c = case(size, C, fmt)
    y, dx = run(lib, gpu_device, fmt, size, C, c)
    ok = bound_ok(y, c["y"], rel, "forward")
    ok &= bound_ok(dx, c["dx"], rel, "adjoint")
    # the adjoint identity <resize(x), g> == <x, adjoint(g)> in fp64 on the dequantised 16-bit results: each side is a sum of
    # products of one 16-bit-rounded factor, so the two differ by at most rel * sum |terms| (+ the 1e-4 fp32 share)
    lhs, rhs = float((y.double().cpu() * c["gy"]).sum()), float((c["x"] * dx.double().cpu()).sum())
    scale = float((c["y"].abs() * c["gy"].abs()).sum()) + float((c["x"].abs() * c["dx"].abs()).sum())
    print(f"  adjoint identity: {lhs:.6e} vs {rhs:.6e}, |diff| / bound {abs(lhs - rhs) / ((rel + 1e-4) * scale):.3f}")
    ok &= abs(lhs - rhs) <= (rel + 1e-4) * scale
    y2, dx2 = run(lib, gpu_device, fmt, size, C, c)
    assert torch.equal(y, y2) and torch.equal(dx, dx2), "two runs differ"
    assert ok


@pytest.mark.parametrize("fmt", list(FORMATS))
def test_channel_slice_input_is_read_in_place(gpu_device, fmt):
    """24 channels of a 40-channel tensor (pixel pitch > C): the same bits as the dense input."""
    lib = library(fmt)
    size, C = (5, 7, 9, 13), 24
    c = case(size, C, fmt)
    y, dx = run(lib, gpu_device, fmt, size, C, c)
    ys, dxs = run(lib, gpu_device, fmt, size, C, c, pitch=40)
    assert torch.equal(y, ys) and torch.equal(dx, dxs)
    assert bool(torch.isfinite(ys).all()) and bool(torch.isfinite(dxs).all())


def test_bad_arguments_are_rejected(gpu_device):
    lib = library("bf16")
    one = ctypes.c_void_p(16)
    assert lib.xpt_resize_bilinear_fwd(None, 8, one, 8, 1, 2, 2, 3, 3, 8, None) == -1
    assert lib.xpt_resize_bilinear_fwd(one, 8, one, 8, 1, 2, 2, 0, 3, 8, None) == -2
    assert lib.xpt_resize_bilinear_fwd(one, 8, one, 8, 1, 2, 2, 3, 3, 12, None) == -3          # C % 8
    assert lib.xpt_resize_bilinear_adjoint(one, 4, one, 8, 1, 2, 2, 3, 3, 8, None) == -3       # pitch < C
    assert lib.xpt_resize_bilinear_adjoint(ctypes.c_void_p(8), 8, one, 8, 1, 2, 2, 3, 3, 8, None) == -3   # alignment


def test_autograd_op_and_resize_image_dispatch(gpu_device):
    """ops.resize_bilinear in the process's 16-bit format: forward + backward through autograd on a channel-slice input, the
    identity for equal sizes, and layer_ops.resize_image / resize_like calling it for 16-bit device tensors only."""
    from xpt_mde_2021_amd.hip import lib as xl, ops
    from xpt_mde_2021_amd.model.model_util import layer_ops as lo
    half = xl.half()
    fmt = "fp16" if half == torch.float16 else "bf16"
    rel = FORMATS[fmt][1]
    size, C = (5, 7, 9, 13), 24
    c = case(size, C, fmt)
    wide = nhwc(c["x"], half, gpu_device, pitch=40).permute(0, 3, 1, 2)
    x = wide[:, :C].detach().requires_grad_(True)
    assert ops.resize_bilinear(x, (5, 7)) is x
    y = lo.resize_image(x, 9, 13)
    assert y.dtype == half and y.grad_fn is not None and "ResizeBilinear" in type(y.grad_fn).__name__
    y.backward(c["gy"].to(half).to(gpu_device))
    torch.cuda.synchronize()
    assert bound_ok(y.detach(), c["y"], rel, "forward") and bound_ok(x.grad, c["dx"], rel, "backward")
    assert torch.equal(lo.resize_like(x, torch.zeros(1, 1, 9, 13)), y)
    x32 = c["x"].float().to(gpu_device)
    want = F.interpolate(x32, size=(9, 13), mode="bilinear", align_corners=False, antialias=False)
    assert torch.equal(lo.resize_image(x32, 9, 13), want)                                       # fp32: the framework's resize
