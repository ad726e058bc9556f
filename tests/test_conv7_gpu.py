"""7 x 7 dense convolutions (DepthNetBasic's dp_conv0b 3 -> 32 stride 1 and dp_conv1a 32 -> 32 stride 2, reference
model/build_model/depth_net.py:39-40) on the project's own kernels, against fp64 F.conv2d with explicit TF-SAME padding:
 * through the C ABI of BOTH libraries (bf16, IEEE half): xpt_conv2d_fwd (+ bias + ReLU), xpt_conv2d_bwd_data and
   xpt_conv2d_bwd_weight_partials, each with the automatic plan AND with the LDS-staged kernel forced (the family the
   benchmark-sized maps take), operands packed on the host in the layouts of ConvWeightPacker;
 * through layer_ops.Conv2DSame in the process's format: no library call, db, repeats, gradient sink.

Bounds.  16-bit outputs (y, dx): |err| <= 2^-8 |ref| + 1e-4 max|ref| for bf16, 2^-11 for IEEE half (tests/test_mbconv_gpu.py).
fp32 gradients (dw, db): 1.5e-2 of the largest magnitude (tests/test_conv_igemm_gpu.py)."""
import ctypes
import functools
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

FORMATS = {"bf16": (torch.bfloat16, 2.0 ** -8), "fp16": (torch.float16, 2.0 ** -11)}
# (cin, cout, stride, H, W): stride 1 on the image (Cin 3 padded to 8); stride 2 on even extents (pad 2 / 3) and odd ones (3 / 3)
CASES = [(3, 32, 1, 9, 11), (32, 32, 2, 10, 14), (32, 32, 2, 9, 13)]
B, K = 2, 7
NAMES = ("xpt_conv2d_fwd", "xpt_conv2d_bwd_data", "xpt_conv2d_bwd_weight_partials", "xpt_conv2d_bwd_weight_splits",
         "xpt_conv2d_tune", "xpt_half_format")


@functools.lru_cache(maxsize=None)
def library(fmt):
    from xpt_mde_2021_amd.hip import lib as xl
    lib = ctypes.CDLL(xl.LIB_PATH_F16 if fmt == "fp16" else xl.LIB_PATH)
    for name in NAMES:
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = xl.SIGNATURES[name]
    assert lib.xpt_half_format() == (1 if fmt == "fp16" else 0)
    return lib


def same_pads(n, k, s):
    total = max((-(-n // s) - 1) * s + k - n, 0)
    return total // 2, total - total // 2


@functools.lru_cache(maxsize=None)
def case(shape, fmt):
    """Inputs rounded to the 16-bit format (as fp64) and the fp64 references, computed once on the CPU; never modified."""
    cin, cout, stride, H, W = shape
    dtype, _ = FORMATS[fmt]
    g = torch.Generator().manual_seed(100 * cin + 10 * H + stride)
    x = torch.randn(B, cin, H, W, generator=g, dtype=torch.float64).to(dtype).double()
    w = (torch.randn(cout, cin, K, K, generator=g, dtype=torch.float64) / math.sqrt(cin * K * K)).to(dtype).double()
    b = (0.1 * torch.randn(cout, generator=g, dtype=torch.float64)).float().double()
    (pt, pb), (pl, pr) = same_pads(H, K, stride), same_pads(W, K, stride)
    if stride == 2:
        assert (pt, pb) == ((2, 3) if H % 2 == 0 else (3, 3))
    xr, wr, br = (t.clone().requires_grad_(True) for t in (x, w, b))
    y = F.relu(F.conv2d(F.pad(xr, (pl, pr, pt, pb)), wr, br, stride))
    gy = torch.randn(y.shape, generator=g, dtype=torch.float64).to(dtype).double()
    (y * gy).sum().backward()
    assert 0.2 < float((y.detach() > 0).double().mean()) < 0.8
    return dict(x=x, w=w, b=b, gy=gy, y=y.detach(), dx=xr.grad, dw=wr.grad, db=br.grad, pads=(pt, pl))


def bound_ok(got, ref, rel, what):
    err = (got.double().cpu() - ref).abs()
    allowed = rel * ref.abs() + 1e-4 * ref.abs().max()
    worst = float((err / allowed.clamp_min(1e-300)).max())
    print(f"  {what}: max |err| {float(err.max()):.3e}, worst err / bound {worst:.3f}")
    return bool(torch.isfinite(got).all()) and worst <= 1.0


def grad_ok(got, ref, what):
    err = float((got.double().cpu() - ref).abs().max() / ref.abs().max())
    print(f"  {what}: max error {err:.3e} of the largest magnitude")
    return bool(torch.isfinite(got).all()) and err < 1.5e-2


def ptr(t):
    return ctypes.c_void_p(t.data_ptr())


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def run_abi(lib, dev, fmt, shape, c):
    """(y, dx, dw) of the three entry points; g = gy * [y > 0] is formed on the host from the kernel's own stored y (exact in the
    16-bit format: a product with 0 or 1), as the layer's activation backward hands it to the two gradient kernels."""
    cin, cout, stride, H, W = shape
    dtype, _ = FORMATS[fmt]
    cp = (cin + 7) // 8 * 8
    pt, pl = c["pads"]
    OH, OW = -(-H // stride), -(-W // stride)
    x = torch.zeros((B, H, W, cp), dtype=dtype, device=dev)
    x[..., :cin] = c["x"].permute(0, 2, 3, 1).to(dtype).to(dev)
    wf = torch.zeros((cout, K * K, cp), dtype=dtype, device=dev)                    # forward operand [N][T][Cp]
    wf[..., :cin] = c["w"].permute(0, 2, 3, 1).reshape(cout, K * K, cin).to(dtype).to(dev)
    wb = torch.zeros((cp, K * K, cout), dtype=dtype, device=dev)                    # data-gradient operand [Cp][T][Np]
    wb[:cin] = c["w"].permute(1, 2, 3, 0).reshape(cin, K * K, cout).to(dtype).to(dev)
    bias = c["b"].float().to(dev)
    y = torch.zeros((B, OH, OW, cout), dtype=dtype, device=dev)
    assert lib.xpt_conv2d_fwd(ptr(x), ptr(wf), ptr(bias), ptr(y), B, H, W, cp, cp, cout, K, K, stride, pt, pl, OH, OW, cout, 0,
                              0.0, stream()) == 0
    g = (c["gy"].permute(0, 2, 3, 1).to(dtype).to(dev) * (y > 0).to(dtype)).contiguous()
    dx = torch.zeros((B, H, W, cp), dtype=dtype, device=dev)
    assert lib.xpt_conv2d_bwd_data(ptr(g), ptr(wb), ptr(dx), B, OH, OW, cout, cout, cp, K, K, stride, pt, pl, H, W, cp, 0,
                                   stream()) == 0
    nsplit = lib.xpt_conv2d_bwd_weight_splits(B, cp, cout, K, K, stride, OH, OW)
    assert nsplit >= 1
    n = cout * K * K * cin
    part = torch.zeros(nsplit * n, dtype=torch.float32, device=dev)
    assert lib.xpt_conv2d_bwd_weight_partials(ptr(g), ptr(x), ptr(part), part.numel(), B, H, W, cp, cin, cp, cout, cout, K, K,
                                              stride, pt, pl, OH, OW, 0, stream()) == 0
    torch.cuda.synchronize()
    dw = part.view(nsplit, cout, K, K, cin).double().sum(0).permute(0, 3, 1, 2)
    return y.permute(0, 3, 1, 2), dx.permute(0, 3, 1, 2)[:, :cin], dw


@pytest.mark.parametrize("fmt", list(FORMATS))
@pytest.mark.parametrize("lds", [False, True], ids=["auto", "lds"])
@pytest.mark.parametrize("shape", CASES, ids=lambda s: "x".join(str(v) for v in s))
def test_entry_points_accept_49_taps_in_both_formats(gpu_device, shape, lds, fmt):
    lib, (dtype, rel) = library(fmt), FORMATS[fmt]
    c = case(shape, fmt)
    try:
        if lds:
            assert lib.xpt_conv2d_tune(-100000) == 0 and lib.xpt_conv2d_tune(-1001) == 0     # no halo tiles; LDS kernel from 1 workgroup
        y, dx, dw = run_abi(lib, gpu_device, fmt, shape, c)
        y2, dx2, dw2 = run_abi(lib, gpu_device, fmt, shape, c)
    finally:
        assert lib.xpt_conv2d_tune(-100100) == 0 and lib.xpt_conv2d_tune(-1512) == 0          # the defaults
    ok = bound_ok(y, c["y"], rel, "forward")
    if shape[0] != 3:                                          # dp_conv0b reads the image: no data gradient
        ok &= bound_ok(dx, c["dx"], rel, "data gradient")
    ok &= grad_ok(dw, c["dw"], "weight gradient")
    assert torch.equal(y, y2) and torch.equal(dx, dx2) and torch.equal(dw, dw2), "two runs differ"
    assert ok


def _layer(shape, dev, half, c):
    from xpt_mde_2021_amd.model.model_util import layer_ops as lo
    cin, cout, stride, H, W = shape
    layer = lo.Conv2DSame(cin, cout, K, stride, activation="relu")
    with torch.no_grad():
        layer.conv.weight.copy_(c["w"])
        layer.conv.bias.copy_(c["b"])
    return layer.to(dev).to(memory_format=torch.channels_last)


@pytest.mark.parametrize("shape", CASES, ids=lambda s: "x".join(str(v) for v in s))
def test_conv2dsame_layer_runs_7x7_on_own_kernels(gpu_device, shape):
    """Conv2DSame(k = 7) under 16-bit autocast: no library (MIOpen) call, y / dx / dw / db against fp64, a second run bit-identical,
    and with the parameters on a FlatParameters buffer the gradient sink leaves the direct path's gradients bit for bit."""
    from xpt_mde_2021_amd.hip import lib as xl, ops
    from xpt_mde_2021_amd.model.model_util import layer_ops as lo
    from xpt_mde_2021_amd.model.model_util.optimizers import FlatParameters
    half = xl.half()
    fmt = "fp16" if half == torch.float16 else "bf16"
    rel = FORMATS[fmt][1]
    c = case(shape, fmt)
    cin = shape[0]
    layer = _layer(shape, gpu_device, half, c)
    gy = c["gy"].to(half).to(gpu_device)

    def step():
        x = c["x"].float().to(gpu_device).contiguous(memory_format=torch.channels_last).requires_grad_(cin != 3)
        with torch.autocast("cuda", dtype=half):
            y = layer(x)
        y.backward(gy)
        return y.detach(), x.grad

    before = lo.LIBRARY_CONV_CALLS[0]
    y, dx = step()
    dw, db = layer.conv.weight.grad.clone(), layer.conv.bias.grad.clone()
    layer.zero_grad(set_to_none=True)
    y2, dx2 = step()
    torch.cuda.synchronize()
    assert lo.LIBRARY_CONV_CALLS[0] == before, "the 7 x 7 layer went to the library"
    assert y.dtype == half
    ok = bound_ok(y, c["y"], rel, "forward")
    if cin != 3:
        ok &= bound_ok(dx, c["dx"], rel, "data gradient")
        assert torch.equal(dx, dx2)
    ok &= grad_ok(dw, c["dw"], "weight gradient") and grad_ok(db, c["db"], "bias gradient")
    assert torch.equal(y, y2) and torch.equal(dw, layer.conv.weight.grad) and torch.equal(db, layer.conv.bias.grad)
    # the same step with the gradient sink as the destination
    layer.zero_grad(set_to_none=True)
    flat = FlatParameters([layer.conv.weight, layer.conv.bias])
    assert hasattr(layer.conv.weight, "flat_grad") and hasattr(layer.conv.bias, "flat_grad")
    y3, dx3 = step()
    assert layer.conv.weight.grad is None and layer.conv.bias.grad is None and len(ops.grad_sink.pending) == 2
    ops.grad_sink.flush()
    flat.gather_grads()
    torch.cuda.synchronize()
    assert torch.equal(y, y3) and (cin == 3 or torch.equal(dx, dx3))
    assert torch.equal(flat.grad_views[0].detach(), dw), "weight gradient: sink path differs from the direct path"
    assert torch.equal(flat.grad_views[1].detach(), db), "bias gradient: sink path differs from the direct path"
    assert ok
