"""Dilated 3 x 3 convolutions on the library's own kernels (csrc/xpt_conv_dilated.hip) -- Conv2D(3, padding="same",
dilation_rate=d) of PWC-Net's context network (model/build_model/flow_net.py context[1..4]) -- against a plain fp32 PyTorch
reference of the same op on the same 16-bit-rounded operands: forward (+ bias + LeakyReLU), data, weight and bias gradient.

Reference and bars are those of tests/test_conv_igemm_gpu.py::test_conv_fwd_bwd_matches_fp32_reference: products of 16-bit
operands are exact in fp32 and both sides accumulate in fp32, so the forward differs by the final 16-bit rounding of y
(2^-8 relative for bf16) and the summation order (6e-3 of the largest magnitude); gradients see one more 16-bit rounding, of g
(1.5e-2).  At stride 1 TF SAME with an effective extent 2 d + 1 is `d` zeros on every side, i.e. F.conv2d(padding=d, dilation=d).

Achieved on the MI355X (bf16): forward 1.7e-3 .. 3.5e-3, dx 2.0e-3 .. 3.2e-3, dw at most 1.9e-4, db at most 3.5e-7 of the
largest magnitude; one line per case in DESIGN.md section 14."""
import math

import pytest
import torch
import torch.nn.functional as F

from xpt_mde_2021_amd.hip.lib import half as _half_dtype

HALF = _half_dtype()

pytestmark = pytest.mark.gpu

# (cin, cout, d, H, W, slope)
CASES = [
    (32, 128, 2, 16, 24, 0.1),
    (128, 128, 4, 16, 24, 0.1),
    (128, 96, 8, 16, 24, 0.1),
    (96, 64, 16, 16, 24, 0.1),       # d >= H: vertically only the centre tap row is ever in range
    (128, 128, 2, 13, 21, 1.0),      # ragged tiles, linear
    (20, 8, 4, 9, 11, 0.1),          # input padded 20 -> 24, narrowest legal output, map smaller than one tile
    (64, 64, 16, 40, 8, 0.1),        # d >= W but d < H
]
BATCH = 2
_REF = {}


@pytest.fixture(scope="module", autouse=True)
def _leave_nothing_behind():
    """The module's reference cache, its device tensors and the allocator blocks they sat in are released when it ends, and
    the process-wide generator is put back, so that the tests that follow in the same process start from what they would
    have seen without this file."""
    cpu_rng = torch.get_rng_state()
    gpu_rng = torch.cuda.get_rng_state() if torch.cuda.is_available() else None
    yield
    import gc
    _REF.clear()
    gc.collect()
    if torch.cuda.is_available():
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.set_rng_state(gpu_rng)
    torch.set_rng_state(cpu_rng)


def reference(x, w, b, d, slope):
    y = F.conv2d(x, w, b, 1, padding=d, dilation=d)
    return F.leaky_relu(y, slope) if slope != 1.0 else y


def case(cin, cout, d, H, W, slope):
    """Operands (rounded to the 16-bit format) and the fp32 CPU reference of one case, computed once per process."""
    key = (cin, cout, d, H, W, slope)
    if key not in _REF:
        g = torch.Generator().manual_seed(cin * 131 + cout * 7 + d)
        x = torch.randn(BATCH, cin, H, W, generator=g).to(HALF)
        w = (torch.randn(cout, cin, 3, 3, generator=g) / math.sqrt(cin * 9)).to(HALF).float()
        b = 0.1 * torch.randn(cout, generator=g)
        xr = x.float().requires_grad_(True)
        wr = w.clone().requires_grad_(True)
        br = b.clone().requires_grad_(True)
        yr = reference(xr, wr, br, d, slope)
        gy = torch.randn(yr.shape, generator=g).to(HALF)
        (yr * gy.float()).sum().backward()
        _REF[key] = dict(x=x, w=w, b=b, gy=gy, y=yr.detach(), dx=xr.grad, dw=wr.grad, db=br.grad)
    return _REF[key]


def run(dev, c, cin, d, slope):
    from xpt_mde_2021_amd.hip import conv as xc
    cp = xc.round_up(cin, 8)
    xd = F.pad(c["x"], (0, 0, 0, 0, 0, cp - cin)).to(dev).contiguous(memory_format=torch.channels_last).requires_grad_(True)
    wd = c["w"].to(dev).contiguous(memory_format=torch.channels_last).requires_grad_(True)
    bd = c["b"].to(dev).requires_grad_(True)
    yd = xc.conv2d_same(xd, wd, bd, 1, slope, dilation=d)
    (yd.float() * c["gy"].to(dev).float()).sum().backward()
    torch.cuda.synchronize()
    return yd.detach(), xd.grad, wd.grad, bd.grad


def rel_err(a, ref):
    a, ref = a.detach().float().cpu(), ref.detach().float()
    return (a - ref).abs().max().item() / (ref.abs().max().item() + 1e-12)


def close(a, ref, rtol, what):
    err = rel_err(a, ref)
    assert err < rtol, f"{what}: max error {err:.3e} of the largest magnitude (allowed {rtol})"


@pytest.mark.parametrize("cin,cout,d,H,W,slope", CASES)
def test_dilated_conv_fwd_bwd_matches_fp32_reference(gpu_device, cin, cout, d, H, W, slope):
    from xpt_mde_2021_amd.hip import conv as xc
    c = case(cin, cout, d, H, W, slope)
    cp = xc.round_up(cin, 8)
    yd, dx, dw, db = run(gpu_device, c, cin, d, slope)
    assert yd.shape == c["y"].shape and yd.dtype == HALF
    print(f"[dilated] cin {cin} cout {cout} d {d} {H}x{W} slope {slope}: forward {rel_err(yd, c['y']):.2e}  "
          f"dx {rel_err(dx[:, :cin], c['dx']):.2e}  dw {rel_err(dw, c['dw']):.2e}  db {rel_err(db, c['db']):.2e}")
    close(yd, c["y"], 6e-3, "forward")
    close(dx[:, :cin], c["dx"], 1.5e-2, "data gradient")
    if cp > cin:
        assert float(dx[:, cin:].abs().max()) == 0.0, "pad channels of dx are not exactly zero"
    close(dw, c["dw"], 1.5e-2, "weight gradient")
    close(db, c["db"], 1.5e-2, "bias gradient")


def test_dilated_conv_is_deterministic(gpu_device):
    """Two runs of the d = 4 case: y, dx and dw bit for bit (fixed summation order, no atomics)."""
    cin, cout, d, H, W, slope = CASES[1]
    c = case(cin, cout, d, H, W, slope)
    y0, dx0, dw0, _ = run(gpu_device, c, cin, d, slope)
    y1, dx1, dw1, _ = run(gpu_device, c, cin, d, slope)
    assert torch.equal(y0, y1) and torch.equal(dx0, dx1) and torch.equal(dw0, dw1)


def test_dilated_weight_gradient_through_the_gradient_sink(gpu_device):
    """With a flat-gradient destination bound (FlatParameters), the weight gradient that xpt_reduce_partials leaves in the flat
    buffer is, bit for bit, the sum of the plain path's split partials in split order (up to 32 splits the finishing launch
    adds a job's splits one after the other; this shape has 32 units, so at most 32 splits), lands in the parameter's own
    element order, and differs from the plain path's own (framework) sum of the same partials by no more than fp32 reassociation of
    `splits` terms can: splits * 2^-23 * sum_s |partial_s| per element."""
    from xpt_mde_2021_amd.hip import conv as xc, lib as xl, ops
    from xpt_mde_2021_amd.model.model_util.optimizers import FlatParameters
    dev = gpu_device
    cin, cout, d, H, W, _ = CASES[1]
    c = case(cin, cout, d, H, W, 0.1)
    conv = torch.nn.Conv2d(cin, cout, 3, bias=False)
    with torch.no_grad():
        conv.weight.copy_(c["w"])
    conv = conv.to(dev).to(memory_format=torch.channels_last)
    xd = c["x"].to(dev).contiguous(memory_format=torch.channels_last)
    gy = c["gy"].to(dev).contiguous(memory_format=torch.channels_last)

    def step():
        y = xc.conv2d_same(xd, conv.weight, None, 1, 1.0, dilation=d)        # linear, no bias: g is gy itself
        y.backward(gy)

    step()
    torch.cuda.synchronize()
    plain = conv.weight.grad.detach().clone()
    conv.weight.grad = None
    # the plain path's partials, from the entry point it calls
    lib = xl.load()
    ns = lib.xpt_conv2d_dilated_bwd_weight_splits(BATCH, cin, cout, 3, 3, 1, d, H, W)
    assert ns >= 1
    n = cout * 9 * cin
    part = torch.empty(ns * n, dtype=torch.float32, device=dev)
    xl.check(lib.xpt_conv2d_dilated_bwd_weight_partials(gy.data_ptr(), xd.data_ptr(), part.data_ptr(), part.numel(), BATCH, H, W,
                                                        cin, cin, cin, cout, cout, 3, 3, 1, d,
                                                        torch.cuda.current_stream().cuda_stream), "partials")
    part = part.view(ns, cout, 3, 3, cin)
    want = part[0].clone()
    for s in range(1, ns):
        want = want + part[s]
    want = want.permute(0, 3, 1, 2)
    flat = FlatParameters([conv.weight])
    assert hasattr(conv.weight, "flat_grad")
    step()
    assert conv.weight.grad is None and len(ops.grad_sink.pending) == 1
    ops.grad_sink.flush()
    flat.gather_grads()
    torch.cuda.synchronize()
    got = flat.grad_views[0].detach()
    assert torch.equal(got, want), "sink path: not the in-order sum of the plain path's partials"
    bound = ns * 2.0 ** -23 * part.abs().sum(0).permute(0, 3, 1, 2)
    assert bool(((got - plain).abs() <= bound).all()), "sink path and plain path differ by more than fp32 reassociation"
    wr = c["w"].clone().requires_grad_(True)                                 # (the shared reference has bias + LeakyReLU)
    (F.conv2d(c["x"].float(), wr, None, 1, padding=d, dilation=d) * c["gy"].float()).sum().backward()
    close(got, wr.grad, 1.5e-2, "weight gradient (sink)")


def _layer_and_twin(cin, cout, d, dev, seed):
    from xpt_mde_2021_amd.model.model_util import layer_ops as lo
    torch.manual_seed(seed)
    twin = lo.Conv2DSame(cin, cout, 3, dilation_rate=d)                      # fp32, stays on the CPU
    with torch.no_grad():
        twin.conv.weight.copy_((torch.randn(cout, cin, 3, 3) / math.sqrt(cin * 9)).to(HALF).float())
        twin.conv.bias.copy_(0.1 * torch.randn(cout))
    layer = lo.Conv2DSame(cin, cout, 3, dilation_rate=d)
    layer.load_state_dict(twin.state_dict())
    return layer.to(dev).to(memory_format=torch.channels_last), twin


def test_conv2dsame_layer_runs_dilated_on_own_kernels(gpu_device):
    """Conv2DSame(128, 128, 3, dilation_rate=4) forward + backward under 16-bit autocast: no library (MIOpen) call, and y / dx /
    dw / db match the same module evaluated in fp32 on the CPU within the bars above."""
    from xpt_mde_2021_amd.model.model_util import layer_ops as lo
    dev = gpu_device
    layer, twin = _layer_and_twin(128, 128, 4, dev, 11)
    g = torch.Generator().manual_seed(12)
    x = torch.randn(BATCH, 128, 16, 24, generator=g).to(HALF)
    gy = torch.randn(BATCH, 128, 16, 24, generator=g).to(HALF)
    xr = x.float().requires_grad_(True)
    yr = twin(xr)
    yr.backward(gy.float())
    before = lo.LIBRARY_CONV_CALLS[0]
    xd = x.to(dev).contiguous(memory_format=torch.channels_last).requires_grad_(True)
    with torch.autocast("cuda", dtype=HALF):
        yd = layer(xd)
    yd.backward(gy.to(dev))
    torch.cuda.synchronize()
    assert lo.LIBRARY_CONV_CALLS[0] == before, "the dilated layer went to the library"
    assert yd.dtype == HALF
    close(yd, yr, 6e-3, "forward")
    close(xd.grad, xr.grad, 1.5e-2, "data gradient")
    close(layer.conv.weight.grad, twin.conv.weight.grad, 1.5e-2, "weight gradient")
    close(layer.conv.bias.grad, twin.conv.bias.grad, 1.5e-2, "bias gradient")


def test_pwcnet_context_network_runs_without_library_calls(gpu_device):
    """context[1..4] of PWCNet (128 -> 128 d=2, 128 -> 128 d=4, 128 -> 96 d=8, 96 -> 64 d=16) chained on a [2, 128, 16, 32]
    tensor, forward + backward under 16-bit autocast: the library-call counter does not move."""
    from xpt_mde_2021_amd.model.build_model.flow_net import PWCNet
    from xpt_mde_2021_amd.model.model_util import layer_ops as lo
    dev = gpu_device
    torch.manual_seed(3)
    net = PWCNet((2, 3, 64, 128, 3), 2, lo.CustomConv2D(activation="leaky_relu", activation_param=0.1,
                                                        kernel_initializer="truncated_normal", kernel_initializer_param=0.025))
    chain = torch.nn.ModuleList(list(net.context[1:5])).to(dev).to(memory_format=torch.channels_last)
    assert [m.d for m in chain] == [2, 4, 8, 16]
    x = torch.randn(2, 128, 16, 32).to(HALF).to(dev).contiguous(memory_format=torch.channels_last).requires_grad_(True)
    before = lo.LIBRARY_CONV_CALLS[0]
    with torch.autocast("cuda", dtype=HALF):
        c = x
        for conv in chain:
            c = conv(c)
    c.float().sum().backward()
    torch.cuda.synchronize()
    assert lo.LIBRARY_CONV_CALLS[0] == before, "a context-network layer went to the library"
    assert c.shape == (2, 64, 16, 32) and c.dtype == HALF
    assert x.grad is not None and bool(torch.isfinite(x.grad.float()).all())
    assert all(m.conv.weight.grad is not None and bool(torch.isfinite(m.conv.weight.grad).all()) for m in chain)


def test_dilation_misuse_is_refused(gpu_device):
    """dilation = 2 with stride 2, with a 5 x 5 weight, or with up-sampling: XptHipError, nothing falls through."""
    from xpt_mde_2021_amd.hip import conv as xc, lib as xl
    dev = gpu_device
    x = torch.randn(1, 8, 8, 8).to(HALF).to(dev).contiguous(memory_format=torch.channels_last)
    w3 = torch.randn(8, 8, 3, 3, device=dev)
    w5 = torch.randn(8, 8, 5, 5, device=dev)
    with pytest.raises(xl.XptHipError):
        xc.conv2d_same(x, w3, None, 2, 1.0, dilation=2)
    with pytest.raises(xl.XptHipError):
        xc.conv2d_same(x, w5, None, 1, 1.0, dilation=2)
    with pytest.raises(xl.XptHipError):
        xc.conv2d_same(x, w3, None, 1, 1.0, upsample=True, dilation=2)
    with pytest.raises(xl.XptHipError):
        xc.conv2d_same(x, w3, None, 1, 1.0, dilation=0)
