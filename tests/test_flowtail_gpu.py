"""PWC-Net's 2-channel layers on the GPU (csrc/xpt_flowtail.hip, hip/flowtail.py): the flow heads Conv2D(2, 3, "same", linear)
and the transposed up-samplers Conv2DTranspose(2, 4, 2, "same"), against the float64 restatement of tests/ref_flowtail.py.

* exact-integer operands (the method of tests/exact_ops.py): x, w in {-1, 0, 1}, g in 2 x {-1, 0, 1}, a small integer bias; every
  result is then an integer that fp32 and both 16-bit formats hold exactly, so y, dx, dW and db are compared with ==;
* random normal operands: every fp32 result within terms x 2^-23 x sum |terms| of the float64 value (fp32 reassociation,
  DESIGN.md section 14), a 16-bit dx within that plus one rounding in the build's format;
* two runs bit-identical; through a GradSink destination the flat gradient is the in-order sum of the kernel's partial rows;
* misuse raises XptHipError; PWCNet routes its 14 two-channel layers here and keeps the library's error level."""
import copy
import ctypes
import functools
import os
import subprocess
import sys

import pytest
import torch

import ref_flowtail as ref
from exact_ops import assert_equal, fits, require_fits, tri, EXACT_F32, FORMATS, MAP_AXES, DW_AXES

from xpt_mde_2021_amd.hip import lib as xl

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HALF = xl.half()
BATCH = 3
MAPS = [(1, 1), (2, 3), (5, 7), (9, 20)]        # every neighbour out of range; tiny; odd + ragged last wave; > 1 wave and partial row
HEAD_C = [16, 32, 128]
UP_CASES = [(2, True), (8, False), (32, False)]  # (C, fp32 input)
CL = torch.channels_last


def _stream():
    return torch.cuda.current_stream().cuda_stream


# ------------------------------------------------------------------------------------------------ operands and references
@functools.lru_cache(maxsize=None)
def exact_reference(op, C, H, W, bias=True):
    """Integer operands and their float64 results; asserts the method's conditions before any device work.  Read-only."""
    gen = torch.Generator().manual_seed(1000 * (op == "head") + 17 * C + 3 * H + W)
    x = tri((BATCH, C, H, W), 0.6, gen)
    w = tri((2, C, 3, 3) if op == "head" else (C, 2, 4, 4), 0.6, gen)
    b = torch.tensor([3.0, -2.0], dtype=torch.float64) if bias else None
    g = tri((BATCH, 2, H, W) if op == "head" else (BATCH, 2, 2 * H, 2 * W), 0.6, gen, 2)
    r = (ref.flow_head if op == "head" else ref.upconv4x4s2)(x, w, b, g)
    what = f"{op} C={C} {H}x{W}"
    for dtype in FORMATS:                        # the 16-bit tensors: exact in bf16 AND in IEEE half
        require_fits({"x": r["x"], "dx": r["dx"]}, dtype, what)
    require_fits({n: r[n] for n in ("w", "b", "g", "y", "dw", "db")}, torch.float32, what)
    # every partial sum of an fp32 accumulation is bounded by the sum of the magnitudes: integers below 2^24
    assert all(float(r["abs"][n].max()) < EXACT_F32 for n in ("y", "dx", "dw", "db")), what
    return r


@functools.lru_cache(maxsize=None)
def normal_reference(op, C, H, W, f32_input=False):
    """Random normal operands, x rounded to the format the operator reads it in; float64 results of the ROUNDED operands."""
    gen = torch.Generator().manual_seed(5000 + 1000 * (op == "head") + 17 * C + 3 * H + W)
    x = torch.randn((BATCH, C, H, W), generator=gen)
    x = (x if f32_input else x.to(HALF)).double()
    wshape = (2, C, 3, 3) if op == "head" else (C, 2, 4, 4)
    w = (torch.randn(wshape, generator=gen) / (9 * C if op == "head" else 4 * C) ** 0.5).double()
    b = (0.1 * torch.randn(2, generator=gen)).double()
    g = torch.randn((BATCH, 2, H, W) if op == "head" else (BATCH, 2, 2 * H, 2 * W), generator=gen).double()
    return (ref.flow_head if op == "head" else ref.upconv4x4s2)(x, w, b, g)


def run(op, r, dev, bias=True, f32_input=False, slice_of=0, weight_format=CL):
    """The operator and its backward on the operands of reference r -> (y, dx, dw, db) on the device."""
    from xpt_mde_2021_amd.hip import flowtail as ft
    xdtype = torch.float32 if f32_input else HALF
    x = r["x"].to(xdtype).to(dev).contiguous(memory_format=CL)
    if slice_of:                                 # channels [8, 8 + C) of a wider channels-last tensor, read in place
        wide = torch.full((x.shape[0], slice_of, x.shape[2], x.shape[3]), 7.0, dtype=xdtype, device=dev).contiguous(memory_format=CL)
        wide[:, 8:8 + x.shape[1]] = x
        x = wide[:, 8:8 + x.shape[1]]
        assert x.stride(3) == slice_of or x.shape[3] == 1
    x = x.detach().requires_grad_(True)
    w = r["w"].float().to(dev).contiguous(memory_format=weight_format).requires_grad_(True)
    b = r["b"].float().to(dev).requires_grad_(True) if (bias and r["b"] is not None) else None
    y = (ft.flow_head if op == "head" else ft.upconv4x4s2)(x, w, b)
    y.backward(r["g"].float().to(dev))
    return y.detach(), x.grad, w.grad, None if b is None else b.grad


def blocks(op, C, H, W, f32_input=False):
    lib = xl.load()
    return lib.xpt_flowhead_bwd_blocks(BATCH, H, W, C) if op == "head" else lib.xpt_upconv4x4s2_bwd_blocks(BATCH, H, W, C, int(f32_input))


def check_exact(op, r, got, what):
    y, dx, dw, db = got
    assert y.dtype == torch.float32 and dw.dtype == torch.float32
    assert_equal(y, r["y"], f"{what}: y", MAP_AXES)
    assert_equal(dx, r["dx"], f"{what}: dx", MAP_AXES)
    assert_equal(dw, r["dw"], f"{what}: dW", DW_AXES if op == "head" else ("cin", "cout", "ky", "kx"))
    if db is not None:
        assert_equal(db, r["db"], f"{what}: db")


# ------------------------------------------------------------------------------------------------ exact integers
@pytest.mark.parametrize("H,W", MAPS)
@pytest.mark.parametrize("C", HEAD_C)
def test_flow_head_equals_the_restatement_on_integers(gpu_device, C, H, W):
    r = exact_reference("head", C, H, W)
    if (H, W) == MAPS[-1]:
        assert blocks("head", C, H, W) > 1, "the largest map must span more than one partial row: enlarge it"
    got = run("head", r, gpu_device)
    assert got[1].dtype == HALF
    check_exact("head", r, got, f"head C={C} {H}x{W}")


@pytest.mark.parametrize("H,W", MAPS)
@pytest.mark.parametrize("C,f32_input", UP_CASES)
def test_upconv_equals_the_restatement_on_integers(gpu_device, C, f32_input, H, W):
    r = exact_reference("up", C, H, W)
    if (H, W) == MAPS[-1]:
        assert blocks("up", C, H, W, f32_input) > 1, "the largest map must span more than one partial row: enlarge it"
    got = run("up", r, gpu_device, f32_input=f32_input)
    assert got[0].shape == (BATCH, 2, 2 * H, 2 * W) and got[1].dtype == (torch.float32 if f32_input else HALF)
    check_exact("up", r, got, f"upconv C={C} fp32={f32_input} {H}x{W}")


@pytest.mark.parametrize("op,C", [("head", 32), ("head", 16), ("up", 32), ("up", 8)])
def test_pitched_channel_slice_input_is_read_in_place(gpu_device, op, C):
    H, W = 5, 7
    r = exact_reference(op, C, H, W)
    check_exact(op, r, run(op, r, gpu_device, slice_of=C + 24), f"{op} C={C} slice of {C + 24}")


@pytest.mark.parametrize("op,C,f32_input", [("head", 32, False), ("up", 2, True), ("up", 32, False)])
def test_without_bias(gpu_device, op, C, f32_input):
    H, W = 5, 7
    r = exact_reference(op, C, H, W, bias=False)
    got = run(op, r, gpu_device, bias=False, f32_input=f32_input)
    assert got[3] is None
    check_exact(op, r, got, f"{op} C={C} no bias")


@pytest.mark.parametrize("op,C,f32_input", [("head", 32, False), ("up", 2, True), ("up", 32, False)])
def test_weight_in_the_other_memory_order_is_permuted_outside_the_kernel(gpu_device, op, C, f32_input):
    H, W = 5, 7
    r = exact_reference(op, C, H, W)
    check_exact(op, r, run(op, r, gpu_device, f32_input=f32_input, weight_format=torch.contiguous_format), f"{op} C={C} NCHW weight")


# ------------------------------------------------------------------------------------------------ random normal operands
def _half_rounding(v):
    """One round-to-nearest of |v| in the build's 16-bit format: half a unit in the last place, 2^-9 (bf16: 8 significand bits)
    or 2^-12 (IEEE half: 11 bits) of the binade's upper end, i.e. at most 2^-8 / 2^-11 of |v|; half subnormals step by 2^-24."""
    return v.abs() * (2.0 ** -8) if HALF == torch.bfloat16 else v.abs() * (2.0 ** -11) + 2.0 ** -25


def check_bounds(r, got, what, dx_is_16bit):
    y, dx, dw, db = got
    worst = {}
    for name, t in (("y", y), ("dx", dx), ("dw", dw), ("db", db)):
        want = r[name]
        bound = r["terms"][name] * 2.0 ** -23 * r["abs"][name]
        if name == "dx" and dx_is_16bit:
            bound = bound + _half_rounding(want.abs() + bound)
        err = (t.detach().double().cpu() - want).abs()
        worst[name] = float((err / (bound + 1e-300)).max())
        print(f"{what}: {name} max |err| {float(err.max()):.3e}, max |ref| {float(want.abs().max()):.3e}, "
              f"largest share of the bound {worst[name]:.3f}")
    assert all(v <= 1.0 for v in worst.values()), (what, worst)


@pytest.mark.parametrize("H,W", MAPS)
@pytest.mark.parametrize("C", HEAD_C)
def test_flow_head_within_the_reassociation_bound(gpu_device, C, H, W):
    r = normal_reference("head", C, H, W)
    check_bounds(r, run("head", r, gpu_device), f"head C={C} {H}x{W}", True)


@pytest.mark.parametrize("H,W", MAPS)
@pytest.mark.parametrize("C,f32_input", UP_CASES)
def test_upconv_within_the_reassociation_bound(gpu_device, C, f32_input, H, W):
    r = normal_reference("up", C, H, W, f32_input)
    check_bounds(r, run("up", r, gpu_device, f32_input=f32_input), f"upconv C={C} fp32={f32_input} {H}x{W}", not f32_input)


@pytest.mark.parametrize("op,C,f32_input", [("head", 32, False), ("head", 128, False), ("up", 2, True), ("up", 32, False)])
def test_two_runs_are_bit_identical(gpu_device, op, C, f32_input):
    r = normal_reference(op, C, 9, 20, f32_input)
    a = run(op, r, gpu_device, f32_input=f32_input)
    b = run(op, r, gpu_device, f32_input=f32_input)
    for name, s, t in zip(("y", "dx", "dw", "db"), a, b):
        assert torch.equal(s, t), (op, C, name)


# ------------------------------------------------------------------------------------------------ the gradient sink
@pytest.mark.parametrize("op,C,f32_input,H,W", [("head", 32, False, 9, 20), ("head", 16, False, 9, 20), ("up", 2, True, 9, 20),
                                                ("up", 8, False, 9, 20), ("up", 32, False, 5, 7)])
def test_flat_gradient_is_the_in_order_sum_of_the_partial_rows(gpu_device, op, C, f32_input, H, W):
    """With flat-gradient destinations on weight and bias the backward returns no tensors and the step's finishing launch
    (ops.grad_sink.flush) writes the gradient: bit for bit the sum, in row order, of the partial rows the kernel writes (2..8
    rows here, which the finishing launch adds in order; read through the C entry point into a buffer of the test's own)."""
    from xpt_mde_2021_amd.hip import flowtail as ft, ops
    dev = gpu_device
    lib = xl.load()
    r = normal_reference(op, C, H, W, f32_input)
    nblk = blocks(op, C, H, W, f32_input)
    assert 2 <= nblk <= 8, nblk
    nw = (18 if op == "head" else 32) * C
    row = nw + 2
    x = r["x"].to(torch.float32 if f32_input else HALF).to(dev).contiguous(memory_format=CL).requires_grad_(True)
    w = r["w"].float().to(dev).contiguous(memory_format=CL).requires_grad_(True)
    b = r["b"].float().to(dev).requires_grad_(True)
    w.flat_grad = torch.full((nw,), float("nan"), device=dev)
    b.flat_grad = torch.full((2,), float("nan"), device=dev)
    g = r["g"].float().to(dev)
    y = (ft.flow_head if op == "head" else ft.upconv4x4s2)(x, w, b)
    y.backward(g)
    ops.grad_sink.flush()
    torch.cuda.synchronize()
    assert w.grad is None and b.grad is None, "with a sink destination autograd gets no parameter gradient"
    # the same launch into the test's own buffer
    part = torch.full((nblk * row,), float("nan"), device=dev)
    gl = g.permute(0, 2, 3, 1).contiguous()
    xl_ = x.detach().permute(0, 2, 3, 1).contiguous()
    wl = w.detach().permute(0, 2, 3, 1).contiguous()
    dx2 = torch.empty_like(xl_)
    if op == "head":
        xl.check(lib.xpt_flowhead_bwd(xl_.data_ptr(), C, wl.data_ptr(), gl.data_ptr(), dx2.data_ptr(), part.data_ptr(), part.numel(),
                                      BATCH, H, W, C, _stream()), "xpt_flowhead_bwd")
    else:
        xl.check(lib.xpt_upconv4x4s2_bwd(xl_.data_ptr(), C, int(f32_input), wl.data_ptr(), gl.data_ptr(), dx2.data_ptr(),
                                         part.data_ptr(), part.numel(), BATCH, H, W, C, _stream()), "xpt_upconv4x4s2_bwd")
    torch.cuda.synchronize()
    rows = part.view(nblk, row).cpu()
    assert bool(torch.isfinite(rows).all()), "every element of every partial row is written"
    total = torch.zeros(row)
    for i in range(nblk):
        total = total + rows[i]
    assert torch.equal(w.flat_grad.cpu(), total[:nw]), "dW through the sink"
    assert torch.equal(b.flat_grad.cpu(), total[nw:]), "db through the sink"
    assert torch.equal(dx2.permute(0, 3, 1, 2), x.grad), "dx is the same launch's"
    bound = r["terms"]["dw"] * 2.0 ** -23 * r["abs"]["dw"]
    dw = total[:nw].view((2, 3, 3, C) if op == "head" else (C, 4, 4, 2)).permute(0, 3, 1, 2).double()
    assert bool(((dw - r["dw"]).abs() <= bound).all())


# ------------------------------------------------------------------------------------------------ misuse
def test_misuse_raises(gpu_device, monkeypatch):
    from xpt_mde_2021_amd.hip import flowtail as ft
    dev = gpu_device
    E = xl.XptHipError
    x32 = torch.zeros(1, 32, 4, 4, dtype=HALF, device=dev).contiguous(memory_format=CL)
    flow = torch.zeros(1, 2, 4, 4, device=dev)
    wh, wu = torch.zeros(2, 32, 3, 3, device=dev), torch.zeros(32, 2, 4, 4, device=dev)
    bad = [lambda: ft.flow_head(x32, torch.zeros(1, 32, 3, 3, device=dev), None),           # weight shape
           lambda: ft.flow_head(x32, torch.zeros(2, 32, 5, 5, device=dev), None),
           lambda: ft.flow_head(x32, wh.to(HALF), None),                                     # weight dtype
           lambda: ft.flow_head(x32.cpu(), wh, None), lambda: ft.flow_head(x32, wh.cpu(), None),   # CPU tensors
           lambda: ft.flow_head(x32.float(), wh, None),                                      # fp32 features
           lambda: ft.flow_head(torch.zeros(1, 24, 4, 4, dtype=HALF, device=dev), torch.zeros(2, 24, 3, 3, device=dev), None),
           lambda: ft.flow_head(x32, wh, torch.zeros(3, device=dev)),                         # bias shape
           lambda: ft.upconv4x4s2(x32, torch.zeros(32, 2, 3, 3, device=dev), None),
           lambda: ft.upconv4x4s2(x32, torch.zeros(2, 32, 4, 4, device=dev), None),
           lambda: ft.upconv4x4s2(x32, wu.double(), None),
           lambda: ft.upconv4x4s2(x32.cpu(), wu, None),
           lambda: ft.upconv4x4s2(x32.float(), wu, None),                                    # fp32 input with 32 channels
           lambda: ft.upconv4x4s2(flow.to(HALF), torch.zeros(2, 2, 4, 4, device=dev), None),  # 16-bit input with 2 channels
           lambda: ft.upconv4x4s2(torch.zeros(1, 64, 4, 4, dtype=HALF, device=dev), torch.zeros(64, 2, 4, 4, device=dev), None),
           lambda: ft.upconv4x4s2(flow.double(), torch.zeros(2, 2, 4, 4, device=dev), None)]
    for i, call in enumerate(bad):
        with pytest.raises(E):
            call()
            pytest.fail(f"misuse {i} was accepted")
    # a weight gradient without a flat-gradient destination must not enter a captured step (its rows would be summed by the
    # framework).  The check reads torch.cuda.is_current_stream_capturing() before anything is launched; it is answered
    # "yes" here instead of opening a capture that the refusal would leave half-recorded.
    for op, x, w in (("head", x32, wh), ("up", flow, torch.zeros(2, 2, 4, 4, device=dev))):
        w = w.clone().requires_grad_(True)
        y = (ft.flow_head if op == "head" else ft.upconv4x4s2)(x, w, None)
        monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
        with pytest.raises(E, match="graph capture"):
            y.sum().backward()
        monkeypatch.undo()


# ------------------------------------------------------------------------------------------------ PWCNet
def _pwcnet(seed=5):
    from xpt_mde_2021_amd.model.build_model.flow_net import PWCNet
    from xpt_mde_2021_amd.model.model_util import layer_ops as lo
    torch.manual_seed(seed)
    net = PWCNet((1, 2, 64, 128, 3), 1, lo.CustomConv2D(activation="leaky_relu", activation_param=0.1,
                                                        kernel_initializer="truncated_normal", kernel_initializer_param=0.025))
    for name, p in net.named_parameters():      # zero biases and ~1e-6 flows hide mistakes: biases of size, flows of ~1 pixel
        if p.dim() == 1:
            torch.nn.init.uniform_(p, -0.1, 0.1)
    for m in _tail_layers(net).values():
        if hasattr(m, "conv"):                  # the heads' TruncatedNormal(0.025) kernels
            with torch.no_grad():
                m.conv.weight.mul_(8.0)
    return net


def _tail_layers(net):
    """The 14 two-channel layers by name: six flow heads, eight transposed up-samplers."""
    out = {}
    for p in (6, 5, 4, 3, 2):
        est = getattr(net, f"flow{p}")
        out[f"flow{p}.out"] = est.out
        if est.up:
            out[f"flow{p}.up_flow"], out[f"flow{p}.up_feat"] = est.up_flow, est.up_feat
    out["context.6"] = net.context[6]
    assert len(out) == 14
    return out


def _frames():
    return torch.rand((1, 2, 64, 128, 3), generator=torch.Generator().manual_seed(9))


def _cotangents():
    gen = torch.Generator().manual_seed(10)
    return [torch.randn((1, 1, 64 >> p, 128 >> p, 2), generator=gen) for p in (2, 3, 4, 5)]


def _forward_backward(net, dev, autocast):
    net.zero_grad(set_to_none=True)
    frames = _frames().to(dev)
    if autocast:
        with torch.autocast("cuda", dtype=HALF):
            flows = net(frames)["flow_ms"]
    else:
        flows = net(frames)["flow_ms"]
    sum((f.float() * c.to(dev)).sum() for f, c in zip(flows, _cotangents())).backward()
    grads = {}
    for name, m in _tail_layers(net).items():
        w, b = (m.conv.weight, m.conv.bias) if hasattr(m, "conv") else (m.weight, m.bias)
        assert w.grad is not None and b.grad is not None, f"{name}: a parameter was left without a gradient"
        grads[name] = torch.cat([w.grad.detach().float().cpu().reshape(-1), b.grad.detach().float().cpu().reshape(-1)])
    return [f.detach().float().cpu() for f in flows], grads


def test_pwcnet_routes_its_two_channel_layers_to_the_own_kernels(gpu_device, monkeypatch):
    """One forward of PWCNet at 64 x 128 under 16-bit autocast goes to the library exactly once per 196-channel layer (encoder
    level 6, the only layers left there); with either A/B switch on it goes there more often; every head and up-sampler
    parameter receives a gradient."""
    from xpt_mde_2021_amd.model.build_model import flow_net as fn
    from xpt_mde_2021_amd.model.model_util import layer_ops as lo
    dev = gpu_device
    net = _pwcnet().to(dev).to(memory_format=CL)
    n196 = sum(1 for m in net.modules() if isinstance(m, lo.Conv2DSame) and m.conv.out_channels == 196)
    assert n196 == 6

    def forward_calls():
        before = lo.LIBRARY_CONV_CALLS[0]
        with torch.autocast("cuda", dtype=HALF):
            out = net(_frames().to(dev))["flow_ms"]
        torch.cuda.synchronize()
        assert all(f.dtype == torch.float32 and bool(torch.isfinite(f).all()) for f in out)
        return lo.LIBRARY_CONV_CALLS[0] - before

    assert forward_calls() == n196
    monkeypatch.setattr(fn, "_LIBRARY_FLOWHEAD", True)
    assert forward_calls() > n196
    monkeypatch.setattr(fn, "_LIBRARY_FLOWHEAD", False)
    monkeypatch.setattr(fn, "_LIBRARY_UPCONV", True)
    assert forward_calls() > n196
    monkeypatch.setattr(fn, "_LIBRARY_UPCONV", False)
    _forward_backward(net, dev, True)            # asserts a gradient on all 28 parameters


def test_pwcnet_keeps_the_library_routes_error_level(gpu_device, monkeypatch):
    """flow_ms and the 14 layers' parameter gradients (each bias with its kernel) against the same module in fp32 on the CPU:
    per tensor the own route's error is at most twice the library route's (both switches on) -- the rule of DESIGN.md
    section 13, in that rule's metric: relative L2 (tests/test_depthnet_basic_gpu.py _rel_l2).  A first version of this test
    took the largest |difference| over the largest |reference| instead; on a 2-pixel map that is a single draw of bf16 noise
    (flow6.up_flow read 1.03e-2 own against 4.50e-3 library, flow4.up_flow 1.75e-2 against 6.45e-2, on one MI355X).
    Measured in relative L2 (bf16): all four flows closer to fp32 on the own route, largest gradient ratio 1.70 at
    flow3.up_feat (7.06e-2 / 4.16e-2); the table is in DESIGN.md section 16."""
    from xpt_mde_2021_amd.model.build_model import flow_net as fn
    dev = gpu_device
    cpu_net = _pwcnet()
    gpu_net = copy.deepcopy(cpu_net).to(dev).to(memory_format=CL)
    ref_flows, ref_grads = _forward_backward(cpu_net, torch.device("cpu"), False)
    own = _forward_backward(gpu_net, dev, True)
    monkeypatch.setattr(fn, "_LIBRARY_FLOWHEAD", True)
    monkeypatch.setattr(fn, "_LIBRARY_UPCONV", True)
    library = _forward_backward(gpu_net, dev, True)

    def share(got, want):
        return float((got.double() - want.double()).norm() / want.double().norm().clamp_min(1e-300))

    rows = [(f"flow_ms[{i}]", share(own[0][i], ref_flows[i]), share(library[0][i], ref_flows[i])) for i in range(4)]
    rows += [(name, share(own[1][name], ref_grads[name]), share(library[1][name], ref_grads[name])) for name in ref_grads]
    for name, e_own, e_lib in rows:
        print(f"{name:18s} own {e_own:.3e}   library {e_lib:.3e}")
    worse = [(n, a, b) for n, a, b in rows if not a <= 2.0 * b]
    assert not worse, worse


# ------------------------------------------------------------------------------------------------ the IEEE-half build
def test_kernel_tests_pass_on_the_half_precision_build(gpu_device):
    """libxpt_hip_f16.so compiles the same file; one 16-bit format per process, so the operator tests of this file run once more
    in a child process with XPT_HALF=fp16 (the mechanism of tests/test_fp16_build_gpu.py)."""
    if os.environ.get("XPT_HALF") == "fp16":
        return                                   # this IS the child
    run_ = subprocess.run([sys.executable, "-m", "pytest", "tests/test_flowtail_gpu.py", "-m", "gpu", "-q", "-p", "no:cacheprovider",
                           "-k", "not pwcnet and not half_precision_build"], cwd=ROOT, capture_output=True, text=True, timeout=600,
                          env=dict(os.environ, XPT_HALF="fp16"))
    tail = (run_.stdout + run_.stderr)[-3000:]
    assert run_.returncode == 0, tail
    assert " passed" in run_.stdout and "failed" not in run_.stdout.splitlines()[-1], tail
