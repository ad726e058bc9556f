"""Exact-integer parity of the dense (xc.conv2d_same, xc.head_conv) and depthwise (ops.depthwise_conv2d) convolutions: operands
are small integers chosen so that every value a kernel stores -- y, g = dy * act'(y), the bilinear path's scratch gradient and dx
in 16 bits; dW, db and the split partials in fp32 -- is exactly representable (tests/exact_ops.py asserts that on the fp64
reference before any device work).  Then every correct kernel gives the SAME values in any summation order, split count or
workgroup numbering, and a dropped, duplicated or mis-indexed term changes some element by at least 1: results are compared
with ==, no tolerance anywhere.  tests/test_conv_exact_cpu.py shows what this catches that the "fraction of the largest
magnitude" bars of tests/test_conv_igemm_gpu.py cannot (DESIGN.md "Exact-integer parity")."""
import pytest
import torch
import torch.nn.functional as F

from tests import exact_ops as ex
from tests.conv_plans import PLANS, conv_plan  # noqa: F401  (the plan-forcing fixture of tests/test_conv_igemm_gpu.py)
from tests.exact_ops import ConvCase

pytestmark = pytest.mark.gpu

# ---- PoseNetImproved / decoder layers (tests/test_conv_igemm_gpu.py SHAPES) on the smallest maps that still span two tiles plus a
# ragged remainder in each direction (8 x 16-pixel tiles), odd H and W (one even H at stride 2), batch 3
PRODUCT = [
    ConvCase(1056, 256, 3, 1, 4, 13, "nearest"), ConvCase(432, 256, 3, 1, 8, 26), ConvCase(256, 256, 3, 2, 4, 13),
    ConvCase(256, 256, 3, 1, 2, 7), ConvCase(256, 24, 1, 1, 2, 7, slope=1.0),
    ConvCase(15, 32, 5, 2, 19, 45), ConvCase(32, 32, 5, 2, 18, 35), ConvCase(32, 64, 3, 2, 17, 27),
    ConvCase(64, 128, 3, 2, 9, 21), ConvCase(216, 128, 3, 1, 9, 21), ConvCase(128, 64, 3, 1, 9, 19, "nearest"),
    ConvCase(87, 64, 3, 1, 17, 35), ConvCase(65, 32, 3, 1, 19, 37), ConvCase(32, 16, 3, 1, 11, 21, "nearest"),
    ConvCase(17, 16, 3, 1, 25, 49),
]
# ---- batch 8: the tile count AND the split count of conv_wgrad_fast_kernel are multiples of 8 (its XCD-renumbered branch), the
# grids of the LDS-staged / halo-tile kernels are multiples of 8 with at least 64 workgroups (xpt_xcd_remap)
XCD = [ConvCase(17, 16, 3, 1, 25, 49, batch=8), ConvCase(32, 16, 3, 1, 11, 21, "nearest", batch=8),
       ConvCase(32, 64, 3, 2, 17, 27, batch=8), ConvCase(15, 32, 5, 2, 19, 45, batch=8)]
# ---- modes the plan fixture does not reach
BILINEAR = [ConvCase(64, 32, 3, 1, 5, 7, "bilinear", xs=16, gs=32, wd=0.08, gd=0.03),
            ConvCase(24, 16, 3, 1, 9, 11, "bilinear", xs=16, gs=32, wd=0.1, gd=0.04)]
MODES = BILINEAR + [
    ConvCase(3, 32, 7, 1, 17, 35), ConvCase(32, 32, 7, 2, 17, 35),                        # DepthNetBasic dp_conv0b / dp_conv1a
    ConvCase(32, 32, 7, 2, 18, 36, slope=1.0),
    ConvCase(64, 64, 3, 2, 18, 34, pad=1), ConvCase(3, 64, 7, 2, 18, 34, pad=3),          # keras ZeroPadding2D + VALID, even extent
    ConvCase(64, 64, 3, 1, 17, 35, pad=1),                                                # (= SAME at stride 1: the specialised paths)
    ConvCase(3, 8, 3, 2, 19, 37, valid=True), ConvCase(3, 32, 3, 2, 19, 37, valid=True),  # the stem: 3 -> 8 padded input channels
    ConvCase(32, 16, 3, 1, 17, 35, slice_of=48), ConvCase(20, 16, 3, 1, 9, 21, slice_of=40),
    ConvCase(32, 32, 3, 1, 19, 37, dilation=2), ConvCase(40, 16, 3, 1, 17, 35, dilation=4),
    ConvCase(32, 32, 3, 1, 13, 37, dilation=16), ConvCase(16, 8, 3, 1, 9, 11, dilation=16),   # d >= H (and d >= W)
]
LINEAR = [ConvCase(**{**c.__dict__, "slope": 1.0}) for c in (PRODUCT[0], PRODUCT[5], PRODUCT[7], PRODUCT[11], PRODUCT[14], BILINEAR[1])]
SINK = [PRODUCT[13], PRODUCT[14], PRODUCT[7], PRODUCT[5], PRODUCT[4], BILINEAR[0], MODES[2], MODES[12]]
ALL_CONV_CASES = PRODUCT + XCD + MODES + LINEAR
HEADS = [(16, 19, 37), (128, 5, 13)]

# 3 x 3 stride-1 layers the persistent weight-stationary family serves under the 6000 plans, forward and data gradient (whose output
# channels are the layer's INPUT channels): the decoder's two last levels.  (87 -> 64: its 96-channel halo exceeds the staging
# registers; 128 -> 64 and deeper: the weight slab exceeds the LDS; more than 96 output channels: no instantiation.)
STREAM_FWD = {str(c) for c in PRODUCT + XCD if c.k == 3 and c.stride == 1 and c.cout <= 32}
STREAM_FWD_K5 = {str(c) for c in PRODUCT + XCD if c.k == 5}                                 # (6001 / 6003: the 5 x 5 stride-2 kernel)


def _geometry(case):
    grow = 2 if case.ups else 1
    H, W = case.H * grow, case.W * grow
    if case.pad is not None:
        return (H + 2 * case.pad - case.k) // case.stride + 1, (W + 2 * case.pad - case.k) // case.stride + 1
    if case.valid:
        return (H - case.k) // case.stride + 1, (W - case.k) // case.stride + 1
    return -(-H // case.stride), -(-W // case.stride)


def _assert_family(lib, case, plan):
    """Where the library answers which family serves a call, a forced plan must not have fallen through to another one."""
    B, N, C, k, s = case.batch, case.cout, case.cin, case.k, case.stride
    cp = ex.round_up(C, 8)
    OH, OW = _geometry(case)
    ups = 1 if case.ups == "nearest" else 0
    plain = case.dilation == 1 and case.ups != "bilinear" and not case.valid and case.pad is None
    if 5000 <= plan < 6000 and plain and s == 1:
        assert lib.xpt_conv2d_splitk_workspace_floats(B * OH * OW, N, cp, k * k, s) > 0, f"{case}: split-K forward not served"
        assert lib.xpt_conv2d_splitk_workspace_floats(B * OH * OW, cp, ex.round_up(N, 8), k * k, s) > 0, \
            f"{case}: split-K data gradient not served"
    if 6000 <= plan < 7000 and plain:
        serves = lib.xpt_conv2d_stream_serves(B, OH, OW, N, cp, k, k, s, ups)
        want = str(case) in STREAM_FWD or (plan < 6100 and str(case) in STREAM_FWD_K5)
        assert bool(serves) == want, f"{case} plan {plan}: persistent forward serves = {serves}, expected {want}"
        if str(case) in STREAM_FWD:
            assert lib.xpt_conv2d_stream_serves(B, OH, OW, cp, ex.round_up(N, 8), k, k, s, ups), f"{case}: persistent data gradient"
    if plain and ((k == 3 and s in (1, 2)) or (k == 5 and s == 2)):
        # conv_wgrad_fast_kernel: three workgroups per CU over the 32 x 32 channel blocks, whole groups of eight from 16 splits on
        ntiles = B * (-(-OH // 8)) * (-(-OW // 16))
        blocks = (-(-cp // 32)) * (-(-N // 32))
        nsplit = min(-(-768 // blocks), (12 << 20) // (N * k * k * cp * 4), ntiles)
        nsplit = max(nsplit & ~7 if nsplit >= 16 else nsplit, 1)
        if ntiles >= (2 if plan == 7002 else 1):
            got = lib.xpt_conv2d_bwd_weight_splits(B, cp, N, k, k, s, OH, OW)
            assert got == nsplit, f"{case}: {got} weight-gradient splits, the specialised kernel's plan has {nsplit}"
            if case.batch == 8:
                assert ntiles % 8 == 0 and nsplit % 8 == 0, f"{case}: {ntiles} tiles, {nsplit} splits: not the XCD-renumbered branch"


def _device_operands(case, ref, dev):
    """x [B, Cp, H, W] (channels padded to 8 with zeros; a channel slice of a wider tensor for case.slice_of), w, b, gy on the
    device in the process's 16-bit format / fp32."""
    HALF = ex.half()
    cp = ex.round_up(case.cin, 8)
    x = F.pad(ref["x"], (0, 0, 0, 0, 0, cp - case.cin)).to(HALF)
    if case.slice_of:
        gen = torch.Generator().manual_seed(case.slice_of)
        wide = ex.tri((case.batch, case.slice_of, case.H, case.W), 0.5, gen).to(HALF)       # live neighbours on both sides
        wide[:, 8:8 + cp] = x
        wide = wide.to(dev).contiguous(memory_format=torch.channels_last)
        xd = wide[:, 8:8 + cp].detach().requires_grad_(True)
        assert not xd.is_contiguous(memory_format=torch.channels_last)
    else:
        xd = x.to(dev).contiguous(memory_format=torch.channels_last).requires_grad_(True)
    wd = ref["w"].float().to(dev).contiguous(memory_format=torch.channels_last).requires_grad_(True)
    bd = ref["b"].float().to(dev).requires_grad_(True)
    return xd, wd, bd, ref["gy"].to(HALF).to(dev)


def _call(xc, case, xd, wd, bd):
    return xc.conv2d_same(xd, wd, bd, case.stride, case.slope, case.ups or False, valid=case.valid, pad=case.pad,
                          dilation=case.dilation)


def _check_conv(xc, dev, case):
    ref = ex.conv_reference(case)                     # (asserts the method's conditions before anything runs on the device)
    xd, wd, bd, gy = _device_operands(case, ref, dev)
    yd = _call(xc, case, xd, wd, bd)
    assert yd.dtype == ex.half()
    yd.backward(gy)
    torch.cuda.synchronize()
    ex.assert_equal(yd, ref["y"], f"{case}: y", ex.MAP_AXES)
    ex.assert_equal(xd.grad[:, :case.cin], ref["dx"], f"{case}: dx", ex.MAP_AXES)
    ex.assert_equal(xd.grad[:, case.cin:], torch.zeros_like(xd.grad[:, case.cin:], device="cpu"), f"{case}: dx pad channels",
                    ex.MAP_AXES)
    assert wd.grad.dtype == torch.float32 and bd.grad.dtype == torch.float32
    ex.assert_equal(wd.grad, ref["dw"], f"{case}: dW", ex.DW_AXES)
    ex.assert_equal(bd.grad, ref["db"], f"{case}: db", ("cout",))


@pytest.mark.parametrize("plan", PLANS)
@pytest.mark.parametrize("case", PRODUCT + XCD, ids=str)
def test_conv_equals_fp64_reference_under_every_plan(gpu_device, conv_plan, case, plan):
    from xpt_mde_2021_amd.hip import conv as xc, lib as _lib
    conv_plan(plan)
    _assert_family(_lib.load(), case, plan)
    _check_conv(xc, gpu_device, case)


@pytest.mark.parametrize("case", MODES + LINEAR, ids=str)
def test_conv_modes_equal_fp64_reference(gpu_device, conv_plan, case):
    """Bilinear-2x input, 7 x 7, explicit padding, VALID stem, channel-slice input, dilation; slope 1.0 (no saved y)."""
    from xpt_mde_2021_amd.hip import conv as xc
    conv_plan(0)
    _check_conv(xc, gpu_device, case)


@pytest.mark.parametrize("case", [PRODUCT[7], PRODUCT[12], PRODUCT[14], XCD[0]], ids=str)
def test_general_weight_gradient_kernel_equals_fp64_reference(gpu_device, conv_plan, case):
    """conv_wgrad_kernel on the 3 x 3 layers the specialised kernel takes away from it in every plan (it keeps 1 x 1, 7 x 7, the
    bilinear mode and dilation, covered above)."""
    from xpt_mde_2021_amd.hip import conv as xc, lib as _lib
    lib = _lib.load()
    conv_plan(0)
    _lib.check(lib.xpt_conv2d_bwd_weight_tune(-1000, 0), "wgrad tune")         # (the fixture's teardown switches it on again)
    _check_conv(xc, gpu_device, case)


@pytest.mark.parametrize("case", SINK, ids=str)
def test_conv_weight_gradient_through_the_flat_parameter_sink(gpu_device, case):
    """The deferred destination (FlatParameters + ops.grad_sink.flush()): dW and db in the flat gradient buffer equal the
    reference -- not merely the plain sum's result."""
    from xpt_mde_2021_amd.hip import conv as xc, ops
    from xpt_mde_2021_amd.model.model_util.optimizers import FlatParameters
    dev = gpu_device
    ref = ex.conv_reference(case)
    conv = torch.nn.Conv2d(case.cin, case.cout, case.k, bias=True)
    with torch.no_grad():
        conv.weight.copy_(ref["w"].float())
        conv.bias.copy_(ref["b"].float())
    conv = conv.to(dev).to(memory_format=torch.channels_last)
    flat = FlatParameters([conv.weight, conv.bias])
    assert hasattr(conv.weight, "flat_grad") and hasattr(conv.bias, "flat_grad")
    xd, _, _, gy = _device_operands(case, ref, dev)
    with torch.autocast("cuda", dtype=ex.half()):
        yd = _call(xc, case, xd, conv.weight, conv.bias)
    yd.backward(gy)
    ops.grad_sink.flush()
    flat.gather_grads()
    torch.cuda.synchronize()
    ex.assert_equal(yd, ref["y"], f"{case}: y", ex.MAP_AXES)
    ex.assert_equal(xd.grad[:, :case.cin], ref["dx"], f"{case}: dx", ex.MAP_AXES)
    ex.assert_equal(flat.grad_views[0], ref["dw"], f"{case}: dW in the flat buffer", ex.DW_AXES)
    ex.assert_equal(flat.grad_views[1], ref["db"], f"{case}: db in the flat buffer", ("cout",))


@pytest.mark.parametrize("C,H,W", HEADS)
def test_head_conv_equals_fp64_reference(gpu_device, C, H, W):
    """xc.head_conv: y, dW, db exact in fp32 (integer fp32 weights on integer features), dx exact in 16 bits."""
    from xpt_mde_2021_amd.hip import conv as xc
    dev = gpu_device
    ref = ex.head_reference(C, H, W)
    xd = ref["x"].to(ex.half()).to(dev).contiguous(memory_format=torch.channels_last).requires_grad_(True)
    wd = ref["w"].float().to(dev).contiguous(memory_format=torch.channels_last).requires_grad_(True)
    bd = ref["b"].float().to(dev).requires_grad_(True)
    yd = xc.head_conv(xd, wd, bd)
    assert yd.dtype == torch.float32
    yd.backward(ref["gy"].float().to(dev))
    torch.cuda.synchronize()
    ex.assert_equal(yd, ref["y"], f"head {C}: y", ex.MAP_AXES)
    assert xd.grad.dtype == ex.half()
    ex.assert_equal(xd.grad, ref["dx"], f"head {C}: dx", ex.MAP_AXES)
    ex.assert_equal(wd.grad, ref["dw"], f"head {C}: dW", ex.DW_AXES)
    ex.assert_equal(bd.grad, ref["db"], f"head {C}: db", ("cout",))


# ------------------------------------------------------------------------------------------------ depthwise
DW_MAP = (3, 40, 19, 37)            # 8-channel groups, odd extents, above the small-map limit of 256 pixels
DW_C22 = (3, 22, 19, 37)            # 22 channels: 2-channel groups (no 8- or 4-vector)
DW_V2 = (1, 22, 21, 33)             # V = 2 vectors, odd extents, one image
DW_SHAPES = [DW_MAP, DW_C22, DW_V2]
# xpt_dwconv_tune codes.  "tiles": the LDS-staged tile kernels on these small maps -- stride-2 forward from 2^0 input elements on
# (-50000), stride-1 backward tiles on (-70001); "scalar": tile kernels and the vectorised stride-2 data gradient off
DW_TUNES = {"default": [], "tiles": [-50000, -70001], "scalar": [-20000, -30000, -3]}
DW_RESTORE = [-50021, -70000, -21616, -30001, -4]


@pytest.fixture
def dw_tune():
    from xpt_mde_2021_amd.hip import lib as _lib
    lib = _lib.load()

    def apply(name):
        for code in DW_TUNES[name]:
            _lib.check(lib.xpt_dwconv_tune(code), "xpt_dwconv_tune")

    yield apply
    for code in DW_RESTORE:
        lib.xpt_dwconv_tune(code)


@pytest.mark.parametrize("tune", list(DW_TUNES))
@pytest.mark.parametrize("shape", DW_SHAPES, ids=lambda s: "x".join(str(v) for v in s))
@pytest.mark.parametrize("k,stride", [(3, 1), (5, 1), (7, 1), (3, 2), (5, 2), (7, 2)])
@pytest.mark.parametrize("fmt", ["fp32", "half"])
@pytest.mark.parametrize("relu_in", [False, True])
def test_depthwise_equals_fp64_reference(gpu_device, dw_tune, k, stride, shape, fmt, relu_in, tune):
    """The exact counterpart of tests/test_hip_parity.py::test_depthwise_conv_fwd_bwd: y, dx and dW (a sum of integers in fp32)
    with ==, through the plain weight-gradient destination and through the FlatParameters sink (one launch for both gradients)."""
    from xpt_mde_2021_amd.hip import ops
    from xpt_mde_2021_amd.model.model_util.optimizers import FlatParameters
    dev = gpu_device
    dtype = torch.float32 if fmt == "fp32" else ex.half()
    ref = ex.depthwise_reference(k, stride, shape, relu_in)
    dw_tune(tune)
    for sink in (False, True):
        xg = ref["x"].to(dtype).to(dev).contiguous(memory_format=torch.channels_last).requires_grad_(True)
        wg = torch.nn.Parameter(ref["w"].float().to(dev))
        flat = FlatParameters([wg]) if sink else None
        assert hasattr(wg, "flat_grad") == sink
        y = ops.depthwise_conv2d(xg, wg, stride, ref["pads"], relu_in)
        assert y.dtype == dtype
        y.backward(ref["gy"].to(dtype).to(dev))
        if sink:
            ops.grad_sink.flush()
            flat.gather_grads()
        torch.cuda.synchronize()
        what = f"depthwise k{k} s{stride} {shape} {fmt} relu_in={relu_in} {tune} sink={sink}"
        ex.assert_equal(y, ref["y"], what + ": y", ex.MAP_AXES)
        ex.assert_equal(xg.grad, ref["dx"], what + ": dx", ex.MAP_AXES)
        ex.assert_equal(flat.grad_views[0] if sink else wg.grad, ref["dw"], what + ": dW", ("c", "one", "kh", "kw"))
