"""PWC-Net's 2-channel layers (csrc/xpt_flowtail.hip, hip/flowtail.py) without a GPU: the float64 restatement the GPU tests
compare against equals the framework's operators and their autograd, the `*_usable` predicates admit exactly what the kernels
serve, and the C entry points refuse bad arguments before any launch, through both builds of the library."""
import ctypes
import os
import types

import pytest
import torch
import torch.nn.functional as F

import ref_flowtail as ref

SHAPES = [(1, 1), (2, 3), (5, 7), (4, 6)]


def _operands(shape_x, shape_w, out_hw, seed, bias=True):
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(shape_x, generator=gen, dtype=torch.float64)
    w = torch.randn(shape_w, generator=gen, dtype=torch.float64)
    b = torch.randn(2, generator=gen, dtype=torch.float64) if bias else None
    g = torch.randn((shape_x[0], 2, *out_hw), generator=gen, dtype=torch.float64)
    return x, w, b, g


def _autograd(fn, x, w, b, g):
    x, w = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
    b = None if b is None else b.clone().requires_grad_(True)
    y = fn(x, w, b)
    y.backward(g)
    return y.detach(), x.grad, w.grad, None if b is None else b.grad


def _check(r, y, dx, dw, db, what):
    for name, want in (("y", y), ("dx", dx), ("dw", dw), ("db", db)):
        if want is None:
            continue
        got = r[name]
        assert got.shape == want.shape, (what, name)
        tol = 1e-12 * (1.0 + float(r["abs"][name].max()))
        assert float((got - want).abs().max()) <= tol, (what, name, float((got - want).abs().max()))
        assert bool((r["abs"][name] + 1e-12 >= got.abs()).all()), (what, name, "sum of magnitudes below the magnitude of the sum")


@pytest.mark.parametrize("C", [1, 3, 16])
@pytest.mark.parametrize("H,W", SHAPES)
@pytest.mark.parametrize("bias", [True, False])
def test_flow_head_restatement_equals_conv2d_and_its_autograd(C, H, W, bias):
    x, w, b, g = _operands((3, C, H, W), (2, C, 3, 3), (H, W), 11 * C + H, bias)
    r = ref.flow_head(x, w, b, g)
    y, dx, dw, db = _autograd(lambda x_, w_, b_: F.conv2d(x_, w_, b_, 1, 1), x, w, b, g)
    _check(r, y, dx, dw, db if bias else g.sum(dim=(0, 2, 3)), f"head C={C} {H}x{W}")
    assert r["terms"] == {"y": 9 * C + bias, "dx": 18, "dw": 3 * H * W, "db": 3 * H * W}


@pytest.mark.parametrize("C", [1, 2, 8])
@pytest.mark.parametrize("H,W", SHAPES)
@pytest.mark.parametrize("bias", [True, False])
def test_upconv_restatement_equals_conv_transpose2d_and_its_autograd(C, H, W, bias):
    x, w, b, g = _operands((3, C, H, W), (C, 2, 4, 4), (2 * H, 2 * W), 13 * C + W, bias)
    r = ref.upconv4x4s2(x, w, b, g)
    y, dx, dw, db = _autograd(lambda x_, w_, b_: F.conv_transpose2d(x_, w_, b_, 2, 1), x, w, b, g)
    assert y.shape == (3, 2, 2 * H, 2 * W)
    _check(r, y, dx, dw, db if bias else g.sum(dim=(0, 2, 3)), f"upconv C={C} {H}x{W}")
    assert r["terms"] == {"y": 4 * C + bias, "dx": 32, "dw": 3 * H * W, "db": 12 * H * W}


def test_upconv_restatement_phase_table():
    """The per-phase reading of the sum: even output rows take ky = 1 from input row iy and ky = 3 from iy - 1, odd rows ky = 2
    from iy and ky = 0 from iy + 1 (the same in x) -- checked with a one-hot weight per tap."""
    x = torch.arange(1.0, 13.0, dtype=torch.float64).view(1, 1, 3, 4)
    g = torch.zeros(1, 2, 6, 8, dtype=torch.float64)
    taps = {0: (1, 1), 1: (0, 0), 2: (1, 0), 3: (0, -1)}               # k -> (output phase, input offset)
    for ky, (py, dr) in taps.items():
        for kx, (px, dc) in taps.items():
            w = torch.zeros(1, 2, 4, 4, dtype=torch.float64)
            w[0, 1, ky, kx] = 1.0
            y = ref.upconv4x4s2(x, w, None, g)["y"]
            assert float(y[:, 0].abs().max()) == 0.0
            for iy in range(3):
                for ix in range(4):
                    src = x[0, 0, iy + dr, ix + dc] if 0 <= iy + dr < 3 and 0 <= ix + dc < 4 else 0.0
                    assert float(y[0, 1, 2 * iy + py, 2 * ix + px]) == float(src), (ky, kx, iy, ix)
            other = torch.ones(6, 8, dtype=torch.bool)
            other[py::2, px::2] = False
            assert float(y[0, 1][other].abs().max()) == 0.0, (ky, kx)


# ------------------------------------------------------------------------------------------------ the predicates
def _conv(cin=32, cout=2, k=(3, 3), stride=(1, 1), dilation=(1, 1), groups=1, dtype=torch.float32):
    return types.SimpleNamespace(in_channels=cin, out_channels=cout, kernel_size=k, stride=stride, dilation=dilation, groups=groups,
                                 weight=torch.zeros(1, dtype=dtype))


class _FakeCuda:
    """A stand-in with the attributes the predicates read: the truth tables run without a device."""

    def __init__(self, shape, dtype, is_cuda=True):
        self.shape, self.dtype, self.is_cuda = torch.Size(shape), dtype, is_cuda

    def dim(self):
        return len(self.shape)


@pytest.fixture
def as_tensors(monkeypatch):
    """torch.is_tensor accepts the stand-ins; autocast reads as enabled in the library's 16-bit format unless a test says so."""
    from xpt_mde_2021_amd.hip import lib as xl
    state = {"enabled": True, "dtype": xl.half()}
    real = torch.is_tensor
    monkeypatch.setattr(torch, "is_tensor", lambda t: isinstance(t, _FakeCuda) or real(t))
    monkeypatch.setattr(torch, "is_autocast_enabled", lambda *a: state["enabled"])
    monkeypatch.setattr(torch, "get_autocast_dtype", lambda *a: state["dtype"])
    return state


def test_flow_head_usable_truth_table(as_tensors):
    from xpt_mde_2021_amd.hip import flowtail as ft, lib as xl
    half = xl.half()
    x = _FakeCuda((4, 32, 8, 12), half)
    assert ft.flow_head_usable(x, _conv()) is True
    for C in (16, 64, 128):
        assert ft.flow_head_usable(_FakeCuda((4, C, 8, 12), half), _conv(cin=C))
    assert ft.flow_head_usable(_FakeCuda((4, 32, 8, 12), torch.float32), _conv())          # autocast supplies the format
    assert not ft.flow_head_usable(_FakeCuda((4, 32, 8, 12), half, is_cuda=False), _conv())  # the CPU path
    assert not ft.flow_head_usable(torch.zeros(4, 32, 8, 12), _conv())
    assert not ft.flow_head_usable(x, _conv(cout=1)) and not ft.flow_head_usable(x, _conv(cout=8))
    assert not ft.flow_head_usable(_FakeCuda((4, 24, 8, 12), half), _conv(cin=24))         # unsupported C
    assert not ft.flow_head_usable(_FakeCuda((4, 196, 8, 12), half), _conv(cin=196))
    assert not ft.flow_head_usable(_FakeCuda((4, 40, 8, 12), half), _conv(cin=32))         # a padded tensor is not the layer's input
    assert not ft.flow_head_usable(x, _conv(k=(1, 1))) and not ft.flow_head_usable(x, _conv(k=(5, 5)))
    assert not ft.flow_head_usable(x, _conv(stride=(2, 2))) and not ft.flow_head_usable(x, _conv(dilation=(2, 2)))
    assert not ft.flow_head_usable(x, _conv(groups=2))
    assert not ft.flow_head_usable(x, _conv(dtype=torch.bfloat16))                         # no fp32 master weight
    as_tensors["enabled"] = False                                                           # fp32 mode
    assert not ft.flow_head_usable(_FakeCuda((4, 32, 8, 12), torch.float32), _conv())
    as_tensors["enabled"], as_tensors["dtype"] = True, (torch.float16 if half == torch.bfloat16 else torch.bfloat16)
    assert not ft.flow_head_usable(_FakeCuda((4, 32, 8, 12), torch.float32), _conv())      # the other 16-bit format


def test_upconv_usable_truth_table(as_tensors):
    from xpt_mde_2021_amd.hip import flowtail as ft, lib as xl
    half = xl.half()
    w = lambda C, dtype=torch.float32: _FakeCuda((C, 2, 4, 4), dtype)      # noqa: E731
    flow, feat = _FakeCuda((4, 2, 8, 12), torch.float32), _FakeCuda((4, 32, 8, 12), half)
    assert ft.upconv_usable(flow, w(2)) is True and ft.upconv_usable(feat, w(32)) is True
    assert ft.upconv_usable(_FakeCuda((4, 8, 8, 12), half), w(8)) and ft.upconv_usable(_FakeCuda((4, 16, 8, 12), half), w(16))
    assert not ft.upconv_usable(_FakeCuda((4, 2, 8, 12), half), w(2))              # the 16-bit path starts at 8 channels
    assert not ft.upconv_usable(_FakeCuda((4, 32, 8, 12), torch.float32), w(32))   # fp32 input is the 2-channel flow only
    assert not ft.upconv_usable(_FakeCuda((4, 64, 8, 12), half), w(64)) and not ft.upconv_usable(_FakeCuda((4, 24, 8, 12), half), w(24))
    assert not ft.upconv_usable(feat, w(16)) and not ft.upconv_usable(feat, _FakeCuda((32, 2, 3, 3), torch.float32))
    assert not ft.upconv_usable(feat, _FakeCuda((32, 4, 4, 4), torch.float32))
    assert not ft.upconv_usable(feat, w(32, half))                                  # no fp32 master weight
    assert not ft.upconv_usable(_FakeCuda((4, 32, 8, 12), half, is_cuda=False), w(32))
    assert not ft.upconv_usable(torch.zeros(4, 2, 8, 12), torch.zeros(2, 2, 4, 4))   # the CPU path
    as_tensors["enabled"] = False
    assert not ft.upconv_usable(flow, w(2)) and not ft.upconv_usable(feat, w(32))   # fp32 mode keeps the framework path
    as_tensors["enabled"], as_tensors["dtype"] = True, (torch.float16 if half == torch.bfloat16 else torch.bfloat16)
    assert not ft.upconv_usable(flow, w(2))


def test_library_switches_are_module_flags_read_at_call_time():
    from xpt_mde_2021_amd.model.build_model import flow_net as fn
    assert fn._LIBRARY_FLOWHEAD is (os.environ.get("XPT_DEBUG_LIBRARY_FLOWHEAD", "0") == "1")
    assert fn._LIBRARY_UPCONV is (os.environ.get("XPT_DEBUG_LIBRARY_UPCONV", "0") == "1")


# ------------------------------------------------------------------------------------------------ the C ABI
NULL_, SHAPE, ARG, WORKSPACE = -1, -2, -3, -4


def _libraries():
    import __graft_entry__ as ge
    from xpt_mde_2021_amd.hip import lib as xl
    if not (os.path.isfile(xl.LIB_PATH) and os.path.isfile(xl.LIB_PATH_F16)):
        ge.build()
    names = ("xpt_flowhead_bwd_blocks", "xpt_flowhead_fwd", "xpt_flowhead_bwd", "xpt_upconv4x4s2_bwd_blocks",
             "xpt_upconv4x4s2_fwd", "xpt_upconv4x4s2_bwd")
    for path in (xl.LIB_PATH, xl.LIB_PATH_F16):
        lib = ctypes.CDLL(path)
        fn = {}
        for name in names:
            fn[name] = getattr(lib, name)
            fn[name].restype, fn[name].argtypes = xl.SIGNATURES[name]
        yield path, fn


def test_entry_points_reject_bad_arguments_before_any_launch_through_both_libraries():
    p = ctypes.c_void_p(4096)                                    # never dereferenced: the argument check fails first
    odd8, odd4 = ctypes.c_void_p(4096 + 8), ctypes.c_void_p(4096 + 4)
    big = 10 ** 9
    for path, fn in _libraries():
        def hfwd(x=p, w=p, pre=p, bias=p, pitch=32, B=2, H=8, W=12, C=32):
            return fn["xpt_flowhead_fwd"](x, pitch, w, bias, pre, B, H, W, C, None)

        def hbwd(x=p, w=p, g=p, dx=p, part=p, floats=big, pitch=32, B=2, H=8, W=12, C=32):
            return fn["xpt_flowhead_bwd"](x, pitch, w, g, dx, part, floats, B, H, W, C, None)

        def ufwd(x=p, w=p, y=p, bias=p, pitch=32, f32=0, B=2, H=8, W=12, C=32):
            return fn["xpt_upconv4x4s2_fwd"](x, pitch, f32, w, bias, y, B, H, W, C, None)

        def ubwd(x=p, w=p, g=p, dx=p, part=p, floats=big, pitch=32, f32=0, B=2, H=8, W=12, C=32):
            return fn["xpt_upconv4x4s2_bwd"](x, pitch, f32, w, g, dx, part, floats, B, H, W, C, None)

        nulls = [hfwd(x=None), hfwd(w=None), hfwd(pre=None), hbwd(x=None), hbwd(w=None), hbwd(g=None), hbwd(dx=None),
                 hbwd(part=None), ufwd(x=None), ufwd(w=None), ufwd(y=None), ubwd(x=None), ubwd(w=None), ubwd(g=None),
                 ubwd(dx=None), ubwd(part=None)]
        assert set(nulls) == {NULL_}, (path, nulls)
        for call in (hfwd, hbwd, ufwd, ubwd):
            shapes = {"B 0": call(B=0), "H 0": call(H=0), "W -1": call(W=-1), "2^31 pixels": call(B=1 << 15, H=1 << 8, W=1 << 8),
                      "W 2^24": call(B=1, H=1, W=1 << 24)}
            assert set(shapes.values()) == {SHAPE}, (path, call.__name__, shapes)
            args = {"pitch < C": call(pitch=24), "pitch % 8": call(pitch=36), "x alignment": call(x=odd8)}
            assert set(args.values()) == {ARG}, (path, call.__name__, args)
        assert {hfwd(C=8), hfwd(C=24), hfwd(C=196), hfwd(C=0), hbwd(C=8), hbwd(C=256)} == {ARG}, path
        assert {ufwd(C=2), ufwd(C=64), ufwd(C=12), ubwd(C=2), ubwd(C=64), ufwd(f32=2), ubwd(f32=-1)} == {ARG}, path
        assert {ufwd(f32=1, C=32), ufwd(f32=1, C=2, pitch=8), ubwd(f32=1, C=8, pitch=2), ubwd(f32=1, C=2, pitch=4)} == {ARG}, path
        assert {ufwd(f32=1, C=2, pitch=2, x=odd4), ubwd(f32=1, C=2, pitch=2, dx=odd4), ufwd(y=odd8), ubwd(dx=odd8), ubwd(g=odd4),
                hbwd(dx=odd8), hbwd(g=odd4), hfwd(pre=odd4)} == {ARG}, path
        # the up-sampler counts OUTPUT pixels: 2^29 input pixels are 2^31 output pixels
        assert ufwd(B=1 << 13, H=1 << 8, W=1 << 8) == SHAPE and ubwd(B=1 << 13, H=1 << 8, W=1 << 8) == SHAPE
        # a partials buffer one float short
        nh = fn["xpt_flowhead_bwd_blocks"](2, 8, 12, 32)
        assert nh >= 1 and hbwd(floats=nh * (18 * 32 + 2) - 1) == WORKSPACE
        for f32, C, pitch in ((0, 32, 32), (0, 8, 8), (1, 2, 2)):
            nu = fn["xpt_upconv4x4s2_bwd_blocks"](2, 8, 12, C, f32)
            assert nu >= 1 and ubwd(f32=f32, C=C, pitch=pitch, floats=nu * (32 * C + 2) - 1) == WORKSPACE, (path, f32, C)


def test_bwd_blocks_follow_the_documented_plan():
    """At least one partial row for every served shape, never more than one row per pixel group of a workgroup pass, capped;
    0 for what the kernels do not serve.  The GPU tests' largest map has more than one row for every channel count."""
    for path, fn in _libraries():
        hb, ub = fn["xpt_flowhead_bwd_blocks"], fn["xpt_upconv4x4s2_bwd_blocks"]
        for B, H, W in ((3, 1, 1), (3, 2, 3), (3, 5, 7), (3, 9, 20), (32, 32, 96), (8, 256, 512)):
            P = B * H * W
            for C in (16, 32, 64, 128):
                n = hb(B, H, W, C)
                per_pass = 4 * (64 // (C // 8))
                assert 1 <= n <= max(1, -(-P // per_pass)) and n <= 512, (path, B, H, W, C, n)
            for C, f32 in ((2, 1), (8, 0), (16, 0), (32, 0)):
                n = ub(B, H, W, C, f32)
                per_pass = 4 * (64 // (1 if f32 else C // 4))
                assert 1 <= n <= max(1, -(-P // per_pass)) and n <= 512, (path, B, H, W, C, n)
        assert all(hb(3, 9, 20, C) > 1 for C in (16, 32, 128))
        assert all(ub(3, 9, 20, C, f32) > 1 for C, f32 in ((2, 1), (8, 0), (32, 0)))
        assert hb(3, 1, 1, 32) == 1 and ub(3, 1, 1, 2, 1) == 1
        assert hb(0, 4, 4, 32) == 0 and hb(2, 4, 4, 24) == 0 and ub(2, 4, 4, 2, 0) == 0 and ub(2, 4, 4, 32, 1) == 0
        assert ub(2, 4, 4, 32, 2) == 0 and ub(2, 0, 4, 32, 0) == 0


def test_ops_refuse_cpu_tensors_and_wrong_weights():
    from xpt_mde_2021_amd.hip import flowtail as ft
    from xpt_mde_2021_amd.hip.lib import XptHipError
    with pytest.raises(XptHipError):
        ft.flow_head(torch.zeros(1, 32, 4, 4), torch.zeros(2, 32, 3, 3), None)
    with pytest.raises(XptHipError):
        ft.upconv4x4s2(torch.zeros(1, 2, 4, 4), torch.zeros(2, 2, 4, 4), None)
