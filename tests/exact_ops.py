"""Exact-integer operands and fp64 CPU references for the equality tests of the dense and depthwise convolutions
(tests/test_conv_exact_cpu.py, tests/test_conv_exact_gpu.py; DESIGN.md "Exact-integer parity").

The matrix cores multiply 16-bit operands exactly and accumulate in fp32.  With operands that are small integers, and every
intermediate a kernel stores in 16 bits (y, g = dy * act'(y), the bilinear path's scratch gradient, dx) an integer or dyadic
value that fits the format's significand, every correct implementation gives the same values whatever its summation order,
split count or workgroup numbering -- and a dropped, duplicated or mis-indexed term moves some element by at least 1.  The
references below are plain F.pad / F.conv2d / F.interpolate / F.leaky_relu and autograd in float64; each asserts `fits` on those
intermediates for the 16-bit format of the process BEFORE any device work: a condition of the method, not a tolerance."""
import functools
import math
from dataclasses import dataclass
from typing import Optional

import torch
import torch.nn.functional as F

from xpt_mde_2021_amd.hip import lib as _lib

FORMATS = (torch.bfloat16, torch.float16)
EXACT_F32 = float(1 << 24)          # integers (and dyadic values of the same span) below this are exact in fp32


def half():
    return _lib.half()


def tri(shape, density, gen, scale=1):
    """float64 tensor with values in scale * {-1, 0, 1}; a share `density` of the elements is non-zero."""
    r = torch.rand(shape, generator=gen, dtype=torch.float64)
    return float(scale) * ((r < 0.5 * density).double() - ((r >= 0.5 * density) & (r < density)).double())


def fits(t, dtype):
    """True iff every element of t survives a round trip through `dtype` unchanged."""
    t = t.detach().double()
    return bool((t.to(dtype).double() == t).all())


def require_fits(named, dtype, what):
    bad = [f"{n} (max |v| {float(t.detach().abs().max()):g})" for n, t in named.items() if t is not None and not fits(t, dtype)]
    assert not bad, f"{what}: not exact in {dtype}: {', '.join(bad)} -- lower the densities of this case"


def same_pad(n, k, s, d=1):
    total = max((math.ceil(n / s) - 1) * s + (k - 1) * d + 1 - n, 0)
    return total // 2, total - total // 2


def round_up(n, m):
    return (n + m - 1) // m * m


# ------------------------------------------------------------------------------------------------ dense convolutions
@dataclass(frozen=True)
class ConvCase:
    """One conv2d_same call.  ups: None | "nearest" | "bilinear"; pad: ZeroPadding2D(pad) + VALID; slice_of: the input is the
    channels [8, 8 + round_up(cin, 8)) of a tensor this wide; xd / wd / gd: share of non-zero elements of x / w / gy, whose values
    are xs * {-1, 0, 1}, {-1, 0, 1} and gs * {-1, 0, 1} (gs even: g = gy / 2 under slope 0.5 stays an integer)."""
    cin: int
    cout: int
    k: int
    stride: int
    H: int
    W: int
    ups: Optional[str] = None
    slope: float = 0.5
    batch: int = 3
    valid: bool = False
    pad: Optional[int] = None
    dilation: int = 1
    slice_of: int = 0
    xd: float = 0.25
    wd: float = 0.25
    gd: float = 0.25
    xs: int = 1
    gs: int = 2

    def __str__(self):
        s = f"{self.cin}-{self.cout}-k{self.k}s{self.stride}-{self.H}x{self.W}-b{self.batch}"
        for flag, text in ((self.ups, self.ups), (self.slope != 0.5, f"slope{self.slope:g}"), (self.valid, "valid"),
                           (self.pad is not None, f"pad{self.pad}"), (self.dilation != 1, f"d{self.dilation}"),
                           (self.slice_of, f"slice{self.slice_of}")):
            if flag:
                s += f"-{text}"
        return s

    def seed(self):
        return (self.cin * 131 + self.cout * 7 + self.k * 17 + self.stride * 3 + self.H * 1009 + self.W * 37 + self.batch * 5
                + self.dilation * 11 + (0 if self.pad is None else 100 + self.pad))


def conv_forward(x, w, b, case):
    """The layer in the dtype of its arguments: (pre-activation, y, the up-sampled input or x itself, the padded input the
    convolution reads).  TF SAME unless case.valid / case.pad."""
    xu = x
    if case.ups == "nearest":
        xu = F.interpolate(x, scale_factor=2, mode="nearest")
    elif case.ups == "bilinear":
        xu = F.interpolate(x, scale_factor=2, mode="bilinear", align_corners=False)
    if case.ups == "bilinear" and xu.requires_grad:
        xu.retain_grad()
    if case.pad is not None:
        xp = F.pad(xu, (case.pad,) * 4)
    elif case.valid:
        xp = xu
    else:
        (pt, pb) = same_pad(xu.shape[2], case.k, case.stride, case.dilation)
        (pl, pr) = same_pad(xu.shape[3], case.k, case.stride, case.dilation)
        xp = F.pad(xu, (pl, pr, pt, pb))
    pre = F.conv2d(xp, w, b, case.stride, 0, case.dilation)
    if pre.requires_grad:
        pre.retain_grad()
    y = F.leaky_relu(pre, case.slope) if case.slope != 1.0 else pre
    return pre, y, xu, xp


@functools.lru_cache(maxsize=None)
def conv_reference(case):
    """float64 operands and results of `case`: x, w, b, gy and y, g (= dL/d pre-activation, what the kernels store as
    dy * act'(y)), gu (gradient w.r.t. the bilinear-2x map, the data gradient's 16-bit scratch; None otherwise), dx, dw, db,
    xu, xp (the up-sampled / padded input).  Asserts that x, w, gy, xu, y, g, gu and dx are exact in the process's 16-bit format
    and that every fp32 sum is one of exactly representable terms.  Shared between tests: treat the tensors as read-only."""
    gen = torch.Generator().manual_seed(case.seed())
    x = tri((case.batch, case.cin, case.H, case.W), case.xd, gen, case.xs).requires_grad_(True)
    w = tri((case.cout, case.cin, case.k, case.k), case.wd, gen).requires_grad_(True)
    b = tri((case.cout,), 0.5, gen, 3).requires_grad_(True)
    pre, y, xu, xp = conv_forward(x, w, b, case)
    gy = tri(y.shape, case.gd, gen, case.gs)
    (y * gy).sum().backward()
    ref = {"x": x.detach(), "w": w.detach(), "b": b.detach(), "gy": gy, "y": y.detach(), "g": pre.grad, "dx": x.grad, "dw": w.grad,
           "db": b.grad, "xu": xu.detach(), "xp": xp.detach(), "gu": xu.grad if case.ups == "bilinear" else None}
    check_conv_reference(case, ref, half())
    return ref


def check_conv_reference(case, ref, dtype):
    """The method's conditions on a reference, for one 16-bit format."""
    require_fits({n: ref[n] for n in ("x", "w", "gy", "xu", "y", "g", "gu", "dx")}, dtype, str(case))
    mx = {n: float(ref[n].abs().max()) for n in ("xu", "w", "b", "g")}
    K = case.cin * case.k * case.k
    # fp32 accumulations: every partial sum of the forward, of dW / db and of dx is bounded by the sum of the magnitudes
    assert mx["xu"] * mx["w"] * K + mx["b"] < EXACT_F32, f"{case}: forward sums leave the exact fp32 range"
    assert mx["g"] * max(mx["xu"], 1.0) * ref["g"][:, 0].numel() < EXACT_F32, f"{case}: dW / db sums leave the exact fp32 range"
    assert mx["g"] * mx["w"] * case.cout * case.k * case.k * 4 < EXACT_F32, f"{case}: dx sums leave the exact fp32 range"
    for n in ("dw", "db"):
        assert fits(ref[n], torch.float32), f"{case}: {n} is not exact in fp32"


# ------------------------------------------------------------------------------------------------ depth head (1 output channel)
@functools.lru_cache(maxsize=None)
def head_reference(C, H, W, batch=3):
    """xc.head_conv: Conv2D(1, 3, "same", linear) in fp32 on 16-bit features; integer fp32 weights, bias and cotangent.
    y, dw, db are fp32 results (exact integers), dx is stored in 16 bits."""
    gen = torch.Generator().manual_seed(C * 7 + H)
    x = tri((batch, C, H, W), 0.5, gen).requires_grad_(True)
    w = tri((1, C, 3, 3), 0.7, gen, 3).requires_grad_(True)
    b = torch.tensor([5.0], dtype=torch.float64, requires_grad=True)
    y = F.conv2d(x, w, b, 1, 1)
    gy = tri(y.shape, 0.5, gen, 2)
    (y * gy).sum().backward()
    ref = {"x": x.detach(), "w": w.detach(), "b": b.detach(), "gy": gy, "y": y.detach(), "dx": x.grad, "dw": w.grad, "db": b.grad}
    require_fits({"x": ref["x"], "dx": ref["dx"]}, half(), f"head {C} {H}x{W}")
    require_fits({n: ref[n] for n in ("w", "b", "gy", "y", "dw", "db")}, torch.float32, f"head {C} {H}x{W}")
    assert 3.0 * 9 * C + 5 < EXACT_F32 and 2.0 * batch * H * W < EXACT_F32
    return ref


# ------------------------------------------------------------------------------------------------ depthwise convolutions
@functools.lru_cache(maxsize=None)
def depthwise_reference(k, stride, shape, relu_in):
    """ops.depthwise_conv2d (TF SAME at stride 2, symmetric k // 2 at stride 1): x, w, gy in {-1, 0, 1}; y and dx are sums of at
    most k * k = 49 unit terms (exact in both 16-bit formats and in fp32), dw a sum of integers in fp32."""
    B, C, H, W = shape
    gen = torch.Generator().manual_seed(60 + k * 5 + stride + H)
    if stride == 2:
        (pt, pb), (pl, pr) = same_pad(H, k, 2), same_pad(W, k, 2)
    else:
        pt = pb = pl = pr = k // 2
    x = tri(shape, 0.6, gen).requires_grad_(True)
    w = tri((C, 1, k, k), 0.7, gen).requires_grad_(True)
    xin = F.relu(x) if relu_in else x
    y = F.conv2d(F.pad(xin, (pl, pr, pt, pb)), w, None, stride, 0, 1, C)
    gy = tri(y.shape, 0.6, gen)
    y.backward(gy)
    ref = {"x": x.detach(), "w": w.detach(), "gy": gy, "y": y.detach(), "dx": x.grad, "dw": w.grad, "pads": (pt, pb, pl, pr)}
    for dtype in FORMATS:
        require_fits({n: ref[n] for n in ("x", "gy", "y", "dx")}, dtype, f"depthwise k{k} s{stride} {shape}")
    assert fits(ref["dw"], torch.float32) and B * H * W < EXACT_F32
    return ref


# ------------------------------------------------------------------------------------------------ comparison
def mismatches(got, want):
    """(count, [(index, got, want)] of the first few) of the elements where got != want as VALUES (-0 equals +0, NaN never)."""
    got, want = got.detach().double().cpu(), want.detach().double().cpu()
    assert got.shape == want.shape, f"shape {tuple(got.shape)}, reference {tuple(want.shape)}"
    bad = ~(got == want)
    n = int(bad.sum())
    first = [(tuple(int(i) for i in idx), float(got[tuple(idx)]), float(want[tuple(idx)])) for idx in bad.nonzero()[:6]]
    return n, first


def assert_equal(got, want, what, axes=None):
    """torch.equal on values; on a mismatch: how many elements differ and the first few (index, got, want), the index decoded
    along `axes` (dW: ("cout", "cin", "kh", "kw"))."""
    n, first = mismatches(got, want)
    if n:
        def show(idx):
            return "(" + ", ".join(f"{a}={i}" for a, i in zip(axes, idx)) + ")" if axes else str(idx)
        lines = "; ".join(f"{show(idx)}: got {g:g}, want {w:g}" for idx, g, w in first)
        raise AssertionError(f"{what}: {n} of {want.numel()} elements differ -- {lines}")


DW_AXES = ("cout", "cin", "kh", "kw")
MAP_AXES = ("b", "c", "h", "w")


# ------------------------------------------------------------------------------------------------ corruptions a kernel could commit
def dw_of_pixels(ref, case, mask):
    """The part of dW that the output pixels selected by `mask` ([B, 1, OH, OW] bool) contribute, in the dtype of ref."""
    g = ref["g"] * mask.to(ref["g"].dtype)
    return torch.nn.grad.conv2d_weight(ref["xp"], ref["w"].shape, g, case.stride, 0, case.dilation)


def drop_dw_boundary_column(ref, case, kh, kw, rows=None):
    """dW without the last output column's terms of tap (kh, kw) -- of every row, or of the first `rows` (one row of tiles) only:
    a ragged-tile / range-check slip of the weight gradient."""
    B, _, OH, OW = ref["g"].shape
    mask = torch.zeros(B, 1, OH, OW, dtype=torch.bool)
    mask[..., :(OH if rows is None else rows), OW - 1] = True
    out = ref["dw"].clone()
    out[:, :, kh, kw] -= dw_of_pixels(ref, case, mask)[:, :, kh, kw]
    return out


def duplicate_dw_tile(ref, case, b=0, th=8, tw=16):
    """dW with the first th x tw pixel tile of image b counted twice: a split that also reduces its neighbour's tile."""
    B, _, OH, OW = ref["g"].shape
    mask = torch.zeros(B, 1, OH, OW, dtype=torch.bool)
    mask[b, :, :th, :tw] = True
    return ref["dw"] + dw_of_pixels(ref, case, mask)


def drop_y_tap_group(ref, case, kh, kw, c0):
    """y without the terms of tap (kh, kw), input channels [c0, c0 + 8), on the output columns of the ragged right-edge tile
    (columns from the last multiple of 16 on): one skipped 8-channel operand load."""
    wm = torch.zeros_like(ref["w"])
    wm[:, c0:c0 + 8, kh, kw] = ref["w"][:, c0:c0 + 8, kh, kw]
    delta = F.conv2d(ref["xp"], wm, None, case.stride, 0, case.dilation)
    OW = delta.shape[3]
    edge = (OW - 1) // 16 * 16
    delta[..., :edge] = 0
    pre = F.conv2d(ref["xp"], ref["w"], ref["b"], case.stride, 0, case.dilation) - delta
    return F.leaky_relu(pre, case.slope) if case.slope != 1.0 else pre


def normal_recipe(case, batch=2, slope=0.1):
    """The operands of the tolerance tests (tests/test_conv_igemm_gpu.py: random normal x and gy rounded to 16 bits, w scaled by
    1 / sqrt(fan-in)) on the geometry of `case`, and their fp32 reference, in the layout of conv_reference."""
    case = ConvCase(**{**case.__dict__, "batch": batch, "slope": slope})
    gen = torch.Generator().manual_seed(case.cin * 131 + case.cout * 7 + case.k)
    x = torch.randn(batch, case.cin, case.H, case.W, generator=gen).to(half()).float().requires_grad_(True)
    w = (torch.randn(case.cout, case.cin, case.k, case.k, generator=gen) / math.sqrt(case.cin * case.k * case.k)).to(half()).float()
    w.requires_grad_(True)
    b = (0.1 * torch.randn(case.cout, generator=gen)).requires_grad_(True)
    pre, y, xu, xp = conv_forward(x, w, b, case)
    gy = torch.randn(y.shape, generator=gen).to(half()).float()
    (y * gy).sum().backward()
    return case, {"x": x.detach(), "w": w.detach(), "b": b.detach(), "gy": gy, "y": y.detach(), "g": pre.grad, "dx": x.grad,
                  "dw": w.grad, "db": b.grad, "xu": xu.detach(), "xp": xp.detach()}


def largest_magnitude_error(got, want):
    """The tolerance tests' metric: max |got - want| as a fraction of max |want|."""
    return float((got - want).abs().max()) / (float(want.abs().max()) + 1e-12)
