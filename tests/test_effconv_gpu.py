"""The kernels of csrc/xpt_effconv.hip through the C ABI of BOTH libraries (bf16, IEEE half) against fp64 computed on the CPU:
the middle of `block` of tf.keras.applications.EfficientNetB<n> (the backbones model/build_model/pretrained_nets.py:11-117
instantiates) -- depthwise k x k -> BatchNorm -> swish, squeeze-and-excite, multiply -- and its backward.

Bounds (the project's, tests/test_mbconv_gpu.py).  16-bit outputs (v, z, dx): |err| <= 2^-8 |ref| + 1e-4 max|ref| for bf16, 2^-11
for IEEE half -- the output format's rounding plus the 1e-4 bar for fp32 arithmetic against fp64.  fp32 outputs (pooled sums, p,
r, gate, dgate, dp and every parameter-gradient sum): 1e-4 max|ref|.  Swish has no kink, so nothing is excluded.

Every entry point is compared with the fp64 value of ITS OWN function of ITS OWN inputs: the backward kernels take the stored
16-bit v as an input (they form sw'(v) from it on load), so the test hands them the fp64 forward's v rounded to the format and the
fp64 reference uses that same tensor; the forward's v and pooled sums are compared with the unrounded fp64 forward."""
import ctypes
import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

EPS = 1e-3
# (B, H, W, C, k, stride): even extents (pads 1/2 at k = 5), odd extents (2/2), a map smaller than the window, the widest
# 5 x 5 stages of B0 on the 1/16 and 1/32 maps of a 64 x 96 image, and several chunks per image
SHAPES = [(2, 5, 7, 8, 3, 1), (2, 6, 10, 24, 5, 2), (1, 9, 5, 16, 5, 2), (1, 7, 9, 16, 3, 2), (2, 2, 3, 1152, 5, 1),
          (2, 4, 6, 672, 5, 2), (8, 16, 24, 96, 3, 2)]
EXCITE = [(2, 8, 1), (2, 32, 8), (2, 96, 4), (1, 144, 6), (3, 1152, 48), (2, 3840, 160)]
FORMATS = {"bf16": (torch.bfloat16, 2.0 ** -8), "fp16": (torch.float16, 2.0 ** -11)}
NAMES = ("xpt_dwconv_bn_swish_chunks", "xpt_dwconv_bn_swish_fwd", "xpt_se_excite_fwd", "xpt_se_scale_fwd", "xpt_se_scale_bwd_reduce",
         "xpt_se_excite_bwd", "xpt_dwconv_bn_swish_bwd", "xpt_half_format")


@functools.lru_cache(maxsize=None)
def library(fmt):
    from xpt_mde_2021_amd.hip import lib as xl
    lib = ctypes.CDLL(xl.LIB_PATH_F16 if fmt == "fp16" else xl.LIB_PATH)
    for name in NAMES:
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = xl.SIGNATURES[name]
    assert lib.xpt_half_format() == (1 if fmt == "fp16" else 0)
    return lib


def same_pads(h, w, k, stride):
    oh, ow = -(-h // stride), -(-w // stride)
    th, tw = max((oh - 1) * stride + k - h, 0), max((ow - 1) * stride + k - w, 0)
    return th // 2, th - th // 2, tw // 2, tw - tw // 2, oh, ow


def swish(t):
    return t * torch.sigmoid(t)


def dswish(t):
    g = torch.sigmoid(t)
    return g * (1 + t * (1 - g))


@functools.lru_cache(maxsize=None)
def case(shape, act_in, fmt):
    """Inputs (rounded to the formats the kernels read) and the fp64 references of one depthwise case, computed once on the CPU;
    never modified.  Image b is shifted by 0.4 b: its pooled sums differ from every other image's by far more than the bound."""
    B, H, W, C, k, stride = shape
    dtype, _ = FORMATS[fmt]
    g = torch.Generator().manual_seed(1000 * C + 10 * H + stride + 100 * k + (7 if act_in else 0))
    rnd = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)                  # noqa: E731
    f32 = lambda t: t.float().double()                                                  # noqa: E731
    x = (1.5 * rnd(B, C, H, W) + 0.4 * torch.arange(B, dtype=torch.float64).view(B, 1, 1, 1)).to(dtype).double()
    w = f32(rnd(C, 1, k, k) / k)
    gamma, beta = f32(0.5 + torch.rand(C, generator=g, dtype=torch.float64)), f32(0.5 * rnd(C))
    mean, var = f32(0.3 * rnd(C)), f32(0.5 + 1.5 * torch.rand(C, generator=g, dtype=torch.float64))
    pt, pb, pl, pr, OH, OW = same_pads(H, W, k, stride)
    xr, wr, gr, br = (t.clone().requires_grad_(True) for t in (x, w, gamma, beta))
    a = swish(xr) if act_in else xr
    u = F.conv2d(F.pad(a, (pl, pr, pt, pb)), wr, None, stride, 0, 1, C)
    s = gr / (var + EPS).sqrt()
    v = u * s.view(1, C, 1, 1) + (br - mean * s).view(1, C, 1, 1)
    pooled = swish(v.detach()).sum((2, 3))                                              # [B, C] sums (not means)
    # the backward's inputs: the stored v, a gate in (0, 1), dL/dp and dL/dz
    v_in = v.detach().to(dtype).double()
    gate = f32(torch.sigmoid(1.5 * rnd(B, C)))
    dp = f32(rnd(B, C))
    dz = rnd(B, C, OH, OW).to(dtype).double()
    gz = dswish(v_in) * (dz * gate.view(B, C, 1, 1) + dp.view(B, C, 1, 1) / (OH * OW))
    (v * gz).sum().backward()
    ref = dict(v=v.detach(), pooled=pooled, dx=xr.grad, dw=wr.grad, dgamma=gr.grad, dbeta=br.grad,
               z=swish(v_in) * gate.view(B, C, 1, 1), dgate=(dz * swish(v_in)).sum((2, 3)))
    assert float((pooled[0] - pooled[-1]).abs().max()) > 1e-2 * float(pooled.abs().max()) or B == 1
    return dict(x=x, w=w, gamma=gamma, beta=beta, mean=mean, var=var, v_in=v_in, gate=gate, dp=dp, dz=dz, ref=ref,
                geom=(pt, pl, OH, OW))


def nhwc(t, dtype, dev):
    """NCHW fp64 CPU tensor -> dense NHWC 16-bit device tensor."""
    return t.permute(0, 2, 3, 1).contiguous().to(dtype).to(dev)


def ptr(t):
    return ctypes.c_void_p(t.data_ptr())


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def bound_ok(got, ref, rel, what):
    err = (got.double().cpu() - ref).abs()
    allowed = rel * ref.abs() + 1e-4 * ref.abs().max()
    worst = float((err / allowed.clamp_min(1e-300)).max())
    print(f"  {what}: max |err| {float(err.max()):.3e}, worst err / bound {worst:.3f}")
    return bool(torch.isfinite(got).all()) and worst <= 1.0


def fp32_ok(got, ref, what):
    err = float((got.double().cpu() - ref).abs().max())
    print(f"  {what}: max |err| {err:.3e} of max|ref| {float(ref.abs().max()):.3e}")
    return bool(torch.isfinite(got).all()) and err <= 1e-4 * float(ref.abs().max())


def run_fwd(lib, dev, fmt, shape, act_in, c):
    B, H, W, C, k, stride = shape
    dtype, _ = FORMATS[fmt]
    pt, pl, OH, OW = c["geom"]
    x = nhwc(c["x"], dtype, dev)
    w, gamma, beta, mean, var = (c[n].float().contiguous().to(dev) for n in ("w", "gamma", "beta", "mean", "var"))
    chunks = lib.xpt_dwconv_bn_swish_chunks(B, OH, OW, C)
    assert chunks >= B and chunks % B == 0
    v = torch.full((B, OH, OW, C), float("nan"), dtype=dtype, device=dev)
    pool = torch.full((chunks, C), float("nan"), dtype=torch.float32, device=dev)
    rc = lib.xpt_dwconv_bn_swish_fwd(ptr(x), ptr(w), ptr(gamma), ptr(beta), ptr(mean), ptr(var), EPS, ptr(v), ptr(pool), pool.numel(),
                                     B, H, W, C, k, stride, pt, pl, OH, OW, int(act_in), stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    return v, pool


def run_bwd(lib, dev, fmt, shape, act_in, c, dz_dev, dz_pitch, want_dx=True):
    B, H, W, C, k, stride = shape
    dtype, _ = FORMATS[fmt]
    pt, pl, OH, OW = c["geom"]
    x, v = nhwc(c["x"], dtype, dev), nhwc(c["v_in"], dtype, dev)
    w, gamma, mean, var, gate, dp = (c[n].float().contiguous().to(dev) for n in ("w", "gamma", "mean", "var", "gate", "dp"))
    chunks = lib.xpt_dwconv_bn_swish_chunks(B, OH, OW, C)
    partials = torch.full((chunks, (k * k + 2) * C), float("nan"), dtype=torch.float32, device=dev)
    dx = torch.full((B, H, W, C), float("nan"), dtype=dtype, device=dev) if want_dx else None
    rc = lib.xpt_dwconv_bn_swish_bwd(ptr(x), ptr(v), ctypes.c_void_p(dz_dev), dz_pitch, ptr(gate), ptr(dp), ptr(w), ptr(gamma),
                                     ptr(mean), ptr(var), EPS, None if dx is None else ptr(dx), ptr(partials), partials.numel(), B, H,
                                     W, C, k, stride, pt, pl, OH, OW, int(act_in), stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    return dx, partials


@pytest.mark.parametrize("fmt", ["bf16", "fp16"])
@pytest.mark.parametrize("act_in", [0, 1])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(str(v) for v in s))
def test_depthwise_bn_swish_forward_and_backward_against_fp64(gpu_device, shape, act_in, fmt):
    """v, the per-image pooled sums, dx, the three partial pieces; dx = NULL, a pitched dz slice, and a repeat call bit for bit.
    The forward has one variant (no plan-selected alternatives), which every shape runs."""
    import xpt_mde_2021_amd.hip.lib  # noqa: F401  (torch's HIP runtime first)
    lib, dev = library(fmt), gpu_device
    B, H, W, C, k, stride = shape
    dtype, rel = FORMATS[fmt]
    c = case(shape, bool(act_in), fmt)
    ref = c["ref"]
    pt, pl, OH, OW = c["geom"]
    print(f"\n{shape} act_in={act_in} {fmt}: pads {pt}/{pl}, output {OH} x {OW}")
    v, pool = run_fwd(lib, dev, fmt, shape, act_in, c)
    assert bound_ok(v.permute(0, 3, 1, 2), ref["v"], rel, "v")
    assert bool(torch.isfinite(pool).all())
    assert fp32_ok(pool.view(B, -1, C).double().sum(1), ref["pooled"], f"pooled sums ({pool.shape[0] // B} rows per image)")
    dz = nhwc(c["dz"], dtype, dev)
    dx, partials = run_bwd(lib, dev, fmt, shape, act_in, c, dz.data_ptr(), C)
    assert bound_ok(dx.permute(0, 3, 1, 2), ref["dx"], rel, "dx")
    assert bool(torch.isfinite(partials).all())
    total = partials.double().sum(0).cpu()
    kk = k * k
    assert fp32_ok(total[:kk * C].view(C, 1, k, k), ref["dw"], "dw")
    assert fp32_ok(total[kk * C:(kk + 1) * C], ref["dgamma"], "dgamma")
    assert fp32_ok(total[(kk + 1) * C:], ref["dbeta"], "dbeta")
    # a second run: bit-identical (fixed order, no atomics)
    v2, pool2 = run_fwd(lib, dev, fmt, shape, act_in, c)
    dx2, partials2 = run_bwd(lib, dev, fmt, shape, act_in, c, dz.data_ptr(), C)
    assert torch.equal(v.view(torch.int16), v2.view(torch.int16)) and torch.equal(pool, pool2)
    assert torch.equal(partials, partials2) and torch.equal(dx.view(torch.int16), dx2.view(torch.int16))
    # dz as a channel slice of a wider tensor, read in place: bit for bit the dense result; dx = NULL leaves the partials alone
    pitch = C + 16
    wide = torch.full((B, OH, OW, pitch), float("nan"), dtype=dtype, device=dev)
    wide[..., 8:8 + C] = dz
    dx3, partials3 = run_bwd(lib, dev, fmt, shape, act_in, c, wide.data_ptr() + 16, pitch)
    assert torch.equal(partials, partials3) and torch.equal(dx.view(torch.int16), dx3.view(torch.int16))
    none, partials4 = run_bwd(lib, dev, fmt, shape, act_in, c, dz.data_ptr(), C, want_dx=False)
    assert none is None and torch.equal(partials, partials4)


@pytest.mark.parametrize("fmt", ["bf16", "fp16"])
@pytest.mark.parametrize("shape", SHAPES[:4], ids=lambda s: "x".join(str(v) for v in s))
def test_scale_forward_and_gate_gradient_against_fp64(gpu_device, shape, fmt):
    """z = sw(v) gate and dgate = sum_hw dz sw(v) on the first four depthwise output maps, dz dense and as a pitched slice."""
    import xpt_mde_2021_amd.hip.lib  # noqa: F401
    lib, dev = library(fmt), gpu_device
    B, H, W, C, k, stride = shape
    dtype, rel = FORMATS[fmt]
    c = case(shape, True, fmt)
    ref = c["ref"]
    _, _, OH, OW = c["geom"]
    v, gate = nhwc(c["v_in"], dtype, dev), c["gate"].float().contiguous().to(dev)
    z = torch.full((B, OH, OW, C), float("nan"), dtype=dtype, device=dev)
    assert lib.xpt_se_scale_fwd(ptr(v), ptr(gate), ptr(z), B, OH, OW, C, stream()) == 0
    torch.cuda.synchronize()
    print(f"\n{(B, OH, OW, C)} {fmt}")
    assert bound_ok(z.permute(0, 3, 1, 2), ref["z"], rel, "z")
    chunks = lib.xpt_dwconv_bn_swish_chunks(B, OH, OW, C)
    dz = nhwc(c["dz"], dtype, dev)
    wide = torch.full((B, OH, OW, C + 16), float("nan"), dtype=dtype, device=dev)
    wide[..., 8:8 + C] = dz
    outs = []
    for base, pitch in ((dz.data_ptr(), C), (wide.data_ptr() + 16, C + 16), (dz.data_ptr(), C)):
        rows = torch.full((chunks, C), float("nan"), dtype=torch.float32, device=dev)
        dgate = torch.full((B, C), float("nan"), dtype=torch.float32, device=dev)
        assert lib.xpt_se_scale_bwd_reduce(ptr(v), ctypes.c_void_p(base), pitch, ptr(rows), rows.numel(), ptr(dgate), B, OH, OW, C,
                                           stream()) == 0
        torch.cuda.synchronize()
        outs.append(dgate)
    assert fp32_ok(outs[0], ref["dgate"], "dgate")
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])


@functools.lru_cache(maxsize=None)
def excite_case(B, C, S):
    g = torch.Generator().manual_seed(C * 7 + S)
    rnd = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)                  # noqa: E731
    f32 = lambda t: t.float().double()                                                  # noqa: E731
    cpi, HW = 3, 24
    rows = f32(rnd(B, cpi, C) * HW / cpi + 4.0 * torch.arange(B, dtype=torch.float64).view(B, 1, 1))
    wr, br = f32(rnd(S, C) * 2.0 / C ** 0.5), f32(rnd(S))
    we, be = f32(rnd(C, S) * 2.0 / S ** 0.5), f32(rnd(C))
    dgate = f32(rnd(B, C))
    leaves = [t.clone().requires_grad_(True) for t in (wr, br, we, be)]
    p = (rows.sum(1) / HW).requires_grad_(True)
    r = p @ leaves[0].t() + leaves[1]
    gate = torch.sigmoid(swish(r) @ leaves[2].t() + leaves[3])
    (gate * dgate).sum().backward()
    ref = dict(p=p.detach(), r=r.detach(), gate=gate.detach(), dp=p.grad, dwr=leaves[0].grad, dbr=leaves[1].grad,
               dwe=leaves[2].grad, dbe=leaves[3].grad)
    return dict(rows=rows, cpi=cpi, HW=HW, wr=wr, br=br, we=we, be=be, dgate=dgate, ref=ref)


@pytest.mark.parametrize("fmt", ["bf16", "fp16"])
@pytest.mark.parametrize("B,C,S", EXCITE)
def test_excite_forward_and_backward_against_fp64(gpu_device, B, C, S, fmt):
    """pool finish -> reduce (bias, swish) -> expand (bias, sigmoid) and the whole backward, all in fp32: p, r, gate, dp and the
    four parameter gradients summed over the batch; S = 1 and S no multiple of anything included; a repeat is bit-identical."""
    import xpt_mde_2021_amd.hip.lib  # noqa: F401
    lib, dev = library(fmt), gpu_device
    c = excite_case(B, C, S)
    ref = c["ref"]
    dv = lambda t: t.float().contiguous().to(dev)                                      # noqa: E731
    rows, wr, br, we, be, dgate = (dv(c[n]) for n in ("rows", "wr", "br", "we", "be", "dgate"))
    print(f"\n{(B, C, S)} {fmt}: gate in [{float(ref['gate'].min()):.3f}, {float(ref['gate'].max()):.3f}]")
    runs = []
    for _ in range(2):
        nan = lambda *s: torch.full(s, float("nan"), dtype=torch.float32, device=dev)   # noqa: E731
        o = dict(p=nan(B, C), r=nan(B, S), gate=nan(B, C), dp=nan(B, C), dwr=nan(S, C), dbr=nan(S), dwe=nan(C, S), dbe=nan(C))
        assert lib.xpt_se_excite_fwd(ptr(rows), c["cpi"], c["HW"], ptr(wr), ptr(br), ptr(we), ptr(be), ptr(o["p"]), ptr(o["r"]),
                                     ptr(o["gate"]), B, C, S, stream()) == 0
        assert lib.xpt_se_excite_bwd(ptr(dgate), ptr(o["gate"]), ptr(o["p"]), ptr(o["r"]), ptr(wr), ptr(we), ptr(o["dwr"]),
                                     ptr(o["dbr"]), ptr(o["dwe"]), ptr(o["dbe"]), ptr(o["dp"]), B, C, S, stream()) == 0
        torch.cuda.synchronize()
        runs.append(o)
    for name in ("p", "r", "gate", "dp", "dwr", "dbr", "dwe", "dbe"):
        assert fp32_ok(runs[0][name], ref[name], name), name
        assert torch.equal(runs[0][name], runs[1][name]), name


def test_gradients_land_on_their_parameters_through_the_gradient_sink(gpu_device):
    """hip.ops.mbconv_se with all seven parameters on `flat_grad` views (as optimizers.FlatParameters sets them): the backward
    leaves [C k k | C | C] partial rows and one [S C | S | C S | C] row behind and GradSink.flush() adds them.  Each destination
    equals what the same op returns to autograd without a sink, within the fp32 bar (the two differ in summation order only),
    and nothing is written between the destinations."""
    from xpt_mde_2021_amd.hip import lib as xl, ops
    from xpt_mde_2021_amd.model.build_model.pretrained_nets import FrozenBatchNorm
    fmt = xl.half_format()
    dtype, rel = FORMATS[fmt]
    shape = (2, 4, 6, 672, 5, 2)
    B, H, W, C, k, stride = shape
    S = 28
    c = case(shape, True, fmt)
    e = excite_case(2, C, S)
    dev = gpu_device
    bn = FrozenBatchNorm(C).to(dev)
    with torch.no_grad():
        bn.weight.copy_(c["gamma"]), bn.bias.copy_(c["beta"]), bn.running_mean.copy_(c["mean"]), bn.running_var.copy_(c["var"])
    P = lambda t: torch.nn.Parameter(t.float().to(dev))                                # noqa: E731
    weight, wr, br, we, be = P(c["w"]), P(e["wr"].view(S, C, 1, 1)), P(e["br"]), P(e["we"].view(C, S, 1, 1)), P(e["be"])
    params = [weight, bn.weight, bn.bias, wr, br, we, be]
    x = c["x"].to(dtype).to(dev).contiguous(memory_format=torch.channels_last)
    dz = c["dz"].to(dtype).to(dev).contiguous(memory_format=torch.channels_last)

    def step():
        xin = x.clone().requires_grad_(True)
        z = ops.mbconv_se(xin, weight, bn, wr, br, we, be, k, stride, act_in=True, eps=EPS)
        z.backward(dz)
        return z.detach(), xin.grad

    z0, dx0 = step()
    plain = [p.grad.clone() for p in params]
    assert all(bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0 for g in plain)
    for p in params:
        p.grad = None
    sizes = [p.numel() for p in params]
    step8 = lambda n: (n + 7) // 8 * 8 + 8                                             # noqa: E731  (8-element alignment, as FlatParameters)
    flat = torch.full((sum(step8(n) for n in sizes),), float("nan"), device=dev)
    at = 0
    for p, n in zip(params, sizes):
        p.flat_grad = flat[at:at + n].view(p.shape)
        at += step8(n)
    sink = ops.grad_sink
    assert sink.enabled and not sink.pending
    z1, dx1 = step()
    assert all(p.grad is None for p in params) and len(sink.pending) == 7           # deferred, not returned
    sink.flush()
    torch.cuda.synchronize()
    assert torch.equal(z0, z1) and torch.equal(dx0, dx1)
    for name, p, want in zip(("dw", "dgamma", "dbeta", "dW_r", "db_r", "dW_e", "db_e"), params, plain):
        assert fp32_ok(p.flat_grad, want.double().cpu(), f"{name} through the sink"), name
    at = 0
    for n in sizes:
        assert bool(torch.isnan(flat[at + n:at + step8(n)]).all())                   # nothing beyond a destination
        at += step8(n)
    # and the op's dx is the C ABI's (same kernels): against the fp64 reference of the whole middle in the 16-bit bound is the
    # encoder-level test's business (tests/test_efficientnet_gpu.py); here only that it is finite and not zero
    assert bool(torch.isfinite(dx1).all()) and float(dx1.float().abs().max()) > 0


def cotangent_layouts(dz):
    """dz (dense channels_last, C channels) three ways with the same values: as it is; channels [8, 8 + C) of a channels_last
    tensor with C + 16 channels (16-byte aligned rows: read in place); channels [4, 4 + C) of such a tensor (base 8 bytes off a
    16-byte boundary: copied first)."""
    B, C, H, W = dz.shape
    out = [dz]
    for first in (8, 4):
        wide = torch.full((B, C + 16, H, W), float("nan"), dtype=dz.dtype, device=dz.device).contiguous(memory_format=torch.channels_last)
        wide[:, first:first + C] = dz
        out.append(wide[:, first:first + C])
        assert out[-1].stride() == (H * W * (C + 16), 1, W * (C + 16), C + 16) and torch.equal(out[-1], dz)
        assert out[-1].data_ptr() % 16 == (0 if first == 8 else 8)
    return out


@pytest.mark.parametrize("shape", [(2, 5, 7, 16, 3, 1), (1, 6, 10, 24, 5, 2)], ids=lambda s: "x".join(str(v) for v in s))
def test_backward_is_bit_identical_for_dense_in_place_and_copied_cotangent_slices(gpu_device, shape):
    """hip.ops.mbconv_se backward with the cotangent dense, as an aligned channel slice (the 16-byte loads take it in place) and
    as a misaligned one (copied): dx, the weight / gamma / beta gradients and the four squeeze-excite gradients are the same bits
    all three times."""
    from xpt_mde_2021_amd.hip import lib as xl, ops
    from xpt_mde_2021_amd.model.build_model.pretrained_nets import FrozenBatchNorm
    fmt = xl.half_format()
    dtype, _ = FORMATS[fmt]
    B, H, W, C, k, stride = shape
    S = C // 4
    c = case(shape, True, fmt)
    e = excite_case(B, C, S)
    dev = gpu_device
    bn = FrozenBatchNorm(C).to(dev)
    with torch.no_grad():
        bn.weight.copy_(c["gamma"]), bn.bias.copy_(c["beta"]), bn.running_mean.copy_(c["mean"]), bn.running_var.copy_(c["var"])
    P = lambda t: torch.nn.Parameter(t.float().to(dev))                                # noqa: E731
    weight, wr, br, we, be = P(c["w"]), P(e["wr"].view(S, C, 1, 1)), P(e["br"]), P(e["we"].view(C, S, 1, 1)), P(e["be"])
    params = (weight, bn.weight, bn.bias, wr, br, we, be)
    x = c["x"].to(dtype).to(dev).contiguous(memory_format=torch.channels_last)
    dz = c["dz"].to(dtype).to(dev).contiguous(memory_format=torch.channels_last)
    results = []
    for cot in cotangent_layouts(dz):
        for p in params:
            p.grad = None
        xin = x.clone().requires_grad_(True)
        ops.mbconv_se(xin, weight, bn, wr, br, we, be, k, stride, act_in=True, eps=EPS).backward(cot)
        results.append([xin.grad] + [p.grad.clone() for p in params])
    torch.cuda.synchronize()
    assert all(bool(torch.isfinite(g).all()) and float(g.float().abs().max()) > 0 for g in results[0])
    for name, dense, in_place, copied in zip(("dx", "dw", "dgamma", "dbeta", "dW_r", "db_r", "dW_e", "db_e"), *results):
        assert torch.equal(dense, in_place), f"{name}: in-place slice"
        assert torch.equal(dense, copied), f"{name}: copied slice"
