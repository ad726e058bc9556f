"""The gfx950 code ResNet50V2 adds (csrc/xpt_resnet.hip, the explicit-padding entry of hip/conv.py), kernel by kernel, against fp64
evaluated on the same 16-bit-rounded operands.

Error bars of the junction: nobody has measured them, so the SAME relative-L2 error is measured for the torch-op twin
(hip.ops.res_join_torch: a GEMM plus element-wise framework ops in the same 16-bit dtype) and the kernel is allowed twice that,
because the accumulation order differs (the MobileNetV2 convention, tests/test_mbconv_gpu.py).  Both figures are printed."""
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

EPS = 1.001e-5


def _rel_l2(a, b):
    return float((a.detach().double().cpu() - b).norm() / b.norm().clamp_min(1e-300))


class _Bn:
    def __init__(self, gamma, beta, mean, var):
        self.weight, self.bias, self.running_mean, self.running_var = gamma, beta, mean, var


def _junction_case(K, N, hw, kind, half, seed):
    """Operands (16-bit-rounded activations and kernels, fp32 vectors) and the fp64 results of one junction."""
    g = torch.Generator().manual_seed(seed)
    B, (OH, OW) = 2, hw
    IH, IW = (2 * OH - 1, 2 * OW - 1) if kind == "strided" else (OH, OW)       # 5 x 7 <- 9 x 13, 8 x 12 <- 15 x 23 (odd extents)
    if kind == "strided" and OH == 8:
        IH, IW = 16, 24                                                          # and an even one
    r16 = lambda t: t.to(half).double()                                          # noqa: E731
    t = dict(h=r16(torch.randn(B, K, OH, OW, generator=g).relu()), w3=r16(torch.randn(N, K, 1, 1, generator=g) / math.sqrt(K)),
             b3=(0.1 * torch.randn(N, generator=g)).double(), gamma=(0.8 + 0.4 * torch.rand(N, generator=g)).double(),
             beta=(0.2 * torch.randn(N, generator=g)).double())
    mean, var = (0.2 * torch.randn(N, generator=g)).double(), (0.5 + torch.rand(N, generator=g)).double()
    SK = K if K == 64 else 2 * K                                                 # conv2_block1: 64 -> 256; conv5_block1: 1024 -> 2048
    if kind == "conv":
        t.update(sc_x=r16(torch.randn(B, SK, OH, OW, generator=g).relu()), sc_w=r16(torch.randn(N, SK, 1, 1, generator=g) / math.sqrt(SK)),
                 sc_b=(0.1 * torch.randn(N, generator=g)).double())
    else:
        t.update(shortcut=r16(torch.randn(B, N, IH, IW, generator=g)))
    cot_out = r16(torch.randn(B, N, OH, OW, generator=g))
    cot_pre = r16(torch.randn(B, N, OH, OW, generator=g))
    leaves = {k: v.clone().requires_grad_(True) for k, v in t.items()}
    out = F.conv2d(leaves["h"], leaves["w3"], leaves["b3"])
    if kind == "conv":
        out = out + F.conv2d(leaves["sc_x"], leaves["sc_w"], leaves["sc_b"])
    else:
        out = out + (leaves["shortcut"][:, :, ::2, ::2] if kind == "strided" else leaves["shortcut"])
    pre = torch.relu((out - mean.view(1, -1, 1, 1)) / torch.sqrt(var.view(1, -1, 1, 1) + EPS) * leaves["gamma"].view(1, -1, 1, 1)
                     + leaves["beta"].view(1, -1, 1, 1))
    ((out * cot_out).sum() + (pre * cot_pre).sum()).backward()
    ref = {"out": out.detach(), "pre": pre.detach(), **{"d" + k: v.grad for k, v in leaves.items()}}
    return t, mean, var, cot_out, cot_pre, ref, (1 if kind != "strided" else 2)


def _run_junction(fn, t, mean, var, cot_out, cot_pre, stride, dev, half):
    act = ("h", "shortcut", "sc_x")
    leaves = {k: (v.to(dev).to(half).contiguous(memory_format=torch.channels_last) if k in act else v.float().to(dev))
              .requires_grad_(True) for k, v in t.items()}
    bn = _Bn(leaves["gamma"], leaves["beta"], mean.float().to(dev), var.float().to(dev))
    out, pre = fn(leaves["h"], leaves["w3"], leaves["b3"], bn, EPS, shortcut=leaves.get("shortcut"), stride=stride,
                  sc_x=leaves.get("sc_x"), sc_w=leaves.get("sc_w"), sc_b=leaves.get("sc_b"))
    assert out.dtype == half and pre.dtype == half
    ((out.float() * cot_out.float().to(dev)).sum() + (pre.float() * cot_pre.float().to(dev)).sum()).backward()
    torch.cuda.synchronize()
    return {"out": out.detach(), "pre": pre.detach(), **{"d" + k: v.grad for k, v in leaves.items()}}


@pytest.mark.parametrize("kind", ["plain", "strided", "conv"])
@pytest.mark.parametrize("hw", [(5, 7), (8, 12)])
@pytest.mark.parametrize("K,N", [(64, 256), (512, 2048)])
def test_junction_against_fp64_within_twice_the_torch_op_twin(gpu_device, K, N, hw, kind):
    """out, pre, the gradient g at `out` (seen as the shortcut gradient: g itself for a plain block, g on the even pixels and
    exact zeros elsewhere for a strided one; through dh / dsc_x / dsc_w for a conv shortcut), dh, dW3, db3, dgamma, dbeta.
    70 rows (5 x 7, batch 2) leave ragged 32-row tiles; 192 rows (8 x 12) whole ones.

    Measured (bf16, MI355X), worst case over the 12 cases, kernel / twin relative L2 error: out 1.67e-3 / 2.51e-3, pre 2.33e-3 /
    3.60e-3; gradients kernel <= 3.91e-2, twin <= 2.91e-2, largest single ratio 1.60 (dbeta, 70 rows, strided: 3.91e-2 / 2.44e-2 --
    ReLU-mask flips between 16 and 64 bits), typical ratio 0.4 - 0.8."""
    from xpt_mde_2021_amd.hip import lib as xl, ops
    half = xl.half()
    t, mean, var, cot_out, cot_pre, ref, stride = _junction_case(K, N, hw, kind, half, seed=K + 7 * hw[0] + len(kind))
    mine = _run_junction(ops.res_join, t, mean, var, cot_out, cot_pre, stride, gpu_device, half)
    twin = _run_junction(ops.res_join_torch, t, mean, var, cot_out, cot_pre, stride, gpu_device, half)
    bad = {}
    for name, r in ref.items():
        a, b = _rel_l2(mine[name], r), _rel_l2(twin[name], r)
        print(f"K={K} N={N} {hw} {kind} {name}: kernel {a:.3e}  twin {b:.3e}")
        if not a <= 2.0 * b:
            bad[name] = (a, b)
    assert not bad, bad
    if kind == "strided":                                       # MaxPooling2D(1, 2) backward: nothing lands off the even pixels
        d = mine["dshortcut"].clone()
        d[:, :, ::2, ::2] = 0
        assert float(d.abs().max()) == 0.0


def test_junction_backward_is_bit_reproducible(gpu_device):
    from xpt_mde_2021_amd.hip import lib as xl, ops
    half = xl.half()
    t, mean, var, cot_out, cot_pre, _, stride = _junction_case(64, 256, (5, 7), "strided", half, seed=3)
    a = _run_junction(ops.res_join, t, mean, var, cot_out, cot_pre, stride, gpu_device, half)
    b = _run_junction(ops.res_join, t, mean, var, cot_out, cot_pre, stride, gpu_device, half)
    for name in a:
        assert torch.equal(a[name], b[name]), name


def test_junction_refuses_bad_shapes_before_any_launch(gpu_device):
    from xpt_mde_2021_amd.hip import lib as xl
    lib = xl.load()
    one = 16
    assert lib.xpt_res_join_fwd(one, 12, one, None, None, 0, None, None, 0, None, one, one, one, one, EPS, one, one, 70, 12, 256,
                                1, 5, 7, 5, 7, None) == -2              # K % 8
    assert lib.xpt_res_join_fwd(one, 64, one, None, None, 0, None, None, 0, None, one, one, one, one, EPS, one, one, 70, 64, 256,
                                2, 5, 7, 9, 13, None) == -3             # stride 2 without a shortcut tensor
    assert lib.xpt_res_join_fwd(one, 64, one, None, None, 0, None, None, 0, one, one, one, one, one, EPS, one, one, 70, 64, 256,
                                2, 5, 7, 8, 13, None) == -2             # pixel (2 * 4, .) outside an 8-row input map
    assert lib.xpt_res_join_bwd(None, one, one, one, one, one, one, EPS, one, None, one, 1, 70, 256, 1, 5, 7, 5, 7, None) == -4


@pytest.mark.parametrize("H,W", [(6, 10), (7, 9)])
def test_zero_padded_max_pooling_equals_the_twin_exactly(gpu_device, H, W):
    """Forward: max and zero padding are exact in any dtype.  Backward: integer cotangents (sums of up to four of them are exact
    in 16 bits), so equality means the SAME routing -- on a random map and on one built from five values, full of ties with each
    other and with the padding."""
    from xpt_mde_2021_amd.hip import lib as xl, ops
    half = xl.half()
    g = torch.Generator().manual_seed(H * 16 + W)
    maps = [torch.randn(2, 64, H, W, generator=g), torch.randint(-2, 3, (2, 64, H, W), generator=g).float()]
    for x in maps:
        outs = []
        for fn in (ops.maxpool3s2_zero, ops.maxpool3s2_zero_torch):
            xd = x.to(gpu_device).to(half).contiguous(memory_format=torch.channels_last).requires_grad_(True)
            y = fn(xd)
            cot = torch.randint(-8, 9, tuple(y.shape), generator=torch.Generator().manual_seed(1)).to(gpu_device).to(half)
            (y * cot).sum().backward()
            outs.append((y.detach(), xd.grad))
        torch.cuda.synchronize()
        assert outs[0][0].shape == (2, 64, (H - 1) // 2 + 1, (W - 1) // 2 + 1)
        assert torch.equal(outs[0][0], outs[1][0])
        assert torch.equal(outs[0][1], outs[1][1])
    neg = (-1 - torch.rand(2, 64, H, W, generator=g)).to(gpu_device).to(half)
    y = ops.maxpool3s2_zero(neg)
    assert float(y[:, :, 0].abs().max()) == 0.0 and float(y[:, :, :, 0].abs().max()) == 0.0      # the padding wins at the border


CONV_CASES = [(7, 2, 3, 8, 64, 16, 24), (3, 2, 1, 64, 64, 8, 12), (3, 2, 1, 64, 64, 7, 9), (3, 1, 1, 512, 512, 2, 3)]


@pytest.mark.parametrize("k,stride,pad,cin,cout,H,W", CONV_CASES)
def test_explicit_padding_convolution(gpu_device, k, stride, pad, cin, cout, H, W):
    """ZeroPadding2D(pad) + VALID through conv2d_same(pad=...): forward, data, weight and bias gradient against fp32 F.conv2d on
    the padded input, at the tolerances of tests/test_conv_igemm_gpu.py (6e-3 forward, 1.5e-2 gradients, of the largest magnitude)."""
    from xpt_mde_2021_amd.hip import conv as xc, lib as xl
    half = xl.half()
    g = torch.Generator().manual_seed(k * 1000 + cin + H)
    real = 3 if k == 7 else cin                                   # the stem: 3 image channels padded to 8
    x = torch.randn(2, cin, H, W, generator=g).to(half)
    x[:, real:] = 0
    w = (torch.randn(cout, real, k, k, generator=g) / math.sqrt(real * k * k)).to(half).float()
    b = 0.1 * torch.randn(cout, generator=g)
    xr, wr, br = x.float()[:, :real].clone().requires_grad_(True), w.clone().requires_grad_(True), b.clone().requires_grad_(True)
    yr = F.conv2d(F.pad(xr, (pad, pad, pad, pad)), wr, br, stride)
    gy = torch.randn(yr.shape, generator=g).to(half)
    (yr * gy.float()).sum().backward()
    xd = x.to(gpu_device).contiguous(memory_format=torch.channels_last).requires_grad_(True)
    wd = w.to(gpu_device).contiguous(memory_format=torch.channels_last).requires_grad_(True)
    bd = b.to(gpu_device).requires_grad_(True)
    yd = xc.conv2d_same(xd, wd, bd, stride, 1.0, pad=pad)
    assert yd.shape == yr.shape and yd.dtype == half
    (yd.float() * gy.to(gpu_device).float()).sum().backward()
    torch.cuda.synchronize()
    for what, a, r, tol in (("forward", yd, yr, 6e-3), ("data gradient", xd.grad[:, :real], xr.grad, 1.5e-2),
                            ("weight gradient", wd.grad, wr.grad, 1.5e-2), ("bias gradient", bd.grad, br.grad, 1.5e-2)):
        err = float((a.detach().float().cpu() - r.detach()).abs().max() / (r.detach().abs().max() + 1e-12))
        print(f"{k}x{k}/{stride} pad {pad} {cin}->{cout} {H}x{W} {what}: {err:.3e}")
        assert err < tol, (what, err)
