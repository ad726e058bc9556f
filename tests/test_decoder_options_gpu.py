"""DEPTH_UPSAMPLE_INTERP = "bilinear" as an operand-load mode of the dense convolutions (conv2d_same(..., upsample="bilinear"):
no up-sampled tensor in HBM) and DEPTH_ACTIVATION = "Exponential" in the batched head launch, on the GPU.

Accuracy bars: nobody had measured these errors, so the SAME relative quantity (max abs error over the largest reference
magnitude, as tests/test_conv_igemm_gpu.py computes it) is measured for the framework route -- 16-bit F.interpolate followed by
conv2d_same without up-sampling, the XPT_DEBUG_ATEN_BILINEAR route -- against the same fp32 reference, and the fused route is
allowed twice that: the accumulation order differs, the rounding points do not.  Both figures are printed; DESIGN.md section 12
records what has been measured on an MI355X.

Every bilinear-mode shape runs on the same kernel families (the library has the mode in one family per direction): forward =
the halo-tile kernel of xpt_conv2d_fwd, weight gradient = the general kernel of xpt_conv2d_bwd_weight_partials, data gradient =
the mode-0 data gradient (family printed per case) + the adjoint launch."""
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

WIDTHS = [(1056, 256), (2048, 256), (256, 128), (128, 64), (64, 32), (32, 16)]       # conv1 of up4 (NASNet, ResNet) .. up0
# batch 2; 2 x 3 and 4 x 6: every pixel at or next to a clamped edge; 17 x 23 / 9 x 40: tile remainders, both parities, interior
CASES = [(ci, co, h, w) for (ci, co) in WIDTHS for (h, w) in ((2, 3), (4, 6))] + [(64, 32, 17, 23), (32, 16, 9, 40)]


def _rel(a, r):
    return float((a.detach().float().cpu() - r.detach()).abs().max() / (r.detach().abs().max() + 1e-12))


def _dgrad_family(lib, B, cp, n, H, W):
    """which family serves the mode-0 data gradient of the up-sampled map (the library's own queries)"""
    if lib.xpt_conv2d_splitk_workspace_floats(B * H * W, cp, n, 9, 1):
        return "split-K"
    if lib.xpt_conv2d_stream_serves(B, H, W, cp, n, 3, 3, 1, 0):
        return "persistent"
    return "general"


def _run_gpu(xc, dev, x, w, b, gy, route):
    """(y, dx, dw, db) of one forward + backward on the GPU; route: "bilinear" | "nearest" (fused) or "framework"."""
    xd = x.to(dev).contiguous(memory_format=torch.channels_last).requires_grad_(True)
    wd = w.to(dev).contiguous(memory_format=torch.channels_last).requires_grad_(True)
    bd = b.to(dev).requires_grad_(True)
    if route == "framework":
        up = F.interpolate(xd, scale_factor=2, mode="bilinear", align_corners=False)
        y = xc.conv2d_same(up, wd, bd, 1, 0.1)
    else:
        y = xc.conv2d_same(xd, wd, bd, 1, 0.1, upsample=route)
    (y.float() * gy.to(dev).float()).sum().backward()
    torch.cuda.synchronize()
    return y, xd.grad, wd.grad, bd.grad


@pytest.mark.parametrize("cin,cout,H,W", CASES)
def test_bilinear_conv_layer_against_fp32_within_twice_the_framework_route(gpu_device, cin, cout, H, W):
    from xpt_mde_2021_amd.hip import conv as xc, lib as xl
    half, lib = xl.half(), xl.load()
    g = torch.Generator().manual_seed(cin * 131 + cout * 7 + H)
    x = torch.randn(2, cin, H, W, generator=g).to(half)
    w = (torch.randn(cout, cin, 3, 3, generator=g) / math.sqrt(cin * 9)).to(half).float()
    b = 0.1 * torch.randn(cout, generator=g)
    xr, wr, br = x.float().requires_grad_(True), w.clone().requires_grad_(True), b.clone().requires_grad_(True)
    yr = F.leaky_relu(F.conv2d(F.interpolate(xr, scale_factor=2, mode="bilinear", align_corners=False), wr, br, 1, 1), 0.1)
    gy = torch.randn(yr.shape, generator=g).to(half)
    (yr * gy.float()).sum().backward()
    refs = (yr, xr.grad, wr.grad, br.grad)
    print(f"{cin}->{cout} {H}x{W}: forward halo-tile (bilinear), weight gradient general kernel "
          f"({lib.xpt_conv2d_bwd_weight_splits_mode(2, cin, cout, 3, 3, 1, 2 * H, 2 * W, 2)} splits), data gradient "
          f"{_dgrad_family(lib, 2, cin, cout, 2 * H, 2 * W)} + adjoint")
    fused = _run_gpu(xc, gpu_device, x, w, b, gy, "bilinear")
    frame = _run_gpu(xc, gpu_device, x, w, b, gy, "framework")
    assert fused[0].shape == yr.shape and fused[0].dtype == half and fused[1].shape == x.shape
    errs = []
    for what, a, f_, r in zip(("forward", "data gradient", "weight gradient", "bias gradient"), fused, frame, refs):
        e_fused, e_frame = _rel(a, r), _rel(f_, r)
        errs.append((what, e_fused, e_frame))
        print(f"  {what}: fused {e_fused:.3e}  framework {e_frame:.3e}")
    # live-ness: the nearest mode is far from the bilinear reference, i.e. the mode was not ignored
    near = _rel(_run_gpu(xc, gpu_device, x, w, b, gy, "nearest")[0], yr)
    print(f"  forward in nearest mode against the bilinear reference: {near:.3e}")
    for what, e_fused, e_frame in errs:
        assert e_fused <= 2.0 * e_frame, (what, e_fused, e_frame)
    assert near > 10.0 * errs[0][1], (near, errs[0][1])


def test_bilinear_borders_equal_the_framework_route_exactly(gpu_device):
    """A 16-bit-exact input that is zero but for one corner and one edge pixel, read through a centre-tap identity on 8
    channels: the output IS the interpolated operand (0.75 / 0.25 products of small integers: exact in either format), so
    it equals the framework route element for element; so does the data gradient of sum(y)."""
    from xpt_mde_2021_amd.hip import conv as xc, lib as xl
    half = xl.half()
    x = torch.zeros(2, 8, 3, 5)
    x[0, :, 0, 0] = torch.arange(1, 9).float()          # corner: both clamps
    x[1, :, 2, 3] = -2.0 * torch.arange(1, 9).float()   # bottom edge: one clamp
    x[0, :, 1, 4] = 4.0                                 # right edge
    w = torch.zeros(8, 8, 3, 3)
    w[torch.arange(8), torch.arange(8), 1, 1] = 1.0
    outs = {}
    for route in ("bilinear", "framework"):
        xd = x.to(half).to(gpu_device).contiguous(memory_format=torch.channels_last).requires_grad_(True)
        wd = w.to(gpu_device).contiguous(memory_format=torch.channels_last).requires_grad_(True)
        if route == "framework":
            y = xc.conv2d_same(F.interpolate(xd, scale_factor=2, mode="bilinear", align_corners=False), wd, None, 1, 1.0)
        else:
            y = xc.conv2d_same(xd, wd, None, 1, 1.0, upsample="bilinear")
        y.float().sum().backward()
        torch.cuda.synchronize()
        outs[route] = (y.detach().float().cpu(), xd.grad.float().cpu())
    expect = F.interpolate(x, scale_factor=2, mode="bilinear", align_corners=False)
    assert torch.equal(outs["bilinear"][0], outs["framework"][0])
    assert torch.equal(outs["bilinear"][0], expect)
    assert float(outs["bilinear"][0][0, 0, 0, 0]) == 1.0 and float(outs["bilinear"][0][0, 0, 1, 1]) == 0.5625
    assert torch.equal(outs["bilinear"][1], outs["framework"][1])
    assert torch.equal(outs["bilinear"][1], torch.full_like(x, 4.0))      # every input pixel carries a total weight of 2 x 2


def _exp_reference(xs, cots):
    """fp64 formula on the same fp32 inputs: depth, disp and the gradient of sum(depth * cd + disp * cs)"""
    out = []
    for x, (cd, cs) in zip(xs, cots):
        x64 = x.double().requires_grad_(True)
        depth = torch.exp(torch.sigmoid(x64 + 1.) * 10. - 5.)
        disp = torch.where(depth > 1e-5, 1. / depth, torch.zeros_like(depth))
        ((depth * cd.double()).sum() + (disp * cs.double()).sum()).backward()
        out.append((depth.detach(), disp.detach(), x64.grad))
    return out


@pytest.mark.parametrize("maps", [((16, 24),), ((2, 3), (4, 6), (8, 12), (16, 24))], ids=["one", "four"])
def test_exponential_head_against_fp64_within_twice_the_torch_chain(gpu_device, maps):
    from xpt_mde_2021_amd.hip import ops
    from xpt_mde_2021_amd.model.build_model.model_factory import ExponentialActivation
    from xpt_mde_2021_amd.utils import util_funcs as uf
    act = ExponentialActivation()
    g = torch.Generator().manual_seed(len(maps))
    xs = [torch.rand(2, 1, h, w, generator=g) * 24 - 12 for h, w in maps]       # both sigmoid tails
    xs[-1].view(-1)[:2] = torch.tensor([-12.0, 12.0])
    cots = [(torch.randn(x.shape, generator=g), torch.randn(x.shape, generator=g)) for x in xs]
    ref = _exp_reference(xs, cots)

    def run(kernel):
        leaves = [x.to(gpu_device).requires_grad_(True) for x in xs]
        if kernel:
            depths, disps = ops.exponential_depth_multi(leaves) if len(leaves) > 1 else [[t] for t in ops.exponential_depth(leaves[0])]
        else:
            depths = [act(x) for x in leaves]
            disps = [uf.safe_reciprocal_number(d) for d in depths]
        sum((d * cd.to(gpu_device)).sum() + (s * cs.to(gpu_device)).sum() for d, s, (cd, cs) in zip(depths, disps, cots)).backward()
        torch.cuda.synchronize()
        return [(d.detach().double().cpu(), s.detach().double().cpu(), x.grad.double().cpu())
                for d, s, x in zip(depths, disps, leaves)]

    hip, chain = run(True), run(False)
    for i, (h_, c_, r_) in enumerate(zip(hip, chain, ref)):
        for what, a, c, r in zip(("depth", "disp", "gradient"), h_, c_, r_):
            e_hip = float((a - r).abs().max() / r.abs().max())
            e_chain = float((c - r).abs().max() / r.abs().max())
            print(f"map {maps[i]} {what}: kernel {e_hip:.3e}  torch fp32 chain {e_chain:.3e}")
            assert e_hip <= 2.0 * e_chain, (maps[i], what, e_hip, e_chain)
        assert h_[0].dtype == torch.float64 and hip[i][0].shape == xs[i].shape


def _trainer(mode):
    from xpt_mde_2021_amd.config import opts
    from xpt_mde_2021_amd.model import model_main as mm, train_val as tv
    torch.manual_seed(0)
    dataset, cfg, _ = mm.get_dataset("synthetic", "train", True)
    model, aug, loss_object, optimizer = mm.create_training_parts(0, cfg, 1e-4, opts.LOSS_RIGID_T1, opts.SCALE_WEIGHT_T1,
                                                                  {"depth": "MobileNetV2", "camera": "PoseNetImproved"},
                                                                  ckpt_name="__decoder_options__")
    trainer, _ = tv.train_val_factory(mode, model, loss_object, 0, False, None, optimizer)
    return trainer, dataset, optimizer


def test_training_step_with_both_options_captured_equals_eager(gpu_device, monkeypatch):
    """{"depth": "MobileNetV2", "camera": "PoseNetImproved"} with DEPTH_UPSAMPLE_INTERP = "bilinear" and DEPTH_ACTIVATION =
    "Exponential", batch 2 at 64 x 96: three eager and three captured steps from one seed leave bit-identical flat weights and
    equal finite losses; no memset node, no library convolution, NO call of torch.nn.functional.interpolate (the up-sampling
    is the convolutions' operand load) and the decoder hands out disp_ms (the batched head launch)."""
    from xpt_mde_2021_amd.config import opts
    from xpt_mde_2021_amd.model.build_model import depth_net as dn
    from xpt_mde_2021_amd.model.model_util import layer_ops as lo
    calls, decoded = [], []
    real_interpolate, real_decode = F.interpolate, dn.DepthNetPretrained.decode

    def counting_interpolate(*args, **kwargs):
        calls.append(kwargs.get("mode"))
        return real_interpolate(*args, **kwargs)

    def recording_decode(self, *args, **kwargs):
        out = real_decode(self, *args, **kwargs)
        decoded.append("disp_ms" in out and len(out["disp_ms"]) == 4)
        return out

    saved = (opts.PER_REPLICA_BATCH, opts.BATCH_SIZE, dict(opts.IMAGE_SIZES), opts.DEPTH_UPSAMPLE_INTERP, opts.DEPTH_ACTIVATION)
    opts.PER_REPLICA_BATCH = opts.BATCH_SIZE = 2
    opts.IMAGE_SIZES["kitti_raw"] = (64, 96)
    opts.DEPTH_UPSAMPLE_INTERP, opts.DEPTH_ACTIVATION = "bilinear", "Exponential"
    monkeypatch.setattr(torch.nn.functional, "interpolate", counting_interpolate)
    monkeypatch.setattr(dn.DepthNetPretrained, "decode", recording_decode)
    try:
        before = lo.LIBRARY_CONV_CALLS[0]
        runs = {}
        for mode in ("eager", "graph"):
            trainer, dataset, optimizer = _trainer(mode)
            ups = [m for m in trainer.model.models["depthnet"].modules() if isinstance(m, dn.UpconvWithSkip)]
            assert len(ups) == 5 and all(m.interp == "bilinear" for m in ups)
            del calls[:]
            losses = [float(trainer.run_a_batch(dataset.batches[i % len(dataset.batches)])[1]) for i in range(3)]
            torch.cuda.synchronize()
            runs[mode] = (losses, optimizer.flat.data.clone(), trainer, list(calls))
        assert lo.LIBRARY_CONV_CALLS[0] == before, "a convolution of the step went to the library"
    finally:
        opts.PER_REPLICA_BATCH, opts.BATCH_SIZE = saved[:2]
        opts.IMAGE_SIZES.clear()
        opts.IMAGE_SIZES.update(saved[2])
        opts.DEPTH_UPSAMPLE_INTERP, opts.DEPTH_ACTIVATION = saved[3:]
    graph = runs["graph"][2]._graph
    assert graph.graph is not None and not graph.library_path, "the step was not captured"
    print("census", graph.census, "losses", runs["graph"][0])
    assert graph.census["memset"] == 0 and graph.census["kernel"] > 100
    assert all(math.isfinite(v) for v in runs["graph"][0])
    assert runs["eager"][0] == runs["graph"][0], (runs["eager"][0], runs["graph"][0])
    assert torch.equal(runs["eager"][1], runs["graph"][1])
    assert runs["eager"][3] == [] and runs["graph"][3] == [], (runs["eager"][3], runs["graph"][3])
    assert decoded and all(decoded), decoded
