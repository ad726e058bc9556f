"""The depth decoder's two FixedOptions choices off the GPU: DEPTH_UPSAMPLE_INTERP = "bilinear" (the interpolation the dense
convolutions read through, restated as explicit 0.75 / 0.25 stencils, and its adjoint) and DEPTH_ACTIVATION = "Exponential"
(ExponentialActivation with InverseSigmoidActivation's with_disparity contract), and that the factory carries both into the model."""
import pytest
import torch
import torch.nn.functional as F

# the sizes at which both clamps meet (1 x 1: every tap clamps; 1 x 5, 2 x 3: one axis without an interior; 5 x 4: interior pixels)
MAPS = [(1, 1), (1, 5), (2, 3), (5, 4)]


@pytest.mark.parametrize("h,w", MAPS)
def test_stencil_twin_equals_interpolate(h, w):
    from xpt_mde_2021_amd.hip import ops
    g = torch.Generator().manual_seed(h * 17 + w)
    x = torch.randn(2, 3, h, w, generator=g, dtype=torch.float64)
    ref = F.interpolate(x, scale_factor=2, mode="bilinear", align_corners=False)
    out = ops.upsample2x_bilinear_torch(x)
    assert out.shape == ref.shape == (2, 3, 2 * h, 2 * w)
    assert float((out - ref).abs().max()) <= 1e-12


@pytest.mark.parametrize("h,w", MAPS)
def test_adjoint_formula_equals_autograd_of_the_twin(h, w):
    """The gather the data-gradient kernel implements (border outputs count 1.0: their clamped tap fell onto the border pixel)
    is the autograd gradient of the twin -- and of F.interpolate -- for an arbitrary cotangent."""
    from xpt_mde_2021_amd.hip import ops
    g = torch.Generator().manual_seed(h * 31 + w)
    x = torch.randn(2, 3, h, w, generator=g, dtype=torch.float64, requires_grad=True)
    cot = torch.randn(2, 3, 2 * h, 2 * w, generator=g, dtype=torch.float64)
    (ops.upsample2x_bilinear_torch(x) * cot).sum().backward()
    adj = ops.upsample2x_bilinear_adjoint_torch(cot)
    assert adj.shape == x.shape
    assert float((adj - x.grad).abs().max()) <= 1e-12
    x2 = x.detach().clone().requires_grad_(True)
    (F.interpolate(x2, scale_factor=2, mode="bilinear", align_corners=False) * cot).sum().backward()
    assert float((adj - x2.grad).abs().max()) <= 1e-12


def test_upsample_mode_names():
    from xpt_mde_2021_amd.hip import conv as xc
    from xpt_mde_2021_amd.hip.lib import XptHipError
    assert [xc.upsample_mode(v) for v in (False, True, "nearest", "bilinear", 0, 1, 2)] == [0, 1, 1, 2, 0, 1, 2]
    with pytest.raises(XptHipError):
        xc.upsample_mode("bicubic")


def test_exponential_with_disparity_host_path():
    from xpt_mde_2021_amd.model.build_model.model_factory import ExponentialActivation
    from xpt_mde_2021_amd.utils import util_funcs as uf
    act = ExponentialActivation()
    g = torch.Generator().manual_seed(5)
    xs = [torch.rand(2, 1, h, w, generator=g) * 24 - 12 for h, w in ((2, 3), (4, 6), (8, 12), (16, 24))]
    depth, disp = act.with_disparity(xs[0])
    assert torch.equal(depth, act(xs[0])) and torch.equal(disp, uf.safe_reciprocal_number(act(xs[0])))
    depths, disps = act.with_disparity_multi(xs)
    assert len(depths) == len(disps) == 4
    for x, d, s in zip(xs, depths, disps):
        assert torch.equal(d, act(x)) and torch.equal(s, uf.safe_reciprocal_number(act(x)))
    # differentiable: d depth / dx = 10 depth sg (1 - sg)
    x = xs[1].clone().requires_grad_(True)
    d, s = act.with_disparity(x)
    (d.sum() + s.sum()).backward()
    sg = torch.sigmoid(xs[1] + 1)
    expect = (1 - 1 / d.detach() ** 2) * d.detach() * 10 * sg * (1 - sg)
    assert torch.allclose(x.grad, expect, rtol=1e-4, atol=1e-6)


def test_factory_carries_both_options_and_the_cpu_forward_emits_disp_ms():
    from xpt_mde_2021_amd.config import opts
    from xpt_mde_2021_amd.model.build_model import depth_net as dn
    from xpt_mde_2021_amd.model.build_model.model_factory import ExponentialActivation, ModelFactory
    saved = opts.DEPTH_UPSAMPLE_INTERP
    opts.DEPTH_UPSAMPLE_INTERP = "bilinear"
    try:
        torch.manual_seed(0)
        model = ModelFactory({"imshape": (64, 96, 3)}, global_batch=1, net_names={"depth": "MobileNetV2"},
                             depth_activation="Exponential", pretrained_weight=False).get_model()
    finally:
        opts.DEPTH_UPSAMPLE_INTERP = saved
    depthnet = model.models["depthnet"]
    ups = [m for m in depthnet.modules() if isinstance(m, dn.UpconvWithSkip)]
    assert len(ups) == 5 and all(m.interp == "bilinear" for m in ups)
    assert isinstance(depthnet.depth0.predict_depth, ExponentialActivation)
    g = torch.Generator().manual_seed(1)
    image5d = torch.rand(1, 3, 64, 96, 3, generator=g) * 2 - 1
    with torch.no_grad():
        out = depthnet(image5d)
    assert "disp_ms" in out and len(out["disp_ms"]) == 4
    for depth, disp in zip(out["depth_ms"], out["disp_ms"]):
        assert depth.shape == disp.shape and torch.isfinite(depth).all()
        assert torch.allclose(disp, 1 / depth)
