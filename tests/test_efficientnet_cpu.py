"""EfficientNet backbones without a GPU: structure pins of B0 / B3 / B5 / B7, fp64 parity of the B0 encoder's host path with the
independent restatement (tests/ref_efficientnet.py), the Keras weight map, fp64 gradcheck of the MBConv middle's torch twin,
factory dispatch and the C ABI's argument checks.  (Reference: tf.keras.applications.EfficientNetB<n> behind
model/build_model/pretrained_nets.py:11-117; config-example.py RIGID_EF0 / EF3 / EF5 / EF7.)"""
import ctypes
import json
import os
import types

import pytest
import torch

from tests import ref_efficientnet as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MANIFEST = os.path.join(ROOT, "tests", "golden", "efficientnet_b0_manifest.json")


def _encoder(dtype=torch.float64, name="EfficientNetB0"):
    from xpt_mde_2021_amd.model.build_model import efficientnet as eff
    torch.manual_seed(0)
    return eff, eff.EfficientNetEncoder(name).to(dtype)


@pytest.fixture(scope="module")
def loaded():
    """(module, B0 encoder in fp64 filled with the restatement's random weights, those weights)."""
    eff, enc = _encoder()
    weights = ref.random_weights(3)
    assert eff.load_keras_weights(enc, weights) == len(weights)
    return eff, enc, weights


# Keras' published no-top totals (normalization's 7 values included), block counts, tap widths
PINS = {"EfficientNetB0": (4_049_571, 16, (96, 144, 240, 672, 1280)), "EfficientNetB3": (10_783_535, 26, (144, 192, 288, 816, 1536)),
        "EfficientNetB5": (28_513_527, 39, (144, 240, 384, 1056, 2048)), "EfficientNetB7": (64_097_687, 55, (192, 288, 480, 1344, 2560))}


@pytest.mark.parametrize("name", list(PINS))
def test_parameter_count_blocks_and_tap_widths_are_keras_published_numbers(name):
    total, nblocks, widths = PINS[name]
    with torch.device("meta"):
        from xpt_mde_2021_amd.model.build_model import efficientnet as eff
        enc = eff.EfficientNetEncoder(name)
    trainable = sum(p.numel() for p in enc.parameters())
    frozen = sum(b.numel() for b in enc.buffers())
    assert trainable + frozen == total
    assert len(enc.blocks) == nblocks and enc.TAP_CHANNELS == widths and enc.out_channels == widths[-1]
    assert sum(int(torch.tensor(s).prod()) for s in ref.manifest(name[-2:]).values()) == total
    if name == "EfficientNetB0":
        assert trainable == 4_007_548 and frozen == 42_016 + 7 and frozen == 2 * 21_008 + 7


def test_manifest_file_is_the_restatement():
    disk = json.load(open(MANIFEST))
    assert [(k, tuple(v)) for k, v in disk["variables"]] == list(ref.manifest("B0").items())


def test_tap_sizes_of_a_256_by_384_image():
    _, enc = _encoder(torch.float32)
    with torch.no_grad():
        taps = enc(torch.rand(1, 3, 256, 384) * 2 - 1)
    assert [tuple(t.shape) for t in taps] == [(1, 96, 128, 192), (1, 144, 64, 96), (1, 240, 32, 48), (1, 672, 16, 24),
                                              (1, 1280, 8, 12)]
    assert enc.tap_layout() == [(c, None) for c in (96, 144, 240, 672, 1280)]
    from xpt_mde_2021_amd.utils.util_class import WrongInputException
    with pytest.raises(WrongInputException):
        enc(torch.zeros(1, 3, 48, 64))


def test_encoder_host_path_equals_the_restatement_in_fp64(loaded):
    _, enc, weights = loaded
    g = torch.Generator().manual_seed(5)
    image = torch.rand(2, 64, 96, 3, generator=g, dtype=torch.float64) * 2 - 1
    with torch.no_grad():
        mine = enc(image.permute(0, 3, 1, 2))
    theirs = ref.forward(weights, image)
    for name, a, b in zip(ref.TAP_NAMES, mine, theirs):
        b = b.permute(0, 3, 1, 2)
        assert a.shape == b.shape
        assert float(b.abs().max()) > 1e-3 and float(b.std()) > 1e-4, name                   # a live comparison
        err = float((a - b).abs().max() / b.abs().max())
        print(f"{name}: relative error {err:.2e}, max |tap| {float(b.abs().max()):.3f}, std {float(b.std()):.3f}")
        assert err <= 1e-10, (name, err)


def test_keras_variables_cover_the_encoder_exactly(loaded):
    eff, enc, weights = loaded
    table = eff.keras_variable_map(enc)
    manifest = {k: tuple(v) for k, v in json.load(open(MANIFEST))["variables"]}
    assert set(table) == set(manifest)
    tensors = {id(t) for t, _ in table.values()}
    assert len(tensors) == len(table)                                        # every variable its own tensor
    assert tensors == {id(t) for t in list(enc.parameters()) + list(enc.buffers())}     # every tensor filled
    exported = eff.export_keras_weights(enc)
    for name, shape in manifest.items():
        assert tuple(exported[name].shape) == shape, name
    _, other = _encoder()
    eff.load_keras_weights(other, exported)
    again = eff.export_keras_weights(other)
    assert all(torch.equal(exported[k], again[k]) for k in exported)          # export -> load round trip is the identity
    assert all(torch.equal(exported[k], weights[k].float()) for k in exported)


def test_missing_extra_and_misshaped_variables_raise(loaded):
    eff, enc, weights = loaded
    from xpt_mde_2021_amd.utils.util_class import WrongInputException
    before = eff.export_keras_weights(enc)
    w = dict(weights)
    del w["block5b_se_reduce/bias"]
    with pytest.raises(WrongInputException):
        eff.load_keras_weights(enc, w)
    w = dict(weights)
    w["predictions/kernel"] = torch.zeros(1280, 1000)
    with pytest.raises(WrongInputException):
        eff.load_keras_weights(enc, w)
    w = {k: torch.zeros_like(v) for k, v in weights.items()}
    w["block3a_dwconv/depthwise_kernel"] = torch.zeros(3, 3, 144, 1)          # a 5 x 5 window in the model
    with pytest.raises(WrongInputException):
        eff.load_keras_weights(enc, w)
    after = eff.export_keras_weights(enc)
    assert all(torch.equal(before[k], after[k]) for k in before)              # nothing was loaded partially


@pytest.mark.parametrize("k,stride", [(3, 1), (5, 1), (3, 2), (5, 2)])
@pytest.mark.parametrize("act_in", [True, False])
def test_mbconv_se_torch_gradcheck_fp64(k, stride, act_in):
    """hip.ops.mbconv_se_torch (the host path of mbconv_se and the yardstick of its kernels) on a 5 x 6 map, C = 8, S = 2:
    every input and parameter.  Swish has no kink."""
    from xpt_mde_2021_amd.hip import ops
    g = torch.Generator().manual_seed(10 * k + stride)
    C, S = 8, 2
    rnd = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)                    # noqa: E731
    mean, var = 0.2 * rnd(C), 0.5 + torch.rand(C, generator=g, dtype=torch.float64)
    x = rnd(2, C, 5, 6).mul_(1.5).requires_grad_(True)
    leaves = [x, (rnd(C, 1, k, k) / k).requires_grad_(True), (1.0 + 0.2 * rnd(C)).requires_grad_(True), rnd(C).requires_grad_(True),
              rnd(S, C, 1, 1).requires_grad_(True), rnd(S).requires_grad_(True), rnd(C, S, 1, 1).requires_grad_(True),
              rnd(C).requires_grad_(True)]

    def fn(x, w, gamma, beta, wr, br, we, be):
        bn = types.SimpleNamespace(weight=gamma, bias=beta, running_mean=mean, running_var=var)
        return ops.mbconv_se(x, w, bn, wr, br, we, be, k, stride, act_in=act_in, eps=1e-3)

    z = fn(*leaves)
    assert z.shape == (2, C, -(-5 // stride), -(-6 // stride))
    assert torch.autograd.gradcheck(fn, leaves, eps=1e-6, atol=1e-6, rtol=1e-5)


def test_model_factory_builds_efficientnet_and_still_refuses_densenet():
    from xpt_mde_2021_amd.model.build_model.model_factory import ModelFactory
    from xpt_mde_2021_amd.model.build_model.efficientnet import EfficientNetEncoder
    from xpt_mde_2021_amd.model.build_model.pretrained_nets import PretrainedModel
    from xpt_mde_2021_amd.utils.util_class import WrongInputException
    cfg = {"imshape": (5, 64, 96, 3)}
    model = ModelFactory(cfg, global_batch=2, net_names={"depth": "EfficientNetB0", "camera": "PoseNetImproved"},
                         pretrained_weight=False).get_model()
    depth = model.models["depthnet"]
    assert isinstance(depth.encoder, EfficientNetEncoder) and depth.encoder.net_name == "EfficientNetB0"
    # the decoder's dense layers at the new widths
    assert depth.up4.conv1.conv.weight.shape[:2] == (256, 1280) and depth.up4.conv2.conv.weight.shape[:2] == (256, 256 + 672)
    assert depth.up3.conv2.conv.weight.shape[:2] == (128, 128 + 240) and depth.up2.conv2.conv.weight.shape[:2] == (64, 64 + 144 + 1)
    assert depth.up1.conv2.conv.weight.shape[:2] == (32, 32 + 96 + 1)
    assert set(PretrainedModel.SUPPORTED) >= {"EfficientNetB0", "EfficientNetB3", "EfficientNetB5", "EfficientNetB7"}
    with pytest.raises(WrongInputException):
        ModelFactory(cfg, global_batch=2, net_names={"depth": "DenseNet121", "camera": "PoseNetImproved"},
                     pretrained_weight=False).get_model()
    for n in (0, 3, 5, 7):
        env = f"XPT_EFFICIENTNETB{n}_WEIGHTS"
        os.environ.pop(env, None)
        with pytest.raises(WrongInputException, match=env):
            ModelFactory(cfg, global_batch=2, net_names={"depth": f"EfficientNetB{n}"}, pretrained_weight=True).get_model()


def test_c_abi_rejects_bad_arguments_before_any_launch_through_both_libraries():
    import __graft_entry__ as ge
    from xpt_mde_2021_amd.hip import lib as xl
    if not (os.path.isfile(xl.LIB_PATH) and os.path.isfile(xl.LIB_PATH_F16)):
        ge.build()
    one, odd = ctypes.c_void_p(16), ctypes.c_void_p(24)          # never dereferenced: the argument check fails first
    ARG = -3                                                     # XPT_ERR_ARG; the other codes are told apart below
    for path in (xl.LIB_PATH, xl.LIB_PATH_F16):
        lib = ctypes.CDLL(path)
        fn = {}
        for name in ("xpt_dwconv_bn_swish_chunks", "xpt_dwconv_bn_swish_fwd", "xpt_se_excite_fwd", "xpt_se_scale_fwd",
                     "xpt_se_scale_bwd_reduce", "xpt_se_excite_bwd", "xpt_dwconv_bn_swish_bwd"):
            fn[name] = getattr(lib, name)
            fn[name].restype, fn[name].argtypes = xl.SIGNATURES[name]
        big = 10 ** 9

        def fwd(C=16, k=5, stride=1, pad=2, x=one, pool=big, H=4, W=6, OH=4, OW=6):
            return fn["xpt_dwconv_bn_swish_fwd"](x, one, one, one, one, one, 1e-3, one, one, pool, 1, H, W, C, k, stride, pad, pad, OH,
                                                 OW, 1, None)

        def bwd(C=16, k=5, stride=1, pad=2, pitch=16, part=big, dp=one):
            return fn["xpt_dwconv_bn_swish_bwd"](one, one, one, pitch, one, dp, one, one, one, one, 1e-3, one, one, part, 1, 4, 6, C, k,
                                                 stride, pad, pad, 4, 6, 1, None)

        ok_codes = {fwd(C=12), fwd(k=4), fwd(k=7), fwd(stride=3), fwd(pad=3), fwd(x=odd), bwd(C=12), bwd(k=4), bwd(dp=odd)}
        assert ok_codes == {ARG}, ok_codes
        shape = fwd(OH=5)                                       # a window centre below the input
        assert shape < 0 and shape != ARG
        assert bwd(pitch=12) == shape and fwd(C=0) == shape
        workspace = fwd(pool=3)
        assert workspace < 0 and workspace not in (ARG, shape) and bwd(part=5) == workspace
        assert fn["xpt_dwconv_bn_swish_fwd"](None, one, one, one, one, one, 1e-3, one, one, big, 1, 4, 6, 16, 5, 1, 2, 2, 4, 6, 1,
                                             None) not in (0, ARG, shape, workspace)            # XPT_ERR_NULL
        assert fn["xpt_dwconv_bn_swish_chunks"](2, 4, 6, 16) >= 2 and fn["xpt_dwconv_bn_swish_chunks"](2, 4, 6, 12) == 0
        assert fn["xpt_se_excite_fwd"](one, 1, 24, one, one, one, one, one, one, one, 2, 12, 4, None) == ARG
        assert fn["xpt_se_excite_fwd"](one, 1, 24, one, one, one, one, one, one, one, 2, 16, 0, None) == shape
        assert fn["xpt_se_excite_fwd"](one, 1, 24, one, one, one, one, one, one, odd, 2, 16, 4, None) == ARG
        assert fn["xpt_se_excite_fwd"](one, 1, 24, one, one, one, one, one, one, one, 2, 8192, 8192, None) == shape
        assert fn["xpt_se_scale_fwd"](one, one, one, 2, 4, 6, 12, None) == ARG
        assert fn["xpt_se_scale_fwd"](one, odd, one, 2, 4, 6, 16, None) == ARG
        assert fn["xpt_se_scale_bwd_reduce"](one, one, 12, one, big, one, 2, 4, 6, 12, None) == ARG
        assert fn["xpt_se_scale_bwd_reduce"](one, one, 20, one, big, one, 2, 4, 6, 16, None) == shape
        assert fn["xpt_se_scale_bwd_reduce"](one, one, 16, one, 7, one, 2, 4, 6, 16, None) == workspace
        assert fn["xpt_se_excite_bwd"](*([one] * 11), 2, 12, 4, None) == ARG
        assert fn["xpt_se_excite_bwd"](*([one] * 10), odd, 2, 16, 4, None) == ARG
        assert fn["xpt_se_excite_bwd"](*([one] * 11), 64, 16, 160, None) == shape
