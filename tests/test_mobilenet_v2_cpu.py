"""MobileNetV2 backbone without a GPU: structure pins, fp64 parity of the encoder's host path with the independent restatement
(tests/ref_mobilenet_v2.py), the Keras weight map, fp64 gradcheck of the block arithmetic, factory dispatch and the C ABI's
argument check.  (Reference: tf.keras.applications.MobileNetV2 behind model/build_model/pretrained_nets.py:31-34.)"""
import ctypes
import json
import os

import pytest
import torch

from tests import ref_mobilenet_v2 as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MANIFEST = os.path.join(ROOT, "tests", "golden", "mobilenet_v2_manifest.json")


def _encoder(dtype=torch.float64):
    from xpt_mde_2021_amd.model.build_model import mobilenet_v2 as mv2
    torch.manual_seed(0)
    return mv2, mv2.MobileNetV2Encoder().to(dtype)


@pytest.fixture(scope="module")
def loaded():
    """(module, encoder in fp64 filled with the restatement's random weights, those weights)."""
    mv2, enc = _encoder()
    weights = ref.random_weights(3)
    assert mv2.load_keras_weights(enc, weights) == len(weights)
    return mv2, enc, weights


def test_parameter_count_is_keras_published_number():
    _, enc = _encoder(torch.float32)
    trainable = sum(p.numel() for p in enc.parameters())
    frozen = sum(b.numel() for b in enc.buffers())
    assert trainable == 2_223_872
    assert frozen == 34_112 == 2 * 17_056
    assert trainable + frozen == 2_257_984
    assert sum(int(torch.tensor(s).prod()) for s in ref.manifest().values()) == 2_257_984


def test_manifest_file_is_the_restatement():
    disk = json.load(open(MANIFEST))
    assert [(k, tuple(v)) for k, v in disk["variables"]] == list(ref.manifest().items())


def test_tap_sizes_of_a_256_by_384_image():
    _, enc = _encoder(torch.float32)
    with torch.no_grad():
        taps = enc(torch.rand(1, 3, 256, 384) * 2 - 1)
    assert [tuple(t.shape) for t in taps] == [(1, 96, 128, 192), (1, 144, 64, 96), (1, 192, 32, 48), (1, 576, 16, 24),
                                              (1, 1280, 8, 12)]
    assert enc.TAP_CHANNELS == (96, 144, 192, 576, 1280) and enc.tap_layout() == [(c, None) for c in enc.TAP_CHANNELS]
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
        assert float(b.abs().max()) > 0 and float((b == 0).double().mean()) < 0.9, name      # a live comparison
        err = float((a - b).abs().max() / b.abs().max())
        print(f"{name}: relative error {err:.2e}, at 0 {float((b == 0).double().mean()):.2f}, at 6 {float((b == 6).double().mean()):.3f}")
        assert err <= 1e-10, (name, err)


def test_keras_variables_cover_the_encoder_exactly(loaded):
    mv2, enc, weights = loaded
    table = mv2.keras_variable_map(enc)
    manifest = {k: tuple(v) for k, v in json.load(open(MANIFEST))["variables"]}
    assert set(table) == set(manifest)
    tensors = {id(t) for t, _ in table.values()}
    assert len(tensors) == len(table)                                        # every variable its own tensor
    assert tensors == {id(t) for t in list(enc.parameters()) + list(enc.buffers())}     # every tensor filled
    exported = mv2.export_keras_weights(enc)
    for name, shape in manifest.items():
        assert tuple(exported[name].shape) == shape, name
    _, other = _encoder()
    mv2.load_keras_weights(other, exported)
    again = mv2.export_keras_weights(other)
    assert all(torch.equal(exported[k], again[k]) for k in exported)          # export -> load round trip is the identity
    assert all(torch.equal(exported[k], weights[k].float()) for k in exported)


def test_missing_extra_and_misshaped_variables_raise(loaded):
    mv2, enc, weights = loaded
    from xpt_mde_2021_amd.utils.util_class import WrongInputException
    w = dict(weights)
    del w["block_7_depthwise_BN/beta"]
    with pytest.raises(WrongInputException):
        mv2.load_keras_weights(enc, w)
    w = dict(weights)
    w["predictions/kernel"] = torch.zeros(1280, 1000)
    with pytest.raises(WrongInputException):
        mv2.load_keras_weights(enc, w)
    w = dict(weights)
    w["block_3_depthwise/depthwise_kernel"] = torch.zeros(3, 3, 1, 144)
    with pytest.raises(WrongInputException):
        mv2.load_keras_weights(enc, w)


@pytest.mark.parametrize("stride,cin,cout", [(1, 8, 8), (2, 8, 16)])
def test_block_gradcheck_fp64(stride, cin, cout):
    """One stride-1 residual block and one stride-2 block (host path) at 1 x 8 x 4 x 6; the inputs of both clamps
    (expand and depthwise BatchNorm outputs) are checked to lie away from the kinks, where a finite difference would straddle them."""
    from xpt_mde_2021_amd.model.build_model import mobilenet_v2 as mv2
    torch.manual_seed(stride)
    block = mv2.InvertedResidual(cin, cout, stride, 6).double()
    assert block.use_res == (stride == 1)
    with torch.no_grad():
        for bn in (block.expand_bn, block.depthwise_bn, block.project_bn):
            bn.running_mean.normal_(0, 0.2)
            bn.running_var.uniform_(0.5, 1.5)
            bn.weight.uniform_(0.8, 1.2)
            bn.bias.normal_(0, 0.5)
    x = torch.randn(1, cin, 4, 6, dtype=torch.float64).mul_(1.5).requires_grad_(True)
    params = [p for p in block.parameters()]

    def fn(x, *ps):
        return block(x)[0]

    def kink_distance():
        """Smallest distance of BOTH clamp inputs -- the expand BatchNorm's output and the depthwise BatchNorm's output -- from
        the kinks at 0 and 6, and how much of each clamp is live."""
        import torch.nn.functional as F
        with torch.no_grad():
            _, pre = block(x)
            a = pre.clamp(0, 6)
            if stride == 2:
                a = F.pad(a, (0, 1, 0, 1))                        # correct_pad of the even 4 x 6 map
            u = F.conv2d(a, block.depthwise.weight, None, stride, 1 if stride == 1 else 0, 1, a.shape[1])
            bn = block.depthwise_bn
            mid = F.batch_norm(u, bn.running_mean, bn.running_var, bn.weight, bn.bias, False, 0.0, 1e-3)
            d = min(float(torch.cat([t.flatten().abs(), (t - 6).flatten().abs()]).min()) for t in (pre, mid))
            return d, float((pre > 0).double().mean()), float((mid > 0).double().mean())

    d, live, live_mid = kink_distance()
    assert d > 1e-4 and 0.2 < live < 0.9 and 0.1 < live_mid < 0.95, (d, live, live_mid)
    assert torch.autograd.gradcheck(fn, (x, *params), eps=1e-6, atol=1e-6, rtol=1e-5)


def test_model_factory_builds_mobilenet_and_still_refuses_vgg():
    from xpt_mde_2021_amd.model.build_model.model_factory import ModelFactory
    from xpt_mde_2021_amd.model.build_model.mobilenet_v2 import MobileNetV2Encoder
    from xpt_mde_2021_amd.utils.util_class import WrongInputException
    cfg = {"imshape": (5, 64, 96, 3)}
    model = ModelFactory(cfg, global_batch=2, net_names={"depth": "MobileNetV2", "camera": "PoseNetImproved"},
                         pretrained_weight=False).get_model()
    depth = model.models["depthnet"]
    assert isinstance(depth.encoder, MobileNetV2Encoder)
    # the decoder's dense layers at the new widths
    assert depth.up4.conv1.conv.weight.shape[:2] == (256, 1280) and depth.up4.conv2.conv.weight.shape[:2] == (256, 256 + 576)
    assert depth.up3.conv2.conv.weight.shape[:2] == (128, 128 + 192) and depth.up2.conv2.conv.weight.shape[:2] == (64, 64 + 144 + 1)
    assert depth.up1.conv2.conv.weight.shape[:2] == (32, 32 + 96 + 1)
    with pytest.raises(WrongInputException):
        ModelFactory(cfg, global_batch=2, net_names={"depth": "VGG16", "camera": "PoseNetImproved"},
                     pretrained_weight=False).get_model()
    with pytest.raises(WrongInputException, match="XPT_MOBILENETV2_WEIGHTS"):
        os.environ.pop("XPT_MOBILENETV2_WEIGHTS", None)
        ModelFactory(cfg, global_batch=2, net_names={"depth": "MobileNetV2"}, pretrained_weight=True).get_model()


def test_depthwise_stage_rejects_channels_that_are_no_multiple_of_8_through_both_libraries():
    import __graft_entry__ as ge
    from xpt_mde_2021_amd.hip import lib as xl
    if not (os.path.isfile(xl.LIB_PATH) and os.path.isfile(xl.LIB_PATH_F16)):
        ge.build()
    one = ctypes.c_void_p(16)            # never dereferenced: the argument check fails first
    for path in (xl.LIB_PATH, xl.LIB_PATH_F16):
        lib = ctypes.CDLL(path)
        restype, argtypes = xl.SIGNATURES["xpt_dwconv_bn_relu6_fwd"]
        lib.xpt_dwconv_bn_relu6_fwd.restype, lib.xpt_dwconv_bn_relu6_fwd.argtypes = restype, argtypes
        args = lambda C: (one, one, one, one, one, one, 1e-3, one, 1, 4, 6, C, 1, 1, 1, 4, 6, 1, None)      # noqa: E731
        assert lib.xpt_dwconv_bn_relu6_fwd(*args(12)) == -3                     # XPT_ERR_ARG, before any launch
        restype, argtypes = xl.SIGNATURES["xpt_dwconv_bn_relu6_bwd"]
        lib.xpt_dwconv_bn_relu6_bwd.restype, lib.xpt_dwconv_bn_relu6_bwd.argtypes = restype, argtypes
        assert lib.xpt_dwconv_bn_relu6_bwd(one, one, one, 12, one, one, one, one, 1e-3, one, one, 10 ** 9, 1, 4, 6, 12, 1, 1, 1, 4, 6,
                                           1, None) == -3
        lib.xpt_dwconv_bn_relu6_bwd_chunks.restype = ctypes.c_int
        assert lib.xpt_dwconv_bn_relu6_bwd_chunks(2, 4, 6, 16) >= 1
