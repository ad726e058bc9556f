"""The Keras weight path of every DepthNetPretrained backbone, on the CPU with random weights: export -> load is the identity on
every tensor (NASNet's structurally-zero entries included), a load that fails changes nothing, and the message of a failed load
names the backbone."""
import functools

import pytest
import torch

BACKBONES = {"NASNetMobile": "NASNet-Mobile weights", "MobileNetV2": "MobileNetV2 weights",
             "EfficientNetB0": "EfficientNetB0 weights", "ResNet50V2": "ResNet50V2 weights"}


@functools.lru_cache(maxsize=None)
def backbone(name):
    """(module with keras_variable_map / load_keras_weights / export_keras_weights, encoder filled with random variables)."""
    from xpt_mde_2021_amd.model.build_model import efficientnet, mobilenet_v2, pretrained_nets, resnet_v2
    module, make = {"NASNetMobile": (pretrained_nets, pretrained_nets.NASNetMobileEncoder),
                    "MobileNetV2": (mobilenet_v2, mobilenet_v2.MobileNetV2Encoder),
                    "EfficientNetB0": (efficientnet, lambda: efficientnet.EfficientNetEncoder("EfficientNetB0")),
                    "ResNet50V2": (resnet_v2, resnet_v2.ResNet50V2Encoder)}[name]
    torch.manual_seed(11)
    encoder = make()
    g = torch.Generator().manual_seed(12)
    noise = {k: torch.randn(v.shape, generator=g) for k, v in module.export_keras_weights(encoder).items()}
    assert module.load_keras_weights(encoder, noise) == len(noise)
    return module, encoder


def tensors_of(module, encoder):
    return [t for t, _ in module.keras_variable_map(encoder).values()]


def snapshot(module, encoder):
    return [t.detach().clone() for t in tensors_of(module, encoder)]


def unchanged(module, encoder, before):
    return all(torch.equal(t.detach(), b) for t, b in zip(tensors_of(module, encoder), before))


@pytest.mark.parametrize("name", BACKBONES)
def test_export_then_load_restores_every_tensor_bit_for_bit(name):
    module, encoder = backbone(name)
    before = snapshot(module, encoder)
    # (cloned: on the CPU an exported fp32 vector IS the encoder's tensor, nothing converts or copies it)
    exported = {k: v.clone() for k, v in module.export_keras_weights(encoder).items()}
    assert all(v.dtype == torch.float32 and v.device.type == "cpu" and v.is_contiguous() for v in exported.values())
    g = torch.Generator().manual_seed(13)
    with torch.no_grad():
        for t in tensors_of(module, encoder):
            t.copy_(torch.randn(t.shape, generator=g) + 3.0)               # (no entry keeps its value, 0.0 or 1.0 by accident)
    assert not any(torch.equal(t.detach(), b) for t, b in zip(tensors_of(module, encoder), before))
    assert module.load_keras_weights(encoder, exported) == len(exported)
    assert unchanged(module, encoder, before)
    if name == "NASNetMobile":
        # the entries no Keras variable addresses: 0 again, 1 for a moving variance
        from xpt_mde_2021_amd.model.build_model.pretrained_nets import logical_entries
        sel = logical_entries(encoder)
        checked = 0
        for key, (t, _) in module.keras_variable_map(encoder).items():
            if id(t) not in sel:
                continue
            o, i = sel[id(t)]
            structural = torch.ones_like(t, dtype=torch.bool)
            rows = o if o is not None else torch.arange(t.shape[0])
            if i is not None:
                structural[rows[:, None], i[None, :]] = False
            else:
                structural[rows] = False
            assert bool(structural.any()), key
            fill = 1.0 if key.endswith("/moving_variance") else 0.0
            assert bool((t.detach()[structural] == fill).all()), key
            checked += 1
        assert checked > 0


@pytest.mark.parametrize("name", BACKBONES)
def test_a_load_that_fails_on_the_last_variable_changes_nothing(name):
    module, encoder = backbone(name)
    from xpt_mde_2021_amd.utils.util_class import WrongInputException
    before = snapshot(module, encoder)
    g = torch.Generator().manual_seed(14)
    weights = {k: torch.randn(v.shape, generator=g) for k, v in module.export_keras_weights(encoder).items()}
    last = list(module.keras_variable_map(encoder))[-1]
    weights[last] = torch.zeros(tuple(weights[last].shape) + (2,))
    with pytest.raises(WrongInputException, match=last):
        module.load_keras_weights(encoder, weights)
    assert unchanged(module, encoder, before)


@pytest.mark.parametrize("name", BACKBONES)
def test_a_missing_variable_is_reported_under_the_backbones_label(name):
    module, encoder = backbone(name)
    from xpt_mde_2021_amd.utils.util_class import WrongInputException
    before = snapshot(module, encoder)
    weights = module.export_keras_weights(encoder)
    gone = sorted(weights)[len(weights) // 2]
    del weights[gone]
    with pytest.raises(WrongInputException, match=f"^{BACKBONES[name]}: 1 variables missing") as info:
        module.load_keras_weights(encoder, weights)
    assert gone in str(info.value)
    assert unchanged(module, encoder, before)
