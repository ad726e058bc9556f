"""Dynamic loss scaling of the half-precision configuration (model/model_util/loss_scale.py) without a GPU: the host-tensor
state machine through KerasAdam / KerasSGD.apply_gradients(scaler=...) and a whole CPU training step, the options, and the
C ABI of the four device entry points (declared, exported by both libraries, bound, arguments checked before any launch)."""
import ctypes
import os
import subprocess
import sys

import pytest
import torch

from xpt_mde_2021_amd.config import opts
from xpt_mde_2021_amd.model.model_util import loss_scale as ls
from xpt_mde_2021_amd.model.model_util.optimizers import FlatParameters, KerasAdam, KerasSGD
from xpt_mde_2021_amd.utils.util_class import WrongInputException

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["xpt_grad_nonfinite", "xpt_loss_scale_update", "xpt_adam_step_dyn", "xpt_sgd_step_dyn"]


def reference_rule(s0, growth, bad_steps, steps):
    """TF's DynamicLossScale update rule, written out: the expected (scale before the step, skipped?) sequence."""
    s, good, out = s0, 0, []
    for k in range(steps):
        out.append((s, k in bad_steps))
        if k in bad_steps:
            s, good = max(s / 2, 1.0), 0
        else:
            good += 1
            if good >= growth:
                s, good = s * 2, 0
    return out, s


def _flat(n=37, seed=0):
    gen = torch.Generator().manual_seed(seed)            # (a generator of its own: the global RNG stays as other tests left it)
    params = [torch.nn.Parameter(torch.randn(n, generator=gen)), torch.nn.Parameter(torch.randn(3, 5, generator=gen))]
    return params, FlatParameters(params)


@pytest.mark.parametrize("opt_cls", [KerasAdam, KerasSGD])
def test_host_state_machine_skips_halves_grows_and_floors(opt_cls):
    s0, growth = 4.0, 2
    poison = {2: float("inf"), 5: float("-inf"), 6: float("nan"), 7: float("inf"), 8: float("inf")}
    steps = 12
    expected, final = reference_rule(s0, growth, set(poison), steps)
    assert [s for s, _ in expected] == [4, 4, 8, 4, 4, 8, 4, 2, 1, 1, 1, 2]          # halving, growth, floor at 1
    params, flat = _flat()
    opt = opt_cls(1e-2)
    opt.bind(flat)
    twin = opt_cls(1e-2)                                   # the static optimizer from the same state, step by step
    twin.bind(FlatParameters([torch.nn.Parameter(p.detach().clone()) for p in params]))
    scaler = ls.DynamicLossScale(s0, growth)
    gen = torch.Generator().manual_seed(1)
    for k in range(steps):
        st = scaler.read()
        assert st["scale"] == expected[k][0] and st["inv_scale"] == 1.0 / expected[k][0] and st["found_inf"] == 0, (k, st)
        true_grad = torch.randn(flat.numel, generator=gen)
        flat.grad.copy_(true_grad * st["scale"])          # the backward pass seeded with the live scale
        if k in poison:
            flat.grad[(7 * k) % flat.numel] = poison[k]
        before = [t.clone() for t in (flat.data, opt.m, opt.v)]
        t_before = float(opt.step_count)
        twin.flat.data.copy_(flat.data)
        twin.m.copy_(opt.m)
        twin.v.copy_(opt.v)
        twin.step_count.copy_(opt.step_count)
        twin.flat.grad.copy_(flat.grad)
        opt.apply_gradients(grad_scale=1.0, scaler=scaler)
        assert float(opt.step_count) == t_before + 1                # t counts skipped steps too (as TF's iterations)
        assert bool((flat.grad == 0).all())                         # the gradient is zeroed either way
        if k in poison:
            for a, b in zip(before, (flat.data, opt.m, opt.v)):
                assert torch.equal(a.view(torch.int32), b.view(torch.int32)), k         # bit-unchanged
        else:
            twin.apply_gradients(grad_scale=1.0 / st["scale"])    # static step with grad_scale x 1/S: the same bits
            assert torch.equal(twin.flat.data, flat.data) and torch.equal(twin.m, opt.m) and torch.equal(twin.v, opt.v), k
            assert not torch.equal(before[0], flat.data), k
    st = scaler.read()
    assert st["scale"] == final == 2.0 and st["skipped"] == len(poison) and st["found_inf"] == 0
    assert bool(torch.isfinite(flat.data).all())


def test_growth_stops_at_the_largest_finite_scale():
    scaler = ls.DynamicLossScale(2.0 ** 127, 1)
    for _ in range(3):
        scaler.update()
    st = scaler.read()
    assert st["scale"] == 2.0 ** 127 and st["good_steps"] == 0 and st["inv_scale"] == 2.0 ** -127


def test_check_sees_every_kind_of_non_finite_value_and_nothing_else():
    scaler = ls.DynamicLossScale(8.0, 5)
    finite = torch.tensor([3e38, -3e38, 1e-45, -1e-45, -0.0, 0.0, 1.0], dtype=torch.float32)
    scaler.check(finite)
    assert scaler.read()["found_inf"] == 0
    for bad in (float("inf"), float("-inf"), float("nan")):
        g = finite.clone()
        g[3] = bad
        scaler.check(g)
        assert scaler.read()["found_inf"] == 1
        scaler.update()
        assert scaler.read()["found_inf"] == 0


def test_state_is_one_32_byte_int_block_with_float_views():
    scaler = ls.DynamicLossScale(2.0 ** 40, 7)
    assert scaler.state.dtype == torch.int32 and scaler.state.numel() * 4 == 32
    assert not scaler.state.is_floating_point()         # outside _StepGraph's finiteness / 1e8 bound
    assert float(scaler.scale_tensor) == 2.0 ** 40
    assert scaler.seed_like(torch.zeros(())).shape == () and scaler.seed_like(torch.zeros(1)).shape == (1,)
    assert scaler.seed_like(torch.zeros(())).data_ptr() == scaler.state.data_ptr()      # a view: the live scale


@pytest.mark.parametrize("bad", [3000.0, 0.5, 0.0, -4.0, float("inf"), float("nan"), 3.0])
def test_initial_scale_must_be_a_power_of_two(bad):
    with pytest.raises(WrongInputException):
        ls.DynamicLossScale(bad, 2000)


def test_growth_steps_must_be_positive():
    with pytest.raises(WrongInputException):
        ls.DynamicLossScale(1024.0, 0)


def test_options_are_read_from_the_environment():
    code = ("from xpt_mde_2021_amd.config import opts; "
            "print(opts.LOSS_SCALE_FP16_DYNAMIC, opts.LOSS_SCALE_GROWTH_STEPS, opts.LOSS_SCALE_FP16)")
    env = {k: v for k, v in os.environ.items() if not k.startswith("XPT_LOSS_SCALE")}
    run = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=120, env=env)
    assert run.stdout.split() == ["False", "2000", "32768.0"], run.stderr[-2000:]
    env.update(XPT_LOSS_SCALE_DYNAMIC="1", XPT_LOSS_SCALE_GROWTH_STEPS="7", XPT_LOSS_SCALE_FP16="1024")
    run = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=120, env=env)
    assert run.stdout.split() == ["True", "7", "1024.0"], run.stderr[-2000:]


# ---------------------------------------------------------------------------------------------- a whole CPU training step
class _TinyModel:
    def __init__(self):
        gen = torch.Generator().manual_seed(3)
        self.w = torch.nn.Parameter(torch.randn(6, generator=gen))
        self.b = torch.nn.Parameter(torch.randn(2, generator=gen))

    def trainable_weights(self):
        return [self.w, self.b]

    def __call__(self, features):
        return {"out": (self.w.view(2, 3) * features["x"]).sum(dim=1) + self.b}


def _tiny_loss(preds, features):
    loss = ((preds["out"] - features["y"]) ** 2).mean()
    return loss, {"sq": loss.detach()}


def _trainer(dynamic, s0, growth, monkeypatch, dtype="fp16"):
    from xpt_mde_2021_amd.model import train_val as tv
    monkeypatch.setattr(opts, "CONV_DTYPE", dtype)
    monkeypatch.setattr(opts, "LOSS_SCALE_FP16", s0)
    monkeypatch.setattr(opts, "LOSS_SCALE_FP16_DYNAMIC", dynamic)
    monkeypatch.setattr(opts, "LOSS_SCALE_GROWTH_STEPS", growth)
    model = _TinyModel()
    return tv.ModelTrainer(model, _tiny_loss, 0, False, None, KerasAdam(1e-2)), model


def _batches(n):
    g = torch.Generator().manual_seed(5)
    return [{"x": torch.randn(2, 3, generator=g), "y": torch.randn(2, generator=g)} for _ in range(n)]


def test_cpu_trainer_dynamic_equals_unscaled_without_overflow(monkeypatch):
    """Seeded with S and unscaled by 1 / S (a power of two): the same bits as the unscaled fp32 step (host tensors)."""
    static, ms = _trainer(False, 1024.0, 100, monkeypatch, dtype="fp32")
    dynamic, md = _trainer(True, 1024.0, 100, monkeypatch)
    assert static.scaler is None and dynamic.scaler is not None and dynamic.grad_unscale() == 1.0
    for f in _batches(6):
        monkeypatch.setattr(opts, "CONV_DTYPE", "fp32")
        ls_ = static.run_a_batch(f)[1]
        monkeypatch.setattr(opts, "CONV_DTYPE", "fp16")
        ld = dynamic.run_a_batch(f)[1]
        assert float(ls_) == float(ld)
    assert torch.equal(ms.w.detach(), md.w.detach()) and torch.equal(ms.b.detach(), md.b.detach())
    assert dynamic.loss_scale_state()["scale"] == 1024.0 and dynamic.loss_scale_state()["good_steps"] == 6
    assert static.loss_scale_state() is None
    assert len(dynamic.optimizer_state()) == len(static.optimizer_state()) + 1


def test_cpu_trainer_skips_a_poisoned_step_and_reports_per_epoch(monkeypatch, capsys):
    trainer, model = _trainer(True, 256.0, 2, monkeypatch)
    poison = {"on": False}
    base = trainer.reduce_gradients

    def poisoned():
        base()
        if poison["on"]:
            trainer.optimizer.flat.grad[1] = float("nan")

    trainer.reduce_gradients = poisoned
    batches = _batches(4)
    trainer.run_a_batch(batches[0])
    w = model.w.detach().clone()
    poison["on"] = True
    trainer.run_a_batch(batches[1])
    assert torch.equal(model.w.detach(), w) and trainer.loss_scale_state()["scale"] == 128.0
    poison["on"] = False
    trainer.run_an_epoch(batches[2:])                     # 2 finite steps: the scale grows back
    out = capsys.readouterr()
    assert "loss_scale=256, skipped_steps=1" in out.out and "WARNING" not in out.err
    poison["on"] = True
    trainer.run_an_epoch(batches)
    out = capsys.readouterr()
    assert "loss_scale=16, skipped_steps=4" in out.out
    assert "WARNING" in out.err and "EVERY one of the 4 steps" in out.err
    assert bool(torch.isfinite(model.w).all())


def test_cpu_trainer_rejects_a_non_power_of_two_initial_scale(monkeypatch):
    with pytest.raises(WrongInputException):
        _trainer(True, 3000.0, 2000, monkeypatch)
    trainer, _ = _trainer(False, 3000.0, 2000, monkeypatch)        # the static mode keeps accepting any scale
    assert trainer.scaler is None


def test_pieces_are_refused_in_dynamic_mode():
    params, flat = _flat(64)
    opt = KerasAdam(1e-3)
    opt.bind(flat)
    with pytest.raises(WrongInputException):
        opt.apply_gradients(lo=0, hi=32, scaler=ls.DynamicLossScale(2.0, 2))


# ---------------------------------------------------------------------------------------------- C ABI
@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    from xpt_mde_2021_amd.hip import lib as xl
    if not (os.path.isfile(xl.LIB_PATH) and os.path.isfile(xl.LIB_PATH_F16)):
        ge.build()
    return xl.load()


def test_new_symbols_are_declared_exported_by_both_builds_and_bound(lib):
    from xpt_mde_2021_amd.hip import lib as xl
    header = open(os.path.join(ROOT, "include", "xpt_hip.h")).read()
    assert "xpt_loss_scale_state" in header and "LossScaleOptimizer" in header
    f16 = ctypes.CDLL(xl.LIB_PATH_F16)
    for name in NEW_SYMBOLS:
        assert f"{name}(" in header, name
        assert hasattr(lib, name) and hasattr(f16, name), name
        assert name in xl.SIGNATURES, name


def test_new_entry_points_reject_bad_arguments_without_gpu(lib):
    null = None
    one = ctypes.c_void_p(16)          # never dereferenced: argument checks fail first
    odd = ctypes.c_void_p(20)          # not 16-byte aligned
    assert lib.xpt_grad_nonfinite(null, 8, one, null) == -1
    assert lib.xpt_grad_nonfinite(one, 8, null, null) == -1
    assert lib.xpt_grad_nonfinite(one, 0, one, null) == -2
    assert lib.xpt_grad_nonfinite(one, -5, one, null) == -2
    assert lib.xpt_grad_nonfinite(odd, 8, one, null) == -3
    assert lib.xpt_grad_nonfinite(one, 8, odd, null) == -3
    assert lib.xpt_loss_scale_update(null, 2, null) == -1
    assert lib.xpt_loss_scale_update(one, 0, null) == -3
    assert lib.xpt_loss_scale_update(odd, 2, null) == -3
    adam = lambda p, n, st: lib.xpt_adam_step_dyn(p, one, one, one, n, one, 1e-3, 0.9, 0.999, 1e-7, 1.0, 1, null, st, null)  # noqa: E731
    assert adam(one, 8, null) == -1
    assert adam(null, 8, one) == -1
    assert adam(one, 0, one) == -2
    assert adam(odd, 8, one) == -3
    assert adam(one, 8, odd) == -3
    assert lib.xpt_sgd_step_dyn(one, one, 8, 1e-3, 1.0, 1, null, null, null) == -1
    assert lib.xpt_sgd_step_dyn(null, one, 8, 1e-3, 1.0, 1, null, one, null) == -1
    assert lib.xpt_sgd_step_dyn(one, one, 0, 1e-3, 1.0, 1, null, one, null) == -2
    assert lib.xpt_sgd_step_dyn(one, one, 8, 1e-3, 1.0, 1, null, odd, null) == -3
