"""Dynamic loss scaling on the device (csrc/xpt_loss_scale.hip, the _dyn optimizer kernels of csrc/xpt_optim.hip,
model/model_util/loss_scale.py): the kernels bit for bit against their static twins and the state machine, on both builds
(the half-precision one in a child process, one 16-bit format per process), and full fp16 training runs of the bench
configuration in child processes (tools/loss_scale_train.py): dynamic == static without overflow, an injected overflow
skipped identically by the captured and the eager step, a real overflow survived, the distributed and early-update paths."""
import functools
import os
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

INF, NAN = float("inf"), float("nan")
SCALE, INV_SCALE, FOUND_INF, GOOD_STEPS, SKIPPED = 0, 1, 2, 3, 4


@pytest.fixture(scope="module")
def lib(gpu_device):
    from xpt_mde_2021_amd.hip import lib as xl
    return xl.load()


def _state(scale=1024.0, found=0, good=0, skipped=0, dev="cuda"):
    st = torch.zeros(8, dtype=torch.int32)
    st.view(torch.float32)[SCALE] = scale
    st.view(torch.float32)[INV_SCALE] = 1.0 / scale
    st[FOUND_INF], st[GOOD_STEPS], st[SKIPPED] = found, good, skipped
    st[5:] = torch.tensor([11, 12, 13], dtype=torch.int32)          # reserved words: never touched
    return st.to(dev)


def _stream():
    return torch.cuda.current_stream().cuda_stream


# ---------------------------------------------------------------------------------------------- xpt_grad_nonfinite
@pytest.mark.parametrize("n", [1, 2, 3, 4, 4096, 4097, 4098, 4099, (1 << 20) + 6])
def test_grad_nonfinite_flags_any_inf_or_nan_and_nothing_else(lib, n):
    g0 = torch.linspace(-1, 1, n, dtype=torch.float32)
    special = torch.tensor([3e38, -3e38, 1e-45, -1e-45, 1.2e-38, -0.0, 0.0], dtype=torch.float32)   # finite: extremes, subnormals, -0
    g0[:min(n, special.numel())] = special[:min(n, special.numel())]
    if n > 16:
        g0[-7:] = special
    g = g0.cuda()
    st = _state()
    assert lib.xpt_grad_nonfinite(g.data_ptr(), n, st.data_ptr(), _stream()) == 0
    torch.cuda.synchronize()
    assert torch.equal(st.cpu(), _state(dev="cpu")), "all-finite input raised the flag"
    n4 = n // 4 * 4
    positions = sorted({0, n // 2, n - 1} | ({n4} if n4 < n else set()))
    for pos in positions:
        for bad in (INF, -INF, NAN):
            h = g0.clone()
            h[pos] = bad
            h = h.cuda()
            st = _state()
            assert lib.xpt_grad_nonfinite(h.data_ptr(), n, st.data_ptr(), _stream()) == 0
            out = st.cpu()
            ref = _state(found=1, dev="cpu")
            assert torch.equal(out, ref), (n, pos, bad, out.tolist())
    # the flag is an OR: a finite gradient does not clear it
    st = _state(found=1)
    assert lib.xpt_grad_nonfinite(g.data_ptr(), n, st.data_ptr(), _stream()) == 0
    assert int(st[FOUND_INF]) == 1


# ---------------------------------------------------------------------------------------------- xpt_loss_scale_update
@pytest.mark.parametrize("before, growth, after", [
    ((8.0, 1, 5, 2), 2000, (4.0, 0, 0, 3)),                # skipped: halve, reset the count, one more skip
    ((1.0, 1, 3, 0), 2000, (1.0, 0, 0, 1)),                # floor at 1
    ((1024.0, 0, 0, 4), 3, (1024.0, 0, 1, 4)),             # one good step
    ((1024.0, 0, 2, 4), 3, (2048.0, 0, 0, 4)),             # the growth_steps-th good step doubles S
    ((2.0 ** 127, 0, 0, 0), 1, (2.0 ** 127, 0, 0, 0)),     # 2 S would overflow: S stays, the count restarts
])
def test_loss_scale_update_transitions(lib, before, growth, after):
    st = _state(scale=before[0], found=before[1], good=before[2], skipped=before[3])
    assert lib.xpt_loss_scale_update(st.data_ptr(), growth, _stream()) == 0
    out = st.cpu()
    assert torch.equal(out, _state(scale=after[0], found=after[1], good=after[2], skipped=after[3], dev="cpu")), out.tolist()
    assert out.view(torch.float32)[INV_SCALE] == 1.0 / after[0]


# ---------------------------------------------------------------------------------------------- _dyn optimizer kernels
def _buffers(n, seed, dev="cuda"):
    from xpt_mde_2021_amd.hip import lib as xl
    gen = torch.Generator().manual_seed(seed)
    p, g, m = (torch.randn(n, generator=gen) for _ in range(3))
    v = torch.rand(n, generator=gen)
    g = g * 1024.0
    shadow = p.to(xl.half())
    return [t.to(dev) for t in (p, g, m, v, shadow)]


def _adam(lib, bufs, n, grad_scale, zero_grad, state=None, off=0):
    p, g, m, v, sh = bufs
    step = torch.full((1,), 3.0, device="cuda")
    args = (p.data_ptr() + 4 * off, g.data_ptr() + 4 * off, m.data_ptr() + 4 * off, v.data_ptr() + 4 * off, n - off,
            step.data_ptr(), 1e-3, 0.9, 0.999, 1e-7, grad_scale, zero_grad, sh.data_ptr() + sh.element_size() * off)
    rc = lib.xpt_adam_step(*args, _stream()) if state is None else lib.xpt_adam_step_dyn(*args, state.data_ptr(), _stream())
    assert rc == 0
    torch.cuda.synchronize()


def _sgd(lib, bufs, n, grad_scale, zero_grad, state=None, off=0):
    p, g, _, _, sh = bufs
    args = (p.data_ptr() + 4 * off, g.data_ptr() + 4 * off, n - off, 1e-2, grad_scale, zero_grad,
            sh.data_ptr() + sh.element_size() * off)
    rc = lib.xpt_sgd_step(*args, _stream()) if state is None else lib.xpt_sgd_step_dyn(*args, state.data_ptr(), _stream())
    assert rc == 0
    torch.cuda.synchronize()


def _bits(t):
    return t.view(torch.int16) if t.element_size() == 2 else t.view(torch.int32)


# (n, piece offset): a tail of n % 4 elements, a grid-strided buffer, a piece of the buffers (Adam pieces start at multiples
# of 4 elements: 16-byte vectors; SGD's may start anywhere)
@pytest.mark.parametrize("opt, n, off", [("adam", 4099, 0), ("adam", (1 << 18) + 2, 0), ("adam", 4099, 4),
                                         ("sgd", 4099, 0), ("sgd", (1 << 18) + 2, 0), ("sgd", 4103, 1)])
@pytest.mark.parametrize("scale", [1024.0, 3.0])
@pytest.mark.parametrize("zero_grad", [1, 0])
def test_dyn_optimizer_kernels_match_their_static_twins(lib, opt, n, off, scale, zero_grad):
    """No overflow: p, m, v, shadow, grad bit-equal to the static kernel called with grad_scale x inv_scale (also for an
    inv_scale that is not a power of two); overflow: p, m, v, shadow bit-unchanged, grad zeroed (or kept: zero_grad 0)."""
    step = _adam if opt == "adam" else _sgd
    grad_scale = 0.5
    st = _state(scale=scale)
    inv = float(st.cpu().view(torch.float32)[INV_SCALE])
    product = float(torch.tensor(grad_scale, dtype=torch.float32) * torch.tensor(inv, dtype=torch.float32))
    a, b = _buffers(n, 7), _buffers(n, 7)
    step(lib, a, n, product, zero_grad, off=off)
    step(lib, b, n, grad_scale, zero_grad, state=st, off=off)
    for x, y, name in zip(a, b, ["p", "g", "m", "v", "shadow"]):
        assert torch.equal(_bits(x), _bits(y)), name
    assert not torch.equal(a[0], _buffers(n, 7)[0])
    assert torch.equal(st, _state(scale=scale))              # the optimizer only reads the state
    # overflow: the same launch leaves everything but the gradient bit-unchanged
    fresh = _buffers(n, 7)
    c = _buffers(n, 7)
    st_bad = _state(scale=scale, found=1)
    step(lib, c, n, grad_scale, zero_grad, state=st_bad, off=off)
    for x, y, name in zip(fresh, c, ["p", "g", "m", "v", "shadow"]):
        if name == "g" and zero_grad:
            assert bool((y[off:] == 0).all()) and torch.equal(x[:off], y[:off]), name
        else:
            assert torch.equal(_bits(x), _bits(y)), name
    assert torch.equal(st_bad, _state(scale=scale, found=1))


def _child(args, timeout, **env):
    env = {k: v for k, v in dict(os.environ, **env).items() if v is not None}
    return subprocess.run([sys.executable, *args], cwd=ROOT, capture_output=True, text=True, timeout=timeout, env=env)


def test_kernels_on_the_half_precision_build(gpu_device):
    """The kernel tests above once more in a child process on libxpt_hip_f16.so (the shadow copy is IEEE half there)."""
    if os.environ.get("XPT_HALF") == "fp16":
        pytest.skip("this process already is the half-precision child")
    run = _child(["-m", "pytest", __file__, "-m", "gpu", "-q", "-p", "no:cacheprovider", "-k", "not training and not half"],
                 900, XPT_HALF="fp16")
    tail = (run.stdout + run.stderr)[-3000:]
    assert run.returncode == 0, tail
    assert " passed" in run.stdout and "failed" not in run.stdout.splitlines()[-1], tail


# ---------------------------------------------------------------------------------------------- fp16 training runs
# An initial scale at which this model's half-precision gradients overflow on the first step.  Measured on the MI355X with
# tools/loss_scale_train.py (graph, dynamic, from 2^40, 40 steps): from the seeded initial weights every scale >= 2^19
# overflows (22 skipped steps, halving from 2^40), 2^18 does not and training proceeds there (loss 0.59 -> 0.19).  2^21 leaves
# a factor of 4 of margin above the first overflowing scale; the static default, 2^15, is 8x below it.
REAL_OVERFLOW_SCALE = 2.0 ** 21


@functools.lru_cache(maxsize=None)
def _train(mode, steps, poison=-1, dynamic=True, s0=None, growth=None, extra=()):
    env = {"XPT_HALF": "fp16", "XPT_LOSS_SCALE_DYNAMIC": "1" if dynamic else "0",
           "XPT_LOSS_SCALE_FP16": None if s0 is None else repr(float(s0)),
           "XPT_LOSS_SCALE_GROWTH_STEPS": None if growth is None else str(growth), **dict(extra)}
    args = [os.path.join("tools", "loss_scale_train.py"), mode, str(steps)] + ([str(poison)] if poison >= 0 else [])
    run = _child(args, 900, **env)
    assert run.returncode == 0, (run.stdout + run.stderr)[-3000:]
    out = {}
    for line in run.stdout.splitlines():
        head, _, rest = line.partition(" ")
        if head.isupper():
            out[head] = rest
    out["text"] = run.stdout
    return out


def _floats(s):
    return [float(v) for v in s.split()[1:]] if s.split()[0] in ("eager", "graph", "distributed") else [float(v) for v in s.split()]


def test_training_dynamic_equals_static_without_overflow(gpu_device):
    """Growth interval longer than the run: the dynamic step (device seed, device 1/S, the check and update launches) gives
    the same losses and weights, bit for bit, as the static step in graph mode."""
    dyn = _train("graph", 6, growth=1000)
    sta = _train("graph", 6, dynamic=False)
    assert dyn["LOSSES"] == sta["LOSSES"] and dyn["PARAMSUM"] == sta["PARAMSUM"], (dyn["text"][-1500:], sta["LOSSES"])
    assert _floats(dyn["SCALES"]) == [32768.0] * 6 and dyn["SKIPPED"].split() == ["0"] * 6
    assert "'memset': 0" in dyn["CAPTURED"] and dyn["CAPTURED"].startswith("True"), dyn["CAPTURED"]
    assert dyn["HINT_MISSES"] == "0" and dyn["FINITE"] == "True True True"


def test_training_injected_overflow_captured_equals_eager(gpu_device):
    """An inf multiplied into one gradient element before step 3 (inside the captured step): the step is skipped -- the
    weights after it are those before it --, S halves there and grows again after G = 2 good steps; the captured and the
    eager trainer agree bit for bit, the one-pass march's hint never misses and the capture holds no memset node."""
    k = 3
    graph = _train("graph", 8, poison=k, s0=1024, growth=2)
    eager = _train("eager", 8, poison=k, s0=1024, growth=2)
    assert graph["LOSSES"].split()[1:] == eager["LOSSES"].split()[1:], (graph["LOSSES"], eager["LOSSES"])
    assert graph["SCALES"] == eager["SCALES"] and graph["PARAMSUM"] == eager["PARAMSUM"]
    scales = _floats(graph["SCALES"])                      # S after each step
    assert scales == [1024, 2048, 2048, 1024, 1024, 2048, 2048, 4096], scales
    assert graph["SKIPPED"].split() == ["0", "0", "0", "1", "1", "1", "1", "1"]
    for run in (graph, eager):
        assert run["POISONED_STEP_UNCHANGED"] == "True" and run["HINT_MISSES"] == "0" and run["FINITE"] == "True True True"
        sums = [line.split()[-1] for line in run["text"].splitlines() if line.startswith("STEP")]
        assert sums[k] == sums[k - 1] and sums[k + 1] != sums[k]
    assert "'memset': 0" in graph["CAPTURED"] and graph["CAPTURED"].startswith("True"), graph["CAPTURED"]


def test_training_survives_a_real_overflow(gpu_device):
    """At an initial scale of 2^21 (REAL_OVERFLOW_SCALE: the first overflowing scale of this model is 2^19, measured on the
    MI355X) the static mode's half-precision gradients overflow and its weights are non-finite within 3 steps; the dynamic
    mode skips the overflowing steps (2^21, 2^20, 2^19), backs the scale off to 2^18, keeps every weight finite and learns."""
    sta = _train("eager", 3, dynamic=False, s0=REAL_OVERFLOW_SCALE)
    assert sta["FINITE"] != "True True True", sta["text"][-1500:]
    dyn = _train("graph", 10, s0=REAL_OVERFLOW_SCALE)
    scales, skipped = _floats(dyn["SCALES"]), [int(v) for v in dyn["SKIPPED"].split()]
    losses = _floats(dyn["LOSSES"])
    assert skipped[-1] >= 1 and scales[-1] < REAL_OVERFLOW_SCALE, (scales, skipped)
    assert dyn["FINITE"] == "True True True" and all(v == v for v in losses), dyn["text"][-1500:]
    assert losses[-1] < losses[0], losses


def test_training_distributed_one_rank_equals_graph(gpu_device):
    """The data-parallel trainer's two-graph step (XPT_DP_OVERLAP=1, no other rank), dynamic mode: same as graph mode."""
    dist = _train("distributed", 6, growth=1000, extra=(("XPT_DP_OVERLAP", "1"),))
    graph = _train("graph", 6, growth=1000)
    assert dist["LOSSES"].split()[1:] == graph["LOSSES"].split()[1:] and dist["PARAMSUM"] == graph["PARAMSUM"], \
        (dist["LOSSES"], graph["LOSSES"])
    assert dist["SCALES"] == graph["SCALES"] and dist["FINITE"] == "True True True"


def test_training_early_update_takes_the_one_piece_step(gpu_device):
    """XPT_EARLY_UPDATE=1 cannot skip a whole buffer it updates in pieces: dynamic mode takes the one-piece step, with the
    graph mode's results."""
    early = _train("graph", 6, growth=1000, extra=(("XPT_EARLY_UPDATE", "1"),))
    graph = _train("graph", 6, growth=1000)
    assert early["EARLY_UPDATE"] == "False"
    assert early["LOSSES"] == graph["LOSSES"] and early["PARAMSUM"] == graph["PARAMSUM"]
