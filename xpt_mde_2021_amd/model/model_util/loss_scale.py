"""Dynamic loss scaling of the half-precision configuration (opts.CONV_DTYPE = "fp16", opts.LOSS_SCALE_FP16_DYNAMIC).

The counterpart of tf.keras.mixed_precision.LossScaleOptimizer with its dynamic loss scale (TF 2.4: initial scale,
growth_steps, multiplier 2), kept on the device: the backward pass is seeded with the CURRENT scale S read from device
memory; once the flat gradient is final, xpt_grad_nonfinite raises a flag when it holds an inf / NaN; the optimizer
(xpt_adam_step_dyn / xpt_sgd_step_dyn) skips the update on that flag and otherwise unscales by 1/S; xpt_loss_scale_update
then halves S (skipped step, floor 1) or doubles it after `growth_steps` finite steps in a row, and clears the flag.  No
host round trip per step, so the whole step replays from a hipGraph.

As in TF, a skipped step still counts: the Adam step count t is bumped (LossScaleOptimizer's do-not-apply branch runs
`iterations.assign_add(1)`), and the gradient is zeroed.

The state is ONE 32-byte device block (xpt_loss_scale_state, include/xpt_hip.h) held as an int32 tensor: the replay check
of the captured step (train_val._StepGraph) saves and restores it with the optimizer state and skips integer tensors in
its finiteness / magnitude bound (S may legitimately exceed 1e8).  Host (CPU) tensors run the same state machine with
torch ops (the CPU unit tests and the gloo data-parallel tests).
"""
import math

import torch

from ...hip import lib as _lib
from ...utils.util_class import WrongInputException

# int32 words of xpt_loss_scale_state (include/xpt_hip.h); SCALE and INV_SCALE hold float32 bits
SCALE, INV_SCALE, FOUND_INF, GOOD_STEPS, SKIPPED = 0, 1, 2, 3, 4
STATE_WORDS = 8


def check_initial_scale(scale):
    """The initial scale must be a finite power of two >= 1: scaling and unscaling are then exact."""
    s = float(scale)
    if not (math.isfinite(s) and s >= 1.0 and math.frexp(s)[0] == 0.5):
        raise WrongInputException(f"dynamic loss scaling needs a power of two >= 1 as the initial scale "
                                  f"(config.LOSS_SCALE_FP16 / XPT_LOSS_SCALE_FP16), got {scale!r}")
    return s


class DynamicLossScale:
    def __init__(self, initial_scale, growth_steps=2000, device="cpu"):
        s = check_initial_scale(initial_scale)
        if int(growth_steps) < 1:
            raise WrongInputException(f"LOSS_SCALE_GROWTH_STEPS must be >= 1, got {growth_steps!r}")
        self.initial_scale = s
        self.growth_steps = int(growth_steps)
        host = torch.zeros(STATE_WORDS, dtype=torch.int32)
        host.view(torch.float32)[SCALE] = s
        host.view(torch.float32)[INV_SCALE] = 1.0 / s
        self.state = host.to(device)                          # written by the device from here on, never by the host
        self._floats = self.state.view(torch.float32)
        self._reported_skipped = 0

    @property
    def scale_tensor(self):
        """[1] float32 view of the live scale S."""
        return self._floats[SCALE:SCALE + 1]

    def seed_like(self, total_loss):
        """The seed of the backward pass: the live scale, viewed in the shape of the (one-element) loss."""
        if total_loss.numel() != 1 or total_loss.dtype != torch.float32:
            raise WrongInputException(f"dynamic loss scaling seeds a one-element float32 loss, got "
                                      f"{tuple(total_loss.shape)} {total_loss.dtype}")
        return self.scale_tensor.view(total_loss.shape)

    # ---- the three per-step launches (or their host-tensor counterparts)
    def check(self, grad):
        """found_inf |= any element of the flat gradient is +-inf / NaN."""
        if grad.is_cuda:
            lib = _lib.load()
            _lib.check(lib.xpt_grad_nonfinite(grad.data_ptr(), grad.numel(), self.state.data_ptr(),
                                              torch.cuda.current_stream().cuda_stream), "xpt_grad_nonfinite")
            return
        with torch.no_grad():
            bad = (~torch.isfinite(grad)).any().to(torch.int32)
            self.state[FOUND_INF:FOUND_INF + 1].bitwise_or_(bad)

    def skipped_step(self):
        """Host tensors only: the flag of this step (the device kernels read it themselves)."""
        return bool(self.state[FOUND_INF])

    def inv_scale(self):
        """Host tensors only: 1 / S of this step."""
        return float(self._floats[INV_SCALE])

    def update(self):
        """Halve S on a skipped step (floor 1), double it after growth_steps finite steps; clear the flag."""
        if self.state.is_cuda:
            lib = _lib.load()
            _lib.check(lib.xpt_loss_scale_update(self.state.data_ptr(), self.growth_steps,
                                                 torch.cuda.current_stream().cuda_stream), "xpt_loss_scale_update")
            return
        with torch.no_grad():
            st, fl = self.state, self._floats
            s = fl[SCALE:SCALE + 1]
            if bool(st[FOUND_INF]):
                s.copy_(torch.clamp(s * 0.5, min=1.0))
                st[GOOD_STEPS] = 0
                st[SKIPPED] += 1
            else:
                st[GOOD_STEPS] += 1
                if int(st[GOOD_STEPS]) >= self.growth_steps:
                    grown = s * 2.0
                    if bool(torch.isfinite(grown).all()):
                        s.copy_(grown)
                    st[GOOD_STEPS] = 0
            fl[INV_SCALE:INV_SCALE + 1].copy_(1.0 / s)
            st[FOUND_INF] = 0

    # ---- reporting (one fetch; never per step)
    def read(self):
        host = self.state.detach().cpu()
        fl = host.view(torch.float32)
        return {"scale": float(fl[SCALE]), "inv_scale": float(fl[INV_SCALE]), "found_inf": int(host[FOUND_INF]),
                "good_steps": int(host[GOOD_STEPS]), "skipped": int(host[SKIPPED])}

    def epoch_report(self, steps):
        """(current scale, steps skipped since the last report, every one of `steps` skipped?)."""
        st = self.read()
        skipped = st["skipped"] - self._reported_skipped
        self._reported_skipped = st["skipped"]
        return st["scale"], skipped, steps > 0 and skipped >= steps
