#!/usr/bin/env python3
"""K full training steps of the bench configuration on the half-precision build, printing per step the loss, the loss scale
S, the skipped-step count and a parameter checksum (tests/test_loss_scale_gpu.py; modelled on tools/determinism_train.py).

    XPT_HALF=fp16 python tools/loss_scale_train.py [eager|graph|distributed] [K] [poison step]

Static or dynamic loss scaling as the environment says (XPT_LOSS_SCALE_DYNAMIC, XPT_LOSS_SCALE_FP16,
XPT_LOSS_SCALE_GROWTH_STEPS).  With a poison step k, ModelTrainer.reduce_gradients -- which runs inside the captured step,
between the backward pass and the update -- multiplies one element of the flat gradient by a device tensor that is set to
inf before step k and back to 1 after it: an overflow injected as ordinary data, from this driver, not from product code."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from xpt_mde_2021_amd.config import opts  # noqa: E402
from xpt_mde_2021_amd.hip import lib as _xlib  # noqa: E402
from xpt_mde_2021_amd.hip import ops as _ops  # noqa: E402
from xpt_mde_2021_amd.model import model_main as mm, train_val as tv  # noqa: E402

mode = sys.argv[1] if len(sys.argv) > 1 else "graph"
K = int(sys.argv[2]) if len(sys.argv) > 2 else 8
poison_step = int(sys.argv[3]) if len(sys.argv) > 3 else -1
opts.CONV_DTYPE = "fp16"
_xlib.set_half_format("fp16")
opts.PER_REPLICA_BATCH = opts.BATCH_SIZE = 8
opts.TRAIN_MODE = mode

poison = torch.ones(1, dtype=torch.float32, device="cuda")
POISON_INDEX = 4099
if poison_step >= 0:
    _reduce = tv.ModelTrainer.reduce_gradients

    def _poisoned_reduce(self):
        _reduce(self)
        g = self.optimizer.flat.grad
        g[POISON_INDEX:POISON_INDEX + 1].mul_(poison)       # one capturable launch; 1 except at the poisoned step

    tv.ModelTrainer.reduce_gradients = _poisoned_reduce

torch.manual_seed(0)
dataset, cfg, _ = mm.get_dataset("synthetic", "train", True)
model, aug, loss_object, optimizer = mm.create_training_parts(0, cfg, 1e-4, opts.LOSS_RIGID_T1, opts.SCALE_WEIGHT_T1,
                                                              opts.RIGID_NET, ckpt_name="__lossscale__")
trainer, _ = tv.train_val_factory(mode, model, loss_object, 0, False, None, optimizer)
flat = optimizer.flat
losses, scales, skipped, sums, unchanged = [], [], [], [], None
for i in range(K):
    before = flat.data.clone() if i == poison_step else None
    if i == poison_step:
        poison.fill_(float("inf"))
    out = trainer.run_a_batch(dataset.batches[i % len(dataset.batches)])
    torch.cuda.synchronize()
    if i == poison_step:
        poison.fill_(1.0)
        unchanged = torch.equal(before.view(torch.int32), flat.data.view(torch.int32))
    st = trainer.loss_scale_state() or {"scale": opts.LOSS_SCALE_FP16, "skipped": 0}
    losses.append(float(out[1]))
    scales.append(st["scale"])
    skipped.append(st["skipped"])
    sums.append(float(flat.data.double().abs().sum()))
    print(f"STEP {i} loss {losses[-1]:.9f} scale {scales[-1]:g} skipped {skipped[-1]} checksum {sums[-1]:.9f}", flush=True)
graph = getattr(trainer, "_graph", None)
print("CAPTURED", graph is not None and graph.graph is not None, getattr(graph, "census", None))
print("EARLY_UPDATE", getattr(trainer, "_early_start", None) is not None)
print("LOSSES", mode, " ".join(f"{v:.9f}" for v in losses))
print("SCALES", " ".join(f"{v:g}" for v in scales))
print("SKIPPED", " ".join(str(v) for v in skipped))
print("PARAMSUM", f"{sums[-1]:.9f}")
print("FINITE", bool(torch.isfinite(flat.data).all()), bool(torch.isfinite(optimizer.m).all()),
      bool(torch.isfinite(optimizer.v).all()))
print("HINT_MISSES", len(_ops.PHOTO_HINT_MISSES))
if poison_step >= 0:
    print("POISONED_STEP_UNCHANGED", unchanged)
