#!/usr/bin/env python3
"""bench.py -- train images/sec of the self-supervised depth/pose training step on MI355X.

    python bench.py --gpus N --steps K --warmup W [--config c2|c4|c5] [--dump-outputs DIR] [--full]
    N > 1 works both ways: under an external `python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py
    --gpus N ...` (RANK / WORLD_SIZE set), or stand-alone -- then this process starts that launcher itself (one fresh
    child per GPU, before anything here touches the GPU) and relays rank 0's JSON line.

One "step" = one full training step over one batch of synthetic KITTI-shaped snippets already resident in HBM:
DepthNet(NASNet-Mobile)+PoseNetImproved forward in bf16 (gfx950 MFMA kernels of this repo + rocBLAS GEMMs), view synthesis + multi-scale
L1 + SSIM + smoothness loss in the gfx950 HIP kernels, backward, [RCCL all-reduce of the flat gradient], fused Adam.
One "image" = one 5-frame 128x416 snippet (BASELINE.json).  Workload at N=1 = BASELINE.json configs[1]
(batch 8 per GPU); N>1 keeps 8 snippets per GPU (weak scaling, configs[2]).

Rank 0 prints ONE JSON line.  A plain run sets up, warms up, times the K steps, writes --dump-outputs and prints the
line; everything else it can measure runs only with --full: the "did it train" check over four more steps,
`all_reduce_us`, `sustained`, `epoch_loop`, `host_fed`, `roofline` (the warp+photometric HIP kernel of the largest
scale priced against the HBM peak with HIP events on the launch stream) and `cpu_baseline` (the oracle / CPU port of
the same step timed on the host cores, N=1 only).  Nothing here reads the reference project.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

NETS_LABEL = {"rigid": "DepthNet(NASNetMobile)+PoseNetImproved", "flow": "PWCNet",
              "joint": "DepthNet(NASNetMobile)+PoseNetImproved+PWCNet"}
LOSS_LABEL = {"flow": "flowL2+flow_reg", "joint": "cmbL1+cmbSSIM+smoothness"}
HBM_PEAK_GBS = 8000.0           # MI355X_MICROARCH.md: 8.0 TB/s spec (6.29 TB/s measured float4 copy)
MFMA_PEAK_TFLOPS = 2500.0       # MI355X_MICROARCH.md: ~2.5 PFLOP/s dense bf16


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--batch", type=int, default=8, help="snippets per GPU")
    ap.add_argument("--height", type=int, default=128)
    ap.add_argument("--width", type=int, default=416)
    ap.add_argument("--mode", default=None, help="eager | graph | distributed (default: graph at N=1, distributed at N>1)")
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "fp16", "fp32"])
    ap.add_argument("--stereo", action="store_true", help="stereo feature dict + LOSS_RIGID_T2 (configs[4]-style)")
    ap.add_argument("--nets", default="rigid", choices=["rigid", "flow", "joint"],
                    help="rigid = DepthNet + PoseNet (the headline workload); flow = PWC-Net with flowL2 + flow_reg; joint = "
                         "all three with cmbL1 + cmbSSIM + smoothe (SURVEY 8f-4; PWC-Net needs --width divisible by 64)")
    ap.add_argument("--config", default=None, choices=["c2", "c4", "c5"],
                    help="BASELINE.json configs: c2 = batch 8 128x416 (default), c4 = configs[3]: 256x832 batch 4, "
                         "c5 = configs[4]: stereo + mono losses over the mixed dataset shapes cycled per step")
    ap.add_argument("--no-miopen-find", action="store_true", help="MIOpen immediate-mode heuristics instead of the fast find")
    ap.add_argument("--net-streams", type=int, default=None, help="1: PoseNet on a side stream next to DepthNet (fork/join in the graph)")
    ap.add_argument("--selftest-launch", action="store_true",
                    help="only exercise the launcher path: every rank joins the process group (gloo without a GPU), one "
                         "all-reduce, rank 0 prints the JSON line with the rank count")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-roofline", action="store_true")
    ap.add_argument("--cpu-baseline-seconds", type=float, default=20.0)
    ap.add_argument("--data", default="resident", choices=["resident", "tfrecord"],
                    help="tfrecord (with --full): ALSO write a synthetic shard set with the repo's TFRecord writer and train from it through the "
                         "prefetching reader (`host_fed`: reader alone, and the step fed from the host; never `value`)")
    ap.add_argument("--no-host-fed", action="store_true",
                    help="skip the `host_fed` leg (TFRecord shards written, read back through the prefetching reader, trained on)")
    ap.add_argument("--sustained-seconds", type=float, default=6.0,
                    help="back-to-back steps after the timed region, reported separately (`sustained`); 0 disables")
    ap.add_argument("--full", action="store_true",
                    help="also run the legs beyond the headline figure: the loss-decrease check, all_reduce_us, sustained, "
                         "epoch_loop, host_fed, roofline and cpu_baseline (the --no-* / --sustained-seconds options trim them)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write what the last timed step returned (predictions, total loss, loss by type) as DIR/<name>.npy")
    args = ap.parse_args()
    if args.config == "c4":
        args.height, args.width, args.batch = 256, 832, 4
    elif args.config == "c5":
        args.stereo = True
    return args


# SURVEY.md 8(d) / config-example.py:25-30: image sizes of the mixed pretrain stream (cityscapes, waymo, a2d2, kitti-odom ...)
MIXED_SHAPES = [(128, 512), (192, 512), (256, 384), (192, 384)]


def launch_children(args):
    """`python bench.py --gpus N` without a launcher around it: start `torch.distributed.run` with N fresh workers (this
    process has not touched the GPU), pass rank 0's JSON line through and return the launcher's exit code."""
    import socket
    import subprocess
    with socket.socket() as sock:
        sock.bind(("127.0.0.1", 0))
        port = sock.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}",
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ)
    # the pool's host driver supports dmabuf IPC only: with the legacy IPC mode RCCL's peer buffer exchange fails with
    # `hipIpcGetMemHandle: invalid argument` (the image exports this value; a launcher-less start keeps it for its ranks)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    print(f"[bench] starting {args.gpus} ranks: {' '.join(cmd)}", file=sys.stderr, flush=True)
    proc = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, env=env)
    line = None
    for text in proc.stdout.splitlines():
        if text.startswith("{") and '"metric"' in text:
            line = text
        else:
            print(text, file=sys.stderr)
    if line is not None:
        print(line, flush=True)
    return proc.returncode if line is not None or proc.returncode else 1


def build_step(args, world):
    from xpt_mde_2021_amd.config import opts
    opts.CONV_DTYPE = args.dtype
    if args.dtype in ("bf16", "fp16"):      # the 16-bit format is a property of the library this process loads (hip/lib.py)
        from xpt_mde_2021_amd.hip import lib as _xlib
        _xlib.set_half_format(args.dtype)
    opts.PER_REPLICA_BATCH = args.batch
    opts.BATCH_SIZE = args.batch * world
    opts.IMAGE_SIZES["kitti_raw"] = (args.height, args.width)
    mode = args.mode or ("graph" if world == 1 else "distributed")
    opts.TRAIN_MODE = mode
    from xpt_mde_2021_amd.model import model_main as mm
    from xpt_mde_2021_amd.model import train_val as tv
    if world > 1 or mode == "distributed":
        from xpt_mde_2021_amd.model.model_util.distributer import DistributionStrategy
        DistributionStrategy.get_strategy()                     # per-rank data seeds, global batch = replicas x per-GPU
        opts.BATCH_SIZE = args.batch * world
    if args.net_streams is not None:
        opts.NET_STREAMS = bool(args.net_streams)
    opts.MIOPEN_FIND = not args.no_miopen_find                  # fast find over the ~30 dense convolutions (seconds)
    name = "synthetic_stereo" if args.stereo else "synthetic"
    dataset, tfr_config, _ = mm.get_dataset(name, "train", True)
    loss_weights = opts.LOSS_RIGID_T2 if args.stereo else opts.LOSS_RIGID_T1
    net_names = opts.RIGID_NET
    if args.nets == "flow":
        net_names, loss_weights = opts.FLOW_NET, opts.LOSS_FLOW
    elif args.nets == "joint":
        net_names, loss_weights = opts.JOINT_NET, {"cmbL1": 5.0, "cmbSSIM": 0.5, "smoothe": opts.SMOOTHNESS_FACTOR}
    model, augmenter, loss_object, optimizer = mm.create_training_parts(
        0, tfr_config, 1e-4, loss_weights, opts.SCALE_WEIGHT_T1, net_names, ckpt_name="__bench__")
    trainer, _ = tv.train_val_factory(mode, model, loss_object, 0, opts.STEREO, augmenter, optimizer)
    if args.config == "c5":
        # configs[4]: the mixed pretrain stream -- every step another dataset's image size (one captured graph per size)
        batches = []
        for hw in MIXED_SHAPES:
            opts.IMAGE_SIZES["kitti_raw"] = hw
            batches.append(mm.get_dataset(name, "train", True)[0].batches)
        dataset.batches = [b[i] for i in range(len(batches[0])) for b in batches]
        opts.IMAGE_SIZES["kitti_raw"] = (args.height, args.width)
    return trainer, dataset, mode, loss_object


def roofline_leg(args, dataset, repeats=50):
    """HIP-event timing (on the launch stream) of the dominant hand-written kernel at the step's own shapes:
    the full-resolution warp + photometric pass.  Returns the `roofline` object."""
    from xpt_mde_2021_amd.hip import ops
    from xpt_mde_2021_amd.hip import roofline as rf
    feats = dataset.batches[0]
    return rf.measure(ops, feats, repeats, HBM_PEAK_GBS)


def host_fed_leg(args, trainer, dataset, note):
    """--data tfrecord: the input contract end to end.  Writes `n` KITTI-shaped snippets (uint8 image 5H x W x 3, intrinsic,
    depth_gt, pose_gt: what tfrecords/tfr_util.py serialises) with the repo's own TFRecord writer, then (a) drains the
    prefetching reader alone -> reader_snippets_per_s, (b) trains from it -> value_host_fed.  tfrecord_reader.py:61-108."""
    import shutil
    import tempfile
    from xpt_mde_2021_amd.tfrecords.tfrecord_reader import TfrecordReader, TfrecordWriter
    n = 64 * args.batch
    feats = dataset.batches[0]
    root = tempfile.mkdtemp(prefix="xpt_bench_tfr_", dir=os.environ.get("TMPDIR", "/tmp"))
    try:
        host = {k: v.detach().cpu() for k, v in feats.items() if k in ("image", "intrinsic", "depth_gt", "pose_gt")}
        writer = TfrecordWriter(root, shard_size=128)
        B = host["image"].shape[0]
        for i in range(n):
            b = i % B
            img = ((host["image"][b] + 1.0) * 127.5).round().clamp(0, 255).to(torch.uint8).numpy()
            img = np.roll(img, i // B, axis=1)                       # distinct snippets
            writer.write({"image": img, "intrinsic": host["intrinsic"][b].numpy(), "depth_gt": host["depth_gt"][b].numpy(),
                          "pose_gt": host["pose_gt"][b].numpy()})
        writer.close([feats["image5d"].shape[1], args.height, args.width, 3])
        nbytes = sum(os.path.getsize(os.path.join(root, f)) for f in os.listdir(root))
        note(f"host-fed leg: {n} snippets, {nbytes / 1e6:.0f} MB of TFRecord shards in {root}")
        from xpt_mde_2021_amd.tfrecords.tfrecord_reader import default_workers
        workers = default_workers()
        kw = dict(shuffle=True, batch_size=args.batch, device="cuda", prefetch=3, workers=workers)
        # (a) the reader alone
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        count = 0
        for batch in TfrecordReader(root, epochs=3, **kw).get_dataset():
            count += batch["image5d"].shape[0]
        torch.cuda.synchronize()
        reader_rate = count / (time.perf_counter() - t0)
        # (b) the training step fed by it (same captured graph: the batch is copied into its static inputs)
        ds = TfrecordReader(root, epochs=6, **kw).get_dataset()
        it = iter(ds)
        for _ in range(8):
            trainer.run_a_batch(next(it))
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        steps = 0
        for batch in it:
            trainer.run_a_batch(batch)
            steps += 1
        torch.cuda.synchronize()
        fed = time.perf_counter() - t0
        return {"reader_snippets_per_s": round(reader_rate, 1), "value_host_fed": round(args.batch * steps / fed, 3),
                "unit": "images/sec", "steps": steps, "ms_per_step": round(1000.0 * fed / steps, 4),
                "wait_for_reader_ms_per_step": round(1000.0 * ds.reader_seconds / max(steps + 8, 1), 4),
                "shard_bytes": int(nbytes), "snippets": n, "decode_workers": workers, "prefetch": 3,
                "what": "synthetic KITTI-shaped snippets written with the repo's TFRecord writer, read back (framing, masked "
                        "CRC32C, tf.train.Example walked by xpt_tfrecord_decode, uint8 -> float on the device), shuffled, batched, uploaded from "
                        "pinned memory on a side stream and trained on; `value` itself is measured on HBM-resident inputs"}
    finally:
        shutil.rmtree(root, ignore_errors=True)


def cpu_baseline(args, seconds):
    """The oracle (CPU restatement, "port") of config C1: 4 synthetic 5x128x416 snippets, DepthNet+PoseNet forward,
    synthesis, L1+SSIM+smoothness, backward -- timed on the host cores with torch's intra-op thread pool."""
    from oracle import cpu_step
    return cpu_step.timed_baseline(height=args.height, width=args.width, batch=4, budget_s=seconds)


DUMP_LIMIT_BYTES = 64_000_000


def dump_outputs(out, path):
    """--dump-outputs: what one training step hands its caller, (predictions, total loss, loss by type), as
    <path>/<name>.npy, one file per tensor (`preds.depth_ms.0`, `loss`, `loss_by_type.SSIM`, ...), float64 tensors as
    float64 and all others as float32.  Above DUMP_LIMIT_BYTES in all, the arrays that do not fit an even split of what is
    left of the budget (smallest first) keep a sample of their elements, drawn with a fixed seed and flattened: runs with
    the same arguments keep the same positions, and small arrays (losses, poses) stay whole."""
    leaves = {}

    def walk(name, obj):
        if torch.is_tensor(obj):
            leaves[name] = obj
        elif isinstance(obj, dict):
            for k, v in obj.items():
                walk(f"{name}.{k}", v)
        elif isinstance(obj, (list, tuple)):
            for i, v in enumerate(obj):
                walk(f"{name}.{i}", v)

    for name, obj in zip(("preds", "loss", "loss_by_type"), out):
        walk(name, obj)
    arrays = {k: v.detach().to("cpu", torch.float64 if v.dtype == torch.float64 else torch.float32).numpy()
              for k, v in leaves.items()}
    if sum(a.nbytes for a in arrays.values()) > DUMP_LIMIT_BYTES:
        rng = np.random.default_rng(20211119)
        left = DUMP_LIMIT_BYTES
        order = sorted(arrays, key=lambda k: (arrays[k].nbytes, k))
        for i, k in enumerate(order):
            a = arrays[k]
            cap = left // (len(order) - i)
            if a.nbytes > cap:
                keep = max(1, cap // a.itemsize)
                a = arrays[k] = a.reshape(-1)[np.sort(rng.choice(a.size, keep, replace=False))]
            left -= a.nbytes
    os.makedirs(path, exist_ok=True)
    for k, a in arrays.items():
        np.save(os.path.join(path, k.replace(os.sep, "_") + ".npy"), a)


def main():
    args = parse()
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ and "RANK" not in os.environ:
        sys.exit(launch_children(args))
    # stdout carries exactly ONE line (the JSON); everything the model / loss factories print goes to stderr -- at the file
    # descriptor level too: RCCL writes its version banner ("RCCL version : ...") to the C stdout when a process group starts
    import contextlib
    sys.stdout.flush()
    real_stdout = os.dup(1)
    os.dup2(2, 1)
    try:
        with contextlib.redirect_stdout(sys.stderr):
            result, world = run(args)
    finally:
        sys.stdout.flush()
        os.dup2(real_stdout, 1)
        os.close(real_stdout)
    if result is not None:
        print(json.dumps(result), flush=True)
    if dist.is_available() and dist.is_initialized():
        if world > 1:
            dist.barrier()
        dist.destroy_process_group()


def launcher_selftest(args, world, rank, local_rank):
    """--selftest-launch: the distributed plumbing of this file without the training step (runs on CPU with gloo)."""
    use_gpu = torch.cuda.device_count() >= max(world, 1)
    if world > 1:
        if use_gpu:
            torch.cuda.set_device(local_rank)
        dist.init_process_group(backend="nccl" if use_gpu else "gloo")
    ones = torch.ones(4, device=f"cuda:{local_rank}" if use_gpu else "cpu")
    if world > 1:
        dist.all_reduce(ones)
    assert world == args.gpus, f"--gpus {args.gpus} but WORLD_SIZE={world}"
    assert float(ones[0]) == float(max(world, 1))
    if rank != 0:
        return None
    return {"metric": "launcher selftest (ranks joined, all-reduce of ones)", "value": float(ones[0]), "unit": "ranks",
            "n_gpus": world, "steps": 0, "warmup": 0, "ms_per_step": 0.0, "higher_is_better": True, "scaling": "weak",
            "vs_baseline": None, "dtype": "f32", "data": "synthetic",
            "config": {"workload": "launcher selftest", "ranks": dist.get_world_size() if world > 1 else 1,
                       "backend": ("nccl" if use_gpu else "gloo") if world > 1 else "none"}}


def run(args):
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    # every rank keeps its own MIOpen user database (eight ranks tuning into one file is an untested hazard)
    os.environ.setdefault("MIOPEN_USER_DB_PATH", os.path.join(os.environ.get("TMPDIR", "/tmp"), f"xpt_miopen_db_rank{rank}"))
    os.makedirs(os.environ["MIOPEN_USER_DB_PATH"], exist_ok=True)
    if args.selftest_launch:
        return launcher_selftest(args, world, rank, local_rank), world
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a GPU (the HIP ops have no CPU fallback)")
    # (XPT_DIST_BACKEND=gloo + several ranks on one card: the rehearsal of the data-parallel GPU path on a one-GPU box,
    #  tests/test_dp_gpu_rehearsal.py; the real thing is nccl = RCCL with one card per rank)
    backend = os.environ.get("XPT_DIST_BACKEND", "nccl")
    ndev = torch.cuda.device_count()
    if backend == "nccl" and world > 1 and int(os.environ.get("LOCAL_WORLD_SIZE", world)) > ndev:
        raise SystemExit(f"bench.py: {world} RCCL ranks but {ndev} GPUs on this node (one card per rank; "
                         "XPT_DIST_BACKEND=gloo rehearses several ranks on one card)")
    torch.cuda.set_device(local_rank % ndev if backend == "gloo" else local_rank)
    if args.mode == "distributed" and world == 1:
        # one GPU, "distributed" asked for: a real one-rank process group (nccl = RCCL) whose collectives ARE issued (the
        # identity), with the two-graph step and its overlapped bucket -- so that the line measures the data-parallel
        # step's structure including its communication launches, not a communication-free copy of the graph mode
        os.environ["XPT_DP_FORCE_COLLECTIVES"] = "1"
        os.environ.setdefault("XPT_DP_OVERLAP", "1")
        if "RANK" not in os.environ:
            import socket
            with socket.socket() as sock:
                sock.bind(("127.0.0.1", 0))
                port = sock.getsockname()[1]
            os.environ.update(RANK="0", WORLD_SIZE="1", LOCAL_RANK="0", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    if world > 1 or (args.mode == "distributed" and "RANK" in os.environ):
        dist.init_process_group(backend=backend)
    assert world == args.gpus, f"--gpus {args.gpus} but WORLD_SIZE={world} (launch with torch.distributed.run)"

    # seeded weights and augmentation draws (per rank): "final_loss" is then the same number in every run of one build
    import random
    random.seed(20211119)
    torch.manual_seed(20211119)
    trainer, dataset, mode, _ = build_step(args, world)
    random.seed(20211119 + rank)
    torch.manual_seed(20211119 + rank)
    batches = dataset.batches

    def sync():
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()

    def note(msg):
        if rank == 0:
            print(f"[bench] {msg}", file=sys.stderr, flush=True)

    note(f"mode={mode} world={world} batch/GPU={args.batch} {args.height}x{args.width} dtype={args.dtype}")
    if args.config == "c5":
        args.warmup = max(args.warmup, len(MIXED_SHAPES))          # every image size is captured before the timed region
    first_loss = None
    for i in range(args.warmup):
        out = trainer.run_a_batch(batches[i % len(batches)])
        if i == 0:
            torch.cuda.synchronize()
            first_loss = float(out[1])
            note("first step done (graph captured)")
    sync()
    note("warm-up done")
    # the timed region: EXACTLY args.steps steps between two barrier + synchronize pairs (wall clock -> `value`); a HIP event
    # after every step on the launch stream gives the per-step spread (`step_ms`: median, p10, p90)
    marks = [torch.cuda.Event(enable_timing=True) for _ in range(args.steps + 1)]
    t0 = time.perf_counter()
    marks[0].record()
    for i in range(args.steps):
        out = trainer.run_a_batch(batches[i % len(batches)])
        marks[i + 1].record()
    host_elapsed = time.perf_counter() - t0          # the host is done enqueueing here; the device may still be running
    sync()
    elapsed = time.perf_counter() - t0
    loss = float(out[1])
    if first_loss is None:
        first_loss = loss
    if not (loss == loss and abs(loss) < 1e30):
        raise SystemExit(f"bench.py: the training loss is not finite ({loss}): the timed steps did not train")
    if args.dump_outputs and rank == 0:
        # before any later step: a captured step returns its graph's static outputs, which the next replay overwrites
        dump_outputs(out, args.dump_outputs)
    settled = None
    if args.full:
        # "did it train": the loss of ONE step is noisy under augmentation (a colour-jittered or cropped batch costs 0.85
        # where its neighbours cost 0.2, in eager execution as in the captured step: tools/determinism_train.py ... aug), so
        # the check compares the first step with the MEDIAN of the last timed step and four more steps after the timed region
        tail = [loss]
        for i in range(4):
            tail.append(float(trainer.run_a_batch(batches[(args.steps + i) % len(batches)])[1]))
        torch.cuda.synchronize()
        settled = sorted(tail)[len(tail) // 2]
    per_step = sorted(marks[i].elapsed_time(marks[i + 1]) for i in range(args.steps))
    pick = lambda q: per_step[min(len(per_step) - 1, int(q * len(per_step)))]          # noqa: E731
    step_ms = {"median": round(pick(0.5), 4), "p10": round(pick(0.1), 4), "p90": round(pick(0.9), 4),
               "how": "HIP events after every step on the launch stream (device time between step ends)"}
    rank_ms = None
    if world > 1:
        t = torch.tensor([elapsed], device="cuda")
        gathered = [torch.zeros_like(t) for _ in range(world)]
        dist.all_gather(gathered, t)
        rank_ms = [round(1000.0 * float(g.item()) / args.steps, 4) for g in gathered]
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())

    result = None
    step_graph = getattr(trainer, "_graph", None)
    if step_graph is not None and getattr(step_graph, "library_path", False) and getattr(step_graph, "eager_fallback", False):
        mode += " (library convolutions on the path and memset nodes in its capture: executed eagerly, DESIGN.md section 6)"
    elif step_graph is not None and getattr(step_graph, "library_path", False):
        mode += " (library convolutions on the path; captured: the graph audit found no memset node)"
    elif step_graph is not None and getattr(step_graph, "eager_fallback", False):
        mode += " (eager fallback: no captured step passed the replay check)"
    if getattr(trainer, "trains_flow_net", False):
        mode += " (PWC-Net is trained eagerly: see DESIGN.md section 6)"
    if rank == 0:
        global_batch = args.batch * world
        result = {
            "metric": "train images/sec (5-frame mixed-size snippets: " + ", ".join(f"{h}x{w}" for h, w in MIXED_SHAPES) + ")"
            if args.config == "c5" else "train images/sec (5-frame 128x416 snippets)" if (args.height, args.width) == (128, 416)
            else f"train images/sec (5-frame {args.height}x{args.width} snippets)",
            "value": round(global_batch * args.steps / elapsed, 3),
            "unit": "images/sec",
            "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": round(1000.0 * elapsed / args.steps, 4),
            "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
            "dtype": args.dtype, "data": "synthetic",
            "config": {"workload": f"{NETS_LABEL[args.nets]} train step, KITTI-raw-shaped "
                                   f"5x{args.height}x{args.width} snippets, batch {args.batch}/GPU, "
                                   f"{LOSS_LABEL[args.nets] if args.nets != 'rigid' else ('stereo LOSS_RIGID_T2' if args.stereo else 'mono L1+SSIM+smoothness')}, 4 scales",
                       "global_batch": global_batch, "per_gpu_batch": args.batch, "mode": mode,
                       "parallelism": f"dp{world}", "ranks": (dist.get_world_size() if world > 1 else 1),
                       "graph_nodes": getattr(step_graph, "census", None),
                       "first_loss": round(first_loss, 6), "final_loss": round(loss, 6)},
            "step_ms": step_ms,
            "host_enqueue_ms_per_step": round(1000.0 * host_elapsed / args.steps, 4),
        }
        if settled is not None:
            result["config"].update(settled_loss=round(settled, 6), loss_decreased=bool(settled < first_loss))
            if args.nets == "rigid" and not (settled < first_loss) and args.warmup + args.steps >= 10:
                raise SystemExit(f"bench.py: the loss did not decrease over {args.warmup + args.steps} steps on the same "
                                 f"batches ({first_loss} -> median of the last five steps {settled}): the timed steps did "
                                 "not train")
        early = getattr(trainer, "_early_start", None)
        if world > 1:
            result["config"]["rank_ms_per_step"] = rank_ms
            result["config"]["backend"] = os.environ.get("XPT_DIST_BACKEND", "nccl")
            try:
                result["config"]["rccl_version"] = ".".join(str(v) for v in torch.cuda.nccl.version())
            except Exception:          # noqa: BLE001  (gloo rehearsal / build without the binding)
                result["config"]["rccl_version"] = None
        if world > 1 or mode.startswith("distributed"):
            flat = trainer.optimizer.flat
            # gradient exchange: the decoder / PoseNet bucket is all-reduced while the encoder's backward runs
            result["config"]["grad_exchange"] = {
                "buckets": 2 if early is not None else 1, "bytes": int(flat.numel) * 4,
                "overlapped_bytes": (int(flat.numel) - int(early)) * 4 if early is not None else 0,
                "how": "two-graph step, backward cut between decoder and encoder" if early is not None else "after the step",
                "collectives_issued": bool(world > 1 or os.environ.get("XPT_DP_FORCE_COLLECTIVES") == "1")}
        if (args.full and dist.is_available() and dist.is_initialized() and rank == 0
                and "grad_exchange" in (result or {}).get("config", {})):
            result["config"]["grad_exchange"]["measure_all_reduce"] = True
    if args.full and dist.is_available() and dist.is_initialized():
        # the all-reduce of the two buckets by itself (every rank takes part): HIP events around 10 back-to-back collectives
        flat = trainer.optimizer.flat
        early = getattr(trainer, "_early_start", None)
        cut = int(early) if early is not None else 0
        scratch = torch.zeros_like(flat.grad)

        def timed_all_reduce(lo, hi):
            if hi <= lo:
                return None
            for _ in range(2):
                dist.all_reduce(scratch[lo:hi])
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(10):
                dist.all_reduce(scratch[lo:hi])
            e1.record()
            torch.cuda.synchronize()
            return round(e0.elapsed_time(e1) * 100.0, 2)          # us per collective

        late_us, early_us = timed_all_reduce(0, cut), timed_all_reduce(cut, int(flat.numel))
        if rank == 0 and "grad_exchange" in result["config"]:
            result["config"]["grad_exchange"].pop("measure_all_reduce", None)
            result["config"]["grad_exchange"]["all_reduce_us"] = {
                "overlapped_bucket": early_us, "trailing_bucket": late_us, "ranks": world,
                "how": "10 back-to-back dist.all_reduce(SUM) of the bucket's fp32 range on this process group, HIP events "
                       "(one rank: RCCL's identity collective -- its launch and copy cost, no link traffic)"}
    note(f"timed region done: {elapsed:.3f} s")
    if not args.full:
        return (result if rank == 0 else None), world
    if args.sustained_seconds > 0 and world == 1 and args.config != "c5":
        # a longer stretch of the same steps (outside `value`): long enough for an outside observer's GPU-busy sampling
        torch.cuda.synchronize()
        n_sus, t1 = 0, time.perf_counter()
        while time.perf_counter() - t1 < args.sustained_seconds:
            for i in range(50):
                trainer.run_a_batch(batches[(n_sus + i) % len(batches)])
            n_sus += 50
            torch.cuda.synchronize()
        sus = time.perf_counter() - t1
        if rank == 0:
            result["sustained"] = {"seconds": round(sus, 3), "steps": n_sus, "ms_per_step": round(1000.0 * sus / n_sus, 4),
                                   "value": round(args.batch * n_sus / sus, 3), "unit": "images/sec",
                                   "what": "back-to-back training steps after the timed region (not part of `value`)"}
        note(f"sustained leg done: {n_sus} steps in {sus:.2f} s")
    if rank == 0 and world == 1 and args.config != "c5" and not args.no_roofline:
        # the real loop (train_val.py:43-64 run_an_epoch): the same steps PLUS merge_results per step (abs-rel with two
        # sorts per sample, centre depths, pose errors, eager, outside the captured graph) and the per-epoch fetch
        import contextlib
        import io
        dataset.steps = args.steps
        trainer.steps_per_epoch = args.steps
        with contextlib.redirect_stdout(io.StringIO()):
            trainer.run_an_epoch(dataset)              # untimed: captures the per-step metrics graph
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        with contextlib.redirect_stdout(io.StringIO()):
            trainer.run_an_epoch(dataset)
        torch.cuda.synchronize()
        loop = time.perf_counter() - t1
        result["epoch_loop"] = {"value": round(global_batch * args.steps / loop, 3), "unit": "images/sec",
                                "ms_per_step": round(1000.0 * loop / args.steps, 4),
                                "what": "run_an_epoch over the same batches: training step + per-step metrics (merge_results)"}
        note(f"epoch loop done: {loop:.3f} s")
    if (rank == 0 and world == 1 and (args.data == "tfrecord" or not args.no_host_fed) and args.config != "c5"
            and args.nets == "rigid" and not args.stereo and mode.startswith("graph")):
        result["host_fed"] = host_fed_leg(args, trainer, dataset, note)
        result["host_fed"]["vs_resident"] = round(result["host_fed"]["value_host_fed"] / result["value"], 4)
        note("host-fed leg done")
    if rank == 0 and not args.no_roofline:
        result["roofline"] = roofline_leg(args, dataset)
        note("roofline leg done")
        if args.nets == "rigid" and args.config != "c5":
            from xpt_mde_2021_amd.hip import roofline as rf
            result["roofline"]["mfma"] = rf.mfma_utilisation(args.height, args.width, args.batch, elapsed / args.steps,
                                                             MFMA_PEAK_TFLOPS, args.stereo)
            note("conv MAC count done")
    if rank == 0 and world == 1 and not args.no_cpu_baseline:
        result["cpu_baseline"] = cpu_baseline(args, args.cpu_baseline_seconds)
    return (result if rank == 0 else None), world


if __name__ == "__main__":
    main()
