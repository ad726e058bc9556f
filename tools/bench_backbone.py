#!/usr/bin/env python3
"""ms/step and graph node count of the training step with another DepthNetPretrained backbone, at bench.py's default workload
(one GPU, batch 8, snippets 5 x 128 x 416, bf16, graph mode, synthetic data -- the trainer
is built the way bench.py builds it).  bench.py measures the flagship (NASNet-Mobile) and is not edited for this.

    python tools/bench_backbone.py [MobileNetV2|EfficientNetB0|ResNet50V2|NASNetMobile|DepthNetBasic] [--steps 200] [--warmup 20]

(any name depth_net_factory builds; DepthNetNoResize needs --height / --width that are multiples of 128)

Prints one JSON line; with XPT_BENCH_DW=1 also the device time of every depthwise-stage launch (replayed back to back from a
captured graph, as tools/hot_replay.py does) against its algorithmic bytes at 8 TB/s; with XPT_BENCH_JUNCTION=1 (ResNet50V2) the
residual junction's forward and backward launch at the four stack widths beside the composed torch-op twin, same method."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from xpt_mde_2021_amd.config import opts  # noqa: E402


def depthwise_stage_floor(dev, batch, height, width, repeats=20, rounds=10):
    """Every depthwise stage of MobileNetV2 at this input size: device time of its forward and backward launch and the share of
    8 TB/s their algorithmic bytes (x + y forward; x + y + dy + dx backward) reach.  Each launch is issued `repeats` times back
    to back inside one captured hipGraph through the C ABI and the graph replayed `rounds` times between two HIP events (the
    method of tools/hot_replay.py): time per launch with hot caches, launch floor included, no host in the way."""
    import ctypes
    from xpt_mde_2021_amd.hip import lib as xl
    from xpt_mde_2021_amd.model.build_model import mobilenet_v2 as mv2
    lib = xl.load()
    P = lambda t: ctypes.c_void_p(t.data_ptr())                      # noqa: E731
    rows, (h, w), cin = [], (height // 2, width // 2), 16
    stages = [(32, 1, h, w)]
    for cout, stride in mv2.BLOCKS:
        stages.append((cin * 6, stride, h, w))
        h, w, cin = -(-h // stride), -(-w // stride), cout
    tot = {"fwd_us": 0.0, "bwd_us": 0.0, "fwd_bytes": 0, "bwd_bytes": 0}

    def graph_time(launch):
        launch(torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            s = torch.cuda.current_stream().cuda_stream
            for _ in range(repeats):
                launch(s)
        g.replay()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(rounds):
            g.replay()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1000.0 / (rounds * repeats)

    for C, stride, h, w in stages:
        oh, ow = -(-h // stride), -(-w // stride)
        pt, pl = (1, 1) if stride == 1 else (((oh - 1) * 2 + 3 - h) // 2, ((ow - 1) * 2 + 3 - w) // 2)
        x = (2.5 + 3 * torch.randn(batch, h, w, C, device=dev)).to(xl.half())
        y, dy, dx = (torch.empty(batch, oh, ow, C, device=dev, dtype=xl.half()), torch.randn(batch, oh, ow, C, device=dev).to(xl.half()),
                     torch.empty_like(x))
        wt, gamma, beta, mean = (torch.randn(C, 9, device=dev) / 3, torch.ones(C, device=dev), torch.full((C,), 3.0, device=dev),
                                 torch.zeros(C, device=dev))
        var = torch.ones(C, device=dev)
        chunks = lib.xpt_dwconv_bn_relu6_bwd_chunks(batch, oh, ow, C)
        part = torch.empty(chunks * 11 * C, device=dev)

        def fwd(s):
            xl.check(lib.xpt_dwconv_bn_relu6_fwd(P(x), P(wt), P(gamma), P(beta), P(mean), P(var), 1e-3, P(y), batch, h, w, C, stride,
                                                 pt, pl, oh, ow, 1, s), "fwd")

        def bwd(s):
            xl.check(lib.xpt_dwconv_bn_relu6_bwd(P(x), P(y), P(dy), C, P(wt), P(gamma), P(mean), P(var), 1e-3, P(dx), P(part),
                                                 part.numel(), batch, h, w, C, stride, pt, pl, oh, ow, 1, s), "bwd")

        tf, tb = graph_time(fwd), graph_time(bwd)
        fb, bb = 2 * (x.numel() + y.numel()), 2 * (2 * x.numel() + 2 * y.numel())
        rows.append({"C": C, "stride": stride, "hw": [h, w], "fwd_outputs_per_lane": lib.xpt_dwconv_bn_relu6_fwd_outputs(batch, oh, ow, C),
                     "bwd_chunks": chunks, "fwd_us": round(tf, 2), "bwd_us": round(tb, 2),
                     "fwd_of_hbm": round(fb / (tf * 1e-6) / 8e12, 4), "bwd_of_hbm": round(bb / (tb * 1e-6) / 8e12, 4)})
        tot["fwd_us"] += tf
        tot["bwd_us"] += tb
        tot["fwd_bytes"] += fb
        tot["bwd_bytes"] += bb
    tot["fwd_of_hbm"] = round(tot["fwd_bytes"] / (tot["fwd_us"] * 1e-6) / 8e12, 4)
    tot["bwd_of_hbm"] = round(tot["bwd_bytes"] / (tot["bwd_us"] * 1e-6) / 8e12, 4)
    tot["how"] = f"{repeats} launches back to back in a captured graph, {rounds} replays between HIP events; hot caches"
    return {"stages": rows, "total": {k: (round(v, 2) if isinstance(v, float) else v) for k, v in tot.items()}}


def junction_hot_replay(dev, batch, height, width, repeats=20, rounds=10):
    """The residual junction (csrc/xpt_resnet.hip) at the four stack widths of ResNet50V2 for this input size, plain shortcut:
    device time per call of the fused forward launch, of the composed forward (hip.ops.res_join_torch: library GEMM plus
    element-wise launches, same 16-bit dtype) and of the junction's streaming backward launch.  Each is issued `repeats` times
    back to back inside one captured hipGraph, the graph replayed `rounds` times between two HIP events (tools/hot_replay.py's
    method: hot caches, launch floor included, no host in the way)."""
    import ctypes
    from xpt_mde_2021_amd.hip import lib as xl, ops
    from xpt_mde_2021_amd.model.build_model import resnet_v2 as rn2
    lib = xl.load()
    P = lambda t: ctypes.c_void_p(t.data_ptr())                      # noqa: E731

    def graph_time(launch):
        launch()
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            for _ in range(repeats):
                launch()
        g.replay()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(rounds):
            g.replay()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1000.0 / (rounds * repeats)

    rows, scale = [], 4
    for K, _, stride1 in rn2.STACKS:
        N, h, w = 4 * K, height // scale, width // scale
        M = batch * h * w
        x = torch.randn(batch, K, h, w, device=dev).relu().to(xl.half()).contiguous(memory_format=torch.channels_last)
        sc = torch.randn(batch, N, h, w, device=dev).to(xl.half()).contiguous(memory_format=torch.channels_last)
        w3 = (torch.randn(N, K, 1, 1, device=dev) / K ** 0.5)
        w3h = w3.to(xl.half()).reshape(N, K).contiguous()
        b3 = 0.1 * torch.randn(N, device=dev)
        bn = rn2.ResBatchNorm(N).to(dev)
        out, pre, g = (torch.empty_like(sc) for _ in range(3))
        gy = torch.randn_like(sc)
        nblk = lib.xpt_res_join_bwd_blocks(M, N)
        part = torch.empty(nblk * 3 * N, device=dev)
        vec = (P(bn.weight), P(bn.bias), P(bn.running_mean), P(bn.running_var))

        def fused():
            xl.check(lib.xpt_res_join_fwd(P(x), K, P(w3h), P(b3), None, 0, None, None, 0, P(sc), *vec, rn2.RES_BN_EPS, P(out), P(pre),
                                          M, K, N, 1, h, w, h, w, torch.cuda.current_stream().cuda_stream), "fwd")

        def composed():
            with torch.no_grad():
                ops.res_join_torch(x, w3h.view(N, K, 1, 1), b3, bn, rn2.RES_BN_EPS, shortcut=sc)

        def bwd():
            xl.check(lib.xpt_res_join_bwd(P(gy), P(gy), P(out), *vec, rn2.RES_BN_EPS, P(g), None, P(part), part.numel(), M, N, 1,
                                          h, w, h, w, torch.cuda.current_stream().cuda_stream), "bwd")

        rows.append({"K": K, "N": N, "rows": M, "fused_fwd_us": round(graph_time(fused), 2),
                     "composed_fwd_us": round(graph_time(composed), 2), "bwd_us": round(graph_time(bwd), 2), "bwd_blocks": nblk})
        scale *= stride1
    return {"widths": rows, "how": f"{repeats} calls back to back in a captured graph, {rounds} replays between HIP events; hot caches"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("backbone", nargs="?", default="MobileNetV2")
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--height", type=int, default=128)
    ap.add_argument("--width", type=int, default=416)
    args = ap.parse_args()
    from xpt_mde_2021_amd.model import model_main as mm, train_val as tv
    opts.PER_REPLICA_BATCH = opts.BATCH_SIZE = args.batch
    opts.IMAGE_SIZES["kitti_raw"] = (args.height, args.width)
    opts.TRAIN_MODE = "graph"
    torch.manual_seed(0)
    dataset, cfg, _ = mm.get_dataset("synthetic", "train", True)
    nets = dict(opts.RIGID_NET, depth=args.backbone)
    model, aug, loss_object, optimizer = mm.create_training_parts(0, cfg, 1e-4, opts.LOSS_RIGID_T1, opts.SCALE_WEIGHT_T1, nets,
                                                                  ckpt_name="__bench_backbone__")
    trainer, _ = tv.train_val_factory("graph", model, loss_object, 0, opts.STEREO, aug, optimizer)
    batches = dataset.batches
    first = None
    for i in range(args.warmup):
        out = trainer.run_a_batch(batches[i % len(batches)])
        first = float(out[1]) if first is None else first
    torch.cuda.synchronize()
    marks = [torch.cuda.Event(enable_timing=True) for _ in range(args.steps + 1)]
    t0 = time.perf_counter()
    marks[0].record()
    for i in range(args.steps):
        out = trainer.run_a_batch(batches[i % len(batches)])
        marks[i + 1].record()
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    per = sorted(marks[i].elapsed_time(marks[i + 1]) for i in range(args.steps))
    graph = getattr(trainer, "_graph", None)
    result = {"backbone": args.backbone, "batch": args.batch, "image": [args.height, args.width], "mode": "graph",
              "ms_per_step": round(1000.0 * wall / args.steps, 4), "images_per_s": round(args.batch * args.steps / wall, 1),
              "step_ms_median": round(per[len(per) // 2], 4), "graph_nodes": getattr(graph, "census", None),
              "captured": graph is not None and graph.graph is not None, "first_loss": first, "final_loss": float(out[1])}
    if os.environ.get("XPT_BENCH_DW") == "1" and args.backbone == "MobileNetV2":
        result["depthwise_stage"] = depthwise_stage_floor(torch.device("cuda:0"), args.batch, args.height, args.width)
    if os.environ.get("XPT_BENCH_JUNCTION") == "1" and args.backbone == "ResNet50V2":
        result["junction"] = junction_hot_replay(torch.device("cuda:0"), args.batch, args.height, args.width)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
