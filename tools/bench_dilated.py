#!/usr/bin/env python3
"""Hot-replay time of the dilated 3 x 3 layers of PWC-Net's context network (flow_net.py context[1..4]) at their workload
shape: forward, data gradient and weight gradient of csrc/xpt_conv_dilated.hip against the library path they replace
(layer_ops.conv2d_library: 16-bit forward and data gradient, fp32 weight gradient with its two up-casts).

Each call is issued R times back to back inside one captured hipGraph and timed between HIP events over a few replays (as
tools/hot_replay.py: hot caches, launch floor included).  The bias / activation epilogue of the library path (a separate
launch there, fused here) is not part of either number.

    python tools/bench_dilated.py [--images 32] [--height 32] [--width 96] [--repeats 20]
"""
import argparse
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from xpt_mde_2021_amd.hip import conv as xc, lib as xl  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--images", type=int, default=32)
ap.add_argument("--height", type=int, default=32)
ap.add_argument("--width", type=int, default=96)
ap.add_argument("--repeats", type=int, default=20)
cli = ap.parse_args()
dev = torch.device("cuda:0")
half = xl.half()
lib = xl.load()
B, H, W, R = cli.images, cli.height, cli.width, cli.repeats


def hot(fn):
    """us per call of fn(), R calls per replay of one captured graph."""
    fn()
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):
            fn()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(R):
            fn()
    g.replay()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(3):
        g.replay()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / (3 * R) * 1e3


print(f"# {B} images of {H}x{W}, {'fp16' if half == torch.float16 else 'bf16'}, {R} calls per replay; us per call")
print(f"# {'layer':<22}{'':>6}{'own':>10}{'library':>10}{'own/lib':>9}")
for cin, cout, d in ((128, 128, 2), (128, 128, 4), (128, 96, 8), (96, 64, 16)):
    x = torch.randn(B, cin, H, W, device=dev).to(half).contiguous(memory_format=torch.channels_last)
    gy = torch.randn(B, cout, H, W, device=dev).to(half).contiguous(memory_format=torch.channels_last)
    w = (torch.randn(cout, cin, 3, 3, device=dev) / (3 * cin ** 0.5)).contiguous(memory_format=torch.channels_last)
    bias = torch.zeros(cout, device=dev)
    e = xc.packer.get(w, need_bwd=True)
    y = torch.empty_like(gy)
    dx = torch.empty_like(x)
    ns = lib.xpt_conv2d_dilated_bwd_weight_splits(B, cin, cout, 3, 3, 1, d, H, W)
    part = torch.empty(ns * cout * 9 * cin, dtype=torch.float32, device=dev)

    def st():
        return torch.cuda.current_stream().cuda_stream

    def own_fwd():
        xl.check(lib.xpt_conv2d_dilated_fwd(x.data_ptr(), e["fwd"].data_ptr(), bias.data_ptr(), y.data_ptr(), B, H, W, cin, cin,
                                            cout, 3, 3, 1, d, cout, 0.1, st()), "fwd")

    def own_dgrad():
        xl.check(lib.xpt_conv2d_dilated_bwd_data(gy.data_ptr(), e["bwd"].data_ptr(), dx.data_ptr(), B, H, W, cout, cout, cin,
                                                 3, 3, 1, d, cin, st()), "dgrad")

    def own_wgrad():
        xl.check(lib.xpt_conv2d_dilated_bwd_weight_partials(gy.data_ptr(), x.data_ptr(), part.data_ptr(), part.numel(), B, H, W,
                                                            cin, cin, cin, cout, cout, 3, 3, 1, d, st()), "wgrad")

    wh = w.to(half)
    cfg = ([1, 1], [d, d], [d, d], False, [0, 0], 1)

    def lib_fwd():
        return F.conv2d(x, wh, None, 1, d, d)

    def lib_dgrad():
        return torch.ops.aten.convolution_backward(gy, x, wh, None, *cfg, [True, False, False])[0]

    def lib_wgrad():
        return torch.ops.aten.convolution_backward(gy.float(), x.float(), w, None, *cfg, [False, True, False])[1]

    for what, own, ref in (("fwd", own_fwd, lib_fwd), ("dgrad", own_dgrad, lib_dgrad), ("wgrad", own_wgrad, lib_wgrad)):
        t_own = hot(own)
        try:
            t_lib = hot(ref)
            note = ""
        except RuntimeError as err:                     # a library solver that cannot be captured: say so, no number
            t_lib, note = float("nan"), f"  (library call not capturable: {str(err).splitlines()[0][:60]})"
        print(f"  {cin:>3} -> {cout:<3} d={d:<2} {'(' + str(ns) + ' splits)' if what == 'wgrad' else '':<12}{what:>6}{t_own:10.1f}{t_lib:10.1f}"
              f"{t_own / t_lib:9.2f}{note}", flush=True)
