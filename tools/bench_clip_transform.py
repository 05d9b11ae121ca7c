#!/usr/bin/env python3
"""transforms.ClipPlan.apply (csrc/clip_transform.h) at the C3 clip — 64 decoder frames of 360 x 640 — for the two plans
the training transforms produce: the single resize at the 720 cap (-> 405 x 720) and flip + resize 500 x 888 -> crop
431 x 577 -> resize 416 x 556; against the same plan as torch ops on the same device (ToTensor, flip, F.interpolate,
slice, normalise), in ONE process, alternating, warmed up, device events around each call with a synchronise per
repetition.

    python tools/bench_clip_transform.py [--reps 20] [--warmup 3] [--frames 64]
    python tools/bench_clip_transform.py --cpu [--reps 3]       # what ONE loader worker pays per clip today

Prints per plan and path the median ms with min and max, the bytes the plan has to move (source window read once, every
resize output written once, an intermediate read once) over the median beside the part's streaming rate (about 6.3 TB/s
achievable), whether the kernel is faster by more than the spread (the gap of the medians against the larger min-max
spread), and the host-to-device bytes per clip of the two source formats.  --cpu times the float32 evaluation of the two
plans with torch on ONE CPU thread instead (no GPU needed; a host clock, since nothing is asynchronous there)."""
import argparse
import os
import statistics
import sys
import time

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from stcat_amd import _lib as L  # noqa: E402
from stcat_amd.transforms import ClipPlan  # noqa: E402

STREAM_TBS = 6.3        # achievable HBM streaming rate of the part


def plans(h, w):
    return {"resize 405x720": ClipPlan(h, w, False, [("resize", 405, 720)]),
            "flip, 500x888, crop 431x577, 416x556": ClipPlan(h, w, True, [("resize", 500, 888), ("crop", 37, 111, 431, 577),
                                                                         ("resize", 416, 556)])}


def torch_plan(u8, plan):
    """the worker's float32 tensor ops, on whatever device u8 lives"""
    x = u8.permute(0, 3, 1, 2).float() / 255
    if plan.flip:
        x = x.flip(-1)
    for s in plan.steps:
        if s[0] == "resize":
            x = F.interpolate(x, size=(s[1], s[2]), mode="bilinear", align_corners=False, antialias=plan.antialias)
        else:
            x = x[:, :, s[1]:s[1] + s[3], s[2]:s[2] + s[4]]
    mean = torch.tensor(plan.mean, device=x.device)[:, None, None]
    std = torch.tensor(plan.std, device=x.device)[:, None, None]
    return (x - mean) / std


def bytes_moved(plan, n):
    """what one apply has to move: per launch its source window (1 byte per value from the decoder's frames, 4 from an
    intermediate) and its output window in fp32"""
    total, first = 0, True
    for ln in plan.launches():
        total += n * 3 * (ln["window"][2] * ln["window"][3] * (1 if first else 4) + ln["out_window"][2] * ln["out_window"][3] * 4)
        first = False
    return total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--cpu", action="store_true")
    a = ap.parse_args()
    h, w = 360, 640
    u8 = torch.randint(0, 256, (a.frames, h, w, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(0))
    if a.cpu:
        torch.set_num_threads(1)
        print(f"float32 CPU evaluation, 1 thread, {a.frames} frames of {h} x {w}, {a.reps} repetitions after one warm-up")
        for name, plan in plans(h, w).items():
            torch_plan(u8, plan)
            t = []
            for _ in range(a.reps):
                t0 = time.perf_counter()
                torch_plan(u8, plan)
                t.append((time.perf_counter() - t0) * 1e3)
            print(f"{name}: median {statistics.median(t):.1f} ms  (min {min(t):.1f}, max {max(t):.1f})")
        return
    assert a.reps >= 1 and torch.cuda.is_available(), "needs the GPU"
    L.load()
    dev = torch.device("cuda:0")
    src = u8.to(dev)
    print(f"{a.frames} frames of {h} x {w}, {a.reps} alternating repetitions after {a.warmup} warm-up; "
          f"{torch.cuda.get_device_name(0)}")
    print(f"host-to-device bytes per clip: uint8 source {u8.numel() / 1e6:.1f} MB; the transformed fp32 clip "
          + ", ".join(f"{a.frames * 3 * p.out_size()[0] * p.out_size()[1] * 4 / 1e6:.1f} MB" for p in plans(h, w).values()))
    for name, plan in plans(h, w).items():
        out = torch.empty(a.frames, 3, *plan.out_size(), device=dev)
        paths = {"kernel": lambda: plan.apply(src, out=out), "torch": lambda: torch_plan(src, plan)}
        times = {k: [] for k in paths}
        for rep in range(a.warmup + a.reps):
            for k, fn in paths.items():                              # alternating: kernel, torch, kernel, ...
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                torch.cuda.synchronize()
                if rep >= a.warmup:
                    times[k].append(e0.elapsed_time(e1))
        err = (out - torch_plan(src, plan)).abs().max().item()
        moved = bytes_moved(plan, a.frames)
        print(f"\n{name}: {len(plan.launches())} launch(es), {moved / 1e6:.1f} MB to move "
              f"({moved / STREAM_TBS / 1e9:.3f} ms at {STREAM_TBS} TB/s); max |kernel - torch| = {err:.2e}")
        st = {}
        for k, v in times.items():
            st[k] = (statistics.median(v), min(v), max(v))
            print(f"{k:7s} median {st[k][0]:8.3f} ms  (min {st[k][1]:.3f}, max {st[k][2]:.3f})  "
                  f"{moved / st[k][0] / 1e9:6.2f} TB/s of the plan's bytes")
        gap = st["torch"][0] - st["kernel"][0]
        spread = max(st["kernel"][2] - st["kernel"][1], st["torch"][2] - st["torch"][1])
        print(f"torch - kernel = {gap:.3f} ms ({st['torch'][0] / st['kernel'][0]:.2f}x), larger min-max spread {spread:.3f} ms")
        print(f"faster by more than the spread: {'yes' if gap > spread else 'no'}")


if __name__ == "__main__":
    main()
