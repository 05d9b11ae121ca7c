#!/usr/bin/env python3
"""stcat_rank_sum (csrc/rank_sum.h) at the full model's 8-rank shape — one shard of the 824 MB gradient message, eight
ranks' copies of it — against the same chain computed with torch kernels (7 adds + 1 multiply, each a pass over HBM): in
ONE process, alternating, warmed up, device events around each call with a synchronise per repetition.

    python tools/bench_rank_sum.py [--reps 20] [--warmup 3] [--ranks 8] [--message-mb 824]

Prints per path the median ms, the min-max spread over the repetitions and the achieved GB/s against the bytes the sum has
to move (n_ranks * n * 4 read once, n * 4 written), and whether the two results are bitwise equal (same chain, same
order).  Verdict: the kernel counts as faster only when the gap of the medians exceeds the larger of the two spreads."""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from stcat_amd import _lib as L  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--ranks", type=int, default=8)
    ap.add_argument("--message-mb", type=float, default=824.0)
    a = ap.parse_args()
    assert a.reps >= 1 and a.ranks >= 2 and torch.cuda.is_available(), "needs the GPU"
    L.load()
    dev = torch.device("cuda:0")
    n = int(a.message_mb * 1e6 / 4 / a.ranks) // 64 * 64          # one shard of the padded message, in floats
    g = torch.Generator(device=dev).manual_seed(0)
    recv = torch.randn(a.ranks, n, device=dev, generator=g) * 10.0 ** torch.randint(-3, 4, (a.ranks, n), device=dev, generator=g).float()
    out = {"kernel": torch.empty(n, device=dev), "torch": torch.empty(n, device=dev)}
    scale = 1.0 / a.ranks

    def kernel():
        L.call("stcat_rank_sum", out["kernel"].data_ptr(), recv.data_ptr(), a.ranks, n, n, scale, L.stream_of(recv))

    def eager():
        o = out["torch"]
        torch.add(recv[0], recv[1], out=o)
        for k in range(2, a.ranks):
            o.add_(recv[k])
        o.mul_(scale)

    paths = {"kernel": kernel, "torch": eager}
    times = {name: [] for name in paths}
    for rep in range(a.warmup + a.reps):
        for name, fn in paths.items():                               # alternating: kernel, torch, kernel, ...
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            if rep >= a.warmup:
                times[name].append(e0.elapsed_time(e1))
    moved = (a.ranks + 1) * n * 4
    print(f"rank sum: {a.ranks} ranks x {n} floats ({n * 4 / 1e6:.1f} MB per shard, {moved / 1e6:.1f} MB to move), {a.reps} "
          f"alternating repetitions after {a.warmup} warm-up; {torch.cuda.get_device_name(0)}")
    stats = {}
    for name, v in times.items():
        med, lo, hi = statistics.median(v), min(v), max(v)
        stats[name] = (med, lo, hi)
        print(f"{name:7s} median {med:8.3f} ms  (min {lo:.3f}, max {hi:.3f}, spread {hi - lo:.3f})  {moved / med / 1e6:8.1f} GB/s")
    print(f"bitwise equal results: {'yes' if torch.equal(out['kernel'], out['torch']) else 'NO'}")
    k, t = stats["kernel"], stats["torch"]
    gap, spread = t[0] - k[0], max(k[2] - k[1], t[2] - t[1])
    print(f"torch - kernel = {gap:.3f} ms ({t[0] / k[0]:.2f}x), larger min-max spread {spread:.3f} ms")
    print(f"faster by more than the spread: {'yes' if gap > spread else 'no'}")


if __name__ == "__main__":
    main()
