#!/usr/bin/env python3
"""The reference-sized 2D-map head (models/map2d_head.py: N = 128, 256 channels, four 9 x 9 convolutions) on the fp32-tensor
path and on the bf16 plane path (TempPredictionHead(planes=True)): forward and forward + backward, in ONE process,
alternating, warmed up, device events around each phase with a synchronise per repetition.

    python tools/bench_map2d.py [--reps 20] [--warmup 3] [--nl 6] [--T 64] [--mode bf16x6p]

Prints per path the mean ms per phase, the min-max spread over the repetitions and the algorithmic TFLOP/s from shapes
(2 M N K per conv launch: forward, data gradient, weight gradient of every layer).  The plane path's time includes its
split, per-pixel scale, join and weight-plane launches.  Verdict: the plane path counts as faster only when the gap of
the mean forward + backward times exceeds the larger of the two paths' min-max spreads."""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from stcat_amd import _lib as L, synth  # noqa: E402
from stcat_amd.map2d import TempPredictionHead  # noqa: E402


def conv_flops(head, maps):
    """(forward, forward + backward) algorithmic flops of the conv stack for `maps` maps"""
    N, k, n, D = head.map_maker.map_size, head.k, head.n, head.predictor.weight.shape[1]
    H, fwd, bwd = N + 2 * head.pad0, 0.0, 0.0
    for i in range(n):
        OH = H - (k - 1)
        IN = N if i == 0 else H                                       # layer 0 reads the N x N map (its padding is implicit)
        fwd += 2.0 * maps * OH * OH * D * (k * k * D)                 # M = output pixels, N = Cout, K = taps * Cin
        bwd += 2.0 * maps * IN * IN * D * (k * k * D)                 # data gradient: M = the pixels of dx it writes
        bwd += 2.0 * D * (k * k * D) * maps * OH * OH                 # weight gradient: reduction over the output pixels
        H = OH
    return fwd, fwd + bwd


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--nl", type=int, default=6)
    ap.add_argument("--b", type=int, default=1)
    ap.add_argument("--T", type=int, default=64)
    ap.add_argument("--mode", default="bf16x6p")
    a = ap.parse_args()
    assert a.reps >= 1 and torch.cuda.is_available(), "needs the GPU"
    L.load()
    L.set_mma_mode(a.mode)
    dev = torch.device("cuda:0")
    heads = {}
    for name, planes in (("tensor", False), ("planes", True)):
        h = TempPredictionHead(planes=planes)
        with torch.no_grad():
            for k, v in h.state_dict().items():
                v.copy_(torch.from_numpy(synth.synth_value("map2d_full_head." + k, tuple(v.shape)).copy()))
        heads[name] = h.to(dev).train()
    D = 256
    x = torch.from_numpy(synth.hash_normal("bench/map2d/x", a.nl * a.b * a.T * D).reshape(a.nl, a.b, a.T, D)).to(dev)
    x.requires_grad_(True)
    G = torch.from_numpy(synth.hash_normal("bench/map2d/G", a.nl * a.b * 128 * 128).reshape(a.nl, a.b, 128, 128)).to(dev)
    f_fwd, f_all = conv_flops(heads["tensor"], a.nl * a.b)

    def step(head):
        e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        x.grad = None
        for p in head.parameters():
            p.grad = None
        e[0].record()
        sc = head(x)
        e[1].record()
        sc.backward(G)
        e[2].record()
        torch.cuda.synchronize()
        return e[0].elapsed_time(e[1]), e[0].elapsed_time(e[2])

    times = {name: [] for name in heads}
    for rep in range(a.warmup + a.reps):
        for name, head in heads.items():                                # alternating: tensor, planes, tensor, ...
            t = step(head)
            if rep >= a.warmup:
                times[name].append(t)
    print(f"map2d head: N=128, 256 channels, four 9x9 convs, nl={a.nl} b={a.b} T={a.T}, mode {a.mode}, {a.reps} alternating "
          f"repetitions after {a.warmup} warm-up; {torch.cuda.get_device_name(0)}")
    print(f"algorithmic work: forward {f_fwd / 1e12:.3f} TFLOP, forward + backward {f_all / 1e12:.3f} TFLOP")
    stats = {}
    for name, ts in times.items():
        for phase, col, fl in (("fwd", 0, f_fwd), ("fwd+bwd", 1, f_all)):
            v = [t[col] for t in ts]
            mean, lo, hi = sum(v) / len(v), min(v), max(v)
            stats[name, phase] = (mean, lo, hi)
            print(f"{name:7s} {phase:8s} {mean:9.3f} ms  (min {lo:.3f}, max {hi:.3f}, spread {hi - lo:.3f})  "
                  f"{fl / mean / 1e9:7.1f} TFLOP/s")
    mt, mp = stats["tensor", "fwd+bwd"], stats["planes", "fwd+bwd"]
    gap, spread = mt[0] - mp[0], max(mt[2] - mt[1], mp[2] - mp[1])
    print(f"fwd+bwd: tensor - planes = {gap:.3f} ms ({mt[0] / mp[0]:.2f}x), larger min-max spread {spread:.3f} ms")
    print(f"faster by more than the spread: {'yes' if gap > spread else 'no'}")


if __name__ == "__main__":
    main()
