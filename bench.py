#!/usr/bin/env python3
"""Headline benchmark: videos/sec, forward + VideoSTGLoss + backward of the STCAT hot path
(BASELINE.json metric; config C3 = VidSTG e2e_STCAT_R101: T=64, 448x448, d=256, 10 text tokens, one video per GPU).

    python bench.py --gpus 1 --steps 5 --warmup 2
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P \
        bench.py --gpus N --steps K --warmup W

Prints ONE JSON line on rank 0.  A step = forward, loss, backward of one synthetic video per rank, gradients
averaged across ranks (RCCL all-reduce overlapped with backward) and usable at the end of the step; inputs
are resident in HBM before the timed region.  Weights are the deterministic synthetic set (no checkpoints
offline).  Default arithmetic (--mma bf16x6p) is fp32-class: backbone tensors are three bf16 planes whose sum IS the
fp32 value, products keep the six cross terms down to 2^-16 (error ~2^-24, like an fp32 product), accumulation is
fp32; Linear layers run the same six-term contraction on fp32 tensors and attention runs on the fp32 matrix pipe.

A plain run sets up, warms up, times --steps steps and prints the line; the legs of that line that need runs of their
own are null unless --full is given.  With --full the exact-fp32-MFMA mode (`exact_f32_mode`) and the 16-bit-operand
throughput mode (`throughput_mode`, bf16x3p) are timed beside it on the same step,
`roofline` is measured live with HIP events (torch.cuda.Event on the launch stream) around every C-ABI
launch in one extra instrumented step after the timed region, and `cpu_baseline` times the CPU oracle
(a port of the reference path) on a bounded sample on the host cores (the --no-* options switch single legs off).

--dump-outputs DIR writes what the last timed step computed (model outputs, losses, a fixed sample of every gradient
tensor and every gradient tensor's norm) as DIR/<name>.npy, for comparing two builds output for output.
"""
import argparse
import json
import os
import sys
import time

import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

from stcat_amd import _lib, ops, plans, synth  # noqa: E402
from stcat_amd.harness import TrainStep  # noqa: E402
from stcat_amd.misc import NestedTensor  # noqa: E402

PEAK_TFLOPS_F32_MFMA = 157.3   # MI355X_MICROARCH.md: v_mfma_f32_32x32x2_f32 dense peak
PEAK_TFLOPS_BF16_MFMA = 2500.0  # dense bf16 MFMA peak; a split-bf16 xN product costs N bf16 MFMA flops per flop
PEAK_HBM_GBS = 8000.0


# ------------------------------------------------------------------------------------------------
# algorithmic FLOPs of one C-ABI launch (2*MAC of the contraction it performs), from its arguments
# ------------------------------------------------------------------------------------------------
def _flops(name, a):
    if name == "stcat_conv_fwd":
        n, H, W, Cin, Cout, KH, KW, stride, pad = a[6:15]
        OH, OW = (H + 2 * pad - KH) // stride + 1, (W + 2 * pad - KW) // stride + 1
        return 2.0 * n * OH * OW * Cout * KH * KW * Cin
    if name == "stcat_conv_dgrad":
        n, H, W, Cin, Cout, KH, KW, stride, pad = a[9:18]
        OH, OW = (H + 2 * pad - KH) // stride + 1, (W + 2 * pad - KW) // stride + 1
        return 2.0 * n * OH * OW * Cout * KH * KW * Cin  # algorithmic MACs of the transposed conv
    if name == "stcat_conv_wgrad":
        n, H, W, Cin, Cout, KH, KW, stride, pad = a[3:12]
        OH, OW = (H + 2 * pad - KH) // stride + 1, (W + 2 * pad - KW) // stride + 1
        return 2.0 * n * OH * OW * Cout * KH * KW * Cin
    if name in ("stcat_pl_conv_fwd", "stcat_pl_conv_dgrad", "stcat_pl_conv_wgrad"):
        o = {"stcat_pl_conv_fwd": 12, "stcat_pl_conv_dgrad": 15, "stcat_pl_conv_wgrad": 6}[name]
        n, H, W, Cin, Cout, KH, KW, stride, pad = a[o:o + 9]
        OH, OW = (H + 2 * pad - KH) // stride + 1, (W + 2 * pad - KW) // stride + 1
        return 2.0 * n * OH * OW * Cout * KH * KW * Cin
    if name == "stcat_stem_fwd":
        n, H, W = a[5:8]
        return 2.0 * n * (H // 2) * (W // 2) * 64 * 147
    if name == "stcat_linear_fwd":
        return 2.0 * a[5] * a[6] * a[7]
    if name in ("stcat_linear_dgrad", "stcat_linear_wgrad"):
        o = 5 if name == "stcat_linear_dgrad" else 4
        return 2.0 * a[o] * a[o + 1] * a[o + 2]
    if name == "stcat_mha_self_fwd":
        B, H, S = a[6:9]
        return 2.0 * 2 * B * H * S * S * 32
    if name == "stcat_mha_self_bwd":
        B, H, S = a[12:15]
        return 2.0 * 4 * B * H * S * S * 32
    # round 6: every other contraction entry point of the step (the whole-step figure of `roofline.whole_step`)
    if name in ("stcat_mha_bs_fwd", "stcat_mha_self_fwd_lse"):
        B, H, S = a[6:9]
        return 2.0 * 2 * B * H * S * S * 32
    if name in ("stcat_mha_bs_bwd", "stcat_mha_self_bwd_lse"):   # dV, dP, dQ, dK (the recomputed score tiles are not counted)
        B, H, S = a[10:13]
        return 2.0 * 4 * B * H * S * S * 32
    if name == "stcat_pl_conv_wgrad_ws":
        n, H, W, Cin, Cout, KH, KW, stride, pad = a[6:15]
        OH, OW = (H + 2 * pad - KH) // stride + 1, (W + 2 * pad - KW) // stride + 1
        return 2.0 * n * OH * OW * Cout * KH * KW * Cin
    if name == "stcat_pl_conv_dgrad_cadd":
        n, H, W, Cin, Cout = a[11:16]
        return 2.0 * n * H * W * Cin * Cout
    if name == "stcat_pl_linear_fwd":
        return 2.0 * a[10] * a[11] * a[12]
    if name == "stcat_pl_linear_dgrad_mask":
        return 2.0 * a[9] * a[10] * a[11]
    if name in ("stcat_linear_fwd_acc", "stcat_linear_fwd_drop"):
        return 2.0 * a[5] * a[6] * a[7]
    if name == "stcat_linear_dgrad_acc":
        return 2.0 * a[4] * a[5] * a[6]
    if name == "stcat_linear_dgrad_mask":
        return 2.0 * a[7] * a[8] * a[9]
    if name in ("stcat_linear_fwd_multi", "stcat_linear_dgrad_multi", "stcat_linear_wgrad_multi"):
        return 2.0 * a[0] * a[33] * a[34] * a[35]
    if name == "stcat_stem_u8_fwd":
        n, H, W = a[7:10]
        return 2.0 * n * (H // 2) * (W // 2) * 64 * 147
    return 0.0


def _alg_elems(name, a):
    """operand ELEMENTS a plane conv forward / data-gradient launch has to move once (SURVEY.md section 8d's algorithmic
    bytes = this x 4 for fp32 tensors, x 6 for the three-plane format): gathered operand + weights + output (+ the
    residual / `add` operand when present; bit masks are 1/48 of a plane set and not counted)"""
    if name == "stcat_pl_conv_fwd":
        n, H, W, Cin, Cout, KH, KW, stride, pad = a[12:21]
        OH, OW = (H + 2 * pad - KH) // stride + 1, (W + 2 * pad - KW) // stride + 1
        e = n * H * W * Cin + n * OH * OW * Cout + Cout * KH * KW * Cin
        return e + (n * OH * OW * Cout if a[6] else 0)
    if name == "stcat_pl_conv_dgrad":
        n, H, W, Cin, Cout, KH, KW, stride, pad = a[15:24]
        OH, OW = (H + 2 * pad - KH) // stride + 1, (W + 2 * pad - KW) // stride + 1
        e = n * OH * OW * Cout + n * H * W * Cin + Cout * KH * KW * Cin
        return e + (n * H * W * Cin if a[4] else 0) + (n * H * W * Cin if a[12] else 0)
    return 0


def source_sha() -> str:
    """fingerprint of everything a PMC replay depends on: the kernel sources, the C ABI and this file"""
    import hashlib
    h = hashlib.sha256()
    cdir = os.path.join(ROOT, "stcat_amd", "csrc")
    for f in sorted(os.listdir(cdir)):
        h.update(open(os.path.join(cdir, f), "rb").read())
    h.update(open(os.path.join(ROOT, "bench.py"), "rb").read())
    return h.hexdigest()[:16]


def _replay_tag(path: str, d: dict) -> dict:
    """PMC counters cannot be read from inside the process: these figures are REPLAYED from a file committed by
    tools/gpu_round_artifacts.sh (rocprofv3 --pmc passes of this same command).  The file carries the source
    fingerprint it was measured on; `stale` says whether the kernels / this script changed since."""
    sha = d.get("source_sha")
    return {"replayed_from": os.path.relpath(path, ROOT), "measured_on_source_sha": sha,
            "stale": (sha != source_sha()) if sha else None}


def _pmc_traffic(entry: str, mma: str):
    """HBM bytes per launch of the dominant kernel family, from the committed rocprofv3 PMC passes of this same command
    (profiles/*hbm_traffic*<mode>*.json: FETCH_SIZE / WRITE_SIZE collected in separate passes, x1024, reads x2 per
    MI355X_MICROARCH.md §HBM).  PMC counters cannot be read from inside the process, hence the file."""
    import glob
    files = sorted(glob.glob(os.path.join(ROOT, "profiles", f"*hbm_traffic*{mma}.json")))
    if not files:
        return None
    doc = json.load(open(files[-1]))
    k = doc["kernels"]
    if "igemm_pl_fwd" in entry:
        pick = lambda n: "igemm_pl_fwd_kernel" in n or "igemm_pl_as_kernel" in n  # noqa: E731
    elif "igemm_bs_fwd" in entry:
        pick = lambda n: "igemm_bs_fwd_kernel<128" in n or "igemm_bs_fwd_kernel<256" in n  # noqa: E731
    else:
        fam = {"stcat_conv_fwd": "_fwd_kernel", "stcat_conv_dgrad": "_dgrad_kernel", "stcat_conv_wgrad": "_wgrad_kernel",
               "stcat_pl_conv_wgrad": "igemm_pl_wgrad_kernel"}.get(entry)
        if not fam:
            return None
        pick = lambda n: fam in n and "igemm" in n  # noqa: E731
    sel = [(v["launches"], v["read_MB_per_launch"], v["write_MB_per_launch"]) for n, v in k.items() if pick(n)]
    n = sum(a for a, _, _ in sel)
    if not n:
        return None
    steps_in_pass = doc.get("steps_traced") or 0
    return {"launches_per_step_in_pmc_pass": (n / steps_in_pass) if steps_in_pass else None,
            "MB_per_launch": round(sum(a * (r + w) for a, r, w in sel) / n, 1),
            "read_MB_per_launch": round(sum(a * r for a, r, _ in sel) / n, 1),
            "write_MB_per_launch": round(sum(a * w for a, _, w in sel) / n, 1), **_replay_tag(files[-1], doc),
            "note": "all launches of the kernel family in one step; PMC, separate FETCH_SIZE / WRITE_SIZE passes"}


def _pmc_mfma_util(mma: str):
    """MFMA utilisation of the dominant GEMM and of the encoder self-attention from the committed rocprofv3 PMC pass
    of this command (profiles/*mfma_util*.json, written by tools/pmc_mfma_util.py: SQ_VALU_MFMA_BUSY_CYCLES /
    (SQ_BUSY_CU_CYCLES or GRBM_GUI_ACTIVE x CUs), collected in its own run as the guide prescribes)."""
    import glob
    files = sorted(glob.glob(os.path.join(ROOT, "profiles", f"*mfma_util_bench*{mma}.json")))
    if not files:
        return None
    d = json.load(open(files[-1]))
    d.update(_replay_tag(files[-1], d))
    return d


def _flush_c_stdio():
    import ctypes
    try:
        ctypes.CDLL(None).fflush(None)
    except OSError:
        pass
    sys.stdout.flush()


def _shape_key(name, a):
    """conv shape of a plane-GEMM launch, for the per-shape table of the instrumented step"""
    if name in ("stcat_pl_conv_fwd", "stcat_pl_conv_dgrad", "stcat_pl_conv_wgrad"):
        o = {"stcat_pl_conv_fwd": 12, "stcat_pl_conv_dgrad": 15, "stcat_pl_conv_wgrad": 6}[name]
        n, H, W, Cin, Cout, KH, KW, stride, pad = a[o:o + 9]
        return f"{name[9:]} {n}x{H}x{W} {Cin}->{Cout} k{KH} s{stride}"
    if name in ("stcat_linear_fwd", "stcat_linear_dgrad", "stcat_linear_wgrad"):
        o = {"stcat_linear_fwd": 5, "stcat_linear_dgrad": 5, "stcat_linear_wgrad": 4}[name]
        return f"{name[6:]} M{a[o]} N{a[o + 1]} K{a[o + 2]}"
    return None


class LaunchProfiler:
    """Wraps _lib.call with a pair of HIP events per launch (same stream as the launch)."""

    def __init__(self):
        self.records = []
        self._orig = None

    def __enter__(self):
        self._orig = _lib.call

        def timed(name, *args):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            self._orig(name, *args)
            e1.record()
            self.records.append((name, _flops(name, args), e0, e1, _shape_key(name, args), _alg_elems(name, args)))

        _lib.call = timed
        import stcat_amd.ops as ops_mod
        ops_mod.L.call = timed
        return self

    def __exit__(self, *exc):
        _lib.call = self._orig
        torch.cuda.synchronize()

    def summary(self):
        agg = {}
        self.shapes = {}
        for name, fl, e0, e1, key, el in self.records:
            ms = e0.elapsed_time(e1)
            d = agg.setdefault(name, {"launches": 0, "ms": 0.0, "flop": 0.0, "elems": 0})
            d["launches"] += 1
            d["ms"] += ms
            d["flop"] += fl
            d["elems"] += el
            if key:
                d = self.shapes.setdefault(key, {"launches": 0, "ms": 0.0, "flop": 0.0})
                d["launches"] += 1
                d["ms"] += ms
                d["flop"] += fl
        return agg

    def shape_table(self, top=24):
        """the heaviest GEMM shapes of the instrumented step: launches, total ms, algorithmic TFLOP/s"""
        rows = sorted(self.shapes.items(), key=lambda kv: -kv[1]["ms"])[:top]
        return {k: {"launches": v["launches"], "ms": round(v["ms"], 3), "tflops": round(v["flop"] / v["ms"] / 1e9, 1)}
                for k, v in rows if v["ms"] > 0}


def _cpu_timed(fn, reps: int = 3, max_warm: int = 3, settle: float = 0.07):
    """warm-ups until two consecutive runs agree within `settle` (thread pools, allocator, page faults of the first big
    tensors: the round-5 samples 10.6 / 9.2 / 8.3 s were still trending — VERDICT r05 weak #7), at most `max_warm` + 1 of
    them; then `reps` timed repetitions.  Returns (median seconds, timed samples, warm-up samples)."""
    warm = []
    while len(warm) < max_warm + 1:
        t0 = time.perf_counter()
        fn()
        warm.append(time.perf_counter() - t0)
        if len(warm) >= 2 and abs(warm[-1] - warm[-2]) <= settle * warm[-2]:
            break
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        times.append(time.perf_counter() - t0)
    return sorted(times)[len(times) // 2], times, warm


def cpu_baseline(T_sample: int, res: int, L: int, T_full: int, threads: int, reps: int = 3, configs=("C1", "C3")):
    """the reference's CPU path (the oracle port) timed beside the GPU figure, forward-only AND
    forward + loss + backward, at C1 (the reference's own CPU-runnable case, measured in full) and at the headline
    workload C3 — on a bounded sample of T_sample of its T_full frames at full resolution, scaled by frames ("extrapolated":
    the per-frame backbone is 93 % of the work and attention is per frame, so cost is linear in frames).  The top-level
    value / unit / cores / kind / sample describe the headline leg (C3 forward + loss + backward)."""
    from oracle import stcat_oracle as O
    torch.set_num_threads(threads)
    sd = synth.synth_state_dict()
    frozen = ("vis_encoder.0.body.conv1", "vis_encoder.0.body.bn1", "vis_encoder.0.body.layer1")
    for k, v in sd.items():
        v.requires_grad_(not (k.startswith(frozen) or ".bn" in k or "downsample.1" in k or k.endswith(".te")))
    lines = {}
    for cfg in configs:
        Tc, rc, Lc = synth.CONFIGS[cfg]
        full = cfg != "C3" or T_sample >= Tc
        Ts = Tc if full else T_sample
        frames = synth.synth_frames(Ts, rc)
        mask = torch.zeros(Ts, rc, rc, dtype=torch.bool)
        act, tb = synth.synth_targets(Ts)
        text = synth.synth_text(Lc)

        def fwd():
            with torch.no_grad():
                O.stcat_forward(sd, frames, mask, text)

        def fwd_loss_bwd():
            for v in sd.values():
                v.grad = None
            out = O.stcat_forward(sd, frames, mask, text)
            O.total_loss(O.criterion(out, act, tb)).backward()

        entry = {}
        for name, fn in (("fwd", fwd), ("fwd_loss_bwd", fwd_loss_bwd)):
            dt, times, warm = _cpu_timed(fn, reps)
            entry[name] = {"videos_per_sec": round((Ts / Tc) / dt, 5), "seconds_per_sample": round(dt, 3),
                           "frames_timed": Ts, "frames_of_config": Tc, "extrapolated": not full,
                           "timed_s": [round(t, 2) for t in times], "warmup_s": [round(t, 2) for t in warm]}
        lines[cfg] = entry
        for v in sd.values():
            v.grad = None
    head = lines["C3"]["fwd_loss_bwd"] if "C3" in lines else lines[configs[-1]]["fwd_loss_bwd"]
    return {"value": head["videos_per_sec"], "unit": "videos/sec", "cores": threads, "kind": "port",
            "sample": f"oracle (CPU port of the reference path) fwd+loss+bwd on T={head['frames_timed']} of "
                      f"{head['frames_of_config']} frames at {res}x{res}, scaled by frames (extrapolated="
                      f"{head['extrapolated']}): median of {reps} repetitions ({', '.join(str(t) for t in head['timed_s'])} s) "
                      f"after {len(head['warmup_s'])} warm-up runs that settled within 7 % "
                      f"({', '.join(str(t) for t in head['warmup_s'])} s); `lines` holds forward-only and "
                      f"forward+loss+backward for C1 (in full) and C3",
            "lines": lines}


GRAD_SAMPLE = 4096          # elements per gradient tensor in grad_sample.npy (tensors this small are written whole)
DUMP_LIMIT_BYTES = 64 << 20


def dump_outputs(ts, total, out_dir: str) -> dict:
    """What a caller of the timed step receives after its LAST step, as out_dir/<name>.npy: the model outputs and aux
    outputs (kept before the criterion edits pred_boxes), the weighted total and every loss term, and the gradients —
    every tensor's L2 norm (float64, grad_norm.npy) and a sample of each drawn at indices from a fixed seed
    (grad_sample.npy, named_parameters order), so the whole set stays far below 64 MB.  Returns name -> shape."""
    import numpy as np
    os.makedirs(out_dir, exist_ok=True)
    arrays = {}

    def put(name, t):
        t = t.detach().cpu()
        t = t.double() if t.dtype == torch.float64 else t.float()
        arrays[name] = t.numpy()

    for k, v in ts.last_out.items():
        if k != "aux":
            put(k, v)
    for i, aux in enumerate(ts.last_out["aux"]):
        for k, v in aux.items():
            put(f"aux{i}_{k}", v)
    put("loss_total", total.reshape(1).double())
    for k, v in ts.last_losses.items():
        put(k if k.startswith("loss_") else f"loss_{k}", v.reshape(-1).double())
    gen = torch.Generator().manual_seed(20261016)
    norms, samples = [], []
    for _, g in ts.gradients().items():
        flat = g.reshape(-1)
        norms.append(flat.double().norm())
        if flat.numel() <= GRAD_SAMPLE:
            samples.append(flat.float())
        else:
            idx = torch.randint(0, flat.numel(), (GRAD_SAMPLE,), generator=gen)
            samples.append(flat[idx.to(flat.device)].float())
    put("grad_norm", torch.stack(norms))
    put("grad_sample", torch.cat(samples))
    size = sum(a.nbytes for a in arrays.values())
    assert size <= DUMP_LIMIT_BYTES, f"--dump-outputs: {size} bytes"
    for name, a in arrays.items():
        np.save(os.path.join(out_dir, name + ".npy"), a)
    return {name: list(a.shape) for name, a in arrays.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--config", default="C3", choices=list(synth.CONFIGS))
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-profile", action="store_true")
    ap.add_argument("--no-pin", action="store_true", help="do not pin the process to the GPU's NUMA node")
    ap.add_argument("--no-auto-graph", action="store_true", help="(accepted for compatibility; there is no automatic "
                    "eager/graph switch any more: every N runs the same launch mode)")
    ap.add_argument("--cpu-sample-frames", type=int, default=16,
                    help="frames of C3's bounded CPU-baseline sample (warm-ups until settled + 3 repetitions, forward-only "
                         "and forward+loss+backward; C1 is timed in full)")
    ap.add_argument("--cpu-threads", type=int, default=32, help="torch CPU threads for the oracle baseline")
    ap.add_argument("--mma", default="bf16x6p", choices=["f32", "bf16x3", "bf16x6", "bf16x3p", "bf16x6p", "f16x3p"],
                    help="arithmetic of the conv/Linear GEMM family.  Default bf16x6p: fp32-class (three bf16 planes per "
                         "backbone tensor = the fp32 value exactly, six cross terms per product, fp32 accumulate); "
                         "bf16x3p is the 16-significand-bit throughput mode (reported beside it with its measured error)")
    ap.add_argument("--eval-mode", action="store_true",
                    help="run the step with dropout off (the parity configuration); default is train mode, "
                         "dropout 0.1 / 0.3 active as in the reference's training loop")
    ap.add_argument("--graph", action="store_true",
                    help="replay the step as one captured hipGraph (stcat_amd/graph.py) instead of enqueuing it launch "
                         "by launch from Python; measured SLOWER on ROCm 7.2 (hipGraphLaunch walks ~3500 nodes on the "
                         "host: 99.5 vs 88.5 ms/step), so it is opt-in")
    ap.add_argument("--no-plans", action="store_true",
                    help="issue every launch from Python (round-2 behaviour) instead of replaying the composite nodes' "
                         "recorded launch plans with one C call each (stcat_amd/plans.py, csrc/launch_plan.h)")
    ap.add_argument("--serial", action="store_true",
                    help="run EVERY step on one stream (ops.single_stream: no forked decoder, no second forward chain, no "
                         "weight-gradient stream) — the schedule whose rocprofv3 kernel stats are per-kernel isolated "
                         "durations (profiles/*_kernel_stats_serial.csv); never the headline")
    ap.add_argument("--no-optim", action="store_true", help="skip the (untimed-in-metric) optimizer-tail timing")
    ap.add_argument("--no-exact", action="store_true", help="skip the extra exact-fp32-MFMA timing (N=1 only)")
    ap.add_argument("--roberta-dummy", action="store_true",
                    help="append a 124.6M-element dummy bucket so the all-reduce message matches the reference's (824 MB); "
                         "default at N > 1 (SURVEY.md §8d: the reference's DDP also reduces the RoBERTa gradients)")
    ap.add_argument("--no-roberta-dummy", action="store_true", help="N > 1: exchange the hot path's 327 MB only")
    ap.add_argument("--no-prefix-pipeline", action="store_true",
                    help="compute every clip's frozen prefix (stem + max-pool + layer1) at the head of its own step "
                         "(round-5 schedule); default: step k declares step k + 1's frames and their prefix runs on a side "
                         "stream under step k's grounding section (Backbone.stage_next) — every step still computes exactly "
                         "one prefix from its frame buffer, none is reused")
    ap.add_argument("--hoist-loss-plan", action="store_true",
                    help="build the loss's target-only index tensors and run its 1-element box-count all-reduce once, "
                         "outside the steps (round-3 behaviour); default: inside every timed step, as the reference does")
    ap.add_argument("--full", action="store_true",
                    help="after the timed steps also run every side measurement of the line: the instrumented roofline / "
                         "per-kernel steps, the other arithmetic modes, the optimizer tail, the evaluation path, the input "
                         "side, the hot-path-only exchange at N > 1 and the CPU baseline (each can be switched off by its "
                         "--no-* option); default: only the timed steps, those entries are null")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write what the last timed step computed as DIR/<name>.npy (float32 / float64): outputs, aux "
                         "outputs, losses, a seeded sample of every gradient tensor and every gradient tensor's L2 norm")
    args = ap.parse_args()

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a GPU (the product path has no CPU fallback)")
    # STCAT_DIST_BACKEND=gloo + several ranks on one GPU is a test configuration for 1-GPU boxes (RCCL itself
    # refuses duplicate devices); the driver's multi-GPU runs use nccl (= RCCL) with one GPU per rank
    backend = os.environ.get("STCAT_DIST_BACKEND", "nccl")
    local = min(local, torch.cuda.device_count() - 1) if backend != "nccl" else local
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    # one process per GPU, on the CPUs of the socket that GPU hangs off (two-socket hosts, four GPUs per socket)
    host_cpus = None if args.no_pin else _lib.pin_host_threads_to_gpu(local)
    # STCAT_FORCE_COMM=1: run the complete RCCL path (process group, barriers, bucketed async all-reduce, the
    # loss's box-count all-reduce) even with ONE rank — the only way to exercise it on a 1-GPU box
    force_comm = bool(os.environ.get("STCAT_FORCE_COMM")) and world == 1
    if force_comm:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29533")
        os.environ.setdefault("RANK", "0")
        os.environ.setdefault("WORLD_SIZE", "1")
    if world > 1 or force_comm:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if backend == "nccl":
            from stcat_amd.dist import init_rccl_process_group
            init_rccl_process_group(dev)
        else:
            dist.init_process_group(backend)
    assert world == args.gpus, f"--gpus {args.gpus} but WORLD_SIZE={world}"
    roberta_dummy = args.roberta_dummy or (world > 1 and not args.no_roberta_dummy)
    _lib.load()
    _lib.set_mma_mode(args.mma)

    T, res, L = synth.CONFIGS[args.config]
    # the step itself lives in stcat_amd/harness.py (tests/test_model_parity.py runs the same object against the
    # reference's fixtures): model, criterion, bucketed reducer, zero arena, per-step loss plan
    # two different synthetic clips per rank, resident in HBM, visited alternately: the step after this one always runs
    # OTHER pixels, so the pipelined prefix below is provably computed per step (tests/test_plans.py: every pipelined
    # step equals the un-pipelined step on the same clip)
    pipeline = not (args.no_prefix_pipeline or args.graph)
    clips = [(synth.synth_frames(T, res, seed=1000 * 3 + rank + 500 * j), torch.zeros(T, res, res, dtype=torch.bool))
             for j in range(2)]
    ts = TrainStep(dev, args.config, rank=rank, train=not args.eval_mode, roberta_dummy=roberta_dummy,
                   force_comm=force_comm, loss_plan_inside=not (args.hoist_loss_plan or args.graph),   # (a capture cannot hold the plan's H2D copy)
                   clips=clips, pipeline_prefix=pipeline)
    ts.keep_outputs = bool(args.dump_outputs)   # (every step keeps a copy of its outputs: the last timed one is dumped)
    model, criterion, wd, reducer, arena = ts.model, ts.criterion, ts.wd, ts.reducer, ts.arena
    videos, mask, targets = ts.videos, ts.videos.mask, ts.targets
    uniform_w = ts.uniform_w
    compute = ts.compute
    ts.loss_plan()

    comm = world > 1 or force_comm
    comm_events = []  # (end of backward, gradients averaged) per step: the EXPOSED part of the gradient exchange

    def eager_step():
        reducer.zero_grad()
        total = compute()
        if comm:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            reducer.finish()
            e1.record()
            comm_events.append((e0, e1))
        else:
            reducer.finish()
        return total


    def fence():
        if comm:
            dist.barrier()
        torch.cuda.synchronize()

    step = eager_step
    graphed = None
    if args.graph:
        # the whole step as ONE hipGraph launch (stcat_amd/graph.py); gradient exchange runs after each replay
        from stcat_amd.graph import GraphedStep
        # no eager autograd pass on the default stream before this point: AccumulateGrad nodes remember the stream
        # they were created on, and default-stream ones break capture; GraphedStep warms up on a side stream
        reducer.zero_grad()
        reducer.defer(True)
        graphed = GraphedStep(compute, dev, warmup=1)
        reducer.bind_static_grads()

        def step():
            total = graphed.replay()
            reducer.finish()
            return total

    if args.serial:
        ops.FORK_ENABLED = ops.WGRAD_STREAM_ENABLED = False
    use_plans = not args.no_plans and not args.graph
    plans.enable(use_plans)
    if use_plans:
        # a node runs eagerly the first time it sees a signature and is recorded the second time: both happen here, so
        # the W warm-up steps and the K timed steps are all replays, whatever W is
        # (with the pipelined prefix the backbone node has two signatures: the first step computes its prefix in place,
        #  the following ones find it staged — eager, eager + staged, record, then replays; the staged prefix itself is a
        #  launch plan per resident buffer, and the two buffers alternate: eager, eager, record, record — five steps)
        for _ in range(5 if pipeline else 2):
            step()
    for _ in range(args.warmup):
        step()
    fence()
    comm_events.clear()
    pstats0 = dict(ts.model.vis_encoder[0].prefix_stats)
    t0 = time.perf_counter()
    c0 = time.process_time()
    for _ in range(args.steps):
        last_total = step()
    pstats1 = dict(ts.model.vis_encoder[0].prefix_stats)
    host_s = time.perf_counter() - t0  # host time to ENQUEUE the steps (no sync): ~= elapsed means launch-bound
    host_cpu_s = time.process_time() - c0  # CPU time of all threads of this process while enqueuing (python + autograd
    #                                        engine thread + HIP runtime): excludes the time a full launch queue blocks
    fence()
    dt = torch.tensor([time.perf_counter() - t0], device=dev)
    if comm:
        dist.all_reduce(dt, op=dist.ReduceOp.MAX)
    elapsed = dt.item()
    # exposed gradient-exchange time: device time between the last backward kernel and the averaged gradients
    # (all-reduces that did not finish under the backward pass + the 1/world scaling), rank 0, mean over the timed steps
    exposed_ms = (sum(a.elapsed_time(b) for a, b in comm_events) / len(comm_events)) if comm_events else None
    dumped = None
    if args.dump_outputs and rank == 0:
        dumped = dump_outputs(ts, last_total, args.dump_outputs)

    # Everything below measures something other than the headline and runs with --full only.
    full = args.full
    profile = full and not args.no_profile

    if graphed is not None:  # the instrumented / side measurements below time individual launches: eager mode
        reducer.defer(False)
        step = eager_step
    roof, kernels, gemm_shapes = None, None, None
    if profile:
        # Two extra instrumented steps; EVERY rank runs them (a step contains collectives), rank 0 records events.  They
        # bracket every launch with HIP events on the launch's own stream, launch by launch from Python (same kernels,
        # same order as the replayed plans).  (1) the step as scheduled — three streams, kernels of different streams
        # overlap, so a launch's duration there is a CO-SCHEDULED figure; (2) the same step on ONE stream
        # (ops.single_stream): kernels run one at a time, a launch's duration is the kernel's own.  The roofline is
        # priced on (2) (297 x 0.306 ms of the dominant kernel "inside" an 84.9 ms step).
        plans.enable(False)
        if rank == 0:
            with LaunchProfiler() as prof:
                step()
            with ops.single_stream():
                step()                                   # (allocator / cache warm-up of the one-stream schedule)
                with LaunchProfiler() as prof_iso:
                    step()
        else:
            step()
            with ops.single_stream():
                step()
                step()
        plans.enable(use_plans)

    def family(agg):
        # dominant KERNEL: in the split-bf16 modes the conv forward and the conv data gradient (pre-transposed
        # weights) are the same device kernel — price them together
        fam = dict(agg)
        if args.mma in ("bf16x3p", "bf16x6p", "f16x3p") and "stcat_pl_conv_fwd" in agg and "stcat_pl_conv_dgrad" in agg:
            a, b = agg["stcat_pl_conv_fwd"], agg["stcat_pl_conv_dgrad"]
            fam = {k: v for k, v in agg.items() if k not in ("stcat_pl_conv_fwd", "stcat_pl_conv_dgrad")}
            fam["igemm_pl_fwd_kernel + igemm_pl_as_kernel (stcat_pl_conv_fwd + stcat_pl_conv_dgrad)"] = {
                "launches": a["launches"] + b["launches"], "ms": a["ms"] + b["ms"], "flop": a["flop"] + b["flop"],
                "elems": a.get("elems", 0) + b.get("elems", 0)}
        elif args.mma != "f32" and "stcat_conv_fwd" in agg and "stcat_conv_dgrad" in agg:
            a, b = agg["stcat_conv_fwd"], agg["stcat_conv_dgrad"]
            fam = {k: v for k, v in agg.items() if k not in ("stcat_conv_fwd", "stcat_conv_dgrad")}
            fam["igemm_bs_fwd_kernel (stcat_conv_fwd + stcat_conv_dgrad)"] = {
                "launches": a["launches"] + b["launches"], "ms": a["ms"] + b["ms"], "flop": a["flop"] + b["flop"]}
        return fam

    if rank == 0 and profile:
        agg = prof.summary()
        agg_iso = prof_iso.summary()
        kernels = {k: {"launches": v["launches"], "ms": round(v["ms"], 3),
                       "isolated_ms": round(agg_iso[k]["ms"], 3) if k in agg_iso else None,
                       "tflops": (round(v["flop"] / agg_iso[k]["ms"] / 1e9, 2)
                                  if v["flop"] and k in agg_iso and agg_iso[k]["ms"] else None)}
                   for k, v in sorted(agg.items(), key=lambda kv: -kv[1]["ms"])}
        fam, fam_iso = family(agg), family(agg_iso)
        dom = max((k for k in fam if fam[k]["flop"] > 0), key=lambda k: fam[k]["ms"])
        d = fam_iso.get(dom, fam[dom])       # ISOLATED durations: one stream, one kernel at a time
        d_co = fam[dom]
        ach = d["flop"] / d["launches"] / (d["ms"] / d["launches"] * 1e-3) / 1e12
        # `achieved` = ALGORITHMIC flops (2 x MAC of the contraction) / launch time and `frac` = that
        # over the peak of the pipe the kernel runs on.  A split-bf16 product issues 3 (6) bf16 MFMA flops per
        # algorithmic flop: the issued rate — what the matrix pipe actually executes — is reported beside it.
        mult = {"f32": 1, "bf16x3": 3, "bf16x6": 6, "bf16x3p": 3, "bf16x6p": 6, "f16x3p": 3}[args.mma]
        peak = PEAK_TFLOPS_F32_MFMA if args.mma == "f32" else PEAK_TFLOPS_BF16_MFMA
        roof = {"bound": "mfma", "kernel": dom, "achieved": round(ach, 2), "peak": peak,
                "unit": "TFLOP/s", "frac": round(ach / peak, 4), "traffic": None,
                "issued_tflops": round(ach * mult, 2), "issued_frac": round(ach * mult / peak, 4),
                "mfma_flops_per_algorithmic_flop": mult,
                "launches": d["launches"], "avg_launch_ms": round(d["ms"] / d["launches"], 4),
                "isolated_avg_launch_ms": round(d["ms"] / d["launches"], 4),
                "co_scheduled_avg_launch_ms": round(d_co["ms"] / d_co["launches"], 4),
                "duration_note": "achieved / frac use the ISOLATED per-launch duration (instrumented step on one stream: "
                                 "kernels run one at a time); co_scheduled = the same launches inside the three-stream "
                                 "step, where kernels of other streams share the CUs; rocprofv3 kernel stats of both "
                                 "schedules: profiles/r06_bench_c3_kernel_stats_{serial,bf16x6p}.csv",
                "algorithmic_gflop_per_launch": round(d["flop"] / d["launches"] / 1e9, 3)}
        tr = _pmc_traffic(dom, args.mma)
        # `traffic`: HBM bytes per launch of the dominant kernel family (PMC FETCH_SIZE / WRITE_SIZE passes, see the
        # detail entry for the split and the source file); `achieved`'s counterpart in bytes: algorithmic operand bytes
        roof["traffic"] = int(tr["MB_per_launch"] * 1e6) if tr else None
        roof["traffic_detail"] = tr
        # bytes per STEP of the family, next to what the contractions have to move at least
        # (every operand once: fp32 tensors = 4 bytes per element, the three-plane format the kernels use = 6)
        el = d.get("elems", 0)
        planes = {"bf16x3p": 2, "bf16x6p": 3, "f16x3p": 2}.get(args.mma)
        roof["algorithmic_GB_per_step_fp32"] = round(el * 4 / 1e9, 2) if el else None
        roof["algorithmic_GB_per_step_planes"] = round(el * 2 * planes / 1e9, 2) if el and planes else None
        if tr and tr.get("launches_per_step_in_pmc_pass"):
            gb = tr["MB_per_launch"] * tr["launches_per_step_in_pmc_pass"] / 1e3
            roof["traffic_GB_per_step"] = round(gb, 2)
            roof["traffic_over_algorithmic_planes"] = (round(gb / (el * 2 * planes / 1e9), 3) if el and planes else None)
            roof["traffic_over_algorithmic_fp32"] = round(gb / (el * 4 / 1e9), 3) if el else None
        roof["mfma_util"] = _pmc_mfma_util(args.mma)
        mm = sum(v["flop"] for v in agg_iso.values())
        mm_ms = sum(v["ms"] for v in agg_iso.values() if v["flop"] > 0)
        roof["all_mfma_kernels"] = {"tflops": round(mm / mm_ms / 1e9, 2), "ms": round(mm_ms, 2),
                                    "gflop_per_step": round(mm / 1e9, 1)}
        # the WHOLE step against the matrix pipes — every contraction's algorithmic flops (convs, Linears,
        # attention) over the timed step's wall clock: what fraction of the dense bf16 peak the step sustains, the same
        # with the six MFMA flops this arithmetic issues per flop, and against the fp32 matrix pipe (the reference's own
        # arithmetic could not run faster than frac_fp32_pipe = 1)
        step_s = elapsed / args.steps
        roof["whole_step"] = {"gflop_per_step": round(mm / 1e9, 1), "ms_per_step": round(1e3 * step_s, 2),
                              "tflops": round(mm / step_s / 1e12, 2),
                              "frac_bf16": round(mm / step_s / 1e12 / PEAK_TFLOPS_BF16_MFMA, 4),
                              "issued_frac_bf16": round(mm * mult / step_s / 1e12 / PEAK_TFLOPS_BF16_MFMA, 4),
                              "frac_fp32_pipe": round(mm / step_s / 1e12 / PEAK_TFLOPS_F32_MFMA, 4)}
        gemm_shapes = prof_iso.shape_table()
    if comm:
        dist.barrier()

    # report the gradient exchange two ways.  The headline at N > 1 carries the reference-sized message
    # (hot path 327 MB + a 498 MB stand-in for the RoBERTa gradients the reference's DDP also reduces); the same steps
    # with the hot path's own 327 MB only are timed beside it.
    hot_only = None
    if full and world > 1 and roberta_dummy:
        reducer.skip_extra = True
        step()
        fence()
        t1 = time.perf_counter()
        n_hot = max(2, min(args.steps, 10))
        for _ in range(n_hot):
            step()
        fence()
        dt_h = torch.tensor([time.perf_counter() - t1], device=dev)
        dist.all_reduce(dt_h, op=dist.ReduceOp.MAX)
        hot_only = {"allreduce_bytes": reducer.message_bytes, "steps": n_hot, "ms_per_step": round(1e3 * dt_h.item() / n_hot, 2),
                    "value": round(world * n_hot / dt_h.item(), 4)}
        reducer.skip_extra = False
        dist.barrier()

    # The other arithmetic modes, timed on the same step beside the headline: the exact-fp32 mode is the
    # reference's own arithmetic, bf16x6 the fp32-class split mode, bf16x3 the 16-bit-operand mode on fp32 tensors.
    exact, other_modes = None, None
    if full and world == 1 and not args.no_exact:
        other_modes = {}
        notes = {"f32": "f32 (v_mfma_f32_32x32x2_f32, exact products)", "bf16x6": "fp32 tensors, 6 bf16 cross terms (fp32-class)",
                 "bf16x3": "fp32 tensors, 3 bf16 cross terms, operands split in-kernel",
                 "bf16x3p": "3 bf16 cross terms, backbone tensors pre-split into two bf16 planes (16 significand bits)",
                 "bf16x6p": "6 bf16 cross terms, backbone tensors pre-split into three bf16 planes (= fp32 exactly)",
                 "f16x3p": "3 fp16 cross terms, backbone tensors pre-split into two fp16 planes (22 significand bits; weight / "
                           "gradient planes scaled by 2^6 / 2^16 into fp16's range) — experimental"}
        for mode in ("f32", "bf16x6", "bf16x3", "bf16x3p", "bf16x6p", "f16x3p"):
            if mode == args.mma:
                continue
            _lib.set_mma_mode(mode)
            if use_plans:          # the plans of the previous mode hold tens of GB of static activations: drop them
                plans.clear()
                torch.cuda.empty_cache()
            for _ in range(5 if pipeline else 3):   # (a mode switch re-creates the weight-plane / transposed-weight caches:
                step()                              #  warm up; with launch plans: eager, record, first replay — five with the
                #                                      pipelined prefix, whose own two plans record in steps 3 and 4)
            fence()
            n_m = max(10, args.steps) if mode == "f16x3p" else 10      # (the candidate mode gets the headline's step count)
            t1 = time.perf_counter()
            for _ in range(n_m):
                step()
            fence()
            dt_m = (time.perf_counter() - t1) / n_m
            other_modes[mode] = {"mma": notes[mode], "value": round(1.0 / dt_m, 4), "ms_per_step": round(1e3 * dt_m, 2),
                                 "steps": n_m, "warmup": 5 if pipeline else 3}
        _lib.set_mma_mode(args.mma)
        if use_plans:
            plans.clear()
            torch.cuda.empty_cache()
        exact = other_modes.get("f32")
    throughput_mode = None
    if other_modes and "bf16x3p" in other_modes:
        throughput_mode = dict(other_modes["bf16x3p"])
        throughput_mode["measured_error"] = (
            "16 significand bits per operand: outputs pass the same absolute 1e-3 / bit-exact-span tests at C3; "
            "worst gradient tensor rel-L2 vs an fp64 oracle run at C3: layer2 6.7e-3, layer3 4.2e-3, layer4 1.8e-3, "
            "encoder 8.4e-4, decoders 4.1e-3 (profiles/r02_grad_error_C3_bf16x3p_bf16x3.json; the fp32 CPU reference "
            "itself: 1.5e-3) — NOT the headline: narrower than the reference's fp32")

    near_f32_mode = None
    if other_modes and "f16x3p" in other_modes:
        near_f32_mode = dict(other_modes["f16x3p"])
        near_f32_mode["measured_error"] = (
            "22 significand bits per backbone tensor (two fp16 planes), three products, fp32 accumulate; per-product error ~3x "
            "an fp32 product rounding (tools/split_precision_probe.py).  Held by the SAME tests as the default: reference "
            "fixtures at C1 / C2 / C3 / C5 / padded / non-square clips, outputs 1e-3 absolute, spans bit-exact, the calibrated "
            "fp32 gradient bound (tests/test_model_parity.py::test_gpu_c3_full_size_forward_backward_fp16_planes: worst tensor "
            "1.9e-3 from the reference's fp64 run where bf16x6p is 2.0e-3, the exact-fp32 mode 1.75e-3 and the fp32 reference "
            "1.3e-3; profiles/r04_gpu_tests.log, profiles/r04_grad_error_C3_f16x3p_bf16x6p.json).  NOT the headline: its storage "
            "is two bits narrower than fp32 and its power-of-two operand scales (weights 2^6, gradients 2^16) are constants")

    # Optimizer tail (clip_grad_norm_ + AdamW + EMA, scripts/train_net.py:134-143): NOT part of the fwd+bwd metric;
    # timed here on the gradients the last step left behind so the cost of the next stage is on record.
    opt_tail = None
    if full and world == 1 and not args.no_optim:
        import copy
        from stcat_amd import optim
        named = [(n, p) for n, p in model.named_parameters() if p.grad is not None]
        groups = [{"params": [p for n, p in named if "vis_encoder" not in n and "temp_decoder" not in n]},
                  {"params": [p for n, p in named if "vis_encoder" in n], "lr": 2e-5},
                  {"params": [p for n, p in named if "temp_decoder" in n], "lr": 1e-4}]
        opt = optim.AdamW(groups, lr=1e-4, weight_decay=1e-4)
        ema = copy.deepcopy(model)
        numel = sum(p.numel() for _, p in named)
        for _ in range(2):
            opt.step(max_grad_norm=0.1, model_ema=ema, ema_decay=0.9998, model=model)
        fence()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t1 = time.perf_counter()
        e0.record()
        for _ in range(5):
            opt.step(max_grad_norm=0.1, model_ema=ema, ema_decay=0.9998, model=model)
        e1.record()
        fence()
        dt_wall = (time.perf_counter() - t1) / 5
        dt_opt = e0.elapsed_time(e1) / 5e3
        opt_tail = {"ms": round(1e3 * dt_opt, 3), "wall_ms": round(1e3 * dt_wall, 3), "parameters": numel,
                    "launches": 2, "GB_per_s": round(numel * 40 / dt_opt / 1e9, 1),
                    "note": "10 fp32 accesses per parameter (g twice); HBM-bound; ms = device time (HIP events)"}
        del opt, ema

    # Evaluation path (engine/evaluate.py:97-119): two forward passes on the even / odd frames, device-side T x T map
    # argmax, span union, linear_interp of skipped frames — videos/s of test_net.py's inner loop on the same clip.
    eval_path = None
    if full and world == 1 and not args.no_exact:
        from stcat_amd.pipeline import build_postprocessors, evaluate_video
        post = build_postprocessors()
        was_training = model.training
        model.eval()
        sizes = torch.tensor([[float(res), float(res)]], device=dev).repeat(T, 1)
        ids = [list(range(0, 2 * T, 2))]  # every second frame of the source video: the rest are interpolated
        with torch.no_grad():
            evaluate_video(model, post, videos, ["synthetic"], sizes, ids, interpolate=True)
            fence()
            t1 = time.perf_counter()
            for _ in range(5):
                boxes_e, span_e = evaluate_video(model, post, videos, ["synthetic"], sizes, ids, interpolate=True)
            fence()
        dt_e = (time.perf_counter() - t1) / 5
        eval_path = {"value": round(1.0 / dt_e, 3), "unit": "videos/sec", "ms_per_video": round(1e3 * dt_e, 2),
                     "what": f"2-pass eval (2 x {T // 2} frames) + PostProcess + span union + linear_interp "
                             f"({len(boxes_e)} boxes out), no_grad, eval mode"}
        # the same with decoder + heads replayed from a hipGraph (BASELINE configs[4]; STCATNet.capture_decoder)
        try:
            model.capture_decoder(True)
            with torch.no_grad():
                evaluate_video(model, post, videos, ["synthetic"], sizes, ids, interpolate=True)
                fence()
                t1 = time.perf_counter()
                for _ in range(5):
                    boxes_g, span_g = evaluate_video(model, post, videos, ["synthetic"], sizes, ids, interpolate=True)
                fence()
            dt_g = (time.perf_counter() - t1) / 5
            eval_path["captured_decoder"] = {"value": round(1.0 / dt_g, 3), "ms_per_video": round(1e3 * dt_g, 2),
                                             "same_span": span_g == span_e,
                                             "graph_replays": model._graphed_decoder.replays}
        except RuntimeError as e:       # (reported, never fatal for the bench line)
            eval_path["captured_decoder"] = {"error": str(e)[:200]}
        finally:
            model.capture_decoder(False)
        model.train(was_training)

    # Input side: the boundary can also take the decoder's uint8 HWC frames; ToTensor + Normalize are
    # fused into the stem's gather.  PCIe-inclusive rate of the step when every step first uploads its frames from
    # pinned host memory: 38.5 MB (uint8) instead of 154 MB (the normalised fp32 tensor).  Never `value`.
    loader = None
    if full and world == 1 and not args.no_exact:
        u8_host = torch.randint(0, 256, (T, res, res, 3), dtype=torch.uint8).pin_memory()
        f32_host = torch.empty(T, 3, res, res, dtype=torch.float32).pin_memory()
        loader = {"h2d_MB_uint8": round(u8_host.numel() / 1e6, 1), "h2d_MB_fp32": round(f32_host.numel() * 4 / 1e6, 1)}
        for key, host in (("uint8", u8_host), ("fp32", f32_host)):
            # a resident device buffer per input form, refilled by an async copy each step (what a loader does; a fresh
            # `host.to(dev)` per step would hand the allocator a 154 MB block that several streams still hold)
            dev_buf = torch.empty(host.shape, dtype=host.dtype, device=dev)

            def run_once():
                dev_frames = dev_buf.copy_(host, non_blocking=True)
                reducer.zero_grad()
                ops.dropout_begin_step(dev)
                arena.reset()
                out = model(NestedTensor(dev_frames, mask, [T]), ["synthetic"])
                losses = criterion(out, targets, [T], plan=ts.loss_plan())
                total = criterion.weighted_total(wd) if uniform_w else sum(losses[k] * wd[k] for k in losses)
                total.backward()
                reducer.finish()
            for _ in range(5):   # (freshly pinned memory: the first uploads are slow — measured 76 ms vs 61.6 ms steps)
                run_once()
            fence()
            t1 = time.perf_counter()
            for _ in range(5):
                run_once()
            fence()
            loader[f"ms_per_step_with_{key}_h2d"] = round(1e3 * (time.perf_counter() - t1) / 5, 2)
        # ... and with the copy OFF the compute stream: copy stream + two resident device buffers (stcat_amd/loader.py),
        # clip k + 1 is uploaded while clip k computes
        from stcat_amd.loader import DeviceFramePrefetcher

        def clips(host, n):
            for _ in range(n):
                yield host
        for key, host in (("uint8", u8_host), ("fp32", f32_host)):
            def run_on(dev_frames):
                reducer.zero_grad()
                ops.dropout_begin_step(dev)
                arena.reset()
                out = model(NestedTensor(dev_frames, mask, [T]), ["synthetic"])
                losses = criterion(out, targets, [T], plan=ts.loss_plan())
                total = criterion.weighted_total(wd) if uniform_w else sum(losses[k] * wd[k] for k in losses)
                total.backward()
                reducer.finish()
            pf = DeviceFramePrefetcher(clips(host, 12), dev)
            for i_, fr in enumerate(pf):
                if i_ == 5:
                    fence()
                    t1 = time.perf_counter()
                run_on(fr)
            fence()
            loader[f"ms_per_step_with_{key}_h2d_overlapped"] = round(1e3 * (time.perf_counter() - t1) / 7, 2)
        loader["note"] = ("frames uploaded from pinned host memory inside every step (PCIe Gen5 x16); uint8 = decoder "
                          "output [T,H,W,3], normalised inside the stem kernel; fp32 = the reference's normalised [T,3,H,W]; "
                          "_overlapped = the same upload on a copy stream into two resident buffers while the "
                          "previous step computes (stcat_amd/loader.py)")

    cpu = None
    if full and rank == 0 and world == 1 and not args.no_cpu_baseline:  # N=1 only: other ranks would idle at the barrier
        # (cores: the process's CPU budget where OMP_NUM_THREADS states one — more threads than cores only slow the oracle)
        cores = int(os.environ.get("OMP_NUM_THREADS") or 0) or len(os.sched_getaffinity(0)) or os.cpu_count() or 1
        cpu = cpu_baseline(min(args.cpu_sample_frames, T), res, L, T, min(cores, args.cpu_threads))

    if rank == 0:
        line = {
            "metric": "videos/sec fwd+bwd @ T=64 res=448 d=256", "value": round(world * args.steps / elapsed, 4),
            "unit": "videos/sec", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": round(1e3 * elapsed / args.steps, 2), "higher_is_better": True, "scaling": "weak",
            "host_enqueue_ms_per_step": round(1e3 * host_s / args.steps, 2),
            "host_cpu_ms_per_step": round(1e3 * host_cpu_s / args.steps, 2),
            "host_cpus": host_cpus,
            "host_note": "host_enqueue_ms_per_step is wall time of the enqueue loop: it INCLUDES the time hipLaunchKernel "
                         "blocks while the launch queue is full (the host runs ahead of a GPU-bound step); the host's own "
                         "work is the C1 line of profiles/r03_bench_variants.log (same launch sequence, ~no GPU work)",
            "plan_stats": dict(plans.STATS),
            "streams": ops.PICK_REPORT.get(str(dev)),
            "prefix_lane": __import__("stcat_amd.backbone", fromlist=["x"]).PREFIX_LANE_REPORT.get(str(dev)),
            "exposed_comm_ms_per_step": (round(exposed_ms, 3) if exposed_ms is not None else None),
            "vs_baseline": None,
            "dtype": {"f32": "f32", "bf16x3": "f32 tensors, bf16x3 split products, f32 accumulate",
                      "bf16x6": "f32 tensors, bf16x6 split products, f32 accumulate",
                      "bf16x3p": "bf16x3 split products, f32 accumulate; backbone tensors stored as bf16 hi+lo planes "
                                 "(16 significand bits), everything else f32",
                      "f16x3p": "near-f32 (22 significand bits): f16x3 split products on two fp16 planes per backbone tensor, f32 "
                                "accumulate; everything else as bf16x6p — experimental, not the default",
                      "bf16x6p": "f32-class: bf16x6 split products (six cross terms, ~2^-24), f32 accumulate; backbone "
                                 "tensors stored as three bf16 planes (hi+mid+lo = the f32 value exactly), everything "
                                 "else f32, attention on the f32 matrix pipe"}[args.mma], "data": "synthetic",
            "config": {"workload": f"{args.config}: VidSTG e2e_STCAT_R101 hot path, T={T} res={res} d=256 L={L}, "
                                   "fwd+loss+bwd, 1 video/GPU", "parallelism": f"dp{world}",
                       "mode": "eval (dropout off)" if args.eval_mode else "train (dropout 0.1/0.3 on)",
                       "schedule": "ONE stream (--serial)" if args.serial else "three streams (forward chains / forked time "
                                   "decoder, weight gradients)",
                       "launch": ("one hipGraph per step" if args.graph else
                                  "launch plans: one C call replays each composite node's recorded launch sequence "
                                  "(backbone fwd/bwd, encoder, box/time decoder, heads)" if use_plans else
                                  "eager (launch by launch from Python)"),
                       "clips": "two synthetic clips per rank, resident in HBM, visited alternately",
                       "prefix_pipeline": ("on: step k declares step k+1's frames (Backbone.stage_next); their frozen prefix "
                                           "(stem + max-pool + layer1, no backward: backbone.py:78-85) runs on a side stream "
                                           "under step k's grounding section; one prefix computed per step, none reused "
                                           f"(the {args.steps} timed steps: {pstats1['taken'] - pstats0['taken']} started from a "
                                           f"staged prefix, {pstats1['inline'] - pstats0['inline']} computed theirs in place)"
                                           if pipeline else
                                           "off: every step computes its clip's prefix at its own head"),
                       "allreduce_bytes": reducer.message_bytes,
                       "allreduce": ({"allreduce": "all-reduce per bucket (RCCL's algorithm choice)",
                                      "rs_ag": "reduce-scatter + all-gather per bucket"}[reducer.collective]
                                     + "; STCAT_DP_COLLECTIVE switches; no multi-GPU figure has been measured by the builder"),
                       "loss_plan": ("built once outside the steps (--hoist-loss-plan / --graph)" if (args.hoist_loss_plan or args.graph) else
                                     "rebuilt inside every timed step (target index tensors from host-side annotations, "
                                     "one pinned H2D copy, the 1-element box-count all-reduce)")},
            "hot_path_only_exchange": hot_only,
            "roofline": roof, "cpu_baseline": cpu, "exact_f32_mode": exact, "throughput_mode": throughput_mode,
            "near_f32_mode": near_f32_mode,
            "other_modes": other_modes,
            "optimizer_tail": opt_tail, "eval_path": eval_path, "input_side": loader,
            "timed_region": "forward + VideoSTGLoss + backward (+ gradient exchange at N > 1), including the per-step "
                            "split of all conv weights into bf16 planes (as after an optimizer step), the loss's "
                            "target-derived index tensors (LossPlan, criterion.py:160-192) and its 1-element box-count "
                            "all-reduce (criterion.py:175-178) — all inside every timed step since round 4",
            "kernels": kernels,
            "gemm_shapes": gemm_shapes,
            "full": full,            # False: the side legs above (roofline .. input_side, cpu_baseline) were not run
            "dumped_outputs": dumped,
        }
    # The JSON line must be the LAST thing on stdout.  RCCL writes a version banner through C stdio, which is
    # block-buffered when stdout is a pipe and would otherwise be flushed at process exit, AFTER the line: flush
    # it on every rank, tear the process group down, and only then print.
    _flush_c_stdio()
    if comm:
        dist.barrier()
        dist.destroy_process_group()
        _flush_c_stdio()
    if rank == 0:
        sys.stdout.write(json.dumps(line) + "\n")
        sys.stdout.flush()


if __name__ == "__main__":
    main()
