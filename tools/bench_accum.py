#!/usr/bin/env python3
"""What gradient accumulation costs per micro-step at the flagship shape: C3, bf16x6p, train mode, launch plans on, the
pipelined prefix on — spans of four clips and one optimizer step, three loops, alternating, in ONE process:

  (A) four plain TrainStep.step()s, then optimizer.step(): no accumulation (three gradients are thrown away) — the
      floor: what the four steps and the optimizer cost anyway;
  (B) TrainStep.window(optimizer, 4): accumulate() after the first three micro-steps, step() after the last;
  (C) the loop the refusals used to point to: launch plans off, gradients kept in p.grad over four backward passes.
      Timed only if it arrives at (B)'s gradients (checked first, from one seed); otherwise the log says why not.

    python tools/bench_accum.py [--reps 20] [--warmup 3] [--config C3] [--k 4]
    python tools/bench_accum.py --canonical [...]      # the canonical-window leg instead (below)

Prints median / min / max per variant, (B - A) per micro-step with the bytes per second the folds would have reached had
they alone made the difference (a fold moves 12 B per element, 8 B the first of a window), the fold timed on its own,
and for (C) whether (B) is faster by more than the larger min-max spread.  Every learning rate is 0, so all spans see
the same weights; the optimizer's launches do not depend on the values.

--canonical: what the canonical window (stcat_amd.set_canonical_window) costs — deterministic mode on throughout, one
rank, alternating in ONE process:
  (D) TrainStep.window(optimizer, k) with the window off: the deterministic window as it was before the mode existed
      (stcat_grad_accumulate: one accumulator, a chain);
  (E) the same with set_canonical_window(k): stcat_grad_tree_fold through log2(k) level buffers, the dropout counters set
      from the clip number, the loss normalised by the window's box count (one device scalar).
Prints median / min / max of both and whether (E) - (D) exceeds the larger min-max spread."""
import argparse
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from stcat_amd import _lib as L  # noqa: E402
from stcat_amd import ops, optim, plans, synth  # noqa: E402
from stcat_amd.harness import TrainStep  # noqa: E402

SEED = 4242


def canonical_leg(a):
    import stcat_amd
    k = a.k
    L.load()
    L.set_mma_mode("bf16x6p")
    L.set_deterministic(True)
    dev = torch.device("cuda:0")
    T, res, _ = synth.CONFIGS[a.config]
    clips = [(synth.synth_frames(T, res, seed=3000 + 500 * j), torch.zeros(T, res, res, dtype=torch.bool)) for j in range(2)]
    plans.enable(True)
    ts = TrainStep(dev, a.config, train=True, clips=clips, pipeline_prefix=True)
    # one optimizer per variant (every learning rate is 0): neither re-uploads its step table because the other ran
    opts = {w: optim.AdamW([p for p in ts.model.parameters() if p.requires_grad], lr=0.0, weight_decay=0.0) for w in (None, k)}
    kw = dict(max_grad_norm=0.1)

    def span(window):
        stcat_amd.set_canonical_window(window)
        ts.window(opts[window], k, **kw)

    variants = {"D": None, "E": k}
    for _ in range(3):                      # eager, recorded, replayed — under either plan signature
        for w in variants.values():
            span(w)
    torch.cuda.synchronize()
    elems = sum(t.numel() for t in opts[None]._acc.values())
    levels = sum(t.numel() for lv in opts[k]._levels.values() for t in lv)
    print(f"canonical window: {a.config}, bf16x6p, train mode, deterministic mode, plans on, pipelined prefix, one rank, "
          f"window(k={k}) + 1 optimizer step per span; (D) {4 * elems / 1e6:.0f} MB of accumulators, (E) {4 * levels / 1e6:.0f} MB "
          f"of level buffers; {a.reps} alternating repetitions after {a.warmup} warm-up; {torch.cuda.get_device_name(0)}")

    def counters():
        return {key: plans.STATS.get(key, 0) for key in ("eager", "recorded", "refused")}

    times = {name: [] for name in variants}
    host = {name: [] for name in variants}
    moved_on = {name: {} for name in variants}
    for rep in range(a.warmup + a.reps):
        for name, w in variants.items():                             # alternating: D, E, D, E, ...
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            c0, t0 = counters(), time.perf_counter()
            e0.record()
            span(w)
            e1.record()
            t1 = time.perf_counter()
            torch.cuda.synchronize()
            if rep >= a.warmup:
                times[name].append(e0.elapsed_time(e1))
                host[name].append((t1 - t0) * 1e3)
                for key, v in counters().items():
                    moved_on[name][key] = moved_on[name].get(key, 0) + v - c0[key]
    stcat_amd.set_canonical_window(None)
    stats = {}
    for name, v in times.items():
        med, lo, hi = statistics.median(v), min(v), max(v)
        stats[name] = (med, lo, hi)
        print(f"({name}) median {med:9.3f} ms per span  (min {lo:.3f}, max {hi:.3f}, spread {hi - lo:.3f})  "
              f"{med / k:8.3f} ms per clip;  host done after {statistics.median(host[name]):.1f} ms;  over the timed spans: "
              + ", ".join(f"{key} {v}" for key, v in moved_on[name].items()))
    gap = stats["E"][0] - stats["D"][0]
    spread = max(stats["D"][2] - stats["D"][1], stats["E"][2] - stats["E"][1])
    print(f"(E) - (D) = {gap:+.3f} ms per span = {gap / k:+.3f} ms per micro-step ({stats['E'][0] / stats['D'][0]:.4f}x); "
          f"larger min-max spread {spread:.3f} ms per span")
    print(f"the difference exceeds the spread: {'yes' if abs(gap) > spread else 'no'}")
    ts.close()
    L.set_deterministic(False)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--config", default="C3")
    ap.add_argument("--k", type=int, default=4)
    ap.add_argument("--canonical", action="store_true", help="time the canonical window against the plain deterministic one")
    a = ap.parse_args()
    assert a.reps >= 1 and a.k >= 2 and torch.cuda.is_available(), "needs the GPU"
    if a.canonical:
        return canonical_leg(a)
    L.load()
    L.set_mma_mode("bf16x6p")
    dev = torch.device("cuda:0")
    T, res, _ = synth.CONFIGS[a.config]
    clips = [(synth.synth_frames(T, res, seed=3000 + 500 * j), torch.zeros(T, res, res, dtype=torch.bool)) for j in range(2)]
    plans.enable(True)
    ts = TrainStep(dev, a.config, train=True, clips=clips, pipeline_prefix=True)
    opt = optim.AdamW([p for p in ts.model.parameters() if p.requires_grad], lr=0.0, weight_decay=0.0)
    names = {p: n for n, p in ts.model.named_parameters()}
    kw = dict(max_grad_norm=0.1)
    k = a.k

    def span_a():
        for _ in range(k):
            ts.step()
        opt.step(**kw)

    def span_b():
        ts.window(opt, k, **kw)

    def span_c():
        ts.reducer.zero_grad()
        for _ in range(k):
            ts.compute()
        ts.reducer.finish()
        opt.step(**kw)

    for _ in range(6):                      # eager, recorded, and the prefix plans of both resident buffers
        ts.step()
    span_b()                                # accumulators and both optimizer tables exist from here on
    torch.cuda.synchronize()
    elems = sum(acc.numel() for acc in opt._acc.values())
    print(f"gradient accumulation: {a.config}, bf16x6p, train mode, plans on, pipelined prefix, spans of {k} clips + 1 optimizer "
          f"step; {elems / 1e6:.1f} M accumulated elements ({4 * elems / 1e6:.0f} MB of accumulators); "
          f"{a.reps} alternating repetitions after {a.warmup} warm-up; {torch.cuda.get_device_name(0)}")

    # ---- does (C) arrive at (B)'s gradients?  one seed, the same clips, the same (unchanged) weights
    ts.clip_index = 0
    ops.manual_seed(SEED)
    span_b()
    want = {names[p]: acc.clone() for p, acc in opt._acc.items()}
    variants = {"A": span_a, "B": span_b}
    plans.enable(False)
    try:
        ts.clip_index = 0
        ops.manual_seed(SEED)
        ts.reducer.zero_grad()
        for _ in range(k):
            ts.compute()
        ts.reducer.finish()
        torch.cuda.synchronize()
        worst, worst_n = 0.0, ""
        for n, g in ts.gradients().items():
            w = want[n].double()
            err = float(((g.double() / k) - w).norm() / (w.norm() + 2e-6 * w.numel() ** 0.5 / 1.5e-2))
            if err > worst:
                worst, worst_n = err, n
        if worst <= 1.5e-2:                 # (the train-mode run-to-run bar of tests/test_plans.py)
            variants["C"] = span_c
            print(f"(C) plans off, gradients kept in p.grad: sum / {k} equals (B)'s accumulators, worst tensor rel-L2 {worst:.2e}")
        else:
            print(f"(C) left out: plans off with gradients kept in p.grad does NOT arrive at (B)'s gradients — worst tensor "
                  f"{worst_n}: rel-L2 {worst:.2e} of (B)'s mean")
    except (RuntimeError, ValueError) as e:
        print(f"(C) left out: plans off with gradients kept in p.grad raised {type(e).__name__}: {str(e)[:200]}")
    finally:
        plans.enable(True)
    opt.zero_grad()

    def counters():
        c = {key: plans.STATS.get(key, 0) for key in ("eager", "recorded", "refused")}
        c["tables rebuilt"] = sum(t.rebuilds for t in (opt._table, opt._acc_table, opt._win_table) if t is not None)
        return c

    times = {name: [] for name in variants}
    host = {name: [] for name in variants}
    moved_on = {name: {} for name in variants}      # what must not happen in a timed span: eager nodes, rebuilt tables
    for rep in range(a.warmup + a.reps):
        for name, fn in variants.items():                            # alternating: A, B, (C), A, B, ...
            plans.enable(name != "C")
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            c0, t0 = counters(), time.perf_counter()
            e0.record()
            fn()
            e1.record()
            t1 = time.perf_counter()
            torch.cuda.synchronize()
            if rep >= a.warmup:
                times[name].append(e0.elapsed_time(e1))
                host[name].append((t1 - t0) * 1e3)
                for key, v in counters().items():
                    moved_on[name][key] = moved_on[name].get(key, 0) + v - c0[key]
    plans.enable(True)
    stats = {}
    for name, v in times.items():
        med, lo, hi = statistics.median(v), min(v), max(v)
        stats[name] = (med, lo, hi)
        print(f"({name}) median {med:9.3f} ms per span  (min {lo:.3f}, max {hi:.3f}, spread {hi - lo:.3f})  "
              f"{med / k:8.3f} ms per clip;  host done after {statistics.median(host[name]):.1f} ms;  over the timed spans: "
              + ", ".join(f"{key} {v}" for key, v in moved_on[name].items()))
    gap = stats["B"][0] - stats["A"][0]
    spread = max(stats["A"][2] - stats["A"][1], stats["B"][2] - stats["B"][1])
    moved = elems * (8 + 12 * (k - 1))
    print(f"(B) - (A) = {gap:.3f} ms per span = {gap / k:.3f} ms per micro-step (larger min-max spread {spread:.3f} ms per span); "
          f"the folds move {moved / 1e9:.2f} GB per span" +
          (f": {moved / gap / 1e9:.2f} TB/s if they alone made the difference" if gap > 0 else ""))

    # ---- the fold on its own: a non-first fold (12 B per element), device events around the one launch
    ts.step()
    fold, fold_host = [], []
    for rep in range(a.warmup + a.reps):
        opt.accumulate()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        e0.record()
        opt.accumulate()
        e1.record()
        t1 = time.perf_counter()
        torch.cuda.synchronize()
        opt.discard_accumulated()
        if rep >= a.warmup:
            fold.append(e0.elapsed_time(e1))
            fold_host.append((t1 - t0) * 1e3)
    med = statistics.median(fold)
    print(f"one fold alone (acc += g over {elems / 1e6:.1f} M elements): median {med:.3f} ms (min {min(fold):.3f}, max {max(fold):.3f})  "
          f"{12 * elems / med / 1e9:.2f} TB/s;  accumulate() holds the host for {statistics.median(fold_host):.3f} ms")
    if "C" in stats:
        gap_c = stats["C"][0] - stats["B"][0]
        spread_c = max(stats["C"][2] - stats["C"][1], stats["B"][2] - stats["B"][1])
        print(f"(C) - (B) = {gap_c:.3f} ms per span ({stats['C'][0] / stats['B'][0]:.2f}x), larger min-max spread {spread_c:.3f} ms")
        print(f"(B) faster than (C) by more than the spread: {'yes' if gap_c > spread_c else 'no'}")
    ts.close()


if __name__ == "__main__":
    main()
