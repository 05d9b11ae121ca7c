#!/usr/bin/env python3
"""Forward + backward of the native text encoder node (replayed from its launch plan, mode bf16x6p, train mode) against
the same weights run as plain PyTorch modules on the same device — transformers.RobertaModel + the resizer when
transformers is importable, otherwise the fp32 plain-torch restatement of tests/test_text_encoder.py.

    python tools/bench_text.py [--reps 20] [--warmup 4] [--lengths 10,26,40] [--layers 12]

One process, alternating repetitions, a synchronise per repetition; prints per path the median wall-clock ms per step
(host launch time included: both paths are launch-bound) with the min-max spread.  Verdict: the native node counts as
faster only when the gap of the medians exceeds the larger of the two spreads."""
import argparse
import os
import statistics
import sys
import time

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from stcat_amd import _lib as L, ops, plans, synth  # noqa: E402
from stcat_amd.text import TextConfig, TextEncoder  # noqa: E402


def torch_path(native, cfg, dev):
    """-> (label, step(ids) running forward + backward in train mode with torch's own dropout)"""
    sd = {k: v.detach().clone() for k, v in native.state_dict().items()}
    try:
        from transformers import RobertaConfig, RobertaModel
    except ImportError:
        from tests.test_text_encoder import ref_text
        leaves = {k: v.requires_grad_(True) for k, v in sd.items()}

        def step(ids):
            for v in leaves.values():
                v.grad = None
            mem, cls = ref_text(leaves, ids[0], cfg.layers)
            (F.dropout(mem, 0.1).sum() + F.dropout(cls, 0.1).sum()).backward()
        return "plain-torch restatement (fp32, no dropout inside)", step
    body = RobertaModel(RobertaConfig(vocab_size=cfg.vocab, num_hidden_layers=cfg.layers, max_position_embeddings=cfg.max_pos,
                                      type_vocab_size=1, layer_norm_eps=cfg.eps, pad_token_id=1))
    body.load_state_dict({k[5:]: v for k, v in sd.items() if k.startswith("body.")}, strict=True)
    fc, ln = torch.nn.Linear(768, 256), torch.nn.LayerNorm(256, eps=1e-12)
    fc.load_state_dict({"weight": sd["resizer.fc.weight"], "bias": sd["resizer.fc.bias"]})
    ln.load_state_dict({"weight": sd["resizer.layer_norm.weight"], "bias": sd["resizer.layer_norm.bias"]})
    mods = torch.nn.ModuleList([body, fc, ln]).to(dev).train()

    def step(ids):
        for p in mods.parameters():
            p.grad = None
        out = body(input_ids=ids, attention_mask=torch.ones_like(ids))
        mem = F.dropout(ln(fc(out.last_hidden_state.transpose(0, 1))), 0.1)
        cls = F.dropout(ln(fc(out.pooler_output)), 0.1)
        (mem.sum() + cls.sum()).backward()
    return "transformers.RobertaModel + resizer (eager PyTorch, fp32)", step


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--lengths", default="10,26,40")
    ap.add_argument("--layers", type=int, default=12)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    L.load()
    L.set_mma_mode("bf16x6p")
    dev = torch.device("cuda:0")
    cfg = TextConfig(layers=a.layers)
    native = TextEncoder(cfg)
    synth.fill_module_(native, skip_prefixes=())
    native.to(dev).train()
    label, torch_step = torch_path(native, cfg, dev)
    plans.enable(True)
    ops.manual_seed(1)
    print(f"text encoder: {a.layers} layers, vocab {cfg.vocab}, mode bf16x6p, train mode, {a.reps} alternating repetitions after "
          f"{a.warmup} warm-up; {torch.cuda.get_device_name(0)}")
    print(f"torch path: {label}")

    def native_step(ids):
        for p in native.parameters():
            p.grad = None
        ops.dropout_begin_step(dev)
        (_, mem, _), cls = native.forward_ids(ids, torch.ones_like(ids))
        (mem.sum() + cls.sum()).backward()

    for S in (int(s) for s in a.lengths.split(",")):
        g = torch.Generator().manual_seed(S)
        ids = torch.cat([torch.tensor([0]), torch.randint(3, cfg.vocab, (S - 2,), generator=g), torch.tensor([2])])[None]
        ids_dev = ids.to(dev)
        times = {"native": [], "torch": []}
        for rep in range(a.warmup + a.reps):
            for name, fn, arg in (("native", native_step, ids), ("torch", torch_step, ids_dev)):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn(arg)
                torch.cuda.synchronize()
                if rep >= a.warmup:
                    times[name].append((time.perf_counter() - t0) * 1e3)
        st = {}
        for name, v in times.items():
            st[name] = (statistics.median(v), min(v), max(v))
            print(f"L={S:3d} {name:6s} fwd+bwd median {st[name][0]:8.3f} ms  (min {st[name][1]:.3f}, max {st[name][2]:.3f}, "
                  f"spread {st[name][2] - st[name][1]:.3f})")
        gap = st["torch"][0] - st["native"][0]
        spread = max(st["native"][2] - st["native"][1], st["torch"][2] - st["torch"][1])
        print(f"L={S:3d} torch - native = {gap:.3f} ms ({st['torch'][0] / st['native'][0]:.2f}x), larger spread {spread:.3f} ms; "
              f"native faster by more than the spread: {'yes' if gap > spread else 'no'}")
    print("plans:", {k: v for k, v in plans.STATS.items() if k != "run_s"})


if __name__ == "__main__":
    main()
