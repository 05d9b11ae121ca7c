#!/usr/bin/env python3
"""Thin a model fixture of tests/golden/make_golden.py so that it fits the 1 MiB limit of a committed file.

    python tests/golden/make_golden.py model HR8        # the imported reference: tests/golden/model_HR8.npz, ~3 MB
    python tools/thin_model_fixture.py HR8              # rewrites it in place, < 1 MiB

`make_golden.py model` keeps up to 1024 elements of every parameter gradient (synth.sample_indices), from the fp32 and from
the fp64 run of the reference; with 626 tensors those two float arrays alone are 2.9 MB and do not compress.  This keeps at
most K of each tensor's stored elements, evenly spaced over the sample (synth.thinned_positions), and drops the
`stage/*` samples that no loader of model fixtures reads.  Everything else — outputs, spans, losses, the full-tensor norms — is copied bit for bit,
and the file keeps the layout tests.test_model_parity.Ref.fixture reads; `meta/grad_sample_k` = K marks it as thinned.  A
test compares the same elements of its own gradients: synth.sample_indices(name, numel)[synth.thinned_positions(n, K)]."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from stcat_amd.synth import thinned_positions  # noqa: E402

LIMIT = 1 << 20


def thin(g, k: int) -> dict:
    out = {key: g[key] for key in g.files if not key.startswith("stage/") and key != "meta/grad_sample_k"}
    offs = g["grad/offsets"]
    keep = [offs[i] + thinned_positions(int(offs[i + 1] - offs[i]), k) for i in range(len(offs) - 1)]
    out["grad/offsets"] = np.concatenate([[0], np.cumsum([len(p) for p in keep])]).astype(np.int64)
    sel = np.concatenate(keep)
    out["grad/sample32"], out["grad/sample64"] = g["grad/sample32"][sel], g["grad/sample64"][sel]
    out["meta/grad_sample_k"] = np.asarray(k, dtype=np.int64)
    return out


def main():
    name = sys.argv[1]
    k = int(sys.argv[2]) if len(sys.argv) > 2 else 224
    path = os.path.join(ROOT, "tests", "golden", f"model_{name}.npz")
    g = np.load(path)
    assert "meta/grad_sample_k" not in g.files, f"{path} is thinned already: regenerate it with make_golden.py first"
    out = thin(g, k)
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    print(f"{path}: {len(out['grad/names'])} gradient tensors, <= {k} elements each, {size} bytes")
    assert size <= LIMIT, f"{size} bytes: above the limit of a committed file, choose a smaller K"


if __name__ == "__main__":
    main()
