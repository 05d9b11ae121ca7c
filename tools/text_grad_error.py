#!/usr/bin/env python3
"""Per-tensor gradient error of the native text encoder against the fixtures' fp64 gradients (tests/golden/text_*.npz):
relative L2 with the absolute floor of tests/test_model_parity.py, eval mode, for every mma mode asked for.

    python tools/text_grad_error.py [--emu] [--modes bf16x3p,bf16x6p,f32] [--out profiles/text_encoder_grad_error.json]

The split-bf16 modes are measured on the grouped launches the replayed node takes.  Rows are MERGED into the output file
under the backend's name ("emu" = the host emulator build of the same kernels,
"hip" = the MI355X), so one file holds both measurements.  tests/test_text_encoder.py derives the bf16x3p cap from it:
1.5 x the worst tensor, never above 2e-2."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from stcat_amd import _lib as L  # noqa: E402
from tests import backends  # noqa: E402
from tests import test_text_encoder as T  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--emu", action="store_true")
    ap.add_argument("--modes", default="bf16x3p,bf16x6p,f32")
    ap.add_argument("--cases", default="text_T2,text_T2_L40,text_R12")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "text_encoder_grad_error.json"))
    a = ap.parse_args()
    dev = backends.use_emu() if a.emu else backends.use_hip()
    backend = "emu" if a.emu else "hip"
    rows = []
    for mode in a.modes.split(","):
        for case in a.cases.split(","):
            L.set_mma_mode(mode)
            m = T.build(case, dev)
            _, _, grads = T.run_module_grouped(m, case, dev)     # the launches the replayed node takes
            for name, e_hip, e_ref in T.grad_rows(grads, case):
                rows.append({"backend": backend, "mode": mode, "case": case, "tensor": name, "e_hip": float("%.4e" % e_hip),
                             "e_ref32": float("%.4e" % e_ref)})
            worst = max((r for r in rows if r["mode"] == mode and r["case"] == case), key=lambda r: r["e_hip"])
            print(f"{backend} {mode:8s} {case:12s} worst {worst['e_hip']:.3e} ({worst['tensor']}; fp32 reference {worst['e_ref32']:.3e})")
    doc = {"what": "rel-L2 error of every text-encoder gradient against the fp64 fixture gradients (floor 2e-6 sqrt(n) / 1e-3 "
                   "in the norm), eval mode, grouped launches; cases[c].e_ref32 = the fp32 reference's own error; "
                   "rows[i].e_hip[k] belongs to cases[rows[i].case].tensors[k]", "cases": {}, "rows": []}
    if os.path.exists(a.out):
        with open(a.out) as fh:
            doc = json.load(fh)
    redo = {(m, c) for m in a.modes.split(",") for c in a.cases.split(",")}
    doc["rows"] = [r for r in doc["rows"] if r["backend"] != backend or (r["mode"], r["case"]) not in redo]
    for mode in a.modes.split(","):
        for case in a.cases.split(","):
            mine = [r for r in rows if r["mode"] == mode and r["case"] == case]
            doc["cases"][case] = {"tensors": [r["tensor"] for r in mine], "e_ref32": [r["e_ref32"] for r in mine]}
            doc["rows"].append({"backend": backend, "mode": mode, "case": case, "e_hip": [r["e_hip"] for r in mine]})
    with open(a.out, "w") as fh:      # one (backend, mode, case) per line
        fh.write('{"what": %s,\n "cases": {\n' % json.dumps(doc["what"]))
        fh.write(",\n".join("  %s: %s" % (json.dumps(c), json.dumps(t)) for c, t in doc["cases"].items()))
        fh.write('\n },\n "rows": [\n' + ",\n".join("  " + json.dumps(r) for r in doc["rows"]) + "\n ]}\n")


if __name__ == "__main__":
    main()
