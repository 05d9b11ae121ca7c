#!/usr/bin/env python3
"""Golden vectors for the plane path of the 2D-map head (tests/test_map2d_planes.py), from the imported reference
(models/map2d_head.py) exactly as make_golden.py::map2d_vectors does it; runs only where the reference exists.

    python tests/golden/make_map2d_planes_golden.py      # writes tests/golden/map2d_planes.npz

The configuration is the smallest that keeps both features of the reference-sized head: a first-layer padding larger
than k / 2 (pad0 = (k - 1) n / 2 = 4 > 2) and output pixels whose mask-normalisation weight is exactly zero; HIDDEN = 128
is the plane weight gradient's smallest width.  Inputs [2, 1, T, 128] for T = 10 (T <= N: the adaptive max-pool branch)
and T = 24 (T > N: adaptive average).  Stored per T: eval scores, train scores, the upstream gradient G of sum(scores * G),
dx, and per parameter the full gradient (<= 65536 elements) or its fp64 norm + 4096 seeded sample positions and values.
"""
from __future__ import annotations

import importlib.util
import os
import sys
from types import SimpleNamespace as NS

import numpy as np
import torch

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), "..", ".."))
sys.path.insert(0, REPO)

from stcat_amd import synth  # noqa: E402
from tests.golden.make_golden import MAP2D_CFG, REF  # noqa: E402

CFG = dict(MAP2D_CFG, MAX_MAP_SIZE=16, POOLING_COUNTS=[3, 2, 2], HIDDEN=128, KERNAL_SIZE=5, CONV_LAYERS=2, TEMP_HEAD="conv")
PREFIX = "map2d_planes_head."
TS = (10, 24)
FULL_GRAD_MAX = 65536
N_SAMPLES = 4096


def sample_positions(key: str, numel: int) -> np.ndarray:
    """the seeded flat positions at which a large gradient is stored (the test recomputes nothing: they are in the file)"""
    seed = int.from_bytes(key.encode()[-4:], "little") ^ 0x2D3A9
    return np.sort(np.random.RandomState(seed).choice(numel, N_SAMPLES, replace=False)).astype(np.int64)


def vectors():
    orig_to = torch.Tensor.to

    def to_cpu(self, *a, **k):       # the reference hard-codes .to("cuda") (map2d_head.py:33)
        return orig_to(self, *tuple("cpu" if (isinstance(x, str) and x == "cuda") else x for x in a), **k)
    torch.Tensor.to = to_cpu
    try:
        spec = importlib.util.spec_from_file_location("ref_map2d_head", os.path.join(REF, "models", "map2d_head.py"))
        m = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(m)
        head = m.TempPredictionHead(NS(MODEL=NS(TEMPFORMER=NS(**CFG))))
        with torch.no_grad():
            for k, v in head.state_dict().items():
                v.copy_(torch.from_numpy(synth.synth_value(PREFIX + k, tuple(v.shape)).copy()))
        g = {"keys": np.array(list(head.state_dict().keys())), "mask": head.map_maker.mask2d.numpy().copy()}
        for i, w in enumerate(head.encoder.weights):
            g[f"weight{i}"] = w.numpy().copy()
        for T in TS:
            tag = f"T{T}"
            x = torch.from_numpy(synth.hash_normal(f"op/map2d_planes/x{T}", 2 * T * CFG["HIDDEN"]).reshape(2, 1, T, CFG["HIDDEN"]))
            g[f"{tag}/x"] = x.numpy()
            head.eval()
            with torch.no_grad():
                g[f"{tag}/scores"] = head(x.clone()).numpy().copy()
            head.train()
            xr = x.clone().requires_grad_(True)
            for p in head.parameters():
                p.grad = None
            sc = head(xr)
            G = torch.from_numpy(synth.hash_normal(f"op/map2d_planes/{tag}/G", sc.numel()).reshape(tuple(sc.shape)))
            g[f"{tag}/train_scores"] = sc.detach().numpy().copy()
            g[f"{tag}/G"] = G.numpy()
            (sc * G).sum().backward()
            g[f"{tag}/dx"] = xr.grad.numpy().copy()
            for k, prm in head.named_parameters():
                gr = prm.grad.detach()
                if gr.numel() <= FULL_GRAD_MAX:
                    g[f"{tag}/grad/{k}"] = gr.numpy().copy()
                else:
                    pos = sample_positions(f"{tag}/{k}", gr.numel())
                    g[f"{tag}/gradnorm/{k}"] = np.array(float(gr.double().norm()))
                    g[f"{tag}/gradpos/{k}"] = pos
                    g[f"{tag}/gradval/{k}"] = gr.reshape(-1).numpy()[pos].copy()
    finally:
        torch.Tensor.to = orig_to
    return g


if __name__ == "__main__":
    out = os.path.join(os.path.dirname(os.path.abspath(__file__)), "map2d_planes.npz")
    np.savez_compressed(out, **vectors())
    print(f"{out} written ({os.path.getsize(out)} bytes)")
