"""The 2D-map head (models/map2d_head.py) on the bf16 plane pipeline (TempPredictionHead(planes=True)), the per-pixel
scale on planes, and the ordered (gather) backward of Gen2DMap that lets the head train in deterministic mode.

Fixture: tests/golden/map2d_planes.npz (make_map2d_planes_golden.py, from the imported reference): 16 x 16 map, 128
channels, two 5 x 5 convolutions — first-layer padding 4 > k / 2 and 30 % / 11 % zero-weight output pixels, as at the
reference size — for T = 10 (adaptive max-pool branch) and T = 24 (adaptive average).  Bars: those tests/test_map2d.py
applies to the tensor path (scores 1e-3 absolute, gradients 2e-4 of scale; full size 1e-3 / 2e-3 relative norms) in mode
bf16x6p, 10 x in bf16x3p (the ratio tests/test_ops.py keeps between the two modes)."""
import contextlib
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import stcat_amd
from stcat_amd import _lib as L
from stcat_amd import ops, plans, synth
from stcat_amd.map2d import TempPredictionHead
from tests.backends import both, close, use_hip
from tests.golden.make_golden import MAP2D_CFG

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden", "map2d_planes.npz")
GOLD_TENSOR = os.path.join(HERE, "golden", "map2d.npz")
CFG = dict(MAX_MAP_SIZE=16, POOLING_COUNTS=[3, 2, 2], HIDDEN=128, KERNAL_SIZE=5, CONV_LAYERS=2)
PREFIX = "map2d_planes_head."
MODES = (("bf16x6p", 1.0), ("bf16x3p", 10.0))
_gold = {}


def gold(path=GOLD):
    if path not in _gold:
        with np.load(path) as z:
            _gold[path] = {k: z[k] for k in z.files}
    return _gold[path]


@contextlib.contextmanager
def mma(mode):
    old = L.get_mma_mode()
    L.set_mma_mode(mode)
    try:
        yield
    finally:
        L.set_mma_mode(old)


@contextlib.contextmanager
def deterministic():
    old = L.is_deterministic()
    stcat_amd.set_deterministic(True)
    try:
        yield
    finally:
        stcat_amd.set_deterministic(old)


def _fill(head, prefix):
    with torch.no_grad():
        for k, v in head.state_dict().items():
            v.copy_(torch.from_numpy(synth.synth_value(prefix + k, tuple(v.shape)).copy()))
    return head


def _small_head(dev, **kw):
    c = CFG
    head = TempPredictionHead(c["HIDDEN"], c["MAX_MAP_SIZE"], c["POOLING_COUNTS"], c["KERNAL_SIZE"], c["CONV_LAYERS"], **kw)
    return _fill(head, PREFIX).to(dev)


def _train_grads(dev, head, x, G):
    """train-mode scores and the gradients of sum(scores * G): (scores, dx, {name: grad})"""
    head.train()
    xr = torch.from_numpy(x).to(dev).requires_grad_(True)
    sc = head(xr)
    (sc * torch.from_numpy(G).to(dev)).sum().backward()
    return sc.detach(), xr.grad, {k: p.grad for k, p in head.named_parameters()}


def _check_grads(g, tag, dx, grads, tol, what):
    close(dx, torch.from_numpy(g[f"{tag}/dx"]), tol, f"{what} {tag} dx")
    for k, gr in grads.items():
        if f"{tag}/grad/{k}" in g:
            close(gr, torch.from_numpy(g[f"{tag}/grad/{k}"]), tol, f"{what} {tag} grad {k}")
        else:      # a large gradient: 4096 stored positions + its fp64 norm (the existing full-size bar: 2e-3 relative)
            pos = torch.from_numpy(g[f"{tag}/gradpos/{k}"])
            close(gr.detach().cpu().reshape(-1)[pos], torch.from_numpy(g[f"{tag}/gradval/{k}"]), tol, f"{what} {tag} grad {k} samples")
            ref = float(g[f"{tag}/gradnorm/{k}"])
            got = gr.double().norm().item()
            assert abs(got - ref) <= 2e-3 * max(ref, 1e-6), (what, tag, k, got, ref)


# 1 -------------------------------------------------------------------------------------------------------------------
@both
def _pl_rowscale(dev, big):
    """rows = 70 (2 x 7 x 5), C = 64, period = 35, weights with zeros: exact on three planes, the split round trip on two"""
    gen = torch.Generator().manual_seed(7)
    x = torch.randn(2, 7, 5, 64, generator=gen).to(dev)
    w = torch.rand(35, generator=gen)
    w[::4] = 0.0
    w = w.to(dev)
    # (f16x3p: the kernel is plane-format aware like its neighbours although the head excludes the mode; two fp16 planes
    # carry 22 significand bits: tests/test_ops.py's round-trip bar for that format, 2e-6)
    for mode, rt in (("bf16x6p", 0.0), ("bf16x3p", 2e-5), ("f16x3p", 2e-6)):
        with mma(mode):
            p = ops.pl_split(x)
            before = ops.pl_join(p)
            assert ops.pl_rowscale(p, w) is p                 # in place
            want = before * w.view(1, 7, 5, 1)
            got = ops.pl_join(p)
            if mode == "bf16x6p":
                assert torch.equal(got, want), (got - want).abs().max().item()
            else:
                close(got, want, rt, f"pl_rowscale {mode}")
            assert float(got.view(2, 35, 64)[:, ::4].abs().max()) == 0.0


# 2 -------------------------------------------------------------------------------------------------------------------
@both
def _planes_head_fixture(dev, big):
    g = gold()
    for mode, mul in MODES:
        with mma(mode):
            head = _small_head(dev, planes=True)
            assert list(head.state_dict().keys()) == list(g["keys"])          # the reference's parameter names
            close(head.weight0, torch.from_numpy(g["weight0"]), 1e-6, "mask weight 0")
            close(head.weight1, torch.from_numpy(g["weight1"]), 1e-6, "mask weight 1")
            for T in (10, 24):
                tag = f"T{T}"
                head.eval()
                with torch.no_grad():
                    sc = head(torch.from_numpy(g[f"{tag}/x"]).to(dev))
                close(sc, torch.from_numpy(g[f"{tag}/scores"]), 1e-3 * mul, f"{mode} {tag} eval scores", absolute=True)
                for p in head.parameters():
                    p.grad = None
                sc, dx, grads = _train_grads(dev, head, g[f"{tag}/x"], g[f"{tag}/G"])
                close(sc, torch.from_numpy(g[f"{tag}/train_scores"]), 1e-3 * mul, f"{mode} {tag} train scores", absolute=True)
                _check_grads(g, tag, dx, grads, 2e-4 * mul, mode)


# 3 -------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_gpu_planes_head_full_size():
    """the reference-sized head (128 x 128 map, 256 channels, four 9 x 9 convolutions) on the plane path: GPU only (no
    emulator variant is registered: at this size it would take hours)"""
    dev = use_hip()
    g = gold(GOLD_TENSOR)
    with mma("bf16x6p"):
        full = _fill(TempPredictionHead(planes=True), "map2d_full_head.").to(dev).eval()
        with torch.no_grad():
            sc = full(torch.from_numpy(g["map2d/full/x"]).to(dev))
        close(sc, torch.from_numpy(g["map2d/full/scores"]), 1e-3, "full-size eval scores", absolute=True)
        sc, dx, grads = _train_grads(dev, full, g["map2d/full/x"], g["map2d/full/G"])
        close(sc, torch.from_numpy(g["map2d/full/train_scores"]), 1e-3, "full-size train scores", absolute=True)
        close(dx, torch.from_numpy(g["map2d/full/dx"]), 1e-3, "full-size dx")
        for k, gr in grads.items():
            ref = float(g[f"map2d/full/gradnorm/{k}"])
            got = gr.double().norm().item()
            assert abs(got - ref) <= 2e-3 * max(ref, 1e-6), (k, got, ref)


# 4 -------------------------------------------------------------------------------------------------------------------
@both
def _planes_guard_rails(dev, big):
    c = CFG
    with pytest.raises(ValueError, match="attn"):
        TempPredictionHead(256, c["MAX_MAP_SIZE"], c["POOLING_COUNTS"], temp_head="attn", planes=True)
    with pytest.raises(ValueError, match="128"):
        TempPredictionHead(64, c["MAX_MAP_SIZE"], c["POOLING_COUNTS"], c["KERNAL_SIZE"], c["CONV_LAYERS"], planes=True)
    x = torch.from_numpy(gold()["T10/x"]).to(dev)
    with mma("f32"):
        head = _small_head(dev, planes=True).eval()
        with pytest.raises(ValueError, match="f32"), torch.no_grad():
            head(x)
    # planes=False is the head constructed without the argument: equal outputs, bit for bit (eval and train-mode scores; the
    # default backward adds with float atomics, so its gradients are not compared for equal bits)
    m = MAP2D_CFG
    gt = gold(GOLD_TENSOR)
    outs = []
    for kw in ({}, {"planes": False}):
        head = TempPredictionHead(m["HIDDEN"], m["MAX_MAP_SIZE"], m["POOLING_COUNTS"], m["KERNAL_SIZE"], m["CONV_LAYERS"], **kw)
        _fill(head, "map2d_head.").to(dev).eval()
        with torch.no_grad():
            ev = head(torch.from_numpy(gt["map2d/head/x"]).to(dev))
        head.train()
        outs.append([ev, head(torch.from_numpy(gt["map2d/head/x"]).to(dev)).detach()])
    assert all(torch.equal(a, b) for a, b in zip(*outs))


# 5 -------------------------------------------------------------------------------------------------------------------
@both
def _planes_plan_hygiene(dev, big):
    """two forwards of a planes=True head: the weight-plane table is built once (same key, same table, same staging
    buffers) and plans.invalidate() is never called — the main model's launch plans survive the head"""
    x = torch.from_numpy(gold()["T10/x"]).to(dev)
    calls = []
    saved = plans.invalidate
    plans.invalidate = lambda *a, **k: (calls.append(1), saved(*a, **k))[1]
    try:
        with mma("bf16x6p"):
            head = _small_head(dev, planes=True).eval()
            with torch.no_grad():
                a = head(x)
                cache = head._wplanes
                key, table, staging = cache.key, cache.table.data_ptr(), [s.data_ptr() for s in head._w_ohwi]
                state = cache.state
                b = head(x)
            assert cache.key == key and cache.table.data_ptr() == table
            assert [s.data_ptr() for s in head._w_ohwi] == staging
            assert cache.state == state                       # unchanged weights: not even a second plane launch
            assert torch.equal(a, b) and not calls
            with torch.no_grad():
                head.encoder.convs[0].weight.mul_(0.5)        # a changed weight is picked up (without a rebuild)
                c = head(x)
            assert cache.key == key and cache.state != state and not calls
            assert not torch.equal(a, c)
            # a launch-plan recording cannot hold the staging copy: the head refuses instead of replaying stale weights
            rec, L.RECORDER = L.RECORDER, SimpleNamespace(add_call=lambda *a: None)
            try:
                with pytest.raises(L.StcatHipError, match="launch plan"), torch.no_grad():
                    head(x)
            finally:
                L.RECORDER = rec
    finally:
        plans.invalidate = saved


# 6 -------------------------------------------------------------------------------------------------------------------
def _gather_vs_scatter(dev):
    """the gather entries called directly (mode off) against the scatter entries: b = 1, N = 4, D = 4"""
    b, N, D = 1, 4, 4
    gen = torch.Generator().manual_seed(3)
    cells = [(i, j) for i in range(N) for j in range(i, N)]
    ci = torch.tensor([c[0] for c in cells], dtype=torch.int32).to(dev)
    cj = torch.tensor([c[1] for c in cells], dtype=torch.int32).to(dev)
    pooled = torch.randn(b, N, D, generator=gen)
    pooled[0, 2] = pooled[0, 1]                               # ties: the first maximum takes the gradient
    pooled = pooled.to(dev)
    dmap = torch.randn(b, N, N, D, generator=gen).to(dev)
    st = L.stream_of(dmap)
    want = torch.zeros(b, N, D, device=dev)
    L.call("stcat_map2d_cells_bwd", pooled.data_ptr(), ci.data_ptr(), cj.data_ptr(), len(cells), dmap.data_ptr(),
           want.data_ptr(), b, N, D, st)
    got = torch.full((b, N, D), float("nan"), device=dev)     # (not zeroed by the caller)
    arg = torch.empty(b, len(cells), D, dtype=torch.int32, device=dev)
    L.call("stcat_map2d_cells_bwd_gather", pooled.data_ptr(), ci.data_ptr(), cj.data_ptr(), len(cells), dmap.data_ptr(),
           arg.data_ptr(), got.data_ptr(), b, N, D, st)
    close(got, want, 1e-6, "cells_bwd gather vs scatter")
    for T in (3, 4, 6, 9):                                     # T <= N: first maximum of the window; T > N: average
        x = torch.randn(b, T, D, generator=gen)
        if T > 1:
            x[0, 1] = x[0, 0]
        x = x.to(dev)
        dpooled = torch.randn(b, N, D, generator=gen).to(dev)
        want = torch.zeros(b, T, D, device=dev)
        L.call("stcat_map2d_pool_bwd", x.data_ptr(), dpooled.data_ptr(), want.data_ptr(), b, T, N, D, st)
        got = torch.full((b, T, D), float("nan"), device=dev)
        L.call("stcat_map2d_pool_bwd_gather", x.data_ptr(), dpooled.data_ptr(), got.data_ptr(), b, T, N, D, st)
        close(got, want, 1e-6, f"pool_bwd gather vs scatter T={T}")


@both
def _head_trains_in_deterministic_mode(dev, big):
    assert not L.is_deterministic()
    _gather_vs_scatter(dev)
    gt, g = gold(GOLD_TENSOR), gold()
    m = MAP2D_CFG
    with deterministic():
        # the tensor path at the existing small configuration (HIDDEN = 64), the existing test's bars
        runs = []
        for _ in range(2):
            head = TempPredictionHead(m["HIDDEN"], m["MAX_MAP_SIZE"], m["POOLING_COUNTS"], m["KERNAL_SIZE"], m["CONV_LAYERS"])
            _fill(head, "map2d_head.").to(dev)
            runs.append(_train_grads(dev, head, gt["map2d/head/x"], gt["map2d/head/G"]))
        (sa, dxa, ga), (sb, dxb, gb) = runs
        assert torch.equal(sa, sb) and torch.equal(dxa, dxb) and all(torch.equal(ga[k], gb[k]) for k in ga)
        close(sa, torch.from_numpy(gt["map2d/head/train_scores"]), 1e-3, "det tensor train scores", absolute=True)
        close(dxa, torch.from_numpy(gt["map2d/head/dx"]), 2e-4, "det tensor dx")
        for k in ga:
            close(ga[k], torch.from_numpy(gt[f"map2d/head/grad/{k}"]), 2e-4, f"det tensor grad {k}")
        # the plane path on the new fixture, the bars of test 2
        with mma("bf16x6p"):
            for T in (10, 24):
                tag = f"T{T}"
                runs = [_train_grads(dev, _small_head(dev, planes=True), g[f"{tag}/x"], g[f"{tag}/G"]) for _ in range(2)]
                (sa, dxa, ga), (sb, dxb, gb) = runs
                assert torch.equal(sa, sb) and torch.equal(dxa, dxb) and all(torch.equal(ga[k], gb[k]) for k in ga), tag
                close(sa, torch.from_numpy(g[f"{tag}/train_scores"]), 1e-3, f"det planes {tag} train scores", absolute=True)
                _check_grads(g, tag, dxa, ga, 2e-4, "det planes")
    assert not L.is_deterministic()
