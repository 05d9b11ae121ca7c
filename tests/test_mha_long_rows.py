"""Self-attention rows longer than 256 tokens trained on the bf16 pipe (csrc/attention_bs.h: mha_bs_bwd_dq_long_kernel /
mha_bs_bwd_dkv_long_kernel — one 32-row tile per wave, the other operand streamed through LDS in 128-row super-chunks,
probabilities rebuilt from the row log-sum-exp, no atomics and no workspace).

Routing (ops.mha_self_fwd_raw): rows above 512 tokens with gradients always take these kernels in the modes whose forward runs on
the bf16 pipe; 256 < S <= 512 keeps the fp32 long-row kernels unless ops.MHA_BS_LONG (STCAT_MHA_BS_LONG=1) is set.

Op level (`@both`: host emulator and GPU): shapes / masks / packing against the fp32 PyTorch reference at the bar of
tests/test_ops.py, dropout against the mask rebuilt from the counter stream, the C entry point called directly, the accuracy
class of the six-product form against fp64, bitwise reproducibility, and the unchanged routes.  GPU: the memory the opt-in
frees, and the 517-token clip HR8 (704 x 736 frames: 22 x 23 map + 10 text tokens + [CLS]) at model level against the
reference's fixture.

The fixture tests/golden/model_HR8.npz is what `python tests/golden/make_golden.py model HR8` writes (the imported
reference in fp32 and fp64, 2.98 MB) after `python tools/thin_model_fixture.py HR8`: a committed file may hold 1 MiB, so of the
<= 1024 sampled elements of each of the 626 gradient tensors it keeps at most 224, evenly spaced over the sample; outputs,
spans and losses are untouched.  Ref.fixture reads it as it is; `_compare_with_fixture` cuts a run's gradients to the same
elements before the unchanged `_compare` sees them, so the bars are those of every other model case, on a quarter of the sample."""
import contextlib
import os

import numpy as np
import pytest
import torch

from stcat_amd import _lib as L
from stcat_amd import ops, plans, synth
from tests.backends import both, close, use_emu, use_hip
from tests.test_model_parity import (BENCH_MMA, GRAD_ABS_FLOOR, GRAD_CAPS_16BIT, GRAD_TOL, HARD_CAP, SMALL_NET,
                                     THROUGHPUT_MMA, Ref, _compare, _hip_case, _run_bench_step, _run_hip)
from tests.test_ops import TOL, _mha_dropout_case, _mha_ref, rnd

MODES = ("bf16x3", "bf16x6p")
SCALE = 32 ** -0.5


@contextlib.contextmanager
def _route(mode, long_rows=True, deterministic=False):
    """mma mode `mode` with every row length on the bf16-pipe kernels (MHA_BS6_MIN_ROWS = 0) and the 257..512 opt-in"""
    saved = (ops.MHA_BS_LONG, ops.MHA_BS6_MIN_ROWS)
    L.set_mma_mode(mode)
    L.set_deterministic(deterministic)
    ops.MHA_BS_LONG, ops.MHA_BS6_MIN_ROWS = long_rows, 0
    try:
        yield
    finally:
        ops.MHA_BS_LONG, ops.MHA_BS6_MIN_ROWS = saved
        L.set_deterministic(False)
        L.set_mma_mode("f32")


def _kpm(kind, B, S):
    """key-padding masks [B,S] (True = padded); every row keeps unpadded keys"""
    if kind is None:
        return None
    m = torch.zeros(B, S, dtype=torch.bool)
    if kind == "ragged":          # a padded tail of a different length per batch element
        for b in range(B):
            m[b, S - 3 - 37 * (b % 5):] = True
    elif kind == "scattered":     # every third key, shifted per batch element, and a short run at the front
        for b in range(B):
            m[b, (b % 3)::3] = True
        m[0, 1:4] = True
    elif kind == "chunk":         # keys 128..255 — one whole 128-key chunk in the middle of the row — fully padded
        m[:, 128:256] = True
        m[B - 1, S - 5:] = True
    else:
        raise ValueError(kind)
    return m


def _run_dev(dev, qk, v, go, kpm, packed):
    D = v.shape[-1]
    qkd, vd = qk.clone().to(dev).requires_grad_(True), v.clone().to(dev).requires_grad_(True)   # (fresh leaves on the CPU too)
    kd = kpm.to(dev) if kpm is not None else None
    if packed:
        o, _ = ops.mha_self_packed(qkd, vd, kd, SCALE)
    else:
        o, _ = ops.mha_self(qkd[..., :D], qkd[..., D:], vd, kd, SCALE)
    saved = [t for t in o.grad_fn.saved_tensors if t is not None]
    (o * go.to(dev)).sum().backward()
    return o.detach(), qkd.grad, vd.grad, saved


def _case(dev, B, S, H, packed, mask):
    """forward + backward against the fp32 PyTorch reference at the bar of tests/test_ops.py"""
    D = H * 32
    qk, v, go = rnd(B, S, 2 * D, seed=1), rnd(B, S, D, seed=2), rnd(B, S, D, seed=3)
    kpm = _kpm(mask, B, S)
    qkr, vr = qk.clone().requires_grad_(True), v.clone().requires_grad_(True)
    o_ref, _ = _mha_ref(qkr[..., :D], qkr[..., D:], vr, kpm, SCALE, H)
    (o_ref * go).sum().backward()
    o, dqk, dv, saved = _run_dev(dev, qk, v, go, kpm, packed)
    # the route under test: (q, k, v, o, lse[, kpm]) saved — no S x S tensor
    SP = (S + 31) // 32 * 32
    assert not any(t.dim() == 4 and t.shape[-1] == SP for t in saved), [tuple(t.shape) for t in saved]
    assert any(tuple(t.shape) == (B, H, S) for t in saved), [tuple(t.shape) for t in saved]
    tag = f"long-row mha {L.get_mma_mode()} B{B} S{S} H{H} packed{packed} mask={mask}"
    errs = (close(o, o_ref, TOL, tag + " out"), close(dqk, qkr.grad, TOL, tag + " dqk"), close(dv, vr.grad, TOL, tag + " dv"))
    assert all(torch.isfinite(t).all() for t in (o, dqk, dv)), tag
    print(f"[long rows] {tag}: max abs err out {errs[0]:.2e} dqk {errs[1]:.2e} dv {errs[2]:.2e}")


@both
def _mha_long_rows_shapes_and_masks(dev, big):
    """S = 310 (13 x 23 map), 277 (4:3 clip) and 530 (above the fp32-pipe kernels' 512): S % 32 != 0 everywhere, packed and
    unpacked q / k, ragged / scattered / whole-chunk key padding, two and three planes per operand"""
    for mode in MODES:
        with _route(mode):
            _case(dev, 2, 310, 1, packed=True, mask="ragged")
            _case(dev, 1, 310, 2, packed=False, mask="chunk")
            _case(dev, 2, 277, 1, packed=False, mask="scattered")
            _case(dev, 1, 277, 1, packed=True, mask=None)
        with _route(mode, long_rows=False):         # above 512 tokens no opt-in is needed
            _case(dev, 1, 530, 1, packed=True, mask="chunk")
            _case(dev, 2, 530, 1, packed=False, mask="ragged")
        if big:
            with _route(mode):
                _case(dev, 64, 310, 8, packed=True, mask="ragged")
                _case(dev, 64, 310, 8, packed=False, mask="chunk")
            with _route(mode, long_rows=False):
                _case(dev, 8, 1000, 8, packed=True, mask="scattered")
                _case(dev, 8, 1000, 8, packed=False, mask="chunk")


@both
def _mha_long_rows_dropout(dev, big):
    """the backward regenerates the forward's dropout decisions: counter ((b*H + h)*SP + key)*SP + query, expected mask
    rebuilt on the host from the stream (tests/test_ops.py: _mha_dropout_case)"""
    for mode in MODES:
        with _route(mode):
            _mha_dropout_case(dev, 1, 310, 1, need_w=False, pdrop=0.1)
            _mha_dropout_case(dev, 1, 530, 2, need_w=False, pdrop=0.25)
            _mha_dropout_case(dev, 1, 310, 1, need_w=False, pdrop=0.25)
            _mha_dropout_case(dev, 1, 530, 1, need_w=False, pdrop=0.1)
            if big:
                _mha_dropout_case(dev, 4, 310, 8, need_w=False, pdrop=0.25)
                _mha_dropout_case(dev, 2, 530, 8, need_w=False, pdrop=0.1)


@both
def _mha_long_rows_c_abi(dev, big):
    """stcat_mha_bs_bwd called directly at S = 310: it used to refuse every S > 256"""
    B, S, H = 2, 310, 2
    D = H * 32
    qk, v, go = rnd(B, S, 2 * D, seed=5), rnd(B, S, D, seed=6), rnd(B, S, D, seed=7)
    kpm = _kpm("ragged", B, S)
    qkr, vr = qk.clone().requires_grad_(True), v.clone().requires_grad_(True)
    o_ref, _ = _mha_ref(qkr[..., :D], qkr[..., D:], vr, kpm, SCALE, H)
    (o_ref * go).sum().backward()
    for mode in MODES:
        L.set_mma_mode(mode)
        try:
            qkd, vd, god = qk.to(dev), v.to(dev), go.to(dev)
            kp = kpm.to(torch.uint8).to(dev)
            o, lse = torch.empty(B, S, D, device=dev), torch.empty(B, H, S, device=dev)
            dqk, dv = torch.full((B, S, 2 * D), float("nan"), device=dev), torch.full((B, S, D), float("nan"), device=dev)
            q_, k_ = qkd[:, :, :D], qkd[:, :, D:]
            st = L.stream_of(vd)
            L.call("stcat_mha_bs_fwd", q_.data_ptr(), k_.data_ptr(), vd.data_ptr(), kp.data_ptr(), o.data_ptr(), lse.data_ptr(),
                   B, H, S, 2 * D, 2 * D, D, D, SCALE, 0.0, 0, 0, None, st)
            L.call("stcat_mha_bs_bwd", q_.data_ptr(), k_.data_ptr(), vd.data_ptr(), kp.data_ptr(), o.data_ptr(), god.data_ptr(),
                   lse.data_ptr(), dqk[:, :, :D].data_ptr(), dqk[:, :, D:].data_ptr(), dv.data_ptr(), B, H, S, 2 * D, 2 * D, D,
                   D, 2 * D, D, SCALE, 0.0, 0, 0, None, st)
            close(o, o_ref, TOL, f"C ABI {mode} out")
            close(dqk, qkr.grad, TOL, f"C ABI {mode} dqk")       # (every element written: no NaN of the fill is left)
            close(dv, vr.grad, TOL, f"C ABI {mode} dv")
        finally:
            L.set_mma_mode("f32")


def _rel_errs(got, exact):
    return tuple(((x.detach().double().cpu() - y.detach()).abs().max() / y.detach().abs().max()).item()
                 for x, y in zip(got, exact))


@both
def _mha_long_rows_six_product_accuracy(dev, big):
    """bf16x6p at S = 530 is fp32-class: error of out / dqk / dv against an fp64 evaluation <= max(3e-6, 3 e_ref), e_ref = the
    error of the fp32 PyTorch evaluation of the same case, and < 0.2 x the three-product form's (the bars of
    tests/test_ops.py: _mha_bs_six_products)"""
    B, S, H = 1, 530, 2
    D = H * 32
    qk, v, go = rnd(B, S, 2 * D, seed=31) * 2.0, rnd(B, S, D, seed=32), rnd(B, S, D, seed=33)

    def ref(dtype):
        a, b_ = qk.clone().to(dtype).requires_grad_(True), v.clone().to(dtype).requires_grad_(True)
        o, _ = _mha_ref(a[..., :D], a[..., D:], b_, None, SCALE, H)
        (o * go.to(dtype)).sum().backward()
        return o.detach(), a.grad, b_.grad

    exact = ref(torch.float64)
    e_ref = max(_rel_errs(ref(torch.float32), exact))
    errs = {}
    for mode in ("bf16x6p", "bf16x3"):
        with _route(mode, long_rows=False):
            errs[mode] = _rel_errs(_run_dev(dev, qk, v, go, None, True)[:3], exact)
    print(f"[long rows] S=530 error vs fp64 (out, dqk, dv): bf16x6p {errs['bf16x6p']}, bf16x3 {errs['bf16x3']}, fp32 torch {e_ref:.2e}")
    assert max(errs["bf16x6p"]) <= max(3e-6, 3 * e_ref), (errs, e_ref)
    assert max(errs["bf16x6p"]) < 0.2 * max(errs["bf16x3"]), errs


@both
def _mha_long_rows_reproducible(dev, big):
    """one writer and one summation order per element: two forward + backward runs are bit-identical, deterministic mode off
    and on, with dropout active (same seed) and a padding mask"""
    B, S, H = (8, 310, 8) if big else (1, 310, 1)
    D = H * 32
    qk, v, go = rnd(B, S, 2 * D, seed=41), rnd(B, S, D, seed=42), rnd(B, S, D, seed=43)
    kpm = _kpm("ragged", B, S).to(dev)
    for mode in MODES:
        for det in (False, True):
            with _route(mode, deterministic=det):
                runs = []
                for _ in range(2):
                    ops.manual_seed(5)
                    a, b_ = qk.clone().to(dev).requires_grad_(True), v.clone().to(dev).requires_grad_(True)
                    o, _ = ops.mha_self_packed(a, b_, kpm, SCALE, drop_p=0.1)
                    (o * go.to(dev)).sum().backward()
                    runs.append((o.detach(), a.grad, b_.grad))
                for x, y, what in zip(runs[0], runs[1], ("out", "dqk", "dv")):
                    assert torch.equal(x, y), f"{mode} deterministic={det}: {what} differs between two runs"


@both
def _mha_long_rows_routes_unchanged(dev, big):
    """S <= 256: the opt-in changes nothing (bitwise).  256 < S <= 512 without the opt-in: still the fp32 long-row kernels —
    the S x S probability stash is what the forward saves.  Above 512 tokens the fp32-pipe modes refuse by name."""
    for mode in MODES:
        for S in (207, 256):
            qk, v, go = rnd(1, S, 128, seed=51), rnd(1, S, 64, seed=52), rnd(1, S, 64, seed=53)
            kpm = _kpm("ragged", 1, S)
            with _route(mode, long_rows=False):
                off = _run_dev(dev, qk, v, go, kpm, True)
            with _route(mode, long_rows=True):
                on = _run_dev(dev, qk, v, go, kpm, True)
            for x, y in zip(off[:3], on[:3]):
                assert torch.equal(x, y), (mode, S)
        S, SP = 310, 320
        qk, v, go = rnd(1, S, 64, seed=54), rnd(1, S, 32, seed=55), rnd(1, S, 32, seed=56)
        with _route(mode, long_rows=False):
            saved = _run_dev(dev, qk, v, go, None, True)[3]
        assert any(tuple(t.shape) == (1, 1, SP, SP) for t in saved), [tuple(t.shape) for t in saved]
        with _route(mode, long_rows=True):
            saved = _run_dev(dev, qk, v, go, None, True)[3]
        assert not any(tuple(t.shape) == (1, 1, SP, SP) for t in saved), [tuple(t.shape) for t in saved]
    qk, v = rnd(1, 530, 64, seed=57).to(dev).requires_grad_(True), rnd(1, 530, 32, seed=58).to(dev)
    L.set_mma_mode("f32")
    with pytest.raises(ValueError, match=r"mma mode 'f32'.*512 tokens"):
        ops.mha_self_packed(qk, v, None, SCALE)
    with _route("bf16x6p"):
        with pytest.raises(ValueError, match=r"head-mean attention weights.*512 tokens"):
            ops.mha_self_packed(qk, v, None, SCALE, need_weights=True)


def test_plan_signature_holds_the_long_row_route():
    """a launch plan recorded on one route of the 257..512 band is never replayed on the other"""
    dev = use_emu()
    saved = ops.MHA_BS_LONG
    try:
        ops.MHA_BS_LONG = False
        a = plans._global_sig(dev)
        ops.MHA_BS_LONG = True
        b = plans._global_sig(dev)
    finally:
        ops.MHA_BS_LONG = saved
    assert a != b


# ---------------------------------------------------------------------------------------------------------------------
# memory, GPU
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_gpu_long_rows_free_the_probability_stash():
    """B = 64, H = 8, S = 310: the fp32 long-row route keeps the S x S probabilities and allocates a same-sized dS scratch
    (2 x B H SP^2 x 4 B = 2 x 210 MB); the bf16-pipe route keeps the row log-sum-exp.  0.95 = allocator rounding."""
    dev = use_hip()
    B, H, S = 64, 8, 310
    D, SP = H * 32, 320
    qk, v, go = rnd(B, S, 2 * D, seed=61).to(dev), rnd(B, S, D, seed=62).to(dev), rnd(B, S, D, seed=63).to(dev)
    peak = {}
    for flag in (False, True):
        with _route(BENCH_MMA, long_rows=flag):
            for _ in range(2):           # (first pass: one-time allocations of the library)
                a, b_ = qk.clone().requires_grad_(True), v.clone().requires_grad_(True)
                torch.cuda.synchronize()
                torch.cuda.reset_peak_memory_stats()
                base = torch.cuda.memory_allocated()
                o, _ = ops.mha_self_packed(a, b_, None, SCALE)
                (o * go).sum().backward()
                torch.cuda.synchronize()
                peak[flag] = torch.cuda.max_memory_allocated() - base
                del a, b_, o
    drop, want = peak[False] - peak[True], 2 * B * H * SP * SP * 4
    print(f"[long rows] peak of fwd + bwd at B64 H8 S310: fp32 long-row {peak[False] / 2**20:.0f} MiB, bf16 pipe "
          f"{peak[True] / 2**20:.0f} MiB: drop {drop / 2**20:.0f} MiB (stash + dS scratch = {want / 2**20:.0f} MiB)")
    assert drop >= 0.95 * want, (peak, want)


# ---------------------------------------------------------------------------------------------------------------------
# model level
# ---------------------------------------------------------------------------------------------------------------------
def _compare_with_fixture(hip, name, **kw):
    """_compare(hip, Ref.fixture(name)) for a fixture that tools/thin_model_fixture.py cut to at most K sampled elements per
    gradient tensor: the run's gradients are reduced to exactly the elements the file keeps, and the reference is marked as
    holding every element of what is then compared.  A fixture that was not thinned is compared as it is."""
    ref = Ref.fixture(name)
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", f"model_{name}.npz"))
    if "meta/grad_sample_k" in g.files:
        K = int(g["meta/grad_sample_k"])
        keep, losses, grads = hip
        grads, stored = dict(grads), ref.grads
        ref.sampled, ref.grads = False, {}
        for n, (g32, g64, numel) in stored.items():
            idx = synth.sample_indices(n, numel)
            idx = idx[synth.thinned_positions(idx.size, K)]
            assert idx.size == g32.size == g64.size, (n, idx.size, g32.size)
            ref.grads[n] = (g32, g64, idx.size)
            hip_name = "ground_decoder.decoder." + n if n.startswith("bbox_embed.") else n
            if hip_name in grads:
                assert grads[hip_name].numel() == numel, (n, grads[hip_name].shape, numel)
                grads[hip_name] = grads[hip_name].reshape(-1)[torch.from_numpy(idx).to(grads[hip_name].device)]
        hip = (keep, losses, grads)
    _compare(hip, ref, **kw)


@contextlib.contextmanager
def _long_rows(on=True):
    saved = ops.MHA_BS_LONG
    ops.MHA_BS_LONG = on
    try:
        yield
    finally:
        ops.MHA_BS_LONG = saved


def test_hr8_fixture_is_a_usable_yardstick():
    """The HR8 fixture is the case synth.MODEL_CASES defines (Ref.fixture asserts the dimensions) and fits a committed file.
    Its fp32 gradients, held to what `_compare` asks of a run, pass: the calibrated bound e <= 3 e_ref + 1e-3 holds for every
    tensor by construction (e = e_ref), so none of OUTSIDE_FRACTION is used up by the yardstick itself; what is NOT given
    by construction is checked from the file, on the elements it keeps — every tensor's e_ref stays below HARD_CAP (the
    reference's own error never lifts a tensor's hard cap max(HARD_CAP, 3 e_ref + 1e-3); a
    sample whose fp32 and fp64 halves were misaligned has e_ref ~ 1) and its largest element error stays below the 0.1
    of `_compare`'s gross-mismatch bar.  In the file: e_ref max 1.96e-3 (backbone.layer2), median 1.1e-6."""
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "model_HR8.npz")
    assert os.path.getsize(path) <= 1 << 20
    ref = Ref.fixture("HR8")
    assert ref.dims == (8, 704, 736, 10, None) and len(ref.grads) > 600
    assert ref.out["pred_boxes"].shape[0] == 8 and len(ref.losses) == 31
    e_ref, gross = [], []
    for name, (g32, g64, numel) in ref.grads.items():
        assert g32.size == g64.size == min(numel, 224), (name, g32.size, numel)
        nrm = float(np.linalg.norm(g64)) + GRAD_ABS_FLOOR * g64.size ** 0.5 / GRAD_TOL
        e_ref.append(float(np.linalg.norm(g32 - g64)) / nrm)
        gross.append(float(np.abs(g32 - g64).max()) / (float(np.abs(g64).max()) + GRAD_ABS_FLOOR / GRAD_TOL))
    e_ref, gross = np.asarray(e_ref), np.asarray(gross)
    print(f"[long rows] HR8 fixture: {e_ref.size} gradient tensors, e_ref max {e_ref.max():.2e} median {np.median(e_ref):.2e}, "
          f"{int((3 * e_ref > GRAD_TOL).sum())} with 3 e_ref > {GRAD_TOL}; largest element error {gross.max():.2e}")
    assert e_ref.max() < HARD_CAP, e_ref.max()
    assert gross.max() <= 0.1, gross.max()


@pytest.mark.gpu
def test_gpu_hr8_forward_backward():
    """704 x 736 frames: 517 encoder tokens per frame (above the fp32-pipe attention's 512), 516 keys = three 256-key chunks in
    the decoders' one-query cross-attention.  Forward + loss + backward in the default arithmetic against the reference's
    fixture: outputs 1e-3 absolute, span exact, 30 losses, calibrated gradients."""
    dev = use_hip()
    _compare_with_fixture(_hip_case(dev, "HR8", mma=BENCH_MMA), "HR8")


@pytest.mark.gpu
def test_gpu_hr8_throughput_mode():
    """the same clip in the 16-bit throughput mode, with the caps of test_gpu_nonsquare_clip_throughput_mode"""
    dev = use_hip()
    _compare_with_fixture(_hip_case(dev, "HR8", mma=THROUGHPUT_MMA), "HR8",
                          grad_caps={k: min(4 * v, 5e-2) for k, v in GRAD_CAPS_16BIT.items()})


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["NS8", "NS8_ragged"])
@pytest.mark.parametrize("mma", [BENCH_MMA, THROUGHPUT_MMA])
def test_gpu_nonsquare_clip_on_the_bf16_pipe(case, mma):
    """the 405 x 720 clips (310 tokens per frame) with the opt-in on, against their existing fixtures: the bars of the
    existing non-square tests (calibrated bound in bf16x6p, the 16-bit caps in bf16x3p)"""
    dev = use_hip()
    caps = {k: min(4 * v, 5e-2) for k, v in GRAD_CAPS_16BIT.items()} if mma == THROUGHPUT_MMA else None
    with _long_rows():
        _compare(_hip_case(dev, case, mma=mma), Ref.fixture(case), grad_caps=caps)


def _sampled(grads):
    return {n: g.reshape(-1)[torch.from_numpy(synth.sample_indices(n, g.numel()))] for n, g in grads.items()}


@pytest.mark.gpu
def test_gpu_hr8_deterministic_step_twice_bitwise():
    """two HR8 steps under set_deterministic(True): outputs, losses and the sampled elements of every gradient bit-equal"""
    dev = use_hip()
    L.set_deterministic(True)
    try:
        a = _hip_case(dev, "HR8", mma=BENCH_MMA)
        b = _hip_case(dev, "HR8", mma=BENCH_MMA)
    finally:
        L.set_deterministic(False)
    for k in ("pred_boxes", "pred_sted", "pred_actioness", "weights"):
        assert torch.equal(a[0][k], b[0][k]), k
    assert a[1] == b[1]
    ga, gb = _sampled(a[2]), _sampled(b[2])
    assert ga.keys() == gb.keys() and len(ga) > 100
    bad = [n for n in ga if not torch.equal(ga[n], gb[n])]
    assert not bad, f"{len(bad)} gradients differ bitwise, e.g. {bad[:6]}"


@pytest.mark.gpu
def test_gpu_hr8_replayed_step_equals_eager():
    """HR8 through bench.py's step object: the step replayed from the launch plans against the eager one, with the bars of
    tests/test_plans.py (outputs / loss 2e-4 of scale, gradients 3e-3 rel-L2), and against the reference's fixture"""
    from tests.test_plans import _check_equal
    dev = use_hip()
    rep = _run_bench_step(dev, "HR8", BENCH_MMA, use_plans=True)
    eag = _run_bench_step(dev, "HR8", BENCH_MMA, steps=1, use_plans=False)
    keys = ("pred_boxes", "pred_sted", "pred_actioness", "weights")
    form = lambda r: ({k: r[0][k] for k in keys}, r[1]["total"], r[2])  # noqa: E731
    _check_equal([form(eag)], [form(rep)], 2e-4, grad_l2=3e-3)
    assert rep[0]["post_sted"] == eag[0]["post_sted"]
    _compare_with_fixture(rep, "HR8")


@pytest.mark.gpu
def test_gpu_plans_follow_a_flip_of_the_long_row_route():
    """NS8 under launch plans: after three steps (eager, recorded, replayed) ops.MHA_BS_LONG flips — the signature changes,
    the next step replays nothing recorded on the other route, and computes the same step"""
    from stcat_amd.harness import TrainStep
    from stcat_amd.misc import BoxList
    dev = use_hip()
    T, res, Lt, pad, _ = synth.MODEL_CASES["NS8"]
    frames, mask, H, W = synth.synth_clip(T, res, pad)
    act, tb = synth.synth_targets(T)
    L.set_mma_mode(BENCH_MMA)
    plans.clear()
    plans.enable(True)
    plans.STATS.update(recorded=0, replayed=0, eager=0, run_s=0.0, refused=0)
    ts = None
    try:
        with _long_rows(False):
            ts = TrainStep(dev, (T, res, Lt), train=False, clip=(frames, mask),
                           targets=[{"actioness": act, "boxs": BoxList(tb, (W, H))}])
            for _ in range(3):
                t_off = ts.step().item()
            sig_off, before = plans._global_sig(dev), dict(plans.STATS)
            assert before["replayed"] >= 8, before
            g_off = {n: g.clone() for n, g in ts.gradients().items()}
            ops.MHA_BS_LONG = True
            assert plans._global_sig(dev) != sig_off
            t_on = ts.step().item()
            after = dict(plans.STATS)
            assert after["replayed"] == before["replayed"], (before, after)
            assert after["eager"] + after["recorded"] > before["eager"] + before["recorded"], (before, after)
            assert not after.get("refused"), after
            assert abs(t_on - t_off) <= 2e-4 * max(1.0, abs(t_off)), (t_on, t_off)
            enc = [n for n in g_off if n.startswith("ground_encoder.") and "self_attn.in_proj_weight" in n]
            assert enc
            for n in enc:
                close(ts.gradients()[n], g_off[n], 3e-3, "gradient across the flip: " + n)
                assert not torch.equal(ts.gradients()[n], g_off[n]), n     # other kernels ran: not the same bits
    finally:
        plans.enable(False)
        plans.clear()
        if ts is not None:
            ts.close()
        L.set_mma_mode("f32")


# ---------------------------------------------------------------------------------------------------------------------
# model level on the emulator: T = 2, 96 x 160 frames (3 x 5 map), 520 text tokens -> 536 tokens per frame
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.skipif(not os.environ.get("STCAT_SLOW"), reason="536-token rows of the assembled model through the emulator: "
                    "several minutes; STCAT_SLOW=1 runs it (the GPU runs HR8 at full size)")
def test_emu_long_text_clip_forward_backward():
    dev = use_emu()
    _compare(_run_hip(dev, 2, (96, 160), 520, mma=BENCH_MMA, blocks=SMALL_NET), Ref.oracle(2, (96, 160), 520, blocks=SMALL_NET))
