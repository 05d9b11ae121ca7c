"""The canonical window (stcat_amd.set_canonical_window(N)): the mean gradient of an optimizer step as ONE
fp32 expression over its N clips — the balanced binary tree ((g0 + g1) + (g2 + g3)) + ..., times fp32(1 / N) once — for
every split of the clips into `world` ranks x k micro-steps.

Every expected value is the tree restated in numpy fp32 inside this file (`_tree`), never a result of the code under
test, and every comparison is bitwise.  Kernels (stcat_grad_tree_fold through AdamW, stcat_rank_tree_sum): emulator and
GPU.  Layouts: gloo workers on the emulator, a toy model with dropout and several buckets, weights / EMA / moments equal
across all ranks of all layouts.  GPU: the C1 model in train mode under launch plans, (1, 4) against (2, 2)."""
import contextlib
import hashlib
import os

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.nn as nn

import stcat_amd
from stcat_amd import _lib as L
from stcat_amd import optim
from tests.backends import both
from tests.test_dist_ordered import _count_calls, _init, _run_ranks

F32 = np.float32
CHUNK = optim.CHUNK


# ---- the reference: numpy fp32 -----------------------------------------------------------------------------------------
def _tree(gs):
    """adjacent pairs in index order, level by level: ((g0 + g1) + (g2 + g3)) + ((g4 + g5) + (g6 + g7))"""
    gs = [np.asarray(g, dtype=F32) for g in gs]
    assert len(gs) & (len(gs) - 1) == 0
    while len(gs) > 1:
        gs = [gs[i] + gs[i + 1] for i in range(0, len(gs), 2)]
    return gs[0]


def _chain(gs):
    """what stcat_rank_sum / stcat_grad_accumulate add: left to right"""
    acc = np.asarray(gs[0], dtype=F32).copy()
    for g in gs[1:]:
        acc = acc + np.asarray(g, dtype=F32)
    return acc


def _values(rng, *shape):
    """normal times 2^[-12, 12], element by element"""
    return (rng.standard_normal(shape) * np.exp2(rng.integers(-12, 13, shape))).astype(F32)


def _bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.int32)


def _same_bits(got, want):
    got = got.detach().cpu().numpy() if torch.is_tensor(got) else got
    return got.shape == want.shape and np.array_equal(_bits(got), _bits(want))


class _mode:
    """deterministic mode + a canonical window of n clips, both off again afterwards"""

    def __init__(self, n):
        self.n = n

    def __enter__(self):
        self.saved = L._window
        L.set_deterministic(True)
        stcat_amd.set_canonical_window(self.n)

    def __exit__(self, *exc):
        L._window = self.saved
        L.set_deterministic(False)


@contextlib.contextmanager
def _counted():
    """the library calls by name while the block runs (the workers use tests.test_dist_ordered._count_calls, which stays on)"""
    counts, orig = {}, L.call

    def call(name, *a):
        counts[name] = counts.get(name, 0) + 1
        return orig(name, *a)
    L.call = call
    try:
        yield counts
    finally:
        L.call = orig


# ---- the switch --------------------------------------------------------------------------------------------------------
def test_switch_needs_deterministic_mode_and_a_power_of_two():
    from stcat_amd import plans
    from tests.backends import use_emu
    dev = use_emu()
    os.environ.pop("STCAT_CANONICAL_WINDOW", None)
    L.set_deterministic(False)
    was = L._window
    assert stcat_amd.canonical_window() is None
    with pytest.raises(ValueError, match="deterministic"):
        stcat_amd.set_canonical_window(4)
    assert stcat_amd.canonical_window() is None
    sig_off = plans._global_sig(dev)
    L.set_deterministic(True)
    try:
        sig_det = plans._global_sig(dev)
        for bad in (3, 0, -4, 6, 2.0, True, 256):
            with pytest.raises(ValueError, match="power of two"):
                stcat_amd.set_canonical_window(bad)
        stcat_amd.set_canonical_window(4)
        assert stcat_amd.canonical_window() == 4
        sig_on = plans._global_sig(dev)
        assert sig_on != sig_det != sig_off          # a plan recorded without the window is not replayed with it
        assert L.window_micro_steps(1) == 4 and L.window_micro_steps(2) == 2 and L.window_micro_steps(4) == 1
        for world in (3, 8):
            with pytest.raises(ValueError, match="does not divide"):
                L.window_micro_steps(world)
        stcat_amd.set_canonical_window(None)
        assert stcat_amd.canonical_window() is None and plans._global_sig(dev) == sig_det
        # the environment does the same where the setter was never called
        saved, L._window = L._window, L._UNSET
        try:
            os.environ["STCAT_CANONICAL_WINDOW"] = "8"
            assert stcat_amd.canonical_window() == 8
            os.environ["STCAT_CANONICAL_WINDOW"] = "12"
            with pytest.raises(ValueError, match="power of two"):
                stcat_amd.canonical_window()
            os.environ["STCAT_CANONICAL_WINDOW"] = "8"
            L.set_deterministic(False)
            with pytest.raises(ValueError, match="deterministic"):
                stcat_amd.canonical_window()
        finally:
            os.environ.pop("STCAT_CANONICAL_WINDOW", None)
            L._window = saved
    finally:
        L._window = was
        L.set_deterministic(False)


def test_entries_are_in_the_table():
    from tests.backends import use_emu
    use_emu()
    assert L.SIGNATURES["stcat_rank_tree_sum"] == L.SIGNATURES["stcat_rank_sum"] == "ppillfs"
    assert L.SIGNATURES["stcat_grad_tree_fold"] == "pppiiiifs"


# ---- tree fold: through AdamW.accumulate / step ------------------------------------------------------------------------
FOLD_SIZES = (CHUNK + 37, 1031, 1024)            # longer than one chunk (and n % 4 == 1); n % 4 == 3; misaligned levels
_fold_cache = {}


def _fold_inputs():
    """gradients [window][micro-step][tensor] for the largest k; smaller k use the first k micro-steps"""
    if not _fold_cache:
        rng = np.random.default_rng(20261021)
        _fold_cache["g"] = [[[_values(rng, n) for n in FOLD_SIZES] for _ in range(8)] for _ in range(2)]
        _fold_cache["p0"] = [_values(np.random.default_rng(7), n) * F32(2.0 ** -6) for n in FOLD_SIZES]
    return _fold_cache["g"], _fold_cache["p0"]


def _new_params(dev, p0):
    return [torch.from_numpy(p.copy()).to(dev).requires_grad_(True) for p in p0]


def _misaligned(dev, n):
    """n floats that start 4 bytes behind a 16-byte boundary"""
    room = torch.full((n + 8,), float("nan"), device=dev)
    off = 1 + (-(room.data_ptr() // 4) % 4)
    v = room[off:off + n]
    assert v.data_ptr() % 16 == 4
    return v


STEP_KW = dict(max_grad_norm=0.5)


@both
def _tree_fold_through_adamw(dev, big):
    g, p0 = _fold_inputs()
    # the inputs tell the tree from the chain: at k = 4 at least 10 % of the elements differ (measured on the CPU: 22 %)
    differ = total = 0
    for w in range(2):
        for ti in range(len(FOLD_SIZES)):
            gs = [g[w][m][ti] for m in range(4)]
            differ += int((_bits(_tree(gs)) != _bits(_chain(gs))).sum())
            total += gs[0].size
    print(f"k = 4: tree and chain differ in {differ} of {total} elements ({100.0 * differ / total:.1f} %)")
    assert differ >= 0.10 * total
    for k in (1, 2, 4, 8):
        q = k.bit_length() - 1
        with _mode(k):
            params = _new_params(dev, p0)
            opt = optim.AdamW(params, lr=1e-3)
            if q:
                opt._levels[params[2]] = [_misaligned(dev, FOLD_SIZES[2]) for _ in range(q)]
            with _counted() as counts:
                for w in range(2):                   # the second window reuses the level buffers, nothing is cleared
                    for m in range(k):
                        for p, gm in zip(params, g[w][m]):
                            p.grad = torch.from_numpy(gm.copy()).to(dev)
                        if m < k - 1:
                            opt.accumulate()
                            assert opt.accumulated == m + 1
                            with pytest.raises(RuntimeError, match="window is open"):
                                opt.state_dict()
                        else:
                            opt.step(**STEP_KW)
                    assert opt.accumulated == 0
                    for ti, p in enumerate(params):
                        want = _tree([g[w][m][ti] for m in range(k)]) * (F32(1.0) / F32(k))
                        got = opt._levels[p][q - 1] if q else p.grad
                        assert _same_bits(got, want), (k, w, ti, int((_bits(got.detach().cpu().numpy()) != _bits(want)).sum()))
            assert counts.get("stcat_grad_tree_fold", 0) == (2 * k if q else 0), counts
            assert "stcat_grad_accumulate" not in counts
            assert len(opt._levels.get(params[0], [])) == q     # log2(k) level buffers per parameter, none at k = 1
        # ... and the optimizer read the mean from there: a second optimizer, mode off, stepping on the numpy tree itself
        L.set_deterministic(True)
        try:
            ref_params = _new_params(dev, p0)
            ref = optim.AdamW(ref_params, lr=1e-3)
            for w in range(2):
                for ti, p in enumerate(ref_params):
                    p.grad = torch.from_numpy(_tree([g[w][m][ti] for m in range(k)]) * (F32(1.0) / F32(k))).to(dev)
                    if q and ti == 2:    # where the first optimizer read it: 4 bytes behind a 16-byte boundary (AdamW's own
                        p.grad = _misaligned(dev, FOLD_SIZES[2]).copy_(p.grad)    # kernels take their scalar form there)
                ref.step(**STEP_KW)
        finally:
            L.set_deterministic(False)
        for ti, (p, r) in enumerate(zip(params, ref_params)):
            assert torch.equal(p.detach().cpu().view(torch.int32), r.detach().cpu().view(torch.int32)), (k, ti)
            for key in ("exp_avg", "exp_avg_sq"):
                assert torch.equal(opt.state[p][key].cpu().view(torch.int32), ref.state[r][key].cpu().view(torch.int32)), (k, ti, key)


@both
def _tree_fold_refusals(dev, big):
    g, p0 = _fold_inputs()
    L.set_deterministic(True)
    try:
        with pytest.raises(ValueError, match="power of two"):       # k = 3
            stcat_amd.set_canonical_window(3)
    finally:
        L.set_deterministic(False)

    def grads(params, m):
        for p, gm in zip(params, g[0][m]):
            p.grad = torch.from_numpy(gm.copy()).to(dev)

    with _mode(4):
        params = _new_params(dev, p0)
        opt = optim.AdamW(params, lr=1e-3)
        before = [p.detach().clone() for p in params]
        grads(params, 0)
        with pytest.raises(ValueError, match=r"\b4 micro-steps.*after 1\b"):     # step() with no fold before it
            opt.step(**STEP_KW)
        opt.accumulate()
        grads(params, 1)
        with pytest.raises(ValueError, match=r"\b4 micro-steps.*after 2\b"):     # ... and after one
            opt.step(**STEP_KW)
        opt.accumulate()
        opt.accumulate()
        with pytest.raises(ValueError, match=r"\b4 micro-steps.*3 are folded"):  # a fourth accumulate(): that is step()'s
            opt.accumulate()
        assert opt.accumulated == 3 and opt.step_count == 0
        assert all(torch.equal(p.detach(), b) for p, b in zip(params, before))
        opt.discard_accumulated()
        assert opt.accumulated == 0
    with _mode(1):
        params = _new_params(dev, p0)
        opt = optim.AdamW(params, lr=1e-3)
        grads(params, 0)
        with pytest.raises(ValueError, match=r"\b1 micro-steps"):
            opt.accumulate()
    # the entry point itself: refused on the host, before any launch
    tab = torch.zeros(56, dtype=torch.uint8, device=dev)
    ct = torch.zeros(1, dtype=torch.int32, device=dev)
    co = torch.zeros(1, dtype=torch.int64, device=dev)
    st = L.stream_of(tab)
    args = (tab.data_ptr(), ct.data_ptr(), co.data_ptr())
    with pytest.raises(L.StcatHipError, match="n_carry"):
        L.call("stcat_grad_tree_fold", *args, 1, CHUNK, 5, 1, 1.0, st)
    with pytest.raises(L.StcatHipError, match="n_carry"):
        L.call("stcat_grad_tree_fold", *args, 1, CHUNK, -1, 0, 1.0, st)
    with pytest.raises(L.StcatHipError, match="n_carry=0"):
        L.call("stcat_grad_tree_fold", *args, 1, CHUNK, 0, 1, 1.0, st)
    with pytest.raises(L.StcatHipError, match="level 4"):
        L.call("stcat_grad_tree_fold", *args, 1, CHUNK, 4, 0, 1.0, st)
    with pytest.raises(L.StcatHipError, match="null"):
        L.call("stcat_grad_tree_fold", None, ct.data_ptr(), co.data_ptr(), 1, CHUNK, 0, 0, 1.0, st)
    with pytest.raises(L.StcatHipError, match="chunking"):
        L.call("stcat_grad_tree_fold", *args, 1, 0, 0, 0, 1.0, st)
    L.call("stcat_grad_tree_fold", *args, 0, CHUNK, 0, 0, 1.0, st)             # no chunks: nothing to do


# ---- rank tree ---------------------------------------------------------------------------------------------------------
RT_N = 1031
RT_STRIDE = -(-RT_N // 64) * 64


def _rank_inputs(n_ranks, seed):
    return _values(np.random.default_rng(seed), n_ranks, RT_N)


def _slices(dev, x, stride):
    """the slices with NaN between them and behind the last"""
    buf = torch.full((x.shape[0] * stride + 8,), float("nan"))
    for r in range(x.shape[0]):
        buf[r * stride:r * stride + x.shape[1]] = torch.from_numpy(x[r])
    return buf.to(dev)


def _tree_call(out, buf, n_ranks, n, stride, scale):
    L.call("stcat_rank_tree_sum", L._ptr(out), L._ptr(buf), n_ranks, n, stride, float(F32(scale)), L.stream_of(buf))


@both
def _rank_tree_sum(dev, big):
    x4 = _rank_inputs(4, 4)
    differ = int((_bits(_tree(list(x4))) != _bits(_chain(list(x4)))).sum())
    assert differ >= 0.10 * RT_N, differ           # the inputs tell the tree from the chain
    for n_ranks in (1, 2, 4, 8):
        x = _rank_inputs(n_ranks, n_ranks)
        for scale in (1.0, 1.0 / n_ranks):
            want = _tree(list(x)) * F32(scale)
            # out of its own
            buf = _slices(dev, x, RT_STRIDE)
            room = torch.full((RT_N + 8,), float("nan"), device=dev)
            _tree_call(room, buf, n_ranks, RT_N, RT_STRIDE, scale)
            assert _same_bits(room[:RT_N], want), (n_ranks, scale)
            assert bool(torch.isnan(room[RT_N:]).all())
            # out = slice 0, in place: nothing but its n floats changes
            before = buf.cpu().clone()
            _tree_call(buf, buf, n_ranks, RT_N, RT_STRIDE, scale)
            after = buf.cpu()
            assert _same_bits(after[:RT_N], want), (n_ranks, scale, "in place")
            assert torch.equal(after[RT_N:].view(torch.int32), before[RT_N:].view(torch.int32))
    # a -0.0f alone stays a -0.0f (one rank, scale 1: a copy — infinities and a NaN's payload as well)
    x = _rank_inputs(1, 11)
    x[0, :4] = np.array([-0.0, np.inf, -np.inf, 0.0], dtype=F32)
    src = _slices(dev, x, RT_STRIDE)
    out = torch.full((RT_N,), 7.0, device=dev)
    _tree_call(out, src, 1, RT_N, RT_STRIDE, 1.0)
    assert np.array_equal(_bits(out.cpu().numpy()), _bits(x[0]))
    assert _bits(out.cpu().numpy())[0] == np.int32(-2 ** 31)
    if big:                                          # more than one grid-stride pass of 2048 workgroups x 256 lanes
        n = 4 * 2048 * 256 + 4 * 300 + 3
        stride = -(-n // 64) * 64
        xb = _values(np.random.default_rng(5), 2, n)
        buf = _slices(dev, xb, stride)
        _tree_call(buf[stride:], buf, 2, n, stride, 0.5)
        assert _same_bits(buf[stride:stride + n], (xb[0] + xb[1]) * F32(0.5))


@both
def _rank_tree_refusals(dev, big):
    """refused on the host, before any launch, and nothing is written"""
    buf = torch.ones(4 * 64 + 8, device=dev)
    out = torch.full((64,), 7.0, device=dev)
    st = L.stream_of(buf)
    bp, op = buf.data_ptr(), out.data_ptr()
    for bad in (3, 0, 5, 6, 16, -2):
        with pytest.raises(L.StcatHipError, match="n_ranks"):
            L.call("stcat_rank_tree_sum", op, bp, bad, 64, 64, 1.0, st)
    with pytest.raises(L.StcatHipError, match="out"):
        L.call("stcat_rank_tree_sum", None, bp, 2, 64, 64, 1.0, st)
    with pytest.raises(L.StcatHipError, match=r"\bin\b"):
        L.call("stcat_rank_tree_sum", op, None, 2, 64, 64, 1.0, st)
    with pytest.raises(L.StcatHipError, match="stride"):            # a misaligned stride
        L.call("stcat_rank_tree_sum", op, bp, 2, 61, 62, 1.0, st)
    with pytest.raises(L.StcatHipError, match="stride"):            # slices that overlap each other
        L.call("stcat_rank_tree_sum", op, bp, 2, 64, 60, 1.0, st)
    with pytest.raises(L.StcatHipError, match="aligned"):
        L.call("stcat_rank_tree_sum", op + 4, bp, 2, 32, 64, 1.0, st)
    with pytest.raises(L.StcatHipError, match="aligned"):
        L.call("stcat_rank_tree_sum", op, bp + 4, 2, 32, 64, 1.0, st)
    with pytest.raises(L.StcatHipError, match=r"\bn="):
        L.call("stcat_rank_tree_sum", op, bp, 2, -1, 64, 1.0, st)
    for off in (4, 64 + 4, 3 * 64 + 60, 64 - 4):                    # out overlaps a slice without being it
        with pytest.raises(L.StcatHipError, match="out overlaps"):
            L.call("stcat_rank_tree_sum", bp + 4 * off, bp, 4, 64, 64, 1.0, st)
    assert float(out.min()) == 7.0 == float(out.max()) and float(buf.min()) == 1.0 == float(buf.max())
    L.call("stcat_rank_tree_sum", bp + 4 * 2 * 64, bp, 2, 64, 64, 0.5, st)     # directly behind the last slice: fine
    assert torch.equal(buf[128:192].cpu(), torch.ones(64))
    L.call("stcat_rank_tree_sum", op, bp, 4, 0, 0, 1.0, st)                    # n = 0: nothing runs
    assert float(out.min()) == 7.0


@both
def _tree_is_close_to_the_chain(dev, big):
    """the tree is another rounding of the sum the existing entry points compute, not another sum: elementwise
    |tree - chain| <= N * 2^-24 * sum |g_i| — N adds, each within half an ulp of a partial sum that |g_0| + ... bounds
    (both from the kernels: stcat_rank_tree_sum and stcat_rank_sum)"""
    for n_ranks in (4, 8):
        x = _rank_inputs(n_ranks, 40 + n_ranks)
        buf = _slices(dev, x, RT_STRIDE)
        tree = torch.empty(RT_N, device=dev)
        chain = torch.empty(RT_N, device=dev)
        _tree_call(tree, buf, n_ranks, RT_N, RT_STRIDE, 1.0)
        L.call("stcat_rank_sum", chain.data_ptr(), buf.data_ptr(), n_ranks, RT_N, RT_STRIDE, 1.0, L.stream_of(buf))
        assert _same_bits(chain, _chain(list(x)))
        diff = np.abs(tree.cpu().numpy().astype(np.float64) - chain.cpu().numpy().astype(np.float64))
        bound = n_ranks * 2.0 ** -24 * np.abs(x.astype(np.float64)).sum(0)
        print(f"N = {n_ranks}: max |tree - chain| / bound = {float((diff / bound).max()):.3f}")
        assert bool((diff <= bound).all())
        assert bool((diff > 0).any())


# ---- layouts: gloo workers on the emulator -----------------------------------------------------------------------------
class DropToy(nn.Module):
    """conv -> mean -> dropout -> linear -> dropout -> linear: three buckets at ~1 KB.  The head's bias has 3 elements:
    packed back to back the next parameter of its bucket would start 12 bytes behind a 16-byte boundary, and the optimizer's
    kernels (which choose their float4 or scalar form by alignment) would add the squared norm in another order on the
    layouts that step from the bucket views (k = 1) than on those that step from the level buffers"""

    def __init__(self):
        super().__init__()
        self.conv = nn.Conv2d(8, 16, 3, bias=False)
        self.lin = nn.Linear(16, 24)
        self.head = nn.Linear(24, 3)

    def forward(self, x):
        from stcat_amd import ops
        h = self.conv(x).mean((2, 3))
        h = ops.dropout(h, 0.25)
        h = ops.dropout(torch.tanh(self.lin(h)), 0.25)
        return self.head(h)


def _toy_clip(g):
    """global clip g of the shared list: (frames, box count) — magnitudes mixed, counts differ"""
    gen = torch.Generator().manual_seed(5000 + g)
    x = torch.randn(2, 8, 5, 5, generator=gen) * 2.0 ** torch.randint(-6, 7, (2, 8, 1, 1), generator=gen).float()
    return x, 1 + (5 * g + 3) % 7


def _layout_worker(rank, world, port, q, n_win, mode_on):
    torch.set_num_threads(1)
    import copy
    from stcat_amd import ops
    from stcat_amd.dist import GradBucketReducer
    from stcat_amd.harness import window_num_boxes
    from tests.backends import use_emu
    dev = use_emu()
    L.set_deterministic(True)
    if mode_on:
        stcat_amd.set_canonical_window(n_win)
    if world > 1:
        _init(rank, world, port)
    counts = _count_calls()
    k = n_win // world
    ops.manual_seed(1234, rank)
    torch.manual_seed(0)
    model = DropToy()
    ema = copy.deepcopy(model)
    red = GradBucketReducer(model, bucket_mb=0.001)      # ~1 KB: three buckets
    assert len(red.buckets) >= 3
    assert red.ordered == (world > 1 and (mode_on or world > 2))
    if world > 1:
        aligned = [v.data_ptr() % 16 == 0 for b in red.buckets for v in b["views"]]
        assert all(aligned) if mode_on else not all(aligned)
    opt = optim.AdamW(list(model.parameters()), lr=1e-2)
    for s in range(2):
        numbers = [s * n_win + m * world + rank for m in range(k)]
        if mode_on:
            nb = window_num_boxes([_toy_clip(g)[1] for g in numbers], n_win, dev)
        for m, g in enumerate(numbers):
            x, boxes = _toy_clip(g)
            red.zero_grad()
            if mode_on:
                ops.dropout_begin_step(dev, clip=g)
            else:
                ops.dropout_begin_step(dev)
                nb = torch.tensor([float(boxes)])
                if world > 1:
                    dist.all_reduce(nb)
                nb = torch.clamp(nb / world, min=1)
            (model(x).square().sum() / nb[0]).backward()
            red.finish()
            if m < k - 1:
                opt.accumulate()
            else:
                opt.step(max_grad_norm=0.5, model_ema=ema, ema_decay=0.9, model=model)
    out = {}
    for n, p in model.named_parameters():
        out["w/" + n] = p.detach().numpy().copy()
        out["m/" + n] = opt.state[p]["exp_avg"].numpy().copy()
        out["v/" + n] = opt.state[p]["exp_avg_sq"].numpy().copy()
    for n, p in ema.named_parameters():
        out["ema/" + n] = p.detach().numpy().copy()
    want_tree = 2 * k * len(red.buckets) if (mode_on and world > 1) else 0
    assert counts.get("stcat_rank_tree_sum", 0) == want_tree, counts
    assert counts.get("stcat_grad_tree_fold", 0) == (2 * k if (mode_on and k > 1) else 0), counts
    q.put((rank, out))
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


def _layout(world, n_win, mode_on=True):
    from tests.backends import use_emu
    use_emu()
    return _run_ranks(_layout_worker, world, n_win, mode_on)


def _first_difference(a, b):
    for key in sorted(a):
        if not np.array_equal(_bits(a[key]), _bits(b[key])):
            return key
    return None


@pytest.mark.parametrize("n_win, worlds", [(4, (1, 2, 4)), (8, (1, 2, 8))])
def test_layouts_give_the_same_bits(n_win, worlds):
    """two optimizer steps (clip, EMA) over 2 N distinct clips with differing box counts, dropout on: weights, EMA weights
    and both moments are equal bit for bit across every rank of every layout world x (N / world)"""
    results = {w: _layout(w, n_win) for w in worlds}
    first = results[worlds[0]][0][1]
    assert any(np.abs(v).max() > 0 for k_, v in first.items() if k_.startswith("m/"))
    for w, out in results.items():
        assert [o[0] for o in out] == list(range(w))
        for rank, got in out:
            assert set(got) == set(first)
            assert _first_difference(got, first) is None, (n_win, w, rank, _first_difference(got, first))


def test_layouts_differ_with_the_mode_off():
    """the same script without the canonical window: (1, 4) and (2, 2) part ways — the comparison above can fail"""
    a = _layout(1, 4, mode_on=False)[0][1]
    b = _layout(2, 4, mode_on=False)
    assert _first_difference(b[0][1], a) is not None
    assert _first_difference(b[0][1], b[1][1]) is None         # (deterministic mode: the two ranks still agree)


def test_dropout_masks_follow_the_clip_number():
    """in the mode the seed leaves the rank out and begin_step(clip=G) sets the counter base to (G + 1) * STEP_SPAN —
    whatever came before; out of the mode both are as they were"""
    from stcat_amd import ops
    from tests.backends import use_emu
    dev = use_emu()
    ds = ops._dropout_stream
    try:
        with _mode(4):
            ops.manual_seed(99, 3)
            seed3 = ds.seed
            ops.manual_seed(99, 0)
            assert ds.seed == seed3
            ops.dropout_begin_step(dev)
            ops.dropout_begin_step(dev, clip=6)
            assert int(ds.base(dev)[0]) == 7 * ds.STEP_SPAN and ds.offset == 0
            ops.dropout_begin_step(dev, clip=0)
            assert int(ds.base(dev)[0]) == ds.STEP_SPAN
            with pytest.raises(ValueError, match="clip"):
                ops.dropout_begin_step(dev, clip=-1)
        ops.manual_seed(99, 3)
        assert ds.seed != seed3 and ds.seed == ops._mix_seed(99, 3)
        ops.dropout_begin_step(dev)
        ops.dropout_begin_step(dev)
        assert int(ds.base(dev)[0]) == 2 * ds.STEP_SPAN
    finally:
        ops.manual_seed(0, 0)


def test_loss_plan_takes_the_window_normaliser():
    """a plan built with num_boxes= returns it (no collective, no clamp of its own); window_num_boxes is
    clamp(total / N, 1) as a device scalar"""
    from stcat_amd import synth
    from stcat_amd.harness import window_num_boxes
    from stcat_amd.misc import BoxList
    from stcat_amd.pipeline import VideoSTGLoss
    act, tb = synth.synth_targets(8)
    targets = [{"actioness": act, "boxs": BoxList(tb)}]
    crit = VideoSTGLoss()
    nb = window_num_boxes([3, 4, 6], 4, "cpu")
    assert nb.dtype == torch.float32 and nb.shape == (1,) and float(nb) == 3.25
    assert float(window_num_boxes([1], 4, "cpu")) == 1.0
    buf = torch.zeros(1)
    assert window_num_boxes([8, 9], 2, "cpu", out=buf) is buf and float(buf) == 8.5
    plan = crit.plan(targets, [8], "cpu", num_boxes=nb)
    assert plan.num_boxes("cpu") is nb
    assert crit.plan(targets, [8], "cpu").num_boxes("cpu") == 4.0


# ---- GPU: the C1 model in train mode under launch plans ------------------------------------------------------------------
def _model_clips(T, res, n):
    from stcat_amd import synth
    from stcat_amd.misc import BoxList
    clips, targets = [], []
    for c in range(n):
        frames = synth.synth_frames(T, res, seed=700 + c)
        clips.append((frames, torch.zeros(T, res, res, dtype=torch.bool)))
        lo, hi = 1 + c % 3, T - 1 - (c // 3) % 2          # spans (and so box counts) differ from clip to clip
        act = torch.zeros(T, dtype=torch.long)
        act[lo:hi] = 1
        _, tb = synth.synth_targets(T, seed=c)
        boxes = tb[:1].repeat(hi - lo, 1) + 0.01 * torch.arange(hi - lo)[:, None]
        targets.append([{"actioness": act, "boxs": BoxList(boxes.float())}])
    assert len({len(t[0]["boxs"]) for t in targets}) >= 3
    return clips, targets


def _model_worker(rank, world, port, q, n_win, steps):
    from stcat_amd import plans, synth
    from stcat_amd.harness import TrainStep
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    L.load()
    L.set_mma_mode("bf16x6p")
    L.set_deterministic(True)
    stcat_amd.set_canonical_window(n_win)
    if world > 1:
        _init(rank, world, port)
    counts = _count_calls()
    T, res, _ = synth.CONFIGS["C1"]
    clips, targets = _model_clips(T, res, 6)             # 6 does not divide the 12 clips' numbering evenly into ranks
    plans.enable(True)
    ts = TrainStep(dev, "C1", rank=rank, train=True, clips=clips, clip_targets=targets)
    assert ts.reducer.ordered == (world > 1)
    opt = optim.AdamW([p for p in ts.model.parameters() if p.requires_grad], lr=1e-4)
    k = n_win // world
    per_step = []
    for s in range(steps):                               # micro-steps run eager, recorded, then replayed
        before = counts.get("stcat_rank_tree_sum", 0)
        ts.window(opt, k, max_grad_norm=0.1)
        per_step.append(counts.get("stcat_rank_tree_sum", 0) - before)
    torch.cuda.synchronize()
    h = hashlib.sha256()
    n_tensors = 0
    for n, p in sorted(ts.model.named_parameters(), key=lambda t: t[0]):
        st = opt.state.get(p)
        for t in (p,) + ((st["exp_avg"], st["exp_avg_sq"]) if st else ()):
            assert bool(torch.isfinite(t).all()), n
            h.update(n.encode())
            h.update(t.detach().cpu().contiguous().numpy().tobytes())
            n_tensors += 1
    stats = dict(plans.STATS)
    res_ = (rank, h.hexdigest(), n_tensors, per_step, len(ts.reducer.buckets), stats.get("refused"), stats["replayed"],
            counts.get("stcat_grad_tree_fold", 0))
    plans.enable(False)
    ts.close()
    q.put(res_)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


@pytest.mark.gpu
def test_gpu_model_one_rank_four_steps_equals_two_ranks_two_steps():
    """C1, train mode (dropout), bf16x6p, launch plans on, N = 4, three optimizer steps: one process running 4 micro-steps
    and two gloo ranks on the card running 2 each end with the same SHA-256 over every weight and both moments; in the
    two-rank run stcat_rank_tree_sum ran buckets x micro-steps times per optimizer step and no recording was refused"""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    one = _run_ranks(_model_worker, 1, 4, 3)
    two = _run_ranks(_model_worker, 2, 4, 3)
    digests = [o[1] for o in one + two]
    for rank, digest, n_tensors, per_step, n_buckets, refused, replayed, n_fold in one + two:
        assert n_tensors > 300 and not refused and replayed >= 10, (rank, n_tensors, refused, replayed)
    assert one[0][3] == [0, 0, 0] and one[0][7] == 3 * 4
    for o in two:
        assert o[3] == [o[4] * 2] * 3 and o[4] >= 2, o[3:5]
        assert o[7] == 3 * 2
    assert digests[0] == digests[1] == digests[2], digests
