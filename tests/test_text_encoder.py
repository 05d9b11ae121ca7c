"""Native text encoder (stcat_amd/text.py, csrc/text_encoder.h): kernel tests against in-test torch fp64, module tests
against the fixtures tests/golden/text_*.npz (the reference's Roberta + FeatureResizer around the real
transformers.RobertaModel, fp32 and fp64: tests/golden/make_text_golden.py) and against an fp64 plain-torch restatement
of the module that lives here (pinned to the fixtures, then used for train mode with the traced dropout masks).

Kernel tolerances: TOL = 2e-4 relative to the tensor scale, the number tests/test_ops.py applies to the head-dimension-32
attention kernels, LayerNorm and stcat_ew.  Module bars: OUT_TOL / GRAD_TOL / GRAD_ABS_FLOOR of tests/test_model_parity.py.
"""
import json
import os
import socket

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from stcat_amd import _lib as L
from stcat_amd import ops, plans, synth
from stcat_amd.text import TextConfig, TextEncoder, build_text_encoder
from tests.backends import both, close, host_memory_slot

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
TOL = 2e-4                  # tests/test_ops.py
OUT_TOL = 1e-3              # tests/test_model_parity.py
GRAD_TOL = 1e-3
GRAD_ABS_FLOOR = 2e-6
D = 768


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed + sum(shape))
    return (torch.randn(*shape, generator=g, dtype=torch.float64) * scale)


def _mask_of(p, seed, offset, n):
    keep = ops.dropout_keep_mask(seed, offset, n, p)
    return torch.from_numpy(keep.astype(np.float64)) * float(np.float32(1.0 / (1.0 - float(np.float32(p)))))


# ---------------------------------------------------------------------------------------
# kernels
# ---------------------------------------------------------------------------------------
def _embed_case(dev, ids, V, P, pdrop=0.0):
    n = len(ids)
    ids_t = torch.tensor(ids, dtype=torch.int64)
    pos_t = torch.arange(n, dtype=torch.int64) + 2
    word, pos, typ = rnd(V, D, seed=1, scale=0.5), rnd(P, D, seed=2, scale=0.5), rnd(1, D, seed=3, scale=0.5)
    gam, bet, gy = rnd(D, seed=4) * 0.1 + 1, rnd(D, seed=5) * 0.1, rnd(n, D, seed=6)
    drop = (0.0, 0, 0, None)
    m = torch.ones(n, D, dtype=torch.float64)
    if pdrop > 0.0:
        ops.manual_seed(31)
        seed, off, base = ops._dropout_stream.take(n * D, dev)
        drop = (pdrop, seed, off, base)
        m = _mask_of(pdrop, seed, off, n * D).view(n, D)
    leaves = [t.clone().requires_grad_(True) for t in (word, pos, typ, gam, bet)]
    e = leaves[0][ids_t] + leaves[1][pos_t] + leaves[2][0]
    e.retain_grad()
    ref = F.layer_norm(e, (D,), leaves[3], leaves[4], 1e-5) * m
    (ref * gy).sum().backward()
    dv = [t.float().to(dev) for t in (word, pos, typ, gam, bet)]
    idd, pdd = ids_t.to(dev), pos_t.to(dev)
    y, mean, rstd = ops.embed_ln_fwd_raw(idd, pdd, *dv, 1e-5, drop)
    grads = ops.embed_ln_bwd_raw(gy.float().to(dev), idd, pdd, *dv[:4], mean, rstd, drop)
    tag = f"embed_ln L{n} p{pdrop}"
    close(y, ref, TOL, tag + " y")
    for g, r, nm in zip(grads, leaves, ("dword", "dpos", "dtype", "dgamma", "dbeta")):
        close(g, r.grad, TOL, f"{tag} {nm}")
    dword = grads[0].cpu()
    # a repeated id: its row is the sum over its positions; rows no token names stay exactly zero
    for tok in set(ids):
        where = [t for t, i in enumerate(ids) if i == tok]
        close(dword[tok], e.grad[where].sum(0), TOL, f"{tag} row of id {tok} ({len(where)} positions)")
    untouched = torch.ones(V, dtype=torch.bool)
    untouched[ids_t] = False
    assert float(dword[untouched].abs().max()) == 0.0 if untouched.any() else True
    upos = torch.ones(P, dtype=torch.bool)
    upos[pos_t] = False
    assert float(grads[1].cpu()[upos].abs().max()) == 0.0
    # a second run gives the same bits (one owner per element, fixed order)
    y2, mean2, rstd2 = ops.embed_ln_fwd_raw(idd, pdd, *dv, 1e-5, drop)
    grads2 = ops.embed_ln_bwd_raw(gy.float().to(dev), idd, pdd, *dv[:4], mean2, rstd2, drop)
    assert torch.equal(y.cpu(), y2.cpu())
    for a, b in zip(grads, grads2):
        assert torch.equal(a.cpu(), b.cpu())


@both
def _embed_ln(dev, big):
    V, P = 50, 140
    _embed_case(dev, [0], V, P)
    _embed_case(dev, [7, 3, 7, 7, 2], V, P)
    _embed_case(dev, [7, 3, 7, 7, 2], V, P, pdrop=0.1)
    g = torch.Generator().manual_seed(5)
    ids = torch.randint(0, V, (128,), generator=g).tolist()
    ids[0], ids[17], ids[127] = 0, V - 1, V - 1
    _embed_case(dev, ids, V, P)
    # an id at the vocabulary size is refused with an error (and the kernel never reads that row)
    tabs = [torch.zeros(s, D).to(dev) for s in (V, P, 1)] + [torch.ones(D).to(dev), torch.zeros(D).to(dev)]
    with pytest.raises(L.StcatHipError, match="outside the vocabulary"):
        ops.embed_ln_fwd_raw(torch.tensor([3, V]).to(dev), torch.tensor([2, 3]).to(dev), *tabs)
    with pytest.raises(L.StcatHipError, match="position"):
        ops.embed_ln_fwd_raw(torch.tensor([3, 4]).to(dev), torch.tensor([2, P]).to(dev), *tabs)
    # the C entry point itself cannot refuse (the ids live on the device): the kernel reads nothing for such a token and
    # writes a NaN row; its neighbours are untouched.  Row V of the table does not exist: the table is exactly V rows long.
    tabs[0] = torch.ones(V, D).to(dev)
    ids_bad, pos_ok = torch.tensor([3, V, 4, -1]).to(dev), torch.tensor([2, 3, 4, 5]).to(dev)
    y, mean, rstd = (torch.zeros(4, D).to(dev), torch.zeros(4).to(dev), torch.zeros(4).to(dev))
    L.call("stcat_embed_ln_fwd", ids_bad.data_ptr(), pos_ok.data_ptr(), *(t.data_ptr() for t in tabs), y.data_ptr(),
           mean.data_ptr(), rstd.data_ptr(), 4, D, V, P, 1e-5, 0.0, 0, 0, None, L.stream_of(y))
    y = y.cpu()
    assert bool(torch.isnan(y[1]).all()) and bool(torch.isnan(y[3]).all()) and bool(torch.isfinite(y[[0, 2]]).all())
    # padding_idx: the rows of the padding id keep a zero gradient in both tables, as nn.Embedding(padding_idx=1) does
    ids_p, pos_p = torch.tensor([7, 1, 7, 1, 2]), torch.tensor([2, 1, 3, 1, 4])
    emb = [torch.nn.Embedding(V, D, padding_idx=1).double(), torch.nn.Embedding(P, D, padding_idx=1).double()]
    typ, gam, bet, gy = rnd(1, D, seed=3, scale=0.5), rnd(D, seed=4) * 0.1 + 1, rnd(D, seed=5) * 0.1, rnd(5, D, seed=6)
    (F.layer_norm(emb[0](ids_p) + emb[1](pos_p) + typ[0], (D,), gam, bet, 1e-5) * gy).sum().backward()
    dv = [t.detach().float().to(dev) for t in (emb[0].weight, emb[1].weight, typ, gam, bet)]
    _, mean, rstd = ops.embed_ln_fwd_raw(ids_p.to(dev), pos_p.to(dev), *dv)
    g = ops.embed_ln_bwd_raw(gy.float().to(dev), ids_p.to(dev), pos_p.to(dev), *dv[:4], mean, rstd, pad=1)
    close(g[0], emb[0].weight.grad, TOL, "padding_idx dword")
    close(g[1], emb[1].weight.grad, TOL, "padding_idx dpos")
    assert float(g[0][1].abs().max()) == 0.0 and float(g[1][1].abs().max()) == 0.0


def _ln768_case(dev, M, with_res, pdrop):
    x, r = rnd(M, D, seed=1, scale=3.0), rnd(M, D, seed=2)
    gam, bet, gy = rnd(D, seed=3) * 0.1 + 1, rnd(D, seed=4) * 0.1, rnd(M, D, seed=5)
    ops.manual_seed(99)
    seed, off = ops.dropout_stream_state()
    m = _mask_of(pdrop, seed, off, M * D).view(M, D) if pdrop > 0.0 else 1.0
    leaves = [t.clone().requires_grad_(True) for t in (x, r, gam, bet)]
    ref = F.layer_norm(leaves[0] * m + (leaves[1] if with_res else 0.0), (D,), leaves[2], leaves[3], 1e-5)
    ref.backward(gy)
    dl = [t.float().to(dev).requires_grad_(True) for t in (x, r, gam, bet)]
    y = ops.layer_norm(dl[0], dl[2], dl[3], res=dl[1] if with_res else None, drop_p=pdrop)
    y.backward(gy.float().to(dev))
    tag = f"layernorm768 M{M} res{with_res} p{pdrop}"
    close(y, ref, TOL, tag + " y")
    for i, nm in enumerate(("dx", "dres", "dgamma", "dbeta")):
        if nm == "dres" and not with_res:
            continue
        close(dl[i].grad, leaves[i].grad, TOL, f"{tag} {nm}")


@both
def _layernorm_768(dev, big):
    for M in (1, 5, 130):
        for with_res in (False, True):
            for p in (0.0, 0.1):
                _ln768_case(dev, M, with_res, p)


def _mha_d64_case(dev, B, S, H, masked, pdrop):
    SP = ((S + 31) // 32) * 32
    Dm = 64 * H
    q, k, v, go = (rnd(B, S, Dm, seed=s) for s in (1, 2, 3, 4))
    kpm = None
    if masked:
        kpm = torch.zeros(B, S, dtype=torch.bool)
        kpm[B - 1, S - max(1, S // 3):] = True           # the tail of the last row is padding
        if S == 1:
            kpm[:] = False
    drop = (0.0, 0, 0, None)
    m = 1.0
    if pdrop > 0.0:
        ops.manual_seed(77)
        seed, off, base = ops._dropout_stream.take(B * H * SP * SP, dev)
        drop = (pdrop, seed, off, base)
        # counter layout: ((b H + h) SP + key) SP + query
        m = _mask_of(pdrop, seed, off, B * H * SP * SP).view(B, H, SP, SP)[:, :, :S, :S].transpose(-1, -2)
    leaves = [t.clone().requires_grad_(True) for t in (q, k, v)]
    qh, kh, vh = (t.view(B, S, H, 64).transpose(1, 2) for t in leaves)
    sc = qh @ kh.transpose(-1, -2) * 0.125
    if kpm is not None:
        sc = sc.masked_fill(kpm[:, None, None, :], float("-inf"))
    ref = ((sc.softmax(-1) * m) @ vh).transpose(1, 2).reshape(B, S, Dm)
    (ref * go).sum().backward()
    qd, kd, vd = (t.float().to(dev) for t in (q, k, v))
    o, P = ops.mha_d64_fwd_raw(qd, kd, vd, kpm.to(dev) if kpm is not None else None, 0.125, drop)
    dq, dk, dv = ops.mha_d64_bwd_raw(qd, kd, vd, go.float().to(dev), P, 0.125, drop)
    tag = f"mha_d64 B{B} S{S} H{H} masked{masked} p{pdrop}"
    close(o, ref, TOL, tag + " out")
    for g, r, nm in zip((dq, dk, dv), leaves, ("dq", "dk", "dv")):
        close(g, r.grad, TOL, f"{tag} {nm}")
    o_inf, none = ops.mha_d64_fwd_raw(qd, kd, vd, kpm.to(dev) if kpm is not None else None, 0.125, drop, keep=False)
    assert none is None and torch.equal(o_inf.cpu(), o.cpu())


@both
def _mha_d64(dev, big):
    for S in (1, 5, 31, 32, 33, 64, 65, 128):
        _mha_d64_case(dev, 1, S, 1, False, 0.0)
    for S in (5, 33, 128):
        _mha_d64_case(dev, 1, S, 12, False, 0.0)
    for S in (5, 33, 65):
        _mha_d64_case(dev, 2, S, 1, True, 0.0)
    _mha_d64_case(dev, 2, 40, 12, True, 0.1)
    _mha_d64_case(dev, 1, 128, 1, False, 0.1)
    x = torch.zeros(1, 129, 64).to(dev)
    with pytest.raises(L.StcatHipError, match="128"):
        ops.mha_d64_fwd_raw(x, x, x, None)
    with pytest.raises(L.StcatHipError, match="128"):
        ops.mha_d64_bwd_raw(x, x, x, x, torch.zeros(1, 1, 129, 129).to(dev))


@both
def _gelu(dev, big):
    for n in (1, 7, 4096 + 3):
        x = rnd(n, seed=1, scale=2.0)
        x[: min(n, 3)] = torch.tensor([-6.0, 0.0, 6.0])[: min(n, 3)]
        gy = rnd(n, seed=2)
        xr = x.clone().requires_grad_(True)
        ref = F.gelu(xr)
        ref.backward(gy)
        xd = x.float().to(dev)
        close(ops.gelu_raw(xd), ref, TOL, f"gelu n{n}")
        close(ops.gelu_bwd_raw(gy.float().to(dev), xd), xr.grad, TOL, f"gelu backward n{n}")


# ---------------------------------------------------------------------------------------
# the module
# ---------------------------------------------------------------------------------------
CASES = {"text_T2": (2, 1024), "text_T2_L40": (2, 1024), "text_R12": (12, 50265)}
_FIX = {}


def fixture(case):
    if case not in _FIX:
        _FIX[case] = dict(np.load(os.path.join(GOLDEN, case + ".npz")))
    return _FIX[case]


def loss_weights(case, n, d=256):
    return (torch.from_numpy(synth.hash_normal(f"text/w1/{case}", n * d).reshape(n, 1, d)),
            torch.from_numpy(synth.hash_normal(f"text/w2/{case}", d).reshape(1, d)))


def build(case, dev, train=False, freeze=False, tokenizer=None, layers=None):
    vocab = CASES[case][1]
    layers = layers or CASES[case][0]
    m = TextEncoder(TextConfig(vocab=vocab, layers=layers), tokenizer, freeze=freeze)
    synth.fill_module_(m, skip_prefixes=())
    return m.to(dev).train(train)


class grouped_path:
    """Make the eager node take the launches the replayed node takes — the grouped Q/K/V projection, its grouped data and
    weight gradients, the skinny accumulating GEMMs — by giving it the zeroed arena they need (split-bf16 modes), and count
    the grouped launches so that a test can assert the branch was taken."""

    def __init__(self, dev):
        self.dev = dev
        self.count = {"linear_fwd_multi": 0, "linear_dgrad_multi": 0, "linear_wgrad_multi": 0}

    def __enter__(self):
        self.arena = ops.enable_zero_arena(self.dev, 1 << 23)
        self.saved = {k: getattr(ops, k) for k in self.count}
        for k, fn in self.saved.items():
            def counted(*a, _k=k, _fn=fn):
                self.count[_k] += 1
                return _fn(*a)
            setattr(ops, k, counted)
        return self

    def __exit__(self, *exc):
        for k, fn in self.saved.items():
            setattr(ops, k, fn)
        ops.disable_zero_arena()
        return False

    def taken(self, layers, steps=1):
        return all(v >= layers * steps for v in self.count.values())


def run_module(m, case, dev):
    """forward + backward of the fixture's loss -> (memory, cls, {name: grad})"""
    ids = torch.from_numpy(fixture(case)["input_ids"])[None]
    for p in m.parameters():
        p.grad = None
    (mask, mem, _), cls = m.forward_ids(ids, torch.ones_like(ids))
    assert mask.dtype == torch.bool and not bool(mask.any()) and mem.shape == (ids.shape[1], 1, 256) and cls.shape == (1, 256)
    w1, w2 = loss_weights(case, ids.shape[1])
    ((mem * w1.to(dev)).sum() + (cls * w2.to(dev)).sum()).backward()
    return mem.detach().cpu(), cls.detach().cpu(), {n: p.grad.detach().cpu() for n, p in m.named_parameters() if p.grad is not None}


def run_module_grouped(m, case, dev):
    """run_module on the grouped path in the split-bf16 modes (mode f32 has no grouped launches: plain run_module)"""
    if L.get_mma_mode() == "f32":
        return run_module(m, case, dev)
    with grouped_path(dev) as gp:
        out = run_module(m, case, dev)
    assert gp.taken(m.config.layers), gp.count
    return out


def ref_text(sd, ids, layers, masks=None, H=12, eps=1e-5):
    """plain-torch restatement of RobertaModel + FeatureResizer on a state dict (any dtype); masks: the dropout multipliers
    of the sites in launch order (embeddings; per layer attention [H,S,S], the two hidden dropouts; memory; cls) or None"""
    it = iter(masks) if masks is not None else None

    def drop(x):
        return x if it is None else x * next(it).view(x.shape).to(x.dtype)

    S = ids.shape[0]
    e = "body.embeddings."
    pos = torch.arange(S) + 2
    x = sd[e + "word_embeddings.weight"][ids] + sd[e + "position_embeddings.weight"][pos] + sd[e + "token_type_embeddings.weight"][0]
    x = drop(F.layer_norm(x, (D,), sd[e + "LayerNorm.weight"], sd[e + "LayerNorm.bias"], eps))
    for i in range(layers):
        p = f"body.encoder.layer.{i}."
        lin = lambda t, nm: F.linear(t, sd[p + nm + ".weight"], sd[p + nm + ".bias"])  # noqa: E731
        ln = lambda t, nm: F.layer_norm(t, (D,), sd[p + nm + ".weight"], sd[p + nm + ".bias"], eps)  # noqa: E731
        q, k, v = (lin(x, "attention.self." + nm).view(S, H, 64).transpose(0, 1) for nm in ("query", "key", "value"))
        pr = drop((q @ k.transpose(-1, -2) * 0.125).softmax(-1))
        a = (pr @ v).transpose(0, 1).reshape(S, D)
        h1 = ln(x + drop(lin(a, "attention.output.dense")), "attention.output.LayerNorm")
        x = ln(h1 + drop(lin(F.gelu(lin(h1, "intermediate.dense")), "output.dense")), "output.LayerNorm")
    pooled = torch.tanh(F.linear(x[:1], sd["body.pooler.dense.weight"], sd["body.pooler.dense.bias"]))
    rs = lambda t: F.layer_norm(F.linear(t, sd["resizer.fc.weight"], sd["resizer.fc.bias"]), (256,),  # noqa: E731
                                sd["resizer.layer_norm.weight"], sd["resizer.layer_norm.bias"], 1e-12)
    return drop(rs(x)).view(S, 1, 256), drop(rs(pooled))


def run_ref(case, dtype, masks=None):
    layers, vocab = CASES[case]
    proto = TextEncoder(TextConfig(vocab=vocab, layers=layers))
    synth.fill_module_(proto, skip_prefixes=())
    sd = {k: v.detach().to(dtype).requires_grad_(True) for k, v in proto.state_dict().items()}
    ids = torch.from_numpy(fixture(case)["input_ids"])
    mem, cls = ref_text(sd, ids, layers, masks)
    w1, w2 = loss_weights(case, ids.shape[0])
    ((mem * w1.to(dtype)).sum() + (cls * w2.to(dtype)).sum()).backward()
    return mem.detach(), cls.detach(), {k: v.grad.detach() for k, v in sd.items()}


def fixture_grads(case):
    """name -> (positions of the sample in the flat tensor, fp32 sample, fp64 sample, numel)"""
    f = fixture(case)
    k = int(f["grad_k"])
    out = {}
    for i, name in enumerate(f["grad_names"].tolist()):
        numel = int(f["grad_numel"][i])
        idx = synth.sample_indices(name, numel)
        idx = idx[synth.thinned_positions(idx.size, k)]
        a, b = int(f["grad_offsets"][i]), int(f["grad_offsets"][i + 1])
        assert b - a == idx.size
        out[name] = (idx, f["grad32"][a:b].astype(np.float64), f["grad64"][a:b].astype(np.float64), numel)
    return out


def rel_l2(a, g64):
    """tests/test_model_parity.py::_compare: relative L2 with the absolute floor GRAD_ABS_FLOOR sqrt(n) / GRAD_TOL in the norm"""
    floor = GRAD_ABS_FLOOR * g64.size ** 0.5 / GRAD_TOL
    return float(np.linalg.norm(a - g64)) / (float(np.linalg.norm(g64)) + floor)


def grad_rows(grads, case):
    """per tensor (name, e_hip, e_ref) against the fixture's fp64 gradients: the sample of every parameter, and the full
    rows of the two embedding tables at the ids in use"""
    f = fixture(case)
    rows = []
    ref = fixture_grads(case)
    assert set(grads) == set(ref), set(grads) ^ set(ref)
    for name, (idx, g32, g64, numel) in ref.items():
        assert grads[name].numel() == numel, name
        a = grads[name].reshape(-1)[torch.from_numpy(idx)].double().numpy()
        rows.append((name, rel_l2(a, g64), rel_l2(g32, g64)))
    for tag, name in (("word", "body.embeddings.word_embeddings.weight"), ("pos", "body.embeddings.position_embeddings.weight")):
        a = grads[name][torch.from_numpy(f[tag + "_rows"])].double().numpy().reshape(-1)
        g32, g64 = (f[f"{tag}_rows{b}"].astype(np.float64).reshape(-1) for b in (32, 64))
        rows.append((name + "[rows in use]", rel_l2(a, g64), rel_l2(g32, g64)))
    return rows


def check_fp32_class(rows, what):
    over = [(n, h, r) for n, h, r in rows if h > 3 * r + GRAD_TOL]
    assert not over, f"{what}: gradients further from fp64 than 3 e_ref + {GRAD_TOL}: " + "; ".join(
        f"{n}: hip {h:.2e} ref32 {r:.2e}" for n, h, r in over[:8])


def cap_16bit():
    """bf16x3p: 1.5 x the worst tensor measured (emulator and MI355X rows of profiles/text_encoder_grad_error.json), never
    above 2e-2 — the rule of GRAD_CAPS_16BIT (tests/test_model_parity.py)"""
    with open(os.path.join(ROOT, "profiles", "text_encoder_grad_error.json")) as fh:
        rows = json.load(fh)["rows"]
    return min(1.5 * max(max(r["e_hip"]) for r in rows if r["mode"] == "bf16x3p"), 2e-2)


def check_16bit(rows, what):
    cap = cap_16bit()
    over = [(n, h) for n, h, r in rows if h > cap]
    assert not over, f"{what}: gradient rel-L2 above the cap {cap:.3e}: {over[:8]}"


def _eval_parity(dev, case, mode):
    L.set_mma_mode(mode)
    try:
        m = build(case, dev)
        mem, cls, grads = run_module_grouped(m, case, dev)
    finally:
        L.set_mma_mode("f32")
    f = fixture(case)
    close(mem, torch.from_numpy(f["memory64"]), OUT_TOL, f"{case} [{mode}] memory", absolute=True)
    close(cls, torch.from_numpy(f["cls64"]), OUT_TOL, f"{case} [{mode}] cls", absolute=True)
    rows = grad_rows(grads, case)
    if mode == "bf16x3p":
        check_16bit(rows, f"{case} [{mode}]")
    else:
        check_fp32_class(rows, f"{case} [{mode}]")
    return rows


def test_state_dict_names_and_strict_load():
    for case, (layers, vocab) in CASES.items():
        m = TextEncoder(TextConfig(vocab=vocab, layers=layers))
        assert list(m.state_dict().keys()) == fixture(case)["keys"].tolist()
    m = TextEncoder(TextConfig(vocab=1024, layers=2))
    sd = {k: torch.zeros_like(v) for k, v in m.state_dict().items()}
    sd["body.embeddings.position_ids"] = torch.arange(514)[None]          # persistent buffers of older checkpoints
    sd["body.embeddings.token_type_ids"] = torch.zeros(1, 514, dtype=torch.long)
    m.load_state_dict(sd, strict=True)
    # ... and under the model's prefix
    holder = torch.nn.Module()
    holder.text_encoder = TextEncoder(TextConfig(vocab=1024, layers=2))
    holder.load_state_dict({"text_encoder." + k: v for k, v in sd.items()}, strict=True)
    with pytest.raises(RuntimeError):
        m.load_state_dict({k: v for k, v in sd.items() if k != "resizer.fc.bias"}, strict=True)


def test_geometry_is_checked():
    with pytest.raises(ValueError):
        TextConfig(hidden=1024, heads=16)
    with pytest.raises(ValueError):
        TextConfig(heads=8)

    class N:
        pass
    for name in ("bert-base", "roberta-large"):
        cfg = N()
        cfg.MODEL = N()
        cfg.MODEL.USE_LSTM = False
        cfg.MODEL.TEXT_MODEL = N()
        cfg.MODEL.TEXT_MODEL.NAME, cfg.MODEL.TEXT_MODEL.FREEZE = name, False
        with pytest.raises(ValueError):
            build_text_encoder(cfg)
    m = TextEncoder(TextConfig(vocab=1024, layers=1))
    with pytest.raises(AssertionError, match="b = 1"):
        m.forward_ids(torch.zeros(2, 4, dtype=torch.long), torch.ones(2, 4, dtype=torch.long))
    with pytest.raises(ValueError, match="128"):
        m.forward_ids(torch.zeros(1, 129, dtype=torch.long), torch.ones(1, 129, dtype=torch.long))


def test_restatement_is_pinned_to_the_fixtures():
    """the fp64 restatement of this file reproduces the reference's fp64 run to 1e-9: outputs and every gradient sample"""
    for case in CASES:
        mem, cls, grads = run_ref(case, torch.float64)
        f = fixture(case)
        assert float((mem - torch.from_numpy(f["memory64"])).abs().max()) < 1e-9
        assert float((cls - torch.from_numpy(f["cls64"])).abs().max()) < 1e-9
        for name, (idx, g32, g64, numel) in fixture_grads(case).items():
            a = grads[name].reshape(-1)[torch.from_numpy(idx)].numpy()
            assert float(np.abs(a - g64).max()) <= 1e-9 * max(1.0, float(np.abs(g64).max())), name


@both
def _eval_parity_T2(dev, big):
    for mode in ("f32", "bf16x6p", "bf16x3p"):
        _eval_parity(dev, "text_T2", mode)


@both
def _eval_parity_T2_L40(dev, big):
    for mode in ("f32", "bf16x6p", "bf16x3p"):
        _eval_parity(dev, "text_T2_L40", mode)


def _r12(dev, mode):
    """roberta-base geometry (12 layers, vocabulary 50265): ~2 GB of host memory on the emulator, hence the slot"""
    if dev.type == "cpu":
        with host_memory_slot():
            _eval_parity(dev, "text_R12", mode)
    else:
        _eval_parity(dev, "text_R12", mode)


@both
def _eval_parity_R12_f32(dev, big):
    _r12(dev, "f32")


@both
def _eval_parity_R12_bf16x6p(dev, big):
    _r12(dev, "bf16x6p")


@both
def _eval_parity_R12_bf16x3p(dev, big):
    _r12(dev, "bf16x3p")


def _train_masks(trace, seed, base, p, S, H=12):
    """the traced sites of one step -> multipliers in the order ref_text consumes them"""
    SP = ((S + 31) // 32) * 32
    out = []
    for off, n in trace:
        m = _mask_of(p, seed, base + off, n)
        if n == H * SP * SP:        # attention probabilities: counter ((h SP) + key) SP + query
            m = m.view(H, SP, SP)[:, :S, :S].transpose(-1, -2).contiguous()
        out.append(m)
    return out


@both
def _train_mode(dev, big):
    """train mode (p = 0.1 at every site) against the restatement fed the keep masks of the traced sites; same bars as eval.
    In the split-bf16 modes the checked step is the third of three under launch plans — eager, recorded, REPLAYED — on the
    grouped path: the replayed node draws its masks from the same host offsets and the device base of its own step."""
    case = "text_T2"
    S = fixture(case)["input_ids"].shape[0]
    for mode in ("f32", "bf16x6p", "bf16x3p"):
        planned = mode != "f32"
        L.set_mma_mode(mode)
        plans.clear()
        plans.enable(planned)
        plans.STATS.update(recorded=0, replayed=0, eager=0, run_s=0.0, refused=0)
        try:
            ops.manual_seed(1234)
            m = build(case, dev, train=True)
            seed = ops.dropout_stream_state()[0]
            with grouped_path(dev) as gp:
                for k in range(3 if planned else 1):
                    gp.arena.reset()
                    ops.dropout_begin_step(dev)
                    trace = ops.dropout_trace(True) if k == 0 else None
                    base = int(ops._dropout_stream.base(dev).item())
                    mem, cls, grads = run_module(m, case, dev)
                    if k == 0:
                        sites = list(trace)
                        ops.dropout_trace(False)
            if planned:
                assert gp.taken(CASES[case][0], 2), gp.count          # (a replay runs no Python: two counted steps)
                assert plans.STATS["replayed"] == 2 and not plans.STATS["refused"], plans.STATS
        finally:
            ops.dropout_trace(False)
            plans.enable(False)
            plans.clear()
            L.set_mma_mode("f32")
        assert len(sites) == 1 + 3 * CASES[case][0] + 2, sites          # every site is visible to the trace
        masks = _train_masks(sites, seed, base, 0.1, S)
        mem64, cls64, g64 = run_ref(case, torch.float64, masks)
        _, _, g32 = run_ref(case, torch.float32, masks)
        close(mem, mem64, OUT_TOL, f"train [{mode}] memory", absolute=True)
        close(cls, cls64, OUT_TOL, f"train [{mode}] cls", absolute=True)
        assert float((mem == 0).float().mean()) > 0.05                   # the resizer's dropout did act
        rows = [(n, rel_l2(grads[n].double().numpy().reshape(-1), g64[n].numpy().reshape(-1)),
                 rel_l2(g32[n].double().numpy().reshape(-1), g64[n].numpy().reshape(-1))) for n in g64]
        if mode == "bf16x3p":
            check_16bit(rows, f"train [{mode}]")
        else:
            check_fp32_class(rows, f"train [{mode}]")


def _steps(dev, case, n, use_plans, train, lengths=None, layers=1):
    """n steps of a `layers`-deep module on the fixture's ids (or on their first `lengths[k]` tokens) -> [(mem, cls, grads)];
    one layer holds every kind of launch of the node and keeps the emulator twins short"""
    ids_all = torch.from_numpy(fixture(case)["input_ids"])
    plans.clear()
    plans.enable(use_plans)
    plans.STATS.update(recorded=0, replayed=0, eager=0, run_s=0.0, refused=0)
    arena = ops.enable_zero_arena(dev, 1 << 23)      # the eager steps take the same skinny / grouped launches as the plans
    out = []
    try:
        ops.manual_seed(5)
        m = build(case, dev, train=train, layers=layers)
        for k in range(n):
            S = ids_all.shape[0] if lengths is None else lengths[k]
            ids = torch.cat([ids_all[:S - 1], ids_all[-1:]])[None]
            for p in m.parameters():
                p.grad = None
            arena.reset()
            ops.dropout_begin_step(dev)
            (_, mem, _), cls = m.forward_ids(ids, torch.ones_like(ids))
            w1, w2 = loss_weights(case, S)
            ((mem * w1.to(dev)).sum() + (cls * w2.to(dev)).sum()).backward()
            out.append((mem.detach().cpu().clone(), cls.detach().cpu().clone(),
                        {nm: p.grad.detach().cpu().clone() for nm, p in m.named_parameters()}))
        return out, dict(plans.STATS)
    finally:
        ops.disable_zero_arena()
        plans.enable(False)
        plans.clear()


def _same_bits(a, b, what):
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), what + ": outputs differ"
    assert set(a[2]) == set(b[2])
    bad = [n for n in a[2] if not torch.equal(a[2][n], b[2][n])]
    assert not bad, f"{what}: {len(bad)} gradients differ, e.g. {bad[:4]}"


@both
def _launch_plan(dev, big):
    """deterministic mode: the recorded and the replayed node equal the eager node bit for bit; a second length records its
    own plan; nothing is refused"""
    L.set_mma_mode("bf16x6p")
    L.set_deterministic(True)
    try:
        lengths = [9, 9, 9, 6, 6]
        eager, _ = _steps(dev, "text_T2", len(lengths), False, False, lengths)
        planned, stats = _steps(dev, "text_T2", len(lengths), True, False, lengths)
        for k, (a, b) in enumerate(zip(eager, planned)):
            _same_bits(a, b, f"step {k} (L = {lengths[k]})")
        assert not stats.get("refused"), stats
        assert stats["recorded"] == 4 and stats["replayed"] == 2, stats      # two lengths x (forward + backward); L = 9 replayed once
    finally:
        L.set_deterministic(False)
        L.set_mma_mode("f32")


@both
def _deterministic_mode(dev, big):
    """two fresh train-mode runs from one seed: every gradient, the embedding tables included, has the same bits"""
    L.set_mma_mode("bf16x6p")
    L.set_deterministic(True)
    try:
        a, _ = _steps(dev, "text_T2", 2, False, True)
        b, _ = _steps(dev, "text_T2", 2, False, True)
        for k in range(2):
            _same_bits(a[k], b[k], f"step {k}")
        assert not torch.equal(a[0][0], a[1][0])          # (a new step draws new masks)
    finally:
        L.set_deterministic(False)
        L.set_mma_mode("f32")


# ---------------------------------------------------------------------------------------
# inside the grounding model: a tiny clip (T = 2, 64 x 64, one bottleneck per ResNet stage)
# ---------------------------------------------------------------------------------------
TINY_T, TINY_RES = 2, 64
# gradients that are zero by construction: the key biases (softmax shift invariance) and the pooler, whose output `cls`
# the grounding model receives and never reads (models/pipeline.py:69-79, query_decoder.py:83-98)
ZERO_BY_CONSTRUCTION = ("attention.self.key.bias", "body.pooler.")


def _tiny_tokenizer(texts):
    ids = torch.from_numpy(fixture("text_T2")["input_ids"])[None]
    return ids, torch.ones_like(ids)


def _tiny_model(dev, text_encoder, train=False):
    from stcat_amd import backbone
    from stcat_amd.pipeline import build_model
    saved = backbone.BLOCKS
    backbone.BLOCKS = (1, 1, 1, 1)
    try:
        model, criterion, wd = build_model(None, text_encoder)
    finally:
        backbone.BLOCKS = saved
    synth.fill_module_(model)               # (skips text_encoder.*: filled by build())
    return model.to(dev).train(train), criterion, wd


def _tiny_step(model, criterion, wd, dev, seed=0, reset=True):
    from stcat_amd.misc import BoxList, NestedTensor
    for p in model.parameters() if reset else ():      # (a gradient reducer owns the gradients: reset=False)
        p.grad = None
    frames = synth.synth_frames(TINY_T, TINY_RES, seed=seed).to(dev)
    mask = torch.zeros(TINY_T, TINY_RES, TINY_RES, dtype=torch.bool, device=dev)
    out = model(NestedTensor(frames, mask, [TINY_T]), ["synthetic"])
    act, tb = synth.synth_targets(TINY_T, seed=seed)
    targets = [{"actioness": act.to(dev), "boxs": BoxList(tb).to(dev)}]
    plan = criterion.plan(targets, [TINY_T], dev)
    plan._num_boxes = max(plan.num_boxes_local, 1.0)
    criterion(out, targets, [TINY_T], plan=plan)
    criterion.weighted_total(wd).backward()
    return {k: out[k].detach().cpu().clone() for k in ("pred_boxes", "pred_sted", "pred_actioness", "weights")}


class _Cfg:
    pass


def _solver_cfg():
    cfg = _Cfg()
    cfg.SOLVER = _Cfg()
    cfg.SOLVER.OPTIMIZER, cfg.SOLVER.BASE_LR, cfg.SOLVER.VIS_BACKBONE_LR = "adamw", 1e-4, 1e-5
    cfg.SOLVER.TEXT_LR, cfg.SOLVER.TEMP_LR, cfg.SOLVER.WEIGHT_DECAY = 2e-5, 1e-4, 1e-4
    return cfg


@both
def _integration_tiny_clip(dev, big):
    from stcat_amd import optim
    from stcat_amd.pipeline import SyntheticText
    L.set_mma_mode("f32")
    L.set_deterministic(True)         # two forward passes are compared bit for bit
    try:
        enc = build("text_T2", dev, tokenizer=_tiny_tokenizer)
        model, criterion, wd = _tiny_model(dev, enc)
        outs = _tiny_step(model, criterion, wd, dev)
        grads = {n: p.grad for n, p in model.named_parameters() if n.startswith("text_encoder.")}
        assert len(grads) == len(list(enc.parameters()))
        for n, g in grads.items():
            if any(z in n for z in ZERO_BY_CONSTRUCTION):
                assert g is None or float(g.abs().max()) < 1e-6, n
            else:
                assert g is not None and float(g.abs().max()) > 0.0, f"{n} has no gradient"
        ids = fixture("text_T2")["input_ids"]
        gw = grads["text_encoder.body.embeddings.word_embeddings.weight"].cpu()
        unused = torch.ones(gw.shape[0], dtype=torch.bool)
        unused[torch.from_numpy(ids)] = False
        assert float(gw[unused].abs().max()) == 0.0 and float(gw[~unused].abs().min(1).values.min()) >= 0.0
        assert all(float(gw[i].abs().max()) > 0.0 for i in set(ids.tolist()))
        # the optimizer takes a step over the text group (SOLVER.TEXT_LR)
        before = enc.body.encoder.layer[0].intermediate.dense.weight.detach().clone()
        opt = optim.make_optimizer(_solver_cfg(), model)
        assert sum(p.numel() for p in opt.param_groups[2]["params"]) == sum(p.numel() for p in enc.parameters())
        opt.step(max_grad_norm=0.1)
        assert not torch.equal(before, enc.body.encoder.layer[0].intermediate.dense.weight.detach())
        # the same net fed this encoder's own outputs as constants gives the same bits
        enc2 = build("text_T2", dev, tokenizer=_tiny_tokenizer)
        with torch.no_grad():
            (mask, mem, _), cls = enc2(["synthetic"], dev)
        model2, criterion2, wd2 = _tiny_model(dev, SyntheticText(((mask, mem, None), cls)))
        outs2 = _tiny_step(model2, criterion2, wd2, dev)
        for k in outs:
            assert torch.equal(outs[k], outs2[k]), k
        # a frozen body: only the resizer trains
        encf = build("text_T2", dev, freeze=True, tokenizer=_tiny_tokenizer)
        modelf, criterionf, wdf = _tiny_model(dev, encf)
        outsf = _tiny_step(modelf, criterionf, wdf, dev)
        for k in outs:
            assert torch.equal(outs[k], outsf[k]), k
        got = sorted(n for n, p in encf.named_parameters() if p.grad is not None)
        assert got == sorted(n for n, _ in encf.named_parameters() if n.startswith("resizer.")), got
        for n, p in encf.resizer.named_parameters():
            assert torch.equal(p.grad, grads["text_encoder.resizer." + n]), n
    finally:
        L.set_deterministic(False)


def test_install_rebinds_the_text_factory_on_request():
    import sys
    import types

    import stcat_amd
    names = ("models", "models.pipeline", "models.vision_model", "models.grounding_model", "models.language_model")
    saved = {k: sys.modules.get(k) for k in names}
    try:
        for flag in (False, True):
            for name in names:
                sys.modules[name] = types.ModuleType(name)
            sentinel = object()
            sys.modules["models.pipeline"].build_text_encoder = sentinel
            sys.modules["models.language_model"].build_text_encoder = sentinel
            stcat_amd.install(text_encoder=True) if flag else stcat_amd.install()
            from stcat_amd.backbone import build_vis_encoder
            assert sys.modules["models.pipeline"].build_vis_encoder is build_vis_encoder
            for name in ("models.pipeline", "models.language_model"):
                assert (sys.modules[name].build_text_encoder is build_text_encoder) == flag
                assert (sys.modules[name].build_text_encoder is sentinel) != flag
    finally:
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _dp_worker(rank, world, port, q):
    try:
        _dp_body(rank, world, port, q)
    except BaseException as e:              # the parent reports it instead of waiting for the queue
        q.put((rank, float("inf"), f"{type(e).__name__}: {e}", 0))
        raise


def _dp_body(rank, world, port, q):
    import torch.distributed as dist
    from stcat_amd.dist import GradBucketReducer
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    dev = torch.device("cuda:0")
    L.load()
    L.set_mma_mode("bf16x6p")
    enc = build("text_T2", dev, tokenizer=_tiny_tokenizer)
    model, criterion, wd = _tiny_model(dev, enc)         # eval mode: the two schedules must see the same arithmetic
    red = GradBucketReducer(model)
    red.zero_grad()
    _tiny_step(model, criterion, wd, dev, 100 + rank, reset=False)
    red.finish()
    torch.cuda.synchronize()
    got = {n: p.grad.detach().clone() for n, p in model.named_parameters() if p.grad is not None}
    red.close()
    red.deferred = True
    ref = {}
    for r in range(world):
        for p in model.parameters():
            p.grad = None
        _tiny_step(model, criterion, wd, dev, 100 + r, reset=False)
        for n, p in model.named_parameters():
            if p.grad is not None:
                ref[n] = ref.get(n, 0) + p.grad.detach() / world
    assert set(got) == set(ref), sorted(set(got) ^ set(ref))[:6]
    typical = float(torch.stack([ref[n].norm() / ref[n].numel() ** 0.5 for n in ref]).median())
    worst, worst_n, n_text = 0.0, "", 0
    for n in ref:
        if not n.startswith("text_encoder."):
            continue
        n_text += 1
        scale = max(float(ref[n].norm()), typical * ref[n].numel() ** 0.5)
        err = float((got[n] - ref[n]).norm()) / scale
        if err > worst:
            worst, worst_n = err, n
    q.put((rank, worst, worst_n, n_text))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.gpu
def test_gpu_two_rank_text_gradients_equal_single_process_mean():
    """two ranks over gloo on the one GPU, the tiny model with the native text encoder (tests/test_dp_model.py's pattern
    and bar): the reduced text-encoder gradients equal the mean of the two single-process gradients"""
    import torch.multiprocessing as mp
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_dp_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    out = [q.get(timeout=120) for _ in procs]
    for p in procs:
        p.join(timeout=60)
    for rank, worst, name, n_text in out:
        assert worst < 1e-2, (rank, worst, name)
    assert all(p.exitcode == 0 for p in procs)
    for rank, worst, name, n_text in out:
        assert n_text == 2 * 16 + 5 + 2 + 4, n_text        # every text tensor (the unread pooler's gradients are zeros)
        assert worst < 1e-2, (rank, worst, name)
