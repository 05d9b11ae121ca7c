"""Native text encoder: RoBERTa + FeatureResizer (models/language_model/bert.py:42-96) as ONE composite node.

``TextEncoder`` has the module tree and state-dict names of the reference's ``Roberta`` (``body.*`` = HuggingFace
``RobertaModel``, ``resizer.*`` = ``FeatureResizer``), so the ``text_encoder.*`` entries of a zoo checkpoint load strictly;
nothing here imports ``transformers``.  ``TextEncoderFn`` is a launch sequence with a hand-written backward over the C ABI
(csrc/text_encoder.h: embedding gather + LayerNorm, attention at head dimension 64, erf-GELU; LayerNorm at D = 768 and the
Linear GEMMs are the kernels of the rest of the model), recorded into a launch plan and replayed like the other nodes.
None of its own kernels uses a float atomic, so the node runs unchanged in deterministic mode.

Limits: one text per call (b = 1, the project's rule), at most 128 tokens, hidden / heads = 64 (roberta-base geometry).
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Callable, Optional

import torch
import torch.nn as nn
from torch.autograd import Function

from . import _lib as L
from . import composite as C
from . import ops, plans

MAX_TOKENS = 128


@dataclass(frozen=True)
class TextConfig:
    """geometry of the encoder; the default is roberta-base"""
    vocab: int = 50265
    max_pos: int = 514
    layers: int = 12
    hidden: int = 768
    heads: int = 12
    ffn: int = 3072
    eps: float = 1e-5
    p: float = 0.1
    pad_id: int = 1
    out: int = 256

    def __post_init__(self):
        if self.hidden != 768 or self.hidden % self.heads != 0 or self.hidden // self.heads != 64:
            raise ValueError(f"TextEncoder: hidden = {self.hidden}, heads = {self.heads}: the kernels are built for "
                             "hidden = 768 and a head dimension of 64 (roberta-base)")
        if self.ffn % 128 != 0 or self.out != 256:
            raise ValueError("TextEncoder: ffn must be a multiple of 128 and the resized width 256")


ROBERTA_BASE = TextConfig()


def config_for(name: str) -> TextConfig:
    """MODEL.TEXT_MODEL.NAME -> geometry; only roberta-base has native kernels"""
    if name == "roberta-base":
        return ROBERTA_BASE
    raise ValueError(f"TextEncoder: text model {name!r} is not supported (roberta-base only: bert-base has another "
                     "embedding scheme, roberta-large a hidden size of 1024)")


# ------------------------------------------------------------------------------------------------------------------
# the node
# ------------------------------------------------------------------------------------------------------------------
_N_EMB, _N_LAYER = 5, 16


def _layer_f(x, kpm, H, eps, p, keep, Wq, bq, Wk, bk, Wv, bv, Wo, bo, g1, be1, Wi, bi, Wo2, bo2, g2, be2):
    """one RobertaLayer on x [S,768] (post-LN): self-attention, output + norm, GELU FFN + norm"""
    S, D = x.shape
    multi = ops.linear_multi_ok(S, D, D, x)
    if multi:      # the three projections as ONE grouped launch
        q, k, v = (ops._zeros(x, S, D) for _ in range(3))      # (_zeros: a full arena falls back to a fill launch)
        ops.linear_fwd_multi([x, x, x], [Wq, Wk, Wv], [bq, bk, bv], [q, k, v], S, D, D)
    else:
        q, k, v = (C._lin_f(x, W, b)[0] for W, b in ((Wq, bq), (Wk, bk), (Wv, bv)))
    att = ops._empty(x, S, D)
    P = ops._empty(x, H, S, S) if keep else None
    SP = ((S + 31) // 32) * 32
    drop = ops._drop_args(p, H * SP * SP, x.device)
    L.call("stcat_mha_d64_fwd", q.data_ptr(), k.data_ptr(), v.data_ptr(), L._ptr(kpm), att.data_ptr(), L._ptr(P), 1, H, S,
           D, D, D, D, 0.125, *drop, L.stream_of(x))
    h1, st1 = C._outln_f(att, Wo, bo, x, g1, be1, p, eps)
    i1, x_i = C._lin_f(h1, Wi, bi)
    a1 = ops.ew(L.EW_GELU, i1)
    y, st2 = C._outln_f(a1, Wo2, bo2, h1, g2, be2, p, eps)
    return y, (x, q, k, v, P, drop, H, st1, x_i, i1, st2, (Wq, Wk, Wv, Wi), multi)


def _layer_b(st, dy, need_x):
    """-> (d_x | None, the 16 parameter gradients in parameter order)"""
    x, q, k, v, P, drop, H, st1, x_i, i1, st2, (Wq, Wk, Wv, Wi), multi = st
    S, D = x.shape
    d_a1, d_h1r, dWo2, dbo2, dg2, dbe2 = C._outln_b(st2, dy)
    d_i1 = ops.ew(L.EW_GELU_BWD, d_a1, i1)
    d_h1, dWi, dbi, _ = C._lin_b(d_i1, x_i, Wi, add=d_h1r)
    d_att, d_xr, dWo, dbo, dg1, dbe1 = C._outln_b(st1, d_h1)
    d_att = d_att if d_att.is_contiguous() else d_att.contiguous()
    dq, dk, dv = ops._empty(x, S, D), ops._empty(x, S, D), ops._empty(x, S, D)
    delta = ops._empty(x, H, S)
    L.call("stcat_mha_d64_bwd", q.data_ptr(), k.data_ptr(), v.data_ptr(), d_att.data_ptr(), P.data_ptr(), delta.data_ptr(),
           dq.data_ptr(), dk.data_ptr(), dv.data_ptr(), 1, H, S, D, D, D, D, D, D, 0.125, *drop, L.stream_of(x))
    d_xr = d_xr.reshape(S, D)
    d_xr = d_xr if d_xr.is_contiguous() else d_xr.contiguous()
    if multi:
        d_x = None
        if need_x:
            d_x = ops._zeros(x, S, D)
            ops.linear_dgrad_multi([dq, dk, dv], [Wq, Wk, Wv], [d_xr, None, None], [d_x, d_x, d_x], S, D, D)
        dWs = [ops._zeros(x, D, D) for _ in range(3)]
        dbs = [ops._zeros(x, D) for _ in range(3)]
        C._wgrad_multi([dq, dk, dv], [x, x, x], dWs, dbs, S, D, D)
    else:
        d_x = d_xr if need_x else None
        dWs, dbs = [], []
        for g, W in ((dq, Wq), (dk, Wk), (dv, Wv)):
            d_x, dW, db, _ = C._lin_b(g, x, W, need_dx=need_x, add=d_x)
            dWs.append(dW)
            dbs.append(db)
    return d_x, (dWs[0], dbs[0], dWs[1], dbs[1], dWs[2], dbs[2], dWo, dbo, dg1, dbe1, dWi, dbi, dWo2, dbo2, dg2, dbe2)


class TextEncoderFn(Function):
    """(input_ids [L] int64, position_ids [L] int64, key padding [1,L] bytes | None, p, heads, layers, eps, frozen body,
    padding_idx, *parameters) -> (memory [L,256], cls [1,256]): RobertaModel (embeddings, `layers` post-LN layers, tanh pooler) and the
    FeatureResizer applied to the last hidden state and to the pooled [CLS] (bert.py:59-74).  Parameters: 5 of the
    embeddings, 16 per layer, pooler weight / bias, resizer fc weight / bias and LayerNorm weight / bias."""

    @staticmethod
    def forward(ctx, ids, pos_ids, kpm, p, H, nl, eps, frozen, pad, *prm):
        S = ids.shape[0]
        word, pos, typ, eg, eb = prm[:_N_EMB]
        Wp, bp, Wr, br, gr, ber = prm[_N_EMB + nl * _N_LAYER:]
        V, D = word.shape
        dev = word.device
        like = eg
        keep = (not frozen) and any(ctx.needs_input_grad)
        ctx.set_materialize_grads(False)      # an output nobody consumed (the grounding model ignores cls) costs nothing
        drop_e = ops._drop_args(p, S * D, dev)
        x = ops._empty(like, S, D)
        mean, rstd = ops._empty(like, S), ops._empty(like, S)
        L.call("stcat_embed_ln_fwd", ids.data_ptr(), pos_ids.data_ptr(), word.data_ptr(), pos.data_ptr(), typ.data_ptr(),
               eg.data_ptr(), eb.data_ptr(), x.data_ptr(), mean.data_ptr(), rstd.data_ptr(), S, D, V, pos.shape[0], eps,
               *drop_e, L.stream_of(like))
        states = []
        for i in range(nl):
            lp = prm[_N_EMB + i * _N_LAYER:_N_EMB + (i + 1) * _N_LAYER]
            x, st = _layer_f(x, kpm, H, eps, p, keep, *lp)
            states.append(st if keep else None)
        # pooler: tanh(dense(hidden[0]))  (RobertaPooler)
        pl, x_p = C._lin_f(x[:1], Wp, bp)
        pooled = ops.ew(L.EW_TANH, pl)
        # FeatureResizer on the memory and on the pooled [CLS]: fc -> LayerNorm(eps 1e-12) -> dropout, each its own site
        outs, tails = [], []
        for t in (x, pooled):
            h, x_r = C._lin_f(t, Wr, br)
            y, s_n = ops.layernorm_fwd_raw(h, None, gr, ber, 1e-12)
            s_d = None
            if p > 0.0:
                y, s_d = ops.dropout_fwd_raw(y, None, p)
            outs.append(y)
            tails.append((x_r, s_n, s_d))
        ctx.save_for_backward(ids, pos_ids, mean, rstd, pooled, *prm)
        ctx.misc = (states, tails, x_p, drop_e, nl, eps, frozen, pad)
        return outs[0], outs[1]

    @staticmethod
    def backward(ctx, d_mem, d_cls):
        ids, pos_ids, mean, rstd, pooled, *prm = ctx.saved_tensors
        states, tails, x_p, drop_e, nl, eps, frozen, pad = ctx.misc
        word, pos, typ, eg, eb = prm[:_N_EMB]
        Wp, bp, Wr, br, gr, ber = prm[_N_EMB + nl * _N_LAYER:]
        like = eg
        S, D = ids.shape[0], word.shape[1]
        n_body = _N_EMB + nl * _N_LAYER + 2
        grads = [None] * len(prm)
        with C.wgrad_batch(like):
            # resizer (shared weights: the two applications accumulate into one set of gradient buffers)
            dWr, dbr = ops._zeros(like, *Wr.shape), ops._zeros(like, Wr.shape[0])
            dgr = dber = None
            d_in = []
            for (x_r, s_n, s_d), g in zip(tails, (d_mem, d_cls)):
                if g is None:
                    d_in.append(None)
                    continue
                g = g if g.is_contiguous() else g.contiguous()
                if s_d is not None:
                    g = ops.dropout_bwd_raw(s_d, g)[0]
                r = ops.layernorm_bwd_raw(s_n, g)
                dgr = r[2] if dgr is None else ops.ew(L.EW_ADD, dgr, r[2], out=dgr)
                dber = r[3] if dber is None else ops.ew(L.EW_ADD, dber, r[3], out=dber)
                d_t, _, _, _ = C._lin_b(r[0], x_r, Wr, need_dx=not frozen, dw=dWr, db=dbr)
                d_in.append(d_t)
            grads[n_body:] = [dWr, dbr, dgr, dber]
            if not frozen:
                d_x, d_pooled = d_in
                if d_x is None:
                    d_x = ops._zeros(like, S, D)
                if d_pooled is not None:
                    d_pl = ops.ew(L.EW_TANH_BWD, d_pooled, pooled)
                    d_x0, dWp, dbp, _ = C._lin_b(d_pl, x_p, Wp, add=d_x[:1])
                    ops.ew2d(L.EW_COPY, d_x0, out=d_x[:1])
                    grads[n_body - 2:n_body] = [dWp, dbp]
                else:      # cls unread (the grounding model): a zero gradient, so a gradient reducer sees every parameter
                    grads[n_body - 2:n_body] = [ops._zeros(like, *Wp.shape), ops._zeros(like, Wp.shape[0])]
                for i in reversed(range(nl)):
                    d_x, lg = _layer_b(states[i], d_x, True)
                    grads[_N_EMB + i * _N_LAYER:_N_EMB + (i + 1) * _N_LAYER] = lg
                    C.wgrad_flush(like)
                # embeddings: LayerNorm backward, then the three table gradients by a gather (csrc/text_encoder.h)
                de = ops._empty(like, S, D)
                dword, dpos = ops._zeros(like, *word.shape), ops._zeros(like, *pos.shape)
                dtyp, dg, dbe = ops._zeros(like, *typ.shape), ops._zeros(like, D), ops._zeros(like, D)
                d_x = d_x if d_x.is_contiguous() else d_x.contiguous()
                L.call("stcat_embed_ln_bwd", d_x.data_ptr(), ids.data_ptr(), pos_ids.data_ptr(), word.data_ptr(),
                       pos.data_ptr(), typ.data_ptr(), eg.data_ptr(), mean.data_ptr(), rstd.data_ptr(), de.data_ptr(),
                       dword.data_ptr(), dpos.data_ptr(), dtyp.data_ptr(), dg.data_ptr(), dbe.data_ptr(), S, D,
                       word.shape[0], pos.shape[0], pad, *drop_e, L.stream_of(like))
                grads[:_N_EMB] = [dword, dpos, dtyp, dg, dbe]
        if not getattr(ctx, "static", False):
            ctx.misc = None
        return (None,) * 9 + tuple(g if ctx.needs_input_grad[9 + i] else None for i, g in enumerate(grads))


# ------------------------------------------------------------------------------------------------------------------
# the module tree of the reference's Roberta (parameter containers: the arithmetic is the node above)
# ------------------------------------------------------------------------------------------------------------------
def _linear(i, o):
    return nn.Linear(i, o)


class _Embeddings(nn.Module):
    def __init__(self, c: TextConfig):
        super().__init__()
        # (registration order = RobertaEmbeddings', so state_dict() lists the keys as the reference does)
        self.word_embeddings = nn.Embedding(c.vocab, c.hidden, padding_idx=c.pad_id)
        self.token_type_embeddings = nn.Embedding(1, c.hidden)
        self.LayerNorm = nn.LayerNorm(c.hidden, eps=c.eps)
        self.position_embeddings = nn.Embedding(c.max_pos, c.hidden, padding_idx=c.pad_id)


class _SelfAttention(nn.Module):
    def __init__(self, c):
        super().__init__()
        self.query, self.key, self.value = _linear(c.hidden, c.hidden), _linear(c.hidden, c.hidden), _linear(c.hidden, c.hidden)


class _Output(nn.Module):
    def __init__(self, i, o, eps):
        super().__init__()
        self.dense = _linear(i, o)
        self.LayerNorm = nn.LayerNorm(o, eps=eps)


class _Attention(nn.Module):
    def __init__(self, c):
        super().__init__()
        self.self = _SelfAttention(c)
        self.output = _Output(c.hidden, c.hidden, c.eps)


class _Dense(nn.Module):
    def __init__(self, i, o):
        super().__init__()
        self.dense = _linear(i, o)


class _Layer(nn.Module):
    def __init__(self, c):
        super().__init__()
        self.attention = _Attention(c)
        self.intermediate = _Dense(c.hidden, c.ffn)
        self.output = _Output(c.ffn, c.hidden, c.eps)

    def params(self):
        a, o = self.attention, self.output
        s = a.self
        return [s.query.weight, s.query.bias, s.key.weight, s.key.bias, s.value.weight, s.value.bias,
                a.output.dense.weight, a.output.dense.bias, a.output.LayerNorm.weight, a.output.LayerNorm.bias,
                self.intermediate.dense.weight, self.intermediate.dense.bias, o.dense.weight, o.dense.bias,
                o.LayerNorm.weight, o.LayerNorm.bias]


class _Stack(nn.Module):
    def __init__(self, c):
        super().__init__()
        self.layer = nn.ModuleList(_Layer(c) for _ in range(c.layers))


class _Body(nn.Module):
    """HuggingFace RobertaModel's names"""

    def __init__(self, c):
        super().__init__()
        self.embeddings = _Embeddings(c)
        self.encoder = _Stack(c)
        self.pooler = _Dense(c.hidden, c.hidden)


class _Resizer(nn.Module):
    """FeatureResizer (bert.py:77-96): fc -> LayerNorm(eps 1e-12) -> dropout(0.1)"""

    def __init__(self, i, o):
        super().__init__()
        self.fc = _linear(i, o)
        self.layer_norm = nn.LayerNorm(o, eps=1e-12)


# persistent buffers of older transformers releases: not parameters of the model, dropped when a checkpoint is loaded
_DROPPED = ("body.embeddings.position_ids", "body.embeddings.token_type_ids")


class TextEncoder(plans.InvalidatesPlans, nn.Module):
    """Drop-in for the reference's `Roberta(name, outdim, freeze)`; `tokenizer` is any callable
    `texts -> (input_ids [b,L] int64, attention_mask [b,L])` (RobertaTokenizerFast, wrapped, satisfies it)."""

    def __init__(self, config: TextConfig = ROBERTA_BASE, tokenizer: Optional[Callable] = None, freeze: bool = False):
        super().__init__()
        self.config = config
        self.tokenizer = tokenizer
        self.freeze = bool(freeze)
        self.body = _Body(config)
        self.resizer = _Resizer(config.hidden, config.out)
        if self.freeze:
            for q in self.body.parameters():
                q.requires_grad_(False)

    def _load_from_state_dict(self, state_dict, prefix, *a, **k):
        for name in _DROPPED:          # (as FrozenBatchNorm2d drops num_batches_tracked)
            state_dict.pop(prefix + name, None)
        super()._load_from_state_dict(state_dict, prefix, *a, **k)

    def _params(self):
        e = self.body.embeddings
        prm = [e.word_embeddings.weight, e.position_embeddings.weight, e.token_type_embeddings.weight,
               e.LayerNorm.weight, e.LayerNorm.bias]
        for layer in self.body.encoder.layer:
            prm += layer.params()
        prm += [self.body.pooler.dense.weight, self.body.pooler.dense.bias, self.resizer.fc.weight, self.resizer.fc.bias,
                self.resizer.layer_norm.weight, self.resizer.layer_norm.bias]
        return prm

    def forward_ids(self, input_ids: torch.Tensor, attention_mask: torch.Tensor):
        """-> ((mask [b,L] bool, True = padding, memory [L,b,256], None), cls [b,256])"""
        c = self.config
        assert input_ids.dim() == 2 and input_ids.shape[0] == 1, \
            f"TextEncoder: b = 1 only (one video and one sentence per rank), got a batch of {tuple(input_ids.shape)}"
        S = input_ids.shape[1]
        if S > MAX_TOKENS:
            raise ValueError(f"TextEncoder: {S} tokens, the attention kernel stops at {MAX_TOKENS}")
        dev = self.resizer.fc.weight.device
        # host side: the ids are checked against the vocabulary BEFORE any kernel sees them, and RoBERTa's position ids
        # cumsum(mask) * mask + padding_idx are computed here (create_position_ids_from_input_ids)
        ids = input_ids.detach().to("cpu", torch.int64)
        am = attention_mask.detach().to("cpu", torch.int64)
        pos_ids = torch.cumsum(am, 1) * am + c.pad_id
        ops.check_token_ids(ids, c.vocab, pos_ids, c.max_pos)
        pad = am.ne(1)
        kpm = pad.to(torch.uint8).to(dev) if bool(pad.any()) else None
        train = self.training
        mem, cls = plans.apply(TextEncoderFn, ids[0].to(dev), pos_ids[0].to(dev), kpm, c.p if train else 0.0, c.heads,
                               c.layers, c.eps, self.freeze, c.pad_id, *self._params())
        return (pad.to(dev), mem.view(S, 1, c.out), None), cls

    def forward(self, texts, device=None):
        if self.tokenizer is None:
            raise RuntimeError("TextEncoder: no tokenizer was given (build_text_encoder(cfg, tokenizer=...)); "
                               "forward_ids(input_ids, attention_mask) takes token ids directly")
        tok = self.tokenizer(texts)
        input_ids, attention_mask = (tok["input_ids"], tok["attention_mask"]) if hasattr(tok, "keys") else tok
        (mask, mem, _), cls = self.forward_ids(torch.as_tensor(input_ids), torch.as_tensor(attention_mask))
        return (mask, mem, tok), cls


def build_text_encoder(cfg=None, tokenizer: Optional[Callable] = None) -> TextEncoder:
    """The fourth factory of the seam (models/language_model/__init__.py): cfg = None builds roberta-base, trainable."""
    if cfg is None:
        return TextEncoder(ROBERTA_BASE, tokenizer)
    if getattr(cfg.MODEL, "USE_LSTM", False):
        raise ValueError("TextEncoder: MODEL.USE_LSTM is not supported (the LSTM encoder has no native form)")
    return TextEncoder(config_for(cfg.MODEL.TEXT_MODEL.NAME), tokenizer, freeze=cfg.MODEL.TEXT_MODEL.FREEZE)
