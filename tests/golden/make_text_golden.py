"""Fixtures of the native text encoder (tests/golden/text_*.npz) — runs in the build container only.

The reference's own `Roberta` / `FeatureResizer` (models/language_model/bert.py:42-96) around the real
`transformers.RobertaModel` (random-init from a `RobertaConfig`: `from_pretrained` is patched, nothing is downloaded),
filled with the synthetic weights of `stcat_amd.synth` (a function of the parameter NAME), run in eval mode in fp32 and in
fp64.  Loss = sum(w1 * memory) + sum(w2 * cls) with w1, w2 from `synth.hash_normal`.

Each file keeps: the ordered state-dict key list, the token ids, memory / cls (fp64 and fp32), and for every parameter the
`synth.sample_indices` sample of its fp32 and fp64 gradient (thinned to at most `k` elements per tensor where the file
would pass 1 MiB), plus — the sample of a [50265, 768] table almost never meets one of the dozen rows that have a
gradient — the full gradient rows of the two embedding tables at the ids in use.

    python tests/golden/make_text_golden.py            # all cases
"""
import os
import sys
import types

import numpy as np
import torch

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), "..", ".."))
REF = "/root/reference"
sys.path.insert(0, REPO)

from stcat_amd import synth  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))

# case -> (layers, vocab, thinning of the gradient samples)
CASES = {"text_T2": (2, 1024, 1024), "text_T2_L40": (2, 1024, 224), "text_R12": (12, 50265, 224)}


def case_ids(name: str) -> np.ndarray:
    """token ids of a case: <s> = 0 first, </s> = 2 last, never the padding id 1"""
    layers, vocab, _ = CASES[name]

    def draw(n, salt):
        u = synth.hash_uniform("text/ids/" + name, n, salt=salt).astype(np.float64)
        return (3 + np.floor((u + 1.0) / 2.0 * (vocab - 3))).astype(np.int64).clip(3, vocab - 1)

    if name == "text_T2":
        a, b, c, d, e = draw(5, 0).tolist()
        return np.array([0, a, b, c, b, d, b, e, 2], dtype=np.int64)      # one id three times
    if name == "text_T2_L40":
        return np.concatenate([[0], draw(38, 1), [2]]).astype(np.int64)
    mid = draw(9, 2)
    return np.concatenate([[0], mid[:5], [vocab - 1], mid[5:8], [mid[1]], [2]]).astype(np.int64)   # L = 12, mid[1] twice


def loss_weights(name: str, L: int, d: int = 256):
    w1 = synth.hash_normal(f"text/w1/{name}", L * d).reshape(L, 1, d)
    w2 = synth.hash_normal(f"text/w2/{name}", d).reshape(1, d)
    return w1, w2


def build_reference(layers: int, vocab: int):
    def mod(name, **attrs):
        m = types.ModuleType(name)
        m.__dict__.update(attrs)
        sys.modules[name] = m
        return m

    ppb = mod("pytorch_pretrained_bert.modeling", BertModel=object)
    mod("pytorch_pretrained_bert", modeling=ppb)
    if "cgitb" not in sys.modules:
        try:
            import cgitb  # noqa: F401
        except ImportError:
            mod("cgitb", text=None)
    mod("utils.video_list", NestedTensor=object)
    if "utils" not in sys.modules:
        mod("utils", video_list=sys.modules["utils.video_list"])
    import transformers
    from transformers import RobertaConfig, RobertaModel

    cfg = RobertaConfig(vocab_size=vocab, num_hidden_layers=layers, hidden_size=768, num_attention_heads=12,
                        intermediate_size=3072, max_position_embeddings=514, type_vocab_size=1, layer_norm_eps=1e-5,
                        pad_token_id=1, bos_token_id=0, eos_token_id=2, attn_implementation="eager")
    RobertaModel.from_pretrained = classmethod(lambda cls, name, *a, **k: RobertaModel(cfg))
    transformers.RobertaTokenizerFast.from_pretrained = classmethod(lambda cls, name, *a, **k: None)
    sys.path.insert(0, os.path.join(REF, "models", "language_model"))
    import importlib.util
    spec = importlib.util.spec_from_file_location("ref_bert", os.path.join(REF, "models", "language_model", "bert.py"))
    ref_bert = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref_bert)
    m = ref_bert.Roberta("roberta-base", 256)
    synth.fill_module_(m, skip_prefixes=())
    return m.eval()


class _Tok:
    """stands in for RobertaTokenizerFast.batch_encode_plus: returns the case's ids"""

    def __init__(self, ids):
        self.ids = ids

    def batch_encode_plus(self, texts, **kw):
        from transformers import BatchEncoding
        ids = torch.from_numpy(self.ids)[None]
        return BatchEncoding({"input_ids": ids, "attention_mask": torch.ones_like(ids)})


def run_case(name: str):
    layers, vocab, k = CASES[name]
    ids = case_ids(name)
    assert 1 not in ids.tolist() and ids.max() < vocab
    L = ids.shape[0]
    w1, w2 = loss_weights(name, L)
    res = {}
    for dtype in (torch.float32, torch.float64):
        m = build_reference(layers, vocab).to(dtype)
        m.tokenizer = _Tok(ids)
        (mask, mem, _), cls = m(["synthetic"], torch.device("cpu"))
        assert not bool(mask.any()) and mem.shape == (L, 1, 256) and cls.shape == (1, 256)
        loss = (mem * torch.from_numpy(w1).to(dtype)).sum() + (cls * torch.from_numpy(w2).to(dtype)).sum()
        loss.backward()
        res[dtype] = (mem.detach(), cls.detach(), {n: p.grad.detach() for n, p in m.named_parameters()},
                      list(m.state_dict().keys()))
    mem32, cls32, g32, keys = res[torch.float32]
    mem64, cls64, g64, _ = res[torch.float64]
    names = list(g32.keys())
    offs, s32, s64 = [0], [], []
    for n in names:
        a, b = g32[n].reshape(-1), g64[n].reshape(-1)
        idx = synth.sample_indices(n, a.numel())
        idx = torch.from_numpy(idx[synth.thinned_positions(idx.size, k)])
        s32.append(a[idx].numpy().astype(np.float32))
        s64.append(b[idx].numpy().astype(np.float64))
        offs.append(offs[-1] + idx.numel())
    out = {
        "keys": np.array(keys), "grad_names": np.array(names), "grad_numel": np.array([g32[n].numel() for n in names]),
        "grad_offsets": np.array(offs, dtype=np.int64), "grad_k": np.array(k),
        "grad32": np.concatenate(s32), "grad64": np.concatenate(s64),
        "input_ids": ids, "memory64": mem64.numpy(), "cls64": cls64.numpy(),
        "memory32": mem32.numpy(), "cls32": cls32.numpy(),
    }
    uid = np.unique(ids)
    pos = np.arange(L, dtype=np.int64) + 2
    for tag, nm, rows in (("word", "body.embeddings.word_embeddings.weight", uid),
                          ("pos", "body.embeddings.position_embeddings.weight", pos)):
        out[f"{tag}_rows"] = rows
        out[f"{tag}_rows32"] = g32[nm][torch.from_numpy(rows)].numpy().astype(np.float32)
        out[f"{tag}_rows64"] = g64[nm][torch.from_numpy(rows)].numpy().astype(np.float64)
    path = os.path.join(OUT, name + ".npz")
    np.savez_compressed(path, **out)
    print(name, "L", L, "tensors", len(names), "bytes", os.path.getsize(path))
    assert os.path.getsize(path) < (1 << 20)


if __name__ == "__main__":
    for case in (sys.argv[1:] or list(CASES)):
        run_case(case)
