"""Optimizer tail of the training step as two multi-tensor HIP launches.

Mirrors the reference's interface for this part of the loop (scripts/train_net.py:134-143):

    optimizer = make_optimizer(cfg, model)                      # engine/optimizer.py:25-55 (AdamW, 4 groups)
    ...
    optimizer.zero_grad(); losses.backward()
    optimizer.step(max_grad_norm=cfg.SOLVER.MAX_GRAD_NORM,      # clip_grad_norm_ + AdamW.step + update_ema
                   model_ema=model_ema, ema_decay=cfg.MODEL.EMA_DECAY)
    adjust_learning_rate(cfg, optimizer, iteration, max_iter)   # engine/lr_scheduler.py:212-252

`clip_grad_norm_` and `update_ema` are also available on their own with the reference's signatures.  There is no
PyTorch fallback: every update runs in csrc/optim.h through the C ABI.
"""
from bisect import bisect_right
from typing import Dict, Iterable, List, Optional

import numpy as np
import torch

from . import _lib as L

CHUNK = 1 << 16  # elements per workgroup


class _TensorTable:
    """Device table of (p, g, m, v, ema, n, group) entries + the chunk lists of csrc/optim.h.  The rows are uploaded
    again only when a pointer changes (gradient tensors are re-allocated by autograd unless they live in the reducer's
    flat buckets, the zero arena or a launch plan's static buffers, where they are stable from step to step), the
    chunk lists only when a tensor's length does."""

    def __init__(self, device):
        self.device = device
        self.key = None
        self._sizes = None
        self.table = self.chunk_tensor = self.chunk_off = None
        self.n_chunks = 0
        self.partials = None
        self.rebuilds = 0            # how often update() found a changed pointer (tools/bench_accum.py reports it)
        self.entry = L.load().stcat_optim_table_entry_bytes()
        assert self.entry == 56, self.entry

    def update(self, rows):
        """rows: list of (p_ptr, g_ptr, m_ptr, v_ptr, ema_ptr, numel, group)"""
        key = tuple(rows)
        if key == self.key:
            return
        self.key = key
        self.rebuilds += 1
        dt = np.dtype([("p", "<u8"), ("g", "<u8"), ("m", "<u8"), ("v", "<u8"), ("ema", "<u8"), ("n", "<i8"),
                       ("group", "<i4"), ("pad", "<i4")])
        assert dt.itemsize == self.entry
        cols = np.array(rows, dtype=np.uint64).reshape(len(rows), 7)
        sizes = tuple(r[5] for r in rows)
        if sizes != self._sizes:
            # the chunk lists depend on the tensors' lengths alone: built once, however often a pointer moves
            self._sizes = sizes
            ct, co = [], []
            for i, n in enumerate(sizes):
                for off in range(0, n, CHUNK):
                    ct.append(i)
                    co.append(off)
            self.table = torch.empty(len(rows) * self.entry, dtype=torch.uint8, device=self.device)
            self.chunk_tensor = torch.tensor(ct, dtype=torch.int32).to(self.device)
            self.chunk_off = torch.tensor(co, dtype=torch.int64).to(self.device)
            self.n_chunks = len(ct)
            # one partial sum per chunk: the workspace of the ordered squared norm (stcat_grad_sqnorm_ws, deterministic mode)
            self.partials = torch.empty(max(self.n_chunks, 1), dtype=torch.float32, device=self.device)
        # A moved pointer (a gradient that autograd allocates afresh every step: two small tensors of the hot path) costs
        # one stream-ordered copy of the rows from a pinned staging buffer — the host does not wait for the device, so a
        # micro-step that ends in accumulate() leaves no bubble in front of the next one.  (The staging buffer is new each
        # time: torch's pinned allocator does not hand it out again before the copy has run.)
        pin = self.table.is_cuda
        host = torch.empty(len(rows) * self.entry, dtype=torch.uint8, pin_memory=pin)
        tab = host.numpy().view(dt)
        for j, name in enumerate(("p", "g", "m", "v", "ema")):
            tab[name] = cols[:, j]
        tab["n"] = cols[:, 5].astype(np.int64)
        tab["group"] = cols[:, 6].astype(np.int32)
        tab["pad"] = 0
        self.table.copy_(host, non_blocking=pin)


def _dense(t: torch.Tensor) -> bool:
    """element-wise kernels only need a gap-free buffer: row-major, or channels_last (the conv weights' OHWI)"""
    return t.is_contiguous() or (t.dim() == 4 and t.is_contiguous(memory_format=torch.channels_last))


def _same_layout(a: torch.Tensor, b: torch.Tensor) -> bool:
    """same element order in memory (strides of size-1 dims are arbitrary and ignored)"""
    return a.shape == b.shape and all(sa == sb for n, sa, sb in zip(a.shape, a.stride(), b.stride()) if n > 1)


def _ptr(t: Optional[torch.Tensor]) -> int:
    return 0 if t is None else t.data_ptr()


def _grad_sqnorm(t: _TensorTable, sq: torch.Tensor, stream) -> None:
    """sq[0] = sum |g|^2 over the table; in deterministic mode through the table's per-chunk workspace (ordered sum)"""
    if L.is_deterministic():
        L.call("stcat_grad_sqnorm_ws", t.table.data_ptr(), t.chunk_tensor.data_ptr(), t.chunk_off.data_ptr(),
               t.n_chunks, CHUNK, sq.data_ptr(), t.partials.data_ptr(), t.partials.numel(), stream)
    else:
        L.call("stcat_grad_sqnorm", t.table.data_ptr(), t.chunk_tensor.data_ptr(), t.chunk_off.data_ptr(),
               t.n_chunks, CHUNK, sq.data_ptr(), stream)


class AdamW:
    """torch.optim.AdamW semantics (decoupled weight decay, bias correction, eps outside the sqrt) with the
    gradient-norm clip and the EMA model update folded into the same pass.  `param_groups` is a list of dicts with
    "params", "lr", "weight_decay" (what adjust_learning_rate and checkpoint code touch)."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2):
        groups = list(params)
        if groups and not isinstance(groups[0], dict):
            groups = [{"params": groups}]
        self.param_groups: List[Dict] = []
        for g in groups:
            g = dict(g)
            g["params"] = [p for p in g["params"]]
            g.setdefault("lr", lr)
            g.setdefault("weight_decay", weight_decay)
            g.setdefault("betas", betas)
            g.setdefault("eps", eps)
            self.param_groups.append(g)
        if len(self.param_groups) > 8:
            raise ValueError("at most 8 parameter groups")
        self.betas, self.eps = betas, eps
        self.state: Dict[torch.Tensor, Dict[str, torch.Tensor]] = {}
        self.step_count = 0
        self._table = None
        self._sq = None
        self._plist = [p for g in self.param_groups for p in g["params"]]
        self._gkey = None
        self._any = None
        # gradient accumulation (accumulate()): one fp32 accumulator per parameter, allocated on first use and kept
        self.param_names: Dict[torch.Tensor, str] = {}   # optional, for messages (make_optimizer fills it)
        self._acc: Dict[torch.Tensor, torch.Tensor] = {}
        self._acc_n = 0              # micro-steps folded into the open window (0: no window)
        self._acc_set = None         # which parameters of _plist had a gradient at the window's first fold
        self._acc_table = None       # rows (g = p.grad, m = accumulator), keyed on the gradient pointers
        self._acc_gkey = None
        self._win_table = None       # step()'s table with the g column on the accumulators
        self._win_key = None
        # canonical window (stcat_amd.set_canonical_window): the micro-steps are added as a balanced tree — a binary
        # counter over log2(k) fp32 level buffers per parameter, allocated on first use and kept
        self._levels: Dict[torch.Tensor, List[torch.Tensor]] = {}
        self._tree_table = None      # rows (g = p.grad, p / m / v / ema = levels 0 .. 3)
        self._tree_key = None

    def zero_grad(self, set_to_none: bool = True):
        for g in self.param_groups:
            for p in g["params"]:
                if set_to_none:
                    p.grad = None
                elif p.grad is not None:
                    p.grad.zero_()

    def _rows(self, ema_of, src=None):
        """src (parameter -> tensor): the g column points at the window's mean gradient there instead of at p.grad"""
        rows = []
        for gi, g in enumerate(self.param_groups):
            for p in g["params"]:
                if p.grad is None:
                    continue
                if not _dense(p) or not _same_layout(p.grad, p):
                    raise L.StcatHipError("optimizer tensors must be dense and share one memory layout")
                st = self.state.get(p)
                if st is None:
                    st = self.state[p] = {"exp_avg": torch.zeros_like(p), "exp_avg_sq": torch.zeros_like(p)}
                e = ema_of.get(p) if ema_of else None
                if e is not None and not _same_layout(e, p):
                    raise L.StcatHipError("EMA tensor layout differs from its parameter")
                g = src[p] if src is not None else p.grad
                rows.append((p.data_ptr(), g.data_ptr(), st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr(),
                             _ptr(e), p.numel(), gi))
        return rows

    @staticmethod
    def _ema_of(model_ema, model):
        if model_ema is None:
            return None
        if model is None:
            raise ValueError("model_ema needs the model it tracks")
        ema_sd = dict(model_ema.named_parameters())
        return {p: ema_sd[n] for n, p in model.named_parameters() if n in ema_sd}

    # ---- gradient accumulation --------------------------------------------------------------------------------------
    @property
    def accumulated(self) -> int:
        """micro-steps folded into the open accumulation window (0: no window is open)"""
        return self._acc_n

    def discard_accumulated(self) -> None:
        """drop the open window; the accumulators stay allocated, their contents are never read again (the next
        window's first fold overwrites them)"""
        self._acc_n = 0
        self._acc_set = None

    def _name(self, p) -> str:
        n = self.param_names.get(p)
        if n is not None:
            return n
        i = next(i for i, q in enumerate(self._plist) if q is p)
        return f"parameter {i} of the optimizer (shape {tuple(p.shape)})"

    def _grad_key(self):
        """(the gradient pointers, which parameters have one); inside a window the set must be the first fold's"""
        plist = self._plist
        gkey = tuple(p.grad.data_ptr() if p.grad is not None else 0 for p in plist)
        have = tuple(k != 0 for k in gkey)
        if self._acc_n and have != self._acc_set:
            p = next(p for p, a, b in zip(plist, have, self._acc_set) if a != b)
            raise ValueError(f"gradient accumulation: {self._name(p)} "
                             f"{'has' if p.grad is not None else 'has no'} gradient in this micro-step, unlike in the "
                             "window's first; every micro-step of a window must produce the same set of gradients "
                             "(discard_accumulated() drops the window)")
        return gkey, have

    def _fold(self, scale: float) -> None:
        """acc = (first fold of the window ? g : acc + g) * scale for every parameter with a gradient: ONE launch"""
        plist = self._plist
        gkey, have = self._grad_key()
        if gkey != self._acc_gkey:
            rows = []
            for p in plist:
                if p.grad is None:
                    continue
                L.check_tensor(p.grad, "gradient")
                if p.grad.dtype != torch.float32 or not _dense(p) or not _same_layout(p.grad, p):
                    raise L.StcatHipError("optimizer tensors must be dense fp32 and share one memory layout")
                acc = self._acc.get(p)
                if acc is None:
                    acc = self._acc[p] = torch.empty_like(p)      # the parameter's own layout; first fold overwrites
                rows.append((0, p.grad.data_ptr(), acc.data_ptr(), 0, 0, p.numel(), 0))
            if not rows:
                raise ValueError("gradient accumulation: no parameter has a gradient")
            self._any = next(p for p in plist if p.grad is not None)
            if self._acc_table is None:
                self._acc_table = _TensorTable(self._any.device)
            self._acc_table.update(rows)
            self._acc_gkey = gkey
        t = self._acc_table
        L.call("stcat_grad_accumulate", t.table.data_ptr(), t.chunk_tensor.data_ptr(), t.chunk_off.data_ptr(),
               t.n_chunks, CHUNK, 1 if self._acc_n == 0 else 0, float(np.float32(scale)), L.stream_of(self._any))
        self._acc_set = have
        self._acc_n += 1

    @staticmethod
    def _tree_k() -> Optional[int]:
        """micro-steps per optimizer step of the canonical window on this world size; None: the mode is off"""
        if L.canonical_window() is None:
            return None
        import torch.distributed as dist
        world = dist.get_world_size() if dist.is_available() and dist.is_initialized() else 1
        return L.window_micro_steps(world)

    def _fold_tree(self, k: int, last: bool):
        """micro-step j = self._acc_n of a canonical window of k: carry = g, carry = level[i] + carry for the trailing
        one bits i of j, into level[number of them] — on the last micro-step times fp32(1 / N) in place into the top
        level, which is returned per parameter (where step() reads the mean gradient).  ONE launch."""
        j = self._acc_n
        if not last and j + 1 >= k:
            raise ValueError(f"AdamW.accumulate: the canonical window has {k} micro-steps per optimizer step on this "
                             f"world size and {j} are folded: micro-step {j + 1} belongs to step(), which closes the window")
        q = k.bit_length() - 1
        n_carry = (~j & (j + 1)).bit_length() - 1          # trailing one bits of j
        assert q <= 4 and (n_carry == q if last else n_carry < q), (k, j, last)
        plist = self._plist
        gkey, have = self._grad_key()
        key = (q,) + gkey
        if key != self._tree_key:
            rows = []
            for p in plist:
                if p.grad is None:
                    continue
                L.check_tensor(p.grad, "gradient")
                if p.grad.dtype != torch.float32 or not _dense(p) or not _same_layout(p.grad, p):
                    raise L.StcatHipError("optimizer tensors must be dense fp32 and share one memory layout")
                lv = self._levels.setdefault(p, [])
                while len(lv) < q:
                    lv.append(torch.empty_like(p))             # the parameter's own layout; never cleared, never read first
                ptrs = [lv[i].data_ptr() if i < q else 0 for i in range(4)]
                rows.append((ptrs[0], p.grad.data_ptr(), ptrs[1], ptrs[2], ptrs[3], p.numel(), 0))
            if not rows:
                raise ValueError("gradient accumulation: no parameter has a gradient")
            self._any = next(p for p in plist if p.grad is not None)
            if self._tree_table is None:
                self._tree_table = _TensorTable(self._any.device)
            self._tree_table.update(rows)
            self._tree_key = key
        t = self._tree_table
        scale = float(np.float32(1.0) / np.float32(L.canonical_window())) if last else 1.0
        L.call("stcat_grad_tree_fold", t.table.data_ptr(), t.chunk_tensor.data_ptr(), t.chunk_off.data_ptr(),
               t.n_chunks, CHUNK, n_carry, 1 if last else 0, scale, L.stream_of(self._any))
        self._acc_set = have
        self._acc_n += 1
        return {p: self._levels[p][q - 1] for p in plist if p.grad is not None} if last else None

    @torch.no_grad()
    def accumulate(self) -> None:
        """Gradient accumulation: fold the current `p.grad` of every parameter that has one into the optimizer's fp32
        accumulators (one multi-tensor launch on the current stream) and open — or extend — a window of micro-steps.
        The next `step()` folds its own gradients too, scales the sum by 1 / (number of micro-steps) and updates from
        that mean.  Call it where step() would be called (after the reducer's finish()); `p.grad` is left alone — the
        loop's zero_grad at the top of the next micro-step resets it as in any other step, so every micro-step runs
        the replayed launch plans and the overlapped gradient exchange unchanged:

            for j in range(k):
                reducer.zero_grad(); forward; backward; reducer.finish()
                optimizer.accumulate() if j < k - 1 else optimizer.step(...)

        The accumulators cost one more fp32 copy of the trainable parameters and are not checkpointed.
        With a canonical window (stcat_amd.set_canonical_window(N)) the micro-steps are added as a balanced binary tree
        (stcat_grad_tree_fold) through log2(k) level buffers per parameter, k = N / world, and step() multiplies by
        fp32(1 / N): the mean is then the same fp32 expression over the window's N clips on every world size."""
        tree_k = self._tree_k()
        if tree_k is not None:
            self._fold_tree(tree_k, last=False)
        else:
            self._fold(1.0)

    @torch.no_grad()
    def step(self, max_grad_norm: float = 0.0, model_ema=None, ema_decay: float = 0.0, model=None):
        """One optimizer step.  max_grad_norm > 0 clips by the global norm first (train_net.py:136-137); with
        `model_ema` (and the `model` it shadows) the EMA weights are updated in the same launch
        (engine/optimizer.py:5-22).  Returns the squared gradient norm as a device scalar (no sync).
        With an accumulation window open (accumulate()), the current gradients are folded in as its last micro-step and
        everything — clip, non-finite skip, moments, EMA, the returned squared norm — refers to the window's MEAN
        gradient; the window is closed."""
        plist = self._plist
        tree_k = self._tree_k()
        if tree_k is not None and (tree_k > 1 or self._acc_n):
            # canonical window: exactly k = N / world folds, this one included — the tree has no other shape
            if self._acc_n + 1 != tree_k:
                raise ValueError(f"AdamW.step: the canonical window has {tree_k} micro-steps per optimizer step on this "
                                 f"world size, and this step would close it after {self._acc_n + 1} "
                                 "(discard_accumulated() drops the open window)")
            top = self._fold_tree(tree_k, last=True)
            self._acc_n = 0
            self._acc_set = None
            wkey = (id(model_ema), "tree") + tuple(top[p].data_ptr() if p.grad is not None else 0 for p in plist)
            if wkey != self._win_key:
                if self._win_table is None:
                    self._win_table = _TensorTable(self._any.device)
                self._win_table.update(self._rows(self._ema_of(model_ema, model), src=top))
                self._win_key = wkey
            t = self._win_table
        elif self._acc_n:
            self._fold(1.0 / (self._acc_n + 1))
            self._acc_n = 0
            self._acc_set = None
            wkey = (id(model_ema),) + tuple(self._acc[p].data_ptr() if p.grad is not None else 0 for p in plist)
            if wkey != self._win_key:
                if self._win_table is None:
                    self._win_table = _TensorTable(self._any.device)
                self._win_table.update(self._rows(self._ema_of(model_ema, model), src=self._acc))
                self._win_key = wkey
            t = self._win_table
        else:
            # cheap staleness key: the gradient pointers (everything else in the table is stable between steps)
            gkey = (id(model_ema),) + tuple(p.grad.data_ptr() if p.grad is not None else 0 for p in plist)
            if gkey != self._gkey:
                rows = self._rows(self._ema_of(model_ema, model))
                if not rows:
                    return None
                self._any = next(p for p in plist if p.grad is not None)
                if self._table is None:
                    self._table = _TensorTable(self._any.device)
                self._table.update(rows)
                self._gkey = gkey
            t = self._table
        any_p = self._any
        if self._sq is None:
            self._sq = torch.zeros(1, device=any_p.device)
        stream = L.stream_of(any_p)
        self.step_count += 1
        from . import ops
        ops.WEIGHT_EPOCH += 1  # parameters change below through raw pointers: derived copies (weight planes) are stale
        sq = None
        if max_grad_norm and max_grad_norm > 0:
            _grad_sqnorm(t, self._sq, stream)
            sq = self._sq
        lr = np.array([g["lr"] for g in self.param_groups], dtype=np.float32)
        wd = np.array([g["weight_decay"] for g in self.param_groups], dtype=np.float32)
        L.call("stcat_adamw_ema_step", t.table.data_ptr(), t.chunk_tensor.data_ptr(), t.chunk_off.data_ptr(),
               t.n_chunks, CHUNK, _ptr(sq), lr.ctypes.data, wd.ctypes.data, len(self.param_groups),
               float(self.betas[0]), float(self.betas[1]), float(self.eps), self.step_count,
               float(max_grad_norm or 0.0), float(ema_decay), stream)
        return sq

    def state_dict(self):
        """torch.optim.AdamW's layout (what the reference's Checkpointer round-trips, utils/checkpoint.py):
        state[idx] = {step, exp_avg, exp_avg_sq}, param_groups[i]["params"] = [idx, ...].
        The accumulators of an open accumulation window are not part of it: checkpoint between optimizer steps."""
        if self._acc_n:
            raise RuntimeError(f"AdamW.state_dict: an accumulation window is open ({self._acc_n} micro-steps folded) and "
                               "accumulators are not checkpointed; call step() or discard_accumulated() first")
        idx, groups = {}, []
        for g in self.param_groups:
            ids = []
            for p in g["params"]:
                idx[p] = len(idx)
                ids.append(idx[p])
            d = {k: v for k, v in g.items() if k != "params"}
            d.setdefault("amsgrad", False)
            d["params"] = ids
            groups.append(d)
        state = {}
        for p, st in self.state.items():
            state[idx[p]] = {"step": torch.tensor(float(st.get("step", self.step_count))),
                             "exp_avg": st["exp_avg"].clone(), "exp_avg_sq": st["exp_avg_sq"].clone()}
        return {"state": state, "param_groups": groups}

    def load_state_dict(self, sd):
        """accepts a torch.optim.AdamW checkpoint (per-parameter `step`) as well as its own"""
        params = [p for g in self.param_groups for p in g["params"]]
        saved_ids = [i for g in sd["param_groups"] for i in g["params"]] if sd["param_groups"] and \
            "params" in sd["param_groups"][0] else list(range(len(params)))
        if len(saved_ids) != len(params):
            raise ValueError("loaded state dict has a different number of parameters")
        where = {sid: p for sid, p in zip(saved_ids, params)}
        steps = []
        self.state = {}
        for i, st in sd["state"].items():
            p = where[int(i)]
            # moments take the parameter's own memory layout (channels_last conv weights); copy_ maps by index
            self.state[p] = {k: torch.zeros_like(p).copy_(st[k].to(p.device, torch.float32))
                             for k in ("exp_avg", "exp_avg_sq")}
            if "step" in st:
                steps.append(int(float(st["step"])))
        # one bias-correction counter for the fused launch: every parameter of the hot path receives a gradient at
        # every step (statically dead ones never enter `state`), so the per-parameter counters agree
        self.step_count = max(steps) if steps else int(sd.get("step", 0))
        for g, saved in zip(self.param_groups, sd["param_groups"]):
            g.update({k: v for k, v in saved.items() if k != "params"})
        self._gkey = None
        self._win_key = None         # (the moments were re-allocated: both step tables are stale)
        self.discard_accumulated()


def make_optimizer(cfg, model, logger=None) -> AdamW:
    """engine/optimizer.py:25-55: four groups (rest / vis_encoder / text_encoder / ground_decoder.temp_decoder) with
    their own learning rates; only SOLVER.OPTIMIZER == 'adamw' (both experiment files) is implemented."""
    named = [(n, p) for n, p in model.named_parameters() if p.requires_grad]
    vis = [p for n, p in named if "vis_encoder" in n]
    txt = [p for n, p in named if "text_encoder" in n]
    tmp = [p for n, p in named if "ground_decoder.temp_decoder" in n]
    rest = [p for n, p in named if "vis_encoder" not in n and "text_encoder" not in n
            and "ground_decoder.temp_decoder" not in n]
    if cfg.SOLVER.OPTIMIZER != "adamw":
        raise ValueError("stcat_amd.optim implements SOLVER.OPTIMIZER='adamw' only")
    groups = [{"params": rest}, {"params": vis, "lr": cfg.SOLVER.VIS_BACKBONE_LR},
              {"params": txt, "lr": cfg.SOLVER.TEXT_LR}, {"params": tmp, "lr": cfg.SOLVER.TEMP_LR}]
    opt = AdamW(groups, lr=cfg.SOLVER.BASE_LR, weight_decay=cfg.SOLVER.WEIGHT_DECAY)
    opt.param_names = {p: n for n, p in named}
    return opt


def adjust_learning_rate(cfg, optimizer, curr_step: int, num_training_steps: int) -> None:
    """engine/lr_scheduler.py:212-252 (host-side scalars: the fused step reads the group learning rates by value)."""
    warm = round(cfg.SOLVER.WARMUP_PROP * num_training_steps)
    per_epoch = round(num_training_steps / cfg.SOLVER.MAX_EPOCH)
    epoch = curr_step // per_epoch
    kind = cfg.SOLVER.SCHEDULE.TYPE
    stepped = 0.1 ** bisect_right(cfg.SOLVER.SCHEDULE.DROP_STEP, epoch)
    if kind == "multistep_with_warmup":
        gamma = stepped
        if curr_step < warm:
            side = float(curr_step) / float(max(1, warm))
        else:
            side = max(0.0, float(num_training_steps - curr_step) / float(max(1, num_training_steps - warm)))
    elif kind == "multistep_with_warmup_all":
        gamma = float(curr_step) / float(max(1, warm)) if curr_step < warm else stepped
        side = gamma
    else:
        raise ValueError(f"Unsupported Schedule Type : {kind}")
    base = [cfg.SOLVER.BASE_LR, cfg.SOLVER.VIS_BACKBONE_LR, cfg.SOLVER.TEXT_LR, cfg.SOLVER.TEMP_LR]
    assert len(optimizer.param_groups) == len(base)
    for group, lr, gm in zip(optimizer.param_groups, base, [gamma, gamma, side, side]):
        group["lr"] = lr * gm


@torch.no_grad()
def clip_grad_norm_(parameters: Iterable[torch.Tensor], max_norm: float) -> torch.Tensor:
    """torch.nn.utils.clip_grad_norm_ (L2): returns the total norm (device scalar) and scales the gradients in
    place when it exceeds max_norm.  The fused AdamW.step(max_grad_norm=...) does not need this call.
    Both launches walk every gradient buffer in flat memory order (the ops are element-wise), so channels_last
    conv gradients — the layout of every 3x3 weight gradient of the backbone — are handled without a layout copy."""
    ps = [p for p in parameters if p.grad is not None]
    if not ps:
        return torch.zeros(())
    for p in ps:
        L.check_tensor(p.grad, "gradient")
        if not _dense(p.grad):
            raise L.StcatHipError("clip_grad_norm_: gradients must be dense (row-major or channels_last)")
    dev = ps[0].device
    tab = _TensorTable(dev)
    tab.update([(0, p.grad.data_ptr(), 0, 0, 0, p.grad.numel(), 0) for p in ps])
    sq = torch.zeros(1, device=dev)
    st = L.stream_of(ps[0])
    _grad_sqnorm(tab, sq, st)
    # g *= min(1, max_norm / (norm + 1e-6)) with the coefficient computed on the device: no host sync
    L.call("stcat_grad_clip_scale", tab.table.data_ptr(), tab.chunk_tensor.data_ptr(), tab.chunk_off.data_ptr(),
           tab.n_chunks, CHUNK, sq.data_ptr(), float(max_norm), st)
    return sq.sqrt()[0]


@torch.no_grad()
def update_ema(model, model_ema, decay: float) -> None:
    """engine/optimizer.py:5-22 on its own: every floating-point state_dict entry of model_ema moves toward the
    model's (integer buffers are copied)."""
    if hasattr(model, "module"):
        model = model.module
    msd = model.state_dict()
    rows, dev, any_t = [], None, None
    for k, ema_v in model_ema.state_dict().items():
        src = msd[k].detach()
        if ema_v.dtype != torch.float32:
            ema_v.copy_(src)
            continue
        if not _dense(ema_v) or not _same_layout(src, ema_v):
            raise L.StcatHipError("update_ema: tensors must be dense and share one memory layout")
        rows.append((src.data_ptr(), 0, 0, 0, ema_v.data_ptr(), ema_v.numel(), 0))
        dev, any_t = ema_v.device, ema_v
    if not rows:
        return
    tab = _TensorTable(dev)
    tab.update(rows)
    L.call("stcat_ema_update", tab.table.data_ptr(), tab.chunk_tensor.data_ptr(), tab.chunk_off.data_ptr(),
           tab.n_chunks, CHUNK, float(decay), L.stream_of(any_t))



def set_f16_scales(weight_log2: int, grad_log2: int) -> None:
    """the only supported way to change mode f16x3p's operand scales: a new WEIGHT scale makes every cached weight plane
    stale (they hold w * 2^old), so the weight-plane caches are forced to refresh (ops.WEIGHT_EPOCH) and every launch plan
    is dropped (the caches are keyed on pointers + mode, not on the scales)"""
    from . import ops, plans
    old_w = L.load().stcat_get_f16_scale(0)
    L.call("stcat_set_f16_scales", int(weight_log2), int(grad_log2))
    if int(weight_log2) != int(old_w):
        ops.WEIGHT_EPOCH += 1
    plans.invalidate()


class PlaneLossScale:
    """Dynamic gradient (loss) scale of the experimental mma mode `f16x3p` — torch.cuda.amp.GradScaler's policy on the one
    number that mode needs: every GRADIENT plane of the backbone holds dy * 2^log2 (fp16's range; csrc/igemm_pl.h), the
    weight-gradient epilogue divides it out again, so the scale never reaches the optimizer.  An overflow shows up as a
    non-finite global gradient norm: `AdamW.step(max_grad_norm=...)` then skips the update on the device, and `update()`
    halves the scale; after `growth_interval` finite steps in a row it doubles (up to `max_log2`).  `update()` reads one
    device scalar (a sync) every `check_every` steps.  Changing the scale invalidates the launch plans (they bake the
    epilogue factor into their recorded arguments)."""

    def __init__(self, init_log2: int = 16, growth_interval: int = 2000, check_every: int = 1, max_log2: int = 24):
        self.log2 = int(init_log2)
        self.growth_interval = int(growth_interval)
        self.check_every = max(1, int(check_every))
        self.max_log2 = int(max_log2)
        self.good = 0
        self.calls = 0
        self.skipped = 0
        self._apply()

    def _apply(self):
        from . import plans
        wlog = L.load().stcat_get_f16_scale(0)
        set_f16_scales(int(wlog), int(self.log2))

    def update(self, sqnorm) -> bool:
        """sqnorm: what AdamW.step() returned.  -> True when the step was applied (finite norm)"""
        self.calls += 1
        if sqnorm is None or self.calls % self.check_every:
            return True
        ok = bool(torch.isfinite(sqnorm).all().item())
        if not ok:
            self.skipped += 1
            self.good = 0
            if self.log2 > 0:
                self.log2 -= 1
                self._apply()
            return False
        self.good += self.check_every
        if self.good >= self.growth_interval and self.log2 < self.max_log2:
            self.log2 += 1
            self.good = 0
            self._apply()
        return True
