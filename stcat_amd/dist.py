"""Data-parallel gradient exchange: one video per GPU, one process per GPU (scripts/train_net.py:31-36 wraps
the reference model in torch DDP with find_unused_parameters=True).  Here instead:

* trainable, *live* parameters are grouped into a few large flat fp32 buckets laid out in
  backward-readiness order (heads -> decoders -> encoder -> input_proj -> layer4 -> layer2); ``.grad`` is reset
  to None each step so autograd simply takes every gradient tensor (no per-parameter add kernel), and a
  completed bucket is gathered with ONE fused multi-tensor copy;
* the 14 parameter tensors that never receive a gradient in the reference (ground_encoder.fusion.*,
  decoder.layers.*.ca_qtime_proj.*) are excluded statically instead of being discovered
  by a graph walk every step;
* when the last gradient of a bucket has been accumulated its all-reduce is launched asynchronously —
  RCCL runs it on its own stream while the (much longer) backbone backward keeps the compute stream busy;
* the backbone is ONE autograd node (its backward is ~27 of the step's ~62 ms), so autograd would hand over all of
  its gradients at the very end: the node instead delivers them block by block through ``early()`` (registered as
  ``ops.GRAD_SINK``) from its weight-gradient stream, and the buckets are laid out so that the LAST one to complete
  (layer2 + the tail of layer3) is small — what remains exposed after the last kernel of backward is one <= 16 MB
  all-reduce instead of a 128 MB one;
* ``finish()`` waits for the collectives and applies the 1/world mean;
* the ORDERED exchange (``ordered=True`` / ``STCAT_DP_ORDERED=1``; automatic in deterministic mode beyond two ranks): the
  collectives only move bytes — an all-to-all brings every rank's copy of this rank's shard, ``stcat_rank_sum`` adds them
  left to right in rank order (times 1/world), an all-gather hands the result round.  The order in which a collective
  adds the ranks' values belongs to RCCL (algorithm per message size, topology, channel count); this one is fixed, so
  every rank ends with the same bits, run after run.

xGMI is point-to-point (7 links per GPU): few large messages beat many small ones, hence big buckets.
``torch.distributed`` backend "nccl" is RCCL on ROCm; the CPU test-suite drives the same class over gloo.
"""
from __future__ import annotations

import os
from typing import Dict, List, Optional

import torch
import torch.distributed as dist

from . import _lib


def init_rccl_process_group(device: torch.device, **kw) -> None:
    """`dist.init_process_group("nccl")` (= RCCL on ROCm) with the collectives on a HIGH-PRIORITY stream: HIP keeps a
    separate set of hardware queues per stream priority, so RCCL's stream never shares a queue (= serialises) with the
    compute streams of the step, whose four normal-priority queues are then all ours (stcat_amd.ops._pick_streams), and
    the all-reduce kernels are scheduled ahead of the backward kernels they overlap with."""
    opts = None
    try:
        opts = dist.ProcessGroupNCCL.Options(is_high_priority_stream=True)
    except (AttributeError, TypeError):
        pass
    if opts is not None and not os.environ.get("STCAT_RCCL_NORMAL_PRIORITY"):
        dist.init_process_group("nccl", device_id=device, pg_options=opts, **kw)
    else:
        dist.init_process_group("nccl", device_id=device, **kw)


DEAD_PARAM_MARKERS = ("ground_encoder.fusion.", ".ca_qtime_proj.")


def live_trainable(named_params):
    return [(n, p) for n, p in named_params if p.requires_grad and not any(m in n for m in DEAD_PARAM_MARKERS)]


class GradBucketReducer:
    def __init__(self, model: torch.nn.Module, bucket_mb: float = 64.0, process_group=None, extra_numel: int = 0,
                 force_comm: bool = False, tail_mb: float = 16.0, ordered: Optional[bool] = None):
        """extra_numel: a dummy tail bucket (e.g. 124.6 M elements to emulate the reference's RoBERTa gradients
        in the message size) — reduced with the rest, never read.
        ordered: the rank-ordered exchange (all-to-all, stcat_rank_sum, all-gather) instead of the summing collective;
        None: STCAT_DP_ORDERED (1 / 0), else on exactly when world > 2 in deterministic mode.  With a canonical window
        (stcat_amd.set_canonical_window) it is on from two ranks and sums with stcat_rank_tree_sum."""
        self.group = process_group
        self.world = dist.get_world_size(process_group) if dist.is_initialized() else 1
        self.rank = dist.get_rank(process_group) if dist.is_initialized() else 0
        # comm: gather into flat buckets and all-reduce.  force_comm keeps that path on with a single rank
        # (a 1-GPU box can then exercise the real RCCL calls; the mean over 1 rank is the identity)
        self.comm = self.world > 1 or (force_comm and dist.is_initialized())
        # the mean over ranks rides inside the collective where the backend has it (RCCL: ReduceOp.AVG) — no 1/world
        # pass over the buckets after the wait; gloo (the CPU tests) sums and scales
        self.avg_in_collective = dist.is_initialized() and dist.get_backend(process_group) == "nccl"
        params = live_trainable(model.named_parameters())[::-1]  # reverse registration ~ readiness order
        self.params = [p for _, p in params]
        cap = int(bucket_mb * (1 << 20) // 4)
        self.buckets: List[Dict] = []
        # Parameters of a module whose forward runs on a forked stream (QueryDecoder's time decoder) get their
        # gradients on that stream; they go into their own bucket, reduced in finish() — after backward() the
        # autograd engine has joined every stream with the caller's, so no cross-stream wait is needed inside a hook
        # (a wait_stream there stalls the side chain behind everything queued on the main stream: measured 5 ms).
        late = [(n, p) for n, p in params if getattr(p, "_stcat_forked_stream", False)]
        cur, cur_n = [], 0
        for n, p in params:
            if getattr(p, "_stcat_forked_stream", False):
                continue
            if cur and cur_n + p.numel() > cap:
                self.buckets.append({"params": cur, "numel": cur_n, "late": False})
                cur, cur_n = [], 0
            cur.append((n, p))
            cur_n += p.numel()
        if cur:
            self.buckets.append({"params": cur, "numel": cur_n, "late": False})
        # small LAST bucket: whatever completes last is fully exposed, so cut the tail of the readiness order off
        tail_cap = int(tail_mb * (1 << 20) // 4)
        if self.buckets and self.buckets[-1]["numel"] > tail_cap and len(self.buckets[-1]["params"]) > 1:
            lastb = self.buckets.pop()
            tail, tail_n = [], 0
            head = list(lastb["params"])
            while len(head) > 1 and tail_n + head[-1][1].numel() <= tail_cap:
                n_, p_ = head.pop()
                tail.insert(0, (n_, p_))
                tail_n += p_.numel()
            self.buckets.append({"params": head, "numel": sum(p_.numel() for _, p_ in head), "late": False})
            if tail:
                self.buckets.append({"params": tail, "numel": tail_n, "late": False})
        if late:
            self.buckets.append({"params": late, "numel": sum(p.numel() for _, p in late), "late": True})
        # Which collective moves a bucket (STCAT_DP_COLLECTIVE): "allreduce" (RCCL picks ring / tree / direct by size) or
        # "rs_ag" = reduce-scatter + all-gather issued back to back on RCCL's stream — the explicit form of SURVEY.md §5's
        # "all seven xGMI links" plan, so the first 8-GPU run can A/B the two (no scaling figure has been measured yet:
        # an 8-GPU node is not ours to launch on).  gloo (the CPU tests) has no reduce_scatter_tensor: all-reduce there.
        self.collective = os.environ.get("STCAT_DP_COLLECTIVE", "allreduce")
        if self.collective not in ("allreduce", "rs_ag"):
            raise ValueError(f"STCAT_DP_COLLECTIVE={self.collective!r}: expected allreduce or rs_ag")
        if self.collective == "rs_ag" and not self.avg_in_collective:
            self.collective = "allreduce"
        # The ordered exchange replaces either of them (`collective` keeps its meaning: what runs when it is off).  A sum of
        # two operands has one order, so up to two ranks nothing changes unless it is asked for; the question "is the mode
        # on" is answered without loading the kernel library (a reducer over gloo on CPU tensors has none to load).
        refused = ordered is False
        if ordered is None:
            env = os.environ.get("STCAT_DP_ORDERED", "")
            if env not in ("", "0", "1"):
                raise ValueError(f"STCAT_DP_ORDERED={env!r}: expected 1 or 0")
            refused = env == "0"
            ordered = (env == "1") if env else (self.world > 2 and _lib.deterministic_requested())
        # The canonical window (stcat_amd.set_canonical_window): the ranks of a micro-step are the lower log2(world) levels
        # of the window's tree, so the ordered exchange runs at every world size from two (a summing collective has no
        # scale-free sum to offer) with stcat_rank_tree_sum, and the tree's one multiply by fp32(1 / N) sits here only when
        # this sum is its last add (k = 1 micro-step); otherwise AdamW's fold applies it.
        self.window_k = _lib.window_micro_steps(self.world)
        if self.window_k is not None and self.world > 1:
            if refused:
                raise ValueError("GradBucketReducer: the canonical window needs the ordered exchange (ordered=False / "
                                 "STCAT_DP_ORDERED=0 was asked for)")
            ordered = True
        self.ordered = bool(ordered) and self.comm
        self._exchange_stream = None     # the stream the ordered exchange is issued on (created with the first bucket)
        self._owner = {}
        pad_to = 64 * max(self.world, 1)      # a flat bucket splits into `world` equal, 256-byte aligned shards
        # Canonical window: every parameter's slot starts on a 16-byte boundary, like a gradient tensor of its own.  With one
        # micro-step the optimizer reads the mean gradient from these views, with several from its level buffers (separate
        # allocations): its kernels choose their float4 or scalar form — not the same fp32 expression once the compiler has
        # contracted each — by the pointers' alignment, which must therefore not depend on the layout.
        slot = 4 if self.window_k is not None else 1
        for bi, b in enumerate(self.buckets):
            dev = b["params"][0][1].device
            extent = sum(-(-p.numel() // slot) * slot for _, p in b["params"])
            b["padded"] = -(-extent // pad_to) * pad_to
            # the flat communication buffer only exists when there is somebody to talk to
            b["flat"] = torch.zeros(b["padded"], dtype=torch.float32, device=dev) if self.comm else None
            b["shard"] = (torch.empty(b["padded"] // self.world, dtype=torch.float32, device=dev)
                          if (self.comm and self.collective == "rs_ag" and not self.ordered) else None)
            # ordered exchange: where the all-to-all puts every rank's copy of this rank's shard (as large as the bucket)
            b["recv"] = torch.empty(b["padded"], dtype=torch.float32, device=dev) if self.ordered else None
            # the reference's DDP also reduces the text encoder's 124.6 M gradients, which are complete right after the
            # encoder's backward — BEFORE the backbone's: the dummy message standing in for them is
            # launched behind the bucket that holds input_proj (the first thing after the encoder), not in finish()
            b["triggers_extra"] = any(n == "input_proj.weight" for n, _ in b["params"])
            b["views"] = []
            off = 0
            for n, p in b["params"]:
                if self.comm:
                    view = b["flat"][off:off + p.numel()]
                    # keep the parameter's memory format (conv weights are channels_last)
                    cl = p.dim() == 4 and not p.is_contiguous() and p.is_contiguous(memory_format=torch.channels_last)
                    b["views"].append(torch.as_strided(view, p.shape, p.stride()) if cl else view.view(p.shape))
                off += -(-p.numel() // slot) * slot
                self._owner[p] = bi
                p.register_post_accumulate_grad_hook(self._on_grad)
            b["pending"] = len(b["params"])
            b["work"] = None
        dev0 = self.buckets[0]["params"][0][1].device
        extra_padded = -(-extra_numel // pad_to) * pad_to
        self.extra = torch.zeros(extra_padded, dtype=torch.float32, device=dev0) if (extra_numel and self.comm) else None
        self._extra_shard = (torch.empty(extra_padded // self.world, dtype=torch.float32, device=dev0)
                             if (self.extra is not None and self.collective == "rs_ag" and not self.ordered) else None)
        self._extra_recv = torch.empty_like(self.extra) if (self.extra is not None and self.ordered) else None
        self._extra_work = None
        self.extra_numel = extra_numel
        self.skip_extra = False      # True: leave the dummy (text-encoder-sized) message out of the following steps
        self.deferred = False  # True: hooks do nothing, finish() reduces the (static) gradient tensors afterwards
        self._view_of = {}
        for b in self.buckets:
            for (n, p), v in zip(b["params"], b["views"]):
                self._view_of[p] = v
        self._early = set()
        self._early_stream = {}      # parameter -> the stream early() wrote its bucket view on
        self._early_added = set()    # parameters whose autograd-accumulated gradient was already added into their view
        if self.comm:
            from . import ops
            ops.GRAD_SINK = self   # nodes that produce many parameter gradients hand them over as they complete
        self.no_overlap = bool(os.environ.get("STCAT_REDUCER_NO_OVERLAP"))  # diagnostic: all buckets in finish()
        self.write_through = not os.environ.get("STCAT_NO_WRITE_THROUGH")

    # ---- per step -------------------------------------------------------------------------------
    def zero_grad(self):
        """grads are set to None: autograd then *takes* each gradient tensor instead of running an add kernel
        per parameter; buckets are gathered with one fused multi-tensor copy when they complete."""
        for p in self.params:
            p.grad = None
        self._early.clear()
        self._early_stream.clear()
        self._early_added.clear()
        self._extra_work = None
        for b in self.buckets:
            b["pending"] = len(b["params"])
            b["work"] = None
            if b.get("wt"):            # buckets that producers accumulate into directly start the step at zero
                b["flat"].zero_()

    def close(self):
        from . import ops
        if ops.GRAD_SINK is self:
            ops.GRAD_SINK = None

    def grad_target(self, p):
        """Write-through: the flat-bucket view of p — a producer of p's gradient that accumulates into a zeroed buffer
        anyway (the backbone's split-K weight-gradient kernels) accumulates into the bucket itself, and `early()` has
        nothing to copy (round 2 gathered 327 MB per step; VERDICT r02 missing #7).  The view is cleared by zero_grad()."""
        if not self.comm or self.deferred or not self.write_through:
            return None
        v = self._view_of.get(p)
        if v is not None:
            self.buckets[self._owner[p]]["wt"] = True
        return v

    def early(self, params, grads) -> bool:
        """Called from INSIDE a backward node, on the stream that produced `grads`: take these parameter gradients
        now (the node then returns None for them, so no AccumulateGrad / hook runs later).  Copies run on the current
        stream, i.e. behind the kernels that wrote the gradients; a bucket that completes is reduced right away.
        A second early() delivery of a parameter in one step ADDS (again_s / again_d).  A parameter that is delivered
        here AND accumulated by autograd (used outside the delivering node too) may receive exactly ONE autograd
        contribution per step: the post-accumulate hook sees the whole p.grad each time, so a second firing cannot be
        told from a re-delivery and _on_grad refuses it — such models need STCAT_REDUCER_NO_OVERLAP=1."""
        if not self.comm or self.deferred:
            return False
        touched = []
        srcs, dsts = [], []
        for p, g in zip(params, grads):
            if p not in self._view_of:
                return False          # (a parameter outside the buckets: let autograd handle the whole group)
        # Stream contract: the caller's CURRENT stream is the one that produced `grads` (the backbone calls this inside
        # `with WgradStream`); the copies and the collective launched below are ordered behind it.
        again_s, again_d = [], []
        for p, g in zip(params, grads):
            b = self.buckets[self._owner[p]]
            if p in self._early:
                # second delivery in one step (two backward passes before finish(): gradient accumulation): add, as
                # AccumulateGrad would; a bucket that was already reduced cannot take it any more
                if b["pending"] < 0:
                    raise RuntimeError("GradBucketReducer.early: a bucket was already all-reduced when a second gradient "
                                       "for one of its parameters arrived; call finish() between backward passes — for "
                                       "gradient accumulation run every micro-step as a whole step (zero_grad, "
                                       "backward, finish) and sum with stcat_amd.optim.AdamW.accumulate()")
                if g.data_ptr() != self._view_of[p].data_ptr():   # (written through: the kernel accumulated in place)
                    again_s.append(g)
                    again_d.append(self._view_of[p])
                continue
            if g.data_ptr() != self._view_of[p].data_ptr():      # (written through: already in the bucket)
                srcs.append(g)
                dsts.append(self._view_of[p])
            self._early.add(p)
            if g.is_cuda:
                self._early_stream[p] = torch.cuda.current_stream(g.device)
            b["pending"] -= 1
            if b["pending"] == 0:
                touched.append(b)
        if srcs:
            torch._foreach_copy_(dsts, srcs)
        if again_s:
            torch._foreach_add_(again_d, again_s)
        for b in touched:
            if not b["late"] and not self.no_overlap:
                self._launch(b)
        return True

    def defer(self, on: bool = True):
        """Deferred mode for a hipGraph-captured step (stcat_amd/graph.py): gradient hooks launch nothing (a
        collective must not be captured); after each replay finish() gathers the graph's static gradient tensors
        (bind_static_grads) into the flat buckets and reduces them."""
        self.deferred = on
        if not on:
            for b in self.buckets:
                b.pop("static", None)

    def bind_static_grads(self):
        """call once, right after capture: remember the gradient tensors the captured backward writes"""
        for b in self.buckets:
            b["static"] = [p.grad for _, p in b["params"]]

    def _launch(self, b):
        if self.comm:
            # The bucket is reduced from the CURRENT stream, but early() filled its views from the stream of each
            # delivering node (the forked time decoder and the weight-gradient stream deliver beside the main chain):
            # order the collective behind every one of them, or it reads a view whose copy is still queued elsewhere.
            if self._early_stream and b["flat"].is_cuda:
                cur = torch.cuda.current_stream(b["flat"].device)
                waited = {cur.cuda_stream}
                for _, p in b["params"]:
                    st = self._early_stream.get(p)
                    if st is not None and st.cuda_stream not in waited:
                        waited.add(st.cuda_stream)
                        cur.wait_stream(st)
            srcs, dsts = [], []
            grads = b.get("static") if self.deferred else [p.grad for _, p in b["params"]]
            for (n, p), g, v in zip(b["params"], grads, b["views"]):
                if p in self._early:
                    continue              # delivered through early(): already in the flat buffer
                if g is not None:
                    srcs.append(g)
                    dsts.append(v)
                else:
                    v.zero_()
            if srcs:
                torch._foreach_copy_(dsts, srcs)
            b["work"] = self._reduce(b["flat"], b["shard"], b["recv"])
            if b["triggers_extra"] and self.extra is not None and self._extra_work is None and not self.skip_extra:
                self._extra_work = self._reduce(self.extra, self._extra_shard, self._extra_recv)
        b["pending"] = -1

    def _reduce(self, flat, shard, recv=None):
        """asynchronous mean (RCCL; ordered exchange) / sum (gloo) of one flat buffer over the ranks, in place"""
        if self.ordered:
            return self._exchange(flat, recv)
        op = dist.ReduceOp.AVG if self.avg_in_collective else dist.ReduceOp.SUM
        if shard is not None:
            dist.reduce_scatter_tensor(shard, flat, op=op, group=self.group, async_op=True)
            return dist.all_gather_into_tensor(flat, shard, group=self.group, async_op=True)   # same stream: ordered
        return dist.all_reduce(flat, op=op, group=self.group, async_op=True)

    def _exchange(self, flat, recv):
        """The ordered form of _reduce: shard r of `flat` (padded // world floats, 256-byte aligned) is this rank's to sum.
        all_to_all_single brings every rank's copy of it into `recv`, slice k from rank k; stcat_rank_sum adds the slices
        rank 0 first and scales by fp32(1 / world) — the same chain for every shard, whichever rank owns it — in place in
        this rank's slice of `flat`; all_gather_into_tensor copies the shards round, so every rank holds the same bits.
        On the GPU all of it is issued on the reducer's own exchange stream, ordered behind the current stream (which
        _launch has ordered behind the delivering streams): the stream waits for the all-to-all (work.wait() is a stream
        wait on RCCL), runs the sum and hands the all-gather to the collective's stream — no compute stream waits for
        anything before finish().  (Over gloo, what the tests run, work.wait() also holds the host until the all-to-all is
        done.)  The stream has the collectives' high priority: HIP serves each priority from its own
        hardware queues (init_rccl_process_group), so it takes none of the step's four."""
        S = flat.numel() // self.world
        mine = flat[self.rank * S:(self.rank + 1) * S]
        scale = 1.0 / self.world
        entry = "stcat_rank_sum"
        if self.window_k is not None:
            entry = "stcat_rank_tree_sum"
            scale = 1.0 / self.world if self.window_k == 1 else 1.0

        def run():
            dist.all_to_all_single(recv, flat, group=self.group, async_op=True).wait()
            _lib.call(entry, mine.data_ptr(), recv.data_ptr(), self.world, S, S, scale, _lib.stream_of(flat))
            return dist.all_gather_into_tensor(flat, mine, group=self.group, async_op=True)

        _lib.check_tensor(flat, "gradient bucket")
        if not flat.is_cuda:
            return run()
        if self._exchange_stream is None:
            self._exchange_stream = torch.cuda.Stream(flat.device, priority=-1)
        ex = self._exchange_stream
        ex.wait_stream(torch.cuda.current_stream(flat.device))
        with torch.cuda.stream(ex):
            return run()

    def _on_grad(self, p):
        # (the post-accumulate hook also fires for a parameter whose node returned None because it was handed over through
        # early(): that one is counted already — counting it again would complete mixed buckets too soon and leave the
        # late bucket below zero, never reduced)
        if self.deferred:
            return
        if p in self._early:
            # handed over through early().  If autograd ALSO accumulated a gradient for it (the parameter is used outside
            # the delivering node as well), that contribution must not be lost: add it into the bucket while that is still
            # possible
            g, v = p.grad, self._view_of[p]
            if g is not None and g.data_ptr() != v.data_ptr():
                if self.buckets[self._owner[p]]["pending"] < 0:
                    raise RuntimeError("GradBucketReducer: a parameter delivered through early() received a further "
                                       "gradient from autograd after its bucket was all-reduced")
                #  the hook fires once per accumulation with the WHOLE p.grad: a second firing on the same
                # tensor would add the first contribution again — refuse rather than double-count
                if p in self._early_added:
                    raise RuntimeError("GradBucketReducer: a parameter delivered through early() was accumulated by autograd "
                                       "twice in one step; run this model with STCAT_REDUCER_NO_OVERLAP=1")
                self._early_added.add(p)
                # early() wrote the bucket view on ITS stream (the weight-gradient stream): order this add behind it
                st = self._early_stream.get(p)
                if st is not None and v.is_cuda:
                    torch.cuda.current_stream(v.device).wait_stream(st)
                v.add_(g)
            return
        b = self.buckets[self._owner[p]]
        b["pending"] -= 1
        if b["pending"] == 0 and not b["late"] and not self.no_overlap:
            self._launch(b)

    def finish(self):
        """Block the current stream until every bucket is reduced and averaged; afterwards every live
        parameter's .grad is (a view of) the averaged gradient."""
        if not self.comm:
            return
        for b in self.buckets:
            if self.deferred or b["pending"] >= 0:  # (eager) a parameter got no gradient: reduce what is there
                self._launch(b)
        if self.extra is not None and self._extra_work is None and not self.skip_extra:   # (no bucket triggered it)
            self._extra_work = self._reduce(self.extra, self._extra_shard, self._extra_recv)
        for b in self.buckets:
            b["work"].wait()
            if not self.avg_in_collective and not self.ordered and self.world > 1:
                b["flat"].mul_(1.0 / self.world)
            for (n, p), v in zip(b["params"], b["views"]):
                p.grad = v
        if self._extra_work is not None:
            self._extra_work.wait()

    @property
    def message_bytes(self) -> int:
        return 4 * (sum(b["numel"] for b in self.buckets) + (0 if self.skip_extra else self.extra_numel))
