"""The synthetic training step — counterpart of the reference's inner loop (scripts/train_net.py:97-143, without the
optimizer) on one synthetic video per rank: zero_grad, forward, VideoSTGLoss, weighted sum, backward, gradient exchange.

`bench.py` times exactly `TrainStep.step()`, and `tests/test_model_parity.py` compares exactly that — the launch plans
replayed, the zero arena, the bucketed reducer, the loss plan — with the reference's fixtures ("the
path the bench times is not the path the oracle tests check").
"""
from __future__ import annotations

import torch

from . import _lib, ops, plans, synth
from .dist import GradBucketReducer
from .misc import BoxList, NestedTensor
from .pipeline import SyntheticText, build_model


def window_num_boxes(counts, n_clips: int, dev, out=None):
    """The loss normaliser of a canonical window (stcat_amd.set_canonical_window): `counts` are the box counts of the clips
    THIS rank runs in the window; their integer sum is all-reduced once (exact in any order) and
    clamp(total / n_clips, 1) comes back as a 1-element fp32 device tensor (written into `out` when given) — the mean box
    count over the window's clips, the same value for every split of them over ranks and micro-steps, and with one
    micro-step the reference's own normaliser (criterion.py:175-178).  No host sync."""
    import torch.distributed as dist
    cuda = torch.device(dev).type == "cuda"
    host = torch.empty(1, dtype=torch.int64, pin_memory=cuda)
    host[0] = int(sum(counts))
    total = host.to(dev, non_blocking=True) if cuda else host
    if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
        dist.all_reduce(total)
    nb = torch.clamp(total.to(torch.float32) / float(n_clips), min=1)
    if out is None:
        return nb
    out.copy_(nb)
    return out


class TrainStep:
    """model + criterion + reducer + the per-step host sequence.

    frames / mask / targets default to the benchmark's synthetic clip of `config` (seeded per rank); a test passes the
    clip of a fixture instead.  `loss_plan_inside=True` (default): the loss's target-derived index tensors and its
    1-element box-count all-reduce (criterion.py:160-192, 175-178) are rebuilt inside EVERY step, as the reference does;
    the targets stay on the host side of the input pipeline, so building them costs no device -> host sync."""

    def __init__(self, dev, config="C3", rank: int = 0, train: bool = True, roberta_dummy: bool = False,
                 force_comm: bool = False, clip=None, targets=None, loss_plan_inside: bool = True, seed: int = 20260929,
                 arena_elems: int = 120_000_000, clips=None, pipeline_prefix: bool = False, clip_targets=None):
        self.dev = dev
        T, res, L = synth.CONFIGS[config] if isinstance(config, str) else config
        self.T, self.res, self.L = T, res, L
        self.model, self.criterion, self.wd = build_model(None, SyntheticText(synth.synth_text(L)))
        if train:
            self.model.train()       # the measured workload: dropout active (FrozenBN has no train-mode state)
            ops.manual_seed(seed, rank)
        else:
            self.model.eval()        # dropout off (the parity configuration); gradients flow
        synth.fill_module_(self.model)
        self.model.to(dev)
        self.reducer = GradBucketReducer(self.model, extra_numel=124_645_632 if roberta_dummy else 0,
                                         force_comm=force_comm)
        self.arena = ops.enable_zero_arena(dev, arena_elems)   # weight-gradient accumulators etc.: one memset per step
        if clip is None:
            frames = synth.synth_frames(T, res, seed=1000 * 3 + rank)
            mask = torch.zeros(T, res, res, dtype=torch.bool)
        else:
            frames, mask = clip
        # `clips`: several (frames, mask) of one geometry, visited round-robin (step k runs clips[k % len]); with
        # `pipeline_prefix` each step declares the NEXT step's frames to the backbone (Backbone.stage_next), which computes
        # their frozen prefix under this step's grounding section — what a training loop with a look-ahead loader does
        if clips is None:
            clips = [(frames, mask)]
        self.clips = [NestedTensor(f.to(dev), m.to(dev), [T]) for f, m in clips]
        self.clip_index = 0
        self.pipeline_prefix = pipeline_prefix
        self.videos = self.clips[0]
        if targets is None:
            act, tb = synth.synth_targets(T, seed=rank)
            targets = [{"actioness": act, "boxs": BoxList(tb)}]
        self.targets_host = targets                      # annotations as the loader holds them (host memory)
        self.targets = [{"actioness": t["actioness"].to(dev), "boxs": t["boxs"].to(dev)} for t in targets]
        # `clip_targets`: the annotations of each of `clips` (one target list per clip); without it every clip is paired
        # with `targets`
        if clip_targets is not None and len(clip_targets) != len(self.clips):
            raise ValueError(f"TrainStep: {len(clip_targets)} target lists for {len(self.clips)} clips")
        self.clip_targets_host = clip_targets
        self.clip_targets = None if clip_targets is None else [
            [{"actioness": t["actioness"].to(dev), "boxs": t["boxs"].to(dev)} for t in ts] for ts in clip_targets]
        # canonical window (window()): optimizer steps taken, the global clip number of the micro-step under way, the
        # window's loss normaliser (one device scalar, kept: the loss node's launch plan holds its address)
        self.window_index = 0
        self._clip_number = None
        self._window_nb = None
        self.loss_plan_inside = loss_plan_inside
        self._plan = None
        self.uniform_w = len({self.wd[k] for k in self.wd if k.startswith("loss_bbox")}) == 1
        self.last_out = None
        self.keep_outputs = False

    # ---- the loss's target-only tensors ---------------------------------------------------------------------------
    def loss_plan(self):
        if self._clip_number is not None:
            self._plan = self.criterion.plan(self.targets_host, [self.T], self.dev, num_boxes=self._window_nb)
        elif self.loss_plan_inside or self._plan is None:
            self._plan = self.criterion.plan(self.targets_host, [self.T], self.dev)
            self._plan.num_boxes(self.dev)               # criterion.py:175-178: the 1-element all-reduce (no host sync)
        return self._plan

    # ---- one video: forward + loss + backward; no host syncs ------------------------------------------------------
    def compute(self):
        dev = self.dev
        if self._clip_number is not None:    # canonical window: the clip and its dropout masks follow its global number
            ops.dropout_begin_step(dev, clip=self._clip_number)
            self.clip_index = self._clip_number
        else:
            ops.dropout_begin_step(dev)
        if self.clip_targets is not None:
            i = self.clip_index % len(self.clips)
            self.targets_host, self.targets = self.clip_targets_host[i], self.clip_targets[i]
        self.arena.reset()
        # training updates the fp32 weights between steps, so the per-step split of all conv weights into bf16 planes
        # (+ the transposed, FrozenBN-scaled copies for the data gradients) is part of every step: no optimizer runs
        # inside the timed region, hence the epoch bump that makes the refresh launch run as it does in training
        ops.WEIGHT_EPOCH += 1
        plan = self.loss_plan()
        self.videos = self.clips[self.clip_index % len(self.clips)]
        self.clip_index += 1
        if self.pipeline_prefix:
            # (canonical window: this rank's next clip is world numbers on, within the window and across its end)
            nxt_i = self.clip_index if self._clip_number is None else self._clip_number + self.reducer.world
            nxt = self.clips[nxt_i % len(self.clips)]
            self.model.vis_encoder[0].stage_next(nxt.tensors)
        out = self.model(self.videos, ["synthetic"])
        if self.keep_outputs:        # (tests: the criterion overwrites pred_boxes with the GT-span rows, criterion.py:168-171)
            keys = ("pred_boxes", "pred_sted", "pred_actioness", "weights")
            self.last_out = {k: out[k].detach().clone() for k in keys}
            self.last_out["aux"] = [{k: a[k].detach().clone() for k in keys} for a in out["aux_outputs"]]
        losses = self.criterion(out, self.targets, [self.T], plan=plan)
        self.last_losses = losses
        total = self.criterion.weighted_total(self.wd) if self.uniform_w else sum(losses[k] * self.wd[k] for k in losses)
        total.backward()
        return total

    def step(self):
        self.reducer.zero_grad()
        total = self.compute()
        self.reducer.finish()
        return total

    def window(self, optimizer, k: int, **step_kwargs):
        """One optimizer step over `k` consecutive clips (gradient accumulation): k ordinary step()s — zero_grad, replayed
        forward / backward, gradient exchange — the first k - 1 each followed by `optimizer.accumulate()`, the last by
        `optimizer.step(**step_kwargs)`, which updates from the mean gradient.  Returns (the k loss totals, the squared
        norm optimizer.step returned); no host sync.  Each total is copied: with launch plans the loss lives in a
        static buffer that the next micro-step overwrites.
        With a canonical window of N clips (stcat_amd.set_canonical_window, set before this object is built) k must be
        N / world, and micro-step m of the s-th window runs global clip G = s * N + m * world + rank — clips[G % len(clips)]
        with its clip_targets, what a DistributedSampler over the shared list hands out — with the dropout counters of clip G
        and the loss normalised by the window's box count (window_num_boxes): the update is then bit for bit the same for
        every world size that divides N."""
        if k < 1:
            raise ValueError("TrainStep.window: k >= 1 micro-steps")
        n_win = _lib.canonical_window()
        if n_win is not None:
            return self._canonical_window(optimizer, k, n_win, step_kwargs)
        totals = []
        for j in range(k):
            totals.append(self.step().detach().clone())
            if j < k - 1:
                optimizer.accumulate()
        return totals, optimizer.step(**step_kwargs)

    def _canonical_window(self, optimizer, k, n_win, step_kwargs):
        world, rank = self.reducer.world, self.reducer.rank
        want = _lib.window_micro_steps(world)
        if k != want:
            raise ValueError(f"TrainStep.window: k={k}, but the canonical window of {n_win} clips is {want} micro-steps "
                             f"on {world} rank(s)")
        numbers = [self.window_index * n_win + m * world + rank for m in range(k)]
        tg = self.clip_targets_host
        counts = [sum(len(t["boxs"]) for t in (tg[g % len(self.clips)] if tg is not None else self.targets_host))
                  for g in numbers]
        if self._window_nb is None:
            self._window_nb = torch.empty(1, dtype=torch.float32, device=self.dev)
        window_num_boxes(counts, n_win, self.dev, out=self._window_nb)
        totals = []
        try:
            for m, g in enumerate(numbers):
                self._clip_number = g
                totals.append(self.step().detach().clone())
                if m < k - 1:
                    optimizer.accumulate()
        finally:
            self._clip_number = None
        self.window_index += 1
        return totals, optimizer.step(**step_kwargs)

    def gradients(self):
        return {n: p.grad.detach() for n, p in self.model.named_parameters() if p.grad is not None}

    def close(self):
        """undo the process-wide state a step object installs (tests build several in one process)"""
        self.reducer.close()
        ops.disable_zero_arena()
        plans.clear()
