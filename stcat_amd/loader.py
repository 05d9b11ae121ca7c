"""Input side of the hot path (scripts/train_net.py:105-108 moves every batch with `.to(device)` on the
compute stream): frames go host -> HBM on a COPY stream into one of two resident device buffers while the previous
step computes, so the step never waits for PCIe.  Works on the video decoder's uint8 [T,H,W,3] frames (normalised
inside the stem's gather, 38.5 MB per C3 clip) and on the reference's normalised fp32 [T,3,H,W] tensor (154 MB) alike.
`DeviceClipLoader` takes clips that still need the input transforms (flip, resize, crop, normalise: transforms.ClipPlan)
and runs those on the device behind the copy.
"""
from __future__ import annotations

from typing import Iterable, Iterator, Tuple

import torch


class DeviceFramePrefetcher:
    """`for frames in DeviceFramePrefetcher(host_clips, device): step(frames)`.

    host_clips yields CPU tensors of one fixed shape / dtype (pinned or not: they are staged through a pinned buffer
    when they are not).  The tensor handed out stays valid until the next-but-one clip is requested (two buffers): the
    consumer's kernels of step k are ordered before the copy of clip k + 2 into the same buffer."""

    def __init__(self, host_clips: Iterable[torch.Tensor], device: torch.device, stage=None):
        """stage: optional `Backbone.stage_next` (round 6) — every time a clip is handed out, the NEXT one (already
        being copied) is declared to the backbone with its copy event, so its frozen prefix (stem + max-pool + layer1)
        runs under the current step's grounding section"""
        self.declare = stage
        self.it: Iterator[torch.Tensor] = iter(host_clips)
        self.dev = torch.device(device)
        self.copy_stream = torch.cuda.Stream(device=self.dev)
        self.bufs = [None, None]
        self.stage = [None, None]
        self.ready = [torch.cuda.Event(), torch.cuda.Event()]     # copy of buffer i finished
        self.free = [None, None]                                   # consumer is done with buffer i
        self.k = 0
        self._pending = None
        self._issue()

    def _issue(self) -> None:
        try:
            clip = next(self.it)
        except StopIteration:
            self._pending = None
            return
        i = self.k & 1
        if self.bufs[i] is None or self.bufs[i].shape != clip.shape or self.bufs[i].dtype != clip.dtype:
            self.bufs[i] = torch.empty(clip.shape, dtype=clip.dtype, device=self.dev)
            # allocated on the CURRENT stream, first written on the copy stream: the block may have served kernels still
            # queued on the current stream, so the copy stream waits for them, and the allocator is told
            # about the second stream
            self.copy_stream.wait_stream(torch.cuda.current_stream(self.dev))
            self.bufs[i].record_stream(self.copy_stream)
        src = clip
        if not clip.is_pinned():
            if self.stage[i] is None or self.stage[i].shape != clip.shape or self.stage[i].dtype != clip.dtype:
                self.stage[i] = torch.empty(clip.shape, dtype=clip.dtype).pin_memory()
            self.ready[i].synchronize()            # the previous copy out of this staging buffer has left the host
            self.stage[i].copy_(clip)
            src = self.stage[i]
        with torch.cuda.stream(self.copy_stream):
            if self.free[i] is not None:
                self.copy_stream.wait_event(self.free[i])          # step k - 2 no longer reads this buffer
            self.bufs[i].copy_(src, non_blocking=True)
            self.ready[i].record(self.copy_stream)
        self._pending = i
        self.k += 1

    def __iter__(self):
        return self

    def __next__(self) -> torch.Tensor:
        if self._pending is None:
            raise StopIteration
        i = self._pending
        cur = torch.cuda.current_stream(self.dev)
        cur.wait_event(self.ready[i])               # device-side wait: the host does not block
        out = self.bufs[i]
        j = i ^ 1                                   # the consumer has moved on from the other buffer: mark it free
        ev = torch.cuda.Event()
        ev.record(cur)
        self.free[j] = ev
        self._issue()                               # clip k + 1 starts copying while the caller computes on clip k
        if self.declare is not None and self._pending is not None:
            self.declare(self.bufs[self._pending], self.ready[self._pending])
        return out


class DeviceClipLoader:
    """`for frames in DeviceClipLoader(clips, device): step(frames)` with clips yielding (source frames, ClipPlan):
    the decoder's frames as a CPU tensor — uint8 [T,h,w,3] or fp32 [T,3,h,w], any shape from clip to clip, pinned or not —
    and the geometry drawn for them (transforms.sample_train_plan / eval_plan).  The source goes host -> HBM on a copy
    stream into one of two buffers that grow to the largest clip seen; `plan.apply` runs behind the copy on a transform
    stream into one of two output buffers; the consumer gets normalised fp32 [T,3,H,W] frames and never waits for
    either.  As with DeviceFramePrefetcher, the tensor handed out stays valid until the next-but-one clip is requested.
    stage: optional `Backbone.stage_next`; the NEXT clip is declared with the event of its transform."""

    def __init__(self, clips: Iterable[Tuple[torch.Tensor, "object"]], device: torch.device, stage=None):
        self.declare = stage
        self.it = iter(clips)
        self.dev = torch.device(device)
        self.copy_stream = torch.cuda.Stream(device=self.dev)
        self.xform_stream = torch.cuda.Stream(device=self.dev)
        self.src = [None, None]            # device bytes the source is copied into
        self.pin = [None, None]            # pinned host bytes, for sources that are not pinned
        self.dst = [None, None]            # device floats the plan writes
        self.out = [None, None]            # the view of dst handed out
        self.copied = [torch.cuda.Event(), torch.cuda.Event()]    # source i is in HBM
        self.ready = [torch.cuda.Event(), torch.cuda.Event()]     # output i is transformed
        self.free = [None, None]                                   # the consumer is done with output i
        self.allocations = 0               # device buffers allocated so far (4 once every buffer has its final size)
        self.k = 0
        self._pending = None
        self._issue()

    def _grown(self, buf, count: int, dtype, streams):
        """buf if it holds `count` elements, else a new device buffer that does (allocated on the current stream and made
        known to the streams that write it, as in DeviceFramePrefetcher._issue)"""
        if buf is not None and buf.numel() >= count:
            return buf
        buf = torch.empty(count, dtype=dtype, device=self.dev)
        self.allocations += 1
        for st in streams:
            st.wait_stream(torch.cuda.current_stream(self.dev))
            buf.record_stream(st)
        return buf

    def _issue(self) -> None:
        try:
            clip, plan = next(self.it)
        except StopIteration:
            self._pending = None
            return
        i = self.k & 1
        clip = clip.contiguous()
        nbytes = clip.numel() * clip.element_size()
        T = clip.shape[0]
        oh, ow = plan.out_size()
        self.src[i] = self._grown(self.src[i], nbytes, torch.uint8, (self.copy_stream, self.xform_stream))
        self.dst[i] = self._grown(self.dst[i], T * 3 * oh * ow, torch.float32, (self.xform_stream,))
        host = clip.view(-1).view(torch.uint8)
        if not clip.is_pinned():
            if self.pin[i] is None or self.pin[i].numel() < nbytes:
                self.pin[i] = torch.empty(nbytes, dtype=torch.uint8).pin_memory()
            self.copied[i].synchronize()           # the previous copy out of this staging buffer has left the host
            self.pin[i][:nbytes].copy_(host)
            host = self.pin[i][:nbytes]
        src = self.src[i][:nbytes]
        with torch.cuda.stream(self.copy_stream):
            if self.k >= 2:
                self.copy_stream.wait_event(self.ready[i])         # the transform of clip k - 2 has read this buffer
            src.copy_(host, non_blocking=True)
            self.copied[i].record(self.copy_stream)
        self.out[i] = self.dst[i][:T * 3 * oh * ow].view(T, 3, oh, ow)
        with torch.cuda.stream(self.xform_stream):
            self.xform_stream.wait_event(self.copied[i])
            if self.free[i] is not None:
                self.xform_stream.wait_event(self.free[i])         # step k - 2 no longer reads this output
            plan.apply(src.view(clip.dtype).view(clip.shape), out=self.out[i])
            self.ready[i].record(self.xform_stream)
        self._pending = i
        self.k += 1

    def __iter__(self):
        return self

    def __next__(self) -> torch.Tensor:
        if self._pending is None:
            raise StopIteration
        i = self._pending
        cur = torch.cuda.current_stream(self.dev)
        cur.wait_event(self.ready[i])               # device-side wait: the host does not block
        out = self.out[i]
        ev = torch.cuda.Event()
        ev.record(cur)
        self.free[i ^ 1] = ev                       # the consumer has moved on from the other output
        self._issue()                               # clip k + 1 is copied and transformed while the caller computes on clip k
        if self.declare is not None and self._pending is not None:
            self.declare(self.out[self._pending], self.ready[self._pending])
        return out
