"""The clip transforms of the training / evaluation input pipeline, on the device (datasets/build.py:20-64 composes
them, datasets/transforms.py:47-168 runs them as float tensor ops on a loader worker: horizontal flip, one bilinear resize
or resize -> random crop -> resize, per-channel normalise).

A loader worker only DRAWS the geometry (`sample_train_plan` / `eval_plan`: a few random numbers, no pixel is touched)
and hands the decoder's frames on as they are; `ClipPlan.apply` then runs the whole chain on the GPU with one launch of
`stcat_clip_resize` per resize (csrc/clip_transform.h): the flip and a crop in front of a resize narrow / mirror that
launch's source window, a crop behind a resize becomes its output window, the normalise rides on the last launch.

Limits: one clip per call (the reference trains with one video per GPU), fp32 [T,3,H,W] output, no ColorJitter /
NormalizeAndPad (build_transforms uses neither).  `antialias` defaults to False: the reference pins torchvision 0.11,
where resizing a tensor is `interpolate(mode="bilinear", align_corners=False)` without antialiasing; newer torchvision
releases antialias tensors by default, pass antialias=True to reproduce a run made with one of those.
"""
from __future__ import annotations

import random
import re
from typing import List, Optional, Sequence, Tuple

import torch

from . import ops

MAX_SIZE = 720                     # the long-side cap of build_transforms
CROP_RESIZES = (400, 500, 600)     # first resize of the crop branch (no cap)
CROP_MIN, CROP_MAX, CROP_TRIES = 384, 600, 50

_CONST = {}


def _affine(device, scale: Sequence[float], shift: Sequence[float]):
    """per-channel (a, b) as fp32 device vectors, computed in float64 and cached"""
    key = (str(device), tuple(scale), tuple(shift))
    if key not in _CONST:
        _CONST[key] = (torch.tensor(scale, dtype=torch.float64).float().to(device),
                       torch.tensor(shift, dtype=torch.float64).float().to(device))
    return _CONST[key]


class ClipPlan:
    """Geometry of one clip's transforms: source (h, w), flip, steps ("resize", oh, ow) / ("crop", i, j, th, tw) in the
    order they apply, mean / std of the final normalise, antialias."""

    def __init__(self, h: int, w: int, flip: bool = False, steps: Sequence[tuple] = (), mean=ops.PIXEL_MEAN,
                 std=ops.PIXEL_STD, antialias: bool = False):
        self.h, self.w, self.flip = int(h), int(w), bool(flip)
        self.steps: List[tuple] = [tuple(s) for s in steps]
        self.mean, self.std, self.antialias = tuple(mean), tuple(std), bool(antialias)
        ch, cw = self.h, self.w
        for s in self.steps:
            if s[0] == "resize":
                _, ch, cw = s
                ok = ch > 0 and cw > 0
            else:
                _, i, j, th, tw = s
                ok = s[0] == "crop" and i >= 0 and j >= 0 and th > 0 and tw > 0 and i + th <= ch and j + tw <= cw
                ch, cw = th, tw
            if not ok:
                raise ValueError(f"ClipPlan: step {s} does not fit the {self.h} x {self.w} clip")
        self._out = (ch, cw)

    def __repr__(self):
        return f"ClipPlan({self.h}x{self.w}, flip={self.flip}, {self.steps}, antialias={self.antialias})"

    def out_size(self) -> Tuple[int, int]:
        return self._out

    def launches(self) -> List[dict]:
        """the kernel launches of this plan: window (of the launch's source), flip, size (virtual output), out_window.
        Only the first launch reads the clip; an identity resize is dropped unless the plan would have no launch left."""
        win = (0, 0, self.h, self.w)           # of the first launch's source, in FLIPPED window coordinates
        done, cur = [], None
        for s in self.steps:
            if s[0] == "resize":
                if cur is not None:
                    done.append(cur)
                    win = (0, 0) + cur["out_window"][2:]
                if (s[1], s[2]) == win[2:]:
                    cur = None
                    continue
                cur = {"window": win, "size": (s[1], s[2]), "out_window": (0, 0, s[1], s[2])}
            else:
                _, i, j, th, tw = s
                if cur is None:
                    win = (win[0] + i, win[1] + j, th, tw)
                else:
                    oy, ox = cur["out_window"][:2]
                    cur["out_window"] = (oy + i, ox + j, th, tw)
        if cur is not None:
            done.append(cur)
        elif not done or win != (0, 0) + done[-1]["out_window"][2:]:
            done.append({"window": win, "size": win[2:], "out_window": (0, 0) + win[2:]})
        for k, ln in enumerate(done):
            ln["flip"] = self.flip and k == 0
            if ln["flip"]:                     # columns [j, j + tw) of the mirrored clip are these source columns
                y, x, hh, ww = ln["window"]
                ln["window"] = (y, self.w - x - ww, hh, ww)
        return done

    def apply(self, frames: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """frames: the clip on the device, uint8 [T,h,w,3] (decoder layout) or fp32 [T,3,h,w] in [0,1] -> normalised
        fp32 [T,3,H,W] with (H, W) = out_size().  One launch per resize (one in all when the plan has none)."""
        u8 = frames.dtype == torch.uint8
        hw = tuple(frames.shape[1:3]) if u8 else tuple(frames.shape[2:4])
        if hw != (self.h, self.w):
            raise ValueError(f"ClipPlan for a {self.h} x {self.w} clip applied to {hw[0]} x {hw[1]} frames")
        inv_std = [1.0 / s for s in self.std]
        shift = [-m / s for m, s in zip(self.mean, self.std)]
        lns = self.launches()
        x = frames
        for k, ln in enumerate(lns):
            last = k == len(lns) - 1
            raw = x.dtype == torch.uint8
            if last:
                a, b = ops.u8_norm(x.device, self.mean, self.std) if raw else _affine(x.device, inv_std, shift)
            else:
                a, b = _affine(x.device, [1.0 / 255.0 if raw else 1.0] * 3, [0.0] * 3)
            x = ops.clip_resize_raw(x, a, b, ln["size"], window=ln["window"], flip=ln["flip"],
                                    out_window=ln["out_window"], antialias=self.antialias, out=out if last else None)
        return x

    def apply_to_boxes(self, boxs):
        """the same geometry on the clip's boxes: calls, in order, what the reference's transforms call on its box list
        (utils/bounding_box.py) — transpose(0), resize((w, h)), crop(region), normalize().  Duck-typed."""
        if self.flip:
            boxs = boxs.transpose(0)
        for s in self.steps:
            boxs = boxs.resize((s[2], s[1])) if s[0] == "resize" else boxs.crop(tuple(s[1:]))
        return boxs.normalize()

    def swap_left_right(self, text: str) -> str:
        """a mirrored clip's sentence: 'left' and 'right' change places"""
        if not self.flip:
            return text
        return re.sub("left|right", lambda m: "right" if m.group() == "left" else "left", text)


def _scales(resolution: int, aug_scale: bool) -> Tuple[int, ...]:
    return tuple(resolution - 32 * i for i in range(4)) if aug_scale else (resolution,)


def _draw_resize(h: int, w: int, sizes: Sequence[int], max_size: Optional[int]) -> Tuple[int, int]:
    """one draw (random.choice) of the short side; the long side follows the aspect ratio and is capped at max_size"""
    size = random.choice(sizes)
    if max_size is not None:
        short, long_ = float(min(h, w)), float(max(h, w))
        if long_ / short * size > max_size:
            size = int(round(max_size * short / long_))
    if (w <= h and w == size) or (h <= w and h == size):
        return h, w
    if w < h:
        return int(size * h / w), size
    return size, int(size * w / h)


def _draw_corner(h: int, w: int, th: int, tw: int) -> Tuple[int, int, int, int]:
    """top-left corner of a th x tw crop, uniform: torch.randint for the row, then for the column; no draw when the
    crop is the whole image.  Restates torchvision's RandomCrop.get_params from its documentation; torchvision is not
    available where this was written, so THIS STEP IS UNCHECKED against it (everything else is checked against the
    reference's own transforms in tests/test_clip_transform.py)."""
    if h == th and w == tw:
        return 0, 0, h, w
    i = int(torch.randint(0, h - th + 1, size=(1,)).item())
    j = int(torch.randint(0, w - tw + 1, size=(1,)).item())
    return i, j, th, tw


def sample_train_plan(h: int, w: int, *, resolution: int = 448, aug_scale: bool = True, flip_prob: float = 0.5,
                      boxs=None, mean=ops.PIXEL_MEAN, std=ops.PIXEL_STD, antialias: bool = False) -> ClipPlan:
    """Draw one training clip's geometry with the draws of the reference's training transforms, in their order and from
    their generators (python's `random`, and torch's global generator for the crop corner): flip; which branch; the
    resize(s); in the crop branch up to 50 crop candidates, the first one `boxs.check_crop_valid(region)` accepts
    (boxs: the clip's box list, duck-typed; None accepts the first)."""
    flip = random.random() < flip_prob
    sizes = _scales(resolution, aug_scale)
    steps: List[tuple] = []
    if random.random() < 0.5:
        steps.append(("resize",) + _draw_resize(h, w, sizes, MAX_SIZE))
    else:
        ch, cw = _draw_resize(h, w, CROP_RESIZES, None)
        steps.append(("resize", ch, cw))
        if boxs is not None:
            boxs = (boxs.transpose(0) if flip else boxs).resize((cw, ch))
        for _ in range(CROP_TRIES):
            tw = random.randint(CROP_MIN, min(cw, CROP_MAX))
            th = random.randint(CROP_MIN, min(ch, CROP_MAX))
            region = _draw_corner(ch, cw, th, tw)
            if boxs is None or boxs.check_crop_valid(region):
                steps.append(("crop",) + region)
                ch, cw = th, tw
                break
        steps.append(("resize",) + _draw_resize(ch, cw, sizes, MAX_SIZE))
    return ClipPlan(h, w, flip, steps, mean, std, antialias)


def eval_plan(h: int, w: int, resolution: int = 448, *, mean=ops.PIXEL_MEAN, std=ops.PIXEL_STD,
              antialias: bool = False) -> ClipPlan:
    """the evaluation transforms: one resize to `resolution` (long side capped at 720) and the normalise"""
    return ClipPlan(h, w, False, [("resize",) + _draw_resize(h, w, (resolution,), MAX_SIZE)], mean, std, antialias)
