"""Device-side clip transforms: the stcat_clip_resize kernel (csrc/clip_transform.h), transforms.ClipPlan / the plan
sampling, loader.DeviceClipLoader.

Yardstick: torch on the CPU, never our own output.  R64 is the plan evaluated in float64 (`_reference`), R32 the same
evaluation in float32 — what a loader worker of the reference computes.  The bar is

    max|ours - R64| <= 2 * max|R32 - R64| + 4.8e-7

(the factor 2 for a different order of the four products and the constants folded into one multiply-add; the floor is
one fp32 ulp at the largest normalised magnitude, 2.64).  Setting CLIP_TRANSFORM_ERROR_JSON=<path> records every
measured pair there (one process: `-n1`; profiles/clip_transform_error.json is such a record).  max|R32 - R64| is 1e-5 to
2e-4 at these sizes, not a few 1e-6: torch forms the scale and the source coordinate in the tensor's own precision, so in
float32 a coordinate near column 640 is off by up to 4e-5 of a pixel; the kernel forms them the same way, so its distance
to R64 is R32's own (measured ratio to the bar: 0.28 - 0.51)."""
import importlib.util
import json
import os
import random
import sys
import types

import pytest
import torch
import torch.nn.functional as F

from stcat_amd import _lib as L
from stcat_amd import ops, transforms
from stcat_amd.transforms import ClipPlan, eval_plan, sample_train_plan
from tests.backends import both

REFERENCE = "/root/reference"
SIZES = (448, 416, 384, 352)


def _source(T, h, w, u8, seed):
    g = torch.Generator().manual_seed(seed)
    if u8:
        return torch.randint(0, 256, (T, h, w, 3), dtype=torch.uint8, generator=g)
    return torch.rand(T, 3, h, w, generator=g)


def _reference(src, plan, dtype):
    """the plan as torch CPU ops in `dtype`: ToTensor, flip, interpolate / slice per step, normalise"""
    x = src.permute(0, 3, 1, 2).to(dtype) / 255 if src.dtype == torch.uint8 else src.to(dtype)
    if plan.flip:
        x = x.flip(-1)
    for s in plan.steps:
        if s[0] == "resize":
            x = F.interpolate(x, size=(s[1], s[2]), mode="bilinear", align_corners=False, antialias=plan.antialias)
        else:
            _, i, j, th, tw = s
            x = x[:, :, i:i + th, j:j + tw]
    mean = torch.tensor(plan.mean, dtype=dtype)[:, None, None]
    std = torch.tensor(plan.std, dtype=dtype)[:, None, None]
    return (x - mean) / std


_R = {}


def _yardstick(src, plan, key):
    """(R64, max|R32 - R64|), computed once per case and shared by the emulator and the GPU test"""
    if key not in _R:
        r64 = _reference(src, plan, torch.float64)
        _R[key] = (r64, (_reference(src, plan, torch.float32).double() - r64).abs().max().item())
    return _R[key]


def _bar(ours, src, plan, key):
    r64, e32 = _yardstick(src, plan, key)
    assert tuple(ours.shape) == tuple(r64.shape), (key, tuple(ours.shape), tuple(r64.shape))
    err = (ours.detach().cpu().double() - r64).abs().max().item()
    print(f"{L.backend()} {key}: ours {err:.3e}  R32 {e32:.3e}")
    path = os.environ.get("CLIP_TRANSFORM_ERROR_JSON")
    if path:
        rec = json.load(open(path)) if os.path.exists(path) else {}
        rec[f"{L.backend()} {key}"] = {"ours_vs_R64": err, "R32_vs_R64": e32}
        json.dump(rec, open(path, "w"), indent=1, sort_keys=True)
    assert err <= 2 * e32 + 4.8e-7, f"{key}: max|ours - R64| = {err:.3e} > 2 * {e32:.3e} + 4.8e-7"


def _norm(dev, u8):
    if u8:
        return ops.u8_norm(dev)
    return transforms._affine(dev, [1.0 / s for s in ops.PIXEL_STD], [-m / s for m, s in zip(ops.PIXEL_MEAN, ops.PIXEL_STD)])


def _unit(dev):
    return torch.ones(3, device=dev), torch.zeros(3, device=dev)


@both
def _resize_kernel(dev, big):
    """one launch against torch's interpolate: up, down, mixed and same size; rows of 41, 91, 70, 53 floats start
    unaligned; (64,91) and (20,70) span several tiles"""
    for u8 in (True, False):
        src = _source(2, 37, 53, u8, 1)
        a, b = _norm(dev, u8)
        for size in ((29, 41), (64, 91), (20, 70), (37, 53)):
            for aa in (False, True):
                for flip in (False, True):
                    plan = ClipPlan(37, 53, flip, [("resize",) + size], antialias=aa)
                    y = ops.clip_resize_raw(src.to(dev), a, b, size, flip=flip, antialias=aa)
                    _bar(y, src, plan, f"resize u8={int(u8)} {size[0]}x{size[1]} aa={int(aa)} flip={int(flip)}")


@both
def _identity_is_exact(dev, big):
    src = _source(2, 37, 53, False, 2)
    a, b = _unit(dev)
    for aa in (False, True):
        assert torch.equal(ops.clip_resize_raw(src.to(dev), a, b, antialias=aa).cpu(), src)
        assert torch.equal(ops.clip_resize_raw(src.to(dev), a, b, flip=True, antialias=aa).cpu(), src.flip(-1))


@both
def _output_window(dev, big):
    """an output window is the slice of the full result, bit for bit: tap weights and sums do not depend on the tiling"""
    for u8 in (True, False):
        src = _source(2, 37, 53, u8, 3).to(dev)
        a, b = _norm(dev, u8)
        for aa in (False, True):
            for flip in (False, True):
                full = ops.clip_resize_raw(src, a, b, (50, 72), flip=flip, antialias=aa)
                for win in ((0, 0, 50, 72), (7, 11, 31, 41), (33, 49, 17, 23)):
                    y, x, h, w = win
                    part = ops.clip_resize_raw(src, a, b, (50, 72), flip=flip, antialias=aa, out_window=win)
                    assert torch.equal(part, full[:, :, y:y + h, x:x + w]), (u8, aa, flip, win)


@both
def _clamp_window(dev, big):
    """taps clamp at the window, not at the image: a window equals the resize of the sliced source, bit for bit"""
    y0, x0, wh, ww = 3, 5, 29, 41
    for u8 in (True, False):
        src = _source(2, 37, 53, u8, 4)
        cut = (src[:, y0:y0 + wh, x0:x0 + ww] if u8 else src[:, :, y0:y0 + wh, x0:x0 + ww]).contiguous()
        a, b = _norm(dev, u8)
        for aa in (False, True):
            for flip in (False, True):
                for size in ((40, 64), (17, 23)):
                    got = ops.clip_resize_raw(src.to(dev), a, b, size, window=(y0, x0, wh, ww), flip=flip, antialias=aa)
                    want = ops.clip_resize_raw(cut.to(dev), a, b, size, flip=flip, antialias=aa)
                    assert torch.equal(got, want), (u8, aa, flip, size)


@both
def _reference_geometries(dev, big):
    """the two plans of the training transforms at a 360 x 640 clip, through ClipPlan.apply: the single resize at the 720
    cap, and resize -> crop -> resize with a flip — two launches, the crop folded into the first one's output window"""
    src = _source(3, 360, 640, True, 5)
    single = ClipPlan(360, 640, False, [("resize", 405, 720)])
    cropped = ClipPlan(360, 640, True, [("resize", 500, 888), ("crop", 37, 111, 431, 577), ("resize", 416, 556)])
    assert single.out_size() == (405, 720) and cropped.out_size() == (416, 556)
    calls = []
    real = L.call

    def counting(name, *args):
        calls.append(name)
        return real(name, *args)

    L.call = counting
    try:
        y1 = single.apply(src.to(dev))
        assert calls == ["stcat_clip_resize"], calls
        del calls[:]
        y2 = cropped.apply(src.to(dev))
        assert calls == ["stcat_clip_resize"] * 2, calls
    finally:
        L.call = real
    _bar(y1, src, single, "plan 360x640 -> 405x720")
    _bar(y2, src, cropped, "plan 360x640 flip -> 500x888 -> crop 431x577 -> 416x556")


@both
def _bad_arguments(dev, big):
    src = _source(1, 37, 53, True, 6).to(dev)
    a, b = _norm(dev, True)
    out = torch.full((1, 3, 8, 8), 7.0, device=dev)
    for window, what in (((0, 0, 0, 5), "empty"), ((30, 0, 10, 53), "leaves"), ((0, 50, 37, 4), "leaves")):
        with pytest.raises(L.StcatHipError, match=r"rc=-1.*" + what):
            ops.clip_resize_raw(src, a, b, (8, 8), window=window, out=out)
    with pytest.raises(L.StcatHipError, match=r"rc=-1.*output window"):
        ops.clip_resize_raw(src, a, b, (8, 8), out_window=(1, 0, 8, 8), out=out)
    assert bool((out == 7.0).all())          # nothing was launched


@both
def _plan_without_resize(dev, big):
    """flip + crop + normalise alone still run as one identity-scale launch; every value is one rounded multiply-add"""
    src = _source(2, 37, 53, True, 7)
    plan = ClipPlan(37, 53, True, [("crop", 3, 6, 30, 41)])
    assert len(plan.launches()) == 1
    _bar(plan.apply(src.to(dev)), src, plan, "plan flip + crop only")


@pytest.mark.gpu
def test_gpu_loader():
    """five clips of three source shapes and both formats through DeviceClipLoader: each equals a direct apply bit for
    bit while a queue of consumer work reads the previous output; four device buffers serve all five"""
    from stcat_amd.loader import DeviceClipLoader
    from tests.backends import use_hip
    dev = use_hip()
    shapes = [(4, 96, 128), (4, 90, 120), (4, 64, 80), (4, 90, 120), (4, 64, 80)]    # each slot's largest clip first
    random.seed(11)
    torch.manual_seed(11)
    clips = []
    for k, (T, h, w) in enumerate(shapes):
        src = _source(T, h, w, k != 0, 20 + k)
        if k == 1:
            src = src.pin_memory()
        plan = ClipPlan(h, w, k % 2 == 1, [("resize", 150, 200), ("crop", 5, 7, 100 + k, 131), ("resize", 90 - k, 117)]) \
            if k % 2 == 0 else ClipPlan(h, w, True, [("resize", 96 - k, 131 - k)])
        clips.append((src, plan))
    want = [plan.apply(src.to(dev)).clone() for src, plan in clips]
    loader = DeviceClipLoader(iter(clips), dev)
    got, ptrs = [], []
    acc = torch.zeros((), device=dev)
    for fr in loader:
        ptrs.append(fr.data_ptr())
        for _ in range(20):
            acc = acc * 0.5 + fr.sum()
        got.append(fr.clone())
    torch.cuda.synchronize()
    assert len(got) == len(clips)
    for a, b in zip(got, want):
        assert a.shape == b.shape and torch.equal(a, b)
    assert loader.allocations == 4, loader.allocations
    assert ptrs[0] == ptrs[2] == ptrs[4] and ptrs[1] == ptrs[3] and ptrs[0] != ptrs[1]


@pytest.mark.gpu
def test_gpu_loader_declares_the_next_clip_to_the_backbone():
    """DeviceClipLoader(stage=Backbone.stage_next): every hand-over declares the NEXT clip with the event of its
    transform, its frozen prefix runs under the current step, and the features equal a plain pass over the directly
    transformed frames bit for bit (the pattern of tests/test_loader.py, with sources of three shapes)"""
    from stcat_amd import backbone
    from stcat_amd.loader import DeviceClipLoader
    from stcat_amd import synth
    from tests.backends import use_hip
    dev = use_hip()
    L.set_mma_mode("bf16x6p")
    try:
        enc = backbone.build_vis_encoder(None)
        synth.fill_module_(enc)
        enc.to(dev)
        bb = enc[0]
        clips = []
        for k, (h, w) in enumerate(((120, 160), (96, 128), (120, 160), (150, 200))):
            clips.append((_source(8, h, w, True, 40 + k), ClipPlan(h, w, k % 2 == 1, [("resize", 224, 224)])))
        with torch.no_grad():
            want = [bb.features_nhwc(plan.apply(src.to(dev))).clone() for src, plan in clips]
            got = []
            taken0 = bb.prefix_stats["taken"]
            for fr in DeviceClipLoader(iter(clips), dev, stage=bb.stage_next):
                got.append(bb.features_nhwc(fr).clone())
                ops.run_deferred()
        torch.cuda.synchronize()
        assert bb.prefix_stats["taken"] - taken0 == len(clips) - 1, bb.prefix_stats
        for a, b in zip(got, want):
            assert torch.equal(a, b)
    finally:
        L.set_mma_mode("f32")


# ---- the plan sampling: CPU only --------------------------------------------------------------------------------------

def _rule(h, w, size, cap):
    """the resize rule, restated: short side `size`, long side by the aspect ratio (truncated), the long side capped"""
    short, long_ = min(h, w), max(h, w)
    if cap is not None and long_ / short * size > cap:
        size = int(round(cap * short / long_))
    if short == size:
        return h, w
    other = int(size * long_ / short)
    return (other, size) if w < h else (size, other)


class _RejectAll:
    def __init__(self):
        self.checked = 0

    def transpose(self, method):
        return self

    def resize(self, size):
        return self

    def check_crop_valid(self, region):
        self.checked += 1
        return False


def test_plan_draws():
    assert _rule(360, 640, 448, 720) == (405, 720) and _rule(640, 360, 448, 720) == (720, 405)
    assert _rule(360, 640, 384, 720) == (384, 682) and _rule(480, 480, 416, 720) == (416, 416)
    for h, w in ((360, 640), (640, 360), (480, 480), (1080, 1920)):
        allowed = {_rule(h, w, s, 720) for s in SIZES}
        firsts = {_rule(h, w, s, None) for s in (400, 500, 600)}
        seen = set()
        for seed in range(60):
            random.seed(seed)
            torch.manual_seed(seed)
            plan = sample_train_plan(h, w)
            random.seed(seed)
            torch.manual_seed(seed)
            again = sample_train_plan(h, w)
            assert repr(plan) == repr(again)               # a pure function of the two seeds
            kinds = [s[0] for s in plan.steps]
            seen.add((plan.flip, tuple(kinds)))
            if kinds == ["resize"]:
                assert plan.steps[0][1:] in allowed, plan
                continue
            assert kinds == ["resize", "crop", "resize"], plan       # (without boxes the first candidate is taken)
            assert plan.steps[0][1:] in firsts, plan
            rh, rw = plan.steps[0][1:]
            _, i, j, th, tw = plan.steps[1]
            assert 384 <= th <= min(rh, 600) and 384 <= tw <= min(rw, 600), plan
            assert 0 <= i <= rh - th and 0 <= j <= rw - tw, plan
            assert plan.steps[2][1:] in {_rule(th, tw, s, 720) for s in SIZES}, plan
            assert plan.out_size() == plan.steps[2][1:]
        assert seen == {(f, k) for f in (False, True) for k in (("resize",), ("resize", "crop", "resize"))}, seen
    # the short side already has the drawn size: the clip keeps its size
    assert eval_plan(448, 600).steps == [("resize", 448, 600)]
    assert eval_plan(360, 640).steps == [("resize", 405, 720)] and eval_plan(360, 640).flip is False
    assert sample_train_plan(448, 600, aug_scale=False, flip_prob=0.0).steps[-1][0] == "resize"
    # boxes that no crop keeps: 50 candidates are drawn, then the clip goes on uncropped
    n_crop_branch = 0
    for seed in range(12):
        random.seed(seed)
        torch.manual_seed(seed)
        boxs = _RejectAll()
        plan = sample_train_plan(360, 640, boxs=boxs)
        if len(plan.steps) == 1:
            assert boxs.checked == 0
            continue
        n_crop_branch += 1
        assert boxs.checked == 50 and [s[0] for s in plan.steps] == ["resize", "resize"], plan
        assert plan.steps[1][1:] in {_rule(*plan.steps[0][1:], s, 720) for s in SIZES}
    assert n_crop_branch >= 2
    # the words of a mirrored clip
    assert ClipPlan(8, 8, True).swap_left_right("the left man right of the leftmost") == "the right man left of the rightmost"
    assert ClipPlan(8, 8, False).swap_left_right("left") == "left"


def _torchvision_stand_in(log):
    """a minimal torchvision over torch: what datasets/transforms.py of the reference uses, the tensor forms of
    torchvision 0.11 (resize = bilinear interpolate without antialiasing).  RandomCrop.get_params is the corner draw as
    the issue describes it — the one thing this test cannot pin against the real library."""
    tv = types.ModuleType("torchvision")
    tt = types.ModuleType("torchvision.transforms")
    tf = types.ModuleType("torchvision.transforms.functional")

    def hflip(img):
        log.append(("flip",))
        return img.flip(-1)

    def resize(img, size):
        log.append(("resize", int(size[0]), int(size[1])))
        return F.interpolate(img, size=tuple(size), mode="bilinear", align_corners=False)

    def crop(img, top, left, height, width):
        log.append(("crop", top, left, height, width))
        return img[..., top:top + height, left:left + width]

    def normalize(img, mean, std):
        m = torch.tensor(mean, dtype=img.dtype)[:, None, None]
        s = torch.tensor(std, dtype=img.dtype)[:, None, None]
        return (img - m) / s

    class RandomCrop:
        @staticmethod
        def get_params(img, output_size):
            h, w = img.shape[-2:]
            th, tw = output_size
            if h == th and w == tw:
                return 0, 0, h, w
            i = torch.randint(0, h - th + 1, size=(1,)).item()
            j = torch.randint(0, w - tw + 1, size=(1,)).item()
            return i, j, th, tw

    class ColorJitter:
        def __init__(self, **kwargs):
            pass

        def __call__(self, img):
            return img

    tf.hflip, tf.resize, tf.crop, tf.normalize = hflip, resize, crop, normalize
    tt.functional, tt.RandomCrop, tt.ColorJitter = tf, RandomCrop, ColorJitter
    tv.transforms = tt
    return {"torchvision": tv, "torchvision.transforms": tt, "torchvision.transforms.functional": tf}


@pytest.mark.skipif(not os.path.isdir(REFERENCE), reason="the reference checkout is not on this machine")
def test_plan_matches_reference_transforms(monkeypatch):
    """The reference's own datasets/transforms.py, composed as its training pipeline is (datasets/build.py:33-51), over
    a stand-in torchvision: for 20 seeds the flip, every resize size and every crop region equal sample_train_plan's, the
    boxes and the sentence equal ClipPlan's, and its output frames meet the bar against R64 of OUR plan.  This pins the
    order and the generator of every draw except the stand-in's own crop-corner draw (RandomCrop.get_params), which is
    written from the same description as transforms._draw_corner."""
    log = []
    for name, mod in _torchvision_stand_in(log).items():
        monkeypatch.setitem(sys.modules, name, mod)
    for name in [m for m in sys.modules if m == "utils" or m.startswith("utils.")]:
        monkeypatch.delitem(sys.modules, name)
    monkeypatch.syspath_prepend(REFERENCE)
    try:
        spec = importlib.util.spec_from_file_location("_reference_transforms", os.path.join(REFERENCE, "datasets", "transforms.py"))
        T = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(T)
        from utils.bounding_box import BoxList
        pipeline = T.Compose([
            T.RandomHorizontalFlip(0.5),
            T.RandomSelect(T.RandomResize(list(SIZES), max_size=720),
                           T.Compose([T.RandomResize([400, 500, 600]), T.RandomSizeCrop(384, 600),
                                      T.RandomResize(list(SIZES), max_size=720)])),
            T.Normalize(mean=list(ops.PIXEL_MEAN), std=list(ops.PIXEL_STD))])
        h, w = 90, 160
        src = _source(1, h, w, False, 9)
        boxes = torch.tensor([[20.0, 10.0, 90.0, 70.0]])
        branches = set()
        for seed in range(20):
            random.seed(seed)
            torch.manual_seed(seed)
            del log[:]
            ref = pipeline({"frames": src.clone(), "boxs": BoxList(boxes.clone(), (w, h), "xyxy"),
                            "text": "a man on the left turns right"})
            random.seed(seed)
            torch.manual_seed(seed)
            plan = sample_train_plan(h, w, boxs=BoxList(boxes.clone(), (w, h), "xyxy"))
            assert plan.flip == (("flip",) in log), (seed, plan, log)
            assert plan.steps == [s for s in log if s[0] != "flip"], (seed, plan, log)
            branches.add(tuple(s[0] for s in plan.steps))
            assert plan.swap_left_right("a man on the left turns right") == ref["text"]
            ours = plan.apply_to_boxes(BoxList(boxes.clone(), (w, h), "xyxy"))
            assert ours.mode == ref["boxs"].mode and ours.size == ref["boxs"].size
            assert torch.equal(ours.bbox, ref["boxs"].bbox)
            r64 = _reference(src, plan, torch.float64)
            e32 = (_reference(src, plan, torch.float32).double() - r64).abs().max().item()
            err = (ref["frames"].double() - r64).abs().max().item()
            assert ref["frames"].shape[-2:] == plan.out_size()
            assert err <= 2 * e32 + 4.8e-7, (seed, err, e32)
        assert ("resize",) in branches and ("resize", "crop", "resize") in branches, branches
    finally:
        for name in [m for m in sys.modules if m == "utils" or m.startswith("utils.") or m == "_reference_transforms"]:
            del sys.modules[name]
