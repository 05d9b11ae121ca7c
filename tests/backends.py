"""Backend selection for the kernel tests.

`hip`  : the product library stcat_amd/lib/libstcat_hip.so on cuda:0 (tests marked gpu).
`emu`  : the SAME kernel sources compiled for the host SIMT emulator (tests/emu/), CPU
         tensors — checks index logic and the autograd wiring without a GPU.
"""
import contextlib
import fcntl
import os
import subprocess
import time

import pytest
import torch

from stcat_amd import _lib as L

HERE = os.path.dirname(os.path.abspath(__file__))
BUILD_DIR = os.path.join(HERE, "emu", "_build")
EMU_SO = os.path.join(BUILD_DIR, "libstcat_emu.so")
_emu_state = {"built": False, "error": None}


@contextlib.contextmanager
def _file_lock(path):
    """exclusive lock shared by every test process of this checkout (pytest-xdist workers included)"""
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "a") as f:
        fcntl.flock(f, fcntl.LOCK_EX)
        try:
            yield
        finally:
            fcntl.flock(f, fcntl.LOCK_UN)


def _build_emu():
    """Build the emulator library once per checkout: when the caller chose the xdist worker count, every worker reaches
    this at the same time — one compiles under the lock (into a temporary file that replaces the library in one rename),
    the others wait and then find it fresh."""
    if _emu_state["built"] or _emu_state["error"]:
        return
    srcs = [os.path.join(HERE, "emu", f) for f in ("hip_emu.h", "emu_main.cpp")]
    csrc = os.path.join(HERE, "..", "stcat_amd", "csrc")
    srcs += [os.path.join(csrc, f) for f in os.listdir(csrc)]
    srcs.append(os.path.join(HERE, "..", "include", "stcat_hip.h"))
    with _file_lock(os.path.join(BUILD_DIR, ".build.lock")):
        fresh = os.path.exists(EMU_SO) and all(os.path.getmtime(EMU_SO) >= os.path.getmtime(s) for s in srcs)
        if not fresh:
            tmp = f"{EMU_SO}.{os.getpid()}.tmp"
            r = subprocess.run(["sh", os.path.join(HERE, "emu", "build_emu.sh"), tmp], capture_output=True, text=True)
            if r.returncode != 0:
                _emu_state["error"] = r.stderr[-2000:]
                if os.path.exists(tmp):
                    os.remove(tmp)
                return
            os.replace(tmp, EMU_SO)
    _emu_state["built"] = True


HEAVY_TEST_BYTES = 4 << 30   # peak host memory of one model-level CPU test (measured: 2.7 - 3.1 GB at C1 / tiny clips)


def _host_memory_bytes():
    """memory this process may use: the machine's, or its cgroup's limit where that is lower"""
    with open("/proc/meminfo") as f:
        total = next(int(l.split()[1]) * 1024 for l in f if l.startswith("MemTotal:"))
    for path in ("/sys/fs/cgroup/memory.max", "/sys/fs/cgroup/memory/memory.limit_in_bytes"):
        try:
            with open(path) as f:
                v = f.read().strip()
        except OSError:
            continue
        if v.isdigit():
            total = min(total, int(v))
    return total


def heavy_test_slots():
    """how many model-level CPU tests may hold memory at once: 60 % of the host (or cgroup) memory in 4 GB slots"""
    return max(1, int(0.6 * _host_memory_bytes()) // HEAVY_TEST_BYTES)


_slot_held = [False]


@contextlib.contextmanager
def host_memory_slot():
    """Hold one of heavy_test_slots() slots for the duration of a model-level CPU test.  With as many pytest-xdist
    workers as the caller asks for, every worker would otherwise start one of these ~3 GB tests at once (they are
    scheduled first); beyond the slots, a worker waits here.  Slots are file locks, released when the process ends."""
    if _slot_held[0]:                # (nested: this process already holds a slot)
        yield
        return
    slots = heavy_test_slots()
    os.makedirs(BUILD_DIR, exist_ok=True)
    while True:
        for i in range(slots):
            f = open(os.path.join(BUILD_DIR, f".memory_slot_{i}.lock"), "a")
            try:
                fcntl.flock(f, fcntl.LOCK_EX | fcntl.LOCK_NB)
            except OSError:
                f.close()
                continue
            _slot_held[0] = True
            try:
                yield
            finally:
                _slot_held[0] = False
                fcntl.flock(f, fcntl.LOCK_UN)
                f.close()
            return
        time.sleep(0.5)


def use_emu():
    _build_emu()
    if _emu_state["error"]:
        pytest.skip("host emulator build failed: " + _emu_state["error"])
    # bind the emulator build in place of libstcat_hip.so (test-side only: the package has no such switch)
    import ctypes
    L._lib = L._bind(ctypes.CDLL(EMU_SO))
    L._backend = "emu"
    L._mode_cache = None
    return torch.device("cpu")


def use_hip():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    L._lib = None
    L._backend = "hip"
    L._mode_cache = None
    L.load()
    return torch.device("cuda:0")


@contextlib.contextmanager
def deterministic(on=True):
    L.set_deterministic(on)
    try:
        yield
    finally:
        L.set_deterministic(False)


def both(fn):
    """Register fn(dev, big) twice: test_emu_<name> (CPU, emulator) and test_gpu_<name> (marked gpu)."""
    import sys
    mod = sys.modules[fn.__module__]
    name = fn.__name__.lstrip("_")

    def emu_test():
        fn(use_emu(), False)

    def gpu_test():
        fn(use_hip(), True)

    emu_test.__name__ = f"test_emu_{name}"
    gpu_test.__name__ = f"test_gpu_{name}"
    setattr(mod, emu_test.__name__, emu_test)
    setattr(mod, gpu_test.__name__, pytest.mark.gpu(gpu_test))
    return fn


def close(a, b, tol, what, absolute=False):
    """max |a - b| <= tol * max(1, |b|max); absolute=True drops the scale factor (the north-star bar for the model's
    box / logit tensors is an ABSOLUTE 1e-3, BASELINE.json)."""
    a = a.detach().double().cpu()
    b = b.detach().double().cpu()
    assert a.shape == b.shape, (what, tuple(a.shape), tuple(b.shape))
    err = (a - b).abs().max().item() if a.numel() else 0.0
    scale = 1.0 if absolute else max(1.0, b.abs().max().item() if b.numel() else 1.0)
    assert err <= tol * scale, f"{what}: max abs err {err:.3e} (scale {scale:.3g}) > tol {tol}"
    return err
