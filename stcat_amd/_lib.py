"""ctypes binding of libstcat_hip.so (C ABI declared in include/stcat_hip.h).

The product path has exactly one backend: the HIP library built for gfx950.
If it is missing, loading fails loudly — there is no CPU or PyTorch fallback.
(The CPU test-suite binds the host SIMT emulator build of the *same* kernel sources
from its own side — tests/backends.py::use_emu — nothing in the package does.)
"""
from __future__ import annotations

import ctypes
import os
from typing import Dict, Optional, Tuple

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libstcat_hip.so")

# name -> argument kinds of the library bound last, read from the library's own table (_bind; csrc/entry_points.h):
# p = device pointer, P = host pointer, s = stream (void*), S = C string, i = int, l = long, f = float, u = unsigned 64-bit
SIGNATURES: Dict[str, str] = {}
_CT = {"p": ctypes.c_void_p, "i": ctypes.c_int, "l": ctypes.c_long, "f": ctypes.c_float, "s": ctypes.c_void_p,
       "P": ctypes.c_void_p,  # P = HOST pointer (small by-value arrays, plan handles)
       "u": ctypes.c_ulonglong, "S": ctypes.c_char_p}

EW_ADD, EW_MUL, EW_SIGMOID, EW_TANH, EW_RELU, EW_INVSIG = 0, 1, 2, 3, 4, 5
EW_SIGMOID_BWD, EW_TANH_BWD, EW_INVSIG_BWD, EW_ADD3, EW_AXPBY, EW_COPY = 6, 7, 8, 9, 10, 11
EW_GELU, EW_GELU_BWD = 12, 13       # erf-GELU and its backward (a = dy, b = x)

_lib: Optional[ctypes.CDLL] = None
_backend = "hip"


class StcatHipError(RuntimeError):
    pass


def _bind(lib: ctypes.CDLL) -> ctypes.CDLL:
    global SIGNATURES
    lib.stcat_entry_name.restype = lib.stcat_entry_kinds.restype = ctypes.c_char_p
    table = {lib.stcat_entry_name(i).decode(): lib.stcat_entry_kinds(i).decode() for i in range(lib.stcat_entry_count())}
    for name, sig in table.items():
        fn = getattr(lib, name)  # AttributeError if the library does not export it
        if not set(sig) <= set(_CT):
            raise StcatHipError(f"{name}: unknown argument kind in {sig!r}")
        fn.argtypes = [_CT[c] for c in sig]
        fn.restype = ctypes.c_int
    SIGNATURES = table
    lib.stcat_plan_create.restype = ctypes.c_void_p
    lib.stcat_version.restype = ctypes.c_int
    lib.stcat_last_error.restype = ctypes.c_char_p
    return lib


def load(path: str = LIB_PATH) -> ctypes.CDLL:
    global _lib
    if _lib is None:
        if not os.path.exists(path):
            raise StcatHipError(
                f"{path} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "(hipcc --offload-arch=gfx950). stcat_amd has no CPU/PyTorch fallback.")
        _lib = _bind(ctypes.CDLL(path))
        flags = os.environ.get("STCAT_PL_FLAGS")       # timing experiments only (stcat_debug_pl_flags: A/B of kernel variants)
        if flags:
            _lib.stcat_debug_pl_flags(int(flags))
    return _lib


def backend() -> str:
    return _backend


MMA_MODES = {"f32": 0, "bf16x3": 2, "bf16x6": 3, "bf16x3p": 4, "bf16x6p": 5, "f16x3p": 6}
PLANE_MODES = {"bf16x3p": 2, "bf16x6p": 3, "f16x3p": 2}   # mode -> 16-bit planes per backbone tensor
_mode_cache = None


def set_mma_mode(mode: str) -> None:
    """Arithmetic of the conv / Linear GEMM family: 'f32' (exact fp32 MFMA), 'bf16x3' or 'bf16x6'
    (fp32 operands split into bf16 pieces on the bf16 matrix pipe, fp32 accumulate), or 'bf16x3p': the bf16x3
    arithmetic with the backbone's activations / gradients / weights kept PRE-SPLIT as bf16 hi/lo planes in HBM
    (csrc/igemm_pl.h: LDS-DMA staged 256-wide tiles); all other GEMMs run as 'bf16x3'.  'bf16x6p' is the fp32-class
    form of that layout: THREE bf16 planes per tensor (hi + mid + lo = the fp32 value exactly), six cross terms per
    product; all other GEMMs run as 'bf16x6' and attention on the fp32 matrix pipe.  'f16x3p' (round 4, experimental): TWO
    fp16 planes per backbone tensor (22 significand bits, three products), weights / gradients scaled by powers of two
    into fp16's range (`f16_grad_scale()`); everything outside the backbone as in 'bf16x6p'."""
    global _mode_cache
    call("stcat_set_mma_mode", MMA_MODES[mode])
    _mode_cache = mode


def get_mma_mode() -> str:
    global _mode_cache
    if _mode_cache is None:
        code = load().stcat_get_mma_mode()
        _mode_cache = {v: k for k, v in MMA_MODES.items()}[code]
    return _mode_cache


_det_cache = (None, False)    # (library handle, mode): the plan signature asks once per node, a ctypes call each is too dear


def set_deterministic(on: bool) -> None:
    """Process-wide deterministic mode (off by default; STCAT_DETERMINISTIC=1 turns it on when the library is loaded):
    every float sum of a training step runs in an order fixed by shapes, the mma mode and the CU count, so two runs from
    one seed give the same bits.  While it is on, an entry point without an ordered form raises instead of falling back
    to float atomics (the contract of torch.use_deterministic_algorithms).  Launch plans recorded in one mode are not
    replayed in the other (the mode is part of the plan signature)."""
    call("stcat_set_deterministic", 1 if on else 0)     # (call() drops the cached mode)


def is_deterministic() -> bool:
    global _det_cache
    lib = load()
    if _det_cache[0] is not lib:
        _det_cache = (lib, bool(lib.stcat_get_deterministic()))
    return _det_cache[1]


def deterministic_requested() -> bool:
    """is_deterministic() without loading the library: the loaded library's mode, else what STCAT_DETERMINISTIC sets it
    to when the library is loaded (the library's own reading: anything but empty or 0)"""
    if _lib is not None:
        return is_deterministic()
    return os.environ.get("STCAT_DETERMINISTIC", "") not in ("", "0")


_UNSET = object()
_window = _UNSET              # set_canonical_window's argument; _UNSET: STCAT_CANONICAL_WINDOW decides
_window_env = (None, None)    # (the variable's text, what it parsed to)
WINDOW_MAX = 128              # clips of one canonical window: world <= 8 ranks (stcat_rank_tree_sum) x k <= 16 micro-steps


def _check_window(n, what: str) -> int:
    if isinstance(n, bool) or not isinstance(n, int) or n < 1 or n & (n - 1) or n > WINDOW_MAX:
        raise ValueError(f"{what}={n!r}: the canonical window is a power of two of clips, 1 .. {WINDOW_MAX}")
    return n


def set_canonical_window(n: Optional[int]) -> None:
    """The canonical window (opt-in, needs deterministic mode): `n` clips per optimizer step, a power of two that the
    world size divides.  While it is on, the mean gradient of an optimizer step is ONE fp32 expression over the clips
    c = 0 .. n - 1 of the step — the balanced binary tree ((g0 + g1) + (g2 + g3)) + ..., times fp32(1 / n) once — whatever
    the split into ranks and micro-steps (clip c = micro-step * world + rank), so a run gives the same weights on 1, 2, 4 or
    8 GPUs: the ordered exchange adds the ranks with stcat_rank_tree_sum at every world size from two, AdamW.accumulate() /
    step() add the micro-steps with stcat_grad_tree_fold, the dropout seed leaves the rank out and its counters follow the
    global clip number (ops.dropout_begin_step(device, clip=...)), and TrainStep.window normalises the loss by the window's
    box count.  `None` turns it off (STCAT_CANONICAL_WINDOW=n is what holds when this was never called).  The setting is
    part of the launch-plan signature."""
    global _window
    if n is not None:
        _check_window(n, "set_canonical_window: n")
        if not deterministic_requested():
            raise ValueError("set_canonical_window: the canonical window needs deterministic mode "
                             "(stcat_amd.set_deterministic(True) or STCAT_DETERMINISTIC=1) — without it the kernels "
                             "of a step add in an order of their own and no layout repeats even itself")
    _window = n


def canonical_window() -> Optional[int]:
    """the canonical window's clip count, None: off.  Does not load the kernel library."""
    global _window_env
    n = _window
    if n is _UNSET:
        env = os.environ.get("STCAT_CANONICAL_WINDOW", "")
        if env != _window_env[0]:
            if env in ("", "0"):
                _window_env = (env, None)
            else:
                if not env.isdigit():
                    raise ValueError(f"STCAT_CANONICAL_WINDOW={env!r}: expected a number of clips")
                _window_env = (env, _check_window(int(env), "STCAT_CANONICAL_WINDOW"))
        n = _window_env[1]
    if n is not None and not deterministic_requested():
        raise ValueError(f"canonical window of {n} clips: it needs deterministic mode, which is off "
                         "(stcat_amd.set_deterministic(True) or STCAT_DETERMINISTIC=1)")
    return n


def window_micro_steps(world: int) -> Optional[int]:
    """k = N / world of the canonical window (None: the mode is off); a world that does not divide N is refused"""
    n = canonical_window()
    if n is None:
        return None
    if world < 1 or n % world:
        raise ValueError(f"canonical window of {n} clips: the world size {world} does not divide it")
    if n // world > 16:
        raise ValueError(f"canonical window of {n} clips on {world} rank(s): {n // world} micro-steps (at most 16)")
    return n // world


def f16_grad_scale() -> float:
    """factor carried by every GRADIENT plane in mode f16x3p (1.0 in every other mode): tools / op tests that build
    gradient planes themselves multiply by it; the product path scales where gradients enter the backbone (pl_act_bwd)"""
    return float(2 ** load().stcat_get_f16_scale(1)) if get_mma_mode() == "f16x3p" else 1.0


def plane_count() -> int:
    """bf16 planes per backbone tensor in the current mode (0: the mode keeps fp32 tensors)"""
    return PLANE_MODES.get(get_mma_mode(), 0)


def _ptr(t):
    if t is None:
        return None
    if isinstance(t, int):
        return t
    return t.data_ptr()


def stream_of(t: torch.Tensor):
    """raw hipStream_t of torch's CURRENT stream on t's device (honours torch.cuda.stream(...) contexts)"""
    if _backend == "emu":
        return None
    # torch.cuda.current_stream() builds a Stream object (~5 us, ~1750 launches per step); the raw getter is ~0.3 us
    return torch._C._cuda_getCurrentRawStream(t.device.index if t.device.index is not None else torch.cuda.current_device())


def check_tensor(t: torch.Tensor, name: str = "tensor") -> torch.Tensor:
    if _backend == "hip" and not t.is_cuda:
        raise StcatHipError(f"{name} must live on the GPU (got {t.device}); stcat_amd has no CPU path")
    if _backend == "emu" and t.is_cuda:
        raise StcatHipError("emulator backend takes CPU tensors")
    return t


RECORDER = None  # stcat_amd.plans.Recorder while a launch plan is being recorded (the calls still execute)


def call(name: str, *args) -> None:
    global _det_cache
    lib = load()
    rc = getattr(lib, name)(*args)
    if name == "stcat_set_deterministic":
        _det_cache = (None, False)      # re-read from the library: the setter may refuse
    if rc != 0:
        msg = lib.stcat_last_error()
        raise StcatHipError(f"{name} failed (rc={rc}): {msg.decode() if msg else ''}")
    if RECORDER is not None:
        RECORDER.add_call(name, args)


def pin_host_threads_to_gpu(device_index: int = 0) -> Optional[str]:
    """Restrict this process to the CPUs of the NUMA node the GPU hangs off (`/sys/bus/pci/devices/<bdf>/local_cpulist`).
    The 8-GPU MI355X hosts are two-socket machines with four GPUs per socket; one process per GPU keeps its launching
    threads (python, the autograd engine thread, the HIP runtime's) on the GPU's socket, so eight ranks do not migrate
    across each other's cores.  On an otherwise idle host the step time is the same from either socket (measured:
    62.9 ms pinned, unpinned and from the remote socket) — this is hygiene for the 8-rank launch, not a speed-up.
    Returns the cpulist used, or None when the topology is not visible (then nothing changes)."""
    import torch
    try:
        pr = torch.cuda.get_device_properties(device_index)
        bdf = f"{getattr(pr, 'pci_domain_id', 0):04x}:{pr.pci_bus_id:02x}:{getattr(pr, 'pci_device_id', 0):02x}.0"
        with open(f"/sys/bus/pci/devices/{bdf}/local_cpulist") as f:
            cpulist = f.read().strip()
        cpus = set()
        for part in cpulist.split(","):
            if "-" in part:
                a, b = part.split("-")
                cpus.update(range(int(a), int(b) + 1))
            elif part:
                cpus.add(int(part))
        cpus &= os.sched_getaffinity(0)
        if not cpus:
            return None
        for tid in os.listdir("/proc/self/task"):      # every thread that already exists (HIP runtime, torch pools);
            try:                                        # threads created later inherit the mask
                os.sched_setaffinity(int(tid), cpus)
            except OSError:
                pass
        return cpulist
    except (OSError, AttributeError, ValueError, RuntimeError):
        return None
