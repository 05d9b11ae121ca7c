"""stcat_rank_sum (csrc/rank_sum.h): the cross-rank sum of the ordered gradient exchange as a fixed left-to-right chain,
   acc = in[0][i]; acc = acc + in[k][i] (k = 1 .. n_ranks - 1); out[i] = acc * scale
in fp32.  The expected result is that very loop on torch CPU tensors, compared BITWISE (torch.equal, no tolerance).  The
inputs mix magnitudes over seven decades, and every case with three or more ranks first shows that the reversed chain
gives other bits somewhere — a kernel that adds in any other order cannot pass."""
import numpy as np
import pytest
import torch

from stcat_amd import _lib as L
from tests.backends import both

RANKS = (1, 2, 3, 5, 8, 11)                      # 11 crosses the 8-rank batch boundary
SIZES = (1, 4, 63, 1000, 4096 + 3)
SCALES = (1.0, 1.0 / 3.0, 1.0 / 8.0)


def _strides(n):
    return (n, n + 5, -(-n // 64) * 64 + 64)


def _inputs(n_ranks, n, seed):
    """randn * 10 ** randint(-3, 4), element by element"""
    g = torch.Generator().manual_seed(seed)
    return torch.randn(n_ranks, n, generator=g) * 10.0 ** torch.randint(-3, 4, (n_ranks, n), generator=g).float()


def _chain(x, scale, order=None):
    order = range(x.shape[0]) if order is None else order
    order = list(order)
    acc = x[order[0]].clone()
    for k in order[1:]:
        acc = acc + x[k]
    return acc * torch.tensor(np.float32(scale))


def _check_inputs(x, scale):
    """the condition on the INPUTS: forward and reversed chains differ somewhere"""
    if x.shape[0] >= 3 and x.shape[1] >= 63:
        assert not torch.equal(_chain(x, scale), _chain(x, scale, reversed(range(x.shape[0])))), \
            "inputs do not tell the rank order apart: pick another seed"


def _call(out, buf, n_ranks, n, stride, scale):
    L.call("stcat_rank_sum", out.data_ptr(), buf.data_ptr(), n_ranks, n, stride, float(np.float32(scale)), L.stream_of(buf))


def _run(dev, n_ranks, n, stride, scale, seed, out_off=0, alias=None, in_off=0):
    """the slices laid out with `stride` in one buffer (NaN between them and behind the last: nothing else may be read
    into the result), out either a buffer of its own (offset by out_off floats from a 16-byte boundary) or slice `alias`"""
    x = _inputs(n_ranks, n, seed)
    _check_inputs(x, scale)
    want = _chain(x, scale)
    buf = torch.full((in_off + n_ranks * stride + 8,), float("nan"))
    for k in range(n_ranks):
        buf[in_off + k * stride:in_off + k * stride + n] = x[k]
    buf = buf.to(dev)
    src = buf[in_off:]
    if alias is None:
        room = torch.full((n + out_off + 8,), float("nan"), device=dev)
        out = room[out_off:out_off + n]
    else:
        room = buf
        out = src[alias * stride:alias * stride + n]
    before = room.cpu().clone()
    _call(out, src, n_ranks, n, stride, scale)
    got = out.cpu()
    assert torch.equal(got, want), (f"ranks {n_ranks} n {n} stride {stride} scale {scale} out_off {out_off} alias {alias}: "
                                    f"{int((got != want).sum())} of {n} elements differ")
    # nothing but out[0 .. n) was written
    after = room.cpu()
    lo = out_off if alias is None else in_off + alias * stride
    keep = torch.ones(after.numel(), dtype=torch.bool)
    keep[lo:lo + n] = False
    assert torch.equal(after[keep].view(torch.int32), before[keep].view(torch.int32)), "wrote outside out[0 .. n)"


@both
def _rank_sum_order(dev, big):
    seed = 0
    for n_ranks in RANKS:
        for n in SIZES:
            for si, stride in enumerate(_strides(n)):
                seed += 1
                _run(dev, n_ranks, n, stride, SCALES[(seed + si) % 3], seed)
    for scale in SCALES:                         # every scale at the batch boundary and on the vector + tail path
        for n_ranks in (3, 8, 11):
            seed += 1
            _run(dev, n_ranks, 4096 + 3, 4096 + 64, scale, seed)
    # one unaligned out (offset by one float): the scalar path; an unaligned in likewise
    _run(dev, 5, 1000, 1024, 1.0 / 3.0, 901, out_off=1)
    _run(dev, 3, 1000, 1024, 1.0 / 3.0, 902, in_off=1)
    # in place in slice 2, aligned (vector path) and with an odd stride (scalar path)
    _run(dev, 5, 4096 + 3, 4096 + 64, 1.0 / 3.0, 903, alias=2)
    _run(dev, 11, 1000, 1005, 1.0 / 8.0, 904, alias=2)
    _run(dev, 3, 63, 63, 1.0 / 3.0, 905, alias=2)
    if big:
        n = (1 << 20) + 12
        n2 = (1 << 21) + 12 + 3                  # more than one grid-stride pass of 2048 workgroups x 256 lanes x 4 floats
        assert n2 // 4 > 2048 * 256
        _run(dev, 8, n2, (1 << 21) + 64, 1.0 / 8.0, 906)
        _run(dev, 8, n, n, 1.0 / 8.0, 907)
        _run(dev, 8, n, n, 1.0 / 8.0, 908, alias=7)


@both
def _rank_sum_copy_and_empty(dev, big):
    """one rank with scale 1 is a copy (bit for bit: -0.0, infinities and NaN payloads included); n = 0 launches nothing"""
    x = _inputs(1, 1000, 5)[0]
    x[:4] = torch.tensor([-0.0, float("inf"), float("-inf"), 0.0])
    src = x.to(dev)
    out = torch.full((1000,), 7.0, device=dev)
    _call(out, src, 1, 1000, 1000, 1.0)
    assert torch.equal(out.cpu().view(torch.int32), x.view(torch.int32))
    out.fill_(7.0)
    _call(out, src, 3, 0, 0, 1.0)
    assert float(out.min()) == 7.0 and float(out.max()) == 7.0


@both
def _rank_sum_refusals(dev, big):
    """every refusal is made on the host, before any launch, and names the argument"""
    buf = torch.zeros(3 * 64 + 8, device=dev)
    out = torch.full((64,), 7.0, device=dev)
    st = L.stream_of(buf)
    bp, op = buf.data_ptr(), out.data_ptr()
    with pytest.raises(L.StcatHipError, match="n_ranks"):
        L.call("stcat_rank_sum", op, bp, 0, 64, 64, 1.0, st)
    with pytest.raises(L.StcatHipError, match="stride"):
        L.call("stcat_rank_sum", op, bp, 3, 64, 63, 1.0, st)
    with pytest.raises(L.StcatHipError, match=r"\bn="):
        L.call("stcat_rank_sum", op, bp, 3, -1, 64, 1.0, st)
    with pytest.raises(L.StcatHipError, match="out"):
        L.call("stcat_rank_sum", None, bp, 3, 64, 64, 1.0, st)
    with pytest.raises(L.StcatHipError, match=r"\bin\b"):
        L.call("stcat_rank_sum", op, None, 3, 64, 64, 1.0, st)
    buf.fill_(1.0)
    for off in (4, 64 + 4, 2 * 64 + 60, -4 + 64):          # partial overlaps with slice 0, 1, 2 and 0 / 1
        with pytest.raises(L.StcatHipError, match="out overlaps"):
            L.call("stcat_rank_sum", bp + 4 * off, bp, 3, 64, 64, 1.0, st)
    with pytest.raises(L.StcatHipError, match="out overlaps"):   # out = in + 1
        L.call("stcat_rank_sum", bp + 4, bp, 3, 64, 64, 1.0, st)
    assert float(out.min()) == 7.0 and float(buf.min()) == 1.0 and float(buf.max()) == 1.0     # nothing ran
    # directly behind the last slice is no overlap
    L.call("stcat_rank_sum", bp + 4 * 2 * 64, bp, 2, 64, 64, 0.5, st)
    assert torch.equal(buf[128:192].cpu(), torch.ones(64))


def test_rank_sum_is_in_the_entry_table():
    from tests.backends import use_emu
    use_emu()
    assert L.SIGNATURES["stcat_rank_sum"] == "ppillfs"
