"""conv_stack2's copy-out (each layer's output frame, and the forward's ReLU bits, stored to HBM
under the next layer's K-steps, the last layer's after the loop) at the smallest shapes that
take every copy-out path, bit for bit against the integer-data oracles of
deep_go_amd/ops/exact.py:

  nl = 1  only the exposed copy-out after the loop
  nl = 2  one in-loop copy-out, then the exposed one
  nl = 3  an in-loop copy-out under a layer whose own output is copied out in the loop too
  B = 1 and 3 (odd: a wrong board stride shows), forward and backward-data (both schedules).

Every output buffer has one board more than the launch uses and is pre-filled with a sentinel:
afterwards the frames' border rows and columns and the extra board (frames and ReLU bytes) must
still hold it, so a store through a wrong table entry — pixel 360's clamp, a row wrap — is seen
even where it lands outside the compared interior.
"""
import os

import numpy as np
import pytest
import torch

from deep_go_amd.ops import exact as E
from deep_go_amd.ops import layouts as LY
from test_stack_copyout_cpu import COPYOUT_CASES, HEAD_CASE, L1_CASE

pytestmark = pytest.mark.gpu

FRAME_SENTINEL = 0x5A5A      # bf16 bits (1.5e13: no output of the integer data)
BYTE_SENTINEL = 0xA5
DEV = "cuda"


def _hip():
    from deep_go_amd.ops.native import hip, stream_handle
    return hip(), stream_handle()


def _env_sched():
    """The schedule the library starts with: DG_STACK2_STAG = "MODE[,PRIO[,DELAY]]" (2,1,0)."""
    v = [2, 1, 0]
    for i, t in enumerate((os.environ.get("DG_STACK2_STAG") or "").split(",")[:3]):
        if t.strip().lstrip("-").isdigit():
            v[i] = int(t)
    if not 0 <= v[0] <= 2:
        v[0] = 2
    return tuple(v)


def _sentinel_frames(B, nl):
    ys = [torch.empty((B + 1, 21, 21, 128), dtype=torch.bfloat16, device=DEV) for _ in range(nl)]
    for y in ys:
        y.view(torch.int16).fill_(FRAME_SENTINEL)
    return ys


def _sentinel_masks(B, nl):
    return [torch.full((B + 1, E.NPTS, 16), BYTE_SENTINEL, dtype=torch.uint8, device=DEV)
            for _ in range(nl)]


def _operands(c, l1=False):
    ops = []
    for l, A in enumerate(c["As"]):
        a16 = A.to(torch.bfloat16).to(DEV)
        ops.append(LY.stack_frag_linear(a16, 128) if (l1 and l == 0) else LY.stack_frag(a16))
    return ops


def _pbias(c):
    return [LY.stack_pbias_frag(torch.zeros(128, device=DEV), pb.float().to(DEV))
            for pb in c["pbs"]]


def _table(ops, pf, ys, ms):
    return np.ascontiguousarray(np.array(
        [[ops[i].data_ptr(), pf[i].data_ptr() if pf else 0, ys[i].data_ptr(), ms[i].data_ptr()]
         for i in range(len(ops))], dtype=np.int64))


def _check_frame(y, B, want, tag):
    """Boards 0..B-1: interior == want, border still the sentinel; board B untouched."""
    got = y.cpu()
    inner = got[:B, 1:20, 1:20].double()
    assert torch.equal(inner, want), (tag, int((inner != want).sum()))
    bits = got.view(torch.int16).clone()
    bits[:B, 1:20, 1:20] = FRAME_SENTINEL
    bad = (bits != FRAME_SENTINEL).nonzero()
    assert bad.numel() == 0, (tag, "sentinel overwritten at [board, row, col, ch]", bad[:4].tolist())


def _check_untouched(t, sentinel, tag):
    v = t.cpu()
    v = v.view(torch.int16) if v.dtype == torch.bfloat16 else v
    assert bool((v == sentinel).all()), (tag, "written")


def _launch(epi, c, B, l1=False, stag=None):
    """conv_stack2 into sentinel-filled outputs.  -> (frames, masks) still on the GPU."""
    h, st = _hip()
    nl = len(c["As"])
    fwd = epi == "fwd"
    xf = E.frame_of(c["x"], 2 if l1 else 1, DEV)
    ops = _operands(c, l1)
    ys = _sentinel_frames(B, nl)
    if fwd:
        ms, pf = _sentinel_masks(B, nl), _pbias(c)
    else:
        ms, pf = _sentinel_masks(B, nl), None
        for m, src in zip(ms, c["masks"]):
            m[:B] = src.to(DEV)
    tab = _table(ops, pf, ys, ms)
    try:
        if stag is not None:
            h.conv_stack2_set_sched(stag, 1, 0)
        h.conv_stack2(h.EPI_FWD if fwd else h.EPI_DGRAD, tab.ctypes.data, nl, xf.data_ptr(),
                      int(l1), B, st)
        torch.cuda.synchronize()
    finally:
        if stag is not None:
            h.conv_stack2_set_sched(*_env_sched())
    return ys, ms


def _check_stack(c, B, epi, ys, ms, tag):
    for l, (_, y, _) in enumerate(c["ref"]):
        _check_frame(ys[l], B, y, (tag, l))
        m = ms[l].cpu()
        if epi == "fwd":
            assert torch.equal(m[:B], E.pack_mask(y != 0)), (tag, l, "ReLU bits")
        else:   # inputs: untouched
            assert torch.equal(m[:B], c["masks"][l]), (tag, l, "mask input changed")
        assert bool((m[B] == BYTE_SENTINEL).all()), (tag, l, "bytes past the last board")


@pytest.mark.parametrize("case", [c for c in COPYOUT_CASES if c[3] == "fwd"])
def test_forward_copy_out(case):
    C, B, nl, epi, seed, l1 = case
    c = E.stack_case(C, B, nl, epi, seed, l1)
    ys, ms = _launch(epi, c, B)
    _check_stack(c, B, epi, ys, ms, case)


@pytest.mark.parametrize("stag", [0, 1])
@pytest.mark.parametrize("case", [c for c in COPYOUT_CASES if c[3] == "dgrad"])
def test_backward_data_copy_out(case, stag):
    """Both schedules of the backward-data chain (barrier / staggered two-group)."""
    C, B, nl, epi, seed, l1 = case
    c = E.stack_case(C, B, nl, epi, seed, l1)
    ys, ms = _launch(epi, c, B, stag=stag)
    _check_stack(c, B, epi, ys, ms, (case, stag))


def test_l1_mode_two_layers():
    """l1 mode at nl = 2: layer 0 (the 5x5 first layer) copies nothing out while it runs; its
    output leaves under layer 1, layer 1's after the loop."""
    C, B, nl, epi, seed, l1 = L1_CASE
    c = E.stack_case(C, B, nl, epi, seed, l1)
    ys, ms = _launch(epi, c, B, l1=True)
    _check_stack(c, B, epi, ys, ms, L1_CASE)


def _head_params(B, seed):
    g = torch.Generator().manual_seed(seed)
    w = (0.01 * torch.randn(9 * 128, generator=g)).to(DEV)
    bias = torch.randn(1, generator=g).to(DEV)
    posb = (0.1 * torch.randn(E.NPTS, generator=g)).to(DEV)
    labels = torch.randint(0, E.NPTS, (B,), generator=g).to(torch.int32).to(DEV)
    return w, bias, posb, labels


def _head_outputs(B):
    return {"loss": torch.zeros(B, dtype=torch.float32, device=DEV),
            "pred": torch.full((B,), -1, dtype=torch.int32, device=DEV),
            "dz": LY.alloc_frame(B, 128, 1, DEV),
            "gw": torch.zeros((B, 9 * 128), dtype=torch.float32, device=DEV),
            "dzb": torch.zeros((B, E.NPTS), dtype=torch.float32, device=DEV)}


def _standalone_head(frame, B, hp, relu):
    """The standalone policy head (its own launch) on a bf16 pad-1 frame: the oracle path of
    the head fused behind the stack."""
    h, st = _hip()
    w, bias, posb, labels = hp
    o = _head_outputs(B)
    h.head(3, frame.data_ptr(), 1, 128, B, w.data_ptr(), bias.data_ptr(), posb.data_ptr(),
           labels.data_ptr(), o["loss"].data_ptr(), o["pred"].data_ptr(), 0, o["dz"].data_ptr(), 1,
           o["gw"].data_ptr(), 0, o["dzb"].data_ptr(), relu, 1.0 / B, st)
    torch.cuda.synchronize()
    return o


def _assert_head_equal(got, want, tag):
    for k in ("loss", "pred", "dz", "gw", "dzb"):
        assert torch.equal(got[k], want[k]), (tag, k)
    assert bool(torch.isfinite(got["loss"]).all()) and bool((got["pred"] >= 0).all())


def test_fused_head_two_layers():
    """Forward with the fused head at nl = 2: layer 0 leaves by the in-loop copy-out, the last
    layer is not copied out at all (the head reads the resident image); loss, predictions and
    the head's backward outputs equal the standalone head on the oracle's last frame."""
    C, B, nl, epi, seed, l1 = HEAD_CASE
    c = E.stack_case(C, B, nl, epi, seed, l1)
    h, st = _hip()
    hp = _head_params(B, seed)
    want = _standalone_head(E.frame_of(c["ref"][-1][1], 1, DEV), B, hp, 0)
    xf = E.frame_of(c["x"], 1, DEV)
    ops, pf = _operands(c), _pbias(c)
    ys, ms = _sentinel_frames(B, nl), _sentinel_masks(B, nl)
    tab = _table(ops, pf, ys, ms)
    o = _head_outputs(B)
    w, bias, posb, labels = hp
    h.conv_stack2_fwd_head(tab.ctypes.data, nl, xf.data_ptr(), 0, B, w.data_ptr(), bias.data_ptr(),
                           posb.data_ptr(), labels.data_ptr(), o["loss"].data_ptr(),
                           o["pred"].data_ptr(), o["dz"].data_ptr(), o["gw"].data_ptr(),
                           o["dzb"].data_ptr(), 0, 1.0 / B, st)
    torch.cuda.synchronize()
    y0 = c["ref"][0][1]
    _check_frame(ys[0], B, y0, "layer 0")
    m0 = ms[0].cpu()
    assert torch.equal(m0[:B], E.pack_mask(y0 != 0)) and bool((m0[B] == BYTE_SENTINEL).all())
    _check_untouched(ys[1], FRAME_SENTINEL, "last layer's frame")
    _check_untouched(ms[1], BYTE_SENTINEL, "last layer's ReLU bytes")
    _assert_head_equal(o, want, "fused head")


def test_l1_fused_expansion_two_layers():
    """l1 mode with the feature expansion fused into the prologue (and the head behind the
    stack) at nl = 2, against the separate launches: expansion, stack in l1 mode (checked
    against the float64 oracle above), standalone head.  The expanded input frame, layer 0's
    frame and ReLU bits, and the head's outputs are bit-identical."""
    from deep_go_amd.data.synthetic import random_planes
    C, B, nl, epi, seed, l1 = L1_CASE
    c = E.stack_case(C, B, nl, epi, seed, l1)
    h, st = _hip()
    planes, player, rank, _ = (torch.from_numpy(a).to(DEV) for a in random_planes(B, seed=seed))
    hp = _head_params(B, seed)
    ops, pf = _operands(c, l1=True), _pbias(c)
    # the separate launches
    x0a = LY.alloc_frame(B, 40, 2, DEV)
    h.expand_features(planes.data_ptr(), player.data_ptr(), rank.data_ptr(), x0a.data_ptr(), B, 2,
                      40, st)
    ya = [LY.alloc_frame(B, 128, 1, DEV) for _ in range(nl)]
    ma = [torch.zeros(B, E.NPTS, 16, dtype=torch.uint8, device=DEV) for _ in range(nl)]
    ta = _table(ops, pf, ya, ma)
    h.conv_stack2(h.EPI_FWD, ta.ctypes.data, nl, x0a.data_ptr(), 1, B, st)
    torch.cuda.synchronize()
    assert float(ya[0].float().abs().sum()) > 0 and float(ya[1].float().abs().sum()) > 0
    want = _standalone_head(ya[1], B, hp, 0)
    # one launch
    x0b = LY.alloc_frame(B, 40, 2, DEV)
    ys, ms = _sentinel_frames(B, nl), _sentinel_masks(B, nl)
    tb = _table(ops, pf, ys, ms)
    o = _head_outputs(B)
    w, bias, posb, labels = hp
    h.conv_stack2_fwd_head_x(tb.ctypes.data, nl, x0b.data_ptr(), B, planes.data_ptr(),
                             player.data_ptr(), rank.data_ptr(), w.data_ptr(), bias.data_ptr(),
                             posb.data_ptr(), labels.data_ptr(), o["loss"].data_ptr(),
                             o["pred"].data_ptr(), o["dz"].data_ptr(), o["gw"].data_ptr(),
                             o["dzb"].data_ptr(), 0, 1.0 / B, st)
    torch.cuda.synchronize()
    assert torch.equal(x0a, x0b)
    _check_frame(ys[0], B, ya[0].cpu()[:, 1:20, 1:20].double(), "layer 0")
    m0 = ms[0].cpu()
    assert torch.equal(m0[:B], ma[0].cpu()) and bool((m0[B] == BYTE_SENTINEL).all())
    _check_untouched(ys[1], FRAME_SENTINEL, "last layer's frame")
    _check_untouched(ms[1], BYTE_SENTINEL, "last layer's ReLU bytes")
    _assert_head_equal(o, want, "fused expansion + head")
