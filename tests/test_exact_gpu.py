"""Tolerance-free kernel tests: every assertion here is an equality.

The data (deep_go_amd/ops/exact.py) makes every product and every partial sum an integer
multiple of one power-of-two quantum q with sum |a||x| < 2^24 q, so the MFMAs' fp32 sums are
exact in any order and a kernel's value before its final rounding is one determined number:
the float64 CPU reference, pushed through the same final rounding (bf16 nearest-even, or the
fp8 emulation), must be reproduced bit for bit — frames, borders, ReLU bits, fp8 copy bytes,
|y| maxima, fp32 gradients.  The builders check that condition on the inputs before anything
is launched (tests/test_exact_cpu.py proves it is sufficient).  The chained layers are checked
in order, so a layer is compared only after its input was found equal to the reference's
(teacher forcing by induction).  The sensitivity tests change one operand element behind the
reference's back and require the predicted single-term footprint, which pins the fragment
orders element by element and shows that a one-term error cannot pass.
"""
import os

import pytest
import torch

from deep_go_amd.ops import exact as E
from test_exact_cpu import (BOARD_FP8_CASES, CONV_CASES, CONV_NT_TILES, F8_CASES, F8_SR_CASE,
                            L1_CASES, L1_FRAG_M, STACK_CASES, WGRAD_IM2COL_CASES,
                            WGRAD_WIN8_CASES, WGRAD_WIN_CASES)

pytestmark = pytest.mark.gpu


def _hip():
    from deep_go_amd.ops.native import hip
    return hip()


def _check_frames(frames, masks_out, ref, fwd, tag):
    """Every layer's frame interior == bf16(reference), borders zero, forward ReLU bytes =
    'stored output != 0' of the reference."""
    for l, (v, y, _) in enumerate(ref):
        inner, border = E.frame_split(frames[l])
        assert border == 0, (tag, l, "border written")
        assert torch.equal(inner, y), (tag, l, int((inner != y).sum()))
        if fwd:
            assert torch.equal(masks_out[l], E.pack_mask(y != 0)), (tag, l, "mask")
    # layer 0 needed no rounding at all
    assert torch.equal(ref[0][1], ref[0][0])


# ------------------------------------------------------------------ (a) bf16 board-resident
@pytest.mark.parametrize("stag", [0, 1])
@pytest.mark.parametrize("case", [c for c in STACK_CASES if c[0] == 128 and c[1] == 5 or c[5]])
def test_conv_stack2_exact(case, stag):
    """conv_stack2 forward (integer bias tables through stack_pbias_frag, ReLU bits written),
    backward-data (random masks) and l1 mode (5x5 over the {0, 1} 23x23x40 frame, weights
    through stack_frag_linear), three layers, barrier and staggered schedules."""
    C, B, nl, epi, seed, l1 = case
    c = E.stack_case(C, B, nl, epi, seed, l1)
    h = _hip()
    try:
        h.conv_stack2_set_sched(stag, 1, 0)
        frames, masks = E.run_stack2(epi, c["As"], c["x"], c["pbs"], c["masks"], l1=l1)
    finally:
        h.conv_stack2_set_sched(2, 1, 0)
    _check_frames(frames, masks, c["ref"], epi == "fwd", case)
    if epi == "dgrad":   # the masks are inputs: untouched
        assert all(torch.equal(a, b) for a, b in zip(masks, c["masks"]))


@pytest.mark.parametrize("multi", [False, True])
@pytest.mark.parametrize("case", [c for c in STACK_CASES if c[1] == 3 and not c[5]])
def test_conv_layer2_exact(case, multi):
    """conv_layer2 (one launch per layer) and conv_layer2_multi (one launch), C = 256 and 128,
    three layers, forward and backward-data."""
    C, B, nl, epi, seed, _ = case
    c = E.stack_case(C, B, nl, epi, seed)
    frames, masks = E.run_layer2(epi, C, c["As"], c["x"], c["pbs"], c["masks"], multi=multi)
    _check_frames(frames, masks, c["ref"], epi == "fwd", (case, multi))


@pytest.mark.parametrize("M", L1_FRAG_M)
def test_conv_l1_frag_exact(M):
    from deep_go_amd.ops import functional as Fn
    c = E.conv_case(3, 40, M, 5, 150)
    y, mask = Fn.conv_l1_frag(E.nchw(c["x"]).float(), c["w"].float().cuda(),
                              torch.zeros(M), c["pb"].float())
    torch.cuda.synchronize()
    got = E.nhwc(y.cpu().double())
    assert torch.equal(got, c["fwd"])          # |v| <= 256: no rounding enters
    assert c["fwd"].max().item() <= 256
    assert torch.equal(mask.cpu(), E.pack_mask(c["fwd"] != 0))


# ------------------------------------------------------------------ (b) fp8 stacks
def _check_f8(out, c, fwd, y8, tag):
    ref = c["ref"]
    L = ref["layers"]
    nl = len(L)
    amax = out["amax"]
    assert amax[0].item() == c["x"].abs().max().item(), (tag, "amax x0")
    if y8:
        inner, rest = E.fp8_frame_split(out["x8"])
        assert rest == 0 and torch.equal(inner, ref["x8"]), (tag, "x8")
    for l in range(nl):
        last = l == nl - 1
        if not last:
            assert amax[l + 1].item() == L[l]["v"].abs().max().item(), (tag, l, "amax")
        if out["frames"][l] is not None:
            inner, border = E.frame_split(out["frames"][l])
            assert border == 0, (tag, l, "border written")
            assert torch.equal(inner, L[l]["y"]), (tag, l, int((inner != L[l]["y"]).sum()))
        else:
            assert y8 and not last
        if y8 and not last:
            inner, rest = E.fp8_frame_split(out["y8"][l])
            assert rest == 0, (tag, l, "fp8 border written")
            # (-0 and +0 are one value: compare the bytes with the sign of zero cleared)
            nz = lambda b: torch.where((b & 0x7F) == 0, torch.zeros_like(b), b)  # noqa: E731
            assert torch.equal(nz(inner), nz(L[l]["y8"])), (tag, l, "fp8 bytes")
        if fwd:
            assert torch.equal(out["masks"][l], E.pack_mask(L[l]["y"] != 0)), (tag, l, "mask")


def _f8_sched_params():
    out = []
    for case in F8_CASES:
        for stag in ((0, 1) if case[0] == 128 else (1,)):
            for y8 in (False, True):
                out.append((case, stag, y8))
    return out


@pytest.mark.parametrize("case,stag,y8", _f8_sched_params())
def test_conv_stack_f8_exact(case, stag, y8):
    """conv_stack_f8 forward (e4m3 {0, 1, 2} inputs at scale 1, e4m3 +-1 weight bytes, power-of-
    two s_w / s_y, integer bias tables) and backward-data (e5m2, round to nearest even), three
    layers, C = 128 (barrier and staggered schedules) and 256; the bf16-frame variant and the
    production variant (fp8 copies, no bf16 frame below the last layer).  With zero tolerance
    and for every element: frames, fp8 copy bytes, ReLU bits, |v| maxima, zero borders."""
    C, B, nl, epi = case[:4]
    c = E.stack_f8_case(*case)
    h = _hip()
    try:
        h.conv_stack_f8_set_sched(stag, 0)
        out = E.run_stack_f8(C, epi, c["W8"], c["x"], c["s"], c["ws"], c["pbs"], c["masks"],
                             y8=y8)
    finally:
        h.conv_stack_f8_set_sched(1, 0)
    _check_f8(out, c, epi == "fwd", y8, (case, stag, y8))


@pytest.mark.parametrize("y8", [False, True])
def test_conv_stack_f8_stochastic_rounding_of_representable_values(y8):
    """Stochastic rounding of a representable value is the identity: with one nonzero input
    channel on a checkerboard every |acc| of layer 0 is at most 5, an e5m2 number at scale 1,
    so the stochastically rounded chain equals the nearest-even reference."""
    C, B, nl, epi = F8_SR_CASE[:4]
    c = E.stack_f8_case(*F8_SR_CASE)
    out = E.run_stack_f8(C, epi, c["W8"], c["x"], c["s"], c["ws"], None, c["masks"], y8=y8,
                         sr_step=12345)
    _check_f8(out, c, False, y8, ("sr", y8))


# ------------------------------------------------------------------ (c) weight gradients
def _dz_x(c):
    return E.nchw(c["dz"]).float().cuda(), E.nchw(c["x"]).float().cuda()


@pytest.mark.parametrize("B,cin,cout,splits", WGRAD_WIN_CASES)
def test_conv_wgrad_win_exact(B, cin, cout, splits):
    from deep_go_amd.ops import functional as Fn
    c = E.wgrad_case(B, cin, cout, 3, 120 + B)
    sf = E.new_step_tag()
    dz, x = _dz_x(c)
    got = Fn.conv_wgrad(dz, x, 3, splits=splits, algo="win", sf=sf)
    assert torch.equal(got.cpu(), c["ref"].float())
    assert sf.tolist() == [5, 0]


@pytest.mark.parametrize("B,cin,cout,k,splits,real", WGRAD_IM2COL_CASES)
def test_conv_wgrad_im2col_exact(B, cin, cout, k, splits, real):
    """conv_wgrad: the three-slice tiles, the 2-stage kernel and the 5x5 kernels (2-stage and
    pipelined) with 37 real channels of 40 — the padded channels' gradients exactly zero; the
    fused bias gradients are integer sums too."""
    from deep_go_amd.ops import functional as Fn
    c = E.wgrad_case(B, cin, cout, k, 130 + B, real)
    dz, x = _dz_x(c)
    h = _hip()
    for ns in ((0, 4) if k == 5 else (None,)):
        sf = E.new_step_tag()
        try:
            if ns is not None:
                h.conv_wgrad5_set_ns(ns)
            got, gp, gb = Fn.conv_wgrad(dz, x, k, splits=splits, cinp=cin, with_bias=True,
                                        algo="im2col", sf=sf)
            torch.cuda.synchronize()
        finally:
            if ns is not None:
                h.conv_wgrad5_set_ns(int(os.environ.get("DG_WGRAD5_NS", "4")))
        assert torch.equal(got.cpu(), c["ref"].float()), ns
        if real is not None:
            assert got[..., real:].abs().sum().item() == 0
        assert torch.equal(gp.cpu().double(), c["dz"].sum(0).reshape(361, cout))
        assert torch.equal(gb.cpu().double(), c["dz"].sum((0, 1, 2)))
        assert sf.tolist() == [5, 0]


def test_conv_wgrad_multi_exact():
    cs = [E.wgrad_case(3, 128, 128, 3, 160 + i) for i in range(2)]
    got, sf = E.run_wgrad_multi([c["dz"] for c in cs], [c["x"] for c in cs], splits=4)
    for g, c in zip(got, cs):
        assert torch.equal(g, c["ref"].float())
    assert sf.tolist() == [5, 0]


@pytest.mark.parametrize("B,cin,cout,splits", WGRAD_WIN8_CASES)
@pytest.mark.parametrize("log2_s", [(0, 0), (-3, 2)])
def test_conv_wgrad_win8_exact(B, cin, cout, splits, log2_s):
    """conv_wgrad_win8 on e5m2 dz / e4m3 x bytes in 448-row frames, power-of-two scales, split
    counts whose ranges begin and end inside a board (2 .. 26 super-steps per split)."""
    c = E.wgrad_case(B, cin, cout, 3, 120 + B)
    s_dz, s_x = 2.0 ** log2_s[0], 2.0 ** log2_s[1]
    got, sf, used = E.run_wgrad_win8(c["dz"] * s_dz, c["x"] * s_x, s_dz, s_x, splits)
    assert used >= 1 and (splits is None or used == splits)
    assert torch.equal(got, (c["ref"] * (s_dz * s_x)).float()), int(
        (got != (c["ref"] * (s_dz * s_x)).float()).sum())
    assert sf.tolist() == [5, 0]


# ------------------------------------------------------------------ (d) remaining conv paths
def _tab(c):
    cout = c["pb"].shape[1]
    return torch.zeros(cout), c["pb"].float()


@pytest.mark.parametrize("B,cin,cout,k,tiles", [c + (t,) for c in CONV_CASES
                                                for t in CONV_NT_TILES[c[2]]])
def test_conv_nt_exact(B, cin, cout, k, tiles):
    from deep_go_amd.ops import functional as Fn
    c = E.conv_case(B, cin, cout, k, 140 + B)
    x, w = E.nchw(c["x"]).float().cuda(), c["w"].float().cuda()
    b, pb = _tab(c)
    assert torch.equal(E.nhwc(Fn.conv_forward(x, w, epi="linear", tiles=tiles).cpu().double()),
                       c["lin"])
    assert torch.equal(E.nhwc(Fn.conv_forward(x, w, b, pb, tiles=tiles).cpu().double()), c["fwd"])
    got = Fn.conv_dgrad(E.nchw(c["dz"]).float().cuda(), w, E.nchw(c["aux"]).float().cuda(),
                        tiles=tiles)
    assert torch.equal(E.nhwc(got.cpu().double()), E.bf16_round(c["dgrad"]))


@pytest.mark.parametrize("B,cin,cout,k", CONV_CASES)
@pytest.mark.parametrize("bm", ["64", "128"])
def test_conv_board_exact(B, cin, cout, k, bm, monkeypatch):
    from deep_go_amd.ops import functional as Fn
    monkeypatch.setenv("DG_BOARD_BM", bm)
    c = E.conv_case(B, cin, cout, k, 140 + B)
    x, w = E.nchw(c["x"]).float().cuda(), c["w"].float().cuda()
    b, pb = _tab(c)
    assert torch.equal(E.nhwc(Fn.conv_board(x, w, epi="linear").cpu().double()), c["lin"])
    assert torch.equal(E.nhwc(Fn.conv_board(x, w, b, pb, epi="fwd").cpu().double()), c["fwd"])
    got = Fn.conv_board(E.nchw(c["dz"]).float().cuda(), w, epi="dgrad",
                        aux=E.nchw(c["aux"]).float().cuda())
    assert torch.equal(E.nhwc(got.cpu().double()), E.bf16_round(c["dgrad"]))


@pytest.mark.parametrize("B,cin,cout,k", L1_CASES)
def test_conv_l1_exact(B, cin, cout, k):
    from deep_go_amd.ops import functional as Fn
    c = E.conv_case(B, cin, cout, k, 140 + B)
    b, pb = _tab(c)
    y, mask = Fn.conv_l1(E.nchw(c["x"]).float(), c["w"].float().cuda(), b, pb, with_mask=True)
    assert torch.equal(E.nhwc(y.cpu().double()), c["fwd"])
    assert torch.equal(mask.cpu(), E.pack_mask(c["fwd"] != 0))


@pytest.mark.parametrize("B,cin,cout,bm", BOARD_FP8_CASES)
def test_conv_board_fp8_exact(B, cin, cout, bm):
    """conv_board_fp8 at scale 1 on {0, 1, 2} inputs and +-1 weights: the bf16 output, its e4m3
    copy at s_y = 2 (ties to even), the |y| max."""
    from deep_go_amd.ops import functional as Fn
    c = E.conv_case(B, cin, cout, 3, 144, 2)
    b, pb = _tab(c)
    y, y8, s_y, amax = Fn.conv_board_fp8(E.nchw(c["x"]).float().cuda(), c["w"].float().cuda(),
                                         b, pb, bm=bm, s_x=1.0, s_w=1.0, s_y=2.0)
    ref = c["fwd"]
    assert torch.equal(E.nhwc(y.cpu().double()), E.bf16_round(ref))
    assert torch.equal(E.nhwc(y8.cpu().double()), E.d_e4m3(E.q_e4m3(ref / 2.0)) * 2.0)
    assert amax == ref.max().item() and s_y == 2.0


# ------------------------------------------------------------------ (e) bias partials
def test_bias_grad_partial_exact():
    """bias_grad_partial at B = 17: one full chunk of 16 boards and one board."""
    dz = E.int_grads((17, 19, 19, 128), 170)
    part, rowpart, _ = E.run_bias_partials(dz, multi=False)
    wp, wr = E.bias_partials64(dz, 16)
    assert part.shape[0] == 2
    assert torch.equal(part.double(), wp) and torch.equal(rowpart.double(), wr)


@pytest.mark.parametrize("s8", [None, 0.25])
def test_bias_grad_partial_multi_exact(s8):
    """bias_grad_partial_multi at B = 70 (64 + 6 boards), on the bf16 frame and on the e5m2
    copy with its scale: integer sums, every slot written (NaN pre-fill), tag untouched."""
    dz = E.int_grads((70, 19, 19, 128), 171) * (s8 or 1.0)
    part, rowpart, sf = E.run_bias_partials(dz, multi=True, s8=s8)
    wp, wr = E.bias_partials64(dz, 64)
    assert part.shape[0] == 2
    assert torch.equal(part.double(), wp) and torch.equal(rowpart.double(), wr)
    assert sf.tolist() == [5, 0]


# ------------------------------------------------------------------ (f) sensitivity
def _flips(C):
    """(row, tap, channel): (0, 0), (last row, last k), the pair across the 64-channel
    boundary, taps 0 / 4 / 8, and a k in every lane group of stack_frag_f8 (channel blocks of
    32, both parities of the half-major unit 9 (c / 64) + tap) — all in different rows."""
    return [(0, 0, 0), (C - 1, 8, C - 1), (65, 4, 63), (66, 4, 64), (17, 0, 37), (18, 1, 5),
            (19, 1, 37), (33, 8, 101), (34, 4, 69), (35, 3, 69), (100, 0, C - 27),
            (101, 8, C - 59), (64, 4, 0), (63, 8, 64)]


def _flips_l1(M):
    """The 5x5 / 40-channel first layer (k = tap*40 + c, linear in the fragment order): (0, 0),
    (last row, last real k = 999), the pairs across the 8-element lane chunk and across the
    64-wide K-step (k = 63 | 64: tap 1, c = 23 | 24), taps 0 / 12 / 24."""
    return [(0, 0, 0), (M - 1, 24, 39), (65, 12, 7), (66, 12, 8), (17, 1, 23), (18, 1, 24),
            (33, 24, 0), (34, 0, 39), (64, 12, 20), (63, 6, 31)]


def _flip(A, C, flips=None):
    A2 = A.clone()
    for r, tap, ch in flips or _flips(C):
        A2[r, tap * C + ch] = -A2[r, tap * C + ch]
    return A2


def _check_footprint(got, ref, A, x, C, tag, flips=None, k=3):
    """got: kernel output with the flipped operand; ref: the reference of the UNflipped one.
    got - ref is -2 A[r][k] x[p + off(tap)][c] at row r for each flip, exactly zero elsewhere."""
    d = got - ref
    rows = []
    for r, tap, ch in flips or _flips(C):
        pred = -2 * A[r, tap * C + ch] * E.shifted(x, tap, k)[..., ch]
        assert pred.abs().sum().item() > 0
        assert torch.equal(d[..., r], pred), (tag, r, tap, ch)
        rows.append(r)
    assert len(set(rows)) == len(rows)
    keep = torch.ones(d.shape[-1], dtype=torch.bool)
    keep[rows] = False
    assert d[..., keep].abs().sum().item() == 0, (tag, "other rows changed")


def _l1_linear_case(M, seed):
    """The first layer in its linear range: {0, 1} inputs, bias table + 120 (ReLU inactive)."""
    x = E.int_acts((3, 19, 19, 40), 1, seed)
    A = E.sign_weights((M, 1000), seed + 1)
    pb = E.bias_table(M, 120)
    ref = E.fwd64(x, A, pb, 5)
    E.assert_order_independent(x, A, 1.0, bias=pb, ref=ref + 2, k=5)
    assert ref.min().item() > 2
    return x, A, pb, ref


@pytest.mark.parametrize("M", [128, 384])
def test_sensitivity_conv_l1_frag(M):
    """conv_l1_frag (weights through stack_frag_linear): 10 weight signs flipped."""
    from deep_go_amd.ops import functional as Fn
    x, A, pb, ref = _l1_linear_case(M, 186)
    fl = _flips_l1(M)
    w2 = _flip(A, 40, fl).reshape(M, 5, 5, 40)
    y, _ = Fn.conv_l1_frag(E.nchw(x).float(), w2.float().cuda(), torch.zeros(M), pb.float())
    torch.cuda.synchronize()
    _check_footprint(E.nhwc(y.cpu().double()), ref, A, x, 40, ("l1_frag", M), fl, 5)


def test_sensitivity_conv_stack2_l1():
    """conv_stack2 in l1 mode: the same flips in its fused first layer (row 0), seen in layer
    0's frame; a second, untouched layer follows (l1 mode needs two)."""
    x, A, pb, ref = _l1_linear_case(128, 188)
    fl = _flips_l1(128)
    pad = torch.zeros(128, 24, dtype=torch.float64)
    A1 = E.sign_weights((128, 1152), 189)
    frames, _ = E.run_stack2("fwd", [torch.cat([_flip(A, 40, fl), pad], 1), A1], x,
                             [pb, E.bias_table(128)], l1=True)
    _check_footprint(E.frame_split(frames[0])[0], ref, A, x, 40, "stack2 l1", fl, 5)


def test_sensitivity_conv_stack2():
    """One conv_stack2 forward layer in its linear range (bias table + 120: every value in
    1 .. 256, the ReLU inactive): 14 weight signs flipped behind the reference's back."""
    C, B = 128, 3
    x = E.int_acts((B, 19, 19, C), 1, 180)
    A = E.sign_weights((C, 9 * C), 181)
    pb = E.bias_table(C, 120)
    ref = E.fwd64(x, A, pb)
    E.assert_order_independent(x, A, 1.0, bias=pb, ref=ref + 2)
    assert ref.min().item() > 2
    frames, _ = E.run_stack2("fwd", [_flip(A, C)], x, [pb])
    _check_footprint(E.frame_split(frames[0])[0], ref, A, x, C, "stack2")


@pytest.mark.parametrize("C,multi", [(256, False), (128, True)])
def test_sensitivity_conv_layer2(C, multi):
    """conv_layer2 / conv_layer2_multi backward-data with an all-ones mask (linear)."""
    B = 3
    x = E.int_grads((B, 19, 19, C), 182, 1)
    A = E.sign_weights((C, 9 * C), 183)
    ones = torch.full((B, 361, C // 8), 255, dtype=torch.uint8)
    ref = E.conv64(x, A)
    E.assert_order_independent(x, A, 1.0, ref=ref.abs() + 2)
    frames, _ = E.run_layer2("dgrad", C, [_flip(A, C)], x, masks=[ones], multi=multi)
    _check_footprint(E.frame_split(frames[0])[0], ref, A, x, C, ("layer2", C))


@pytest.mark.parametrize("C", [128, 256])
def test_sensitivity_conv_stack_f8(C):
    """One conv_stack_f8 backward-data layer (e5m2 {-1, 0, 1} inputs, all-ones mask, bf16
    output): 14 e4m3 weight bytes flipped 0x38 <-> 0xB8 behind the reference's back."""
    B = 3
    x = E.int_grads((B, 19, 19, C), 184, 1)
    A = E.sign_weights((C, 9 * C), 185)
    ones = torch.full((B, 361, C // 8), 255, dtype=torch.uint8)
    ref = E.conv64(x, A)
    E.assert_order_independent(x, A, 1.0, ref=ref.abs() + 2)
    W8 = E.q_e4m3(_flip(A, C)).reshape(C, 9, C)
    out = E.run_stack_f8(C, "dgrad", [W8], x, (1.0, 1.0), (1.0,), None, [ones])
    _check_footprint(E.frame_split(out["frames"][0])[0], ref, A, x, C, ("stack_f8", C))


def _dz_changes(B, M):
    """(board, pixel, co): first / last of everything, the 64-channel boundary, pixels in
    different 32-row sub-steps of the window kernels — all in different co rows."""
    return [(0, 0, 0), (B - 1, 360, M - 1), (1, 180, 63), (1, 181, 64), (0, 37, 17),
            (B - 1, 75, 33), (2 % B, 300, 100), (0, 18, 5), (B - 1, 342, 90)]


def _x_changes(B, Cx):
    """(board, pixel, ci): as _dz_changes for the activation operand, different ci columns."""
    return [(0, 0, 0), (B - 1, 360, Cx - 1), (1, 180, 63), (1, 181, 64), (0, 37, 16),
            (B - 1, 75, 47), (2 % B, 300, 101), (0, 18, 15), (B - 1, 342, 80)]


def _check_wgrad_footprint(run, c, B, M, tag):
    """run(dz, x) -> dW OHWI.  (1) dz[b][p][co] += 1 behind the reference's back: dW changes
    by x[b][p + off(tap)][ci] in row co only.  (2) x[b][p][ci] += 1: dW changes by
    dz[b][p - off(tap)][co] in column ci only."""
    dz2 = c["dz"].clone()
    for b, p, co in _dz_changes(B, M):
        dz2[b, p // 19, p % 19, co] += 1
    d = run(dz2, c["x"]).double() - c["ref"]
    rows = []
    for b, p, co in _dz_changes(B, M):
        pred = torch.stack([E.shifted(c["x"], t)[b, p // 19, p % 19] for t in range(9)])
        assert pred.abs().sum().item() > 0
        assert torch.equal(d[co].reshape(9, -1), pred), (tag, b, p, co)
        rows.append(co)
    keep = torch.ones(M, dtype=torch.bool)
    keep[rows] = False
    assert d[keep].abs().sum().item() == 0, (tag, "other rows changed")
    Cx = c["x"].shape[-1]
    x2 = c["x"].clone()
    for b, p, ci in _x_changes(B, Cx):
        x2[b, p // 19, p % 19, ci] += 1
    d = (run(c["dz"], x2).double() - c["ref"]).reshape(M, 9, Cx)
    cols = []
    for b, p, ci in _x_changes(B, Cx):
        pred = torch.stack([E.shifted(c["dz"], 8 - t)[b, p // 19, p % 19] for t in range(9)], 1)
        assert pred.abs().sum().item() > 0
        assert torch.equal(d[:, :, ci], pred), (tag, "x", b, p, ci)
        cols.append(ci)
    keep = torch.ones(Cx, dtype=torch.bool)
    keep[cols] = False
    assert d[:, :, keep].abs().sum().item() == 0, (tag, "other columns changed")


def test_sensitivity_wgrad_win():
    from deep_go_amd.ops import functional as Fn
    B, C = 3, 128
    c = E.wgrad_case(B, C, C, 3, 120 + B)
    _check_wgrad_footprint(
        lambda dz, x: Fn.conv_wgrad(E.nchw(dz).float().cuda(), E.nchw(x).float().cuda(), 3,
                                    algo="win").cpu(), c, B, C, "win")


def test_sensitivity_wgrad_im2col():
    from deep_go_amd.ops import functional as Fn
    B, C = 3, 128
    c = E.wgrad_case(B, C, C, 3, 130 + B)
    _check_wgrad_footprint(
        lambda dz, x: Fn.conv_wgrad(E.nchw(dz).float().cuda(), E.nchw(x).float().cuda(), 3,
                                    splits=7, algo="im2col").cpu(), c, B, C, "im2col")


def test_sensitivity_wgrad_win8():
    B, C = 4, 128
    c = E.wgrad_case(B, C, C, 3, 120 + B)
    _check_wgrad_footprint(lambda dz, x: E.run_wgrad_win8(dz, x, 1.0, 1.0, 5)[0], c, B, C,
                           "win8")


# ------------------------------------------------------------------ the head's argmax
@pytest.mark.parametrize("B,C,k,relu", [(5, 128, 3, True), (4, 256, 3, False), (3, 64, 3, False)])
def test_head_pred_is_argmax_on_integer_logits(B, C, k, relu):
    """{0, 1} activations, +-1 weights and a position bias p' / 512 with p' a permutation of
    0 .. 360: every logit is an exact multiple of 2^-9 whose fraction is distinct per point, so
    each board has a unique maximum and the head's prediction must be the reference's argmax
    on EVERY board.  (The head's log-softmax and gradients stay tolerance-based: test_head.)"""
    from deep_go_amd.ops import functional as Fn
    x = E.int_acts((B, 19, 19, C), 1, 190 + B)
    w = E.sign_weights((1, k * k * C), 191)
    posb = ((torch.arange(361) * 37) % 361).double() / 512
    E.assert_order_independent(x, w, 2.0 ** -9, bias=posb + 3, k=k)
    z = E.conv64(x, w, k).reshape(B, 361) + 3 + posb
    if relu:
        z = z.relu()
    top2 = z.topk(2, 1).values
    assert bool((top2[:, 0] > top2[:, 1]).all())          # unique maxima (reference only)
    out = Fn.head(E.nchw(x).float().cuda(), w.reshape(1, k, k, C).float().cuda(),
                  torch.full((1,), 3.0).cuda(), posb.float().cuda(),
                  torch.zeros(B, dtype=torch.long), head_relu=relu)
    assert torch.equal(out["pred"].cpu().long(), z.argmax(1))
