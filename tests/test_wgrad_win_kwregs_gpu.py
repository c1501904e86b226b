"""The window weight gradient's kw taps from registers (conv_wgrad_win.hip).

Per kernel row the kernel reads only the centre tap's X fragment from LDS and shifts the
kw = 0 / 2 fragments together in registers, with one narrow read for the row in front of a
lane's eight K rows (m) and one for the row behind (p).  Three checks:

  * the raw split slabs are bit-identical to the kept nine-taps-from-LDS path (ablation bit 64)
    on random bf16 data;
  * one-hot X pixels at the K rows where m / p cross a lane group or the K-step boundary,
    against a float64 conv2d weight gradient, exactly;
  * the step tag: clean data leaves it alone, an out-of-range slab value sets it.
"""
import numpy as np
import pytest
import torch

from deep_go_amd.ops import layouts as LY

pytestmark = pytest.mark.gpu

WF = 21


def _hip():
    from deep_go_amd.ops.native import hip, stream_handle
    return hip(), stream_handle()


def _run_win(h, s, dzf, xf, splits, ablate=0, sf=None):
    """One conv_wgrad_win launch on raw frames -> the slab buffer [splits][Mpad][KP] (fp32).
    The buffer is pre-filled so that an unwritten element shows."""
    B, M, Cx = dzf.shape[0], dzf.shape[-1], xf.shape[-1]
    _, KP, _ = LY.conv_dims(3, Cx, M, 128)
    Mpad = LY.round_up(M, 128)
    slab = torch.full((splits, Mpad, KP), -7.0, dtype=torch.float32, device="cuda")
    table = np.array([[dzf.data_ptr(), xf.data_ptr(), slab.data_ptr()]], dtype=np.int64)
    try:
        h.conv_wgrad_win_set_ablate(ablate)
        h.conv_wgrad_win(table.ctypes.data, 1, M, Mpad, Cx, B, KP, splits,
                         0 if sf is None else sf.data_ptr(), s)
        torch.cuda.synchronize()
    finally:
        h.conv_wgrad_win_set_ablate(0)
    return slab


# (B, M, Cx, splits): baseline; one step per split (every step-in-board index starts a
# prologue); a second split starting mid-board at step 19 across two board edges; uneven
# splits; the s_setprio variant (M >= 256) with 4 ci-chunks; a long stream (many ring wraps)
IDENT_CASES = [(1, 128, 64, 1), (1, 128, 64, 13), (3, 128, 128, 2), (3, 128, 128, 5),
               (2, 256, 256, 3), (5, 128, 128, 1)]


@pytest.mark.parametrize("B,M,Cx,splits", IDENT_CASES)
def test_slabs_bit_identical_to_nine_lds_taps(B, M, Cx, splits):
    h, s = _hip()
    g = torch.Generator(device="cuda").manual_seed(1000 + 17 * B + M + Cx + splits)
    dzf = LY.alloc_frame(B, M, 1, "cuda")
    LY.frame_interior(dzf, 1).copy_(torch.randn(B, 19, 19, M, device="cuda", generator=g))
    xf = LY.alloc_frame(B, Cx, 1, "cuda")
    LY.frame_interior(xf, 1).copy_(torch.randn(B, 19, 19, Cx, device="cuda", generator=g).relu())
    new = _run_win(h, s, dzf, xf, splits, 0)
    old = _run_win(h, s, dzf, xf, splits, 64)
    assert torch.equal(new, old), int((new != old).sum())
    # the written part is a real gradient, not the fill
    _, KP, _ = LY.conv_dims(3, Cx, M, 128)
    assert (new[:, :M, :9 * Cx] != -7.0).any() and new[:, :M, :9 * Cx].abs().max() > 1


def _edge_pixels():
    """(board, frame-linear index) of the one-hot X pixels, B = 2: the K rows 0, 7, 8, 24, 31
    of the steps j = 0, 6, 12 of a board (step j starts at frame row index 21 + 32 j) — the
    rows at which m / p come from the next lane group or from beyond the step — alternating
    between the boards, then board columns 0 and 18 and the corners on the last board.  (Three
    of the fifteen fall on the frame's border ring, where the network's X is zero; the kernel
    and the oracle treat the frame as plain data.)"""
    px = []
    for j in (0, 6, 12):
        for r in (0, 7, 8, 24, 31):
            px.append((len(px) % 2, WF + 32 * j + r))
    for row, col in ((9, 0), (9, 18), (0, 0), (0, 18), (18, 0), (18, 18)):
        px.append((1, (row + 1) * WF + col + 1))
    return px


@pytest.fixture(scope="module")
def ones_dz():
    dzf = LY.alloc_frame(2, 128, 1, "cuda")
    LY.frame_interior(dzf, 1).fill_(1.0)
    return dzf


@pytest.mark.parametrize("board,idx", _edge_pixels())
def test_edge_rows_against_conv2d_oracle(ones_dz, board, idx):
    """X one-hot at one frame pixel in one channel of each 16-channel wave quarter (lane
    n = 3, 8, 15, 0 of waves 0..3), dZ all ones in the interior: all nine taps of every output
    equal the float64 conv2d weight gradient."""
    h, s = _hip()
    B, M, Cx = 2, 128, 64
    chans = (3, 16 + 8, 32 + 15, 48)
    x = torch.zeros(B, WF * WF, Cx, dtype=torch.bfloat16)
    for k, ch in enumerate(chans):
        x[board, idx, ch] = k + 1
    xf = x.view(B, WF, WF, Cx).cuda()
    # the frame is the (already padded) input of a valid 3x3 convolution
    ref = torch.nn.grad.conv2d_weight(
        x.view(B, WF, WF, Cx).permute(0, 3, 1, 2).double(), (M, Cx, 3, 3),
        torch.ones(B, M, 19, 19, dtype=torch.float64)).permute(0, 2, 3, 1)
    assert ref.abs().sum() > 0
    for splits in (1, 2):
        slab = _run_win(h, s, ones_dz, xf, splits)
        got = slab[:, :M, :9 * Cx].double().sum(0).view(M, 3, 3, Cx).cpu()
        assert torch.equal(got, ref), (splits, (got != ref).nonzero()[:8].tolist())


def test_step_tag_clean_and_out_of_range():
    """The slab range check beside the stores: clean data leaves the tag [5, 0]; one X element
    of 2^125 (products >= the 2^120 bound) sets it to the step + 1."""
    from deep_go_amd.ops import exact as E
    h, s = _hip()
    B, M, Cx = 1, 128, 64
    dzf = LY.alloc_frame(B, M, 1, "cuda")
    LY.frame_interior(dzf, 1).fill_(1.0)
    xf = LY.alloc_frame(B, Cx, 1, "cuda")
    LY.frame_interior(xf, 1).fill_(1.0)
    sf = E.new_step_tag()
    _run_win(h, s, dzf, xf, 2, sf=sf)
    assert sf.tolist() == [5, 0]
    xf[0, 10, 8, 17] = 2.0 ** 125
    _run_win(h, s, dzf, xf, 2, sf=sf)
    assert sf.tolist() == [5, 6]
