"""conv_stack2's copy-out table (csrc/kernels/conv_stack2.hip builds it in LDS; its formula is
mirrored by layouts.stack_copyout_table): every pixel's entry against the frame row and swizzle
signature written out independently, and the three addresses the kernel derives from an entry
against the ones it used to compute per K-step."""
import pytest
import torch

from deep_go_amd.ops import exact as E
from deep_go_amd.ops import layouts as LY

# the (exact.stack_case arguments) tests/test_stack_copyout_gpu.py launches: B = 1 and an odd
# count, nl = 1 (exposed copy-out only), 2 (one in-loop copy-out), 3 (a copy-out under a layer
# that is itself copied out), both directions; l1 mode and the fused head at nl = 2
COPYOUT_CASES = [(128, B, nl, epi, 300 + 10 * B + nl + (50 if epi == "dgrad" else 0), False)
                 for B in (1, 3) for nl in (1, 2, 3) for epi in ("fwd", "dgrad")]
L1_CASE = (128, 3, 2, "fwd", 103, True)
HEAD_CASE = (128, 3, 2, "fwd", 332, False)

SCRATCH = 12 * 1024      # the head scratch the table lives in; its last 16 B are the counters


def test_table_entries_for_all_pixels():
    tab = LY.stack_copyout_table().tolist()
    assert len(tab) == 384 and 4 * len(tab) <= SCRATCH - 16
    for h in range(19):
        for w in range(19):
            p = 19 * h + w
            e = tab[p]
            f = (h + 1) * 21 + (w + 1)
            sig = ((w + 1) + 3 * (h + 1)) & 7
            assert e & 0xFFFF == f * 128 + sig * 16, (h, w)
            assert e & 0xF == 0 and (e >> 4) & 7 == sig and (e & 0xFF80) == f * 128, (h, w)
            assert e >> 16 == p, (h, w)
            for q in range(8):
                # LDS byte offset of channel piece q: slot q ^ sig of frame row f
                assert (e & 0xFFF0) ^ (q << 4) == f * 128 + ((q ^ sig) << 4), (h, w, q)
                # byte offset in the [21][21][128] bf16 frame (image half hf adds 128)
                assert ((e & 0xFF80) << 1) + (q << 4) == (f * 128 + q * 8) * 2, (h, w, q)
    assert max(tab) < 1 << 25


def test_entries_past_the_board_repeat_the_last_pixel():
    tab = LY.stack_copyout_table().tolist()
    assert all(e == tab[360] for e in tab[361:])
    # the 6 copy-out steps of an image cover tid / 8 + 64 j for 512 threads: entries 0..383
    assert {t // 8 + 64 * j for t in range(512) for j in range(6)} == set(range(384))


def test_interior_rows_only():
    """No entry addresses a border row or column of the frame (the copy-out never writes one)."""
    for e in LY.stack_copyout_table().tolist():
        f = (e & 0xFF80) >> 7
        assert 1 <= f // 21 <= 19 and 1 <= f % 21 <= 19


@pytest.mark.parametrize("case", COPYOUT_CASES + [L1_CASE, HEAD_CASE])
def test_cases_meet_the_exactness_condition(case):
    """The builders assert order independence on the inputs; here also that every layer has
    zero and nonzero outputs (both values of a ReLU bit, a gated and an ungated gradient)."""
    C, B, nl, epi, seed, l1 = case
    c = E.stack_case(C, B, nl, epi, seed, l1)
    assert len(c["ref"]) == nl
    for v, y, _ in c["ref"]:
        nz = (y != 0).float().mean().item()
        assert 0.05 < nz < 0.95
    assert torch.equal(c["ref"][0][1], c["ref"][0][0])
