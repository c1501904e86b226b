"""The CPU side of the bit-exact kernel tests (deep_go_amd/ops/exact.py): the integer data
meets the order-independence condition at every shape tests/test_exact_gpu.py launches, that
condition really makes a float32 sum independent of its order, and the fp8 emulation produces
the known byte patterns."""
import pytest
import torch

from deep_go_amd.ops import exact as E

# every (builder, arguments) the GPU tests use: kept here so that a shape added there without
# the condition holding fails on the CPU first (test_exact_gpu.py imports these lists)
STACK_CASES = [(128, 5, 3, "fwd", 101, False), (128, 5, 3, "dgrad", 102, False),
               (128, 3, 3, "fwd", 103, True),
               (256, 3, 3, "fwd", 104, False), (256, 3, 3, "dgrad", 105, False),
               (128, 3, 3, "fwd", 106, False), (128, 3, 3, "dgrad", 107, False)]
F8_CASES = [(128, 5, 3, "fwd", 111, -1, 1), (128, 5, 3, "dgrad", 112, 0, 0),
            (256, 3, 3, "fwd", 113, 0, 0), (256, 3, 3, "dgrad", 114, -1, 1)]
F8_SR_CASE = (128, 3, 2, "dgrad", 115, 0, 0, True)
WGRAD_WIN_CASES = [(3, 128, 128, None), (1, 128, 128, 1), (2, 128, 128, 26), (5, 256, 256, None),
                   (4, 64, 128, 7), (3, 192, 256, 2), (6, 128, 128, 5), (3, 128, 64, None)]
WGRAD_WIN8_CASES = [(4, 128, 128, 1), (4, 128, 128, 5), (8, 128, 128, 13), (8, 256, 256, None),
                    (4, 256, 256, 3)]
WGRAD_IM2COL_CASES = [(3, 128, 128, 3, 7, None),     # three-slice (K % 384 == 0)
                      (3, 64, 64, 3, None, None),    # 2-stage
                      (3, 40, 128, 5, 3, 37)]        # 5x5 pipe, 37 real channels of 40
CONV_CASES = [(2, 64, 64, 3), (3, 256, 256, 3)]      # the smallest current shape, and C = 256
CONV_NT_TILES = {64: [None, (64, 128), (64, 256)], 256: [None, (128, 128), (128, 192)]}
L1_CASES = [(3, 40, 128, 5), (3, 64, 128, 3), (2, 40, 256, 5)]
L1_FRAG_M = [128, 256, 384]
BOARD_FP8_CASES = [(3, 128, 128, 64), (2, 256, 256, 128)]


@pytest.mark.parametrize("case", STACK_CASES)
def test_stack_cases_order_independent(case):
    C, B, nl, epi, seed, l1 = case
    c = E.stack_case(C, B, nl, epi, seed, l1)
    assert len(c["ref"]) == nl
    v0 = c["ref"][0][0]
    assert v0.abs().max().item() <= 256 and torch.equal(v0, v0.round())
    # several boards with independent draws: nearly every (pixel, channel) is nonzero on some
    # board while the ReLU / the masks still zero a good part of each (both sides are seen)
    nz = c["ref"][0][1] != 0
    assert nz.any(0).float().mean().item() > 0.8 and nz.float().mean().item() < 0.9


@pytest.mark.parametrize("case", F8_CASES + [F8_SR_CASE])
def test_fp8_cases_order_independent(case):
    c = E.stack_f8_case(*case)
    L = c["ref"]["layers"]
    assert len(L) == case[2] and L[-1]["y8"] is None
    if case == F8_SR_CASE:
        # stochastic rounding of a representable value is the identity: layer 0's values
        # are e5m2 numbers at its output scale
        v = L[0]["v"] / c["s"][1]
        assert torch.equal(E.d_e5m2(E.q_e5m2(v)), v) and v.abs().max().item() >= 2


def test_wgrad_and_conv_cases_order_independent():
    for B, cin, cout, _ in WGRAD_WIN_CASES + WGRAD_WIN8_CASES:
        E.wgrad_case(B, cin, cout, 3, 120 + B)
    for B, cin, cout, k, _, real in WGRAD_IM2COL_CASES:
        c = E.wgrad_case(B, cin, cout, k, 130 + B, real)
        if real is not None:
            assert c["ref"][..., real:].abs().sum().item() == 0
    for B, cin, cout, k in CONV_CASES + L1_CASES:
        c = E.conv_case(B, cin, cout, k, 140 + B)
        assert max(c["lin"].abs().max().item(), c["fwd"].max().item()) <= 256
    for M in L1_FRAG_M:
        assert E.conv_case(3, 40, M, 5, 150)["fwd"].max().item() <= 256
    for B, cin, cout, _ in BOARD_FP8_CASES:
        E.conv_case(B, cin, cout, 3, 144, 2)


def test_condition_rejects_inexact_data():
    x = E.int_acts((1, 19, 19, 128), 1, 1)
    A = E.sign_weights((128, 1152), 2)
    E.assert_order_independent(x, A, 1.0)
    with pytest.raises(AssertionError):       # products that are not multiples of q
        E.assert_order_independent(x * 0.5, A, 1.0)
    with pytest.raises(AssertionError):       # a sum past 2^24 q
        E.assert_order_independent(x * 2 ** 15, A, 1.0)
    with pytest.raises(AssertionError):       # an unrounded bf16 comparison past 256 q
        E.assert_order_independent(x, A, 1.0, ref=torch.full((1,), 257.0))
    with pytest.raises(AssertionError):
        E.assert_order_independent(x, A, 1.0, bias=torch.full((1,), 0.5))


@pytest.mark.parametrize("layer", [0, 1, 2])
def test_float64_oracle_equals_shuffled_float32_sum(layer):
    """What proves exactness: under the condition, a float32 evaluation that adds one product
    at a time with K visited in a shuffled order equals the float64 oracle bit for bit — at
    layer 0 ({0, 1} inputs) and at the deeper layers' bf16 inputs in the thousands."""
    c = E.stack_case(128, 3, 3, "fwd", 106)
    _, _, inp = c["ref"][layer]
    A = c["As"][layer]
    want = E.conv64(inp[:2], A)
    for seed in (1, 2):
        got = E.shuffled_fp32_conv(inp[:2], A, seed)
        assert torch.equal(got.double(), want)
    # and it does NOT hold without the condition: Gaussian data changes with the order
    g = torch.randn(1, 19, 19, 128, generator=torch.Generator().manual_seed(0)).double()
    assert not torch.equal(E.shuffled_fp32_conv(g, A, 1), E.shuffled_fp32_conv(g, A, 2))


def test_shuffled_sum_5x5_and_wgrad_reference():
    c = E.stack_case(128, 3, 3, "fwd", 103, True)
    x, A = c["x"][:1], c["As"][0]
    assert torch.equal(E.shuffled_fp32_conv(x, A[:, :1000], 3, k=5).double(),
                       E.conv64(x, A[:, :1000], 5))
    # the weight-gradient oracle against an explicit shifted sum
    w = E.wgrad_case(3, 64, 64, 3, 133)
    for tap in (0, 4, 8):
        want = torch.einsum("bhwo,bhwi->oi", w["dz"], E.shifted(w["x"], tap))
        assert torch.equal(w["ref"][:, tap // 3, tap % 3, :], want)


def test_fp8_emulation_known_bytes():
    """e4m3 (OCP, no infinities, max 448) and e5m2 (max finite 57344) bytes: exact values, ties
    to even in the normal and subnormal ranges, saturation."""
    t = lambda v: torch.tensor(v, dtype=torch.float64)   # noqa: E731
    e4 = {0.0: 0x00, 1.0: 0x38, -1.0: 0xB8, 2.0: 0x40, 0.5: 0x30, 448.0: 0x7E, 1000.0: 0x7E,
          -1000.0: 0xFE, 16.0: 0x58, 17.0: 0x58, 18.0: 0x59, 19.0: 0x5A, 21.0: 0x5A,
          2.0 ** -9: 0x01, 2.0 ** -10: 0x00, 3 * 2.0 ** -10: 0x02, 224.0: 0x76, 464.0: 0x7E}
    got = E.q_e4m3(t(list(e4.keys()))).tolist()
    assert got == list(e4.values())
    e5 = {0.0: 0x00, 1.0: 0x3C, -2.0: 0xC0, 4.0: 0x44, 5.0: 0x45, 8.0: 0x48, 9.0: 0x48,
          10.0: 0x49, 11.0: 0x4A, 13.0: 0x4A, 57344.0: 0x7B, 1e6: 0x7B, -1e6: 0xFB,
          2.0 ** -16: 0x01, 2.0 ** -17: 0x00, 3 * 2.0 ** -17: 0x02}
    got = E.q_e5m2(t(list(e5.keys()))).tolist()
    assert got == list(e5.values())
    # decode is the inverse on every finite byte
    allb = torch.arange(256, dtype=torch.uint8)
    f4 = E.d_e4m3(allb)
    ok4 = torch.isfinite(f4)
    assert int(ok4.sum()) == 254 and torch.equal(E.q_e4m3(f4[ok4]), allb[ok4])
    f5 = E.d_e5m2(allb)
    ok5 = torch.isfinite(f5)
    assert int(ok5.sum()) == 248
    assert torch.equal(E.q_e5m2(f5[ok5]), allb[ok5])


def test_fp8_stack_emulation_rules():
    """stack_f8_64: non-last layers store q(v / s_out) and the frame bf16(q s_out), the last
    bf16(v); the masks gate the backward-data values; saturation shows in the deep layers."""
    c = E.stack_f8_case(128, 5, 3, "fwd", 111, -1, 1)
    L = c["ref"]["layers"]
    s = c["s"]
    assert torch.equal(L[0]["y"], E.d_e4m3(L[0]["y8"]) * s[1])
    assert torch.equal(L[1]["xq"], E.d_e4m3(L[0]["y8"]))
    assert torch.equal(L[2]["y"], E.bf16_round(L[2]["v"]))
    assert (L[1]["v"] / s[2]).max().item() > 448 and E.d_e4m3(L[1]["y8"]).max().item() == 448
    d = E.stack_f8_case(128, 5, 3, "dgrad", 112, 0, 0)
    Ld = d["ref"]["layers"]
    assert torch.equal(Ld[0]["v"] != 0, (E.mask_bits(d["masks"][0]) != 0) & (Ld[0]["v"] != 0))
    assert Ld[0]["v"][E.mask_bits(d["masks"][0]) == 0].abs().sum().item() == 0


def test_layout_helpers():
    from deep_go_amd.ops import layouts as LY
    A = torch.arange(128 * 1152, dtype=torch.float32).reshape(128, 1152)
    assert torch.equal(E.frag_bf16(A, 128), LY.stack_frag(A))
    m = E.relu_masks(2, 128, 3)
    assert torch.equal(E.pack_mask(E.mask_bits(m) != 0), m)
    x = E.int_acts((1, 19, 19, 2), 5, 4)
    assert torch.equal(E.shifted(x, 4), x)
    assert torch.equal(E.shifted(x, 0)[:, 1:, 1:], x[:, :-1, :-1])
    assert E.shifted(x, 0)[:, 0].abs().sum().item() == 0
    assert E.quantum(torch.tensor([0.75, 2.0])) == 0.25
