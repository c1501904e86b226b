"""Oracles for gradient pass 2 (the split-K slab sums and the bias-partial sums), their
self-checks, and the refusals of the reduce launchers (CPU).

Pass 2 has two homes: wgrad_reduce_kernel (conv_mfma.hip) and the deferred path of
grad_update_kernel (elementwise.hip).  Both sum with the helpers of dg_common.h, whose comments
document one fixed order per sum.  tests/test_grad_reduce_gpu.py compares both homes with

* the float64 references reduce64 / bias64 (what is summed, and where it lands), and
* slab_order32 / chunk_order32 / rows_order32: numpy float32 emulations of the DOCUMENTED
  orders, one rounding per addition, written from those comments and not from device code.

The self-checks here keep a mistake in an oracle from passing as a kernel's: the references
against index loops, the emulations against hand-worked sums whose value depends on the order,
against float64 to the derived bound, and — the condition the GPU bit tests rest on — against a
left-to-right fp32 sum, from which the documented order must differ on a good share of the
Gaussian inputs.  The refusal tests call the real launchers with arguments they must reject
before any GPU work (skipped when _dghip is not built).
"""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

NPTS, BOARD = 361, 19
PAD_VALUE = 7.0          # what the builders put in the K padding: finite, in range, never read
U = 2.0 ** -24           # the unit roundoff of fp32
# integer-data totals that sit on bf16 ties (8 significant bits: 256 + 1 and 256 + 3 lie half
# way between neighbours): round-to-nearest-even gives 256, 260, -256
TIE_TOTALS = (257.0, 259.0, -257.0)
TIE_ROUNDED = (256.0, 260.0, -256.0)

# (M, Mpad, KP, taps, cin, cinp): the smallest shapes that reach each branch of the reduce
SHAPES = {
    "tiny": (8, 128, 128, 9, 5, 8),
    "first": (128, 128, 1024, 25, 37, 40),
    "hidden": (128, 128, 1152, 9, 128, 128),
    "wide": (256, 256, 2304, 9, 256, 256),
}
# what the GPU bit tests (Gaussian data) may use: sizes at which the documented order differs
# from a left-to-right sum on >= 20 % of the elements (test_documented_orders_are_telling)
GAUSS_SPLITS = (5, 13)
GAUSS_BCHUNKS = (4, 7)
MIN_DIFFERING_SHARE = 0.20


# ------------------------------------------------------------------- float64 references
def reduce64(slab, splits, M, Mpad, KP, taps, cin, cinp) -> torch.Tensor:
    """out[co][t][ci] = sum_z slab[z][co][t * cinp + ci] for co < M, t < taps, ci < cin
    (float64, [M][taps][cin]).  Rows co >= M and the K padding are never read."""
    s = torch.as_tensor(slab).reshape(splits, Mpad, KP)[:, :M, :taps * cinp]
    return s.reshape(splits, M, taps, cinp)[..., :cin].double().sum(0)


def split_bpart(bpart, bchunks, C):
    """bpart = [bchunks][361][C] position partials, then [bchunks][19][C] row partials."""
    b = torch.as_tensor(bpart).reshape(-1)
    assert b.numel() == bchunks * (NPTS + BOARD) * C
    n = bchunks * NPTS * C
    return b[:n].reshape(bchunks, NPTS, C), b[n:].reshape(bchunks * BOARD, C)


def bias64(bpart, bchunks, C):
    """(gposb [361][C], gbias [C]) in float64: gposb[p][c] = sum_chunk part[chunk][p][c],
    gbias[c] = sum_{chunk, h} rowpart[chunk][h][c]."""
    part, rows = split_bpart(bpart, bchunks, C)
    return part.double().sum(0), rows.double().sum(0)


# ---------------------------------------------- fp32 emulations of the documented orders
def _f32(x) -> np.ndarray:
    x = x.numpy() if isinstance(x, torch.Tensor) else np.asarray(x)
    assert x.dtype == np.float32
    return x


def slab_order32(x) -> np.ndarray:
    """Sum over axis 0 (the S split slabs) as dg_common.h documents it: four accumulators
    indexed z mod 4 over z < 4 floor(S / 4), the tail into accumulator 0, then
    (s0 + s1) + (s2 + s3).  float32, one rounding per addition."""
    x = _f32(x)
    S = x.shape[0]
    s = [np.zeros(x.shape[1:], np.float32) for _ in range(4)]
    for z in range(4 * (S // 4)):
        s[z % 4] = s[z % 4] + x[z]
    for z in range(4 * (S // 4), S):
        s[0] = s[0] + x[z]
    return (s[0] + s[1]) + (s[2] + s[3])


def chunk_order32(x) -> np.ndarray:
    """Sum over axis 0 (the board chunks): an even and an odd accumulator over the chunk pairs,
    a last unpaired chunk into the even one, then s0 + s1."""
    x = _f32(x)
    n = x.shape[0]
    s0 = np.zeros(x.shape[1:], np.float32)
    s1 = np.zeros(x.shape[1:], np.float32)
    for z in range(0, 2 * (n // 2), 2):
        s0 = s0 + x[z]
        s1 = s1 + x[z + 1]
    if n % 2:
        s0 = s0 + x[n - 1]
    return s0 + s1


def rows_order32(x) -> np.ndarray:
    """Sum over axis 0 (the R = chunks x 19 row partials): four partial sums indexed r mod 4
    over r < 4 floor(R / 4), in increasing r; the tail rows into partial 0; then
    (p0 + p1) + (p2 + p3)."""
    x = _f32(x)
    R = x.shape[0]
    p = [np.zeros(x.shape[1:], np.float32) for _ in range(4)]
    for r in range(4 * (R // 4)):
        p[r % 4] = p[r % 4] + x[r]
    for r in range(4 * (R // 4), R):
        p[0] = p[0] + x[r]
    return (p[0] + p[1]) + (p[2] + p[3])


def left_to_right32(x) -> np.ndarray:
    """The plain fp32 sum over axis 0, in index order: what the documented orders are NOT."""
    x = _f32(x)
    acc = np.zeros(x.shape[1:], np.float32)
    for z in range(x.shape[0]):
        acc = acc + x[z]
    return acc


ORDERS = {"slab": slab_order32, "chunks": chunk_order32, "rows": rows_order32}
# fp32 additions on the longest path of each documented tree, as a function of the length
N_ADD = {"slab": lambda S: S + 2, "chunks": lambda n: n + 1, "rows": lambda R: R + 2}


def sum_bound(kind: str, x) -> np.ndarray:
    """|fp32 sum in the documented order - exact sum| <= n_add 2^-24 sum|x| to first order (each
    of the n_add additions on an element's path rounds a partial sum of magnitude <= sum|x|)."""
    x = _f32(x).astype(np.float64)
    return N_ADD[kind](x.shape[0]) * U * np.abs(x).sum(0)


def reduce_order32(slab, splits, M, Mpad, KP, taps, cin, cinp) -> np.ndarray:
    """reduce64's selection summed by slab_order32: [M][taps][cin] float32."""
    s = _f32(slab).reshape(splits, Mpad, KP)[:, :M, :taps * cinp]
    return slab_order32(np.ascontiguousarray(s.reshape(splits, M, taps, cinp)[..., :cin]))


def bias_order32(bpart, bchunks, C):
    """(gposb, gbias) by chunk_order32 / rows_order32."""
    part, rows = split_bpart(bpart, bchunks, C)
    return chunk_order32(part), rows_order32(rows)


def reduce_bound(slab, splits, M, Mpad, KP, taps, cin, cinp) -> np.ndarray:
    s = _f32(slab).reshape(splits, Mpad, KP)[:, :M, :taps * cinp]
    return sum_bound("slab", np.ascontiguousarray(s.reshape(splits, M, taps, cinp)[..., :cin]))


def bias_bound(bpart, bchunks, C):
    part, rows = split_bpart(bpart, bchunks, C)
    return sum_bound("chunks", part), sum_bound("rows", rows)


# ------------------------------------------------------------------------ input builders
INT_MAX_ABS = 300    # integer data: |entry| <= 300 (+ a tie correction), sums far below 2^24


def _values(kind: str, shape, seed: int) -> torch.Tensor:
    gen = torch.Generator().manual_seed(seed)
    if kind == "int":
        return torch.randint(-INT_MAX_ABS, INT_MAX_ABS + 1, shape, generator=gen).float()
    assert kind == "gauss"
    return torch.randn(shape, generator=gen)


def assert_sums_exact(x: torch.Tensor):
    """Integer data whose fp32 sum over axis 0 is exact in ANY order: every entry is an integer
    and sum|x| < 2^24, so every partial sum of every order is an integer below 2^24."""
    x = x.double()
    assert torch.equal(x, x.round()), "entries are not integers"
    assert x.abs().sum(0).max().item() < 2 ** 24


def build_slab(kind, splits, M, Mpad, KP, taps, cin, cinp, seed) -> torch.Tensor:
    """[splits][Mpad][KP] fp32: `kind` values where the reduce reads, NaN in the rows co >= M,
    PAD_VALUE in the K padding (ci in [cin, cinp) and k >= taps * cinp).  kind 'int': the
    totals of (co 0, tap 0, ci 0 / 1 / 2) are TIE_TOTALS."""
    slab = torch.full((splits, Mpad, KP), PAD_VALUE)
    live = slab[:, :M, :taps * cinp].reshape(splits, M, taps, cinp)   # (a view: KP-strided)
    live[..., :cin] = _values(kind, (splits, M, taps, cin), seed)
    slab[:, M:, :] = float("nan")
    if kind == "int":
        assert cin >= len(TIE_TOTALS)
        for ci, total in enumerate(TIE_TOTALS):
            slab[0, 0, ci] += total - slab[:, 0, ci].sum()
        assert_sums_exact(live[..., :cin])
        assert reduce64(slab, splits, M, Mpad, KP, taps, cin, cinp)[0, 0, :3].tolist() == list(
            TIE_TOTALS)
    return slab


def build_bpart(kind, bchunks, C, seed) -> torch.Tensor:
    """Flat [bchunks][361][C] + [bchunks][19][C] fp32.  kind 'int': the totals of gposb[0][0..2]
    and of gbias[0..2] are TIE_TOTALS."""
    b = _values(kind, (bchunks * (NPTS + BOARD) * C,), seed)
    if kind == "int":
        part, rows = split_bpart(b, bchunks, C)       # views of b
        for c, total in enumerate(TIE_TOTALS):
            part[0, 0, c] += total - part[:, 0, c].sum()
            rows[0, c] += total - rows[:, c].sum()
        assert_sums_exact(part)
        assert_sums_exact(rows)
        gp, gb = bias64(b, bchunks, C)
        assert gp[0, :3].tolist() == list(TIE_TOTALS) and gb[:3].tolist() == list(TIE_TOTALS)
    return b


# ============================================================== self-checks of the oracles
def test_bf16_ties_round_to_even():
    got = torch.tensor(TIE_TOTALS).to(torch.bfloat16).float().tolist()
    assert got == list(TIE_ROUNDED)


def test_reduce64_against_index_loops():
    splits, M, Mpad, KP, taps, cin, cinp = 3, 2, 4, 16, 3, 3, 4
    slab = build_slab("int", splits, M, Mpad, KP, taps, cin, cinp, 1)
    got = reduce64(slab, splits, M, Mpad, KP, taps, cin, cinp)
    assert got.shape == (M, taps, cin) and got.dtype == torch.float64
    flat = slab.reshape(-1).tolist()
    for co in range(M):
        for t in range(taps):
            for ci in range(cin):
                want = sum(flat[(z * Mpad + co) * KP + t * cinp + ci] for z in range(splits))
                assert got[co, t, ci].item() == want
    # the padding is where the builder says, and nowhere else
    s = slab.reshape(splits, Mpad, KP)
    assert torch.isnan(s[:, M:, :]).all() and not torch.isnan(s[:, :M, :]).any()
    assert (s[:, :M, taps * cinp:] == PAD_VALUE).all()
    assert (s[:, :M, :taps * cinp].reshape(splits, M, taps, cinp)[..., cin:] == PAD_VALUE).all()


def test_bias64_against_index_loops():
    bchunks, C = 3, 8
    b = build_bpart("int", bchunks, C, 2)
    gp, gb = bias64(b, bchunks, C)
    assert gp.shape == (NPTS, C) and gb.shape == (C,)
    flat = b.tolist()
    base = bchunks * NPTS * C
    for p in (0, 1, 200, NPTS - 1):
        for c in range(C):
            assert gp[p, c].item() == sum(flat[(z * NPTS + p) * C + c] for z in range(bchunks))
    for c in range(C):
        want = sum(flat[base + (z * BOARD + h) * C + c] for z in range(bchunks)
                   for h in range(BOARD))
        assert gb[c].item() == want


def test_orders_on_hand_worked_sums():
    """2^24 + 1 rounds back to 2^24 (a tie, to even), so where the ones are added decides the
    result.  Worked by hand from the documented orders."""
    big, one = 2.0 ** 24, 1.0
    col = lambda *v: np.array(v, np.float32).reshape(-1, 1)   # noqa: E731
    # slab, S = 5: s0 = (2^24 + x4 = 1) -> 2^24, s1 = s2 = s3 = 1; (2^24 + 1 -> 2^24) + (1 + 1)
    x = col(big, one, one, one, one)
    assert slab_order32(x)[0] == big + 2 and left_to_right32(x)[0] == big
    # (the tail in accumulator 1 instead would give (2^24 + 2) + 2)
    # chunks, n = 4: s0 = 2^24 + 1 -> 2^24, s1 = 1 + 1; 2^24 + 2
    x = col(big, one, one, one)
    assert chunk_order32(x)[0] == big + 2 and left_to_right32(x)[0] == big
    # chunks, n = 3: the unpaired chunk joins the even accumulator: (1 + 1) + 2^24
    x = col(one, big, one)
    assert chunk_order32(x)[0] == big + 2 and left_to_right32(x)[0] == big
    # rows, R = 9: p0 = 2^24 + x4 + x8 -> 2^24, p1 = p2 = p3 = 2; (2^24 + 2) + 4
    x = col(big, *([one] * 8))
    assert rows_order32(x)[0] == big + 6 and left_to_right32(x)[0] == big
    # rows, R = 6: rows 4 and 5 are the tail, both into partial 0
    x = col(one, big, one, one, one, one)
    # p0 = 1 + 1 + 1, p1 = 2^24: (3 + 2^24 -> 2^24 + 4, a tie to even) + (1 + 1); spread over
    # partials 0 and 1 instead the tail would give (2 + 2^24) + 2
    assert rows_order32(x)[0] == big + 6 and left_to_right32(x)[0] == big


def _kind_input(kind, n, data):
    """[n][4096] inputs of one kind, from the builders the GPU tests use."""
    if kind == "slab":
        _, Mpad, KP, taps, cin, cinp = SHAPES["tiny"]
        s = build_slab(data, n, 64, Mpad, KP, taps, cin, cinp, 10 + n)
        return np.ascontiguousarray(s[:, :64, :taps * cinp].reshape(n, 64, taps, cinp)[..., :cin]
                                    .reshape(n, -1).numpy())
    if kind == "chunks":
        part, _ = split_bpart(build_bpart(data, n, 8, 20 + n), n, 8)
        return np.ascontiguousarray(part.reshape(n, -1).numpy())
    chunks = n // BOARD
    assert chunks * BOARD == n
    _, rows = split_bpart(build_bpart(data, chunks, 256, 30 + n), chunks, 256)
    return np.ascontiguousarray(rows.numpy())


SIZES = {"slab": (1, 3, 4, 5, 8, 13, 64), "chunks": (1, 2, 3, 4, 5, 7),
         "rows": (19, 38, 76, 133)}
ALL_SIZES = [(k, n) for k, v in SIZES.items() for n in v]


@pytest.mark.parametrize("kind,n", ALL_SIZES)
def test_emulation_within_derived_bound_of_float64(kind, n):
    x = _kind_input(kind, n, "gauss")
    err = np.abs(ORDERS[kind](x).astype(np.float64) - x.astype(np.float64).sum(0))
    bound = sum_bound(kind, x)
    assert (err <= bound).all(), (err / bound).max()
    assert err.max() > 0 or n == 1      # (an fp32 sum: it does round)


@pytest.mark.parametrize("kind,n", ALL_SIZES)
def test_emulation_is_exact_on_integer_data(kind, n):
    x = _kind_input(kind, n, "int")
    assert_sums_exact(torch.from_numpy(x))
    got = ORDERS[kind](x)
    assert got.dtype == np.float32
    assert np.array_equal(got.astype(np.float64), x.astype(np.float64).sum(0))
    assert np.array_equal(got, left_to_right32(x))


TELLING = ([("slab", s) for s in GAUSS_SPLITS] + [("chunks", c) for c in GAUSS_BCHUNKS]
           + [("rows", c * BOARD) for c in GAUSS_BCHUNKS])


@pytest.mark.parametrize("kind,n", TELLING)
def test_documented_orders_are_telling(kind, n):
    """The condition on the INPUTS of the GPU bit tests: at every (kind, size) they use, the
    documented order and a left-to-right fp32 sum differ on at least 20 % of the Gaussian
    elements — a kernel that summed in another order would not pass by luck.  (S = 3 and 2
    chunks differ nowhere: the tail-only paths ARE left to right, so those sizes serve the
    integer-data tests only.)"""
    x = _kind_input(kind, n, "gauss")
    share = float((ORDERS[kind](x) != left_to_right32(x)).mean())
    print(f"ORDER_SHARE kind={kind} n={n} differing={share:.3f}")
    assert share >= MIN_DIFFERING_SHARE, share


def test_tail_only_sizes_are_left_to_right():
    for kind, n in (("slab", 3), ("chunks", 2)):
        x = _kind_input(kind, n, "gauss")
        assert np.array_equal(ORDERS[kind](x), left_to_right32(x))


# ======================================================= refusals of the reduce launchers
@pytest.fixture
def h():
    from deep_go_amd.ops import native
    if not native.hip_available():
        pytest.skip("_dghip is not built")
    return native.hip()


# Addresses that are never dereferenced: every call below must be refused on the host.  The
# base is the 'tiny' shape with a bias part, which tests/test_grad_reduce_gpu.py launches with
# real buffers — so each case differs from an accepted call in the named field(s) only.
A_SLAB, A_OUT, A_BPART, A_GPOSB, A_GBIAS, A_TWIN = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000, \
    0x60000
BASE = dict(slab=A_SLAB, out=A_OUT, splits=5, M=8, Mpad=128, KP=128, taps=9, cin=5, cinp=8,
            bpart=A_BPART, bchunks=4, gposb=A_GPOSB, gbias=A_GBIAS)
ROW_ORDER = ("slab", "out", "bpart", "gposb", "gbias", "splits", "M", "Mpad", "KP", "taps",
             "cin", "cinp", "bchunks")
NO_BIAS = dict(bpart=0, bchunks=0, gposb=0, gbias=0)
RULES = {
    "slab null": dict(slab=0),
    "out null": dict(out=0),
    "slab not 16-byte aligned": dict(slab=A_SLAB + 4),
    "slab 8-byte aligned only": dict(slab=A_SLAB + 8),
    "splits 0": dict(splits=0),
    "splits negative": dict(splits=-1),
    "M 0": dict(M=0),
    "M > Mpad": dict(M=129),
    "KP 0": dict(KP=0),
    "KP negative": dict(KP=-128),
    "KP % 4": dict(KP=126),
    "KP % 4 (odd)": dict(KP=129),
    "taps 0": dict(taps=0),
    "cin 0": dict(cin=0),
    "cinp 0": dict(cin=0, cinp=0),
    "cinp 0, cin 1": dict(cin=1, cinp=0),
    "cin > cinp": dict(cin=9),
    "taps * cinp > KP": dict(taps=17),
    "taps * cinp > KP (cinp)": dict(cin=5, cinp=16),
    "M * KP / 4 past int": dict(M=1 << 20, Mpad=1 << 20, KP=1 << 13),
    "bchunks 0": dict(bchunks=0),
    "bchunks negative": dict(bchunks=-2),
    "gposb null": dict(gposb=0),
    "gbias null": dict(gbias=0),
    "gposb and gbias null": dict(gposb=0, gbias=0),
}
# the same rules hold without a bias part
for _name in ("slab null", "out null", "slab not 16-byte aligned", "splits 0", "M > Mpad",
              "KP % 4", "cinp 0", "cin > cinp", "taps * cinp > KP", "M * KP / 4 past int"):
    RULES[_name + ", no bias part"] = {**NO_BIAS, **RULES[_name]}
MULTI_ONLY_RULES = {"bpart null": NO_BIAS, "bpart null, outputs given": dict(bpart=0)}


def _single_args(f, api):
    a = [f["slab"], f["out"], f["splits"], f["M"], f["Mpad"], f["KP"], f["taps"], f["cin"],
         f["cinp"], f["bpart"], f["bchunks"], f["gposb"], f["gbias"]]
    if api == "wgrad_reduce_w":
        a += [f.get("out16", 0), f.get("gposb16", 0), f.get("gbias16", 0)]
    return a + [0, 0]      # sf, stream


def _refused(fn, name, *args):
    with pytest.raises(RuntimeError) as e:
        fn(*args)
    assert str(e.value) == f"{name}: invalid argument"


@pytest.mark.parametrize("rule", list(RULES))
@pytest.mark.parametrize("api", ["wgrad_reduce", "wgrad_reduce_w"])
def test_single_layer_reduce_refuses(h, api, rule):
    f = {**BASE, **RULES[rule]}
    _refused(getattr(h, api), api, *_single_args(f, api))
    if api == "wgrad_reduce_w":     # twins given change nothing
        f.update(out16=A_TWIN, gposb16=A_TWIN + 0x1000, gbias16=A_TWIN + 0x2000)
        _refused(getattr(h, api), api, *_single_args(f, api))


def _row(f, cols):
    r = [f[k] for k in ROW_ORDER]
    if cols == 16:
        r += [f.get("out16", 0), f.get("gposb16", 0), f.get("gbias16", 0)]
    return r


MULTI = {"wgrad_reduce_multi": 13, "wgrad_reduce_multi_w": 16}


@pytest.mark.parametrize("rule", list(RULES) + list(MULTI_ONLY_RULES))
@pytest.mark.parametrize("api", list(MULTI))
def test_multi_reduce_refuses_a_bad_row(h, api, rule):
    """The bad row alone, and as the last of three rows behind two good ones."""
    cols = MULTI[api]
    bad = {**BASE, **{**RULES, **MULTI_ONLY_RULES}[rule]}
    good = dict(BASE)
    if cols == 16:
        good.update(out16=A_TWIN)       # (twins are optional, each on its own)
    for rows in ([bad], [good, good, bad]):
        t = np.ascontiguousarray(np.array([_row(f, cols) for f in rows], dtype=np.int64))
        _refused(getattr(h, api), api, t.ctypes.data, len(rows), 0)


@pytest.mark.parametrize("api", list(MULTI))
def test_multi_reduce_refuses_a_bad_table(h, api):
    cols = MULTI[api]
    t = np.ascontiguousarray(np.array([_row(BASE, cols)] * 17, dtype=np.int64))
    _refused(getattr(h, api), api, t.ctypes.data, 17, 0)      # more rows than the kernel holds
    _refused(getattr(h, api), api, t.ctypes.data, 0, 0)
    _refused(getattr(h, api), api, t.ctypes.data, -1, 0)
    _refused(getattr(h, api), api, 0, 1, 0)                   # no table
    # an int64 column that only looks valid once narrowed to int: splits = 2^32 + 5
    f = dict(BASE, splits=(1 << 32) + 5)
    t = np.ascontiguousarray(np.array([_row(f, cols)], dtype=np.int64))
    _refused(getattr(h, api), api, t.ctypes.data, 1, 0)
