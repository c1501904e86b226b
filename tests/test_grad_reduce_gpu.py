"""Gradient pass 2 — the split-K slab sums and the bias-partial sums — against the oracles of
tests/test_grad_reduce_cpu.py (GPU).

Part A drives wgrad_reduce / wgrad_reduce_w / wgrad_reduce_multi / wgrad_reduce_multi_w on
synthetic slabs and partials (no convolution runs).  Part B drives the deferred path of
grad_update on a hand-built parameter vector.  On integer data every sum is exact in any order,
so the outputs equal the float64 references exactly (and the bf16 twins the once-rounded fp32
result, designed ties included); on Gaussian data they are bit-identical to the fp32 emulations
of the orders dg_common.h documents — at sizes where those differ from a left-to-right sum on
>= 20 % of the elements (the CPU file asserts it) — and within the derived bound of float64.

Every output sits between sentinel guards and is pre-filled with NaN; slab rows co >= M are
NaN and the K padding is 7, so a read of either, or an entry left unwritten, shows.
"""
import numpy as np
import pytest
import torch

from test_grad_reduce_cpu import (BOARD, GAUSS_BCHUNKS, GAUSS_SPLITS, NPTS, PAD_VALUE, SHAPES,
                                  TIE_ROUNDED, bias64, bias_bound, bias_order32, build_bpart,
                                  build_slab, reduce64, reduce_bound, reduce_order32)
from test_update_gpu import guarded, guards_intact, same_bits

pytestmark = pytest.mark.gpu

DEV = "cuda"
NAN = float("nan")
OUTS = ("out", "gposb", "gbias")
TWINS = ("out16", "gposb16", "gbias16")


def _h():
    from deep_go_amd.ops.native import hip
    return hip()


def _s():
    from deep_go_amd.ops.native import stream_handle
    return stream_handle()


def _tag():
    from deep_go_amd.ops.exact import new_step_tag
    return new_step_tag(DEV)


# ================================================================ A: the reduce family
class Case:
    """One layer's pass-2 inputs (CPU and device) and its references, computed once."""

    def __init__(self, shape, splits, bchunks, kind, seed):
        self.shape = SHAPES[shape] if isinstance(shape, str) else shape
        self.splits, self.bchunks, self.kind = splits, bchunks, kind
        M = self.shape[0]
        self.slab = build_slab(kind, splits, *self.shape, seed)
        self.bpart = build_bpart(kind, bchunks, M, seed + 1) if bchunks else None
        self.slab_d = self.slab.to(DEV)
        self.bpart_d = self.bpart.to(DEV) if bchunks else None
        self.sizes = {"out": M * self.shape[3] * self.shape[4], "gposb": NPTS * M, "gbias": M}
        self._ref64 = self._ref32 = self._bound = None

    def dims(self):
        """(splits, M, Mpad, KP, taps, cin, cinp)"""
        return (self.splits,) + tuple(self.shape)

    def names(self, twins=False):
        n = OUTS if self.bchunks else OUTS[:1]
        return n + tuple(t for t in TWINS if t[:-2] in n) if twins else n

    def ref64(self):
        if self._ref64 is None:
            r = {"out": reduce64(self.slab, *self.dims()).reshape(-1)}
            if self.bchunks:
                gp, gb = bias64(self.bpart, self.bchunks, self.shape[0])
                r.update(gposb=gp.reshape(-1), gbias=gb)
            self._ref64 = r
        return self._ref64

    def ref32(self):
        if self._ref32 is None:
            r = {"out": torch.from_numpy(reduce_order32(self.slab, *self.dims()).reshape(-1))}
            if self.bchunks:
                gp, gb = bias_order32(self.bpart, self.bchunks, self.shape[0])
                r.update(gposb=torch.from_numpy(gp.reshape(-1)), gbias=torch.from_numpy(gb))
            self._ref32 = r
        return self._ref32

    def bound(self):
        if self._bound is None:
            r = {"out": torch.from_numpy(reduce_bound(self.slab, *self.dims()).reshape(-1))}
            if self.bchunks:
                gp, gb = bias_bound(self.bpart, self.bchunks, self.shape[0])
                r.update(gposb=torch.from_numpy(gp.reshape(-1)), gbias=torch.from_numpy(gb))
            self._bound = r
        return self._bound

    def outputs(self, twins=()):
        """{name: (allocation, view)}: NaN-filled, guarded; fp32 outputs and the asked twins."""
        o = {n: guarded(torch.full((self.sizes[n],), NAN)) for n in self.names()}
        for t in twins:
            if t[:-2] in o:
                o[t] = guarded(torch.full((self.sizes[t[:-2]],), NAN, dtype=torch.bfloat16))
        return o


def _ptr(o, name):
    return o[name][1].data_ptr() if name in o else 0


def launch_single(c: Case, api: str, twins=(), sf=None):
    """One single-layer launch; returns {name: CPU tensor} after checking the guards."""
    h = _h()
    o = c.outputs(twins)
    a = [c.slab_d.data_ptr(), _ptr(o, "out"), *c.dims(),
         c.bpart_d.data_ptr() if c.bchunks else 0, c.bchunks, _ptr(o, "gposb"), _ptr(o, "gbias")]
    if api == "wgrad_reduce_w":
        a += [_ptr(o, t) for t in TWINS]
    else:
        assert not twins
    getattr(h, api)(*a, sf.data_ptr() if sf is not None else 0, _s())
    torch.cuda.synchronize()
    for n, (buf, _) in o.items():
        assert guards_intact(buf), (api, n)
    return {n: v.cpu() for n, (_, v) in o.items()}


def multi_row(c: Case, o, cols):
    r = [c.slab_d.data_ptr(), _ptr(o, "out"), c.bpart_d.data_ptr(), _ptr(o, "gposb"),
         _ptr(o, "gbias"), *c.dims(), c.bchunks]
    return r + [_ptr(o, t) for t in TWINS] if cols == 16 else r


def launch_multi(cases, cols, twins_of=None):
    """One wgrad_reduce_multi(_w) launch over `cases`; twins_of[i]: the twins row i is given."""
    h = _h()
    twins_of = twins_of or [()] * len(cases)
    outs = [c.outputs(t) for c, t in zip(cases, twins_of)]
    tab = np.ascontiguousarray(np.array([multi_row(c, o, cols) for c, o in zip(cases, outs)],
                                        dtype=np.int64))
    fn = h.wgrad_reduce_multi_w if cols == 16 else h.wgrad_reduce_multi
    fn(tab.ctypes.data, len(cases), _s())
    torch.cuda.synchronize()
    for i, o in enumerate(outs):
        for n, (buf, _) in o.items():
            assert guards_intact(buf), (i, n)
    return [{n: v.cpu() for n, (_, v) in o.items()} for o in outs]


def check_written(c: Case, got, ctx=""):
    """Every entry written, nothing of the NaN rows or of the K padding in it."""
    ref = c.ref64()
    for n, v in got.items():
        v = v.float()
        assert not torch.isnan(v).any(), (ctx, n, int(torch.isnan(v).sum()))
        r = ref[n[:-2] if n.endswith("16") else n]
        leaked = (v == PAD_VALUE) & (r != PAD_VALUE)
        if n.endswith("16"):
            leaked &= r.float().to(torch.bfloat16).float() != PAD_VALUE
        assert not leaked.any(), (ctx, n, "the K padding reached the output")


def check_exact(c: Case, got, ctx=""):
    """Integer data: fp32 outputs equal float64 exactly; twins = the fp32 result rounded once."""
    check_written(c, got, ctx)
    ref = c.ref64()
    for n in c.names():
        bad = (got[n].double() != ref[n]).nonzero().reshape(-1)
        assert bad.numel() == 0, (ctx, n, bad.numel(), bad[:8].tolist())
    for t in TWINS:
        if t in got:
            assert same_bits(got[t], got[t[:-2]].to(torch.bfloat16)), (ctx, t)
            # the designed ties (the first three totals of every output): to nearest even
            assert got[t][:3].float().tolist() == list(TIE_ROUNDED), (ctx, t)


def check_order(c: Case, got, ctx=""):
    """Gaussian data: the documented order bit for bit; float64 to the derived bound.  Returns
    {name: max err / bound}."""
    check_written(c, got, ctx)
    ref32, ref64, bound = c.ref32(), c.ref64(), c.bound()
    worst = {}
    for n in c.names():
        a, b = got[n].view(torch.int32), ref32[n].view(torch.int32)
        bad = (a != b).nonzero().reshape(-1)
        assert bad.numel() == 0, (ctx, n, "differs from the documented order", bad.numel(),
                                  bad.numel() / a.numel(), bad[:8].tolist())
        err = (got[n].double() - ref64[n]).abs()
        ratio = (err / bound[n].clamp_min(1e-300)).max().item()
        assert (err <= bound[n]).all(), (ctx, n, ratio)
        worst[n] = ratio
    for t in TWINS:
        if t in got:
            assert same_bits(got[t], got[t[:-2]].to(torch.bfloat16)), (ctx, t)
    return worst


def _same_outputs(a, b, names):
    return all(same_bits(a[n], b[n]) for n in names)


ALL_SPLITS = (1, 3, 4, 5, 8, 13)
ALL_BCHUNKS = (1, 2, 4, 7)   # R = 19 (tail only), 38 (tail of 2), 76 (one 16-row pass, no
#                              tail), 133 (two passes + the plain loop + a tail of 1)


@pytest.mark.parametrize("splits", ALL_SPLITS)
@pytest.mark.parametrize("shape", list(SHAPES))
def test_reduce_exact_on_integer_data(shape, splits):
    """wgrad_reduce and wgrad_reduce_w (all twins, one twin, none) on integer data: out, gposb
    and gbias equal reduce64 / bias64 exactly; the twins are the fp32 result rounded once to
    nearest even (totals of 257, 259, -257 included); both bindings give the same fp32 bits;
    the step tag stays [5, 0].  bchunks cycles through 1, 2, 4, 7 with the splits, and a launch
    without a bias part runs too."""
    bchunks = ALL_BCHUNKS[(ALL_SPLITS.index(splits) + list(SHAPES).index(shape)) % 4]
    c = Case(shape, splits, bchunks, "int", 1000 + splits)
    sf = _tag()
    ctx = (shape, splits, bchunks)
    plain = launch_single(c, "wgrad_reduce", sf=sf)
    check_exact(c, plain, ctx)
    full = launch_single(c, "wgrad_reduce_w", TWINS, sf=sf)
    check_exact(c, full, ctx)
    assert set(full) == set(c.names(twins=True))
    assert _same_outputs(plain, full, OUTS), ctx
    one = launch_single(c, "wgrad_reduce_w", ("gposb16",), sf=sf)
    check_exact(c, one, ctx)
    none = launch_single(c, "wgrad_reduce_w", (), sf=sf)
    assert _same_outputs(plain, none, OUTS) and _same_outputs(plain, one, OUTS), ctx
    assert sf.tolist() == [5, 0], ctx
    # no bias part: only out is written (with and without its twin)
    c.bchunks, c._ref64 = 0, None
    got = launch_single(c, "wgrad_reduce_w", ("out16",), sf=sf)
    check_exact(c, got, ctx)
    assert same_bits(got["out"], plain["out"]) and sf.tolist() == [5, 0]


def test_reduce_past_the_block_cap():
    """M KP / 4 = 2 105 344 work items > 8192 blocks x 256: the main part's grid-stride loop
    takes a second pass.  Integer data, no bias part, exact."""
    shape = (256, 256, 32896, 257, 128, 128)
    assert shape[0] * shape[2] // 4 > 8192 * 256
    c = Case(shape, 2, 0, "int", 77)
    sf = _tag()
    got = launch_single(c, "wgrad_reduce", sf=sf)
    check_exact(c, got)
    assert sf.tolist() == [5, 0]


GAUSS_PAIRS = list(zip(GAUSS_SPLITS, GAUSS_BCHUNKS)) + list(zip(GAUSS_SPLITS, GAUSS_BCHUNKS[::-1]))


@pytest.mark.parametrize("shape", list(SHAPES))
def test_reduce_matches_documented_order(shape):
    """Gaussian data at splits in {5, 13} x bchunks in {4, 7}: out, gposb, gbias are bit-identical
    to slab_order32 / chunk_order32 / rows_order32 and within n_add 2^-24 sum|x| of float64
    (n_add = S + 2, chunks + 1, R + 2); wgrad_reduce_w gives the same bits and once-rounded
    twins.

    Measured on an MI355X, the largest error / bound per shape (REDUCE_ERR in the output):
    tiny out 0.19, gposb 0.34, gbias 0.009; first 0.30, 0.36, 0.010; hidden 0.30, 0.36, 0.010;
    wide 0.33, 0.36, 0.011 — a third of the bound at most, and far less for the 76- and 133-row
    sums, whose bound grows with R while the error of a sum of signed terms does not."""
    worst = {}
    for splits, bchunks in GAUSS_PAIRS:
        c = Case(shape, splits, bchunks, "gauss", 2000 + 10 * splits + bchunks)
        sf = _tag()
        ctx = (shape, splits, bchunks)
        plain = launch_single(c, "wgrad_reduce", sf=sf)
        w = check_order(c, plain, ctx)
        full = launch_single(c, "wgrad_reduce_w", TWINS, sf=sf)
        check_order(c, full, ctx)
        assert _same_outputs(plain, full, OUTS), ctx
        assert sf.tolist() == [5, 0], ctx
        for n, v in w.items():
            worst[n] = max(worst.get(n, 0.0), v)
            print(f"REDUCE_ERR kind={n} shape={shape} splits={splits} bchunks={bchunks} "
                  f"err_over_bound={v:.4f}")
    print(f"REDUCE_ERR worst shape={shape} " + " ".join(f"{n}={v:.4f}" for n, v in worst.items()))


# ------------------------------------------------------------------------------ multi
# four rows of different shapes and splits; the row with the largest grid (wide: 1193 blocks)
# is neither first nor last, so the shorter rows' surplus blocks must return early
MIXED = [("first", 5, 4), ("wide", 13, 7), ("tiny", 13, 4), ("hidden", 5, 7)]


@pytest.fixture(scope="module")
def mixed_cases():
    return [Case(s, sp, bc, "gauss", 3000 + i) for i, (s, sp, bc) in enumerate(MIXED)]


def _grid_x(c: Case):
    M, KP = c.shape[0], c.shape[2]
    return min((M * (KP // 4) + 255) // 256, 8192) + (NPTS * M + 255) // 256 + M


@pytest.mark.parametrize("cols", [13, 16])
def test_reduce_multi_mixed_shapes(mixed_cases, cols):
    """One wgrad_reduce_multi launch (13 columns) / wgrad_reduce_multi_w launch (16 columns,
    twins for rows 0 and 2 — all three, and gbias16 alone — and none for rows 1 and 3) over
    four rows of different shapes: each row equals its own single-layer launch bit for bit and
    the documented order, and is within the bound of float64.

    Measured on an MI355X, error / bound at most: out 0.32, gposb 0.35, gbias 0.007."""
    grids = [_grid_x(c) for c in mixed_cases]
    assert grids.index(max(grids)) not in (0, len(grids) - 1) and len(set(grids)) == 4
    twins_of = [TWINS, (), ("gbias16",), ()] if cols == 16 else None
    got = launch_multi(mixed_cases, cols, twins_of)
    for i, (c, g) in enumerate(zip(mixed_cases, got)):
        w = check_order(c, g, ("row", i))
        single = launch_single(c, "wgrad_reduce")
        assert _same_outputs(single, g, OUTS), i
        if cols == 16:
            assert set(g) == set(OUTS) | set(twins_of[i]), i
        print(f"REDUCE_ERR multi cols={cols} row={i} "
              + " ".join(f"{n}={v:.4f}" for n, v in w.items()))


@pytest.mark.parametrize("kind", ["int", "gauss"])
def test_reduce_multi_sixteen_rows(kind):
    """nl = 16, the most one launch holds: sixteen tiny layers with their own data, splits and
    chunk counts; every row against its oracle."""
    cases = [Case("tiny", ALL_SPLITS[i % 6] if kind == "int" else GAUSS_SPLITS[i % 2],
                  ALL_BCHUNKS[i % 4] if kind == "int" else GAUSS_BCHUNKS[(i // 2) % 2], kind,
                  4000 + i) for i in range(16)]
    got = launch_multi(cases, 16, [TWINS if i % 3 else () for i in range(16)])
    for i, (c, g) in enumerate(zip(cases, got)):
        (check_exact if kind == "int" else check_order)(c, g, ("row", i))


# --------------------------------------------------------------------------- step tag
BOUND = 2.0 ** 120
BELOW = float(np.nextafter(np.float32(BOUND), np.float32(0)))
TAG_SPLITS, TAG_BCHUNKS = 5, 4
# (where, entries to set: (chunk or slab index, value)..., tags?)
TAG_VALUES = [
    ("2^120", [(0, BOUND)], True),
    ("-2^120", [(3, -BOUND)], True),
    ("below 2^120", [(2, BELOW)], False),
    ("-below 2^120", [(4 % TAG_BCHUNKS, -BELOW)], False),
    ("2^119 + 2^119", [(0, BOUND / 2), (3, BOUND / 2)], True),
    ("2^119 alone", [(1, BOUND / 2)], False),
    ("nan", [(2, NAN)], True),
    ("-inf", [(1, float("-inf"))], True),
    ("+inf", [(0, float("inf"))], True),
]


def _tag_case(which, entries):
    """The tiny shape, all zeros (+ NaN rows, padding) but for `entries` at one summed
    element of `which` in {'out', 'gposb', 'gbias'}."""
    c = Case("tiny", TAG_SPLITS, TAG_BCHUNKS, "int", 1)
    M, Mpad, KP, taps, cin, cinp = c.shape
    live = c.slab[:, :M, :taps * cinp].reshape(TAG_SPLITS, M, taps, cinp)
    live[..., :cin] = 0
    c.bpart.zero_()
    part = c.bpart[:TAG_BCHUNKS * NPTS * M].reshape(TAG_BCHUNKS, NPTS, M)
    rows = c.bpart[TAG_BCHUNKS * NPTS * M:].reshape(TAG_BCHUNKS, BOARD, M)
    for z, v in entries:
        if which == "out":
            c.slab[z, 3, 4 * cinp + 2] = v          # co 3, tap 4, ci 2
        elif which == "gposb":
            part[z, 200, 5] = v
        else:
            rows[z, (7 * z + 3) % BOARD, 6] = v     # (different rows, different lane partials)
    c.slab_d, c.bpart_d = c.slab.to(DEV), c.bpart.to(DEV)
    return c


@pytest.mark.parametrize("which", OUTS)
def test_reduce_step_tag(which):
    """Each of the reduce's three range checks alone (weight sum, position-bias sum,
    channel-bias sum), both single-layer bindings: a total of exactly +-2^120 tags the step
    (sf[1] = sf[0] + 1), the largest float below does not, two addends of 2^119 in different
    slabs / chunks do although every input is in range, NaN and +-inf do; a clean launch and
    the NaN rows co >= M do not; with sf null the launch runs and writes the same outputs."""
    idx = {"out": (3 * 9 + 4) * 5 + 2, "gposb": 200 * 8 + 5, "gbias": 6}[which]
    for name, entries, tags in TAG_VALUES:
        c = _tag_case(which, entries)
        assert torch.isnan(c.slab[:, c.shape[0]:, :]).all()
        want = sum(np.float32(v) for _, v in entries)       # exact: powers of two
        for api in ("wgrad_reduce", "wgrad_reduce_w"):
            sf = _tag()
            got = launch_single(c, api, TWINS if api.endswith("_w") else (), sf=sf)
            assert sf.tolist() == ([5, 6] if tags else [5, 0]), (which, name, api)
            v = got[which][idx].item()
            assert (np.isnan(v) and np.isnan(want)) or v == want, (which, name, api, v)
            for n in OUTS:      # everything else is a sum of zeros
                rest = got[n].clone()
                if n == which:
                    rest[idx] = 0
                assert (rest == 0).all(), (which, name, api, n)
            nosf = launch_single(c, api, TWINS if api.endswith("_w") else (), sf=None)
            assert _same_outputs(got, nosf, got.keys()), (which, name, api)
    # a tag already set is left alone by a clean launch (the kernel only ever sets it)
    c = _tag_case(which, [])
    sf = _tag()
    launch_single(c, "wgrad_reduce", sf=sf)
    assert sf.tolist() == [5, 0]


# ========================================================= B: grad_update's deferred path
GAP = 16
GAP_VALUE = 3.0
LR0, DECAY, STEP0 = 2.0 ** -6, 2.0 ** -10, 5
PLAIN_N = 37
# row: (cout, cin, cinp, taps, KP, Mpad, splits, bchunks)
GU_ROWS = [(128, 128, 128, 9, 1152, 128, 5, 4),     # the 4-wide path (slab_sums4)
           (8, 6, 8, 9, 128, 128, 13, 7)]           # per element (slab_sum1), one channel block


class GULayout:
    """Flat P / G of two conv layers + a plain range, every region at a multiple of 4 with a
    GAP-element sentinel run before, between and after."""

    def __init__(self):
        self.off = {}
        o = GAP
        for r, (cout, cin, _, taps, *_rest) in enumerate(GU_ROWS):
            for name, n in (("w", cout * taps * cin), ("b", cout), ("pos", NPTS * cout)):
                assert o % 4 == 0
                self.off[(r, name)] = (o, n)
                o += (n + 3) // 4 * 4 + GAP
        self.off["plain"] = (o, PLAIN_N)
        self.numel = o + (PLAIN_N + 3) // 4 * 4 + GAP

    def region(self, flat, key):
        o, n = self.off[key]
        return flat[o:o + n]

    def gap_mask(self):
        m = torch.ones(self.numel, dtype=torch.bool)
        for o, n in self.off.values():
            m[o:o + n] = False
        return m


def _gu_cases(kind):
    return [Case((cout, Mpad, KP, taps, cin, cinp), splits, bchunks, kind, 5000 + 10 * r)
            for r, (cout, cin, cinp, taps, KP, Mpad, splits, bchunks) in enumerate(GU_ROWS)]


def _gu_params(lay: GULayout, kind):
    """P: multiples of 2^-6 (integer data: p - lr g is then exact) or Gaussian; G: NaN where
    the launch must write, values in the plain range, sentinels in the gaps."""
    gen = torch.Generator().manual_seed(99)
    P = torch.full((lay.numel,), GAP_VALUE)
    G = torch.full((lay.numel,), GAP_VALUE)
    for key, (o, n) in lay.off.items():
        if kind == "int":
            P[o:o + n] = torch.randint(-2 ** 12, 2 ** 12 + 1, (n,), generator=gen).float() / 64
        else:
            P[o:o + n] = torch.randn(n, generator=gen)
        G[o:o + n] = NAN
    o, n = lay.off["plain"]
    G[o:o + n] = (torch.randint(-300, 301, (n,), generator=gen).float() if kind == "int"
                  else torch.randn(n, generator=gen))
    return P, G


def run_grad_update(cases, lay, P0, G0, gate=None, flag=0):
    """One final SGD grad_update launch (write_grads = 1) over the two deferred rows and the
    plain range.  Returns the device state on the CPU."""
    h = _h()
    pbuf, P = guarded(P0)
    gbuf, G = guarded(G0)
    pbias_buf, pbias = guarded(torch.full((NPTS * GU_ROWS[0][0],), NAN, dtype=torch.bfloat16))
    lr = torch.tensor([LR0], dtype=torch.float64, device=DEV)
    step = torch.tensor([STEP0], dtype=torch.int64, device=DEV)
    gflag = torch.tensor([flag], dtype=torch.int64, device=DEV)
    tickets = torch.zeros(h.grad_update_tickets(), dtype=torch.int32, device=DEV)
    bad = torch.zeros(1, dtype=torch.int32, device=DEV)
    gt = None if gate is None else torch.tensor([gate], dtype=torch.float32, device=DEV)
    rows = []
    for r, (c, (cout, cin, cinp, taps, KP, Mpad, splits, bchunks)) in enumerate(
            zip(cases, GU_ROWS)):
        w_off, b_off, pos_off = (lay.off[(r, k)][0] for k in ("w", "b", "pos"))
        at = lambda off: P.data_ptr() + 4 * off    # noqa: E731
        row = [0] * 29
        row[0], row[3], row[4], row[5], row[6], row[7] = at(w_off), cout, cin, taps, cinp, KP
        row[13], row[14] = at(b_off), at(pos_off)
        row[15] = pbias.data_ptr() if r == 0 else 0
        row[20:29] = [c.slab_d.data_ptr(), c.bpart_d.data_ptr(), splits, Mpad, KP, bchunks,
                      w_off, b_off, pos_off]
        rows.append(row)
    tab = np.ascontiguousarray(np.array(rows, dtype=np.int64))
    assert tab.shape[1] == h.grad_update_cols()
    h.grad_update(tab.ctypes.data, len(rows), lay.off["plain"][0], PLAIN_N, P.data_ptr(),
                  G.data_ptr(), 0, 0, 0.0, 1.0, gt.data_ptr() if gt is not None else 0,
                  lr.data_ptr(), DECAY, step.data_ptr(), tickets.data_ptr(), bad.data_ptr(), 1, 1,
                  gflag.data_ptr(), _s())
    torch.cuda.synchronize()
    assert guards_intact(pbuf) and guards_intact(gbuf) and guards_intact(pbias_buf)
    return dict(P=P.cpu(), G=G.cpu(), pbias=pbias.cpu(), lr=lr.item(), step=int(step.item()),
                bad=int(bad.item()), tickets=tickets.cpu(), flag=int(gflag.item()))


def _gu_regions(lay, flat, r):
    return {"out": lay.region(flat, (r, "w")), "gposb": lay.region(flat, (r, "pos")),
            "gbias": lay.region(flat, (r, "b"))}


def _gu_common(lay, st, P0, G0):
    """What holds after every launch: gaps untouched, tickets zero, lr decayed, step + 1."""
    m = lay.gap_mask()
    assert same_bits(st["P"][m], P0[m]) and same_bits(st["G"][m], G0[m])
    assert same_bits(lay.region(st["G"], "plain"), lay.region(G0, "plain"))
    assert int(st["tickets"].abs().sum()) == 0
    assert st["lr"] == LR0 * (1.0 - DECAY) and st["step"] == STEP0 + 1


def test_grad_update_deferred_exact_on_integer_data():
    """Integer slabs and partials, P on a 2^-6 grid, SGD with lr = 2^-6: the G regions equal
    reduce64 / bias64 exactly (the per-channel bias gradient included), P = p - lr g exactly,
    row 0's pbias[p][c] = bf16(b_new[c] + posb_new[p][c]) bit for bit; gaps, guards, tickets,
    lr, step and bad_steps as they should be."""
    lay, cases = GULayout(), _gu_cases("int")
    P0, G0 = _gu_params(lay, "int")
    st = run_grad_update(cases, lay, P0, G0, gate=1.0)
    _gu_common(lay, st, P0, G0)
    assert st["bad"] == 0 and st["flag"] == 0
    g64 = torch.zeros(lay.numel, dtype=torch.float64)
    for r, c in enumerate(cases):
        got = _gu_regions(lay, st["G"], r)
        check_exact(c, got, ("row", r))
        for n, v in c.ref64().items():
            _gu_regions(lay, g64, r)[n].copy_(v)
    lay.region(g64, "plain").copy_(lay.region(G0, "plain").double())
    # p - lr g is exact in fp32 for this data: the product and the difference are multiples of
    # 2^-6 below 2^24 x 2^-6 (asserted, not assumed)
    live = ~lay.gap_mask()
    want = P0.double() - LR0 * g64
    assert (want[live].abs() < 2.0 ** 18).all() and torch.equal(want * 64, (want * 64).round())
    assert torch.equal(want.float().double(), want)
    assert same_bits(st["P"][live], want.float()[live])
    assert not torch.equal(st["P"][live], P0[live])
    b_new = lay.region(st["P"], (0, "b"))
    pos_new = lay.region(st["P"], (0, "pos")).reshape(NPTS, -1)
    exp = (b_new.reshape(1, -1) + pos_new)                 # exact: multiples of 2^-6 below 2^13
    assert torch.equal(exp.double(), b_new.double().reshape(1, -1) + pos_new.double())
    assert same_bits(st["pbias"], exp.to(torch.bfloat16))


def test_grad_update_deferred_matches_reduce_and_documented_order():
    """Gaussian data at shapes the model never builds (cin % 4 != 0, 7 chunks, 13 splits): the
    gradient grad_update writes is bit-identical to what wgrad_reduce_multi writes from the
    same slabs and partials — the promise of dg_common.h across its two homes — and to the
    emulations of the documented orders; within the bound of float64.

    Measured on an MI355X, error / bound: row 0 out 0.31, gposb 0.34, gbias 0.007; row 1 0.08,
    0.24, 0.002."""
    lay, cases = GULayout(), _gu_cases("gauss")
    P0, G0 = _gu_params(lay, "gauss")
    st = run_grad_update(cases, lay, P0, G0)
    _gu_common(lay, st, P0, G0)
    assert st["bad"] == 0
    other = launch_multi(cases, 13)
    for r, c in enumerate(cases):
        got = _gu_regions(lay, st["G"], r)
        w = check_order(c, got, ("row", r))
        assert _same_outputs(got, other[r], OUTS), r
        print(f"REDUCE_ERR grad_update row={r} " + " ".join(f"{n}={v:.4f}" for n, v in w.items()))
    live = ~lay.gap_mask()
    assert not torch.isnan(st["P"]).any() and not torch.equal(st["P"][live], P0[live])


@pytest.mark.parametrize("how", ["gate closed", "tagged"])
def test_grad_update_deferred_skips_the_whole_step(how):
    """gate = 0, or the producers' tag equal to step + 1: P keeps its bits, the gradient is
    still written (exactly), the lr still decays; a tagged step counts in bad_steps, a closed
    gate does not (the gate kernel counted it)."""
    lay, cases = GULayout(), _gu_cases("int")
    P0, G0 = _gu_params(lay, "int")
    if how == "gate closed":
        st = run_grad_update(cases, lay, P0, G0, gate=0.0)
        assert st["bad"] == 0
    else:
        st = run_grad_update(cases, lay, P0, G0, gate=1.0, flag=STEP0 + 1)
        assert st["bad"] == 1 and st["flag"] == STEP0 + 1
    _gu_common(lay, st, P0, G0)
    assert same_bits(st["P"], P0)
    for r, c in enumerate(cases):
        check_exact(c, _gu_regions(lay, st["G"], r), (how, r))
