"""The tail of the optimizer step against independent references (GPU).

Part A drives the raw bindings — sgd / rmsprop (fp32 and bf16-wire gradients), the finite
gates, the fp8 casts and weight_refresh — and compares them with the plain-Python oracles of
tests/test_update_oracles_cpu.py.  Part B runs whole training steps through HipGoNet on both
update paths (the fused grad_update launch and the separate launches) and checks the new
parameters, the optimizer state and every operand copy against the same oracles, computed from
the gradient the step itself reports.

Device buffers are slices at 16-element offsets inside sentinel-filled allocations: at least
16-byte aligned for every dtype (uint8 included: the refresh writes e4m3 fragments with
16-byte stores), as the model's buffers are, and a write past either end shows in the sentinels.
"""
import numpy as np
import pytest
import torch

from test_update_oracles_cpu import (E4M3_TABLE, e4m3_bytes, gate_places, refresh_expected,
                                     rmsprop_ref, sgd_ref)

pytestmark = pytest.mark.gpu

DEV = "cuda"
GUARD = 16         # sentinel elements on either side of a buffer under test (>= 16 bytes)
BIG = 2097152      # 2048 blocks x 256 threads x 4: the sgd grid cap (x 8 / 1024: frame_to_fp8's)


def _h():
    from deep_go_amd.ops.native import hip
    return hip()


def _s():
    from deep_go_amd.ops.native import stream_handle
    return stream_handle()


def _sentinel(dtype):
    return 165 if dtype == torch.uint8 else 3


def guarded(x: torch.Tensor):
    """(whole allocation, view) with a copy of the 1-D CPU tensor x on the device between two
    GUARD-element sentinel runs."""
    n = x.numel()
    buf = torch.full((n + 2 * GUARD,), _sentinel(x.dtype), dtype=x.dtype, device=DEV)
    view = buf[GUARD:GUARD + n]
    view.copy_(x.reshape(-1))
    return buf, view


def guards_intact(buf: torch.Tensor) -> bool:
    g = torch.cat([buf[:GUARD], buf[-GUARD:]]).cpu()
    return bool((g == _sentinel(buf.dtype)).all())


def bits(t: torch.Tensor) -> torch.Tensor:
    """The raw bits of t (CPU, flat) for bit-exact comparison (-0 != 0)."""
    t = t.detach().cpu().contiguous().reshape(-1)
    ints = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}
    return t.view(ints[t.element_size()])


def same_bits(a, b) -> bool:
    a, b = bits(a), bits(b)
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a, b)


# =============================================================== A1 / A2 / A3: optimizers
SIZES = [1, 3, 4, 5, 1001, BIG + 1203]   # the last: past the 2048-block cap, 3-element tail
GSCALES = [1.0, 0.37]
GATES = [None, 1.0, 0.0]
LR = 0.0137


def _grad(n, kind, gen, scale=2.0):
    g = torch.randn(n, generator=gen) * scale
    return g.to(torch.bfloat16) if kind == "bf16" else g


def sgd_bound(ref, g, lr, gscale):
    """One rounding each for the product and the difference, doubled."""
    l = float(np.float32(lr) * np.float32(gscale))
    return 2.0 ** -23 * (ref.abs() + (l * g.double()).abs())


def rmsprop_check(p0, ms0, p1, ms1, g, lr, decay, gscale):
    """A2's bounds (d = p0 - p1).  Returns the three largest observed figures: ms's relative
    error in units of 2^-24 (bound 8); |d_got - d_ref| / bound; and the update's error in
    units of 2^-24 |d_ref| over the elements with |p| <= |d_ref|, where the final rounding of
    p adds at most one such unit (bound 16 + 1) — the figure that rsqrtf's error shows in."""
    pr, mr = rmsprop_ref(p0, g, ms0, lr, decay, gscale)
    u = 2.0 ** -24
    rel_ms = ((ms1.double() - mr).abs() / mr).max().item()
    assert rel_ms <= 8 * u, f"ms relative error {rel_ms / u:.2f} x 2^-24"
    d_ref = p0.double() - pr
    d_got = p0.double() - p1.double()
    bound = 16 * u * d_ref.abs() + u * pr.abs()
    err = (d_got - d_ref).abs()
    ratio = (err / bound.clamp_min(1e-300)).max().item()
    assert (err <= bound).all(), f"update error / bound = {ratio:.3f}"
    sel = (d_ref != 0) & (pr.abs() <= d_ref.abs())
    upd = (err[sel] / (u * d_ref.abs()[sel])).max().item() if sel.any() else 0.0
    return np.array([rel_ms / u, ratio, upd])


def _fmt_err(w):
    return (f"ms_err={w[0]:.2f}x2^-24 update_err_over_bound={w[1]:.3f} "
            f"update_err={w[2]:.2f}x2^-24|d|")


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("kind", ["fp32", "bf16"])
def test_sgd_matches_float64_reference(kind, n):
    """sgd / sgd_bf16 against sgd_ref: |got - ref| <= 2^-23 (|ref| + |l g|) for every gscale
    and gate; gate = 0 leaves the parameters bit-identical, also under an all-NaN gradient."""
    h, gen = _h(), torch.Generator().manual_seed(100 + n % 1000)
    fn = h.sgd_bf16 if kind == "bf16" else h.sgd
    p0 = torch.randn(n, generator=gen)
    g = _grad(n, kind, gen)
    gbuf, gd = guarded(g)
    nanbuf, nand = guarded(torch.full_like(g, float("nan")))
    lrt = torch.tensor([LR], dtype=torch.float64, device=DEV)
    for gscale in GSCALES:
        for gate in GATES:
            pbuf, pd = guarded(p0)
            gt = None if gate is None else torch.tensor([gate], device=DEV)
            fn(pd.data_ptr(), gd.data_ptr(), n, lrt.data_ptr(), gscale,
               gt.data_ptr() if gt is not None else 0, _s())
            torch.cuda.synchronize()
            got = pd.cpu()
            assert guards_intact(pbuf) and guards_intact(gbuf), (gscale, gate)
            if gate == 0.0:
                assert same_bits(got, p0), (gscale, gate)
                continue
            ref = sgd_ref(p0, g.float(), LR, gscale)
            err = (got.double() - ref).abs()
            bound = sgd_bound(ref, g.float(), LR, gscale)
            assert (err <= bound).all(), (gscale, gate, (err / bound).max().item())
            assert not torch.equal(got, p0)
    assert lrt.item() == LR
    pbuf, pd = guarded(p0)
    gt = torch.zeros(1, device=DEV)
    fn(pd.data_ptr(), nand.data_ptr(), n, lrt.data_ptr(), 1.0, gt.data_ptr(), _s())
    torch.cuda.synchronize()
    assert same_bits(pd, p0) and guards_intact(pbuf)


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("kind", ["fp32", "bf16"])
def test_rmsprop_matches_float64_reference(kind, n):
    """rmsprop / rmsprop_bf16 against rmsprop_ref over two consecutive steps (the second reads
    the mean square the first wrote; each is compared from the state it started from):
    ms to 8 x 2^-24 relative, the update d = p0 - p1 to 16 x 2^-24 |d_ref| + 2^-24 |p| (about
    6 fp32 roundings, half of ms's error, rsqrtf at its documented 1 ulp).  gate = 0 leaves p
    and ms bit-identical.

    Measured on an MI355X (the largest figures, at n = 2 098 355): ms is off by at most
    3.6 x 2^-24 relative (bound 8); the update, where the final rounding of p is negligible, by
    3.3 x 2^-24 |d| for fp32 gradients and 2.8 for bf16 (bound 16) — rsqrtf and the roundings
    around it together use a fifth of the budget; |d_got - d_ref| / bound peaks at 0.998, which
    is the 2^-24 |p| term alone: an element whose update is far below its half ulp."""
    h, gen = _h(), torch.Generator().manual_seed(200 + n % 1000)
    fn = h.rmsprop_bf16 if kind == "bf16" else h.rmsprop
    decay = 0.9
    p_init = torch.randn(n, generator=gen)
    ms_init = torch.rand(n, generator=gen) * (2.0 - 1e-3) + 1e-3
    grads = [_grad(n, kind, gen), _grad(n, kind, gen, 0.3)]
    gdev = [guarded(g) for g in grads]
    lrt = torch.tensor([LR], dtype=torch.float64, device=DEV)
    worst = np.zeros(3)
    for gscale in GSCALES:
        for gate in GATES:
            pbuf, pd = guarded(p_init)
            mbuf, md = guarded(ms_init)
            gt = None if gate is None else torch.tensor([gate], device=DEV)
            for g, (gbuf, gd) in zip(grads, gdev):
                p0, ms0 = pd.cpu(), md.cpu()
                fn(pd.data_ptr(), gd.data_ptr(), md.data_ptr(), n, lrt.data_ptr(), decay, gscale,
                   gt.data_ptr() if gt is not None else 0, _s())
                torch.cuda.synchronize()
                p1, ms1 = pd.cpu(), md.cpu()
                assert guards_intact(pbuf) and guards_intact(mbuf) and guards_intact(gbuf)
                if gate == 0.0:
                    assert same_bits(p1, p0) and same_bits(ms1, ms0), (gscale, gate)
                    continue
                worst = np.maximum(worst, rmsprop_check(p0, ms0, p1, ms1, g.float(), LR, decay,
                                                        gscale))
                assert not torch.equal(p1, p0)
    print(f"RMSPROP_ERR kind={kind} n={n} " + _fmt_err(worst))


def test_rmsprop_zero_gradient_horizon():
    """1200 zero-gradient launches from ms = 1: the parameters stay bit-identical and ms stays
    finite.  (With fp32 denormals the mean square settles at 4 denormal units, 5.6e-45, and
    the update is 0 x finite = 0; a device that flushed them would reach ms = 0 and
    0 x rsqrt(0) = NaN.)  Measured on an MI355X: ms settles at 5.6e-45, no NaN."""
    h = _h()
    p0 = torch.randn(64, generator=torch.Generator().manual_seed(3))
    pbuf, pd = guarded(p0)
    mbuf, md = guarded(torch.ones(64))
    gbuf, gd = guarded(torch.zeros(64))
    lrt = torch.tensor([LR], dtype=torch.float64, device=DEV)
    s = _s()
    for _ in range(1200):
        h.rmsprop(pd.data_ptr(), gd.data_ptr(), md.data_ptr(), 64, lrt.data_ptr(), 0.9, 1.0, 0, s)
    torch.cuda.synchronize()
    ms = md.cpu()
    print(f"ZERO_GRAD_HORIZON ms min={ms.min().item():.3e} max={ms.max().item():.3e}")
    assert torch.isfinite(ms).all() and not torch.isnan(pd).any()
    assert same_bits(pd, p0)
    assert guards_intact(pbuf) and guards_intact(mbuf)


# ======================================================================= A4: finite gates
LOSS_LENS = [1, 256, 300]
# 0: no gradient; 5: one vector + a 1-element tail; 4*2048*3 - 5: 3 blocks, some lanes only in
# the remainder loop, 3-element tail; 2 200 003: past finite_gate1's 256-block cap (unrolled
# loop + remainder loop + tail all run) and finite_gate's 1024-block cap
GRAD_LENS = [0, 5, 4 * 2048 * 3 - 5, 2200003]
GATE_APIS = ["finite_gate", "finite_gate_bf16", "finite_gate1", "finite_gate1_bf16"]
FLT_MAX = 3.4028234663852886e38
BF16_NONFINITE = [0x7FC0, 0x7F80, 0xFF80]     # NaN, +inf, -inf
BF16_LARGEST = [0x7F7F, 0xFF7F]               # +- the largest finite bf16


class _Gate:
    """One gate API on fixed buffers; check() launches once and compares gate, bad_count and
    the ticket word with the torch.isfinite oracle."""

    def __init__(self, api, ng):
        self.h, self.api, self.ng = _h(), api, ng
        self.bf16 = api.endswith("bf16")
        self.one = api.startswith("finite_gate1")
        gen = torch.Generator().manual_seed(ng % 977)
        self.gbuf = self.g = None
        if ng:
            g = torch.randn(ng, generator=gen)
            self.gbuf, self.g = guarded(g.to(torch.bfloat16) if self.bf16 else g)
        self.gate = torch.zeros(1, device=DEV)
        self.bad = torch.zeros(1, dtype=torch.int32, device=DEV)
        self.ticket = torch.zeros(1, dtype=torch.int32, device=DEV)
        self.loss = None

    def set_loss(self, nl):
        self.loss = None
        if nl:
            gen = torch.Generator().manual_seed(nl)
            self.lbuf, self.loss = guarded(torch.rand(nl, generator=gen) * 6)

    def poke(self, idx, value):
        """Write a value (fp32) or raw bf16 bits at gradient element(s) idx."""
        if self.bf16:
            v = value if value < 0x8000 else value - 0x10000
            self.g.view(torch.int16)[idx] = v
        else:
            self.g[idx] = value

    def launch(self):
        h, s = self.h, _s()
        lp = self.loss.data_ptr() if self.loss is not None else 0
        nl = self.loss.numel() if self.loss is not None else 0
        gp = self.g.data_ptr() if self.g is not None else 0
        a = (self.gate.data_ptr(), self.bad.data_ptr())
        if self.api == "finite_gate":
            h.finite_gate(lp, nl, gp, self.ng, *a, s)
        elif self.api == "finite_gate_bf16":
            h.finite_gate_bf16(lp, nl, gp, self.ng, *a, s)
        elif self.api == "finite_gate1":
            h.finite_gate1(lp, nl, gp, 0, self.ng, *a, self.ticket.data_ptr(), s)
        else:
            h.finite_gate1(lp, nl, 0, gp, self.ng, *a, self.ticket.data_ptr(), s)

    def oracle(self) -> bool:
        ok = True
        if self.loss is not None:
            ok = ok and bool(torch.isfinite(self.loss).all())
        if self.g is not None:
            ok = ok and bool(torch.isfinite(self.g).all())
        return ok

    def check(self, want_ok: bool, what=""):
        assert self.oracle() == want_ok, f"test set-up: {what}"
        self.gate.fill_(0.5)
        b0 = int(self.bad.item())
        self.launch()
        torch.cuda.synchronize()
        ctx = (self.api, self.ng, what)
        assert self.gate.item() == (1.0 if want_ok else 0.0), ctx
        assert int(self.bad.item()) == b0 + (0 if want_ok else 1), ctx
        if self.one:
            assert int(self.ticket.item()) == 0, ctx


# (without a gradient the bf16 twins launch exactly what the fp32 entry points launch)
@pytest.mark.parametrize("api,ng", [(a, n) for a in GATE_APIS for n in GRAD_LENS
                                    if n or not a.endswith("bf16")])
def test_finite_gates_match_isfinite(api, ng):
    """finite_gate, finite_gate_bf16 and finite_gate1 (fp32 and grads16) against
    torch.isfinite(loss).all() and torch.isfinite(g).all(): one NaN / +inf / -inf at the first
    and last index, in the n % 4 tail, in the last block's share and where only the remainder
    loop reads; in the loss only, the gradient only, both.  The largest finite values and
    denormals do not trip.  bad_count rises by exactly 1 per bad launch and finite_gate1's
    ticket word is 0 after every launch."""
    G = _Gate(api, ng)
    places = gate_places(ng) if ng else {}
    nonfinite = BF16_NONFINITE if G.bf16 else [float("nan"), float("inf"), float("-inf")]
    for nl in LOSS_LENS + ([0] if ng else []):
        G.set_loss(nl)
        G.check(True, f"clean nl={nl}")
        # ---- must not trip: the largest finite values, a denormal
        if ng:
            keep = G.g.clone()
            idx = sorted(set(places.values()))
            big = BF16_LARGEST if G.bf16 else [FLT_MAX, -FLT_MAX]
            for k, i in enumerate(idx):
                G.poke(i, big[k % 2])
            if not G.bf16:
                G.poke(idx[0], 1e-45)
        if nl:
            lkeep = G.loss.clone()
            G.loss[nl - 1] = FLT_MAX
            G.loss[0] = 1e-45
        G.check(True, f"largest finite nl={nl}")
        if ng:
            G.g.copy_(keep)
        if nl:
            G.loss.copy_(lkeep)
        # ---- the gradient only
        for v in nonfinite:
            for name, i in places.items():
                old = G.g[i].clone()
                G.poke(i, v)
                G.check(False, f"grad[{name}={i}]={v} nl={nl}")
                G.g[i] = old
        # ---- the loss only (the last index is past the block's 256 lanes at nl = 300)
        if nl:
            for v in (float("nan"), float("inf"), float("-inf")):
                for i in sorted({0, nl // 2, nl - 1}):
                    old = G.loss[i].clone()
                    G.loss[i] = v
                    G.check(False, f"loss[{i}]={v} nl={nl}")
                    G.loss[i] = old
        # ---- both, and bad values in many blocks: still one count
        if ng and nl:
            keep = G.g.clone()
            G.loss[nl - 1] = float("nan")
            G.poke(places["last"], nonfinite[1])
            G.check(False, f"loss and gradient nl={nl}")
            G.loss.copy_(lkeep)
            G.g.copy_(keep)
        if ng:
            keep = G.g.clone()
            for i in set(places.values()):
                G.poke(i, nonfinite[0])
            many = torch.arange(0, ng, max(1, ng // 997), device=DEV)
            G.poke(many, nonfinite[2])
            G.check(False, f"many bad values nl={nl}")
            G.g.copy_(keep)
        G.check(True, f"clean again nl={nl}")
    # ---- bad, good, bad on the same buffers: gate 0, 1, 0 and two counts
    G.set_loss(300)
    b0 = int(G.bad.item())
    for want_ok in (False, True, False):
        if ng:
            i = places["last"]
            old = G.g[i].clone()
            if not want_ok:
                G.poke(i, nonfinite[0])
            G.check(want_ok, "bad, good, bad")
            G.g[i] = old
        else:
            G.loss[299] = 1.0 if want_ok else float("inf")
            G.check(want_ok, "bad, good, bad")
    assert int(G.bad.item()) == b0 + 2
    assert guards_intact(G.lbuf) and (G.gbuf is None or guards_intact(G.gbuf))


# ========================================================================= A5: frame_to_fp8
# the non-negative part of the e4m3 table, the most telling values first (n = 8 takes 8)
_TABLE_POS = [448.0, 464.0, 2.0 ** -9, 2.0 ** -10, 3 * 2.0 ** -10, 17.0, 19.0, 0.0, 500.0, 21.0,
              23.0]
assert set(_TABLE_POS) == {v for v, _ in E4M3_TABLE if v >= 0}


@pytest.mark.parametrize("s", [2.0 ** -3, 1.0, 2.0 ** 4, 0.0123])
@pytest.mark.parametrize("n", [8, BIG + 24])
def test_frame_to_fp8_bytes_and_amax(n, s):
    """frame_to_fp8 (non-negative bf16 frame, n % 8 == 0): bytes equal e4m3_bytes exactly — at
    power-of-two scales and at s = 0.0123 (both sides are IEEE fp32: 1 / s, the product, the
    round-to-nearest-even cast) — and amax is the input's max bit for bit."""
    h, gen = _h(), torch.Generator().manual_seed(n % 1000)
    tab = torch.tensor(_TABLE_POS, dtype=torch.float32) * s
    x = torch.rand(n, generator=gen) * (3 * 448.0 * s)
    if n == 8:
        x = tab[:8].clone()
    else:
        x[:len(tab)] = tab
        x[n - 16:n - 16 + len(tab)] = tab      # in the grid-stride pass past the block cap
    x = x.to(torch.bfloat16)
    assert (x.float() >= 0).all()
    want = e4m3_bytes(x.float(), s)
    if s in (2.0 ** -3, 1.0, 2.0 ** 4):        # the table arrives exactly: the known bytes
        tb = {v: b for v, b in E4M3_TABLE if b < 0x80}
        assert want[:8].tolist() == [tb[v] for v in _TABLE_POS[:8]]
    xbuf, xd = guarded(x)
    st = torch.tensor([s], dtype=torch.float32, device=DEV)
    xmax = x.float().max().reshape(1)
    for start in (0.0, None, 2.0 * xmax.item()):
        dbuf, dd = guarded(torch.zeros(n, dtype=torch.uint8))
        amax = None
        if start is not None:
            amax = torch.tensor([start], dtype=torch.float32, device=DEV).view(torch.int32)
        h.frame_to_fp8(xd.data_ptr(), dd.data_ptr(), n, st.data_ptr(),
                       amax.data_ptr() if amax is not None else 0, _s())
        torch.cuda.synchronize()
        got = dd.cpu()
        assert guards_intact(dbuf) and guards_intact(xbuf)
        bad = (got != want).nonzero().reshape(-1)
        assert bad.numel() == 0, (start, bad.numel(), [
            (int(i), x[i].item(), int(got[i]), int(want[i])) for i in bad[:8]])
        if start == 0.0:
            assert same_bits(amax.view(torch.float32), xmax)
        elif start is not None:
            assert amax.view(torch.float32).item() == np.float32(start)


# =========================================================================== A6: weight_fp8
def _fp8_weights(cout, taps, cin, s, gen):
    """Signed weights: +-448 s, values beyond it, the tie table, then uniform noise."""
    w = (torch.rand(cout * taps * cin, generator=gen) * 2 - 1) * (1.2 * 448.0 * s)
    tab = torch.tensor([v for v, _ in E4M3_TABLE], dtype=torch.float32)
    special = torch.cat([tab, -tab, torch.tensor([449.0, -449.0, 1e4, -1e4])]) * s
    assert special.numel() <= w.numel()
    w[:special.numel()] = special
    return w.reshape(cout, taps, cin)


def _refresh_row(w=0, wf=0, wd=0, cout=0, cin=0, taps=0, cinp=0, kpf=0, kpd=0, pbias_frag=0,
                 wf8=0, s_w=0, amax_w=0, bias=0, posb=0, pbias=0, wf_frag=0, wd_frag=0,
                 wf8_frag=0, wd8_frag=0):
    """One 20-word weight_refresh row in the column order documented above parse_refresh_row."""
    p = lambda t: t if isinstance(t, int) else t.data_ptr()   # noqa: E731
    return np.ascontiguousarray(np.array([[
        p(w), p(wf), p(wd), cout, cin, taps, cinp, kpf, kpd, p(pbias_frag), p(wf8), p(s_w),
        p(amax_w), p(bias), p(posb), p(pbias), p(wf_frag), p(wd_frag), p(wf8_frag),
        p(wd8_frag)]], dtype=np.int64))


@pytest.mark.parametrize("s", [2.0 ** -3, 0.0123])
@pytest.mark.parametrize("shape", [(5, 3, 9, 8, 80), (128, 128, 9, 128, 1152)])
def test_weight_fp8_bytes(shape, s):
    """weight_fp8: byte [co][t * cinp + ci] = e4m3_bytes(w[co][t][ci], s_w), padding columns
    stay 0 ((5, 3, 9, 8, 80): total % 4 != 0); the wf8 weight_refresh writes for the same
    weights and scale is identical."""
    cout, cin, taps, cinp, kp = shape
    h, gen = _h(), torch.Generator().manual_seed(cout)
    w = _fp8_weights(cout, taps, cin, s, gen)
    want = torch.zeros((cout, kp), dtype=torch.uint8)
    tmp = torch.zeros((cout, taps, cinp), dtype=torch.uint8)
    tmp[:, :, :cin] = e4m3_bytes(w, s)
    want[:, :taps * cinp] = tmp.reshape(cout, -1)
    if s == 2.0 ** -3:
        n = len(E4M3_TABLE)
        flat = e4m3_bytes(w, s).reshape(-1)
        assert flat[:n].tolist() == [b for _, b in E4M3_TABLE]
    wbuf, wdv = guarded(w.reshape(-1))
    st = torch.tensor([s], dtype=torch.float32, device=DEV)
    obuf, od = guarded(torch.zeros(cout * kp, dtype=torch.uint8))
    h.weight_fp8(wdv.data_ptr(), od.data_ptr(), cout, cin, taps, cinp, kp, st.data_ptr(), _s())
    torch.cuda.synchronize()
    assert guards_intact(obuf) and guards_intact(wbuf)
    got = od.cpu().reshape(cout, kp)
    bad = (got != want).nonzero()
    assert bad.numel() == 0, [(r.tolist(), int(got[tuple(r)]), int(want[tuple(r)]))
                              for r in bad[:8]]
    rbuf, rd = guarded(torch.zeros(cout * kp, dtype=torch.uint8))
    row = _refresh_row(w=wdv, cout=cout, cin=cin, taps=taps, cinp=cinp, kpf=kp, wf8=rd, s_w=st)
    h.weight_refresh(row.ctypes.data, 1, _s())
    torch.cuda.synchronize()
    assert guards_intact(rbuf) and guards_intact(wbuf)
    assert torch.equal(rd.cpu().reshape(cout, kp), want)


# ================================================================= A7: weight_refresh rows
AMAX_SENTINEL = 0x12345678
_COPY_DTYPES = {"wf": torch.bfloat16, "wd": torch.bfloat16, "wf_frag": torch.bfloat16,
                "wd_frag": torch.bfloat16, "wf8": torch.uint8, "wf8_frag": torch.uint8,
                "wd8_frag": torch.uint8, "pbias": torch.bfloat16, "pbias_frag": torch.bfloat16}


def _run_refresh(w, cinp, KP, Mpad, KPd, Mpad_d, copies, fp8, gen):
    """weight_refresh on one row writing `copies`; returns ({name: (alloc, view)}, expected,
    amax slots or None)."""
    h = _h()
    cout, k, _, cin = w.shape
    bias = torch.randn(cout, generator=gen)
    posb = torch.randn(361, cout, generator=gen)
    # fp8: the scale as a fraction of |w|max / 448 (below 1: the largest weights saturate)
    s = (w.abs().max() * fp8 / 448.0).to(torch.float32) if fp8 else None
    exp = refresh_expected(w, cinp, KP, Mpad, KPd, Mpad_d, s_w=s, bias=bias, posb=posb)
    src = {n: guarded(t.reshape(-1)) for n, t in (("w", w), ("bias", bias), ("posb", posb))}
    out = {n: guarded(torch.zeros(exp[n].numel(), dtype=_COPY_DTYPES[n])) for n in copies}
    kw = {n: v for n, (_, v) in out.items()}
    amax = None
    if fp8:
        st = s.reshape(1).to(DEV)
        amax = torch.full((512,), AMAX_SENTINEL, dtype=torch.int32, device=DEV)
        kw.update(s_w=st, amax_w=amax)
    if "pbias" in copies or "pbias_frag" in copies:
        kw.update(bias=src["bias"][1], posb=src["posb"][1])
    row = _refresh_row(w=src["w"][1], cout=cout, cin=cin, taps=k * k, cinp=cinp, kpf=KP, kpd=KPd,
                       **kw)
    h.weight_refresh(row.ctypes.data, 1, _s())
    torch.cuda.synchronize()
    for n, (buf, _) in {**src, **out}.items():
        assert guards_intact(buf), n
    return out, exp, amax


def _assert_copies(out, exp):
    for n, (_, view) in out.items():
        got, want = bits(view), bits(exp[n])
        assert got.shape == want.shape, n
        bad = (got != want).nonzero().reshape(-1)
        assert bad.numel() == 0, (n, bad.numel(), bad[:8].tolist())


@pytest.mark.parametrize("C", [128, 256])
def test_weight_refresh_square_fp8_row(C):
    """A 3x3 C -> C fp8 row with every copy: wf / wd (layouts.fwd_weight / dgrad_weight),
    wf_frag / wd_frag (frag_bf16; the 256-wide order), wf8 (e4m3_bytes), wf8_frag / wd8_frag
    (stack_frag_f8 of the bytes / of their transposed, tap-flipped dgrad operand), pbias,
    pbias_frag, and the |w| max slots (the grid's slots hold the max, the rest are untouched).
    The scale is half of |w|max / 448, so a good part of the weights lies beyond +-448 s and
    the clamps of the plain and of both fragment-ordered e4m3 copies all saturate."""
    gen = torch.Generator().manual_seed(C)
    w = torch.randn(C, 3, 3, C, generator=gen) * 0.05
    out, exp, amax = _run_refresh(w, C, 9 * C, C, 9 * C, C, list(_COPY_DTYPES), 0.5, gen)
    sat = (exp["wf8"] & 0x7F) == 0x7E
    assert 0.002 < sat.float().mean().item() < 0.5      # saturated, and not only saturated
    _assert_copies(out, exp)
    tiles = 9 * (C // 64) ** 2
    slots = amax.cpu()
    assert (slots[tiles:] == AMAX_SENTINEL).all()
    assert same_bits(slots[:tiles].view(torch.float32).max().reshape(1), exp["amax"].reshape(1))


@pytest.mark.parametrize("cout", [128, 256])
def test_weight_refresh_first_layer_row(cout):
    """The 5x5 first layer (38 channels in a 40-channel frame): wf, the linear-K fragment
    order (layouts.stack_frag_linear, K padded 1000 -> 1024 with zeros) and the bias tables."""
    gen = torch.Generator().manual_seed(cout + 1)
    w = torch.randn(cout, 5, 5, 38, generator=gen) * 0.1
    out, exp, _ = _run_refresh(w, 40, 1024, cout, 0, 0, ["wf", "wf_frag", "pbias", "pbias_frag"],
                               False, gen)
    _assert_copies(out, exp)


def test_weight_refresh_partial_tiles_row():
    """3x3, 24 -> 40 channels: both tile edges cut, plain wf / wd only; the padding of both
    operand matrices stays 0."""
    from deep_go_amd.ops import layouts as LY
    gen = torch.Generator().manual_seed(7)
    w = torch.randn(40, 3, 3, 24, generator=gen)
    KP, _, Mpad = LY.conv_dims(3, 24, 40, 64)
    KPd, _, Mpad_d = LY.conv_dims(3, 40, 24, 64)
    assert (KP, Mpad, KPd, Mpad_d) == (256, 64, 384, 64)
    out, exp, _ = _run_refresh(w, 24, KP, Mpad, KPd, Mpad_d, ["wf", "wd"], False, gen)
    _assert_copies(out, exp)


# ============================================================ B: one whole step, both paths
STEP_CONFIGS = {
    "4x128-bf16-sgd": dict(layers=4, ch=128, dtype="bf16", opt="sgd", wire="fp32"),
    "4x128-bf16-rmsprop": dict(layers=4, ch=128, dtype="bf16", opt="rmsprop", wire="fp32"),
    "3x64-bf16-sgd": dict(layers=3, ch=64, dtype="bf16", opt="sgd", wire="fp32"),
    "4x128-bf16wire-rmsprop": dict(layers=4, ch=128, dtype="bf16", opt="rmsprop", wire="bf16"),
    "5x128-fp8-sgd": dict(layers=5, ch=128, dtype="fp8", opt="sgd", wire="fp32"),
    "4x256-fp8-sgd": dict(layers=4, ch=256, dtype="fp8", opt="sgd", wire="fp32"),
}
# refresh-table column -> (oracle name, the model's list of that copy)
_RT_COPIES = {1: ("wf", "wf"), 2: ("wd", "wd"), 10: ("wf8", "wf8"), 16: ("wf_frag", "wfrag"),
              17: ("wd_frag", "wdfrag"), 18: ("wf8_frag", "wf8frag"), 19: ("wd8_frag", "wd8frag"),
              9: ("pbias_frag", "pbias_frag"), 15: ("pbias", "pbias")}
RT_S_W, RT_AMAX_W = 11, 12


def _check_operand_copies(net, pnew):
    """Every non-zero copy column of the per-step refresh table against refresh_expected of
    the new parameters (fp8 copies with the weight scale the step left)."""
    lay = net.layout
    t = net._step_refresh_table()
    seen = set()
    for r, p in enumerate(net.plans):
        w = lay.weight(pnew, p.index)
        wd = net.wd[p.index]
        s_w = net.fp8_scales[2 * p.index].cpu() if t[r, RT_S_W] else None
        exp = refresh_expected(w, p.cinp, net.wf[p.index].shape[1], net.wf[p.index].shape[0],
                               wd.shape[1] if wd is not None else 0,
                               wd.shape[0] if wd is not None else 0, s_w=s_w,
                               bias=lay.bias(pnew, p.index), posb=lay.pos_bias(pnew, p.index))
        for col, (name, attr) in _RT_COPIES.items():
            if not t[r, col]:
                continue
            ten = getattr(net, attr)[p.index]
            assert ten is not None and ten.data_ptr() == int(t[r, col]), (p.index, name)
            assert name in exp, (p.index, name)
            got, want = bits(ten), bits(exp[name])
            assert got.shape == want.shape, (p.index, name)
            bad = (got != want).nonzero().reshape(-1)
            assert bad.numel() == 0, (p.index, name, bad.numel(), bad[:8].tolist())
            seen.add(name)
        if t[r, RT_AMAX_W]:
            slots = net.fp8_amax_w[p.index].cpu().view(torch.float32)
            assert same_bits(slots.max().reshape(1), exp["amax"].reshape(1)), p.index
            seen.add("amax")
    return seen


@pytest.mark.parametrize("fused", ["1", "0"])
@pytest.mark.parametrize("name", list(STEP_CONFIGS))
def test_train_step_matches_references(name, fused, monkeypatch):
    """Two train_step() calls at B = 4 with rateDecay = 1e-3, on the fused update launch
    (DG_FUSED_UPDATE=1: deferred slabs where the model can, else the flat gradient) and on the
    separate launches (0).  After each: params (and ms) equal sgd_ref / rmsprop_ref of the
    snapshot and the gradient the step reports, to A1's / A2's bounds — the head's plain range
    and the per-channel biases included; lr = lr0 (1 - 1e-3), step_count + 1, tickets 0; the
    bf16 wire twin is the fp32 gradient rounded once; every operand copy the step refreshes
    equals the layouts of the NEW parameters.  (On the deferred path the reported gradient is
    written by the update launch itself: that its slab and partial sums are right rests on
    tests/test_grad_reduce_gpu.py — test_grad_update_deferred_exact_on_integer_data and
    test_grad_update_deferred_matches_reduce_and_documented_order — not on this test.)

    Measured on an MI355X (RMSProp configs, both paths alike): ms within 1.2 x 2^-24, the
    update within 1.4 x 2^-24 |d| where p's final rounding is negligible."""
    from deep_go_amd.config import ExperimentConfig
    from deep_go_amd.data.synthetic import random_planes
    from deep_go_amd.models.hip_model import HipGoNet
    c = STEP_CONFIGS[name]
    monkeypatch.setenv("DG_FUSED_UPDATE", fused)
    B = 4
    kw = dict(optimizer="rmsprop", rate=1e-3) if c["opt"] == "rmsprop" else {}
    cfg = ExperimentConfig(numLayers=c["layers"], channelSize=c["ch"], batchSize=B, seed=5,
                           dtype=c["dtype"], rateDecay=1e-3, **kw)
    net = HipGoNet(cfg, B, device="cuda", grad_wire=c["wire"])
    net.set_batch(*[torch.from_numpy(a).cuda() for a in random_planes(B, seed=12)])
    net.keep_grads = True
    wire16 = c["wire"] == "bf16"
    assert net.can_defer() == (fused == "1" and c["ch"] >= 128 and not wire16)
    assert (net.ms is not None) == (c["opt"] == "rmsprop")
    seen = set()
    worst = np.zeros(3)
    for step in range(2):
        torch.cuda.synchronize()
        p0 = net.params.cpu().clone()
        ms0 = net.ms.cpu().clone() if net.ms is not None else None
        lr0, st0 = net.lr.item(), int(net.step_count.item())
        net.train_step()
        torch.cuda.synchronize()
        assert int(net.bad_steps.item()) == 0 and net.gate.item() == 1.0
        if wire16:
            assert torch.equal(net.grads16, net.grads.to(torch.bfloat16))
        g = (net.grads16.float() if wire16 else net.grads).cpu()
        assert torch.isfinite(g).all() and g.abs().max() > 0
        p1 = net.params.cpu()
        if ms0 is not None:
            worst = np.maximum(worst, rmsprop_check(p0, ms0, p1, net.ms.cpu(), g, lr0,
                                                    cfg.rmsprop_decay, 1.0))
        else:
            ref = sgd_ref(p0, g, lr0, 1.0)
            err, bound = (p1.double() - ref).abs(), sgd_bound(ref, g, lr0, 1.0)
            k = int((err - bound).argmax())
            assert (err <= bound).all(), (step, k, err[k].item(), bound[k].item())
        assert abs(net.lr.item() - lr0 * (1.0 - 1e-3)) <= 1e-15
        assert int(net.step_count.item()) == st0 + 1
        assert int(net.gu_tickets.abs().sum().item()) == 0
        seen |= _check_operand_copies(net, p1)
    if ms0 is not None:
        print(f"RMSPROP_ERR step name={name} fused={fused} " + _fmt_err(worst))
    print(f"STEP_COPIES name={name} fused={fused} checked={sorted(seen)}")
    assert seen, "the step refreshed no operand copy"
    if c["dtype"] == "fp8":
        assert {"wf8_frag", "amax"} <= seen
    elif c["ch"] == 128:
        assert {"wf_frag", "wd_frag"} <= seen
