"""The policy head kernels (csrc/kernels/head.hip, head_mfma.hip / head_body.h) and the batch
reduce against the float64 oracle and the staged bounds of tests/test_head_cpu.py.

``h.head`` is called directly on frames built with ops/layouts.py, so that the test owns every
buffer: each output sits between sentinel runs (test_update_gpu.guarded) and is pre-filled
with FILL, the dZ frame included — the head may write its 361 interior pixels only.  The
references come from the inputs (forward) or from the kernel's own output of the stage before
(backward); the kernel under test never produces them.  The figures in the docstrings are the
largest error / bound measured on an MI355X.
"""
import numpy as np
import pytest
import torch

import test_head_cpu as H
from deep_go_amd.ops import layouts as LY
from test_update_gpu import guarded, guards_intact, same_bits

pytestmark = pytest.mark.gpu

NPTS = H.NPTS
FILL = -1232.0            # a bf16 number no output takes
PRED_FILL = -77
EDGE_SHAPES = [(3, 128, 2, 1, 1), (3, 64, 2, 1, 1)]


def _h():
    from deep_go_amd.ops.native import hip
    return hip()


def _s():
    from deep_go_amd.ops.native import stream_handle
    return stream_handle()


def _filled(n, dtype, value=FILL):
    return guarded(torch.full((n,), value, dtype=dtype))


def _ptr(t):
    return 0 if t is None else t[1].data_ptr()


class Head:
    """One launch of h.head over buffers of its own.  x: NHWC interior (CPU); labels: CPU int64
    or None (a null pointer); train False: dZ = 0; logp False: logp_out = 0."""

    def __init__(self, x, w, bias, posb, labels, head_relu, grad_scale, k, x_pad, dz_pad,
                 train=True, logp=True):
        B, C = x.shape[0], x.shape[-1]
        self.B, self.C, self.k, self.dz_pad = B, C, k, dz_pad
        fr = torch.zeros(B, 19 + 2 * x_pad, 19 + 2 * x_pad, C, dtype=torch.bfloat16)
        LY.frame_interior(fr, x_pad).copy_(x.to(torch.bfloat16))
        assert torch.equal(LY.frame_interior(fr, x_pad).double(), x.double())
        self.ins = [guarded(fr), guarded(w.float().contiguous()),
                    guarded(torch.tensor([bias], dtype=torch.float32)), guarded(posb.float())]
        self.lab = None if labels is None else guarded(labels.to(torch.int32))
        Fd = 19 + 2 * dz_pad
        self.loss = _filled(B, torch.float32)
        self.pred = _filled(B, torch.int32, PRED_FILL)
        self.logp = _filled(B * NPTS, torch.float32) if logp else None
        self.dzf = _filled(B * Fd * Fd * C, torch.bfloat16)
        self.gwp = _filled(B * k * k * C, torch.float32)
        self.dzb = _filled(B * NPTS, torch.float32)
        self.outs = [t for t in (self.loss, self.pred, self.logp, self.dzf, self.gwp, self.dzb)
                     if t is not None]
        xf, wd, bd, pd = self.ins
        self.args = (k, xf[1].data_ptr(), x_pad, C, B, wd[1].data_ptr(), bd[1].data_ptr(),
                     pd[1].data_ptr(), _ptr(self.lab), self.loss[1].data_ptr(),
                     self.pred[1].data_ptr(), _ptr(self.logp),
                     self.dzf[1].data_ptr() if train else 0, dz_pad, self.gwp[1].data_ptr(), 0,
                     self.dzb[1].data_ptr(), int(head_relu), float(grad_scale))

    def launch(self):
        _h().head(*self.args, _s())
        torch.cuda.synchronize()
        for buf, _ in self.ins + self.outs + ([self.lab] if self.lab else []):
            assert guards_intact(buf)
        return self

    def untouched(self, which):
        buf, view = which
        fill = PRED_FILL if view.dtype == torch.int32 else FILL
        return bool((view == fill).all().item())

    def got(self):
        """CPU outputs; dz: the bf16 interior, after the frame's border was found untouched."""
        B, C, p = self.B, self.C, self.dz_pad
        Fd = 19 + 2 * p
        fr = self.dzf[1].cpu().view(B, Fd, Fd, C)
        inner = LY.frame_interior(fr, p)
        border = torch.ones(B, Fd, Fd, dtype=torch.bool)
        border[:, p:p + 19, p:p + 19] = False
        assert (fr[border] == FILL).all(), "the head wrote outside the dZ frame's interior"
        out = {"loss": self.loss[1].cpu(), "pred": self.pred[1].cpu(),
               "dzb": self.dzb[1].cpu().view(B, NPTS),
               "gw_part": self.gwp[1].cpu().view(B, -1), "dz": inner.contiguous()}
        if self.logp is not None:
            out["logp"] = self.logp[1].cpu().view(B, NPTS)
        return out


def _run_case(kind, shape, relu, gs):
    k, C, B, xp, dp = shape
    mfma = H.is_mfma(k, C, xp, dp)
    c, labels, ref, lb, zb = H.case_ref(kind, k, C, B, relu, gs)
    boards, amb = None, None
    if zb is not None:
        boards = H.pred_boards(ref, zb)
        assert boards.all()
        if relu:
            amb = H.ambiguous_gate(ref, zb)
            assert amb.double().mean().item() <= 0.01
    got = Head(c["x"], c["w"], c["bias"], c["posb"], labels, relu, gs, k, xp, dp).launch().got()
    tag = (kind, shape, relu, gs)
    rf = H.check_forward(got, ref, lb, labels, boards, tag)
    rb = H.check_backward(got, c["x"], c["w"], labels, gs, k, mfma, ref["gate"] if relu else None,
                          amb, tag)
    live = (c["x"] > 0)
    for name in ("logp", "loss", "dzb", "gw_part", "dz"):
        assert torch.isfinite(got[name]).all(), (tag, name)
    assert (got["dz"].double()[live] != 0).any() and (got["dzb"] != 0).any()
    return np.array([rf, *rb])


def _sweep(kind, shape):
    worst = np.zeros(4)
    for relu in (False, True):
        for gs in H.grad_scales(shape[2]):
            worst = np.maximum(worst, _run_case(kind, shape, relu, gs))
    print("HEAD_ERR %s %s logp %.3f dzb %.3f gw_part %.3f dZ %.3f"
          % ((kind, H.shape_id(shape)) + tuple(worst)))
    assert (worst <= 1).all(), worst            # (False for a NaN ratio too)
    return worst


# ===================================================================== a: designed forward
@pytest.mark.parametrize("shape", H.SHAPES, ids=H.shape_id)
def test_designed_data(shape):
    """x in {0, 1}, w = +-(1 + 2^-10), posb a permutation over 512: the logits are exact in any
    order, so logp and loss are held to the softmax's own roundings and pred to the oracle on
    every board — a forward on the fp32 master weights is off by 2^-10 |sum|, thousands of
    bounds; the staged backward follows, where bf16 weights in dX are off by 2^-10 against a
    bound of 2^-15.  head_relu off / on, grad_scale 1/B, 1/2048, 1; labels at the corners.

    Measured on an MI355X (largest error / bound over the nine shapes): logp 0.32 (C = 256),
    dzb 0.97 at C = 256 and 0.46 at C = 128 — both an exp(logp) just below 2^-126 (1.137e-38 at
    logp = -87.37) that __expf returns as 0, which is what the bound's absolute floor is for;
    at most 0.29 elsewhere.  Off the label and at grad_scale 1 dzb is __expf(logp) itself: over
    logp in [-87.3, 0] it is within 1.2 * 2^-24 |logp| relative of float64 (55 ulps at -87),
    against the 4 * 2^-24 |logp| + EXP_ULPS ulps allowed.  gw_part 0.064
    (MFMA) and 0.006 (VALU); dZ's least pre-rounding error 0.26 of its bound (MFMA), no element
    outside its bf16 bracket."""
    _sweep("designed", shape)


# ===================================================================== b: Gaussian data
@pytest.mark.parametrize("shape", H.SHAPES, ids=H.shape_id)
def test_gaussian_data(shape):
    """x = bf16(relu(randn)), w = 0.05 randn in fp32 (not bf16 numbers): logp, loss and pred
    from the inputs within the forward bound plus the softmax's; pred on every board (the top-2
    gap exceeds twice the logit bound on all of them, asserted on the reference); dzb, gw_part
    and the bf16 dZ teacher-forced; under head_relu a logit within the bound of 0 (at most 1%)
    may take either side of the gate, every other element is strict.

    Measured on an MI355X (largest error / bound over the nine shapes): logp 0.19 at (1, 8) and
    below 0.01 from C = 64 up, where the worst-case forward term dominates the bound; dzb 0.24;
    gw_part 0.048 (MFMA) and 0.005 (VALU); dZ's least pre-rounding error 0.42 (MFMA) and 0.026
    (VALU) of its bound, no element outside its bf16 bracket."""
    _sweep("gaussian", shape)


# ===================================================================== c: edges
def _launch_ref(c, labels, relu, gs, shape, **kw):
    k, C, B, xp, dp = shape
    ref = H.head_ref(c["x"], c["w"], c["bias"], c["posb"], labels, relu, gs, k)
    hd = Head(c["x"], c["w"], c["bias"], c["posb"], labels, relu, gs, k, xp, dp, **kw).launch()
    return ref, hd


@pytest.mark.parametrize("shape", EDGE_SHAPES, ids=H.shape_id)
def test_ties_go_to_the_lowest_index(shape):
    """Integer logits whose maximum sits at two points, and at all 361: pred is the lowest."""
    k, C, B, xp, dp = shape
    pairs = [(3, 60), (63, 64), (10, 300), (0, 360), tuple(range(NPTS))]
    for i in range(0, len(pairs), B):
        pp = (pairs[i:i + B] + pairs[:B])[:B]
        c = H.tie_case(k, C, B, pp)
        labels = torch.tensor([p[-1] for p in pp])
        for relu in (False, True):
            ref, hd = _launch_ref(c, labels, relu, 1.0 / B, shape)
            assert ref["pred"].tolist() == [min(p) for p in pp]
            H.check_forward(hd.got(), ref, H.logp_bound(ref), labels, None, (pp, relu))


@pytest.mark.parametrize("shape", EDGE_SHAPES, ids=H.shape_id)
def test_peaked_logits(shape):
    """posb[p*] = 60 over otherwise small logits: the loss is about 60 off p* and about 0 at
    it, the other probabilities are about exp(-60) = 9e-27 — small but normal fp32 numbers
    (results below 2^-126, which __expf returns as 0, occur on the designed data instead);
    logp, loss, pred and the staged backward hold their bounds.  Measured on an MI355X: logp
    0.008, dzb 0.24, gw_part 0.028, dZ 0.23 of the bound."""
    k, C, B, xp, dp = shape
    c = dict(H.gaussian_case(k, C, B))
    star = 200
    posb = c["posb"].clone()
    posb[star] = 60.0
    c["posb"] = posb
    labels = torch.tensor([star, 360])[:B]
    worst = np.zeros(4)
    for relu in (False, True):
        gs = 1.0 / B
        ref, hd = _launch_ref(c, labels, relu, gs, shape)
        zb = H.z_bound(c["x"], c["w"], c["bias"], c["posb"], k)
        got = hd.got()
        assert abs(ref["loss"][1].item() - 60) < 10 and ref["loss"][0].item() < 1e-10
        assert ref["pred"].tolist() == [star] * B
        rf = H.check_forward(got, ref, H.logp_bound(ref, zb), labels, None, relu)
        amb = H.ambiguous_gate(ref, zb) if relu else None
        rb = H.check_backward(got, c["x"], c["w"], labels, gs, k, H.is_mfma(k, C, xp, dp),
                              ref["gate"] if relu else None, amb, relu)
        worst = np.maximum(worst, np.array([rf, *rb]))
    print("HEAD_ERR peaked %s logp %.3f dzb %.3f gw_part %.3f dZ %.3f"
          % ((H.shape_id(shape),) + tuple(worst)))
    assert (worst <= 1).all(), worst


@pytest.mark.parametrize("shape", EDGE_SHAPES, ids=H.shape_id)
def test_flat_logits(shape):
    """w = 0, posb = 0, bias = 0: logp is -ln 361 within the softmax bound, pred is 0.
    Measured on an MI355X: 0.10 of the bound."""
    k, C, B, xp, dp = shape
    c = dict(H.gaussian_case(k, C, B))
    c.update(w=torch.zeros(k * k, C), posb=torch.zeros(NPTS), bias=0.0)
    labels = torch.tensor([0, 360])[:B]
    for relu in (False, True):
        ref, hd = _launch_ref(c, labels, relu, 1.0, shape)
        got = hd.got()
        assert ref["pred"].tolist() == [0] * B
        assert (ref["logp"] + np.log(361)).abs().max().item() < 1e-14
        r = H.check_forward(got, ref, H.logp_bound(ref), labels, None, relu)
        print("HEAD_ERR flat %s relu %d logp %.3f" % (H.shape_id(shape), relu, r))
        assert r <= 1


@pytest.mark.parametrize("shape", EDGE_SHAPES, ids=H.shape_id)
def test_dead_logits_give_exact_zeros(shape):
    """head_relu with every z <= 0 (bias = -100): the softmax is uniform, the loss ln 361, and
    dzb, gw_part and the dZ interior are +0 in every bit (test_head_relu_dead_logits_quirk)."""
    k, C, B, xp, dp = shape
    c = dict(H.gaussian_case(k, C, B))
    c["bias"] = -100.0
    labels = torch.tensor([18, 342])[:B]
    ref, hd = _launch_ref(c, labels, True, 1.0 / B, shape)
    assert (ref["z"] < 0).all()
    got = hd.got()
    zb = H.z_bound(c["x"], c["w"], c["bias"], c["posb"], k)
    assert (ref["z"] + zb < 0).all()
    H.check_forward(got, ref, H.logp_bound(ref), labels)       # (l = 0 exactly: softmax alone)
    for name in ("dzb", "gw_part", "dz"):                 # +0 bit for bit: -0 fails too
        assert same_bits(got[name], torch.zeros_like(got[name])), name


@pytest.mark.parametrize("shape", EDGE_SHAPES, ids=H.shape_id)
def test_eval_mode_and_null_pointers(shape):
    """dZ = 0: loss, pred and logp keep the training call's bits, gw_part, dzb and the dZ frame
    their fill.  labels = 0: loss keeps its fill, pred and logp their bits.  logp_out = 0: every
    other output keeps its bits."""
    k, C, B, xp, dp = shape
    for relu in (False, True):
        c, labels, ref, lb, zb = H.case_ref("gaussian", k, C, B, relu, 1.0 / B)
        a = (c["x"], c["w"], c["bias"], c["posb"])
        t = Head(*a, labels, relu, 1.0 / B, k, xp, dp).launch()
        tg = t.got()
        e = Head(*a, labels, relu, 1.0 / B, k, xp, dp, train=False).launch()
        for name in ("loss", "pred", "logp"):
            assert same_bits(getattr(e, name)[1], getattr(t, name)[1]), name
        assert e.untouched(e.gwp) and e.untouched(e.dzb) and e.untouched(e.dzf)
        n = Head(*a, None, relu, 1.0 / B, k, xp, dp, train=False).launch()
        assert n.untouched(n.loss)
        assert same_bits(n.pred[1], t.pred[1]) and same_bits(n.logp[1], t.logp[1])
        q = Head(*a, labels, relu, 1.0 / B, k, xp, dp, logp=False).launch()
        qg = q.got()
        for name in ("loss", "pred", "dzb", "gw_part", "dz"):
            assert same_bits(qg[name], tg[name]), name


# ===================================================================== d: launcher
@pytest.mark.parametrize("k,C,x_pad", [(5, 128, 2), (5, 256, 2), (3, 12, 1), (3, 132, 1),
                                       (3, 0, 1), (2, 64, 1), (7, 64, 3), (4, 128, 1)])
def test_launcher_refuses_before_any_launch(k, C, x_pad):
    """A VALU head whose LDS request exceeds 160 KB (5x5 at C >= 128), C % 8 != 0, C = 0 and
    an unsupported kernel size: hipErrorInvalidValue (a RuntimeError) and no output touched."""
    B = 2
    x = torch.zeros(B, 19, 19, C)
    hd = Head(x, torch.zeros(k * k, C), 0.0, torch.zeros(NPTS), torch.tensor([0, 360]), True,
              0.5, k, x_pad, 1)
    with pytest.raises(RuntimeError):
        hd.launch()
    torch.cuda.synchronize()
    for buf, view in hd.outs:
        assert guards_intact(buf) and hd.untouched((buf, view))


# ===================================================================== 3: head_reduce
RB = [1, 8, 9, 16, 17, 240, 241, 256, 272]
RN = [8, 23, 576, 1152, 2304]


class Reduce:
    def __init__(self, dzb, gwp, twins, sf=(5, 0)):
        B, n = gwp.shape
        self.B, self.n = B, n
        self.dzb, self.gwp = guarded(dzb), guarded(gwp)
        self.gw = _filled(n, torch.float32)
        self.gb = _filled(1, torch.float32)
        self.gp = _filled(NPTS, torch.float32)
        self.tw = [_filled(m, torch.bfloat16) for m in (n, 1, NPTS)] if twins else None
        self.sf0 = torch.tensor(list(sf), dtype=torch.int64)
        self.sf = guarded(self.sf0)

    def launch(self):
        a = (self.dzb[1].data_ptr(), self.gwp[1].data_ptr(), self.B, self.n,
             self.gw[1].data_ptr(), self.gb[1].data_ptr(), self.gp[1].data_ptr())
        if self.tw:
            _h().head_reduce_w(*a, *[t[1].data_ptr() for t in self.tw], self.sf[1].data_ptr(), _s())
        else:
            _h().head_reduce(*a, self.sf[1].data_ptr(), _s())
        torch.cuda.synchronize()
        for buf, _ in [self.dzb, self.gwp, self.gw, self.gb, self.gp, self.sf] + (self.tw or []):
            assert guards_intact(buf)
        return self

    def outs(self):
        return self.gw[1].cpu(), self.gb[1].cpu()[0], self.gp[1].cpu()


@pytest.mark.parametrize("B", RB)
def test_head_reduce(B):
    """head_reduce and head_reduce_w over synthetic partials, n = 8, 23, 576, 1152, 2304 (the
    last: B = 272 only): integer partials in -8 .. 8 give the float64 sums exactly, Gaussian
    ones stay within B roundings (gbias: its loop shape), doubled; the bf16 twins are the fp32
    outputs rounded, the two entry points' fp32 outputs share their bits, the step tag is left
    alone.  B covers both sides of the gbias unroll (B 361 against 3072: 8 | 9) and of the
    16-board loop (per = 15, 16, 17: 240, 241 .. 256, 272).

    Measured on an MI355X, Gaussian partials: gw 0.16, gposb 0.13 (both at B = 8) and gbias
    0.001 of the bound; every integer case exact."""
    worst = np.zeros(3)
    for n in RN:
        if n == 2304 and B != 272:
            continue
        for integer in (True, False):
            dzb, gwp = H.reduce_case(B, n, integer)
            r = Reduce(dzb, gwp, False).launch()
            worst = np.maximum(worst, H.check_reduce(*r.outs(), dzb, gwp, integer, (B, n)))
            assert same_bits(r.sf[1], r.sf0)
            w = Reduce(dzb, gwp, True).launch()
            for a, b, t in zip((w.gw, w.gb, w.gp), (r.gw, r.gb, r.gp), w.tw):
                assert same_bits(a[1], b[1])
                assert same_bits(t[1], a[1].to(torch.bfloat16))
            assert same_bits(w.sf[1], w.sf0)
    print("REDUCE_ERR B=%d gw %.3f gposb %.3f gbias %.3f" % ((B,) + tuple(worst)))
    assert (worst <= 1).all(), worst


@pytest.mark.parametrize("bad", [2.0 ** 121, float("nan")])
@pytest.mark.parametrize("where", ["gw_part", "dzb", "gbias"])
def test_head_reduce_tags_a_bad_step(where, bad):
    """One partial at 2^121 or NaN in gw_part, or in dzb (its gposb column); and through the
    gbias sum alone, every gposb column staying in range: four columns of 2^119 sum to 2^121,
    and (no NaN can arise there without an infinite column) one 0.99 2^120 in each of the 361
    columns overflows gbias.  sf[1] = sf[0] + 1, sf[0] is left alone."""
    B, n = 17, 23
    dzb, gwp = H.reduce_case(B, n, True)
    if where == "gw_part":
        gwp[B - 1, n - 1] = bad
    elif where == "dzb":
        dzb[3, 360] = bad
    elif bad == bad:
        dzb[0, :4] = 2.0 ** 119
    else:
        dzb[torch.arange(NPTS) % B, torch.arange(NPTS)] = 0.99 * 2.0 ** 120
    if where == "gbias":
        assert (dzb.double().sum(0).abs() < 2.0 ** 120).all()
        assert not dzb.double().sum().float().abs() < 2.0 ** 120
    for twins in (False, True):
        r = Reduce(dzb, gwp, twins, sf=(41, 7)).launch()
        assert r.sf[1].cpu().tolist() == [41, 42], (where, bad, twins)
