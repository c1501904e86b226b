"""optimizer=lamb on the GPU: the kernels of csrc/kernels/optim.hip (module _dglamb) against
the float64 oracle of tests/test_lamb_cpu.py within its counted bounds, stage by stage (m, v, u;
the recorded norms; the ratio that follows from them exactly; the parameters), the segmented
sums' edge cases, inside HipGoNet (eager and as step graphs, bf16 and fp8, with the bf16 wire
twin, with grad_clip, ema_decay and lr_schedule), the skip policy, exact resume and the fp32
CPU trainer.

Buffers under test — the record, the partials and the table of ratios included — sit between
sentinel runs (test_update_gpu.guarded); the partials start as NaN, so a slot read without
having been written shows.  The float64 references of the large vectors are evaluated with
torch on the device; the kernels under test never produce them.
"""
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from test_adamw_cpu import APPLY, BETAS, EPS, adam_corrections
from test_lamb_cpu import (LR, N_EMU, RANGES_EMU, STAGES, WD, check_lamb_step,
                           trust_ratio32)
from test_momentum_gpu import _np_table
from test_update_gpu import DEV, guarded, guards_intact, same_bits

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROWS = 20


def _lamb():
    from deep_go_amd.ops.native import lamb
    return lamb()


class Bufs:
    """p, m, v, u, the record (t = t0), the partials (NaN) and the table between sentinels."""

    def __init__(self, n, ranges, p, m, v, t0=0):
        t = _np_table(ranges)
        need = _lamb().lamb_partials(n, t.ctypes.data if len(t) else 0, len(t))
        self.n, self.ranges, self.table = n, ranges, t
        self.pbuf, self.p = guarded(p)
        self.mbuf, self.m = guarded(m)
        self.vbuf, self.v = guarded(v)
        self.ubuf, self.u = guarded(torch.full((n,), 7.0))
        self.rbuf, self.rec = guarded(torch.tensor([t0, 0], dtype=torch.int64))
        self.partbuf, self.part = guarded(torch.full((need,), float("nan")))
        self.tabbuf, self.tab = guarded(torch.full((ROWS * 3,), -2.0))

    def launch(self, g, lrt, wd=WD, gscale=1.0, gt=None):
        from deep_go_amd.ops.native import stream_handle
        fn = _lamb().lamb_bf16 if g.dtype == torch.bfloat16 else _lamb().lamb
        t = self.table
        fn(self.p.data_ptr(), g.data_ptr(), self.m.data_ptr(), self.v.data_ptr(),
           self.u.data_ptr(), self.n, lrt.data_ptr(), self.rec.data_ptr(), self.part.data_ptr(),
           self.part.numel(), self.tab.data_ptr(), BETAS[0], BETAS[1], EPS, wd,
           t.ctypes.data if len(t) else 0, len(t), gscale,
           gt.data_ptr() if gt is not None else 0, stream_handle())
        torch.cuda.synchronize()

    def state(self):
        return [x.clone() for x in (self.p, self.m, self.v, self.u, self.rec, self.part,
                                    self.tab)]

    def same(self, st):
        return all(same_bits(a, b) for a, b in zip(
            (self.p, self.m, self.v, self.u, self.rec, self.part, self.tab), st))

    def intact(self):
        return all(guards_intact(b) for b in (self.pbuf, self.mbuf, self.vbuf, self.ubuf,
                                              self.rbuf, self.partbuf, self.tabbuf))

    def stats(self):
        rows = self.tab.cpu().view(ROWS, 3)
        assert (rows[len(self.ranges):] == -2.0).all()      # (rows without a range: untouched)
        return [tuple(r) for r in rows[:len(self.ranges)].tolist()]

    def t(self):
        return int(self.rec[0].item())


# ===================================================================== A: the kernels
# CAP + 1203: past the kernels' grid cap (8192 workgroups x 256 threads x 4), where a workgroup
# takes a second pass over another chunk; 3-element tail
CAP = 8192 * 256 * 4
SIZES = [1, 3, 4, 1023, 1024, 1025, 4099, CAP + 1203]


def range_tables(n):
    """{name: table}, each clipped to what fits n: no range; one range ending at n; one ending
    in the middle of a 4-vector; three short ones inside one 1024-element chunk; one from the
    first element to the last; as many ranges as fit (16 at 4099: four per chunk; 20 beyond),
    some across chunk boundaries."""
    t = {"none": [], "whole": [(0, n)]}
    t["to n"] = [((n // 2) // 64 * 64, n)]
    if n >= 3:
        t["mid-vector"] = [(0, min(n - 1, 64 * 3 + 1))]
    if n >= 1023:
        t["three in a chunk"] = [(64, 69), (128, 191), (256, 386)]
    if n == 4099:
        t["sixteen"] = [(256 * i, 256 * i + (250 if i % 3 else 7)) for i in range(15)] + \
            [(3840, n)]
    if n > 10 ** 6:
        # four short ones in the first chunk, the rest spread out, a few thousand elements or a
        # few million each, the last ending inside the tail
        short = [(0, 3), (64, 127), (256, 258), (512, 1023)]
        step = (n - 4096) // 16 // 64 * 64
        long_ = [(4096 + step * i, 4096 + step * i + (step - 64 if i % 2 else 4097))
                 for i in range(15)] + [(4096 + step * 15, n)]
        t["twenty"] = short + long_
        assert len(t["twenty"]) == 20
    return t


def _inputs(n, kind, seed):
    gen = torch.Generator().manual_seed(seed)
    p = torch.randn(n, generator=gen)
    m = torch.randn(n, generator=gen) * 0.05
    v = torch.rand(n, generator=gen) * 0.01 + 1e-4
    grads = []
    for scale in (2.0, 0.3):
        g = torch.randn(n, generator=gen) * scale
        grads.append(g.to(torch.bfloat16) if kind == "bf16" else g)
    return p, m, v, grads


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("kind", ["fp32", "bf16"])
def test_lamb_matches_float64_reference(kind, n):
    """lamb / lamb_bf16 against lamb_ref over two consecutive launches (the second reads the
    moments and the count the first wrote; each is compared from the state it started from), for
    every range table, gscale, gate and starting count, stage by stage within lamb_bounds.
    gate = 0 leaves p, m, v, u, the record, the partials and the table bit-identical, also under
    an all-NaN gradient; the sentinels around every buffer stay; the device lr is not
    written."""
    p_init, m_init, v_init, grads = _inputs(n, kind, 600 + n % 1000)
    gdev = [guarded(g) for g in grads]
    nanbuf, nand = guarded(torch.full_like(grads[0], float("nan")))
    lrt = torch.tensor([LR], dtype=torch.float64, device=DEV)
    big = n > 10 ** 6
    worst = {}
    for name, ranges in range_tables(n).items():
        for t0 in [0, 7]:
            for gscale in ([0.37] if big else [1.0, 0.37]):
                for gate in ([None, 0.0] if big else [None, 1.0, 0.0]):
                    tag = (name, t0, gscale, gate)
                    b = Bufs(n, ranges, p_init, m_init, v_init, t0)
                    gt = None if gate is None else torch.tensor([gate], device=DEV)
                    t = t0
                    for gbuf, gd in gdev:
                        st = b.state()
                        b.launch(gd, lrt, WD, gscale, gt)
                        assert b.intact() and guards_intact(gbuf), tag
                        if gate == 0.0:
                            assert b.same(st), tag
                            continue
                        t += 1
                        assert b.t() == t, tag
                        out = check_lamb_step(st[0], gd.float(), st[1], st[2], b.p, b.m, b.v,
                                              b.u, b.stats(), t, LR, BETAS, EPS, WD, ranges,
                                              gscale, tag)
                        worst = {k: max(worst.get(k, 0.0), x) for k, x in out.items()}
                        assert not torch.equal(b.p, st[0]) and not torch.equal(b.m, st[1])
        # a closed gate over an all-NaN gradient
        b = Bufs(n, ranges, p_init, m_init, v_init, 7)
        st = b.state()
        b.launch(nand, lrt, WD, 1.0, torch.zeros(1, device=DEV))
        assert b.same(st) and b.intact() and guards_intact(nanbuf)
    assert lrt.item() == LR
    print(f"LAMB_ERR kind={kind} n={n} error over bound "
          + " ".join(f"{k}={worst[k]:.3f}" for k in STAGES))


# ===================================================================== B: the segmented sums
@pytest.mark.parametrize("n", [N_EMU, 65541])
def test_integer_parameters_pin_the_weight_norms_bit_for_bit(n):
    """Integer p with |p| <= 8: every fp32 partial is an exact integer below 2^24 and their
    double sum is exact, so wn = fp32(sqrt(fp32(sum p^2))) whatever the order — bit for bit,
    for a range ending mid-vector, three in one chunk, and one across chunks into the tail."""
    gen = torch.Generator().manual_seed(40)
    ranges = RANGES_EMU[:-1] + [(RANGES_EMU[-1][0], n)]
    p = torch.randint(-8, 9, (n,), generator=gen).float()
    _, m, v, grads = _inputs(n, "fp32", 41)
    b = Bufs(n, ranges, p, m, v)
    lrt = torch.tensor([LR], dtype=torch.float64, device=DEV)
    b.launch(guarded(grads[0])[1], lrt)
    for (lo, hi), (wn, un, phi) in zip(ranges, b.stats()):
        s = int((p[lo:hi].long() ** 2).sum())
        want = np.float32(np.sqrt(np.float64(np.float32(s))))
        assert np.float32(wn) == want, (lo, hi, wn, want)
        assert phi == trust_ratio32(wn, un) and phi != 1.0
    assert b.intact()


def test_degenerate_ranges_take_ratio_one():
    """A range of zero parameters (wn = 0), a range with zero update (g = m = v = 0, wd = 0:
    un = 0) and a range whose squares overflow fp32 (wn = inf) all take phi = 1, bit for bit;
    every output stays finite, and each range's update is then Adam's: p - lr u."""
    n, ranges = 4099, [(0, 193), (1024 + 64, 1024 + 64 + 5), (2048 - 64, 4099)]
    p, m, v, grads = _inputs(n, "fp32", 42)
    g = grads[0].clone()
    p[0:193] = 0.0
    g[1088:1093] = 0.0
    m[1088:1093] = 0.0
    v[1088:1093] = 0.0
    p[1984:4099] = 3e19 * torch.sign(p[1984:4099] + 1e-3)       # 2115 squares of 9e38
    b = Bufs(n, ranges, p, m, v, 5)
    lrt = torch.tensor([LR], dtype=torch.float64, device=DEV)
    st = b.state()
    b.launch(guarded(g)[1], lrt, wd=0.0)
    s = b.stats()
    assert s[0][0] == 0.0 and s[0][1] > 0 and s[0][2] == 1.0
    assert s[1][0] > 0 and s[1][1] == 0.0 and s[1][2] == 1.0
    assert s[2][0] == math.inf and s[2][2] == 1.0
    for x in (b.p, b.m, b.v, b.u):
        assert torch.isfinite(x).all()
    check_lamb_step(st[0], g.to(DEV), st[1], st[2], b.p, b.m, b.v, b.u, s, 6, LR, BETAS, EPS, 0.0,
                    ranges, 1.0, "degenerate")
    assert b.intact()


def test_one_element_moves_only_its_own_ratio():
    """Changing one element of p or of g — the first of a range, its mid-vector last, one of a
    short range, the very last (in the n % 4 tail), one outside every range — changes the row
    of its own range only (none when it lies outside); every other row keeps its bits."""
    n, ranges = N_EMU, RANGES_EMU
    p, m, v, grads = _inputs(n, "fp32", 43)
    lrt = torch.tensor([LR], dtype=torch.float64, device=DEV)

    def rows(pp, gg):
        b = Bufs(n, ranges, pp, m, v, 3)
        b.launch(guarded(gg)[1], lrt)
        assert b.intact()
        return np.array(b.stats(), dtype=np.float32).view(np.int32)
    base = rows(p, grads[0])
    spots = {0: 0, 192: 0, 1024 + 64 + 4: 1, 1024 + 128: 2, 1024 + 256 + 129: 3, n - 1: 4,
             n - 3: 4, 193: None, 1024 + 64 + 5: None, 1983: None}
    for i, own in spots.items():
        for which in ("p", "g"):
            pp, gg = p.clone(), grads[0].clone()
            (pp if which == "p" else gg)[i] += 3.0
            got = rows(pp, gg)
            changed = [k for k in range(len(ranges)) if not np.array_equal(got[k], base[k])]
            assert changed == ([] if own is None else [own]), (i, which, changed)


def test_two_runs_give_identical_bits():
    n = CAP + 1203
    ranges = range_tables(n)["twenty"]
    p, m, v, grads = _inputs(n, "bf16", 44)
    lrt = torch.tensor([LR], dtype=torch.float64, device=DEV)
    gd = guarded(grads[0])[1]
    outs = []
    for _ in range(2):
        b = Bufs(n, ranges, p, m, v, 2)
        b.launch(gd, lrt)
        outs.append(b.state())
    for x, y in zip(*outs):
        # (the partials hold NaN where no range meets a chunk: compared as bits)
        assert same_bits(x, y)


# ===================================================================== C: in the model
MODEL_CASES = {"3x64-bf16": (3, 64, "bf16"), "4x128-bf16": (4, 128, "bf16"),
               "4x128-fp8": (4, 128, "fp8")}
B = 8
RATE_DECAY = 1e-3


def _cfg(layers, ch, dtype, **kw):
    from deep_go_amd.config import ExperimentConfig
    base = dict(numLayers=layers, channelSize=ch, batchSize=B, seed=5, dtype=dtype, rate=1e-3,
                rateDecay=RATE_DECAY, optimizer="lamb", weight_decay=1e-2)
    base.update(kw)
    return ExperimentConfig(**base)


def _batch(n, seed):
    from deep_go_amd.data.synthetic import random_planes
    return [torch.from_numpy(a).cuda() for a in random_planes(n, seed=seed)]


def _state(net):
    return net.params.clone(), net.adam_m.clone(), net.adam_v.clone(), net.lr.item()


def _check_model_step(net, state, t, g, tag):
    cfg = net.cfg
    p0, m0, v0, lr0 = state
    assert torch.isfinite(g).all() and g.abs().max() > 0
    betas = (cfg.adam_beta1, cfg.adam_beta2)
    from deep_go_amd.ops.functional import adamw_record_values
    got = adamw_record_values(net.adam_t)
    assert got[0] == t == net.adam_steps() and got[1:] == adam_corrections(t, betas), (tag, got)
    stats = net.lamb_stats()
    assert len(stats) == len(net.layout.layers) and all(s[2] != 1.0 for s in stats), tag
    return check_lamb_step(p0, g, m0, v0, net.params, net.adam_m, net.adam_v, net.lamb_u, stats,
                           t, lr0, betas, cfg.adam_eps, cfg.weight_decay,
                           net.layout.weight_ranges(), 1.0, tag)


def _fmt(out):
    return " ".join(f"{k}={out[k]:.3f}" for k in STAGES)


@pytest.mark.parametrize("name", list(MODEL_CASES))
def test_model_steps_match_reference_and_graph_equals_eager(name):
    """Three whole steps eagerly and as SegmentedStep's step graph from the same parameters:
    the step is not deferred; after each eager step params, adam_m, adam_v, lamb_u and
    lamb_stats() match lamb_ref of the step's own net.grads; t = steps, lr = rate (1 -
    rateDecay)^t, step_count = t; the graphed net holds the same bits throughout."""
    from deep_go_amd.models.hip_model import HipGoNet, SegmentedStep
    layers, ch, dtype = MODEL_CASES[name]
    cfg = _cfg(layers, ch, dtype)
    nets = [HipGoNet(cfg, B, device="cuda") for _ in range(2)]
    steps = []
    for net, graphs in zip(nets, (False, True)):
        assert net.adam_m is not None and not net.adam_m.any() and net.lamb_u is not None
        assert net.adam_steps() == 0 and net.ms is None and net.vel is None
        assert not net.can_defer() and net._own_update
        net.set_batch(*_batch(B, 12))
        steps.append(SegmentedStep(net, None, use_graphs=graphs))
        assert (steps[-1].full_graph is not None) == graphs
        assert net.adam_steps() == 0       # (no warm-up or capture has counted)
    worst = {}
    for t in range(1, 4):
        torch.cuda.synchronize()
        state = _state(nets[0])
        for step in steps:
            step()
        torch.cuda.synchronize()
        e, g = nets
        assert int(e.bad_steps.item()) == 0 and e.gate.item() == 1.0
        out = _check_model_step(e, state, t, e.grads, (name, t))
        worst = {k: max(worst.get(k, 0.0), x) for k, x in out.items()}
        assert e.lr.item() == pytest.approx(cfg.rate * (1.0 - RATE_DECAY) ** t, rel=1e-13)
        assert int(e.step_count.item()) == t
        for a in ("params", "adam_m", "adam_v", "adam_t", "lamb_u", "lamb_rec", "lr"):
            assert same_bits(getattr(e, a), getattr(g, a)), (name, t, a)
    print(f"LAMB_ERR model name={name} error over bound " + _fmt(worst))
    if dtype == "bf16":
        net = nets[0]
        nxt = _batch(B, 13)
        net.set_batch(*nxt)
        net.forward_backward()
        fresh = HipGoNet(cfg, B, device="cuda", flat_params=net.params.clone())
        fresh.set_batch(*nxt)
        fresh.forward_backward()
        torch.cuda.synchronize()
        assert torch.equal(net.loss, fresh.loss) and torch.equal(net.pred, fresh.pred)


def test_model_step_without_a_gate():
    """nan_policy=raise: no gate launch and no gate pointer; the same update."""
    from deep_go_amd.models.hip_model import HipGoNet
    net = HipGoNet(_cfg(3, 64, "bf16", nan_policy="raise"), B, device="cuda")
    net.set_batch(*_batch(B, 12))
    net.gate.zero_()                    # (nothing may read it)
    for t in range(1, 3):
        state = _state(net)
        net.train_step()
        torch.cuda.synchronize()
        _check_model_step(net, state, t, net.grads, ("raise", t))
        assert int(net.step_count.item()) == t and net.gate.item() == 0.0


@pytest.mark.parametrize("wire", ["fp32", "bf16"])
def test_clip_ema_and_schedule_together(wire):
    """grad_clip, ema_decay and lr_schedule on with lamb, eagerly and graphed: [gate] -> clip ->
    lamb -> refresh -> ema -> schedule.  The update matches lamb_ref of the CLIPPED gradient
    (which the clip leaves in net.grads, widened from the twin under the bf16 wire: the fp32
    entry point) at the scheduled rate; the average follows the updated parameters; graph and
    eager hold the same bits."""
    from deep_go_amd.models.hip_model import HipGoNet, SegmentedStep
    kw = dict(global_batch=2 * B, grad_wire="bf16") if wire == "bf16" else {}
    probe = HipGoNet(_cfg(4, 128, "bf16"), B, device="cuda", **kw)
    probe.set_batch(*_batch(B, 12))
    probe.forward_backward()
    torch.cuda.synchronize()
    # a quarter of the first gradient's norm: every one of the three steps clips
    c = 0.25 * (probe.grads16.float() if wire == "bf16" else probe.grads).norm().item()
    cfg = _cfg(4, 128, "bf16", grad_clip=c, ema_decay=0.9, lr_schedule="cosine", lr_warmup=2,
               lr_total=8)
    nets = [HipGoNet(cfg, B, device="cuda", **kw) for _ in range(2)]
    for net in nets:
        net.set_batch(*_batch(B, 12))
    graph = SegmentedStep(nets[1], None, use_graphs=True)
    e, g = nets
    for t in range(1, 4):
        torch.cuda.synchronize()
        state = _state(e)
        ema0 = e.ema.clone()
        e.forward_backward()
        e.optimizer_step()
        graph()
        torch.cuda.synchronize()
        norm, scale, clipped = e.clip_stats()
        assert scale < 1.0 and clipped == t and norm > c
        _check_model_step(e, state, t, e.grads, ("together", wire, t))
        assert e.ema_steps() == t and not torch.equal(e.ema, ema0)
        assert e.lr_schedule_state()[1] == t and e.lr.item() != state[3]
        for a in ("params", "adam_m", "adam_v", "adam_t", "lamb_rec", "ema", "lr"):
            assert same_bits(getattr(e, a), getattr(g, a)), (wire, t, a)


def test_bf16_wire_step_reads_the_twin():
    from deep_go_amd.models.hip_model import HipGoNet
    net = HipGoNet(_cfg(4, 128, "bf16"), B, device="cuda", global_batch=2 * B, grad_wire="bf16")
    assert net.grads16 is not None and not net.can_defer()
    net.set_batch(*_batch(B, 9))
    state = _state(net)
    net.forward_backward()
    net.optimizer_step()
    torch.cuda.synchronize()
    assert torch.equal(net.grads16, net.grads.to(torch.bfloat16))
    assert not torch.equal(net.grads16.float(), net.grads)
    w = _check_model_step(net, state, 1, net.grads16.float(), "wire")
    print("LAMB_ERR model wire error over bound " + _fmt(w))
    assert int(net.bad_steps.item()) == 0 and int(net.step_count.item()) == 1


# ===================================================================== D: skip
def test_skip_pattern_counts_applied_steps():
    """nan_policy=skip, the pattern apply, skip, apply, apply, skip, apply (a skipped step has a
    poisoned gradient entry, then a poisoned loss): a skipped step keeps params, both moments,
    u, the record, the table and the operand copies bit for bit, still decays the rate and
    counts in step_count; each applied step matches lamb_ref with t = 1, 2, 3, 4; t ends at
    4."""
    from deep_go_amd.models.hip_model import HipGoNet
    cfg = _cfg(4, 128, "bf16", nan_policy="skip")
    net = HipGoNet(cfg, B, device="cuda")
    net.set_batch(*_batch(B, 8))
    t = skipped = 0
    for call, apply in enumerate(APPLY, 1):
        net.forward_backward()
        torch.cuda.synchronize()
        state = _state(net)
        keep = [x.clone() for x in (net.lamb_u, net.adam_t, net.lamb_rec)]
        wf0 = [w.clone() for w in net.wf]
        if not apply:
            skipped += 1
            if skipped == 1:
                net.grads[17] = float("nan")
            else:
                net.loss[0] = float("inf")
        net.optimizer_step()
        torch.cuda.synchronize()
        assert int(net.step_count.item()) == call and net.bad_steps.item() == skipped
        assert net.lr.item() == pytest.approx(cfg.rate * (1.0 - RATE_DECAY) ** call, rel=1e-13)
        if not apply:
            assert net.gate.item() == 0.0 and net.adam_steps() == t
            for a, b in zip((net.params, net.adam_m, net.adam_v), state):
                assert same_bits(a, b)
            for a, b in zip((net.lamb_u, net.adam_t, net.lamb_rec), keep):
                assert same_bits(a, b)
            assert all(torch.equal(a, b) for a, b in zip(net.wf, wf0))
            continue
        t += 1
        _check_model_step(net, state, t, net.grads, ("applied", call))
    assert net.adam_steps() == 4


# ===================================================================== E: resume, imports
def test_hip_backend_resume_is_exact(tmp_path):
    """With the second step skipped: 4 steps == 2 steps + state_dict -> a new backend +
    load_state_dict + 2 steps, bit for bit on params and both moments, t equal (3, not 4); the
    state carries Adam's keys under kind="lamb", and an adamw backend loads its moments."""
    from deep_go_amd.data.synthetic import random_planes
    from deep_go_amd.train.backends import HIPBackend
    cfg = _cfg(3, 64, "bf16", batchSize=4, checkpoint_dir=str(tmp_path), nan_policy="skip")
    batches = [random_planes(4, seed=20 + i) for i in range(4)]

    def run(be, which):
        for i in which:
            be.set_batch(*batches[i])
            be.forward_backward()
            if i == 1:
                be.net.grads[17] = float("nan")
            be.optimizer_step()
        torch.cuda.synchronize()

    a = HIPBackend(cfg, 4)
    p_init = a.flat_params().clone()
    run(a, range(4))
    assert a.net.adam_steps() == 3 and a.bad_steps() == 1
    b = HIPBackend(cfg, 4, flat=p_init)
    run(b, range(2))
    sd = b.state_dict()
    o = sd["optimizer"]
    assert o["kind"] == "lamb" and type(o["adam_t"]) is int and o["adam_t"] == 1
    assert o["adam_m"].abs().max() > 0 and o["adam_v"].abs().max() > 0
    c = HIPBackend(cfg, 4, flat=b.flat_params())
    c.load_state_dict(sd)
    assert c.net.adam_steps() == 1 and c.rate == b.rate
    run(c, range(2, 4))
    assert torch.equal(c.net.params, a.net.params)
    assert torch.equal(c.net.adam_m, a.net.adam_m) and torch.equal(c.net.adam_v, a.net.adam_v)
    assert c.net.adam_steps() == a.net.adam_steps() == 3 and c.rate == a.rate
    assert c.lamb_stats() == a.lamb_stats() and len(c.lamb_stats()) == 3
    w = HIPBackend(cfg.replace(optimizer="adamw"), 4, flat=p_init)
    w.load_state_dict(sd)
    assert torch.equal(w.net.adam_m.cpu(), o["adam_m"]) and w.net.adam_steps() == 1
    old = {"optimizer": {k: v for k, v in o.items() if not k.startswith("adam_")}}
    c.load_state_dict(old)
    assert not c.net.adam_m.any() and not c.net.adam_v.any() and c.net.adam_steps() == 0
    for be in (a, b, c, w):
        be.close()


_CHILD = """
import sys
sys.path.insert(0, {root!r})
import torch
from deep_go_amd.config import ExperimentConfig
from deep_go_amd.models.hip_model import HipGoNet
cfg = ExperimentConfig(numLayers=3, channelSize=64, batchSize=8, seed=5, dtype="bf16",
                       optimizer="adamw", rate=1e-3)
net = HipGoNet(cfg, 8, device="cuda")
assert "_dglamb" not in sys.modules, "optimizer=adamw imported _dglamb"
assert net.lamb_u is None and net.lamb_rec is None
s = HipGoNet(cfg.replace(optimizer="lamb"), 8, device="cuda")
assert "_dglamb" in sys.modules and not s.can_defer() and s.adam_steps() == 0
print("CHILD_OK")
"""


def test_module_is_imported_only_for_lamb():
    """In a fresh process: optimizer=adamw does not import _dglamb; lamb does, never defers, and
    its warm-up launch has left t = 0."""
    env = dict(os.environ)
    env.pop("DG_FUSED_UPDATE", None)
    r = subprocess.run([sys.executable, "-c", _CHILD.format(root=ROOT)], env=env,
                       capture_output=True, text=True, timeout=100)
    assert r.returncode == 0 and "CHILD_OK" in r.stdout, r.stderr[-3000:]


# ===================================================================== F: the fp32 trainer
def _planted_step(tmp_path, optimizer):
    """One step of the CPU and the HIP backend from the same planted state (test_adamw_gpu's:
    m ~ 0.01 N(0, 1), v = 1e-4 (1 + U[0, 1)), t = 100) -> the relative differences of the
    gradient-linear part of m, of v's, and of the parameter update."""
    from deep_go_amd.config import ExperimentConfig
    from deep_go_amd.data.synthetic import random_planes
    from deep_go_amd.train.backends import CPUBackend, HIPBackend
    cfg = ExperimentConfig(numLayers=4, channelSize=64, batchSize=32, validationSize=64,
                           validation_interval=10, log_interval=5, useCuda=True, synthetic=True,
                           checkpoint_dir=str(tmp_path), seed=2, loader_threads=4, prefetch=3,
                           rate=1e-3, head_relu=False, optimizer=optimizer, weight_decay=1e-2)
    cpu_be = CPUBackend(cfg, 16)
    gpu_be = HIPBackend(cfg, 16, flat=cpu_be.flat_params().clone())
    gen = torch.Generator().manual_seed(11)
    n = cpu_be.layout.numel
    m0 = torch.randn(n, generator=gen) * 0.01
    v0 = 1e-4 * (1.0 + torch.rand(n, generator=gen))
    cpu_be.opt.m.copy_(m0), cpu_be.opt.v.copy_(v0)
    cpu_be.opt.t = 100
    gpu_be.net.adam_m.copy_(m0), gpu_be.net.adam_v.copy_(v0)
    gpu_be.net.set_adam_steps(100)
    batch = random_planes(16, seed=4)
    for be in (cpu_be, gpu_be):
        be.set_batch(*batch)
        be.forward_backward()
        be.optimizer_step()
    b1, b2 = cfg.adam_beta1, cfg.adam_beta2
    dm_c, dm_g = cpu_be.opt.m - b1 * m0, gpu_be.net.adam_m.cpu() - b1 * m0
    dv_c, dv_g = cpu_be.opt.v - b2 * v0, gpu_be.net.adam_v.cpu() - b2 * v0
    relm = ((dm_c - dm_g).norm() / dm_c.norm()).item()
    relv = ((dv_c - dv_g).norm() / dv_c.norm()).item()
    p0 = CPUBackend(cfg, 16).flat_params()
    da, db = cpu_be.flat_params() - p0, gpu_be.flat_params() - p0
    relp = ((da - db).norm() / da.norm()).item()
    assert cpu_be.opt.t == gpu_be.net.adam_steps() == 101
    assert gpu_be.rate == pytest.approx(cpu_be.rate, rel=1e-12)
    phis = None
    if optimizer == "lamb":
        phis = ([s[2] for s in cpu_be.lamb_stats()], [s[2] for s in gpu_be.lamb_stats()])
    gpu_be.close()
    return relm, relv, relp, phis


def test_gpu_step_matches_cpu_step(tmp_path):
    """One step from the planted state against the fp32 CPU trainer, held to the bounds
    test_adamw_gpu.py uses for the same comparison: 0.05 / 0.10 on the gradient-linear parts of
    m / v, 0.05 on the parameter update — or, should lamb's update exceed 0.05, twice what
    adamw's differs by on the same config in this same run.  Both are printed."""
    relm, relv, relp, (phi_c, phi_g) = _planted_step(tmp_path, "lamb")
    _, _, relp_adamw, _ = _planted_step(tmp_path, "adamw")
    dphi = max(abs(a - b) / a for a, b in zip(phi_c, phi_g))
    print(f"LAMB_CPU_GPU relative difference: m part {relm:.4f}, v part {relv:.4f}, parameter "
          f"update {relp:.4f} (adamw on the same config: {relp_adamw:.4f}), trust ratios "
          f"{dphi:.5f}")
    assert relm < 0.05, relm
    assert relv < 0.10, relv
    assert relp < max(0.05, 2 * relp_adamw), (relp, relp_adamw)
