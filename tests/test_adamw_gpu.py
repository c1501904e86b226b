"""optimizer=adamw on the GPU: the kernels of csrc/kernels/optim.hip (module _dgadam) against
the float64 oracle of tests/test_adamw_cpu.py within its counted bounds, the per-element decay
mask, the count of applied steps, inside HipGoNet (eager and as step graphs, bf16 and fp8, with
the bf16 wire twin), the skip policy, exact resume and the fp32 CPU trainer.

Buffers under test, the 16-byte record {int64 t; float c1; float c2} included, sit between
sentinel runs (test_update_gpu.guarded).  The float64 references of the large vectors are
evaluated with torch on the device (one rounding per op, as on the CPU); the kernel under test
never produces them.
"""
import numpy as np
import pytest
import torch

from test_adamw_cpu import (APPLY, BETAS, EPS, adam_corrections, adamw_ref, check_adamw_step)
from test_momentum_cpu import ranges_mask
from test_momentum_gpu import _np_table, range_tables
from test_update_gpu import BIG, DEV, guarded, guards_intact, same_bits

pytestmark = pytest.mark.gpu


def _adam():
    from deep_go_amd.ops.native import adam
    return adam()


def _record(t0):
    """(whole allocation, the two int64 of the record) with t = t0, c1 = c2 = 0."""
    return guarded(torch.tensor([t0, 0], dtype=torch.int64))


def _record_values(rec):
    from deep_go_amd.ops.functional import adamw_record_values
    return adamw_record_values(rec)


def _assert_record(rec, t, tag):
    """t applied steps, and c1, c2 the float64 values rounded to fp32."""
    got = _record_values(rec)
    want = (t,) + tuple(np.float32(c) for c in adam_corrections(t, BETAS))
    assert got[0] == want[0] and np.float32(got[1]) == want[1] and \
        np.float32(got[2]) == want[2], (tag, got, want)


# ===================================================================== A: the kernel
# BIG + 1203: past sgd's 2048-block cap, 3-element tail; CAP + 1203: past this kernel's own cap
# (8192 workgroups x 256 threads x 4), where its workgroups take a second pass
CAP = 8192 * 256 * 4
SIZES = [1, 3, 4, 5, 1001, BIG + 1203, CAP + 1203]
GSCALES = [1.0, 0.37]
GATES = [None, 1.0, 0.0]
T0S = [0, 7, 10 ** 6]                  # at 10^6 both bias corrections are exactly 1
LR, WD = 0.0137, 0.05


def _launch(fn, pd, gd, md, vd, n, lrt, rec, wd, ranges, gscale, gt):
    from deep_go_amd.ops.native import stream_handle
    t = _np_table(ranges)
    fn(pd.data_ptr(), gd.data_ptr(), md.data_ptr(), vd.data_ptr(), n, lrt.data_ptr(),
       rec.data_ptr(), BETAS[0], BETAS[1], EPS, wd, t.ctypes.data if len(t) else 0, len(t),
       gscale, gt.data_ptr() if gt is not None else 0, stream_handle())
    torch.cuda.synchronize()


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("kind", ["fp32", "bf16"])
def test_adamw_matches_float64_reference(kind, n):
    """adamw / adamw_bf16 against adamw_ref over three consecutive launches (each reads the
    moments and the count the one before wrote; each is compared from the state it started
    from), for every gscale, gate, range table and starting count, within adamw_bounds.  The
    record reads t0 + the applied launches, its c1, c2 the float64 values rounded to fp32.
    gate = 0 leaves p, m, v and the record bit-identical, also under an all-NaN gradient; the
    sentinels around every buffer stay; the device lr is not written."""
    h, gen = _adam(), torch.Generator().manual_seed(500 + n % 1000)
    fn = h.adamw_bf16 if kind == "bf16" else h.adamw
    p_init = torch.randn(n, generator=gen)
    m_init = torch.randn(n, generator=gen) * 0.5
    v_init = torch.rand(n, generator=gen) * 2.0
    grads = []
    for scale in (2.0, 0.3, 1.0):
        g = torch.randn(n, generator=gen) * scale
        grads.append(g.to(torch.bfloat16) if kind == "bf16" else g)
    gdev = [guarded(g) for g in grads]
    nanbuf, nand = guarded(torch.full_like(grads[0], float("nan")))
    lrt = torch.tensor([LR], dtype=torch.float64, device=DEV)
    worst = np.zeros(3)
    for ranges in range_tables(n):
        mask = ranges_mask(n, ranges).to(DEV)
        for t0 in T0S:
            for gscale in GSCALES:
                for gate in GATES:
                    tag = (ranges, t0, gscale, gate)
                    pbuf, pd = guarded(p_init)
                    mbuf, md = guarded(m_init)
                    vbuf, vd = guarded(v_init)
                    rbuf, rec = _record(t0)
                    gt = None if gate is None else torch.tensor([gate], device=DEV)
                    t = t0
                    for g, (gbuf, gd) in zip(grads, gdev):
                        p0, m0, v0, r0 = pd.clone(), md.clone(), vd.clone(), rec.clone()
                        _launch(fn, pd, gd, md, vd, n, lrt, rec, WD, ranges, gscale, gt)
                        assert guards_intact(pbuf) and guards_intact(mbuf), tag
                        assert guards_intact(vbuf) and guards_intact(rbuf), tag
                        assert guards_intact(gbuf), tag
                        if gate == 0.0:
                            assert same_bits(pd, p0) and same_bits(md, m0), tag
                            assert same_bits(vd, v0) and same_bits(rec, r0), tag
                            continue
                        t += 1
                        _assert_record(rec, t, tag)
                        worst = np.maximum(worst, check_adamw_step(
                            p0, gd.float(), m0, v0, pd, md, vd, t, LR, BETAS, EPS, WD, mask,
                            gscale, tag))
                        assert not torch.equal(pd, p0) and not torch.equal(md, m0)
                        assert not torch.equal(vd, v0)
        # a closed gate over an all-NaN gradient
        pbuf, pd = guarded(p_init)
        mbuf, md = guarded(m_init)
        vbuf, vd = guarded(v_init)
        rbuf, rec = _record(7)
        r0 = rec.clone()
        _launch(fn, pd, nand, md, vd, n, lrt, rec, WD, ranges, 1.0, torch.zeros(1, device=DEV))
        assert same_bits(pd, p_init) and same_bits(md, m_init) and same_bits(vd, v_init)
        assert same_bits(rec, r0)
        assert guards_intact(pbuf) and guards_intact(mbuf) and guards_intact(vbuf)
        assert guards_intact(rbuf) and guards_intact(nanbuf)
    assert lrt.item() == LR
    print(f"ADAMW_ERR kind={kind} n={n} p_err_over_bound={worst[0]:.3f} "
          f"m_err_over_bound={worst[1]:.3f} v_err_over_bound={worst[2]:.3f}")


# ===================================================================== B: the mask
def test_weight_decay_mask_is_per_element():
    """g = 0, m = v = 0: one launch moves exactly the elements of the ranges — ends in the
    middle of a 4-vector, two ranges inside one workgroup pass, one range across passes and
    into the n % 4 tail — each to fp32(p fp32(1 - lr wd)) within two roundings; everything
    else keeps its bits, m and v stay zero, t advances by one."""
    from deep_go_amd.ops.functional import adamw_, adamw_record
    n = 3 * 2048 + 64 * 5 + 3
    ranges = [(0, 1), (64, 64 * 3 + 2), (64 * 4, 64 * 4 + 3), (2048 - 64, 2048 + 5),
              (2048 + 64, 2 * 2048 + 7), (3 * 2048, n)]
    mask = ranges_mask(n, ranges)
    lr, wd = 0.3, 0.1
    p_init = torch.randn(n, generator=torch.Generator().manual_seed(3)) + 3.0
    pbuf, pd = guarded(p_init)
    mbuf, md = guarded(torch.zeros(n))
    vbuf, vd = guarded(torch.zeros(n))
    gbuf, gd = guarded(torch.zeros(n))
    rec = adamw_record(0)
    lrt = torch.tensor([lr], dtype=torch.float64, device=DEV)
    adamw_(pd, gd, md, vd, lrt, rec, BETAS[0], BETAS[1], EPS, wd=wd, ranges=ranges)
    torch.cuda.synchronize()
    got = pd.cpu()
    assert torch.equal(got != p_init, mask)
    assert same_bits(got[~mask], p_init[~mask])
    dk = np.float32(1.0) - np.float32(lr) * np.float32(wd)
    want = torch.from_numpy(p_init[mask].numpy() * dk)
    assert want.dtype == torch.float32
    err = (got[mask].double() - want.double()).abs()
    assert (err <= 2 * 2.0 ** -23 * want.double().abs()).all(), err.max().item()
    assert same_bits(md, torch.zeros(n)) and same_bits(vd, torch.zeros(n))
    assert _record_values(rec)[0] == 1
    assert guards_intact(pbuf) and guards_intact(mbuf) and guards_intact(vbuf)
    assert guards_intact(gbuf)


# ===================================================================== C: applied steps
@pytest.mark.parametrize("n", [1001, CAP + 1203])
def test_bias_correction_counts_applied_launches(n):
    """test_adamw_cpu's skip pattern through the kernel with gate tensors [1, 0, 1, 1, 0, 1] and
    distinct gradients: each applied launch equals adamw_ref with t = 1, 2, 3, 4 from the state
    it started from, a gated one keeps p, m, v and the record bit for bit, and the record reads
    t = 4 after six launches.  The large size has more workgroups than are resident at once
    and a second pass: a count written and read inside one launch would show there.  With t
    taken from the launch's index the reference misses by far more than the bound."""
    fn, gen = _adam().adamw, torch.Generator().manual_seed(9)
    ranges = range_tables(n)[2]
    mask = ranges_mask(n, ranges).to(DEV)
    pbuf, pd = guarded(torch.randn(n, generator=gen))
    mbuf, md = guarded(torch.zeros(n))
    vbuf, vd = guarded(torch.zeros(n))
    rbuf, rec = _record(0)
    lrt = torch.tensor([LR], dtype=torch.float64, device=DEV)
    worst, miss, t = np.zeros(3), [], 0
    for call, apply in enumerate(APPLY, 1):
        gbuf, gd = guarded(torch.randn(n, generator=gen) * 0.1 * call)
        gt = torch.tensor([float(apply)], device=DEV)
        p0, m0, v0, r0 = pd.clone(), md.clone(), vd.clone(), rec.clone()
        _launch(fn, pd, gd, md, vd, n, lrt, rec, WD, ranges, 1.0, gt)
        if not apply:
            assert same_bits(pd, p0) and same_bits(md, m0) and same_bits(vd, v0)
            assert same_bits(rec, r0)
            continue
        t += 1
        _assert_record(rec, t, call)
        st = (p0, gd, m0, v0, pd, md, vd)
        args = (LR, BETAS, EPS, WD, mask, 1.0)
        worst = np.maximum(worst, check_adamw_step(*st, t, *args, ("applied", call)))
        if call != t:
            miss.append(check_adamw_step(*st, call, *args, ("by index", call), must_pass=False)[0])
        assert guards_intact(gbuf)
    assert _record_values(rec)[0] == 4 and len(miss) == 3 and min(miss) > 100.0
    assert guards_intact(pbuf) and guards_intact(mbuf) and guards_intact(vbuf)
    assert guards_intact(rbuf)
    print(f"ADAMW_APPLIED n={n} p/m/v error over bound "
          + " ".join(f"{x:.3f}" for x in worst)
          + " ; with t = launch index, p error over bound " + " ".join(f"{x:.0f}" for x in miss))


# ===================================================================== D: in the model
MODEL_CASES = {"3x64-bf16": (3, 64, "bf16"), "4x128-bf16": (4, 128, "bf16"),
               "4x128-fp8": (4, 128, "fp8")}
B = 8
RATE_DECAY = 1e-3


def _cfg(layers, ch, dtype, **kw):
    from deep_go_amd.config import ExperimentConfig
    base = dict(numLayers=layers, channelSize=ch, batchSize=B, seed=5, dtype=dtype, rate=1e-3,
                rateDecay=RATE_DECAY, optimizer="adamw", weight_decay=1e-2)
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
    mask = ranges_mask(net.layout.numel, net.layout.weight_ranges()).to(DEV)
    assert torch.isfinite(g).all() and g.abs().max() > 0
    betas = (cfg.adam_beta1, cfg.adam_beta2)
    got = _record_values(net.adam_t)
    want = adam_corrections(t, betas)
    assert got[0] == t == net.adam_steps() and got[1:] == want, (tag, got, want)
    return check_adamw_step(p0, g, m0, v0, net.params, net.adam_m, net.adam_v, t, lr0, betas,
                            cfg.adam_eps, cfg.weight_decay, mask, 1.0, tag)


@pytest.mark.parametrize("mode", ["eager", "graph"])
@pytest.mark.parametrize("name", list(MODEL_CASES))
def test_model_steps_match_reference(name, mode):
    """Three whole steps (eagerly; as SegmentedStep's step graph): the step is not deferred,
    params, adam_m and adam_v after each equal adamw_ref of the step's own net.grads within A's
    bounds, t = steps, lr = rate (1 - rateDecay)^t, step_count = t.  bf16: the next batch's loss
    and pred on the trained net equal those of a fresh net built from its parameters — the
    operand copies were refreshed from the updated weights."""
    from deep_go_amd.models.hip_model import HipGoNet, SegmentedStep
    layers, ch, dtype = MODEL_CASES[name]
    cfg = _cfg(layers, ch, dtype)
    net = HipGoNet(cfg, B, device="cuda")
    assert net.adam_m is not None and not net.adam_m.any() and not net.adam_v.any()
    assert net.adam_steps() == 0 and net.ms is None and net.vel is None
    assert not net.can_defer()
    net.set_batch(*_batch(B, 12))
    step = SegmentedStep(net, None, use_graphs=(mode == "graph"))
    assert (step.full_graph is not None) == (mode == "graph")
    assert net.adam_steps() == 0       # (no warm-up or capture has counted)
    worst = np.zeros(3)
    for t in range(1, 4):
        torch.cuda.synchronize()
        state = _state(net)
        step()
        torch.cuda.synchronize()
        assert int(net.bad_steps.item()) == 0 and net.gate.item() == 1.0
        worst = np.maximum(worst, _check_model_step(net, state, t, net.grads, (name, t)))
        assert net.lr.item() == pytest.approx(cfg.rate * (1.0 - RATE_DECAY) ** t, rel=1e-13)
        assert int(net.step_count.item()) == t
        assert not torch.equal(net.params, state[0]) and not torch.equal(net.adam_m, state[1])
    print(f"ADAMW_ERR model name={name} mode={mode} p/m/v error over bound "
          + " ".join(f"{x:.3f}" for x in worst))
    if dtype == "bf16":
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
    cfg = _cfg(3, 64, "bf16", nan_policy="raise")
    net = HipGoNet(cfg, B, device="cuda")
    net.set_batch(*_batch(B, 12))
    net.gate.zero_()                    # (nothing may read it)
    for t in range(1, 3):
        state = _state(net)
        net.train_step()
        torch.cuda.synchronize()
        _check_model_step(net, state, t, net.grads, ("raise", t))
        assert int(net.step_count.item()) == t and net.gate.item() == 0.0


# ===================================================================== E: skip
def test_skipped_steps_do_not_count():
    """nan_policy=skip: a clean step, then a poisoned gradient entry, then a poisoned loss:
    params, both moments, the record and the operand copies keep their bits; bad_steps = 2,
    step_count = 3, t = 1, the rate decayed twice.  The next clean step matches the reference
    with t = 2 — and not with t = 4, the step's number."""
    from deep_go_amd.models.hip_model import HipGoNet
    cfg = _cfg(4, 128, "bf16", nan_policy="skip")
    net = HipGoNet(cfg, B, device="cuda")
    net.set_batch(*_batch(B, 8))
    net.forward_backward()
    net.optimizer_step()                # a clean step: the moments are no longer zero
    net.forward_backward()
    torch.cuda.synchronize()
    p0, m0, v0, lr0 = _state(net)
    r0 = net.adam_t.clone()
    wf0 = [w.clone() for w in net.wf]
    assert m0.abs().max() > 0 and v0.abs().max() > 0 and net.bad_steps.item() == 0
    assert net.adam_steps() == 1

    def unchanged():
        return (same_bits(net.params, p0) and same_bits(net.adam_m, m0)
                and same_bits(net.adam_v, v0) and same_bits(net.adam_t, r0)
                and all(torch.equal(a, b) for a, b in zip(net.wf, wf0)))
    net.grads[17] = float("nan")
    net.optimizer_step()
    torch.cuda.synchronize()
    assert unchanged()
    assert net.bad_steps.item() == 1 and net.gate.item() == 0.0
    assert net.lr.item() == pytest.approx(lr0 * (1.0 - RATE_DECAY), rel=1e-13)
    net.forward_backward()
    net.loss[0] = float("inf")
    net.optimizer_step()
    torch.cuda.synchronize()
    assert unchanged()
    assert net.bad_steps.item() == 2 and int(net.step_count.item()) == 3
    assert net.adam_steps() == 1
    assert net.lr.item() == pytest.approx(lr0 * (1.0 - RATE_DECAY) ** 2, rel=1e-13)
    net.forward_backward()
    torch.cuda.synchronize()
    state = _state(net)
    net.optimizer_step()
    torch.cuda.synchronize()
    assert net.gate.item() == 1.0 and net.bad_steps.item() == 2
    assert int(net.step_count.item()) == 4
    w = _check_model_step(net, state, 2, net.grads, "after the skips")
    mask = ranges_mask(net.layout.numel, net.layout.weight_ranges()).to(DEV)
    miss = check_adamw_step(state[0], net.grads, state[1], state[2], net.params, net.adam_m,
                            net.adam_v, 4, state[3], (cfg.adam_beta1, cfg.adam_beta2),
                            cfg.adam_eps, cfg.weight_decay, mask, 1.0, "t = 4",
                            must_pass=False)[0]
    print(f"ADAMW_ERR skip p/m/v error over bound " + " ".join(f"{x:.3f}" for x in w)
          + f" ; against t = 4: {miss:.0f}")
    assert miss > 100.0


# ===================================================================== F: bf16 wire
def test_bf16_wire_step_reads_the_twin():
    from deep_go_amd.models.hip_model import HipGoNet
    cfg = _cfg(4, 128, "bf16")
    net = HipGoNet(cfg, B, device="cuda", global_batch=2 * B, grad_wire="bf16")
    assert net.grads16 is not None and not net.can_defer()
    net.set_batch(*_batch(B, 9))
    state = _state(net)
    net.forward_backward()
    net.optimizer_step()
    torch.cuda.synchronize()
    assert torch.equal(net.grads16, net.grads.to(torch.bfloat16))
    assert not torch.equal(net.grads16.float(), net.grads)
    w = _check_model_step(net, state, 1, net.grads16.float(), "wire")
    print("ADAMW_ERR model wire p/m/v error over bound " + " ".join(f"{x:.3f}" for x in w))
    assert int(net.bad_steps.item()) == 0 and int(net.step_count.item()) == 1


# ===================================================================== G: resume
def test_hip_backend_resume_is_exact(tmp_path):
    """With the second step skipped: 4 steps == 2 steps + state_dict -> a new backend +
    load_state_dict + 2 steps, bit for bit on params and both moments, t equal (3, not 4); a
    state without moments loads zeros and t = 0."""
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
    assert o["kind"] == "adamw" and type(o["adam_t"]) is int and o["adam_t"] == 1
    assert o["adam_m"].abs().max() > 0 and o["adam_v"].abs().max() > 0
    c = HIPBackend(cfg, 4, flat=b.flat_params())
    c.load_state_dict(sd)
    assert torch.equal(c.net.adam_m.cpu(), o["adam_m"]) and c.rate == b.rate
    assert c.net.adam_steps() == 1
    run(c, range(2, 4))
    assert torch.equal(c.net.params, a.net.params)
    assert torch.equal(c.net.adam_m, a.net.adam_m) and torch.equal(c.net.adam_v, a.net.adam_v)
    assert c.net.adam_steps() == a.net.adam_steps() == 3 and c.rate == a.rate
    old = {"optimizer": {k: v for k, v in o.items() if not k.startswith("adam_")}}
    c.load_state_dict(old)
    assert not c.net.adam_m.any() and not c.net.adam_v.any() and c.net.adam_steps() == 0
    assert c.rate == b.rate
    for be in (a, b, c):
        be.close()


# ===================================================================== H: the fp32 trainer
def test_gpu_step_matches_cpu_step(tmp_path):
    """test_momentum_gpu.test_gpu_step_matches_cpu_step's set-up with optimizer=adamw and the
    same state planted on both backends: m ~ 0.01 N(0, 1), v = 1e-4 (1 + U[0, 1)), t = 100.  (A
    first step from zero state is lr g / (|g| + eps): it flips sign with the bf16 gradient's
    noise on tiny entries and measures nothing.)  The gradient-linear parts inherit the
    existing test's tolerance: m1 - beta1 m0 differs by < 0.05 relative, v1 - beta2 v0 —
    quadratic in g — by < 0.10; t and the rate are equal.  The parameter update's relative
    difference is printed, without a pass mark."""
    from deep_go_amd.config import ExperimentConfig
    from deep_go_amd.data.synthetic import random_planes
    from deep_go_amd.train.backends import CPUBackend, HIPBackend
    cfg = ExperimentConfig(numLayers=4, channelSize=64, batchSize=32, validationSize=64,
                           validation_interval=10, log_interval=5, useCuda=True, synthetic=True,
                           checkpoint_dir=str(tmp_path), seed=2, loader_threads=4, prefetch=3,
                           rate=1e-3, head_relu=False, optimizer="adamw", weight_decay=1e-2)
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
    print(f"ADAMW_CPU_GPU relative difference: m part {relm:.4f}, v part {relv:.4f}, "
          f"parameter update {relp:.4f} (no pass mark)")
    assert relm < 0.05, relm
    assert relv < 0.10, relv
    assert cpu_be.opt.t == gpu_be.net.adam_steps() == 101
    assert gpu_be.rate == pytest.approx(cpu_be.rate, rel=1e-12)
    gpu_be.close()
