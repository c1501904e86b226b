"""optimizer=momentum on the GPU: the kernel of csrc/kernels/optim.hip (module _dgopt) against
the float64 oracle of tests/test_momentum_cpu.py, bit-exactly on designed data, inside HipGoNet
(eager and as step graphs, bf16 and fp8, with the bf16 wire twin), the skip policy, exact
resume and the fp32 CPU trainer.

Buffers under test sit between sentinel runs (test_update_gpu.guarded).  The float64 references
of the large vectors are evaluated with torch on the device (one rounding per op, as on the
CPU); the kernel under test never produces them.
"""
import numpy as np
import pytest
import torch

from test_momentum_cpu import exact_case, momentum_ref, ranges_mask
from test_update_gpu import BIG, DEV, guarded, guards_intact, same_bits

pytestmark = pytest.mark.gpu

U24 = 2.0 ** -24


def _opt():
    from deep_go_amd.ops.native import opt
    return opt()


def momentum_bounds(p0, g, v0, pr, vr, lr, mu, nesterov, wd, mask, gscale):
    """The fp32 roundings counted as sgd_bound counts them, then doubled.  v = mu v0 + gi +
    wd p takes at most 4 (the two products, the two sums; gi's own when gscale != 1 is the
    fourth): 2 * 4 * 2^-24 (|mu v0| + |gi| + |wd p|).  p = p - lr u takes one for the product
    and one for the difference, 2^-23 (|p_ref| + |lr u|), on top of lr times v's bound — times
    (1 + mu) under Nesterov, where u = gw + mu v carries gw's error (below v's) as well."""
    l, m, w, s = (float(np.float32(x)) for x in (lr, mu, wd, gscale))
    gi = g.double() * s
    wp = w * mask.double() * p0.double()
    bv = 2 * 4 * U24 * ((m * v0.double()).abs() + gi.abs() + wp.abs())
    gw = gi + wp
    u = gw + m * vr if nesterov else vr
    bp = 2 * U24 * (pr.abs() + (l * u).abs()) + l * bv * (1 + m if nesterov else 1)
    return bp, bv


def check_step(p0, g, v0, p1, v1, lr, mu, nesterov, wd, mask, gscale, tag):
    """(p1, v1) against momentum_ref from (p0, v0); -> the largest error / bound of (p, v)."""
    pr, vr = momentum_ref(p0, g, v0, lr, mu, nesterov, wd, mask, gscale)
    bp, bv = momentum_bounds(p0, g, v0, pr, vr, lr, mu, nesterov, wd, mask, gscale)
    ep, ev = (p1.double() - pr).abs(), (v1.double() - vr).abs()
    rp = (ep / bp.clamp_min(1e-300)).max().item()
    rv = (ev / bv.clamp_min(1e-300)).max().item()
    assert (ev <= bv).all(), (tag, "v error / bound", rv, int((ev - bv).argmax()))
    assert (ep <= bp).all(), (tag, "p error / bound", rp, int((ep - bp).argmax()))
    return np.array([rp, rv])


# ===================================================================== A: the kernel
# BIG + 1203: past sgd's 2048-block cap, 3-element tail; CAP + 1203: past this kernel's own cap
# (8192 workgroups x 256 threads x 4), where its workgroups take a second pass
CAP = 8192 * 256 * 4
SIZES = [1, 3, 4, 5, 1001, BIG + 1203, CAP + 1203]
GSCALES = [1.0, 0.37]
GATES = [None, 1.0, 0.0]
LR, MU, WD = 0.0137, 0.9, 0.05


def range_tables(n):
    """No range; [0, 7); [0, 64 k + 1) and a second range from a later multiple of 64 to n —
    each clipped to what fits n."""
    tables = [[], [(0, min(7, n))]]
    if n > 64 * 8:
        k = max(3, n // 2048)            # (n = 1001: both ranges inside one workgroup pass)
        b2 = (n * 5 // 8) // 64 * 64
        tables.append([(0, 64 * k + 1), (b2, n)])
        assert 64 * k + 1 < b2 < n
    else:
        tables.append([(0, n)])
    return tables


def _np_table(ranges):
    return np.ascontiguousarray(np.array(ranges, dtype=np.int64).reshape(-1, 2))


def _launch(fn, pd, gd, vd, n, lrt, mu, nes, wd, ranges, gscale, gt):
    from deep_go_amd.ops.native import stream_handle
    t = _np_table(ranges)
    fn(pd.data_ptr(), gd.data_ptr(), vd.data_ptr(), n, lrt.data_ptr(), mu, int(nes), wd,
       t.ctypes.data if len(t) else 0, len(t), gscale, gt.data_ptr() if gt is not None else 0,
       stream_handle())
    torch.cuda.synchronize()


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("kind", ["fp32", "bf16"])
def test_momentum_matches_float64_reference(kind, n):
    """momentum / momentum_bf16 against momentum_ref over two consecutive steps (the second
    reads the velocity the first wrote; each is compared from the state it started from), for
    every gscale, gate, nesterov setting and range table, within momentum_bounds.  gate = 0
    leaves p and v bit-identical, also under an all-NaN gradient; the sentinels around every
    buffer stay; the device lr is not written.

    Measured on an MI355X (the largest figures, at n >= 2 098 355): v's error reaches 0.25 of
    its bound with fp32 gradients and 0.27 with bf16 — two of the eight counted half-ulps; p's
    reaches 0.496 of its bound, which is the final rounding of p alone (half an ulp of p
    against the doubled 2^-23 |p| term): the update's own error is far below it."""
    h, gen = _opt(), torch.Generator().manual_seed(300 + n % 1000)
    fn = h.momentum_bf16 if kind == "bf16" else h.momentum
    p_init = torch.randn(n, generator=gen)
    v_init = torch.randn(n, generator=gen) * 3.0
    grads = []
    for scale in (2.0, 0.3):
        g = torch.randn(n, generator=gen) * scale
        grads.append(g.to(torch.bfloat16) if kind == "bf16" else g)
    gdev = [guarded(g) for g in grads]
    nanbuf, nand = guarded(torch.full_like(grads[0], float("nan")))
    lrt = torch.tensor([LR], dtype=torch.float64, device=DEV)
    worst = np.zeros(2)
    for ranges in range_tables(n):
        mask = ranges_mask(n, ranges).to(DEV)
        for nes in (False, True):
            for gscale in GSCALES:
                for gate in GATES:
                    tag = (ranges, nes, gscale, gate)
                    pbuf, pd = guarded(p_init)
                    vbuf, vd = guarded(v_init)
                    gt = None if gate is None else torch.tensor([gate], device=DEV)
                    for g, (gbuf, gd) in zip(grads, gdev):
                        p0, v0 = pd.clone(), vd.clone()
                        _launch(fn, pd, gd, vd, n, lrt, MU, nes, WD, ranges, gscale, gt)
                        assert guards_intact(pbuf) and guards_intact(vbuf), tag
                        assert guards_intact(gbuf), tag
                        if gate == 0.0:
                            assert same_bits(pd, p0) and same_bits(vd, v0), tag
                            continue
                        worst = np.maximum(worst, check_step(
                            p0, gd.float(), v0, pd, vd, LR, MU, nes, WD, mask, gscale, tag))
                        assert not torch.equal(pd, p0) and not torch.equal(vd, v0)
        # a closed gate over an all-NaN gradient
        pbuf, pd = guarded(p_init)
        vbuf, vd = guarded(v_init)
        _launch(fn, pd, nand, vd, n, lrt, MU, True, WD, ranges, 1.0, torch.zeros(1, device=DEV))
        assert same_bits(pd, p_init) and same_bits(vd, v_init)
        assert guards_intact(pbuf) and guards_intact(vbuf) and guards_intact(nanbuf)
    assert lrt.item() == LR
    print(f"MOMENTUM_ERR kind={kind} n={n} p_err_over_bound={worst[0]:.3f} "
          f"v_err_over_bound={worst[1]:.3f}")


def test_weight_decay_mask_is_per_element():
    """g = 0, v = 0: one step moves exactly the elements of the ranges — ends in the middle
    of a 4-vector, two ranges inside one workgroup pass, one range across passes and into
    the n % 4 tail."""
    from deep_go_amd.ops.functional import momentum_
    n = 3 * 2048 + 64 * 5 + 3
    ranges = [(0, 1), (64, 64 * 3 + 2), (64 * 4, 64 * 4 + 3), (2048 - 64, 2048 + 5),
              (2048 + 64, 2 * 2048 + 7), (3 * 2048, n)]
    mask = ranges_mask(n, ranges)
    pbuf, pd = guarded(torch.full((n,), 0.75))
    vbuf, vd = guarded(torch.zeros(n))
    gbuf, gd = guarded(torch.zeros(n))
    lrt = torch.tensor([0.5], dtype=torch.float64, device=DEV)
    momentum_(pd, gd, vd, lrt, 0.5, nesterov=False, wd=0.25, ranges=ranges)
    torch.cuda.synchronize()
    assert torch.equal(pd.cpu() != 0.75, mask)
    assert torch.equal(vd.cpu() != 0, mask)
    assert guards_intact(pbuf) and guards_intact(vbuf) and guards_intact(gbuf)


# ===================================================================== B: exact
@pytest.mark.parametrize("nesterov", [False, True])
@pytest.mark.parametrize("kind", ["fp32", "bf16"])
def test_exact_data_is_bit_exact(kind, nesterov):
    """exact_case at n = 64 * 37 + 3 with two ranges that end inside a 4-vector: p and v after
    one step equal the float64 reference cast to fp32, every element — those on either side
    of each range boundary among them, so a mask off by one fails."""
    h = _opt()
    fn = h.momentum_bf16 if kind == "bf16" else h.momentum
    n = 64 * 37 + 3
    ranges = [(0, 64 * 9 + 1), (64 * 20, 64 * 30 + 2)]
    mask = ranges_mask(n, ranges)
    for seed in range(3):
        p, g, v, c = exact_case(n, seed)
        pr, vr = momentum_ref(p, g, v, c["lr"], c["mu"], nesterov, c["wd"], mask)
        assert torch.equal(pr.float().double(), pr) and torch.equal(vr.float().double(), vr)
        gk = g.to(torch.bfloat16) if kind == "bf16" else g
        assert torch.equal(gk.float(), g)
        pbuf, pd = guarded(p)
        vbuf, vd = guarded(v)
        gbuf, gd = guarded(gk)
        lrt = torch.tensor([c["lr"]], dtype=torch.float64, device=DEV)
        _launch(fn, pd, gd, vd, n, lrt, c["mu"], nesterov, c["wd"], ranges, 1.0, None)
        bad = (pd.cpu() != pr.float()).nonzero().reshape(-1)
        assert bad.numel() == 0, ("p", bad[:8].tolist())
        bad = (vd.cpu() != vr.float()).nonzero().reshape(-1)
        assert bad.numel() == 0, ("v", bad[:8].tolist())
        for b, e in ranges:        # (the designed data moves both sides of each boundary)
            assert (pr[e - 1] != p[e - 1]) or (vr[e - 1] != v[e - 1])
        assert guards_intact(pbuf) and guards_intact(vbuf) and guards_intact(gbuf)


# ===================================================================== C: in the model
MODEL_CASES = {"3x64-bf16": (3, 64, "bf16"), "4x128-bf16": (4, 128, "bf16"),
               "4x128-fp8": (4, 128, "fp8")}
B = 8
RATE_DECAY = 1e-3


def _cfg(layers, ch, dtype, **kw):
    from deep_go_amd.config import ExperimentConfig
    base = dict(numLayers=layers, channelSize=ch, batchSize=B, seed=5, dtype=dtype,
                rateDecay=RATE_DECAY, optimizer="momentum", momentum=0.9, nesterov=True,
                weight_decay=1e-3)
    base.update(kw)
    return ExperimentConfig(**base)


def _batch(n, seed):
    from deep_go_amd.data.synthetic import random_planes
    return [torch.from_numpy(a).cuda() for a in random_planes(n, seed=seed)]


def _check_model_step(net, p0, v0, lr0, g, tag):
    cfg = net.cfg
    mask = ranges_mask(net.layout.numel, net.layout.weight_ranges()).to(DEV)
    assert torch.isfinite(g).all() and g.abs().max() > 0
    return check_step(p0, g, v0, net.params, net.vel, lr0, cfg.momentum, cfg.nesterov,
                      cfg.weight_decay, mask, 1.0, tag)


@pytest.mark.parametrize("mode", ["eager", "graph"])
@pytest.mark.parametrize("name", list(MODEL_CASES))
def test_model_steps_match_reference(name, mode):
    """Three whole steps (eagerly; as SegmentedStep's step graph): the step is not deferred,
    params and vel after each equal momentum_ref of the step's own net.grads within A's
    bounds, lr = rate (1 - rateDecay)^t, step_count = t.  bf16: the next batch's loss and
    pred on the trained net equal those of a fresh net built from its parameters — the
    operand copies were refreshed from the updated weights."""
    from deep_go_amd.models.hip_model import HipGoNet, SegmentedStep
    layers, ch, dtype = MODEL_CASES[name]
    cfg = _cfg(layers, ch, dtype, nesterov=(mode == "graph"))
    net = HipGoNet(cfg, B, device="cuda")
    assert net.vel is not None and not net.vel.any() and net.ms is None
    assert not net.can_defer()
    net.set_batch(*_batch(B, 12))
    step = SegmentedStep(net, None, use_graphs=(mode == "graph"))
    assert (step.full_graph is not None) == (mode == "graph")
    worst = np.zeros(2)
    for t in range(1, 4):
        torch.cuda.synchronize()
        p0, v0, lr0 = net.params.clone(), net.vel.clone(), net.lr.item()
        step()
        torch.cuda.synchronize()
        assert int(net.bad_steps.item()) == 0 and net.gate.item() == 1.0
        worst = np.maximum(worst, _check_model_step(net, p0, v0, lr0, net.grads, (name, t)))
        assert net.lr.item() == pytest.approx(cfg.rate * (1.0 - RATE_DECAY) ** t, rel=1e-13)
        assert int(net.step_count.item()) == t
        assert not torch.equal(net.params, p0) and not torch.equal(net.vel, v0)
    print(f"MOMENTUM_ERR model name={name} mode={mode} p_err_over_bound={worst[0]:.3f} "
          f"v_err_over_bound={worst[1]:.3f}")
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
        p0, v0, lr0 = net.params.clone(), net.vel.clone(), net.lr.item()
        net.train_step()
        torch.cuda.synchronize()
        _check_model_step(net, p0, v0, lr0, net.grads, ("raise", t))
        assert int(net.step_count.item()) == t and net.gate.item() == 0.0


# ===================================================================== D: skip
def test_skipped_step_leaves_parameters_and_velocity():
    """nan_policy=skip: a poisoned gradient entry, then a poisoned loss: params and vel keep
    their bits, the step is counted and the rate decays; the next clean step moves both."""
    from deep_go_amd.models.hip_model import HipGoNet
    cfg = _cfg(4, 128, "bf16", nan_policy="skip")
    net = HipGoNet(cfg, B, device="cuda")
    net.set_batch(*_batch(B, 8))
    net.forward_backward()
    net.optimizer_step()                # a clean step: the velocity is no longer zero
    net.forward_backward()
    torch.cuda.synchronize()
    p0, v0, lr0 = net.params.clone(), net.vel.clone(), net.lr.item()
    wf0 = [w.clone() for w in net.wf]
    assert v0.abs().max() > 0 and net.bad_steps.item() == 0
    net.grads[17] = float("nan")
    net.optimizer_step()
    torch.cuda.synchronize()
    assert same_bits(net.params, p0) and same_bits(net.vel, v0)
    assert all(torch.equal(a, b) for a, b in zip(net.wf, wf0))
    assert net.bad_steps.item() == 1 and net.gate.item() == 0.0
    assert net.lr.item() == pytest.approx(lr0 * (1.0 - RATE_DECAY), rel=1e-13)
    net.forward_backward()
    net.loss[0] = float("inf")
    net.optimizer_step()
    torch.cuda.synchronize()
    assert same_bits(net.params, p0) and same_bits(net.vel, v0)
    assert net.bad_steps.item() == 2 and int(net.step_count.item()) == 3
    assert net.lr.item() == pytest.approx(lr0 * (1.0 - RATE_DECAY) ** 2, rel=1e-13)
    net.forward_backward()
    net.optimizer_step()
    torch.cuda.synchronize()
    assert net.gate.item() == 1.0 and net.bad_steps.item() == 2
    assert not torch.equal(net.params, p0) and not torch.equal(net.vel, v0)
    assert torch.isfinite(net.params).all() and torch.isfinite(net.vel).all()


# ===================================================================== E: bf16 wire
def test_bf16_wire_step_reads_the_twin():
    from deep_go_amd.models.hip_model import HipGoNet
    cfg = _cfg(4, 128, "bf16")
    net = HipGoNet(cfg, B, device="cuda", global_batch=2 * B, grad_wire="bf16")
    assert net.grads16 is not None and not net.can_defer()
    net.set_batch(*_batch(B, 9))
    p0, v0, lr0 = net.params.clone(), net.vel.clone(), net.lr.item()
    net.forward_backward()
    net.optimizer_step()
    torch.cuda.synchronize()
    assert torch.equal(net.grads16, net.grads.to(torch.bfloat16))
    assert not torch.equal(net.grads16.float(), net.grads)
    w = _check_model_step(net, p0, v0, lr0, net.grads16.float(), "wire")
    print(f"MOMENTUM_ERR model wire p_err_over_bound={w[0]:.3f} v_err_over_bound={w[1]:.3f}")
    assert int(net.bad_steps.item()) == 0 and int(net.step_count.item()) == 1


# ===================================================================== F: resume
def test_hip_backend_resume_is_exact(tmp_path):
    """4 steps == 2 steps + state_dict -> a new backend + load_state_dict + 2 steps; a state
    without a velocity loads with zeros."""
    from deep_go_amd.data.synthetic import random_planes
    from deep_go_amd.train.backends import HIPBackend
    cfg = _cfg(3, 64, "bf16", batchSize=4, checkpoint_dir=str(tmp_path))
    batches = [random_planes(4, seed=20 + i) for i in range(4)]

    def run(be, which):
        for i in which:
            be.set_batch(*batches[i])
            be.train_step()
        torch.cuda.synchronize()

    a = HIPBackend(cfg, 4)
    p_init = a.flat_params().clone()
    run(a, range(4))
    b = HIPBackend(cfg, 4, flat=p_init)
    run(b, range(2))
    sd = b.state_dict()
    assert sd["optimizer"]["kind"] == "momentum" and sd["optimizer"]["vel"].abs().max() > 0
    c = HIPBackend(cfg, 4, flat=b.flat_params())
    c.load_state_dict(sd)
    assert torch.equal(c.net.vel.cpu(), sd["optimizer"]["vel"]) and c.rate == b.rate
    run(c, range(2, 4))
    assert torch.equal(c.net.params, a.net.params) and torch.equal(c.net.vel, a.net.vel)
    assert c.rate == a.rate
    old = {"optimizer": {k: v for k, v in sd["optimizer"].items() if k != "vel"}}
    c.load_state_dict(old)
    assert not c.net.vel.any() and c.rate == b.rate
    for be in (a, b, c):
        be.close()


# ===================================================================== G: the fp32 trainer
def test_gpu_step_matches_cpu_step(tmp_path):
    """test_train_gpu.test_gpu_step_matches_cpu_step's set-up and tolerance with
    optimizer=momentum, weight decay, Nesterov and the same random velocity planted on both
    backends before the step: relative update difference < 0.05."""
    from deep_go_amd.config import ExperimentConfig
    from deep_go_amd.data.synthetic import random_planes
    from deep_go_amd.train.backends import CPUBackend, HIPBackend
    cfg = ExperimentConfig(numLayers=4, channelSize=64, batchSize=32, validationSize=64,
                           validation_interval=10, log_interval=5, useCuda=True, synthetic=True,
                           checkpoint_dir=str(tmp_path), seed=2, loader_threads=4, prefetch=3,
                           rate=0.05, head_relu=False, optimizer="momentum", momentum=0.9,
                           nesterov=True, weight_decay=1e-3)
    cpu_be = CPUBackend(cfg, 16)
    gpu_be = HIPBackend(cfg, 16, flat=cpu_be.flat_params().clone())
    vel = torch.randn(cpu_be.layout.numel, generator=torch.Generator().manual_seed(11)) * 0.01
    cpu_be.opt.vel.copy_(vel)
    gpu_be.net.vel.copy_(vel)
    batch = random_planes(16, seed=4)
    for be in (cpu_be, gpu_be):
        be.set_batch(*batch)
        be.forward_backward()
        be.optimizer_step()
    a = cpu_be.flat_params()
    b = gpu_be.flat_params()
    p0 = CPUBackend(cfg, 16).flat_params()
    da, db = a - p0, b - p0
    rel = (da - db).norm() / da.norm()
    print(f"MOMENTUM_CPU_GPU relative update difference {rel.item():.4f}")
    assert rel < 0.05, rel.item()
    relv = (cpu_be.opt.vel - gpu_be.net.vel.cpu()).norm() / cpu_be.opt.vel.norm()
    assert relv < 0.05, relv.item()
    assert gpu_be.rate == pytest.approx(cpu_be.rate, rel=1e-12)
    gpu_be.close()
