"""optimizer=adamw without a GPU: the config, the float64 oracle ``adamw_ref`` (checked against
``torch.optim.AdamW``), the counted fp32 bounds, the CPU optimizer, the count of APPLIED steps,
exact resume on the CPU backend, the argument checks of the ``_dgadam`` launcher and two gloo
ranks.

The definition (train/optim.py AdamW), per flat element, with m = v = 0 and t = 0 at the start,
only when the step is applied:

    t += 1;  c1 = 1 / (1 - beta1^t);  c2 = 1 / sqrt(1 - beta2^t)        (double, then fp32)
    gi = g * gscale
    m  = beta1 m + (1 - beta1) gi;   v = beta2 v + (1 - beta2) gi^2
    p  = p (1 - lr wd) on the conv weights
    p -= (lr c1) m / (sqrt(v) c2 + eps)

A skipped step leaves p, m, v and t alone and still decays the rate.

tests/test_adamw_gpu.py imports ``adamw_ref``, ``adamw_bounds``, ``check_adamw_step`` and the
skip pattern from here.
"""
import math
import os

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from deep_go_amd.config import ExperimentConfig
from deep_go_amd.train.optim import AdamW
from test_dist_cpu import _free_port
from test_momentum_cpu import BAD_RANGES, _table, ranges_mask

U24 = 2.0 ** -24
# the documented error, in ulps, of the square root and the division the kernel uses: plain
# sqrtf and `/`, which clang compiles correctly rounded for HIP by default (the kernel's ISA
# has the v_div_scale / v_div_fmas / v_div_fixup sequence and v_sqrt_f32 with its two fma
# corrections), as are torch's on the CPU.  adamw_bounds doubles them with everything else.
SQRT_ULPS = 0.5
DIV_ULPS = 0.5
BETAS, EPS = (0.9, 0.999), 1e-8


def _f32(x) -> float:
    return float(np.float32(x))


# ------------------------------------------------------------------------------ oracle
def adam_corrections(t: int, betas, c32: bool = True):
    """(c1, c2) of applied step t from the fp32 betas, in double; c32: rounded to fp32, as
    the device record and train/optim.py keep them."""
    b1, b2 = _f32(betas[0]), _f32(betas[1])
    c1 = 1.0 / (1.0 - b1 ** t)
    c2 = 1.0 / math.sqrt(1.0 - b2 ** t)
    return (_f32(c1), _f32(c2)) if c32 else (c1, c2)


def adamw_ref(p, g, m, v, t: int, lr: float, betas, eps: float, wd: float, mask,
              gscale: float = 1.0, c32: bool = True):
    """Applied step number t (1 for the first) in float64 with the fp32 constants float32(lr),
    float32(beta), float32(eps), float32(wd), float32(gscale) (as momentum_ref rounds its
    constants); 1 - beta is exact.  mask: bool per element, True where weight decay applies.
    c32=False keeps the bias corrections in double (for the comparison with torch).
    Returns (p, m, v)."""
    l, b1, b2, e, w, s = (_f32(x) for x in (lr, betas[0], betas[1], eps, wd, gscale))
    c1, c2 = adam_corrections(t, betas, c32)
    gi = g.double() * s
    mn = b1 * m.double() + (1.0 - b1) * gi
    vn = b2 * v.double() + (1.0 - b2) * gi * gi
    pd = p.double() * (1.0 - l * w * mask.double())
    return pd - (l * c1) * mn / (vn.sqrt() * c2 + e), mn, vn


def adamw_bounds(p0, g, m0, v0, pr, mr, vr, t, lr, betas, eps, wd, mask, gscale):
    """The fp32 roundings (2^-24 relative each) counted as momentum_bounds counts them, then
    doubled.  -> (bp, bm, bv), absolute.

    m = b1 m0 + o1 gi: four (the two products, the sum, gi's own when gscale != 1), absolute
      in |b1 m0| + |o1 gi| because the sum may cancel.
    v = b2 v0 + (o2 gi) gi: six (gi's own counts twice, the three products, the sum) on a sum of
      non-negative terms, so relative to v.
    u = (lc m) / (sqrt(v) c2 + eps), lc = l c1: relative 7 + 2 (SQRT_ULPS + DIV_ULPS) — lc, lc m,
      half of v's six through the root, the root's and the quotient's own error (an ulp is at
      most 2^-23 relative), the product with c2 and the sum with eps (both terms positive) —
      plus m's absolute bound times lc / denominator.
    p = p0 (1 - l wd) - u: on the decayed elements three on |p0| (l wd and 1 - l wd, each
      below one rounding of 1; the product); the final difference's rounding on |p|; u's
      bound."""
    l, b1, b2, e, w, s = (_f32(x) for x in (lr, betas[0], betas[1], eps, wd, gscale))
    c1, c2 = adam_corrections(t, betas)
    gi = g.double() * s
    bm = 2 * 4 * U24 * ((b1 * m0.double()).abs() + ((1.0 - b1) * gi).abs())
    bv = 2 * 6 * U24 * vr
    den = vr.sqrt() * c2 + e
    u = (l * c1) * mr / den
    bu = 2 * (7 + 2 * (SQRT_ULPS + DIV_ULPS)) * U24 * u.abs() + (l * c1) / den * bm
    bp = 2 * U24 * (3 * mask.double() * p0.double().abs() + pr.abs()) + bu
    return bp, bm, bv


def check_adamw_step(p0, g, m0, v0, p1, m1, v1, t, lr, betas, eps, wd, mask, gscale, tag,
                     must_pass: bool = True):
    """(p1, m1, v1) against adamw_ref (applied step t) from (p0, m0, v0); -> the largest
    error / bound of (p, m, v).  must_pass=False only measures."""
    pr, mr, vr = adamw_ref(p0, g, m0, v0, t, lr, betas, eps, wd, mask, gscale)
    bp, bm, bv = adamw_bounds(p0, g, m0, v0, pr, mr, vr, t, lr, betas, eps, wd, mask, gscale)
    out = []
    for name, got, ref, b in (("p", p1, pr, bp), ("m", m1, mr, bm), ("v", v1, vr, bv)):
        err = (got.double() - ref).abs()
        # (a zero bound belongs to an exact result: 0 / 0 counts as 0, anything else as inf)
        ratio = torch.where(err == 0, torch.zeros_like(err), err / b.clamp_min(1e-300))
        r = ratio.max().item()
        out.append(r)
        if must_pass:
            assert (err <= b).all(), (tag, name + " error / bound", r, int(ratio.argmax()))
    return np.array(out)


# the skip pattern of the applied-steps tests: call k is applied where APPLY[k - 1] is 1
APPLY = [1, 0, 1, 1, 0, 1]


# ------------------------------------------------------------------------------ 1: config
def test_config_accepts_adamw_and_rejects_misuse():
    cfg = ExperimentConfig().replace(optimizer="adamw", adam_beta1="0.8", adam_beta2="0.99",
                                     adam_eps="1e-6", weight_decay="1e-2")
    assert (cfg.optimizer, cfg.adam_beta1, cfg.adam_beta2, cfg.adam_eps, cfg.weight_decay) == (
        "adamw", 0.8, 0.99, 1e-6, 1e-2)
    assert ExperimentConfig.from_dict(cfg.to_dict()) == cfg
    d = ExperimentConfig().to_dict()
    for k in ("adam_beta1", "adam_beta2", "adam_eps"):
        del d[k]                       # an older checkpoint's config
    old = ExperimentConfig.from_dict(d)
    assert (old.optimizer, old.adam_beta1, old.adam_beta2, old.adam_eps) == (
        "sgd", 0.9, 0.999, 1e-8)
    # adamw with weight_decay = 0 is Adam; beta = 0 is in range
    assert ExperimentConfig().replace(optimizer="adamw", adam_beta1=0.0).weight_decay == 0.0
    base = ExperimentConfig()
    for kw in (dict(optimizer="adamw", adam_beta1=1.0), dict(optimizer="adamw", adam_beta1=-0.1),
               dict(optimizer="adamw", adam_beta2=1.0), dict(optimizer="adamw", adam_beta2=-1e-3),
               dict(optimizer="adamw", adam_eps=0.0), dict(optimizer="adamw", adam_eps=-1e-8),
               dict(optimizer="adamw", weight_decay=-1e-3),
               dict(optimizer="adamw", nesterov=True),
               dict(adam_beta1=0.8), dict(adam_beta2=0.99), dict(adam_eps=1e-6),
               dict(optimizer="momentum", adam_beta1=0.8),
               dict(optimizer="rmsprop", adam_eps=1e-6),
               dict(weight_decay=1e-4), dict(optimizer="rmsprop", weight_decay=1e-4),
               dict(optimizer="adam")):
        with pytest.raises(ValueError):
            base.replace(**kw)
    # weight_decay alone moves between the two optimizers that have it
    assert cfg.replace(optimizer="momentum", adam_beta1=0.9, adam_beta2=0.999,
                       adam_eps=1e-8).weight_decay == 1e-2
    with pytest.raises(ValueError):
        cfg.replace(optimizer="momentum")      # (the adam_* fields are still set)


# ------------------------------------------------------------- 2: the oracle's own oracle
@pytest.mark.parametrize("t0", [0, 1000])
def test_adamw_ref_matches_float64_torch_adamw(t0):
    """torch.optim.AdamW with two parameter groups (decayed / not), 37 + 23 elements, five
    steps; then again from t = 1000 by setting the optimizer's state["step"].  Same recurrence,
    float64 rounding only.  The bound: p ~ 1 moves by ~lr per step through about ten float64
    operations, each within 2^-53 relative of a value <= 2: 1e-14 is 45 ulps of 1."""
    gen = torch.Generator().manual_seed(5)
    na, nb = 37, 23
    lr, wd = 0.0137, 1e-2
    l, b1, b2, e, w = (_f32(x) for x in (lr, BETAS[0], BETAS[1], EPS, wd))
    p0 = torch.randn(na + nb, generator=gen, dtype=torch.float64)
    a = p0[:na].clone().requires_grad_(True)
    b = p0[na:].clone().requires_grad_(True)
    opt = torch.optim.AdamW([{"params": [a], "weight_decay": w},
                             {"params": [b], "weight_decay": 0.0}],
                            lr=l, betas=(b1, b2), eps=e, amsgrad=False)
    mask = ranges_mask(na + nb, [(0, na)])
    p = p0.clone()
    m = torch.zeros(na + nb, dtype=torch.float64)
    v = torch.zeros(na + nb, dtype=torch.float64)
    if t0:
        # a state to continue from: moments of a plausible size, the count at t0
        m = torch.randn(na + nb, generator=gen, dtype=torch.float64) * 0.1
        v = torch.rand(na + nb, generator=gen, dtype=torch.float64) * 0.01 + 1e-4
        a.grad, b.grad = torch.zeros_like(a), torch.zeros_like(b)
        opt.step()                     # (creates the state; undone below)
        with torch.no_grad():
            a.copy_(p0[:na]), b.copy_(p0[na:])
        for q, sl in ((a, slice(0, na)), (b, slice(na, None))):
            st = opt.state[q]
            st["exp_avg"].copy_(m[sl]), st["exp_avg_sq"].copy_(v[sl])
            st["step"] = torch.tensor(float(t0))
    worst = 0.0
    for k in range(1, 6):
        g = torch.randn(na + nb, generator=gen, dtype=torch.float64)
        a.grad, b.grad = g[:na].clone(), g[na:].clone()
        opt.step()
        p, m, v = adamw_ref(p, g, m, v, t0 + k, lr, BETAS, EPS, wd, mask, c32=False)
        worst = max(worst, (torch.cat([a, b]).detach() - p).abs().max().item())
        assert int(opt.state[a]["step"]) == t0 + k
    print(f"ADAMW_REF_VS_TORCH t0={t0} max_abs_diff={worst:.3e}")
    assert worst <= 1e-14


def test_bias_corrections_at_a_large_count_are_exactly_one():
    assert adam_corrections(10 ** 6 + 1, BETAS) == (1.0, 1.0)
    c1, c2 = adam_corrections(2, BETAS)
    c1b, c2b = adam_corrections(3, BETAS)
    assert c2 / c2b > 1.2              # (what the applied-steps tests rely on)


# ------------------------------------------------------------------ 3: the CPU optimizer
def test_adamw_ref_matches_cpu_optimizer():
    """train/optim.AdamW (fp32 torch ops) against adamw_ref within adamw_bounds over two
    steps, each compared from the state it started from, with a mask that ends mid-vector."""
    gen = torch.Generator().manual_seed(6)
    n, ranges = 301, [(0, 101), (128, 203)]
    lr, wd = 0.02, 5e-2
    opt = AdamW(lr, 0.0, BETAS[0], BETAS[1], EPS, wd, n, ranges)
    p = torch.randn(n, generator=gen)
    mask = ranges_mask(n, ranges)
    worst = np.zeros(3)
    for t in (1, 2):
        g = torch.randn(n, generator=gen) * (2.0 if t == 1 else 0.3)
        p0, m0, v0 = p.clone(), opt.m.clone(), opt.v.clone()
        opt.step(p, g.clone())
        assert opt.t == t
        worst = np.maximum(worst, check_adamw_step(p0, g, m0, v0, p, opt.m, opt.v, t, lr, BETAS,
                                                   EPS, wd, mask, 1.0, ("cpu", t)))
        assert not torch.equal(p, p0)
    print("ADAMW_CPU_ERR p/m/v error over bound " + " ".join(f"{x:.3f}" for x in worst))
    sd = opt.state_dict()
    assert sd["kind"] == "adamw" and set(sd) == {"kind", "rate", "rate_decay", "adam_m",
                                                 "adam_v", "adam_t"}
    assert type(sd["adam_t"]) is int and sd["adam_t"] == 2


def test_cpu_optimizer_rate_decay():
    opt = AdamW(0.5, 1e-2, 0.9, 0.999, 1e-8, 0.0, 4)
    for _ in range(3):
        opt.step(torch.zeros(4), torch.zeros(4))
    assert opt.rate == 0.5 * (1 - 1e-2) * (1 - 1e-2) * (1 - 1e-2) and opt.t == 3


# ------------------------------------------------------------ 4: applied steps, not steps
def _exp_cfg(tmp_path, **kw):
    base = dict(numLayers=3, channelSize=16, batchSize=4, validationSize=4,
                validation_interval=1000, log_interval=1000, useCuda=False, synthetic=True,
                checkpoint_dir=str(tmp_path), seed=3, loader_threads=2, prefetch=2,
                rate=1e-2, rateDecay=1e-2, optimizer="adamw", weight_decay=1e-2,
                nan_policy="skip")
    base.update(kw)
    return ExperimentConfig(**base)


def test_bias_correction_counts_applied_steps(tmp_path):
    """Six optimizer steps of the CPU backend with distinct planted gradients, the second and
    the fifth skipped (a non-finite loss).  Each applied step equals adamw_ref with t = 1, 2,
    3, 4 from the state it started from and the rate of its call (the skipped calls decayed it
    too); a skipped one keeps p, m, v and t bit for bit; t ends at 4 after six calls.  The same
    reference with t taken from the call's index (3, 4, 6 for the last three) misses by far
    more than the bound: the test can tell the two apart."""
    from deep_go_amd.train.backends import CPUBackend
    cfg = _exp_cfg(tmp_path)
    be = CPUBackend(cfg, 4)
    n = be.layout.numel
    mask = ranges_mask(n, be.layout.weight_ranges())
    gen = torch.Generator().manual_seed(8)
    worst, miss, t = np.zeros(3), [], 0
    for call, apply in enumerate(APPLY, 1):
        g = torch.randn(n, generator=gen) * 0.1 * call
        be.params.grad = g.clone()
        be._loss_sum = 1.0 if apply else float("nan")
        p0, m0, v0 = be.flat_params().clone(), be.opt.m.clone(), be.opt.v.clone()
        lr0 = be.rate
        assert lr0 == pytest.approx(cfg.rate * (1.0 - cfg.rateDecay) ** (call - 1), rel=1e-13)
        be.optimizer_step()
        st = (p0, g, m0, v0, be.flat_params(), be.opt.m, be.opt.v)
        if not apply:
            assert be.opt.t == t
            for x, y in ((st[4], p0), (st[5], m0), (st[6], v0)):
                assert torch.equal(x.view(torch.int32), y.view(torch.int32))
            continue
        t += 1
        assert be.opt.t == t
        args = (lr0, BETAS, EPS, cfg.weight_decay, mask, 1.0)
        worst = np.maximum(worst, check_adamw_step(*st, t, *args, ("applied", call)))
        if call != t:
            miss.append(check_adamw_step(*st, call, *args, ("by index", call), must_pass=False)[0])
    assert be.opt.t == 4 and be.bad_steps() == 2 and len(miss) == 3
    print("ADAMW_APPLIED_CPU p/m/v error over bound " + " ".join(f"{x:.3f}" for x in worst)
          + " ; with t = call index, p error over bound " + " ".join(f"{x:.0f}" for x in miss))
    assert min(miss) > 100.0


# ------------------------------------------------------------------ 5: the CPU backend
def _skip_call(exp, k):
    """Make the k-th optimizer step of exp's backend a skipped one (a non-finite loss)."""
    be, calls = exp.backend, [0]
    step = be.optimizer_step

    def poisoned():
        calls[0] += 1
        if calls[0] == k:
            be._loss_sum = float("inf")
        step()
    be.optimizer_step = poisoned


def test_cpu_backend_resume_is_exact_and_reset_starts_from_zero(tmp_path):
    """With the second step skipped (so t != iterations): 4 steps == 2 steps + save + load + 2
    steps, bit for bit, t included and an int in the file; --reset-optimizer starts from zero
    moments, t = 0 and the configured rate; a momentum checkpoint loads zero moments, t = 0."""
    from deep_go_amd.train.experiment import Experiment
    from deep_go_amd.utils.checkpoint import load_checkpoint
    cfg = _exp_cfg(tmp_path)
    a = Experiment(cfg, id="a")
    a.init()
    _skip_call(a, 2)
    a.run(2)
    assert (a.backend.opt.t, a.iterations, a.backend.bad_steps()) == (1, 2, 1)
    path = a.save()
    opt_saved = load_checkpoint(path)[3]
    assert type(opt_saved["adam_t"]) is int and opt_saved["adam_t"] == 1
    assert torch.equal(opt_saved["adam_m"], a.backend.opt.m)
    a2 = Experiment.load(path)
    a2.id = "a2"
    a2.run(2)
    b = Experiment(cfg, id="b")
    b.init()
    _skip_call(b, 2)
    b.run(4)
    assert (b.backend.opt.t, b.iterations) == (3, 4)
    assert torch.equal(a2.backend.flat_params(), b.backend.flat_params())
    assert torch.equal(a2.backend.opt.m, b.backend.opt.m)
    assert torch.equal(a2.backend.opt.v, b.backend.opt.v)
    assert a2.backend.opt.t == 3 and a2.backend.rate == b.backend.rate and a2.iterations == 4
    assert not torch.equal(a.backend.opt.m, b.backend.opt.m)
    r = Experiment.load(path, reset_optimizer=True)
    r.init()
    assert r.backend.rate == cfg.rate and r.backend.opt.t == 0
    assert not r.backend.opt.m.any() and not r.backend.opt.v.any()
    assert torch.equal(r.backend.flat_params(), a.backend.flat_params())
    # another optimizer's checkpoint
    mcfg = _exp_cfg(tmp_path, optimizer="momentum")
    mo = Experiment(mcfg, id="mo")
    mo.run(2)
    c = Experiment.load(mo.save(), optimizer="adamw")
    c.init()
    assert c.backend.opt.t == 0 and not c.backend.opt.m.any() and not c.backend.opt.v.any()
    assert c.backend.rate == mo.backend.rate
    assert torch.equal(c.backend.flat_params(), mo.backend.flat_params())


# ------------------------------------------------------------------ 6: the launcher
def _adam():
    from deep_go_amd.ops import native
    try:
        return native.adam()
    except Exception as e:                                   # noqa: BLE001
        pytest.skip(f"_dgadam is not built: {e}")


# fake, suitably aligned, non-null addresses: every call below is refused before any launch
_P, _G, _M, _V, _LR, _REC = 0x1000, 0x2000, 0x3000, 0x4000, 0x5008, 0x6008


def _call(fn, p=_P, g=_G, m=_M, v=_V, n=1000, lr=_LR, rec=_REC, b1=0.9, b2=0.999, eps=1e-8,
          wd=1e-2, table=None):
    t = _table(table or [])
    fn(p, g, m, v, n, lr, rec, b1, b2, eps, wd, t.ctypes.data if len(t) else 0, len(t), 1.0, 0, 0)


@pytest.mark.parametrize("name", ["adamw", "adamw_bf16"])
def test_launcher_refuses_invalid_arguments_without_a_gpu(name):
    """Every refusal happens before any GPU work (no GPU here, and the addresses are fake: a
    launch would not survive them).  The kernels live in optim.hip beside momentum's; they are
    bound in a module of their own, _dgadam, because test_momentum_cpu pins the public names of
    _dgopt to its two — which this test checks are still on offer."""
    from deep_go_amd.ops import native
    fn = getattr(_adam(), name)
    assert sorted(x for x in dir(_adam()) if not x.startswith("_")) == [
        "adamw", "adamw_bf16", "adamw_tick"]
    assert {"momentum", "momentum_bf16"} <= set(dir(native.opt()))
    bad = {what: dict(table=rows) for what, rows in BAD_RANGES.items()}
    bad.update({
        "null p": dict(p=0), "null m": dict(m=0), "null v": dict(v=0), "null lr": dict(lr=0),
        "null record": dict(rec=0), "null gradient": dict(g=0),
        "beta1 = 1": dict(b1=1.0), "beta1 < 0": dict(b1=-0.1), "beta1 nan": dict(b1=math.nan),
        "beta2 = 1": dict(b2=1.0), "beta2 < 0": dict(b2=-1e-3),
        "eps = 0": dict(eps=0.0), "eps < 0": dict(eps=-1e-8), "eps nan": dict(eps=math.nan),
        "record off 8 bytes": dict(rec=_REC + 4),
        "p off 16 bytes": dict(p=_P + 4), "m off 16 bytes": dict(m=_M + 8),
        "v off 16 bytes": dict(v=_V + 4),
        "gradient misaligned": dict(g=_G + (4 if name == "adamw" else 2)),
    })
    for what, kw in bad.items():
        with pytest.raises(RuntimeError) as e:
            _call(fn, **kw)
        assert str(e.value) == f"{name}: invalid argument", what
    with pytest.raises(RuntimeError) as e:     # a count without a table
        fn(_P, _G, _M, _V, 1000, _LR, _REC, 0.9, 0.999, 1e-8, 0.0, 0, 1, 1.0, 0, 0)
    assert str(e.value) == f"{name}: invalid argument"
    # n = 0 with a valid (empty) table: nothing to do, no launch
    fn(0, 0, 0, 0, 0, 0, 0, 0.9, 0.999, 1e-8, 0.0, 0, 0, 1.0, 0, 0)
    with pytest.raises(RuntimeError) as e:     # (the ranges and betas are checked even then)
        fn(0, 0, 0, 0, 0, 0, 0, 1.0, 0.999, 1e-8, 0.0, 0, 0, 1.0, 0, 0)
    assert str(e.value) == f"{name}: invalid argument"


def test_tick_launcher_refuses_invalid_arguments_without_a_gpu():
    tick = _adam().adamw_tick
    for args in ((0, 0.9, 0.999), (_REC + 4, 0.9, 0.999), (_REC, 1.0, 0.999),
                 (_REC, 0.9, -0.5)):
        with pytest.raises(RuntimeError) as e:
            tick(*args, 0, 0)
        assert str(e.value) == "adamw_tick: invalid argument"


# ------------------------------------------------------------------ 7: two ranks
def _dp_worker(rank, world, port, out_dir):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank),
                      WORLD_SIZE=str(world), LOCAL_RANK=str(rank))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from deep_go_amd.data.synthetic import random_planes
    from deep_go_amd.train.backends import CPUBackend
    cfg = ExperimentConfig(numLayers=3, channelSize=16, rate=1e-2, seed=5, bucket_mb=0.01,
                           optimizer="adamw", weight_decay=1e-2)
    B = 8
    be = CPUBackend(cfg, B // world, world=world, bucket_mb=0.01)
    for step in range(3):
        planes, player, rank_, labels = random_planes(B, seed=step)
        sl = slice(rank * (B // world), (rank + 1) * (B // world))
        be.set_batch(planes[sl], player[sl], rank_[sl], labels[sl])
        be.forward_backward()
        be.optimizer_step()
    torch.save({"params": be.flat_params().clone(), "m": be.opt.m, "v": be.opt.v,
                "t": be.opt.t}, os.path.join(out_dir, f"rank{rank}.pt"))
    dist.barrier()
    dist.destroy_process_group()


def test_two_gloo_ranks_keep_identical_parameters_and_count(tmp_path):
    """Every rank applies the same all-reduced gradient: after three steps the parameters, both
    moments and t are identical on both ranks."""
    mp.spawn(_dp_worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True)
    a = torch.load(str(tmp_path / "rank0.pt"), weights_only=True)
    b = torch.load(str(tmp_path / "rank1.pt"), weights_only=True)
    assert a["t"] == b["t"] == 3
    for k in ("params", "m", "v"):
        assert torch.equal(a[k], b[k]), k
    assert a["m"].abs().max() > 0 and a["v"].abs().max() > 0
