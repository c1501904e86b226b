"""ema_decay without a GPU: the float64 oracle ``ema_ref`` (checked against the closed form of
the average's weights), the counted fp32 bound ``ema_bound`` and an honest fp32 emulation of the
kernel, designed data, planted defects that each check catches, the config, the CPU trainer,
checkpoints and the ``--ema`` interfaces, two gloo ranks and the argument checks of the
``_dgema`` launcher.

The definition (train/optim.py WeightEMA, csrc/kernels/ema.hip), after the optimizer's update
of an APPLIED step, with p the parameters as the update left them:

    t    = t + 1
    d    = min(ema_decay, (1 + t) / (10 + t))        (double)
    omd  = float32(1.0 - d)
    e[i] = fmaf(omd, p[i] - e[i], e[i])              (fp32: one rounded subtraction, one fma)

e starts as the parameters, t at 0; a skipped step moves neither.

tests/test_ema_gpu.py imports ``ema_ref``, ``ema_bound``, ``omd_of``, ``check_ema``,
``designed_case``, ``SIZES`` and ``CAP`` from here.
"""
import json
import math
import os
from fractions import Fraction

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from deep_go_amd.config import ExperimentConfig
from deep_go_amd.train.optim import ema_omd, fma32
from test_dist_cpu import _free_port

U24 = 2.0 ** -24
MT, CAP = 256, 8192               # ema.hip: threads per workgroup, the grid's cap
# the kernel tests' sizes: below one 4-vector, tails of 1 and 3, one full vector and one more
# element, several workgroups with a partial last one, and two past the 4 * 256 * CAP elements
# one pass of the capped grid covers, which force a second grid-stride pass with a partial last
# workgroup: 4 * 256 * CAP + 1029 + 3 (a multiple of 4: no tail) and 4 * 256 * CAP + 1031 (a
# 3-element tail)
SIZES = [1, 3, 4, 5, 1027, 4 * MT * CAP + 1029 + 3, 4 * MT * CAP + 1031]
assert SIZES[-2] % 4 == 0 and SIZES[-1] % 4 == 3


def _f32(x) -> float:
    return float(np.float32(x))


# ------------------------------------------------------------------------------ oracle
def omd_of(decay: float, t: int) -> float:
    """float32(1 - min(decay, (1 + t) / (10 + t))) of averaging step t (counted from 1), every
    operation an IEEE double one, written out here independently of train/optim.py."""
    td = float(t)
    ramp = (1.0 + td) / (10.0 + td)
    d = decay if decay < ramp else ramp
    return _f32(1.0 - d)


def ema_ref(e0, ps, decay: float, t0: int = 0, gates=None):
    """(e, t) in float64 after the parameter vectors ps (each as the update left it), from the
    average e0 and the count t0; gates[k] false: step k is skipped."""
    e, t = e0.double().clone(), int(t0)
    for k, p in enumerate(ps):
        if gates is not None and not gates[k]:
            continue
        t += 1
        e = e + omd_of(decay, t) * (p.double() - e)
    return e, t


def ema_bound(e_prev, p, omd: float, prev=None):
    """Per element, the counted roundings of e' = fmaf(omd, fl(p - e), e) against the float64
    value from the same fp32 e, p and omd: the rounding of p - e (2^-24 relative) scaled by
    omd, plus the final half ulp (2^-24 of the value that is rounded, which is the result moved
    by the first term; 2^-150 absolute covers a subnormal one).  The float64 side's own
    roundings are 2^-29 of that.  prev: the bound the average e itself carried into the step
    (several steps without teacher forcing): it shrinks by 1 - omd and widens the magnitudes
    the two roundings act on."""
    e_prev, p = e_prev.double(), p.double()
    pv = torch.zeros_like(e_prev) if prev is None else prev
    res = e_prev + omd * (p - e_prev)
    first = U24 * omd * ((p - e_prev).abs() + pv)
    b = first + U24 * (res.abs() + pv + first) + 2.0 ** -150
    return (1.0 - omd) * pv + b * (1.0 + 2.0 ** -29)


def check_ema(got, e0, ps, decay, t0=0, gates=None):
    """Whether the fp32 average `got` lies within the accumulated ema_bound of ema_ref over
    the steps ps -> (ok, the largest error over its bound)."""
    e, t, bound = e0.double().clone(), int(t0), None
    for k, p in enumerate(ps):
        if gates is not None and not gates[k]:
            continue
        t += 1
        omd = omd_of(decay, t)
        bound = ema_bound(e, p, omd, bound)
        e = e + omd * (p.double() - e)
    if bound is None:
        return bool(torch.equal(got.double(), e)), 0.0
    ratio = ((got.double() - e).abs() / bound).max().item()
    return ratio <= 1.0, ratio


# --------------------------------------------------------------- an fp32 emulation, honest
def emulate(e0, ps, decay, gates=None, t0=0, defect: str = "", p_before=None):
    """The kernel pair in fp32 numpy arithmetic, step by step: the count, omd, one rounded
    subtraction and one fused multiply-add per element (train/optim.py fma32).  defect: one of
    the planted ones.  p_before: the parameters before each update (for that defect).
    -> (e fp32, t)."""
    e = (torch.zeros_like(e0) if defect == "seeded with zeros" else e0).float().numpy().copy()
    t = int(t0)
    n = e.size
    for k, p in enumerate(ps):
        if defect == "t from the call index":
            t = t0 + k + 1
        if gates is not None and not gates[k]:
            continue
        if defect != "t from the call index":
            t += 1
        td = float(t)
        d = decay if defect == "ramp missing" else min(decay, (1.0 + td) / (10.0 + td))
        omd = np.float32(d if defect == "omd and d swapped" else 1.0 - d)
        src = (p_before[k] if defect == "pre-update p" else p).float().numpy()
        new = fma32(omd, src - e, e)
        if defect == "tail dropped":
            new[n - n % 4:] = e[n - n % 4:]
        e = new
    return torch.from_numpy(e), t


def designed_case(n: int, seed: int):
    """Small integers: e in -8..8 times 4 and p - e a multiple of 4 in -32..32, so with omd =
    0.25 the update e + (p - e) / 4 is an integer below 2^24: exact in fp32 whatever the order
    and with or without the fma.  -> (e0, p, the exact result), fp32."""
    gen = torch.Generator().manual_seed(seed)
    e0 = torch.randint(-8, 9, (n,), generator=gen) * 4
    diff = torch.randint(-8, 9, (n,), generator=gen) * 4
    return e0.float(), (e0 + diff).float(), (e0 + diff // 4).float()


# decay 0.75 past the ramp's crossover ((1 + t) / (10 + t) >= 0.75 from t = 26): omd = 0.25
DESIGNED_DECAY, DESIGNED_T0 = 0.75, 99


# ------------------------------------------------------------- 1: the oracle's own oracle
def test_ema_ref_matches_the_closed_form():
    """Two parameter groups of 37 + 23 elements over five steps: e_T = w_0 e_0 + sum_k w_k p_k
    with w_k = omd_k prod_{j > k} (1 - omd_j) and w_0 = prod_j (1 - omd_j), summed in exact
    rational arithmetic from the fp32 inputs; the float64 recursion agrees to a few ulp of
    float64 (measured: 0.82).  The weights add up to one."""
    gen = torch.Generator().manual_seed(3)
    decay, T = 0.3, 5
    groups = [37, 23]
    e0 = torch.cat([torch.randn(g, generator=gen) for g in groups])
    ps = [torch.cat([torch.randn(g, generator=gen) * (1 + k) for g in groups]) for k in range(T)]
    e, t = ema_ref(e0, ps, decay)
    assert t == T
    om = [Fraction(omd_of(decay, k)) for k in range(1, T + 1)]
    w = [om[k] * math.prod((1 - om[j] for j in range(k + 1, T)), start=Fraction(1))
         for k in range(T)]
    w0 = math.prod((1 - o for o in om), start=Fraction(1))
    assert w0 + sum(w) == 1
    # (the ramp rules the first steps, the cap the later ones)
    assert omd_of(decay, 1) == _f32(1.0 - 2.0 / 11.0) and omd_of(decay, 5) == _f32(1.0 - 0.3)
    worst = 0.0
    for i in range(sum(groups)):
        want = w0 * Fraction(float(e0[i])) + sum(w[k] * Fraction(float(ps[k][i]))
                                                 for k in range(T))
        scale = abs(w0 * Fraction(float(e0[i]))) + sum(abs(w[k] * Fraction(float(ps[k][i])))
                                                       for k in range(T))
        worst = max(worst, float(abs(Fraction(float(e[i])) - want) / scale))
    print(f"EMA_REF_VS_CLOSED_FORM worst relative difference {worst / 2.0 ** -52:.2f} ulp64")
    assert worst <= 8 * 2.0 ** -52


def test_omd_of_agrees_with_the_trainers():
    for decay in (0.5, 0.999, 0.9999):
        for t in (1, 2, 8, 9, 10, 1000, 10 ** 9 + 1):
            assert ema_omd(decay, t) == omd_of(decay, t)
    # the crossover of the ramp and the cap at decay = 0.5: (1 + t) / (10 + t) = 0.5 at t = 8
    assert omd_of(0.5, 7) == _f32(1.0 - 8.0 / 17.0) and omd_of(0.5, 8) == omd_of(0.5, 9) == 0.5


# ------------------------------------------------------------------------------ 2: the bound
def _fma_exact(a, b, c) -> float:
    """fmaf on three fp32 values by exact rational arithmetic and one rounding."""
    x = Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c))
    lo = np.float32(float(x))              # (near x: one of it and its neighbours is nearest)
    cands = [lo, np.nextafter(lo, np.float32(np.inf)), np.nextafter(lo, np.float32(-np.inf))]
    return float(min(cands, key=lambda v: (abs(Fraction(float(v)) - x),
                                           int(np.float32(v).view(np.int32)) & 1)))


def test_honest_fp32_emulation_stays_inside_the_bound():
    """One step in fp32 — the subtraction rounded, the fused multiply-add by exact rational
    arithmetic and one rounding — over magnitudes from 1e-6 to 1e6, e near p and far from it:
    inside ema_bound of the float64 value.  Measured: 0.999 of the bound (it is tight: a
    result just above a power of two, rounded by nearly half an ulp, reaches it).  train/optim.py
    fma32 gives the same bits."""
    rng = np.random.default_rng(11)
    n = 3000
    p = (rng.standard_normal(n) * 10.0 ** rng.integers(-6, 7, n)).astype(np.float32)
    e = (p * (1 + rng.standard_normal(n) * 10.0 ** rng.integers(-7, 1, n))).astype(np.float32)
    worst = 0.0
    for decay, t in ((0.999, 5), (0.999, 5000), (0.5, 100)):
        omd = np.float32(omd_of(decay, t))
        diff = p - e
        got = np.array([_fma_exact(omd, diff[i], e[i]) for i in range(n)], dtype=np.float32)
        assert np.array_equal(got, fma32(omd, diff, e))
        pt, et = torch.from_numpy(p), torch.from_numpy(e)
        ref = ema_ref(et, [pt], decay, t0=t - 1)[0]
        b = ema_bound(et, pt, float(omd))
        worst = max(worst, ((torch.from_numpy(got).double() - ref).abs() / b).max().item())
    print(f"EMA_EMULATION err_over_bound={worst:.3f}")
    assert worst <= 1.0
    # the result lies between e and p, and e == p is a fixed point
    lo, hi = np.minimum(e, p), np.maximum(e, p)
    assert ((got >= lo) & (got <= hi)).all()
    assert np.array_equal(fma32(omd, p - p, p), p)


def test_two_roundings_more_miss_the_bound_somewhere():
    """(the bound is tight enough to tell: an unfused multiply and add, one rounding more,
    exceeds it on some element of the same data)"""
    rng = np.random.default_rng(11)
    n = 20000
    p = (rng.standard_normal(n)).astype(np.float32)
    e = (p + rng.standard_normal(n).astype(np.float32) * 4).astype(np.float32)
    omd = np.float32(omd_of(0.3, 50))
    got = (omd * (p - e)) + e
    pt, et = torch.from_numpy(p), torch.from_numpy(e)
    ratio = ((torch.from_numpy(got).double() - ema_ref(et, [pt], 0.3, t0=49)[0]).abs()
             / ema_bound(et, pt, float(omd))).max().item()
    assert ratio > 1.0, ratio


# ------------------------------------------------------------------------- 3: designed data
def test_designed_data_is_exact():
    for n in (5, 1027):
        e0, p, want = designed_case(n, n)
        assert omd_of(DESIGNED_DECAY, DESIGNED_T0 + 1) == 0.25
        got, t = emulate(e0, [p], DESIGNED_DECAY, t0=DESIGNED_T0)
        assert t == DESIGNED_T0 + 1 and torch.equal(got, want)
        assert torch.equal(ema_ref(e0, [p], DESIGNED_DECAY, t0=DESIGNED_T0)[0], want.double())
        assert not torch.equal(want, e0) and not torch.equal(want, p)


# --------------------------------------------------------------------- 4: planted defects
DEFECTS = ["omd and d swapped", "t from the call index", "ramp missing", "seeded with zeros",
           "pre-update p", "tail dropped"]


def _defect_case():
    gen = torch.Generator().manual_seed(9)
    n = 1027                      # a 3-element tail
    p0 = torch.randn(n, generator=gen)
    ps, before = [], []
    cur = p0
    for _ in range(3):
        before.append(cur)
        cur = cur + torch.randn(n, generator=gen) * 0.1
        ps.append(cur)
    return p0, ps, before, [True, False, True]       # apply, skip, apply


@pytest.mark.parametrize("defect", DEFECTS)
def test_planted_defect_fails_its_check(defect):
    """Each defect, planted in the emulation, fails check_ema (or the count) on the pattern
    apply, skip, apply at decay 0.9 (where the ramp rules); the clean emulation passes."""
    p0, ps, before, gates = _defect_case()
    decay = 0.9
    got, t = emulate(p0, ps, decay, gates, p_before=before)
    ok, ratio = check_ema(got, p0, ps, decay, gates=gates)
    assert ok and t == 2, ratio
    got, t = emulate(p0, ps, decay, gates, defect=defect, p_before=before)
    ok, ratio = check_ema(got, p0, ps, decay, gates=gates)
    assert not ok and ratio > 100, (defect, ratio)
    if defect == "t from the call index":
        assert t == 3


def test_designed_data_catches_the_swap_too():
    e0, p, want = designed_case(1027, 1)
    got, _ = emulate(e0, [p], DESIGNED_DECAY, t0=DESIGNED_T0, defect="omd and d swapped")
    assert not torch.equal(got, want)


# ------------------------------------------------------------------------------ 5: config
def test_config_defaults_old_checkpoints_and_rejections():
    base = ExperimentConfig()
    assert base.ema_decay == 0.0
    d = base.to_dict()
    assert d["ema_decay"] == 0.0
    del d["ema_decay"]                          # an older checkpoint's config
    assert ExperimentConfig.from_dict(d).ema_decay == 0.0
    for opt in ("sgd", "rmsprop", "momentum", "adamw"):
        cfg = base.replace(optimizer=opt, ema_decay="0.999")    # (as the command line gives it)
        assert cfg.ema_decay == 0.999 and ExperimentConfig.from_dict(cfg.to_dict()) == cfg
    assert base.replace(ema_decay=0).ema_decay == 0.0
    for bad in (-1, -1e-9, 1, 1.0, 1.5, float("nan"), float("inf"), "-0.1", "nan", "1"):
        with pytest.raises(ValueError):
            base.replace(ema_decay=bad)


# ------------------------------------------------------------------ 6: the CPU trainer
def _exp_cfg(tmp_path, data_root, **kw):
    base = dict(numLayers=3, channelSize=16, batchSize=4, validationSize=4,
                validation_interval=2, log_interval=1, useCuda=False, synthetic=False,
                data_root=data_root, checkpoint_dir=str(tmp_path), seed=3, loader_threads=2,
                prefetch=2, rate=1e-3, rateDecay=1e-2, nan_policy="skip", head_relu=False)
    base.update(kw)
    return ExperimentConfig(**base)


def _rows(path):
    from deep_go_amd.utils.metrics import read_jsonl
    drop = ("time", "boards_per_sec", "runningTime", "name")     # (the clock, the run's id)
    return [{k: v for k, v in r.items() if k not in drop} for r in read_jsonl(path)]


@pytest.mark.parametrize("opt", ["sgd", "rmsprop", "momentum", "adamw"])
def test_cpu_trainer_is_bit_identical_with_the_average_on(tmp_path, packed_fixture, opt):
    """Five iterations with ema_decay = 0.9 and with 0: the parameters, the optimizer's state,
    the rate and every existing record are the same; with it on each validation is followed by
    one kind="validation_ema" record; the average follows ema_ref."""
    from deep_go_amd.train.experiment import Experiment
    out = []
    for decay in (0.0, 0.9):
        mpath = str(tmp_path / f"m{decay}.jsonl")
        e = Experiment(_exp_cfg(tmp_path, packed_fixture, optimizer=opt, ema_decay=decay,
                                metrics_path=mpath), id=f"{opt}{decay}")
        e.init()
        p0 = e.backend.flat_params().clone()
        ps = []
        for _ in range(5):
            e.run(1)
            ps.append(e.backend.flat_params().clone())
        e.metrics.close()
        out.append((e, _rows(mpath), p0, ps))
    (a, ra, _, _), (b, rb, p0, ps) = out
    assert torch.equal(a.backend.flat_params().view(torch.int32),
                       b.backend.flat_params().view(torch.int32))
    assert a.backend.rate == b.backend.rate
    sa, sb = a.backend.opt.state_dict(), b.backend.opt.state_dict()
    assert set(sa) == set(sb)
    for k in sa:
        assert torch.equal(sa[k], sb[k]) if isinstance(sa[k], torch.Tensor) else sa[k] == sb[k]
    assert a.validation_costs == b.validation_costs
    ema_rows = [r for r in rb if r.get("kind") == "validation_ema"]
    assert ra == [r for r in rb if r.get("kind") != "validation_ema"]
    assert not [r for r in ra if r.get("kind") == "validation_ema"]
    # (e.run(1) draws its validation set anew: iterations 2 and 4 validate)
    assert [r["step"] for r in ema_rows] == [2, 4]
    assert set(ema_rows[0]) == {"kind", "step", "val_cost", "val_acc"}
    kinds = [r["kind"] for r in rb if r.get("kind", "").startswith("validation")]
    assert kinds == ["validation", "validation_ema"] * 2
    assert all(math.isfinite(r["val_cost"]) for r in ema_rows)
    # plot.py filters by kind: the same series from both files
    from deep_go_amd.utils.plot import _series
    assert _series(str(tmp_path / "m0.9.jsonl")) == _series(str(tmp_path / "m0.0.jsonl"))
    assert len(_series(str(tmp_path / "m0.9.jsonl"))[0]) == 2
    with pytest.raises(RuntimeError):
        a.backend.ema_params()
    assert b.backend.ema_steps() == 5
    ok, ratio = check_ema(b.backend.ema_params(), p0, ps, 0.9)
    assert ok, ratio
    assert not torch.equal(b.backend.ema_params(), b.backend.flat_params())


def test_cpu_apply_skip_apply_apply_counts_three(tmp_path, packed_fixture):
    from deep_go_amd.data.synthetic import random_planes
    from deep_go_amd.train.backends import CPUBackend
    cfg = _exp_cfg(tmp_path, packed_fixture, optimizer="adamw", ema_decay=0.9)
    be = CPUBackend(cfg, 4)
    p0 = be.flat_params().clone()
    assert torch.equal(be.ema_params(), p0) and be.ema_steps() == 0
    be.set_batch(*random_planes(4, seed=0))
    ps, gates = [], [True, False, True, True]
    for k, g in enumerate(gates):
        be.forward_backward()
        e_before, rate = be.ema_params().clone(), be.rate
        if not g:
            be._loss_sum = float("nan")
        be.optimizer_step()
        ps.append(be.flat_params().clone())
        if not g:
            assert torch.equal(be.ema_params().view(torch.int32), e_before.view(torch.int32))
            assert be.ema_steps() == 1 and be.bad_steps() == 1
            assert be.rate == rate * (1.0 - cfg.rateDecay)      # (the rate still decays)
    assert be.ema_steps() == 3 and be.opt.t == 3
    ok, ratio = check_ema(be.ema_params(), p0, ps, 0.9, gates=gates)
    assert ok, ratio
    ok, _ = check_ema(be.ema_params(), p0, ps, 0.9)          # (the skip matters)
    assert not ok


def test_cpu_ema_weights_context(tmp_path, packed_fixture):
    from deep_go_amd.data.synthetic import random_planes
    from deep_go_amd.train.backends import CPUBackend
    cfg = _exp_cfg(tmp_path, packed_fixture, ema_decay=0.5, rate=0.05)
    be = CPUBackend(cfg, 4)
    be.set_batch(*random_planes(4, seed=0))
    for _ in range(3):
        be.train_step()
    live = be.evaluate().clone()
    other = CPUBackend(cfg.replace(ema_decay=0.0), 4, flat=be.ema_params().clone())
    other.set_batch(*random_planes(4, seed=0))
    want = other.evaluate()
    with be.ema_weights():
        got = be.evaluate().clone()
        with pytest.raises(RuntimeError):
            with be.ema_weights():
                pass
        for fn in (be.forward_backward, be.optimizer_step, be.train_step):
            with pytest.raises(RuntimeError):
                fn()
    assert torch.equal(got, want) and not torch.equal(got, live)
    assert torch.equal(be.evaluate(), live)
    with pytest.raises(RuntimeError):
        other.ema_weights().__enter__()


# ------------------------------------------------------------------ 7: checkpoints
def test_checkpoint_round_trip_resume_and_reset(tmp_path, packed_fixture):
    """ema and ema_t travel through the checkpoint (a tensor and an integer); 2 + 2 iterations
    through a checkpoint equal 4, bit for bit, also with a skipped step before the save;
    --reset-optimizer, and a checkpoint without an average, start from the loaded parameters
    with t = 0; a checkpoint with an average loaded under ema_decay = 0 ignores it."""
    from deep_go_amd.train.experiment import Experiment
    from deep_go_amd.utils.checkpoint import load_checkpoint
    cfg = _exp_cfg(tmp_path, packed_fixture, optimizer="adamw", ema_decay=0.9,
                   validation_interval=1000)
    a = Experiment(cfg, id="a")
    a.run(2)
    # a skipped step: the count falls behind the iterations
    a.backend.forward_backward()
    a.backend._loss_sum = float("nan")
    a.backend.optimizer_step()
    path = a.save()
    _, flat, _, opt = load_checkpoint(path)
    assert opt["ema_t"] == 2 and isinstance(opt["ema_t"], int)
    assert torch.equal(opt["ema"].view(torch.int32), a.backend.ema_params().view(torch.int32))
    assert opt["ema"].shape == flat.shape
    a2 = Experiment.load(path)
    a2.id = "a2"
    a2.run(2)
    a.run(2)
    assert a2.backend.ema_steps() == a.backend.ema_steps() == 4
    assert torch.equal(a2.backend.flat_params(), a.backend.flat_params())
    assert torch.equal(a2.backend.ema_params().view(torch.int32),
                       a.backend.ema_params().view(torch.int32))
    # --reset-optimizer
    r = Experiment.load(path, reset_optimizer=True)
    r.init()
    assert r.backend.ema_steps() == 0 and torch.equal(r.backend.ema_params(), flat)
    assert not torch.equal(opt["ema"], flat)
    # loaded under ema_decay = 0: ignored
    z = Experiment.load(path, ema_decay=0.0)
    z.init()
    assert z.backend.ema is None and "ema" not in z.backend.state_dict()["optimizer"]
    # a checkpoint without an average, resumed with the average on
    plain = Experiment(cfg.replace(ema_decay=0.0), id="plain")
    plain.run(2)
    ppath = plain.save()
    assert "ema" not in load_checkpoint(ppath)[3]
    s = Experiment.load(ppath, ema_decay=0.9)
    s.init()
    assert s.backend.ema_steps() == 0
    assert torch.equal(s.backend.ema_params(), plain.backend.flat_params())
    # the average in the place of the parameters
    assert torch.equal(Experiment.load(path, ema=True)._restore_params, opt["ema"])
    with pytest.raises(ValueError):
        Experiment.load(ppath, ema=True)


def test_cli_ema_refuses_a_checkpoint_without_an_average(tmp_path, packed_fixture, capsys):
    from deep_go_amd import cli
    from deep_go_amd.predict import Predictor
    from deep_go_amd.train.experiment import Experiment
    from deep_go_amd.utils.checkpoint import import_t7, load_checkpoint
    cfg = _exp_cfg(tmp_path, packed_fixture, validation_interval=1000)
    plain = Experiment(cfg, id="plain")
    plain.run(1)
    ppath = plain.save()
    sgf = str(tmp_path / "none.sgf")
    for argv in (["eval", ppath, "--ema", "--device", "cpu"],
                 ["export", ppath, str(tmp_path / "x.t7"), "--ema"],
                 ["predict", ppath, sgf, "--ema", "--device", "cpu"]):
        with pytest.raises(SystemExit) as e:
            cli.main(argv)
        assert "carries no weight average" in str(e.value) and argv[0] in str(e.value)
    assert not os.path.exists(str(tmp_path / "x.t7"))
    with pytest.raises(ValueError):
        Predictor.load(ppath, ema=True, device="cpu")
    # and with one: eval and export serve the average
    e = Experiment(cfg.replace(ema_decay=0.5, rate=0.05), id="avg")
    e.run(3)
    path = e.save()
    capsys.readouterr()
    assert cli.main(["eval", path, "--ema", "--device", "cpu", "--n", "4"]) == 0
    row = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert row["ema"] is True and math.isfinite(row["cost"])
    want = Experiment.load(path, ema=True)
    want.cfg = want.cfg.replace(useCuda=False)
    assert row["cost"] == want.evaluate_split("test", 4)[0]
    live = Experiment.load(path)
    live.cfg = live.cfg.replace(useCuda=False)
    assert row["cost"] != live.evaluate_split("test", 4)[0]
    out = str(tmp_path / "avg.t7")
    assert cli.main(["export", path, out, "--ema"]) == 0
    assert torch.equal(import_t7(out, e.cfg)[1], load_checkpoint(path)[3]["ema"])
    p = Predictor.load(path, ema=True, device="cpu")
    assert p is not None


# ------------------------------------------------------------------ 8: two ranks
def _dp_worker(rank, world, port, out_dir):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank),
                      WORLD_SIZE=str(world), LOCAL_RANK=str(rank))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from deep_go_amd.data.synthetic import random_planes
    from deep_go_amd.parallel import dp
    from deep_go_amd.train.backends import CPUBackend
    # (a seed per rank: the broadcast of rank 0's parameters, then the reseeding, matter)
    cfg = ExperimentConfig(numLayers=3, channelSize=16, rate=1e-2, seed=5 + rank, bucket_mb=0.01,
                           ema_decay=0.9)
    B = 8
    be = CPUBackend(cfg, B // world, world=world, bucket_mb=0.01)
    dp.broadcast_(be.params.data, 0)
    be.reset_ema()
    p0 = be.flat_params().clone()
    ps = []
    for step in range(3):
        planes, player, rank_, labels = random_planes(B, seed=step)
        sl = slice(rank * (B // world), (rank + 1) * (B // world))
        be.set_batch(planes[sl], player[sl], rank_[sl], labels[sl])
        be.forward_backward()
        be.optimizer_step()
        ps.append(be.flat_params().clone())
    torch.save({"ema": be.ema_params().clone(), "t": be.ema_steps(), "p0": p0, "ps": ps},
               os.path.join(out_dir, f"rank{rank}.pt"))
    dist.barrier()
    dist.destroy_process_group()


def test_two_gloo_ranks_average_alike(tmp_path):
    """Every rank holds the same parameters after every step, so the same average: bit
    identical after three steps, with no collective of its own."""
    mp.spawn(_dp_worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True)
    a = torch.load(str(tmp_path / "rank0.pt"), weights_only=True)
    b = torch.load(str(tmp_path / "rank1.pt"), weights_only=True)
    assert torch.equal(a["ema"].view(torch.int32), b["ema"].view(torch.int32))
    assert a["t"] == b["t"] == 3
    ok, ratio = check_ema(a["ema"], a["p0"], a["ps"], 0.9)
    assert ok, ratio


# ------------------------------------------------------------------ 9: the launcher
def _ema():
    from deep_go_amd.ops import native
    try:
        return native.ema()
    except Exception as e:                                   # noqa: BLE001
        pytest.skip(f"_dgema is not built: {e}")


# fake, suitably aligned, non-null addresses: every call below is refused before any launch
_P, _E, _REC = 0x1000, 0x2000, 0x4008


def test_module_public_names():
    m = _ema()
    assert sorted(x for x in dir(m) if not x.startswith("_")) == ["ema", "ema_tick"]


def test_launcher_refuses_invalid_arguments_without_a_gpu():
    """Every refusal happens before any GPU work (no GPU here, and the addresses are fake: a
    launch would not survive them)."""
    m = _ema()

    def call(p=_P, e=_E, n=1000, rec=_REC, decay=0.999):
        m.ema(p, e, n, rec, decay, 0, 0)
    bad = {"null p": dict(p=0), "null e": dict(e=0), "null record": dict(rec=0),
           "p misaligned": dict(p=_P + 4), "e misaligned": dict(e=_E + 8),
           "record off 8 bytes": dict(rec=_REC + 4), "decay = 1": dict(decay=1.0),
           "decay < 0": dict(decay=-1e-9), "decay > 1": dict(decay=1.5),
           "decay nan": dict(decay=math.nan), "decay inf": dict(decay=math.inf)}
    for what, kw in bad.items():
        with pytest.raises(RuntimeError) as e:
            call(**kw)
        assert str(e.value) == "ema: invalid argument", what
    # n = 0: nothing to do, no launch, whatever the pointers
    call(p=0, e=0, n=0, rec=0)
    with pytest.raises(RuntimeError) as e:      # (the decay is checked even then)
        call(p=0, e=0, n=0, rec=0, decay=1.0)
    assert str(e.value) == "ema: invalid argument"
    for args in ((0, 0.5), (_REC + 4, 0.5), (_REC, 1.0), (_REC, math.nan), (_REC, -0.5)):
        with pytest.raises(RuntimeError) as e:
            m.ema_tick(*args, 0, 0)
        assert str(e.value) == "ema_tick: invalid argument"
