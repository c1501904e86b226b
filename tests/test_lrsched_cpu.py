"""lr_schedule without a GPU: the float64 oracle ``lr_ref``, ``LRSchedule`` against it bit for
bit, exact landmarks, planted defects that each fail a check, the config, the CPU trainer,
checkpoints, the ``cli train`` fill-in of ``lr_total``, two gloo ranks and the argument checks of
the ``_dgsched`` launcher.

The definition (train/optim.py LRSchedule, csrc/kernels/sched.hip), with base = cfg.rate and
s = 0 at the start; the rate step s uses, every operation an IEEE double one:

    w  = min(1, (s + 1) / W)            if W > 0 else 1
    u  = clamp((s - W) / (T - W), 0, 1)                          (linear, cosine)
    d  = 1                                                        constant
         1 - (1 - m) * u                                          linear
         m + (1 - m) * 0.5 * (1 + cos(pi * u))                    cosine
         max(m, g ** floor(max(s - W, 0) / E))                    step
    lr = base * (w * d)

and, for linear and cosine, d = m exactly for every s >= T ("past T the factor stays at m": in
double 1 - (1 - 0.1) * 1 is 0.09999999999999998, not 0.1, so the floor is taken literally there,
which the landmark "exactly m * rate for every s >= T" needs).  After every step, applied or
skipped: base = base * (1 - rateDecay); s = s + 1.

tests/test_lrsched_gpu.py imports ``lr_ref``, ``factor_ref``, ``mk_cfg``, ``lr_fields``, ``LR_OFF`` and ``KINDS`` from here.
"""
import json
import math
import os

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from deep_go_amd.config import ExperimentConfig
from test_dist_cpu import _free_port

KINDS = ("constant", "linear", "cosine", "step")
# a power of two: rate * x is then exact for every double x, so that "lr(0) = rate / W" and
# "rate * g**k" hold with == whatever W and g are (rate / W and rate * (1 / W) are one rounding
# of the same quotient scaled by a power of two)
RATE2 = 2.0 ** -7


# ------------------------------------------------------------------------------ oracle
def factor_ref(kind, s, W, T, m, E, g):
    """w(s) * d(s), written out from the definition independently of train/optim.py."""
    w = min(1.0, (s + 1) / W) if W > 0 else 1.0
    if kind == "constant":
        d = 1.0
    elif kind in ("linear", "cosine"):
        u = min(max((s - W) / (T - W), 0.0), 1.0)
        if s >= T:
            d = m
        elif kind == "linear":
            d = 1.0 - (1.0 - m) * u
        else:
            d = m + (1.0 - m) * (0.5 * (1.0 + math.cos(math.pi * u)))
    else:
        d = max(m, g ** float(math.floor(max(s - W, 0) / E)))
    return w * d


def lr_ref(cfg, n_steps, rate_decay, base0=None, s0=0):
    """[(lr, base, s)] for the n_steps + 1 states a run goes through: entry k is the state
    after k steps (applied or skipped alike), lr the rate step s0 + k uses."""
    base, s = float(cfg.rate if base0 is None else base0), int(s0)
    out = []
    for _ in range(n_steps + 1):
        f = factor_ref(cfg.lr_schedule, s, cfg.lr_warmup, cfg.lr_total, cfg.lr_min,
                       cfg.lr_step_every, cfg.lr_gamma)
        out.append((base * f, base, s))
        base = base * (1.0 - rate_decay)
        s += 1
    return out


def mk_cfg(kind, W=0, T=40, m=0.0, E=5, g=0.1, **kw):
    """A config of one schedule with only the fields that schedule takes moved."""
    f = dict(lr_schedule=kind, lr_warmup=W, lr_min=m)
    if kind in ("linear", "cosine"):
        f["lr_total"] = T
    if kind == "step":
        f.update(lr_step_every=E, lr_gamma=g)
    f.update(kw)
    return ExperimentConfig().replace(**f)


LR_OFF = ("lr_schedule", "lr_warmup", "lr_total", "lr_min", "lr_step_every", "lr_gamma")


def lr_fields(cfg):
    """The schedule's fields of a config, to lay over another one."""
    return {k: getattr(cfg, k) for k in LR_OFF}


# ------------------------------------------------------------------ 1: LRSchedule == oracle
@pytest.mark.parametrize("kind", KINDS)
def test_lrschedule_equals_the_oracle_bit_for_bit(kind):
    from deep_go_amd.train.optim import LRSchedule
    for W in (0, 1, 7):
        for m in (0.0, 0.1, 1.0):
            for rd in (0.0, 1e-7, 1e-2):
                cfg = mk_cfg(kind, W=W, T=40, m=m, E=5, rate=0.01, rateDecay=rd)
                sch = LRSchedule(cfg)
                want = lr_ref(cfg, 45, rd)
                for lr, base, s in want:
                    assert (sch.rate, sch.base, sch.s) == (lr, base, s), (W, m, rd, s)
                    assert sch.factor(s) == factor_ref(kind, s, W, 40, m, 5, 0.1)
                    sch.step()
                assert 0.0 <= min(x[0] for x in want) and max(x[0] for x in want) <= 0.01


def test_exact_landmarks():
    from deep_go_amd.train.optim import LRSchedule
    T, E, g = 40, 5, 0.1
    for kind in KINDS:
        for W in (1, 7):
            for m in (0.0, 0.1, 1.0):
                sch = LRSchedule(mk_cfg(kind, W=W, T=T, m=m, E=E, g=g, rate=RATE2, rateDecay=0.0))
                lr = lambda s: RATE2 * sch.factor(s)
                # the warm-up starts at rate / W and reaches 1 on step W - 1 (d = 1 until W)
                if kind == "constant":
                    assert sch.factor(W - 1) == 1.0 and lr(0) == RATE2 / W
                    assert all(sch.factor(s) == 1.0 for s in range(W, T + 6))
                if kind in ("linear", "cosine"):
                    assert lr(0) == RATE2 / W                       # (u = 0 through the warm-up)
                    assert sch.factor(W - 1) == 1.0
                    assert lr(W) == RATE2
                    for s in (T, T + 1, T + 5, 10 ** 9):
                        assert lr(s) == m * RATE2
                    if m == 0.0:
                        assert lr(T) == 0.0 and lr(10 ** 9) == 0.0
                if kind == "step":
                    assert lr(0) == RATE2 / W
                    for s in range(W, T + 6):
                        k = (s - W) // E
                        assert lr(s) == RATE2 * max(m, g ** k), (W, m, s)
    # W = 0: no warm-up at all
    for kind in KINDS:
        sch = LRSchedule(mk_cfg(kind, W=0, rate=RATE2, rateDecay=0.0))
        assert sch.factor(0) == 1.0


def test_factor_is_monotone_and_bounded():
    """The warm-up rises to 1, the decay falls to m and stays: a property no single landmark
    gives."""
    for kind in KINDS:
        for m in (0.0, 0.1):
            f = [factor_ref(kind, s, 7, 40, m, 5, 0.1) for s in range(60)]
            assert all(a < b for a, b in zip(f[:6], f[1:7]))
            assert all(a >= b for a, b in zip(f[7:], f[8:]))
            assert all(0.0 <= x <= 1.0 for x in f)
            if kind != "constant":
                assert min(f[7:]) >= m


# ------------------------------------------------------------------ 2: planted defects
def _simulate(cfg, pattern, rd, defect=None):
    """The rates a backend's loop gives over ``pattern`` (True applied, False skipped): entry k
    is the rate step k uses.  ``defect`` plants one mistake."""
    kind, W, T, m = cfg.lr_schedule, cfg.lr_warmup, cfg.lr_total, cfg.lr_min
    E, g = cfg.lr_step_every, cfg.lr_gamma

    def factor(s):
        if defect == "warmup_off_by_one":
            w = min(1.0, s / W) if W > 0 else 1.0
        else:
            w = min(1.0, (s + 1) / W) if W > 0 else 1.0
        if kind == "constant":
            d = 1.0
        elif kind in ("linear", "cosine"):
            u = (s - W) / (T - W)
            if defect != "u_unclamped_below":
                u = max(u, 0.0)
            if defect != "no_floor_past_T":
                u = min(u, 1.0)
            if s >= T and defect != "no_floor_past_T":
                d = m
            elif kind == "linear":
                d = 1.0 - (1.0 - m) * u
            else:
                d = m + (1.0 - m) * (0.5 * (1.0 + math.cos(math.pi * u)))
        else:
            d = max(m, g ** float(max(s - W, 0) // E))
        return w * d

    base, s = float(cfg.rate), 0
    lr = base * factor(s)
    out = []
    for applied in pattern:
        out.append(lr)
        if defect != "base_not_decaying":
            base = base * (1.0 - rd)
        if applied or defect != "s_counts_applied_only":
            s += 1
        if defect == "factor_compounds":
            lr = lr * (1.0 - rd) * factor(s)
        else:
            lr = base * factor(s)
    out.append(lr)
    return out


def _check(lrs, cfg, rd):
    return lrs == [x[0] for x in lr_ref(cfg, len(lrs) - 1, rd)]


DEFECTS = ["warmup_off_by_one", "s_counts_applied_only", "factor_compounds",
           "base_not_decaying", "no_floor_past_T", "u_unclamped_below"]
PATTERN = [True, False, True] + [True] * 45


@pytest.mark.parametrize("kind", ["linear", "cosine"])
def test_the_honest_simulation_passes_the_check(kind):
    cfg = mk_cfg(kind, W=7, T=40, m=0.1, rate=0.01)
    assert _check(_simulate(cfg, PATTERN, 1e-2), cfg, 1e-2)


@pytest.mark.parametrize("kind", ["linear", "cosine"])
@pytest.mark.parametrize("defect", DEFECTS)
def test_planted_defect_fails_the_check(kind, defect):
    cfg = mk_cfg(kind, W=7, T=40, m=0.1, rate=0.01)
    assert not _check(_simulate(cfg, PATTERN, 1e-2, defect), cfg, 1e-2)


# ------------------------------------------------------------------------------ 3: config
def test_config_defaults_old_checkpoints_and_rejections():
    base = ExperimentConfig()
    want = dict(lr_schedule="none", lr_warmup=0, lr_total=0, lr_min=0.0, lr_step_every=0,
                lr_gamma=0.1)
    d = base.to_dict()
    for k, v in want.items():
        assert getattr(base, k) == v and d[k] == v
        del d[k]                                    # an older checkpoint's config
    assert ExperimentConfig.from_dict(d) == base
    # (as the command line gives them)
    cfg = base.replace(lr_schedule="cosine", lr_warmup="200", lr_total="1000", lr_min="0.1")
    assert (cfg.lr_warmup, cfg.lr_total, cfg.lr_min) == (200, 1000, 0.1)
    assert ExperimentConfig.from_dict(cfg.to_dict()) == cfg
    assert base.replace(lr_schedule="constant").lr_schedule == "constant"
    assert base.replace(lr_schedule="step", lr_step_every=3, lr_gamma=1).lr_gamma == 1.0
    assert base.replace(lr_schedule="linear", lr_total=1, lr_min=1).lr_min == 1.0
    with pytest.raises(KeyError):
        base.replace(lr_sched="cosine")

    def refused(field, **kw):
        with pytest.raises(ValueError) as e:
            base.replace(**kw)
        assert field in str(e.value), (field, str(e.value))
    refused("lr_schedule", lr_schedule="exponential")
    ok = dict(lr_schedule="cosine", lr_total=10)
    for bad in (-1, "-3"):
        refused("lr_warmup", **ok, lr_warmup=bad)
        refused("lr_total", lr_schedule="constant", lr_total=bad)
        refused("lr_step_every", lr_schedule="constant", lr_step_every=bad)
    for bad in (-1e-9, 1.0000001, float("nan"), float("inf"), "nan", "-0.5"):
        refused("lr_min", **ok, lr_min=bad)
    for bad in (0, 0.0, -0.1, 1.5, float("nan"), float("inf"), "nan"):
        refused("lr_gamma", lr_schedule="step", lr_step_every=2, lr_gamma=bad)
    # linear | cosine need T > W
    for kind in ("linear", "cosine"):
        refused("lr_total", lr_schedule=kind)
        refused("lr_total", lr_schedule=kind, lr_total=5, lr_warmup=5)
        refused("lr_total", lr_schedule=kind, lr_total=5, lr_warmup=9)
    # step needs E > 0
    refused("lr_step_every", lr_schedule="step")
    # any field moved off its default while lr_schedule=none
    for k, v in (("lr_warmup", 5), ("lr_total", 100), ("lr_min", 0.1), ("lr_step_every", 4),
                 ("lr_gamma", 0.5)):
        refused(k, **{k: v})
    # and a schedule switched off with its fields left behind
    with pytest.raises(ValueError):
        cfg.replace(lr_schedule="none")


# ------------------------------------------------------------------ 4: the CPU trainer
def _exp_cfg(tmp_path, data_root, **kw):
    base = dict(numLayers=3, channelSize=16, batchSize=4, validationSize=4,
                validation_interval=2, log_interval=1, useCuda=False, synthetic=False,
                data_root=data_root, checkpoint_dir=str(tmp_path), seed=3, loader_threads=2,
                prefetch=2, rate=1e-3, rateDecay=1e-2, nan_policy="skip", head_relu=False)
    base.update(kw)
    return ExperimentConfig().replace(**base)


def _rows(path):
    from deep_go_amd.utils.metrics import read_jsonl
    drop = ("time", "boards_per_sec", "runningTime", "name")     # (the clock, the run's id)
    return [{k: v for k, v in r.items() if k not in drop} for r in read_jsonl(path)]


def _cpu_decay(cfg):
    """(the CPU RMSProp never decayed its rate)"""
    return 0.0 if cfg.optimizer == "rmsprop" else cfg.rateDecay


@pytest.mark.parametrize("opt", ["sgd", "rmsprop", "momentum", "adamw"])
def test_constant_without_warmup_trains_bit_identically_to_none(tmp_path, packed_fixture, opt):
    """Five iterations with lr_schedule=constant (W = 0) and with none: parameters, optimizer
    state, rates, validation costs and every record but kind="lr" are the same; none writes no
    lr record; constant writes one per logging iteration, after the others."""
    from deep_go_amd.train.experiment import Experiment
    out = []
    for kind in ("none", "constant"):
        mpath = str(tmp_path / f"m_{kind}.jsonl")
        e = Experiment(_exp_cfg(tmp_path, packed_fixture, optimizer=opt, lr_schedule=kind,
                                metrics_path=mpath), id=f"{opt}_{kind}")
        rates = []
        for _ in range(5):
            e.run(1)
            rates.append(e.backend.rate)
        e.metrics.close()
        out.append((e, _rows(mpath), rates))
    (a, ra, rates_a), (b, rb, rates_b) = out
    assert torch.equal(a.backend.flat_params().view(torch.int32),
                       b.backend.flat_params().view(torch.int32))
    assert rates_a == rates_b
    sa, sb = a.backend.opt.state_dict(), b.backend.opt.state_dict()
    assert set(sa) == set(sb)
    for k in sa:
        assert torch.equal(sa[k], sb[k]) if isinstance(sa[k], torch.Tensor) else sa[k] == sb[k]
    assert a.validation_costs == b.validation_costs and a.train_costs == b.train_costs
    assert not [r for r in ra if r.get("kind") == "lr"]
    assert ra == [r for r in rb if r.get("kind") != "lr"]
    lr_rows = [r for r in rb if r.get("kind") == "lr"]
    assert [r["step"] for r in lr_rows] == [1, 2, 3, 4, 5]
    assert set(lr_rows[0]) == {"kind", "step", "rate", "base_rate", "lr_step"}
    want = lr_ref(b.cfg, 5, _cpu_decay(b.cfg))
    for k, r in enumerate(lr_rows, 1):
        assert (r["rate"], r["base_rate"], r["lr_step"]) == want[k]
        assert r["rate"] == rates_b[k - 1]
    # the lr record is the last one of its iteration
    for k in range(1, 6):
        assert [r["kind"] for r in rb if r.get("step") == k and "kind" in r][-1] == "lr"
    assert (a.backend.base_rate, a.backend.lr_step) == (a.backend.rate, 0)
    assert (b.backend.base_rate, b.backend.lr_step) == (want[5][1], 5)


@pytest.mark.parametrize("opt", ["sgd", "rmsprop", "momentum", "adamw"])
@pytest.mark.parametrize("kind", ["cosine", "step"])
def test_cpu_backend_follows_the_oracle(tmp_path, packed_fixture, opt, kind):
    """The rate of every step equals the oracle's, so the optimizers' own rate *= does not
    compound with the factor; the update really uses it (a run with the oracle's rates set by
    hand ends on the same bits)."""
    from deep_go_amd.data.synthetic import random_planes
    from deep_go_amd.train.backends import CPUBackend
    cfg = _exp_cfg(tmp_path, packed_fixture, optimizer=opt, rate=0.02,
                   **lr_fields(mk_cfg(kind, W=2, T=5, m=0.1, E=2, g=0.5)))
    want = lr_ref(cfg, 6, _cpu_decay(cfg))
    be = CPUBackend(cfg, 4)
    off = {k: getattr(ExperimentConfig(), k) for k in LR_OFF}
    hand = CPUBackend(cfg.replace(**off), 4)
    be.set_batch(*random_planes(4, seed=0))
    hand.set_batch(*random_planes(4, seed=0))
    for k in range(6):
        assert (be.rate, be.base_rate, be.lr_step) == want[k]
        hand.opt.rate = want[k][0]
        be.train_step()
        hand.train_step()
    assert (be.rate, be.base_rate, be.lr_step) == want[6]
    assert torch.equal(be.flat_params().view(torch.int32), hand.flat_params().view(torch.int32))


def test_cpu_apply_skip_apply_counts_three(tmp_path, packed_fixture):
    from deep_go_amd.data.synthetic import random_planes
    from deep_go_amd.train.backends import CPUBackend
    cfg = _exp_cfg(tmp_path, packed_fixture, optimizer="adamw",
                   **lr_fields(mk_cfg("cosine", W=2, T=5, m=0.1)))
    rd = cfg.rateDecay
    want = lr_ref(cfg, 3, rd)
    be = CPUBackend(cfg, 4)
    be.set_batch(*random_planes(4, seed=0))
    assert (be.rate, be.base_rate, be.lr_step) == want[0] and be.rate == cfg.rate / 2
    for k, applied in enumerate([True, False, True]):
        be.forward_backward()
        p = be.flat_params().clone()
        if not applied:
            be._loss_sum = float("nan")
        be.optimizer_step()
        assert (be.rate, be.base_rate, be.lr_step) == want[k + 1]
        assert torch.equal(be.flat_params(), p) == (not applied)
    assert be.lr_step == 3 and be.opt.t == 2 and be.bad_steps() == 1
    assert be.base_rate == cfg.rate * (1 - rd) * (1 - rd) * (1 - rd)


# ------------------------------------------------------------------ 5: checkpoints
def test_checkpoint_round_trip_resume_and_reset(tmp_path, packed_fixture):
    """rate holds base and lr_step travels as an integer; 2 + skip + 2 iterations through a
    checkpoint equal the uninterrupted run bit for bit; --reset-optimizer restarts at base =
    cfg.rate, s = 0; a checkpoint without lr_step loads s = 0 with base = its rate; resumed with
    the schedule off a run continues from base."""
    from deep_go_amd.train.experiment import Experiment
    from deep_go_amd.utils.checkpoint import load_checkpoint
    cfg = _exp_cfg(tmp_path, packed_fixture, optimizer="adamw", validation_interval=1000,
                   **lr_fields(mk_cfg("cosine", W=5, T=9, m=0.1)))
    a = Experiment(cfg, id="a")
    a.run(2)
    a.backend.forward_backward()
    a.backend._loss_sum = float("nan")
    a.backend.optimizer_step()                       # a skipped step: s counts it
    path = a.save()
    _, flat, _, opt = load_checkpoint(path)
    want = lr_ref(cfg, 5, cfg.rateDecay)
    assert opt["lr_step"] == 3 and isinstance(opt["lr_step"], int)
    assert opt["rate"] == want[3][1] == a.backend.base_rate
    assert a.backend.rate == want[3][0] != opt["rate"]       # (still inside the warm-up)
    a2 = Experiment.load(path)
    a2.id = "a2"
    a2.init()
    assert (a2.backend.rate, a2.backend.base_rate, a2.backend.lr_step) == want[3]
    a2.run(2)
    a.run(2)
    assert (a2.backend.rate, a2.backend.base_rate, a2.backend.lr_step) == want[5]
    assert (a.backend.rate, a.backend.base_rate, a.backend.lr_step) == want[5]
    assert torch.equal(a2.backend.flat_params().view(torch.int32),
                       a.backend.flat_params().view(torch.int32))
    # --reset-optimizer: a warm restart
    r = Experiment.load(path, reset_optimizer=True)
    r.init()
    assert (r.backend.rate, r.backend.base_rate, r.backend.lr_step) == want[0]
    # resumed with the schedule off: from the undamped rate
    off = {k: getattr(ExperimentConfig(), k) for k in LR_OFF}
    z = Experiment.load(path, **off)
    z.init()
    assert z.backend.rate == want[3][1] and z.backend.lr_step == 0
    assert "lr_step" not in z.backend.state_dict()["optimizer"]
    # a checkpoint without lr_step, resumed with a schedule
    plain = Experiment(cfg.replace(**off), id="plain")
    plain.run(2)
    ppath = plain.save()
    popt = load_checkpoint(ppath)[3]
    assert "lr_step" not in popt
    s = Experiment.load(ppath, **lr_fields(cfg))
    s.init()
    assert (s.backend.base_rate, s.backend.lr_step) == (popt["rate"], 0)
    assert s.backend.rate == popt["rate"] * factor_ref("cosine", 0, 5, 9, 0.1, 0, 0.1)


def test_cli_train_fills_in_lr_total(tmp_path, packed_fixture, capsys):
    from deep_go_amd import cli
    from deep_go_amd.utils.checkpoint import load_checkpoint
    common = ["numLayers=3", "channelSize=16", "batchSize=4", "validationSize=4",
              "validation_interval=1000", f"data_root={packed_fixture}",
              f"checkpoint_dir={tmp_path}", "loader_threads=2", "prefetch=2", "rate=1e-3"]
    assert cli.main(["train", "--iters", "3", "--device", "cpu", "id=fill", "lr_schedule=cosine",
                     "lr_warmup=1", *common]) == 0
    row = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    cfg, _, _, opt = load_checkpoint(row["checkpoint"])
    assert cfg.lr_total == 3 and cfg.lr_schedule == "cosine"
    assert opt["lr_step"] == 3
    # a given lr_total stays; constant and step take none
    assert cli.main(["train", "--iters", "2", "--device", "cpu", "id=given", "lr_schedule=linear",
                     "lr_total=50", *common]) == 0
    row = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert load_checkpoint(row["checkpoint"])[0].lr_total == 50
    assert cli.main(["train", "--iters", "2", "--device", "cpu", "id=const",
                     "lr_schedule=constant", "lr_warmup=2", *common]) == 0
    row = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert load_checkpoint(row["checkpoint"])[0].lr_total == 0
    # --iters no larger than the warm-up: refused as override refuses it
    with pytest.raises(ValueError):
        cli.main(["train", "--iters", "2", "--device", "cpu", "id=bad", "lr_schedule=cosine",
                  "lr_warmup=2", *common])


# ------------------------------------------------------------------ 6: two ranks
def _dp_worker(rank, world, port, out_dir):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank),
                      WORLD_SIZE=str(world), LOCAL_RANK=str(rank))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from deep_go_amd.data.synthetic import random_planes
    from deep_go_amd.parallel import dp
    from deep_go_amd.train.backends import CPUBackend
    cfg = ExperimentConfig().replace(numLayers=3, channelSize=16, rate=1e-2, seed=5 + rank,
                                     bucket_mb=0.01, lr_schedule="cosine", lr_warmup=2,
                                     lr_total=5, lr_min=0.1)
    B = 8
    be = CPUBackend(cfg, B // world, world=world, bucket_mb=0.01)
    dp.broadcast_(be.params.data, 0)
    rates = [be.rate]
    for step in range(3):
        planes, player, rank_, labels = random_planes(B, seed=step)
        sl = slice(rank * (B // world), (rank + 1) * (B // world))
        be.set_batch(planes[sl], player[sl], rank_[sl], labels[sl])
        be.forward_backward()
        be.optimizer_step()
        rates.append(be.rate)
    torch.save({"rates": rates, "base": be.base_rate, "s": be.lr_step,
                "p": be.flat_params().clone()}, os.path.join(out_dir, f"rank{rank}.pt"))
    dist.barrier()
    dist.destroy_process_group()


def test_two_gloo_ranks_hold_equal_rates(tmp_path):
    mp.spawn(_dp_worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True)
    a = torch.load(str(tmp_path / "rank0.pt"), weights_only=True)
    b = torch.load(str(tmp_path / "rank1.pt"), weights_only=True)
    cfg = mk_cfg("cosine", W=2, T=5, m=0.1, rate=1e-2)
    want = lr_ref(cfg, 3, cfg.rateDecay)
    assert a["rates"] == b["rates"] == [x[0] for x in want]
    assert (a["base"], a["s"]) == (b["base"], b["s"]) == want[3][1:]
    assert torch.equal(a["p"].view(torch.int32), b["p"].view(torch.int32))


# ------------------------------------------------------------------ 7: the launcher
def _sched():
    from deep_go_amd.ops import native
    try:
        return native.sched()
    except Exception as e:                                   # noqa: BLE001
        pytest.skip(f"_dgsched is not built: {e}")


# fake, suitably aligned, non-null addresses: every call below is refused before any launch
_REC, _LR = 0x4000, 0x2008


def test_module_public_names():
    m = _sched()
    assert sorted(x for x in dir(m) if not x.startswith("_")) == ["lr_sched"]


def test_launcher_refuses_invalid_arguments_without_a_gpu():
    """Every refusal happens before any GPU work (no GPU here, and the addresses are fake: a
    launch would not survive them)."""
    m = _sched()

    def call(rec=_REC, lr=_LR, kind=2, W=7, T=40, mn=0.1, E=5, g=0.1, rd=1e-7, advance=1):
        m.lr_sched(rec, lr, kind, W, T, mn, E, g, rd, advance, 0)
    nan, inf = math.nan, math.inf
    bad = {"null rec": dict(rec=0), "null lr": dict(lr=0), "rec misaligned": dict(rec=_REC + 4),
           "lr misaligned": dict(lr=_LR + 4), "kind -1": dict(kind=-1), "kind 4": dict(kind=4),
           "W < 0": dict(W=-1), "T < 0": dict(kind=0, T=-1), "E < 0": dict(E=-1),
           "m < 0": dict(mn=-1e-9), "m > 1": dict(mn=1.5), "m nan": dict(mn=nan),
           "g = 0": dict(g=0.0), "g > 1": dict(g=1.5), "g nan": dict(g=nan), "g inf": dict(g=inf),
           "rd nan": dict(rd=nan), "rd inf": dict(rd=inf), "rd -inf": dict(rd=-inf),
           "cosine T = W": dict(T=7), "cosine T < W": dict(T=3), "linear T = W": dict(kind=1, T=7),
           "cosine T = 0": dict(W=0, T=0), "step E = 0": dict(kind=3, E=0),
           "advance 2": dict(advance=2), "advance -1": dict(advance=-1)}
    for what, kw in bad.items():
        with pytest.raises(RuntimeError) as e:
            call(**kw)
        assert str(e.value) == "lr_sched: invalid argument", what
