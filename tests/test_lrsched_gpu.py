"""lr_schedule on the GPU: ``lr_sched_tick`` (csrc/kernels/sched.hip, module ``_dgsched``) on a
record and a rate of its own between sentinel words against the float64 oracle of
tests/test_lrsched_cpu.py, then inside HipGoNet (eager and as step graphs, bf16 and fp8, every
optimizer, the bf16 wire, without a gate, a skipped step) and through HIPBackend.

The bound.  base and s are the same IEEE double / integer operations on both sides: ``==``.  lr =
base * f(s) with f in [0, 1]: |lr - oracle| <= base * K * 2^-53, K the count of the formula's
double roundings plus the device library's error in ulps:

    constant  w = (s + 1) / W, w * d, base * f                                       K = 3
    linear    those, (s - W) / (T - W), 1 - m, (1 - m) * u, 1 - ...                  K = 7
    cosine    those of linear with m + ... for 1 - ..., pi * u, 1 + cos, and cos     K = 9 + COS_ULPS
    step      those of constant and g^k                                               K = 3 + POW_ULPS

ROCm's OCML documentation is not installed beside the compiler, so COS_ULPS and POW_ULPS are
measured: the worst error of lr over this file's sweep on an MI355X, in units of base * 2^-53,
was 0.000 for cosine and 0.000 for step (test_tick_matches_the_oracle prints them: lr had the
oracle's bits at every point); each constant is twice that, rounded up to an integer, so both
are 0 and the formula's own roundings are the whole bound.  POW_ULPS stands for g^k, which the
kernel does not take from the device library: see test_exact_landmarks.
"""
import math
import os
import subprocess
import sys

import pytest
import torch

from test_lrsched_cpu import KINDS, LR_OFF, RATE2, factor_ref, lr_ref, mk_cfg
from test_update_gpu import guarded, guards_intact, same_bits

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U53 = 2.0 ** -53
MEASURED_COS, MEASURED_POW = 0.0, 0.0       # (worst |lr - oracle| / (base * 2^-53), see above)
COS_ULPS, POW_ULPS = math.ceil(2 * MEASURED_COS), math.ceil(2 * MEASURED_POW)
K_OF = {"constant": 3, "linear": 7, "cosine": 9 + COS_ULPS, "step": 3 + POW_ULPS}

T, E, G = 40, 5, 0.1
BASE = 0.0137


def _m():
    from deep_go_amd.ops.native import sched
    return sched()


def _s():
    from deep_go_amd.ops.native import stream_handle
    return stream_handle()


class Tick:
    """A record {double base; int64 s} and a rate, each between sentinel words."""

    def __init__(self, base, s, lr=-1.0):
        rec = torch.zeros(2, dtype=torch.int64)
        rec[0:1].view(torch.float64)[0] = base
        rec[1] = s
        self.rbuf, self.rec = guarded(rec)
        self.lbuf, self.lr = guarded(torch.tensor([lr], dtype=torch.float64))

    def run(self, cfg, rd, advance):
        _m().lr_sched(self.rec.data_ptr(), self.lr.data_ptr(), KINDS.index(cfg.lr_schedule),
                      cfg.lr_warmup, cfg.lr_total, cfg.lr_min, cfg.lr_step_every, cfg.lr_gamma,
                      rd, advance, _s())
        torch.cuda.synchronize()
        return self.state()

    def state(self):
        """(lr, base, s)"""
        return (self.lr.item(), self.rec[0:1].view(torch.float64).item(), int(self.rec[1].item()))

    def intact(self):
        return guards_intact(self.rbuf) and guards_intact(self.lbuf)


def _s_cases(W):
    return [s for s in (0, 1, W - 1, W, W + 1, (W + T) // 2, T - 1, T, T + 1, 10 ** 9) if s >= 0]


def _f(cfg, s):
    return factor_ref(cfg.lr_schedule, s, cfg.lr_warmup, cfg.lr_total, cfg.lr_min,
                      cfg.lr_step_every, cfg.lr_gamma)


# ===================================================================== A: the tick
@pytest.mark.parametrize("kind", KINDS)
def test_tick_matches_the_oracle(kind):
    """From a planted (base, s): advance = 0 writes lr = base * f(s) within the bound and leaves
    the record's bits; advance = 1 gives base * (1 - rd) and s + 1 exactly and lr within the
    bound; a second launch from the same state gives the same bits; sentinels intact."""
    worst = 0.0
    for W in (0, 7):
        for m in (0.0, 0.1):
            cfg = mk_cfg(kind, W=W, T=T, m=m, E=E, g=G)
            for rd in (0.0, 1e-7):
                for s in _s_cases(W):
                    t = Tick(BASE, s)
                    before = t.rec.clone()
                    lr, base, s_ = t.run(cfg, rd, 0)
                    assert same_bits(t.rec, before) and (base, s_) == (BASE, s)
                    err = abs(lr - BASE * _f(cfg, s)) / (BASE * U53)
                    assert err <= K_OF[kind], (W, m, rd, s, lr, err)
                    worst = max(worst, err)
                    lr1, base1, s1 = t.run(cfg, rd, 1)
                    want = BASE * (1.0 - rd)
                    assert (base1, s1) == (want, s + 1), (W, m, rd, s)
                    err = abs(lr1 - want * _f(cfg, s + 1)) / (want * U53)
                    assert err <= K_OF[kind], (W, m, rd, s + 1, lr1, err)
                    worst = max(worst, err)
                    assert t.intact()
                    again = Tick(BASE, s, lr=7.0)
                    assert again.run(cfg, rd, 1) == (lr1, base1, s1)
                    assert same_bits(again.rec, t.rec) and same_bits(again.lr, t.lr)
                    if m == 0.0 and kind in ("linear", "cosine") and s + 1 >= T:
                        assert lr1 == 0.0
    print(f"LRSCHED_ERR kind={kind} worst |lr - oracle| / (base * 2^-53) = {worst:.3f}")


def test_exact_landmarks():
    """rateDecay = 0 and a power-of-two base (base * x is then exact): the landmarks of
    tests/test_lrsched_cpu.py hold with ==.  step: g = 0.5, whose powers are exact doubles, and
    g = 0.1 against the host's pow (the kernel raises g to an integer power in double-double
    arithmetic and rounds once; the device library's pow returned 0.5^4 one ulp low)."""
    def lr(cfg, s):
        return Tick(RATE2, s).run(cfg, 0.0, 0)[0]
    for W in (1, 7):
        for m in (0.0, 0.1):
            for kind in KINDS:
                cfg = mk_cfg(kind, W=W, T=T, m=m, E=E, g=0.5)
                assert lr(cfg, 0) == RATE2 / W, (kind, W, m)
                assert lr(cfg, W - 1) == RATE2, (kind, W, m)        # (w(W - 1) = 1, d = 1)
                if kind == "constant":
                    assert lr(cfg, W) == RATE2 and lr(cfg, 10 ** 9) == RATE2
                if kind in ("linear", "cosine"):
                    assert lr(cfg, W) == RATE2
                    for s in (T, T + 1, 10 ** 9):
                        assert lr(cfg, s) == m * RATE2, (kind, W, m, s)
                if kind == "step":
                    for g in (0.5, 0.1):
                        cfg = mk_cfg(kind, W=W, T=T, m=m, E=E, g=g)
                        for s in list(range(W, T + 6, 2)) + [10 ** 9]:
                            k = (s - W) // E
                            assert lr(cfg, s) == RATE2 * max(m, g ** k), (W, m, g, s)


# ===================================================================== B: in the model
# (tests/test_ema_gpu.py's model cases and helpers, which are tests/test_clip_gpu.py's)
MODEL_CASES = {"3x64-bf16": (3, 64, "bf16"), "4x128-bf16": (4, 128, "bf16"),
               "4x128-fp8": (4, 128, "fp8")}
B = 8
RATE_DECAY = 1e-3
OPTIMIZERS = ["sgd", "rmsprop", "momentum", "adamw"]
_OPT_KW = {"sgd": dict(rate=0.01), "rmsprop": dict(rate=1e-3),
           "momentum": dict(rate=0.01, momentum=0.9, nesterov=True, weight_decay=1e-3),
           "adamw": dict(rate=1e-5, weight_decay=1e-2)}
COSINE = dict(lr_schedule="cosine", lr_warmup=2, lr_total=5, lr_min=0.1)


def _cfg(layers, ch, dtype, opt, **kw):
    from deep_go_amd.config import ExperimentConfig
    base = dict(numLayers=layers, channelSize=ch, batchSize=B, seed=5, dtype=dtype,
                rateDecay=RATE_DECAY, optimizer=opt, head_relu=False, **_OPT_KW[opt])
    base.update(kw)
    return ExperimentConfig().replace(**base)


def _batch(n, seed):
    from deep_go_amd.data.synthetic import random_planes
    return [torch.from_numpy(a).cuda() for a in random_planes(n, seed=seed)]


def _opt_state(net):
    """name -> tensor of whatever the net's optimizer keeps"""
    out = {}
    for k in ("ms", "vel", "adam_m", "adam_v", "adam_t"):
        t = getattr(net, k)
        if t is not None:
            out[k] = t
    return out


def _net(name, opt, sched=COSINE, **kw):
    from deep_go_amd.models.hip_model import HipGoNet
    layers, ch, dtype = MODEL_CASES[name]
    net_kw = {k: kw.pop(k) for k in ("global_batch", "grad_wire") if k in kw}
    return HipGoNet(_cfg(layers, ch, dtype, opt, **sched, **kw), B, device="cuda", **net_kw)


def _follows(net, before, want, tag):
    """After a step from the state ``before`` = (base, s): the record equals the oracle's entry
    ``want`` = (lr, base, s) exactly, and lr has the bits of a standalone tick fed ``before``
    (and so lies within the bound of the oracle)."""
    cfg = net.cfg
    base, s = net.lr_schedule_state()
    assert (base, s) == want[1:], tag
    lr = Tick(*before).run(cfg, cfg.rateDecay, 1)[0]
    assert net.lr.item() == lr, tag
    assert abs(lr - want[0]) <= base * K_OF[cfg.lr_schedule] * U53, tag


@pytest.mark.parametrize("opt", OPTIMIZERS)
@pytest.mark.parametrize("name", list(MODEL_CASES))
def test_five_steps_follow_the_oracle(name, opt):
    """cosine, W = 2, T = 5, m = 0.1 over five train_step()s (warm-up, the decay, the floor): after
    every step lr equals a standalone tick fed the same state and (base, s) the oracle.  A net
    without a schedule whose rate is set by hand to the scheduled one before every step ends on
    the same parameters and optimizer state, bit for bit: every launch of the step that reads
    the rate read the scheduled one (4x128: with the early update of the deferred step forced
    for sgd | rmsprop)."""
    net, hand = _net(name, opt), _net(name, opt, sched={})
    assert net.lr_rec is not None and hand.lr_rec is None
    if name != "3x64-bf16" and opt in ("sgd", "rmsprop"):
        for x in (net, hand):
            x._early_ok, x._early_env = True, "1"
    want = lr_ref(net.cfg, 5, RATE_DECAY)
    assert net.lr_schedule_state() == want[0][1:] and net.lr.item() == want[0][0]
    assert net.lr.item() == net.cfg.rate * 0.5
    for k in range(1, 6):
        before = net.lr_schedule_state()
        hand.lr.copy_(net.lr)
        batch = _batch(B, 12 + k)
        for x in (net, hand):
            x.set_batch(*batch)
            x.train_step()
        torch.cuda.synchronize()
        _follows(net, before, want[k], (name, opt, k))
        assert same_bits(net.params, hand.params), (name, opt, k)
        sa, sb = _opt_state(net), _opt_state(hand)
        assert set(sa) == set(sb) and all(same_bits(sa[x], sb[x]) for x in sa), (name, opt, k)
        assert int(net.step_count.item()) == k
    assert net.lr.item() == net.lr_schedule_state()[0] * 0.1        # (the floor, from s = T on)


@pytest.mark.parametrize("opt", OPTIMIZERS)
@pytest.mark.parametrize("name", list(MODEL_CASES))
def test_constant_without_warmup_equals_none_bit_for_bit(name, opt):
    """lr_schedule=constant, W = 0 beside none over three train_step()s: parameters, optimizer
    state, loss, pred, the rate and _stepflag are equal after every step; sgd | rmsprop keep the
    fused, deferred update either way."""
    a, b = _net(name, opt, sched=dict(lr_schedule="constant")), _net(name, opt, sched={})
    assert a.can_defer() == b.can_defer()
    if name == "4x128-bf16":
        assert a.can_defer() == (opt in ("sgd", "rmsprop"))
    for k in range(1, 4):
        batch = _batch(B, 12 + k)
        for x in (a, b):
            x.set_batch(*batch)
            x.train_step()
        torch.cuda.synchronize()
        tag = (name, opt, k)
        assert same_bits(a.params, b.params) and same_bits(a.lr, b.lr), tag
        assert same_bits(a.loss, b.loss) and same_bits(a.pred, b.pred), tag
        sa, sb = _opt_state(a), _opt_state(b)
        assert set(sa) == set(sb) and all(same_bits(sa[x], sb[x]) for x in sa), tag
        assert same_bits(a._stepflag, b._stepflag) and same_bits(a.bad_steps, b.bad_steps), tag
        assert a.lr_schedule_state() == (a.lr.item(), k)
    assert a.lr.item() < a.cfg.rate


@pytest.mark.parametrize("opt", ["sgd", "adamw"])
@pytest.mark.parametrize("name", list(MODEL_CASES))
def test_step_graph_gives_the_eager_bits(name, opt):
    """SegmentedStep(use_graphs=True) against the eager step from the same state over three
    steps, then forward_backward() and optimizer() as graphs of their own: parameters,
    optimizer state, the rate and the record, bit for bit.  Construction, warm-up and capture
    leave s = 0 and lr at its first value."""
    from deep_go_amd.models.hip_model import SegmentedStep
    nets = [_net(name, opt) for _ in range(2)]
    want = lr_ref(nets[0].cfg, 4, RATE_DECAY)
    steps = []
    for net, graphs in zip(nets, (False, True)):
        net.set_batch(*_batch(B, 12))
        steps.append(SegmentedStep(net, None, use_graphs=graphs))
        torch.cuda.synchronize()
        assert net.lr_schedule_state() == want[0][1:] and net.lr.item() == want[0][0]
    assert steps[1].full_graph is not None and steps[0].full_graph is None
    e, g = nets
    for k in range(1, 4):
        before = g.lr_schedule_state()
        for step in steps:
            step()
        torch.cuda.synchronize()
        assert same_bits(e.params, g.params) and same_bits(e.lr, g.lr), k
        assert same_bits(e.lr_rec, g.lr_rec), k
        se, sg = _opt_state(e), _opt_state(g)
        assert all(same_bits(se[x], sg[x]) for x in se), k
        _follows(g, before, want[k], (name, opt, k))
    before = g.lr_schedule_state()
    for step in steps:
        step.forward_backward()
        step.optimizer()
    torch.cuda.synchronize()
    assert same_bits(e.params, g.params) and same_bits(e.lr, g.lr)
    assert same_bits(e.lr_rec, g.lr_rec)
    _follows(g, before, want[4], (name, opt, "segments"))


@pytest.mark.parametrize("opt", ["sgd", "adamw"])
def test_bf16_wire_keeps_the_schedule(opt):
    """grad_wire=bf16 (the optimizer reads the twin) beside fp32 gradients: the schedule's state
    and the rate are equal after every step, and follow the oracle."""
    w = _net("4x128-bf16", opt, global_batch=2 * B, grad_wire="bf16")
    f = _net("4x128-bf16", opt, global_batch=2 * B)
    assert w.grads16 is not None and f.grads16 is None
    want = lr_ref(w.cfg, 3, RATE_DECAY)
    batch = _batch(B, 12)
    p0 = w.params.clone()
    for k in range(1, 4):
        before = w.lr_schedule_state()
        for x in (w, f):
            x.set_batch(*batch)
            x.forward_backward()
            x.optimizer_step()
        torch.cuda.synchronize()
        assert same_bits(w.lr_rec, f.lr_rec) and same_bits(w.lr, f.lr), (opt, k)
        _follows(w, before, want[k], (opt, k))
    assert not torch.equal(w.params, p0)


@pytest.mark.parametrize("opt", ["sgd", "adamw"])
def test_schedule_without_a_gate(opt):
    """nan_policy=raise: no gate launch and no gate pointer; the launch takes none anyway."""
    net = _net("3x64-bf16", opt, nan_policy="raise")
    want = lr_ref(net.cfg, 2, RATE_DECAY)
    net.set_batch(*_batch(B, 12))
    net.gate.zero_()                        # (nothing may read it)
    for k in (1, 2):
        before = net.lr_schedule_state()
        p = net.params.clone()
        net.forward_backward()
        net.optimizer_step()
        torch.cuda.synchronize()
        _follows(net, before, want[k], (opt, k))
        assert not torch.equal(net.params, p) and net.gate.item() == 0.0


@pytest.mark.parametrize("opt", ["sgd", "adamw"])
def test_skipped_step_counts(opt):
    """nan_policy=skip: a clean step, then a poisoned loss: the parameters keep their bits while
    s and base advance and lr follows (the rate already decayed on a skipped step); then a clean
    step again (sgd: grad_update's gate; adamw: its own launches')."""
    net = _net("4x128-bf16", opt, nan_policy="skip")
    want = lr_ref(net.cfg, 3, RATE_DECAY)
    net.set_batch(*_batch(B, 12))
    before = net.lr_schedule_state()
    net.forward_backward()
    net.optimizer_step()
    torch.cuda.synchronize()
    _follows(net, before, want[1], "clean")
    p0, before = net.params.clone(), net.lr_schedule_state()
    net.forward_backward()
    net.loss[0] = float("inf")
    net.optimizer_step()
    torch.cuda.synchronize()
    assert same_bits(net.params, p0) and net.bad_steps.item() == 1 and net.gate.item() == 0.0
    _follows(net, before, want[2], "skipped")
    assert net.lr_schedule_state()[1] == 2 == int(net.step_count.item())
    before = net.lr_schedule_state()
    net.forward_backward()
    net.optimizer_step()
    torch.cuda.synchronize()
    assert net.gate.item() == 1.0 and not torch.equal(net.params, p0)
    _follows(net, before, want[3], "after the skip")


def test_set_and_reset_rewrite_the_rate_on_the_device():
    net = _net("3x64-bf16", "sgd")
    net.set_lr_schedule_state(0.5, 3)
    torch.cuda.synchronize()
    assert net.lr_schedule_state() == (0.5, 3)
    assert net.lr.item() == Tick(0.5, 3).run(net.cfg, RATE_DECAY, 0)[0]
    net.reset_lr_schedule()
    assert net.lr_schedule_state() == (net.cfg.rate, 0) and net.lr.item() == net.cfg.rate * 0.5
    plain = _net("3x64-bf16", "sgd", sched={})
    plain.reset_lr_schedule()                        # (nothing to do)
    with pytest.raises(RuntimeError):
        plain.lr_schedule_state()
    with pytest.raises(RuntimeError):
        plain.set_lr_schedule_state(0.1, 0)


_CHILD = """
import sys
sys.path.insert(0, {root!r})
import torch
from deep_go_amd.config import ExperimentConfig
from deep_go_amd.models.hip_model import HipGoNet
cfg = ExperimentConfig(numLayers=4, channelSize=128, batchSize=8, seed=5, dtype="bf16")
net = HipGoNet(cfg, 8, device="cuda")
assert "_dgsched" not in sys.modules, "lr_schedule=none imported _dgsched"
assert net.lr_rec is None
assert net.can_defer(), "lr_schedule=none: the default step no longer defers"
s = HipGoNet(cfg.replace(lr_schedule="cosine", lr_warmup=2, lr_total=5), 8, device="cuda")
assert "_dgsched" in sys.modules and s.can_defer()
print("CHILD_OK")
"""


def test_module_is_imported_only_for_a_schedule():
    """In a fresh process: with lr_schedule=none _dgsched is not imported; with a schedule it is,
    and the default 4x128 step defers either way."""
    env = dict(os.environ)
    env.pop("DG_FUSED_UPDATE", None)
    r = subprocess.run([sys.executable, "-c", _CHILD.format(root=ROOT)], env=env,
                       capture_output=True, text=True, timeout=100)
    assert r.returncode == 0 and "CHILD_OK" in r.stdout, r.stderr[-3000:]


# ===================================================================== C: HIPBackend
def test_hip_backend_resume_in_the_warmup_is_exact(tmp_path):
    """cosine, W = 5, T = 9, the second step skipped: 5 steps == 2 steps + state_dict -> a new
    backend + load_state_dict + 3 steps, bit for bit on the parameters, the moments, the rate and
    the record.  rate holds base, lr_step is an integer; a state without lr_step loads s = 0 with
    base = its rate."""
    from deep_go_amd.data.synthetic import random_planes
    from deep_go_amd.train.backends import HIPBackend
    sched = dict(lr_schedule="cosine", lr_warmup=5, lr_total=9, lr_min=0.1)
    cfg = _cfg(3, 64, "bf16", "adamw", batchSize=4, checkpoint_dir=str(tmp_path),
               nan_policy="skip", **sched)
    want = lr_ref(cfg, 5, RATE_DECAY)
    batches = [random_planes(4, seed=20 + i) for i in range(5)]

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
    assert (a.rate, a.base_rate, a.lr_step) == want[0]
    run(a, range(5))
    assert a.bad_steps() == 1 and a.net.adam_steps() == 4 and a.lr_step == 5
    b = HIPBackend(cfg, 4, flat=p_init)
    run(b, range(2))
    o = b.state_dict()["optimizer"]
    assert o["lr_step"] == 2 and type(o["lr_step"]) is int
    assert o["rate"] == want[2][1] == b.base_rate and b.rate != o["rate"]
    c = HIPBackend(cfg, 4, flat=b.flat_params())
    assert c.lr_step == 0
    c.load_state_dict({"optimizer": o})
    assert same_bits(c.net.lr, b.net.lr) and same_bits(c.net.lr_rec, b.net.lr_rec)
    run(c, range(2, 5))
    assert torch.equal(c.net.params, a.net.params)
    assert torch.equal(c.net.adam_m, a.net.adam_m) and torch.equal(c.net.adam_v, a.net.adam_v)
    assert same_bits(c.net.lr, a.net.lr) and same_bits(c.net.lr_rec, a.net.lr_rec)
    assert (c.base_rate, c.lr_step) == want[5][1:]
    assert abs(c.rate - want[5][0]) <= c.base_rate * K_OF["cosine"] * U53
    # a state without lr_step
    old = {"optimizer": {k: v for k, v in o.items() if k != "lr_step"}}
    c.load_state_dict(old)
    assert (c.base_rate, c.lr_step) == (o["rate"], 0) and c.rate == o["rate"] * 0.2
    # a backend without a schedule: rate is base, no lr_step in its state
    off = {k: getattr(type(cfg)(), k) for k in LR_OFF}
    d = HIPBackend(cfg.replace(**off), 4, flat=p_init)
    d.load_state_dict({"optimizer": o})
    assert d.rate == d.base_rate == o["rate"] and d.lr_step == 0
    assert "lr_step" not in d.state_dict()["optimizer"]
    for be in (a, b, c, d):
        be.close()


def test_gpu_step_matches_cpu_step(tmp_path):
    """test_momentum_gpu.test_gpu_step_matches_cpu_step's set-up and tolerance with
    optimizer=sgd and one step inside the warm-up (W = 2: half the rate): relative update
    difference < 0.05; the two backends' schedule states are equal."""
    from deep_go_amd.config import ExperimentConfig
    from deep_go_amd.data.synthetic import random_planes
    from deep_go_amd.train.backends import CPUBackend, HIPBackend
    cfg = ExperimentConfig(numLayers=4, channelSize=64, batchSize=32, validationSize=64,
                           validation_interval=10, log_interval=5, useCuda=True, synthetic=True,
                           checkpoint_dir=str(tmp_path), seed=2, loader_threads=4, prefetch=3,
                           rate=0.05, head_relu=False, optimizer="sgd").replace(**COSINE)
    cpu_be = CPUBackend(cfg, 16)
    gpu_be = HIPBackend(cfg, 16, flat=cpu_be.flat_params().clone())
    assert cpu_be.rate == gpu_be.rate == 0.025
    batch = random_planes(16, seed=4)
    for be in (cpu_be, gpu_be):
        be.set_batch(*batch)
        be.forward_backward()
        be.optimizer_step()
    p0 = CPUBackend(cfg, 16).flat_params()
    da, db = cpu_be.flat_params() - p0, gpu_be.flat_params() - p0
    rel = ((da - db).norm() / da.norm()).item()
    print(f"LRSCHED_CPU_GPU relative update difference {rel:.4f}")
    assert rel < 0.05, rel
    assert (cpu_be.base_rate, cpu_be.lr_step) == (gpu_be.base_rate, gpu_be.lr_step)
    assert cpu_be.rate == gpu_be.rate == cpu_be.base_rate       # (s = 1 = W - 1: w = 1, d = 1)
    gpu_be.close()
