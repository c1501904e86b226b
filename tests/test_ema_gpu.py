"""ema_decay on the GPU: the two kernels of csrc/kernels/ema.hip (module _dgema) against the
float64 oracle and the counted bound of tests/test_ema_cpu.py, bit-exactly on designed data,
inside HipGoNet (eager and as step graphs, bf16 and fp8, every optimizer, without a gate
pointer), the skip policy, the import check, ``ema_weights()``, exact resume and the fp32 CPU
trainer.

Buffers under test — the parameters, the average and the 16-byte record {int64 t; float omd;
float pad} — sit between sentinel runs (test_update_gpu.guarded).
"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from test_clip_gpu import B, MODEL_CASES, OPTIMIZERS, _batch, _cfg, _opt_state
from test_ema_cpu import (CAP, DESIGNED_DECAY, DESIGNED_T0, MT, SIZES, designed_case, ema_bound,
                          ema_ref, omd_of)
from test_update_gpu import DEV, guarded, guards_intact, same_bits

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAD = 0x5A5A5A5A           # what the record's pad holds before a launch: nothing writes it
BIG = SIZES[-1]


def _ema():
    from deep_go_amd.ops.native import ema
    return ema()


def _s():
    from deep_go_amd.ops.native import stream_handle
    return stream_handle()


def _rec(t: int, omd_bits: int = 0x7FC00000) -> torch.Tensor:
    """the record as two int64: t | omd's bits (a NaN unless given) with the pad above them"""
    return torch.tensor([t, (PAD << 32) | omd_bits], dtype=torch.int64)


class _Bufs:
    """The device buffers of one kernel-level case, each between sentinels."""

    def __init__(self, p: torch.Tensor, e: torch.Tensor, t0: int):
        self.n, self.p_in, self.e_in, self.t0 = p.numel(), p.float(), e.float(), t0
        self.pbuf, self.p = guarded(self.p_in)
        self.ebuf, self.e = guarded(self.e_in)
        self.rbuf, self.rec = guarded(_rec(t0))

    def launch(self, decay, gate=None):
        _ema().ema(self.p.data_ptr(), self.e.data_ptr(), self.n, self.rec.data_ptr(), decay,
                   gate.data_ptr() if gate is not None else 0, _s())
        torch.cuda.synchronize()
        assert all(guards_intact(b) for b in (self.pbuf, self.ebuf, self.rbuf))
        assert same_bits(self.p, self.p_in)            # (the parameters are only read)

    def reset(self):
        self.e.copy_(self.e_in)
        self.rec.copy_(_rec(self.t0))

    def record(self):
        """(t, omd, pad bits)"""
        t, w = self.rec.tolist()
        omd = np.array([w & 0xFFFFFFFF], dtype=np.uint32).view(np.float32)[0]
        return t, float(omd), (w >> 32) & 0xFFFFFFFF


def _check_step(got, e0, p, omd, tag):
    """got (fp32) against the float64 step from e0, p with omd, within ema_bound -> the largest
    error over its bound."""
    ref = e0.double() + omd * (p.double() - e0.double())
    ratio = ((got.double() - ref).abs() / ema_bound(e0, p, omd).to(got.device)).max().item()
    assert ratio <= 1.0, (tag, ratio)
    return ratio


# ===================================================================== A: the kernels
@pytest.mark.parametrize("n", SIZES)
def test_ema_matches_float64_reference(n):
    """Gaussian parameters and an average near them, decay 0.999, on the ramp (t 0 -> 1) and
    past it (t 5000 -> 5001): the average within ema_bound of ema_ref, the record's count and
    omd exactly the oracle's, the pad and the parameters untouched.  A closed gate keeps the
    average and the record; an open one behaves as none; two launches on the same input give
    the same bits.

    Measured on an MI355X, the largest error over its bound: 0.16 / 0.77 / 0.55 / 0.73 at n = 1
    / 3 / 4 / 5, 0.96 at 1027, 0.999 and 1.000 (to three places) at the two sizes past 8 M elements:
    the bound is tight, a result just above a power of two rounded by nearly half an ulp
    reaches it."""
    gen = torch.Generator().manual_seed(700 + n % 1000)
    p = torch.randn(n, generator=gen) * 0.7
    e = p + torch.randn(n, generator=gen) * 0.05
    worst = 0.0
    for t0 in (0, 5000):
        b = _Bufs(p, e, t0)
        b.launch(0.999)
        t, omd, pad = b.record()
        assert t == t0 + 1 and omd == omd_of(0.999, t0 + 1) and pad == PAD
        got = b.e.cpu()
        ref, _ = ema_ref(e, [p], 0.999, t0=t0)
        ratio = ((got.double() - ref).abs() / ema_bound(e, p, omd)).max().item()
        worst = max(worst, ratio)
        assert ratio <= 1.0, (t0, ratio)
        assert not torch.equal(got, e)
        first = (b.rec.clone(), b.e.clone())
        # ---- again on the same input: the same bits
        b.reset()
        b.launch(0.999)
        assert same_bits(b.rec, first[0]) and same_bits(b.e, first[1])
        # ---- a closed gate, over what the last launch left
        b.launch(0.999, gate=torch.zeros(1, device=DEV))
        assert same_bits(b.rec, first[0]) and same_bits(b.e, first[1])
        # ---- an open gate behaves as none
        b.reset()
        b.launch(0.999, gate=torch.ones(1, device=DEV))
        assert same_bits(b.rec, first[0]) and same_bits(b.e, first[1])
    print(f"EMA_ERR n={n} worst err_over_bound={worst:.3f}")


@pytest.mark.parametrize("n", SIZES)
def test_designed_data_is_bit_exact(n):
    """Integers with omd = 0.25 (decay 0.75 past the ramp): the result is exact."""
    e0, p, want = designed_case(n, 40 + n % 1000)
    b = _Bufs(p, e0, DESIGNED_T0)
    b.launch(DESIGNED_DECAY)
    assert b.record() == (DESIGNED_T0 + 1, 0.25, PAD)
    assert same_bits(b.e, want)


@pytest.mark.parametrize("n", [1027, BIG])
def test_every_region_counts(n):
    """One parameter replaced at a time — in the first vector, in a vector of the second
    grid-stride pass, in the last vector, each tail element: exactly that element of the
    average moves, to the oracle's value."""
    gen = torch.Generator().manual_seed(900 + n % 1000)
    p = torch.randn(n, generator=gen) * 0.7
    e = p + torch.randn(n, generator=gen) * 0.05
    n4 = n // 4
    places = {"first vector": 2, "last vector": 4 * n4 - 3}
    if n > 4 * MT * CAP:
        places["second pass"] = 4 * MT * CAP + 5
    for j in range(n % 4):
        places[f"tail {j}"] = 4 * n4 + j
    assert n % 4 == 3
    b = _Bufs(p, e, 50)
    b.launch(0.9)
    base = b.e.clone()
    omd = omd_of(0.9, 51)
    for what, i in places.items():
        p2 = p.clone()
        p2[i] = 64.0
        b2 = _Bufs(p2, e, 50)
        b2.launch(0.9)
        moved = (b2.e != base).nonzero().flatten().tolist()
        assert moved == [i], (what, i, moved[:5])
        _check_step(b2.e[i:i + 1].cpu(), e[i:i + 1], p2[i:i + 1], omd, what)


TICK_T = [0, 1, 7, 8, 9, 999, 10 ** 9]
TICK_DECAY = [0.5, 0.999, 0.9999]


def test_tick_is_the_float64_value():
    """ema_tick alone from a planted count: t + 1 and omd == float32(1 - min(decay, (2 + t) /
    (11 + t))) exactly (both sides are the same IEEE double operations), the pad untouched;
    the cases include the crossover of the ramp and the cap (decay 0.5: t + 1 = 8).  Behind a
    closed gate nothing is written."""
    m = _ema()
    for decay in TICK_DECAY:
        for t in TICK_T:
            rbuf, rec = guarded(_rec(t))
            m.ema_tick(rec.data_ptr(), decay, 0, _s())
            torch.cuda.synchronize()
            t1, w = rec.tolist()
            omd = float(np.array([w & 0xFFFFFFFF], dtype=np.uint32).view(np.float32)[0])
            assert t1 == t + 1 and omd == omd_of(decay, t + 1), (decay, t, omd)
            assert (w >> 32) & 0xFFFFFFFF == PAD and guards_intact(rbuf)
            before = rec.clone()
            m.ema_tick(rec.data_ptr(), decay, torch.zeros(1, device=DEV).data_ptr(), _s())
            torch.cuda.synchronize()
            assert same_bits(rec, before)
    assert omd_of(0.5, 8) == 0.5 and omd_of(0.5, 7) > 0.5 and omd_of(0.9999, 10 ** 9 + 1) < 2e-4


# ===================================================================== B: in the model
DECAY = 0.9


def _nets(name, opt, **kw):
    from deep_go_amd.models.hip_model import HipGoNet
    layers, ch, dtype = MODEL_CASES[name]
    a = HipGoNet(_cfg(layers, ch, dtype, opt, ema_decay=DECAY, **kw), B, device="cuda")
    b = HipGoNet(_cfg(layers, ch, dtype, opt, **kw), B, device="cuda")
    assert a.ema is not None and a.ema_rec is not None and b.ema is None and b.ema_rec is None
    assert same_bits(a.ema, a.params) and a.ema_steps() == 0 and not a.ema_rec.any()
    assert a.ema.data_ptr() != a.params.data_ptr()
    return a, b


def _same_training_state(a, b, tag):
    assert torch.equal(a.params, b.params), tag
    assert torch.equal(a.loss, b.loss) and torch.equal(a.pred, b.pred), tag
    sa, sb = _opt_state(a), _opt_state(b)
    assert set(sa) == set(sb) and all(torch.equal(sa[k], sb[k]) for k in sa), tag
    assert a.lr.item() == b.lr.item(), tag
    assert torch.equal(a._stepflag, b._stepflag) and torch.equal(a.bad_steps, b.bad_steps), tag


@pytest.mark.parametrize("opt", OPTIMIZERS)
@pytest.mark.parametrize("name", list(MODEL_CASES))
def test_average_follows_the_oracle_and_changes_nothing(name, opt):
    """An ema_decay net beside a plain one over three train_step()s (sgd | rmsprop: the fused,
    deferred update, which both keep): parameters, optimizer state, losses, predictions and the
    rate are equal after every step; the average follows the oracle fed the net's own
    parameters, step by step within ema_bound; the count follows."""
    a, b = _nets(name, opt)
    assert a.can_defer() == b.can_defer()
    if name == "4x128-bf16":
        assert a.can_defer() == (opt in ("sgd", "rmsprop"))
    worst = 0.0
    for t in range(1, 4):
        batch = _batch(B, 12 + t)
        e0 = a.ema.clone()
        for net in (a, b):
            net.set_batch(*batch)
            net.train_step()
        torch.cuda.synchronize()
        _same_training_state(a, b, (name, opt, t))
        assert a.ema_steps() == t == int(a.step_count.item())
        worst = max(worst, _check_step(a.ema, e0, a.params, omd_of(DECAY, t), (name, opt, t)))
        assert not torch.equal(a.ema, e0) and not torch.equal(a.ema, a.params)
    print(f"EMA_ERR model name={name} opt={opt} worst err_over_bound={worst:.3f}")


@pytest.mark.parametrize("opt", ["sgd", "adamw"])
@pytest.mark.parametrize("name", list(MODEL_CASES))
def test_step_graph_gives_the_eager_bits(name, opt):
    """SegmentedStep(use_graphs=True) against the eager step from the same state over three
    steps: parameters, optimizer state, the average and its record, bit for bit; warm-up and
    capture leave t = 0 and the average equal to the parameters."""
    from deep_go_amd.models.hip_model import HipGoNet, SegmentedStep
    layers, ch, dtype = MODEL_CASES[name]
    cfg = _cfg(layers, ch, dtype, opt, ema_decay=DECAY)
    nets = [HipGoNet(cfg, B, device="cuda") for _ in range(2)]
    steps = []
    for net, graphs in zip(nets, (False, True)):
        net.set_batch(*_batch(B, 12))
        steps.append(SegmentedStep(net, None, use_graphs=graphs))
        torch.cuda.synchronize()
        assert not net.ema_rec.any() and same_bits(net.ema, net.params)
    assert steps[1].full_graph is not None and steps[0].full_graph is None
    e, g = nets
    for t in range(1, 4):
        for step in steps:
            step()
        torch.cuda.synchronize()
        assert same_bits(e.params, g.params) and same_bits(e.ema, g.ema), t
        assert same_bits(e.ema_rec, g.ema_rec) and g.ema_steps() == t, t
        se, sg = _opt_state(e), _opt_state(g)
        assert all(same_bits(se[k], sg[k]) for k in se), t
        assert not torch.equal(g.ema, g.params)
    # forward/backward and the optimizer as graphs of their own
    for net, step in zip(nets, steps):
        step.forward_backward()
        step.optimizer()
    torch.cuda.synchronize()
    assert same_bits(e.params, g.params) and same_bits(e.ema, g.ema)
    assert same_bits(e.ema_rec, g.ema_rec) and g.ema_steps() == 4


@pytest.mark.parametrize("opt", ["sgd", "adamw"])
def test_average_without_a_gate(opt):
    """nan_policy=raise: no gate launch and no gate pointer; the same average."""
    a, b = _nets("3x64-bf16", opt, nan_policy="raise")
    batch = _batch(B, 12)
    for net in (a, b):
        net.set_batch(*batch)
        net.gate.zero_()                    # (nothing may read it)
    for t in (1, 2):
        e0 = a.ema.clone()
        for net in (a, b):
            net.forward_backward()
            net.optimizer_step()
        torch.cuda.synchronize()
        _same_training_state(a, b, (opt, t))
        _check_step(a.ema, e0, a.params, omd_of(DECAY, t), (opt, t))
        assert a.ema_steps() == t and a.gate.item() == 0.0


@pytest.mark.parametrize("opt", ["sgd", "adamw"])
def test_skipped_step_moves_nothing(opt):
    """nan_policy=skip: a clean step, then a poisoned loss: the parameters, the average and its
    record keep their bits while step_count advances and the rate decays; the next clean step
    averages again with t = 2 (sgd: grad_update's gate; adamw: its own launches')."""
    from deep_go_amd.models.hip_model import HipGoNet
    net = HipGoNet(_cfg(4, 128, "bf16", opt, ema_decay=DECAY, nan_policy="skip"), B,
                   device="cuda")
    net.set_batch(*_batch(B, 12))
    net.forward_backward()
    net.optimizer_step()
    torch.cuda.synchronize()
    assert net.ema_steps() == 1 and net.bad_steps.item() == 0
    p0, e0, rec0, lr0 = net.params.clone(), net.ema.clone(), net.ema_rec.clone(), net.lr.item()
    net.forward_backward()
    net.loss[0] = float("inf")
    net.optimizer_step()
    torch.cuda.synchronize()
    assert same_bits(net.params, p0) and same_bits(net.ema, e0) and same_bits(net.ema_rec, rec0)
    assert net.bad_steps.item() == 1 and net.gate.item() == 0.0
    assert int(net.step_count.item()) == 2 and net.ema_steps() == 1
    assert net.lr.item() < lr0
    net.forward_backward()
    net.optimizer_step()
    torch.cuda.synchronize()
    assert net.gate.item() == 1.0 and net.ema_steps() == 2 and int(net.step_count.item()) == 3
    _check_step(net.ema, e0, net.params, omd_of(DECAY, 2), "after the skip")
    assert not torch.equal(net.params, p0)


_CHILD = """
import sys
sys.path.insert(0, {root!r})
import torch
from deep_go_amd.config import ExperimentConfig
from deep_go_amd.models.hip_model import HipGoNet
cfg = ExperimentConfig(numLayers=4, channelSize=128, batchSize=8, seed=5, dtype="bf16")
net = HipGoNet(cfg, 8, device="cuda")
assert "_dgema" not in sys.modules, "ema_decay=0 imported _dgema"
assert net.ema is None and net.ema_rec is None
assert net.can_defer(), "ema_decay=0: the default step no longer defers"
avg = HipGoNet(cfg.replace(ema_decay=0.999), 8, device="cuda")
assert "_dgema" in sys.modules and avg.can_defer()
print("CHILD_OK")
"""


def test_module_is_imported_only_for_the_average():
    """In a fresh process: with ema_decay = 0 _dgema is not imported; with ema_decay > 0 it is,
    and the default 4x128 step defers either way."""
    env = dict(os.environ)
    env.pop("DG_FUSED_UPDATE", None)
    r = subprocess.run([sys.executable, "-c", _CHILD.format(root=ROOT)], env=env,
                       capture_output=True, text=True, timeout=100)
    assert r.returncode == 0 and "CHILD_OK" in r.stdout, r.stderr[-3000:]


# ===================================================================== C: ema_weights()
def _eval(net):
    net.evaluate()
    torch.cuda.synchronize()
    return net.eval_loss.clone(), net.eval_pred.clone()


def _other_vector(net, seed=6):
    from deep_go_amd.models.gocnn import init_params
    v = init_params(net.layout, seed).to(DEV)
    assert v.shape == net.params.shape and not torch.equal(v, net.params)
    return v


@pytest.mark.parametrize("name", ["4x128-bf16", "4x128-fp8"])
def test_ema_weights_on_a_copy_of_the_parameters(name):
    """The average set to the parameters: evaluate() inside the context gives the bits of a
    plain evaluate()."""
    from deep_go_amd.models.hip_model import HipGoNet
    layers, ch, dtype = MODEL_CASES[name]
    net = HipGoNet(_cfg(layers, ch, dtype, "sgd", ema_decay=DECAY), B, device="cuda")
    net.set_batch(*_batch(B, 12))
    net.train_step()
    net.ema.copy_(net.params)
    loss, pred = _eval(net)
    with net.ema_weights():
        loss_e, pred_e = _eval(net)
    assert torch.equal(loss, loss_e) and torch.equal(pred, pred_e)
    assert torch.isfinite(loss).all()


def test_ema_weights_serves_another_vector_bf16():
    """The average set to another seed's parameters: evaluate() and predict_logp() inside the
    context equal a net built with that vector, bit for bit (weights, biases and the head all
    come from the average); outside, the net is itself again."""
    from deep_go_amd.models.hip_model import HipGoNet
    cfg = _cfg(4, 128, "bf16", "sgd", ema_decay=DECAY)
    net = HipGoNet(cfg, B, device="cuda")
    v = _other_vector(net)
    other = HipGoNet(cfg.replace(ema_decay=0.0), B, device="cuda", flat_params=v.clone())
    batch = _batch(B, 12)
    for x in (net, other):
        x.set_batch(*batch)
    net.ema.copy_(v)
    live = _eval(net)
    want = _eval(other)
    want_logp = other.predict_logp().clone()
    with net.ema_weights():
        got = _eval(net)
        got_logp = net.predict_logp().clone()
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    assert torch.equal(got_logp, want_logp)
    assert not torch.equal(got[0], live[0])
    again = _eval(net)
    assert torch.equal(again[0], live[0]) and torch.equal(again[1], live[1])


def test_ema_weights_serves_another_vector_fp8():
    """The same on fp8: the average is quantised with the live weight scales, so the outputs
    differ from the live ones and the mean loss lies within 3% of the bf16 net on that vector
    (test_fp8_forward_model_tracks_bf16's tolerance)."""
    from deep_go_amd.models.hip_model import HipGoNet
    cfg = _cfg(4, 128, "fp8", "sgd", ema_decay=DECAY)
    net = HipGoNet(cfg, B, device="cuda")
    v = _other_vector(net)
    other = HipGoNet(cfg.replace(ema_decay=0.0, dtype="bf16"), B, device="cuda",
                     flat_params=v.clone())
    batch = _batch(B, 12)
    with pytest.raises(RuntimeError):          # (the fp8 scales are not calibrated yet)
        with net.ema_weights():
            pass
    for x in (net, other):
        x.set_batch(*batch)
    net.ema.copy_(v)
    live = _eval(net)
    want = _eval(other)
    scales = net.fp8_scales.clone()
    with net.ema_weights():
        got = _eval(net)
    assert not torch.equal(got[0], live[0])
    lb, l8 = want[0].mean().item(), got[0].mean().item()
    print(f"EMA_FP8 mean loss bf16={lb:.5f} fp8 average={l8:.5f} live={live[0].mean().item():.5f}")
    assert abs(lb - l8) < 0.03 * abs(lb), (lb, l8)
    assert torch.equal(net.fp8_scales, scales)


_FP8_STATE = ("fp8_scales", "fp8_amax", "fp8_amax_w", "fp8_sat", "fp8_gscales", "fp8_gamax",
              "fp8_ghist")


@pytest.mark.parametrize("name", ["4x128-bf16", "4x128-fp8"])
def test_entering_and_leaving_leaves_the_net_as_it_was(name):
    """A net that enters the context between steps, evaluates inside and leaves, against a net
    that never did: every later step gives equal parameters, optimizer state, losses, averages
    and fp8 scale tensors.  Inside, nesting, forward_backward, optimizer_step and train_step
    raise RuntimeError."""
    from deep_go_amd.models.hip_model import HipGoNet
    layers, ch, dtype = MODEL_CASES[name]
    cfg = _cfg(layers, ch, dtype, "adamw", ema_decay=DECAY)
    x, y = (HipGoNet(cfg, B, device="cuda") for _ in range(2))
    for t in range(4):
        batch = _batch(B, 12 + t)
        for net in (x, y):
            net.set_batch(*batch)
            net.train_step()
        torch.cuda.synchronize()
        _same_training_state(x, y, (name, t))
        assert torch.equal(x.ema, y.ema) and torch.equal(x.ema_rec, y.ema_rec)
        for k in _FP8_STATE:
            assert torch.equal(getattr(x, k), getattr(y, k)), (name, t, k)
        if t in (0, 1):
            with x.ema_weights():
                loss, _ = _eval(x)
                assert torch.isfinite(loss).all()
                with pytest.raises(RuntimeError):
                    with x.ema_weights():
                        pass
                for fn in (x.forward_backward, x.optimizer_step, x.train_step):
                    with pytest.raises(RuntimeError):
                        fn()
            torch.cuda.synchronize()
            for k in _FP8_STATE:
                assert torch.equal(getattr(x, k), getattr(y, k)), (name, t, k, "after leaving")
    assert x.ema_steps() == 4
    with pytest.raises(RuntimeError):
        HipGoNet(cfg.replace(ema_decay=0.0), B, device="cuda").ema_weights().__enter__()


# ===================================================================== D: HIPBackend
def test_hip_backend_resume_is_exact(tmp_path):
    """4 steps == 2 steps + state_dict -> a new backend + load_state_dict + 2 steps, bit for
    bit on the parameters, both moments, the average and its count; a state without an average
    seeds from the parameters with t = 0; load_params reseeds."""
    from deep_go_amd.data.synthetic import random_planes
    from deep_go_amd.train.backends import HIPBackend
    cfg = _cfg(3, 64, "bf16", "adamw", batchSize=4, checkpoint_dir=str(tmp_path),
               ema_decay=DECAY)
    batches = [random_planes(4, seed=20 + i) for i in range(4)]

    def run(be, which):
        for i in which:
            be.set_batch(*batches[i])
            be.train_step()
        torch.cuda.synchronize()

    a = HIPBackend(cfg, 4)
    p_init = a.flat_params().clone()
    run(a, range(4))
    assert a.ema_steps() == 4
    b = HIPBackend(cfg, 4, flat=p_init)
    run(b, range(2))
    sd = b.state_dict()
    assert sd["optimizer"]["ema_t"] == 2 and isinstance(sd["optimizer"]["ema_t"], int)
    assert torch.equal(sd["optimizer"]["ema"], b.ema_params())
    assert not sd["optimizer"]["ema"].is_cuda
    cb = HIPBackend(cfg, 4, flat=b.flat_params())
    assert cb.ema_steps() == 0 and torch.equal(cb.ema_params(), b.flat_params())
    cb.load_state_dict(sd)
    assert cb.ema_steps() == 2
    run(cb, range(2, 4))
    assert torch.equal(cb.net.params, a.net.params)
    assert torch.equal(cb.net.adam_m, a.net.adam_m) and torch.equal(cb.net.adam_v, a.net.adam_v)
    assert same_bits(cb.net.ema, a.net.ema) and cb.ema_steps() == 4 and cb.rate == a.rate
    # a state without an average; load_params
    del sd["optimizer"]["ema"], sd["optimizer"]["ema_t"]
    cb.load_state_dict(sd)
    assert cb.ema_steps() == 0 and same_bits(cb.net.ema, cb.net.params)
    run(cb, [0])
    cb.load_params(p_init)
    assert cb.ema_steps() == 0 and torch.equal(cb.ema_params(), p_init)
    # evaluate() inside the backend's context reads the average
    cb.set_batch(*batches[0])
    run(cb, [1, 2])
    cb.evaluate()
    live = cb.loss_sum()
    with cb.ema_weights():
        cb.evaluate()
        avg = cb.loss_sum()
        with pytest.raises(RuntimeError):
            cb.train_step()
    cb.evaluate()
    assert cb.loss_sum() == live and avg != live and np.isfinite(avg)
    for be in (a, b, cb):
        be.close()


def test_gpu_average_matches_cpu_average(tmp_path):
    """test_momentum_gpu.test_gpu_step_matches_cpu_step's set-up and tolerance with
    optimizer=sgd and one step: the average's move away from the initial parameters on the two
    backends differs by < 0.05 relative, as the update itself."""
    from deep_go_amd.config import ExperimentConfig
    from deep_go_amd.data.synthetic import random_planes
    from deep_go_amd.train.backends import CPUBackend, HIPBackend
    cfg = ExperimentConfig(numLayers=4, channelSize=64, batchSize=32, validationSize=64,
                           validation_interval=10, log_interval=5, useCuda=True, synthetic=True,
                           checkpoint_dir=str(tmp_path), seed=2, loader_threads=4, prefetch=3,
                           rate=0.05, head_relu=False, optimizer="sgd", ema_decay=0.999)
    cpu_be = CPUBackend(cfg, 16)
    gpu_be = HIPBackend(cfg, 16, flat=cpu_be.flat_params().clone())
    batch = random_planes(16, seed=4)
    for be in (cpu_be, gpu_be):
        be.set_batch(*batch)
        be.forward_backward()
        be.optimizer_step()
    p0 = CPUBackend(cfg, 16).flat_params()
    da, db = cpu_be.flat_params() - p0, gpu_be.flat_params() - p0
    ea, eb = cpu_be.ema_params() - p0, gpu_be.ema_params() - p0
    rel, rele = ((da - db).norm() / da.norm()).item(), ((ea - eb).norm() / ea.norm()).item()
    print(f"EMA_CPU_GPU relative update difference {rel:.4f}, of the average's move {rele:.4f}")
    assert cpu_be.ema_steps() == gpu_be.ema_steps() == 1
    assert ea.norm() > 0 and rel < 0.05 and rele < 0.05, (rel, rele)
    # the GPU's average against the oracle fed the GPU's own parameters
    _check_step(gpu_be.ema_params(), p0, gpu_be.flat_params(), omd_of(0.999, 1), "backend")
    gpu_be.close()
