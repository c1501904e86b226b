"""grad_clip on the GPU: the two kernels of csrc/kernels/clip.hip (module _dgclip) against the
float64 oracle and the counted bound of tests/test_clip_cpu.py, bit-exactly on designed data,
inside HipGoNet (eager and as step graphs, bf16 and fp8, every optimizer, with the bf16 wire
twin, without a gate pointer), the skip policy, the import check, exact resume and the fp32 CPU
trainer.

Buffers under test — the gradient, the bf16 variant's output, the partials and the 16-byte
record {float norm; float scale; int64 clipped} — sit between sentinel runs
(test_update_gpu.guarded); the outputs are pre-filled.
"""
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from test_clip_cpu import (PARTIALS, SIZES, clip_checks, clip_ref, designed_case, expected_scale,
                           kernel_shape, norm_bound)
from test_update_gpu import DEV, guarded, guards_intact, same_bits

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILL = 7.0                 # what the bf16 variant's output buffer holds before a launch
REC0 = 5                   # the record's count before a launch


def _clip():
    from deep_go_amd.ops.native import clip
    return clip()


def _f32(x) -> float:
    return float(np.float32(x))


class _Bufs:
    """The device buffers of one kernel-level case, each between sentinels."""

    def __init__(self, g: torch.Tensor, kind: str):
        self.kind, self.n = kind, g.numel()
        self.g_in = g.to(torch.bfloat16) if kind == "bf16" else g.float()
        self.gbuf, self.g = guarded(self.g_in)
        self.obuf, self.out = guarded(torch.full((self.n,), FILL))
        self.pbuf, self.part = guarded(torch.full((PARTIALS,), -1.0))
        self.rbuf, self.rec = guarded(torch.tensor([0, REC0], dtype=torch.int64))

    def launch(self, c, gscale, gate=None):
        from deep_go_amd.ops.native import stream_handle
        m = _clip()
        gt = gate.data_ptr() if gate is not None else 0
        if self.kind == "bf16":
            m.grad_clip_bf16(self.g.data_ptr(), self.out.data_ptr(), self.n,
                             self.part.data_ptr(), PARTIALS, self.rec.data_ptr(), c, gscale, gt,
                             stream_handle())
        else:
            m.grad_clip(self.g.data_ptr(), self.n, self.part.data_ptr(), PARTIALS,
                        self.rec.data_ptr(), c, gscale, gt, stream_handle())
        torch.cuda.synchronize()
        assert all(guards_intact(b) for b in (self.gbuf, self.obuf, self.pbuf, self.rbuf))

    def reset(self):
        self.g.copy_(self.g_in)
        self.out.fill_(FILL)
        self.rec.copy_(torch.tensor([0, REC0], dtype=torch.int64))

    def record(self):
        """(norm, scale, clipped)"""
        norm, scale = self.rec[0:1].view(torch.float32).tolist()
        return norm, scale, int(self.rec[1].item())

    def result(self) -> torch.Tensor:
        """the scaled fp32 gradient, on the CPU"""
        return (self.out if self.kind == "bf16" else self.g).cpu()

    def source(self) -> torch.Tensor:
        """the input as fp32 values, on the CPU"""
        return self.g_in.float()


# ===================================================================== A: the kernels
GSCALES = [1.0, 0.37]


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("kind", ["fp32", "bf16"])
def test_clip_matches_float64_reference(kind, n):
    """Gaussian data, c = half the norm (clipping) and twice the norm (not clipping), for both
    gscales: the norm within norm_bound of clip_ref; the scale the one that follows from the
    kernel's own fp32 norm, exactly; the output teacher-forced: the input times that scale, one
    fp32 multiply, bit for bit (bf16: the widened twin times the scale, the twin unchanged).
    Unclipped: scale == 1.0 exactly, the fp32 gradient keeps its bits and the count stays; the
    bf16 variant writes the widened twin.  A closed gate keeps the gradient, the output, the
    partials and the record; two launches on the same input give the same bits.

    Measured on an MI355X: the norm's largest error is 0.050 of norm_bound (bf16, n = 1024),
    0.026 with fp32 inputs; at the two sizes with several passes 0.016 and 0.013."""
    gen = torch.Generator().manual_seed(700 + n % 1000)
    b = _Bufs(torch.randn(n, generator=gen) * 0.7, kind)
    src = b.source()
    worst = 0.0
    for gscale in GSCALES:
        ref_norm = clip_ref(src, gscale, 1.0)[0]
        assert ref_norm > 0
        # ---- clipping
        c = 0.5 * ref_norm
        b.reset()
        b.launch(c, gscale)
        norm, scale, clipped = b.record()
        ok, ratio = clip_checks(src, gscale, c, norm, scale, b.result())
        print(f"CLIP_ERR kind={kind} n={n} gscale={gscale} norm_err_over_bound={ratio:.3f}")
        worst = max(worst, ratio)
        assert all(ok.values()), (gscale, ok, ratio, norm, ref_norm, scale)
        assert scale < 1.0 and clipped == REC0 + 1
        assert 0.4 < scale < 0.51
        if kind == "bf16":
            assert same_bits(b.g, b.g_in)
        first = (b.rec.clone(), b.result().clone(), b.part.clone())
        # ---- again on the same input: the same bits
        b.reset()
        b.launch(c, gscale)
        assert same_bits(b.rec, first[0]) and same_bits(b.result(), first[1])
        assert same_bits(b.part, first[2])
        # ---- not clipping
        b.reset()
        b.launch(2.0 * ref_norm, gscale)
        norm2, scale2, clipped2 = b.record()
        assert _f32(norm2) == _f32(norm) and scale2 == 1.0 and clipped2 == REC0
        assert same_bits(b.g, b.g_in)
        if kind == "bf16":
            assert same_bits(b.out, src)
        else:
            assert bool((b.out == FILL).all())
        # ---- a closed gate, over what the last launch left
        before = [t.clone() for t in (b.g, b.out, b.part, b.rec)]
        b.launch(c, gscale, gate=torch.zeros(1, device=DEV))
        for t, t0 in zip((b.g, b.out, b.part, b.rec), before):
            assert same_bits(t, t0)
        # ---- an open gate behaves as none
        b.reset()
        b.launch(c, gscale, gate=torch.ones(1, device=DEV))
        assert same_bits(b.rec, first[0]) and same_bits(b.result(), first[1])
    print(f"CLIP_ERR kind={kind} n={n} worst norm_err_over_bound={worst:.3f} "
          f"bound={norm_bound(n, kernel_shape(n)[1]):.3e}")


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("kind", ["fp32", "bf16"])
def test_designed_data_pins_the_norm(kind, n):
    """Integers in -2..2 times 2^-7 (exact in bf16 too): every fp32 partial is exact in any
    order, so the record's norm is float32(|gscale| sqrt(S)) with S exact — which pins the
    double-precision sum of the partials, the root and the one rounding — and grad_norm's
    partials add up to S exactly."""
    from deep_go_amd.ops.native import stream_handle
    g, S = designed_case(n, 40 + n % 1000)
    if S == 0:
        g[0], S = 2.0 ** -6, 2.0 ** -12
    b = _Bufs(g, kind)
    assert torch.equal(b.source(), g)
    for gscale in (1.0, -0.75):
        b.reset()
        b.launch(1e30, gscale)
        norm, scale, clipped = b.record()
        assert norm == _f32(abs(gscale) * math.sqrt(S)), (gscale, norm, S)
        assert scale == 1.0 and clipped == REC0
    b.part.fill_(-1.0)
    fn = _clip().grad_norm_bf16 if kind == "bf16" else _clip().grad_norm
    fn(b.g.data_ptr(), n, b.part.data_ptr(), PARTIALS, 0, stream_handle())
    torch.cuda.synchronize()
    grid = kernel_shape(n)[0]
    part = b.part.cpu().double()
    assert part[:grid].sum().item() == S and bool((part[grid:] == -1.0).all())
    assert guards_intact(b.pbuf) and guards_intact(b.gbuf)


@pytest.mark.parametrize("n", [7, 1027, 4099, 2 ** 20 + 1029, 3 * 2 ** 20 + 7])
@pytest.mark.parametrize("kind", ["fp32", "bf16"])
def test_every_region_counts(kind, n):
    """One element replaced by 64 — element 0, element n - 1 (inside the tail when n % 4 != 0),
    one element of the second pass, one of the last workgroup's chunk: norm^2 moves by
    gscale^2 (64^2 - old^2) within the bound (relative on each norm, so twice that on its
    square)."""
    gen = torch.Generator().manual_seed(900 + n % 1000)
    g = torch.randn(n, generator=gen) * 0.7
    if kind == "bf16":
        g = g.to(torch.bfloat16).float()
    grid, passes = kernel_shape(n)
    places = {"first": 0, "last": n - 1, "last workgroup": min((grid - 1) * 1024, n - 1)}
    if passes > 1:
        places["second pass"] = 2 ** 20 + 5
    gscale = 0.37
    s2 = _f32(gscale) ** 2
    bd = norm_bound(n, passes)
    b = _Bufs(g, kind)
    b.launch(1e30, gscale)
    base = b.record()[0]
    for what, i in places.items():
        g2 = g.clone()
        g2[i] = 64.0
        b2 = _Bufs(g2, kind)
        b2.launch(1e30, gscale)
        moved = b2.record()[0]
        want = s2 * (64.0 ** 2 - float(g[i]) ** 2)
        tol = 2 * bd * (moved ** 2 + base ** 2)
        assert abs((moved ** 2 - base ** 2) - want) <= tol, (what, i, moved, base, want, tol)
        assert want > 100 * tol       # (the test can tell)


@pytest.mark.parametrize("kind", ["fp32", "bf16"])
def test_overflow_gives_an_infinite_norm_and_a_zero_scale(kind):
    """One element at 1e25: its fp32 square overflows, norm = inf, scale = 0, the output is
    all zero and the step counts as clipped, as torch does."""
    n = 4099
    g = torch.randn(n, generator=torch.Generator().manual_seed(1)) * 0.7
    g[n // 2] = 1e25
    b = _Bufs(g, kind)
    b.launch(1.0, 1.0)
    norm, scale, clipped = b.record()
    assert norm == math.inf and scale == 0.0 and clipped == REC0 + 1
    assert not b.result().any()
    assert expected_scale(norm, 1.0) == 0.0


# ===================================================================== B: in the model
MODEL_CASES = {"3x64-bf16": (3, 64, "bf16"), "4x128-bf16": (4, 128, "bf16"),
               "4x128-fp8": (4, 128, "fp8")}       # (tests/test_momentum_gpu.py's)
B = 8
RATE_DECAY = 1e-3
OPTIMIZERS = ["sgd", "rmsprop", "momentum", "adamw"]
_OPT_KW = {"sgd": dict(rate=0.01), "rmsprop": dict(rate=1e-3),
           "momentum": dict(rate=0.01, momentum=0.9, nesterov=True, weight_decay=1e-3),
           "adamw": dict(rate=1e-5, weight_decay=1e-2)}
# (small rates and no ReLU on the head: the gradient norm of the later steps stays near the
# first step's, so half of that keeps clipping; a small net with the head's ReLU can die under
# adamw at 1e-3 within a few steps, and its gradient is then exactly zero)


def _cfg(layers, ch, dtype, opt, **kw):
    from deep_go_amd.config import ExperimentConfig
    base = dict(numLayers=layers, channelSize=ch, batchSize=B, seed=5, dtype=dtype,
                rateDecay=RATE_DECAY, optimizer=opt, head_relu=False, **_OPT_KW[opt])
    base.update(kw)
    return ExperimentConfig(**base)


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


_NORMS = {}


def _first_norm(name, wire=False) -> float:
    """The first step's gradient norm of a model case (batch seed 12), measured once on a net
    without clipping: what the clipping tests take half of."""
    from deep_go_amd.models.hip_model import HipGoNet
    if (name, wire) not in _NORMS:
        layers, ch, dtype = MODEL_CASES[name]
        kw = dict(global_batch=2 * B, grad_wire="bf16") if wire else {}
        net = HipGoNet(_cfg(layers, ch, dtype, "sgd"), B, device="cuda", **kw)
        net.set_batch(*_batch(B, 12))
        net.forward_backward()
        torch.cuda.synchronize()
        g = net.grads16 if wire else net.grads
        _NORMS[(name, wire)] = g.double().norm().item()
        assert _NORMS[(name, wire)] > 0
    return _NORMS[(name, wire)]


def _no_fused_knobs():
    import dataclasses
    from deep_go_amd.models.hip_model import Knobs
    return dataclasses.replace(Knobs.from_env(), FUSED_UPDATE=False)


@pytest.mark.parametrize("opt", OPTIMIZERS)
@pytest.mark.parametrize("name", list(MODEL_CASES))
def test_never_clipping_changes_nothing(name, opt):
    """grad_clip = 1e30 over three steps against a grad_clip = 0 net (sgd | rmsprop: with the
    separate launches of DG_FUSED_UPDATE=0, which clipping makes them take): parameters,
    optimizer state, losses and predictions are equal after every step; the clipping net never
    defers; its record holds a norm, scale 1 and no clipped step."""
    from deep_go_amd.models.hip_model import HipGoNet
    layers, ch, dtype = MODEL_CASES[name]
    a = HipGoNet(_cfg(layers, ch, dtype, opt, grad_clip=1e30), B, device="cuda")
    kn = _no_fused_knobs() if opt in ("sgd", "rmsprop") else None
    b = HipGoNet(_cfg(layers, ch, dtype, opt), B, device="cuda", knobs=kn)
    assert not a.can_defer() and not b.can_defer()
    assert a.clip_part is not None and a.clip_rec is not None and not a.clip_rec.any()
    assert b.clip_part is None and b.clip_rec is None
    for t in range(3):
        batch = _batch(B, 12 + t)
        for net in (a, b):
            net.set_batch(*batch)
            net.train_step()
        torch.cuda.synchronize()
        assert torch.equal(a.params, b.params), t
        assert torch.equal(a.loss, b.loss) and torch.equal(a.pred, b.pred), t
        assert torch.equal(a.grads, b.grads), t
        sa, sb = _opt_state(a), _opt_state(b)
        assert set(sa) == set(sb) and all(torch.equal(sa[k], sb[k]) for k in sa), t
        assert a.lr.item() == b.lr.item()
        norm, scale, clipped = a.clip_stats()
        assert norm > 0 and scale == 1.0 and clipped == 0
    assert int(a.step_count.item()) == 3 and int(a.bad_steps.item()) == 0


def _check_update(net, opt, p0, st0, lr0, g, tag):
    """The parameters (and state) after one step against the optimizer's existing float64
    reference fed the gradient g, within that optimizer's existing bounds."""
    from test_adamw_cpu import check_adamw_step
    from test_momentum_cpu import ranges_mask
    from test_momentum_gpu import check_step
    from test_update_gpu import rmsprop_check, sgd_bound
    from test_update_oracles_cpu import sgd_ref
    cfg = net.cfg
    if opt == "sgd":
        ref = sgd_ref(p0, g, lr0, 1.0)
        err = (net.params.double() - ref).abs()
        bound = sgd_bound(ref, g, lr0, 1.0)
        assert (err <= bound).all(), (tag, (err / bound.clamp_min(1e-300)).max().item())
    elif opt == "rmsprop":
        rmsprop_check(p0, st0["ms"], net.params, net.ms, g, lr0, cfg.rmsprop_decay, 1.0)
    else:
        mask = ranges_mask(net.layout.numel, net.layout.weight_ranges()).to(DEV)
        if opt == "momentum":
            check_step(p0, g, st0["vel"], net.params, net.vel, lr0, cfg.momentum, cfg.nesterov,
                       cfg.weight_decay, mask, 1.0, tag)
        else:
            t = net.adam_steps()
            check_adamw_step(p0, g, st0["adam_m"], st0["adam_v"], net.params, net.adam_m,
                             net.adam_v, t, lr0, (cfg.adam_beta1, cfg.adam_beta2), cfg.adam_eps,
                             cfg.weight_decay, mask, 1.0, tag)
    assert not torch.equal(net.params, p0)


def _check_clipped(net, g0, c, count, tag):
    """After a clipped optimizer_step from the gradient clone g0 (fp32 values): the record
    against clip_ref within norm_bound, the scale the one of the kernel's own norm, the count;
    net.grads == g0 * scale bit for bit.  -> (norm, scale, error over bound)."""
    n = g0.numel()
    norm, scale, clipped = net.clip_stats()
    ref_norm = clip_ref(g0.cpu(), 1.0, c)[0]
    ratio = abs(norm - ref_norm) / (norm_bound(n, kernel_shape(n)[1]) * ref_norm)
    assert ratio <= 1.0, (tag, norm, ref_norm, ratio)
    assert scale == expected_scale(norm, c) and scale < 1.0 and clipped == count, (tag, scale)
    assert torch.equal(net.grads, g0 * torch.tensor(scale, dtype=torch.float32, device=DEV)), tag
    return norm, scale, ratio


@pytest.mark.parametrize("opt", OPTIMIZERS)
@pytest.mark.parametrize("name", list(MODEL_CASES))
def test_clipped_steps_match_references(name, opt):
    """c = half the first step's measured norm; two eager steps.  After forward_backward the
    gradient is cloned; after optimizer_step clip_stats() matches clip_ref of the clone within
    norm_bound, net.grads is the clone times the kernel's scale bit for bit, and the parameters
    (and the optimizer's state) match the optimizer's own float64 reference fed that scaled
    gradient within its existing bounds."""
    from deep_go_amd.models.hip_model import HipGoNet
    layers, ch, dtype = MODEL_CASES[name]
    c = 0.5 * _first_norm(name)
    net = HipGoNet(_cfg(layers, ch, dtype, opt, grad_clip=c), B, device="cuda")
    assert not net.can_defer()
    net.set_batch(*_batch(B, 12))
    for t in (1, 2):
        net.forward_backward()
        torch.cuda.synchronize()
        g0, p0, lr0 = net.grads.clone(), net.params.clone(), net.lr.item()
        st0 = {k: v.clone() for k, v in _opt_state(net).items()}
        net.optimizer_step()
        torch.cuda.synchronize()
        norm, scale, ratio = _check_clipped(net, g0, c, t, (name, opt, t))
        print(f"CLIP_ERR model name={name} opt={opt} t={t} norm={norm:.5f} scale={scale:.4f} "
              f"norm_err_over_bound={ratio:.3f}")
        if t == 1:
            assert abs(scale - 0.5) < 0.05
        _check_update(net, opt, p0, st0, lr0, net.grads, (name, opt, t))
        assert int(net.step_count.item()) == t and int(net.bad_steps.item()) == 0
        assert net.lr.item() == pytest.approx(net.cfg.rate * (1.0 - RATE_DECAY) ** t, rel=1e-13)


@pytest.mark.parametrize("opt", ["sgd", "adamw"])
@pytest.mark.parametrize("name", list(MODEL_CASES))
def test_step_graph_gives_the_eager_bits(name, opt):
    """SegmentedStep(use_graphs=True) against the eager step from the same state over three
    steps: parameters, optimizer state, gradient and the clip record, bit for bit; the capture
    itself counts nothing."""
    from deep_go_amd.models.hip_model import HipGoNet, SegmentedStep
    layers, ch, dtype = MODEL_CASES[name]
    c = 0.5 * _first_norm(name)
    cfg = _cfg(layers, ch, dtype, opt, grad_clip=c)
    nets = [HipGoNet(cfg, B, device="cuda") for _ in range(2)]
    steps = []
    for net, graphs in zip(nets, (False, True)):
        net.set_batch(*_batch(B, 12))
        steps.append(SegmentedStep(net, None, use_graphs=graphs))
        assert not net.clip_rec.any()
    assert steps[1].full_graph is not None and steps[0].full_graph is None
    e, g = nets
    for t in range(1, 4):
        for step in steps:
            step()
        torch.cuda.synchronize()
        assert same_bits(e.params, g.params) and same_bits(e.grads, g.grads), t
        assert same_bits(e.clip_rec, g.clip_rec), t
        se, sg = _opt_state(e), _opt_state(g)
        assert all(same_bits(se[k], sg[k]) for k in se), t
        assert e.clip_stats()[2] == t and e.clip_stats()[1] < 1.0
    # forward/backward and the optimizer as graphs of their own
    for net, step in zip(nets, steps):
        step.forward_backward()
        step.optimizer()
    torch.cuda.synchronize()
    assert same_bits(e.params, g.params) and same_bits(e.clip_rec, g.clip_rec)
    assert g.clip_stats()[2] == 4


def test_bf16_wire_scales_into_the_fp32_gradient():
    """grad_wire=bf16: the twin keeps its bits, net.grads == twin.float() * scale (one bf16
    rounding, the wire's), and the update is read from net.grads (momentum's reference fed
    net.grads holds; fed the unscaled twin it misses by far)."""
    from deep_go_amd.models.hip_model import HipGoNet
    from test_momentum_gpu import check_step
    name = "4x128-bf16"
    c = 0.5 * _first_norm(name, wire=True)
    net = HipGoNet(_cfg(4, 128, "bf16", "momentum", grad_clip=c), B, device="cuda",
                   global_batch=2 * B, grad_wire="bf16")
    assert net.grads16 is not None and not net.can_defer()
    net.set_batch(*_batch(B, 12))
    net.forward_backward()
    torch.cuda.synchronize()
    twin0, p0, lr0 = net.grads16.clone(), net.params.clone(), net.lr.item()
    st0 = {k: v.clone() for k, v in _opt_state(net).items()}
    net.optimizer_step()
    torch.cuda.synchronize()
    assert same_bits(net.grads16, twin0)
    norm, scale, ratio = _check_clipped(net, twin0.float(), c, 1, "wire")
    print(f"CLIP_ERR model wire norm={norm:.5f} scale={scale:.4f} norm_err_over_bound={ratio:.3f}")
    _check_update(net, "momentum", p0, st0, lr0, net.grads, "wire")
    with pytest.raises(AssertionError):
        _check_update(net, "momentum", p0, st0, lr0, twin0.float(), "wire, unscaled")
    assert int(net.bad_steps.item()) == 0 and int(net.step_count.item()) == 1


def test_clipped_step_without_a_gate():
    """nan_policy=raise: no gate launch and no gate pointer; the same clip and update."""
    from deep_go_amd.models.hip_model import HipGoNet
    c = 0.5 * _first_norm("3x64-bf16")
    net = HipGoNet(_cfg(3, 64, "bf16", "adamw", grad_clip=c, nan_policy="raise"), B,
                   device="cuda")
    net.set_batch(*_batch(B, 12))
    net.gate.zero_()                    # (nothing may read it)
    for t in (1, 2):
        net.forward_backward()
        torch.cuda.synchronize()
        g0, p0, lr0 = net.grads.clone(), net.params.clone(), net.lr.item()
        st0 = {k: v.clone() for k, v in _opt_state(net).items()}
        net.optimizer_step()
        torch.cuda.synchronize()
        _check_clipped(net, g0, c, t, ("raise", t))
        _check_update(net, "adamw", p0, st0, lr0, net.grads, ("raise", t))
        assert int(net.step_count.item()) == t and net.gate.item() == 0.0


def test_skipped_step_clips_nothing():
    """nan_policy=skip: a clean clipped step, then a poisoned gradient entry, then a poisoned
    loss: the parameters, the optimizer's state, net.grads and the clip record keep their bits;
    the next clean step clips again."""
    from deep_go_amd.models.hip_model import HipGoNet
    c = 0.5 * _first_norm("4x128-bf16")
    net = HipGoNet(_cfg(4, 128, "bf16", "adamw", grad_clip=c, nan_policy="skip"), B,
                   device="cuda")
    net.set_batch(*_batch(B, 12))
    net.forward_backward()
    net.optimizer_step()
    torch.cuda.synchronize()
    assert net.clip_stats()[2] == 1 and net.bad_steps.item() == 0
    p0, rec0 = net.params.clone(), net.clip_rec.clone()
    part0 = net.clip_part.clone()
    st0 = {k: v.clone() for k, v in _opt_state(net).items()}

    def unchanged():
        st = _opt_state(net)
        return (same_bits(net.params, p0) and same_bits(net.clip_rec, rec0)
                and same_bits(net.clip_part, part0)
                and all(same_bits(st[k], st0[k]) for k in st0))
    net.forward_backward()
    net.grads[17] = float("nan")
    torch.cuda.synchronize()
    g0 = net.grads.clone()
    net.optimizer_step()
    torch.cuda.synchronize()
    assert unchanged() and same_bits(net.grads, g0)
    assert net.bad_steps.item() == 1 and net.gate.item() == 0.0
    net.forward_backward()
    net.loss[0] = float("inf")
    torch.cuda.synchronize()
    g0 = net.grads.clone()
    net.optimizer_step()
    torch.cuda.synchronize()
    assert unchanged() and same_bits(net.grads, g0)
    assert net.bad_steps.item() == 2 and int(net.step_count.item()) == 3
    net.forward_backward()
    torch.cuda.synchronize()
    g0 = net.grads.clone()
    net.optimizer_step()
    torch.cuda.synchronize()
    assert net.gate.item() == 1.0 and net.bad_steps.item() == 2
    _check_clipped(net, g0, c, 2, "after the skips")
    assert not torch.equal(net.params, p0) and net.adam_steps() == 2


_CHILD = """
import sys
sys.path.insert(0, {root!r})
import torch
from deep_go_amd.config import ExperimentConfig
from deep_go_amd.models.hip_model import HipGoNet
cfg = ExperimentConfig(numLayers=4, channelSize=128, batchSize=8, seed=5, dtype="bf16")
net = HipGoNet(cfg, 8, device="cuda")
assert "_dgclip" not in sys.modules, "grad_clip=0 imported _dgclip"
assert net.clip_part is None and net.clip_rec is None
assert net.can_defer(), "grad_clip=0: the default step no longer defers"
clipped = HipGoNet(cfg.replace(grad_clip=1.0), 8, device="cuda")
assert "_dgclip" in sys.modules and not clipped.can_defer()
print("CHILD_OK")
"""


def test_module_is_imported_only_for_clipping():
    """In a fresh process: with grad_clip = 0 _dgclip is not imported and the default 4x128
    step defers as before; with grad_clip > 0 it is imported and the step does not defer."""
    env = dict(os.environ)
    env.pop("DG_FUSED_UPDATE", None)
    r = subprocess.run([sys.executable, "-c", _CHILD.format(root=ROOT)], env=env,
                       capture_output=True, text=True, timeout=100)
    assert r.returncode == 0 and "CHILD_OK" in r.stdout, r.stderr[-3000:]


# ===================================================================== C: HIPBackend
def test_hip_backend_resume_is_exact(tmp_path):
    """4 steps == 2 steps + state_dict -> a new backend + load_state_dict + 2 steps with
    grad_clip > 0, bit for bit on the parameters and both moments; clipped_steps is a statistic
    of the run and restarts at 0."""
    from deep_go_amd.data.synthetic import random_planes
    from deep_go_amd.train.backends import HIPBackend
    c = 0.25 * _first_norm("3x64-bf16")
    cfg = _cfg(3, 64, "bf16", "adamw", batchSize=4, checkpoint_dir=str(tmp_path), grad_clip=c)
    batches = [random_planes(4, seed=20 + i) for i in range(4)]

    def run(be, which):
        for i in which:
            be.set_batch(*batches[i])
            be.train_step()
        torch.cuda.synchronize()

    a = HIPBackend(cfg, 4)
    p_init = a.flat_params().clone()
    run(a, range(4))
    assert a.clip_stats()[2] == 4
    b = HIPBackend(cfg, 4, flat=p_init)
    run(b, range(2))
    sd = b.state_dict()
    assert not any("clip" in k for k in sd["optimizer"])
    cb = HIPBackend(cfg, 4, flat=b.flat_params())
    cb.load_state_dict(sd)
    run(cb, range(2, 4))
    assert torch.equal(cb.net.params, a.net.params)
    assert torch.equal(cb.net.adam_m, a.net.adam_m) and torch.equal(cb.net.adam_v, a.net.adam_v)
    assert cb.rate == a.rate and cb.clip_stats()[2] == 2
    assert cb.clip_stats()[:2] == a.clip_stats()[:2]
    for be in (a, b, cb):
        be.close()


def test_gpu_step_matches_cpu_step(tmp_path):
    """test_momentum_gpu.test_gpu_step_matches_cpu_step's set-up and tolerance with
    optimizer=sgd and one clipped step: grad_norm on the two backends differs by < 0.05
    relative, and so does the parameter update; both count one clipped step.  The figures are
    printed (profiles/clip.txt quotes them)."""
    from deep_go_amd.config import ExperimentConfig
    from deep_go_amd.data.synthetic import random_planes
    from deep_go_amd.train.backends import CPUBackend, HIPBackend
    cfg = ExperimentConfig(numLayers=4, channelSize=64, batchSize=32, validationSize=64,
                           validation_interval=10, log_interval=5, useCuda=True, synthetic=True,
                           checkpoint_dir=str(tmp_path), seed=2, loader_threads=4, prefetch=3,
                           rate=0.05, head_relu=False, optimizer="sgd", grad_clip=0.01)
    cpu_be = CPUBackend(cfg, 16)
    gpu_be = HIPBackend(cfg, 16, flat=cpu_be.flat_params().clone())
    batch = random_planes(16, seed=4)
    for be in (cpu_be, gpu_be):
        be.set_batch(*batch)
        be.forward_backward()
        be.optimizer_step()
    p0 = CPUBackend(cfg, 16).flat_params()
    da, db = cpu_be.flat_params() - p0, gpu_be.flat_params() - p0
    rel = ((da - db).norm() / da.norm()).item()
    nc, sc, kc = cpu_be.clip_stats()
    ng, sg, kg = gpu_be.clip_stats()
    reln = abs(nc - ng) / nc
    print(f"CLIP_CPU_GPU grad_norm cpu={nc:.6f} gpu={ng:.6f} relative difference {reln:.5f}; "
          f"relative update difference {rel:.4f}")
    assert kc == kg == 1 and sc < 1.0 and sg < 1.0
    assert reln < 0.05, reln
    assert rel < 0.05, rel
    assert gpu_be.rate == pytest.approx(cpu_be.rate, rel=1e-12)
    gpu_be.close()
