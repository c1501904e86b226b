"""optimizer=momentum without a GPU: the config, the float64 oracle ``momentum_ref`` (checked
against ``torch.optim.SGD``), the CPU optimizer, the weight-decay ranges, exact resume on the
CPU backend and the argument checks of the ``_dgopt`` launcher.

The definition (train/optim.py Momentum), per flat element, with v = 0 at the start:

    gi = g * gscale;  gw = gi + wd * p on the conv weights, else gi
    v  = mu * v + gw
    p -= lr * (gw + mu * v if nesterov else v)

tests/test_momentum_gpu.py imports ``momentum_ref`` and the exact-data generator from here.
"""
import numpy as np
import pytest
import torch

from deep_go_amd.config import ExperimentConfig, get_preset
from deep_go_amd.models.gocnn import ParamLayout, init_params
from deep_go_amd.train.optim import Momentum


# ------------------------------------------------------------------------------ oracle
def momentum_ref(p, g, v, lr: float, mu: float, nesterov: bool, wd: float, mask,
                 gscale: float = 1.0):
    """One step in float64 with the fp32 constants float32(lr), float32(mu), float32(wd) and
    float32(gscale) (as rmsprop_ref rounds its constants).  mask: bool per element, True where
    weight decay applies.  Returns (p, v)."""
    l, m = float(np.float32(lr)), float(np.float32(mu))
    w = float(np.float32(wd)) * mask.double()
    gw = g.double() * float(np.float32(gscale)) + w * p.double()
    vn = m * v.double() + gw
    u = gw + m * vn if nesterov else vn
    return p.double() - l * u, vn


def ranges_mask(n: int, ranges) -> torch.Tensor:
    mask = torch.zeros(n, dtype=torch.bool)
    for b, e in ranges:
        mask[b:e] = True
    return mask


def exact_case(n: int, seed: int = 0):
    """The exact-data condition: p in multiples of 2^-6 with |p| <= 1, v in multiples of 1/4
    with |v| <= 4, integer g with |g| <= 8; with mu = 1/2, lr = 2^-6, wd = 2^-4 every
    intermediate of one step is a multiple of 2^-17 below 32 in magnitude, so fp32 in any
    association or FMA contraction equals float64 bit for bit.  -> (p, g, v, constants)."""
    gen = torch.Generator().manual_seed(seed)
    p = torch.randint(-64, 65, (n,), generator=gen).float() / 64
    v = torch.randint(-16, 17, (n,), generator=gen).float() / 4
    g = torch.randint(-8, 9, (n,), generator=gen).float()
    return p, g, v, dict(lr=2.0 ** -6, mu=0.5, wd=2.0 ** -4)


# ------------------------------------------------------------------------------ 1: config
def test_config_accepts_momentum_and_rejects_misuse():
    cfg = ExperimentConfig().replace(optimizer="momentum", momentum="0.8", nesterov="1",
                                     weight_decay="1e-4")
    assert (cfg.optimizer, cfg.momentum, cfg.nesterov, cfg.weight_decay) == (
        "momentum", 0.8, True, 1e-4)
    assert ExperimentConfig.from_dict(cfg.to_dict()) == cfg
    d = ExperimentConfig().to_dict()
    for k in ("momentum", "nesterov", "weight_decay"):
        del d[k]                       # an older checkpoint's config
    old = ExperimentConfig.from_dict(d)
    assert (old.optimizer, old.momentum, old.nesterov, old.weight_decay) == (
        "sgd", 0.9, False, 0.0)
    base = ExperimentConfig()
    for kw in (dict(optimizer="momentum", momentum=1.0), dict(optimizer="momentum", momentum=-0.1),
               dict(optimizer="momentum", weight_decay=-1e-3),
               dict(nesterov=True), dict(weight_decay=1e-4),
               dict(optimizer="rmsprop", nesterov=True),
               dict(optimizer="rmsprop", weight_decay=1e-4),
               dict(optimizer="adam")):
        with pytest.raises(ValueError):
            base.replace(**kw)
    # (leaving momentum again needs the two fields back at their defaults)
    with pytest.raises(ValueError):
        cfg.replace(optimizer="sgd")
    assert cfg.replace(optimizer="sgd", nesterov=False, weight_decay=0.0).optimizer == "sgd"


# ------------------------------------------------------------- 2: the oracle's own oracle
@pytest.mark.parametrize("nesterov", [False, True])
def test_momentum_ref_matches_float64_torch_sgd(nesterov):
    """torch.optim.SGD keeps the learning rate outside the velocity too (p -= lr * u), so with
    two parameter groups (decayed / not) it is the same recurrence: float64 rounding only
    (measured 4.4e-16)."""
    gen = torch.Generator().manual_seed(5)
    na, nb = 37, 23
    lr, mu, wd = 0.0137, 0.9, 1e-2
    l, m, w = (float(np.float32(x)) for x in (lr, mu, wd))
    p0 = torch.randn(na + nb, generator=gen, dtype=torch.float64)
    a = p0[:na].clone().requires_grad_(True)
    b = p0[na:].clone().requires_grad_(True)
    sgd = torch.optim.SGD([{"params": [a], "weight_decay": w},
                           {"params": [b], "weight_decay": 0.0}],
                          lr=l, momentum=m, dampening=0.0, nesterov=nesterov)
    mask = ranges_mask(na + nb, [(0, na)])
    p, v = p0.clone(), torch.zeros(na + nb, dtype=torch.float64)
    worst = 0.0
    for _ in range(4):
        g = torch.randn(na + nb, generator=gen, dtype=torch.float64)
        a.grad, b.grad = g[:na].clone(), g[na:].clone()
        sgd.step()
        p, v = momentum_ref(p, g, v, lr, mu, nesterov, wd, mask)
        worst = max(worst, (torch.cat([a, b]).detach() - p).abs().max().item())
    print(f"MOMENTUM_REF_VS_TORCH nesterov={nesterov} max_abs_diff={worst:.3e}")
    assert worst <= 1e-12


# ------------------------------------------------------------------ 3: the CPU optimizer
@pytest.mark.parametrize("nesterov", [False, True])
def test_momentum_ref_matches_cpu_optimizer(nesterov):
    """momentum_ref and train/optim.Momentum (fp32 torch ops) agree to 1e-6 relative on the
    velocity and on every parameter over three steps, each compared from the state it started
    from.  Parameters start in [1, 2) and every gradient is positive, so no sum cancels (a
    relative bound on an fp32 difference does not survive cancellation, as
    test_rmsprop_ref_matches_cpu_optimizer notes): about four roundings of 2^-24 each."""
    gen = torch.Generator().manual_seed(6)
    n, ranges = 300, [(0, 101), (128, 200)]
    lr, mu, wd = 0.02, 0.9, 1e-2
    opt = Momentum(lr, 0.0, mu, nesterov, wd, n, ranges)
    p = 1.0 + torch.rand(n, generator=gen)
    mask = ranges_mask(n, ranges)
    for _ in range(3):
        g = torch.rand(n, generator=gen) + 0.1
        p0, v0 = p.clone(), opt.vel.clone()
        opt.step(p, g.clone())
        pr, vr = momentum_ref(p0, g, v0, lr, mu, nesterov, wd, mask)
        assert (pr > 0.5).all() and (vr > 0).all()
        assert ((p.double() - pr).abs() <= 1e-6 * pr).all()
        assert ((opt.vel.double() - vr).abs() <= 1e-6 * vr).all()
    sd = opt.state_dict()
    assert sd["kind"] == "momentum" and set(sd) == {"kind", "rate", "rate_decay", "vel"}


def test_cpu_optimizer_rate_decay():
    opt = Momentum(0.5, 1e-2, 0.9, False, 0.0, 4)
    for _ in range(3):
        opt.step(torch.zeros(4), torch.zeros(4))
    assert opt.rate == 0.5 * (1 - 1e-2) * (1 - 1e-2) * (1 - 1e-2)


# ---------------------------------------------------------------- 4: the decay ranges
def _layout_cfgs():
    return [get_preset("cpu-1layer-k16"),
            ExperimentConfig(numLayers=3, channelSize=64),
            ExperimentConfig(numLayers=12, channelSize=128)]


@pytest.mark.parametrize("cfg", _layout_cfgs(), ids=["1layer-k16", "3x64", "12x128"])
def test_weight_ranges_cover_exactly_the_conv_weights(cfg):
    """g = 0, v = 0, wd > 0: one step moves exactly the conv-weight elements; the biases, the
    per-position biases and the padding keep their bits."""
    lay = ParamLayout(cfg)
    ranges = lay.weight_ranges()
    assert len(ranges) == len(lay.layers) <= 20
    assert all(b % 64 == 0 and b < e for b, e in ranges)
    assert all(ranges[i][1] <= ranges[i + 1][0] for i in range(len(ranges) - 1))
    p0 = init_params(lay, 1)
    pad = torch.ones(lay.numel, dtype=torch.bool)
    for _, off, numel in lay.tensor_ranges():
        pad[off:off + numel] = False
    p0[pad] = 0.25                     # (padding is zero after init: give it a value to lose)
    assert (p0 != 0).all()
    opt = Momentum(0.1, 0.0, 0.9, True, 0.5, lay.numel, ranges)
    p = p0.clone()
    opt.step(p, torch.zeros(lay.numel))
    changed = p != p0
    want = torch.zeros(lay.numel, dtype=torch.bool)
    for i in range(len(lay.layers)):
        w = lay.weight(want, i)
        w[...] = True
    assert torch.equal(changed, want)
    assert torch.equal(changed, ranges_mask(lay.numel, ranges))
    assert torch.equal(p[~want].view(torch.int32), p0[~want].view(torch.int32))
    assert int(want.sum()) == sum(L.w_numel for L in lay.layers)


# ------------------------------------------------------------------ 5: exact data
@pytest.mark.parametrize("nesterov", [False, True])
def test_exact_data_fp32_equals_float64(nesterov):
    """Op by op in fp32 (every product and sum rounded) on exact_case: equal to the float64
    reference bit for bit.  One step per designed state: a second step from the result is not
    exact (its velocity is no multiple of 1/4)."""
    n = 64 * 37 + 3
    ranges = [(0, 64 * 9 + 1), (64 * 20, 64 * 30 + 2)]
    mask = ranges_mask(n, ranges)
    for seed in range(3):
        p, g, v, c = exact_case(n, seed)
        pr, vr = momentum_ref(p, g, v, c["lr"], c["mu"], nesterov, c["wd"], mask)
        f = torch.float32
        gw = g + (torch.tensor(c["wd"], dtype=f) * p) * mask.to(f)
        vn = torch.tensor(c["mu"], dtype=f) * v + gw
        u = gw + torch.tensor(c["mu"], dtype=f) * vn if nesterov else vn
        pn = p - torch.tensor(c["lr"], dtype=f) * u
        assert pn.dtype == f and vn.dtype == f
        assert torch.equal(pn.double(), pr) and torch.equal(vn.double(), vr)
        assert torch.equal(pr.float().double(), pr) and torch.equal(vr.float().double(), vr)
        assert (pr * 2 ** 17 == (pr * 2 ** 17).round()).all() and pr.abs().max() < 32
        assert not torch.equal(pn, p) and mask.any() and not mask.all()


# ------------------------------------------------------------------ 6: the CPU backend
def _exp_cfg(tmp_path, **kw):
    base = dict(numLayers=3, channelSize=16, batchSize=4, validationSize=4,
                validation_interval=1000, log_interval=1000, useCuda=False, synthetic=True,
                checkpoint_dir=str(tmp_path), seed=3, loader_threads=2, prefetch=2,
                rateDecay=1e-2, optimizer="momentum", momentum=0.9, nesterov=True,
                weight_decay=1e-3)
    base.update(kw)
    return ExperimentConfig(**base)


def test_cpu_backend_resume_is_exact_and_reset_starts_from_rest(tmp_path):
    from deep_go_amd.train.experiment import Experiment
    cfg = _exp_cfg(tmp_path)
    a = Experiment(cfg, id="a")
    a.run(3)
    path = a.save()
    assert a.backend.opt.vel.abs().max() > 0
    a2 = Experiment.load(path)
    a2.id = "a2"
    a2.run(3)
    b = Experiment(cfg, id="b")
    b.run(6)
    assert torch.equal(a2.backend.flat_params(), b.backend.flat_params())
    assert torch.equal(a2.backend.opt.vel, b.backend.opt.vel)
    assert a2.backend.rate == b.backend.rate and a2.iterations == 6
    assert not torch.equal(a.backend.opt.vel, b.backend.opt.vel)
    r = Experiment.load(path, reset_optimizer=True)
    r.init()
    assert r.backend.rate == cfg.rate
    assert not r.backend.opt.vel.any()
    assert torch.equal(r.backend.flat_params(), a.backend.flat_params())


def test_cpu_backend_nonfinite_step_keeps_state_and_decays_rate(tmp_path):
    from deep_go_amd.data.synthetic import random_planes
    from deep_go_amd.train.backends import CPUBackend
    cfg = _exp_cfg(tmp_path, nan_policy="skip")
    be = CPUBackend(cfg, 4)
    be.set_batch(*random_planes(4, seed=0))
    be.train_step()
    p0, v0, r0 = be.flat_params().clone(), be.opt.vel.clone(), be.rate
    assert v0.abs().max() > 0
    be.forward_backward()
    be._loss_sum = float("inf")
    be.optimizer_step()
    assert torch.equal(be.flat_params().view(torch.int32), p0.view(torch.int32))
    assert torch.equal(be.opt.vel.view(torch.int32), v0.view(torch.int32))
    assert be.rate == r0 * (1.0 - cfg.rateDecay) and be.bad_steps() == 1
    be.train_step()
    assert not torch.equal(be.flat_params(), p0) and not torch.equal(be.opt.vel, v0)


# ------------------------------------------------------------------ 7: the launcher
def _table(rows):
    return np.ascontiguousarray(np.array(rows, dtype=np.int64).reshape(-1, 2))


BAD_RANGES = {
    "21 ranges": [(64 * i, 64 * i + 8) for i in range(21)],
    "unsorted": [(128, 130), (0, 7)],
    "overlapping": [(0, 100), (64, 128)],
    "misaligned begin": [(4, 40)],
    "past n": [(0, 7), (960, 1001)],
    "empty": [(64, 64)],
}


@pytest.mark.parametrize("name", ["momentum", "momentum_bf16"])
def test_launcher_rejects_invalid_ranges_without_a_gpu(name):
    """The module builds and imports on a machine without a GPU, exposes both entry points,
    and every invalid range table is refused before any GPU work (all pointers are null
    here: a launch would not survive them)."""
    from deep_go_amd.ops import native
    m = native.opt()
    assert sorted(x for x in dir(m) if not x.startswith("_")) == ["momentum", "momentum_bf16"]
    fn = getattr(m, name)
    for what, rows in BAD_RANGES.items():
        t = _table(rows)
        with pytest.raises(RuntimeError) as e:
            fn(0, 0, 0, 1000, 0, 0.9, 0, 1e-4, t.ctypes.data, len(t), 1.0, 0, 0)
        assert str(e.value) == f"{name}: invalid argument", what
    with pytest.raises(RuntimeError) as e:     # a count without a table
        fn(0, 0, 0, 1000, 0, 0.9, 0, 1e-4, 0, 1, 1.0, 0, 0)
    assert str(e.value) == f"{name}: invalid argument"
    # n = 0 with a valid (empty) table: nothing to do, no launch
    fn(0, 0, 0, 0, 0, 0.9, 0, 1e-4, 0, 0, 1.0, 0, 0)
