"""grad_clip without a GPU: the float64 oracle ``clip_ref`` (checked against
``torch.nn.utils.clip_grad_norm_``), the config, the counted fp32 bound of the kernel's sum and
an honest fp32 emulation of it, planted defects that each check catches, the CPU trainer, two
gloo ranks and the argument checks of the ``_dgclip`` launcher.

The definition (train/optim.py clip_grad_, csrc/kernels/clip.hip), with c = grad_clip > 0, over
the whole flat gradient, once per applied step:

    norm  = |gscale| * sqrt(sum_i g[i]^2)
    r     = c / (norm + 1e-6)
    scale = r < 1 ? r : 1
    g[i]  = g[i] * scale          (the optimizer behind it still applies gscale)

A skipped step clips nothing and changes no statistic.

tests/test_clip_gpu.py imports ``clip_ref``, ``norm_bound``, ``kernel_shape``, ``SIZES``,
``expected_scale`` and ``designed_case`` from here.
"""
import math
import os

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from deep_go_amd.config import ExperimentConfig
from deep_go_amd.train.optim import clip_grad_
from test_dist_cpu import _free_port

U24 = 2.0 ** -24
MT, PARTIALS = 256, 1024          # clip.hip: threads per workgroup, the first launch's grid cap
# the kernel tests' sizes: below one 4-vector, tails of 1..3, one and several workgroups, and
# two past the 2^20 elements one pass of the capped grid covers (a partly filled second pass;
# three full passes and one more vector)
SIZES = [1, 2, 3, 4, 7, 1024, 1027, 4099, 65541, 2 ** 20 + 1029, 3 * 2 ** 20 + 7]


def _f32(x) -> float:
    return float(np.float32(x))


# ------------------------------------------------------------------------------ oracle
def clip_ref(g, gscale: float, c: float):
    """(norm, scale, g_clipped) in float64 from the gradient g (any dtype, taken as float64)
    with the fp32 constants float32(gscale), float32(c), as the kernel receives them."""
    gd = g.double()
    norm = abs(_f32(gscale)) * math.sqrt(float((gd * gd).sum()))
    r = _f32(c) / (norm + 1e-6)
    scale = r if r < 1.0 else 1.0
    return norm, scale, gd * scale


def expected_scale(norm32: float, c: float) -> float:
    """The fp32 scale the kernel (and train/optim.py) derives from ITS OWN fp32 norm: r in
    double from the fp32 norm, rounded to fp32 when below 1.  inf -> 0, NaN -> 1."""
    r = _f32(c) / (float(norm32) + 1e-6)
    return _f32(r) if r < 1.0 else 1.0


def kernel_shape(n: int):
    """(workgroups, passes) of clip.hip's first launch over n elements."""
    n4 = n // 4
    grid = max(1, min(-(-n4 // MT), PARTIALS))
    return grid, max(1, -(-n4 // (grid * MT)))


def norm_bound(n: int, passes: int) -> float:
    """Relative bound on the kernel's fp32 norm against the float64 one.  The fp32 roundings on
    the way to one partial, each 2^-24 relative on a sum of non-negative terms, so they add up
    relatively: the square (1; none when it is fused into the sum), the per-thread chain of
    4 * passes sums and one more for the n % 4 tail, the six levels of the wave's butterfly and
    the two levels over the four waves.  The sum of the partials in double and the root add
    far less than one more; the root halves the relative error of the sum of squares, which is
    not used.  The final conversions: the product with |gscale| and the root are formed in
    double and rounded to fp32 once (1), and one more is counted for the double arithmetic
    around it.  Doubled, as the other bounds here."""
    count = 1 + (4 * passes + 1) + 6 + 2 + 2
    return 2 * count * U24


# --------------------------------------------------------------- an fp32 emulation, honest
def emulate_norm(g: torch.Tensor, gscale: float, rng=None, defect: str = ""):
    """The kernel's summation in fp32 numpy arithmetic: the same assignment of elements to
    threads and workgroups and the same tree shape, every product and sum rounded to fp32 (no
    fused multiply-add: one rounding more than the kernel may take).  rng: shuffle the order
    inside each thread's chain and the lanes of the trees.  Returns the fp32 norm.  defect:
    one of the planted ones."""
    x = g.float().numpy()
    n = x.size
    n4 = n // 4
    grid, passes = kernel_shape(n)
    slots = np.zeros((passes * grid * MT, 4), np.float32)
    slots[:n4] = x[:n4 * 4].reshape(n4, 4)
    # [pass, workgroup, thread, element] -> per thread a chain of 4 * passes (+ 1) terms
    chain = slots.reshape(passes, grid, MT, 4).transpose(1, 2, 0, 3).reshape(grid, MT, -1)
    tail = np.zeros((grid, MT, 1), np.float32)
    if defect != "tail dropped":
        tail[0, :n - n4 * 4, 0] = x[n4 * 4:]
    chain = np.concatenate([chain, tail], axis=2)
    if rng is not None:
        chain = chain[:, :, rng.permutation(chain.shape[2])]
    sq = np.abs(chain) if defect == "L1 norm" else chain * chain
    s = np.zeros((grid, MT), np.float32)
    for k in range(sq.shape[2]):
        s = s + sq[:, :, k]
    if rng is not None:            # (lanes within a wave, then the waves)
        s = s.reshape(grid, 4, 64)[:, :, rng.permutation(64)][:, rng.permutation(4), :]
        s = s.reshape(grid, MT)
    w = s.reshape(grid, 4, 64)
    for _ in range(6):
        w = w[:, :, 0::2] + w[:, :, 1::2]
    w = w[:, :, 0]
    part = (w[:, 0] + w[:, 1]) + (w[:, 2] + w[:, 3])
    assert part.dtype == np.float32
    if defect == "last partial dropped":
        part = part[:-1]
    S = float(part.astype(np.float64).sum())
    root = S if defect in ("no square root", "L1 norm") else math.sqrt(S)
    scale = 1.0 if defect == "gscale ignored" else abs(_f32(gscale))
    return _f32(scale * root)


def emulate_clip(g, gscale, c, defect: str = ""):
    """(norm, scale, out) as the kernel pair computes them, with a planted defect."""
    norm = emulate_norm(g, gscale, defect=defect)
    if defect == "1e-6 missing":
        r = _f32(c) / norm
        scale = _f32(r) if r < 1.0 else 1.0
    else:
        scale = expected_scale(norm, c)
    s32 = torch.tensor(scale, dtype=torch.float32)
    out = g.float() * s32
    if defect == "scale applied twice":
        out = out * s32
    return norm, scale, out


def clip_checks(g, gscale, c, norm, scale, out):
    """The three checks the GPU tests make of a (norm, scale, out): the norm within norm_bound
    of clip_ref; the scale the one expected from that very norm, exactly; the output the fp32
    product of the input and that scale, exactly.  -> {name: passed}, the norm's error over
    its bound."""
    n = g.numel()
    ref_norm = clip_ref(g, gscale, c)[0]
    b = norm_bound(n, kernel_shape(n)[1])
    ratio = abs(norm - ref_norm) / (b * ref_norm) if ref_norm > 0 else float(norm != 0)
    ok = {"norm": ratio <= 1.0,
          "scale": scale == expected_scale(norm, c),
          "out": torch.equal(out, g.float() * torch.tensor(scale, dtype=torch.float32))}
    return ok, ratio


def designed_case(n: int, seed: int):
    """Integers in -2..2 times 2^-7, at most 2^20 of them nonzero: every square is a multiple of
    the quantum 2^-14 and every partial sum stays below 2^24 quanta, so fp32 sums them exactly
    in any order.  -> (g fp32, S = sum g^2 exactly, a Python float)."""
    gen = torch.Generator().manual_seed(seed)
    k = torch.randint(-2, 3, (n,), generator=gen)
    if n > 2 ** 20:                        # (4 * 2^20 < 2^24 quanta)
        keep = torch.rand(n, generator=gen) < 0.3
        k = k * keep
        k[0], k[n - 1] = 2, -1             # (both ends count)
    S = int((k * k).sum())
    assert S < 2 ** 24
    return k.float() * 2.0 ** -7, S * 2.0 ** -14


# ------------------------------------------------------------- 1: the oracle's own oracle
@pytest.mark.parametrize("c,clips", [(0.5, True), (100.0, False)])
def test_clip_ref_matches_float64_torch(c, clips):
    """torch.nn.utils.clip_grad_norm_ over two float64 tensors of 37 + 23 elements holding
    g * gscale, against clip_ref: the norm, and the clipped gradient (times gscale).  Measured:
    the norms agree to the last bit, the gradients differ by at most 0.98 ulp of float64 of
    their values (torch scales g * gscale, the oracle g); the bound allows 8."""
    gen = torch.Generator().manual_seed(3)
    gscale = _f32(0.37)
    g = torch.randn(60, generator=gen, dtype=torch.float64) * 3.0
    a = torch.zeros(37, dtype=torch.float64, requires_grad=True)
    b = torch.zeros(23, dtype=torch.float64, requires_grad=True)
    a.grad, b.grad = (g[:37] * gscale).clone(), (g[37:] * gscale).clone()
    total = torch.nn.utils.clip_grad_norm_([a, b], _f32(c), norm_type=2)
    norm, scale, gc = clip_ref(g, gscale, c)
    assert (scale < 1.0) == clips
    got = torch.cat([a.grad, b.grad])
    want = gc * gscale
    ulp = 2.0 ** -52
    dn = abs(float(total) - norm) / norm
    dg = ((got - want).abs() / want.abs()).max().item()
    print(f"CLIP_REF_VS_TORCH c={c} norm_rel_diff={dn / ulp:.2f}ulp grad_rel_diff={dg / ulp:.2f}ulp")
    assert dn <= 8 * ulp and dg <= 8 * ulp
    if not clips:
        assert scale == 1.0 and torch.equal(gc, g)


def test_clip_ref_overflow_and_nan():
    assert expected_scale(float("inf"), 1.0) == 0.0
    assert expected_scale(float("nan"), 1.0) == 1.0
    assert expected_scale(2.0, 1.0) == _f32(1.0 / (2.0 + 1e-6))
    assert expected_scale(0.5, 1.0) == 1.0


# ------------------------------------------------------------------------------ 2: config
def test_config_defaults_old_checkpoints_and_rejections():
    base = ExperimentConfig()
    assert base.grad_clip == 0.0
    d = base.to_dict()
    assert d["grad_clip"] == 0.0
    del d["grad_clip"]                          # an older checkpoint's config
    assert ExperimentConfig.from_dict(d).grad_clip == 0.0
    for opt in ("sgd", "rmsprop", "momentum", "adamw"):
        cfg = base.replace(optimizer=opt, grad_clip="1.0")      # (as the command line gives it)
        assert cfg.grad_clip == 1.0 and ExperimentConfig.from_dict(cfg.to_dict()) == cfg
    assert base.replace(grad_clip=2).grad_clip == 2.0
    for bad in (-1, -1e-9, float("nan"), float("inf"), "-1", "nan", "inf"):
        with pytest.raises(ValueError):
            base.replace(grad_clip=bad)


# ------------------------------------------------------------------------------ 3: the bound
def test_kernel_shape_of_the_sizes():
    shapes = {n: kernel_shape(n) for n in SIZES}
    assert shapes[1] == shapes[7] == (1, 1) and shapes[1024] == (1, 1)
    assert shapes[1027] == (1, 1) and shapes[4099] == (4, 1) and shapes[65541] == (65, 1)
    assert shapes[2 ** 20 + 1029] == (1024, 2) and shapes[3 * 2 ** 20 + 7] == (1024, 4)


@pytest.mark.parametrize("n", SIZES)
def test_honest_fp32_emulation_stays_inside_the_bound(n):
    """The emulation with every product and sum rounded, in the kernel's order and in a
    shuffled one, against clip_ref.  Measured: at most 0.04 of the bound (the roundings of a
    sum of positive terms mostly cancel; the bound counts each at its worst)."""
    gen = torch.Generator().manual_seed(n % 1000)
    g = torch.randn(n, generator=gen) * 0.7
    ref = clip_ref(g, 0.37, 1.0)[0]
    b = norm_bound(n, kernel_shape(n)[1])
    worst = 0.0
    for rng in (None, np.random.default_rng(n), np.random.default_rng(n + 1)):
        got = emulate_norm(g, 0.37, rng)
        worst = max(worst, abs(got - ref) / (b * ref))
    print(f"CLIP_EMULATION n={n} err_over_bound={worst:.3f} bound={b:.3e}")
    assert worst <= 1.0


def test_designed_data_is_exact_in_the_emulation():
    for n in (7, 4099, 2 ** 20 + 1029):
        g, S = designed_case(n, n)
        for rng in (None, np.random.default_rng(5)):
            assert emulate_norm(g, 0.75, rng) == _f32(0.75 * math.sqrt(S))


# --------------------------------------------------------------------- 4: planted defects
DEFECTS = {"gscale ignored": "norm", "no square root": "norm", "scale applied twice": "out",
           "tail dropped": "norm", "last partial dropped": "norm", "L1 norm": "norm",
           "1e-6 missing": "scale"}


@pytest.mark.parametrize("defect", list(DEFECTS))
def test_planted_defect_fails_its_check(defect):
    """Each defect, planted in the emulation, fails the check named for it (and the clean
    emulation passes all three on the same data)."""
    gen = torch.Generator().manual_seed(9)
    n = 4099                     # four workgroups, a 3-element tail
    g = torch.randn(n, generator=gen) * 0.7
    gscale, c = 0.37, 1.0
    if defect == "1e-6 missing":
        g = g * (1e-5 / clip_ref(g, gscale, c)[0])        # norm ~ 1e-5
        c = 5e-6
        assert abs(clip_ref(g, gscale, c)[0] - 1e-5) < 1e-7
    ok, _ = clip_checks(g, gscale, c, *emulate_clip(g, gscale, c))
    assert all(ok.values()), ok
    ok, ratio = clip_checks(g, gscale, c, *emulate_clip(g, gscale, c, defect))
    assert not ok[DEFECTS[defect]], (defect, ok, ratio)


# --------------------------------------------------------------- 5: train/optim.py clip_grad_
def test_cpu_clip_matches_the_oracle():
    gen = torch.Generator().manual_seed(4)
    g = torch.randn(3001, generator=gen) * 0.3
    for gscale, c in ((1.0, 0.5), (0.37, 0.5), (1.0, 1e30)):
        x = g.clone()
        norm, scale = clip_grad_(x, c, gscale)
        rn, rs, rg = clip_ref(g, gscale, c)
        assert abs(norm - rn) <= 2 * U24 * rn and scale == expected_scale(norm, c)
        assert torch.equal(x, g * torch.tensor(scale, dtype=torch.float32))
        assert (scale < 1.0) == (rs < 1.0)
        assert ((x.double() - rg).abs() <= 4 * U24 * rg.abs()).all()
    x = g.clone()
    x[5] = float("inf")
    assert clip_grad_(x, 1.0)[1] == 0.0
    x = g.clone()
    x[5] = float("nan")
    assert clip_grad_(x, 1.0)[1] == 1.0


# ------------------------------------------------------------------ 6: the CPU trainer
def _exp_cfg(tmp_path, data_root, **kw):
    base = dict(numLayers=3, channelSize=16, batchSize=4, validationSize=4,
                validation_interval=1000, log_interval=1000, useCuda=False, synthetic=False,
                data_root=data_root, checkpoint_dir=str(tmp_path), seed=3, loader_threads=2,
                prefetch=2, rate=1e-3, rateDecay=1e-2, nan_policy="skip",
                # (with the head's ReLU this tiny net dies under adamw within three steps: its
                # gradient is then exactly zero, and there is no norm to look at)
                head_relu=False)
    base.update(kw)
    return ExperimentConfig(**base)


@pytest.mark.parametrize("opt", ["sgd", "rmsprop", "momentum", "adamw"])
def test_cpu_trainer_never_clipping_is_bit_identical(tmp_path, packed_fixture, opt):
    from deep_go_amd.train.experiment import Experiment
    out = []
    for clip in (0.0, 1e30):
        e = Experiment(_exp_cfg(tmp_path, packed_fixture, optimizer=opt, grad_clip=clip),
                       id=f"{opt}{clip}")
        e.run(5)
        out.append(e)
    a, b = (e.backend.flat_params() for e in out)
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert out[0].backend.rate == out[1].backend.rate
    norm, scale, clipped = out[1].backend.clip_stats()
    assert norm > 0 and scale == 1.0 and clipped == 0
    assert out[0].backend.clip_stats() == (0.0, 0.0, 0)


def test_cpu_trainer_clipped_sgd_steps_are_bounded(tmp_path, packed_fixture):
    """sgd with a small grad_clip: every step moves the parameters by at most rate_t * c *
    (1 + 1e-6) in L2, up to the fp32 roundings of p - rate * g (2^-24 |p| per element for the
    difference, as much again for the product: 2^-23 ||p|| in all), and all five steps clip.
    With log_interval = 1 each step writes one kind="clip" record after its "train" record."""
    from deep_go_amd.train.experiment import Experiment
    from deep_go_amd.utils.metrics import read_jsonl
    c = 0.05
    mpath = str(tmp_path / "metrics.jsonl")
    e = Experiment(_exp_cfg(tmp_path, packed_fixture, grad_clip=c, log_interval=1, rate=1e-2,
                            metrics_path=mpath), id="clipped")
    e.init()
    be = e.backend
    for t in range(5):
        p0, rate = be.flat_params().clone(), be.rate
        e.run(1)
        d = (be.flat_params().double() - p0.double()).norm().item()
        lim = rate * c * (1 + 1e-6) + 2.0 ** -23 * p0.double().norm().item()
        norm, scale, clipped = be.clip_stats()
        print(f"CLIP_CPU_STEP t={t} step_norm={d:.6e} limit={lim:.6e} grad_norm={norm:.4f}")
        assert 0 < d <= lim
        assert clipped == t + 1 and scale == expected_scale(norm, c) and norm > c
    e.metrics.close()
    rows = read_jsonl(mpath)
    clips = [r for r in rows if r.get("kind") == "clip"]
    assert [r["step"] for r in clips] == [1, 2, 3, 4, 5]
    assert [r["clipped_steps"] for r in clips] == [1, 2, 3, 4, 5]
    assert set(clips[0]) == {"kind", "step", "grad_norm", "clip_scale", "clipped_steps", "time"}
    kinds = [r["kind"] for r in rows if r.get("kind") in ("train", "clip")]
    assert kinds == ["train", "clip"] * 5
    assert all(r["clip_scale"] < 1.0 and r["grad_norm"] > c for r in clips)


def test_cpu_skipped_step_clips_nothing(tmp_path, packed_fixture):
    from deep_go_amd.data.synthetic import random_planes
    from deep_go_amd.train.backends import CPUBackend
    cfg = _exp_cfg(tmp_path, packed_fixture, grad_clip=1e-3)
    be = CPUBackend(cfg, 4)
    be.set_batch(*random_planes(4, seed=0))
    be.train_step()
    p0, stats0 = be.flat_params().clone(), be.clip_stats()
    assert stats0[2] == 1
    be.forward_backward()
    g0 = be.params.grad.clone()
    be._loss_sum = float("nan")
    be.optimizer_step()
    assert torch.equal(be.flat_params().view(torch.int32), p0.view(torch.int32))
    assert torch.equal(be.params.grad.view(torch.int32), g0.view(torch.int32))
    assert be.clip_stats() == stats0 and be.bad_steps() == 1
    be.train_step()
    assert be.clip_stats()[2] == 2 and not torch.equal(be.flat_params(), p0)


def test_checkpoint_does_not_carry_the_statistic(tmp_path, packed_fixture):
    """clipped_steps is a statistic of the run; resume is exact in parameters and state."""
    from deep_go_amd.train.experiment import Experiment
    cfg = _exp_cfg(tmp_path, packed_fixture, optimizer="adamw", grad_clip=1e-3)
    a = Experiment(cfg, id="a")
    a.run(2)
    a2 = Experiment.load(a.save())
    a2.id = "a2"
    a2.run(2)
    b = Experiment(cfg, id="b")
    b.run(4)
    assert torch.equal(a2.backend.flat_params(), b.backend.flat_params())
    assert torch.equal(a2.backend.opt.m, b.backend.opt.m)
    assert torch.equal(a2.backend.opt.v, b.backend.opt.v)
    assert a2.backend.clip_stats()[2] == 2 and b.backend.clip_stats()[2] == 4
    assert a2.backend.clip_stats()[:2] == b.backend.clip_stats()[:2]


# ------------------------------------------------------------------ 7: two ranks
def _dp_worker(rank, world, port, out_dir):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank),
                      WORLD_SIZE=str(world), LOCAL_RANK=str(rank))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from deep_go_amd.data.synthetic import random_planes
    from deep_go_amd.train.backends import CPUBackend
    cfg = ExperimentConfig(numLayers=3, channelSize=16, rate=1e-2, seed=5, bucket_mb=0.01,
                           grad_clip=1e-3)
    B = 8
    be = CPUBackend(cfg, B // world, world=world, bucket_mb=0.01)
    norms = []
    for step in range(3):
        planes, player, rank_, labels = random_planes(B, seed=step)
        sl = slice(rank * (B // world), (rank + 1) * (B // world))
        be.set_batch(planes[sl], player[sl], rank_[sl], labels[sl])
        be.forward_backward()
        be.optimizer_step()
        norms.append(be.clip_stats()[0])
    torch.save({"params": be.flat_params().clone(), "norms": norms,
                "clipped": be.clip_stats()[2]}, os.path.join(out_dir, f"rank{rank}.pt"))
    dist.barrier()
    dist.destroy_process_group()


def test_two_gloo_ranks_clip_alike(tmp_path):
    """Every rank scans the same all-reduced gradient: after three clipped steps both ranks
    hold bit-identical parameters and report the same norms.  No collective is added."""
    mp.spawn(_dp_worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True)
    a = torch.load(str(tmp_path / "rank0.pt"), weights_only=True)
    b = torch.load(str(tmp_path / "rank1.pt"), weights_only=True)
    assert torch.equal(a["params"].view(torch.int32), b["params"].view(torch.int32))
    assert a["norms"] == b["norms"] and all(x > 1e-3 for x in a["norms"])
    assert a["clipped"] == b["clipped"] == 3


# ------------------------------------------------------------------ 8: the launcher
def _clip():
    from deep_go_amd.ops import native
    try:
        return native.clip()
    except Exception as e:                                   # noqa: BLE001
        pytest.skip(f"_dgclip is not built: {e}")


# fake, suitably aligned, non-null addresses: every call below is refused before any launch
_G, _OUT, _PART, _REC = 0x1000, 0x2000, 0x3000, 0x4008


def _call(m, name, g=_G, out=_OUT, n=1000, part=_PART, part_n=PARTIALS, rec=_REC, c=1.0,
          gscale=1.0):
    if name == "grad_clip":
        m.grad_clip(g, n, part, part_n, rec, c, gscale, 0, 0)
    else:
        m.grad_clip_bf16(g, out, n, part, part_n, rec, c, gscale, 0, 0)


def test_module_public_names():
    m = _clip()
    assert sorted(x for x in dir(m) if not x.startswith("_")) == [
        "clip_partials", "grad_clip", "grad_clip_bf16", "grad_norm", "grad_norm_bf16"]
    assert m.clip_partials() == PARTIALS


@pytest.mark.parametrize("name", ["grad_clip", "grad_clip_bf16"])
def test_launcher_refuses_invalid_arguments_without_a_gpu(name):
    """Every refusal happens before any GPU work (no GPU here, and the addresses are fake: a
    launch would not survive them)."""
    m = _clip()
    bad = {
        "null gradient": dict(g=0), "null partials": dict(part=0), "null record": dict(rec=0),
        "gradient misaligned": dict(g=_G + (4 if name == "grad_clip" else 2)),
        "record off 8 bytes": dict(rec=_REC + 4),
        "partials too few": dict(part_n=PARTIALS - 1), "no partials": dict(part_n=0),
        "max_norm = 0": dict(c=0.0), "max_norm < 0": dict(c=-1.0),
        "max_norm nan": dict(c=math.nan), "max_norm inf": dict(c=math.inf),
        "gscale nan": dict(gscale=math.nan), "gscale inf": dict(gscale=-math.inf),
    }
    if name == "grad_clip_bf16":
        bad.update({"no out": dict(out=0), "out off 16 bytes": dict(out=_OUT + 8)})
    for what, kw in bad.items():
        with pytest.raises(RuntimeError) as e:
            _call(m, name, **kw)
        assert str(e.value) == f"{name}: invalid argument", what
    # n = 0: nothing to do, no launch, whatever the pointers
    _call(m, name, g=0, out=0, n=0, part=0, part_n=0, rec=0)
    with pytest.raises(RuntimeError) as e:     # (max_norm and gscale are checked even then)
        _call(m, name, g=0, out=0, n=0, part=0, part_n=0, rec=0, c=-1.0)
    assert str(e.value) == f"{name}: invalid argument"


@pytest.mark.parametrize("name", ["grad_norm", "grad_norm_bf16"])
def test_norm_launcher_refuses_invalid_arguments_without_a_gpu(name):
    fn = getattr(_clip(), name)
    off = 4 if name == "grad_norm" else 2
    for args in ((0, 1000, _PART, PARTIALS), (_G + off, 1000, _PART, PARTIALS),
                 (_G, 1000, 0, PARTIALS), (_G, 1000, _PART, PARTIALS - 1)):
        with pytest.raises(RuntimeError) as e:
            fn(*args, 0, 0)
        assert str(e.value) == f"{name}: invalid argument"
    fn(0, 0, 0, 0, 0, 0)
