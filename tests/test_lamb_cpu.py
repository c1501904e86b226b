"""optimizer=lamb without a GPU: the config, the float64 oracle ``lamb_ref`` (checked three
independent ways), the counted fp32 bounds ``lamb_bounds`` with an fp32 emulation of the
kernels' summation order, planted defects, the CPU optimizer, the count of APPLIED steps, exact
resume on the CPU backend (and the move adamw -> lamb), the argument checks of the ``_dglamb``
launcher and two gloo ranks.

The definition (train/optim.py Lamb), per flat element, with m = v = 0 and t = 0 at the start,
only when the step is applied; R_k are the conv-weight ranges:

    t += 1;  c1 = 1 / (1 - beta1^t);  c2 = 1 / sqrt(1 - beta2^t)        (double, then fp32)
    gi = g * gscale
    m  = beta1 m + (1 - beta1) gi;   v = beta2 v + (1 - beta2) gi^2
    r  = (c1 m) / (sqrt(v) c2 + eps)
    u  = r + wd p inside a range, r elsewhere
    per k: SP = sum_{R_k} p^2, SU = sum_{R_k} u^2 (each rounded to fp32), wn = fp32(sqrt(SP)),
           un = fp32(sqrt(SU)), phi = fp32(double(wn) / double(un)) if both are finite and > 0,
           else 1
    p -= (lr phi_k) u                                   (phi = 1 outside every range)

A skipped step leaves p, m, v and t alone and still decays the rate.

tests/test_lamb_gpu.py imports ``check_lamb_step`` (which applies ``lamb_ref`` and
``lamb_bounds``), ``trust_ratio32`` and the emulation's case from here.
"""
import math
import os

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from deep_go_amd.config import ExperimentConfig
from deep_go_amd.train.optim import Lamb, trust_ratio
from test_adamw_cpu import (APPLY, BETAS, DIV_ULPS, EPS, SQRT_ULPS, U24, _f32, _skip_call,
                            adam_corrections, adamw_ref)
from test_dist_cpu import _free_port
from test_momentum_cpu import BAD_RANGES, _table, ranges_mask

FLT_MAX = float(np.finfo(np.float32).max)
MT, CE, SLOTS = 256, 1024, 4     # optim.hip: threads per workgroup, elements per chunk, slots
STAGES = ("m", "v", "u", "wn", "un", "phi", "p")


# ------------------------------------------------------------------------------ oracle
def lamb_ref(p, g, m, v, t: int, lr: float, betas, eps: float, wd: float, ranges,
             gscale: float = 1.0, c32: bool = True):
    """Applied step number t (1 for the first) in float64 with the fp32 constants float32(lr),
    float32(beta), float32(eps), float32(wd), float32(gscale), as adamw_ref rounds them.  The
    norms and ratios stay in double (no fp32 rounding).  -> (p, m, v, u, [(wn, un, phi)])."""
    l, b1, b2, e, w, s = (_f32(x) for x in (lr, betas[0], betas[1], eps, wd, gscale))
    c1, c2 = adam_corrections(t, betas, c32)
    gi = g.double() * s
    mn = b1 * m.double() + (1.0 - b1) * gi
    vn = b2 * v.double() + (1.0 - b2) * gi * gi
    u = (c1 * mn) / (vn.sqrt() * c2 + e)
    pd = p.double()
    phi = torch.ones_like(u)
    for b_, e_ in ranges:
        u[b_:e_] += w * pd[b_:e_]
    stats = []
    for b_, e_ in ranges:
        wn = math.sqrt(float((pd[b_:e_] * pd[b_:e_]).sum()))
        un = math.sqrt(float((u[b_:e_] * u[b_:e_]).sum()))
        ok = wn > 0 and un > 0 and math.isfinite(wn) and math.isfinite(un)
        stats.append((wn, un, wn / un if ok else 1.0))
        phi[b_:e_] = stats[-1][2]
    return pd - l * phi * u, mn, vn, u, stats


def trust_ratio32(wn: float, un: float) -> float:
    """phi as both backends derive it from the recorded fp32 norms, exactly."""
    wn, un = np.float32(wn), np.float32(un)
    ok = np.isfinite(wn) and np.isfinite(un) and wn > 0 and un > 0
    return float(np.float32(np.float64(wn) / np.float64(un))) if ok else 1.0


# the fp32 roundings on the way from the elements to one norm, each 2^-24 relative on a sum of
# non-negative terms (as test_clip_cpu.norm_bound counts them): the square (1), a thread's chain
# of at most 4 sums, the six levels of the wave's butterfly, the two levels over the four
# waves; the partials are summed in double (counted as 1 with everything else in double), the
# sum is rounded to fp32 (1) and so is the root (1).  The root halves the relative error of the
# sum, which is not used.  Doubled, as the other bounds here.
NORM_COUNT = 1 + 4 + 6 + 2 + 1 + 1 + 1
NORM_REL = 2 * NORM_COUNT * U24


def lamb_bounds(p0, g, m0, v0, ref, t, lr, betas, eps, wd, ranges, gscale):
    """Counted as adamw_bounds counts, then doubled.  ref = lamb_ref's result.
    -> (bm, bv, bu absolute per element; [(rel wn, rel un)] per range).

    m, v: as adamw_bounds (four roundings on |b1 m0| + |o1 gi|; six on v).
    r = (c1 m) / (sqrt(v) c2 + eps): relative 6 + 2 (SQRT_ULPS + DIV_ULPS) — c1 m, half of v's six
      through the root, the product with c2, the sum with eps, the root's and the quotient's own
      error (an ulp is at most 2^-23 relative) — plus m's bound times c1 / denominator.
    u = r + wd p: one for the product on |wd p|, one for the sum on |u|.
    wn: NORM_REL.  un: NORM_REL plus ||bu over the range||_2 / un, because | ||a|| - ||b|| | <=
      ||a - b||."""
    l, b1, b2, e, w, s = (_f32(x) for x in (lr, betas[0], betas[1], eps, wd, gscale))
    c1, c2 = adam_corrections(t, betas)
    pr, mr, vr, ur, stats = ref
    gi = g.double() * s
    bm = 2 * 4 * U24 * ((b1 * m0.double()).abs() + ((1.0 - b1) * gi).abs())
    bv = 2 * 6 * U24 * vr
    den = vr.sqrt() * c2 + e
    r = c1 * mr / den
    mask = ranges_mask(p0.numel(), ranges).to(p0.device).double()
    wp = w * mask * p0.double()
    bu = 2 * U24 * ((6 + 2 * (SQRT_ULPS + DIV_ULPS)) * r.abs() + wp.abs() + ur.abs()) \
        + c1 / den * bm
    rel = []
    for (b_, e_), (wn, un, _) in zip(ranges, stats):
        extra = float((bu[b_:e_] * bu[b_:e_]).sum()) ** 0.5 / un if un > 0 else 0.0
        rel.append((NORM_REL, NORM_REL + extra))
    return bm, bv, bu, rel


def check_lamb_step(p0, g, m0, v0, p1, m1, v1, u1, stats1, t, lr, betas, eps, wd, ranges, gscale,
                    tag, must_pass: bool = True):
    """One applied step in stages, each against its own reference.  -> {stage: error / bound}
    (phi: 0 or inf).

      m, v, u   elementwise against lamb_ref within lamb_bounds
      wn, un    the recorded fp32 norms against lamb_ref's within their relative bounds; a
                reference norm above fp32's range must be recorded as inf
      phi       the recorded ratio is trust_ratio32 of the recorded norms, bit for bit
      p         against p0 - (lr phi) u_ref with the RECORDED phi (1 outside every range): the
                product lr phi, the product with u and the difference (2^-24 each, doubled), plus
                lr phi times u's bound."""
    ref = lamb_ref(p0, g, m0, v0, t, lr, betas, eps, wd, ranges, gscale)
    pr, mr, vr, ur, rstats = ref
    bm, bv, bu, rel = lamb_bounds(p0, g, m0, v0, ref, t, lr, betas, eps, wd, ranges, gscale)
    out = {}

    def stage(name, got, want, b):
        err = (got.double() - want).abs()
        ratio = torch.where(err == 0, torch.zeros_like(err), err / b.clamp_min(1e-300))
        ratio = torch.where(torch.isnan(ratio), torch.full_like(ratio, math.inf), ratio)
        out[name] = max(out.get(name, 0.0), ratio.max().item() if ratio.numel() else 0.0)

    stage("m", m1, mr, bm)
    stage("v", v1, vr, bv)
    stage("u", u1, ur, bu)
    assert len(stats1) == len(ranges), tag
    phi = torch.ones_like(pr)
    out.update(wn=0.0, un=0.0, phi=0.0)
    for k, ((b_, e_), (wn, un, ph), (rw, ru, _), (relw, relu)) in enumerate(
            zip(ranges, stats1, rstats, rel)):
        for name, got, want, rb in (("wn", wn, rw, relw), ("un", un, ru, relu)):
            if want > math.sqrt(FLT_MAX) * 1.001:
                r_ = 0.0 if got == math.inf else math.inf
            elif want == 0.0:
                r_ = 0.0 if got == 0.0 else math.inf
            else:
                r_ = abs(got - want) / (rb * want)
                r_ = math.inf if math.isnan(r_) else r_
            out[name] = max(out[name], r_)
        if not ph == trust_ratio32(wn, un):
            out["phi"] = math.inf
        phi[b_:e_] = ph
    l = _f32(lr)
    step = l * phi * ur
    stage("p", p1, p0.double() - step, 2 * U24 * ((p0.double() - step).abs() + 2 * step.abs())
          + l * phi.abs() * bu)
    if must_pass:
        bad = {k: v for k, v in out.items() if not v <= 1.0}
        assert not bad, (tag, "error / bound", bad)
    return out


# ------------------------------------------------- an fp32 emulation of the kernels' order
def _chain32(x, rng=None):
    """[..., k] -> fp32 sum of each row, left to right (rng: in a shuffled order)."""
    if rng is not None:
        x = x[..., rng.permutation(x.shape[-1])]
    s = np.zeros(x.shape[:-1], np.float32)
    for k in range(x.shape[-1]):
        s = (s + x[..., k]).astype(np.float32)
    return s


def _chunk_sum32(sq, rng=None):
    """One chunk's 1024 squares (zeros where an element is not counted) as lamb_moments sums
    them: thread chains of 4, the xor butterfly of each wave, (w0 + w1) + (w2 + w3)."""
    s = _chain32(sq.reshape(MT, 4), rng)
    w = s.reshape(4, 64)
    if rng is not None:
        w = w[:, rng.permutation(64)]
    for o in (32, 16, 8, 4, 2, 1):
        w = (w + w[:, np.arange(64) ^ o]).astype(np.float32)
    w = w[:, 0]
    return np.float32(np.float32(w[0] + w[1]) + np.float32(w[2] + w[3]))


def emulate_sumsq(x, b, e, rng=None, defect=""):
    """sum x[b:e]^2 in the kernels' order: fp32 per (chunk, range), the n % 4 tail in a chain of
    its own, the partials in double."""
    n = x.size
    n4 = n // 4
    if defect == "last element dropped":
        e -= 1
    total = 0.0
    lim = min(e, n4 * 4)
    for c in range(b // CE, (lim - 1) // CE + 1 if b < lim else 0):
        lo, hi = max(b, c * CE), min(lim, (c + 1) * CE)
        sq = np.zeros(CE, np.float32)
        with np.errstate(over="ignore"):
            sq[lo - c * CE:hi - c * CE] = x[lo:hi] * x[lo:hi]
            total += float(_chunk_sum32(sq, rng))
    if e > n4 * 4:
        t = x[max(b, n4 * 4):e]
        total += float(_chain32((t * t).astype(np.float32)[None, :], rng)[0])
    return total


def emulate_lamb(p0, g, m0, v0, t, lr, betas, eps, wd, ranges, gscale=1.0, rng=None,
                 defect="", call=None):
    """(p, m, v, u, stats) in fp32 numpy arithmetic, every product, sum, root and quotient
    rounded to fp32 (no fused multiply-add: one rounding more than the kernel may take), the
    sums in the kernels' order.  defect: one of the planted ones."""
    f = np.float32
    l, b1, b2, e, w, s = (f(x) for x in (lr, betas[0], betas[1], eps, wd, gscale))
    c1, c2 = (f(c) for c in adam_corrections(call if defect == "t from the call" else t, betas))
    p, gi = p0.numpy().astype(f), (g.float().numpy().astype(f) * s).astype(f)
    m = (b1 * m0.numpy() + (f(1) - b1) * gi).astype(f)
    v = (b2 * v0.numpy() + ((f(1) - b2) * gi).astype(f) * gi).astype(f)
    u = ((c1 * m) / (np.sqrt(v).astype(f) * c2 + e).astype(f)).astype(f)
    mask = ranges_mask(p.size, ranges).numpy()
    if defect != "decay left out of u":
        u = np.where(mask, (u + (w * p).astype(f)).astype(f), u)
    phi = np.ones_like(p)
    stats = []
    for b_, e_ in ranges:
        sp = emulate_sumsq(p, b_, e_, rng, defect)
        su = emulate_sumsq(gi if defect == "ratio from g" else u, b_, e_, rng, defect)
        wn, un, ph = trust_ratio(sp, su)
        if defect == "zero norm gives 0" and not (wn > 0 and un > 0):
            ph = 0.0
        stats.append((wn, un, ph))
    if defect == "one global ratio":
        allp = math.sqrt(sum(s_[0] ** 2 for s_ in stats))
        allu = math.sqrt(sum(s_[1] ** 2 for s_ in stats))
        stats = [(wn, un, trust_ratio32(allp, allu)) for wn, un, _ in stats]
    for (b_, e_), (_, _, ph) in zip(ranges, stats):
        phi[b_:e_] = ph
    if defect == "biases adapted":
        phi[~mask] = f(0.5)
    lp = (l * phi).astype(f)
    if defect == "ratio applied twice":
        lp = (lp * phi).astype(f)
    pn = (p - (lp * u).astype(f)).astype(f)
    return tuple(torch.from_numpy(a) for a in (pn, m, v, u)) + (stats,)


def _case(n, seed, p_scale=1.0):
    gen = torch.Generator().manual_seed(seed)
    p = torch.randn(n, generator=gen) * p_scale
    g = torch.randn(n, generator=gen) * 0.3
    m = torch.randn(n, generator=gen) * 0.05
    v = torch.rand(n, generator=gen) * 0.01 + 1e-4
    return p, g, m, v


LR, WD = 0.0137, 0.05
# n = 4099: four chunks and a 3-element tail.  A range ending
# in the middle of a 4-vector, three short ones inside one chunk, one over several chunks that
# ends at n (inside the tail)
N_EMU = 4099
RANGES_EMU = [(0, 64 * 3 + 1), (1024 + 64, 1024 + 64 + 5), (1024 + 128, 1024 + 128 + 63),
              (1024 + 256, 1024 + 256 + 130), (2048 - 64, N_EMU)]


# ------------------------------------------------------------------------------ 1: config
def test_config_accepts_lamb_and_rejects_misuse():
    cfg = ExperimentConfig().replace(optimizer="lamb", adam_beta1="0.8", adam_beta2="0.99",
                                     adam_eps="1e-6", weight_decay="1e-2")
    assert (cfg.optimizer, cfg.adam_beta1, cfg.adam_beta2, cfg.adam_eps, cfg.weight_decay) == (
        "lamb", 0.8, 0.99, 1e-6, 1e-2)
    assert ExperimentConfig.from_dict(cfg.to_dict()) == cfg
    # the state's fields move between the two optimizers that share them
    assert cfg.replace(optimizer="adamw").adam_beta1 == 0.8
    base = ExperimentConfig()
    for kw in (dict(optimizer="lamb", nesterov=True), dict(optimizer="lamb", adam_beta1=1.0),
               dict(optimizer="lamb", adam_eps=0.0), dict(optimizer="lamb", weight_decay=-1e-3),
               dict(optimizer="lambda")):
        with pytest.raises(ValueError):
            base.replace(**kw)
    # the existing wording stays as a prefix
    with pytest.raises(ValueError, match="^adam_beta1 needs optimizer=adamw"):
        base.replace(adam_beta1=0.8)
    with pytest.raises(ValueError, match="^weight_decay needs optimizer=momentum or adamw"):
        base.replace(weight_decay=1e-4)
    with pytest.raises(ValueError, match="^nesterov needs optimizer=momentum"):
        base.replace(optimizer="lamb", nesterov=True)
    d = ExperimentConfig().to_dict()            # an older checkpoint's config is unaffected
    assert ExperimentConfig.from_dict(d).optimizer == "sgd"


# ------------------------------------------------------------- 2: the oracle's own oracles
def test_lamb_ref_without_ranges_is_adam():
    """No range, weight_decay = 0: every ratio is 1 and the step is adamw_ref's, over five
    steps from t = 0.  The two differ in association only (lr (c1 m / d) against (lr c1) m / d):
    a few float64 roundings on an update below 0.02, on p ~ 1."""
    p, g, m, v = (x.double() for x in _case(301, 1))
    m, v = torch.zeros_like(m), torch.zeros_like(v)
    pa, ma, va = p.clone(), m.clone(), v.clone()
    mask = torch.zeros(301, dtype=torch.bool)
    gen = torch.Generator().manual_seed(2)
    worst = 0.0
    for t in range(1, 6):
        g = torch.randn(301, generator=gen, dtype=torch.float64)
        p, m, v, _, stats = lamb_ref(p, g, m, v, t, LR, BETAS, EPS, 0.0, [])
        pa, ma, va = adamw_ref(pa, g, ma, va, t, LR, BETAS, EPS, 0.0, mask)
        assert stats == [] and torch.equal(m, ma) and torch.equal(v, va)
        worst = max(worst, (p - pa).abs().max().item())
    print(f"LAMB_REF_VS_ADAMW_REF max_abs_diff={worst:.3e}")
    assert worst <= 5e-16


def test_lamb_ref_moves_every_range_by_rate_times_its_norm():
    """What defines a trust ratio: ||delta p_k||_2 = lr ||p_k||_2 for every range with positive
    norms, whatever the gradient's scale; outside the ranges the step is Adam's."""
    n, ranges = 700, [(0, 130), (192, 193), (256, 601)]
    p, g, m, v = _case(n, 3)
    g[0:130] *= 1e3
    g[256:601] *= 1e-3
    pr, _, _, u, stats = lamb_ref(p, g, m, v, 7, LR, BETAS, EPS, WD, ranges)
    l = _f32(LR)
    for (b, e), (wn, un, phi) in zip(ranges, stats):
        d = (pr[b:e] - p[b:e].double()).norm().item()
        assert abs(d - l * wn) <= 1e-14 * l * wn, (b, e, d, l * wn)
    mask = ranges_mask(n, ranges)
    assert torch.equal(pr[~mask], p.double()[~mask] - l * u[~mask])
    assert len({round(s[2], 6) for s in stats}) == 3


def test_lamb_ref_hand_worked_case():
    """Two ranges of 3 + 2 elements and one element outside, one step from t = 0 with beta1 =
    beta2 = 1/2, eps = 2^-40 ~ 0 against exact numbers (the corrections kept in double): c1 = 2,
    c2 = sqrt(2); m = g / 2, v = g^2 / 2, so r = g / (|g| + eps) = sign(g) up to eps.  With wd = 1/2:
    range 0: p = (3, 0, -4), g = (+, -, +): u = (1 + 1.5, -1, 1 - 2) = (2.5, -1, -1);
      wn = 5, un = sqrt(8.25), phi = 5 / sqrt(8.25)
    range 1: p = (0, 0): wn = 0 -> phi = 1, u = (1, -1)
    outside: p = 2, g = -: u = -1 (no decay), phi = 1."""
    n = 64 + 2 + 62 + 1
    ranges = [(0, 3), (64, 66)]
    p, g = torch.zeros(n), torch.zeros(n)
    p[0:3] = torch.tensor([3.0, 0.0, -4.0])
    g[0:3] = torch.tensor([2.0, -8.0, 0.5])
    g[64:66] = torch.tensor([1.0, -1.0])
    p[128], g[128] = 2.0, -3.0
    lr, eps = 0.25, 2.0 ** -40
    pr, mr, vr, u, stats = lamb_ref(p, g, torch.zeros(n), torch.zeros(n), 1, lr, (0.5, 0.5),
                                    eps, 0.5, ranges, c32=False)
    assert torch.equal(mr, g.double() / 2) and torch.equal(vr, g.double() ** 2 / 2)
    want_u = torch.zeros(n, dtype=torch.float64)
    want_u[0:3] = torch.tensor([2.5, -1.0, -1.0])
    want_u[64:66] = torch.tensor([1.0, -1.0])
    want_u[128] = -1.0
    assert (u - want_u).abs().max() < 1e-10
    phi0 = 5.0 / math.sqrt(8.25)
    assert stats[0][0] == 5.0 and abs(stats[0][1] - math.sqrt(8.25)) < 1e-10
    assert abs(stats[0][2] - phi0) < 1e-10 and stats[1] == (0.0, pytest.approx(math.sqrt(2)), 1.0)
    want_p = p.double() - 0.25 * want_u * torch.where(
        torch.arange(n) < 3, torch.tensor(phi0, dtype=torch.float64),
        torch.tensor(1.0, dtype=torch.float64))
    assert (pr - want_p).abs().max() < 1e-10
    assert abs(pr[0].item() - (3.0 - 0.25 * phi0 * 2.5)) < 1e-10 and pr[128].item() == \
        pytest.approx(2.25, abs=1e-10)


# ------------------------------------------------------------------ 3: the bounds
@pytest.mark.parametrize("shuffled", [False, True])
def test_fp32_emulation_of_the_kernels_stays_inside_the_bounds(shuffled):
    """Every stage of check_lamb_step on an fp32 emulation that takes one rounding more than
    the kernels may (no fused multiply-add), in their order and in a shuffled one."""
    rng = np.random.default_rng(5) if shuffled else None
    worst = {}
    for seed, gscale, t in ((11, 1.0, 1), (12, 0.37, 7), (13, 1.0, 10 ** 6)):
        p, g, m, v = _case(N_EMU, seed, p_scale=0.1 * seed)
        got = emulate_lamb(p, g, m, v, t, LR, BETAS, EPS, WD, RANGES_EMU, gscale, rng)
        out = check_lamb_step(p, g, m, v, *got, t, LR, BETAS, EPS, WD, RANGES_EMU, gscale,
                              (seed, shuffled))
        worst = {k: max(worst.get(k, 0.0), x) for k, x in out.items()}
    print("LAMB_EMU shuffled=%s error over bound " % shuffled
          + " ".join(f"{k}={worst[k]:.3f}" for k in STAGES))


DEFECTS = {
    "one global ratio": "phi", "ratio from g": "un", "decay left out of u": "u",
    "biases adapted": "p", "t from the call": "u", "ratio applied twice": "p",
    "zero norm gives 0": "phi", "last element dropped": "wn",
}


@pytest.mark.parametrize("defect", list(DEFECTS))
def test_planted_defect_fails_its_stage(defect):
    """Each planted defect leaves its own stage's bound by a wide margin; the clean emulation
    of the same case passes every stage."""
    p, g, m, v = _case(N_EMU, 21)
    ranges = list(RANGES_EMU)
    g[0:193] *= 30.0                     # (the ranges' ratios differ by far more than a bound)
    p[192] = 40.0                        # the mid-vector last element of range 0 carries weight
    if defect == "zero norm gives 0":
        p[1024 + 64:1024 + 64 + 5] = 0.0
    t, call = 4, 6
    args = (t, LR, BETAS, EPS, WD, ranges)
    clean = emulate_lamb(p, g, m, v, *args)
    check_lamb_step(p, g, m, v, *clean, *args, 1.0, "clean")
    bad = emulate_lamb(p, g, m, v, *args, defect=defect, call=call)
    out = check_lamb_step(p, g, m, v, *bad, *args, 1.0, defect, must_pass=False)
    print(f"LAMB_DEFECT {defect!r}: " + " ".join(f"{k}={out[k]:.3g}" for k in STAGES))
    assert out[DEFECTS[defect]] > 10.0, out


# ------------------------------------------------------------------ 4: the CPU optimizer
def test_cpu_optimizer_matches_lamb_ref():
    """train/optim.Lamb (fp32 torch ops, the sums in double) against lamb_ref within the bounds
    over two steps, each from the state it started from; lamb_stats() holds the fp32 norms and
    the ratio that follows from them."""
    n, ranges = 301, [(0, 101), (128, 203)]
    p, g, _, _ = _case(n, 31)
    opt = Lamb(LR, 0.0, BETAS[0], BETAS[1], EPS, WD, n, ranges)
    assert opt.lamb_stats() == [(0.0, 0.0, 1.0)] * 2
    worst = {}
    for t in (1, 2):
        g = torch.randn(n, generator=torch.Generator().manual_seed(t)) * (2.0 if t == 1 else 0.3)
        p0, m0, v0 = p.clone(), opt.m.clone(), opt.v.clone()
        opt.step(p, g.clone())
        assert opt.t == t
        ref = lamb_ref(p0, g, m0, v0, t, LR, BETAS, EPS, WD, ranges)
        # (the optimizer keeps no u: the stage is checked with the reference's own)
        out = check_lamb_step(p0, g, m0, v0, p, opt.m, opt.v, ref[3], opt.lamb_stats(), t, LR,
                              BETAS, EPS, WD, ranges, 1.0, ("cpu", t))
        worst = {k: max(worst.get(k, 0.0), x) for k, x in out.items()}
    print("LAMB_CPU_ERR error over bound " + " ".join(f"{k}={worst[k]:.3f}" for k in STAGES))
    sd = opt.state_dict()
    assert sd["kind"] == "lamb" and set(sd) == {"kind", "rate", "rate_decay", "adam_m", "adam_v",
                                                "adam_t"}
    assert type(sd["adam_t"]) is int and sd["adam_t"] == 2


def test_cpu_optimizer_edge_ratios_and_rate_decay():
    """A range of zero parameters, a range with zero update and a range whose squares overflow
    fp32 all take phi = 1, and the outputs stay finite; the rate decays as after every other
    optimizer."""
    n, ranges = 256, [(0, 5), (64, 70), (128, 131)]
    p = torch.ones(n)
    p[0:5] = 0.0
    p[128:131] = 3e19                    # squares ~ 9e38 > FLT_MAX
    g = torch.ones(n)
    g[64:70] = 0.0
    opt = Lamb(0.5, 1e-2, 0.9, 0.999, 1e-8, 0.0, n, ranges)
    opt.step(p, g)
    st = opt.lamb_stats()
    assert st[0][0] == 0.0 and st[0][2] == 1.0
    assert st[1][1] == 0.0 and st[1][2] == 1.0
    assert st[2][0] == math.inf and st[2][2] == 1.0
    assert torch.isfinite(p).all() and opt.rate == 0.5 * (1 - 1e-2)


# ------------------------------------------------------------ 5: applied steps, not steps
def _exp_cfg(tmp_path, **kw):
    base = dict(numLayers=3, channelSize=16, batchSize=4, validationSize=4,
                validation_interval=1000, log_interval=1000, useCuda=False, synthetic=True,
                checkpoint_dir=str(tmp_path), seed=3, loader_threads=2, prefetch=2,
                rate=1e-2, rateDecay=1e-2, optimizer="lamb", weight_decay=1e-2,
                nan_policy="skip")
    base.update(kw)
    return ExperimentConfig(**base)


def test_skip_pattern_counts_applied_steps(tmp_path):
    """apply, skip, apply, apply, skip, apply on the CPU backend: each applied step equals
    lamb_ref with t = 1, 2, 3, 4 and the rate of its call; a skipped one keeps p, m, v, t and the
    statistics; t ends at 4."""
    from deep_go_amd.train.backends import CPUBackend
    cfg = _exp_cfg(tmp_path)
    be = CPUBackend(cfg, 4)
    n, ranges = be.layout.numel, be.layout.weight_ranges()
    gen = torch.Generator().manual_seed(8)
    t = 0
    for call, apply in enumerate(APPLY, 1):
        g = torch.randn(n, generator=gen) * 0.1 * call
        be.params.grad = g.clone()
        be._loss_sum = 1.0 if apply else float("nan")
        p0, m0, v0 = be.flat_params().clone(), be.opt.m.clone(), be.opt.v.clone()
        s0, lr0 = be.lamb_stats(), be.rate
        assert lr0 == pytest.approx(cfg.rate * (1.0 - cfg.rateDecay) ** (call - 1), rel=1e-13)
        be.optimizer_step()
        if not apply:
            assert be.opt.t == t and be.lamb_stats() == s0
            for x, y in ((be.flat_params(), p0), (be.opt.m, m0), (be.opt.v, v0)):
                assert torch.equal(x.view(torch.int32), y.view(torch.int32))
            continue
        t += 1
        assert be.opt.t == t
        ref = lamb_ref(p0, g, m0, v0, t, lr0, BETAS, EPS, cfg.weight_decay, ranges)
        check_lamb_step(p0, g, m0, v0, be.flat_params(), be.opt.m, be.opt.v, ref[3],
                        be.lamb_stats(), t, lr0, BETAS, EPS, cfg.weight_decay, ranges, 1.0,
                        ("applied", call))
    assert be.opt.t == 4 and be.bad_steps() == 2


# ------------------------------------------------------------------ 6: the CPU backend
def test_cpu_backend_resume_is_exact_and_adamw_moments_move(tmp_path):
    """With the second step skipped: 4 steps == 2 steps + save + load + 2 steps bit for bit, t
    included; --reset-optimizer starts from zero; a checkpoint moves adamw -> lamb with its
    moments and count, and one of another optimizer loads zeros and t = 0.  The trainer's
    kind="lamb" record is written on logging iterations."""
    from deep_go_amd.train.experiment import Experiment
    from deep_go_amd.utils.checkpoint import load_checkpoint
    from deep_go_amd.utils.metrics import read_jsonl
    cfg = _exp_cfg(tmp_path, log_interval=2)
    mpath = str(tmp_path / "metrics.jsonl")
    a = Experiment(cfg, id="a")
    a.init()
    _skip_call(a, 2)
    a.run(2)
    assert (a.backend.opt.t, a.iterations, a.backend.bad_steps()) == (1, 2, 1)
    path = a.save()
    saved = load_checkpoint(path)[3]
    assert saved["kind"] == "lamb" and type(saved["adam_t"]) is int and saved["adam_t"] == 1
    a2 = Experiment.load(path)
    a2.id = "a2"
    a2.run(2)
    b = Experiment(cfg.replace(metrics_path=mpath), id="b")
    b.init()
    _skip_call(b, 2)
    b.run(4)
    assert torch.equal(a2.backend.flat_params(), b.backend.flat_params())
    assert torch.equal(a2.backend.opt.m, b.backend.opt.m)
    assert torch.equal(a2.backend.opt.v, b.backend.opt.v)
    assert a2.backend.opt.t == b.backend.opt.t == 3 and a2.backend.rate == b.backend.rate
    b.metrics.close()
    lamb = [r for r in read_jsonl(mpath) if r.get("kind") == "lamb"]
    assert [r["step"] for r in lamb] == [2, 4]
    assert set(lamb[0]) == {"kind", "step", "phi", "phi_min", "phi_max", "time"}
    assert len(lamb[0]["phi"]) == 3 and lamb[0]["phi_min"] == min(lamb[0]["phi"])
    assert lamb[0]["phi_max"] == max(lamb[0]["phi"])
    assert lamb[1]["phi"] == [s[2] for s in b.backend.lamb_stats()]
    r = Experiment.load(path, reset_optimizer=True)
    r.init()
    assert r.backend.rate == cfg.rate and r.backend.opt.t == 0 and not r.backend.opt.m.any()
    # adamw -> lamb keeps the moments
    w = Experiment(_exp_cfg(tmp_path, optimizer="adamw"), id="w")
    w.run(2)
    c = Experiment.load(w.save(), optimizer="lamb")
    c.init()
    assert isinstance(c.backend.opt, Lamb) and c.backend.opt.t == 2
    assert torch.equal(c.backend.opt.m, w.backend.opt.m) and c.backend.opt.m.any()
    assert torch.equal(c.backend.opt.v, w.backend.opt.v)
    mo = Experiment(_exp_cfg(tmp_path, optimizer="momentum"), id="mo")
    mo.run(2)
    d = Experiment.load(mo.save(), optimizer="lamb")
    d.init()
    assert d.backend.opt.t == 0 and not d.backend.opt.m.any() and not d.backend.opt.v.any()


# ------------------------------------------------------------------ 7: the launcher
def _lamb():
    from deep_go_amd.ops import native
    try:
        return native.lamb()
    except Exception as e:                                   # noqa: BLE001
        pytest.skip(f"_dglamb is not built: {e}")


# fake, suitably aligned, non-null addresses: every call below is refused before any launch
_P, _G, _M, _V, _U, _LR, _REC, _PART, _TAB = (0x1000, 0x2000, 0x3000, 0x4000, 0x5000, 0x6008,
                                              0x7008, 0x8008, 0x9004)


def _call(fn, p=_P, g=_G, m=_M, v=_V, u=_U, n=1000, lr=_LR, rec=_REC, part=_PART, part_n=None,
          tab=_TAB, b1=0.9, b2=0.999, eps=1e-8, wd=1e-2, table=None):
    t = _table(table or [])
    if part_n is None:
        part_n = (-(-(n // 4) // MT) + 1) * SLOTS * 2
    fn(p, g, m, v, u, n, lr, rec, part, part_n, tab, b1, b2, eps, wd,
       t.ctypes.data if len(t) else 0, len(t), 1.0, 0, 0)


@pytest.mark.parametrize("name", ["lamb", "lamb_bf16"])
def test_launcher_refuses_invalid_arguments_without_a_gpu(name):
    """Every refusal happens before any GPU work (no GPU here, and the addresses are fake).
    The module's public names are the three; _dgopt's and _dgadam's are still on offer."""
    from deep_go_amd.ops import native
    mod = _lamb()
    fn = getattr(mod, name)
    assert sorted(x for x in dir(mod) if not x.startswith("_")) == [
        "lamb", "lamb_bf16", "lamb_partials"]
    assert {"momentum", "momentum_bf16"} <= set(dir(native.opt()))
    assert {"adamw", "adamw_bf16", "adamw_tick"} <= set(dir(native.adam()))
    bad = {what: dict(table=rows) for what, rows in BAD_RANGES.items()}
    bad.update({
        "null p": dict(p=0), "null m": dict(m=0), "null v": dict(v=0), "null lr": dict(lr=0),
        "null record": dict(rec=0), "null gradient": dict(g=0), "null u": dict(u=0),
        "null partials": dict(part=0), "null table": dict(tab=0),
        "beta1 = 1": dict(b1=1.0), "beta1 nan": dict(b1=math.nan), "beta2 < 0": dict(b2=-1e-3),
        "eps = 0": dict(eps=0.0), "eps nan": dict(eps=math.nan),
        "record off 8 bytes": dict(rec=_REC + 4),
        "p off 16 bytes": dict(p=_P + 4), "m off 16 bytes": dict(m=_M + 8),
        "v off 16 bytes": dict(v=_V + 4), "u off 16 bytes": dict(u=_U + 8),
        "partials off 8 bytes": dict(part=_PART + 4), "table off 4 bytes": dict(tab=_TAB + 2),
        "gradient misaligned": dict(g=_G + (4 if name == "lamb" else 2)),
        "partials too small": dict(part_n=(1 + 1) * SLOTS * 2 - 1),
        "five ranges in one chunk": dict(table=[(64 * i, 64 * i + 8) for i in range(5)]),
    })
    for what, kw in bad.items():
        with pytest.raises(RuntimeError) as e:
            _call(fn, **kw)
        assert str(e.value) == f"{name}: invalid argument", what
    # n = 0 with a valid (empty) table: nothing to do, no launch
    fn(0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0.9, 0.999, 1e-8, 0.0, 0, 0, 1.0, 0, 0)
    with pytest.raises(RuntimeError) as e:     # (the ranges and betas are checked even then)
        fn(0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1.0, 0.999, 1e-8, 0.0, 0, 0, 1.0, 0, 0)
    assert str(e.value) == f"{name}: invalid argument"


def test_partials_size_query():
    """(chunks + 1) x SLOTS pairs; an invalid table or more than SLOTS ranges in a chunk is
    refused; four in one chunk are not."""
    q = _lamb().lamb_partials
    assert q(0, 0, 0) == SLOTS * 2 and q(3, 0, 0) == SLOTS * 2
    assert q(4, 0, 0) == 2 * SLOTS * 2 and q(1024, 0, 0) == 2 * SLOTS * 2
    assert q(1025, 0, 0) == 2 * SLOTS * 2 and q(1028, 0, 0) == 3 * SLOTS * 2
    four = _table([(64 * i, 64 * i + 8) for i in range(4)])
    assert q(4099, four.ctypes.data, 4) == 5 * SLOTS * 2
    # a range reaching in from the chunk before counts
    five = _table([(960, 1030)] + [(1088 + 64 * i, 1088 + 64 * i + 8) for i in range(4)])
    for t in (five, _table(BAD_RANGES["unsorted"])):
        with pytest.raises(RuntimeError) as e:
            q(4099, t.ctypes.data, len(t))
        assert str(e.value) == "lamb_partials: invalid argument"


# ------------------------------------------------------------------ 8: two ranks
def _dp_worker(rank, world, port, out_dir):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank),
                      WORLD_SIZE=str(world), LOCAL_RANK=str(rank))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from deep_go_amd.data.synthetic import random_planes
    from deep_go_amd.train.backends import CPUBackend
    cfg = ExperimentConfig(numLayers=3, channelSize=16, rate=1e-2, seed=5, bucket_mb=0.01,
                           optimizer="lamb", weight_decay=1e-2)
    B = 8
    be = CPUBackend(cfg, B // world, world=world, bucket_mb=0.01)
    for step in range(3):
        planes, player, rank_, labels = random_planes(B, seed=step)
        sl = slice(rank * (B // world), (rank + 1) * (B // world))
        be.set_batch(planes[sl], player[sl], rank_[sl], labels[sl])
        be.forward_backward()
        be.optimizer_step()
    torch.save({"params": be.flat_params().clone(), "m": be.opt.m, "v": be.opt.v,
                "t": be.opt.t, "stats": be.lamb_stats()}, os.path.join(out_dir, f"rank{rank}.pt"))
    dist.barrier()
    dist.destroy_process_group()


def test_two_gloo_ranks_keep_identical_parameters_and_ratios(tmp_path):
    """Every rank derives the same ratios from the same all-reduced gradient: no collective is
    added, and after three steps the parameters, both moments, t and the ratios are identical."""
    mp.spawn(_dp_worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True)
    a = torch.load(str(tmp_path / "rank0.pt"), weights_only=True)
    b = torch.load(str(tmp_path / "rank1.pt"), weights_only=True)
    assert a["t"] == b["t"] == 3 and a["stats"] == b["stats"] and len(a["stats"]) == 3
    for k in ("params", "m", "v"):
        assert torch.equal(a[k], b[k]), k
    assert all(s[2] != 1.0 for s in a["stats"])
