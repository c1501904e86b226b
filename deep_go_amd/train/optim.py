"""Optimizers over the flat parameter vector (CPU path; the GPU path runs the same math in
``sgd_kernel`` / ``rmsprop_kernel``, csrc/kernels/elementwise.hip, and ``momentum_kernel`` /
``adamw_kernel`` / ``lamb_moments``, ``lamb_ratio``, ``lamb_apply``, csrc/kernels/optim.hip).

* ``SGD`` (optimizer.lua:16-27): theta -= rate * g, then rate *= (1 - decay) — so after t
  steps rate_t = rate_0 * (1 - decay)^t.  The rate is a Python float (double), as in Lua.
* ``RMSProp`` — the reference's misnamed ``AdagradOptimizer`` (optimizer.lua:1-14):
  ms = decay*ms + (1-decay)*g^2, theta -= rate * g / sqrt(ms), ms initialised to 1.  The
  reference version crashes (undefined global ``grads``); this one works and is opt-in.
* ``Momentum`` (an addition): SGD with momentum, optional Nesterov step and weight decay on
  the conv weights only.  With gw = g + weight_decay * theta on the decayed elements and
  gw = g elsewhere: v = momentum * v + gw (v starts at 0); theta -= rate * (gw + momentum * v
  if nesterov else v); then rate *= (1 - decay) as SGD.  This is torch.optim.SGD(momentum,
  dampening=0, nesterov, weight_decay) with the rate outside the velocity.
* ``AdamW`` (an addition): Adam with decoupled weight decay on the conv weights only.  With the
  moments m, v (0 at the start) and t, the count of APPLIED steps (0 at the start): t += 1;
  c1 = 1 / (1 - beta1^t), c2 = 1 / sqrt(1 - beta2^t) (in double, then fp32); m = beta1 m +
  (1 - beta1) g; v = beta2 v + (1 - beta2) g^2; theta *= 1 - rate * weight_decay on the decayed
  elements; theta -= (rate c1) m / (sqrt(v) c2 + eps); then rate *= (1 - decay) as SGD.  This is
  torch.optim.AdamW(betas, eps, weight_decay, amsgrad=False); with weight_decay = 0 it is Adam.
  A skipped step (a non-finite loss or gradient) is no call of ``step``: m, v and t stay, only
  the rate decays, so t falls behind the trainer's iteration count.  beta1, beta2, eps are
  taken as their fp32 values, as the kernel receives them.
* ``Lamb`` (an addition): Adam's update rescaled per conv-weight tensor by a trust ratio.  The
  adapted tensors are the ranges R_k of ``ParamLayout.weight_ranges()``; the biases and the
  padding take ratio 1 and no decay (apex's default for tensors without weight decay).  t, c1,
  c2, m, v as ``AdamW``; r = (c1 m) / (sqrt(v) c2 + eps); u = r + weight_decay theta inside a
  range, r elsewhere; per range SP = sum theta^2, SU = sum u^2 (accumulated in double from the
  fp32 values, each rounded to fp32), wn = fp32(sqrt(SP)), un = fp32(sqrt(SU)), phi =
  fp32(double(wn) / double(un)) if both are finite and > 0, else 1 (no clamp; an overflowing
  sum is inf and gives 1); theta -= (rate phi) u; then rate *= (1 - decay).  A skipped step is
  no call of ``step``, as for ``AdamW``.  The state is Adam's and is saved under the same keys
  (``adam_m``, ``adam_v``, ``adam_t``): a checkpoint moves between ``adamw`` and ``lamb`` with
  its moments.

``clip_grad_`` (an addition; ``grad_clip`` > 0) runs before any of them, once per applied step:
norm = |gscale| * sqrt(sum g^2), scale = min(1, c / (norm + 1e-6)), g *= scale, which is
``torch.nn.utils.clip_grad_norm_(params, c)`` applied to g * gscale (the GPU path:
csrc/kernels/clip.hip).

``WeightEMA`` (an addition; ``ema_decay`` > 0) runs after them, once per applied step, and is
read by nothing in training: with the average e (the parameters at the start) and t, the count
of applied averaging steps (0 at the start): t += 1; d = min(ema_decay, (1 + t) / (10 + t)) in
double (the ramp is the usual warm-up: a short run is not dominated by the initialisation);
omd = fp32(1 - d); e = fmaf(omd, theta - e, e) in fp32, theta as the update left it.  The lerp
form makes e == theta a fixed point and keeps the result between e and theta.  A skipped step is
no call of ``step`` (the GPU path: csrc/kernels/ema.hip).

``LRSchedule`` (an addition; ``lr_schedule`` != none) owns the rate: the optimizers' own decay
of it is overwritten after every step, applied or skipped, with base * factor(s), where base
takes that decay in their place (the GPU path: csrc/kernels/sched.hip).
"""
from __future__ import annotations

import math

import numpy as np
import torch

from ..config import LR_KINDS


@torch.no_grad()
def clip_grad_(grads: torch.Tensor, max_norm: float, gscale: float = 1.0):
    """Scale the flat fp32 gradient in place so that |gscale| * ||grads||_2 <= max_norm;
    returns (norm, scale) as the fp32 values the GPU record holds.  The sum of squares is
    accumulated in float64 from the fp32 gradient; the norm is rounded to fp32, r = max_norm /
    (norm + 1e-6) is formed in double from that fp32 norm (max_norm and gscale as their fp32
    values, as the kernel receives them), and scale = fp32(r) if r < 1 else 1 is applied in
    fp32.  An infinite norm gives scale 0, a NaN norm scale 1, as torch does."""
    c, s = float(np.float32(max_norm)), abs(float(np.float32(gscale)))
    g64 = grads.double()
    # (the float64 sum does not overflow where the kernel's fp32 partials do; the norm's own
    # rounding to fp32 may)
    with np.errstate(over="ignore"):
        norm = float(np.float32(s * float(torch.dot(g64, g64)) ** 0.5))
    r = c / (norm + 1e-6)
    scale = float(np.float32(r)) if r < 1.0 else 1.0
    if scale != 1.0:
        grads.mul_(scale)
    return norm, scale


class SGD:
    def __init__(self, rate: float, rate_decay: float):
        self.rate = float(rate)
        self.rate_decay = float(rate_decay)

    @torch.no_grad()
    def step(self, params: torch.Tensor, grads: torch.Tensor):
        params.add_(grads, alpha=-self.rate)
        self.rate = self.rate * (1.0 - self.rate_decay)

    def state_dict(self):
        return {"kind": "sgd", "rate": self.rate, "rate_decay": self.rate_decay}

    def load_state_dict(self, d):
        self.rate = float(d["rate"])
        self.rate_decay = float(d["rate_decay"])


class RMSProp:
    def __init__(self, rate: float, decay: float, numel: int):
        self.rate = float(rate)
        self.decay = float(decay)
        self.ms = torch.ones(numel, dtype=torch.float32)

    @torch.no_grad()
    def step(self, params: torch.Tensor, grads: torch.Tensor):
        self.ms.mul_(self.decay).addcmul_(grads, grads, value=1.0 - self.decay)
        params.addcdiv_(grads, self.ms.sqrt(), value=-self.rate)

    def state_dict(self):
        return {"kind": "rmsprop", "rate": self.rate, "decay": self.decay, "ms": self.ms}

    def load_state_dict(self, d):
        self.rate = float(d["rate"])
        self.decay = float(d["decay"])
        self.ms = d["ms"].float().clone()


class Momentum:
    def __init__(self, rate: float, rate_decay: float, momentum: float, nesterov: bool,
                 weight_decay: float, numel: int, decay_ranges=()):
        self.rate = float(rate)
        self.rate_decay = float(rate_decay)
        self.momentum = float(momentum)
        self.nesterov = bool(nesterov)
        self.vel = torch.zeros(numel, dtype=torch.float32)
        # weight_decay on the elements of decay_ranges ([begin, end) pairs), 0 elsewhere
        self.wd = torch.zeros(numel, dtype=torch.float32)
        for b, e in decay_ranges:
            self.wd[b:e] = float(weight_decay)

    @torch.no_grad()
    def step(self, params: torch.Tensor, grads: torch.Tensor):
        gw = grads + self.wd * params
        self.vel.mul_(self.momentum).add_(gw)
        u = gw.add_(self.vel, alpha=self.momentum) if self.nesterov else self.vel
        params.add_(u, alpha=-self.rate)
        self.rate = self.rate * (1.0 - self.rate_decay)

    def state_dict(self):
        return {"kind": "momentum", "rate": self.rate, "rate_decay": self.rate_decay,
                "vel": self.vel}

    def load_state_dict(self, d):
        self.rate = float(d["rate"])
        self.rate_decay = float(d["rate_decay"])
        # (a checkpoint of another optimizer has no velocity: start from rest)
        self.vel = d["vel"].float().clone() if "vel" in d else torch.zeros_like(self.vel)


class AdamW:
    def __init__(self, rate: float, rate_decay: float, beta1: float, beta2: float, eps: float,
                 weight_decay: float, numel: int, decay_ranges=()):
        self.rate = float(rate)
        self.rate_decay = float(rate_decay)
        f32 = lambda x: torch.tensor(float(x), dtype=torch.float32).item()
        self.beta1, self.beta2, self.eps = f32(beta1), f32(beta2), f32(eps)
        self.m = torch.zeros(numel, dtype=torch.float32)
        self.v = torch.zeros(numel, dtype=torch.float32)
        self.t = 0                     # applied steps: what the bias corrections count
        # weight_decay on the elements of decay_ranges ([begin, end) pairs), 0 elsewhere
        self.wd = torch.zeros(numel, dtype=torch.float32)
        for b, e in decay_ranges:
            self.wd[b:e] = float(weight_decay)

    @torch.no_grad()
    def step(self, params: torch.Tensor, grads: torch.Tensor):
        self.t += 1
        f32 = lambda x: torch.tensor(x, dtype=torch.float32)
        c1 = f32(1.0 / (1.0 - self.beta1 ** self.t))
        c2 = f32(1.0 / (1.0 - self.beta2 ** self.t) ** 0.5)
        rate = f32(self.rate)
        # (1 - beta is exact in fp32 arithmetic and in double alike)
        self.m.mul_(self.beta1).add_(grads, alpha=1.0 - self.beta1)
        self.v.mul_(self.beta2).add_((grads * (1.0 - self.beta2)).mul_(grads))
        params.mul_(1.0 - rate * self.wd)
        params.sub_((self.m * (rate * c1)).div_(self.v.sqrt().mul_(c2).add_(self.eps)))
        self.rate = self.rate * (1.0 - self.rate_decay)

    def state_dict(self):
        return {"kind": "adamw", "rate": self.rate, "rate_decay": self.rate_decay,
                "adam_m": self.m, "adam_v": self.v, "adam_t": int(self.t)}

    def load_state_dict(self, d):
        self.rate = float(d["rate"])
        self.rate_decay = float(d["rate_decay"])
        # (a checkpoint of another optimizer has no moments: start from zero, t = 0)
        has = "adam_m" in d and "adam_v" in d
        self.m = d["adam_m"].float().clone() if has else torch.zeros_like(self.m)
        self.v = d["adam_v"].float().clone() if has else torch.zeros_like(self.v)
        self.t = int(d.get("adam_t", 0)) if has else 0


def trust_ratio(sp: float, su: float):
    """(wn, un, phi) as fp32 values from the two sums of squares (doubles): each sum rounded to
    fp32 (above its range: inf), its root rounded to fp32, phi = fp32(double(wn) / double(un))
    if both norms are finite and > 0, else 1."""
    with np.errstate(over="ignore", invalid="ignore"):
        wn = np.float32(np.sqrt(np.float64(np.float32(sp))))
        un = np.float32(np.sqrt(np.float64(np.float32(su))))
        ok = np.isfinite(wn) and np.isfinite(un) and wn > 0 and un > 0
        phi = np.float32(np.float64(wn) / np.float64(un)) if ok else np.float32(1.0)
    return float(wn), float(un), float(phi)


class Lamb:
    def __init__(self, rate: float, rate_decay: float, beta1: float, beta2: float, eps: float,
                 weight_decay: float, numel: int, ranges=()):
        self.rate = float(rate)
        self.rate_decay = float(rate_decay)
        f32 = lambda x: torch.tensor(float(x), dtype=torch.float32).item()
        self.beta1, self.beta2, self.eps = f32(beta1), f32(beta2), f32(eps)
        self.m = torch.zeros(numel, dtype=torch.float32)
        self.v = torch.zeros(numel, dtype=torch.float32)
        self.t = 0                     # applied steps: what the bias corrections count
        # the adapted tensors ([begin, end) pairs): weight_decay inside them, 0 elsewhere
        self.ranges = [(int(b), int(e)) for b, e in ranges]
        self.wd = torch.zeros(numel, dtype=torch.float32)
        for b, e in self.ranges:
            self.wd[b:e] = float(weight_decay)
        self._stats = [(0.0, 0.0, 1.0)] * len(self.ranges)

    @torch.no_grad()
    def step(self, params: torch.Tensor, grads: torch.Tensor):
        self.t += 1
        f32 = lambda x: torch.tensor(x, dtype=torch.float32)
        c1 = f32(1.0 / (1.0 - self.beta1 ** self.t))
        c2 = f32(1.0 / (1.0 - self.beta2 ** self.t) ** 0.5)
        self.m.mul_(self.beta1).add_(grads, alpha=1.0 - self.beta1)
        self.v.mul_(self.beta2).add_((grads * (1.0 - self.beta2)).mul_(grads))
        u = (self.m * c1).div_(self.v.sqrt().mul_(c2).add_(self.eps)).add_(self.wd * params)
        phi = torch.ones_like(u)
        self._stats = []
        for b, e in self.ranges:
            pd, ud = params[b:e].double(), u[b:e].double()
            st = trust_ratio(float((pd * pd).sum()), float((ud * ud).sum()))
            self._stats.append(st)
            phi[b:e] = st[2]
        params.sub_(u.mul_(phi.mul_(f32(self.rate))))
        self.rate = self.rate * (1.0 - self.rate_decay)

    def lamb_stats(self):
        """Per adapted tensor (wn, un, phi) of the last applied step."""
        return list(self._stats)

    def state_dict(self):
        # (Adam's state under Adam's keys: a checkpoint moves between adamw and lamb)
        return {"kind": "lamb", "rate": self.rate, "rate_decay": self.rate_decay,
                "adam_m": self.m, "adam_v": self.v, "adam_t": int(self.t)}

    def load_state_dict(self, d):
        self.rate = float(d["rate"])
        self.rate_decay = float(d["rate_decay"])
        # (a checkpoint of another optimizer has no moments: start from zero, t = 0)
        has = "adam_m" in d and "adam_v" in d
        self.m = d["adam_m"].float().clone() if has else torch.zeros_like(self.m)
        self.v = d["adam_v"].float().clone() if has else torch.zeros_like(self.v)
        self.t = int(d.get("adam_t", 0)) if has else 0


def ema_omd(decay: float, t: int) -> float:
    """1 - min(decay, (1 + t) / (10 + t)) as the fp32 value averaging step t uses (t counts from
    1; every operation in double, then one rounding)."""
    td = float(t)
    return float(np.float32(1.0 - min(float(decay), (1.0 + td) / (10.0 + td))))


def fma32(a, b: np.ndarray, c: np.ndarray) -> np.ndarray:
    """fmaf(a, b, c) on fp32 arrays with its single rounding.  The product of two fp32 values is
    exact in double; the sum is brought to round-to-odd in double (TwoSum tells whether it was
    exact and on which side the rest lies), and rounding that to fp32 is then the rounding of
    the exact value (53 >= 2 * 24 + 2 bits)."""
    a64 = np.asarray(a, dtype=np.float32).astype(np.float64)
    prod = a64 * b.astype(np.float64)
    c64 = c.astype(np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        s = prod + c64
        bb = s - prod
        err = (prod - (s - bb)) + (c64 - bb)
        fix = np.isfinite(s) & (err != 0.0) & ((s.view(np.int64) & 1) == 0)
        toward = np.where(err > 0.0, np.inf, -np.inf)
        s = np.where(fix, np.nextafter(s, toward), s)
        return s.astype(np.float32)


class WeightEMA:
    def __init__(self, decay: float, params: torch.Tensor):
        self.decay = float(decay)
        self.reset(params)

    @torch.no_grad()
    def reset(self, params: torch.Tensor):
        """e = the parameters, no averaging step applied."""
        self.ema = params.detach().float().clone()
        self.t = 0

    @torch.no_grad()
    def step(self, params: torch.Tensor):
        self.t += 1
        omd = np.float32(ema_omd(self.decay, self.t))
        e = self.ema.numpy()
        diff = params.detach().numpy() - e            # (one fp32 rounding)
        e[...] = fma32(omd, diff, e)

    def state_dict(self):
        return {"ema": self.ema, "ema_t": int(self.t)}

    def load_state_dict(self, d, params: torch.Tensor):
        """(a checkpoint without an average: start from the parameters, t = 0)"""
        if "ema" in d:
            self.ema = d["ema"].float().clone()
            self.t = int(d.get("ema_t", 0))
        else:
            self.reset(params)


def lr_factor(kind: str, s: int, W: int, T: int, m: float, E: int, g: float) -> float:
    """w(s) * d(s) of step s (counted from 0), every operation in double:
    w = min(1, (s + 1) / W) for W > 0, else 1; u = clamp((s - W) / (T - W), 0, 1);
    d = 1 (constant) | 1 - (1 - m) u (linear) | m + (1 - m) 0.5 (1 + cos(pi u)) (cosine), and
    exactly m for s >= T for both | max(m, g ** floor(max(s - W, 0) / E)) (step)."""
    s, m, g = int(s), float(m), float(g)
    w = min(1.0, (s + 1.0) / float(W)) if W > 0 else 1.0
    if kind == "constant":
        d = 1.0
    elif kind in ("linear", "cosine"):
        if s >= T:
            d = m                      # (past the horizon the factor stays at the floor)
        else:
            u = min(max(float(s - W) / float(T - W), 0.0), 1.0)
            if kind == "linear":
                d = 1.0 - (1.0 - m) * u
            else:
                d = m + (1.0 - m) * (0.5 * (1.0 + math.cos(math.pi * u)))
    elif kind == "step":
        d = max(m, g ** float(max(s - W, 0) // E))
    else:
        raise ValueError(f"lr_schedule {kind!r}")
    return w * d


class LRSchedule:
    """``lr_schedule`` != none: base (cfg.rate at the start; it carries the rateDecay) and s (the
    steps taken so far, skipped ones included).  The rate step s uses is base * factor(s)."""

    def __init__(self, cfg, rate_decay: float = None):
        self.kind = cfg.lr_schedule
        if self.kind not in LR_KINDS:
            raise ValueError(f"lr_schedule {self.kind!r}")
        self.W, self.T, self.E = int(cfg.lr_warmup), int(cfg.lr_total), int(cfg.lr_step_every)
        self.m, self.g = float(cfg.lr_min), float(cfg.lr_gamma)
        self.rate0 = float(cfg.rate)
        self.rate_decay = float(cfg.rateDecay if rate_decay is None else rate_decay)
        self.reset()

    def reset(self):
        self.base, self.s = self.rate0, 0

    def factor(self, s: int) -> float:
        return lr_factor(self.kind, s, self.W, self.T, self.m, self.E, self.g)

    @property
    def rate(self) -> float:
        """The rate the next step uses."""
        return self.base * self.factor(self.s)

    def step(self):
        """After every step, applied or skipped."""
        self.base = self.base * (1.0 - self.rate_decay)
        self.s += 1

    def state_dict(self):
        return {"rate": self.base, "lr_step": int(self.s)}

    def load_state_dict(self, d):
        """(a checkpoint without lr_step: its rate is the base, no step taken)"""
        self.base = float(d["rate"])
        self.s = int(d.get("lr_step", 0))
