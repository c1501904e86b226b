"""Compute backends behind the Experiment (one per device type).

Both expose the same small surface used by the training loop:
  set_batch(planes uint8 [B,9,19,19], player, rank, labels)   (host numpy or tensors)
  forward_backward()         loss/argmax of the batch + gradients (global-batch mean)
  optimizer_step()           SGD/RMSProp/Momentum/AdamW/LAMB + per-step LR decay
  evaluate(n)                forward only on the first n boards of the current batch
  loss_sum() / correct()     of the last forward (host floats; synchronising)
  clip_stats()               grad_clip > 0: (grad_norm, clip_scale, clipped_steps) of the last
                             applied step and of the run (synchronising)
  lamb_stats()               optimizer=lamb: per conv-weight tensor (||w||, ||update||, trust
                             ratio) of the last applied step (synchronising)
  ema_params() / ema_steps() ema_decay > 0: the moving average of the weights (on the host) and
                             the count of averaging steps applied
  ema_weights()              ema_decay > 0: a context manager inside which evaluate() runs on
                             the average; no training step may run inside it
  reset_ema()                ema_decay > 0: average = parameters, no step applied
  rate                       the rate the next step will use (with an lr_schedule: the scheduled
                             one)
  base_rate / lr_step        lr_schedule != none: the rate that rateDecay decays, which the
                             schedule's factor multiplies, and the steps taken so far, skipped
                             ones included (without a schedule: rate and 0)
  params / state_dict / load_state_dict

``load_next(loader)`` feeds the next training batch; with ``cfg.augment == "d4"`` it moves every
board by the symmetry ``data/symmetry.py augment_symmetries(cfg.seed, seq, board0 + i)`` draws
for it (``seq``: the batch's loader sequence number, ``board0``: this rank's first board in the
global batch) — the numpy oracle on the CPU, the in-place kernel of augment.hip on the GPU, the
same bytes either way.  ``set_batch`` (validation, eval, predict) is never augmented.

* ``CPUBackend`` — fp32 PyTorch on the CPU (the reference's useCuda=false path,
  experiments.lua:97; also the numerical oracle).  DP over gloo.
* ``HIPBackend`` — the MI355X executor (models/hip_model.py) with hipGraph replay and, for
  world > 1, RCCL gradient buckets overlapped with backward.
"""
from __future__ import annotations

import contextlib
import os
from typing import Optional

import numpy as np

import torch
import torch.nn.functional as F

from ..config import ExperimentConfig
from ..models.gocnn import ParamLayout, init_params, reference_forward
from ..ops.native import cpu
from ..parallel import dp
from .optim import SGD, AdamW, Lamb, LRSchedule, Momentum, RMSProp, WeightEMA, clip_grad_


def _np(x, dtype):
    if isinstance(x, torch.Tensor):
        return x.detach().cpu().numpy().astype(dtype, copy=False)
    return np.asarray(x, dtype=dtype)


def augment_host_batch(cfg: ExperimentConfig, batch, seq: int, board0: int):
    """A host batch (planes, player, rank, labels) as the net sees it at loader sequence
    number ``seq``: unchanged for ``augment=none``, moved by the numpy oracle for ``d4``."""
    if cfg.augment == "none" or batch is None:
        return batch
    from ..data.symmetry import augment_batch, augment_symmetries
    planes, player, rank, labels = batch
    planes, labels = augment_batch(planes, labels,
                                   augment_symmetries(cfg.seed, seq, board0, len(labels)))
    return planes, player, rank, labels


class CPUBackend:
    def __init__(self, cfg: ExperimentConfig, batch: int, flat: Optional[torch.Tensor] = None,
                 world: int = 1, bucket_mb: float = 4.0, board0: int = 0):
        self.cfg = cfg
        self.board0 = board0
        self.layout = ParamLayout(cfg)
        self.B = batch
        self.world = world
        self.params = (flat.clone().float() if flat is not None
                       else init_params(self.layout, cfg.seed)).contiguous()
        self.params.requires_grad_(True)
        if cfg.optimizer == "rmsprop":
            self.opt = RMSProp(cfg.rate, cfg.rmsprop_decay, self.layout.numel)
        elif cfg.optimizer == "momentum":
            self.opt = Momentum(cfg.rate, cfg.rateDecay, cfg.momentum, cfg.nesterov,
                                cfg.weight_decay, self.layout.numel,
                                self.layout.weight_ranges())
        elif cfg.optimizer == "adamw":
            self.opt = AdamW(cfg.rate, cfg.rateDecay, cfg.adam_beta1, cfg.adam_beta2,
                             cfg.adam_eps, cfg.weight_decay, self.layout.numel,
                             self.layout.weight_ranges())
        elif cfg.optimizer == "lamb":
            self.opt = Lamb(cfg.rate, cfg.rateDecay, cfg.adam_beta1, cfg.adam_beta2,
                            cfg.adam_eps, cfg.weight_decay, self.layout.numel,
                            self.layout.weight_ranges())
        else:
            self.opt = SGD(cfg.rate, cfg.rateDecay)
        # lr_schedule != none: base and s live here; the optimizer's rate is rewritten from them
        # after every step, so its own rate *= never compounds with the factor
        self.sched = None
        if cfg.lr_schedule != "none":
            self.sched = LRSchedule(cfg, getattr(self.opt, "rate_decay", 0.0))
            self.opt.rate = self.sched.rate
        # ema_decay > 0: the moving average of the weights, seeded with them
        self.ema = WeightEMA(cfg.ema_decay, self.params) if cfg.ema_decay > 0 else None
        self._ema_on = False          # inside ema_weights(): evaluate() reads the average
        self._x = None
        self._y = None
        self._loss_sum = 0.0
        self._correct = 0
        self.bucketer = None
        if world > 1:
            ranges = [self.layout.layer_range(i) for i in range(len(self.layout.layers))]
            self.buckets = dp.make_buckets(ranges, int(bucket_mb * 2 ** 20))
        self.nan_skipped = 0
        # grad_clip > 0: the last applied step's norm and scale, the applied steps that clipped
        # (a statistic of the run: not part of a checkpoint)
        self._clip = (0.0, 0.0, 0)
        self._last = "train"
        self._eval = (0.0, 0)

    @property
    def rate(self) -> float:
        return self.opt.rate

    @property
    def base_rate(self) -> float:
        return self.sched.base if self.sched is not None else self.opt.rate

    @property
    def lr_step(self) -> int:
        return self.sched.s if self.sched is not None else 0

    def _sched_step(self):
        """lr_schedule != none, after every step, applied or skipped: base takes the decay, s
        counts, and the rate is rewritten from them."""
        self.sched.step()
        self.opt.rate = self.sched.rate

    def load_next(self, loader):
        seq = loader.consumed          # the sequence number of the batch about to be taken
        batch = augment_host_batch(self.cfg, loader.next_numpy(), seq, self.board0)
        self.set_batch(*batch)
        return batch

    def set_batch(self, planes, player, rank, labels):
        pl = _np(planes, np.uint8).reshape(-1, 9, 19, 19)
        self._x = torch.from_numpy(cpu().expand(pl, _np(player, np.uint8), _np(rank, np.uint8),
                                                 self.cfg.ko_plane))
        self._y = torch.from_numpy(_np(labels, np.int64))

    def _forward(self, x):
        w = self.ema.ema if self._ema_on else self.params
        return reference_forward(self.layout, w, x, head_relu=self.cfg.head_relu)

    def forward_backward(self):
        if self._ema_on:
            raise RuntimeError("forward_backward inside ema_weights()")
        if self.params.grad is not None:
            self.params.grad.zero_()
        logp = self._forward(self._x)
        # mean over the GLOBAL batch: local mean / world, then SUM all-reduce
        loss = F.nll_loss(logp, self._y, reduction="sum") / (self.B * self.world)
        loss.backward()
        with torch.no_grad():
            self._loss_sum = float(F.nll_loss(logp, self._y, reduction="sum"))
            self._correct = int((logp.argmax(1) == self._y).sum())
        self._last = "train"
        if self.world > 1:
            g = self.params.grad
            works = [torch.distributed.all_reduce(g[s:e], async_op=True)
                     for s, e, _ in self.buckets]
            for w in works:
                w.wait()

    def train_step(self):
        """forward_backward + optimizer_step with nothing in between."""
        self.forward_backward()
        self.optimizer_step()

    def optimizer_step(self):
        if self._ema_on:
            raise RuntimeError("optimizer_step inside ema_weights()")
        # skip on non-finite (all-reduced) gradients: every rank sees the same reduced
        # gradient, so all ranks skip together (a rank-local loss check would not)
        if self.cfg.nan_policy != "raise" and not (
                np.isfinite(self._loss_sum) if self.world == 1
                else bool(torch.isfinite(self.params.grad).all())):
            self.nan_skipped += 1
            # (nothing of the optimizer's state moves: AdamW's count of applied steps neither,
            # nor the weight average and its count)
            if self.sched is not None:
                self._sched_step()
            else:
                self.opt.rate = self.opt.rate * (1.0 - getattr(self.opt, "rate_decay", 0.0))
            return
        with torch.no_grad():
            if self.cfg.grad_clip > 0:
                norm, scale = clip_grad_(self.params.grad, self.cfg.grad_clip)
                self._clip = (norm, scale, self._clip[2] + (scale < 1.0))
            self.opt.step(self.params, self.params.grad)
            if self.sched is not None:
                self._sched_step()
            if self.ema is not None:
                self.ema.step(self.params)

    @torch.no_grad()
    def evaluate(self, n: Optional[int] = None):
        x, y = self._x, self._y
        if n is not None:
            x, y = x[:n], y[:n]
        logp = self._forward(x)
        self._eval = (float(F.nll_loss(logp, y, reduction="sum")),
                      int((logp.argmax(1) == y).sum()))
        self._last = "eval"
        return logp

    def loss_sum(self) -> float:
        return self._eval[0] if self._last == "eval" else self._loss_sum

    def correct(self) -> int:
        return self._eval[1] if self._last == "eval" else self._correct

    def bad_steps(self) -> int:
        """Updates skipped for a non-finite loss / gradient so far."""
        return self.nan_skipped

    def gradient_tagged(self) -> bool:
        """(HIP only: the gradient producers' range-check tag; the fp32 oracle has none)"""
        return False

    def clip_stats(self):
        """grad_clip > 0: (grad_norm, clip_scale) of the last applied step and the number of
        applied steps that clipped so far."""
        return self._clip

    def lamb_stats(self):
        """optimizer=lamb: per conv-weight tensor (wn, un, phi) of the last applied step."""
        if not isinstance(self.opt, Lamb):
            raise RuntimeError("no trust ratios: optimizer is not lamb")
        return self.opt.lamb_stats()

    def _need_ema(self):
        if self.ema is None:
            raise RuntimeError("no weight average: ema_decay is 0")

    def ema_params(self) -> torch.Tensor:
        """ema_decay > 0: the moving average of the weights."""
        self._need_ema()
        return self.ema.ema

    def ema_steps(self) -> int:
        """ema_decay > 0: the averaging steps applied so far (skipped ones do not count)."""
        self._need_ema()
        return self.ema.t

    def reset_ema(self):
        """ema_decay > 0: average = the parameters as they stand, no step applied."""
        if self.ema is not None:
            self.ema.reset(self.params)

    @contextlib.contextmanager
    def ema_weights(self):
        """evaluate() on the moving average instead of the weights.  Does not nest; no
        training step may run inside it."""
        self._need_ema()
        if self._ema_on:
            raise RuntimeError("ema_weights() does not nest")
        self._ema_on = True
        try:
            yield self
        finally:
            self._ema_on = False

    def flat_params(self) -> torch.Tensor:
        return self.params.detach()

    def load_params(self, flat: torch.Tensor):
        with torch.no_grad():
            self.params.copy_(flat.float())
        self.reset_ema()

    def state_dict(self):
        d = {"optimizer": self.opt.state_dict()}
        if self.sched is not None:
            # rate holds base (resumed with the schedule off, a run continues from the undamped
            # rate); lr_step is an integer: it travels in the checkpoint's metadata
            d["optimizer"].update(self.sched.state_dict())
        if self.ema is not None:
            # (ema_t is an integer: it travels in the checkpoint's metadata)
            d["optimizer"].update(self.ema.state_dict())
        return d

    def load_state_dict(self, d):
        self.opt.load_state_dict(d["optimizer"])
        if self.sched is not None:
            # (a checkpoint without lr_step: base = its rate, s = 0)
            self.sched.load_state_dict(d["optimizer"])
            self.opt.rate = self.sched.rate
        if self.ema is not None:
            # (a checkpoint without an average: seeded from the parameters, t = 0)
            self.ema.load_state_dict(d["optimizer"], self.params)


class HIPBackend:
    def __init__(self, cfg: ExperimentConfig, batch: int, flat: Optional[torch.Tensor] = None,
                 world: int = 1, device=None, use_graphs: bool = True, bucket_mb: float = 4.0,
                 grad_dtype: str = "fp32", comm: str = "auto", board0: int = 0):
        from ..models.hip_model import HipGoNet, SegmentedStep
        self.cfg = cfg
        self.board0 = board0
        self.B = batch
        self.world = world
        self.device = device or torch.device("cuda", torch.cuda.current_device())
        self.net = HipGoNet(cfg, batch, device=self.device, flat_params=flat,
                            global_batch=batch * world,
                            grad_wire=grad_dtype if world > 1 else "fp32")
        self.layout = self.net.layout
        if world > 1 and flat is None:
            dp.broadcast_(self.net.params, 0)
            self.net.refresh_weights()
            # (the average was seeded with this rank's own initial parameters)
            self.net.reset_ema()
        self.bucketer = None
        self.comm = None
        if world > 1:
            # RCCL needs one GPU per rank: a gloo process group (e.g. several ranks sharing
            # one GPU in tests) keeps torch.distributed collectives
            kind = comm if torch.distributed.get_backend() == "nccl" else "torch"
            self.comm = dp.make_communicator(kind, self.device)
            ranges = [self.layout.layer_range(i) for i in range(len(self.layout.layers))]
            self.bucketer = dp.GradBucketer(self.net.grads,
                                            dp.make_buckets(ranges, int(bucket_mb * 2 ** 20),
                                                            groups=self.net.wgroups),
                                            grad_dtype=grad_dtype, comm=self.comm,
                                            shadow=self.net.grads16)
        # the loader's pinned slots are copied on a load stream beside the previous step
        # (HipGoNet.enable_prefetch; +1.1% with host batches, DG_PREFETCH=0: off)
        if os.environ.get("DG_PREFETCH", "auto") != "0":
            self.net.enable_prefetch()
        self.augment = cfg.augment != "none"
        if self.augment:
            self.net.set_augment(cfg.seed, board0)
        self._step = SegmentedStep(self.net, self.bucketer, use_graphs=use_graphs)
        self._eval_n = batch
        self._last = "train"

    @property
    def rate(self) -> float:
        return float(self.net.lr.item())

    @property
    def base_rate(self) -> float:
        return self.net.lr_schedule_state()[0] if self.net.lr_rec is not None else self.rate

    @property
    def lr_step(self) -> int:
        return self.net.lr_schedule_state()[1] if self.net.lr_rec is not None else 0

    @property
    def params(self):
        return self.net.params

    def load_next(self, loader):
        """Next training batch straight from the loader's pinned packed slot into the
        network's input buffer: one async H2D copy, ordered before the step on the same
        stream.  With augmentation the kernel moves the boards right behind that copy, on the
        same stream.  Returns None (the host copy is gone; ``current_batch`` reads it back)."""
        self.net.set_batch_packed_from(loader,
                                       aug_seq=loader.consumed if self.augment else None)
        return None

    def current_batch(self):
        from ..data.batch import unpack_views
        pl, py_, rk, lb = unpack_views(self.net.inbuf.cpu(), self.B)
        return (pl.numpy().reshape(self.B, 9, 19, 19), py_.numpy(), rk.numpy(), lb.numpy())

    def set_batch(self, planes, player, rank, labels):
        dev = self.device
        t = lambda a, dt: (a if isinstance(a, torch.Tensor) else torch.from_numpy(np.asarray(a)))
        self.net.set_batch(t(planes, None).to(dev), t(player, None).to(dev),
                           t(rank, None).to(dev), t(labels, None).to(dev, torch.int32))

    def forward_backward(self):
        self.net._refuse_in_ema("forward_backward")
        self._step.forward_backward()
        self._last = "train"

    def train_step(self):
        """forward_backward + optimizer_step with nothing in between: without DP buckets
        SegmentedStep replays both as ONE hipGraph (no graph boundary before the update)."""
        self.net._refuse_in_ema("train_step")
        self._step()
        self._last = "train"

    def optimizer_step(self):
        self.net._refuse_in_ema("optimizer_step")
        self._step.optimizer()

    def evaluate(self, n: Optional[int] = None):
        self._eval_n = n or self.B
        self.net.evaluate()
        self._last = "eval"

    def loss_sum(self) -> float:
        if self._last == "eval":
            return float(self.net.eval_loss[:self._eval_n].sum().item())
        return float(self.net.loss.sum().item())

    def correct(self) -> int:
        if self._last == "eval":
            n = self._eval_n
            return int((self.net.eval_pred[:n] == self.net.labels[:n]).sum().item())
        return int((self.net.pred == self.net.labels).sum().item())

    def bad_steps(self) -> int:
        """Updates the device gate / fused update skipped so far (syncs)."""
        return int(self.net.bad_steps.item())

    def gradient_tagged(self) -> bool:
        """Whether a gradient producer tagged the step in flight (before its update: a value
        out of range — dg_common.h grad_out_of_range; the update would skip it).  Syncs.
        Single-GPU only: under DP the tag is rank-local and the all-reduced gradient's finite
        gate decides, the same on every rank."""
        if self.world > 1:
            return False
        step, tag = self.net._stepflag.tolist()
        return tag == step + 1

    def clip_stats(self):
        """grad_clip > 0: (grad_norm, clip_scale) of the last applied step and the number of
        applied steps that clipped so far, from the device record (syncs)."""
        return self.net.clip_stats()

    def lamb_stats(self):
        """optimizer=lamb: per conv-weight tensor (wn, un, phi) of the last applied step, from
        the device table (syncs)."""
        return self.net.lamb_stats()

    def ema_params(self) -> torch.Tensor:
        """ema_decay > 0: the moving average of the weights, on the host (syncs)."""
        self.net._need_ema()
        return self.net.ema.detach().cpu()

    def ema_steps(self) -> int:
        """ema_decay > 0: the averaging steps applied so far (skipped ones do not count).
        Syncs."""
        return self.net.ema_steps()

    def reset_ema(self):
        """ema_decay > 0: average = the parameters as they stand, no step applied."""
        self.net.reset_ema()

    def ema_weights(self):
        """A context manager inside which evaluate() runs on the moving average
        (HipGoNet.ema_weights: the operand copies are swapped; no training step inside)."""
        return self.net.ema_weights()

    def flat_params(self) -> torch.Tensor:
        return self.net.params.detach().cpu()

    def load_params(self, flat: torch.Tensor):
        self.net.load_params(flat)

    def state_dict(self):
        d = {"optimizer": {"kind": self.cfg.optimizer, "rate": self.rate,
                           "rate_decay": self.cfg.rateDecay}}
        if self.net.lr_rec is not None:
            # rate holds base (resumed with the schedule off, a run continues from the undamped
            # rate); lr_step is an integer: it travels in the checkpoint's metadata
            d["optimizer"]["rate"], d["optimizer"]["lr_step"] = self.net.lr_schedule_state()
        if self.net.ms is not None:
            d["optimizer"]["ms"] = self.net.ms.detach().cpu()
        if self.net.vel is not None:
            d["optimizer"]["vel"] = self.net.vel.detach().cpu()
        if self.net.adam_m is not None:
            d["optimizer"]["adam_m"] = self.net.adam_m.detach().cpu()
            d["optimizer"]["adam_v"] = self.net.adam_v.detach().cpu()
            # (an integer: it travels in the checkpoint's metadata, not as a float tensor)
            d["optimizer"]["adam_t"] = self.net.adam_steps()
        if self.net.ema is not None:
            d["optimizer"]["ema"] = self.net.ema.detach().cpu()
            d["optimizer"]["ema_t"] = self.net.ema_steps()
        return d

    def close(self):
        if self.comm is not None:
            torch.cuda.synchronize(self.device)
            self.comm.close()
            self.comm = None

    def load_state_dict(self, d):
        o = d["optimizer"]
        self.net.lr.fill_(float(o["rate"]))
        if self.net.lr_rec is not None:
            # (a checkpoint without lr_step: base = its rate, s = 0); lr is then rewritten on
            # the device from them
            self.net.set_lr_schedule_state(float(o["rate"]), int(o.get("lr_step", 0)))
        if "ms" in o and self.net.ms is not None:
            self.net.ms.copy_(o["ms"].to(self.net.ms.device))
        if self.net.vel is not None:
            # (a checkpoint without a velocity: start from rest)
            if "vel" in o:
                self.net.vel.copy_(o["vel"].to(self.net.vel.device))
            else:
                self.net.vel.zero_()
        if self.net.adam_m is not None:
            # (a checkpoint without moments: zero moments, no applied step)
            has = "adam_m" in o and "adam_v" in o
            for name in ("adam_m", "adam_v"):
                t = getattr(self.net, name)
                t.copy_(o[name].to(t.device)) if has else t.zero_()
            self.net.set_adam_steps(int(o.get("adam_t", 0)) if has else 0)
        if self.net.ema is not None:
            # (a checkpoint without an average: seeded from the parameters, t = 0)
            if "ema" in o:
                self.net.ema.copy_(o["ema"].to(self.net.ema.device))
                self.net.set_ema_steps(int(o.get("ema_t", 0)))
            else:
                self.net.reset_ema()
