"""Move prediction: a checkpoint and positions in, a legal-move distribution out.

``Predictor`` averages the policy over the eight symmetries of the board (the dihedral group
D4, ``data/symmetry.py``), removes illegal points, renormalises, and returns the top-k moves
and the rank of the expert move.  The net is not symmetric by construction — every layer has
an untied per-position bias and the training data is not augmented — so the average is a real
ensemble.

Legality here is **"empty, and not the simple-ko point"**: the engine enforces neither ko nor
suicide (``csrc/engine/go_engine.h``), so an empty point is only excluded when the caller
marks it (``extra_illegal``; ``positions_from_sgf`` returns the simple-ko point of every
position for this).  Suicide and superko are not checked.

GPU path (one chunk of ``batch // symmetries`` positions per forward): one upload ->
``symmetry_planes`` into the net's input views -> ``HipGoNet.predict_logp`` ->
``policy_ensemble`` -> one download (csrc/kernels/policy.hip).  CPU path: the fp32 oracle
``models.gocnn.reference_forward`` and ``data.symmetry.ensemble_policy``.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional

import numpy as np
import torch

from .config import NUM_POINTS, ExperimentConfig
from .data.batch import packed_batch_bytes, unpack_views
from .data.symmetry import ensemble_policy, transform_planes
from .models.gocnn import ParamLayout, init_params, reference_forward

MAX_TOP = 64   # policy.hip MAX_TOPK


@dataclass
class Prediction:
    prob: np.ndarray     # float [n, 361]: legal-move distribution (0 at illegal points)
    topk: np.ndarray     # int32 [n, K]: points 19*x + y by decreasing probability (-1: none)
    topk_p: np.ndarray   # float [n, K]: prob at those points
    rank: np.ndarray     # int32 [n]: rank of the label (0 = top-1; -1: no / illegal label)


def _gpu_usable() -> bool:
    from .ops.native import hip_available
    return torch.cuda.is_available() and hip_available()


class Predictor:
    """``predict()`` for one set of weights.  ``batch`` is the number of boards per forward;
    a forward carries ``batch // symmetries`` positions."""

    def __init__(self, cfg: ExperimentConfig, flat_params: Optional[torch.Tensor] = None,
                 batch: int = 64, symmetries: int = 8, device: str = "auto", top: int = 5):
        if symmetries not in (1, 8):
            raise ValueError(f"symmetries = {symmetries}: expected 1 or 8")
        if batch <= 0 or batch % symmetries:
            raise ValueError(f"batch {batch} is not a positive multiple of symmetries "
                             f"{symmetries}")
        if not 1 <= top <= MAX_TOP:
            raise ValueError(f"top = {top}: expected 1..{MAX_TOP}")
        if device not in ("auto", "cpu", "gpu"):
            raise ValueError(f"device {device!r}: expected auto, cpu or gpu")
        if device == "gpu" and not torch.cuda.is_available():
            raise RuntimeError("device='gpu': no GPU present")
        self.cfg = cfg
        self.B, self.S, self.K = batch, symmetries, top
        self.chunk = batch // symmetries
        self.layout = ParamLayout(cfg)
        if flat_params is None:
            flat_params = init_params(self.layout, cfg.seed)
        self.device = "gpu" if device == "gpu" or (device == "auto" and _gpu_usable()) else "cpu"
        self.net = None
        if self.device == "gpu":
            self._init_gpu(flat_params)
        else:
            self.params = flat_params.detach().float().cpu().contiguous()

    @classmethod
    def load(cls, checkpoint: str, ema: bool = False, **kw) -> "Predictor":
        """ema: predict with the checkpoint's moving average of the weights (ema_decay > 0)
        instead of its parameters; a checkpoint without one raises ValueError."""
        from .utils.checkpoint import ema_params, load_checkpoint
        cfg, flat, _, opt = load_checkpoint(checkpoint)
        if ema:
            flat = ema_params(checkpoint, flat, opt)
        return cls(cfg, flat, **kw)

    # ------------------------------------------------------------------ GPU
    def _init_gpu(self, flat_params):
        from .models.hip_model import HipGoNet
        from .ops.native import hip
        self.h = hip()
        dev = torch.device("cuda", torch.cuda.current_device())
        self.net = HipGoNet(self.cfg, self.B, device=dev, flat_params=flat_params)
        self.net.enable_predict()
        m, K = self.chunk, self.K
        # one upload: the chunk as a packed batch of m positions, then extra_illegal [m, 361]
        nb = packed_batch_bytes(m)
        self._src_host = torch.zeros(nb + m * NUM_POINTS, dtype=torch.uint8).pin_memory()
        self._src_dev = torch.zeros_like(self._src_host, device=dev)
        self._src_host_v = tuple(v.numpy() for v in unpack_views(self._src_host[:nb], m) + (
            self._src_host[nb:].view(m, NUM_POINTS),))
        self._src_dev_v = unpack_views(self._src_dev[:nb], m) + (
            self._src_dev[nb:].view(m, NUM_POINTS),)
        # one download: prob [m, 361] | topk_p [m, K] | topk [m, K] | rank [m], 4 bytes each
        words = m * (NUM_POINTS + 2 * K + 1)
        self._out_dev = torch.zeros(words, dtype=torch.float32, device=dev)
        self._out_host = torch.zeros(words, dtype=torch.float32).pin_memory()

    def _out_views(self, buf: torch.Tensor):
        m, K = self.chunk, self.K
        o1 = m * NUM_POINTS
        o2, o3 = o1 + m * K, o1 + 2 * m * K
        return (buf[:o1].view(m, NUM_POINTS), buf[o1:o2].view(m, K),
                buf[o2:o3].view(torch.int32).view(m, K), buf[o3:].view(torch.int32))

    def _predict_gpu(self, planes, player, rank, labels, extra, mask: bool, out: Prediction,
                     lo: int):
        from .ops.native import stream_handle
        net, h, S = self.net, self.h, self.S
        k = len(planes)
        hp, hpl, hrk, hlb, hex_ = self._src_host_v
        hp[:k] = planes.reshape(k, 9, NUM_POINTS)
        hpl[:k], hrk[:k], hlb[:k], hex_[:k] = player, rank, labels, extra
        self._src_dev.copy_(self._src_host, non_blocking=True)
        dp, dpl, drk, dlb, dex = self._src_dev_v
        s = stream_handle()
        # (net.planes ... are the views of the input buffer its launches currently read)
        h.symmetry_planes(dp.data_ptr(), dpl.data_ptr(), drk.data_ptr(), dlb.data_ptr(), k, S,
                          net.planes.data_ptr(), net.player.data_ptr(), net.rank.data_ptr(),
                          net.labels.data_ptr(), net.B, s)
        if not net._fp8_calibrated:
            net.calibrate_fp8()
        logp = net.predict_logp()
        prob, topk_p, topk, rk = self._out_views(self._out_dev)
        h.policy_ensemble(logp.data_ptr(), dp.data_ptr(), 9 * NUM_POINTS, dex.data_ptr(),
                          dlb.data_ptr(), k, S, self.K, int(mask), prob.data_ptr(),
                          topk.data_ptr(), topk_p.data_ptr(), rk.data_ptr(), s)
        self._out_host.copy_(self._out_dev, non_blocking=True)
        torch.cuda.current_stream().synchronize()
        prob, topk_p, topk, rk = self._out_views(self._out_host)
        out.prob[lo:lo + k] = prob[:k].numpy()
        out.topk_p[lo:lo + k] = topk_p[:k].numpy()
        out.topk[lo:lo + k] = topk[:k].numpy()
        out.rank[lo:lo + k] = rk[:k].numpy()

    # ------------------------------------------------------------------ CPU (fp32 oracle)
    def logp_cpu(self, planes: np.ndarray, player: np.ndarray, rank: np.ndarray) -> np.ndarray:
        """fp32 reference log-probabilities [k, S, 361] of the S views of each position."""
        from .ops.native import cpu
        k, S = len(planes), self.S
        views = np.stack([transform_planes(planes, s) for s in range(S)], axis=1)
        x = cpu().expand(np.ascontiguousarray(views.reshape(k * S, 9, 19, 19)),
                         np.repeat(player, S), np.repeat(rank, S), self.cfg.ko_plane)
        with torch.no_grad():
            logp = reference_forward(self.layout, self.params, torch.from_numpy(x),
                                     head_relu=self.cfg.head_relu)
        return logp.numpy().reshape(k, S, NUM_POINTS)

    def _predict_cpu(self, planes, player, rank, labels, extra, mask: bool, out: Prediction,
                     lo: int):
        k = len(planes)
        logp = self.logp_cpu(planes, player, rank)
        legal = np.ones((k, NUM_POINTS), bool)
        if mask:
            legal = (planes[:, 0].reshape(k, NUM_POINTS) == 0) & (extra == 0)
        prob, topk, topk_p, rk = ensemble_policy(logp, legal, self.K, labels)
        out.prob[lo:lo + k], out.topk[lo:lo + k] = prob, topk
        out.topk_p[lo:lo + k], out.rank[lo:lo + k] = topk_p, rk

    # ------------------------------------------------------------------ public
    def predict(self, planes, player, rank, labels=None, extra_illegal=None,
                mask: bool = True) -> Prediction:
        """planes uint8 [n, 9, 19, 19] (stored planes, data/features.py), player [n] (1 black /
        2 white to move), rank [n] (dan of that player); labels [n] (19*x + y, -1 none) and
        extra_illegal [n, 361] (nonzero = illegal, e.g. the simple-ko point) optional.

        mask=True: a point is legal when it is empty and not marked in extra_illegal (ko and
        suicide are NOT derived from the position); mask=False: every point is legal.  Any n:
        the positions run in chunks of ``batch // symmetries``, the last one partly full."""
        planes = np.ascontiguousarray(np.asarray(planes, np.uint8)).reshape(-1, 9, 19, 19)
        n = len(planes)
        player = np.asarray(player, np.uint8).reshape(n)
        rank = np.asarray(rank, np.uint8).reshape(n)
        labels = (np.full(n, -1, np.int32) if labels is None
                  else np.asarray(labels, np.int32).reshape(n))
        extra = (np.zeros((n, NUM_POINTS), np.uint8) if extra_illegal is None
                 else (np.asarray(extra_illegal).reshape(n, NUM_POINTS) != 0).astype(np.uint8))
        gpu = self.device == "gpu"
        ft = np.float32 if gpu else np.float64
        out = Prediction(np.zeros((n, NUM_POINTS), ft), np.full((n, self.K), -1, np.int32),
                         np.zeros((n, self.K), ft), np.full(n, -1, np.int32))
        run = self._predict_gpu if gpu else self._predict_cpu
        for lo in range(0, n, self.chunk):
            sl = slice(lo, min(n, lo + self.chunk))
            run(planes[sl], player[sl], rank[sl], labels[sl], extra[sl], bool(mask), out, lo)
        return out


def ko_mask(ko_points) -> np.ndarray:
    """[n] simple-ko points (19*x + y, -1 none) -> the extra_illegal array [n, 361]."""
    ko = np.asarray(ko_points, np.int64)
    m = np.zeros((len(ko), NUM_POINTS), np.uint8)
    rows = np.flatnonzero(ko >= 0)
    m[rows, ko[rows]] = 1
    return m


def positions_from_sgf(text: str, mark_ko: bool = False):
    """Every move of an SGF game as a prediction input: ``(planes uint8 [n,9,19,19], player
    [n], rank [n], label [n], ko [n])`` — the position before move k, who plays it, that
    player's dan rank (0 when the game has none), the move as ``19*x + y`` and the simple-ko
    point of the position (-1 none).  mark_ko (``cfg.ko_plane``): also mark that point in the
    stored liberty plane, which is where a model built with the ko plane reads it.

    The engine enforces neither ko nor suicide, so the ko point is returned for the caller's
    legality mask (``ko_mask``); the position after the game's last move is not produced."""
    from .ops.native import cpu
    eng = cpu()
    g = eng.parse_sgf(text)
    moves, handicap = g["moves"], g["handicap"]
    n = len(moves)
    planes = np.asarray(eng.game_positions(handicap, moves, bool(mark_ko)), np.uint8)
    planes = planes.reshape(n, 9, 19, 19)
    ko = np.asarray(eng.game_ko_points(handicap, moves), np.int32).reshape(n)
    player = np.array([m[0] for m in moves], np.uint8)
    ranks = {1: int(g["black_rank"]), 2: int(g["white_rank"])}
    rank = np.array([ranks[int(p)] for p in player], np.uint8)
    label = np.array([19 * m[1] + m[2] for m in moves], np.int32)
    return planes, player, rank, label, ko
