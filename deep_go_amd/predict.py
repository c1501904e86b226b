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


@dataclass
class Selection:
    move: np.ndarray     # int32 [n]: the chosen point 19*x + y (-1: no legal point / bad row)
    p: np.ndarray        # float [n]: its tempered, renormalised probability
    kept: np.ndarray     # int32 [n]: size of the top_p nucleus (0: no legal point, -1: bad row)


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
        self._sel_dev = None       # select()'s buffers, made by its first call

    def _out_views(self, buf: torch.Tensor):
        m, K = self.chunk, self.K
        o1 = m * NUM_POINTS
        o2, o3 = o1 + m * K, o1 + 2 * m * K
        return (buf[:o1].view(m, NUM_POINTS), buf[o1:o2].view(m, K),
                buf[o2:o3].view(torch.int32).view(m, K), buf[o3:].view(torch.int32))

    def _predict_gpu(self, planes, player, rank, labels, extra, mask: bool, out: Prediction,
                     lo: int):
        # (_select_gpu repeats this upload / symmetry_planes / forward / policy_ensemble sequence
        # with K = 1: a change here belongs there too)
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

    def _select_gpu(self, planes, player, rank, extra, game, ply, seed, temperature, top_p,
                    out: Selection, lo: int):
        """_predict_gpu's launches with K = 1, then policy_select on the same stream; three
        words per position come back, the prob rows stay on the device."""
        from .ops.native import play, stream_handle
        net, h, S, m = self.net, self.h, self.S, self.chunk
        if self._sel_dev is None:
            # upload: game [m] | ply [m]; download: move [m] | p_move [m] | kept [m]
            self._sel_host = torch.zeros(2 * m, dtype=torch.int32).pin_memory()
            self._sel_dev = torch.zeros(2 * m, dtype=torch.int32, device=self._out_dev.device)
            self._pick_dev = torch.zeros(3 * m, dtype=torch.int32, device=self._out_dev.device)
            self._pick_host = torch.zeros(3 * m, dtype=torch.int32).pin_memory()
        k = len(planes)
        hp, hpl, hrk, hlb, hex_ = self._src_host_v
        hp[:k] = planes.reshape(k, 9, NUM_POINTS)
        hpl[:k], hrk[:k], hlb[:k], hex_[:k] = player, rank, -1, extra
        hs = self._sel_host.numpy()
        hs[:k], hs[m:m + k] = game, ply
        self._src_dev.copy_(self._src_host, non_blocking=True)
        self._sel_dev.copy_(self._sel_host, non_blocking=True)
        dp, dpl, drk, dlb, dex = self._src_dev_v
        s = stream_handle()
        h.symmetry_planes(dp.data_ptr(), dpl.data_ptr(), drk.data_ptr(), dlb.data_ptr(), k, S,
                          net.planes.data_ptr(), net.player.data_ptr(), net.rank.data_ptr(),
                          net.labels.data_ptr(), net.B, s)
        if not net._fp8_calibrated:
            net.calibrate_fp8()
        logp = net.predict_logp()
        # predict()'s device output buffer, laid out for K = 1 (it holds K >= 1):
        # prob [m, 361] | topk_p [m] | topk [m] | rank [m]
        o1 = m * NUM_POINTS
        prob, scratch = self._out_dev[:o1], self._out_dev[o1:o1 + 3 * m]
        h.policy_ensemble(logp.data_ptr(), dp.data_ptr(), 9 * NUM_POINTS, dex.data_ptr(),
                          dlb.data_ptr(), k, S, 1, 1, prob.data_ptr(),
                          scratch[m:].data_ptr(), scratch.data_ptr(), scratch[2 * m:].data_ptr(), s)
        pick = self._pick_dev
        play().policy_select(prob.data_ptr(), self._sel_dev.data_ptr(),
                             self._sel_dev[m:].data_ptr(), k, seed, temperature, top_p,
                             pick.data_ptr(), pick[m:].data_ptr(), pick[2 * m:].data_ptr(), s)
        self._pick_host.copy_(pick, non_blocking=True)
        torch.cuda.current_stream().synchronize()
        got = self._pick_host.numpy()
        out.move[lo:lo + k] = got[:k]
        out.p[lo:lo + k] = got[m:m + k].view(np.float32)
        out.kept[lo:lo + k] = got[2 * m:2 * m + k]

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

    def select(self, planes, player, rank, extra_illegal=None, *, game, ply, seed: int = 0,
               temperature: float = 1.0, top_p: float = 1.0) -> Selection:
        """One move per position, drawn from predict()'s masked distribution (mask=True) with a
        temperature and a nucleus cut: play/select.py is the definition.  game [n] and ply [n]
        (int32) key the draw together with seed, so a position's move does not depend on the
        chunk or slot that carries it.  On the GPU the selection runs on the device
        (csrc/kernels/play.hip) and three words per position are downloaded."""
        planes = np.ascontiguousarray(np.asarray(planes, np.uint8)).reshape(-1, 9, 19, 19)
        n = len(planes)
        player = np.asarray(player, np.uint8).reshape(n)
        rank = np.asarray(rank, np.uint8).reshape(n)
        game = np.asarray(game, np.int32).reshape(n)
        ply = np.asarray(ply, np.int32).reshape(n)
        extra = (np.zeros((n, NUM_POINTS), np.uint8) if extra_illegal is None
                 else (np.asarray(extra_illegal).reshape(n, NUM_POINTS) != 0).astype(np.uint8))
        seed, T, top_p = int(seed) & (2 ** 64 - 1), float(temperature), float(top_p)
        if not (np.isfinite(T) and T >= 0):
            raise ValueError(f"temperature = {temperature}: expected a finite value >= 0")
        if not 0 < top_p <= 1:
            raise ValueError(f"top_p = {top_p}: expected a value in (0, 1]")
        gpu = self.device == "gpu"
        out = Selection(np.full(n, -1, np.int32), np.zeros(n, np.float32 if gpu else np.float64),
                        np.zeros(n, np.int32))
        for lo in range(0, n, self.chunk):
            sl = slice(lo, min(n, lo + self.chunk))
            if gpu:
                self._select_gpu(planes[sl], player[sl], rank[sl], extra[sl], game[sl], ply[sl],
                                 seed, T, top_p, out, lo)
            else:
                from .play.select import select_moves
                k = sl.stop - sl.start
                logp = self.logp_cpu(planes[sl], player[sl], rank[sl])
                legal = (planes[sl, 0].reshape(k, NUM_POINTS) == 0) & (extra[sl] == 0)
                prob = ensemble_policy(logp, legal, 1)[0]
                out.move[sl], out.p[sl], out.kept[sl] = select_moves(prob, game[sl], ply[sl],
                                                                     seed, T, top_p)
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
