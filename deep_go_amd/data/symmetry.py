"""The eight symmetries of the board (the dihedral group D4) and the float64 oracle of the
symmetry-averaged, legality-masked policy.

A point is ``p = 19*x + y`` (the label convention of ``data/features.py``).  For ``s`` in
``0..7``, ``T_s`` maps ``(x, y)``:

* if ``s & 4``, first swap to ``(y, x)``;
* then apply ``(a, b) -> (b, 18 - a)`` exactly ``s & 3`` times.

``s = 0`` is the identity.  The GPU forms are ``symmetry_planes`` and ``policy_ensemble``
(csrc/kernels/policy.hip); this module is what the CPU path of ``deep_go_amd.predict`` runs
and what the tests compare the kernels with.
"""
from __future__ import annotations

from typing import Optional, Tuple

import numpy as np

BOARD = 19
NUM_POINTS = BOARD * BOARD
NUM_SYMMETRIES = 8


def _build_perm() -> np.ndarray:
    out = np.zeros((NUM_SYMMETRIES, NUM_POINTS), np.int16)
    for s in range(NUM_SYMMETRIES):
        for p in range(NUM_POINTS):
            a, b = divmod(p, BOARD)
            if s & 4:
                a, b = b, a
            for _ in range(s & 3):
                a, b = b, BOARD - 1 - a
            out[s, p] = BOARD * a + b
    out.setflags(write=False)
    return out


# SYM_PERM[s][p] = T_s(p)
SYM_PERM = _build_perm()


def transform_planes(planes: np.ndarray, s: int) -> np.ndarray:
    """``dst[..., T_s(p)] = src[..., p]`` for an array whose last axis is the 361 points, or
    whose last two axes are the 19 x 19 board."""
    planes = np.asarray(planes)
    board = planes.shape[-2:] == (BOARD, BOARD)
    flat = planes.reshape(planes.shape[:-2] + (NUM_POINTS,)) if board else planes
    if flat.shape[-1] != NUM_POINTS:
        raise ValueError(f"last axis must hold {NUM_POINTS} points, got {planes.shape}")
    out = np.empty_like(flat)
    out[..., SYM_PERM[s].astype(np.int64)] = flat
    return out.reshape(planes.shape)


def transform_label(label, s: int):
    """``T_s(label)``; ``-1`` (no label) stays ``-1``.  Scalars or arrays."""
    lab = np.asarray(label, dtype=np.int64)
    out = np.where(lab >= 0, SYM_PERM[s].astype(np.int64)[np.clip(lab, 0, NUM_POINTS - 1)], -1)
    return int(out) if out.ndim == 0 else out.astype(np.int32)


def ensemble_policy(logp: np.ndarray, legal: np.ndarray, K: int,
                    labels: Optional[np.ndarray] = None
                    ) -> Tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray]:
    """float64 oracle.  ``logp [n, S, 361]``: the log-probabilities of position ``i`` seen
    through symmetry ``s``; ``legal [n, 361]`` (nonzero = legal).

    * ``q[p] = (1/S) * sum_s exp(logp[i, s, T_s(p)])``
    * ``prob[p] = q[p] / sum of q over legal points`` at legal points, 0 elsewhere; all 0
      when no point is legal
    * ``topk_idx / topk_p [n, K]``: the K legal points of largest ``prob``, ties to the lower
      index; the tail is ``-1`` / ``0`` when fewer than K points are legal
    * ``label_rank [n]``: the number of legal ``r`` with ``prob[r] > prob[y]`` or
      ``prob[r] == prob[y] and r < y``; ``-1`` without labels, for ``y < 0`` or an illegal ``y``

    Returns ``(prob, topk_idx, topk_p, label_rank)``."""
    logp = np.asarray(logp, np.float64)
    n, S, _ = logp.shape
    if S not in (1, NUM_SYMMETRIES):
        raise ValueError(f"S = {S}: expected 1 or {NUM_SYMMETRIES}")
    legal = np.asarray(legal).astype(bool).reshape(n, NUM_POINTS)
    q = np.zeros((n, NUM_POINTS), np.float64)
    for s in range(S):
        q += np.exp(logp[:, s, SYM_PERM[s].astype(np.int64)])
    q /= S
    prob = np.zeros_like(q)
    topk_idx = np.full((n, K), -1, np.int32)
    topk_p = np.zeros((n, K), np.float64)
    rank = np.full(n, -1, np.int32)
    for i in range(n):
        lg = legal[i]
        if not lg.any():
            continue
        prob[i, lg] = q[i, lg] / q[i, lg].sum()
        pts = np.flatnonzero(lg)
        # descending prob, ties to the lower index (stable sort over ascending points)
        order = pts[np.argsort(-prob[i, pts], kind="stable")]
        m = min(K, len(order))
        topk_idx[i, :m] = order[:m]
        topk_p[i, :m] = prob[i, order[:m]]
        if labels is not None:
            y = int(labels[i])
            if 0 <= y < NUM_POINTS and lg[y]:
                py = prob[i, y]
                rank[i] = int(np.sum((prob[i, pts] > py) | ((prob[i, pts] == py) & (pts < y))))
    return prob, topk_idx, topk_p, rank
