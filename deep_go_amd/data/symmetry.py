"""The eight symmetries of the board (the dihedral group D4) and the float64 oracle of the
symmetry-averaged, legality-masked policy.

A point is ``p = 19*x + y`` (the label convention of ``data/features.py``).  For ``s`` in
``0..7``, ``T_s`` maps ``(x, y)``:

* if ``s & 4``, first swap to ``(y, x)``;
* then apply ``(a, b) -> (b, 18 - a)`` exactly ``s & 3`` times.

``s = 0`` is the identity.  The GPU forms are ``symmetry_planes`` and ``policy_ensemble``
(csrc/kernels/policy.hip); this module is what the CPU path of ``deep_go_amd.predict`` runs
and what the tests compare the kernels with.

Training-time augmentation (``augment=d4``): ``augment_symmetries`` defines which symmetry
every board of every training batch gets, ``augment_batch`` is the numpy oracle of the
transform; csrc/kernels/augment.hip is the GPU form of both.
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


# the inverse element: T_{SYM_INVERSE[s]} undoes T_s
SYM_INVERSE = np.array([next(t for t in range(NUM_SYMMETRIES)
                             if (SYM_PERM[t][SYM_PERM[s]] == np.arange(NUM_POINTS)).all())
                        for s in range(NUM_SYMMETRIES)], np.uint8)
SYM_INVERSE.setflags(write=False)

_M32 = 0xFFFFFFFF


def _mix32(x: np.ndarray) -> np.ndarray:
    """The "lowbias32" finaliser on uint32 arrays (arithmetic mod 2^32)."""
    x = x ^ (x >> np.uint32(16))
    x = x * np.uint32(0x7feb352d)
    x = x ^ (x >> np.uint32(15))
    x = x * np.uint32(0x846ca68b)
    return x ^ (x >> np.uint32(16))


def augment_symmetries(seed: int, seq: int, board0: int, n: int) -> np.ndarray:
    """uint8 [n]: the symmetry id of boards ``board0 .. board0 + n - 1`` of the training batch
    with loader sequence number ``seq``.  A pure 32-bit integer hash of all 64 bits of ``seed``
    and ``seq`` and the low 32 bits of the board index, with no generator state: exact under
    resume, and what the kernel repeats bit for bit (augment.hip hash_symmetry).  With ``mix32``
    the lowbias32 finaliser::

        a = mix32((seed_lo ^ 0x9e3779b9) + seed_hi)
        b = mix32(mix32(a + seq_lo) ^ seq_hi)
        s = mix32(b + board_lo) >> 29
    """
    seed, seq = int(seed) & (2 ** 64 - 1), int(seq) & (2 ** 64 - 1)
    u = lambda v: np.array([v & _M32], np.uint32)   # noqa: E731
    with np.errstate(over="ignore"):
        a = _mix32((u(seed) ^ np.uint32(0x9e3779b9)) + u(seed >> 32))
        b = _mix32(_mix32(a + u(seq)) ^ u(seq >> 32))
        board = ((int(board0) + np.arange(n, dtype=np.uint64)) & np.uint64(_M32)).astype(np.uint32)
        return (_mix32(b + board) >> np.uint32(29)).astype(np.uint8)


def augment_batch(planes: np.ndarray, labels: np.ndarray, sym) -> Tuple[np.ndarray, np.ndarray]:
    """The numpy oracle of the training-time augmentation: new ``(planes, labels)`` with board
    ``i`` moved by ``T_sym[i]`` (every stored plane, so a ko mark in the liberty plane moves
    with its point) and a label in ``0..360`` replaced by ``T_s(label)``; any other label value
    stays as it is.  ``planes [n, 9, 19, 19]`` or ``[n, 9, 361]``; player and rank are not
    involved."""
    planes, labels = np.asarray(planes), np.asarray(labels)
    sym = np.asarray(sym).astype(np.int64) & 7
    if not (len(planes) == len(labels) == len(sym)):
        raise ValueError(f"{len(planes)} boards, {len(labels)} labels, {len(sym)} symmetries")
    out_p, out_l = planes.copy(), labels.copy()
    for i, s in enumerate(sym):
        if s == 0:
            continue
        out_p[i] = transform_planes(planes[i], int(s))
        if 0 <= labels[i] < NUM_POINTS:
            out_l[i] = transform_label(int(labels[i]), int(s))
    return out_p, out_l


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
