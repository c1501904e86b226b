"""Move selection: the definition, and its float64 numpy oracle.

``select_moves`` turns rows of ``policy_ensemble``'s ``prob [n, 361]`` (masked to the legal
points and normalised) into one move per row, with a temperature ``T`` and a nucleus
(``top_p``) cut.  csrc/kernels/play.hip (``policy_select``) is the GPU form; the CPU path of
``Predictor.select`` runs this module.  Per row ``i``::

    a row with a non-finite or negative entry: move = -1, p_move = 0, kept = -1
    a row of zeros (no legal point):           move = -1, p_move = 0, kept = 0
    T == 0:  move = the largest prob, ties to the lower index; p_move = 1; kept = 1
    w[p] = prob[p]                          if T == 1
         = exp(log(prob[p]) / T)            otherwise (0 stays 0);   W = sum_p w[p]
    W == 0 (every tempered weight underflowed): as T == 0
    ahead(q, p) := w[q] > w[p] or (w[q] == w[p] and q < p)
    above[p] = sum_{q ahead of p} w[q]          (q in index order)
    keep[p]  = w[p] > 0 and above[p] < top_p * W        (the top point is always kept)
    kept = #keep;   Wk = sum_{keep} w
    u = select_uniform(seed, game[i], ply[i])   in [0, 1)
    c[p] = sum_{q <= p, keep[q]} w[q];   move = the least p with keep[p] and c[p] > u * Wk
           (the last kept point if rounding leaves none);   p_move = w[move] / Wk

``T -> 0`` sharpens towards the argmax, ``T = 1`` with ``top_p = 1`` samples ``prob`` itself,
and ``top_p < 1`` keeps the smallest set of most probable points whose weight reaches
``top_p`` of the whole.

``select_uniform`` has no generator state: a position's draw is a pure 32-bit integer hash of
all 64 bits of ``seed`` and the low 32 bits of ``game`` and ``ply``, so it does not depend on
which chunk or batch slot carries the position.  With ``mix32`` the lowbias32 finaliser
(``data/symmetry.py``; the domain constant differs from ``augment_symmetries``')::

    a = mix32((seed_lo ^ 0x3c6ef372) + seed_hi)
    b = mix32(a + game)
    h = mix32(b ^ ply)
    u = (h >> 8) * 2^-24

``u`` lies on the 2^-24 grid, so it is exact in fp32 and the same on host and device.
"""
from __future__ import annotations

from typing import Tuple

import numpy as np

from ..data.symmetry import NUM_POINTS, _mix32

_M32 = 0xFFFFFFFF
_DOMAIN = 0x3c6ef372


def select_uniform(seed: int, game, ply) -> np.ndarray:
    """float64 array of the draws for ``(seed, game[i], ply[i])`` (``game`` and ``ply``
    broadcast against each other)."""
    seed = int(seed) & (2 ** 64 - 1)
    game = (np.asarray(game, np.int64) & _M32).astype(np.uint32)
    ply = (np.asarray(ply, np.int64) & _M32).astype(np.uint32)
    with np.errstate(over="ignore"):
        a = _mix32(np.array([(seed & _M32) ^ _DOMAIN], np.uint32)
                   + np.array([seed >> 32], np.uint32))
        h = _mix32(_mix32(a + game) ^ ply)
    u = (h >> np.uint32(8)).astype(np.float64) * 2.0 ** -24
    return u.reshape(np.broadcast(game, ply).shape)


def tempered(prob: np.ndarray, T: float) -> np.ndarray:
    """``w`` of the definition for one row or an array of rows (float64)."""
    prob = np.asarray(prob, np.float64)
    if T == 1:
        return prob.copy()
    w = np.zeros_like(prob)
    pos = prob > 0
    with np.errstate(under="ignore"):
        w[pos] = np.exp(np.log(prob[pos]) / T)
    return w


def nucleus(w: np.ndarray, top_p: float) -> Tuple[np.ndarray, np.ndarray]:
    """``(keep, above)`` of one row of weights."""
    w = np.asarray(w, np.float64)
    idx = np.arange(len(w))
    ahead = (w[None, :] > w[:, None]) | ((w[None, :] == w[:, None]) & (idx[None, :] < idx[:, None]))
    above = np.where(ahead, w[None, :], 0.0).sum(1)
    return (w > 0) & (above < top_p * w.sum()), above


def select_moves(prob, game, ply, seed: int = 0, temperature: float = 1.0, top_p: float = 1.0
                 ) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """The float64 oracle: ``(move int32 [n], p_move float64 [n], kept int32 [n])`` for the keys
    ``game [n]``, ``ply [n]``.  ``prob [n, 361]``, or ``[1, 361]``: one row for every key."""
    T = float(temperature)
    if not (np.isfinite(T) and T >= 0):
        raise ValueError(f"temperature = {temperature}: expected a finite value >= 0")
    if not 0 < top_p <= 1:
        raise ValueError(f"top_p = {top_p}: expected a value in (0, 1]")
    prob = np.asarray(prob, np.float64).reshape(-1, NUM_POINTS)
    game = np.asarray(game, np.int64).reshape(-1)
    n = len(game)
    ply = np.asarray(ply, np.int64).reshape(n)
    if len(prob) not in (1, n):
        raise ValueError(f"{len(prob)} rows for {n} keys")
    u = select_uniform(seed, game, ply)
    move = np.full(n, -1, np.int32)
    p_move = np.zeros(n, np.float64)
    kept = np.zeros(n, np.int32)
    for i, row in enumerate(prob):
        sl = slice(i, i + 1) if len(prob) == n else slice(0, n)   # the keys this row serves
        if not (np.isfinite(row).all() and (row >= 0).all()):
            kept[sl] = -1
            continue
        if not (row > 0).any():
            continue
        w = tempered(row, T) if T != 0 else row
        if T == 0 or w.sum() == 0:
            move[sl], p_move[sl], kept[sl] = int(np.argmax(row)), 1.0, 1   # first of the largest
            continue
        keep, _ = nucleus(w, top_p)
        c = np.cumsum(np.where(keep, w, 0.0))
        # the least p with c[p] > u Wk: c rises only at kept points, so that p is a kept one
        m = np.searchsorted(c, u[sl] * c[-1], side="right")
        m[m == NUM_POINTS] = np.flatnonzero(keep)[-1]
        move[sl], p_move[sl], kept[sl] = m, w[m] / c[-1], int(keep.sum())
    return move, p_move, kept
