"""A live game for play: a thin wrapper over the engine's ``_dgcpu.Game``, GTP vertex
conversion, and the move policy that the GTP engine and self-play share.

A point is ``p = 19*x + y`` (``data/features.py``).  Its GTP vertex is the letter of column
``x``, counted ``A..T`` without ``I``, followed by the number ``19 - y``: SGF ``pd`` (x = 15,
y = 3) is ``Q16``.

The move policy, for the player to move:

* candidates are the points of ``legal_mask(player, suicide=False, superko=True,
  eye_fill=False)``: empty, not the simple-ko point, not suicide, not a positional-superko
  repeat, not one of the player's own simple eyes;
* with no candidate the player passes;
* if the opponent has just passed and the Tromp-Taylor score with komi already favours the
  player, the player passes (and so ends the game as its winner);
* otherwise the move is ``Predictor.select`` on ``planes(cfg.ko_plane)`` with the mask as
  ``extra_illegal``.

There is no resignation.
"""
from __future__ import annotations

from typing import List, Optional, Sequence, Tuple

import numpy as np

from ..config import NUM_POINTS

BOARD = 19
COLUMNS = "ABCDEFGHJKLMNOPQRST"
PASS = -1
BLACK, WHITE = 1, 2


def vertex(p: int) -> str:
    """``19*x + y`` -> GTP vertex (``pass`` for PASS)."""
    if p == PASS:
        return "pass"
    x, y = divmod(int(p), BOARD)
    return f"{COLUMNS[x]}{BOARD - y}"


def parse_vertex(text: str) -> int:
    """GTP vertex -> ``19*x + y`` (PASS for ``pass``); ValueError for anything else."""
    t = text.strip().upper()
    if t == "PASS":
        return PASS
    if len(t) < 2 or t[0] not in COLUMNS or not t[1:].isdigit():
        raise ValueError(f"bad vertex {text!r}")
    row = int(t[1:])
    if not 1 <= row <= BOARD:
        raise ValueError(f"bad vertex {text!r}")
    return BOARD * COLUMNS.index(t[0]) + (BOARD - row)


def parse_colour(text: str) -> int:
    t = text.strip().lower()
    if t in ("b", "black"):
        return BLACK
    if t in ("w", "white"):
        return WHITE
    raise ValueError(f"bad colour {text!r}")


def sgf_point(p: int) -> str:
    if p == PASS:
        return ""
    x, y = divmod(int(p), BOARD)
    return chr(ord("a") + x) + chr(ord("a") + y)


class Game:
    """The engine's game plus komi and the list of moves played ``(player, p)``."""

    def __init__(self, komi: float = 7.5):
        from ..ops.native import cpu
        self.g = cpu().Game()
        self.komi = float(komi)
        self.moves: List[Tuple[int, int]] = []

    # engine state, as is
    to_move = property(lambda self: self.g.to_move)
    ply = property(lambda self: self.g.ply)
    last_was_pass = property(lambda self: self.g.last_was_pass)

    def stones(self) -> np.ndarray:
        return self.g.stones()

    def planes(self, mark_ko: bool = False) -> np.ndarray:
        return self.g.planes(mark_ko)

    def legal_mask(self, player: int, suicide: bool = False, superko: bool = True,
                   eye_fill: bool = True) -> np.ndarray:
        return self.g.legal_mask(player, suicide, superko, eye_fill)

    def clear(self):
        self.g.clear()
        self.moves.clear()

    def play(self, player: int, p: int):
        """A stone at ``p``, or a pass for PASS.  Raises on an occupied point."""
        if p == PASS:
            self.g.pass_(player)
        else:
            self.g.play(player, *divmod(int(p), BOARD))
        self.moves.append((player, int(p)))

    def undo(self) -> bool:
        if not self.g.undo():
            return False
        self.moves.pop()
        return True

    @property
    def over(self) -> bool:
        """Two passes in a row."""
        return len(self.moves) >= 2 and self.moves[-1][1] == PASS and self.moves[-2][1] == PASS

    def margin(self) -> float:
        """Tromp-Taylor black area - white area - komi."""
        b, w = self.g.score()
        return b - w - self.komi

    def result(self) -> str:
        """``B+x.5``, ``W+x.5`` or ``0``, as GTP's final_score and SGF's RE spell it."""
        m = self.margin()
        if m == 0:
            return "0"
        return f"{'B' if m > 0 else 'W'}+{abs(m):g}"

    def candidates(self, player: int) -> Optional[np.ndarray]:
        """The move policy up to the net: the ``extra_illegal`` mask [361] to select under, or
        None when the player passes."""
        mask = self.legal_mask(player, suicide=False, superko=True, eye_fill=False)
        if mask.all():
            return None
        if self.last_was_pass and self.to_move == player:    # the opponent's pass, not its own
            m = self.margin()
            if (m > 0 and player == BLACK) or (m < 0 and player == WHITE):
                return None
        return mask


class NonFinitePolicy(RuntimeError):
    """A selection came back with kept = -1: the policy row held a non-finite entry."""


def choose_moves(predictor, games: Sequence[Game], ids: Sequence[int], rank: int, seed: int,
                 temperature: float, top_p: float,
                 players: Optional[Sequence[int]] = None) -> List[int]:
    """The move policy for the player to move of every game (or for ``players[k]``, which GTP
    may ask for out of turn), the net's part in ONE
    ``Predictor.select`` call: the draw of game ``k`` is keyed by ``(seed, ids[k], its ply)``.
    Returns a point or PASS per game; raises NonFinitePolicy on a row with ``kept = -1``
    (nothing is played here in any case)."""
    out = [PASS] * len(games)
    if players is None:
        players = [g.to_move for g in games]
    rows, planes, masks = [], [], []
    for k, g in enumerate(games):
        mask = g.candidates(players[k])
        if mask is not None:
            rows.append(k)
            planes.append(g.planes(bool(predictor.cfg.ko_plane)))
            masks.append(mask)
    if rows:
        sel = predictor.select(
            np.stack(planes), np.array([players[k] for k in rows], np.uint8),
            np.full(len(rows), rank, np.uint8), np.stack(masks),
            game=np.array([ids[k] for k in rows], np.int32),
            ply=np.array([games[k].ply for k in rows], np.int32),
            seed=seed, temperature=temperature, top_p=top_p)
        if (sel.kept < 0).any():
            raise NonFinitePolicy("non-finite policy")
        for k, m in zip(rows, sel.move):
            assert 0 <= m < NUM_POINTS     # (a candidate exists, so a point was chosen)
            out[k] = int(m)
    return out
