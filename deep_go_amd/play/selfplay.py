"""Lock-step batched self-play and matches between two checkpoints.

All games advance one ply at a time.  Per ply there is ONE ``Predictor.select`` call per
predictor, over all unfinished games in which that predictor is to move, so a forward carries
positions of many games; the draw of game ``g`` at move number ``k`` is keyed by ``(seed, g,
k)`` and does not depend on which other games are still running.  Moves follow the move policy
of ``play/game.py``.  With two predictors colours alternate by game index: ``a`` has black in
the even games, ``b`` in the odd ones.  A game ends on two passes or at ``max_moves``; an
unfinished game has result ``Void`` and counts for nobody.

``opening_plies``: that many first plies of every game are drawn with temperature 1 and
top_p 1, whatever the match's settings, so that games at a low temperature still differ.
``setup``: moves ``(player, point)`` played in every game before the match starts (a position
to play out); they are part of the game's record and of its move numbers, not of
``max_moves``.
"""
from __future__ import annotations

import json
import os
import time
from typing import List, Optional, Sequence, Tuple

from .game import BLACK, PASS, WHITE, Game, choose_moves, sgf_point


def game_sgf(g: Game, black: str, white: str, rank: int, result: str) -> str:
    """One property per line in the header: the form the project's own parse_sgf reads."""
    head = ["(;GM[1]", "FF[4]", "SZ[19]", f"KM[{g.komi:g}]", "RU[Tromp-Taylor]", f"PB[{black}]",
            f"PW[{white}]", f"BR[{rank}d]", f"WR[{rank}d]", f"RE[{result}]"]
    body = "".join(f";{'B' if pl == BLACK else 'W'}[{sgf_point(p)}]" for pl, p in g.moves)
    return "\n".join(head + [body, ")"]) + "\n"


def run_match(pred_a, pred_b=None, games: int = 1, max_moves: int = 400, komi: float = 7.5,
              rank: int = 9, seed: int = 0, temperature: float = 1.0, top_p: float = 1.0,
              opening_plies: int = 0, out_dir: Optional[str] = None,
              setup: Sequence[Tuple[int, int]] = ()):
    """-> ``{"sgf": [text per game], "moves": [[(player, point or PASS), ...] per game],
    "summary": {...}, "timing": {...}}``; out_dir: the SGFs and the summary are also written
    there, as ``game_0000.sgf`` ... and ``summary.json``.  sgf, moves and summary depend on the
    arguments alone.  timing (returned only, never written): the seconds of the match, those
    spent in ``select`` (upload, device, download) and the rest, the host engine (masks,
    planes, moves)."""
    preds = [pred_a, pred_b if pred_b is not None else pred_a]
    names = ["a", "b" if pred_b is not None else "a"]
    gs = [Game(komi) for _ in range(games)]
    for g in gs:
        for player, p in setup:
            g.play(player, p)
    # which predictor holds which colour
    holder = [{BLACK: i % 2, WHITE: 1 - i % 2} if pred_b is not None else {BLACK: 0, WHITE: 0}
              for i in range(games)]
    t_select = 0.0
    t0 = time.perf_counter()
    plies = 0
    for ply in range(max_moves):
        live = [i for i, g in enumerate(gs) if not g.over]
        if not live:
            break
        T, P = (1.0, 1.0) if ply < opening_plies else (temperature, top_p)
        turn = {i: holder[i][gs[i].to_move] for i in live}    # before anybody moves
        for k in sorted(set(turn.values())):
            mine = [i for i in live if turn[i] == k]
            sel = _Timed(preds[k])
            moves = choose_moves(sel, [gs[i] for i in mine], mine, rank, seed, T, P)
            t_select += sel.seconds
            for i, p in zip(mine, moves):
                gs[i].play(gs[i].to_move, p)
            plies += len(mine)
    wall = time.perf_counter() - t0

    per_game, sgfs = [], []
    wins = {"B": 0, "W": 0, "a": 0, "b": 0, "draw": 0, "void": 0}
    margins = []
    for i, g in enumerate(gs):
        result = g.result() if g.over else "Void"
        black, white = names[holder[i][BLACK]], names[holder[i][WHITE]]
        if not g.over:
            wins["void"] += 1
        elif result == "0":
            wins["draw"] += 1
        else:
            wins[result[0]] += 1
            if pred_b is not None:
                wins[black if result[0] == "B" else white] += 1
        if g.over:
            margins.append(g.margin())
        per_game.append({"game": i, "black": black, "white": white, "result": result,
                         "moves": len(g.moves)})
        sgfs.append(game_sgf(g, black, white, rank, result))
    if pred_b is None:
        del wins["a"], wins["b"]
    summary = {"games": games, "max_moves": max_moves, "komi": komi, "seed": seed,
               "temperature": temperature, "top_p": top_p, "opening_plies": opening_plies,
               "wins": wins, "mean_score": sum(margins) / len(margins) if margins else None,
               "per_game": per_game}
    if out_dir:
        os.makedirs(out_dir, exist_ok=True)
        for i, text in enumerate(sgfs):
            with open(os.path.join(out_dir, f"game_{i:04d}.sgf"), "w") as f:
                f.write(text)
        with open(os.path.join(out_dir, "summary.json"), "w") as f:
            json.dump(summary, f, indent=1)
            f.write("\n")
    return {"sgf": sgfs, "moves": [list(g.moves) for g in gs], "summary": summary,
            "timing": {"seconds": wall, "plies": plies, "select_seconds": t_select,
                       "host_engine_seconds": wall - t_select}}


class _Timed:
    """A predictor whose select() calls are timed (run_match's timing)."""

    def __init__(self, predictor):
        self.predictor, self.cfg, self.seconds = predictor, predictor.cfg, 0.0

    def select(self, *a, **kw):
        t = time.perf_counter()
        try:
            return self.predictor.select(*a, **kw)
        finally:
            self.seconds += time.perf_counter() - t


def moves_of(sgf_text: str) -> List[tuple]:
    """The stone moves ``(player, x, y)`` of an SGF, by the project's own parser."""
    from ..ops.native import cpu
    return [tuple(m) for m in cpu().parse_sgf(sgf_text)["moves"]]


__all__ = ["run_match", "game_sgf", "moves_of", "PASS"]
