"""A GTP (Go Text Protocol, version 2) front end over a ``Predictor``: what Sabaki, GoGui or
gogui-twogtp need to drive a checkpoint.  ``GtpEngine(predictor).run(sys.stdin, sys.stdout)``.

The board is 19 x 19 only.  ``genmove`` follows the move policy of ``play/game.py`` (it never
resigns); the draw of a move is keyed by ``(seed, game number, ply)``, the game number counting
``clear_board`` commands, so a replayed session repeats its moves.  ``play`` accepts what the
engine's mask with ``eye_fill=True`` accepts: no occupied point, simple-ko point, suicide or
positional-superko repeat.
"""
from __future__ import annotations

import inspect

from .. import __version__ as _VERSION
from .game import (BOARD, COLUMNS, PASS, Game, NonFinitePolicy, choose_moves, parse_colour,
                   parse_vertex, vertex)


class GtpError(Exception):
    pass


class GtpEngine:
    NAME = "deep_go_amd"

    def __init__(self, predictor, rank: int = 9, seed: int = 0, temperature: float = 1.0,
                 top_p: float = 1.0, komi: float = 7.5):
        self.predictor, self.rank, self.seed = predictor, int(rank), int(seed)
        self.temperature, self.top_p = float(temperature), float(top_p)
        self.game = Game(komi)
        self.game_no = 0
        self.commands = {name[4:]: getattr(self, name) for name in dir(self)
                         if name.startswith("cmd_")}

    # ------------------------------------------------------------------ protocol
    def handle(self, line: str):
        """One input line -> (the response text or None for a skipped line, quit?)."""
        line = "".join(c for c in line.split("#", 1)[0].replace("\t", " ")
                       if c == " " or c.isprintable()).strip()
        if not line:
            return None, False
        words = line.split()
        cid = ""
        if words[0].isdigit():
            cid, words = words[0], words[1:]
        if not words:
            return f"?{cid} unknown command\n\n", False
        name, args = words[0].lower(), words[1:]
        fn = self.commands.get(name)
        try:
            if fn is None:
                raise GtpError("unknown command")
            try:
                inspect.signature(fn).bind(*args)       # the argument count, before the call
            except TypeError:
                raise GtpError("syntax error")
            body = fn(*args) or ""
            out = f"={cid} {body}".rstrip(" ") if body else f"={cid}"
        except GtpError as e:
            out = f"?{cid} {e}"
        return out + "\n\n", name == "quit" and fn is not None

    def run(self, fin, fout):
        for line in fin:
            text, quit_ = self.handle(line)
            if text is not None:
                fout.write(text)
                fout.flush()
            if quit_:
                break

    # ------------------------------------------------------------------ administrative
    def cmd_protocol_version(self):
        return "2"

    def cmd_name(self):
        return self.NAME

    def cmd_version(self):
        return _VERSION

    def cmd_known_command(self, name):
        return "true" if name.lower() in self.commands else "false"

    def cmd_list_commands(self):
        return "\n".join(sorted(self.commands))

    def cmd_quit(self):
        return ""

    def cmd_time_settings(self, *_):
        return ""

    def cmd_time_left(self, *_):
        return ""

    # ------------------------------------------------------------------ set-up
    def cmd_boardsize(self, size):
        if not size.isdigit() or int(size) != BOARD:
            raise GtpError("unacceptable size")
        return ""

    def cmd_clear_board(self):
        self.game.clear()
        self.game_no += 1
        return ""

    def cmd_komi(self, komi):
        try:
            self.game.komi = float(komi)
        except ValueError:
            raise GtpError("syntax error")
        return ""

    # ------------------------------------------------------------------ play
    def cmd_play(self, colour, vtx):
        try:
            player, p = parse_colour(colour), parse_vertex(vtx)
        except ValueError:
            raise GtpError("syntax error")
        if p != PASS and self.game.legal_mask(player, suicide=False, superko=True,
                                              eye_fill=True)[p]:
            raise GtpError("illegal move")
        self.game.play(player, p)
        return ""

    def _generate(self, colour, commit: bool):
        try:
            player = parse_colour(colour)
        except ValueError:
            raise GtpError("syntax error")
        g = self.game
        try:
            p = choose_moves(self.predictor, [g], [self.game_no], self.rank, self.seed,
                             self.temperature, self.top_p, players=[player])[0]
        except NonFinitePolicy:
            raise GtpError("non-finite policy")
        if commit:
            g.play(player, p)
        return vertex(p)

    def cmd_genmove(self, colour):
        return self._generate(colour, True)

    def cmd_reg_genmove(self, colour):
        return self._generate(colour, False)

    def cmd_undo(self):
        if not self.game.undo():
            raise GtpError("cannot undo")
        return ""

    def cmd_final_score(self):
        return self.game.result()

    def cmd_showboard(self):
        s = self.game.stones()
        head = "   " + " ".join(COLUMNS)
        rows = [f"{BOARD - y:2d} " + " ".join(".XO"[int(s[x, y])] for x in range(BOARD))
                + f" {BOARD - y}" for y in range(BOARD)]
        side = "black" if self.game.to_move == 1 else "white"
        return "\n" + "\n".join([head, *rows, head, f"{side} to move, ply {self.game.ply}"])
