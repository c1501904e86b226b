"""Play without a GPU: the engine's live game (``_dgcpu.Game``), the selection oracle
(``play/select.py``), the GTP front end and self-play on ``device="cpu"``, and the ``_dgplay``
launcher's refusals (made before any GPU work).
"""
import glob
import io
import json
import os

import numpy as np
import pytest

from deep_go_amd.config import ExperimentConfig
from deep_go_amd.ops import native
from deep_go_amd.play.game import (PASS, Game, choose_moves, parse_vertex, sgf_point, vertex)
from deep_go_amd.play.gtp import GtpEngine
from deep_go_amd.play.select import nucleus, select_moves, select_uniform, tempered
from deep_go_amd.play.selfplay import moves_of, run_match

NP = 361
B, W = 1, 2


def pt(x, y):
    return 19 * x + y


@pytest.fixture(scope="module")
def eng():
    return native.cpu()


def build(eng, black=(), white=()):
    """A Game with the stones given as (x, y) lists, white first (nothing here is captured
    while it is set up)."""
    g = eng.Game()
    for x, y in white:
        g.play(W, x, y)
    for x, y in black:
        g.play(B, x, y)
    return g


def state(g):
    return (g.stones().tobytes(), g.ages().tobytes(), g.ko(), g.to_move, g.ply,
            g.last_was_pass, g.key())


# ------------------------------------------------------------------------------ engine
@pytest.fixture(scope="module")
def fixture_game(eng, ref_data):
    """(handicap, moves, game_positions rows with and without the ko mark) of one bundled game,
    truncated to 120 moves."""
    d = sorted(p for p in glob.glob(ref_data + "/test/*/*.sgf") if os.path.isdir(p))[0]
    n = min(120, len([f for f in os.listdir(d) if not f.startswith(".")]))
    planes, meta = eng.read_positions([f"{d}/{k}" for k in range(1, n + 1)], 4)
    moves = [(int(m[0]), int(m[1]) - 1, int(m[2]) - 1) for m in meta]
    handicap = [(int(planes[0, 0, x, y]), x, y) for x in range(19) for y in range(19)
                if planes[0, 0, x, y]]
    rows = {ko: np.asarray(eng.game_positions(handicap, moves, ko)) for ko in (False, True)}
    assert np.array_equal(rows[False], planes)
    return handicap, moves, rows


def test_game_planes_follow_game_positions_and_reach_the_last_position(eng, fixture_game):
    handicap, moves, rows = fixture_game
    g = eng.Game()
    for pl, x, y in handicap:
        g.play(pl, x, y)
    for k, (pl, x, y) in enumerate(moves):
        for ko in (False, True):
            assert np.array_equal(g.planes(ko), rows[ko][k]), (k, ko)
        assert g.ply == len(handicap) + k
        g.play(pl, x, y)
        assert g.to_move == 3 - pl and not g.last_was_pass
    # the position after the last move: its stone is there with age 1
    last = g.planes()
    pl, x, y = moves[-1]
    assert last.shape == (9, 19, 19) and last.dtype == np.uint8
    assert last[0, x, y] == pl and last[6, x, y] == 1
    assert np.array_equal(last[0], g.stones()) and np.array_equal(last[6], g.ages())
    # and it is what game_positions gives for one further move on an empty point
    ex, ey = np.argwhere(g.stones() == 0)[0]
    more = eng.game_positions(handicap, moves + [(3 - pl, int(ex), int(ey))], True)
    assert np.array_equal(g.planes(True), more[-1])


def test_undo_restores_everything_bit_for_bit(eng, fixture_game):
    handicap, moves, _ = fixture_game
    g = eng.Game()
    assert not g.undo() and g.ply == 0 and g.to_move == B
    trail = []
    for k, (pl, x, y) in enumerate(handicap + moves):
        before = state(g)
        trail.append(before)
        g.play(pl, x, y)
        assert state(g) != before
        assert g.undo() and state(g) == before
        if k % 17 == 5:                       # a pass in between, taken back too
            g.pass_(pl)
            assert g.last_was_pass and g.ko() == -1 and g.ply == before[4] + 1
            assert g.undo() and state(g) == before
        g.play(pl, x, y)
    for before in reversed(trail):            # all the way back
        assert g.undo() and state(g) == before
    assert not g.stones().any() and not g.ages().any() and g.key() == 0
    with pytest.raises(RuntimeError):
        g.play(B, 3, 3) or g.play(W, 3, 3)    # an occupied point
    assert g.ply == 1


def test_pass_ages_like_a_move_and_clears_ko(eng):
    g = build(eng, black=[(3, 3)])
    assert g.ages()[3, 3] == 1
    g.pass_(W)
    assert g.ages()[3, 3] == 2 and g.to_move == B and g.last_was_pass
    assert g.ages().sum() == 2 and g.stones().sum() == 1


def test_suicide_and_capture(eng):
    g = build(eng, white=[(0, 1), (1, 0)])
    assert g.legal_mask(B, suicide=False)[pt(0, 0)] != 0       # kills nothing, no liberty
    assert g.legal_mask(B, suicide=True, superko=False)[pt(0, 0)] == 0
    # (a one-stone suicide leaves the position as it is: a repeat under superko)
    assert g.legal_mask(B, suicide=True, superko=True)[pt(0, 0)] != 0
    assert g.legal_mask(W)[pt(0, 0)] == 0                      # white's own point
    # with the two white stones in atari the same point captures: not suicide
    g = build(eng, white=[(0, 1), (1, 0)], black=[(0, 2), (1, 1), (2, 0)])
    assert g.legal_mask(B, suicide=False)[pt(0, 0)] == 0
    g.play(B, 0, 0)
    assert g.stones()[0, 1] == 0 and g.stones()[1, 0] == 0 and g.stones()[0, 0] == B
    # occupied points are illegal whatever the flags
    m = g.legal_mask(W, suicide=True, superko=False, eye_fill=True)
    assert np.array_equal(m != 0, g.stones().reshape(-1) != 0)


KO_BLACK, KO_WHITE = [(3, 2), (2, 3), (4, 3)], [(3, 5), (2, 4), (4, 4), (3, 3)]


def test_simple_ko_and_its_release(eng):
    g = build(eng, black=KO_BLACK, white=KO_WHITE)
    g.play(B, 3, 4)                                            # takes the stone at (3, 3)
    assert g.stones()[3, 3] == 0 and g.ko() == pt(3, 3)
    for flags in (dict(), dict(superko=False), dict(suicide=True, superko=False)):
        assert g.legal_mask(W, **flags)[pt(3, 3)] != 0
    g.play(W, 10, 10)
    g.play(B, 10, 12)
    assert g.ko() == -1 and g.legal_mask(W)[pt(3, 3)] == 0     # released: no repeat either


def test_positional_superko_beyond_simple_ko(eng):
    g = build(eng, black=KO_BLACK, white=KO_WHITE)
    before = g.key()
    g.play(B, 3, 4)
    g.pass_(W)                                                 # the pass clears the ko point
    g.pass_(B)
    assert g.ko() == -1
    assert g.legal_mask(W, superko=False)[pt(3, 3)] == 0       # simple ko does not see it
    assert g.legal_mask(W, superko=True)[pt(3, 3)] != 0        # the position would repeat
    g.play(W, 3, 3)
    assert g.key() == before
    # only that point is affected
    g.undo()
    a, b = g.legal_mask(W, superko=False), g.legal_mask(W, superko=True)
    assert np.flatnonzero(a != b).tolist() == [pt(3, 3)]


def _ring(x, y, skip=()):
    """The on-board neighbours of (x, y), orthogonal and diagonal, without `skip`."""
    return [(x + dx, y + dy) for dx in (-1, 0, 1) for dy in (-1, 0, 1)
            if (dx or dy) and 0 <= x + dx < 19 and 0 <= y + dy < 19
            and (x + dx, y + dy) not in skip]


@pytest.mark.parametrize("x,y,spare,false_eye", [
    (10, 10, [(9, 9)], [(9, 9), (11, 11)]),      # centre: one diagonal may be missing, not two
    (0, 10, [], [(1, 9)]),                       # edge: none may
    (0, 0, [], [(1, 1)]),                        # corner: none may
])
def test_simple_eyes(eng, x, y, spare, false_eye):
    for skip, eye in (((), True), (tuple(spare), True), (tuple(false_eye), False)):
        g = build(eng, black=_ring(x, y, skip))
        fill = g.legal_mask(B, eye_fill=True)[pt(x, y)]
        nofill = g.legal_mask(B, eye_fill=False)[pt(x, y)]
        assert fill == 0
        assert (nofill != 0) == eye, (skip, eye)
        # the flag changes nothing else, and it is nobody's eye for white
        assert (g.legal_mask(B, eye_fill=False) != g.legal_mask(B, eye_fill=True)).sum() == eye
    # a white stone on the diagonal is as good as an empty one
    g = build(eng, black=_ring(x, y, tuple(false_eye)), white=false_eye[:1])
    assert g.legal_mask(B, eye_fill=False)[pt(x, y)] == 0
    # an orthogonal neighbour missing: no eye
    g = build(eng, black=_ring(x, y, ((x + 1, y),)))
    assert g.legal_mask(B, eye_fill=False)[pt(x, y)] == 0


WALLS = dict(black=[(3, y) for y in range(19)], white=[(10, y) for y in range(19)])


def test_tromp_taylor_scores(eng):
    assert eng.Game().score() == (0, 0)
    assert build(eng, black=[(3, 3)]).score() == (361, 0)
    # two walls: columns 0..3 black, 10..18 white, the six columns between reach both
    assert build(eng, **WALLS).score() == (4 * 19, 9 * 19)
    # a white stone inside black's side makes that region neutral as well
    g = build(eng, black=WALLS["black"], white=WALLS["white"] + [(1, 1)])
    assert g.score() == (19, 9 * 19 + 1)


# ------------------------------------------------------------------------------ oracle
def test_select_uniform_is_a_pure_hash_on_the_grid():
    g, p = np.meshgrid(np.arange(256), np.arange(256), indexing="ij")
    u = select_uniform(0, g, p)
    assert np.array_equal(u, select_uniform(0, g, p))
    assert u.shape == (256, 256) and (u >= 0).all() and (u < 1).all()
    assert np.array_equal(u * 2.0 ** 24, np.round(u * 2.0 ** 24))
    assert np.array_equal(u.astype(np.float32).astype(np.float64), u)      # exact in fp32
    base = select_uniform(5, 7, 9)
    for other in (select_uniform(6, 7, 9), select_uniform(5 + 2 ** 32, 7, 9),
                  select_uniform(5, 8, 9), select_uniform(5, 7, 10), select_uniform(5, 9, 7)):
        assert other != base
    # 65 536 draws in 16 equal bins: chi-square with 15 degrees of freedom, 99.9% quantile
    counts = np.bincount((u * 16).astype(int).ravel(), minlength=16)
    chi2 = float(((counts - 4096.0) ** 2 / 4096.0).sum())
    print(f"\nselect_uniform chi-square (16 bins, 65536 draws): {chi2:.3f}")
    assert chi2 < 37.697
    # the extension's host twin is the same function (no GPU needed: it runs on the host)
    m = native.play()
    for seed in (0, 5, 2 ** 63 + 11):
        for gm, pl in ((0, 0), (7, 9), (-1, 3), (2 ** 31 - 1, 399)):
            assert m.select_uniform(seed, gm, pl) == float(select_uniform(seed, gm, pl))


def _row(points, values):
    r = np.zeros(NP)
    r[list(points)] = values
    return r


def test_select_moves_temperature_zero_is_the_argmax():
    rows = np.stack([_row([300, 7, 150], [0.25, 0.5, 0.25]),
                     _row([300, 7, 150], [0.4, 0.2, 0.4]),       # tie: the lower index
                     np.full(NP, 1 / NP)])
    move, p, kept = select_moves(rows, [0, 1, 2], [0, 0, 0], temperature=0.0)
    assert move.tolist() == [7, 150, 0] and p.tolist() == [1, 1, 1] and kept.tolist() == [1, 1, 1]


def test_select_moves_samples_prob_itself():
    pts, pr = [3, 40, 41, 200, 360], [0.5, 0.25, 0.125, 0.0625, 0.0625]
    g, p = np.meshgrid(np.arange(256), np.arange(256), indexing="ij")
    move, pm, kept = select_moves(_row(pts, pr)[None], g.ravel(), p.ravel(), seed=3)
    assert (kept == 5).all()
    # the counts the draws imply: u in [0, .5) -> 3, [.5, .75) -> 40, ... (all sums exact)
    u = select_uniform(3, g.ravel(), p.ravel())
    want = np.asarray(pts)[np.searchsorted(np.cumsum(pr), u, side="right")]
    assert np.array_equal(move, want)
    assert np.array_equal(np.bincount(move, minlength=NP), np.bincount(want, minlength=NP))
    assert np.array_equal(pm, _row(pts, pr)[move])
    # and one row per key gives what the shared row gives
    m2 = select_moves(np.tile(_row(pts, pr), (50, 1)), g.ravel()[:50], p.ravel()[:50], seed=3)
    assert np.array_equal(m2[0], move[:50])


def test_select_moves_nucleus_by_hand():
    # w = .4 .3 .2 .1 at points 10, 5, 300, 7: above = 0, .4, .7, .9; top_p = .75 keeps the
    # first three (.7 < .75 <= .9), top_p = .4 the first only (above = .4 is not < .4)
    row = _row([10, 5, 300, 7], [0.4, 0.3, 0.2, 0.1])
    keep, above = nucleus(row, 0.75)
    assert np.flatnonzero(keep).tolist() == [5, 10, 300]
    assert np.allclose(above[[10, 5, 300, 7]], [0, 0.4, 0.7, 0.9], atol=1e-15)
    keys = np.arange(2000)
    move, pm, kept = select_moves(row[None], keys, keys * 0, top_p=0.75)
    assert (kept == 3).all() and set(move.tolist()) == {5, 10, 300}
    assert np.allclose(pm, (row / 0.9)[move], rtol=1e-15)
    move, pm, kept = select_moves(row[None], keys, keys * 0, top_p=0.4)
    assert (kept == 1).all() and (move == 10).all() and (pm == 1).all()
    # the temperature acts before the cut: T = 1/2 squares the weights (.16 .09 .04 .01 of .3)
    assert np.allclose(tempered(row, 0.5), row ** 2, rtol=1e-15)
    move, pm, kept = select_moves(row[None], keys, keys * 0, temperature=0.5, top_p=0.75)
    assert (kept == 2).all() and set(move.tolist()) == {5, 10}
    # ties rank by index: four equal weights, top_p = .5 keeps the two lowest points
    move, pm, kept = select_moves(_row([10, 5, 300, 7], 0.25)[None], keys, keys * 0, top_p=0.5)
    assert (kept == 2).all() and set(move.tolist()) == {5, 7}


def test_select_moves_empty_and_bad_rows():
    ok = _row([3], [1.0])
    nan, neg, inf = ok.copy(), ok.copy(), ok.copy()
    nan[17], neg[17], inf[17] = np.nan, -0.5, np.inf
    move, p, kept = select_moves(np.stack([np.zeros(NP), nan, ok, neg, inf]), np.arange(5),
                                 np.zeros(5, int), temperature=0.7, top_p=0.9)
    assert move.tolist() == [-1, -1, 3, -1, -1]
    assert p.tolist() == [0, 0, 1, 0, 0] and kept.tolist() == [0, -1, 1, -1, -1]
    # every tempered weight underflows: as T = 0
    move, p, kept = select_moves(_row([3, 9], [0.25, 0.75])[None], [0], [0], temperature=1e-4)
    assert (move[0], p[0], kept[0]) == (9, 1.0, 1)
    for kw in (dict(temperature=-1.0), dict(temperature=np.inf), dict(top_p=0.0),
               dict(top_p=1.5)):
        with pytest.raises(ValueError):
            select_moves(ok[None], [0], [0], **kw)


# ------------------------------------------------------------------------------ _dgplay
@pytest.fixture
def dgplay():
    return native.play()       # built without a GPU: a missing module is a failure


def test_dgplay_public_names(dgplay):
    assert sorted(x for x in dir(dgplay) if not x.startswith("_")) == [
        "policy_select", "select_uniform"]


#            prob game ply n  seed T    top_p move p_move kept stream
GOOD_ARGS = [64, 64, 64, 1, 0, 1.0, 1.0, 64, 0, 0, 0]


@pytest.mark.parametrize("what,index,value", [
    ("n < 0", 3, -1),
    ("null prob", 0, 0), ("null game", 1, 0), ("null ply", 2, 0), ("null move", 7, 0),
    ("T < 0", 5, -0.5), ("T nan", 5, float("nan")), ("T inf", 5, float("inf")),
    ("top_p = 0", 6, 0.0), ("top_p < 0", 6, -0.1), ("top_p > 1", 6, 1.0001),
    ("top_p nan", 6, float("nan")),
])
def test_policy_select_refuses_before_any_gpu_work(dgplay, what, index, value):
    args = list(GOOD_ARGS)
    args[index] = value
    with pytest.raises(RuntimeError) as e:
        dgplay.policy_select(*args)
    assert str(e.value) == "policy_select: invalid argument", what


def test_policy_select_with_no_rows_is_a_no_op(dgplay):
    args = list(GOOD_ARGS)
    args[3] = 0
    dgplay.policy_select(*args)        # valid arguments, n = 0: returns before any launch


# ------------------------------------------------------------------------------ GTP
TINY = ExperimentConfig(numLayers=3, channelSize=16, batchSize=16, seed=3)


def tiny_predictor(device="cpu", cfg=TINY, batch=16, scale=1.0):
    """scale: the random weights times that (a large one makes the policy peaked, so that two
    predictors choose differently on the same draw)."""
    from deep_go_amd.models.gocnn import ParamLayout, init_params
    from deep_go_amd.predict import Predictor
    flat = init_params(ParamLayout(cfg), cfg.seed) * scale
    return Predictor(cfg, flat, batch=batch, symmetries=8, device=device, top=1)


@pytest.fixture(scope="module")
def pred():
    return tiny_predictor()


def session(engine, text):
    """Run a scripted session; -> the list of responses (without the trailing blank line)."""
    out = io.StringIO()
    engine.run(io.StringIO(text), out)
    return out.getvalue().split("\n\n")[:-1]


def on_board(shown, ch):
    """How often ch is in the 19 board rows of a showboard answer (not its column letters)."""
    rows = [ln for ln in shown.splitlines() if ln[:2].strip().isdigit()]
    assert len(rows) == 19
    return sum(ln[3:-3].count(ch) for ln in rows)


def almost_full(eye_a=(0, 0), eye_b=(18, 18), hole=None):
    """GTP play lines: black on every point but two eyes (and `hole`, if given, with a white
    stone below it whose last liberty it is)."""
    lines = []
    skip = {eye_a, eye_b}
    if hole:
        lines.append(f"play w {vertex(pt(hole[0], hole[1] + 1))}")
        skip |= {hole, (hole[0], hole[1] + 1)}
    lines += [f"play b {vertex(pt(x, y))}" for x in range(19) for y in range(19)
              if (x, y) not in skip]
    return "\n".join(lines) + "\n"


def test_vertices():
    assert vertex(pt(15, 3)) == "Q16" and parse_vertex("q16") == pt(15, 3)
    assert sgf_point(pt(15, 3)) == "pd"
    assert vertex(pt(0, 18)) == "A1" and vertex(pt(18, 0)) == "T19" and vertex(pt(8, 0)) == "J19"
    assert vertex(PASS) == "pass" and parse_vertex("PASS") == PASS
    assert all(parse_vertex(vertex(p)) == p for p in range(NP))
    for bad in ("I5", "A0", "A20", "U3", "Q", "16", ""):
        with pytest.raises(ValueError):
            parse_vertex(bad)


def test_gtp_administrative_commands(pred):
    e = GtpEngine(pred)
    r = session(e, "protocol_version\n7 name\n\n# a comment\n8 version # trailing\n"
                   "known_command genmove\n9 known_command frobnicate\nfrobnicate\n"
                   "12 frobnicate 3\nlist_commands\nboardsize 19\n3 boardsize 13\n"
                   "time_settings 0 5 1\n4 time_left b 30 0\nkomi 6.5\n5 quit\nname\n")
    assert r[:8] == ["= 2", "=7 deep_go_amd", "=8 0.1.0", "= true", "=9 false",
                     "? unknown command", "?12 unknown command",
                     "= " + "\n".join(sorted(e.commands))]
    assert set(e.commands) == {
        "protocol_version", "name", "version", "known_command", "list_commands", "quit",
        "boardsize", "clear_board", "komi", "play", "genmove", "reg_genmove", "undo",
        "showboard", "final_score", "time_settings", "time_left"}
    assert r[8:] == ["=", "?3 unacceptable size", "=", "=4", "=", "=5"]   # nothing after quit
    assert e.game.komi == 6.5


def test_gtp_play_undo_showboard(pred):
    e = GtpEngine(pred)
    r = session(e, "1 play black Q16\n2 showboard\n3 play w q16\n4 play w D4\n5 showboard\n"
                   "6 undo\n7 showboard\n8 play w pass\n9 undo\n10 undo\n11 undo\n"
                   "12 play b Z3\n13 play b\n")
    assert r[0] == "=1" and r[2] == "?3 illegal move" and r[3] == "=4"
    assert e.game.ply == 0
    board1, board2, board3 = r[1][3:], r[4][3:], r[6][3:]
    assert board1 == board3 and board1 != board2
    assert board1.splitlines()[5] == "16 " + " ".join("X" if c == "Q" else "." for c in
                                                     "ABCDEFGHJKLMNOPQRST") + " 16"
    assert on_board(board2, "O") == 1 and on_board(board2, "X") == 1
    assert r[7:] == ["=8", "=9", "=10", "?11 cannot undo", "?12 syntax error",
                     "?13 syntax error"]
    # suicide and the ko point are illegal too
    e = GtpEngine(pred)
    r = session(e, "play w A18\nplay w B19\nplay b A19\n"
                   + "".join(f"play b {vertex(pt(x, y))}\n" for x, y in KO_BLACK)
                   + "".join(f"play w {vertex(pt(x, y))}\n" for x, y in KO_WHITE)
                   + f"play b {vertex(pt(3, 4))}\nplay w {vertex(pt(3, 3))}\n")
    assert r[2] == "? illegal move" and r[-2] == "=" and r[-1] == "? illegal move"


def test_gtp_genmove_single_candidate_and_none(pred):
    e = GtpEngine(pred, temperature=0.0)
    r = session(e, almost_full(hole=(9, 9)) + "reg_genmove b\nshowboard\ngenmove b\nshowboard\n"
                   "genmove w\ngenmove b\nfinal_score\n")
    assert all(x == "=" for x in r[:-7])
    # the only candidate: not an eye (a white stone beside it), and it captures that stone
    assert r[-7] == "= K10" and r[-5] == "= K10"
    assert r[-6] != r[-4] and on_board(r[-6], "O") == 1 and on_board(r[-4], "O") == 0
    # then nobody has a candidate: white's points are suicide, black's are its eyes
    assert r[-3] == "= pass" and r[-2] == "= pass" and e.game.over
    assert r[-1] == "= B+353.5"
    # out of turn, on the board without the hole
    e = GtpEngine(pred)
    r = session(e, "clear_board\n" + almost_full() + "genmove b\ngenmove b\n")
    assert r[-2:] == ["= pass", "= pass"] and e.game_no == 1


def test_gtp_final_score_and_the_pass_rule(pred):
    e = GtpEngine(pred)
    lines = "".join(f"play b {vertex(pt(*p))}\n" for p in WALLS["black"]) + "".join(
        f"play w {vertex(pt(*p))}\n" for p in WALLS["white"])
    r = session(e, lines + "final_score\nplay b pass\ngenmove w\nkomi 0\nfinal_score\n"
                           "clear_board\nfinal_score\nkomi 0.5\nfinal_score\n")
    # 76 black, 171 white: W+102.5; white is ahead after black's pass, so it passes too
    assert r[-9:] == ["= W+102.5", "=", "= pass", "=", "= W+95", "=", "= 0", "=", "= W+0.5"]
    # behind after the opponent's pass, the engine plays on
    e = GtpEngine(pred)
    r = session(e, lines + "play w pass\ngenmove b\n")
    assert r[-1] not in ("= pass", "= resign") and r[-1].startswith("= ")
    # its own pass is not the opponent's: white, ahead, asked again out of turn, plays on
    e = GtpEngine(pred)
    r = session(e, lines + "play w pass\ngenmove w\n")
    assert e.game.to_move == B and r[-1] != "= pass" and r[-1].startswith("= ")


def test_gtp_reports_a_non_finite_policy():
    class Broken:
        cfg = TINY

        def select(self, planes, *a, **kw):
            from deep_go_amd.predict import Selection
            n = len(planes)
            return Selection(np.full(n, -1, np.int32), np.zeros(n), np.full(n, -1, np.int32))

    e = GtpEngine(Broken())
    assert session(e, "5 genmove b\n") == ["?5 non-finite policy"]
    assert e.game.ply == 0


def test_gtp_syntax_errors_are_argument_counts_only(pred):
    e = GtpEngine(pred)
    assert session(e, "1 play b\n2 genmove\n3 komi\n4 boardsize 19 19\n5 undo now\n") == [
        "?1 syntax error", "?2 syntax error", "?3 syntax error", "?4 syntax error",
        "?5 syntax error"]

    class Buggy:
        cfg = TINY

        def select(self, *a, **kw):
            raise TypeError("a bug inside the predictor")

    with pytest.raises(TypeError, match="a bug inside"):     # not answered as a syntax error
        GtpEngine(Buggy()).handle("genmove b\n")


def test_predictor_select_on_cpu_matches_predict_and_the_oracle(pred, eng):
    g = build(eng, black=KO_BLACK, white=KO_WHITE)
    planes = np.stack([g.planes(), eng.Game().planes()])
    extra = np.zeros((2, NP), np.uint8)
    extra[1, :200] = 1
    player, rank = np.array([1, 2], np.uint8), np.array([9, 9], np.uint8)
    r = pred.predict(planes, player, rank, extra_illegal=extra)
    s = pred.select(planes, player, rank, extra, game=[0, 1], ply=[7, 0], temperature=0.0)
    assert np.array_equal(s.move, r.topk[:, 0]) and (s.kept == 1).all() and (s.p == 1).all()
    s = pred.select(planes, player, rank, extra, game=[4, 5], ply=[7, 0], seed=9,
                    temperature=0.8, top_p=0.9)
    want = select_moves(r.prob, [4, 5], [7, 0], 9, 0.8, 0.9)
    for got, ref in zip((s.move, s.p, s.kept), want):
        assert np.array_equal(got, ref)
    assert (r.prob[np.arange(2), s.move] > 0).all()
    for kw in (dict(temperature=-1.0), dict(top_p=0.0)):
        with pytest.raises(ValueError):
            pred.select(planes, player, rank, game=[0, 1], ply=[0, 0], **kw)


# ------------------------------------------------------------------------------ self-play
def replay(eng, sgf_text, moves, setup=0):
    """Every move legal by a replay of its own through the engine (the first `setup` moves are
    the given position: only placed); -> the final Game."""
    g = eng.Game()
    for k, (pl, p) in enumerate(moves):
        if k >= setup:
            assert pl == g.to_move
        if p == PASS:
            g.pass_(pl)
            continue
        if k >= setup:
            assert g.legal_mask(pl, suicide=False, superko=True, eye_fill=False)[p] == 0
        g.play(pl, p // 19, p % 19)
    stones = [(pl, p // 19, p % 19) for pl, p in moves if p != PASS]
    assert moves_of(sgf_text) == stones
    return g


def test_selfplay_on_cpu(pred, eng, tmp_path):
    r = run_match(pred, games=2, max_moves=12, seed=4, out_dir=str(tmp_path / "a"))
    r2 = run_match(pred, games=2, max_moves=12, seed=4, out_dir=str(tmp_path / "b"))
    assert sorted(r) == ["moves", "sgf", "summary", "timing"]
    assert all(r2[k] == r[k] for k in ("moves", "sgf", "summary"))
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == ["game_0000.sgf", "game_0001.sgf", "summary.json"]
    for nm in names:
        assert (tmp_path / "a" / nm).read_bytes() == (tmp_path / "b" / nm).read_bytes()
    assert json.loads((tmp_path / "a" / "summary.json").read_text()) == r["summary"]
    for i, (text, moves) in enumerate(zip(r["sgf"], r["moves"])):
        assert len(moves) == 12 and (tmp_path / "a" / names[i]).read_text() == text
        replay(eng, text, moves)
    assert r["moves"][0] != r["moves"][1]         # the game index keys the draws
    s = r["summary"]
    assert [g["moves"] for g in s["per_game"]] == [12, 12]
    assert [g["result"] for g in s["per_game"]] == ["Void", "Void"]
    assert s["wins"] == {"B": 0, "W": 0, "draw": 0, "void": 2} and s["mean_score"] is None
    assert "timing" not in s and r["timing"]["plies"] == 24
    # another seed plays other games
    assert run_match(pred, games=2, max_moves=12, seed=5)["sgf"] != r["sgf"]


def test_selfplay_cli_writes_files_that_depend_on_the_arguments_alone(tmp_path, capsys):
    from deep_go_amd import cli
    from deep_go_amd.models.gocnn import ParamLayout, init_params
    from deep_go_amd.utils import checkpoint as ck
    path = str(tmp_path / "tiny.model")
    ck.save_checkpoint(path, TINY, init_params(ParamLayout(TINY), 3), {"id": "tiny"},
                       {"kind": "sgd", "rate": 0.1, "rate_decay": 0.0})
    for tag in "ab":
        assert cli.main(["selfplay", path, "--games", "2", "--max-moves", "4", "--device", "cpu",
                         "--batch", "16", "--seed", "3", "--out", str(tmp_path / tag)]) == 0
    printed = [json.loads(ln) for ln in capsys.readouterr().out.splitlines()]
    assert len(printed) == 2 and all(p["timing"]["plies"] == 8 for p in printed)
    for nm in ("game_0000.sgf", "game_0001.sgf", "summary.json"):
        assert (tmp_path / "a" / nm).read_bytes() == (tmp_path / "b" / nm).read_bytes()
    assert "timing" not in json.loads((tmp_path / "a" / "summary.json").read_text())


def test_match_on_cpu_alternates_colours(pred, eng):
    other = tiny_predictor(cfg=TINY.replace(seed=4), scale=8.0)
    r = run_match(pred, other, games=3, max_moves=7, seed=1)
    for i, (text, moves, meta) in enumerate(zip(r["sgf"], r["moves"],
                                                r["summary"]["per_game"])):
        assert len(moves) == 7                       # one move per game and ply
        replay(eng, text, moves)
        assert (meta["black"], meta["white"]) == (("a", "b") if i % 2 == 0 else ("b", "a"))
        assert f"PB[{meta['black']}]" in text and f"PW[{meta['white']}]" in text
    assert r["summary"]["wins"] == {"B": 0, "W": 0, "a": 0, "b": 0, "draw": 0, "void": 3}
    # the predictors differ, and each game asks the one that holds the colour to move
    solo = run_match(pred, games=3, max_moves=7, seed=1)
    assert solo["moves"][0][0] == r["moves"][0][0]   # a opens game 0 alike
    assert solo["moves"] != r["moves"]


def _full_but_two_eyes(colour):
    return [(colour, pt(x, y)) for x in range(19) for y in range(19)
            if (x, y) not in ((0, 0), (18, 18))]


def test_finished_games_are_scored_and_counted(pred, eng):
    """Positions with nothing left to play: both sides pass at once, so the games finish and
    run_match's results, wins per colour and per predictor, draws and mean score are real."""
    other = tiny_predictor(cfg=TINY.replace(seed=4), scale=8.0)
    n = 359
    # black owns the board: white has only suicides, black only its eyes
    r = run_match(pred, other, games=4, max_moves=10, seed=1, setup=_full_but_two_eyes(B))
    for i, (text, moves, meta) in enumerate(zip(r["sgf"], r["moves"],
                                                r["summary"]["per_game"])):
        assert moves[n:] == [(W, PASS), (B, PASS)] and meta["moves"] == n + 2
        g = replay(eng, text, moves, setup=n)
        assert g.score() == (361, 0) and meta["result"] == "B+353.5"
        assert "RE[B+353.5]" in text and text.count(";W[]") == 1 and text.count(";B[]") == 1
    s = r["summary"]
    assert s["wins"] == {"B": 4, "W": 0, "a": 2, "b": 2, "draw": 0, "void": 0}
    assert s["mean_score"] == 353.5 and r["timing"]["plies"] == 8
    # white owns it: the holder of white wins, b in game 0 and a in game 1
    r = run_match(pred, other, games=3, max_moves=10, komi=0.5, setup=_full_but_two_eyes(W))
    s = r["summary"]
    assert [g["result"] for g in s["per_game"]] == ["W+361.5"] * 3
    assert s["wins"] == {"B": 0, "W": 3, "a": 1, "b": 2, "draw": 0, "void": 0}
    assert s["mean_score"] == -361.5
    # a komi that evens the score: a draw for nobody; one predictor: no per-predictor counts
    r = run_match(pred, games=2, max_moves=10, komi=361, setup=_full_but_two_eyes(B))
    s = r["summary"]
    assert [g["result"] for g in s["per_game"]] == ["0", "0"] and "RE[0]" in r["sgf"][0]
    assert s["wins"] == {"B": 0, "W": 0, "draw": 2, "void": 0} and s["mean_score"] == 0
    # max_moves counts the match's plies, not the setup's: one ply leaves the games unfinished
    r = run_match(pred, games=1, max_moves=1, setup=_full_but_two_eyes(B))
    assert r["summary"]["per_game"][0]["result"] == "Void" and len(r["moves"][0]) == n + 1


def test_choose_moves_does_not_depend_on_the_batch(pred):
    games = [Game() for _ in range(3)]
    games[1].play(B, pt(3, 3))
    games[2].play(B, pt(15, 15))
    games[2].play(W, pt(3, 15))
    all3 = choose_moves(pred, games, [0, 1, 2], 9, 1, 1.0, 1.0)
    for k in range(3):
        assert choose_moves(pred, [games[k]], [k], 9, 1, 1.0, 1.0) == [all3[k]]
