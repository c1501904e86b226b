"""Play on the GPU: policy_select (csrc/kernels/play.hip) against the float64 oracle
play/select.py, Predictor.select against predict(), and the GTP engine and self-play on
``device="gpu"``.

The bound DELTA is counted, not fitted.  In units of 2^-24 (one fp32 rounding is at most half
of that, relative):

* W, above and c are sums of at most 361 non-negative fp32 terms: at most 361 each, 3 * 361;
* w = expf(logf(prob) / T): logf within 2, the division and the rounding of the quotient 1,
  together 3 relative to the exponent x = log(prob) / T, that is 3 |x| absolute in x and so
  3 |x| relative in w; expf itself 2.  |x| <= L = |log(smallest positive prob in this file)| /
  (smallest T > 0 in this file);
* the products top_p * W and u * Wk and the quotient w / Wk: 3.

DELTA = 2 * (3 * 361 + 3 L + 2 + 3) * 2^-24, the count doubled as tests/test_predict_gpu.py and
the head tests double theirs.  The rows are chosen (on the CPU, from the oracle alone) so that
no point's ``above`` is within DELTA * W of the nucleus threshold: membership is then never a
rounding question, and ``kept`` must match exactly.
"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from deep_go_amd.data.symmetry import ensemble_policy
from deep_go_amd.config import ExperimentConfig
from deep_go_amd.play.game import PASS, vertex
from deep_go_amd.play.gtp import GtpEngine
from deep_go_amd.play.select import nucleus, select_moves, select_uniform, tempered
from deep_go_amd.play.selfplay import moves_of, run_match

pytestmark = pytest.mark.gpu

NP = 361
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONFIGS = [(0.0, 1.0), (1.0, 1.0), (0.5, 1.0), (2.0, 0.9), (1.0, 0.5), (0.25, 0.3)]
T_MIN = min(T for T, _ in CONFIGS if T > 0)
LOGIT_SPAN = 0.4          # logits uniform in [-0.4, 0.4]: prob >= exp(-0.8) / 361
L = (0.8 + np.log(NP)) / T_MIN
DELTA = 2 * (3 * 361 + 3 * L + 2 + 3) * 2.0 ** -24
SENTINEL = 0x5A5A5A5A
B = 16                    # boards per forward: chunks of 2 positions x 8 symmetries


def _cfg(channels, dtype="bf16"):
    """The smallest nets tests/test_predict_gpu.py builds."""
    return ExperimentConfig(numLayers=4, channelSize=channels, head_relu=False, batchSize=B,
                            dtype=dtype, seed=11)
KINDS = (361, 40, 2, 1, 0, "nan", "ties")
SEED = 20


def _clear_of_the_threshold(row):
    """No point's `above` within DELTA * W of top_p * W, for every configuration."""
    for T, top_p in CONFIGS:
        if T == 0 or not (row > 0).any():
            continue
        w = tempered(row, T)
        _, above = nucleus(w, top_p)
        if (np.abs(above - top_p * w.sum())[w > 0] <= DELTA * w.sum()).any():
            return False
    return True


def _make_row(kind, index):
    """One prob row [361] (fp32) and its logits / legal mask: ensemble_policy's output for
    uniform logits on `kind` legal points; "ties": 37 equal points; "nan": a 40-point row with
    a NaN entry (prob only).  Candidates are drawn until one is clear of every threshold."""
    for attempt in range(200):
        rng = np.random.default_rng([index, attempt, 7])
        k = {"nan": 40, "ties": 37}.get(kind, kind)
        legal = np.zeros(NP, bool)
        legal[rng.permutation(NP)[:k]] = True
        z = rng.uniform(-LOGIT_SPAN, LOGIT_SPAN, NP)
        if kind == "ties":
            z[:] = 0.25
        z = z - np.log(np.exp(z).sum())
        logp = z.astype(np.float32)
        prob = ensemble_policy(logp[None, None], legal[None], 1)[0][0].astype(np.float32)
        if _clear_of_the_threshold(prob.astype(np.float64)):
            return prob, logp, legal
    raise AssertionError(f"no clear row of kind {kind}")


@pytest.fixture(scope="module")
def rows():
    """70 rows cycling through KINDS (ten of each), built once."""
    made = [_make_row(KINDS[i % len(KINDS)], i) for i in range(70)]
    prob = np.stack([m[0] for m in made])
    nan_rows = np.array([KINDS[i % len(KINDS)] == "nan" for i in range(70)])
    prob[nan_rows, 17] = np.nan
    pos = prob[np.isfinite(prob) & (prob > 0)]
    assert pos.min() >= np.exp(-0.8) / NP * (1 - 1e-6)        # what L assumes
    rng = np.random.default_rng(1)
    return dict(prob=prob, logp=np.stack([m[1] for m in made]),
                legal=np.stack([m[2] for m in made]), nan=nan_rows,
                game=rng.integers(0, 1000, 70).astype(np.int32),
                ply=rng.integers(0, 400, 70).astype(np.int32))


def _launch(prob, game, ply, T, top_p, seed=SEED):
    """policy_select with every output between sentinel runs; -> (move, p_move, kept) numpy."""
    from deep_go_amd.ops.native import play, stream_handle
    n, pad = len(prob), 37
    buf = torch.full((4 * pad + 3 * n,), SENTINEL, dtype=torch.int32, device="cuda")
    offs = [pad, 2 * pad + n, 3 * pad + 2 * n]
    d = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (prob, game, ply)]
    play().policy_select(d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), n, seed, T, top_p,
                         *(buf[o:].data_ptr() for o in offs), stream_handle())
    torch.cuda.synchronize()
    got = buf.cpu().numpy()
    keep = np.ones(len(got), bool)
    for o in offs:
        keep[o:o + n] = False
    assert (got[keep] == SENTINEL).all()
    move, p, kept = (got[o:o + n] for o in offs)
    return move.copy(), p.view(np.float32).copy(), kept.copy()


@pytest.mark.parametrize("T,top_p", CONFIGS[1:])
@pytest.mark.parametrize("n", [1, 3, 70])
def test_policy_select_vs_oracle(rows, n, T, top_p):
    # n = 1: a full row; n = 3: 361, 40 and 2 legal points; n = 70: every kind
    prob, game, ply = rows["prob"][:n], rows["game"][:n], rows["ply"][:n]
    finite = np.isfinite(prob).all(1)
    for row in prob[finite].astype(np.float64):               # the precondition, every launch
        if (row > 0).any():
            w = tempered(row, T)
            _, above = nucleus(w, top_p)
            assert (np.abs(above - top_p * w.sum())[w > 0] > DELTA * w.sum()).all()
    move, p, kept = _launch(prob, game, ply, T, top_p)
    ref_move, ref_p, ref_kept = select_moves(prob, game, ply, SEED, T, top_p)
    assert np.array_equal(kept, ref_kept)
    dead = ref_kept <= 0
    assert (move[dead] == -1).all() and (p[dead] == 0).all()
    u = select_uniform(SEED, game, ply)
    worst_p = worst_u = 0.0
    for i in np.flatnonzero(~dead):
        w = tempered(prob[i].astype(np.float64), T)
        keep, _ = nucleus(w, top_p)
        m = int(move[i])
        assert 0 <= m < NP and keep[m], i
        c = np.cumsum(np.where(keep, w, 0.0))
        lo, hi = (c[m] - w[m]) / c[-1], c[m] / c[-1]
        miss = max(lo - u[i], u[i] - hi, 0.0)
        worst_u = max(worst_u, miss / DELTA)
        ref_pm = w[m] / c[-1]           # (the oracle's p_move, had it drawn this point)
        worst_p = max(worst_p, abs(float(p[i]) - ref_pm) / ref_pm / DELTA)
    print(f"\npolicy_select n={n} T={T} top_p={top_p}: p_move error / DELTA = {worst_p:.4f}, "
          f"u outside the interval / DELTA = {worst_u:.4f} (DELTA = {DELTA:.3e}); "
          f"{int((move != ref_move).sum())} of {n} moves differ from the oracle's")
    assert worst_u <= 1 and worst_p <= 1
    # bit-reproducible from run to run
    again = _launch(prob, game, ply, T, top_p)
    for a, b in zip((move, p, kept), again):
        assert a.tobytes() == b.tobytes()


@pytest.mark.parametrize("n", [1, 3, 70])
def test_policy_select_temperature_zero_is_policy_ensembles_top1(rows, n):
    from deep_go_amd.ops import functional as F
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    r = F.policy_ensemble(t(rows["logp"][:n]), t((~rows["legal"][:n]).astype(np.uint8)), None,
                          None, S=1, K=1)
    torch.cuda.synchronize()
    prob = r["prob"].cpu().numpy()
    top1 = r["topk"].cpu().numpy()[:, 0]
    nan = rows["nan"][:n]
    prob[nan, 17] = np.nan
    move, p, kept = _launch(prob, rows["game"][:n], rows["ply"][:n], 0.0, 1.0)
    assert np.array_equal(move[~nan], top1[~nan]) and (move[nan] == -1).all()
    assert (top1 >= 0).sum() >= min(n, 3)
    ok = move >= 0
    assert (p[ok] == 1).all() and (kept[ok] == 1).all() and (p[~ok] == 0).all()
    assert np.array_equal(kept[~ok], np.where(nan[~ok], -1, 0))
    ref = select_moves(prob, rows["game"][:n], rows["ply"][:n], SEED, 0.0, 1.0)
    assert np.array_equal(move, ref[0]) and np.array_equal(kept, ref[2])


# ------------------------------------------------------------------------------ the nets
_predictors = {}


def _predictor(channels, dtype="bf16"):
    from deep_go_amd.predict import Predictor
    key = (channels, dtype)
    if key not in _predictors:
        _predictors[key] = Predictor(_cfg(channels, dtype), batch=B, symmetries=8, device="gpu",
                                     top=5)
    return _predictors[key]


@pytest.fixture(scope="module", autouse=True)
def _free_predictors():
    yield
    _predictors.clear()


@pytest.fixture(scope="module")
def positions(packed_fixture):
    d = np.load(os.path.join(packed_fixture, "test.dgpack.npz"))
    sel = np.linspace(0, len(d["label"]) - 1, 70).astype(int)
    return (np.ascontiguousarray(d["planes"][sel].reshape(-1, 9, 19, 19)), d["player"][sel],
            d["rank"][sel])


def test_predictor_select_chunks_equal_one_kernel_call(positions):
    from deep_go_amd.play.kernel import policy_select
    planes, player, rank = positions
    p = _predictor(64)
    assert p.chunk == 2                                        # 35 chunks
    extra = np.zeros((70, NP), np.uint8)
    extra[::3, 100:200] = 1
    game = np.arange(70, dtype=np.int32) * 3
    ply = (np.arange(70, dtype=np.int32) * 7) % 300
    sel = p.select(planes, player, rank, extra, game=game, ply=ply, seed=5, temperature=0.8,
                   top_p=0.95)
    prob = p.predict(planes, player, rank, extra_illegal=extra).prob
    assert prob.dtype == np.float32
    move, pm, kept = policy_select(torch.from_numpy(prob).cuda(), torch.from_numpy(game).cuda(),
                                   torch.from_numpy(ply).cuda(), 5, 0.8, 0.95)
    torch.cuda.synchronize()
    assert sel.move.tobytes() == move.cpu().numpy().tobytes()
    assert sel.p.tobytes() == pm.cpu().numpy().tobytes()
    assert sel.kept.tobytes() == kept.cpu().numpy().tobytes()
    assert (sel.move >= 0).all() and (prob[np.arange(70), sel.move] > 0).all()
    again = p.select(planes, player, rank, extra, game=game, ply=ply, seed=5, temperature=0.8,
                     top_p=0.95)
    for f in ("move", "p", "kept"):
        assert getattr(sel, f).tobytes() == getattr(again, f).tobytes()
    assert len(set(sel.move.tolist())) > 10


@pytest.mark.parametrize("channels,dtype", [(64, "bf16"), (128, "fp8")])
def test_predictor_select_at_temperature_zero_is_predicts_top1(positions, channels, dtype):
    planes, player, rank = (a[:5] for a in positions)
    p = _predictor(channels, dtype)
    ko = np.zeros((5, NP), np.uint8)
    ko[1, np.flatnonzero(planes[1, 0].reshape(-1) == 0)[4]] = 1
    before = p.predict(planes, player, rank, extra_illegal=ko)
    sel = p.select(planes, player, rank, ko, game=np.arange(5), ply=np.zeros(5), temperature=0)
    after = p.predict(planes, player, rank, extra_illegal=ko)
    assert np.array_equal(sel.move, before.topk[:, 0])
    assert (sel.kept == 1).all() and (sel.p == 1).all()
    for f in ("prob", "topk", "topk_p", "rank"):
        assert torch.equal(torch.from_numpy(getattr(before, f)),
                           torch.from_numpy(getattr(after, f))), f


def test_predict_alone_never_imports_dgplay():
    code = ("import sys, numpy as np\n"
            f"sys.path.insert(0, {ROOT!r})\n"
            "from deep_go_amd.config import ExperimentConfig\n"
            "from deep_go_amd.predict import Predictor\n"
            "cfg = ExperimentConfig(numLayers=4, channelSize=64, head_relu=False, batchSize=16,"
            " seed=11)\n"
            "p = Predictor(cfg, batch=16, symmetries=8, device='gpu', top=5)\n"
            "r = p.predict(np.zeros((3, 9, 19, 19), np.uint8), [1, 2, 1], [9, 9, 9])\n"
            "assert r.topk.shape == (3, 5) and (r.topk >= 0).all()\n"
            "assert '_dghip' in sys.modules and '_dgplay' not in sys.modules\n"
            "p.select(np.zeros((1, 9, 19, 19), np.uint8), [1], [9], game=[0], ply=[0])\n"
            "assert '_dgplay' in sys.modules\n"
            "print('ok')\n")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stderr[-2000:]


# ------------------------------------------------------------------------------ GTP
def test_gtp_genmoves_at_temperature_zero_follow_predict():
    p = _predictor(64)
    e = GtpEngine(p, temperature=0.0)
    assert e.handle("clear_board\n")[0] == "=\n\n"
    for k in range(10):
        player = 1 + k % 2
        g = e.game
        mask = g.candidates(player)
        assert mask is not None
        want = p.predict(g.planes(bool(p.cfg.ko_plane))[None], [player], [9],
                         extra_illegal=mask[None]).topk[0, 0]
        out, _ = e.handle(f"{k} genmove {'bw'[k % 2]}\n")
        assert out == f"={k} {vertex(int(want))}\n\n"
        assert g.ply == k + 1 and g.stones().reshape(-1)[want] == player


# ------------------------------------------------------------------------------ self-play
def _replay(text, moves, setup=0):
    """Every move legal by an independent replay through the engine (the first `setup` moves
    are the given position: only placed), and the SGF holds the same stones; -> the Game."""
    from deep_go_amd.ops.native import cpu
    g = cpu().Game()
    for k, (pl, p) in enumerate(moves):
        if k >= setup:
            assert pl == g.to_move
        if p == PASS:
            g.pass_(pl)
            continue
        if k >= setup:
            assert g.legal_mask(pl, suicide=False, superko=True, eye_fill=False)[p] == 0
        g.play(pl, p // 19, p % 19)
    assert moves_of(text) == [(pl, p // 19, p % 19) for pl, p in moves if p != PASS]
    return g


def _check_match(r, games, names, setup=0, finished=False):
    for i, (text, moves, meta) in enumerate(zip(r["sgf"], r["moves"],
                                                r["summary"]["per_game"])):
        g = _replay(text, moves, setup)
        assert meta["moves"] == len(moves) and (meta["black"], meta["white"]) == names(i)
        over = len(moves) >= 2 and moves[-1][1] == PASS and moves[-2][1] == PASS
        assert over == finished
        if over:                       # a finished game's result is the engine's score
            b, w = g.score()
            m = b - w - 7.5
            assert meta["result"] == f"{'B' if m > 0 else 'W'}+{abs(m):g}"
            assert f"RE[{meta['result']}]" in text
        else:
            assert meta["result"] == "Void" and len(moves) == setup + 30
    assert len(r["sgf"]) == games


def _run(tmp_path, tag, *preds, games, **kw):
    return run_match(*preds, games=games, max_moves=30, seed=2, temperature=1.0,
                     out_dir=str(tmp_path / tag), **kw)


def test_selfplay_on_the_gpu(tmp_path):
    p = _predictor(64)
    a = _run(tmp_path, "a", p, games=8)
    b = _run(tmp_path, "b", p, games=8)
    assert all(a[k] == b[k] for k in ("sgf", "moves", "summary"))
    for nm in sorted(os.listdir(tmp_path / "a")):
        assert (tmp_path / "a" / nm).read_bytes() == (tmp_path / "b" / nm).read_bytes()
    _check_match(a, 8, lambda i: ("a", "a"))
    assert len({tuple(m) for m in a["moves"]}) == 8            # eight different games


ALTERNATING = lambda i: ("a", "b") if i % 2 == 0 else ("b", "a")      # noqa: E731
# black on every point but its two eyes and two adjacent empty points in the centre: a few
# real moves are left (white into the gap, black's capture), then both sides pass
ENDGAME = [(1, 19 * x + y) for x in range(19) for y in range(19)
           if (x, y) not in ((0, 0), (18, 18), (9, 9), (9, 10))]


def test_match_on_the_gpu_alternates_colours(tmp_path):
    pa, pb = _predictor(64), _predictor(128)
    a = _run(tmp_path, "a", pa, pb, games=4)
    b = _run(tmp_path, "b", pa, pb, games=4)
    assert a["sgf"] == b["sgf"]
    _check_match(a, 4, ALTERNATING)
    assert a["summary"]["wins"] == {"B": 0, "W": 0, "a": 0, "b": 0, "draw": 0, "void": 4}
    assert "PB[a]" in a["sgf"][0] and "PB[b]" in a["sgf"][1]


def test_match_on_the_gpu_finishes_and_scores_its_games(tmp_path):
    pa, pb = _predictor(64), _predictor(128)
    r = _run(tmp_path, "e", pa, pb, games=4, setup=ENDGAME)
    _check_match(r, 4, ALTERNATING, setup=len(ENDGAME), finished=True)
    s = r["summary"]
    assert all(len(m) > len(ENDGAME) + 2 for m in r["moves"])       # moves, not only passes
    assert s["wins"]["void"] == 0 and s["wins"]["B"] + s["wins"]["W"] == 4
    assert s["wins"]["a"] + s["wins"]["b"] == 4
    for meta in s["per_game"]:                     # the winner's holder got the win
        assert meta["result"][0] in "BW"
    want = {"a": 0, "b": 0}
    for meta in s["per_game"]:
        want[meta["black"] if meta["result"][0] == "B" else meta["white"]] += 1
    assert (s["wins"]["a"], s["wins"]["b"]) == (want["a"], want["b"])
    margins = [float(m["result"][2:]) * (1 if m["result"][0] == "B" else -1)
               for m in s["per_game"]]
    assert s["mean_score"] == sum(margins) / 4
