"""Move prediction without a GPU: the symmetry tables, the float64 ensemble oracle, the CPU
Predictor (fp32 reference forward) and the predict / eval command lines."""
import json
import os

import numpy as np
import pytest
import torch

from deep_go_amd.config import ExperimentConfig
from deep_go_amd.data.symmetry import (SYM_PERM, ensemble_policy, transform_label,
                                       transform_planes)

NP = 361


# ----------------------------------------------------------------------------- C1
def test_sym_perm_is_the_dihedral_group():
    assert SYM_PERM.shape == (8, NP) and SYM_PERM.dtype == np.int16
    assert np.array_equal(SYM_PERM[0], np.arange(NP))
    perms = {tuple(SYM_PERM[s]) for s in range(8)}
    assert len(perms) == 8
    for s in range(8):
        assert np.array_equal(np.sort(SYM_PERM[s]), np.arange(NP))
    for a in range(8):
        for b in range(8):
            assert tuple(SYM_PERM[a][SYM_PERM[b]]) in perms   # T_a o T_b is some T_c
    # the definition, spelled out for one point: (x, y) = (2, 5)
    p = 19 * 2 + 5
    assert SYM_PERM[1][p] == 19 * 5 + (18 - 2)       # one turn: (a, b) -> (b, 18 - a)
    assert SYM_PERM[4][p] == 19 * 5 + 2              # the swap alone
    assert SYM_PERM[5][p] == 19 * 2 + (18 - 5)       # swap, then one turn


def test_transform_planes_and_label_agree():
    rng = np.random.default_rng(1)
    for s in range(8):
        for label in (0, 18, 342, 360, 47, int(rng.integers(NP))):
            hot = np.zeros((2, 9, 19, 19), np.uint8)
            hot.reshape(2, 9, NP)[:, :, label] = 1
            out = transform_planes(hot, s)
            assert out.shape == hot.shape and out.dtype == hot.dtype
            t = transform_label(label, s)
            assert np.array_equal(np.flatnonzero(out[1, 3].reshape(-1)), [t])
        assert transform_label(-1, s) == -1
        assert np.array_equal(transform_label(np.array([-1, 0, 360]), s),
                              [-1, SYM_PERM[s][0], SYM_PERM[s][360]])
    x = rng.integers(0, 255, (3, NP)).astype(np.uint8)
    for s in range(8):
        y = transform_planes(x, s)
        assert np.array_equal(y[:, SYM_PERM[s].astype(int)], x)   # dst[T_s(p)] = src[p]


# ----------------------------------------------------------------------------- C2
def _log_softmax(z):
    z = z - z.max(-1, keepdims=True)
    return z - np.log(np.exp(z).sum(-1, keepdims=True))


def test_oracle_properties():
    rng = np.random.default_rng(0)
    n, K = 6, 16
    logp = _log_softmax(rng.normal(0, 2, (n, 8, NP)))
    legal = rng.random((n, NP)) > 0.3
    legal[1] = False                       # a full board
    legal[2] = False
    legal[2, [5, 100, 300]] = True         # fewer than K legal points
    labels = np.array([int(np.flatnonzero(legal[0])[0]), 3, 100,
                       int(np.flatnonzero(~legal[3])[0]), -1, int(np.flatnonzero(legal[5])[7])])
    prob, idx, tp, rank = ensemble_policy(logp, legal, K, labels)
    assert prob.dtype == np.float64
    for i in (0, 2, 3, 4, 5):
        assert abs(prob[i][legal[i]].sum() - 1) < 1e-12
        assert (prob[i][~legal[i]] == 0).all()
    # the definition of q, recomputed by hand for one point
    i, p = 0, int(np.flatnonzero(legal[0])[3])
    q = np.mean([np.exp(logp[i, s, SYM_PERM[s][p]]) for s in range(8)])
    qs = sum(np.mean([np.exp(logp[i, s, SYM_PERM[s][r]]) for s in range(8)])
             for r in np.flatnonzero(legal[0]))
    assert abs(prob[i, p] - q / qs) < 1e-15
    # full board: all zero, no move
    assert (prob[1] == 0).all() and (idx[1] == -1).all() and (tp[1] == 0).all()
    assert rank[1] == -1
    # fewer than K: tail -1 / 0
    assert set(idx[2, :3]) == {5, 100, 300} and (idx[2, 3:] == -1).all()
    assert (tp[2, 3:] == 0).all()
    # top-k is sorted, legal, and its probabilities are prob's
    for i in (0, 3, 4, 5):
        assert legal[i][idx[i]].all()
        assert (np.diff(tp[i]) <= 0).all()
        assert np.array_equal(tp[i], prob[i, idx[i]])
        assert tp[i, -1] >= np.delete(prob[i], idx[i]).max()
    # ranks: a legal label's rank is its place in the order; illegal / missing -> -1
    assert rank[3] == -1 and rank[4] == -1
    for i in (0, 2, 5):
        order = sorted(np.flatnonzero(legal[i]), key=lambda r: (-prob[i, r], r))
        assert rank[i] == order.index(labels[i])
    # without labels every rank is -1
    assert (ensemble_policy(logp, legal, K)[3] == -1).all()


def test_oracle_ties_go_to_the_lower_index():
    z = np.zeros((1, 1, NP))
    z[0, 0, [300, 7, 150]] = 3.0           # three exactly equal maxima
    z[0, 0, [20, 10]] = 1.0                # two exactly equal runners-up
    logp = _log_softmax(z)
    legal = np.ones((1, NP), bool)
    prob, idx, tp, rank = ensemble_policy(logp, legal, 6, np.array([150]))
    assert list(idx[0]) == [7, 150, 300, 10, 20, 0]
    assert rank[0] == 1
    assert ensemble_policy(logp, legal, 6, np.array([20]))[3][0] == 4
    assert ensemble_policy(logp, legal, 6, np.array([7]))[3][0] == 0


# ----------------------------------------------------------------------------- C3
@pytest.fixture(scope="module")
def positions(packed_fixture):
    d = np.load(os.path.join(packed_fixture, "test.dgpack.npz"))
    sel = np.linspace(0, len(d["label"]) - 1, 5).astype(int)
    return (d["planes"][sel].reshape(-1, 9, 19, 19), d["player"][sel], d["rank"][sel],
            d["label"][sel].astype(np.int32))


@pytest.fixture(scope="module")
def small_cfg():
    return ExperimentConfig(numLayers=3, channelSize=16, batchSize=16, seed=3)


def test_cpu_predictor_is_equivariant(positions, small_cfg):
    from deep_go_amd.predict import Predictor
    planes, player, rank, labels = (a[:2] for a in positions)
    p = Predictor(small_cfg, batch=16, symmetries=8, device="cpu", top=5)
    base = p.predict(planes, player, rank, labels=labels)
    assert base.prob.dtype == np.float64 and base.prob.shape == (2, NP)
    occupied = planes[:, 0].reshape(2, NP) != 0
    assert (base.prob[occupied] == 0).all()
    assert np.allclose(base.prob.sum(1), 1, atol=1e-12)
    for g in range(8):
        r = p.predict(transform_planes(planes, g), player, rank,
                      labels=transform_label(labels, g))
        # prob_g[T_g(p)] = prob[p]: the same eight boards reach the net, in another order
        np.testing.assert_allclose(r.prob, transform_planes(base.prob, g), rtol=1e-12,
                                   atol=1e-300)
        # (ranks need not match: the head's ReLU leaves exact ties, broken by point index)
    # a single symmetry is NOT equivariant for this net (untied position biases)
    p1 = Predictor(small_cfg, batch=16, symmetries=1, device="cpu")
    a = p1.predict(planes, player, rank).prob
    b = p1.predict(transform_planes(planes, 1), player, rank).prob
    assert np.abs(b - transform_planes(a, 1)).max() > 1e-6


def test_cpu_predictor_chunks(positions, small_cfg):
    from deep_go_amd.predict import Predictor
    planes, player, rank, labels = positions
    p = Predictor(small_cfg, batch=16, symmetries=8, device="cpu", top=5)
    assert p.chunk == 2
    ko = np.zeros((5, NP), np.uint8)
    empty = np.flatnonzero(planes[3, 0].reshape(-1) == 0)
    ko[3, empty[10]] = 1
    allr = p.predict(planes, player, rank, labels=labels, extra_illegal=ko)   # chunks 2, 2, 1
    assert allr.prob[3, empty[10]] == 0
    for i in range(5):
        one = p.predict(planes[i:i + 1], player[i:i + 1], rank[i:i + 1],
                        labels=labels[i:i + 1], extra_illegal=ko[i:i + 1])
        # the same boards through the same fp32 forward, in a batch of 8 instead of 16: equal
        # up to the forward's fp32 rounding (the conv may sum in another order per batch size:
        # up to 25 * 40 = 1000 products per output, 1000 * 2^-24 = 6e-5 relative at worst)
        np.testing.assert_allclose(one.prob[0], allr.prob[i], rtol=1e-4, atol=1e-12)
        assert np.array_equal(one.topk[0], allr.topk[i])
        assert one.rank[0] == allr.rank[i]
    with pytest.raises(ValueError):
        Predictor(small_cfg, batch=12, symmetries=8, device="cpu")


# ----------------------------------------------------------------------------- C4
SGF = ("(;GM[1]SZ[19]\r\nBR[2d]\r\nWR[4d]\r\n;B[de];W[df];B[ed];W[eg];B[fe];W[ff];B[pp];W[ee]\r\n"
       ";B[ef];W[ee];B[pd];W[dd]\r\n)")


@pytest.fixture(scope="module")
def checkpoint(tmp_path_factory, packed_fixture):
    from deep_go_amd.models.gocnn import ParamLayout, init_params
    from deep_go_amd.utils.checkpoint import save_checkpoint
    d = tmp_path_factory.mktemp("ckpt")
    cfg = ExperimentConfig(numLayers=3, channelSize=16, batchSize=8, validationSize=16,
                           data_root=packed_fixture, checkpoint_dir=str(d), seed=4)
    path = str(d / "p.model")
    save_checkpoint(path, cfg, init_params(ParamLayout(cfg), 4), {"id": "p", "iterations": 0},
                    {"kind": "sgd", "rate": cfg.rate, "rate_decay": cfg.rateDecay})
    sgf = d / "game.sgf"
    sgf.write_bytes(SGF.encode())
    return path, str(sgf)


def _cli(capsys, *argv):
    from deep_go_amd.cli import main
    capsys.readouterr()
    assert main(list(argv)) == 0
    # (eval also prints the experiment's "initializing model..." line)
    return [json.loads(l) for l in capsys.readouterr().out.splitlines() if l.startswith("{")]


def test_cli_predict(checkpoint, capsys):
    from deep_go_amd.predict import positions_from_sgf
    ck, sgf = checkpoint
    planes, player, rank, label, ko = positions_from_sgf(SGF)
    assert len(label) == 12 and list(rank[:2]) == [2, 4] and list(player[:2]) == [1, 2]
    assert label[0] == 19 * 3 + 4 and list(ko[9:]) == [80, 81, -1]
    # default: the last move, top 5
    (last,) = _cli(capsys, "predict", ck, sgf, "--device", "cpu")
    assert set(last) == {"move", "player", "top", "played", "rank"}
    assert last["move"] == 12 and last["player"] == "W"
    assert last["played"] == {"sgf": "dd", "x": 3, "y": 3}
    assert len(last["top"]) == 5 and 0 <= last["rank"] < NP
    for t in last["top"]:
        assert set(t) == {"sgf", "x", "y", "p"}
        assert t["sgf"] == chr(97 + t["x"]) + chr(97 + t["y"]) and 0 < t["p"] <= 1
    assert [t["p"] for t in last["top"]] == sorted((t["p"] for t in last["top"]), reverse=True)
    # every move; occupied points and the ko point never appear
    rows = _cli(capsys, "predict", ck, sgf, "--device", "cpu", "--all", "--top", "40",
                "--symmetries", "1")
    assert [r["move"] for r in rows] == list(range(1, 13))
    assert [r["player"] for r in rows] == ["B", "W"] * 6
    for k, r in enumerate(rows):
        pts = [19 * t["x"] + t["y"] for t in r["top"]]
        assert len(pts) == 40 and len(set(pts)) == 40
        assert (planes[k, 0].reshape(-1)[pts] == 0).all()
        assert ko[k] not in pts
        assert r["played"]["x"] * 19 + r["played"]["y"] == label[k]
    assert rows[-1]["played"] == last["played"]
    (m3,) = _cli(capsys, "predict", ck, sgf, "--device", "cpu", "--move", "3", "--top", "2")
    assert m3["move"] == 3 and m3["player"] == "B" and len(m3["top"]) == 2
    with pytest.raises(SystemExit):
        _cli(capsys, "predict", ck, sgf, "--device", "cpu", "--move", "13")


def test_cli_eval_flags(checkpoint, capsys):
    ck, _ = checkpoint
    (plain,) = _cli(capsys, "eval", ck, "--split", "test", "--n", "16", "--device", "cpu")
    assert list(plain) == ["split", "cost", "accuracy"]       # as before the new flags
    (ens,) = _cli(capsys, "eval", ck, "--split", "test", "--n", "16", "--device", "cpu",
                  "--symmetries", "8", "--top", "3")
    assert list(ens)[:3] == ["split", "cost", "accuracy"]
    assert (ens["split"], ens["cost"], ens["accuracy"]) == tuple(plain.values())
    assert {"topk_accuracy", "mean_rank", "ensemble_accuracy"} <= set(ens)
    assert 0 <= ens["ensemble_accuracy"] <= ens["topk_accuracy"] <= 1
    assert 0 <= ens["mean_rank"] < NP
