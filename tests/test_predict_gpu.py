"""Move prediction on the GPU: symmetry_planes / policy_ensemble (csrc/kernels/policy.hip)
against data/symmetry.py, and the Predictor's whole path against the net's own
log-probabilities, its symmetries and the fp32 CPU reference."""
import os

import numpy as np
import pytest
import torch

from deep_go_amd.config import ExperimentConfig
from deep_go_amd.data.symmetry import (SYM_PERM, ensemble_policy, transform_label,
                                       transform_planes)

pytestmark = pytest.mark.gpu

NP = 361
B = 16
# |prob - ref| <= BOUND * ref: at most 8 + 361 fp32 additions in any order, expf and one
# division, with slack
BOUND = 512 * 2.0 ** -24
ULP = 2.0 ** -24


def _log_softmax(z):
    z = z - z.max(-1, keepdims=True)
    return z - np.log(np.exp(z).sum(-1, keepdims=True))


def _F():
    from deep_go_amd.ops import functional
    return functional


def _rel_err(got, ref):
    """max |got - ref| / ref over ref > 0 (and got must be 0 where ref is 0), in 2^-24."""
    got = np.asarray(got, np.float64)
    assert (got[ref == 0] == 0).all()
    nz = ref > 0
    return float((np.abs(got[nz] - ref[nz]) / ref[nz]).max() / ULP) if nz.any() else 0.0


# ----------------------------------------------------------------------------- G1
@pytest.fixture(scope="module")
def positions(packed_fixture):
    d = np.load(os.path.join(packed_fixture, "test.dgpack.npz"))
    sel = np.linspace(0, len(d["label"]) - 1, 5).astype(int)
    return (np.ascontiguousarray(d["planes"][sel].reshape(-1, 9, 19, 19)), d["player"][sel],
            d["rank"][sel], d["label"][sel].astype(np.int32))


@pytest.mark.parametrize("n,S,cap", [(2, 8, 16), (1, 8, 16), (3, 1, 16), (2, 8, 17), (5, 1, 5)])
def test_symmetry_planes_byte_exact(n, S, cap):
    """Every byte of the packed buffer and of a margin around it: boards < n S as
    transform_planes / transform_label give them, everything else untouched (cap = 17 has a
    pad byte between the rank and label views)."""
    from deep_go_amd.data.batch import packed_batch_bytes, unpack_views
    rng = np.random.default_rng(10 * n + S)
    planes = rng.integers(0, 256, (n, 9, 19, 19)).astype(np.uint8)
    player = rng.integers(1, 3, n).astype(np.uint8)
    rank = rng.integers(1, 10, n).astype(np.uint8)
    labels = np.array([-1, 0, 18, 342, 360][:n], np.int32)[::-1].copy()
    nb, pre = packed_batch_bytes(cap), 64
    big = torch.full((pre + nb + 64,), 0xA5, dtype=torch.uint8)
    want = big.clone()
    wp, wpl, wrk, wlb = unpack_views(want[pre:pre + nb], cap)
    for i in range(n):
        for s in range(S):
            j = i * S + s
            wp[j] = torch.from_numpy(transform_planes(planes[i], s).reshape(9, NP))
            wpl[j], wrk[j] = int(player[i]), int(rank[i])
            wlb[j] = int(transform_label(int(labels[i]), s))
    dev = big.cuda()
    _F().symmetry_planes(torch.from_numpy(planes), torch.from_numpy(player),
                         torch.from_numpy(rank), torch.from_numpy(labels), S=S, B=cap,
                         out=dev[pre:pre + nb])
    got = dev.cpu()
    assert torch.equal(got, want)
    if n * S < cap:   # the unwritten boards' labels are still the sentinel
        assert unpack_views(got[pre:pre + nb], cap)[3][n * S] == np.int32(-0x5A5A5A5B)


def test_symmetry_planes_rejects_overflow():
    z = torch.zeros((3, 9, 19, 19), dtype=torch.uint8)
    o = torch.zeros(3, dtype=torch.uint8)
    with pytest.raises(RuntimeError):
        _F().symmetry_planes(z, o, o, torch.zeros(3, dtype=torch.int32), S=8, B=16)


# ----------------------------------------------------------------------------- G2
@pytest.fixture(scope="module")
def synth():
    """The issue's synthetic case and its float64 reference (computed once)."""
    n, S, K = 5, 8, 16
    logp = _log_softmax(np.random.default_rng(0).normal(0, 2, (n, S, NP))).astype(np.float32)
    rng = np.random.default_rng(100)
    illegal = rng.random((n, NP)) < 0.3
    half = rng.random((n, NP)) < 0.5
    stones = (illegal & half).astype(np.uint8) * rng.integers(1, 3, (n, NP)).astype(np.uint8)
    extra = (illegal & ~half).astype(np.uint8) * 7
    legal = ~illegal
    ref0 = ensemble_policy(logp, legal, K + 1)
    # labels: places 2, 0 and 15 of the reference order, an illegal point, none
    labels = np.array([ref0[1][0, 2], ref0[1][1, 0], np.flatnonzero(illegal[2])[0], -1,
                       ref0[1][4, 15]], np.int32)
    prob, idx, tp, rank = ensemble_policy(logp, legal, K, labels)
    # precondition: no near-tie among the top 17 reference values can hide a wrong order
    top17 = ref0[2]
    gap = ((top17[:, :-1] - top17[:, 1:]) / top17[:, :-1]).min()
    assert gap > 2 * BOUND, gap
    assert list(rank) == [2, 0, -1, -1, 15]
    return dict(n=n, S=S, K=K, logp=logp, stones=stones, extra=extra, legal=legal,
                labels=labels, prob=prob, idx=idx, tp=tp, rank=rank)


def _run(logp, stones=None, extra=None, labels=None, S=8, K=16, mask=True):
    t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a))
    r = _F().policy_ensemble(t(logp.reshape(-1, NP)), t(stones), t(extra), t(labels), S=S, K=K,
                             mask=mask)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in r.items()}


def test_policy_ensemble_vs_oracle(synth):
    c = synth
    r = _run(c["logp"], c["stones"], c["extra"], c["labels"])
    err = _rel_err(r["prob"], c["prob"])
    print(f"\npolicy_ensemble max relative error: {err:.2f} x 2^-24 (bound 512)")
    assert err <= 512
    assert np.array_equal(r["topk"], c["idx"])
    assert np.array_equal(r["rank"], c["rank"])
    # topk_p is the very float stored in prob
    assert np.array_equal(r["topk_p"].view(np.uint32),
                          np.take_along_axis(r["prob"], r["topk"].astype(np.int64), 1)
                          .view(np.uint32))
    for i in range(c["n"]):
        assert abs(float(r["prob"][i].astype(np.float64).sum()) - 1) < 1e-5
    # bit-reproducible from run to run
    r2 = _run(c["logp"], c["stones"], c["extra"], c["labels"])
    for k in r:
        assert r[k].tobytes() == r2[k].tobytes(), k
    # stones alone / the extra mask alone carry the same legality
    r3 = _run(c["logp"], (~c["legal"]).astype(np.uint8), None, c["labels"])
    assert r3["prob"].tobytes() == r["prob"].tobytes()


def test_policy_ensemble_unmasked_and_small_sets(synth):
    c = synth
    n, K = c["n"], c["K"]
    # mask = 0: the stones are ignored, every point is legal
    ref = ensemble_policy(c["logp"], np.ones((n, NP), bool), K, c["labels"])
    r = _run(c["logp"], c["stones"], c["extra"], c["labels"], mask=False)
    assert _rel_err(r["prob"], ref[0]) <= 512
    assert (r["prob"] > 0).all()
    assert np.array_equal(r["rank"] >= 0, c["labels"] >= 0)
    rn = _run(c["logp"], None, None, None, mask=False)     # no stones, no labels at all
    assert rn["prob"].tobytes() == r["prob"].tobytes() and (rn["rank"] == -1).all()
    # fewer than K legal points (3, 1), the empty set, and a full set in one launch
    legal = np.zeros((n, NP), bool)
    legal[0, [360, 0, 200]] = True
    legal[1, 77] = True
    legal[3] = True
    legal[4, :K] = True            # exactly K
    labels = np.array([200, 77, 5, 9, K], np.int32)   # [2]: empty board set; [4]: illegal
    ref = ensemble_policy(c["logp"], legal, K, labels)
    r = _run(c["logp"], (~legal).astype(np.uint8), None, labels)
    assert _rel_err(r["prob"], ref[0]) <= 512
    assert np.array_equal(r["topk"], ref[1])
    assert np.array_equal(r["rank"], ref[3])
    assert (r["topk"][0, 3:] == -1).all() and (r["topk_p"][0, 3:] == 0).all()
    assert list(r["topk"][1]) == [77] + [-1] * (K - 1) and r["topk_p"][1, 0] == 1.0
    assert (r["prob"][2] == 0).all() and (r["topk"][2] == -1).all()
    assert (r["topk_p"][2] == 0).all() and r["rank"][2] == -1 and r["rank"][4] == -1
    assert (r["topk"][4] >= 0).all() and sorted(r["topk"][4]) == list(range(K))
    # K = 1 and K = 64
    for k in (1, 64):
        rk = _run(c["logp"], c["stones"], c["extra"], c["labels"], K=k)
        m = min(k, K)
        assert np.array_equal(rk["topk"][:, :m], c["idx"][:, :m])
        assert rk["prob"].tobytes() == _run(c["logp"], c["stones"], c["extra"],
                                            c["labels"])["prob"].tobytes()


def test_policy_ensemble_exact_ties():
    z = np.zeros((2, 1, NP))
    z[0, 0, [300, 7, 150]] = 3.0
    z[0, 0, [20, 10]] = 1.0
    z[1, 0, :] = 0.5                      # everything ties: index order
    logp = _log_softmax(z).astype(np.float32)
    stones = np.zeros((2, NP), np.uint8)
    stones[1, [0, 2]] = 1
    for labels in ([150, 3], [20, 1], [7, 0]):
        labels = np.array(labels, np.int32)
        ref = ensemble_policy(logp, stones == 0, 6, labels)
        r = _run(logp, stones, None, labels, S=1, K=6)
        assert np.array_equal(r["topk"], ref[1])
        assert np.array_equal(r["rank"], ref[3])
    assert list(r["topk"][0]) == [7, 150, 300, 10, 20, 0]
    assert list(r["topk"][1]) == [1, 3, 4, 5, 6, 7] and list(r["rank"]) == [0, -1]


def test_policy_ensemble_rejects_bad_arguments(synth):
    for kw in (dict(K=0), dict(K=65), dict(S=4)):
        with pytest.raises(RuntimeError):
            _run(synth["logp"][:, :kw.get("S", 8)], synth["stones"], **kw)
    with pytest.raises(RuntimeError):
        _run(synth["logp"], None, mask=True)      # a mask without stones


# ----------------------------------------------------------------------------- the nets
def _cfg(channels, dtype="bf16"):
    return ExperimentConfig(numLayers=4, channelSize=channels, head_relu=False, batchSize=B,
                            dtype=dtype, seed=11)


_predictors = {}


def _predictor(channels, dtype="bf16", S=8, device="gpu"):
    from deep_go_amd.predict import Predictor
    key = (channels, dtype, S, device)
    if key not in _predictors:
        _predictors[key] = Predictor(_cfg(channels, dtype), batch=B, symmetries=S,
                                     device=device, top=5)
    return _predictors[key]


@pytest.fixture(scope="module", autouse=True)
def _free_predictors():
    yield
    _predictors.clear()


def _net_logp(net, planes, player, rank):
    """The net's own log-probabilities [n, 8, 361] of the eight views of each position,
    through batches this test builds with transform_planes."""
    n = len(planes)
    views = np.stack([transform_planes(planes, s) for s in range(8)], 1).reshape(n * 8, 9, NP)
    out = np.zeros((n * 8, NP), np.float32)
    for lo in range(0, n * 8, B):
        k = min(B, n * 8 - lo)
        pl = np.zeros((B, 9, NP), np.uint8)
        py, rk = np.ones(B, np.uint8), np.ones(B, np.uint8)
        pl[:k], py[:k], rk[:k] = views[lo:lo + k], np.repeat(player, 8)[lo:lo + k], \
            np.repeat(rank, 8)[lo:lo + k]
        net.set_batch(torch.from_numpy(pl).cuda(), torch.from_numpy(py).cuda(),
                      torch.from_numpy(rk).cuda(),
                      torch.full((B,), -1, dtype=torch.int32, device="cuda"))
        out[lo:lo + k] = net.predict_logp()[:k].cpu().numpy()
    return out.reshape(n, 8, NP)


# ----------------------------------------------------------------------------- G3
@pytest.mark.parametrize("channels,dtype", [(128, "bf16"), (64, "bf16"), (128, "fp8")])
def test_predictor_vs_own_logp(positions, channels, dtype):
    """Exact up to the policy_ensemble bound, no bf16 noise: the Predictor's distribution is
    the oracle applied to what the same net returns for the eight transformed batches (a wrong
    inverse gather, slot order or stale input view shows here)."""
    planes, player, rank, labels = (a[:3] for a in positions)      # chunks of 2 and 1
    p = _predictor(channels, dtype)
    ko = np.zeros((3, NP), np.uint8)
    ko[1, np.flatnonzero(planes[1, 0].reshape(-1) == 0)[4]] = 1
    got = p.predict(planes, player, rank, labels=labels, extra_illegal=ko)
    logp = _net_logp(p.net, planes, player, rank)
    assert np.isfinite(logp).all()
    assert np.abs(np.exp(logp.astype(np.float64)).sum(-1) - 1).max() < 1e-4
    legal = (planes[:, 0].reshape(3, NP) == 0) & (ko == 0)
    ref = ensemble_policy(logp, legal, 5, labels)
    err = _rel_err(got.prob, ref[0])
    print(f"\n{channels} ch {dtype}: Predictor vs oracle(own logp) max rel err {err:.2f} x 2^-24")
    assert err <= 512
    assert got.prob.dtype == np.float32 and (got.prob[~legal] == 0).all()
    assert np.array_equal(got.topk_p, np.take_along_axis(got.prob, got.topk.astype(np.int64), 1))


def test_predict_logp_matches_evaluate_and_follows_the_input_buffer(positions):
    from deep_go_amd.models.hip_model import HipGoNet
    planes, player, rank, labels = positions
    net = HipGoNet(_cfg(128), B, device="cuda:0")
    pl = np.zeros((B, 9, NP), np.uint8)
    pl[:5] = planes.reshape(5, 9, NP)
    lab = np.zeros(B, np.int32)
    lab[:5] = labels
    args = [torch.from_numpy(a).cuda() for a in (pl, np.ones(B, np.uint8), np.ones(B, np.uint8),
                                                 lab)]
    assert net.logp is None and net._head_predict is None      # nothing built by default
    net.set_batch(*args)
    logp = net.predict_logp().clone()
    net.evaluate()
    torch.cuda.synchronize()
    nll = -logp[torch.arange(B), torch.from_numpy(lab).long().cuda()]
    assert torch.equal(nll, net.eval_loss)
    assert torch.equal(logp[torch.arange(B), net.eval_pred.long()], logp.max(1).values)
    # with input prefetch the launch reads the buffer select_inputs points at
    net.enable_prefetch()
    net.set_batch(*args)           # lands in buffer 1 and selects it
    assert net.cur_in == 1
    assert torch.equal(net.predict_logp(), logp)
    assert net._head_predict_in == 1 and net.labels.data_ptr() in net._head_predict.args


# ----------------------------------------------------------------------------- G4
@pytest.mark.parametrize("channels", [128, 64])
def test_predictor_equivariance(positions, channels):
    planes, player, rank, labels = (a[:2] for a in positions)
    p = _predictor(channels)
    base = p.predict(planes, player, rank, labels=labels).prob
    for g in (1, 4, 7):
        got = p.predict(transform_planes(planes, g), player, rank).prob
        err = _rel_err(got, transform_planes(base, g).astype(np.float64))
        print(f"\n{channels} ch: T_{g} equivariance max rel err {err:.2f} x 2^-24")
        assert err <= 512, g


# ----------------------------------------------------------------------------- G5
def test_ensemble_vs_fp32_reference(positions):
    """No fixed tolerance: the ensemble is the mean of the eight single-symmetry policies on
    both sides, so by convexity its total-variation distance to the fp32 CPU reference is at
    most the largest single-symmetry distance (plus the policy_ensemble bound)."""
    planes, player, rank, _ = (a[:3] for a in positions)
    tv = lambda a, b: 0.5 * np.abs(a.astype(np.float64) - b).sum(1)
    g8, c8 = _predictor(128), _predictor(128, device="cpu")
    g1, c1 = _predictor(128, S=1), _predictor(128, S=1, device="cpu")
    ens = tv(g8.predict(planes, player, rank, mask=False).prob,
             c8.predict(planes, player, rank, mask=False).prob)
    single = np.stack([tv(g1.predict(transform_planes(planes, s), player, rank, mask=False).prob,
                          c1.predict(transform_planes(planes, s), player, rank, mask=False).prob)
                       for s in range(8)])
    print(f"\nTV(GPU, fp32 CPU): ensemble {ens.max():.3e}, single symmetry max "
          f"{single.max():.3e} (per position: {ens} vs {single.max(0)})")
    assert (ens <= single.max(0) + BOUND).all()


# ----------------------------------------------------------------------------- G6
@pytest.mark.parametrize("channels", [128, 64])
def test_predictor_chunks_bit_exact(positions, channels):
    planes, player, rank, labels = positions
    p = _predictor(channels)
    assert p.chunk == 2
    allr = p.predict(planes, player, rank, labels=labels)          # chunks of 2, 2, 1
    for i in range(5):
        one = p.predict(planes[i:i + 1], player[i:i + 1], rank[i:i + 1], labels=labels[i:i + 1])
        for f in ("prob", "topk", "topk_p", "rank"):
            assert getattr(one, f)[0].tobytes() == getattr(allr, f)[i].tobytes(), (i, f)
    assert (allr.rank >= 0).all()
