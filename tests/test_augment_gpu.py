"""Training-time symmetry augmentation on the GPU: augment_batch (csrc/kernels/augment.hip)
byte for byte against data/symmetry.py, HipGoNet's ``aug_seq`` path against a net fed
host-augmented batches, and the trainer's HIPBackend against the oracle over the loader's
batches."""

import numpy as np
import pytest
import torch

from deep_go_amd.config import ExperimentConfig
from deep_go_amd.data.batch import pack_batch, packed_batch_bytes, unpack_views
from deep_go_amd.data.symmetry import SYM_INVERSE, augment_batch, augment_symmetries

pytestmark = pytest.mark.gpu

NP = 361
PRE = 64            # margin bytes (0xA5) on each side of the packed buffer
LABELS = [-1, 0, 18, 342, 360, 400]


def _F():
    from deep_go_amd.ops import functional
    return functional


def _case(B, seed):
    """A packed batch of random bytes inside 0xA5 margins (host), and its numpy parts."""
    rng = np.random.default_rng(seed)
    planes = rng.integers(0, 256, (B, 9, 19, 19)).astype(np.uint8)
    player = rng.integers(0, 256, B).astype(np.uint8)
    rank = rng.integers(0, 256, B).astype(np.uint8)
    labels = np.array([LABELS[(i + seed) % len(LABELS)] for i in range(B)], np.int32)
    nb = packed_batch_bytes(B)
    big = torch.full((PRE + nb + PRE,), 0xA5, dtype=torch.uint8)
    big[PRE:PRE + nb] = pack_batch(planes, player, rank, labels)
    return big, planes, labels


def _expected(big, B, planes, labels, sym):
    want = big.clone()
    wp, _, _, wl = unpack_views(want[PRE:PRE + packed_batch_bytes(B)], B)
    p, l = augment_batch(planes, labels, sym)
    wp.copy_(torch.from_numpy(p.reshape(B, 9, NP)))
    wl.copy_(torch.from_numpy(l))
    return want


def _run(big, B, **kw):
    dev = big.cuda()
    ids = _F().augment_batch(dev[PRE:PRE + packed_batch_bytes(B)], B, **kw)
    return dev.cpu(), ids.cpu().numpy()


@pytest.mark.parametrize("s", range(8))
def test_one_board_each_symmetry_byte_exact(s):
    big, planes, labels = _case(1, seed=s)
    sym = np.array([s], np.uint8)
    got, ids = _run(big, 1, sym=torch.from_numpy(sym))
    assert torch.equal(got, _expected(big, 1, planes, labels, sym))
    assert ids.tolist() == [s]


def test_three_boards_explicit_ids_byte_exact():
    """Ids [0, 5, 7]: the first board stays, and the ids are taken & 7."""
    big, planes, labels = _case(3, seed=11)
    sym = np.array([0, 5, 7], np.uint8)
    want = _expected(big, 3, planes, labels, sym)
    got, ids = _run(big, 3, sym=torch.from_numpy(sym))
    assert torch.equal(got, want) and ids.tolist() == [0, 5, 7]
    got, ids = _run(big, 3, sym=torch.from_numpy(sym + 8 * np.array([1, 2, 31], np.uint8)))
    assert torch.equal(got, want) and ids.tolist() == [0, 5, 7]


@pytest.mark.parametrize("seed,seq", [(1234, 3), (2 ** 40 + 7, 2 ** 33 + 5)])
def test_hashed_ids_byte_exact(seed, seq):
    """B = 17 (a pad byte sits between the rank and label views), board0 = 1000, every label
    kind: the buffer and the ids output equal the oracle's."""
    B = 17
    big, planes, labels = _case(B, seed=5)
    assert set(labels.tolist()) == set(LABELS)
    sym = augment_symmetries(seed, seq, 1000, B)
    assert len(set(sym.tolist())) >= 5
    got, ids = _run(big, B, seed=seed, seq=seq, board0=1000)
    assert np.array_equal(ids, sym)
    assert torch.equal(got, _expected(big, B, planes, labels, sym))


def test_symmetry_then_inverse_restores_the_buffer():
    B = 8
    big, _, _ = _case(B, seed=7)
    nb = packed_batch_bytes(B)
    dev = big.cuda()
    orig = dev.clone()
    sym = torch.arange(8, dtype=torch.uint8)
    _F().augment_batch(dev[PRE:PRE + nb], B, sym=sym)
    assert not torch.equal(dev, orig)
    _F().augment_batch(dev[PRE:PRE + nb], B, sym=torch.from_numpy(SYM_INVERSE[sym.numpy()]))
    assert torch.equal(dev, orig)


def test_bad_arguments_raise_without_a_launch():
    from deep_go_amd.ops.native import aug, stream_handle
    a, s = aug(), stream_handle()
    buf = torch.zeros(packed_batch_bytes(2), dtype=torch.uint8, device="cuda")
    v = unpack_views(buf, 2)
    for args in ((v[0].data_ptr(), v[3].data_ptr(), -1), (0, v[3].data_ptr(), 2),
                 (v[0].data_ptr(), 0, 2)):
        with pytest.raises(RuntimeError) as e:
            a.augment_batch(*args, 0, 0, 0, 0, 0, s)
        assert str(e.value) == "augment_batch: invalid argument"
    a.augment_batch(0, 0, 0, 0, 0, 0, 0, 0, s)          # B = 0: nothing to do
    torch.cuda.synchronize()
    assert not buf.any()


# ----------------------------------------------------------------------------- the model
@pytest.fixture(scope="module")
def batches():
    """Four raw batches of 8 boards and, per batch, the same batch moved on the host by the
    oracle with the symmetries of (SEED, seq = index, board0 = BOARD0)."""
    from deep_go_amd.data.synthetic import random_planes
    raw, moved = [], []
    for seq in range(4):
        planes, player, rank, labels = random_planes(8, seed=70 + seq)
        sym = augment_symmetries(SEED, seq, BOARD0, 8)
        p, l = augment_batch(planes, labels, sym)
        raw.append((planes, player, rank, labels))
        moved.append((p, player, rank, l))
    return raw, moved


SEED, BOARD0 = 2 ** 40 + 7, 24


def _train(cfg, feed, graphs, arm):
    """4 steps of a fresh net over feed; (per-step loss vectors and preds, final params,
    the ids of the last batch)."""
    from deep_go_amd.models.hip_model import HipGoNet, SegmentedStep
    net = HipGoNet(cfg, 8, device="cuda")
    if arm:
        net.set_augment(SEED, BOARD0)
    seq_of = (lambda i: i) if arm else (lambda i: None)
    if graphs:
        assert net.enable_prefetch()
        host = [pack_batch(*b).pin_memory() for b in feed]
        load = lambda i: net.set_batch_packed(host[i], aug_seq=seq_of(i))   # noqa: E731
        load(0)
        step = SegmentedStep(net, None, use_graphs=True)
        assert len(step._gsets) == 2
    else:
        dev = [tuple(torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in b) for b in feed]
        load = lambda i: net.set_batch(*dev[i], aug_seq=seq_of(i))          # noqa: E731
        step = net.train_step
    out, bufs = [], set()
    for i in range(4):
        load(i)
        bufs.add(net.cur_in)
        step()
        out.append((net.loss.clone(), net.pred.clone()))
    torch.cuda.synchronize()
    assert len(bufs) == (2 if graphs else 1)       # both input buffers were used
    return out, net.params.clone(), net.aug_sym


@pytest.mark.parametrize("graphs", [False, True], ids=["eager", "prefetch-graphs"])
@pytest.mark.parametrize("dtype", ["bf16", "fp8"])
def test_armed_net_equals_net_fed_host_augmented_batches(batches, dtype, graphs):
    """Net A: set_augment, raw batches with aug_seq = 0..3.  Net B: not armed, the same batches
    moved on the host.  Losses, predictions and parameters after 4 steps are equal bit for bit
    (so the kernel ran before anything read the batch: the step, and for fp8 the calibration);
    once eagerly through set_batch, once with prefetch + step graphs + set_batch_packed from
    pinned host buffers."""
    raw, moved = batches
    cfg = ExperimentConfig(numLayers=4, channelSize=128, batchSize=8, seed=5, dtype=dtype)
    a_out, a_params, a_sym = _train(cfg, raw, graphs, arm=True)
    b_out, b_params, b_sym = _train(cfg, moved, graphs, arm=False)
    assert b_sym is None
    assert np.array_equal(a_sym.cpu().numpy(), augment_symmetries(SEED, 3, BOARD0, 8))
    for (la, pa), (lb, pb) in zip(a_out, b_out):
        assert torch.equal(la, lb) and torch.equal(pa, pb)
    assert torch.equal(a_params, b_params)
    assert not torch.equal(a_out[0][0], a_out[1][0])


def test_aug_seq_without_set_augment_raises():
    from deep_go_amd.models.hip_model import HipGoNet
    cfg = ExperimentConfig(numLayers=4, channelSize=128, batchSize=8)
    net = HipGoNet(cfg, 8, device="cuda")
    buf = torch.zeros(packed_batch_bytes(8), dtype=torch.uint8, device="cuda")
    with pytest.raises(RuntimeError):
        net.set_batch_packed(buf, aug_seq=0)


# ----------------------------------------------------------------------------- the trainer
def test_hip_backend_feeds_the_oracle_batches(packed_fixture, tmp_path):
    """Experiment on the GPU with augment=d4: after each load_next the input buffer holds the
    oracle applied to a fresh loader's batch at the same sequence number (two consecutive
    batches: both input buffers), and after eval_batch_set it holds the validation chunk as
    drawn."""
    from deep_go_amd.train.experiment import Experiment
    B = 8
    cfg = ExperimentConfig(numLayers=4, channelSize=128, batchSize=B, validationSize=B,
                           useCuda=True, data_root=packed_fixture, seed=9, augment="d4",
                           checkpoint_dir=str(tmp_path), loader_threads=2, prefetch=2)
    e = Experiment(cfg, id="g")
    e.init()
    be = e.backend
    assert be.net.load_stream is not None            # prefetch: two input buffers
    e.loader_seq = 3
    loader = e._train_loader()
    raw = Experiment(cfg.replace(augment="none", useCuda=False), id="raw")
    raw.init()
    try:
        used = set()
        for seq in (3, 4):
            assert be.load_next(loader) is None
            used.add(be.net.cur_in)
            src = raw._regenerate_batch(seq)
            sym = augment_symmetries(cfg.seed, seq, 0, B)
            want_p, want_l = augment_batch(src[0], src[3], sym)
            got = be.current_batch()
            assert np.array_equal(be.net.aug_sym.cpu().numpy(), sym)
            assert np.array_equal(got[0], want_p) and np.array_equal(got[3], want_l)
            assert np.array_equal(got[1], src[1]) and np.array_equal(got[2], src[2])
            assert not np.array_equal(got[0], src[0])
            be.train_step()
        assert used == {0, 1}
    finally:
        loader.close()
    val = e.draw_validation(B)
    e.eval_batch_set(val)
    got = be.current_batch()
    for g, w in zip(got, val):
        assert np.array_equal(g, np.asarray(w).reshape(g.shape))
