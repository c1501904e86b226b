"""Training-time symmetry augmentation without a GPU: the hash that draws each board's
symmetry (data/symmetry.py augment_symmetries, the definition), the numpy oracle of the
transform (augment_batch), and the trainer's CPU path (``augment=d4``: exact resume, the
regenerated bad-batch dump, ``augment=none`` unchanged)."""
import dataclasses
import os

import numpy as np
import pytest
import torch

from deep_go_amd.config import ExperimentConfig, override, parse_overrides
from deep_go_amd.data.symmetry import (SYM_INVERSE, SYM_PERM, augment_batch, augment_symmetries,
                                       transform_label, transform_planes)

NP = 361
SEEDS = (0, 1234, 2 ** 40 + 7)


# ----------------------------------------------------------------------------- the hash
def test_symmetries_are_deterministic_and_in_range():
    a = augment_symmetries(1234, 7, 0, 256)
    assert a.dtype == np.uint8 and a.shape == (256,) and a.max() <= 7
    assert np.array_equal(a, augment_symmetries(1234, 7, 0, 256))
    assert augment_symmetries(1234, 7, 0, 0).shape == (0,)


def test_symmetries_change_with_seed_seq_and_board():
    base = augment_symmetries(1234, 7, 0, 256)
    assert not np.array_equal(base, augment_symmetries(1235, 7, 0, 256))
    assert not np.array_equal(base, augment_symmetries(1234, 8, 0, 256))
    assert not np.array_equal(base, augment_symmetries(1234, 7, 1, 256))
    assert len(set(base.tolist())) == 8          # (and the boards of one batch differ)


def test_symmetries_depend_on_the_high_words():
    base = augment_symmetries(5, 9, 0, 256)
    assert not np.array_equal(base, augment_symmetries(5 + 2 ** 32, 9, 0, 256))
    assert not np.array_equal(base, augment_symmetries(5 + 2 ** 63, 9, 0, 256))
    assert not np.array_equal(base, augment_symmetries(5, 9 + 2 ** 32, 0, 256))
    assert not np.array_equal(base, augment_symmetries(5, 9 + 2 ** 63, 0, 256))


def test_symmetries_are_consistent_under_board0_slicing():
    for seed, seq in ((1234, 0), (2 ** 40 + 7, 2 ** 33 + 5)):
        full = augment_symmetries(seed, seq, 0, 16)
        assert np.array_equal(full[8:], augment_symmetries(seed, seq, 8, 8))
        assert np.array_equal(augment_symmetries(seed, seq, 1000, 17)[5:],
                              augment_symmetries(seed, seq, 1005, 12))


def test_symmetries_match_the_written_form():
    """The docstring's three lines in plain Python integers."""
    def mix32(x):
        x ^= x >> 16
        x = x * 0x7feb352d & 0xFFFFFFFF
        x ^= x >> 15
        x = x * 0x846ca68b & 0xFFFFFFFF
        return x ^ x >> 16
    for seed, seq, b0 in ((0, 0, 0), (1234, 3, 1000), (2 ** 40 + 7, 2 ** 35 + 1, 2 ** 32 - 3)):
        a = mix32(((seed & 0xFFFFFFFF ^ 0x9e3779b9) + (seed >> 32)) & 0xFFFFFFFF)
        b = mix32(mix32((a + (seq & 0xFFFFFFFF)) & 0xFFFFFFFF) ^ (seq >> 32))
        want = [mix32((b + ((b0 + i) & 0xFFFFFFFF)) & 0xFFFFFFFF) >> 29 for i in range(9)]
        assert augment_symmetries(seed, seq, b0, 9).tolist() == want


def test_host_twin_of_the_kernel_hash_matches():
    """augment.hip's hash, compiled for the host (the kernel runs the same function)."""
    from deep_go_amd.ops.native import aug
    f = aug().augment_symmetry
    for seed in SEEDS + (2 ** 64 - 1,):
        for seq in (0, 1, 127, 2 ** 32, 2 ** 63 + 11):
            want = augment_symmetries(seed, seq, 2 ** 32 - 8, 16)
            got = [f(seed, seq, 2 ** 32 - 8 + i) for i in range(16)]
            assert got == want.tolist()


@pytest.mark.parametrize("seed", SEEDS)
def test_symmetries_are_uniform_and_unlinked(seed):
    """128 sequence numbers x 256 boards: the 8 counts, the 64 joint counts of (s at seq, s at
    seq + 1) of one board and the 64 of (s of board b, s of board b + 1), each within 5 binomial
    standard deviations of its expectation."""
    g = np.stack([augment_symmetries(seed, q, 0, 256) for q in range(128)]).astype(np.int64)

    def worst(counts, n, cells):
        p = 1.0 / cells
        return float(np.abs(counts - n * p).max() / np.sqrt(n * p * (1 - p)))
    assert g.size == 32768
    assert worst(np.bincount(g.ravel(), minlength=8), g.size, 8) <= 5
    for x, y in ((g[:-1], g[1:]), (g[:, :-1], g[:, 1:])):
        assert worst(np.bincount((8 * x + y).ravel(), minlength=64), x.size, 64) <= 5


# ----------------------------------------------------------------------------- the oracle
def _random_batch(n, seed=0):
    rng = np.random.default_rng(seed)
    planes = rng.integers(0, 256, (n, 9, 19, 19)).astype(np.uint8)
    labels = rng.integers(0, NP, n).astype(np.int32)
    return planes, labels


def test_sym_inverse_is_the_group_inverse():
    for s in range(8):
        assert np.array_equal(SYM_PERM[SYM_INVERSE[s]][SYM_PERM[s]], np.arange(NP))


def test_augment_batch_identity_and_new_arrays():
    planes, labels = _random_batch(5)
    p0, l0 = planes.copy(), labels.copy()
    p, l = augment_batch(planes, labels, np.zeros(5, np.uint8))
    assert np.array_equal(p, planes) and np.array_equal(l, labels)
    assert p is not planes and l is not labels
    p[:] = 0
    augment_batch(planes, labels, np.arange(5, dtype=np.uint8) + 1)
    assert np.array_equal(planes, p0) and np.array_equal(labels, l0)   # inputs untouched


def test_augment_batch_moves_each_board_by_its_own_symmetry():
    planes, labels = _random_batch(8, seed=1)
    sym = np.arange(8, dtype=np.uint8)[::-1].copy()
    p, l = augment_batch(planes, labels, sym)
    assert p.dtype == np.uint8 and l.dtype == np.int32 and p.shape == planes.shape
    for i, s in enumerate(sym):
        assert np.array_equal(p[i], transform_planes(planes[i], int(s)))
        assert l[i] == transform_label(int(labels[i]), int(s))
        # dst[T_s(q)] = src[q], on every plane
        q = int(labels[i])
        assert np.array_equal(p[i].reshape(9, NP)[:, SYM_PERM[s][q]],
                              planes[i].reshape(9, NP)[:, q])
    flat, _ = augment_batch(planes.reshape(8, 9, NP), labels, sym)      # [n, 9, 361] too
    assert np.array_equal(flat, p.reshape(8, 9, NP))
    assert np.array_equal(augment_batch(planes, labels, sym + 8)[0], p)   # ids are taken & 7


def test_augment_batch_then_inverse_restores_every_byte():
    planes, labels = _random_batch(8, seed=2)
    labels[:3] = (-1, 400, 360)
    sym = np.arange(8, dtype=np.uint8)
    p, l = augment_batch(planes, labels, sym)
    back_p, back_l = augment_batch(p, l, SYM_INVERSE[sym])
    assert np.array_equal(back_p, planes) and np.array_equal(back_l, labels)


def test_augment_batch_leaves_other_label_values():
    planes, _ = _random_batch(6, seed=3)
    labels = np.array([-1, 361, 400, -7, 2 ** 31 - 1, 0], np.int32)
    _, l = augment_batch(planes, labels, np.full(6, 5, np.uint8))
    assert l[:5].tolist() == labels[:5].tolist()
    assert l[5] == SYM_PERM[5][0]


def test_augment_batch_moves_the_ko_mark_with_its_point():
    """A ko mark is 255 in the stored liberty plane (plane 1) at an empty point."""
    for s in range(8):
        planes = np.zeros((1, 9, 19, 19), np.uint8)
        x, y = 3, 16
        planes[0, 1, x, y] = 255
        p, _ = augment_batch(planes, np.array([0], np.int32), np.array([s], np.uint8))
        t = int(SYM_PERM[s][19 * x + y])
        assert p[0, 1].reshape(NP)[t] == 255 and int(p[0, 1].sum()) == 255
        assert p[0, 0].reshape(NP)[t] == 0          # the point is still empty


def test_augment_batch_rejects_mismatched_lengths():
    planes, labels = _random_batch(3)
    with pytest.raises(ValueError):
        augment_batch(planes, labels, np.zeros(2, np.uint8))


# ----------------------------------------------------------------------------- the config
def test_augment_field_choices_and_overrides():
    assert ExperimentConfig().augment == "none"
    assert override(ExperimentConfig(), parse_overrides(["augment=d4"])).augment == "d4"
    with pytest.raises(ValueError):
        override(ExperimentConfig(), {"augment": "foo"})
    # a checkpoint written before the field existed
    d = ExperimentConfig(numLayers=4).to_dict()
    del d["augment"]
    assert ExperimentConfig.from_dict(d) == ExperimentConfig(numLayers=4)


# ----------------------------------------------------------------------------- the trainer
def _cfg(tmp_path, packed_fixture, **kw):
    base = dict(numLayers=3, channelSize=16, batchSize=4, validationSize=8,
                validation_interval=100, log_interval=100, useCuda=False,
                data_root=packed_fixture, checkpoint_dir=str(tmp_path), seed=3,
                loader_threads=2, prefetch=2)
    base.update(kw)
    return ExperimentConfig(**base)


def test_augment_foo_raises_in_the_trainer(tmp_path, packed_fixture):
    with pytest.raises(ValueError):
        _cfg(tmp_path, packed_fixture).replace(augment="foo")


def test_d4_resume_is_exact(tmp_path, packed_fixture):
    from deep_go_amd.train.experiment import Experiment
    cfg = _cfg(tmp_path, packed_fixture, augment="d4")
    whole = Experiment(cfg, id="w")
    whole.run(6)
    a = Experiment(cfg, id="a")
    a.run(3)
    path = a.save()
    a2 = Experiment.load(path)
    assert a2.cfg.augment == "d4"
    a2.id = "a2"
    a2.run(3)
    assert a2.loader_seq == whole.loader_seq == 6
    assert torch.equal(a2.backend.flat_params(), whole.backend.flat_params())
    # and the augmentation did change what the net saw
    plain = Experiment(_cfg(tmp_path, packed_fixture), id="p")
    plain.run(6)
    assert not torch.equal(plain.backend.flat_params(), whole.backend.flat_params())


def test_augment_none_is_the_unaugmented_run(tmp_path, packed_fixture):
    """augment=none: load_next hands the loader's batch on as it is, and the run equals one
    that feeds those batches to the backend itself."""
    from deep_go_amd.train.backends import CPUBackend
    from deep_go_amd.train.experiment import Experiment
    explicit = Experiment(_cfg(tmp_path, packed_fixture, augment="none"), id="e")
    explicit.run(4)
    kw = dataclasses.asdict(_cfg(tmp_path, packed_fixture))
    del kw["augment"]                                  # a config that never names the field
    e = Experiment(ExperimentConfig(**kw), id="d")
    e.init()
    loader = e._train_loader()
    be = CPUBackend(e.cfg, e.local_batch)
    try:
        for _ in range(4):
            be.set_batch(*loader.next_numpy())
            be.train_step()
    finally:
        loader.close()
    assert torch.equal(explicit.backend.flat_params(), be.flat_params())


def test_cpu_backend_batch_and_regenerated_batch_are_the_oracle(tmp_path, packed_fixture):
    """What CPUBackend.load_next feeds under d4 = the oracle over a fresh loader's batch at the
    same sequence number, with this rank's board offset; _regenerate_batch gives the same."""
    from deep_go_amd.train.experiment import Experiment
    cfg = _cfg(tmp_path, packed_fixture, augment="d4")
    e = Experiment(cfg, id="r")
    e.init()
    e.loader_seq = 5
    loader, raw = e._train_loader(), Experiment(cfg.replace(augment="none"), id="raw")
    raw.init()
    try:
        for seq in (5, 6):
            got = e.backend.load_next(loader)
            src = raw._regenerate_batch(seq)
            sym = augment_symmetries(cfg.seed, seq, 0, 4)
            want_p, want_l = augment_batch(src[0], src[3], sym)
            assert np.array_equal(got[0], want_p) and np.array_equal(got[3], want_l)
            assert np.array_equal(got[1], src[1]) and np.array_equal(got[2], src[2])
            reg = e._regenerate_batch(seq)
            assert all(np.array_equal(x, y) for x, y in zip(reg, got))
    finally:
        loader.close()
    assert sym.any()        # (not all identity: the comparison above saw moved boards)
