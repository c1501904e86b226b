"""CPU checks of HipGoNet launch-plan rewrites that need no GPU: the merge of consecutive
conv_layer2 launches into conv_layer2_multi runs (hip_model.HipGoNet._merge_layer2_runs)."""
from types import SimpleNamespace

import numpy as np

from deep_go_amd.models.hip_model import HipGoNet, Knobs, L2Row, Op


class _H:
    EPI_FWD, EPI_DGRAD = 1, 2

    @staticmethod
    def conv_layer2(*a):
        pass

    @staticmethod
    def conv_layer2_multi(*a):
        pass

    @staticmethod
    def other(*a):
        pass


C, B = 256, 8


def _net():
    n = HipGoNet.__new__(HipGoNet)
    n.h = _H
    n.knobs = Knobs.from_env()
    n.B = B
    n.plans = [SimpleNamespace(cout=C)] * 32
    n._l2_tables = []
    return n


def _l2(epi, x, y, a=1000, pb=2000, mk=3000, layer=0):
    # conv_layer2 args: (epi, A, pbias, X, Y, mask, C, B)
    row = L2Row(a + x, pb + x, x, y, mk + x)
    return Op(_H.conv_layer2, (epi, *row, C, B), (layer,), epi, row)


def test_chained_run_becomes_one_multi_launch(monkeypatch):
    monkeypatch.delenv("DG_LAYER2_MULTI", raising=False)
    n = _net()
    ops = ([Op(_H.other, (0,), (0,))] + [_l2(1, 10 + i, 11 + i, layer=1 + i) for i in range(10)]
           + [Op(_H.other, (1,), (11,))])
    out = n._merge_layer2_runs(ops)
    assert [f for f, _ in out] == [_H.other, _H.conv_layer2_multi, _H.other]
    assert [op.layers for op in out] == [(0,), tuple(range(1, 11)), (11,)]
    epi, tab_ptr, nl, c, b = out[1].args
    assert (epi, nl, c, b) == (1, 10, 256, 8)
    assert out[1].kind == 1
    tab = n._l2_tables[0]
    assert tab is out[1].table
    assert tab.ctypes.data == tab_ptr and tab.shape == (10, 5)
    # rows {A, pbias, X, Y, mask}; each row's X is the previous row's Y
    assert np.array_equal(tab[:, 2][1:], tab[:, 3][:-1])
    assert tab[0].tolist() == [1010, 2010, 10, 11, 3010]


def test_runs_split_on_chain_break_kind_and_16_layers(monkeypatch):
    monkeypatch.delenv("DG_LAYER2_MULTI", raising=False)
    n = _net()
    ops = [_l2(1, 0, 1), _l2(1, 1, 2),          # run A (2 layers)
           _l2(1, 50, 51),                     # chain break: single launch kept as is
           _l2(2, 51, 52), _l2(2, 52, 53)]     # kind change: run B (dgrad)
    ops += [_l2(2, 100 + i, 101 + i) for i in range(20)]   # 20 chained: 16 + 4
    out = n._merge_layer2_runs(ops)
    kinds = [(f.__name__, a[2] if f is _H.conv_layer2_multi else None) for f, a in out]
    assert kinds == [("conv_layer2_multi", 2), ("conv_layer2", None),
                     ("conv_layer2_multi", 2), ("conv_layer2_multi", 16),
                     ("conv_layer2_multi", 4)]


def test_knobs_from_env_spellings(monkeypatch):
    import os

    import pytest
    for k in [k for k in os.environ if k.startswith("DG_")]:
        monkeypatch.delenv(k)
    assert Knobs.from_env() == Knobs()
    # a switch is off only for "0" ...
    for v, on in (("0", False), ("1", True), ("", True), ("2", True), ("off", True)):
        monkeypatch.setenv("DG_STACK", v)
        monkeypatch.setenv("DG_FUSED_UPDATE", v)
        monkeypatch.setenv("DG_RELU_MASK", v)      # ... except this one: on only for "1"
        k = Knobs.from_env()
        assert (k.STACK, k.FUSED_UPDATE, k.RELU_MASK) == (on, on, v == "1")
    for v, want in (("1", True), ("0", False), ("", None), ("2", None)):
        monkeypatch.setenv("DG_L0_MASK", v)
        assert Knobs.from_env().L0_MASK is want
    for v, want in (("1", True), ("0", False), ("", True), ("2", True)):
        monkeypatch.setenv("DG_EARLY_UPDATE", v)
        assert Knobs.from_env().EARLY_UPDATE is want
    monkeypatch.setenv("DG_WGRAD_GROUP", "5")
    for v, want in (("0", "none"), ("none", "none"), ("bias", "bias")):
        monkeypatch.setenv("DG_SIDE_STREAM", v)
        assert Knobs.from_env().SIDE_STREAM == want and Knobs.from_env().WGRAD_GROUP == 5
    monkeypatch.setenv("DG_SIDE_STREAM", "wgrad")
    with pytest.raises(ValueError):
        Knobs.from_env()


def test_disabled_keeps_per_layer_launches(monkeypatch):
    monkeypatch.setenv("DG_LAYER2_MULTI", "0")
    n = _net()
    ops = [_l2(1, i, i + 1) for i in range(4)]
    out = n._merge_layer2_runs(ops)
    assert out == ops
