"""Independent oracles for the tail of the optimizer step, and their self-checks (CPU).

Everything that runs after the gradients exist — the finite gates, SGD / RMSProp, the fused
grad_update launch, the operand refresh (bf16, e4m3, fragment orders, bias tables) and the fp8
casts — is compared by tests/test_update_gpu.py with the plain-Python references in this
file.  They are written from the layout comments (layouts.py, the WRefreshLayer comments) and
the reference recurrences (optimizer.lua:1-27), not from kernel code, and are checked here on
fixed tables and against the CPU optimizers so that a mistake in an oracle does not pass as a
kernel's.
"""
import numpy as np
import pytest
import torch

from deep_go_amd.ops import layouts as LY

E4M3_MAX = 448.0


# ------------------------------------------------------------------------------ oracles
def e4m3_bytes(x: torch.Tensor, s) -> torch.Tensor:
    """The e4m3 byte of x / s as the kernels form it: inv = float32(1) / float32(s) and
    x * inv in fp32, clamped to +-448, rounded to nearest even (torch.float8_e4m3fn)."""
    s32 = torch.as_tensor(s, dtype=torch.float64).reshape(()).to(torch.float32)
    inv = torch.tensor(1.0, dtype=torch.float32) / s32
    q = (x.to(torch.float32) * inv).clamp(-E4M3_MAX, E4M3_MAX)
    return q.to(torch.float8_e4m3fn).view(torch.uint8)


def frag_bf16(A: torch.Tensor, C: int) -> torch.Tensor:
    """conv_stack2 / conv_layer2 A-operand order of a [C][9 C] operand matrix (k = tap * C +
    channel; C = 128 | 256): flat [h C/128][step = chunk * 9 + tap][wm 2][kk 2][i 4][lane 64]
    [e 8] holding row 128 h + 64 wm + 16 i + (lane & 15), column tap * C + 64 chunk + 32 kk +
    8 (lane >> 4) + e — an explicit index gather."""
    assert C % 128 == 0 and A.shape[0] >= C and A.shape[1] >= 9 * C
    nh, nchunk = C // 128, C // 64
    ar = lambda n: torch.arange(n, dtype=torch.int64)   # noqa: E731
    h, st, wm, kk, i, lane, e = torch.meshgrid(ar(nh), ar(nchunk * 9), ar(2), ar(2), ar(4),
                                               ar(64), ar(8), indexing="ij")
    chunk, tap = st // 9, st % 9
    row = 128 * h + 64 * wm + 16 * i + (lane & 15)
    col = tap * C + 64 * chunk + 32 * kk + 8 * (lane >> 4) + e
    return A[row.reshape(-1), col.reshape(-1)].contiguous()


def dgrad_w8(w8: torch.Tensor) -> torch.Tensor:
    """The backward-data operand of e4m3 forward weights w8 [co][9][ci]:
    A_d[ci][8 - t][co] = W[co][t][ci]."""
    co, T, ci = w8.shape
    assert T == 9
    out = torch.empty((ci, T, co), dtype=w8.dtype)
    for t in range(T):
        out[:, 8 - t, :] = w8[:, t, :].t()
    return out


def sgd_ref(p, g, lr: float, gscale: float = 1.0) -> torch.Tensor:
    """theta - l * g in float64 with l = float32(lr) * float32(gscale) (an fp32 product)."""
    l = float(np.float32(lr) * np.float32(gscale))
    return p.double() - l * g.double()


def rmsprop_ref(p, g, ms, lr: float, decay: float, gscale: float = 1.0):
    """optimizer.lua:10-14 in float64: gi = g * gscale; ms = decay * ms + (1 - decay) * gi^2;
    theta -= lr * gi / sqrt(ms), with the fp32 constants decay32, 1.f - decay32 and
    float32(lr).  Returns (theta, ms)."""
    d = np.float32(decay)
    omd = np.float32(1.0) - d
    gi = g.double() * float(np.float32(gscale))
    m = float(d) * ms.double() + float(omd) * gi * gi
    return p.double() - float(np.float32(lr)) * gi / m.sqrt(), m


def refresh_expected(w, cinp, KP, Mpad, KPd=0, Mpad_d=0, s_w=None, bias=None, posb=None):
    """Every operand copy weight_refresh / grad_update can write for OHWI fp32 weights w
    [cout][k][k][cin] (CPU): name -> expected tensor.
      wf / wd            layouts.fwd_weight / dgrad_weight
      wf_frag / wd_frag  frag_bf16 of them (3x3, C -> C, C = 128 | 256), or for another kernel
                         size layouts.stack_frag_linear of wf zero-padded to K = 1024
      wf8                e4m3_bytes(w, s_w) at [co][t * cinp + ci]
      wf8_frag, wd8_frag layouts.stack_frag_f8 of the bytes / of dgrad_w8(bytes)
      pbias, pbias_frag  bf16(bias + posb) / layouts.stack_pbias_frag
      amax               |w|.max()"""
    cout, k, _, cin = w.shape
    T = k * k
    w = w.float()
    out = {"wf": LY.fwd_weight(w, cinp, KP, Mpad)}
    if KPd:
        out["wd"] = LY.dgrad_weight(w, KPd, Mpad_d)
    square = T == 9 and cin == cout == cinp and cout in (128, 256)
    if square:
        out["wf_frag"] = frag_bf16(out["wf"], cout)
        if KPd:
            out["wd_frag"] = frag_bf16(out["wd"], cout)
    elif T != 9 and cout in (128, 256) and T * cinp <= 1024:
        A = torch.zeros((cout, 1024), dtype=torch.bfloat16)
        A[:, :T * cinp] = out["wf"][:cout, :T * cinp]
        out["wf_frag"] = LY.stack_frag_linear(A, cout)
    if s_w is not None:
        b = e4m3_bytes(w.reshape(cout, T, cin), s_w)
        tmp = torch.zeros((cout, T, cinp), dtype=torch.uint8)
        tmp[:, :, :cin] = b
        wf8 = torch.zeros((Mpad, KP), dtype=torch.uint8)
        wf8[:cout, :T * cinp] = tmp.reshape(cout, -1)
        out["wf8"] = wf8
        if square:
            out["wf8_frag"] = LY.stack_frag_f8(b)
            out["wd8_frag"] = LY.stack_frag_f8(dgrad_w8(b))
        out["amax"] = w.abs().max()
    if bias is not None:
        out["pbias"] = (bias.float()[None, :] + posb.float()).to(torch.bfloat16)
        if cout in (128, 256):
            out["pbias_frag"] = LY.stack_pbias_frag(bias, posb)
    return out


def gate_places(ng: int) -> dict:
    """name -> gradient index worth poisoning, from finite_gate1's documented launch shape
    (ceil(n4 / 2048) <= 256 blocks of 256 lanes, 4 elements per lane and load, 8 loads in
    flight in the main loop, then a one-load remainder loop, then the n % 4 tail)."""
    n4 = ng // 4
    blocks = max(1, min(256, (n4 + 2047) // 2048))
    stride = blocks * 256
    places = {"first": 0, "last": ng - 1}
    if ng % 4:
        places["tail"] = n4 * 4
    if n4:
        places["last_block"] = 4 * min((blocks - 1) * 256 + 3, n4 - 1) + 2
        i0 = np.arange(stride, dtype=np.int64)
        iters = np.maximum(0, -(-(n4 - 7 * stride - i0) // (8 * stride)))   # main-loop trips
        start = i0 + iters * 8 * stride
        rem = start[start < n4]           # vectors only the remainder loop reads
        if len(rem):
            places["remainder"] = 4 * int(rem[len(rem) // 2]) + 1
    return places


# e4m3 rounding table: value -> byte (at scale 1).  The GPU tests feed the same values.
E4M3_TABLE = [
    (448.0, 0x7E), (464.0, 0x7E), (500.0, 0x7E), (-448.0, 0xFE),
    (2.0 ** -9, 0x01), (2.0 ** -10, 0x00), (3 * 2.0 ** -10, 0x02),     # subnormal, two ties
    (17.0, 0x58), (19.0, 0x5A), (21.0, 0x5A), (23.0, 0x5C),            # ties -> 16 20 20 24
    (0.0, 0x00), (-0.0, 0x80),
]


# --------------------------------------------------------------------------- self-checks
def test_e4m3_bytes_table():
    x = torch.tensor([v for v, _ in E4M3_TABLE], dtype=torch.float32)
    want = torch.tensor([b for _, b in E4M3_TABLE], dtype=torch.uint8)
    assert torch.equal(e4m3_bytes(x, 1.0), want)
    # the ties decode to the even neighbour
    dec = e4m3_bytes(torch.tensor([17.0, 19.0, 21.0, 23.0]), 1.0).view(torch.float8_e4m3fn)
    assert dec.float().tolist() == [16.0, 20.0, 20.0, 24.0]
    # a power-of-two scale moves the table exactly
    for s in (2.0 ** -3, 2.0 ** 4):
        assert torch.equal(e4m3_bytes(x * s, s), want)
    # 1 / s is rounded to fp32 before the product (0.0123 is no power of two)
    s = 0.0123
    inv = np.float32(1.0) / np.float32(s)
    v = torch.tensor([1.0, 0.37, 5.5], dtype=torch.float32)
    q = torch.from_numpy((v.numpy() * inv).astype(np.float32))
    assert torch.equal(e4m3_bytes(v, s), q.to(torch.float8_e4m3fn).view(torch.uint8))


def test_frag_bf16_matches_stack_frag_at_128_and_indexes_256():
    A = torch.arange(128 * 1152, dtype=torch.float64).reshape(128, 1152)
    assert torch.equal(frag_bf16(A, 128), LY.stack_frag(A))
    C = 256
    A = torch.arange(C * 9 * C, dtype=torch.int64).reshape(C, 9 * C)
    f = frag_bf16(A, C)
    assert torch.equal(torch.sort(f).values, torch.arange(C * 9 * C))   # a permutation
    # hand-decoded entries of [h 2][step 36][wm 2][kk 2][i 4][lane 64][e 8]
    f7 = f.reshape(2, 36, 2, 2, 4, 64, 8)
    assert f7[0, 0, 0, 0, 0, 0, 0].item() == A[0, 0].item()
    # h 1, step 9 * 2 + 4 (chunk 2, tap 4), wm 1, kk 1, i 3, lane 37 (row 5, group 2), e 6
    row, col = 128 + 64 + 48 + 5, 4 * C + 128 + 32 + 16 + 6
    assert f7[1, 22, 1, 1, 3, 37, 6].item() == A[row, col].item()
    # the first pass of chunk 0 / 1 is the 128-wide layout of the matching sub-matrix
    sub = torch.cat([A[:128, t * C:t * C + 128] for t in range(9)], dim=1)
    assert torch.equal(f7[0, :18].reshape(-1), LY.stack_frag(sub))


def test_dgrad_w8_indexing():
    w8 = torch.arange(6 * 9 * 5, dtype=torch.int64).reshape(6, 9, 5)
    d = dgrad_w8(w8)
    assert tuple(d.shape) == (5, 9, 6)
    for co, t, ci in [(0, 0, 0), (5, 8, 4), (2, 3, 1), (4, 7, 3)]:
        assert d[ci, 8 - t, co].item() == w8[co, t, ci].item()
    # the bf16 dgrad operand is the same map
    w = torch.randn(128, 3, 3, 128, generator=torch.Generator().manual_seed(4))
    wd = LY.dgrad_weight(w, 1152, 128).reshape(128, 9, 128)
    assert torch.equal(dgrad_w8(w.reshape(128, 9, 128).to(torch.bfloat16)), wd)


def test_sgd_ref_constants_and_cpu_optimizer():
    from deep_go_amd.train.optim import SGD
    g = torch.Generator().manual_seed(0)
    p = torch.randn(1001, generator=g)
    gr = torch.randn(1001, generator=g)
    # l is the fp32 product of the two fp32 roundings
    l = np.float32(0.01) * np.float32(0.37)
    assert type(l) is np.float32
    ref = sgd_ref(p, gr, 0.01, 0.37)
    assert torch.equal(ref, p.double() - float(l) * gr.double())
    opt = SGD(0.01, 1e-3)
    q = p.clone()
    opt.step(q, gr)
    ref1 = sgd_ref(p, gr, 0.01)
    bound = 2.0 ** -23 * (ref1.abs() + (0.01 * gr.double()).abs())
    assert ((q.double() - ref1).abs() <= bound).all()
    assert opt.rate == 0.01 * (1.0 - 1e-3)


def test_rmsprop_ref_matches_cpu_optimizer():
    """rmsprop_ref and train/optim.RMSProp (fp32 torch ops) agree to 1e-6 relative on the mean
    square and on every parameter, over two steps.  Half of the parameters start at 0, where
    theta is the update itself (so the update is held to 1e-6 relative); the rest at
    1 <= |theta| < 2, away from the cancellation of theta near 0 that no relative bound on an
    fp32 difference survives (an update is at most rate / sqrt(1 - decay) = 0.032)."""
    from deep_go_amd.train.optim import RMSProp
    g = torch.Generator().manual_seed(1)
    n = 4096
    sign = (torch.rand(n, generator=g) < 0.5).float() * 2 - 1
    p_big = sign * (1.0 + torch.rand(n, generator=g))
    for p in (torch.zeros(n), p_big):
        opt = RMSProp(0.01, 0.9, n)
        opt.ms = torch.rand(n, generator=g) * 1.999 + 1e-3
        for step in range(2 if p is p_big else 1):
            gr = torch.randn(n, generator=g) * 3.0
            p0, ms0 = p.clone(), opt.ms.clone()
            opt.step(p, gr)
            pr, mr = rmsprop_ref(p0, gr, ms0, 0.01, 0.9)
            assert ((opt.ms.double() - mr).abs() <= 1e-6 * mr).all()
            assert (pr != 0).all()
            assert ((p.double() - pr).abs() <= 1e-6 * pr.abs()).all()
    # gscale multiplies the gradient before it is squared
    pr, mr = rmsprop_ref(p0, gr, ms0, 0.01, 0.9, 0.5)
    pr2, mr2 = rmsprop_ref(p0, gr * 0.5, ms0, 0.01, 0.9)
    assert torch.equal(pr, pr2) and torch.equal(mr, mr2)


def test_rmsprop_zero_gradient_horizon_cpu():
    """1200 zero-gradient steps: the mean square decays into the fp32 denormals and stops
    there (0.9 x the smallest ones rounds back up), the update stays 0 x finite = 0."""
    from deep_go_amd.train.optim import RMSProp
    p = torch.randn(64, generator=torch.Generator().manual_seed(2))
    p0 = p.clone()
    opt = RMSProp(0.01, 0.9, 64)
    z = torch.zeros(64)
    for _ in range(1200):
        opt.step(p, z)
    assert torch.equal(p, p0)
    assert torch.isfinite(opt.ms).all() and (opt.ms > 0).all()


@pytest.mark.parametrize("C", [128, 256])
def test_refresh_expected_is_consistent(C):
    """The combined oracle on a square 3x3 fp8 layer: every fragment order is a permutation of
    its plain copy, and the e4m3 dgrad fragments hold the transposed, tap-flipped bytes."""
    g = torch.Generator().manual_seed(3)
    w = torch.randn(C, 3, 3, C, generator=g) * 0.05
    bias = torch.randn(C, generator=g)
    posb = torch.randn(361, C, generator=g)
    s = float(w.abs().max()) / 448.0
    x = refresh_expected(w, C, 9 * C, C, 9 * C, C, s_w=s, bias=bias, posb=posb)
    srt = lambda t: torch.sort(t.reshape(-1).view(torch.int16).int()).values   # noqa: E731
    assert torch.equal(srt(x["wf_frag"]), srt(x["wf"]))
    assert torch.equal(srt(x["wd_frag"]), srt(x["wd"]))
    s8 = lambda t: torch.sort(t.reshape(-1).int()).values   # noqa: E731
    assert torch.equal(s8(x["wf8_frag"]), s8(x["wf8"]))
    assert torch.equal(s8(x["wd8_frag"]), s8(x["wf8"]))
    # the largest |w| quantizes to the largest e4m3 value
    assert int((x["wf8"] & 0x7F).max()) == 0x7E
    assert x["amax"].item() == w.abs().max().item()
    assert torch.equal(x["pbias"], (posb + bias[None, :]).to(torch.bfloat16))


def test_gate_places_cover_every_loop():
    for ng in (4 * 2048 * 3 - 5, 2200003):
        pl = gate_places(ng)
        assert set(pl) == {"first", "last", "tail", "last_block", "remainder"}
        assert len(set(pl.values())) == 5 and all(0 <= v < ng for v in pl.values())
    assert gate_places(5) == {"first": 0, "last": 4, "tail": 4, "last_block": 2, "remainder": 1}
