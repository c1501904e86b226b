"""Integer test data, float64 CPU oracles and launch wrappers for tolerance-free kernel tests.

MFMA accumulates in fp32.  When every product and every partial sum of an output is an integer
multiple of one power-of-two quantum q and sum |a_k| |x_k| < 2^24 q, the fp32 sum is exact in
ANY order, so a kernel's result before its final rounding is one determined number and
``torch.equal`` against a float64 reference pushed through the same final rounding is the
right assertion (tests/test_exact_gpu.py; the CPU side of this module is checked by
tests/test_exact_cpu.py).

Conventions: activations are NHWC board interiors ``[B][19][19][C]``; an operand matrix is
``A[M][T*Cin]`` with ``k = tap*Cin + c`` (layouts.fwd_weight / dgrad_weight); ReLU bitmasks are
``[B][361][C/8]`` bytes, bit e of byte g = channel 8g + e.  Generators and oracles run on the
CPU and never touch the GPU; the ``run_*`` wrappers move data to the GPU, launch and return
CPU tensors.
"""
from __future__ import annotations

import functools
import math

import numpy as np
import torch
import torch.nn.functional as F

from . import layouts as LY

NPTS = 361
E4M3_MAX = 448.0
E5M2_MAX = 57344.0
FP8_ROWS = 448           # rows per board of the fp8 copy frames (441 + 7 zero rows)


# ------------------------------------------------------------------------------ generators
def _gen(seed: int) -> torch.Generator:
    return torch.Generator().manual_seed(int(seed))


def int_acts(shape, hi: int, seed: int) -> torch.Tensor:
    """Activations in {0 .. hi} (float64)."""
    return torch.randint(0, hi + 1, tuple(shape), generator=_gen(seed)).double()


def int_grads(shape, seed: int, lim: int = 2) -> torch.Tensor:
    """Gradients in {-lim .. lim} (float64)."""
    return torch.randint(-lim, lim + 1, tuple(shape), generator=_gen(seed)).double()


def sign_weights(shape, seed: int) -> torch.Tensor:
    """Dense weights in {-1, +1} (float64): every (row, k) term counts."""
    return torch.randint(0, 2, tuple(shape), generator=_gen(seed)).double() * 2 - 1


def bias_table(cout: int, shift: int = 0) -> torch.Tensor:
    """[361][cout] distinct small integers of (pixel, channel): ((3p + 5c) mod 32) - 8 + shift."""
    p = torch.arange(NPTS).view(-1, 1)
    c = torch.arange(cout).view(1, -1)
    return (((3 * p + 5 * c) % 32) - 8 + shift).double()


def relu_masks(B: int, C: int, seed: int) -> torch.Tensor:
    return torch.randint(0, 256, (B, NPTS, C // 8), generator=_gen(seed)).to(torch.uint8)


def mask_bits(mask: torch.Tensor) -> torch.Tensor:
    """[B][361][C/8] bytes -> [B][19][19][C] float64 0/1."""
    B, _, G = mask.shape
    bits = (mask.long().unsqueeze(-1) >> torch.arange(8)) & 1
    return bits.reshape(B, 19, 19, 8 * G).double()


def pack_mask(nz: torch.Tensor) -> torch.Tensor:
    """[B][19][19][C] bool -> [B][361][C/8] bytes."""
    B, C = nz.shape[0], nz.shape[-1]
    b = nz.reshape(B, NPTS, C // 8, 8).long()
    return (b << torch.arange(8)).sum(-1).to(torch.uint8)


# ------------------------------------------------------------------------------ fp8 emulation
def q_e4m3(x: torch.Tensor) -> torch.Tensor:
    """OCP e4m3 bytes of x: saturate at +-448, round to nearest even."""
    return x.double().clamp(-E4M3_MAX, E4M3_MAX).float().to(torch.float8_e4m3fn).view(torch.uint8)


def q_e5m2(x: torch.Tensor) -> torch.Tensor:
    """e5m2 bytes of x: saturate at +-57344, round to nearest even."""
    return x.double().clamp(-E5M2_MAX, E5M2_MAX).float().to(torch.float8_e5m2).view(torch.uint8)


def d_e4m3(b: torch.Tensor) -> torch.Tensor:
    return b.view(torch.float8_e4m3fn).double()


def d_e5m2(b: torch.Tensor) -> torch.Tensor:
    return b.view(torch.float8_e5m2).double()


def bf16_round(x: torch.Tensor) -> torch.Tensor:
    """The final rounding of a bf16 store (nearest even) of an exactly known fp32 value."""
    return x.float().to(torch.bfloat16).double()


# ------------------------------------------------------------------------------ the condition
def quantum(t: torch.Tensor) -> float:
    """The largest power of two in [2^-24, 2^16] of which every entry of t is a multiple."""
    t = t.double()
    for e in range(16, -25, -1):
        v = t / 2.0 ** e
        if torch.equal(v, v.round()):
            return 2.0 ** e
    raise AssertionError("entries are not multiples of 2^-24")


def _conv_w(A: torch.Tensor, M: int, cin: int, k: int) -> torch.Tensor:
    """Operand matrix -> conv2d weight [M][cin][k][k]."""
    return A[:M, :k * k * cin].reshape(M, k, k, cin).permute(0, 3, 1, 2).contiguous()


def conv64(x: torch.Tensor, A: torch.Tensor, k: int = 3) -> torch.Tensor:
    """out[b][p][r] = sum_{tap, c} A[r][tap*Cin + c] x[b][p + off(tap)][c], zero padded, float64."""
    cin = x.shape[-1]
    M = A.shape[0]
    y = F.conv2d(x.double().permute(0, 3, 1, 2), _conv_w(A.double(), M, cin, k),
                 padding=(k - 1) // 2)
    return y.permute(0, 2, 3, 1).contiguous()


def assert_order_independent(absx, absw, q: float, bias=None, ref=None, k: int = 3,
                             kind: str = "conv"):
    """The condition under which an fp32 sum of the products is exact in any order, from the
    INPUTS only (CPU): every product (and the bias) is a multiple of the power-of-two quantum q
    — quantum(x) quantum(w) is — and conv(|x|, |w|).max() + |bias|.max() < 2^24 q.
    kind='wgrad': the sum over boards and pixels of |dz| |x| instead (absx = |x| NHWC, absw =
    |dz| NHWC).  ``ref`` (optional): a float64 reference that is stored as bf16 and compared
    UNROUNDED — it must then be at most 256 q in magnitude (every multiple of q up to there is
    a bf16 number)."""
    absx, absw = absx.double().abs(), absw.double().abs()
    assert math.log2(q) == round(math.log2(q)), "q must be a power of two"
    qp = quantum(absx) * quantum(absw)
    assert qp >= q, f"products are multiples of {qp} only, not of q = {q}"
    if bias is not None:
        assert quantum(bias) >= q, "bias is not a multiple of q"
    if kind == "wgrad":
        bound = wgrad64(absw, absx, k).max().item()
    else:
        bound = conv64(absx, absw, k).max().item()
    if bias is not None:
        bound += bias.double().abs().max().item()
    assert bound < 2 ** 24 * q, f"sum |a||x| = {bound} >= 2^24 q (q = {q})"
    if ref is not None:
        r = ref.double()
        assert r.abs().max().item() <= 256 * q, f"|ref| max {r.abs().max().item()} > 256 q"
        assert torch.equal(r / q, (r / q).round()), "reference is not a multiple of q"
    return bound


def shuffled_fp32_conv(x: torch.Tensor, A: torch.Tensor, seed: int, k: int = 3) -> torch.Tensor:
    """The same sum as conv64 evaluated in float32, one product at a time, with K visited in a
    shuffled order: equal to conv64 bit for bit exactly when the sum is order independent."""
    B, cin = x.shape[0], x.shape[-1]
    M = A.shape[0]
    cols = F.unfold(x.float().permute(0, 3, 1, 2), k, padding=(k - 1) // 2)    # B, cin*k*k, 361
    w = _conv_w(A.float(), M, cin, k).reshape(M, -1)                           # M, cin*k*k
    acc = torch.zeros(B, M, NPTS, dtype=torch.float32)
    for j in torch.randperm(w.shape[1], generator=_gen(seed)).tolist():
        acc += w[:, j].view(1, M, 1) * cols[:, j].view(B, 1, NPTS)
    return acc.permute(0, 2, 1).reshape(B, 19, 19, M)


# ------------------------------------------------------------------------------ oracles
def fwd64(x, A, pb=None, k: int = 3):
    """Forward layer: v = relu(conv + pb[p][r]) float64 (pb None: linear, no ReLU)."""
    v = conv64(x, A, k)
    if pb is None:
        return v
    return (v + pb.double().reshape(1, 19, 19, -1)).relu()


def dgrad64(x, A, mask, k: int = 3):
    """Backward-data layer gated by the ReLU bitmask of the layer below."""
    return conv64(x, A, k) * mask_bits(mask)


def wgrad64(dz, x, k: int = 3):
    """dW[co][tap][ci] = sum_{b, p} dz[b][p][co] x[b][p + off(tap)][ci] as OHWI float64."""
    co, ci = dz.shape[-1], x.shape[-1]
    g = torch.nn.grad.conv2d_weight(x.double().permute(0, 3, 1, 2).contiguous(), (co, ci, k, k),
                                    dz.double().permute(0, 3, 1, 2).contiguous(),
                                    padding=(k - 1) // 2)
    return g.permute(0, 2, 3, 1).contiguous()


def bias_partials64(dz, bt: int):
    """Pass 1 of the bias gradients over chunks of bt boards: (part [nch][361][C], rowpart
    [nch][19][C]) float64."""
    B, C = dz.shape[0], dz.shape[-1]
    nch = (B + bt - 1) // bt
    part = torch.zeros(nch, 19, 19, C, dtype=torch.float64)
    for ch in range(nch):
        part[ch] = dz[ch * bt:(ch + 1) * bt].double().sum(0)
    return part.reshape(nch, NPTS, C), part.sum(2)


def stack64(x, As, pbs=None, masks=None, k0: int = 3):
    """bf16 stack chain (conv_stack2 / conv_layer2): per layer the unrounded float64 value v and
    the stored bf16 frame interior y = bf16(v); the next layer reads y.  pbs: forward; masks:
    backward-data.  k0: kernel size of layer 0 (5 in l1 mode).  Returns [(v, y, inp)]."""
    out = []
    for l, A in enumerate(As):
        k = k0 if l == 0 else 3
        v = fwd64(x, A, pbs[l], k) if pbs is not None else dgrad64(x, A, masks[l], k)
        y = bf16_round(v)
        out.append((v, y, x))
        x = y
    return out


def stack_f8_64(x, W8, s, ws, pbs=None, masks=None):
    """conv_stack_f8 emulation.  x: bf16-exact input interior; W8 [C][9][C] e4m3 operand bytes
    per layer; s [nl + 1] input / output scales, ws [nl] weight scales (powers of two).  Forward
    (pbs): e4m3 images, v = relu(s_in s_w acc + pb); backward-data (masks): e5m2 images,
    v = s_in s_w acc * mask bit.  Non-last layers store q(v / s_out) (bytes) and the bf16 frame
    bf16(q * s_out); the last stores bf16(v).  Returns dict: x8 (input bytes), and per layer
    v, y (frame interior), y8 (bytes or None), xin (dequantized operand values / s_in)."""
    fwd = pbs is not None
    q, d = (q_e4m3, d_e4m3) if fwd else (q_e5m2, d_e5m2)
    nl = len(W8)
    xb = q(x.double() / s[0])
    res = {"x8": xb, "layers": []}
    for l in range(nl):
        C = W8[l].shape[0]
        A = d_e4m3(W8[l]).reshape(C, 9 * C)
        xq = d(xb)
        acc = conv64(xq, A)
        v = acc * (s[l] * ws[l])
        v = (v + pbs[l].double().reshape(1, 19, 19, -1)).relu() if fwd else v * mask_bits(masks[l])
        if l == nl - 1:
            y8, y = None, bf16_round(v)
        else:
            y8 = q(v / s[l + 1])
            y = bf16_round(d(y8) * s[l + 1])
        res["layers"].append({"v": v, "y": y, "y8": y8, "xq": xq, "A": A})
        xb = y8
    return res


# ------------------------------------------------------------------------------ layouts
def frag_bf16(A: torch.Tensor, C: int) -> torch.Tensor:
    """conv_stack2 / conv_layer2 A-operand order of a [C][9 C] operand matrix (C = 128 | 256):
    flat [h C/128][step = chunk*9 + tap][wm 2][kk 2][i 4][lane 64][e 8] with row 128h + 64wm +
    16i + (lane & 15), column tap*C + 64 chunk + 32kk + 8(lane >> 4) + e (layouts.stack_frag at
    C = 128)."""
    a = A[:C, :9 * C].reshape(C // 128, 2, 4, 16, 9, C // 64, 2, 4, 8)   # h wm i lr|tap ch kk lq e
    return a.permute(0, 5, 4, 1, 6, 2, 7, 3, 8).reshape(-1).contiguous()


def frame_of(x: torch.Tensor, pad: int = 1, dev="cuda") -> torch.Tensor:
    """NHWC interior (CPU) -> zero-bordered bf16 frame on the GPU."""
    B, C = x.shape[0], x.shape[-1]
    fr = LY.alloc_frame(B, C, pad, dev)
    LY.frame_interior(fr, pad).copy_(x.to(torch.bfloat16))
    return fr


def fp8_frame_of(b8: torch.Tensor, dev="cuda") -> torch.Tensor:
    """fp8 bytes of an NHWC interior [B][19][19][C] -> the [B][448][C] byte frame on the GPU."""
    B, C = b8.shape[0], b8.shape[-1]
    fr = torch.zeros(B, 21, 21, C, dtype=torch.uint8)
    fr[:, 1:20, 1:20] = b8
    out = torch.zeros(B, FP8_ROWS, C, dtype=torch.uint8)
    out[:, :441] = fr.reshape(B, 441, C)
    return out.to(dev)


def fp8_frame_split(fr: torch.Tensor):
    """[B][448][C] byte frame (CPU) -> (interior [B][19][19][C], everything else summed)."""
    B, C = fr.shape[0], fr.shape[-1]
    f = fr[:, :441].reshape(B, 21, 21, C)
    inner = f[:, 1:20, 1:20]
    return inner, int(fr.long().sum().item() - inner.long().sum().item())


def frame_split(fr: torch.Tensor):
    """bf16 frame (any device) -> (interior float64 CPU, sum |border|)."""
    f = fr.detach().cpu().double()
    inner = f[:, 1:20, 1:20]
    return inner.contiguous(), (f.abs().sum() - inner.abs().sum()).item()


# ------------------------------------------------------------------------------ launches
def _hip():
    from .native import hip, stream_handle
    return hip(), stream_handle()


def run_stack2(epi: str, As, x, pbs=None, masks=None, l1: bool = False, dev="cuda"):
    """conv_stack2 over len(As) layers.  epi 'fwd' (pbs: [361][128] tables, ReLU masks written)
    | 'dgrad' (masks read).  l1: row 0 is the 5x5 / 40-channel first layer ([128][1024] operand,
    k = tap*40 + c) over the pad-2 frame of x [B][19][19][40].  Returns (frames, masks) on the
    CPU: whole bf16 frames [B][21][21][128] and the mask bytes."""
    h, st = _hip()
    nl, B = len(As), x.shape[0]
    xf = frame_of(x, 2 if l1 else 1, dev)
    ops = []
    for l, A in enumerate(As):
        a16 = A.to(torch.bfloat16).to(dev)
        ops.append(LY.stack_frag_linear(a16, 128) if (l1 and l == 0) else LY.stack_frag(a16))
    ys = [LY.alloc_frame(B, 128, 1, dev) for _ in range(nl)]
    fwd = epi == "fwd"
    if fwd:
        ms = [torch.zeros(B, NPTS, 16, dtype=torch.uint8, device=dev) for _ in range(nl)]
        pf = [LY.stack_pbias_frag(torch.zeros(128, device=dev), pb.float().to(dev)) for pb in pbs]
    else:
        ms = [m.to(dev) for m in masks]
        pf = None
    tab = np.array([[ops[i].data_ptr(), pf[i].data_ptr() if fwd else 0, ys[i].data_ptr(),
                     ms[i].data_ptr()] for i in range(nl)], dtype=np.int64)
    h.conv_stack2(h.EPI_FWD if fwd else h.EPI_DGRAD, tab.ctypes.data, nl, xf.data_ptr(),
                  int(l1), B, st)
    torch.cuda.synchronize()
    return [y.cpu() for y in ys], [m.cpu() for m in ms]


def run_layer2(epi: str, C: int, As, x, pbs=None, masks=None, multi: bool = False, dev="cuda"):
    """conv_layer2 (one launch per layer) or conv_layer2_multi (one launch) over len(As) 3x3
    C -> C layers, C = 256 | 128; arguments and results as run_stack2."""
    h, st = _hip()
    nl, B = len(As), x.shape[0]
    fwd = epi == "fwd"
    xs = [frame_of(x, 1, dev)] + [LY.alloc_frame(B, C, 1, dev) for _ in range(nl)]
    ops = [frag_bf16(A.to(torch.bfloat16).to(dev), C) for A in As]
    if fwd:
        ms = [torch.zeros(B, NPTS, C // 8, dtype=torch.uint8, device=dev) for _ in range(nl)]
        pf = [LY.stack_pbias_frag(torch.zeros(C, device=dev), pb.float().to(dev)) for pb in pbs]
    else:
        ms = [m.to(dev) for m in masks]
        pf = None
    e = h.EPI_FWD if fwd else h.EPI_DGRAD
    rows = [[ops[i].data_ptr(), pf[i].data_ptr() if fwd else 0, xs[i].data_ptr(),
             xs[i + 1].data_ptr(), ms[i].data_ptr()] for i in range(nl)]
    if multi:
        tab = np.array(rows, dtype=np.int64)
        h.conv_layer2_multi(e, tab.ctypes.data, nl, C, B, st)
    else:
        for r in rows:
            h.conv_layer2(e, *r, C, B, st)
    torch.cuda.synchronize()
    return [y.cpu() for y in xs[1:]], [m.cpu() for m in ms]


def run_stack_f8(C: int, epi: str, W8, x, s, ws, pbs=None, masks=None, y8: bool = False,
                 sr_step=None, dev="cuda"):
    """conv_stack_f8 over len(W8) layers (operands: [C][9][C] e4m3 bytes).  y8: the production
    variant — fp8 copies of the input and of every non-last output, no bf16 frame for the
    non-last layers.  sr_step (backward-data): the step counter value seeding stochastic
    rounding.  Returns dict of CPU tensors: frames (None where not written), masks, amax
    [nl + 1] float32, x8 / y8 byte frames [B][448][C] (y8 variant)."""
    h, st = _hip()
    nl, B = len(W8), x.shape[0]
    fwd = epi == "fwd"
    xf = frame_of(x, 1, dev)
    sd = torch.tensor(list(s), dtype=torch.float32, device=dev)
    wsd = torch.tensor(list(ws), dtype=torch.float32, device=dev)
    amax = torch.zeros(nl + 1, dtype=torch.int32, device=dev)
    frags = [LY.stack_frag_f8(w.to(dev)) for w in W8]
    ys = [None if (y8 and l < nl - 1) else LY.alloc_frame(B, C, 1, dev) for l in range(nl)]
    if fwd:
        ms = [torch.zeros(B, NPTS, C // 8, dtype=torch.uint8, device=dev) for _ in range(nl)]
        pf = [LY.stack_pbias_frag(torch.zeros(C, device=dev), pb.float().to(dev)) for pb in pbs]
    else:
        ms = [m.to(dev) for m in masks]
        pf = None
    tab = np.array([[frags[i].data_ptr(), pf[i].data_ptr() if fwd else 0,
                     0 if ys[i] is None else ys[i].data_ptr(), ms[i].data_ptr(),
                     sd.data_ptr() + 4 * i, wsd.data_ptr() + 4 * i, sd.data_ptr() + 4 * (i + 1),
                     amax.data_ptr() + 4 * (i + 1)] for i in range(nl)], dtype=np.int64)
    c8 = [torch.zeros(B, FP8_ROWS, C, dtype=torch.uint8, device=dev) for _ in range(nl)] if y8 else []
    y8t = np.array([c.data_ptr() for c in c8] + [0], dtype=np.int64)
    step = None
    if sr_step is not None:
        step = torch.full((1,), int(sr_step), dtype=torch.int64, device=dev)
    if fwd:
        if y8:
            h.conv_stack_f8_y8(C, h.EPI_FWD, tab.ctypes.data, nl, xf.data_ptr(), sd.data_ptr(),
                               amax.data_ptr(), B, y8t.ctypes.data, st)
        else:
            h.conv_stack_f8(C, h.EPI_FWD, tab.ctypes.data, nl, xf.data_ptr(), sd.data_ptr(),
                            amax.data_ptr(), B, st)
    else:
        h.conv_stack_f8_dgrad(C, tab.ctypes.data, nl, xf.data_ptr(), sd.data_ptr(),
                              amax.data_ptr(), B, y8t.ctypes.data if y8 else 0,
                              0 if step is None else step.data_ptr(), st)
    torch.cuda.synchronize()
    return {"frames": [None if y is None else y.cpu() for y in ys],
            "masks": [m.cpu() for m in ms], "amax": amax.view(torch.float32).cpu(),
            "x8": c8[0].cpu() if y8 else None, "y8": [c.cpu() for c in c8[1:]]}


def new_step_tag(dev="cuda") -> torch.Tensor:
    """The int64 {step counter, bad-step tag} pair the gradient producers take as ``sf``."""
    return torch.tensor([5, 0], dtype=torch.int64, device=dev)


def run_wgrad_win8(dz, x, s_dz: float, s_x: float, splits=None, dev="cuda"):
    """conv_wgrad_win8 + the slab reduce.  dz [B][19][19][M] / x [B][19][19][Cx]: VALUES, stored
    as e5m2(dz / s_dz) and e4m3(x / s_x) bytes in 448-row frames.  Returns (dW OHWI fp32 CPU,
    the step-tag words after the launches, splits used)."""
    h, st = _hip()
    B, M, Cx = dz.shape[0], dz.shape[-1], x.shape[-1]
    if splits is None:
        splits = h.conv_wgrad_win8_splits(1, M, Cx, B,
                                          torch.cuda.get_device_properties(dev).multi_processor_count)
    KP, Mpad = 9 * Cx, LY.round_up(M, 128)
    d8 = fp8_frame_of(q_e5m2(dz / s_dz), dev)
    x8 = fp8_frame_of(q_e4m3(x / s_x), dev)
    sc = torch.tensor([s_dz, s_x], dtype=torch.float32, device=dev)
    slab = torch.full((splits * Mpad * KP,), float("nan"), dtype=torch.float32, device=dev)
    out = torch.empty((M, 3, 3, Cx), dtype=torch.float32, device=dev)
    sf = new_step_tag(dev)
    tab = np.array([[d8.data_ptr(), x8.data_ptr(), slab.data_ptr(), sc.data_ptr(),
                     sc.data_ptr() + 4]], dtype=np.int64)
    h.conv_wgrad_win8(tab.ctypes.data, 1, M, Mpad, Cx, B, KP, splits, sf.data_ptr(), st)
    h.wgrad_reduce(slab.data_ptr(), out.data_ptr(), splits, M, Mpad, KP, 9, Cx, Cx,
                   0, 0, 0, 0, sf.data_ptr(), st)
    torch.cuda.synchronize()
    return out.cpu(), sf.cpu(), splits


def run_wgrad_multi(dzs, xs, splits: int, dev="cuda"):
    """conv_wgrad_multi over same-shape 3x3 layers (+ one slab reduce per layer).  dzs / xs:
    lists of NHWC interiors.  Returns (the OHWI fp32 gradients, the step-tag words) on the CPU."""
    h, st = _hip()
    nl = len(dzs)
    B, M, Cx = dzs[0].shape[0], dzs[0].shape[-1], xs[0].shape[-1]
    KP, Mpad = 9 * Cx, LY.round_up(M, 128)
    dzf = [frame_of(d, 1, dev) for d in dzs]
    xf = [frame_of(v, 1, dev) for v in xs]
    slabs = [torch.full((splits * Mpad * KP,), float("nan"), dtype=torch.float32, device=dev)
             for _ in range(nl)]
    outs = [torch.empty((M, 3, 3, Cx), dtype=torch.float32, device=dev) for _ in range(nl)]
    tab = np.array([[dzf[i].data_ptr(), xf[i].data_ptr(), slabs[i].data_ptr()]
                    for i in range(nl)], dtype=np.int64)
    sf = new_step_tag(dev)
    h.conv_wgrad_multi(3, tab.ctypes.data, nl, 1, M, Mpad, 1, Cx, B, KP, splits, st)
    for i in range(nl):
        h.wgrad_reduce(slabs[i].data_ptr(), outs[i].data_ptr(), splits, M, Mpad, KP, 9, Cx, Cx,
                       0, 0, 0, 0, sf.data_ptr(), st)
    torch.cuda.synchronize()
    return [o.cpu() for o in outs], sf.cpu()


def run_bias_partials(dz, multi: bool, s8=None, dev="cuda"):
    """bias_grad_partial (chunks of 16 boards) or bias_grad_partial_multi (chunks of 64) on the
    bf16 frame of dz, or (multi, s8 given) on its e5m2 copy e5m2(dz / s8) with scale s8.
    Every slot is pre-filled with NaN.  Returns (part [nch][361][C], rowpart [nch][19][C],
    step-tag words or None) on the CPU."""
    h, st = _hip()
    B, C = dz.shape[0], dz.shape[-1]
    nch = h.bias_chunks_multi(B) if multi else h.bias_chunks(B)
    part = torch.full((nch * (NPTS + 19) * C,), float("nan"), dtype=torch.float32, device=dev)
    sf = None
    if multi:
        sf = new_step_tag(dev)
        if s8 is None:
            fr, sp = frame_of(dz, 1, dev), 0
        else:
            fr = fp8_frame_of(q_e5m2(dz / s8), dev)
            sc = torch.tensor([s8], dtype=torch.float32, device=dev)
            sp = sc.data_ptr()
        tab = np.array([[fr.data_ptr(), part.data_ptr(), sp]], dtype=np.int64)
        h.bias_grad_partial_multi(tab.ctypes.data, 1, B, C, 1, sf.data_ptr(), st)
    else:
        fr = frame_of(dz, 1, dev)
        h.bias_grad_partial(fr.data_ptr(), B, C, 1, part.data_ptr(), st)
    torch.cuda.synchronize()
    p = part.cpu()
    return (p[:nch * NPTS * C].view(nch, NPTS, C), p[nch * NPTS * C:].view(nch, 19, C),
            None if sf is None else sf.cpu())


# ------------------------------------------------------------------------------ cases
# Inputs + float64 references of the shapes tests/test_exact_gpu.py launches.  Each builder runs
# assert_order_independent on its inputs (the chained layers: on the reference chain's
# activations, which are a function of the inputs alone) BEFORE anything is launched, and is
# cached: one reference per shape, shared by the tests that need it and never modified.
@functools.lru_cache(maxsize=None)
def stack_case(C: int, B: int, nl: int, epi: str, seed: int, l1: bool = False):
    """bf16 stack / layer chain: x in {0, 1} (forward) or {-2 .. 2} (backward-data), dense
    +-1 operands, the integer bias tables / random ReLU masks.  l1: layer 0 is 5x5 over 40
    channels."""
    c0, k0 = (40, 5) if l1 else (C, 3)
    fwd = epi == "fwd"
    # (C = 256 backward-data: {-1, 0, 1} keeps layer 0 within the bf16 integers, |v| <= 256)
    x = (int_acts((B, 19, 19, c0), 1, seed) if fwd
         else int_grads((B, 19, 19, c0), seed, 2 if C == 128 else 1))
    As = []
    for l in range(nl):
        kk, cin = (k0 * k0 * c0, c0) if l == 0 else (9 * C, C)
        A = sign_weights((C, kk), seed + 10 + l)
        if l1 and l == 0:   # K zero-padded 1000 -> 1024
            A = torch.cat([A, torch.zeros(C, 24, dtype=torch.float64)], 1)
        As.append(A)
    pbs = [bias_table(C, l) for l in range(nl)] if fwd else None
    masks = None if fwd else [relu_masks(B, C, seed + 20 + l) for l in range(nl)]
    ref = stack64(x, As, pbs, masks, k0)
    for l, (v, y, inp) in enumerate(ref):
        k = k0 if l == 0 else 3
        assert_order_independent(inp, As[l][:, :k * k * inp.shape[-1]], 1.0,
                                 bias=pbs[l] if fwd else None, k=k)
    # layer 0 is compared unrounded: an integer of at most 256
    assert_order_independent(ref[0][2], As[0][:, :k0 * k0 * c0], 1.0, ref=ref[0][0], k=k0)
    return {"x": x, "As": As, "pbs": pbs, "masks": masks, "ref": ref}


def e4m3_sign_bytes(shape, seed: int) -> torch.Tensor:
    """e4m3 bytes of dense +-1 weights (0x38 | 0xB8)."""
    return q_e4m3(sign_weights(shape, seed))


@functools.lru_cache(maxsize=None)
def stack_f8_case(C: int, B: int, nl: int, epi: str, seed: int, log2_sw: int = 0,
                  log2_sy: int = 0, sparse: bool = False):
    """fp8 stack: forward x in {0, 1, 2} (e4m3 at scale 1), backward-data x in {-2 .. 2} (e5m2
    at scale 1); e4m3 operand bytes +-1 with s_w = 2^log2_sw, output scales 2^log2_sy.
    sparse (backward-data): one nonzero input channel, nonzero on a checkerboard only, so that
    every |acc| of layer 0 is at most 5: exactly representable in e5m2 at scale 1."""
    fwd = epi == "fwd"
    if sparse:
        x = torch.zeros(B, 19, 19, C, dtype=torch.float64)
        hh, ww = torch.meshgrid(torch.arange(19), torch.arange(19), indexing="ij")
        x[..., 7] = int_grads((B, 19, 19), seed, 1) * ((hh + ww) % 2 == 0)
    else:
        x = int_acts((B, 19, 19, C), 2, seed) if fwd else int_grads((B, 19, 19, C), seed)
    W8 = [e4m3_sign_bytes((C, 9, C), seed + 10 + l) for l in range(nl)]
    s = (1.0,) + tuple(2.0 ** log2_sy for _ in range(nl))
    ws = tuple(2.0 ** log2_sw for _ in range(nl))
    pbs = [bias_table(C, l) for l in range(nl)] if fwd else None
    masks = None if fwd else [relu_masks(B, C, seed + 20 + l) for l in range(nl)]
    ref = stack_f8_64(x, W8, s, ws, pbs, masks)
    assert torch.equal((d_e4m3 if fwd else d_e5m2)(ref["x8"]), x)   # the input is fp8-exact
    for l, L in enumerate(ref["layers"]):
        deq = s[l] * ws[l]
        qa = quantum(L["xq"]) * quantum(L["A"])
        assert_order_independent(L["xq"], L["A"], qa, bias=pbs[l] / deq if fwd else None)
        # v = fma(acc, deq, bias) is one rounding of an exactly representable number
        assert L["v"].abs().max().item() < 2 ** 24 * qa * deq
    return {"x": x, "W8": W8, "s": s, "ws": ws, "pbs": pbs, "masks": masks, "ref": ref}


@functools.lru_cache(maxsize=None)
def wgrad_case(B: int, cin: int, cout: int, k: int, seed: int, cin_real: int | None = None):
    """dz in {-2 .. 2}, x in {0, 1, 2} (channels >= cin_real zero); reference OHWI float64."""
    dz = int_grads((B, 19, 19, cout), seed)
    x = int_acts((B, 19, 19, cin), 2, seed + 1)
    if cin_real is not None:
        x[..., cin_real:] = 0
    assert_order_independent(x, dz, 1.0, k=k, kind="wgrad")
    return {"dz": dz, "x": x, "ref": wgrad64(dz, x, k)}


@functools.lru_cache(maxsize=None)
def conv_case(B: int, cin: int, cout: int, k: int, seed: int, hi: int = 1):
    """One conv layer in OHWI terms: x in {0 .. hi}, w +-1 [cout][k][k][cin], integer bias
    table, dz in {-2 .. 2} and a {0, 1} activation that gates the backward-data result."""
    x = int_acts((B, 19, 19, cin), hi, seed)
    w = sign_weights((cout, k, k, cin), seed + 1)
    A = w.reshape(cout, k * k * cin)
    pb = bias_table(cout)
    dz = int_grads((B, 19, 19, cout), seed + 2)
    aux = int_acts((B, 19, 19, cin), 1, seed + 3)
    Ad = w.reshape(cout, k * k, cin).flip(1).permute(2, 1, 0).reshape(cin, k * k * cout)
    lin = conv64(x, A, k)
    # ({0, 1} inputs: the forward results are compared unrounded, integers of at most 256)
    assert_order_independent(x, A, 1.0, bias=pb, k=k, ref=lin if hi == 1 else None)
    assert_order_independent(dz, Ad, 1.0, k=k)
    return {"x": x, "w": w, "pb": pb, "dz": dz, "aux": aux,
            "lin": lin, "fwd": fwd64(x, A, pb, k),
            "dgrad": conv64(dz, Ad, k) * (aux > 0)}


def nchw(x: torch.Tensor) -> torch.Tensor:
    return x.permute(0, 3, 1, 2).contiguous()


def nhwc(x: torch.Tensor) -> torch.Tensor:
    return x.permute(0, 2, 3, 1).contiguous()


def shifted(x: torch.Tensor, tap: int, k: int = 3) -> torch.Tensor:
    """x[b][p + off(tap)][c] with zero padding (tap = kh*k + kw, off = (kh - pad, kw - pad))."""
    pad = (k - 1) // 2
    dh, dw = tap // k - pad, tap % k - pad
    xp = F.pad(x, (0, 0, pad, pad, pad, pad))
    return xp[:, pad + dh:pad + dh + 19, pad + dw:pad + dw + 19]
