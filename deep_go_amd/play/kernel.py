"""``policy_select`` (csrc/kernels/play.hip) on torch tensors: the form the tests and
tools/kbench_play.py call.  ``Predictor.select`` launches the kernel itself, on its own
buffers."""
from __future__ import annotations

import torch

from ..config import NUM_POINTS
from ..ops.native import play, stream_handle


def policy_select(prob: torch.Tensor, game: torch.Tensor, ply: torch.Tensor, seed: int = 0,
                  temperature: float = 1.0, top_p: float = 1.0, out: torch.Tensor = None):
    """prob [n, 361] fp32, game [n] and ply [n] int32, all on the GPU -> (move int32 [n], p_move
    fp32 [n], kept int32 [n]) on the current stream.  out: an int32 tensor of at least 3 n
    words to hold them, in that order (p_move as its fp32 bits)."""
    n = prob.shape[0]
    assert prob.is_cuda and prob.dtype == torch.float32 and prob.is_contiguous()
    assert prob.shape == (n, NUM_POINTS)
    for t in (game, ply):
        assert t.is_cuda and t.dtype == torch.int32 and t.is_contiguous() and t.numel() == n
    if out is None:
        out = torch.empty(3 * n, dtype=torch.int32, device=prob.device)
    assert out.is_cuda and out.dtype == torch.int32 and out.is_contiguous()
    assert out.numel() >= 3 * n
    move, p_move, kept = out[:n], out[n:2 * n], out[2 * n:3 * n]
    play().policy_select(prob.data_ptr(), game.data_ptr(), ply.data_ptr(), n,
                         int(seed) & (2 ** 64 - 1), float(temperature), float(top_p),
                         move.data_ptr(), p_move.data_ptr(), kept.data_ptr(), stream_handle())
    return move, p_move.view(torch.float32), kept
