"""Move selection and self-play (csrc/kernels/play.hip; deep_go_amd/play), measured.

  kernel    policy_select alone at n = 32 and 256 positions: device events around R
            back-to-back launches on one prob buffer (a forward's log-probabilities through
            policy_ensemble), for T = 1 / top_p = 1, T = 0.5 / top_p = 0.9 and T = 0, beside
            policy_ensemble (S = 8, K = 1) over the same positions in the same session.
  selfplay  run_match on 12x128 bf16, 64 lock-step games, 8 symmetries (512 boards per
            forward), random weights, WINDOWS matches of PLIES plies each: games/s and plies/s on
            the host clock, and the
            share of a ply spent in the host engine (masks, planes, moves, the pass rule)
            against Predictor.select (upload, forward, policy_ensemble, policy_select,
            download), whose device part is also timed with events.

Usage: python tools/kbench_play.py kernel [R] | selfplay [PLIES] [GAMES] [WINDOWS]
-> one JSON line per mode.  bench.py is the headline benchmark; this tool only covers what play
adds."""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _events(fn, R):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(R):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return round(1000.0 * e0.elapsed_time(e1) / R, 3)


def kernel(R=2000):
    from deep_go_amd.ops import functional as F
    from deep_go_amd.ops.native import hip, stream_handle
    from deep_go_amd.play.kernel import policy_select
    h, s = hip(), stream_handle()
    out = {"mode": "kernel", "launches": R, "unit": "us per launch"}
    for n in (32, 256):
        rng = np.random.default_rng(n)
        z = torch.from_numpy(rng.normal(0, 2, (n * 8, 361)).astype(np.float32)).cuda()
        logp = torch.log_softmax(z, 1).contiguous()
        stones = torch.from_numpy((rng.random((n, 361)) < 0.4).astype(np.uint8)).cuda()
        r = F.policy_ensemble(logp, stones, None, None, S=8, K=1)
        prob, topk, topk_p, rank = r["prob"], r["topk"], r["topk_p"], r["rank"]
        game = torch.arange(n, dtype=torch.int32, device="cuda")
        ply = torch.full((n,), 17, dtype=torch.int32, device="cuda")
        picks = torch.empty(3 * n, dtype=torch.int32, device="cuda")
        runs = {
            "policy_ensemble_S8_K1": lambda: h.policy_ensemble(
                logp.data_ptr(), stones.data_ptr(), 361, 0, 0, n, 8, 1, 1, prob.data_ptr(),
                topk.data_ptr(), topk_p.data_ptr(), rank.data_ptr(), s),
            "policy_select_T1_p1": lambda: policy_select(prob, game, ply, 3, 1.0, 1.0, picks),
            "policy_select_T0.5_p0.9": lambda: policy_select(prob, game, ply, 3, 0.5, 0.9, picks),
            "policy_select_T0": lambda: policy_select(prob, game, ply, 3, 0.0, 1.0, picks),
        }
        out[f"n{n}"] = {name: [_events(fn, R) for _ in range(5)] for name, fn in runs.items()}
    print(json.dumps(out), flush=True)


def selfplay(plies=300, games=64, windows=5):
    from deep_go_amd.config import get_preset
    from deep_go_amd.play.selfplay import run_match
    from deep_go_amd.predict import Predictor
    cfg = get_preset("12x128-bf16", batchSize=512)
    p = Predictor(cfg, batch=games * 8, symmetries=8, device="gpu", top=1)
    run_match(p, games=games, max_moves=4, seed=1)                   # warm-up
    # the device part of select: events around every call
    spans = []
    real = p.select

    def timed(*a, **kw):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        r = real(*a, **kw)
        e1.record()
        spans.append((e0, e1))
        return r

    p.select = timed
    out = {"mode": "selfplay", "model": "12x128 bf16, random weights", "games": games,
           "symmetries": 8, "boards_per_forward": games * 8, "plies_per_game": plies,
           "windows": []}
    for window in range(windows):                       # one match per window, another seed
        spans.clear()
        torch.cuda.synchronize()
        r = run_match(p, games=games, max_moves=plies, seed=2 + window)
        torch.cuda.synchronize()
        t = r["timing"]
        device = sum(a.elapsed_time(b) for a, b in spans) / 1000.0
        out["windows"].append({
            "seconds": round(t["seconds"], 3), "plies": t["plies"],
            "plies_per_s": round(t["plies"] / t["seconds"], 1),
            "games_per_s_at_this_length": round(games / t["seconds"], 3),
            "ms_per_lockstep_ply": round(1000 * t["seconds"] / plies, 3),
            "host_engine_share": round(t["host_engine_seconds"] / t["seconds"], 4),
            "select_share": round(t["select_seconds"] / t["seconds"], 4),
            "select_device_share": round(device / t["seconds"], 4),
            "ms_per_ply": {"host_engine": round(1000 * t["host_engine_seconds"] / plies, 3),
                           "select_host_clock": round(1000 * t["select_seconds"] / plies, 3),
                           "select_device_events": round(1000 * device / plies, 3)}})
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    mode = sys.argv[1] if len(sys.argv) > 1 else "kernel"
    args = [int(x) for x in sys.argv[2:]]
    {"kernel": kernel, "selfplay": selfplay}[mode](*args)
