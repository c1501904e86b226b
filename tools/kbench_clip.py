"""grad_clip (csrc/kernels/clip.hip, module _dgclip), measured.

  kernel  at the flat sizes of 12x128 and 12x256: device events around R back-to-back launches,
          five timings each in turn, of grad_norm alone (reads 4 bytes per element), the pair
          grad_clip issues when it does not clip (the second launch then only sums the
          partials: 4 bytes per element) and when it clips (12: g read twice, written once),
          beside the sgd kernel of _dghip (12) and the momentum kernel of _dgopt (20) on the
          same vectors, and the one-wave adamw_tick launch as the floor of one more launch.
          The clipping pair's yardstick is sgd's median + the tick's median + sgd's spread.
          The clipping run uses c = 1e-9, below the 1e-6 of the definition, so r < 1 whatever
          the norm and every launch rewrites the gradient (whose values decay to zero within a
          few launches; neither kernel's time depends on the values).  The launches that
          clipped are counted from the record and reported.
  step    the trainer's step through HIPBackend on the packed fixture (12x128 bf16, batch 256,
          input prefetch on, optimizer=adamw): load_next + train_step, K steps per window
          ending in a device synchronise, windows alternating on one device between
          grad_clip = 0, 1e30 (never clips) and 1e-3 (always clips).  The order of the
          variants rotates from round to round, so no variant keeps one place.
  curves  one run pair on the bundled fixture (6x64, adamw, ITERS iterations) with and without
          grad_clip = 1: the logged loss curves, clipped_steps and the range of the norm.

Usage: python tools/kbench_clip.py kernel [R] | step [K] [ROUNDS] | curves [ITERS]
-> one JSON line per mode.  bench.py is the headline benchmark; this tool only covers what
grad_clip adds."""
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
FIXTURE = os.path.join(ROOT, "tests", "fixtures")


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
    from deep_go_amd.config import ExperimentConfig
    from deep_go_amd.models.gocnn import ParamLayout, init_params
    from deep_go_amd.ops.native import adam, clip, hip, opt, stream_handle
    h, o, a, c, s = hip(), opt(), adam(), clip(), stream_handle()
    nbytes = {"grad_norm": 4, "pair_unclipped": 4, "pair_clipping": 12, "sgd": 12,
              "momentum": 20}
    out = {"mode": "kernel", "launches": R, "unit": "us per launch (pair: per two launches)",
           "bytes_per_element": nbytes}
    for ch in (128, 256):
        lay = ParamLayout(ExperimentConfig(numLayers=12, channelSize=ch))
        n = lay.numel
        p = init_params(lay, 1).cuda()
        g0 = torch.zeros(n, device="cuda")                 # sgd's and momentum's: p stays
        g = torch.randn(n, device="cuda", generator=torch.Generator("cuda").manual_seed(1))
        v = torch.zeros(n, device="cuda")
        part = torch.zeros(c.clip_partials(), device="cuda")
        rec = torch.zeros(2, dtype=torch.int64, device="cuda")
        arec = torch.zeros(2, dtype=torch.int64, device="cuda")
        lr = torch.tensor([1e-6], dtype=torch.float64, device="cuda")
        gate = torch.ones(1, device="cuda")
        r = np.ascontiguousarray(np.array(lay.weight_ranges(), dtype=np.int64))
        P, G, LRP, GT = p.data_ptr(), g.data_ptr(), lr.data_ptr(), gate.data_ptr()
        PT, NP, REC = part.data_ptr(), part.numel(), rec.data_ptr()
        runs = {
            "grad_norm": lambda: c.grad_norm(G, n, PT, NP, GT, s),
            "pair_unclipped": lambda: c.grad_clip(G, n, PT, NP, REC, 1e30, 1.0, GT, s),
            "pair_clipping": lambda: c.grad_clip(G, n, PT, NP, REC, 1e-9, 1.0, GT, s),
            "sgd": lambda: h.sgd(P, g0.data_ptr(), n, LRP, 1.0, GT, s),
            "momentum": lambda: o.momentum(P, g0.data_ptr(), v.data_ptr(), n, LRP, 0.9, 1, 1e-4,
                                           r.ctypes.data, len(r), 1.0, GT, s),
            "adamw_tick": lambda: a.adamw_tick(arec.data_ptr(), 0.9, 0.999, GT, s),
        }
        res = {"elements": n, **{k: [] for k in runs}}
        res["clipped_launches"] = {"pair_unclipped": [], "pair_clipping": []}
        for k in range(5):
            for name, fn in runs.items():
                if name == "pair_unclipped":
                    g.normal_()                    # (the clipping run leaves zeros behind)
                before = int(rec[1].item())
                res[name].append(_events(fn, R))
                if name in res["clipped_launches"]:
                    # of R + 1 launches: all of the clipping run, none of the other
                    res["clipped_launches"][name].append(int(rec[1].item()) - before)
        for name in runs:
            med = statistics.median(res[name])
            res[name + "_median"] = med
            if name in nbytes:
                res[name + "_GBps"] = round(nbytes[name] * n / med / 1e3, 1)
        res["sgd_spread_us"] = round(max(res["sgd"]) - min(res["sgd"]), 3)
        res["pair_clipping_spread_us"] = round(
            max(res["pair_clipping"]) - min(res["pair_clipping"]), 3)
        res["pair_clipping_yardstick_us"] = round(
            res["sgd_median"] + res["adamw_tick_median"] + res["sgd_spread_us"], 3)
        res["pair_clipping_minus_yardstick_us"] = round(
            res["pair_clipping_median"] - res["pair_clipping_yardstick_us"], 3)
        assert torch.isfinite(p).all() and torch.isfinite(g).all()
        out[f"12x{ch}"] = res
    print(json.dumps(out), flush=True)


def step(K=300, rounds=6, B=256):
    from deep_go_amd.config import get_preset
    from deep_go_amd.data.dataset import PackedDataset
    from deep_go_amd.data.loader import BatchLoader
    from deep_go_amd.train.backends import HIPBackend
    src = PackedDataset.load(os.path.join(FIXTURE, "train.dgpack.npz"))
    variants = {"clip_off": 0.0, "clip_never": 1e30, "clip_always": 1e-3}
    runs = {}
    for name, clip in variants.items():
        cfg = get_preset("12x128-bf16", batchSize=B, synthetic=False, data_root=FIXTURE,
                         rate=1e-3, optimizer="adamw", weight_decay=1e-2, grad_clip=clip)
        be = HIPBackend(cfg, B)
        assert be.net.load_stream is not None, "input prefetch must be on"
        ld = BatchLoader(src, B, threads=cfg.loader_threads, prefetch=cfg.prefetch,
                         seed=cfg.seed * 1000003)
        runs[name] = (be, ld)

    def window(be, ld, n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            be.load_next(ld)
            be.train_step()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / n * 1e6
    times = {m: [] for m in runs}
    names = list(runs)
    try:
        for be, ld in runs.values():
            window(be, ld, 30)                          # warm-up
        for k in range(rounds):
            for m in names[k % len(names):] + names[:k % len(names)]:
                times[m].append(round(window(*runs[m], K), 2))
    finally:
        for _, ld in runs.values():
            ld.close()
    out = {"mode": "step", "model": "12x128 bf16 adamw", "B": B, "steps_per_window": K,
           "unit": "us per step (load_next + train_step, host clock, device synchronise)"}
    for m, t in times.items():
        out[m] = t
        out[m + "_median"] = round(statistics.median(t), 2)
        out[m + "_spread"] = round(max(t) - min(t), 2)
    for m in ("clip_never", "clip_always"):
        out[m + "_minus_clip_off_median_us"] = round(out[m + "_median"] - out["clip_off_median"], 2)
    steps = 30 + K * rounds
    out["clip_stats"] = {m: list(runs[m][0].clip_stats()) for m in ("clip_never", "clip_always")}
    out["steps_per_backend"] = steps     # (clip_always: every one of them should have clipped)
    for be, _ in runs.values():
        assert torch.isfinite(be.net.params).all()
        be.close()
    print(json.dumps(out), flush=True)


def curves(iters=3000):
    from deep_go_amd.config import get_preset
    from deep_go_amd.train.experiment import Experiment
    from deep_go_amd.utils.metrics import read_jsonl
    out = {"mode": "curves", "model": "6x64 bf16 adamw rate 1e-3, bundled fixture",
           "iterations": iters}
    with tempfile.TemporaryDirectory() as tmp:
        for name, clip in (("clip_off", 0.0), ("clip_1", 1.0)):
            mpath = os.path.join(tmp, name + ".jsonl")
            cfg = get_preset("default-experiment", synthetic=False, data_root=FIXTURE,
                             rate=1e-3, optimizer="adamw", weight_decay=1e-2, grad_clip=clip,
                             log_interval=100, validation_interval=1000, validationSize=512,
                             checkpoint_dir=tmp, metrics_path=mpath)
            e = Experiment(cfg, id=name)
            res = e.run(iters)
            e.metrics.close()
            rows = read_jsonl(mpath)
            r = {"loss_ema_every_100": [round(x["loss_ema"], 4) for x in rows
                                        if x.get("kind") == "train"],
                 "val_cost": [round(x["val_cost"], 4) for x in rows
                              if x.get("kind") == "validation"],
                 "final_train_cost": res["train_cost"], "bad_steps": e.backend.bad_steps()}
            clips = [x for x in rows if x.get("kind") == "clip"]
            if clips:
                norms = [x["grad_norm"] for x in clips]
                r.update(clipped_steps=clips[-1]["clipped_steps"],
                         logged_norm_min=round(min(norms), 4), logged_norm_max=round(max(norms), 4),
                         logged_norms=[round(x, 3) for x in norms])
            out[name] = r
            e.close()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    mode = sys.argv[1] if len(sys.argv) > 1 else "kernel"
    args = [int(x) for x in sys.argv[2:]]
    {"kernel": kernel, "step": step, "curves": curves}[mode](*args)
