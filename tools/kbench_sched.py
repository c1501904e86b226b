"""lr_schedule (csrc/kernels/sched.hip, module _dgsched), measured.

  kernel  device events around R back-to-back launches, five timings each in turn, of
          lr_sched_tick (every kind, advance = 1) beside ema_tick (_dgema) and adamw_tick
          (_dgadam): three one-wave launches.  The yardstick of lr_sched_tick is ema_tick's median
          + the spread of ema_tick's own timings.
  step    the trainer's step through HIPBackend on the packed fixture (12x128 bf16, batch 256,
          input prefetch on): load_next + train_step, K steps per window ending in a device
          synchronise, windows alternating on one device between lr_schedule = none and cosine.
          OPT: sgd (the fused, deferred update) | adamw.  The order of the variants rotates from
          round to round, so no variant keeps one place (profiles/clip.txt describes the position
          effect between backends built in one process; FIRST = 1 builds the cosine backend first
          instead).
  curves  one run pair on the bundled fixture (6x64, adamw, rate 1e-3, ITERS iterations,
          ema_decay = 0.999) with lr_schedule = none and cosine lr_warmup=100: the train loss, and
          the test split's cost and top-1 of the weights and of the average at the end.

Usage: python tools/kbench_sched.py kernel [R] | step OPT [K] [ROUNDS] [FIRST] | curves [ITERS]
-> one JSON line per mode.  bench.py is the headline benchmark; this tool only covers what
lr_schedule adds."""
import json
import os
import statistics
import sys
import tempfile
import time

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
    from deep_go_amd.config import LR_KINDS
    from deep_go_amd.ops.native import adam, ema, sched, stream_handle
    m, e, a, s = sched(), ema(), adam(), stream_handle()
    rec = torch.zeros(2, dtype=torch.int64, device="cuda")
    erec = torch.zeros(2, dtype=torch.int64, device="cuda")
    arec = torch.zeros(2, dtype=torch.int64, device="cuda")
    lr = torch.zeros(1, dtype=torch.float64, device="cuda")
    gate = torch.ones(1, device="cuda")
    REC, LRP, GT = rec.data_ptr(), lr.data_ptr(), gate.data_ptr()
    runs = {f"lr_sched_tick_{kind}": (lambda k=k: m.lr_sched(REC, LRP, k, 200, 10 ** 6, 0.1, 1000,
                                                              0.5, 1e-7, 1, s))
            for k, kind in enumerate(LR_KINDS)}
    runs["ema_tick"] = lambda: e.ema_tick(erec.data_ptr(), 0.999, GT, s)
    runs["adamw_tick"] = lambda: a.adamw_tick(arec.data_ptr(), 0.9, 0.999, GT, s)
    out = {"mode": "kernel", "launches": R, "unit": "us per launch"}
    res = {k: [] for k in runs}
    rec[0:1].view(torch.float64).fill_(0.01)
    for _ in range(5):
        for name, fn in runs.items():
            res[name].append(_events(fn, R))
    for name in runs:
        out[name] = res[name]
        out[name + "_median"] = statistics.median(res[name])
    out["ema_tick_spread_us"] = round(max(res["ema_tick"]) - min(res["ema_tick"]), 3)
    out["yardstick_us"] = round(out["ema_tick_median"] + out["ema_tick_spread_us"], 3)
    for kind in LR_KINDS:
        out[f"{kind}_minus_yardstick_us"] = round(
            out[f"lr_sched_tick_{kind}_median"] - out["yardstick_us"], 3)
    # every launch counted
    assert int(rec[1].item()) == 5 * len(LR_KINDS) * (R + 1) and torch.isfinite(lr).all()
    return out


def step(opt="sgd", K=300, rounds=6, first=0, B=256):
    from deep_go_amd.config import get_preset
    from deep_go_amd.data.dataset import PackedDataset
    from deep_go_amd.data.loader import BatchLoader
    from deep_go_amd.train.backends import HIPBackend
    K, rounds, first = int(K), int(rounds), int(first)
    src = PackedDataset.load(os.path.join(FIXTURE, "train.dgpack.npz"))
    total = 30 + K * rounds
    variants = {"none": {}, "cosine": dict(lr_schedule="cosine", lr_warmup=100, lr_total=total)}
    if first:
        variants = dict(reversed(variants.items()))
    okw = dict(rate=1e-3, weight_decay=1e-2) if opt == "adamw" else {}
    runs = {}
    for name, kw in variants.items():
        cfg = get_preset("12x128-bf16", batchSize=B, synthetic=False, data_root=FIXTURE,
                         optimizer=opt, **okw, **kw)
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
    out = {"mode": "step", "model": f"12x128 bf16 {opt}", "B": B, "steps_per_window": K,
           "built_first": next(iter(variants)), "can_defer": runs["cosine"][0].net.can_defer(),
           "unit": "us per step (load_next + train_step, host clock, device synchronise)"}
    for m, t in times.items():
        out[m] = t
        out[m + "_median"] = round(statistics.median(t), 2)
        out[m + "_spread"] = round(max(t) - min(t), 2)
    out["cosine_minus_none_median_us"] = round(out["cosine_median"] - out["none_median"], 2)
    be = runs["cosine"][0]
    out["lr_step"], out["rate"], out["base_rate"] = be.lr_step, be.rate, be.base_rate
    assert be.lr_step == total
    for be, _ in runs.values():
        assert torch.isfinite(be.net.params).all()
        be.close()
    print(json.dumps(out), flush=True)


def curves(iters=3000):
    from deep_go_amd.config import get_preset
    from deep_go_amd.train.experiment import Experiment
    iters = int(iters)
    out = {"mode": "curves", "iterations": iters,
           "model": "6x64 bf16 adamw rate 1e-3 ema_decay 0.999, bundled fixture"}
    with tempfile.TemporaryDirectory() as tmp:
        for name, kw in (("none", {}), ("cosine", dict(lr_schedule="cosine", lr_warmup=100,
                                                       lr_total=iters))):
            cfg = get_preset("default-experiment", synthetic=False, data_root=FIXTURE,
                             rate=1e-3, optimizer="adamw", weight_decay=1e-2, ema_decay=0.999,
                             log_interval=100, validation_interval=500, validationSize=512,
                             checkpoint_dir=tmp, metrics_path=os.path.join(tmp, name + ".jsonl"),
                             **kw)
            e = Experiment(cfg, id=name)
            res = e.run(iters)
            e.metrics.close()
            data = e.draw_validation(512, split="test", seed_offset=99)
            out[name] = {"final_train_cost": res["train_cost"], "val_cost": res["val_cost"],
                         "bad_steps": e.backend.bad_steps(), "rate": e.backend.rate,
                         "test_live": [round(x, 4) for x in e.eval_batch_set(data)],
                         "test_ema": [round(x, 4) for x in e.eval_batch_set(data, ema=True)]}
            e.close()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    mode = sys.argv[1] if len(sys.argv) > 1 else "kernel"
    if mode == "kernel":
        print(json.dumps(kernel(*[int(x) for x in sys.argv[2:]])), flush=True)
    else:
        {"step": step, "curves": curves}[mode](*sys.argv[2:])
