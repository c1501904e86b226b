"""Training-time symmetry augmentation (csrc/kernels/augment.hip; ``augment=d4``), measured.

  kernel  augment_batch alone at B = 256: device events around R back-to-back launches on one
          packed buffer (hashed ids; the sequence number changes per launch, so 7 boards in 8
          move every time), beside symmetry_planes over the same 256 boards (S = 1), which
          moves the same bytes out of place.
  step    the trainer's step through HIPBackend on the packed fixture (12x128 bf16, batch 256,
          input prefetch on): load_next + train_step, K steps per window ending in a device
          synchronise, windows of augment=none and augment=d4 alternating on one device.
  learn   one run pair on the fixture, 6x64 from the same init, augment=none vs d4: training
          cost at the end, cost / top-1 on every held-out position (validation and test
          game), and the 8-symmetry ensemble's top-1 beside the single view's through the
          Predictor (occupied points masked in both).

Usage: python tools/kbench_aug.py kernel [R] | step [K] [ROUNDS] | learn [ITERS]
-> one JSON line per mode.  bench.py is the headline benchmark; this tool only covers what the
augmentation adds."""
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
    fn(0)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for k in range(R):
        fn(k)
    e1.record()
    torch.cuda.synchronize()
    return round(1000.0 * e0.elapsed_time(e1) / R, 3)


def kernel(R=2000, B=256):
    from deep_go_amd.data.batch import pack_batch, unpack_views
    from deep_go_amd.data.synthetic import random_planes
    from deep_go_amd.ops.native import aug, hip, stream_handle
    a, h, s = aug(), hip(), stream_handle()
    buf = pack_batch(*random_planes(B, seed=1)).cuda()
    v = unpack_views(buf, B)
    ids = torch.zeros(B, dtype=torch.uint8, device="cuda")
    dst = torch.zeros_like(buf)
    d = unpack_views(dst, B)
    runs = {
        "augment_batch": lambda k: a.augment_batch(v[0].data_ptr(), v[3].data_ptr(), B, 0, 1234,
                                                   k, 0, ids.data_ptr(), s),
        "symmetry_planes_S1": lambda k: h.symmetry_planes(
            v[0].data_ptr(), v[1].data_ptr(), v[2].data_ptr(), v[3].data_ptr(), B, 1,
            d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), B, s),
    }
    out = {"mode": "kernel", "B": B, "launches": R, "unit": "us per launch"}
    for name, fn in runs.items():
        out[name] = [_events(fn, R) for _ in range(5)]
    print(json.dumps(out), flush=True)


def step(K=300, rounds=6, B=256):
    from deep_go_amd.config import get_preset
    from deep_go_amd.data.dataset import PackedDataset
    from deep_go_amd.data.loader import BatchLoader
    from deep_go_amd.train.backends import HIPBackend
    src = PackedDataset.load(os.path.join(FIXTURE, "train.dgpack.npz"))
    runs = {}
    for mode in ("none", "d4"):
        cfg = get_preset("12x128-bf16", batchSize=B, synthetic=False, augment=mode,
                         data_root=FIXTURE)
        be = HIPBackend(cfg, B)
        assert be.net.load_stream is not None, "input prefetch must be on"
        ld = BatchLoader(src, B, threads=cfg.loader_threads, prefetch=cfg.prefetch,
                         seed=cfg.seed * 1000003)
        runs[mode] = (be, ld)

    def window(be, ld, n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            be.load_next(ld)
            be.train_step()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / n * 1e6
    times = {m: [] for m in runs}
    try:
        for be, ld in runs.values():
            window(be, ld, 30)                              # warm-up
        for _ in range(rounds):
            for m, (be, ld) in runs.items():
                times[m].append(round(window(be, ld, K), 2))
    finally:
        for _, ld in runs.values():
            ld.close()
    out = {"mode": "step", "model": "12x128 bf16", "B": B, "steps_per_window": K,
           "unit": "us per step (load_next + train_step, host clock, device synchronise)"}
    for m, t in times.items():
        out[m] = t
        out[m + "_median"] = round(statistics.median(t), 2)
        out[m + "_boards_per_s"] = round(B / statistics.median(t) * 1e6)
    out["d4_minus_none_median_us"] = round(out["d4_median"] - out["none_median"], 2)
    print(json.dumps(out), flush=True)


def learn(iters=3000, B=64):
    from deep_go_amd.config import ExperimentConfig
    from deep_go_amd.data.dataset import PackedDataset
    from deep_go_amd.predict import Predictor
    from deep_go_amd.train.experiment import Experiment
    held = {s: PackedDataset.load(os.path.join(FIXTURE, f"{s}.dgpack.npz"))
            for s in ("validation", "test")}
    out = {"mode": "learn", "model": "6x64 bf16", "batch": B, "rate": 0.05, "iterations": iters}
    with tempfile.TemporaryDirectory() as tmp:
        for mode in ("none", "d4"):
            cfg = ExperimentConfig(numLayers=6, channelSize=64, batchSize=B, rate=0.05,
                                   rateDecay=1e-7, useCuda=True, seed=11, data_root=FIXTURE,
                                   validationSize=B, validation_interval=10 ** 9,
                                   log_interval=50, checkpoint_dir=tmp, augment=mode,
                                   metrics_path=os.path.join(tmp, mode + ".jsonl"))
            e = Experiment(cfg, id=mode)
            try:
                res = e.run(iters)
                r = {"train_cost_ema": round(float(res["train_cost"]), 4)}
                flat = e.backend.flat_params()
                for split, ds in held.items():
                    data = (ds.planes, ds.player, ds.rank, ds.label.astype(np.int32))
                    cost, acc = e.eval_batch_set(data, quirks=False)
                    r[split] = {"positions": len(ds), "cost": round(float(cost), 4),
                                "top1": round(float(acc), 4)}
                    for S in (1, 8):
                        p = Predictor(cfg, flat, batch=64, symmetries=S, device="gpu")
                        rank = p.predict(*data[:3], labels=data[3]).rank
                        r[split][f"masked_top1_S{S}"] = round(float(np.mean(rank == 0)), 4)
            finally:
                e.close()
            out[mode] = r
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    mode = sys.argv[1] if len(sys.argv) > 1 else "kernel"
    args = [int(x) for x in sys.argv[2:]]
    {"kernel": kernel, "step": step, "learn": learn}[mode](*args)
