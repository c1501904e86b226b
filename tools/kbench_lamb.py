"""optimizer=lamb (csrc/kernels/optim.hip, module _dglamb), measured.

  kernel  lamb alone (its four launches, the count's included) at the flat sizes of 12x128 and
          12x256 with the model's own ranges: device events around R back-to-back launches,
          beside adamw (tick included), the tick alone and the clipping grad_clip pair (c = 1e-9:
          every launch rewrites the gradient, tools/kbench_clip.py) on vectors of the same size,
          five timings each in turn.  Bytes per element: adamw 28; lamb 40 (Adam's 28 + u
          written, u and p read, p written); the clipping pair 12.  lamb's yardstick at each size
          is adamw's median + the clipping pair's median + the spread of adamw's five timings.
          Gradients are zero and the rate tiny, so the vectors stay finite over thousands of
          launches.
  step    the trainer's step through HIPBackend on the packed fixture (12x128 bf16, batch 256,
          input prefetch on): load_next + train_step, K steps per window ending in a device
          synchronise, adamw and lamb on one device (LAMB_FIRST = 1: lamb's backend is built
          first), the order of the windows rotating from round to round.  (In
          tools/kbench_opt.py one position of a fixed order ran slower whichever variant held
          it; hence the rotation.)
  tail    the optimizer's part of the step alone, as SegmentedStep's optimizer graph replays it
          (finite gate, the optimizer's launches, weight_refresh_decay): device events around R
          back-to-back replays on a 12x128 bf16 net whose gradient stays as one backward left
          it, adamw and lamb in turn, five timings each.
  curves  one run pair on the bundled fixture (6x64, ITERS iterations) with adamw and lamb at the
          same rate: the logged loss curves and the range of the logged trust ratios.

Usage: python tools/kbench_lamb.py kernel [R] | step [K] [ROUNDS] [LAMB_FIRST] | tail [R] |
curves [ITERS]
-> one JSON line per mode.  bench.py is the headline benchmark; this tool only covers what the
optimizer option adds."""
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
    from deep_go_amd.ops.native import adam, clip, lamb, stream_handle
    a, c, lb, s = adam(), clip(), lamb(), stream_handle()
    nbytes = {"adamw": 28, "lamb": 40, "pair_clipping": 12}
    out = {"mode": "kernel", "launches": R, "unit": "us per call of the launcher",
           "bytes_per_element": nbytes}
    for ch in (128, 256):
        lay = ParamLayout(ExperimentConfig(numLayers=12, channelSize=ch))
        n = lay.numel
        p = init_params(lay, 1).cuda()
        g, gc = torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")
        am, av = torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")
        u = torch.zeros(n, device="cuda")
        rec = torch.zeros(2, dtype=torch.int64, device="cuda")
        crec = torch.zeros(2, dtype=torch.int64, device="cuda")
        lr = torch.tensor([1e-6], dtype=torch.float64, device="cuda")
        gate = torch.ones(1, device="cuda")
        r = np.ascontiguousarray(np.array(lay.weight_ranges(), dtype=np.int64))
        part = torch.zeros(lb.lamb_partials(n, r.ctypes.data, len(r)), device="cuda")
        tab = torch.zeros(60, device="cuda")
        cpart = torch.zeros(c.clip_partials(), device="cuda")
        P, G, LRP, GT = p.data_ptr(), g.data_ptr(), lr.data_ptr(), gate.data_ptr()
        runs = {
            "adamw": lambda: a.adamw(P, G, am.data_ptr(), av.data_ptr(), n, LRP, rec.data_ptr(),
                                     0.9, 0.999, 1e-8, 1e-2, r.ctypes.data, len(r), 1.0, GT, s),
            "adamw_tick": lambda: a.adamw_tick(rec.data_ptr(), 0.9, 0.999, GT, s),
            "pair_clipping": lambda: c.grad_clip(gc.data_ptr(), n, cpart.data_ptr(),
                                                 cpart.numel(), crec.data_ptr(), 1e-9, 1.0, GT, s),
            "lamb": lambda: lb.lamb(P, G, am.data_ptr(), av.data_ptr(), u.data_ptr(), n, LRP,
                                    rec.data_ptr(), part.data_ptr(), part.numel(), tab.data_ptr(),
                                    0.9, 0.999, 1e-8, 1e-2, r.ctypes.data, len(r), 1.0, GT, s),
        }
        res = {"elements": n, "ranges": len(r), "partial_floats": part.numel(),
               **{k: [] for k in runs}}
        for _ in range(5):
            for name, fn in runs.items():
                if name == "pair_clipping":
                    gc.normal_()                   # (the clipping run leaves zeros behind)
                res[name].append(_events(fn, R))
        for name in runs:
            med = statistics.median(res[name])
            res[name + "_median"] = med
            if name in nbytes:
                res[name + "_GBps"] = round(nbytes[name] * n / med / 1e3, 1)
        res["adamw_spread_us"] = round(max(res["adamw"]) - min(res["adamw"]), 3)
        res["lamb_spread_us"] = round(max(res["lamb"]) - min(res["lamb"]), 3)
        res["lamb_yardstick_us"] = round(res["adamw_median"] + res["pair_clipping_median"]
                                         + res["adamw_spread_us"], 3)
        res["lamb_minus_yardstick_us"] = round(res["lamb_median"] - res["lamb_yardstick_us"], 3)
        res["phi_last"] = [round(x, 4) for x in tab.view(20, 3)[:len(r), 2].tolist()]
        assert torch.isfinite(p).all() and torch.isfinite(u).all()
        assert torch.isfinite(am).all() and torch.isfinite(av).all()
        out[f"12x{ch}"] = res
    print(json.dumps(out), flush=True)


def step(K=300, rounds=6, lamb_first=0, B=256):
    from deep_go_amd.config import get_preset
    from deep_go_amd.data.dataset import PackedDataset
    from deep_go_amd.data.loader import BatchLoader
    from deep_go_amd.train.backends import HIPBackend
    src = PackedDataset.load(os.path.join(FIXTURE, "train.dgpack.npz"))
    runs = {}
    for name in (("lamb", "adamw") if lamb_first else ("adamw", "lamb")):
        cfg = get_preset("12x128-bf16", batchSize=B, synthetic=False, data_root=FIXTURE,
                         rate=1e-3, optimizer=name, weight_decay=1e-2)
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
    out = {"mode": "step", "model": "12x128 bf16", "B": B, "steps_per_window": K,
           "built_first": names[0],
           "unit": "us per step (load_next + train_step, host clock, device synchronise)"}
    for m, t in times.items():
        out[m] = t
        out[m + "_median"] = round(statistics.median(t), 2)
        out[m + "_spread"] = round(max(t) - min(t), 2)
    out["lamb_minus_adamw_median_us"] = round(out["lamb_median"] - out["adamw_median"], 2)
    out["phi_last"] = [round(s[2], 4) for s in runs["lamb"][0].lamb_stats()]
    for be, _ in runs.values():
        assert torch.isfinite(be.net.params).all()
        be.close()
    print(json.dumps(out), flush=True)


def tail(R=500, B=256):
    from deep_go_amd.config import get_preset
    from deep_go_amd.data.synthetic import random_planes
    from deep_go_amd.models.hip_model import HipGoNet, SegmentedStep
    out = {"mode": "tail", "model": "12x128 bf16", "B": B, "replays": R,
           "unit": "us per replay of the optimizer graph"}
    steps = {}
    for name in ("adamw", "lamb"):
        cfg = get_preset("12x128-bf16", batchSize=B, rate=1e-6, optimizer=name,
                         weight_decay=1e-2)
        net = HipGoNet(cfg, B, device="cuda")
        net.set_batch(*[torch.from_numpy(a).cuda() for a in random_planes(B, seed=1)])
        st = SegmentedStep(net, None, use_graphs=True)
        for _ in range(3):
            st()
        st.forward_backward()
        st.optimizer()
        steps[name] = (net, st)
        out[name] = []
    for _ in range(5):
        for name, (net, st) in steps.items():
            out[name].append(_events(st.optimizer, R))
    for name, (net, _) in steps.items():
        out[name + "_median"] = statistics.median(out[name])
        assert torch.isfinite(net.params).all() and int(net.bad_steps.item()) == 0
    out["lamb_minus_adamw_median_us"] = round(out["lamb_median"] - out["adamw_median"], 3)
    print(json.dumps(out), flush=True)


def curves(iters=3000):
    from deep_go_amd.config import get_preset
    from deep_go_amd.train.experiment import Experiment
    from deep_go_amd.utils.metrics import read_jsonl
    out = {"mode": "curves", "model": "6x64 bf16 rate 1e-3 weight_decay 1e-2, bundled fixture",
           "iterations": iters}
    with tempfile.TemporaryDirectory() as tmp:
        for name in ("adamw", "lamb"):
            mpath = os.path.join(tmp, name + ".jsonl")
            cfg = get_preset("default-experiment", synthetic=False, data_root=FIXTURE,
                             rate=1e-3, optimizer=name, weight_decay=1e-2, log_interval=100,
                             validation_interval=1000, validationSize=512, checkpoint_dir=tmp,
                             metrics_path=mpath)
            e = Experiment(cfg, id=name)
            res = e.run(iters)
            e.metrics.close()
            rows = read_jsonl(mpath)
            r = {"loss_ema_every_100": [round(x["loss_ema"], 4) for x in rows
                                        if x.get("kind") == "train"],
                 "val_cost": [round(x["val_cost"], 4) for x in rows
                              if x.get("kind") == "validation"],
                 "final_train_cost": res["train_cost"], "bad_steps": e.backend.bad_steps()}
            lamb = [x for x in rows if x.get("kind") == "lamb"]
            if lamb:
                r.update(phi_min=round(min(x["phi_min"] for x in lamb), 4),
                         phi_max=round(max(x["phi_max"] for x in lamb), 4),
                         phi_first=[round(x, 4) for x in lamb[0]["phi"]],
                         phi_last=[round(x, 4) for x in lamb[-1]["phi"]])
            out[name] = r
            e.close()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    mode = sys.argv[1] if len(sys.argv) > 1 else "kernel"
    args = [int(x) for x in sys.argv[2:]]
    {"kernel": kernel, "step": step, "tail": tail, "curves": curves}[mode](*args)
