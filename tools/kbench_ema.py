"""ema_decay (csrc/kernels/ema.hip, module _dgema), measured.

  kernel  at the flat sizes of 12x128 and 12x256: device events around R back-to-back launches,
          five timings each in turn, of ema_tick alone (one wave: the floor of one more launch)
          and of the pair ema issues (12 bytes per element: p read, e read and written), beside
          the sgd kernel of _dghip (12 as well: p read and written, g read) and the momentum
          kernel of _dgopt (20) on the same vectors.  The pair's yardstick is sgd's median + the
          tick's median + sgd's spread.
  caps    the same pair from builds of ema.hip with other grid caps, each timed in a child
          process of its own beside the build in the tree:
            caps-build OUTDIR CAP...   compiles OUTDIR/CAP/_dgema<EXT> (-DDG_EMA_MAX_BLOCKS=CAP;
                                       needs no GPU)
            caps OUTDIR [R]            times every OUTDIR/CAP found
  step    the trainer's step through HIPBackend on the packed fixture (12x128 bf16, batch 256,
          input prefetch on): load_next + train_step, K steps per window ending in a device
          synchronise, windows alternating on one device between ema_decay = 0 and 0.999.  The
          order of the variants rotates from round to round, so no variant keeps one place
          (profiles/clip.txt describes the position effect between backends built in one
          process; FIRST = 1 builds the ema_decay = 0.999 backend first instead).
  curves  one run pair on the bundled fixture (6x64, adamw, rate 1e-3, ITERS iterations) with
          ema_decay = 0.999 and 0: the validation records of the weights and of the average,
          and the test split's cost and top-1 of both at the end.

Usage: python tools/kbench_ema.py kernel [R] | caps-build OUTDIR CAP... | caps OUTDIR [R]
       | step [K] [ROUNDS] [FIRST] | curves [ITERS]
-> one JSON line per mode.  bench.py is the headline benchmark; this tool only covers what
ema_decay adds."""
import json
import os
import statistics
import subprocess
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


def _sizes():
    from deep_go_amd.config import ExperimentConfig
    from deep_go_amd.models.gocnn import ParamLayout
    return {ch: ParamLayout(ExperimentConfig(numLayers=12, channelSize=ch)) for ch in (128, 256)}


def kernel(R=2000, module=None, only_pair=False):
    from deep_go_amd.models.gocnn import init_params
    from deep_go_amd.ops.native import ema, hip, opt, stream_handle
    h, o, m, s = hip(), opt(), module or ema(), stream_handle()
    nbytes = {"ema_pair": 12, "sgd": 12, "momentum": 20}
    out = {"mode": "kernel", "launches": R, "unit": "us per launch (pair: per two launches)",
           "bytes_per_element": nbytes}
    for ch, lay in _sizes().items():
        n = lay.numel
        p = init_params(lay, 1).cuda()
        e = p.clone()
        g0 = torch.zeros(n, device="cuda")                 # sgd's and momentum's: p stays
        v = torch.zeros(n, device="cuda")
        rec = torch.zeros(2, dtype=torch.int64, device="cuda")
        trec = torch.zeros(2, dtype=torch.int64, device="cuda")
        lr = torch.tensor([1e-6], dtype=torch.float64, device="cuda")
        gate = torch.ones(1, device="cuda")
        r = np.ascontiguousarray(np.array(lay.weight_ranges(), dtype=np.int64))
        P, E, LRP, GT = p.data_ptr(), e.data_ptr(), lr.data_ptr(), gate.data_ptr()
        runs = {
            "ema_tick": lambda: m.ema_tick(trec.data_ptr(), 0.999, GT, s),
            "ema_pair": lambda: m.ema(P, E, n, rec.data_ptr(), 0.999, GT, s),
            "sgd": lambda: h.sgd(P, g0.data_ptr(), n, LRP, 1.0, GT, s),
            "momentum": lambda: o.momentum(P, g0.data_ptr(), v.data_ptr(), n, LRP, 0.9, 1, 1e-4,
                                           r.ctypes.data, len(r), 1.0, GT, s),
        }
        if only_pair:
            runs = {k: runs[k] for k in ("ema_tick", "ema_pair")}
        res = {"elements": n, **{k: [] for k in runs}}
        for k in range(5):
            for name, fn in runs.items():
                e.normal_()                    # (e == p is a fixed point: keep it moving)
                res[name].append(_events(fn, R))
        for name in runs:
            med = statistics.median(res[name])
            res[name + "_median"] = med
            if name in nbytes:
                res[name + "_GBps"] = round(nbytes[name] * n / med / 1e3, 1)
        res["ema_pair_spread_us"] = round(max(res["ema_pair"]) - min(res["ema_pair"]), 3)
        if not only_pair:
            res["sgd_spread_us"] = round(max(res["sgd"]) - min(res["sgd"]), 3)
            res["ema_pair_yardstick_us"] = round(
                res["sgd_median"] + res["ema_tick_median"] + res["sgd_spread_us"], 3)
            res["ema_pair_minus_yardstick_us"] = round(
                res["ema_pair_median"] - res["ema_pair_yardstick_us"], 3)
        # every launch counted, and the average is still one
        assert int(rec[0].item()) == 5 * (R + 1) and torch.isfinite(e).all()
        out[f"12x{ch}"] = res
    return out


def caps_build(outdir, *caps):
    from deep_go_amd import _build as b
    for cap in caps:
        d = os.path.join(outdir, str(int(cap)))
        os.makedirs(d, exist_ok=True)
        kobj, bobj = os.path.join(d, "ema.o"), os.path.join(d, "ema_bindings.o")
        b._run([b.HIPCC, *b.HIP_FLAGS, f"-DDG_EMA_MAX_BLOCKS={int(cap)}", "-c",
                str(b.KDIR / "ema.hip"), "-o", kobj])
        b._run([b.HIPCC, "-O2", "-std=c++17", "-fPIC", *b._pybind_includes(), "-c",
                str(b.KDIR / "ema_bindings.cpp"), "-o", bobj])
        b._run([b.HIPCC, f"--offload-arch={b.ARCH}", "-shared", "-fPIC", "--hip-link", "-o",
                os.path.join(d, f"_dgema{b.EXT}"), kobj, bobj])
        print(d)


def caps(outdir, R=2000):
    out = {"mode": "caps", "launches": R}
    for cap in sorted((d for d in os.listdir(outdir) if d.isdigit()), key=int):
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "caps-child",
                            os.path.join(outdir, cap), str(R)], capture_output=True, text=True,
                           timeout=300)
        if r.returncode != 0:
            raise RuntimeError(f"cap {cap}: exit {r.returncode}\n{r.stderr[-2000:]}")
        res = json.loads(r.stdout.strip().splitlines()[-1])
        out[cap] = {k: {"ema_pair": v["ema_pair"], "ema_pair_median": v["ema_pair_median"],
                        "ema_tick_median": v["ema_tick_median"]}
                    for k, v in res.items() if k.startswith("12x")}
    print(json.dumps(out), flush=True)


def caps_child(d, R=2000):
    import importlib.util
    from deep_go_amd import _build as b
    spec = importlib.util.spec_from_file_location("_dgema", os.path.join(d, f"_dgema{b.EXT}"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    print(json.dumps(kernel(int(R), module=m, only_pair=True)), flush=True)


def step(K=300, rounds=6, first=0, B=256):
    from deep_go_amd.config import get_preset
    from deep_go_amd.data.dataset import PackedDataset
    from deep_go_amd.data.loader import BatchLoader
    from deep_go_amd.train.backends import HIPBackend
    src = PackedDataset.load(os.path.join(FIXTURE, "train.dgpack.npz"))
    variants = {"ema_off": 0.0, "ema_on": 0.999}
    if first:
        variants = dict(reversed(variants.items()))
    runs = {}
    for name, decay in variants.items():
        cfg = get_preset("12x128-bf16", batchSize=B, synthetic=False, data_root=FIXTURE,
                         ema_decay=decay)
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
    out = {"mode": "step", "model": "12x128 bf16 sgd (the preset)", "B": B,
           "steps_per_window": K, "built_first": next(iter(variants)),
           "unit": "us per step (load_next + train_step, host clock, device synchronise)"}
    for m, t in times.items():
        out[m] = t
        out[m + "_median"] = round(statistics.median(t), 2)
        out[m + "_spread"] = round(max(t) - min(t), 2)
    out["ema_on_minus_ema_off_median_us"] = round(out["ema_on_median"] - out["ema_off_median"], 2)
    out["steps_per_backend"] = 30 + K * rounds
    out["ema_steps"] = runs["ema_on"][0].ema_steps()
    # the same data and seed: the average changes nothing of the training
    out["params_equal"] = bool(torch.equal(runs["ema_on"][0].net.params,
                                           runs["ema_off"][0].net.params))
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
        for name, decay in (("ema_0.999", 0.999), ("ema_off", 0.0)):
            mpath = os.path.join(tmp, name + ".jsonl")
            cfg = get_preset("default-experiment", synthetic=False, data_root=FIXTURE,
                             rate=1e-3, optimizer="adamw", weight_decay=1e-2, ema_decay=decay,
                             log_interval=100, validation_interval=500, validationSize=512,
                             checkpoint_dir=tmp, metrics_path=mpath)
            e = Experiment(cfg, id=name)
            res = e.run(iters)
            e.metrics.close()
            rows = read_jsonl(mpath)
            r = {"final_train_cost": res["train_cost"], "bad_steps": e.backend.bad_steps()}
            for kind in ("validation", "validation_ema"):
                rs = [x for x in rows if x.get("kind") == kind]
                if rs:
                    r[kind] = {"step": [x["step"] for x in rs],
                               "val_cost": [round(x["val_cost"], 4) for x in rs],
                               "val_acc": [round(x["val_acc"], 4) for x in rs]}
            data = e.draw_validation(512, split="test", seed_offset=99)
            r["test_live"] = [round(x, 4) for x in e.eval_batch_set(data)]
            if decay > 0:
                r["test_ema"] = [round(x, 4) for x in e.eval_batch_set(data, ema=True)]
                r["ema_steps"] = e.backend.ema_steps()
            out[name] = r
            e.close()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    mode = sys.argv[1] if len(sys.argv) > 1 else "kernel"
    if mode == "kernel":
        print(json.dumps(kernel(*[int(x) for x in sys.argv[2:]])), flush=True)
    elif mode == "caps-build":
        caps_build(sys.argv[2], *sys.argv[3:])
    elif mode == "caps":
        caps(sys.argv[2], *[int(x) for x in sys.argv[3:]])
    elif mode == "caps-child":
        caps_child(*sys.argv[2:])
    else:
        {"step": step, "curves": curves}[mode](*[int(x) for x in sys.argv[2:]])
