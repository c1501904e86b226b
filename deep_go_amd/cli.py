"""Command line: ``python -m deep_go_amd <command> ...``

  train     [--preset NAME] [key=value ...] --iters N [--export-t7 PATH] [--auto-resume]
            (localtest.lua / default-experiment.lua / notebook equivalents via presets;
            optimizer=sgd|rmsprop|momentum|adamw|lamb — lamb takes adamw's fields adam_beta1,
            adam_beta2, adam_eps, weight_decay and logs one kind="lamb" record of the per-layer
            trust ratios on logging iterations)
  resume    CKPT --iters N [--reset-optimizer] [--id NAME] [key=value ...]
            (experiments/repeated.lua: -gpu/-num/-iters -> --device/--id/--iters)
  eval      CKPT [--split test] [--n N] [--symmetries 8] [--top K] [--ema]
            (top-1 / NLL on a split; never done in the ref.  With --symmetries / --top also the
            symmetry-ensembled, legality-masked top-k accuracy and mean rank: deep_go_amd.predict)
  predict   CKPT GAME.sgf [--move N] [--top K] [--symmetries {1,8}] [--device auto|cpu|gpu] [--all]
            [--ema]
            (where to play and with what probability: one JSON line per requested move)
  gtp       CKPT [--ema] [--device auto|cpu|gpu] [--symmetries {1,8}] [--temperature T] [--top-p P]
            [--seed N] [--rank DAN] [--komi K]
            (a GTP version 2 engine on stdin / stdout for Sabaki, GoGui or gogui-twogtp:
            deep_go_amd.play.gtp)
  selfplay  CKPT [--opponent CKPT2] --games N [--max-moves M] [--out DIR] [--komi K]
            [--temperature T] [--top-p P] [--opening-plies K] [--seed N] [--rank DAN] [--batch B]
            [--ema] [--device ...] [--symmetries {1,8}]
            (lock-step batched self-play, or a match with colours alternating by game; one SGF
            per game and summary.json into DIR, the summary also as one JSON line)
  makedata  scatter SRC DST train=N validation=N test=N | transcribe SRC DST [--threads T] [--ko]
            | count ROOT SPLIT | pack ROOT SPLIT
  export    CKPT OUT.t7 [--ema] (reference Torch7 experiment table)
            (--ema, here and for eval / predict: the checkpoint's moving average of the weights,
            ema_decay > 0, in the place of its parameters; an error if it carries none)
  import    IN.t7 OUT.model
  plot      FILE... [--out PNG] (validation/training curves from checkpoints or JSONL; plot.lua)
  bench     [bench.py args]

Multi-GPU: launch with ``python -m torch.distributed.run --nproc-per-node N -m deep_go_amd
train ...`` (one rank per GPU, RCCL); ``batchSize`` is the GLOBAL batch (split across ranks,
like nn.DataParallelTable).
"""
from __future__ import annotations

import argparse
import json
import os
import sys


def _fill_lr_total(iters):
    """train: lr_schedule=linear | cosine without an lr_total takes --iters as its horizon,
    before the config is built (which refuses the schedule without one); it is then part of the
    checkpoint's config, so a resumed run keeps it."""
    def fill(ov):
        if ov.get("lr_schedule") in ("linear", "cosine") and "lr_total" not in ov:
            ov["lr_total"] = str(iters)
        return ov
    return fill


def _cfg_from(args, base=None, fill=None):
    from .config import ExperimentConfig, get_preset, parse_overrides
    ov = parse_overrides(args.overrides)
    if fill is not None:
        ov = fill(ov)
    if base is not None:
        return base.replace(**ov) if ov else base
    if args.preset:
        return get_preset(args.preset, **ov)
    return ExperimentConfig().replace(**ov) if ov else ExperimentConfig()


def cmd_train(args):
    from .train.experiment import Experiment
    cfg = _cfg_from(args, fill=_fill_lr_total(args.iters))
    if args.device == "cpu":
        cfg = cfg.replace(useCuda=False)
    elif args.device == "gpu":
        cfg = cfg.replace(useCuda=True)
    e = Experiment(cfg)
    iters = args.iters
    if args.auto_resume:
        # restart after a failure: continue <checkpoint_dir>/<id>.model
        # (exact resume: weights, optimizer, iteration, sampler cursor, RNG) up to --iters
        if not cfg.id:
            raise SystemExit("--auto-resume needs a stable experiment id (id=NAME)")
        path = e.checkpoint_path()
        if os.path.exists(path):
            e = Experiment.load(path)
            if args.device == "cpu":
                e.cfg = e.cfg.replace(useCuda=False)
            iters = max(0, args.iters - e.iterations)
            print(json.dumps({"auto_resume": path, "from_iteration": e.iterations}), flush=True)
    try:
        res = e.run(iters) if iters > 0 else {"iterations": e.iterations}
        if e.info.is_main:
            e.save()
            if args.export_t7:
                e.export_t7(args.export_t7)
            print(json.dumps({"id": e.id, "checkpoint": e.checkpoint_path(), **res}))
    finally:
        e.close()
    return 0


def cmd_resume(args):
    from .config import parse_overrides
    from .train.experiment import Experiment
    ov = parse_overrides(args.overrides)
    e = Experiment.load(args.checkpoint, reset_optimizer=args.reset_optimizer, **ov)
    if args.id:
        e.id = args.id
    if args.device == "cpu":
        e.cfg = e.cfg.replace(useCuda=False)
    try:
        res = e.run(args.iters)
        if e.info.is_main:
            e.save()
            print(json.dumps({"id": e.id, "checkpoint": e.checkpoint_path(), **res}))
    finally:
        e.close()
    return 0


def cmd_eval(args):
    from .train.experiment import Experiment
    try:
        e = Experiment.load(args.checkpoint, ema=args.ema)
    except ValueError as err:
        if not args.ema:
            raise
        raise SystemExit(f"eval --ema: {err}")
    if args.device == "cpu":
        e.cfg = e.cfg.replace(useCuda=False)
    extra = {}
    try:
        cost, acc = e.evaluate_split(args.split, args.n)
        if args.symmetries is not None or args.top is not None:
            extra = _eval_ensemble(e, args)
    finally:
        e.close()
    if args.ema:
        extra = {"ema": True, **extra}
    print(json.dumps({"split": args.split, "cost": cost, "accuracy": acc, **extra}))
    return 0


def _eval_ensemble(e, args):
    """eval --symmetries / --top: the same sample set through the Predictor (symmetry
    ensemble, occupied points masked): top-k accuracy, mean rank of the expert move, top-1."""
    import numpy as np
    from .predict import Predictor
    S, K = args.symmetries or 8, args.top or 5
    planes, player, rank, labels = e.draw_validation(args.n or e.cfg.validationSize,
                                                     split=args.split, seed_offset=99)
    p = Predictor(e.cfg, e.backend.flat_params(), batch=64, symmetries=S, top=K,
                  device="cpu" if e._device_kind() == "cpu" else "gpu")
    r = p.predict(planes, player, rank, labels=labels).rank
    ok = r >= 0    # (a label on an occupied point has no rank: counted as a miss)
    return {"symmetries": S, "top": K,
            "topk_accuracy": float(np.mean(ok & (r < K))),
            "mean_rank": float(r[ok].mean()) if ok.any() else None,
            "ensemble_accuracy": float(np.mean(r == 0))}


def _sgf_point(p: int):
    x, y = divmod(int(p), 19)
    return {"sgf": chr(ord("a") + x) + chr(ord("a") + y), "x": x, "y": y}


def cmd_predict(args):
    from .predict import Predictor, ko_mask, positions_from_sgf
    try:
        p = Predictor.load(args.checkpoint, ema=args.ema, symmetries=args.symmetries,
                           top=args.top, device=args.device, batch=64)
    except ValueError as err:
        if not args.ema:
            raise
        raise SystemExit(f"predict --ema: {err}")
    with open(args.sgf, newline="") as f:
        text = f.read()
    planes, player, rank, label, ko = positions_from_sgf(text, mark_ko=p.cfg.ko_plane)
    n = len(label)
    if n == 0:
        raise SystemExit(f"{args.sgf}: no moves")
    move = n if args.move is None else args.move
    if not 1 <= move <= n:
        raise SystemExit(f"--move {move}: the game has moves 1..{n}")
    sel = slice(0, n) if args.all else slice(move - 1, move)
    r = p.predict(planes[sel], player[sel], rank[sel], labels=label[sel],
                  extra_illegal=ko_mask(ko[sel]))
    for k, m in enumerate(range(sel.start, sel.stop)):
        top = [dict(_sgf_point(q), p=float(pr)) for q, pr in zip(r.topk[k], r.topk_p[k])
               if q >= 0]
        print(json.dumps({"move": m + 1, "player": "B" if player[m] == 1 else "W", "top": top,
                          "played": _sgf_point(label[m]), "rank": int(r.rank[k])}))
    return 0


def _play_predictor(args, checkpoint, what, batch=64):
    from .predict import Predictor
    try:
        return Predictor.load(checkpoint, ema=args.ema, symmetries=args.symmetries, top=1,
                              device=args.device, batch=batch)
    except ValueError as err:
        if not args.ema:
            raise
        raise SystemExit(f"{what} --ema: {err}")


def cmd_gtp(args):
    from .play.gtp import GtpEngine
    p = _play_predictor(args, args.checkpoint, "gtp", batch=args.symmetries)
    GtpEngine(p, rank=args.rank, seed=args.seed, temperature=args.temperature,
              top_p=args.top_p, komi=args.komi).run(sys.stdin, sys.stdout)
    return 0


def cmd_selfplay(args):
    from .play.selfplay import run_match
    a = _play_predictor(args, args.checkpoint, "selfplay", batch=args.batch)
    b = _play_predictor(args, args.opponent, "selfplay", batch=args.batch) if args.opponent else None
    r = run_match(a, b, games=args.games, max_moves=args.max_moves, komi=args.komi,
                  rank=args.rank, seed=args.seed, temperature=args.temperature, top_p=args.top_p,
                  opening_plies=args.opening_plies, out_dir=args.out)
    # (the timing is printed only: summary.json depends on the arguments alone)
    print(json.dumps({**r["summary"], "timing": r["timing"]}))
    return 0


def cmd_makedata(args):
    from .data import makedata as md
    a = args.rest
    if not a:
        raise SystemExit("makedata: scatter|transcribe|count|pack")
    op = a[0]
    if op == "scatter":
        cats = dict(x.split("=") for x in a[3:])
        print(json.dumps(md.scatter(a[1], a[2], {k: int(v) for k, v in cats.items()},
                                    seed=args.seed)))
    elif op == "transcribe":
        print(json.dumps(md.transcribe(a[1], a[2], threads=args.threads, mark_ko=args.ko)))
    elif op == "count":
        print(md.count(a[1], a[2]))
    elif op == "pack":
        print(md.pack(a[1], a[2], threads=args.threads))
    else:
        raise SystemExit(f"unknown makedata op {op}")
    return 0


def cmd_export(args):
    from .utils import checkpoint as ck
    cfg, flat, state, opt = ck.load_checkpoint(args.checkpoint)
    if args.ema:
        try:
            flat = ck.ema_params(args.checkpoint, flat, opt)
        except ValueError as err:
            raise SystemExit(f"export --ema: {err}")
    ck.export_t7(args.out, cfg, flat, state, float(opt.get("rate", cfg.rate)))
    print(args.out)
    return 0


def cmd_import(args):
    from .utils import checkpoint as ck
    cfg, flat, state, rate = ck.import_t7(args.t7)
    state.setdefault("id", "imported")
    ck.save_checkpoint(args.out, cfg, flat, state,
                       {"kind": "sgd", "rate": rate, "rate_decay": cfg.rateDecay})
    print(args.out)
    return 0


def cmd_plot(args):
    from .utils.plot import plot_files
    print(plot_files(args.files, args.out))
    return 0


def cmd_bench(args):
    import runpy
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.argv = [os.path.join(root, "bench.py")] + args.rest
    runpy.run_path(sys.argv[0], run_name="__main__")
    return 0


def main(argv=None):
    ap = argparse.ArgumentParser(prog="deep_go_amd")
    sub = ap.add_subparsers(dest="cmd", required=True)
    t = sub.add_parser("train")
    t.add_argument("--preset")
    t.add_argument("--iters", type=int, required=True)
    t.add_argument("--device", choices=["auto", "cpu", "gpu"], default="auto")
    t.add_argument("--export-t7")
    t.add_argument("--auto-resume", action="store_true",
                   help="continue from <checkpoint_dir>/<id>.model if it exists (--iters = total)")
    t.add_argument("overrides", nargs="*")
    t.set_defaults(fn=cmd_train)
    r = sub.add_parser("resume")
    r.add_argument("checkpoint")
    r.add_argument("--iters", type=int, default=100)
    r.add_argument("--reset-optimizer", action="store_true")
    r.add_argument("--id")
    r.add_argument("--device", choices=["auto", "cpu", "gpu"], default="auto")
    r.add_argument("overrides", nargs="*")
    r.set_defaults(fn=cmd_resume)
    e = sub.add_parser("eval")
    e.add_argument("checkpoint")
    e.add_argument("--split", default="test")
    e.add_argument("--n", type=int)
    e.add_argument("--device", choices=["auto", "cpu", "gpu"], default="auto")
    e.add_argument("--symmetries", type=int, choices=[1, 8],
                   help="also report the symmetry-ensembled top-k accuracy / mean rank")
    e.add_argument("--top", type=int, help="k of topk_accuracy (default 5)")
    e.add_argument("--ema", action="store_true",
                   help="evaluate the checkpoint's moving average of the weights (ema_decay > 0)")
    e.set_defaults(fn=cmd_eval)
    q = sub.add_parser("predict")
    q.add_argument("checkpoint")
    q.add_argument("sgf")
    q.add_argument("--move", type=int, help="1-based move number (default: the last move)")
    q.add_argument("--top", type=int, default=5)
    q.add_argument("--symmetries", type=int, choices=[1, 8], default=8)
    q.add_argument("--device", choices=["auto", "cpu", "gpu"], default="auto")
    q.add_argument("--all", action="store_true", help="every move of the game")
    q.add_argument("--ema", action="store_true",
                   help="predict with the checkpoint's moving average of the weights")
    q.set_defaults(fn=cmd_predict)
    for name, fn in (("gtp", cmd_gtp), ("selfplay", cmd_selfplay)):
        g = sub.add_parser(name)
        g.add_argument("checkpoint")
        g.add_argument("--ema", action="store_true",
                       help="play with the checkpoint's moving average of the weights")
        g.add_argument("--device", choices=["auto", "cpu", "gpu"], default="auto")
        g.add_argument("--symmetries", type=int, choices=[1, 8], default=8)
        g.add_argument("--temperature", type=float, default=1.0)
        g.add_argument("--top-p", type=float, default=1.0)
        g.add_argument("--seed", type=int, default=0)
        g.add_argument("--rank", type=int, default=9, help="the dan rank shown to the net")
        g.add_argument("--komi", type=float, default=7.5)
        if name == "selfplay":
            g.add_argument("--opponent", help="a second checkpoint: a match, colours alternating")
            g.add_argument("--games", type=int, required=True)
            g.add_argument("--max-moves", type=int, default=400)
            g.add_argument("--opening-plies", type=int, default=0,
                           help="first plies drawn at temperature 1, top_p 1")
            g.add_argument("--batch", type=int, default=64, help="boards per forward")
            g.add_argument("--out", help="directory for the SGFs and summary.json")
        g.set_defaults(fn=fn)
    m = sub.add_parser("makedata")
    m.add_argument("--threads", type=int, default=32)
    m.add_argument("--ko", action="store_true",
                   help="mark the simple-ko point in the stored liberty plane (for ko_plane=1)")
    m.add_argument("--seed", type=int, default=0)
    m.add_argument("rest", nargs="*")
    m.set_defaults(fn=cmd_makedata)
    x = sub.add_parser("export")
    x.add_argument("checkpoint")
    x.add_argument("out")
    x.add_argument("--ema", action="store_true",
                   help="export the checkpoint's moving average of the weights")
    x.set_defaults(fn=cmd_export)
    i = sub.add_parser("import")
    i.add_argument("t7")
    i.add_argument("out")
    i.set_defaults(fn=cmd_import)
    p = sub.add_parser("plot")
    p.add_argument("files", nargs="+")
    p.add_argument("--out", default="curves.png")
    p.set_defaults(fn=cmd_plot)
    b = sub.add_parser("bench")
    b.add_argument("rest", nargs=argparse.REMAINDER)
    b.set_defaults(fn=cmd_bench)
    args = ap.parse_args(argv)
    return args.fn(args)


if __name__ == "__main__":
    sys.exit(main())
