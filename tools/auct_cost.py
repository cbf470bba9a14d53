#!/usr/bin/env python3
"""What a learned auctioneer costs the cfg2 rollout: three trainers in one process, the runs alternating so that
clock drift falls on all alike:

  plain          Trainer.from_named("cfg2")                              one ms_env_rollout_act launch per rollout
  auct_one       learned_auctioneer=True                                 one ms_env_rollout_act_auct launch
  auct_pairs     learned_auctioneer=True, MS_ENV_FUSED_ACT=0             an act launch, act_compact and env.step per round

Usage: python tools/auct_cost.py [--steps 20] [--warmup 5] [--repeats 3] [--envs N] [--update-step 200] [--curve K]
Prints one JSON line: per variant every repeat's ms per iteration (wall clock over `steps` iterations after a device
synchronisation) with its rollout / update split from the trainer's device timings, the medians, us per round of the
rollout (rollout ms / update_step: the launch and round 0's acting) and the ratio to `plain`. --curve K: also K
iterations of a fourth trainer with metrics, whose replica-averaged auctioneerRew per episode is recorded (a smoke
result: whether the auctioneer learns anything useful is not claimed)."""
import argparse
import importlib
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--envs", type=int, default=None)
    ap.add_argument("--update-step", type=int, default=200)
    ap.add_argument("--curve", type=int, default=0)
    args = ap.parse_args()
    import torch
    tr = importlib.import_module("marl-scheduling_amd.trainer")

    def make(auct, env, **kw):
        old = {k: os.environ.get(k) for k in env}
        os.environ.update(env)
        try:
            return tr.Trainer.from_named("cfg2", n_envs=args.envs, update_step=args.update_step, seed=0,
                                         device="cuda:0", learned_auctioneer=auct, **kw)
        finally:
            for k, v in old.items():
                os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)

    variants = {"plain": make(False, {}), "auct_one": make(True, {}),
                "auct_pairs": make(True, dict(MS_ENV_FUSED_ACT="0"))}
    assert variants["plain"].fused_rollout and variants["auct_one"].fused_rollout
    assert not variants["auct_pairs"].fused_step
    for t in variants.values():
        for _ in range(args.warmup):
            t.iteration()
    torch.cuda.synchronize()
    runs = {k: [] for k in variants}
    for _ in range(args.repeats):
        for name, t in variants.items():
            t.timings = dict(rollout=0.0, update=0.0)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                t.iteration()
            torch.cuda.synchronize()
            ms = (time.perf_counter() - t0) * 1e3 / args.steps
            tm = t.timings
            runs[name].append(dict(ms_per_iteration=ms, rollout_ms=tm["rollout"] * 1e3 / args.steps,
                                   update_ms=tm["update"] * 1e3 / args.steps))
    out = dict(config="cfg2", envs=variants["plain"].E, update_step=args.update_step, steps=args.steps,
               warmup=args.warmup, variants={})
    for name, rs in runs.items():
        ms = [r["ms_per_iteration"] for r in rs]
        ro = statistics.median(r["rollout_ms"] for r in rs)
        out["variants"][name] = dict(runs=rs, median_ms=statistics.median(ms), spread_ms=max(ms) - min(ms),
                                     median_rollout_ms=ro, rollout_us_per_round=ro * 1e3 / args.update_step,
                                     median_update_ms=statistics.median(r["update_ms"] for r in rs))
        assert variants[name].flags() == 0
    base = out["variants"]["plain"]["rollout_us_per_round"]
    for v in out["variants"].values():
        v["rollout_ratio_to_plain"] = v["rollout_us_per_round"] / base
    if args.curve:
        t = make(True, {}, metrics=True)
        for _ in range(args.curve):
            t.iteration()
        out["auctioneerRew_per_episode"] = [float(sum(d["auctioneerRew"] for d in ep) / len(ep))
                                            for ep in t.episode_log]
        out["curve_iterations"] = args.curve
    print(json.dumps(out))


if __name__ == "__main__":
    main()
