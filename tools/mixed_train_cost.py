#!/usr/bin/env python3
"""What a mixed market costs the cfg2 training loop: ms per iteration of three trainers in one process, the runs
alternating so that clock drift falls on all alike:

  unmasked        Trainer.from_named("cfg2")                         one ms_env_rollout_act launch per rollout
  mixed, 1 launch hardcoded_agents=[0]                               one ms_env_rollout_act_mixed launch
  mixed, pairs    hardcoded_agents=[0], MS_ENV_FUSED_ACT=0           an act launch and ms_env_step_mixed per round

Usage: python tools/mixed_train_cost.py [--steps 20] [--warmup 5] [--repeats 3] [--envs N] [--update-step 200]
Prints one JSON line: per variant every repeat's ms per iteration (wall clock over `steps` iterations after a
device synchronisation), its rollout / update split from the trainer's device timings, median and max - min."""
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
    args = ap.parse_args()
    import torch
    tr = importlib.import_module("marl-scheduling_amd.trainer")

    def make(mask, env):
        old = {k: os.environ.get(k) for k in env}
        os.environ.update(env)
        try:
            return tr.Trainer.from_named("cfg2", n_envs=args.envs, update_step=args.update_step, seed=0,
                                         device="cuda:0", hardcoded_agents=mask)
        finally:
            for k, v in old.items():
                os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)

    variants = {"unmasked": make(None, {}), "mixed_one_launch": make([0], {}),
                "mixed_pairs": make([0], dict(MS_ENV_FUSED_ACT="0"))}
    assert variants["mixed_one_launch"].fused_rollout and not variants["mixed_pairs"].fused_step
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
    out = dict(config="cfg2", envs=variants["unmasked"].E, update_step=args.update_step, steps=args.steps,
               warmup=args.warmup, variants={})
    for name, rs in runs.items():
        ms = [r["ms_per_iteration"] for r in rs]
        out["variants"][name] = dict(runs=rs, median_ms=statistics.median(ms), spread_ms=max(ms) - min(ms),
                                     median_rollout_ms=statistics.median(r["rollout_ms"] for r in rs))
        assert variants[name].flags() == 0
    print(json.dumps(out))


if __name__ == "__main__":
    main()
