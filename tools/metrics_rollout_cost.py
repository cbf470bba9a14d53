"""Rollout time of Trainer.iteration() with episode metrics on or off, at the BASELINE sizes (cfg3 16384 x T 200,
cfg2 4096 x T 200, episode_length 100), from Trainer.timings: one JSON line per run. bench.py has no metrics
switch; this is the measurement behind DESIGN §4's "metrics on the one-launch rollouts" table.

Usage: python tools/metrics_rollout_cost.py cfg3|cfg2 [--metrics 0|1] [--iters 20] [--warmup 5] [--label NAME]
A/B against another library: MARLSCHED_LENIENT_ABI=1 MARLSCHED_LIB=tools/_variants/<name>/libmarlsched.so (an
ABI < 21 library runs metrics on the launch-per-round path); MS_ROLLOUT_METRICS=0 does the same on this build."""
import argparse
import importlib
import json
import os
import statistics
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

ap = argparse.ArgumentParser()
ap.add_argument("config", choices=["cfg2", "cfg3"])
ap.add_argument("--metrics", type=int, default=1)
ap.add_argument("--iters", type=int, default=20)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--envs", type=int, default=0)
ap.add_argument("--steps", type=int, default=200)
ap.add_argument("--label", default="")
a = ap.parse_args()

tr_mod = importlib.import_module("marl-scheduling_amd.trainer")
lib_mod = importlib.import_module("marl-scheduling_amd._lib")
E = a.envs or {"cfg3": 16384, "cfg2": 4096}[a.config]
t = tr_mod.Trainer.from_named(a.config, n_envs=E, update_step=a.steps, seed=1, device="cuda:0",
                              metrics=bool(a.metrics), episode_length=100)
for _ in range(a.warmup):
    t.iteration()
torch.cuda.synchronize()
t.timings = dict(rollout=0.0, update=0.0)
per_it, last = [], 0.0
for _ in range(a.iters):
    t.iteration()
    now = t.timings["rollout"]  # (synchronises on the iteration's events)
    per_it.append((now - last) * 1e3)
    last = now
assert t.flags() == 0
tm = t.timings
print(json.dumps(dict(label=a.label, config=a.config, envs=E, steps=a.steps, metrics=a.metrics, abi=lib_mod.ABI_LOADED,
                      fused_rollout=bool(t.fused_rollout), fused_rollout_free=bool(t.fused_rollout_free),
                      episodes=len(t.episode_log), iters=a.iters,
                      rollout_ms=round(tm["rollout"] / a.iters * 1e3, 4), update_ms=round(tm["update"] / a.iters * 1e3, 4),
                      rollout_ms_min=round(min(per_it), 4), rollout_ms_median=round(statistics.median(per_it), 4),
                      rollout_ms_max=round(max(per_it), 4),
                      us_per_round=round(tm["rollout"] / a.iters / a.steps * 1e6, 3))))
