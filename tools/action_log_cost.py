"""What ms_action_hist and ms_action_table cost on the rings of a cfg3 rollout, E = 16384, T = 200: HIP-event times
of ppo.action_hist / ppo.action_table per source (back-to-back launches in blocks, the sources alternating, as
tools/evaluate_cost.py) with the bytes each launch reads and the rate that makes, and k_unit_returns on the offer
rewards as the project's own memory-bound yardstick on the same machine. The rings are those of one eager rollout
(no graph is captured or replayed), read as the rollout left them: the acceptor ring incomplete, the owned acceptor
items by core, the offers compact (the offer table's key is the pair's first byte).

Then what Trainer.iteration() takes with the action log off, with the histograms and with the tables too (graphs
as in training): HIP events around blocks of ITER_PER_BLOCK iterations, the three trainers alternating, medians
over ITER_BLOCKS blocks, with the spread of the log-off blocks. ITER_BLOCKS=0 leaves that part out; LOGS="off"
measures the log-off trainer alone (what a commit without the log can be compared by).

    python tools/action_log_cost.py [out.txt]       (E, BLOCKS, PER_BLOCK, ITER_BLOCKS, ITER_PER_BLOCK, LOGS from
                                                     the environment)
"""
import importlib
import os
import statistics
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
tr_mod = importlib.import_module("marl-scheduling_amd.trainer")
ppo = importlib.import_module("marl-scheduling_amd.ppo")

E = int(os.environ.get("E", 16384))
BLOCKS, PER_BLOCK = int(os.environ.get("BLOCKS", 9)), int(os.environ.get("PER_BLOCK", 20))
out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(REPO, "profiles", "action_log", "cost.txt")


def block(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(PER_BLOCK):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / PER_BLOCK * 1e3


tr = tr_mod.Trainer.from_named("cfg3", n_envs=E, seed=1, device="cuda:0", use_graph=False)  # update_step 200
tr.rollout(defer_common=True)
assert tr.fused_rollout_free and tr.acc_own is not None
T, N, C, L, s = tr.T, tr.N, tr.C, tr.L, tr.env.shape
lines = ["cfg3, E = %d, T = %d, episodes of %d rounds, the rings of the first rollout" % (E, T, tr.ep_len)]
nbytes = lambda *ts: sum(t.numel() for t in ts)
z = lambda bins, A: torch.zeros((3, bins, A), dtype=torch.int64, device=tr.device)
h = dict(offer=z(N * L, s.off_actions), price=z(N * L, s.price_actions), acceptor=z(N * C, s.acc_actions))
kw = dict(round0=0, episode_length=tr.ep_len)
own, off, price, ring = tr.acc_owner[:T], tr.off.actions_raw, tr.price.actions_raw, tr.acc.actions_raw
launches = {
    "offer    (all,   [T][E][%d], A %d)" % (N * L, s.off_actions):
        (lambda: ppo.action_hist(off, h["offer"], **kw), nbytes(off)),
    "price    (gated, [T][E][%d], A %d)" % (N * L, s.price_actions):
        (lambda: ppo.action_hist(price, h["price"], gate=off, **kw), nbytes(price, off)),
    "acceptor (owner, by core [T-1][E][%d], A %d)" % (C, s.acc_actions):
        (lambda: ppo.action_hist(tr.acc_own[0][1:], h["acceptor"], owner=own[1:], n_agents=N, **kw),
         nbytes(tr.acc_own[0][1:], own[1:])),
    "acceptor (owner, by unit, ring slot 0 [1][E][%d]; the wrapper's host time shows)" % (N * C):
        (lambda: ppo.action_hist(ring[:1], h["acceptor"], owner=own[:1], n_agents=N, **kw), nbytes(own[:1]) * 2),
    "acceptor (owner, by unit [T][E][%d], one byte in eight of the ring's lines used)" % (N * C):
        (lambda: ppo.action_hist(ring, h["acceptor"], owner=own, n_agents=N, **kw), nbytes(own) + nbytes(ring)),
}
P = max(tr.cfg.job_priority[: tr.cfg.n_kinds]) + 1
tab = dict(offer=torch.zeros((3, N, P, s.off_actions), dtype=torch.int64, device=tr.device),
           price=torch.zeros((3, N, P, s.price_actions), dtype=torch.int64, device=tr.device))
skipped = torch.zeros(1, dtype=torch.int64, device=tr.device)
if tr.off_compact:
    off_key, key_name = tr.off_pair.view(torch.int8).view(T + 1, E, N * L, 2)[:T, :, :, 0], "off_pair byte 0, stride 2"
else:
    off_key, key_name = tr._off_obs[:T, :, :, 2 * C], "offer rows byte 2C"
price_key = tr.price_obs[..., 2]
launches.update({
    "offer by priority (table, [T][E][%d], key %s, %d x %d per agent)" % (N * L, key_name, P, s.off_actions):
        (lambda: ppo.action_table(off, off_key, tab["offer"], units_per_bin=L, skipped=skipped, **kw),
         nbytes(off) + 2 * nbytes(off_key)),  # (a pair's other byte shares its sector)
    "price by priority (table, [T][E][%d], key price_obs byte 2, stride 4, %d x %d per agent)" % (
        N * L, P, s.price_actions):
        (lambda: ppo.action_table(price, price_key, tab["price"], units_per_bin=L, skipped=skipped, **kw),
         nbytes(price) + 4 * nbytes(price_key)),  # (the state's other bytes share its sector)
})
sel = torch.arange(N, dtype=torch.int32, device=tr.device) * L
launches["k_unit_returns offer rewards [T][E][%d] f32 -> [T][E][%d]" % (N * L, N)] = (
    lambda: ppo.unit_returns(tr.off.rewards, sel, tr.off.group.gamma), 4 * nbytes(tr.off.rewards) + 4 * T * E * N)
for fn, _ in launches.values():
    block(fn)
times = {k: [] for k in launches}
for _ in range(BLOCKS):
    for k, (fn, _) in launches.items():
        times[k].append(block(fn))
for k, (_, nb) in launches.items():
    ts = times[k]
    med = statistics.median(ts)
    lines.append("%s: %.2f us (%.2f .. %.2f), %.1f MB, %.0f GB/s" % (k, med, min(ts), max(ts), nb / 1e6, nb / med / 1e3))

# ---- iteration() with the log off / histograms / tables
ITER_BLOCKS, ITER_PER_BLOCK = int(os.environ.get("ITER_BLOCKS", 7)), int(os.environ.get("ITER_PER_BLOCK", 4))
LOGS = os.environ.get("LOGS", "off,hist,tables").split(",")
if ITER_BLOCKS > 0:
    del tr, launches, h, tab
    torch.cuda.empty_cache()
    kinds = dict(off={}, hist=dict(action_log=True), tables=dict(action_log=True, action_tables=True))
    trs = {k: tr_mod.Trainer.from_named("cfg3", n_envs=E, seed=1, device="cuda:0", **kinds[k]) for k in LOGS}
    for t in trs.values():  # eager, capture, replay
        for _ in range(3):
            t.iteration()
    torch.cuda.synchronize()
    saved, PER_BLOCK = PER_BLOCK, ITER_PER_BLOCK
    it = {k: [] for k in trs}
    for _ in range(ITER_BLOCKS):
        for k, t in trs.items():
            it[k].append(block(t.iteration) / 1e3)
    PER_BLOCK = saved
    lines.append("iteration(), cfg3, E = %d, T = %d: device ms per iteration, median of %d blocks of %d (min .. max)"
                 % (E, T, ITER_BLOCKS, ITER_PER_BLOCK))
    for k, ts in it.items():
        lines.append("  action log %-6s: %.3f ms (%.3f .. %.3f)%s" % (
            k, statistics.median(ts), min(ts), max(ts),
            "" if k == "off" or "off" not in it else ", %+.3f ms against off" % (
                statistics.median(ts) - statistics.median(it["off"]))))
os.makedirs(os.path.dirname(out_path), exist_ok=True)
with open(out_path, "w") as f:
    f.write("\n".join(lines) + "\n")
print("\n".join(lines))
