"""What the update diagnostics cost at cfg3, E = 16384, diagnostics = 8: HIP-event times of ms_policy_evaluate at the
three unit shapes on the rows update_diagnostics gathers (back-to-back launches in blocks, the three alternating,
as tools/greedy_act_cost.py), the whole update_diagnostics pass per iteration beside the iteration itself, and the
bytes of the kept diagnostic tensors.

    python tools/evaluate_cost.py [out.txt]       (E, K, BLOCKS, PER_BLOCK, ITERS from the environment)
"""
import importlib
import os
import statistics
import sys
import time

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
tr_mod = importlib.import_module("marl-scheduling_amd.trainer")

E, K = int(os.environ.get("E", 16384)), int(os.environ.get("K", 8))
BLOCKS, PER_BLOCK = int(os.environ.get("BLOCKS", 15)), int(os.environ.get("PER_BLOCK", 100))
ITERS = int(os.environ.get("ITERS", 20))
out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(REPO, "profiles", "evaluate", "cost.txt")

tr = tr_mod.Trainer.from_named("cfg3", n_envs=E, seed=1, device="cuda:0")  # update_step 200: the benchmark's
for _ in range(3):
    tr.iteration()
slots = [((2 * i + 1) * tr.T) // (2 * K) for i in range(K)]  # what Trainer(diagnostics=K) evaluates
tr.update_diagnostics(slots=slots)
lines =["cfg3, E = %d, T = %d, %d slots, centralisation_sample %d" % (E, tr.T, K, tr.hp.centralisation_sample)]


def launch_of(u):
    b = tr._diag[u.name]
    G = u.group.policy.G
    R = b["act"].numel() // G
    args = (b["obs"].view(R, G, u.stride), b["act"].view(R, G), G)
    outs = dict(logprob=b["new"].view(R, G), value=b["val"].view(R, G), entropy=b["ent"].view(R, G))
    return (lambda: u.group.policy.evaluate_hip(*args, **outs)), R, G


def block(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(PER_BLOCK):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / PER_BLOCK * 1e3


launches = {u.name: launch_of(u) for u in tr.units()}
for fn, _, _ in launches.values():
    block(fn)
times = {k: [] for k in launches}
for _ in range(BLOCKS):
    for k, (fn, _, _) in launches.items():
        times[k].append(block(fn))
for u in tr.units():
    ts, (_, R, G) = times[u.name], launches[u.name]
    lines.append("ms_policy_evaluate %-8s rows %d x %d groups, stride %d, A %d: %.2f us (%.2f .. %.2f)" %
                 (u.name, R, G, u.stride, u.group.policy.A, statistics.median(ts), min(ts), max(ts)))

diag, it = [], []
for _ in range(ITERS):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    tr.iteration()
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    tr.update_diagnostics(slots=slots)
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    it.append((t1 - t0) * 1e3)
    diag.append((t2 - t1) * 1e3)
lines.append("iteration (wall, synchronised): %.2f ms (%.2f .. %.2f)" % (statistics.median(it), min(it), max(it)))
lines.append("update_diagnostics (wall, synchronised, the lists on the host): %.2f ms (%.2f .. %.2f)" %
             (statistics.median(diag), min(diag), max(diag)))
# where the pass spends its time: the rings an iteration() leaves incomplete are completed at their first read
# (offer rows of slots 1..T-1 expanded, the acceptor rings' common items filled), the returns are one scan of the
# reward ring per unit type; the rest is the gathers, the three evaluation launches and the float64 reductions
ppo = importlib.import_module("marl-scheduling_amd.ppo")
stages = {k: [] for k in ("off_obs (offer_expand of the ring)", "acceptor rings (fill_common)", "unit_returns x3",
                          "the rest (rings complete)")}


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


for _ in range(ITERS):
    tr.iteration()
    ms = [timed(lambda: tr.off_obs), timed(lambda: tr.acc.actions),
          timed(lambda: [ppo.unit_returns(u.rewards, tr._diag[u.name]["sel32"], u.group.gamma) for u in tr.units()]),
          timed(lambda: tr.update_diagnostics(slots=slots))]
    for k, v in zip(stages, ms):
        stages[k].append(v)
for k, v in stages.items():
    lines.append("  %s: %.2f ms (%.2f .. %.2f)" % (k, statistics.median(v), min(v), max(v)))
bound = sum(len(tr._last_draws[u.name]) * K * E * u.group.policy.G * (u.stride + 17) for u in tr.units())
lines.append("diagnostic tensors: %d bytes (draws x k x E x G x (stride + 17) over the unit types: %d)" %
             (tr.diagnostics_bytes(), bound))
os.makedirs(os.path.dirname(out_path), exist_ok=True)
with open(out_path, "w") as f:
    f.write("\n".join(lines) + "\n")
print("\n".join(lines))
