"""HIP-event times of one cfg3 round's acting at E = 16384 on a trained round's observations: the greedy launch
(ms_act_round_greedy) beside the sampling launch it parallels (ms_act_round_free, as the trainer issues it:
act fragments + price table, and without them). The launches alternate in blocks, so drift hits both alike;
per launch: the median over the blocks and the blocks' spread.

    python tools/greedy_act_cost.py [out.txt]       (E, BLOCKS, PER_BLOCK from the environment)
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
BLOCKS, PER_BLOCK = int(os.environ.get("BLOCKS", 31)), int(os.environ.get("PER_BLOCK", 200))
out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(REPO, "profiles", "greedy", "act_round.txt")

tr = tr_mod.Trainer.from_named("cfg3", n_envs=E, update_step=8, seed=1, device="cuda:0")
tr.iteration()
tr._prepare_acting()  # the fragments and the price table of the weights the update left
t = 3
N, C, L = tr.N, tr.C, tr.L
core, price, acc = tr.off.group.policy_old, tr.price.group.policy_old, tr.acc.group.policy_old
off_obs, rows, owner = tr.off_obs[t], tr.acc_rows[t], tr.acc_owner[t]
samp = dict(core_action=tr.off.actions[t], core_logprob=tr.off.logprobs[t], price_state=tr.price_obs[t],
            price_action=tr.price.actions[t], price_logprob=tr.price.logprobs[t], env_price=tr.env_price)
i8 = lambda *s: torch.zeros(s, dtype=torch.int8, device=tr.device)
gout = dict(core_action=i8(E, N * L), price_state=i8(E, N * L, 4), price_action=i8(E, N * L), env_price=i8(E, N * L))
gacc = i8(E, N * C)

launches = {
    "ms_act_round_greedy": lambda: ppo.act_round_greedy(core, price, off_obs, acc, rows, owner, tr.acc_common, C, gout,
                                                        gacc),
    "ms_act_round_free (fragments + price table: the trainer's)": lambda: ppo.act_round_free(
        core, price, off_obs, acc, rows, owner, tr.acc_common, C, 1, 1, 3, samp, tr.acc.actions[t], tr.acc.logprobs[t],
        price_table=tr.price_table, core_frag=tr.off_frag, acc_frag=tr.acc_frag),
    "ms_act_round_free (weights and tables derived per wave)": lambda: ppo.act_round_free(
        core, price, off_obs, acc, rows, owner, tr.acc_common, C, 1, 1, 3, samp, tr.acc.actions[t], tr.acc.logprobs[t]),
}


def block(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(PER_BLOCK):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / PER_BLOCK * 1e3


for fn in launches.values():  # warm-up: code objects loaded, clocks up
    block(fn)
times = {k: [] for k in launches}
for _ in range(BLOCKS):
    for k, fn in launches.items():
        times[k].append(block(fn))
own = float((owner > 0).float().mean())
lines = ["cfg3 act round, E = %d (%d offer rows, %d acceptor items, %.0f %% of the cores owned), %s" %
         (E, E * N * L, E * N * C, 100 * own, torch.cuda.get_device_name(0)),
         "us per launch from HIP events around %d back-to-back launches; %d such blocks per launch, alternating" %
         (PER_BLOCK, BLOCKS), ""]
for k, v in times.items():
    q = statistics.quantiles(v, n=4)
    lines.append("%-62s median %7.2f  min %7.2f  max %7.2f  quartiles %7.2f .. %7.2f" %
                 (k, statistics.median(v), min(v), max(v), q[0], q[2]))
text = "\n".join(lines) + "\n"
print(text)
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    f.write(text)
