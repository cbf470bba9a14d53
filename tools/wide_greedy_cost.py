"""What k_wide_greedy costs beside k_wide_act, the yardstick: HIP-event times of PPOGroup.wide_act (three passes over
the actions: maximum, sum, inverse CDF), wide_act_greedy (two: maximum with its index, sum) and wide_act_greedy
without the log-prob (one) on the same rows, at a large action space (G, D, A, H) = (2, 50, 3000, 32) and at cfg1's
fully aggregated net (2, 30, 225, 64), 4096 rows per group. Back-to-back launches in blocks, the three alternating, so
that drift of the machine falls on all of them; the median, minimum and maximum over the blocks.

    python tools/wide_greedy_cost.py [out.txt]       (ROWS, BLOCKS, PER_BLOCK from the environment)
"""
import importlib
import os
import statistics
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
ppo = importlib.import_module("marl-scheduling_amd.ppo")

ROWS = int(os.environ.get("ROWS", 4096))
BLOCKS, PER_BLOCK = int(os.environ.get("BLOCKS", 15)), int(os.environ.get("PER_BLOCK", 100))
SHAPES = [(2, 50, 3000, 32), (2, 30, 225, 64)]
out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(REPO, "profiles", "learner_metrics", "wide_greedy_cost.txt")


def block(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(PER_BLOCK):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / PER_BLOCK * 1e3


lines = ["%d rows per group, %d blocks of %d launches, us per launch: median (min .. max)" % (ROWS, BLOCKS, PER_BLOCK)]
for G, D, A, H in SHAPES:
    torch.manual_seed(1)
    grp = ppo.PPOGroup(G, D, A, 3e-4, 1e-3, 0.99, 0.2, 2, "cuda", hidden=H)
    stride = (D + 3) // 4 * 4
    x = torch.zeros((ROWS, G, stride), dtype=torch.int8, device="cuda")
    x[..., :D] = torch.randint(-2, 12, (ROWS, G, D), device="cuda").to(torch.int8)
    u = torch.rand((ROWS, G), device="cuda")
    act = torch.empty((ROWS, G), dtype=torch.int32, device="cuda")
    lp = torch.empty((ROWS, G), dtype=torch.float32, device="cuda")
    runs = {"wide_act (sample)": lambda: grp.wide_act(x, uniforms=u, action=act, logprob=lp),
            "wide_act_greedy": lambda: grp.wide_act_greedy(x, action=act, logprob=lp),
            "wide_act_greedy, no log-prob": lambda: grp.wide_act_greedy(x, action=act, want_logprob=False)}
    for fn in runs.values():
        block(fn)
    times = {k: [] for k in runs}
    for _ in range(BLOCKS):
        for k, fn in runs.items():
            times[k].append(block(fn))
    # what a launch reads: the int8 rows once, W1 / W2 per 16-row tile (L2), W3 and b3 once per pass and tile
    tiles = -(-ROWS // 16) * G
    w3 = 4 * A * (H + 1)
    lines.append("(G, D, A, H) = %s: %d tiles; a tile reads %d B of rows, %d B of W1 / W2 and %d B of W3 / b3 per pass"
                 % ((G, D, A, H), tiles, 16 * D, 4 * (H * D + H * H + 2 * H), w3))
    for k, ts in times.items():
        lines.append("  %-30s %8.2f (%.2f .. %.2f)" % (k, statistics.median(ts), min(ts), max(ts)))
os.makedirs(os.path.dirname(out_path), exist_ok=True)
with open(out_path, "w") as f:
    f.write("\n".join(lines) + "\n")
print("\n".join(lines))
