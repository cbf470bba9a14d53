"""How far apart the two workgroups of a CU run in the one-launch cfg3 rollout (profiling only).

Loads the probe build (tools/_probe/libmarlsched_probe.so from tools/build_phase_probe.sh, -DMS_PHASE_TIMING),
in which every workgroup of k_env_rollout_act_free records its CU (HW_REG_XCC_ID and the SE / SH / CU fields of
HW_REG_HW_ID), its CU rank (MS_FREE_STAGGER != 0) and the s_memrealtime (100 MHz) after the first barrier of
rounds 0..63 and of the last 16. For every setting on the command line a fresh trainer runs a few iterations; the
last rollout launch is reported:
  - how many CUs hold 0, 1, 2, 3 workgroups;
  - per round, over the CUs with two workgroups, the offset between the two as a fraction of the round, folded
    into 0 .. 0.5 (0: in phase, 0.5: half a round apart);
  - the round length and the rollout's time (of the probe build: its stamps cost a little).

Usage: python tools/free_stagger_probe.py [--envs E] [--rounds T] SETTING ...
  SETTING is MS_FREE_STAGGER's value: 0 (the plain kernels) or 1 (the staggered ones, the default).
  MARLSCHED_LIB names another probe build."""
import argparse
import ctypes as ct
import importlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("MARLSCHED_LIB", os.path.join(ROOT, "tools", "_probe", "libmarlsched_probe.so"))
os.environ["MARLSCHED_LENIENT_ABI"] = "1"

HEAD, TAIL = 64, 16
W = 1 + HEAD + TAIL


def analyse(raw, T, n_cus):
    """raw [wgs][W] uint64 -> text lines"""
    lines = []
    assert (raw[:, 0] >> 63).all(), "a workgroup left no record"
    key = (raw[:, 0] & 0xFFFFFFFF).astype(np.int64)
    rank = ((raw[:, 0] >> 32) & 1).astype(np.int64)
    if T - 1 >= HEAD + TAIL:  # (the last round has no acting: no stamp)
        cols = list(range(1, 1 + HEAD)) + list(range(1 + HEAD, W - 1))
        labels = list(range(HEAD)) + list(range(T - TAIL, T - 1))
    else:
        cols = list(range(1, 1 + min(T - 1, HEAD)))
        labels = list(range(min(T - 1, HEAD)))
    st = raw[:, cols].astype(np.float64)
    keys, inv, cnt = np.unique(key, return_inverse=True, return_counts=True)
    hist = np.bincount(cnt, minlength=4)
    hist[0] = n_cus - len(keys)
    lines.append("CUs holding 0 / 1 / 2 / 3+ workgroups: %d / %d / %d / %d  (%d CUs, %d workgroups, %d XCCs seen)"
                 % (hist[0], hist[1], hist[2], hist[3:].sum(), n_cus, len(key), len(np.unique(keys >> 8))))
    period = np.median(np.diff(st[:, :HEAD], axis=1)) if st.shape[1] > 1 else float("nan")
    lines.append("round length (median over workgroups and rounds): %.2f us" % (period / 100.0))
    first = st[:, 0].min()
    lines.append("first-barrier spread of round 0 over all workgroups: %.2f us" % ((st[:, 0].max() - first) / 100.0))
    two = np.flatnonzero(cnt == 2)
    pairs = np.array([np.flatnonzero(inv == k) for k in two]).reshape(-1, 2)
    if len(pairs) == 0:
        return lines
    lines.append("pairs whose two ranks differ: %d of %d" % (int((rank[pairs[:, 0]] != rank[pairs[:, 1]]).sum()),
                                                              len(pairs)))
    # each round's own length per pair (the mean of the two workgroups' distance to their next stamp)
    d = st[pairs[:, 1]] - st[pairs[:, 0]]
    nxt = np.diff(st, axis=1)
    nxt = np.concatenate([nxt, nxt[:, -1:]], axis=1) if nxt.shape[1] else np.full_like(st, period)
    if st.shape[1] > HEAD:
        nxt[:, HEAD - 1] = nxt[:, HEAD - 2]  # (the gap to the tail is no round)
    rl = 0.5 * (nxt[pairs[:, 0]] + nxt[pairs[:, 1]])
    f = np.abs(d) / rl % 1.0
    folded = np.minimum(f, 1.0 - f)
    lines.append("offset of a CU's two workgroups / round, folded to 0 .. 0.5, over %d CUs:" % len(pairs))
    lines.append("  round    mean    p10    p50    p90   share > 0.25   |offset| us p50")
    for i, t in enumerate(labels):
        v = folded[:, i]
        lines.append("  %5d  %6.3f %6.3f %6.3f %6.3f   %6.3f         %8.2f"
                     % (t, v.mean(), np.percentile(v, 10), np.percentile(v, 50), np.percentile(v, 90),
                        (v > 0.25).mean(), np.median(np.abs(d[:, i])) / 100.0))
    lines.append("all stamped rounds: mean folded offset %.3f, share > 0.25 %.3f (a uniformly random phase: 0.25, 0.5)"
                 % (folded.mean(), (folded > 0.25).mean()))
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=16384)
    ap.add_argument("--rounds", type=int, default=200)
    ap.add_argument("--iters", type=int, default=4)
    ap.add_argument("settings", nargs="+", choices=("0", "1"))
    a = ap.parse_args()
    import torch
    tr_mod = importlib.import_module("marl-scheduling_amd.trainer")
    lib = importlib.import_module("marl-scheduling_amd._lib").lib
    lib.ms_probe_free_rounds.argtypes = [ct.POINTER(ct.c_ulonglong), ct.c_int]
    n_cus = torch.cuda.get_device_properties(0).multi_processor_count
    for mode in a.settings:
        os.environ["MS_FREE_STAGGER"] = mode
        tr = tr_mod.Trainer.from_named("cfg3", n_envs=a.envs, update_step=a.rounds, seed=0, device="cuda:0")
        assert tr.fused_rollout_free and len(tr.env.parts) == 1
        wgs = -(-a.envs // (4 * tr.N))
        ms = []
        for it in range(a.iters):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            tr.rollout(defer_common=True)
            e1.record()
            tr.update()
            torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1))
        buf = (ct.c_ulonglong * (W * wgs))()
        assert lib.ms_probe_free_rounds(buf, wgs) == 0
        raw = np.frombuffer(buf, dtype=np.uint64).reshape(wgs, W)
        lines = analyse(raw, a.rounds, n_cus)
        print("== MS_FREE_STAGGER=%s  E %d  T %d" % (mode, a.envs, a.rounds))
        print("rollout (probe build, graph replays): " + " ".join("%.3f" % x for x in ms[2:]) + " ms")
        print("\n".join(lines))
        sys.stdout.flush()
        del tr
        torch.cuda.synchronize()


if __name__ == "__main__":
    main()
