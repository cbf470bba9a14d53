"""What a checkpoint costs at cfg3, E = 16384, T = 200 (writes profiles/r12_checkpoint/cost.json).

  - bytes (counted): the snapshot's size and the live liability entries per replica (min / mean / max) after 5
    and after 50 iterations of training;
  - snapshot() against torch.clone() of tensors the size of the three raw state arrays (records, both MT halves,
    chains), alternating in the same run, device events, 20 repetitions: what a checkpoint without the pack
    kernel would copy before its transfer. Criterion: median pack <= median raw clone;
  - wall time of save_checkpoint() (split: pack, device-to-host copy, file write) and load_checkpoint(), beside
    one iteration() and the only route there was before: export_state() + pickle.dump.

Usage: python tools/checkpoint_cost.py [--envs 16384] [--steps 200] [--out profiles/r12_checkpoint/cost.json]
"""
import argparse
import importlib
import json
import os
import pickle
import statistics
import sys
import tempfile
import time

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def _stats(xs):
    return dict(median=statistics.median(xs), min=min(xs), max=max(xs), spread=max(xs) - min(xs), n=len(xs))


def _entries(env, snap):
    """Live entries per replica, from the snapshot's liab_off section."""
    E, rb = env.E, env.shape.env_record_bytes
    o_off = ((64 + len(bytes(env.cfg)) + 15) & ~15) + E * (rb + 2496)
    off = snap[o_off:o_off + 8 * (E + 1)].cpu().numpy().view("<u8").astype("int64")
    n = off[1:] - off[:-1]
    return dict(min=int(n.min()), mean=float(n.mean()), max=int(n.max()), total=int(off[-1]))


def _event_ms(fn, sync):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    sync()
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=16384)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "r12_checkpoint", "cost.json"))
    ap.add_argument("--dir", default=None, help="where the checkpoint files are written (default: a temporary directory)")
    args = ap.parse_args()
    trainer = importlib.import_module("marl-scheduling_amd.trainer")
    dev = torch.device("cuda:0")
    sync = lambda: torch.cuda.synchronize(dev)
    tr = trainer.Trainer.from_named("cfg3", n_envs=args.envs, update_step=args.steps, seed=1, device=dev)
    env = tr.env.parts[0][0]
    E, C, s = env.E, env.C, env.shape
    raw_sizes = dict(records=E * s.env_record_bytes, mt=E * 2 * 2496, chains=E * C * s.liability_cap * 8)
    res = dict(config="cfg3", E=E, T=args.steps, raw_bytes=dict(raw_sizes, total=sum(raw_sizes.values())))
    for _ in range(5):
        tr.iteration()
    sync()
    snap = env.snapshot()
    res["after_5_iterations"] = dict(snapshot_bytes=snap.numel(), entries_per_replica=_entries(env, snap))

    # ---- snapshot() against the raw clone, alternating
    raw = [torch.zeros(n, dtype=torch.uint8, device=dev) for n in raw_sizes.values()]
    buf = torch.empty(snap.numel() + (1 << 20), dtype=torch.uint8, device=dev)
    pack, pack_out, clone = [], [], []
    for i in range(args.reps + 3):
        t_pack, _ = _event_ms(env.snapshot, sync)
        t_out, _ = _event_ms(lambda: env.snapshot(out=buf), sync)
        t_clone, keep = _event_ms(lambda: [x.clone() for x in raw], sync)
        del keep
        if i >= 3:  # warm-up: the allocator's blocks, the kernels' code
            pack.append(t_pack)
            pack_out.append(t_out)
            clone.append(t_clone)
    res["snapshot_ms"] = _stats(pack)
    res["snapshot_into_buffer_ms"] = _stats(pack_out)
    res["raw_clone_ms"] = _stats(clone)
    res["criterion_pack_not_above_clone"] = bool(res["snapshot_ms"]["median"] <= res["raw_clone_ms"]["median"])

    # ---- save / load beside an iteration and the export + pickle route
    with tempfile.TemporaryDirectory(dir=args.dir) as d:
        path = os.path.join(d, "run.ckpt")
        saves, loads, iters, exports = [], [], [], []
        for _ in range(5):
            sync()
            t0 = time.perf_counter()
            info = tr.save_checkpoint(path)
            sync()
            saves.append(dict(info, total_s=time.perf_counter() - t0))
            t0 = time.perf_counter()
            tr.iteration()
            sync()
            iters.append(time.perf_counter() - t0)
        for _ in range(3):
            sync()
            t0 = time.perf_counter()
            tr.load_checkpoint(path)
            sync()
            loads.append(time.perf_counter() - t0)
        for _ in range(2):
            sync()
            t0 = time.perf_counter()
            st = env.export_state()
            t1 = time.perf_counter()
            with open(os.path.join(d, "export.pkl"), "wb") as f:
                pickle.dump(st, f, protocol=pickle.HIGHEST_PROTOCOL)
                f.flush()
                os.fsync(f.fileno())
            exports.append(dict(export_s=t1 - t0, pickle_s=time.perf_counter() - t1, total_s=time.perf_counter() - t0,
                                file_bytes=os.path.getsize(os.path.join(d, "export.pkl"))))
            del st
    med = lambda rows, k: statistics.median(r[k] for r in rows)
    res["save_checkpoint_s"] = {k: med(saves, k) for k in ("total_s", "pack_s", "copy_s", "write_s")}
    res["save_checkpoint_s"].update(file_bytes=saves[-1]["file_bytes"], snapshot_bytes=saves[-1]["snapshot_bytes"], n=len(saves))
    res["load_checkpoint_s"] = dict(median=statistics.median(loads), n=len(loads))
    res["iteration_s"] = dict(median=statistics.median(iters), n=len(iters))
    res["export_state_pickle_s"] = {k: med(exports, k) for k in ("total_s", "export_s", "pickle_s")}
    res["export_state_pickle_s"].update(file_bytes=exports[-1]["file_bytes"], n=len(exports))

    # ---- the chains under a policy trained for longer
    while tr.iterations < 50:
        tr.iteration()
    sync()
    snap = env.snapshot()
    res["after_50_iterations"] = dict(snapshot_bytes=snap.numel(), entries_per_replica=_entries(env, snap))
    assert tr.flags() == 0
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(res, sort_keys=True))


if __name__ == "__main__":
    main()
