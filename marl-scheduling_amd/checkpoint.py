"""Checkpoints of a ``Trainer``: stop a run and resume it bit for bit, or evaluate a saved policy elsewhere.

A checkpoint is one ``torch.save`` file that ``torch.load(path, weights_only=True)`` reads: tensors, numbers,
strings, tuples, lists and dicts only (Python's ``random`` state is its tuple of ints, the env configuration
a uint8 tensor of the ``ms_config`` bytes, numpy arrays of the episode log are tensors). It is written to
``path + ".tmp"`` beside the target, flushed and fsynced, then moved over it with ``os.replace``: a save that
fails leaves an existing ``path`` as it was.

The file holds a *manifest* (what the trainer must be for the state to fit; compared field by field on
load) and the *state*: the nets, the Adam moments and step counts, the sub-unit and Philox counters, one
packed env snapshot per replica part (``BatchedEnv.snapshot``) and, with metrics, the episode accumulators
and the episode log. The rollout rings are not saved: the next rollout overwrites them, and ring slot 0 (the
observation the next rollout acts on) is a function of the env state, re-emitted with ``env.reset`` as
``Trainer.__init__`` does.

Several ranks: every rank saves and loads a file of its own (the caller passes a per-rank path); no
collective is used.

The functions of the first half (file and manifest) touch no device.
"""
from __future__ import annotations

import dataclasses
import os
import time

import numpy as np
import torch

from . import abi

MAGIC = "marlsched-checkpoint"
FORMAT_VERSION = 1


# ---- file
def write_file(path: str, manifest: dict, state: dict) -> None:
    """The checkpoint file, atomically: path + ".tmp" (same directory) is written, flushed and fsynced, then
    renamed over path. Whatever fails, an existing path stays untouched and no .tmp is left behind."""
    path = os.fspath(path)
    tmp = path + ".tmp"
    try:
        with open(tmp, "wb") as f:
            torch.save(dict(magic=MAGIC, version=FORMAT_VERSION, manifest=manifest, state=state), f)
            f.flush()
            os.fsync(f.fileno())
        os.replace(tmp, path)
    except BaseException:
        try:
            os.unlink(tmp)
        except OSError:
            pass
        raise
    try:  # the rename itself, where the platform lets a directory be synced
        fd = os.open(os.path.dirname(os.path.abspath(path)), os.O_RDONLY)
        try:
            os.fsync(fd)
        finally:
            os.close(fd)
    except OSError:
        pass


def read_file(path: str):
    """(manifest, state) of a checkpoint file, every tensor on the CPU. ValueError for a file that is not a
    readable checkpoint of this format version (truncated, another magic, another version)."""
    try:
        obj = torch.load(os.fspath(path), map_location="cpu", weights_only=True)
    except FileNotFoundError:
        raise
    except Exception as exc:  # a truncated archive, a pickle weights_only refuses, ...
        raise ValueError("%s is not a readable checkpoint: %s" % (path, exc)) from exc
    if not isinstance(obj, dict) or obj.get("magic") != MAGIC:
        raise ValueError("%s is not a marlsched checkpoint (magic %r)" % (path, obj.get("magic") if isinstance(obj, dict) else None))
    if obj.get("version") != FORMAT_VERSION:
        raise ValueError("%s has checkpoint format version %r, this package reads %d" % (path, obj.get("version"), FORMAT_VERSION))
    if not isinstance(obj.get("manifest"), dict) or not isinstance(obj.get("state"), dict):
        raise ValueError("%s: manifest or state missing" % path)
    return obj["manifest"], obj["state"]


# ---- manifest
def config_tensor(cfg: abi.MsConfig) -> torch.Tensor:
    """The ms_config bytes as a uint8 CPU tensor."""
    return torch.tensor(list(bytes(cfg)), dtype=torch.uint8)


def config_of(t: torch.Tensor) -> abi.MsConfig:
    return abi.MsConfig.from_buffer_copy(bytes(t.to(torch.uint8).tolist()))


def make_manifest(cfg: abi.MsConfig, arch: str, E: int, T: int, hyper, seed: int, rank: int = 0, world_size: int = 1,
                  parts: int = 1, free: bool = False, compact: bool = True, fused: bool = True,
                  price_unit_major: bool = False, metrics: bool = False, ep_len: int = 1, metric_slots: int = 1,
                  hardcoded_agents=None, action_log=None, learned_auctioneer: bool = False) -> dict:
    """What a trainer must be for a checkpoint's state to fit it (compare_manifest's order of fields).
    hardcoded_agents: the rule-based agents of a mixed market, a field only when there are some (a file without
    the field, as every file written before the field existed, has none). action_log: "hist" or "tables" for a
    trainer with the action log, a field only then, in the same way. learned_auctioneer: True for a trainer with
    the auctioneer's net, a field only then."""
    m = dict(format=FORMAT_VERSION, config=config_tensor(cfg), arch=str(arch), E=int(E), T=int(T))
    for f in dataclasses.fields(hyper):
        v = getattr(hyper, f.name)
        m["hyper." + f.name] = dict(v) if isinstance(v, dict) else v
    # seed keys the Philox draws baked into the captured launches; rank / world_size / parts the replicas'
    # seeds and the draws' row bases
    m.update(seed=int(seed), rank=int(rank), world_size=int(world_size), parts=int(parts), free=bool(free),
             compact=bool(compact), fused=bool(fused), price_unit_major=bool(price_unit_major),
             metrics=bool(metrics), ep_len=int(ep_len), metric_slots=int(metric_slots))
    if hardcoded_agents:
        m["hardcoded_agents"] = sorted(int(a) for a in hardcoded_agents)
    if action_log:
        m["action_log"] = str(action_log)
    if learned_auctioneer:
        m["learned_auctioneer"] = True
    return m


def compare_manifest(want: dict, got: dict, fields=None) -> None:
    """ValueError naming the first field (in want's order, or of `fields`) in which the checkpoint's manifest
    `got` differs from the trainer's `want`; a differing configuration names its first differing byte."""
    for k in (fields if fields is not None else want.keys()):
        if k not in got:
            raise ValueError("checkpoint manifest has no field %r" % k)
        a, b = want[k], got[k]
        if isinstance(a, torch.Tensor) or isinstance(b, torch.Tensor):
            a, b = torch.as_tensor(a).reshape(-1), torch.as_tensor(b).reshape(-1)
            if a.numel() != b.numel():
                raise ValueError("checkpoint does not fit: %s has %d bytes, the trainer's %d" % (k, b.numel(), a.numel()))
            d = (a != b).nonzero()
            if d.numel():
                i = int(d[0])
                raise ValueError("checkpoint does not fit: %s byte %d is %d, the trainer's is %d" % (k, i, int(b[i]), int(a[i])))
        elif type(a) is not type(b) or a != b:
            raise ValueError("checkpoint does not fit: %s is %r, the trainer's is %r" % (k, b, a))
    if fields is None:
        extra = [k for k in got if k not in want]
        if extra:
            raise ValueError("checkpoint manifest has an unknown field %r" % extra[0])


def trainer_manifest(tr) -> dict:
    return make_manifest(tr.cfg, tr.arch, tr.E, tr.T, tr.hp, tr.seed, tr.rank, tr.world_size, len(tr.env.parts),
                         tr.free, tr.compact, tr.fused, bool(getattr(tr, "price_unit_major", False)),
                         tr.metric_bufs is not None, tr.ep_len, tr.metric_slots, getattr(tr, "hardcoded", None),
                         action_log_mode(tr), getattr(tr, "auct", None) is not None)


def action_log_mode(tr):
    """The manifest's action_log of a trainer: None (no log), "hist" or "tables"."""
    alog = getattr(tr, "_alog", None)
    return None if alog is None else "tables" if alog.tables else "hist"


# ---- plain-data encoding of the episode log (numpy arrays are not weights_only data)
def _encode(x):
    if isinstance(x, np.ndarray):
        return ("__ndarray__", torch.from_numpy(np.ascontiguousarray(x)))
    if isinstance(x, np.generic):
        return x.item()
    if isinstance(x, dict):
        return {k: _encode(v) for k, v in x.items()}
    if isinstance(x, (list, tuple)):
        return type(x)(_encode(v) for v in x)
    return x


def _decode(x):
    if isinstance(x, tuple) and len(x) == 2 and isinstance(x[0], str) and x[0] == "__ndarray__":
        return x[1].numpy()
    if isinstance(x, dict):
        return {k: _decode(v) for k, v in x.items()}
    if isinstance(x, (list, tuple)):
        return type(x)(_decode(v) for v in x)
    return x


# ---- trainer state
def _net_state(net) -> dict:
    return {k: v.detach().cpu() for k, v in net.state_dict().items()}


def _cpu(x):
    if isinstance(x, torch.Tensor):
        return x.detach().cpu()
    if isinstance(x, dict):
        return {k: _cpu(v) for k, v in x.items()}
    if isinstance(x, (list, tuple)):
        return type(x)(_cpu(v) for v in x)
    return x


def _adam_params(opt):
    return [p for g in opt.param_groups for p in g["params"]]


def save(tr, path: str) -> dict:
    """Trainer.save_checkpoint. Returns where the time went: dict(pack_s, copy_s, write_s, snapshot_bytes,
    file_bytes) (pack: the env snapshots on the device; copy: everything to the host; write: the file)."""
    dev = tr.device
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    snaps = [env.snapshot() for env, _, _ in tr.env.parts]
    torch.cuda.synchronize(dev)
    t1 = time.perf_counter()
    units = {}
    for u in tr.units():
        g = u.group
        st = dict(policy=_net_state(g.policy), policy_old=_net_state(g.policy_old), adam=None, torch_opt=None)
        if g._hip_opt is not None:
            opt = g._hip_opt
            ps = _adam_params(opt)
            # step_dev is the count the Adam kernel reads; the host's step_count is not advanced by graph replays
            st["adam"] = dict(exp_avg=[opt.state[p]["exp_avg"].cpu() for p in ps],
                              exp_avg_sq=[opt.state[p]["exp_avg_sq"].cpu() for p in ps],
                              step_count=int(opt.step_count), step_dev=opt.step_dev.cpu())
        if g._torch_opt is not None:
            st["torch_opt"] = _cpu(g._torch_opt.state_dict())
        units[u.name] = st
    state = dict(units=units, rng=tr.rng.getstate(), rng_ctr=tr.rng_ctr.cpu(), rounds_done=int(tr.rounds_done),
                 iterations=int(tr.iterations), env=[s.cpu() for s in snaps], metric_bufs=None, episode_log=None)
    if tr.metric_bufs is not None:
        state["metric_bufs"] = [b.cpu() for b in tr.metric_bufs]
        state["episode_log"] = _encode(tr.episode_log)
    if action_log_mode(tr):  # the open slots' counters and the episodes read so far (fields only with the log)
        state["action_counters"] = tr._alog.state()
        state["action_log"] = _encode(tr.action_log)
    torch.cuda.synchronize(dev)
    t2 = time.perf_counter()
    write_file(path, trainer_manifest(tr), state)
    t3 = time.perf_counter()
    return dict(pack_s=t1 - t0, copy_s=t2 - t1, write_s=t3 - t2, snapshot_bytes=sum(s.numel() for s in snaps),
                file_bytes=os.path.getsize(path))


def _check_net(name, net, saved: dict):
    own = net.state_dict()
    if own.keys() != saved.keys():
        raise ValueError("checkpoint does not fit: %s has tensors %s, the trainer's %s" % (name, sorted(saved), sorted(own)))
    for k, v in own.items():
        if tuple(v.shape) != tuple(saved[k].shape) or v.dtype != saved[k].dtype:
            raise ValueError("checkpoint does not fit: %s.%s is %s %s, the trainer's %s %s" % (
                name, k, tuple(saved[k].shape), saved[k].dtype, tuple(v.shape), v.dtype))


@torch.no_grad()
def _load_net(net, saved: dict):
    """In place: the captured graphs and the optimizers hold these tensors."""
    own = net.state_dict()
    for k, v in own.items():
        v.copy_(saved[k])


def _check_auctioneer(want: dict, manifest: dict) -> None:
    mine, theirs = bool(want.get("learned_auctioneer")), bool(manifest.get("learned_auctioneer"))
    if mine != theirs:  # (an absent field: the rule-based auctioneer)
        raise ValueError("checkpoint does not fit: learned_auctioneer is %r, the trainer's is %r" % (theirs, mine))


@torch.no_grad()
def load(tr, path: str) -> dict:
    """Trainer.load_checkpoint: the manifest must match (ValueError naming the first differing field, the
    trainer untouched), then every tensor is copied into the trainer's own in place, so a trainer that has
    already run (captured rollout and update graphs) resumes as well as a new one."""
    manifest, state = read_file(path)
    want = trainer_manifest(tr)
    mine, theirs = want.get("hardcoded_agents") or [], manifest.get("hardcoded_agents") or []
    if list(mine) != list(theirs):  # (an absent field: no rule-based agents)
        raise ValueError("checkpoint does not fit: hardcoded_agents is %r, the trainer's is %r" % (theirs, mine))
    mine, theirs = want.get("action_log"), manifest.get("action_log")
    if mine != theirs:  # (an absent field: no action log)
        raise ValueError("checkpoint does not fit: action_log is %r, the trainer's is %r" % (theirs, mine))
    _check_auctioneer(want, manifest)
    compare_manifest(want, manifest)
    units = tr.units()
    if set(state["units"]) != {u.name for u in units} or len(state["env"]) != len(tr.env.parts):
        raise ValueError("checkpoint does not fit: unit types %s, %d env parts" % (sorted(state["units"]), len(state["env"])))
    for u in units:
        st = state["units"][u.name]
        _check_net(u.name + ".policy", u.group.policy, st["policy"])
        _check_net(u.name + ".policy_old", u.group.policy_old, st["policy_old"])
    dev = tr.device
    torch.cuda.synchronize(dev)
    # the envs first: the library validates each snapshot and leaves the env as it was when it refuses one
    for (env, _, _), snap in zip(tr.env.parts, state["env"]):
        env.restore(snap)
    for u in units:
        g, st = u.group, state["units"][u.name]
        _load_net(g.policy, st["policy"])
        _load_net(g.policy_old, st["policy_old"])
        if st["adam"] is not None:
            opt = g.hip_optimizer
            for p, m, v in zip(_adam_params(opt), st["adam"]["exp_avg"], st["adam"]["exp_avg_sq"]):
                opt.state[p]["exp_avg"].copy_(m)
                opt.state[p]["exp_avg_sq"].copy_(v)
            opt.step_dev.copy_(st["adam"]["step_dev"])
            opt.step_count = int(st["adam"]["step_count"])
        elif g._hip_opt is not None:  # saved before its first step
            for s in g._hip_opt.state.values():
                s["exp_avg"].zero_()
                s["exp_avg_sq"].zero_()
            g._hip_opt.step_dev.zero_()
            g._hip_opt.step_count = 0
        if st["torch_opt"] is not None:
            g.optimizer.load_state_dict(st["torch_opt"])
        else:
            g._torch_opt = None  # (created again, with empty state, on first use)
    tr.rng.setstate(_as_random_state(state["rng"]))
    tr.rng_ctr.copy_(state["rng_ctr"])
    tr.rounds_done, tr.iterations = int(state["rounds_done"]), int(state["iterations"])
    if tr.metric_bufs is not None:
        for b, s in zip(tr.metric_bufs, state["metric_bufs"]):
            b.copy_(s)
        tr.episode_log[:] = _decode(state["episode_log"])  # in place: the trainer's EpisodeLog appends to this list
    if action_log_mode(tr):
        tr._alog.load_state(state["action_counters"])
        tr.action_log[:] = _decode(state["action_log"])  # in place: the trainer's ActionLog appends to this list
        tr._actions_logged = tr.rounds_done  # the rings belong to no rollout of this state
    tr._policy_version += 1   # the acting tables are rebuilt from the loaded policy_old
    tr._rings_pending = False  # the rings belong to no rollout of this state
    tr._offers_pending = False
    # ring slot 0: the observation the next rollout acts on, as __init__ emits it (offer rows; a compact rollout
    # compresses them itself)
    for env, e0, e1 in tr.env.parts:
        env.reset(dict(tr._acc_out(0, e0, e1), offer=tr._off_obs[0][e0:e1]))
    torch.cuda.synchronize(dev)
    return manifest


def _as_random_state(s):
    """random.setstate wants tuples (a weights_only load returns them as saved; a list would not do)."""
    return (int(s[0]), tuple(int(x) for x in s[1]), s[2])


POLICY_FIELDS = ("n_agents", "n_cores", "collection_length", "free_prices")


@torch.no_grad()
def load_policy(tr, path: str) -> dict:
    """Trainer.load_policy: the nets only (policy and policy_old of every unit type), from a checkpoint made
    with any E, T, seed or world size; the configuration's shape terms (agents, cores, collection length, price
    mode and the nets' dimensions they and the job priorities give), arch and free must be the trainer's. For evaluate() on a saved policy."""
    manifest, state = read_file(path)
    _check_auctioneer(trainer_manifest(tr), manifest)
    compare_manifest(trainer_manifest(tr), manifest, fields=("format", "arch", "free"))
    theirs = config_of(manifest["config"])
    for f in POLICY_FIELDS:
        if getattr(theirs, f) != getattr(tr.cfg, f):
            raise ValueError("checkpoint does not fit: config.%s is %r, the trainer's is %r" % (f, getattr(theirs, f), getattr(tr.cfg, f)))
    a, b = abi.config_shape(theirs), abi.config_shape(tr.cfg)
    for k in b:
        if a[k] != b[k]:
            raise ValueError("checkpoint does not fit: shape term %s is %r, the trainer's is %r" % (k, a[k], b[k]))
    units = tr.units()
    if set(state["units"]) != {u.name for u in units}:
        raise ValueError("checkpoint does not fit: unit types %s" % sorted(state["units"]))
    for u in units:
        st = state["units"][u.name]
        _check_net(u.name + ".policy", u.group.policy, st["policy"])
        _check_net(u.name + ".policy_old", u.group.policy_old, st["policy_old"])
    for u in units:
        st = state["units"][u.name]
        _load_net(u.group.policy, st["policy"])
        _load_net(u.group.policy_old, st["policy_old"])
    tr._policy_version += 1
    torch.cuda.synchronize(tr.device)
    return manifest
