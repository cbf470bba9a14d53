"""Trainer(action_log=..., action_tables=...) and evaluate(action_log=...): every entry of the log against a numpy
recount of the rings (integers: exact equality). A trainer with the log runs iteration(); its twin without the log
(same seed) is driven by rollout() / update() and its completed rings are copied to the host after every rollout:
the two train bit-identically, so the twin's rings are what the logging trainer's launches read.

update_step 6 and episode_length 4: an episode straddles two iterations, a rollout touches two or three episodes."""
import contextlib
import importlib
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

T, EP, ITERS = 6, 4, 4
ENVS = dict(cfg1=20, cfg2=70, cfg3=72)


def _mod(name):
    return importlib.import_module("marl-scheduling_amd." + name)


def _trainer(name, E=None, seed=3, **kw):
    return _mod("trainer").Trainer.from_named(name, n_envs=E or ENVS[name], update_step=T, seed=seed, device="cuda:0",
                                              episode_length=EP, **kw)


@contextlib.contextmanager
def _environ(**kv):
    old = {k: os.environ.get(k) for k in kv}
    os.environ.update(kv)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _rings(t):
    """The completed rings of the last rollout, on the host."""
    C = t.C
    r = dict(offer=t.off.actions, acceptor=t.acc.actions, offer_key=t.off_obs[:t.T, :, :, 2 * C])
    if t.compact:
        r["owner"] = t.acc_owner[:t.T]
    if t.free:
        r.update(price=t.price.actions, price_key=t.price_obs[:, :, :, 2])
    return {k: v.cpu().numpy().astype(np.int64) for k, v in r.items()}


class Recount:
    """The action log in numpy: rounds are added in order, episode r // ep_len."""

    def __init__(self, t, ep_len):
        s = t.env.shape
        self.N, self.C, self.L, self.ep_len, self.free = t.N, t.C, t.L, ep_len, t.free
        self.P = max(t.cfg.job_priority[: t.cfg.n_kinds]) + 1
        self.A = dict(offer=s.off_actions, price=s.price_actions, acceptor=s.acc_actions)
        self.rounds, self.eps = 0, []

    def _ep(self):
        N, C, L, P, A = self.N, self.C, self.L, self.P, self.A
        z = lambda *shape: np.zeros(shape, dtype=np.int64)
        ep = dict(offer=z(N * L, A["offer"]), acceptor=z(N * C, A["acceptor"]), bad=0,
                  offer_by_priority=z(N, P, A["offer"]), skipped=dict(offer=0))
        if self.free:
            ep.update(price=z(N * L, A["price"]), price_by_priority=z(N, P, A["price"]))
            ep["skipped"]["price"] = 0
            # (not in the log) offers made for a slot without a job: gate != 0, the state's priority byte -1 / -2
            ep["_jobless"], ep["_gate0"] = z(N, A["price"]), 0
        return ep

    def add(self, r):
        """r: arrays [T][E][..] (offer, acceptor, owner or absent, offer_key, price, price_key)."""
        N, C, L, P = self.N, self.C, self.L, self.P
        for t in range(r["offer"].shape[0]):
            e_i = self.rounds // self.ep_len
            while len(self.eps) <= e_i:
                self.eps.append(self._ep())
            ep = self.eps[e_i]
            off, acc = r["offer"][t], r["acceptor"][t]
            unit = np.broadcast_to(np.arange(N * L), off.shape)
            np.add.at(ep["offer"], (unit, off), 1)
            if "owner" in r:
                o = r["owner"][t]
                e, c = np.nonzero(o > 0)
                u = (o[e, c] - 1) * C + c
                np.add.at(ep["acceptor"], (u, acc[e, u]), 1)
            else:
                np.add.at(ep["acceptor"], (np.broadcast_to(np.arange(N * C), acc.shape), acc), 1)
            tables = [("offer", off, r["offer_key"][t])]
            if self.free:
                gate = off != 0
                np.add.at(ep["price"], (unit[gate], r["price"][t][gate]), 1)
                tables.append(("price", r["price"][t], r["price_key"][t]))
                jobless = gate & ((r["price_key"][t] < 0) | (r["price_key"][t] >= P))
                np.add.at(ep["_jobless"], ((unit // L)[jobless], r["price"][t][jobless]), 1)
                ep["_gate0"] += int((~gate).sum())
            for name, a, k in tables:
                ok = (k >= 0) & (k < P)
                np.add.at(ep[name + "_by_priority"], ((unit // L)[ok], k[ok], a[ok]), 1)
                ep["skipped"][name] += int((~ok).sum())
            self.rounds += 1

    def log(self, tables=True):
        N, C, L = self.N, self.C, self.L
        out = []
        for ep in self.eps[: self.rounds // self.ep_len]:
            d = dict(offer=ep["offer"].reshape(N, L, -1), acceptor=ep["acceptor"].reshape(N, C, -1), bad=0)
            if self.free:
                d["price"] = ep["price"].reshape(N, L, -1)
            if tables:
                d.update({k: v for k, v in ep.items() if k.endswith("_by_priority")}, skipped=dict(ep["skipped"]))
            out.append(d)
        return out


def _equal(a, b):
    return _mod("action_log").equal_logs(a, b)


def _params(t):
    out = {}
    for u in t.units():
        g = u.group
        for pol_name, pol in (("policy", g.policy), ("policy_old", g.policy_old)):
            for k, p in pol.named_parameters():
                out["%s.%s.%s" % (u.name, pol_name, k)] = p.detach().clone()
        opt = g.hip_optimizer
        for i, p in enumerate(q for grp in opt.param_groups for q in grp["params"]):
            out["%s.adam%d.m" % (u.name, i)] = opt.state[p]["exp_avg"].clone()
            out["%s.adam%d.v" % (u.name, i)] = opt.state[p]["exp_avg_sq"].clone()
        out[u.name + ".adam.step"] = opt.step_dev.clone()
    return out


def _run_pair(name):
    """(the logging trainer after ITERS iterations, its losses, the twin, its losses, the twin's recount)."""
    name, kw = (name[:4], dict(rollout_streams=2)) if name.endswith("-2parts") else (name, {})
    a = _trainer(name, metrics=True, action_log=True, action_tables=True, **kw)
    b = _trainer(name, **kw)
    rc = Recount(b, EP)
    la, lb = [], []
    for _ in range(ITERS):
        la.append(a.iteration())
        assert len(a.action_log) == len(a.episode_log) == a.rounds_done // EP
        b.rollout()
        rc.add(_rings(b))
        b.log_actions()  # (no log: nothing happens)
        lb.append(b.update())
    return a, la, b, lb, rc


_PAIRS = {}


@pytest.fixture(scope="module")
def pairs():
    def get(name):
        if name not in _PAIRS:
            _PAIRS[name] = _run_pair(name)
        return _PAIRS[name]
    yield get
    _PAIRS.clear()


@pytest.mark.parametrize("name", ["cfg2", "cfg3", "cfg1", "cfg3-2parts"])
def test_log_equals_recount_of_the_rings(ms, pairs, name):
    a, _, b, _, rc = pairs(name)
    if name == "cfg3-2parts":  # two replica parts share the rings; no regenerating gradient, the rings are complete
        assert len(a.env.parts) == 2 and a.fused_rollout_free and not a.acc_regen
    want = rc.log()
    assert len(a.action_log) == len(want) == ITERS * T // EP == 6
    assert a.action_log_info["acceptor_selection"] == ("owner" if a.compact else "all")
    assert a.compact == (name != "cfg1")
    if name == "cfg3":  # the path iteration() leaves the rings in: owners' items by core, compact offers
        assert a.fused_rollout_free and a.acc_regen and a.off_compact and a.acc_own is not None
    for i, (got, ref) in enumerate(zip(a.action_log, want)):
        assert got.keys() == ref.keys(), i
        for k in ref:
            assert _equal([{k: got[k]}], [{k: ref[k]}]), (i, k)
        n_el = EP * a.E * a.N * a.L
        assert got["offer"].sum() == n_el and got["offer"].dtype == np.int64
        assert got["offer_by_priority"].sum() + got["skipped"]["offer"] == n_el
        if a.free:
            # the table against the gated histogram: the prices asked for a job, summed over the priorities, and
            # the prices of offers for a slot without a job (gate != 0, but the state's priority byte is the empty
            # or pad slot's -1 / -2, which key_min = 0 skips) are the agent's gated prices; the skipped elements are
            # the gate-0 ones (the dummy state) and those. Where no offer is made for a jobless slot this is
            # price_by_priority.sum(keys) == price.sum(slots) and skipped == the gate-0 elements; these untrained
            # nets make about every second offer for a jobless slot (episode 0, agent 0, price 0: 33 of 66)
            jobless, gate0 = rc.eps[i]["_jobless"], rc.eps[i]["_gate0"]
            print("episode %d: gated prices %d, keyed by a priority %d, jobless %d, gate 0 %d, skipped %d" % (
                i, got["price"].sum(), got["price_by_priority"].sum(), jobless.sum(), gate0, got["skipped"]["price"]))
            assert np.array_equal(got["price_by_priority"].sum(axis=1) + jobless, got["price"].sum(axis=1)), i
            assert gate0 == n_el - got["price"].sum() == got["offer"][:, :, 0].sum(), i
            assert got["skipped"]["price"] == gate0 + jobless.sum(), i


@pytest.mark.parametrize("name", ["cfg2", "cfg3"])
def test_training_is_bit_identical_with_the_log_on(ms, pairs, name):
    a, la, b, lb, _ = pairs(name)
    pa, pb = _params(a), _params(b)
    assert pa.keys() == pb.keys()
    for k in pa:
        assert torch.equal(pa[k], pb[k]), k
    for x, y in zip(la, lb):
        assert x.keys() == y.keys()
        for k in x:
            assert torch.equal(x[k], y[k]), k


def test_off_is_off(ms, pairs):
    _, _, b, _, _ = pairs("cfg3")
    assert b.action_log == [] and b._alog is None and not hasattr(b, "action_log_info")
    assert not any(isinstance(v, torch.Tensor) and v.dtype == torch.int64 and v.dim() >= 3 for v in vars(b).values())
    done = b.rounds_done
    assert b.log_actions() is None and b.action_log == [] and b.rounds_done == done
    with pytest.raises(ValueError, match="action_log"):
        _trainer("cfg3", action_tables=True)


@pytest.mark.parametrize("env", [dict(MS_OFF_COMPACT="0"), dict(MS_FILL_OWN="0")], ids=["rows", "ring-items"])
def test_other_ring_layouts_give_the_same_log(ms, pairs, env):
    a = pairs("cfg3")[0]
    with _environ(**env):
        v = _trainer("cfg3", action_log=True, action_tables=True)
    assert v.off_compact == ("MS_OFF_COMPACT" not in env) and (v.acc_own is None) == ("MS_FILL_OWN" in env)
    for _ in range(ITERS):
        v.iteration()
    assert _equal(v.action_log, a.action_log)


def test_args_dict_gains_experiment_3s_keys(ms, pairs):
    a, _, b, _, _ = pairs("cfg3")
    mx = _mod("metrics")
    d, keys = a.args_dict(), [str(s) for s in range(a.L)]
    want = mx.action_args(a.action_log)
    assert sorted(want) == sorted(keys) and all(d[k] == want[k] and len(d[k]) == len(a.action_log) for k in keys)
    plain = _trainer("cfg3", E=8, metrics=True)
    assert not any(k in plain.args_dict() for k in keys)
    assert set(d) - set(keys) == set(plain.args_dict())


def _recount_trace(t, res, hc=False):
    rc = Recount(t, EP)
    for rec in res["trace"]:
        r = dict(offer=rec["offer_action"], acceptor=rec["acceptor_action"], offer_key=rec["offer"][:, :, 2 * t.C])
        if t.compact:
            r["owner"] = rec["core_owner"]
        if t.free:
            r.update(price=rec["price_action"], price_key=rec["price_state"][:, :, 2])
        rc.add({k: v.numpy().astype(np.int64)[None] for k, v in r.items()})
    return rc


@pytest.mark.parametrize("name,mode", [("cfg3", "greedy"), ("cfg3", "sample"), ("cfg2", "sample"), ("cfg1", "greedy")])
def test_evaluate_log_equals_recount_of_the_trace(ms, pairs, name, mode):
    a = pairs(name)[0]
    before = (a.action_log[:], a._alog.state(), _params(a), a.rounds_done)
    res = a.evaluate(episodes=2, n_envs=37, mode=mode, trace=True, action_log=True, action_tables=True)
    assert len(res["action_log"]) == 2 and _equal(res["action_log"], _recount_trace(a, res).log())
    hist = a.evaluate(episodes=2, n_envs=37, mode=mode, action_log=True)
    assert set(hist["action_log"][0]) == {"offer", "acceptor", "bad"} | ({"price"} if a.free else set())
    assert _equal(hist["action_log"], _recount_trace(a, res).log(tables=False))
    plain = a.evaluate(episodes=2, n_envs=37, mode=mode)
    assert set(plain) == {"mode", "seed", "n_envs", "episodes", "per_replica"}
    assert repr(plain["episodes"]) == repr(res["episodes"])  # counting changes no evaluation
    # the training log and the training state are as they were
    assert _equal(a.action_log, before[0]) and a.rounds_done == before[3]
    after = a._alog.state()
    assert all(torch.equal(after["counts"][k], v) for k, v in before[1]["counts"].items())
    assert all(torch.equal(v, before[2][k]) for k, v in _params(a).items())


def test_evaluate_with_hardcoded_agents_counts_the_rules_picks(ms, pairs):
    a = pairs("cfg2")[0]
    res = a.evaluate(episodes=2, n_envs=37, mode="greedy", trace=True, hardcoded_agents=[0], action_log=True,
                     action_tables=True)
    assert _equal(res["action_log"], _recount_trace(a, res).log())  # the trace holds the actions the rounds used
    nets = a.evaluate(episodes=2, n_envs=37, mode="greedy", action_log=True, action_tables=True)
    assert not np.array_equal(res["action_log"][0]["offer"][0], nets["action_log"][0]["offer"][0])
    with pytest.raises(ValueError, match="action_log"):
        a.evaluate(mode="hardcoded", action_log=True)
    with pytest.raises(ValueError, match="action_log"):
        a.evaluate(action_tables=True)


def test_checkpoint_resume_and_refusals(ms, tmp_path):
    path, plain_path = str(tmp_path / "log.ckpt"), str(tmp_path / "plain.ckpt")
    kw = dict(metrics=True, action_log=True, action_tables=True)
    a = _trainer("cfg3", **kw)
    a.iteration()
    assert a.rounds_done % EP != 0  # saved mid-episode: the open slot's counters travel
    a.save_checkpoint(path)
    ck = _mod("checkpoint")
    assert ck.read_file(path)[0]["action_log"] == "tables"
    for _ in range(2):
        a.iteration()
    c = _trainer("cfg3", **kw)
    c.load_checkpoint(path)
    for _ in range(2):
        c.iteration()
    assert len(a.action_log) == 3 * T // EP and _equal(c.action_log, a.action_log)
    plain = _trainer("cfg3", metrics=True)
    plain.iteration()
    plain.save_checkpoint(plain_path)
    assert "action_log" not in ck.read_file(plain_path)[0]
    hist = _trainer("cfg3", metrics=True, action_log=True)
    for t, p in ((plain, path), (c, plain_path), (hist, path)):
        with pytest.raises(ValueError, match="action_log"):
            t.load_checkpoint(p)
    plain.load_policy(path)
    c.load_policy(plain_path)
