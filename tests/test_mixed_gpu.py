"""Mixed populations (ms_env_step_mixed, BatchedEnv.step_mixed, Trainer.evaluate(hardcoded_agents=...)): the
agents of a 64-bit mask play DividedHardcodedAgent.getActions inside the env kernel, the others the caller's
rows. Bit-exact against the object-faithful restatement (oracle/pyref.py) with the masked getActions loop
restated here, against the all-agents hard-coded mode and against the plain step."""
import ctypes as ct

import numpy as np
import pytest
import torch

from oracle import pyref
from tests.drivers import compare_state, offer_counts_from_obs, random_actions
from tests.test_hardcoded_gpu import CASES, _pcfg, _pyref_export

pytestmark = pytest.mark.gpu

E, T = 4, 120
_SMALL_JOBS = dict(priorities=[4, 8], lengths=[4, 8], fix_prices=[2, 4], probabilities=[0.5, 0.5])
SHAPES = {
    "ties": CASES["ties"],
    "cfg2": None,
    "cfg3_fixed": CASES["cfg3_fixed"],
    "n17": dict(n_agents=17, n_cores=3, collection_length=2, **_SMALL_JOBS),
    "n34": dict(n_agents=34, n_cores=3, collection_length=2, **_SMALL_JOBS),
    "n64": dict(n_agents=64, n_cores=2, collection_length=1, **_SMALL_JOBS),
}
# every lane-group width (16, 32 and 64 lanes per replica) and the mask bits 31, 32, 33 and 63
MIXED = [
    ("ties", 0b010), ("ties", 0b101),
    ("cfg2", 0b0001), ("cfg2", 0b1010),
    ("cfg3_fixed", 0b10000001), ("cfg3_fixed", 0b01111110),
    ("n17", 1 << 16 | 1 << 8), ("n17", 0xFFFF),
    ("n34", 1 << 33 | 1 << 31 | 1), ("n34", ((1 << 34) - 1) & ~(1 << 32)),
    ("n64", 1 << 63 | 1), ("n64", (1 << 63) - 1),
]


def _config(abi, name):
    kw = SHAPES[name]
    return (abi.named_config(name) if kw is None else abi.make_config(**kw)), kw


def masked_hardcoded_actions(w, mask, acc_act, off_act):
    """PyWorld.hardcoded_agent_actions restricted to the agents of `mask` (DividedHardcodedAgent.getActions,
    Agent.py:630-641, asked in index order by SchedulingEnvironment.py:150-172): per masked agent its
    HardcodedOfferers (HardcodedModules.py:81-109), then its HardcodedAcceptors (:16-45), every tie-break a
    random.sample on the world's stream; an agent outside the mask draws nothing. Overwrites the masked
    agents' rows of acc_act [N][C] and off_act [N][L]."""
    for a in range(w.N):
        if not (mask >> a) & 1:
            continue
        for s in range(w.L):
            row = w.offer_obs(a, s)
            ratios = [pyref.ratio(row[2 * c], row[2 * c + 1]) for c in range(w.C)]
            cands = [(i, r) for i, r in enumerate(ratios) if r == min(ratios)]
            off_act[a][s] = w.rng.sample(cands, 1)[0][0]
        for c in range(w.C):
            row = w.acceptor_obs(a, c)
            acc_act[a][c] = w.O
            if row[0] == 0:
                continue
            offered = [pyref.ratio(row[3 + 2 * k], row[4 + 2 * k]) for k in range(w.O)]
            best = max(offered)
            if best > pyref.ratio(row[1], row[2]):
                cands = [(i, r) for i, r in enumerate(offered) if r == best]
                acc_act[a][c] = w.rng.sample(cands, 1)[0][0]


class Restatement:
    """The E restated worlds of one mixed case (seeds 21 + e), the unmasked agents driven by random_actions
    with np.random.default_rng(100 + e) on the world's own observation counts."""

    def __init__(self, abi, name, mask):
        cfg, kw = _config(abi, name)
        self.mask = mask
        self.worlds = [pyref.PyWorld(_pcfg(abi, cfg, kw), 21 + e) for e in range(E)]
        self.rngs = [np.random.default_rng(100 + e) for e in range(E)]
        self.nonreject = self.executed = 0

    def round(self):
        """One round of every world: (supplied acceptor, supplied offer, taken acceptor, taken offer) int arrays
        [E][N][C] / [E][N][L] and the per-world step results."""
        sup_a, sup_o, tak_a, tak_o, results = [], [], [], [], []
        for w, rng in zip(self.worlds, self.rngs):
            acc_obs = np.array([[w.acceptor_obs(a, c) for c in range(w.C)] for a in range(w.N)])
            acc, off, _ = random_actions(rng, offer_counts_from_obs(acc_obs, w.O), w.N, w.C, w.L, w.O, False, 0,
                                         accept_bias=0.7)
            sup_a.append(acc.copy())
            sup_o.append(off.copy())
            masked_hardcoded_actions(w, self.mask, acc, off)
            tak_a.append(acc)
            tak_o.append(off)
            results.append(w.step(acc.tolist(), off.tolist()))
            self.executed += len(w.accepted)
            self.nonreject += sum(int(acc[a][c] != w.O) for a in range(w.N) if (self.mask >> a) & 1
                                  for c in range(w.C))
        return np.stack(sup_a), np.stack(sup_o), np.stack(tak_a), np.stack(tak_o), results


def _i8(x, dev):
    return torch.tensor(np.asarray(x), dtype=torch.int8, device=dev)


def _state_equal(a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert np.array_equal(a[k], b[k]), k


def _outputs_equal(o1, r1, o2, r2, what):
    for k in o1:
        assert torch.equal(o1[k], o2[k]), ("obs " + k,) + what
    for k in r1:
        if r1[k] is not None:
            assert torch.equal(r1[k], r2[k]), ("reward " + k,) + what


@pytest.mark.parametrize("name", ["cfg2", "ties"])
def test_full_mask_is_hardcoded_mode(ms, name):
    """Every bit set, the supplied rows all 127 (out of range): the round of step(None, None), bit for bit."""
    cfg, _ = _config(ms.abi, name)
    a, b = ms.BatchedEnv(cfg, E, seed=21), ms.BatchedEnv(cfg, E, seed=21)
    N, C, L = a.N, a.C, a.L
    bad_acc = torch.full((E, N, C), 127, dtype=torch.int8, device=a.device)
    bad_off = torch.full((E, N, L), 127, dtype=torch.int8, device=a.device)
    oa, ob = a.obs_buffers(auctioneer=True), b.obs_buffers(auctioneer=True)
    for t in range(T):
        _, ra, _ = a.step_mixed(bad_acc, bad_off, (1 << N) - 1, obs=oa)
        _, rb, _ = b.step(None, None, obs=ob)
        _outputs_equal(oa, ra, ob, rb, (name, t))
    _state_equal(a.export_state(), b.export_state())
    assert a.flags() == 0 and b.flags() == 0 and a.round == b.round == T


@pytest.mark.parametrize("name", ["cfg2", "ties"])
def test_mask_zero_is_step(ms, name):
    """Mask 0: the same random actions through step and step_mixed; the taken arrays are the supplied ones."""
    cfg, _ = _config(ms.abi, name)
    a, b = ms.BatchedEnv(cfg, E, seed=21), ms.BatchedEnv(cfg, E, seed=21)
    N, C, L, O, dev = a.N, a.C, a.L, a.O, a.device
    oa, ob = a.obs_buffers(auctioneer=True), b.obs_buffers(auctioneer=True)
    a.reset(oa)
    b.reset(ob)
    taken = dict(acceptor=torch.full((E, N, C), -1, dtype=torch.int8, device=dev),
                 offer_core=torch.full((E, N, L), -1, dtype=torch.int8, device=dev))
    rng = np.random.default_rng(7)
    executed = 0
    for t in range(T):
        counts = offer_counts_from_obs(ob["acceptor"].cpu().numpy(), O)
        acts = [random_actions(rng, counts[e], N, C, L, O, False, 0, accept_bias=0.7) for e in range(E)]
        acc, off = _i8([x[0] for x in acts], dev), _i8([x[1] for x in acts], dev)
        _, ra, _ = a.step_mixed(acc, off, 0, obs=oa, taken=taken)
        _, rb, _ = b.step(acc, off, obs=ob)
        _outputs_equal(oa, ra, ob, rb, (name, t))
        assert torch.equal(taken["acceptor"], acc) and torch.equal(taken["offer_core"], off)
        executed += int((rb["offer"] != 0).sum())
    _state_equal(a.export_state(), b.export_state())
    assert a.flags() == 0 and b.flags() == 0 and executed > 0


@pytest.mark.parametrize("name,mask", MIXED, ids=["%s-%x" % c for c in MIXED])
def test_mixed_against_restatement(ms, name, mask):
    """Every round: the taken arrays, the observations and the acceptor / agent / auctioneer rewards against the
    restatement; the state every 60 rounds. On the restatement alone the cases (in MIXED's order) see 20, 5, 84,
    74, 148, 165, 48, 16, 32, 9, 16, 7 non-reject acceptor actions of masked agents and at least 189 executed
    offers, so the closing conditions hold with room."""
    abi = ms.abi
    cfg, _ = _config(abi, name)
    s = abi.config_shape(cfg)
    ref = Restatement(abi, name, mask)
    genv = ms.BatchedEnv(cfg, E, seed=21)
    N, C, L, dev = genv.N, genv.C, genv.L, genv.device
    obs = genv.obs_buffers()
    taken = dict(acceptor=torch.empty((E, N, C), dtype=torch.int8, device=dev),
                 offer_core=torch.empty((E, N, L), dtype=torch.int8, device=dev))
    masked = [a for a in range(N) if (mask >> a) & 1]
    for t in range(T):
        sup_a, sup_o, tak_a, tak_o, results = ref.round()
        sup_a[:, masked], sup_o[:, masked] = 127, -128  # a masked agent's rows are ignored whatever they hold
        _, rew, _ = genv.step_mixed(_i8(sup_a, dev), _i8(sup_o, dev), mask, obs=obs, taken=taken)
        np.testing.assert_array_equal(taken["acceptor"].cpu().numpy(), tak_a, err_msg="acceptor taken t=%d" % t)
        np.testing.assert_array_equal(taken["offer_core"].cpu().numpy(), tak_o, err_msg="offer taken t=%d" % t)
        ga, go = obs["acceptor"].cpu().numpy(), obs["offer"].cpu().numpy()
        gr = {k: rew[k].cpu().numpy() for k in ("acceptor", "agent", "auctioneer")}
        for e, ((r_acc, r_off, _), r, _, _) in enumerate(results):
            assert np.array_equal(ga[e, :, :, : s["acc_obs_dim"]], np.array(r_acc)), (t, e)
            assert np.array_equal(go[e, :, :, : s["off_obs_dim"]], np.array(r_off)), (t, e)
            np.testing.assert_array_equal(gr["acceptor"][e], r[1][..., 0], err_msg="t=%d e=%d" % (t, e))
            np.testing.assert_array_equal(gr["auctioneer"][e], r[2], err_msg="t=%d e=%d" % (t, e))
            np.testing.assert_array_equal(gr["agent"][e], r[3], err_msg="t=%d e=%d" % (t, e))
        if t % 60 == 0 or t == T - 1:
            compare_state(genv.export_state(), [_pyref_export(w) for w in ref.worlds], E)
    assert genv.flags() == 0
    # not vacuous: the masked agents accepted offers by their rule, and offers executed
    assert ref.nonreject >= 1 and ref.executed >= 1, (ref.nonreject, ref.executed)


def test_abi_refusals(ms):
    """MS_EINVAL (22) with nothing launched: a free-price env, a mask bit at n_agents, no acceptor actions."""
    abi, lib = ms.abi, ms._lib.lib
    for name, mask, with_acc in (("cfg3", 1, True), ("cfg2", None, True), ("cfg2", 1, False)):
        env = ms.BatchedEnv(abi.named_config(name), E, seed=21)
        N, C, L, dev = env.N, env.C, env.L, env.device
        acc = torch.full((E, N, C), env.O, dtype=torch.int8, device=dev)
        off = torch.zeros((E, N, L), dtype=torch.int8, device=dev)
        price = torch.zeros((E, N, L), dtype=torch.int8, device=dev)
        env.step(acc, off, price if env.free_prices else None)
        before = env.export_state()
        a = abi.MsActions(ms._lib.ptr(acc) if with_acc else None, ms._lib.ptr(off),
                          ms._lib.ptr(price) if env.free_prices else None, None)
        mix = abi.MsMixed(1 << N if mask is None else mask, None, None)
        rc = lib.ms_env_step_mixed(env._h, ct.byref(a), ct.byref(mix), None, None, None, ms._lib.stream_ptr())
        assert rc == abi.EINVAL == 22 and lib.ms_last_error(), (name, mask, with_acc)
        assert env.round == 1
        _state_equal(env.export_state(), before)
    env = ms.BatchedEnv(abi.named_config("cfg2"), E, seed=21)
    rc = lib.ms_env_step_mixed(env._h, ct.byref(a), None, None, None, None, ms._lib.stream_ptr())
    assert rc == 22 and env.round == 0
    # the Python layer: ValueError for a free-price env and for agents outside [0, N)
    with pytest.raises(ValueError):
        env.step_mixed(acc, off, [env.N])
    with pytest.raises(ValueError):
        env.step_mixed(acc, off, 1 << env.N)
    with pytest.raises(ValueError):
        env.step_mixed(acc, off, [-1])
    free = ms.BatchedEnv(abi.named_config("cfg3"), E, seed=21)
    with pytest.raises(ValueError):
        free.step_mixed(None, None, [0])
    assert env.round == 0 and free.round == 0


# ---- Trainer.evaluate(hardcoded_agents=...)

def _ev():
    from tests import test_evaluate_gpu as ev
    return ev


@pytest.mark.parametrize("name", ["cfg2", "cfg1"])
def test_evaluate_mixed(ms, name):
    ev = _ev()
    mx = ev._mods()[2]
    t = ev._trainer(name)
    N, C, L, EE, EP = t.N, t.C, t.L, ev.E, ev.EP
    seed = 77
    # every agent hard-coded: the hard-coded mode's market
    full = t.evaluate(episodes=2, mode="greedy", seed=seed, hardcoded_agents=range(N))
    base = t.evaluate(episodes=2, mode="hardcoded", seed=seed)
    assert ev._same(full["per_replica"], base["per_replica"]) and full["hardcoded_agents"] == list(range(N))
    assert all(e["agentRew_learned"] is None for e in full["episodes"])
    assert "hardcoded_agents" not in base and "agentRew_hardcoded" not in base["episodes"][0]
    # no agent hard-coded: the plain greedy call
    plain = t.evaluate(episodes=2, mode="greedy", seed=seed, trace=True)
    none = t.evaluate(episodes=2, mode="greedy", seed=seed, hardcoded_agents=[])
    assert ev._same(none["per_replica"], plain["per_replica"]) and none["hardcoded_agents"] == []
    for got, want in zip(none["episodes"], plain["episodes"]):
        assert ev._same({k: got[k] for k in want}, want)
        assert got["agentRew_hardcoded"] is None and got["agentRew_learned"] == float(np.mean(want["agentRew"]))
    # one rule-based entrant in the learned market
    res = t.evaluate(episodes=2, mode="greedy", seed=seed, trace=True, hardcoded_agents=[1])
    assert t.eval_env.flags() == 0 and res["hardcoded_agents"] == [1]
    trace = res["trace"]
    assert len(trace) == 2 * EP
    # round 0: both runs act on the same observations, so the learned agents' rows are the nets' greedy picks
    r0, p0 = trace[0], plain["trace"][0]
    assert torch.equal(r0["offer"], p0["offer"])
    learned = [a for a in range(N) if a != 1]
    assert torch.equal(r0["acceptor_action"].view(EE, N, C)[:, learned], p0["acceptor_action"].view(EE, N, C)[:, learned])
    assert torch.equal(r0["offer_action"].view(EE, N, L)[:, learned], p0["offer_action"].view(EE, N, L)[:, learned])
    # The traced (taken) actions replayed through step on a fresh env of that seed reproduce the metrics. The
    # rule's tie-breaks are draws on the env's own stream (before the auctioneer's and the spawn's), which step
    # does not make for supplied actions: the replay makes them with ms_env_randbelow first, their sizes taken
    # from the restatement stepped beside it, whose rule must also pick the traced rows of agent 1.
    env = ms.BatchedEnv(t.cfg, EE, seed=seed)
    mbuf = env.metrics_buffer(2)
    obs = env.compact_obs_buffers() if t.compact else env.obs_buffers()
    env.reset(obs)
    worlds = [pyref.PyWorld(_pcfg(ms.abi, t.cfg, None), seed + e) for e in range(EE)]
    draws = []
    for w in worlds:
        w.rng.sample = lambda pop, k, _sample=w.rng.sample: (draws.append(len(pop)), _sample(pop, k))[1]
    for r in trace:
        assert torch.equal(obs["offer"].cpu().view(r["offer"].shape), r["offer"])
        acc, off = r["acceptor_action"].view(EE, N, C).numpy(), r["offer_action"].view(EE, N, L).numpy()
        for e, w in enumerate(worlds):
            rule_acc, rule_off = acc[e].astype(int), off[e].astype(int)
            rule_acc[1], rule_off[1] = -1, -1
            del draws[:]
            masked_hardcoded_actions(w, 0b10, rule_acc, rule_off)
            assert np.array_equal(rule_acc, acc[e]) and np.array_equal(rule_off, off[e])
            assert len(draws) >= L
            for n in draws:
                env.randbelow(n, e)
        env.step(r["acceptor_action"].cuda().view(EE, N, C), r["offer_action"].cuda().view(EE, N, L), obs=obs,
                 events=dict(metrics=mbuf))
        for e, w in enumerate(worlds):
            w.step(acc[e].tolist(), off[e].tolist())
    raw = mbuf.cpu().numpy()
    replay = [mx.episode_values(mx.view(raw[k]), t.cfg, EP, N, C, L) for k in range(2)]
    assert ev._same(replay, res["per_replica"]) and env.flags() == 0
    for epi, per in zip(res["episodes"], res["per_replica"]):
        rew = np.mean(np.stack([d["agentRew"] for d in per]), axis=0)
        assert np.array_equal(epi["agentRew"], rew)
        assert epi["agentRew_hardcoded"] == float(rew[1])
        assert epi["agentRew_learned"] == float(np.mean(rew[learned]))
    # the rule-based entrant changes the market
    assert not ev._same(res["per_replica"], plain["per_replica"])


def test_evaluate_mixed_refusals(ms):
    ev = _ev()
    t = ev._trainer("cfg2")
    with pytest.raises(ValueError):
        t.evaluate(mode="hardcoded", hardcoded_agents=[0])
    with pytest.raises(ValueError):
        t.evaluate(mode="greedy", hardcoded_agents=[t.N])
    with pytest.raises(ValueError):
        t.evaluate(mode="greedy", hardcoded_agents=[-1])
    with pytest.raises(ValueError):  # (a bool is no agent index, as in Trainer(hardcoded_agents=...))
        t.evaluate(mode="greedy", hardcoded_agents=[True])
    with pytest.raises(ValueError):
        ev._trainer("cfg3").evaluate(mode="greedy", hardcoded_agents=[0])


@pytest.mark.parametrize("mode", ["greedy", "sample"])
def test_evaluate_mixed_leaves_training_untouched(ms, mode):
    ev = _ev()
    t = ev._trainer("cfg2")
    l1 = t.iteration()
    version, acting = t._policy_version, t._acting_version
    res = t.evaluate(episodes=1, mode=mode, hardcoded_agents=[0, 2])
    assert len(res["episodes"]) == 1 and t.eval_env.flags() == 0
    assert (t._policy_version, t._acting_version) == (version, acting)
    l2 = t.iteration()
    got, want = ev._training_state(t, [l1, l2]), ev._plain_run("cfg2")
    assert got.keys() == want.keys()
    for k in want:
        assert ev._same(got[k], want[k]), k
