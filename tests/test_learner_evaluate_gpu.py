"""evaluate() of AggregatedTrainer and DQNTrainer: the rule-based baseline on the same job streams as
Trainer.evaluate, the greedy evaluation against a replay of its recorded actions and (aggregated) a float64
restatement of the nets on the recorded observations, repeatability, training left exactly as it was, and the
argument checks."""
import importlib

import pytest
import torch

from tests.learner_replay import AGGREGATED_KEYS, FIXED, assert_episodes_match, record_class, replay
from tests.test_evaluate_gpu import _same
from tests.test_greedy_gpu import _logits, check_greedy_rows

pytestmark = pytest.mark.gpu

E, T, EP = 4, 15, 10  # replicas, update_step, episode_length
KEYS = ("w1", "b1", "w2", "b2", "w3", "b3")


def _mod(name):
    return importlib.import_module("marl-scheduling_amd." + name)


def _cfg(ms):
    return ms.abi.make_config(episode_length=EP, **FIXED)


def _aggregated(ms, fully=False, seed=2):
    return _mod("aggregated").AggregatedTrainer(_cfg(ms), E, fully=fully, hyper=_mod("trainer").Hyper(update_step=T),
                                                seed=seed)


def _dqn(ms, seed=4):
    dqn = _mod("dqn")
    return dqn.DQNTrainer(_cfg(ms), E, hyper=dqn.DQNHyper(batch_size=4, replay_memory_size=8), seed=seed)


def _without(per_replica, keys):
    return [[{k: v for k, v in d.items() if k not in keys} for d in ep] for ep in per_replica]


def test_hardcoded_baseline_is_the_same_for_every_trainer(ms):
    tr_mod = _mod("trainer")
    seed, n = 777, 5
    agg = _aggregated(ms).evaluate(episodes=2, n_envs=n, mode="hardcoded", seed=seed)
    dq = _dqn(ms).evaluate(episodes=2, n_envs=n, mode="hardcoded", seed=seed)
    ppo = tr_mod.Trainer(_cfg(ms), E, arch="divided", hyper=tr_mod.Hyper(update_step=T), seed=1, device="cuda:0"
                         ).evaluate(episodes=2, n_envs=n, mode="hardcoded", seed=seed)
    for r in (agg, dq, ppo):
        assert (r["mode"], r["seed"], r["n_envs"]) == ("hardcoded", seed, n)
        assert len(r["episodes"]) == 2 and len(r["per_replica"]) == 2 and len(r["per_replica"][0]) == n
    assert _same(dq["per_replica"], ppo["per_replica"]) and _same(dq["episodes"], ppo["episodes"])
    assert _same(_without(agg["per_replica"], AGGREGATED_KEYS), _without(ppo["per_replica"], AGGREGATED_KEYS))
    assert _same(_without([agg["episodes"]], AGGREGATED_KEYS), _without([ppo["episodes"]], AGGREGATED_KEYS))
    # the aggregated drivers' keys (and every other) against the restated driver on the rules' own actions
    want = replay(FIXED, seed, n, EP, [(None, None, None)] * (2 * EP), aggregated=True)
    assert_episodes_match(agg["per_replica"], want, EP)
    assert all(d["terminationRevenues"] == 0.0 for ep in agg["per_replica"] for d in ep)
    assert any(d["terminationRevenues"] != 0.0 for ep in ppo["per_replica"] for d in ep)
    assert_episodes_match(dq["per_replica"], replay(FIXED, seed, n, EP, [(None, None, None)] * (2 * EP)), EP)
    mx = _mod("metrics")
    assert _same(agg["episodes"], [mx.reduce_replicas(ep) for ep in agg["per_replica"]])


@pytest.mark.parametrize("fully", [False, True])
def test_aggregated_greedy_evaluation(ms, fully):
    tr = _aggregated(ms, fully)
    tr.iteration()  # the nets after one update
    seed, n = 4242, 6
    with record_class(ms.BatchedEnv, aggregated=True) as log:
        res = tr.evaluate(episodes=2, n_envs=n, mode="greedy", seed=seed)
    assert len(log.steps) == 2 * EP == len(log.obs) == len(log.numbers)
    assert_episodes_match(res["per_replica"], replay(FIXED, seed, n, EP, log.steps, aggregated=True), EP)
    # every action number is the float64 argmax of its net's logits on the aggregated observation it was taken on
    numbers = torch.stack(log.numbers)  # [rounds, 1 or 2, n, N]
    for i, (name, u) in enumerate(tr.units.items()):
        w = {k: getattr(u.group.policy_old, k).detach().cpu() for k in KEYS}
        rows = torch.stack([o[name] for o in log.obs])  # [rounds, n, N, stride]
        l64 = torch.cat([_logits(w, g, rows[:, :, g, :u.D].reshape(-1, u.D), torch.float64) for g in range(tr.N)])
        l32 = torch.cat([_logits(w, g, rows[:, :, g, :u.D].reshape(-1, u.D), torch.float32) for g in range(tr.N)])
        act = torch.cat([numbers[:, i, :, g].reshape(-1) for g in range(tr.N)]).long()
        check_greedy_rows(act, l64, l32, name + ":", max_near=None)
    # equal arguments, equal results; the default seed is not a training replica's
    assert _same(tr.evaluate(episodes=2, n_envs=n, mode="greedy", seed=seed), res)
    dflt = tr.evaluate()
    base = _mod("trainer").env_seed(2, 0, E)
    assert dflt["seed"] == tr.eval_seed() == base + 500_001 and dflt["n_envs"] == E and len(dflt["episodes"]) == 1


def test_aggregated_sample_evaluation(ms):
    tr = _aggregated(ms)
    seed, n = 99, 5
    with record_class(ms.BatchedEnv, aggregated=True) as log:
        res = tr.evaluate(episodes=1, n_envs=n, mode="sample", seed=seed)
    assert_episodes_match(res["per_replica"], replay(FIXED, seed, n, EP, log.steps, aggregated=True), EP)
    assert _same(tr.evaluate(episodes=1, n_envs=n, mode="sample", seed=seed), res)
    n_acc, n_off = tr.env.aggregated_action_counts()
    numbers = torch.stack(log.numbers)
    assert len(numbers[:, 0].unique()) > 1 and int(numbers[:, 0].max()) < n_acc and int(numbers[:, 1].max()) < n_off


def test_dqn_greedy_evaluation(ms):
    tr = _dqn(ms)
    tr.episode()
    seed, n = 31, 6
    with record_class(ms.BatchedEnv) as log:
        res = tr.evaluate(episodes=2, n_envs=n, mode="greedy", seed=seed)
    assert len(log.steps) == 2 * EP
    assert_episodes_match(res["per_replica"], replay(FIXED, seed, n, EP, log.steps), EP)
    assert _same(tr.evaluate(episodes=2, n_envs=n, mode="greedy", seed=seed), res)
    dflt = tr.evaluate()
    assert dflt["seed"] == tr.eval_seed() == _mod("trainer").env_seed(4, 0, E) + 500_001 and dflt["n_envs"] == E
    # the first round's picks are the first argmax of the policy nets' Q values on the reset observations
    env = ms.BatchedEnv(tr.cfg, n, seed=seed)
    obs = env.reset(env.obs_buffers())
    for grp, key, step_i in ((tr.acc, "acceptor", 0), (tr.off, "offer", 1)):
        x = obs[key].view(n, -1, obs[key].shape[-1])[..., :grp.policy.D].permute(1, 0, 2).double().cpu()
        p = {k: getattr(grp.policy, k).detach().double().cpu() for k in ("w1", "b1", "w2", "b2")}
        q = torch.baddbmm(p["b2"].unsqueeze(1), torch.tanh(torch.baddbmm(p["b1"].unsqueeze(1), x, p["w1"].transpose(1, 2))),
                          p["w2"].transpose(1, 2))  # [U, n, A]
        top2 = q.topk(2, dim=-1).values
        clear = (top2[..., 0] - top2[..., 1]) > 1e-5
        took = log.steps[0][step_i].view(n, -1).T.long()
        assert bool(clear.any()) and torch.equal(took[clear], q.argmax(-1)[clear])


def _agg_state(tr):
    d = {}
    for name, u in tr.units.items():
        for net in ("policy", "policy_old"):
            for k, p in getattr(u.group, net).named_parameters():
                d["%s.%s.%s" % (name, net, k)] = p.detach().clone()
        d.update({name + ".obs": u.obs, name + ".actions": u.actions, name + ".logprobs": u.logprobs,
                  name + ".rewards": u.rewards})
    d["rng_cpu"], d["rng_cuda"] = torch.get_rng_state(), torch.cuda.get_rng_state()
    d["round"] = torch.tensor(tr.env.round)
    return d


@pytest.mark.parametrize("fully", [False, True])
def test_aggregated_evaluate_leaves_training_as_it_was(ms, fully):
    states = []
    for with_eval in (True, False):
        tr = _aggregated(ms, fully)
        tr.iteration()
        if with_eval:
            for mode in ("greedy", "sample", "hardcoded"):
                tr.evaluate(episodes=1, n_envs=3, mode=mode)
        tr.iteration()
        assert tr.flags() == 0 and tr.bad_actions() == 0
        states.append(_agg_state(tr))
    a, b = states
    assert a.keys() == b.keys()
    for k in a:
        assert torch.equal(a[k], b[k]), k


def test_dqn_evaluate_leaves_training_as_it_was(ms):
    states = []
    for with_eval in (True, False):
        tr = _dqn(ms)
        tr.episode()
        if with_eval:
            for mode in ("greedy", "hardcoded"):
                tr.evaluate(episodes=1, n_envs=3, mode=mode)
        tr.episode()
        assert tr.flags() == 0
        d = {}
        for name, grp in (("acc", tr.acc), ("off", tr.off)):
            for net in ("policy", "target"):
                for k, p in getattr(grp, net).named_parameters():
                    d["%s.%s.%s" % (name, net, k)] = p.detach().clone()
        for name, mem in (("mem_acc", tr.mem_acc), ("mem_off", tr.mem_off)):
            d.update({name + ".states": mem.states, name + ".next_states": mem.next_states,
                      name + ".actions": mem.actions, name + ".rewards": mem.rewards})
        d.update(act_acc=tr.act_acc, act_off=tr.act_off, gen=tr.gen.get_state(), rng_cpu=torch.get_rng_state(),
                 rng_cuda=torch.cuda.get_rng_state(), round=torch.tensor(tr.env.round))
        states.append(d)
    a, b = states
    assert a.keys() == b.keys()
    for k in a:
        assert torch.equal(a[k], b[k]), k


def test_argument_checks(ms):
    agg, dq = _aggregated(ms), _dqn(ms)
    for tr in (agg, dq):
        with pytest.raises(ValueError):
            tr.evaluate(mode="argmax")
        with pytest.raises(ValueError):
            tr.evaluate(episodes=0)
        with pytest.raises(ValueError):
            tr.evaluate(n_envs=0)
        with pytest.raises(ValueError):
            tr.evaluate(n_envs=-2, mode="hardcoded")
    with pytest.raises(ValueError):
        dq.evaluate(mode="sample")  # the DQN nets have no sampling policy
    assert agg.env.round == 0 and dq.env.round == 0
