"""metrics=True on AggregatedTrainer and DQNTrainer: every episode of episode_log against the restated
driver (oracle/metrics_ref.py, and the aggregated drivers' reward accumulators restated in tests/learner_replay.py)
on a replay of the recorded actions, training bit-identical with and without metrics, and the argsDict."""
import importlib
import os
import pickle

import pytest
import torch

from tests.learner_replay import FIXED, assert_episodes_match, record_env, replay

pytestmark = pytest.mark.gpu

ARGS_KEYS = {"plotPath", "acceptorRew", "coreChooserRew", "priceChooserRew", "prices", "auctioneerRew", "dwellTimes",
             "meanJob", "agentRew", "acceptionQuality", "acceptionAmount", "terminationRevenues", "tradeRevenues",
             "params"}


def _mod(name):
    return importlib.import_module("marl-scheduling_amd." + name)


def _aggregated(ms, fully, metrics, E=4, T=15, ep=10, seed=2):
    cfg = ms.abi.make_config(episode_length=ep, **FIXED)
    return _mod("aggregated").AggregatedTrainer(cfg, E, fully=fully, hyper=_mod("trainer").Hyper(update_step=T),
                                                seed=seed, metrics=metrics)


def _dqn(ms, metrics, E=3, ep=11, seed=4):
    dqn = _mod("dqn")
    cfg = ms.abi.make_config(episode_length=ep, **FIXED)
    return dqn.DQNTrainer(cfg, E, hyper=dqn.DQNHyper(batch_size=4, replay_memory_size=8), seed=seed, metrics=metrics)


# ---- against the restated driver
@pytest.mark.parametrize("fully", [False, True])
def test_aggregated_episode_log_matches_the_restated_driver(ms, fully):
    E, T, ep, seed = 4, 15, 10, 2  # update_step is no multiple of the episode length
    tr = _aggregated(ms, fully, True, E, T, ep, seed)
    steps = record_env(tr.env)
    tr.iteration()
    assert len(tr.episode_log) == 1  # 15 rounds: one episode finished, the second open
    tr.iteration()
    assert len(tr.episode_log) == 3 and len(steps) == 2 * T
    want = replay(FIXED, _mod("trainer").env_seed(seed, 0, E), E, ep, steps[:3 * ep], aggregated=True)
    assert_episodes_match(tr.episode_log, want, ep)
    assert all(d["terminationRevenues"] == 0.0 and d["priceChooserRew"] == 0.0 for e in tr.episode_log for d in e)
    assert any(d["acceptorRew"] != 0.0 for e in tr.episode_log for d in e)
    assert tr.flags() == 0 and tr.bad_actions() == 0


def test_dqn_episode_log_matches_the_restated_driver(ms):
    E, ep, seed = 3, 11, 4
    tr = _dqn(ms, True, E, ep, seed)
    steps = record_env(tr.env)
    for i in range(3):
        tr.episode()
        assert len(tr.episode_log) == i + 1
    assert tr.mem_acc.next_free + 1 == tr.mem_acc.cap  # the small memories filled and replaced
    want = replay(FIXED, _mod("trainer").env_seed(seed, 0, E), E, ep, steps)
    assert_episodes_match(tr.episode_log, want, ep)
    assert tr.flags() == 0


# ---- metrics on / off: bit-identical training
def _equal(a, b, what):
    assert a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.view(torch.uint8), b.view(torch.uint8)), what


def _rng_states(tr=None):
    st = [torch.get_rng_state(), torch.cuda.get_rng_state()]
    if tr is not None:
        st.append(tr.gen.get_state())
    return st


def _pairs(make, run, state):
    """state(trainer) after run(trainer), for metrics on and off (one trainer after the other: they share torch's
    default generators, which the constructor seeds)."""
    out = []
    for metrics in (True, False):
        tr = make(metrics)
        run(tr)
        out.append((state(tr), tr.flags(), tr))
    (a, fa, ta), (b, fb, tb) = out
    assert fa == fb == 0
    assert a.keys() == b.keys()
    for k in a:
        if isinstance(a[k], torch.Tensor):
            _equal(a[k], b[k], k)
        else:
            assert a[k] == b[k], k
    assert ta.episode_log and tb.episode_log == [] and tb._elog is None
    return ta, tb


@pytest.mark.parametrize("fully", [False, True])
def test_aggregated_training_is_the_same_with_and_without_metrics(ms, fully):
    def state(tr):
        d = {}
        for name, u in tr.units.items():
            for net in ("policy", "policy_old"):
                for k, p in getattr(u.group, net).named_parameters():
                    d["%s.%s.%s" % (name, net, k)] = p.detach()
            d.update({name + ".obs": u.obs, name + ".actions": u.actions, name + ".logprobs": u.logprobs,
                      name + ".rewards": u.rewards})
        d.update({"rew." + k: v for k, v in tr.rew.items() if v is not None})
        d.update({"div_obs." + k: v for k, v in tr.div_obs.items() if v is not None})
        d["numbers"] = tr.numbers
        for i, s in enumerate(_rng_states()):
            d["rng%d" % i] = s
        return d

    def run(tr):
        tr.iteration()
        tr.iteration()
    _pairs(lambda m: _aggregated(ms, fully, m), run, state)


def test_dqn_training_is_the_same_with_and_without_metrics(ms):
    def state(tr):
        d = {}
        for name, grp in (("acc", tr.acc), ("off", tr.off)):
            for net in ("policy", "target"):
                for k, p in getattr(grp, net).named_parameters():
                    d["%s.%s.%s" % (name, net, k)] = p.detach()
        for name, mem in (("mem_acc", tr.mem_acc), ("mem_off", tr.mem_off)):
            d.update({name + ".states": mem.states, name + ".next_states": mem.next_states,
                      name + ".actions": mem.actions, name + ".rewards": mem.rewards, name + ".next_free": mem.next_free})
        d.update({"rew." + k: v for k, v in tr.rew.items()})
        d.update(act_acc=tr.act_acc, act_off=tr.act_off, cur=tr.cur, episodes=tr.episodes)
        for i, o in enumerate(tr.obs):
            d.update({"obs%d.%s" % (i, k): v for k, v in o.items()})
        for i, s in enumerate(_rng_states(tr)):
            d["rng%d" % i] = s
        return d

    def run(tr):
        for _ in range(3):
            tr.episode()
    _pairs(lambda m: _dqn(ms, m), run, state)


# ---- the argsDict
def _check_args_dict(tr, n_episodes, ep, n_kinds, tmp_path):
    d = tr.args_dict()
    assert set(d) >= ARGS_KEYS
    for k in ARGS_KEYS - {"plotPath", "meanJob", "params"}:
        assert len(d[k]) == n_episodes, k
    assert len(d["prices"][0]) == n_kinds and len(d["dwellTimes"][0]) == n_kinds and len(d["agentRew"][0]) == tr.N
    assert all(isinstance(v, float) for v in d["acceptionAmount"] + d["acceptorRew"] + d["coreChooserRew"])
    assert d["params"]["episodeLength"] == ep and d["params"]["n_envs"] == tr.E
    one = tr.args_dict(replica=1, params=dict(note="x"))
    assert one["acceptorRew"] == [e[1]["acceptorRew"] for e in tr.episode_log] and one["params"]["note"] == "x"
    (tmp_path / "data0.pkl").write_bytes(b"taken")
    p = tr.save_args_dict(str(tmp_path))
    assert os.path.basename(p) == "data1.pkl"
    with open(p, "rb") as f:  # our own file, written just above
        saved = pickle.load(f)
    assert set(saved) >= ARGS_KEYS and len(saved["acceptorRew"]) == n_episodes
    assert saved["params"]["episodeLength"] == ep
    assert os.path.basename(tr.save_args_dict(str(tmp_path))) == "data2.pkl"


def test_aggregated_args_dict(ms, tmp_path):
    tr = _aggregated(ms, False, True)
    tr.iteration()
    tr.iteration()
    _check_args_dict(tr, 3, 10, 2, tmp_path)
    assert tr.args_dict()["params"]["UPDATE_STEP"] == 15


def test_dqn_args_dict(ms, tmp_path):
    tr = _dqn(ms, True)
    tr.episode()
    tr.episode()
    _check_args_dict(tr, 2, 11, 2, tmp_path)


def test_without_metrics_the_log_stays_empty(ms):
    tr = _dqn(ms, False)
    tr.episode()
    assert tr.episode_log == [] and tr.args_dict()["acceptorRew"] == []
