"""Shared by the learner metrics / evaluate tests (test infrastructure): recording the action tensors an env was
stepped with, replaying them per replica on the object-faithful world (oracle/pyref.py) beside the restated driver
bookkeeping (oracle/metrics_ref.py), the aggregated drivers' reward accumulators restated on
PyWorld.last_aggregated, and the comparison at tests/test_metrics_gpu.py's tolerances."""
import contextlib
import types
import warnings

import numpy as np
import torch

from oracle import pyref
from oracle.metrics_ref import EpisodeRecorder

# N = 2, C = 2, L = 2, two job kinds
FIXED = dict(n_agents=2, n_cores=2, collection_length=2, priorities=[3, 10], lengths=[6, 3], fix_prices=[2, 7],
             probabilities=[0.8, 0.2])

REWARD_KEYS = ("acceptorRew", "coreChooserRew", "priceChooserRew", "auctioneerRew", "acceptionQuality",
               "acceptionAmount", "terminationRevenues", "tradeRevenues")
AGGREGATED_KEYS = ("acceptorRew", "coreChooserRew", "priceChooserRew", "terminationRevenues")


def pcfg_of(kw, episode_length):
    return pyref.Config(n_agents=kw["n_agents"], n_cores=kw["n_cores"], collection_length=kw["collection_length"],
                        priorities=kw["priorities"], lengths=kw["lengths"], probabilities=kw["probabilities"],
                        fix_prices=kw.get("fix_prices", []), free_prices=kw.get("free_prices", False),
                        commercial=kw.get("commercial", True), episode_length=episode_length)


def _host(t):
    return None if t is None else t.detach().cpu().clone()


def wrap_step(step, log):
    """step with every call's (acceptor, offer_core, offer_price) appended to log as CPU copies (None: the rules)."""
    def recording(acceptor, offer_core, offer_price=None, *args, **kw):
        log.append((_host(acceptor), _host(offer_core), _host(offer_price)))
        return step(acceptor, offer_core, offer_price, *args, **kw)
    return recording


def record_env(env):
    """Record every later step of this env instance; returns the log."""
    log = []
    env.step = wrap_step(env.step, log)
    return log


@contextlib.contextmanager
def record_class(cls, aggregated=False):
    """Record the steps of every env of class cls stepped inside the block (evaluate() makes its own): log.steps,
    and with aggregated also log.obs (the aggregated observations after each aggregate_obs, name -> CPU tensor) and
    log.numbers (the action numbers given to decode_aggregated)."""
    log = types.SimpleNamespace(steps=[], obs=[], numbers=[])
    orig = cls.step, cls.aggregate_obs, cls.decode_aggregated

    def step(self, acceptor, offer_core, offer_price=None, *args, **kw):
        log.steps.append((_host(acceptor), _host(offer_core), _host(offer_price)))
        return orig[0](self, acceptor, offer_core, offer_price, *args, **kw)

    def aggregate_obs(self, *args, **kw):
        out = orig[1](self, *args, **kw)
        log.obs.append({k: _host(v) for k, v in out.items()})
        return out

    def decode_aggregated(self, numbers, *args, **kw):
        log.numbers.append(_host(numbers))
        return orig[2](self, numbers, *args, **kw)

    cls.step = step
    if aggregated:
        cls.aggregate_obs, cls.decode_aggregated = aggregate_obs, decode_aggregated
    try:
        yield log
    finally:
        cls.step, cls.aggregate_obs, cls.decode_aggregated = orig


class AggregatedRecorder:
    """trainPPO.py:141-144, 180-182, 218-220 with aggregatedAgents / fullyAggregatedAgents: [N][1] int64 torch
    accumulators of getAggregatedFixedPricesReward's rewards (PyWorld.last_aggregated), reported as
    (accumulator / episodeLength).numpy().mean(); the price accumulator stays zero and env.terminationRevenues is
    never added to (Reward.py:92-143)."""

    def __init__(self, world):
        self.w = world
        self.core = torch.tensor([[0] for _ in range(world.N)])
        self.price = torch.tensor([[0] for _ in range(world.N)])
        self.acc = torch.tensor([[0] for _ in range(world.N)])

    def add(self):
        off, acc = self.w.last_aggregated
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            self.core += off
            self.acc += acc

    def finish(self, T):
        return dict(coreChooserRew=(self.core / T).numpy().mean(), priceChooserRew=(self.price / T).numpy().mean(),
                    acceptorRew=(self.acc / T).numpy().mean(), terminationRevenues=0 / (T * self.w.N * self.w.C))


def replay(kw, seed, E, T, steps, aggregated=False):
    """The recorded steps on one PyWorld per replica (replica e seeded seed + e) beside the restated driver: a list
    of episodes, each a list of E dicts (EpisodeRecorder.finish, with the aggregated drivers' keys when asked)."""
    pcfg = pcfg_of(kw, T)
    free = bool(kw.get("free_prices", False))
    worlds = [pyref.PyWorld(pcfg, seed + e) for e in range(E)]
    N, C, L = pcfg.n_agents, pcfg.n_cores, pcfg.collection_length
    episodes, recs, aggs = [], None, None
    for t, (acc, off, price) in enumerate(steps):
        if t % T == 0:
            recs = [EpisodeRecorder(w, free) for w in worlds]
            aggs = [AggregatedRecorder(w) for w in worlds]
        for e, w in enumerate(worlds):
            if acc is None:
                a, o = w.hardcoded_agent_actions()
            else:
                a = acc.view(E, N, C)[e].tolist()
                o = off.view(E, N, L)[e].tolist()
                if free:
                    p = price.view(E, N, L)[e].tolist()
                    o = [[(o[i][l], p[i][l]) for l in range(L)] for i in range(N)]
            recs[e].add(w.step(a, o))
            aggs[e].add()
        if (t + 1) % T == 0:
            ep = []
            for e in range(E):
                d = recs[e].finish(pcfg, T)
                if aggregated:
                    d.update(aggs[e].finish(T))
                ep.append(d)
            episodes.append(ep)
    return episodes


def _close(a, b, rel=1e-6):
    if a is None or b is None:
        assert a is None and b is None, (a, b)
        return
    assert abs(float(a) - float(b)) <= rel * max(1.0, abs(float(b))), (a, b)


def assert_episodes_match(got, want, T):
    """Episodes of an episode_log / evaluate()'s per_replica against replay()'s, replica by replica."""
    assert len(got) == len(want), (len(got), len(want))
    for g_ep, w_ep in zip(got, want):
        assert len(g_ep) == len(w_ep)
        for g, w in zip(g_ep, w_ep):
            assert g["rounds"] == T
            for k in REWARD_KEYS:
                _close(g[k], w[k])
            for k in ("prices", "dwellTimes"):
                assert len(g[k]) == len(w[k])
                for x, y in zip(g[k], w[k]):
                    _close(x, y, 1e-12)
            np.testing.assert_allclose(g["agentRew"], w["agentRew"], rtol=1e-12)
