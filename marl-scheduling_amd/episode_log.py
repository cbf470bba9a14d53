"""One episode log for the learners beside ``Trainer`` (AggregatedTrainer, DQNTrainer) and for their
``evaluate()``: the env kernel's episode accumulators (``BatchedEnv.metrics_buffer``, handed to every
``env.step`` as ``events["metrics"]``), the harvest of finished episodes into the drivers' per-episode values
(``metrics.view`` / ``metrics.episode_values``) and the ``argsDict`` of trainPPO.py:229-251 / trainDQN.py.

Aggregated agents. With aggregatedAgents / fullyAggregatedAgents the driver's reward accumulators are not
the divided unit rewards the env accumulators hold: trainPPO.py:141-144, 180-182 sum the per-agent [N][1]
rewards of getAggregatedFixedPricesReward (Reward.py:92-143), and :218-220 report (accumulator /
episodeLength) in float32, averaged over the agents. ``EpisodeLog(aggregated=True)`` keeps a per-replica int64
running sum of those two reward buffers on the device (``add_aggregated``, one torch add per round) and
replaces acceptorRew / coreChooserRew with the driver's values; priceChooserRew is 0.0 (its accumulator
stays zero) and terminationRevenues is 0.0 (that reward function never adds to env.terminationRevenues).
Every other key is the env accumulators', unchanged.
"""
from __future__ import annotations

import numpy as np
import torch

from . import metrics as mx


class EpisodeLog:
    """Accumulator slots of one env and the episodes read from them. Round r (the env's round counter before
    the step) adds into slot (r // episode_length) % slots; a slot is zeroed when its episode is read, so
    `slots` must cover the episodes that can be open or unread at once."""

    def __init__(self, env, slots: int = 1, aggregated: bool = False, log: list | None = None):
        self.env, self.cfg, self.slots = env, env.cfg, int(slots)
        self.ep_len = int(env.cfg.episode_length)
        self.buf = env.metrics_buffer(self.slots)
        self.events = dict(metrics=self.buf)  # env.step(..., events=log.events)
        self.episodes = [] if log is None else log
        self.read = 0  # episodes harvested
        # [slots][2][E][N] int64: the running sums of the aggregated acceptor / offer rewards
        self.agg = (torch.zeros((self.slots, 2, env.E, env.N), dtype=torch.int64, device=env.device)
                    if aggregated else None)

    def add_aggregated(self, round_index: int, acceptor, offer):
        """The [E][N] int32 rewards of the round that started at round_index, into its episode's sums."""
        s = self.agg[(int(round_index) // self.ep_len) % self.slots]
        s[0] += acceptor
        s[1] += offer

    def harvest(self, rounds_done: int) -> int:
        """Append every episode finished after rounds_done rounds and not read yet; returns their number."""
        env = self.env
        n = 0
        while self.read < int(rounds_done) // self.ep_len:
            slot = self.read % self.slots
            raw = self.buf[slot].cpu().numpy()
            self.buf[slot].zero_()
            ep = mx.episode_values(mx.view(raw), self.cfg, self.ep_len, env.N, env.C, env.L)
            if self.agg is not None:
                sums = self.agg[slot].cpu().numpy()
                self.agg[slot].zero_()
                aggregated_values(ep, sums[0], sums[1], self.ep_len)
            self.episodes.append(ep)
            self.read += 1
            n += 1
        return n


def aggregated_values(episode: list, acceptor_sum, offer_sum, episode_length: int) -> list:
    """The aggregated drivers' reward keys of one episode's per-replica dicts, in place: acceptor_sum /
    offer_sum [E][N] int64 are the episode's sums of the per-agent aggregated rewards; the values are
    (sum / episodeLength) in float32, then the mean over the agents (trainPPO.py:218-220)."""
    T = np.float32(episode_length)
    for e, d in enumerate(episode):
        d["acceptorRew"] = float((np.asarray(acceptor_sum[e]).astype(np.float32) / T).mean())
        d["coreChooserRew"] = float((np.asarray(offer_sum[e]).astype(np.float32) / T).mean())
        d["priceChooserRew"] = 0.0
        d["terminationRevenues"] = 0.0
    return episode


class EpisodeLogging:
    """What a learner with ``metrics: bool`` shares: ``episode_log`` (a list of episodes, each a list of
    per-replica dicts), ``args_dict`` and ``save_args_dict`` with ``Trainer``'s meaning and return types."""

    def _init_episode_log(self, metrics: bool, env, slots: int = 1, aggregated: bool = False, **defaults):
        self.episode_log = []
        self._arg_defaults = defaults
        # metrics False: nothing allocated, env.step gets events=None and no harvest runs
        self._elog = EpisodeLog(env, slots, aggregated, log=self.episode_log) if metrics else None

    @property
    def _metric_events(self):
        return None if self._elog is None else self._elog.events

    def args_dict(self, replica="mean", params=None):
        """argsDict of the finished episodes (trainPPO.py:229-243): replica = "mean" averages the replicas'
        values per episode, an int picks one replica."""
        p = dict(params or {})
        for k, v in self._arg_defaults.items():
            p.setdefault(k, v)
        return mx.args_dict(self.episode_log, self.cfg, p, replica=replica)

    def save_args_dict(self, directory: str = ".", file_name: str = "data{}.pkl", replica="mean", params=None):
        """args_dict() pickled as the first free data{i}.pkl in directory (trainPPO.py:245-251)."""
        return mx.save_args_dict(self.args_dict(replica, params), file_name, directory)


def evaluation_result(mode: str, seed: int, n_envs: int, per_replica: list) -> dict:
    """evaluate()'s result (Trainer.evaluate's form) from the harvested episodes."""
    return dict(mode=mode, seed=seed, n_envs=n_envs, episodes=[mx.reduce_replicas(ep) for ep in per_replica],
                per_replica=per_replica)


def check_evaluate_args(episodes, n_envs, default_envs: int, mode: str, modes: tuple):
    if mode not in modes:
        raise ValueError("mode must be one of %s" % ", ".join(repr(m) for m in modes))
    episodes, E = int(episodes), int(default_envs if n_envs is None else n_envs)
    if episodes < 1 or E < 1:
        raise ValueError("episodes and n_envs must be >= 1")
    return episodes, E
