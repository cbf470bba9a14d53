"""The one episode log of the learners (Trainer, AggregatedTrainer, DQNTrainer) and of their ``evaluate()``
(evaluation.py): the env kernel's episode accumulators (``BatchedEnv.metrics_buffer``, handed to every
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
    """Accumulator slots of one env, or of the envs that hold one learner's replicas as contiguous ranges in order
    (EnvParts.parts; bufs[k] is part k's, for the log's life), and the episodes read from them. Round r (the env's
    round counter before the step) adds into slot (r // episode_length) % slots; a slot is zeroed when its episode
    is read, so `slots` must cover the episodes that can be open or unread at once. len(episodes) counts the
    episodes read: a checkpoint load that refills the list in place moves the log with it.
    hook (optional): called with each episode's list of per-replica dicts before it is appended."""

    def __init__(self, envs, slots: int = 1, aggregated: bool = False, log: list | None = None, hook=None):
        envs = list(envs) if isinstance(envs, (list, tuple)) else [envs]
        if aggregated and len(envs) != 1:
            raise ValueError("the aggregated rewards' sums are kept for a single env")
        env = envs[0]
        self.cfg, self.shape, self.slots, self.hook = env.cfg, (env.N, env.C, env.L), int(slots), hook
        self.ep_len = int(env.cfg.episode_length)
        self.bufs = [e.metrics_buffer(self.slots) for e in envs]
        self.events = [dict(metrics=b) for b in self.bufs]  # env.step(..., events=log.events[k])
        self.episodes = [] if log is None else log
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
        n = 0
        while len(self.episodes) < int(rounds_done) // self.ep_len:
            slot = len(self.episodes) % self.slots
            raw = torch.cat([b[slot] for b in self.bufs]).cpu().numpy()  # the parts' replicas, in part order
            for b in self.bufs:
                b[slot].zero_()
            ep = mx.episode_values(mx.view(raw), self.cfg, self.ep_len, *self.shape)
            if self.agg is not None:
                sums = self.agg[slot].cpu().numpy()
                self.agg[slot].zero_()
                aggregated_values(ep, sums[0], sums[1], self.ep_len)
            if self.hook is not None:
                self.hook(ep)
            self.episodes.append(ep)
            n += 1
        return n


def aggregated_values(episode: list, acceptor_sum, offer_sum, episode_length: int):
    """The aggregated drivers' reward keys of one episode's per-replica dicts, in place: acceptor_sum /
    offer_sum [E][N] int64 are the episode's sums of the per-agent aggregated rewards; the values are
    (sum / episodeLength) in float32, then the mean over the agents (trainPPO.py:218-220)."""
    T = np.float32(episode_length)
    for e, d in enumerate(episode):
        d["acceptorRew"] = float((np.asarray(acceptor_sum[e]).astype(np.float32) / T).mean())
        d["coreChooserRew"] = float((np.asarray(offer_sum[e]).astype(np.float32) / T).mean())
        d["priceChooserRew"] = 0.0
        d["terminationRevenues"] = 0.0


class EpisodeLogging:
    """What a learner with ``metrics: bool`` shares: ``episode_log`` (a list of episodes, each a list of
    per-replica dicts), ``args_dict`` and ``save_args_dict``."""

    def _init_episode_log(self, metrics: bool, envs, slots: int = 1, aggregated: bool = False, hook=None, **defaults):
        self.episode_log = []
        self._arg_defaults = defaults
        # metrics False: nothing allocated, env.step gets events=None and no harvest runs
        self._elog = EpisodeLog(envs, slots, aggregated, log=self.episode_log, hook=hook) if metrics else None
        self._metric_events = self._elog.events[0] if metrics else None  # a one-env learner's env.step(events=...)

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
