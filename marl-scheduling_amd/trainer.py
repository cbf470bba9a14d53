"""Batched PPO training loop over E env replicas (the trainPPO.py loop, trainPPO.py:133-227).

One ``iteration`` = UPDATE_STEP rounds of (policy act -> env step -> buffer
writes) followed by the PPO update of every unit type, the cadence of
``trainPPO.py:169`` (update when ``world.round % UPDATE_STEP == 0``).
Everything stays on the device: observations are written by the env kernel
straight into the rollout buffers, actions/log-probs by the act kernel.

Architectures (SchedulingEnvironment.py:253-348):
  ``divided`` — PPODividedFixedPriceEnv / PPODividedFreePriceEnv: one net per unit,
  ``local``   — LocallySharedParamsDividedFixedPriceEnv (+ the free-price variant
                BASELINE cfg3 names): one net per agent and unit type,
                CENTRALISATION_SAMPLE sub-units drawn per agent (Agent.py:708-728),
  ``global``  — GloballySharedParamsDividedFixedPriceEnv: one net per unit type,
                CENTRALISATION_SAMPLE (agent, sub-unit) pairs (SchedulingEnvironment.py:314-329).

Multi-GPU: replicas shard across ranks (weak scaling); the nets are shared, so
each optimizer step all-reduces one flattened gradient buffer (RCCL).
"""
from __future__ import annotations

import ctypes as ct
import os
import random
import time
import warnings
from dataclasses import dataclass, field

import numpy as np
import torch

from . import abi, evaluation
from ._lib import ABI_LOADED, capturing, has, hip_capture, ptr
from .action_log import ActionLog, n_priorities
from .env import BatchedEnv
from .episode_log import EpisodeLogging
from .metrics import action_args as mx_action_args
from .evaluation import env_seed  # (its home; dqn.py, aggregated.py and the tests take it from here too)
from .ppo import (ActFrag, PPOGroup, PriceTable, act_round_free, combine_losses, discounted_returns, offer_act_free,
                  offer_compress, offer_expand, reference_init_order, reference_nets, unit_returns)


@dataclass
class Hyper:
    """RL hyper-parameters of trainPPO.py:66-84 (defaults: trainPPO.py)."""
    lr_actor: float = 0.003
    lr_critic: float = 0.01
    eps_clip: float = 0.2
    acceptor_gamma: float | None = None   # default -((1-maxLen)/maxLen) + 0.04 (trainPPO.py:72)
    offer_gamma: float = 0.5
    raw_k_epochs: int = 3
    centralisation_sample: int = 2
    update_step: int = 200
    extra: dict = field(default_factory=dict)


def _k_epochs(raw, factor):
    return max(round(raw / factor), 1)  # trainPPO.py:76-77 (Python round: half-even)


class _Unit:
    """Rollout buffers + PPO group of one unit type (acceptor / offer / price chooser)."""

    def __init__(self, name, E, T, n_units, per_group, in_dim, stride, n_actions, group: PPOGroup, device,
                 reward_dtype, unit_major: bool = False):
        self.name, self.E, self.T, self.U, self.S = name, E, T, n_units, per_group
        self.D, self.stride = in_dim, stride
        self.group = group
        # unit_major: actions / log-probs stored [U][T][E] (one unit's rows of every replica are
        # contiguous for the update's gathers); .actions / .logprobs stay [T][E][U] views
        self.unit_major = unit_major
        # actions_raw / logprobs_raw: the ring tensors as they are (the kernels' pointers come from these);
        # .actions / .logprobs first run `complete` (Trainer._complete_rings for the acceptors, whose rings an
        # iteration() leaves without the items the gradient regenerates), then return the same tensors
        self.complete = None
        if unit_major:
            self.actions_um = torch.zeros((n_units, T, E), dtype=torch.int8, device=device)
            self.logprobs_um = torch.zeros((n_units, T, E), dtype=torch.float32, device=device)
            self.actions_raw = self.actions_um.permute(1, 2, 0)
            self.logprobs_raw = self.logprobs_um.permute(1, 2, 0)
        else:
            self.actions_raw = torch.zeros((T, E, n_units), dtype=torch.int8, device=device)
            self.logprobs_raw = torch.zeros((T, E, n_units), dtype=torch.float32, device=device)
        self.rewards = torch.zeros((T, E, n_units), dtype=reward_dtype, device=device)

    @property
    def actions(self):
        if self.complete is not None:
            self.complete()
        return self.actions_raw

    @property
    def logprobs(self):
        if self.complete is not None:
            self.complete()
        return self.logprobs_raw

    def batch(self, states_i8, u_sel):
        """Gather the update batch of the selected unit per group (u_sel [G] long)."""
        T, E, G = self.T, self.E, u_sel.numel()
        x = states_i8.index_select(2, u_sel)[..., : self.D]               # [T, E, G, D]
        x = x.permute(2, 0, 1, 3).reshape(G, T * E, self.D).float()
        a = self.actions.index_select(2, u_sel).permute(2, 0, 1).reshape(G, T * E).long()
        lp = self.logprobs.index_select(2, u_sel).permute(2, 0, 1).reshape(G, T * E)
        r = self.rewards.index_select(2, u_sel).float().reshape(T, E * G)
        ret = discounted_returns(r, self.group.gamma)                     # [E*G, T]
        ret = ret.view(E, G, T).permute(1, 2, 0).reshape(G, T * E)
        return x, a, lp, ret


def allreduce_mean_grads(params, world_size: int, group=None):
    """Average the gradients over ranks with one flattened all-reduce (RCCL over xGMI on GPUs,
    gloo on CPU). Shards are equal, so the mean of the per-rank mean losses' gradients is the
    gradient of the mean over all replicas."""
    import torch.distributed as dist
    grads = [p.grad for p in params if p.grad is not None]
    if not grads:
        return
    flat = torch._utils._flatten_dense_tensors(grads)
    dist.all_reduce(flat, op=dist.ReduceOp.SUM, group=group)
    flat.div_(world_size)
    for g, f in zip(grads, torch._utils._unflatten_dense_tensors(flat, grads)):
        g.copy_(f)


def broadcast_params(groups, group=None):
    """Rank 0's weights to every rank (identical start), then policy_old <- policy."""
    import torch.distributed as dist
    for grp in groups:
        for p in grp.policy.parameters():
            dist.broadcast(p.data, src=0, group=group)
        grp.sync_old()


class EnvParts:
    """The rank's E replicas as P contiguous parts [e0, e1), each its own BatchedEnv (replica e keeps
    random.seed(base + e) whatever the split). One part per rollout stream (Trainer.round)."""

    def __init__(self, cfg, E: int, base_seed: int, n_parts: int, device):
        assert E % n_parts == 0
        w = E // n_parts
        self.parts = [(BatchedEnv(cfg, w, seed=base_seed + k * w, device=device), k * w, (k + 1) * w)
                      for k in range(n_parts)]
        self.E = E
        self.shape = self.parts[0][0].shape

    @property
    def round(self) -> int:
        return self.parts[0][0].round

    def flags(self) -> int:
        f = 0
        for env, _, _ in self.parts:
            f |= env.flags()
        return f


class Trainer(EpisodeLogging):
    def __init__(self, cfg: abi.MsConfig, n_envs: int, arch: str = "local", hyper: Hyper | None = None, seed: int = 0,
                 device=None, rank: int = 0, world_size: int = 1, process_group=None, fused: bool = True,
                 use_graph: bool = True, common_rows: bool = True, rollout_streams: int = 1, metrics: bool = False,
                 episode_length: int | None = None, compact: bool = True, hardcoded_agents=None, diagnostics: int = 0,
                 action_log: bool = False, action_tables: bool = False, learned_auctioneer: bool = False):
        """learned_auctioneer (fixed prices; off by default: nothing is allocated, launched or changed): a fourth unit
        type "auctioneer" (self.auct), one net of the acceptor's shape shared by the C cores, that acts every round
        for the cores nobody owns in place of the in-kernel HardcodedAuctioneerAcceptor and trains in update() on
        the per-core auctioneerReward like the other units (centralisation_sample cores drawn per update, after the
        offer draws). Its initial weights are drawn after every agent net's, so a seeded trainer's agent nets start
        as without it. Its states are the compact acceptor rows with core_owner == 0 as the owner (the auctioneer
        row of core c is core row c where nobody owns it, else the foreign row). ValueError under free prices, with
        compact=False, with hardcoded_agents, with world_size > 1 and with diagnostics > 0. action_log keeps
        counting the agents' units only.
        action_log: one entry per finished episode in self.action_log (action_log.py: the histograms of the offer,
        price and acceptor actions, pooled over the replicas), counted from the rollout's rings by log_actions(),
        which iteration() calls between the rollout and the update. action_tables (needs action_log: ValueError
        otherwise) adds the action-by-priority tables to each entry. Both off (the default): nothing is allocated,
        launched or synchronised. hardcoded_agents' rows count what the rules played (the rings hold it). Several
        ranks: each keeps the log of its own replicas.
        diagnostics (k >= 0): the number of ring slots update_diagnostics() evaluates after each update,
        slots (2 i + 1) T // (2 k) for i < min(k, T); with k > 0 iteration() calls it after the update's end event
        and appends the result to self.diagnostics_log. 0 (the default) is off: nothing is allocated or launched.
        The log is not written into checkpoints (the checkpoint format does not know it): a resumed run starts an
        empty one.
        hardcoded_agents (an iterable of 0-based agent indices; fixed prices): train in a mixed market. The given
        agents play the reference's DividedHardcodedAgent rules inside the env kernel in every rollout round (as in
        evaluate(hardcoded_agents=...)), the action rings receive what they played, and they never train: no
        sub-unit of theirs is drawn for an update, and under ``local`` / ``divided`` their nets' groups are frozen
        (weights, policy_old and Adam moments keep their bits; their loss entries are NaN). None (the default)
        changes nothing; an empty list is a trainer without the argument, bit for bit. ValueError under free
        prices, for an index outside [0, N) and for a mask that leaves no agent to train."""
        assert arch in ("divided", "local", "global")
        if learned_auctioneer:  # (before anything touches the device)
            if cfg.free_prices:
                raise ValueError("learned_auctioneer acts under fixed prices only")
            if not compact or not common_rows or abi.config_shape(cfg)["acc_obs_stride"] < 16:
                raise ValueError("learned_auctioneer needs the compact acceptor observations (compact=True)")
            if hardcoded_agents is not None:
                raise ValueError("learned_auctioneer does not go with hardcoded_agents")
            if world_size > 1:
                raise ValueError("learned_auctioneer runs on one rank (world_size == 1)")
            if int(diagnostics) > 0:
                raise ValueError("learned_auctioneer has no update diagnostics (diagnostics == 0)")
        self.fused = fused  # fused HIP gradient (ms_ppo_grad) vs torch autograd
        self.device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        torch.cuda.set_device(self.device)
        self.hp = hyper or Hyper()
        if episode_length is not None:  # episodeLength (world.py:243): the env's `done` cadence
            cfg = abi.MsConfig.from_buffer_copy(cfg)
            cfg.episode_length = int(episode_length)
        self.cfg, self.arch, self.E = cfg, arch, int(n_envs)
        self.rank, self.world_size, self.pg = rank, world_size, process_group
        self.seed = seed
        # rollout_streams > 1: the replicas split into that many parts, each stepped on its own HIP
        # stream, so one part's env round (latency-bound) runs beside another part's act kernels
        # (VALU-bound); the parts share the rollout rings and the nets
        assert rollout_streams >= 1 and self.E % rollout_streams == 0
        self.env = EnvParts(cfg, self.E, env_seed(seed, rank, self.E), rollout_streams, self.device)
        self.streams = [None] + [torch.cuda.Stream(device=self.device) for _ in range(rollout_streams - 1)]
        s = self.env.shape
        N, C, L = s.n_agents, s.n_cores, s.collection_length
        self.N, self.C, self.L = N, C, L
        self.free = bool(cfg.free_prices)
        self.hardcoded = None
        if hardcoded_agents is not None:  # evaluate()'s checks, and somebody must be left to train
            if self.free:
                raise ValueError("the hard-coded agents act under fixed prices only")
            self.hardcoded = evaluation.agent_indices(hardcoded_agents, N)
            if len(self.hardcoded) == N:
                raise ValueError("hardcoded_agents covers every agent: nothing would train")
            if self.hardcoded and arch != "global" and not fused:
                raise ValueError("frozen groups (hardcoded_agents under 'local' / 'divided') need the fused update")
        self.hc_mask = sum(1 << a for a in self.hardcoded or [])
        self.learned = [a for a in range(N) if not (self.hc_mask >> a) & 1]
        # hardcoded_agents=[]: the fused launches go through the mixed library calls with mask 0 (the plain kernels)
        self._empty_mask = 0 if self.hardcoded == [] else None
        T = self.T = self.hp.update_step
        hp = self.hp
        max_len = max(cfg.job_length[: cfg.n_kinds])
        acc_gamma = hp.acceptor_gamma if hp.acceptor_gamma is not None else -((1 - max_len) / max_len) + 0.04
        # K epochs and groups per architecture (trainPPO.py:54-55,76-77; PPOmodules.py:289,304)
        if arch == "divided":
            ga, go, k_acc, k_off = N * C, N * L, _k_epochs(hp.raw_k_epochs, 1), _k_epochs(hp.raw_k_epochs, 1)
            if self.free:
                k_off = hp.raw_k_epochs  # FreePriceOfferPPO uses env.RAW_K_EPOCHS
        elif arch == "local":
            ga, go, k_acc, k_off = N, N, _k_epochs(hp.raw_k_epochs, C), _k_epochs(hp.raw_k_epochs, L)
        else:
            ga, go, k_acc, k_off = 1, 1, _k_epochs(hp.raw_k_epochs, N * C), _k_epochs(hp.raw_k_epochs, N * L)
        self.k_acc, self.k_off = k_acc, k_off
        allreduce = self._allreduce if world_size > 1 else None
        # initial weights: the reference's construction order on torch's CPU generator, so a seeded
        # Trainer starts from the weights the reference's agents would draw (same on every rank)
        torch.manual_seed(seed)
        dims = dict(acc=(s.acc_obs_dim, s.acc_actions), off=(s.off_obs_dim, s.off_actions), price=(4, s.price_actions))
        order = reference_init_order(arch, N, C, L, self.free)
        nets = reference_nets(order, {k: dims[k] for k in set(order)})
        dev = self.device
        mk = lambda G, D, A, gamma, K, init: PPOGroup(G, D, A, hp.lr_actor, hp.lr_critic, gamma, hp.eps_clip, K, dev,
                                                      allreduce, init_nets=init)
        self.acc = _Unit("acceptor", self.E, T, N * C, (N * C) // ga, s.acc_obs_dim, s.acc_obs_stride, s.acc_actions,
                         mk(ga, s.acc_obs_dim, s.acc_actions, acc_gamma, k_acc, nets["acc"]), dev, torch.int32)
        self.off = _Unit("offer", self.E, T, N * L, (N * L) // go, s.off_obs_dim, s.off_obs_stride, s.off_actions,
                         mk(go, s.off_obs_dim, s.off_actions, hp.offer_gamma, k_off, nets["off"]), dev, torch.float32)
        self.price = None
        if self.free:
            # MS_PRICE_UNIT_MAJOR=1: the price chooser's rollout rows unit-major, so its update (keyed
            # rows) gathers one unit's rows of every replica contiguously instead of 4 B of every 256 B
            # [E][U] line. Measured at cfg3: k_key_gather 344 -> 279 us, but the act launch's scattered
            # price writes +1.3 us per round: no net gain, so off by default
            self.price_unit_major = os.environ.get("MS_PRICE_UNIT_MAJOR", "0") == "1"
            self.price = _Unit("price", self.E, T, N * L, (N * L) // go, 4, 4, s.price_actions,
                               mk(go, 4, s.price_actions, hp.offer_gamma, k_off, nets["price"]), dev, torch.float32,
                               unit_major=self.price_unit_major)
        # the learned auctioneer: one net of the acceptor's shape for the C cores, drawn after every agent net
        self.auct = None
        if learned_auctioneer:
            auct_net = reference_nets(["acc"], dict(acc=dims["acc"]))["acc"]
            self.auct = _Unit("auctioneer", self.E, T, C, C, s.acc_obs_dim, s.acc_obs_stride, s.acc_actions,
                              mk(1, s.acc_obs_dim, s.acc_actions, acc_gamma, _k_epochs(hp.raw_k_epochs, C), auct_net),
                              dev, torch.int32)
        # the masked agents' groups never step (HipAdam.freeze); global: the one shared net trains on the others
        self._frozen = {}
        if self.hc_mask and arch != "global":
            for u, per_agent in ((self.acc, C), (self.off, L)):
                G = u.group.policy.G
                flags = [bool((self.hc_mask >> ((g * u.S) // per_agent)) & 1) for g in range(G)]
                u.group.hip_optimizer.freeze(flags, G)
                self._frozen[u.name] = torch.tensor([g for g in range(G) if flags[g]], dtype=torch.long, device=dev)
        if world_size > 1:
            self._broadcast_params()
        # A single net's item i takes word (i >> 6) & 1 of the draw countered by item i & ~64 (k_act_common's rule on
        # the call's group item index e * S + s), so a shard or part draws what one call over all replicas would
        # only when its first group item, (rank * E + e0) * S, is a multiple of 128. Otherwise the
        # streams stay independent but a split run no longer reproduces the unsplit one: say so.
        if world_size > 1 or rollout_streams > 1:
            per_group = [("acceptor", self.acc.S)] + ([] if self.free else [("offer", self.off.S)])
            if self.auct is not None:
                per_group.append(("auctioneer", C))
            for _, e0, _ in self.env.parts:
                for name, S in per_group:
                    if ((rank * self.E + e0) * S) % 128:
                        warnings.warn("%s draws of replicas from %d differ from an unsplit run's: (rank * E + e0) * %d "
                                      "is not a multiple of 128" % (name, rank * self.E + e0, S))
        # observation ring: slot t holds the state acted on at round t; slot T the next state. With
        # compact (and common_rows) the acceptor observations are kept as the env emits them
        # compactly: the owner row of every core + the owners (C rows per replica instead of N*C;
        # Agent.py:167-212), which the act and gradient kernels read directly
        self.compact = bool(compact and common_rows and s.acc_obs_stride >= 16)  # the common-row kernels' range
        if self.compact:
            self.acc_rows = torch.zeros((T + 1, self.E, C, s.acc_obs_stride), dtype=torch.int8, device=dev)
            self.acc_owner = torch.zeros((T + 1, self.E, C), dtype=torch.int8, device=dev)
            self.acc_obs = None
        else:
            self.acc_obs = torch.zeros((T + 1, self.E, N * C, s.acc_obs_stride), dtype=torch.int8, device=dev)
        # the offer rows' ring; readers outside the rollout and the fused update take the off_obs property
        self._off_obs = torch.zeros((T + 1, self.E, N * L, s.off_obs_stride), dtype=torch.int8, device=dev)
        # price chooser inputs [T][E][U][4] (unit-major: stored [U][T][E][4], self.price_obs its view)
        self.price_obs_um = None
        if self.free and self.price_unit_major:
            self.price_obs_um = torch.zeros((N * L, T, self.E, 4), dtype=torch.int8, device=dev)
            self.price_obs = self.price_obs_um.permute(1, 2, 0, 3)
        else:
            self.price_obs = torch.zeros((T, self.E, N * L, 4), dtype=torch.int8, device=dev) if self.free else None
        self.env_price = torch.zeros((self.E, N * L), dtype=torch.int8, device=dev)
        # the price chooser samples from a table of its few possible inputs, rebuilt from the current
        # weights at the start of every rollout (PriceTable; bit-identical to computing the net)
        self.price_table = PriceTable(cfg, self.price.group.policy_old) if (self.free and self.compact) else None
        # the acceptor row of a core the agent does not own (Agent.py:167-212): most acceptor rows
        # equal it, and the act / gradient kernels compute its network output once
        self.common_rows = common_rows
        O = s.max_offers
        crow = [0, -1, -1] + [-2] * (2 * O) + [0] * (s.acc_obs_stride - s.acc_obs_dim)
        self.acc_common = torch.tensor(crow, dtype=torch.int8, device=dev)
        # the acting nets' weight fragments (and the acceptors' common-row table), rebuilt at the start
        # of every rollout like the price table (ActFrag; bit-identical to acting without them)
        self.off_frag = ActFrag(self.off.group.policy_old, s.off_obs_stride)
        self.acc_frag = ActFrag(self.acc.group.policy_old, s.acc_obs_stride, self.acc_common)
        # the auctioneer's states are the compact acceptor rows with this ring as the owners: 1 where nobody owns
        # the core (derived from acc_owner by the round that acts on a slot and by the update)
        self.auct_frag = self.auct_owner0 = None
        if self.auct is not None:
            self.auct_frag = ActFrag(self.auct.group.policy_old, s.acc_obs_stride, self.acc_common)
            self.auct_owner0 = torch.zeros((T + 1, self.E, C), dtype=torch.int8, device=dev)
        self.agent_reward = torch.zeros((self.E, N), dtype=torch.int32, device=dev)
        self.auct_reward = torch.zeros((self.E, C), dtype=torch.int32, device=dev)
        self.rng = random.Random(seed)  # sub-unit draws (random.randint), identical on every rank
        self.rng_ctr = torch.zeros(1, dtype=torch.int64, device=dev)  # device Philox offset base
        self.use_graph = use_graph
        self.graph = None
        self.rounds_done = 0
        self._policy_version = 0  # bumped by update(); the acting tables record the version they saw
        self.iterations = 0
        for env, e0, e1 in self.env.parts:
            env.reset(dict(self._acc_out(0, e0, e1), offer=self._off_obs[0][e0:e1]))
        # episode metrics (trainPPO.py:153-226): the env kernel adds every round into per-replica
        # accumulators, slot (round // episodeLength) % slots; finished episodes are read after each
        # rollout (episode_log.py) and their slots zeroed before reuse
        self.ep_len = int(self.cfg.episode_length)
        self.metric_slots = -(-T // self.ep_len) + 1
        split = None if self.hardcoded is None else (lambda ep: evaluation.split_sides(ep, self.hardcoded))
        self._init_episode_log(metrics, [env for env, _, _ in self.env.parts], slots=self.metric_slots, hook=split,
                               episodeLength=self.ep_len, UPDATE_STEP=T, n_envs=self.E * world_size)
        self.metric_bufs = self._elog.bufs if metrics else None  # one per part; the captured rollouts hold them
        # the action log (action_log.py): per-episode counters with the episode log's slots; log_actions() fills
        # them from the rings after a rollout, outside the captured graphs (round0 changes from rollout to rollout)
        if action_tables and not action_log:
            raise ValueError("action_tables needs action_log=True")
        self.action_log = []
        self._alog = None
        self._actions_logged = 0  # rounds_done at the last log_actions()
        if action_log:
            self._alog = ActionLog(N, C, L, s, n_priorities(cfg), self.free, self.compact, action_tables,
                                   self.metric_slots, self.ep_len, dev, log=self.action_log)
            self.action_log_info = self._alog.info
        # one rank: each unit type's update on its own stream (MS_UPDATE_STREAMS=0: one stream). Round 4: the
        # update 10.06 -> 9.63 ms but the next rollout 14.50 -> 15.63 ms (every rollout launch slower after a
        # multi-stream update graph), so it was off. Round 6, with cfg3's rollout one launch: update 8.50 -> 8.05 ms,
        # rollout 9.99 -> 10.11 ms, iteration 18.50 -> 18.18 ms (profiles/r7b), so it is on
        self.update_streams = os.environ.get("MS_UPDATE_STREAMS", "1") == "1"
        # the fused env launches below add the episode metrics themselves (ABI 21), so metrics=True keeps them
        # (MS_ROLLOUT_METRICS=0, or an older library: metrics force an act launch and an env launch per round,
        # for A/B measurements and equality tests)
        fused_metrics_ok = self.metric_bufs is None or (ABI_LOADED >= 21 and
                                                        os.environ.get("MS_ROLLOUT_METRICS", "1") != "0")
        # fixed-price rounds with one net per role (cfg2): round t's env launch also samples round t + 1's
        # actions from the observations it just built (ms_env_step_act), so a round is one launch
        # (MS_ENV_FUSED_ACT=0: the act launch and the env launch of every round, for A/B measurements)
        # (T > 1: the fused acting writes round t + 1's ring slots)
        self.fused_step = (self.compact and not self.free and self.acc.group.policy.G == 1 and
                           self.off.group.policy.G == 1 and self.T > 1 and
                           os.environ.get("MS_ENV_FUSED_ACT", "1") != "0" and fused_metrics_ok and
                           all(env.fused_act_supported() for env, _, _ in self.env.parts))
        # a mixed market: the fused launches' mixed forms (ABI 24), else an act launch and step_mixed per round
        if self.hc_mask and not all(env.fused_mixed_supported() for env, _, _ in self.env.parts):
            self.fused_step = False
        # a learned auctioneer: the fused launches' forms with its acting (env_auct_kernels.hip), else launch pairs
        if self.auct is not None and not all(env.auct_supported() for env, _, _ in self.env.parts):
            self.fused_step = False
        # ... and the whole rollout's rounds are one launch (ms_env_rollout_act): each wave steps and acts
        # for its replicas round after round (MS_ENV_ROLLOUT=0: one launch per round, for A/B measurements)
        self.fused_rollout = self.fused_step and os.environ.get("MS_ENV_ROLLOUT", "1") != "0"
        # locally shared free-price rounds (cfg3): the whole rollout in one launch too (ms_env_rollout_act_free):
        # a workgroup steps its replicas, then acts for them with one wave per agent, round after round
        # (MS_ENV_ROLLOUT_FREE=0: an act launch and an env launch per round, for A/B measurements)
        self.fused_rollout_free = (self.compact and self.free and arch == "local" and self.price_table is not None and
                                   not self.price_unit_major and self.T > 1 and fused_metrics_ok and
                                   os.environ.get("MS_ENV_ROLLOUT_FREE", "1") != "0" and
                                   all(env.rollout_free_supported() for env, _, _ in self.env.parts))
        # ... and its acceptor items of cores their agent does not own (sampled from the common row's table; the env
        # reads only the owner's acceptor action) are left to a second kernel (ms_env_rollout_fill_common) after the
        # launch. (Running it inside the update instead, on the acceptor's stream beside the offer and price
        # gradients, measured even: 17.84-17.92 ms per iteration either way, profiles/r7.)
        self.rng_snap = torch.zeros(1, dtype=torch.int64, device=self.device)
        # the rollout's owned acceptor items by core ([T][E][C]; ABI 18): the fill then writes the acceptor rings'
        # rows whole (MS_FILL_OWN=0: the rollout writes them into the rings, one item in eight of a line)
        self.acc_own = None
        if self.fused_rollout_free and ABI_LOADED >= 18 and os.environ.get("MS_FILL_OWN", "1") != "0":
            self.acc_own = (torch.zeros((T, self.E, C), dtype=torch.int8, device=dev),
                            torch.zeros((T, self.E, C), dtype=torch.float32, device=dev))
        # the acceptor gradient regenerates the items the fill would write (ms_ppo_batch's regen fields, ABI 20):
        # the rollout always leaves them, iteration() never runs the fill, and whoever reads the acceptor rings
        # afterwards (acc.actions / acc.logprobs) gets them completed by one eager fill (_complete_rings).
        # One replica part only (the fill's arguments and the row base are one part's); any world size.
        # MS_ACC_REGEN=0: the fill after the rollout and a gradient that reads the rings (A/B runs, equality tests)
        self.acc_regen = (self.fused_rollout_free and self.acc_own is not None and self.fused and
                          rollout_streams == 1 and ABI_LOADED >= 20 and os.environ.get("MS_ACC_REGEN", "1") != "0")
        if self.acc_regen:
            self.acc.complete = self._complete_rings
        self._rings_pending = False
        # compact offer observations: a round's N * L offer rows are the replica's template with the slot's pair at
        # byte 2C, so the one-launch rollout writes the template and the pairs (off_tmpl / off_pair, 68 B per replica
        # and round at cfg3 instead of 480) and the offer gradient reads those. Only ring slots 0 (what reset, the
        # carry or a checkpoint wrote: compressed at the start of every rollout) and T (the last round writes its
        # rows as well) hold rows after a rollout; whoever reads off_obs gets slots 1..T-1 expanded by one eager
        # kernel first (_complete_offers). Under acc_regen's conditions.
        # MS_OFF_COMPACT=0: every round writes the rows and the gradient reads them (A/B runs, equality tests)
        self.off_compact = (self.fused_rollout_free and self.fused and rollout_streams == 1 and s.off_obs_dim > 4 and
                            all(has(n) for n in ("ms_env_rollout_act_free_compact", "ms_offer_compress",
                                                 "ms_offer_expand", "ms_ppo_grad_offer_compact")) and
                            os.environ.get("MS_OFF_COMPACT", "1") != "0")
        self.off_tmpl = self.off_pair = None
        if self.off_compact:
            self.off_tmpl = torch.zeros((T + 1, self.E, s.off_obs_stride), dtype=torch.int8, device=dev)
            self.off_pair = torch.zeros((T + 1, self.E, N * L), dtype=torch.int16, device=dev)
        self._offers_pending = False
        self._fill_args = []
        # update diagnostics (update_diagnostics): off unless asked for; the buffers are made at the first call
        self.diagnostics = int(diagnostics)
        if self.diagnostics < 0:
            raise ValueError("diagnostics must be >= 0")
        k = self.diagnostics
        self.diagnostics_slots = [((2 * i + 1) * T) // (2 * k) for i in range(min(k, T))]
        self.diagnostics_log = []
        self._diag = None         # unit name -> the kept device tensors
        self._diag_slot0 = None   # ring slot 0's observations as the rollout acted on them (the update's carry
                                  # overwrites the rings' slot 0): kept only when slot 0 is among the default slots
        self._diag_ready = False  # between an update() and the next rollout()
        self._last_draws = None   # the last update's sub-unit draws on the host
        self.span_every = 0  # > 0: every span_every-th round's env launches record their span (bench)
        self.spans = None
        self.timings = dict(rollout=0.0, update=0.0)

    @classmethod
    def from_named(cls, name: str, n_envs=None, update_step=200, seed=0, device=None, **kw):
        cfg = abi.named_config(name)
        arch = {"cfg1": "divided", "cfg2": "global", "cfg3": "local", "cfg4": "divided", "cfg5": "divided"}[name]
        hp = Hyper(update_step=update_step)
        if name == "cfg3":  # trainPPOExperiment4.py:96-98 (free prices): RAW_K 2, ACCEPTOR_GAMMA 0.95
            hp.raw_k_epochs = 2
            hp.acceptor_gamma = -((1 - 5) / 5) + 0.15
        return cls(cfg, n_envs or abi.NAMED_ENVS[name], arch=kw.pop("arch", arch), hyper=hp, seed=seed, device=device,
                   **kw)

    @property
    def off_obs(self):
        """The offer rows' ring [T + 1, E, N*L, stride], complete (after a compact rollout: slots 1..T-1 expanded)."""
        self._complete_offers()
        return self._off_obs

    def _complete_offers(self):
        """The offer rows of ring slots 1..T-1 a compact rollout left out: one eager expansion of the compact rings
        at the first read after the rollout, never inside a capture (as _complete_rings)."""
        if self._offers_pending and not capturing():
            self._offers_pending = False
            if self.T > 1:
                offer_expand(self.off_tmpl[1:self.T], self.off_pair[1:self.T], self.off.D, self._off_obs[1:self.T])

    def _acc_out(self, t, e0, e1):
        """The env's acceptor observation outputs for ring slot t, replicas [e0, e1)."""
        if self.compact:
            return dict(core_rows=self.acc_rows[t][e0:e1], core_owner=self.acc_owner[t][e0:e1])
        return dict(acceptor=self.acc_obs[t][e0:e1])

    def acceptor_rows(self, t0: int = 0, t1: int | None = None):
        """The [t1 - t0, E, N*C, stride] acceptor rows of ring slots t0..t1-1 (regenerated from the
        compact form when the ring is compact)."""
        t1 = self.T + 1 if t1 is None else t1
        if not self.compact:
            return self.acc_obs[t0:t1]
        from .ppo import regen_acceptor_rows
        return regen_acceptor_rows(self.acc_rows[t0:t1], self.acc_owner[t0:t1], self.acc_common, self.N)

    # ---- distributed helpers
    def _allreduce(self, params):
        allreduce_mean_grads(params, self.world_size, self.pg)

    def _broadcast_params(self):
        broadcast_params([u.group for u in self.units()], self.pg)

    def units(self):
        return [u for u in (self.acc, self.off, self.price, self.auct) if u is not None]

    # ---- rollout
    def _prepare_acting(self):
        """The acting kernels' per-rollout tables from policy_old: the price chooser's table of its
        possible inputs and the act weight fragments (ms_act_prepare). They are rebuilt at the start
        of every rollout (inside the rollout graph) and by round() after an update changed
        policy_old (sync_old bumps _policy_version)."""
        self._complete_rings()  # a pending fill samples from the tables about to be rebuilt
        if self.price_table is not None:
            self.price_table.build(self.price.group.policy_old)
        self.off_frag.build(self.off.group.policy_old)
        self.acc_frag.build(self.acc.group.policy_old)
        if self.auct is not None:
            self.auct_frag.build(self.auct.group.policy_old)
        self._acting_version = self._policy_version

    def round(self, t: int):
        """getActionForAllAgents + env.step + saveRewards for round t of the iteration
        (trainPPO.py:160-167), part by part: part k's launches go to stream k."""
        if getattr(self, "_acting_version", -1) != self._policy_version:
            self._prepare_acting()
        self._complete_offers()  # (rows a compact rollout left out are not expanded over this round's later)
        for k in range(len(self.env.parts)):
            self._round_part(t, k)
        if self.off_compact:  # the round wrote rows: the compact rings the fused update reads follow them
            for slot in ((0, 1) if t == 0 else (t + 1,)):
                offer_compress(self._off_obs[slot], self.off.D, self.off_tmpl[slot], self.off_pair[slot])

    def _round_part(self, t: int, k: int):
        self._act_part(t, k)
        self._step_part(t, k)

    def _act_part(self, t: int, k: int):
        """getActionForAllAgents of round t for replica part k (on stream k)."""
        if self.fused_step and t > 0:
            return  # sampled by round t - 1's env launch (_step_part)
        if self.auct is not None:
            self._act_auct_part(t, k)
        env, e0, e1 = self.env.parts[k]
        st = self.streams[k]
        E, N, C, L = e1 - e0, self.N, self.C, self.L
        # one Philox key for every rank and part; the counter's row is global (replica_base = this
        # part's first replica in the whole job, rank-major), so a replica draws the same numbers on
        # any number of ranks or parts (when rank * E * units per group is a multiple of 128, ms_mlp_params)
        # offsets: static per round + the device counter (advanced per rollout)
        seed = self.seed * 7919
        rb = self.rank * self.E + e0
        base = 8 * t
        sl = lambda x: x[e0:e1]
        # per agent: offer units then acceptors (Agent.py:504-515); separate streams per unit type
        if self.free:
            # FreePriceOfferPPO.selectAction (PPOmodules.py:312-332): core chooser, then the price
            # chooser on [obs[2a:2a+2], obs[-2:]] or the dummy [-5,-5,-5,-5] when a == 0, one launch
            out = dict(core_action=sl(self.off.actions[t]), core_logprob=sl(self.off.logprobs[t]),
                       price_state=sl(self.price_obs[t]), price_action=sl(self.price.actions[t]),
                       price_logprob=sl(self.price.logprobs[t]), env_price=sl(self.env_price))
            pus = 0
            if self.price_unit_major:  # [U][E'] views of the [U][T][E] rings, units T*E rows apart
                out.update(price_state=self.price_obs_um[:, t, e0:e1], price_action=self.price.actions_um[:, t, e0:e1],
                           price_logprob=self.price.logprobs_um[:, t, e0:e1])
                pus = self.T * self.E
            if self.compact:  # the acceptors too, in the same launch
                act_round_free(self.off.group.policy_old, self.price.group.policy_old, sl(self._off_obs[t]),
                               self.acc.group.policy_old, sl(self.acc_rows[t]), sl(self.acc_owner[t]), self.acc_common,
                               C, seed, base + 1, base + 3, out, sl(self.acc.actions[t]), sl(self.acc.logprobs[t]),
                               offset_dev=self.rng_ctr, stream=st, price_table=self.price_table,
                               price_unit_stride=pus, core_frag=self.off_frag, acc_frag=self.acc_frag,
                               replica_base=rb)
            else:
                offer_act_free(self.off.group.policy_old, self.price.group.policy_old, sl(self._off_obs[t]), C, seed,
                               base + 1, out, offset_dev=self.rng_ctr, stream=st, price_unit_stride=pus,
                               core_frag=self.off_frag, replica_base=rb)
        elif self.compact and ABI_LOADED < 16:
            # (an older A/B library: no fixed-price act_round_free; the two launches)
            self.off.group.policy_old.act(sl(self._off_obs[t]), N * L, seed, base + 1, action=sl(self.off.actions[t]),
                                          logprob=sl(self.off.logprobs[t]), offset_dev=self.rng_ctr, stream=st,
                                          frag=self.off_frag, replica_base=rb)
            self.acc.group.policy_old.act_compact(sl(self.acc_rows[t]), sl(self.acc_owner[t]), N * C, seed, base + 3,
                                                  self.acc_common, action=sl(self.acc.actions[t]),
                                                  logprob=sl(self.acc.logprobs[t]), stream=st, offset_dev=self.rng_ctr,
                                                  frag=self.acc_frag, replica_base=rb)
        elif self.compact:
            # a fixed-price round: the offer units and the compact acceptors in one launch
            act_round_free(self.off.group.policy_old, None, sl(self._off_obs[t]), self.acc.group.policy_old,
                           sl(self.acc_rows[t]), sl(self.acc_owner[t]), self.acc_common, C, seed, base + 1, base + 3,
                           dict(core_action=sl(self.off.actions[t]), core_logprob=sl(self.off.logprobs[t])),
                           sl(self.acc.actions[t]), sl(self.acc.logprobs[t]), offset_dev=self.rng_ctr, stream=st,
                           core_frag=self.off_frag, acc_frag=self.acc_frag, replica_base=rb)
        else:
            self.off.group.policy_old.act(sl(self._off_obs[t]), N * L, seed, base + 1, action=sl(self.off.actions[t]),
                                          logprob=sl(self.off.logprobs[t]), offset_dev=self.rng_ctr, stream=st,
                                          frag=self.off_frag, replica_base=rb)
        if not self.compact:  # (compact acceptors acted above, in the offers' launch)
            self.acc.group.policy_old.act(sl(self.acc_obs[t]), N * C, seed, base + 3, action=sl(self.acc.actions[t]),
                                          logprob=sl(self.acc.logprobs[t]), offset_dev=self.rng_ctr,
                                          common_row=self.acc_common if self.common_rows else None, stream=st,
                                          frag=self.acc_frag, replica_base=rb)

    def _act_auct_part(self, t: int, k: int):
        """The auctioneer's actions of round t for replica part k (on stream k): its net on the auctioneer rows,
        which are the compact acceptor rows with "nobody owns the core" as the owner, at Philox offset 8 t + 5
        (rounds use + 1 for the offer units and + 3 for the acceptors)."""
        e0, e1 = self.env.parts[k][1:]
        st = self.streams[k]
        own0 = self.auct_owner0[t][e0:e1]
        with torch.cuda.stream(st if st is not None else torch.cuda.current_stream(self.device)):
            torch.eq(self.acc_owner[t][e0:e1], 0, out=own0)
        self.auct.group.policy_old.act_compact(self.acc_rows[t][e0:e1], own0, self.C, self.seed * 7919, 8 * t + 5,
                                               self.acc_common, action=self.auct.actions[t][e0:e1],
                                               logprob=self.auct.logprobs[t][e0:e1], stream=st,
                                               offset_dev=self.rng_ctr, frag=self.auct_frag,
                                               replica_base=self.rank * self.E + e0)

    def _fused_next_auct(self, t: int, k: int):
        """Round t's acting of the auctioneer (_act_auct_part) for replica part k, as the acting fused into round
        t - 1's env launch beside _fused_next's."""
        e0, e1 = self.env.parts[k][1:]
        rb = self.rank * self.E + e0
        return abi.MsFusedActAuct(self.auct.group.policy_old.mlp_params(self.auct_frag, rb * self.C), 8 * t + 5,
                                  ptr(self.auct.actions[t][e0:e1]), ptr(self.auct.logprobs[t][e0:e1]))

    def _step_part(self, t: int, k: int):
        """env.step + saveRewards of round t for replica part k (on stream k)."""
        env, e0, e1 = self.env.parts[k]
        st = self.streams[k]
        E, N, C, L = e1 - e0, self.N, self.C, self.L
        sl = lambda x: x[e0:e1]
        obs = dict(self._acc_out(t + 1, e0, e1), offer=sl(self._off_obs[t + 1]))
        rew = dict(offer=sl(self.off.rewards[t]).view(E, N, L), acceptor=sl(self.acc.rewards[t]).view(E, N, C),
                   agent=sl(self.agent_reward), auctioneer=sl(self.auct_reward),
                   price=sl(self.price.rewards[t]).view(E, N, L) if self.free else None)
        ev = dict(launch_span=self.spans[t // self.span_every, k]) if self.span_every and t % self.span_every == 0 else None
        if self._elog is not None:
            ev = dict(ev or {}, metrics=self._elog.bufs[k])
        nxt = self._fused_next(t + 1, k) if self.fused_step and t + 1 < self.T else None
        if self.auct is not None:  # the round plays the auctioneer ring's slot and writes its per-core rewards
            rew["auctioneer"] = sl(self.auct.rewards[t])
            acc_t, off_t = sl(self.acc.actions[t]).view(E, N, C), sl(self.off.actions[t]).view(E, N, L)
            if nxt is not None:
                env.step_act_auct(acc_t, off_t, sl(self.auct.actions[t]), nxt, self._fused_next_auct(t + 1, k), obs, rew,
                                  events=ev, stream=st)
            else:
                env.step(acc_t, off_t, auctioneer=sl(self.auct.actions[t]), obs=obs, rewards=rew, events=ev, stream=st)
            return
        if self.hc_mask:  # a mixed market: the ring slot receives what the masked agents played
            acc_t, off_t = sl(self.acc.actions[t]).view(E, N, C), sl(self.off.actions[t]).view(E, N, L)
            if nxt is not None:
                env.step(acc_t, off_t, obs=obs, rewards=rew, events=ev, stream=st, next_act=nxt, hardcoded=self.hc_mask)
            else:
                env.step_mixed(acc_t, off_t, self.hc_mask, obs=obs, rewards=rew, events=ev, stream=st,
                               taken=dict(acceptor=acc_t, offer_core=off_t))
            return
        env.step(sl(self.acc.actions[t]).view(E, N, C), sl(self.off.actions[t]).view(E, N, L),
                 sl(self.env_price).view(E, N, L) if self.free else None, obs=obs, rewards=rew, events=ev, stream=st,
                 next_act=nxt, hardcoded=self._empty_mask)

    def _fused_next(self, t: int, k: int):
        """Round t's getActionForAllAgents (the fixed-price pair of _act_part) for replica part k, as the
        acting fused into round t - 1's env launch."""
        e0, e1 = self.env.parts[k][1:]
        sl = lambda x: x[e0:e1]
        N, C, L = self.N, self.C, self.L
        seed, base, rb = self.seed * 7919, 8 * t, self.rank * self.E + e0
        return abi.MsFusedAct(self.off.group.policy_old.mlp_params(self.off_frag, rb * N * L),
                              self.acc.group.policy_old.mlp_params(self.acc_frag, rb * N * C), ptr(self.acc_common),
                              seed, base + 1, base + 3, ptr(self.rng_ctr), ptr(sl(self.off.actions[t])),
                              ptr(sl(self.off.logprobs[t])), ptr(sl(self.acc.actions[t])), ptr(sl(self.acc.logprobs[t])))

    def _rollout_part(self, k: int):
        """Rounds 0..T-1 of replica part k (env.step + saveRewards, and the acting of rounds 1..T-1) in
        one launch (ms_env_rollout_act); round 0's acting ran before it (_act_part)."""
        env, e0, e1 = self.env.parts[k]
        E, N, C, L = e1 - e0, self.N, self.C, self.L
        sl = lambda x: x[e0:e1]
        obs = dict(self._acc_out(1, e0, e1), offer=sl(self._off_obs[1]))
        rew = dict(offer=sl(self.off.rewards[0]).view(E, N, L), acceptor=sl(self.acc.rewards[0]).view(E, N, C),
                   agent=sl(self.agent_reward), auctioneer=sl(self.auct_reward))
        ev = dict(launch_span=self.spans[0, k]) if self.span_every else None
        if self._elog is not None:  # every round adds into the slot of its own episode (not strided)
            ev = dict(ev or {}, metrics=self._elog.bufs[k])
        b = lambda x: x.stride(0) * x.element_size()  # bytes between ring slots t and t + 1
        strides = abi.MsRoundStrides(b(self.acc.actions), b(self.off.actions), b(self.acc_rows), b(self.acc_owner),
                                     b(self._off_obs), b(self.off.rewards), b(self.acc.rewards), 0, 0,
                                     b(self.off.actions), b(self.off.logprobs), b(self.acc.actions),
                                     b(self.acc.logprobs), 8)
        if self.auct is not None:  # (ms_env_rollout_act_auct) the auctioneer ring is played and written
            au = self.auct
            rew["auctioneer"] = sl(au.rewards[0])
            strides.auctioneer_reward = b(au.rewards)
            astrides = abi.MsRoundStridesAuct(b(au.actions), b(au.actions), b(au.logprobs))
            env.rollout_act_auct(sl(self.acc.actions[0]).view(E, N, C), sl(self.off.actions[0]).view(E, N, L),
                                 sl(au.actions[0]), obs, rew, self._fused_next(1, k), self._fused_next_auct(1, k),
                                 strides, astrides, self.T, act_after_last=False, events=ev, stream=self.streams[k],
                                 next_out=dict(auct_action=sl(au.actions[1]), auct_logprob=sl(au.logprobs[1])))
            return
        env.rollout_act(sl(self.acc.actions[0]).view(E, N, C), sl(self.off.actions[0]).view(E, N, L), obs, rew,
                        self._fused_next(1, k), strides, self.T, act_after_last=False, events=ev,
                        stream=self.streams[k], hardcoded=self.hc_mask or self._empty_mask)

    def _fused_next_free(self, t: int, k: int):
        """Round t's acting of a locally shared free-price round (act_round_free of _act_part) for replica part k,
        fused into round t - 1 of the one-launch rollout: (abi.MsFusedActFree, its output tensors)."""
        e0, e1 = self.env.parts[k][1:]
        sl = lambda x: x[e0:e1]
        N, C, L = self.N, self.C, self.L
        seed, base, rb = self.seed * 7919, 8 * t, self.rank * self.E + e0
        out = dict(core_action=sl(self.off.actions[t]), core_logprob=sl(self.off.logprobs[t]),
                   price_state=sl(self.price_obs[t]), price_action=sl(self.price.actions[t]),
                   price_logprob=sl(self.price.logprobs[t]), env_price=sl(self.env_price),
                   acc_action=sl(self.acc.actions[t]), acc_logprob=sl(self.acc.logprobs[t]))
        names = ("core_action", "core_logprob", "price_state", "price_action", "price_logprob", "env_price",
                 "acc_action", "acc_logprob")
        nxt = abi.MsFusedActFree(self.off.group.policy_old.mlp_params(self.off_frag, rb * N * L),
                                 self.price.group.policy_old.mlp_params(),
                                 self.acc.group.policy_old.mlp_params(self.acc_frag, rb * N * C), ptr(self.acc_common),
                                 ct.addressof(self.price_table.struct), seed, base + 1, base + 3, ptr(self.rng_ctr),
                                 *[ptr(out[n]) for n in names])
        if self.acc_own is not None:
            out.update(own_action=sl(self.acc_own[0][t]), own_logprob=sl(self.acc_own[1][t]))
            nxt.own_action, nxt.own_logprob = ptr(out["own_action"]), ptr(out["own_logprob"])
        return nxt, out

    def _rollout_part_free(self, k: int):
        """Rounds 0..T-1 of replica part k of a locally shared free-price rollout (env.step + saveRewards, and the
        acting of rounds 1..T-1) in one launch (ms_env_rollout_act_free); round 0's acting ran before it."""
        env, e0, e1 = self.env.parts[k]
        E, N, C, L = e1 - e0, self.N, self.C, self.L
        sl = lambda x: x[e0:e1]
        obs = dict(self._acc_out(1, e0, e1), offer=sl(self._off_obs[1]))
        rew = dict(offer=sl(self.off.rewards[0]).view(E, N, L), acceptor=sl(self.acc.rewards[0]).view(E, N, C),
                   agent=sl(self.agent_reward), auctioneer=sl(self.auct_reward),
                   price=sl(self.price.rewards[0]).view(E, N, L))
        ev = dict(launch_span=self.spans[0, k]) if self.span_every else None
        if self._elog is not None:
            ev = dict(ev or {}, metrics=self._elog.bufs[k])
        b = lambda x: x.stride(0) * x.element_size()  # bytes between ring slots t and t + 1
        strides = abi.MsRoundStridesFree(b(self.acc.actions), b(self.off.actions), b(self.acc_rows), b(self.acc_owner),
                                         b(self._off_obs), b(self.off.rewards), b(self.price.rewards),
                                         b(self.acc.rewards), 0, 0, b(self.off.actions), b(self.off.logprobs),
                                         b(self.price_obs), b(self.price.actions), b(self.price.logprobs),
                                         b(self.acc.actions), b(self.acc.logprobs), 8)
        if self.acc_own is not None:
            strides.next_own_action, strides.next_own_logprob = b(self.acc_own[0]), b(self.acc_own[1])
        nxt, out = self._fused_next_free(1, k)
        nxt.defer_common = int(self.acc_regen)
        compact = None
        if self.off_compact:  # (one part) slot 0 from the rows whoever wrote them left, slots 1..T by the launch
            offer_compress(self._off_obs[0], self.off.D, self.off_tmpl[0], self.off_pair[0], stream=self.streams[k])
            compact = (self.off_tmpl[1], self.off_pair[1], b(self.off_tmpl), b(self.off_pair))
        env.rollout_act_free(sl(self.acc.actions[0]).view(E, N, C), sl(self.off.actions[0]).view(E, N, L), obs, rew,
                             nxt, out, strides, self.T, act_after_last=False, events=ev, stream=self.streams[k],
                             compact=compact)
        if self.acc_regen:
            # the fill's arguments: the same call with the offsets of this rollout (snapshot). It reads the owners
            # of ring slots >= 1 (_carry_last_observation rewrites slot 0 only) and the acceptor tables of
            # this rollout (_prepare_acting completes pending rings before it rebuilds them)
            assert obs["core_owner"].data_ptr() == self.acc_owner[1][e0:e1].data_ptr() and self.T > 1
            fill = abi.MsFusedActFree.from_buffer_copy(nxt)
            fill.offset_dev = ptr(self.rng_snap)
            self._fill_args.append((env, obs, fill, strides))

    def fill_common(self, stream=None):
        """The deferred acceptor items of the last one-launch rollout (acc_regen; idempotent)."""
        for env, obs, fill, strides in self._fill_args:
            env.fill_common(obs, fill, strides, self.T, act_after_last=False, stream=stream)

    def _complete_rings(self):
        """The acceptor rings' items an iteration() left to the gradient's regeneration (acc_regen): one eager
        fill on the current stream at the first read after the rollout, never inside a capture."""
        if self._rings_pending and not capturing():
            self._rings_pending = False
            self.fill_common()

    def _acc_regen_args(self):
        """ms_ppo_batch's regen fields for the acceptor epochs (PPOGroup.fused_epoch): ring slot t of the last
        rollout acted with offset 8 t + 3 + the counter the rollout snapshot (_act_part / _fused_next_free), from
        the tables acc_frag holds until the next rollout rebuilds them; slot 0 (ms_act_round_free) is read."""
        T, E, C = self.T, self.E, self.C
        return dict(frag=self.acc_frag.buf, own_action=self.acc_own[0].view(T * E, C),
                    own_logprob=self.acc_own[1].view(T * E, C), seed=self.seed * 7919, offset=3, offset_step=8,
                    offset_dev=self.rng_snap, row_base=self.rank * self.E * self.N * C, slot0=1)

    def record_launch_spans(self, every: int):
        """Every `every`-th round's env launches record their span (first wave start, last wave end
        on the 100 MHz s_memrealtime clock, and each wave's shader-clock cycles) into self.spans
        [ceil(T / every)][parts][waves][4]; read with launch_spans_us() / launch_clock_mhz(). Set before the first
        rollout (the HIP graph captures it)."""
        self.span_every = int(every)
        w = self.env.parts[0][2] - self.env.parts[0][1]
        n = -(-self.T // self.span_every)  # row t // every holds round t's launches (t % every == 0)
        self.spans = torch.zeros((n, len(self.env.parts), w, 4), dtype=torch.int64, device=self.device)

    def sampled_spans(self):
        """The recorded rounds' spans ([ceil(T / span_every)][parts][waves][4], contiguous)."""
        return self.spans

    def launch_spans_us(self, sampled=None):
        """Durations (us) of the recorded env launches of the last rollout (fused_rollout: the one
        launch of each part over T, per round), or of `sampled` (a copy of sampled_spans())."""
        sp = (self.sampled_spans() if sampled is None else sampled).cpu().numpy()  # [rounds][parts][waves][4]
        if self.fused_rollout or self.fused_rollout_free:
            out = []
            for w in sp[0]:  # [parts][waves][4]: round 0's slot holds the launch
                w = w[w[:, 1] > 0]
                out.append(float(w[:, 1].max() - w[:, 0].min()) / 100.0 / self.T)
            return out
        out = []
        for r in range(sp.shape[0]):
            for k in range(sp.shape[1]):
                w = sp[r, k]
                w = w[w[:, 1] > 0]  # the waves of the launch
                out.append(float(w[:, 1].max() - w[:, 0].min()) / 100.0)
        return out

    def launch_clock_mhz(self, sampled=None):
        """Median shader clock (MHz) of the recorded env launches' waves: shader cycles over 100 MHz ticks."""
        sp = (self.sampled_spans() if sampled is None else sampled).cpu().numpy().reshape(-1, 4)
        sp = sp[(sp[:, 1] > sp[:, 0]) & (sp[:, 3] > sp[:, 2])]
        if len(sp) == 0:
            return None
        return float(np.median((sp[:, 3] - sp[:, 2]) / (sp[:, 1] - sp[:, 0]) * 100.0))

    def _rollout_body(self):
        cur = torch.cuda.current_stream(self.device)
        if self.span_every:
            self.spans.zero_()
        self._prepare_acting()
        self._fill_args = []
        if self.acc_regen:
            self.rng_snap.copy_(self.rng_ctr)
        for s in self.streams[1:]:  # fork: the side streams start after everything queued so far
            s.wait_stream(cur)
        if self.fused_rollout or self.fused_rollout_free:
            for k in range(len(self.env.parts)):
                self._act_part(0, k)
                (self._rollout_part_free if self.fused_rollout_free else self._rollout_part)(k)
        else:
            for t in range(self.T):
                self.round(t)
        for s in self.streams[1:]:  # join
            cur.wait_stream(s)
        self.rng_ctr.add_(8 * self.T)

    def rollout(self, defer_common: bool = False):
        """UPDATE_STEP rounds. With use_graph the first rollout runs eagerly and is then
        captured once into a HIP graph (every pointer is static); later rollouts replay it.
        defer_common (iteration(); acc_regen only): leave the pending acceptor rings to be completed at their
        first read (_complete_rings); otherwise the rings are complete when this returns."""
        self._rings_pending = False  # (rings of an earlier rollout nobody read: overwritten now)
        self._offers_pending = False
        self._diag_ready = False
        if 0 in self.diagnostics_slots:
            self._keep_slot0()
        if not self.use_graph:
            self._rollout_body()
        elif self.graph is None:
            self._rollout_body()
            torch.cuda.synchronize(self.device)
            g = torch.cuda.CUDAGraph()
            with hip_capture(g):
                self._rollout_body()
            self.graph = g
        else:
            self.graph.replay()
        if self.acc_regen:
            self._rings_pending = True
            if not defer_common:
                self._complete_rings()
        self._offers_pending = self.off_compact
        self.rounds_done += self.T

    # ---- action log
    def log_actions(self, harvest: bool = True):
        """The last rollout's actions into the action log's counters: eager launches on the current stream, reading
        the rings as the rollout left them (nothing is completed or expanded for it). Call it once after every
        rollout() and before update(), whose carry overwrites ring slot 0 of the observations (iteration() does);
        a second call for the same rollout, a call before the first rollout and a trainer without action_log do
        nothing. harvest: also read the episodes finished by now into self.action_log."""
        if self._alog is None or self._actions_logged == self.rounds_done:
            return
        T, N, C, L = self.T, self.N, self.C, self.L
        own = self.acc_owner[:T] if self.compact else None
        ring = self.acc.actions_raw
        if self._rings_pending:
            # the acceptor ring holds slot 0 only (ms_act_round_free wrote it whole); the owners' items of the later
            # rounds are by core in acc_own
            acceptor = [(0, 1, ring[:1], own[:1]), (1, T, self.acc_own[0][1:], own[1:])]
        else:
            acceptor = [(0, T, ring, own)]
        price = offer_key = price_key = None
        if self.free:
            price = self.price.actions_raw
        if self._alog.tables:
            if self.off_compact:  # the slot's (priority, remaining) pair: the priority is its first byte
                offer_key = self.off_pair.view(torch.int8).view(T + 1, self.E, N * L, 2)[:T, :, :, 0]
            else:
                offer_key = self._off_obs[:T, :, :, 2 * C]
            if self.free:
                price_key = self.price_obs[..., 2]
        self._alog.add(self.rounds_done - T, self.off.actions_raw, acceptor, price, offer_key, price_key)
        self._actions_logged = self.rounds_done
        if harvest:
            self._alog.harvest(self.rounds_done)

    def args_dict(self, replica="mean", params=None):
        """EpisodeLogging.args_dict; with action_log also Experiment 3's keys "0" .. str(L - 1): agent 0's mean
        offer action per slot and episode (metrics.action_args)."""
        d = super().args_dict(replica, params)
        if self._alog is not None:
            d.update(mx_action_args(self.action_log, 0, self.L))
        return d

    # ---- update
    def _draws(self, device=None):
        """Sub-unit selections, in the reference's random.randint order."""
        N, C, L, CS = self.N, self.C, self.L, self.hp.centralisation_sample
        dev = self.device if device is None else device
        if self.arch == "divided":
            sel = dict(acceptor=[torch.arange(N * C, device=dev)], offer=[torch.arange(N * L, device=dev)])
            host = dict(acceptor=[list(range(N * C))], offer=[list(range(N * L))])
        elif self.arch == "local":
            acc = [[0] * N for _ in range(CS)]
            off = [[0] * N for _ in range(CS)]
            for a in range(N):  # per agent: acceptor draws then offer draws (Agent.py:716-728)
                if (self.hc_mask >> a) & 1:
                    # a rule-based agent draws nothing; its frozen group's gradient runs on its first sub-unit
                    # and is discarded by the Adam step
                    for i in range(CS):
                        acc[i][a], off[i][a] = a * C, a * L
                    continue
                for i in range(CS):
                    acc[i][a] = a * C + self.rng.randint(0, C - 1)
                for j in range(CS):
                    off[j][a] = a * L + self.rng.randint(0, L - 1)
            sel = dict(acceptor=[torch.tensor(r, device=dev) for r in acc],
                       offer=[torch.tensor(r, device=dev) for r in off])
            host = dict(acceptor=[list(r) for r in acc], offer=[list(r) for r in off])
        else:
            acc, off = [], []
            host = dict(acceptor=[], offer=[])
            # a mixed market: the agent is drawn among the learned ones (their rows alone hold sampled actions)
            agent = (lambda: self.learned[self.rng.randint(0, len(self.learned) - 1)]) if self.hc_mask else \
                (lambda: self.rng.randint(0, N - 1))
            for _ in range(CS):  # SchedulingEnvironment.py:315-321
                a = agent()
                c = self.rng.randint(0, C - 1)
                acc.append(torch.tensor([a * C + c], device=dev))
                host["acceptor"].append([a * C + c])
            for _ in range(CS):  # SchedulingEnvironment.py:323-329
                a = agent()
                l = self.rng.randint(0, L - 1)
                off.append(torch.tensor([a * L + l], device=dev))
                host["offer"].append([a * L + l])
            sel = dict(acceptor=acc, offer=off)
        sel["price"] = sel["offer"]
        host["price"] = host["offer"]
        if getattr(self, "auct", None) is not None:  # the auctioneer's cores, after the agents' draws under every arch
            cores = [self.rng.randint(0, C - 1) for _ in range(CS)]
            sel["auctioneer"] = [torch.tensor([c], device=dev) for c in cores]
            host["auctioneer"] = [[c] for c in cores]
        self._last_draws = host  # (update_diagnostics reads the rows the update drew)
        return sel

    def update(self):
        """env.updateAgents() (SchedulingEnvironment.py:208-210 / 314-329, Agent.py:524-529,708-728).
        With use_graph the fused update is captured into HIP graphs after its first (eager) run and
        replayed from then on: only this iteration's sub-unit draws are copied to the device
        first. One rank: one graph. Several ranks: one graph per stretch between two gradient
        all-reduces, the RCCL calls eager in between (_capture_update). The returned losses are
        copies of the graph's own tensors."""
        self._policy_version += 1  # policy_old changes: round() rebuilds the acting tables
        if self.use_graph and self.fused:
            losses = self._update_graphed()
        else:
            sel = self._draws()
            if self.fused:
                losses = self._fused_update({k: torch.cat(v).to(torch.int32) for k, v in sel.items()},
                                            {k: [x.numel() for x in v] for k, v in sel.items()})
            else:
                losses = self._torch_update(sel)
        self._diag_ready = True  # until the next rollout() overwrites the rings
        return losses

    def _update_rows(self, u):
        """(states, actions, old log-probs) of unit type u for ms_ppo_grad: [T*E, U(, stride)] rows, or
        [U, T*E(, stride)] for a unit-major unit."""
        T, E = self.T, self.E
        if u.unit_major:
            st = self.price_obs_um if u is self.price else None
            return st.reshape(u.U, T * E, u.stride), u.actions_um.reshape(u.U, T * E), u.logprobs_um.reshape(u.U, T * E)
        if u is self.off and self.off_compact:  # (the fused update: the compact rings stand for the rows)
            return None, u.actions_raw.view(T * E, u.U), u.logprobs_raw.view(T * E, u.U)
        return (self._states_of(u).reshape(T * E, -1, u.stride), u.actions_raw.view(T * E, u.U),
                u.logprobs_raw.view(T * E, u.U))

    def _states_of(self, u):
        T = self.T
        if u is self.acc:
            return self.acc_rows[:T] if self.compact else self.acc_obs[:T]
        if u is self.auct:
            return self.acc_rows[:T]
        return (self.off_obs if u is self.off else self.price_obs)[:T]

    def _update_graphed(self):
        host = {k: [list(map(int, d.tolist())) for d in v] for k, v in self._draws(device="cpu").items()}
        names = [u.name for u in self.units()]
        flat = [x for k in names for d in host[k] for x in d]
        if getattr(self, "_sel_dev", None) is None:
            self._sel_host = torch.empty(len(flat), dtype=torch.int32, pin_memory=True)
            self._sel_dev = torch.empty(len(flat), dtype=torch.int32, device=self.device)
            self._sel_event = torch.cuda.Event()
            self._sel_counts = {k: [len(d) for d in host[k]] for k in names}
            self.update_graph = None
        self._sel_event.synchronize()  # the previous copy out of the pinned buffer is done
        self._sel_host.copy_(torch.tensor(flat, dtype=torch.int32))
        self._sel_dev.copy_(self._sel_host, non_blocking=True)
        self._sel_event.record()
        views, col = {}, 0
        for k in names:
            n = sum(self._sel_counts[k])
            views[k] = self._sel_dev[col:col + n]
            col += n
        if self.update_graph is None:
            losses = self._fused_update(views, self._sel_counts)  # this iteration's update
            eager_last = {u.name: (u.group.last_losses, u.group.last_terms) for u in self.units()}
            torch.cuda.synchronize(self.device)
            self._graph_losses = self._capture_update(views)
            self._graph_last = {u.name: list(u.group.last_losses) for u in self.units()}
            self._graph_terms = {u.name: u.group.last_terms for u in self.units()}
            for u in self.units():  # the eager run's own losses until the first replay
                u.group.last_losses, u.group.last_terms = eager_last[u.name]
            return losses
        self._replay_update()
        # the graph's loss tensors are overwritten by every replay: hand out copies (G floats per
        # unit type), so losses a caller keeps from earlier iterations stay what they were
        for u in self.units():
            u.group.last_losses = [x.clone() for x in self._graph_last[u.name]]
            u.group.last_terms = self._graph_terms[u.name]  # (the graph's own tensor: valid until the next replay)
        return {k: v.clone() for k, v in self._graph_losses.items()}

    def _capture_update(self, views):
        """Capture the fused update: segment i = the kernels between all-reduce i-1 and i (one
        segment on one rank), all in one memory pool. Returns the graph's loss tensors."""
        if self.world_size == 1 and self.update_streams:
            # MS_UPDATE_STREAMS on one rank: the per-unit-type streams are recorded into the graph
            # (fork / join on the capture stream), so replays run the same concurrent form the
            # eager first update ran
            g = torch.cuda.CUDAGraph()
            with hip_capture(g):
                losses = self._fused_update_streams(views, self._sel_counts)
            self.update_graph, self._graph_params = [g], []
            return losses
        out, graphs, params = {}, [], []
        phases = self._fused_phases(views, self._sel_counts, out)
        pool = None
        while True:
            g = torch.cuda.CUDAGraph()
            with hip_capture(g, pool=pool):
                p = next(phases, None)
            if pool is None:
                pool = g.pool()
            graphs.append(g)
            if p is None:
                break
            params.append(p)
        self.update_graph = graphs
        self._graph_params = params
        return out["losses"]

    def _replay_update(self):
        for i, g in enumerate(self.update_graph):
            g.replay()
            if i < len(self._graph_params):
                self._allreduce(self._graph_params[i])

    def _fused_update(self, all_sel, counts):
        """The fused update: all_sel[name] = int32 device [sum of draws' G] sub-units, counts[name]
        = each draw's number of groups."""
        if self.world_size == 1 and self.update_streams:
            return self._fused_update_streams(all_sel, counts)
        out = {}
        for params in self._fused_phases(all_sel, counts, out):
            self._allreduce(params)
        return out["losses"]

    def _fused_phases(self, all_sel, counts, out):
        """_fused_update as a generator: yields the parameters whose gradients the ranks all-reduce
        (several ranks only) and leaves the losses in out["losses"]."""
        losses = {}
        # Each unit type's draws update its nets in sequence (draw d trains on the weights draw d-1
        # left), but the unit types are independent nets: step s of the update = epoch k of draw d
        # of every unit type that has one, with ONE all-reduce of all their gradients (one
        # flattened RCCL call per step) before each type's Adam step.
        steps = {u.name: (u, self._epochs(u, all_sel[u.name], counts[u.name]), []) for u in self.units()}
        # each unit type's loss terms of every (draw, epoch) into one [n][G][3] buffer, combined once at the end
        terms = {name: torch.empty((len(seq), u.group.policy.G, 3), dtype=torch.float32, device=self.device)
                 for name, (u, seq, _) in steps.items()}
        for s in range(max(len(v[1]) for v in steps.values())):
            live = [(u, seq, ls) for u, seq, ls in steps.values() if s < len(seq)]
            for u, seq, ls in live:
                ls.append(seq[s].launch(terms[u.name][s]))
            if self.world_size > 1:
                yield [p for u, _, _ in live for p in u.group.policy.parameters()]
            for u, _, _ in live:
                u.group.hip_optimizer.step()
        for u, _, ls in steps.values():
            losses[u.name] = self._mask_losses(u, combine_losses(terms[u.name]))
            u.group.last_terms = terms[u.name]  # [draws * K][G][3] (a graph's own tensor under use_graph)
            u.group.last_losses = list(losses[u.name].unbind(0))
            u.group.sync_old()
        self._carry_last_observation()
        out["losses"] = losses

    def _epochs(self, u, sel_u, counts_u):
        """The gradient closures of unit type u's K epochs of every draw, in order."""
        T, E = self.T, self.E
        # the returns of every draw's sub-units in one launch: [T][E][sum of G], draw d at column
        # offset d*G (returns depend on the rewards only, not on earlier draws' updates)
        ret_all = unit_returns(u.rewards, sel_u, u.group.gamma)
        common = self.acc_common if (u is self.acc and self.common_rows) else None
        owner = self.acc_owner[:T].reshape(T * E, self.C) if (u is self.acc and self.compact) else None
        if u is self.auct:  # unit c (agent 0): core row c where the derived owner is 1, else the common row
            torch.eq(self.acc_owner[:T], 0, out=self.auct_owner0[:T])
            common, owner = self.acc_common, self.auct_owner0[:T].reshape(T * E, self.C)
        regen = self._acc_regen_args() if (u is self.acc and self.acc_regen) else None
        rows = self._update_rows(u)
        compact = None
        if u is self.off and self.off_compact:
            compact = (self.off_tmpl[:T].view(T * E, u.stride), self.off_pair[:T].view(T * E, u.U))
        col, seq = 0, []
        for n in counts_u:
            ep = u.group.fused_epoch(*rows, ret_all.view(-1)[col:], sel_u[col:col + n], T, E, common_row=common,
                                     returns_ld=sel_u.numel(), core_owner=owner, unit_major=u.unit_major, regen=regen,
                                     off_compact=compact)
            seq += [ep] * u.group.K
            col += n
        return seq

    def _fused_update_streams(self, all_sel, counts):
        """One rank: the unit types' nets are independent, so each type's whole update (its draws'
        epochs, each a gradient then an Adam step) runs on its own stream and the types' gradient
        kernels share the GPU (each is latency-bound at 2-3 waves per SIMD)."""
        cur = torch.cuda.current_stream(self.device)
        units = self.units()
        if getattr(self, "_unit_streams", None) is None:
            self._unit_streams = [torch.cuda.Stream(device=self.device) for _ in units]
        losses = {}
        for st in self._unit_streams:
            st.wait_stream(cur)
        for u, st in zip(units, self._unit_streams):
            with torch.cuda.stream(st):
                seq = self._epochs(u, all_sel[u.name], counts[u.name])
                # every (draw, epoch)'s loss terms into one buffer, combined at once (not four small kernels each)
                terms = torch.empty((len(seq), u.group.policy.G, 3), dtype=torch.float32, device=self.device)
                for i, ep in enumerate(seq):
                    ep.launch(terms[i])
                    u.group.hip_optimizer.step(st)
                losses[u.name] = self._mask_losses(u, combine_losses(terms))
                u.group.last_terms = terms  # [draws * K][G][3] (a graph's own tensor under use_graph)
                u.group.last_losses = list(losses[u.name].unbind(0))
                u.group.sync_old()
        for st in self._unit_streams:
            cur.wait_stream(st)
        self._carry_last_observation()
        return losses

    def _mask_losses(self, u, losses):
        """The frozen groups' entries of a unit type's [n][G] losses as NaN: their gradient ran on rows the rules
        played and was discarded."""
        idx = self._frozen.get(u.name)
        return losses if idx is None else losses.index_fill_(1, idx, float("nan"))

    def _torch_update(self, sel):
        """The torch-autograd update (the numerical reference of the fused one)."""
        T = self.T
        losses = {}
        for u in self.units():
            ls = []
            st_u = self.acceptor_rows(0, T) if (u is self.acc and self.compact) else self._states_of(u)
            if u is self.auct:
                from .ppo import regen_acceptor_rows
                st_u = regen_acceptor_rows(self.acc_rows[:T], (self.acc_owner[:T] == 0).to(torch.int8),
                                           self.acc_common, 1)
            for u_sel in sel[u.name]:
                x, a, lp, ret = u.batch(st_u, u_sel)
                ls += u.group.update(x, a, lp, ret)
            u.group.sync_old()
            losses[u.name] = torch.stack(ls)
        self._carry_last_observation()
        return losses

    def _carry_last_observation(self):
        """The next iteration starts from the last observation."""
        if self.compact:
            self.acc_rows[0].copy_(self.acc_rows[self.T])
            self.acc_owner[0].copy_(self.acc_owner[self.T])
        else:
            self.acc_obs[0].copy_(self.acc_obs[self.T])
        self._off_obs[0].copy_(self._off_obs[self.T])  # (compact: the next rollout compresses slot 0 again)

    # ---- update diagnostics
    def _keep_slot0(self):
        """Ring slot 0's observations before a rollout (eager copies, never inside a capture): the update's carry
        writes the last observation over them, and update_diagnostics may be asked for slot 0 (2 k > T)."""
        if self._diag_slot0 is None:
            src = dict(off=self._off_obs[0])
            if self.compact:
                src.update(acc_rows=self.acc_rows[0], acc_owner=self.acc_owner[0])
            else:
                src.update(acc_obs=self.acc_obs[0])
            self._diag_slot0 = {k: torch.empty_like(v) for k, v in src.items()}
        d = self._diag_slot0
        d["off"].copy_(self._off_obs[0])
        if self.compact:
            d["acc_rows"].copy_(self.acc_rows[0])
            d["acc_owner"].copy_(self.acc_owner[0])
        else:
            d["acc_obs"].copy_(self.acc_obs[0])

    def _diag_buffers(self, u, n_draws: int, n_slots: int):
        """The kept tensors of unit type u's diagnostics, [draws][slots][E][G] rows: made once per shape."""
        if self._diag is None:
            self._diag = {}
        b = self._diag.get(u.name)
        G = u.group.policy.G
        shape = (n_draws, n_slots, self.E, G)
        if b is None or b["act"].shape != shape:
            dev = self.device
            f32 = lambda: torch.empty(shape, dtype=torch.float32, device=dev)
            b = dict(obs=torch.zeros(shape + (u.stride,), dtype=torch.int8, device=dev),
                     act=torch.empty(shape, dtype=torch.int8, device=dev), old=f32(), new=f32(), val=f32(), ent=f32(),
                     sel=torch.empty((n_draws, G), dtype=torch.long, device=dev),
                     sel32=torch.empty((n_draws * G,), dtype=torch.int32, device=dev))
            self._diag[u.name] = b
        return b

    def diagnostics_bytes(self) -> int:
        """Bytes of the kept diagnostic tensors (0 before the first update_diagnostics)."""
        n = sum(t.numel() * t.element_size() for b in (self._diag or {}).values() for t in b.values())
        return n + sum(t.numel() * t.element_size() for t in (self._diag_slot0 or {}).values())

    @torch.no_grad()
    def update_diagnostics(self, slots=None) -> dict:
        """What the last update did to the policy, per unit type (acceptor, offer, and price under free prices) and
        group: legal after update() and before the next rollout() (RuntimeError otherwise: the rings it reads belong
        to the rollout the update consumed). For each group it takes the rows of every sub-unit the update drew for
        it (all centralisation_sample draws, a sub-unit drawn twice counted twice), at ring slots `slots` (default:
        diagnostics_slots), gathers them into explicit [rows][G][stride] rows (offer rows through off_obs, acceptor
        rows regenerated from the core rows, the owners and the common row, price rows from the price ring; actions
        and old log-probs through the completing accessors), evaluates the current `policy` on them with one
        evaluate_hip call per unit type (ms_policy_evaluate) and reduces in float64 on the device. With
        lr = new log-prob - old log-prob and Gt the normalised return the update trained on (unit_returns):
          approx_kl = mean(-lr); approx_kl_k3 = mean(exp(lr) - 1 - lr); clip_fraction = the share of rows with
          exp(lr) outside [1 - eps_clip, 1 + eps_clip]; ratio_max = max exp(lr); entropy = mean entropy;
          value_mse = mean((V - Gt)^2); explained_variance = 1 - var(Gt - V) / var(Gt) (population variances; NaN
          when var(Gt) == 0); rows = the number of rows reduced.
        Returns {unit name: {value name: [G] list}, "slots": [...]}; a group frozen by hardcoded_agents reports
        None. Several ranks: each rank reports its own rows. Slot 0 needs the copy a trainer with 0 among its
        diagnostics_slots keeps (ValueError otherwise). Every launch is eager on the current stream; nothing is
        drawn from self.rng, no Philox counter, ring slot the next iteration reads or captured graph changes. The
        results are not written into checkpoints."""
        if not self._diag_ready or self._last_draws is None:
            raise RuntimeError("update_diagnostics() is legal after update() and before the next rollout()")
        if capturing():
            raise RuntimeError("update_diagnostics() inside a stream capture")
        T, E, C = self.T, self.E, self.C
        slots = list(self.diagnostics_slots if slots is None else slots)
        if not slots or any(int(t) != t or not 0 <= t < T for t in slots):
            raise ValueError("slots must be ring slots in [0, %d)" % T)
        slots = [int(t) for t in slots]
        if 0 in slots and self._diag_slot0 is None:
            raise ValueError("ring slot 0 was overwritten by the update's carry: build the trainer with a "
                             "diagnostics value whose slots include 0")
        out = dict(slots=slots)
        eps = float(self.hp.eps_clip)
        dev = self.device
        gather = torch.ops.aten.index.Tensor_out  # x[idx] into a kept tensor
        i32 = torch.int32  # (rows move as dwords: every stride is a multiple of 4)
        slot_idx = torch.tensor(slots, dtype=torch.long, device=dev).view(1, -1, 1, 1)
        e_idx = torch.arange(E, device=dev).view(1, 1, E, 1)
        pending = []
        for u in self.units():
            draws = self._last_draws[u.name]
            G, n_d = u.group.policy.G, len(draws)
            b = self._diag_buffers(u, n_d, len(slots))
            b["sel"].copy_(torch.tensor(draws, dtype=torch.long))
            b["sel32"].copy_(b["sel"].view(-1))
            sel = b["sel"].view(n_d, 1, 1, G)
            idx = [slot_idx, e_idx, sel]  # [draws][slots][E][G]: ring slot, replica, the draw's sub-unit of the group
            actions, logprobs = u.actions, u.logprobs  # (completes the acceptor rings)
            ret_all = unit_returns(u.rewards, b["sel32"], u.group.gamma)  # [T][E][draws * G], as the update's
            if u is self.acc and self.compact:
                # unit a * C + c: core row c where agent a + 1 owns the core, else the common row
                core = (slot_idx, e_idx, sel % C)
                mine = (self.acc_owner[core] == (sel // C + 1).to(torch.int8)).unsqueeze(-1)
                torch.where(mine, self.acc_rows.view(i32)[core], self.acc_common.view(i32), out=b["obs"].view(i32))
            else:
                src = self.acc_obs if u is self.acc else (self.off_obs if u is self.off else self.price_obs)
                gather(src.view(i32), idx, out=b["obs"].view(i32))  # (off_obs completes the offer rows)
            if 0 in slots and u is not self.price:  # the rings' slot 0 holds the carried observation: the kept copy
                k0, i = self._diag_slot0, slots.index(0)
                for d in range(n_d):
                    if u is self.acc and self.compact:
                        c, a1 = b["sel"][d] % C, (b["sel"][d] // C + 1).to(torch.int8)
                        own = (k0["acc_owner"].index_select(1, c) == a1).unsqueeze(-1)
                        b["obs"][d, i].copy_(torch.where(own, k0["acc_rows"].index_select(1, c), self.acc_common))
                    else:
                        b["obs"][d, i].copy_(k0["acc_obs" if u is self.acc else "off"].index_select(1, b["sel"][d]))
            gather(actions, idx, out=b["act"])
            gather(logprobs, idx, out=b["old"])
            col = (torch.arange(n_d, device=dev) * G).view(n_d, 1, 1, 1) + torch.arange(G, device=dev).view(1, 1, 1, G)
            gt = ret_all[(slot_idx, e_idx, col)].view(-1, G).double()  # (a temporary, as ret_all itself)
            R = n_d * len(slots) * E
            u.group.policy.evaluate_hip(b["obs"].view(R, G, u.stride), b["act"].view(R, G), G, logprob=b["new"].view(R, G),
                                        value=b["val"].view(R, G), entropy=b["ent"].view(R, G))
            lr = b["new"].view(R, G).double() - b["old"].view(R, G).double()
            ratio = torch.exp(lr)
            v = b["val"].view(R, G).double()
            var_gt = gt.var(0, unbiased=False)
            pending.append((u, R, torch.stack([
                (-lr).mean(0), (ratio - 1.0 - lr).mean(0),
                ((ratio < 1.0 - eps) | (ratio > 1.0 + eps)).double().mean(0), ratio.max(0).values,
                b["ent"].view(R, G).double().mean(0), ((v - gt) ** 2).mean(0),
                torch.where(var_gt > 0, 1.0 - (gt - v).var(0, unbiased=False) / var_gt,
                            torch.full_like(var_gt, float("nan")))])))
        names = ("approx_kl", "approx_kl_k3", "clip_fraction", "ratio_max", "entropy", "value_mse", "explained_variance")
        for u, R, res in pending:  # (the first .tolist() waits for the device; every unit type is queued by then)
            res = res.tolist()
            G = u.group.policy.G
            frozen = set(self._frozen[u.name].tolist()) if u.name in self._frozen else set()
            vals = {n: [None if g in frozen else res[j][g] for g in range(G)] for j, n in enumerate(names)}
            vals["rows"] = [None if g in frozen else R for g in range(G)]
            out[u.name] = vals
        return out

    def iteration(self):
        """One PPO iteration; device time of rollout / update accumulates in self.timings (s)."""
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        ev[0].record()
        self.rollout(defer_common=True)
        ev[1].record()
        if self._alog is not None:
            # the action log reads the rings while they are the rollout's (the update's carry rewrites the
            # observations' slot 0), after the rollout's end event and before the update's start event: neither
            # span of `timings` sees it
            self.log_actions(harvest=False)
            ev.insert(2, torch.cuda.Event(enable_timing=True))
            ev[2].record()
        losses = self.update()
        ev[-1].record()
        self._pending_events.append(ev)
        self.iterations += 1
        if self.diagnostics:  # after the update's end event: the rollout and update spans do not see it
            self.diagnostics_log.append(self.update_diagnostics())
        if self._elog is not None:  # the episodes finished by now (trainPPO.py:200-226), into self.episode_log
            self._elog.harvest(self.rounds_done)
        if self._alog is not None:
            self._alog.harvest(self.rounds_done)
        return losses

    # ---- evaluation (evaluation.py)
    def eval_seed(self, n_envs: int | None = None) -> int:
        """Default base seed of evaluate()'s replicas: the training env's base seed of this rank (env_seed)
        plus 500_001, half the distance between two trainer seeds' ranges, so the evaluation replicas
        [base, base + n_envs) meet no training replica's job stream while world_size * E < 500_001."""
        return evaluation.eval_seed(self.seed, self.rank, int(n_envs or self.E))

    def evaluate(self, episodes: int = 1, n_envs: int | None = None, mode: str = "greedy", seed: int | None = None,
                 trace: bool = False, hardcoded_agents=None, action_log: bool = False,
                 action_tables: bool = False, auctioneer: str | None = None) -> dict:
        """Evaluate the current policy (policy_old, the nets the next rollout acts with) for `episodes` episodes
        of episode_length rounds on n_envs (default: E) fresh replicas of their own; replica e is seeded
        seed + e (default seed: eval_seed()). Training state is left untouched: the training env, the rings,
        the sub-unit and Philox counters, the episode log and the captured graphs are neither read nor written.

        mode "greedy": every unit takes the argmax of its actor's logits (no random number drawn);
        mode "sample": the units sample as in training, Philox key from `seed`;
        mode "hardcoded": the in-kernel HardcodedOfferer / HardcodedAcceptor agents, the reference's baseline
        (fixed prices only: ValueError under free prices).

        hardcoded_agents (an iterable of 0-based agent indices; modes "greedy" and "sample", fixed prices): a
        mixed population. The given agents play the reference's DividedHardcodedAgent rules inside the env
        kernel (BatchedEnv.step_mixed: on the env's stream, in ascending index, before the auctioneer) while the
        others act with the nets; the act launch still runs for every unit and the kernel overrides the given
        agents' rows. The result gains hardcoded_agents (the sorted indices) and, per entry of episodes,
        agentRew_hardcoded / agentRew_learned: the mean of the episode's replica-averaged agentRew over the given
        and over the other agents (None for an empty side). With trace, acceptor_action / offer_action are the
        actions the round used (the rules' picks in the given agents' rows), so a trace replays on a restatement
        or through step() once the rules' tie-break draws are made on the replaying env's stream.
        ValueError with mode "hardcoded", under free prices and for an index outside [0, N). None (the default)
        leaves the call and its result's keys as they are without the argument.

        action_log: the result gains action_log, a list with one entry per episode with the keys of
        Trainer(action_log=True)'s entries (action_log.py), counted round by round from the evaluation's own action
        tensors (with hardcoded_agents: from the actions the rounds used); acceptors by core owner where the
        buffers hold owners, else every unit. action_tables (needs action_log) adds the action-by-priority tables.
        ValueError with mode "hardcoded" (no action tensors exist there). The training log is not touched.

        auctioneer ("learned" or "hardcoded"; default: "learned" on a trainer with learned_auctioneer, else
        "hardcoded"): who sells the cores nobody owns. "learned": the trainer's auctioneer net acts on the emitted
        auctioneer rows every round, the argmax under "greedy" (act_greedy with the common row) and sampled at Philox
        offset 8 t + 5 under "sample"; "hardcoded": the in-kernel HardcodedAuctioneerAcceptor, with a learned
        auctioneer's trainer the baseline on the same job streams. ValueError for "learned" on a trainer without a
        learned auctioneer or with mode "hardcoded". The result's "auctioneer" records which one played; with trace
        and a learned auctioneer the rounds gain auctioneer (its rows) / auctioneer_action.

        Eager launches on the current stream (one act launch and one env round per round). Each call steps a
        newly created env (an env's reset re-emits observations; it does not rewind the world or its job
        stream), so equal arguments give equal results; the tensors are kept between calls, and the last env
        as self.eval_env. Several ranks: each evaluates its own replicas, no collective.
        Returns dict(mode, seed, n_envs, episodes=[metrics.reduce_replicas(ep), ...] (the argsDict values
        Plot.py reads, averaged over replicas), per_replica=[[dict per replica] per episode]); with trace also
        trace=[per round: the observations acted on and every action array fed to the env, CPU tensors]."""
        return evaluation.evaluate(self, episodes, n_envs, mode, seed, trace, hardcoded_agents, action_log,
                                   action_tables, auctioneer)

    # ---- checkpoints (checkpoint.py)
    def save_checkpoint(self, path: str) -> dict:
        """Everything a resumed run needs, in one file written atomically: nets, Adam state, counters, one packed
        env snapshot per replica part and (with metrics) the episode accumulators and log. Legal between
        iterations only (after iteration() or update()). Several ranks: a path per rank. Returns the save's
        timing split."""
        from . import checkpoint
        return checkpoint.save(self, path)

    def load_checkpoint(self, path: str) -> dict:
        """Resume from save_checkpoint's file, bit for bit: the trainer must have been built with the same
        arguments (ValueError naming the first differing manifest field; the trainer is left as it was). Works on
        a new trainer and on one that has already run. Returns the manifest."""
        from . import checkpoint
        self._diag_ready = False  # (the rings no longer belong to an update of this trainer's)
        return checkpoint.load(self, path)

    def load_policy(self, path: str) -> dict:
        """The nets only (policy and policy_old) from a checkpoint of any E, T, seed or world size with this
        trainer's shape terms, arch and price mode: evaluate() then runs the saved policy."""
        from . import checkpoint
        return checkpoint.load_policy(self, path)

    @property
    def timings(self):
        for ev in self._pending_events:
            ev[-1].synchronize()  # (with the action log: [rollout start, rollout end, update start, update end])
            self._timings["rollout"] += ev[0].elapsed_time(ev[1]) / 1e3
            self._timings["update"] += ev[-2].elapsed_time(ev[-1]) / 1e3
        self._pending_events = []
        return self._timings

    @timings.setter
    def timings(self, value):
        self._pending_events = []
        self._timings = dict(value)

    def flags(self):
        return self.env.flags()
