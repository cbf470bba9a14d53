"""The action log of ``Trainer`` and ``Trainer.evaluate`` (Experiment 3's "Handlungslogging", and the free-price
experiments' action-by-priority tables): per-episode integer counters on the device, filled by ``ppo.action_hist`` /
``ppo.action_table`` from the action tensors a rollout or a round wrote, and the finished episodes read from them.

An entry of the log is one episode, pooled over the replicas, a dict of int64 numpy arrays:
``offer [N][L][A_off]`` (every unit), ``price [N][L][A_price]`` (free prices; only where the offer unit's core action
is not 0: a price chooser's pick on the dummy state is no offer), ``acceptor [N][C][A_acc]`` (the owner's action of
every core where the learner holds core owners, else every acceptor unit) and ``bad`` (an int: bytes out of range,
never binned). With tables also ``offer_by_priority [N][P][A_off]`` (key: the slot's job priority),
``price_by_priority [N][P][A_price]`` (key: byte 2 of the price state) and ``skipped`` (a dict per table: the
elements whose key is no priority: empty and pad slots, the dummy state). P is the largest job priority + 1.

Slots follow ``EpisodeLog``: round r adds into slot (r // episode_length) % slots, and a slot is zeroed when its
episode is read. A call that spans an episode boundary is split there, one set of launches per episode, so that the
``bad`` / ``skipped`` counters (one number per launch) belong to one episode as the counts do.
"""
from __future__ import annotations

import numpy as np
import torch

from . import ppo

TABLES = ("offer", "price")


class ActionLog:
    def __init__(self, N: int, C: int, L: int, shape, n_priorities: int, free: bool, owners: bool, tables: bool,
                 slots: int, episode_length: int, device, log: list | None = None):
        self.N, self.C, self.L, self.P = N, C, L, int(n_priorities)
        self.free, self.owners, self.tables = bool(free), bool(owners), bool(tables)
        self.slots, self.ep_len = int(slots), int(episode_length)
        self.episodes = [] if log is None else log
        z = lambda *s: torch.zeros(s, dtype=torch.int64, device=device)
        self.counts = dict(offer=z(self.slots, N * L, shape.off_actions), acceptor=z(self.slots, N * C, shape.acc_actions))
        if self.free:
            self.counts["price"] = z(self.slots, N * L, shape.price_actions)
        self.bad = z(self.slots)
        self.skipped = {}
        if self.tables:
            self.counts["offer_by_priority"] = z(self.slots, N, self.P, shape.off_actions)
            self.skipped["offer"] = z(self.slots)
            if self.free:
                self.counts["price_by_priority"] = z(self.slots, N, self.P, shape.price_actions)
                self.skipped["price"] = z(self.slots)

    @property
    def info(self) -> dict:
        return dict(acceptor_selection="owner" if self.owners else "all", tables=self.tables, n_priorities=self.P)

    def _segments(self, round0: int, n_rounds: int):
        """(t0, t1, slot) of every episode the rounds round0 .. round0 + n_rounds - 1 touch."""
        t = 0
        while t < n_rounds:
            ep = (round0 + t) // self.ep_len
            t1 = min(n_rounds, (ep + 1) * self.ep_len - round0)
            yield t, t1, ep % self.slots
            t = t1

    def add(self, round0: int, offer, acceptor, price=None, offer_key=None, price_key=None):
        """The rounds round0 .. round0 + T - 1 into their episodes' counters (eager launches on the current stream).
        offer / price / offer_key / price_key: int8 [T, E, N*L] (or [E, N*L]: one round), strided views allowed.
        acceptor: a list of (t0, t1, actions, owner) covering the rounds: actions [t1 - t0, E, N*C] by unit or
        [t1 - t0, E, C] by core, owner [t1 - t0, E, C] or None (every unit is counted)."""
        r3 = lambda x: None if x is None else (x.unsqueeze(0) if x.dim() == 2 else x)
        offer, price, offer_key, price_key = r3(offer), r3(price), r3(offer_key), r3(price_key)
        T, L = offer.shape[0], self.L
        for t0, t1, slot in self._segments(int(round0), T):
            kw = dict(round0=int(round0) + t0, episode_length=self.ep_len, bad=self.bad[slot:slot + 1])
            ppo.action_hist(offer[t0:t1], self.counts["offer"], **kw)
            if self.free:
                ppo.action_hist(price[t0:t1], self.counts["price"], gate=offer[t0:t1], **kw)
            for a0, a1, actions, owner in acceptor:
                lo, hi = max(a0, t0), min(a1, t1)
                if lo >= hi:
                    continue
                akw = dict(kw, round0=int(round0) + lo)
                actions, owner = r3(actions)[lo - a0:hi - a0], r3(owner)
                if owner is None:
                    ppo.action_hist(actions, self.counts["acceptor"], **akw)
                else:
                    ppo.action_hist(actions, self.counts["acceptor"], owner=owner[lo - a0:hi - a0], n_agents=self.N,
                                    **akw)
            if self.tables:
                ppo.action_table(offer[t0:t1], offer_key[t0:t1], self.counts["offer_by_priority"], units_per_bin=L,
                                 skipped=self.skipped["offer"][slot:slot + 1], **kw)
                if self.free:
                    ppo.action_table(price[t0:t1], price_key[t0:t1], self.counts["price_by_priority"],
                                     units_per_bin=L, skipped=self.skipped["price"][slot:slot + 1], **kw)

    def _read(self, slot: int) -> dict:
        N, C, L = self.N, self.C, self.L
        take = lambda x: x[slot].cpu().numpy().copy()
        ep = dict(offer=take(self.counts["offer"]).reshape(N, L, -1))
        if self.free:
            ep["price"] = take(self.counts["price"]).reshape(N, L, -1)
        ep["acceptor"] = take(self.counts["acceptor"]).reshape(N, C, -1)
        ep["bad"] = int(self.bad[slot])
        if self.tables:
            for name in TABLES:
                if name + "_by_priority" in self.counts:
                    ep[name + "_by_priority"] = take(self.counts[name + "_by_priority"])
            ep["skipped"] = {k: int(v[slot]) for k, v in self.skipped.items()}
        for x in list(self.counts.values()) + [self.bad] + list(self.skipped.values()):
            x[slot].zero_()
        return ep

    def harvest(self, rounds_done: int) -> int:
        """Append every episode finished after rounds_done rounds and not read yet; returns their number."""
        n = 0
        while len(self.episodes) < int(rounds_done) // self.ep_len:
            self.episodes.append(self._read(len(self.episodes) % self.slots))
            n += 1
        return n

    # ---- checkpoints: the open slots' counters (the log list is the owner's)
    def state(self) -> dict:
        return dict(counts={k: v.cpu() for k, v in self.counts.items()}, bad=self.bad.cpu(),
                    skipped={k: v.cpu() for k, v in self.skipped.items()})

    def load_state(self, state: dict):
        if set(state["counts"]) != set(self.counts) or set(state["skipped"]) != set(self.skipped):
            raise ValueError("checkpoint does not fit: action_log counters %s, the trainer's %s" % (
                sorted(state["counts"]), sorted(self.counts)))
        for k, v in self.counts.items():
            if tuple(v.shape) != tuple(state["counts"][k].shape):
                raise ValueError("checkpoint does not fit: action_log counter %s is %s, the trainer's %s" % (
                    k, tuple(state["counts"][k].shape), tuple(v.shape)))
        for k, v in self.counts.items():
            v.copy_(state["counts"][k])
        self.bad.copy_(state["bad"])
        for k, v in self.skipped.items():
            v.copy_(state["skipped"][k])


def n_priorities(cfg) -> int:
    """P of the tables: the largest job priority + 1 (key_min is 0: the empty and pad slots' -1 / -2 and the dummy
    state's -5 are skipped)."""
    return max(cfg.job_priority[: cfg.n_kinds]) + 1


def equal_logs(a: list, b: list) -> bool:
    """Whether two action logs hold the same episodes, entry by entry (arrays by value)."""
    def eq(x, y):
        if isinstance(x, dict):
            return isinstance(y, dict) and x.keys() == y.keys() and all(eq(x[k], y[k]) for k in x)
        if isinstance(x, np.ndarray) or isinstance(y, np.ndarray):
            return np.array_equal(np.asarray(x), np.asarray(y))
        return x == y
    return len(a) == len(b) and all(eq(x, y) for x, y in zip(a, b))
