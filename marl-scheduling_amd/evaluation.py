"""``evaluate()`` of the three learners (Trainer, AggregatedTrainer, DQNTrainer): the argument checks, the seed, the
fresh env with its episode log, the loop over the rounds and the result dict, once; a learner hands over the acting
of a round as ``round_fn``. ``Trainer.evaluate``'s body lives here too (its method delegates, as to checkpoint.py).
"""
import numpy as np
import torch

from . import metrics as mx
from .action_log import ActionLog, n_priorities
from .env import BatchedEnv
from .episode_log import EpisodeLog
from .ppo import act_round_free, act_round_greedy, offer_act_free


def env_seed(seed: int, rank: int, n_envs: int) -> int:
    """Base seed of a rank's replicas: replica e of rank r is random.seed(base + e), so the ranks'
    job streams are disjoint for seeds up to 1000003 / world_size apart."""
    return seed * 1_000_003 + rank * n_envs


def eval_seed(seed: int, rank: int, n_envs: int) -> int:
    """Default base seed of evaluate()'s replicas: half the distance between two trainer seeds' ranges further."""
    return env_seed(seed, rank, n_envs) + 500_001


def agent_indices(given, n_agents: int) -> list:
    """hardcoded_agents as a sorted list of distinct agent indices: integral numbers in [0, N), no bool."""
    given = list(given)
    if any(isinstance(a, bool) or not isinstance(a, (int, np.integer, float, np.floating)) or a != int(a) or
           not 0 <= int(a) < n_agents for a in given):
        raise ValueError("hardcoded_agents must be agent indices in [0, %d)" % n_agents)
    return sorted({int(a) for a in given})


def split_sides(dicts: list, hardcoded: list):
    """agentRew_hardcoded / agentRew_learned of every dict (one per replica, or one per episode), in place."""
    for d in dicts:
        d["agentRew_hardcoded"], d["agentRew_learned"] = mx.split_agent_rew(d["agentRew"], hardcoded)


def check_evaluate_args(episodes, n_envs, default_envs: int, mode: str, modes: tuple):
    if mode not in modes:
        raise ValueError("mode must be one of %s" % ", ".join(repr(m) for m in modes))
    episodes, E = int(episodes), int(default_envs if n_envs is None else n_envs)
    if episodes < 1 or E < 1:
        raise ValueError("episodes and n_envs must be >= 1")
    return episodes, E


def fresh_env(tr, episodes, n_envs, mode: str, modes: tuple, seed, aggregated: bool = False):
    """The checked arguments and (episodes, seed, env, log): n_envs (default tr.E) new replicas seeded seed + e
    (default tr.eval_seed(n_envs)) and their episode log, a slot per episode."""
    episodes, E = check_evaluate_args(episodes, n_envs, tr.E, mode, modes)
    seed = tr.eval_seed(E) if seed is None else int(seed)
    env = BatchedEnv(tr.cfg, E, seed=seed, device=tr.device)
    return episodes, seed, env, EpisodeLog(env, slots=episodes, aggregated=aggregated)


def run_episodes(log: EpisodeLog, episodes: int, round_fn) -> list:
    """round_fn(t) acts and steps the env (events=log.events[0]) for each round t of `episodes` episodes;
    returns the harvested episodes (per-replica dicts)."""
    for t in range(episodes * log.ep_len):
        round_fn(t)
    log.harvest(episodes * log.ep_len)
    return log.episodes


def evaluation_result(mode: str, seed: int, n_envs: int, per_replica: list) -> dict:
    """evaluate()'s result from the harvested episodes."""
    return dict(mode=mode, seed=seed, n_envs=n_envs, episodes=[mx.reduce_replicas(ep) for ep in per_replica],
                per_replica=per_replica)


# ---- Trainer.evaluate
def _buffers(tr, E: int):
    """evaluate()'s observation / action / reward tensors for E replicas (kept between calls)."""
    cache = tr.__dict__.setdefault("_eval_cache", {})
    if E not in cache:
        s, dev, i8, N, C, L = tr.env.shape, tr.device, torch.int8, tr.N, tr.C, tr.L
        z = lambda *shape, dtype=i8: torch.zeros(shape, dtype=dtype, device=dev)
        b = dict(offer=z(E, N * L, s.off_obs_stride), acc_action=z(E, N * C), off_action=z(E, N * L),
                 acc_logprob=z(E, N * C, dtype=torch.float32), off_logprob=z(E, N * L, dtype=torch.float32))
        if tr.compact:
            b.update(core_rows=z(E, C, s.acc_obs_stride), core_owner=z(E, C))
        else:
            b.update(acceptor=z(E, N * C, s.acc_obs_stride))
        if tr.free:
            b.update(price_state=z(E, N * L, 4), price_action=z(E, N * L), env_price=z(E, N * L),
                     price_logprob=z(E, N * L, dtype=torch.float32))
        b["rewards"] = dict(offer=z(E, N, L, dtype=torch.float32), acceptor=z(E, N, C, dtype=torch.int32),
                            agent=z(E, N, dtype=torch.int32), auctioneer=z(E, C, dtype=torch.int32),
                            price=z(E, N, L, dtype=torch.float32) if tr.free else None)
        cache[E] = b
    return cache[E]


def _act(tr, b: dict, mode: str, t: int, philox_seed: int):
    """getActionForAllAgents of evaluation round t on the observations in b, with policy_old (the nets the
    next rollout acts with): greedy (argmax) or sampled picks, into b's action tensors."""
    N, C, L = tr.N, tr.C, tr.L
    off, acc = tr.off.group.policy_old, tr.acc.group.policy_old
    price = tr.price.group.policy_old if tr.free else None
    if mode == "greedy":
        if tr.compact:
            out = dict(core_action=b["off_action"])
            if tr.free:
                out.update(price_state=b["price_state"], price_action=b["price_action"], env_price=b["env_price"])
            act_round_greedy(off, price, b["offer"], acc, b["core_rows"], b["core_owner"], tr.acc_common, C,
                             out, b["acc_action"])
            return
        off.act_greedy(b["offer"], N * L, action=b["off_action"], logprob=b["off_logprob"])
        if tr.free:
            # FreePriceOfferPPO.selectAction (PPOmodules.py:312-332) on the greedy core action a:
            # [obs[2a], obs[2a+1], obs[2C], obs[2C+1]], or the dummy [-5, -5, -5, -5] when a == 0
            a = b["off_action"].long()
            idx = torch.stack([2 * a, 2 * a + 1, torch.full_like(a, 2 * C), torch.full_like(a, 2 * C + 1)], -1)
            st = torch.gather(b["offer"], 2, idx)
            b["price_state"].copy_(torch.where((a == 0).unsqueeze(-1), torch.full_like(st, -5), st))
            price.act_greedy(b["price_state"], N * L, action=b["price_action"], logprob=b["price_logprob"])
            b["env_price"].copy_(torch.where(a == 0, torch.full_like(b["price_action"], -5), b["price_action"]))
        acc.act_greedy(b["acceptor"], N * C, action=b["acc_action"], logprob=b["acc_logprob"])
        return
    # sampled picks: the training calls with the rounds' static Philox offsets (Trainer._act_part), no device counter
    base = 8 * t
    out = dict(core_action=b["off_action"], core_logprob=b["off_logprob"])
    if tr.free:
        out.update(price_state=b["price_state"], price_action=b["price_action"],
                   price_logprob=b["price_logprob"], env_price=b["env_price"])
    if tr.compact:
        act_round_free(off, price, b["offer"], acc, b["core_rows"], b["core_owner"], tr.acc_common, C,
                       philox_seed, base + 1, base + 3, out, b["acc_action"], b["acc_logprob"])
        return
    if tr.free:
        offer_act_free(off, price, b["offer"], C, philox_seed, base + 1, out)
    else:
        off.act(b["offer"], N * L, philox_seed, base + 1, action=b["off_action"], logprob=b["off_logprob"])
    acc.act(b["acceptor"], N * C, philox_seed, base + 3, action=b["acc_action"], logprob=b["acc_logprob"],
            common_row=tr.acc_common if tr.common_rows else None)


@torch.no_grad()
def evaluate(tr, episodes=1, n_envs=None, mode="greedy", seed=None, trace=False, hardcoded_agents=None,
             action_log=False, action_tables=False, auctioneer=None) -> dict:
    """Trainer.evaluate (its docstring is the contract)."""
    has_auct = getattr(tr, "auct", None) is not None
    if auctioneer is None:
        auctioneer = "learned" if (has_auct and mode != "hardcoded") else "hardcoded"
    if auctioneer not in ("learned", "hardcoded"):
        raise ValueError("auctioneer must be 'learned' or 'hardcoded'")
    if auctioneer == "learned" and not has_auct:
        raise ValueError("auctioneer='learned' needs a trainer built with learned_auctioneer=True")
    if auctioneer == "learned" and mode == "hardcoded":
        raise ValueError("auctioneer='learned' goes with mode 'greedy' or 'sample'")
    learned_auct = auctioneer == "learned"
    if action_tables and not action_log:
        raise ValueError("action_tables needs action_log=True")
    if action_log and mode == "hardcoded":
        raise ValueError("action_log counts action tensors, and mode 'hardcoded' has none")
    if tr.free and (mode == "hardcoded" or hardcoded_agents is not None):
        raise ValueError("the hard-coded agents act under fixed prices only")
    if mode == "hardcoded" and hardcoded_agents is not None:
        raise ValueError("hardcoded_agents selects agents of a learned population: mode 'greedy' or 'sample'")
    hc = None if hardcoded_agents is None else agent_indices(hardcoded_agents, tr.N)
    episodes, seed, env, log = fresh_env(tr, episodes, n_envs, mode, ("greedy", "sample", "hardcoded"), seed)
    tr.eval_env = env
    E, N, C, L = env.E, tr.N, tr.C, tr.L
    b = _buffers(tr, E)
    obs_keys = ("core_rows", "core_owner", "offer") if tr.compact else ("acceptor", "offer")
    if learned_auct:  # the auctioneer rows [E][C][stride] beside the agents' observations, and its actions
        if "auctioneer" not in b:
            st = tr.env.shape.acc_obs_stride
            b.update(auctioneer=torch.zeros((E, C, st), dtype=torch.int8, device=tr.device),
                     auct_action=torch.zeros((E, C), dtype=torch.int8, device=tr.device),
                     auct_logprob=torch.zeros((E, C), dtype=torch.float32, device=tr.device))
        obs_keys = obs_keys + ("auctioneer",)
    obs = env.reset({k: b[k] for k in obs_keys})
    philox_seed = (seed * 7919) & 0xFFFFFFFFFFFFFFFF
    rounds = []
    if hc is not None:  # the actions the rounds used (the rules' picks in the given agents' rows)
        taken = dict(acceptor=torch.empty_like(b["acc_action"]), offer_core=torch.empty_like(b["off_action"]))

    alog = None
    if action_log:  # counters of this call's own, a slot per episode
        alog = ActionLog(N, C, L, tr.env.shape, n_priorities(tr.cfg), tr.free, tr.compact, action_tables, episodes,
                         log.ep_len, tr.device)

    # a mixed round's actions exist only after its env step, which rewrites the observations in place: the owners
    # and the offer slots' priorities the round acted on are kept aside
    kept = None
    if alog is not None and hc is not None:
        kept = dict(owner=torch.empty_like(b["core_owner"]) if tr.compact else None,
                    offer_key=torch.empty_like(b["offer"][:, :, 2 * C], memory_format=torch.contiguous_format))

    def count_round(t):
        """Round t's actions into the action log."""
        if kept is None:  # before the env step: b holds what the round acted on
            acc, off, owner = b["acc_action"], b["off_action"], b["core_owner"] if tr.compact else None
            keys = dict(offer_key=b["offer"][:, :, 2 * C], price_key=b["price_state"][:, :, 2] if tr.free else None)
        else:
            acc, off, owner = taken["acceptor"], taken["offer_core"], kept["owner"]
            keys = dict(offer_key=kept["offer_key"])
        alog.add(t, off, [(0, 1, acc, owner)], b["price_action"] if tr.free else None,
                 **(keys if action_tables else {}))

    def one_round(t):
        acts = (None, None, None)
        if kept is not None:
            if kept["owner"] is not None:
                kept["owner"].copy_(b["core_owner"])
            kept["offer_key"].copy_(b["offer"][:, :, 2 * C])
        if mode != "hardcoded":
            _act(tr, b, mode, t, philox_seed)
            acts = (b["acc_action"].view(E, N, C), b["off_action"].view(E, N, L),
                    b["env_price"].view(E, N, L) if tr.free else None)
        auct_act = None
        if learned_auct:
            net = tr.auct.group.policy_old
            if mode == "greedy":
                net.act_greedy(b["auctioneer"], C, common_row=tr.acc_common, action=b["auct_action"],
                               logprob=b["auct_logprob"])
            else:
                net.act(b["auctioneer"], C, philox_seed, 8 * t + 5, action=b["auct_action"],
                        logprob=b["auct_logprob"], common_row=tr.acc_common)
            auct_act = b["auct_action"]
        if trace:
            rec = {k: b[k].cpu() for k in obs_keys}
            if mode != "hardcoded":
                rec.update(acceptor_action=b["acc_action"].cpu(), offer_action=b["off_action"].cpu())
                if learned_auct:
                    rec.update(auctioneer_action=b["auct_action"].cpu())
                if tr.free:
                    rec.update(price_state=b["price_state"].cpu(), price_action=b["price_action"].cpu(),
                               offer_price=b["env_price"].cpu())
            rounds.append(rec)
        if hc is None:
            if alog is not None:
                count_round(t)
            env.step(*acts, auctioneer=auct_act, obs=obs, rewards=b["rewards"], events=log.events[0])
            return
        env.step_mixed(acts[0], acts[1], hc, auctioneer=auct_act, obs=obs, rewards=b["rewards"], events=log.events[0], taken=taken)
        if alog is not None:
            count_round(t)
        if trace:
            rec.update(acceptor_action=taken["acceptor"].cpu(), offer_action=taken["offer_core"].cpu())

    res = evaluation_result(mode, seed, E, run_episodes(log, episodes, one_round))
    if has_auct or learned_auct:
        res["auctioneer"] = auctioneer
    if hc is not None:
        res["hardcoded_agents"] = hc
        split_sides(res["episodes"], hc)
    if alog is not None:
        alog.harvest(episodes * log.ep_len)
        res["action_log"] = alog.episodes
    return dict(res, trace=rounds) if trace else res
