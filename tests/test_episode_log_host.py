"""Host side of the one episode log (episode_log.EpisodeLog) and of evaluation.agent_indices. No device is
touched: the log runs on stub envs that hold only what it reads (cfg, E, N, C, L, device, metrics_buffer), and
the accumulator bytes are written through abi.metrics_dtype() with numbers distinct per replica and slot."""
import importlib

import numpy as np
import pytest
import torch

EP_LEN, SLOTS, PARTS, W = 3, 2, 2, 2  # episode_length, accumulator slots, replica parts, replicas per part


def _mod(name):
    return importlib.import_module("marl-scheduling_amd." + name)


class _Env:
    """What EpisodeLog reads of a BatchedEnv, at 4 agents x 4 cores x 3 offer slots."""
    device = "cpu"

    def __init__(self, abi, E):
        self.cfg = abi.MsConfig.from_buffer_copy(abi.named_config("cfg2"))
        self.cfg.episode_length = EP_LEN
        self.E, self.N, self.C, self.L = E, self.cfg.n_agents, self.cfg.n_cores, self.cfg.collection_length
        assert (self.N, self.C, self.L) == (4, 4, 3)

    def metrics_buffer(self, slots=1):
        return torch.zeros((slots, self.E, _mod("abi").METRICS_BYTES), dtype=torch.uint8)


def _fill(abi, bufs):
    """Every accumulator of replica e (counted over the parts in order) and slot s from v = 100 s + 10 e + 1."""
    e0 = 0
    for b in bufs:
        m = b.numpy().view(abi.metrics_dtype()).reshape(b.shape[:2])  # (shares the tensor's memory)
        for s in range(b.shape[0]):
            for e in range(b.shape[1]):
                v, r = 100 * s + 10 * (e0 + e) + 1, m[s, e]
                r["acceptor_reward"], r["offer_reward"], r["price_reward"] = v, v + 1, v + 0.5
                r["auctioneer_reward"], r["termination_revenue"], r["quality_sum"] = v + 2, v + 3, v + 0.25
                r["quality_rounds"], r["acception_amount"], r["rounds"] = 2, v + 4, EP_LEN
                r["price_sum"], r["price_count"] = v + np.arange(len(r["price_sum"])), 1
                r["dwell_sum"], r["dwell_count"] = v + 5 + np.arange(len(r["dwell_sum"])), 3
                r["agent_reward"] = v + 6 + np.arange(len(r["agent_reward"]))
        e0 += b.shape[1]


def _log(ms, parts=PARTS, **kw):
    envs = [_Env(ms.abi, PARTS * W // parts) for _ in range(parts)]
    log = _mod("episode_log").EpisodeLog(envs if parts > 1 else envs[0], slots=SLOTS, **kw)
    _fill(ms.abi, log.bufs)
    return log


def _same(a, b):
    if isinstance(a, dict):
        return isinstance(b, dict) and a.keys() == b.keys() and all(_same(a[k], b[k]) for k in a)
    if isinstance(a, list):
        return isinstance(b, list) and len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    if isinstance(a, np.ndarray):
        return isinstance(b, np.ndarray) and np.array_equal(a, b)
    return type(a) is type(b) and a == b


def _slot_values(ms, slot):
    """episode_values of the filled bytes of one slot, all replicas in order, by the restated route."""
    mx, env = _mod("metrics"), _Env(ms.abi, PARTS * W)
    buf = env.metrics_buffer(SLOTS)
    _fill(ms.abi, [buf])
    return mx.episode_values(mx.view(buf[slot].numpy()), env.cfg, EP_LEN, env.N, env.C, env.L)


def test_harvest_appends_the_finished_unread_episodes(ms):
    log = _log(ms)
    assert len(log.bufs) == PARTS and all(tuple(b.shape[:2]) == (SLOTS, W) for b in log.bufs)
    for rounds_done in (0, EP_LEN - 1, EP_LEN, EP_LEN, 2 * EP_LEN - 1, 2 * EP_LEN, 2 * EP_LEN):
        want = rounds_done // EP_LEN - len(log.episodes)
        assert log.harvest(rounds_done) == want and len(log.episodes) == rounds_done // EP_LEN
    assert _same(log.episodes, [_slot_values(ms, 0), _slot_values(ms, 1)])
    assert len(log.episodes[0]) == PARTS * W and log.episodes[0][3]["rounds"] == EP_LEN
    assert log.episodes[0][1]["acceptorRew"] != log.episodes[0][2]["acceptorRew"] != log.episodes[1][2]["acceptorRew"]


def test_two_parts_equal_one_part_over_the_concatenated_bytes(ms):
    two, one = _log(ms, parts=2), _log(ms, parts=1)
    assert torch.equal(torch.cat(two.bufs, dim=1), one.bufs[0]) and len(one.bufs) == 1
    assert two.harvest(2 * EP_LEN) == one.harvest(2 * EP_LEN) == 2
    assert _same(two.episodes, one.episodes)


def test_a_read_slot_is_zeroed_and_the_other_untouched(ms):
    log = _log(ms)
    before = [b.clone() for b in log.bufs]
    tensors = [b.data_ptr() for b in log.bufs]
    assert log.harvest(EP_LEN) == 1
    for b, was in zip(log.bufs, before):
        assert not b[0].any() and was[0].any() and torch.equal(b[1], was[1])
    assert [b.data_ptr() for b in log.bufs] == tensors


def test_a_refilled_list_moves_the_log(ms):
    """What a checkpoint load does: the learner's episode_log is the log's list, refilled in place."""
    holder = _mod("episode_log").EpisodeLogging()
    holder._init_episode_log(True, [_Env(ms.abi, W) for _ in range(PARTS)], slots=SLOTS, episodeLength=EP_LEN)
    log = holder._elog
    assert log.episodes is holder.episode_log
    _fill(ms.abi, log.bufs)
    saved = [_slot_values(ms, 0)]
    holder.episode_log[:] = saved
    slot0 = [b[0].clone() for b in log.bufs]
    assert log.harvest(EP_LEN) == 0 and log.harvest(2 * EP_LEN) == 1  # continues from len(saved): slot 1
    assert len(holder.episode_log) == 2 and _same(holder.episode_log[1], _slot_values(ms, 1))
    assert all(torch.equal(b[0], s) and not b[1].any() for b, s in zip(log.bufs, slot0))
    off = _mod("episode_log").EpisodeLogging()
    off._init_episode_log(False, [_Env(ms.abi, W)], slots=SLOTS)
    assert off._elog is None and off.episode_log == []


def test_the_hook_sees_each_episode_once(ms):
    seen = []

    def hook(ep):
        seen.append([d["acceptorRew"] for d in ep])
        for d in ep:
            d["mark"] = len(seen)

    log = _log(ms, hook=hook)
    assert log.harvest(EP_LEN) == 1 and log.harvest(2 * EP_LEN) == 1 and log.harvest(2 * EP_LEN) == 0
    assert seen == [[d["acceptorRew"] for d in _slot_values(ms, s)] for s in (0, 1)]
    assert [[d["mark"] for d in ep] for ep in log.episodes] == [[1] * (PARTS * W), [2] * (PARTS * W)]


def test_aggregated_sums_are_for_one_env(ms):
    el = _mod("episode_log")
    with pytest.raises(ValueError):
        el.EpisodeLog([_Env(ms.abi, W), _Env(ms.abi, W)], slots=SLOTS, aggregated=True)
    assert el.EpisodeLog([_Env(ms.abi, W)], slots=SLOTS, aggregated=True).agg.shape == (SLOTS, 2, W, 4)


def test_agent_indices(ms):
    ev, N = _mod("evaluation"), 4
    assert ev.agent_indices([2, 0, 2, 1.0], N) == [0, 1, 2]
    assert ev.agent_indices(range(N), N) == [0, 1, 2, 3] and ev.agent_indices([], N) == []
    assert ev.agent_indices([np.int64(3), np.float32(1.0)], N) == [1, 3]
    for bad in ([True], ["1"], [0.5], [-1], [N]):
        with pytest.raises(ValueError, match=r"hardcoded_agents must be agent indices in \[0, 4\)"):
            ev.agent_indices(bad, N)
