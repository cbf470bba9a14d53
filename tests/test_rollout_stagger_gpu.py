"""MS_FREE_STAGGER: the two workgroups of a CU told apart in the one-launch free-price rollout
(k_env_rollout_act_free's STAG kernels, env_kernels.hip; the default, and what every value but 0 selects).

A workgroup's rank on its CU (the parity of a ticket it takes once per launch) changes only when it runs: the issue
priorities of the two phases, by rank and clock slice. No workgroup reads what another
wrote, so every value must give the bytes of MS_FREE_STAGGER=0: every ring, the owned acceptor items, the losses,
the weights, the exported env state and the flags, over two iterations of a fresh trainer. The variable is read at
every launch (and kept by a captured launch), so each trainer lives inside its own setting.

The shapes: three workgroups (CUs with one workgroup, whose rank meets no partner), a partial last workgroup, more
workgroups than the device holds at once (late arrivals take tickets on CUs that already gave two), the DynShape
kernel, the metrics kernel, and a launch of one round, which has no acting at all.
The reference of a case is computed once and shared by its modes."""
import ctypes as ct
import importlib

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

MODES = (1, 2, 3, 4, 5)  # (once five modes, now five spellings of "not 0": each must select the staggered kernels)


def _mod(name):
    return importlib.import_module("marl-scheduling_amd." + name)


def _tickets():
    f = _mod("_lib").lib.ms_free_stagger_tickets
    f.restype = ct.c_longlong
    n = f()
    assert n >= 0
    return n


def _mk_cfg3(E, T, **kw):
    return lambda: _mod("trainer").Trainer.from_named("cfg3", n_envs=E, update_step=T, seed=13, device="cuda:0", **kw)


def _mk_dyn(E, T):
    def mk():
        abi, tr_mod = _mod("abi"), _mod("trainer")
        cfg = abi.make_config(6, 6, 3, free_prices=True, commercial=True, **abi.EXP4_JOBS)
        return tr_mod.Trainer(cfg, E, arch="local", hyper=tr_mod.Hyper(update_step=T, raw_k_epochs=2), seed=4,
                              device="cuda:0")
    return mk


CASES = {
    "three_workgroups": _mk_cfg3(96, 8),
    "partial_last_workgroup": _mk_cfg3(1001, 8),
    "late_arrivals": _mk_cfg3(32 * 515, 4),
    "dynshape_6x6x3": _mk_dyn(200, 8),
    "metrics": _mk_cfg3(96, 8, metrics=True, episode_length=7),
}


def _snapshot(t, out, tag):
    rings = {"acc_rows": t.acc_rows, "acc_owner": t.acc_owner, "off_obs": t.off_obs, "env_price": t.env_price,
             "agent_reward": t.agent_reward, "auct_reward": t.auct_reward}
    if t.price_obs is not None:
        rings["price_obs"] = t.price_obs
    if t.acc_own is not None:
        rings["acc_own.action"], rings["acc_own.logprob"] = t.acc_own
    if t.metric_bufs is not None:
        rings["metrics"] = torch.cat(list(t.metric_bufs), dim=1)
    for u in t.units():
        for k in ("actions", "logprobs", "rewards"):
            rings["%s.%s" % (u.name, k)] = getattr(u, k)
    for k, v in rings.items():
        out["%s/%s" % (tag, k)] = v.detach().cpu().numpy().copy()


def _run(mk, iters=2):
    """Two iterations of a fresh trainer: {name: array} of everything the rollout and the update leave, and the
    number of workgroups of one rollout launch."""
    ppo = _mod("ppo")
    t = mk()
    assert t.fused_rollout_free and t.acc_own is not None
    out = {}
    for it in range(iters):
        t.rollout()
        torch.cuda.synchronize()
        _snapshot(t, out, "it%d" % it)
        for k, v in t.update().items():
            out["it%d/loss.%s" % (it, k)] = v.detach().cpu().numpy().copy()
    for u in t.units():
        for k in ppo.ACTOR_KEYS + ppo.CRITIC_KEYS:
            out["weights/%s.%s" % (u.name, k)] = getattr(u.group.policy, k).detach().cpu().numpy().copy()
    parts = [env.export_state() for env, _, _ in t.env.parts]
    for k in parts[0]:
        out["state/%s" % k] = np.concatenate([np.asarray(p[k]) for p in parts])
    out["flags"] = np.asarray(t.flags())
    wgs = sum(-(-(e1 - e0) // (4 * t.N)) for _, e0, e1 in t.env.parts)
    return out, wgs


def _assert_same(ref, got, what):
    assert ref.keys() == got.keys()
    for k in ref:
        a, b = ref[k], got[k]
        assert a.shape == b.shape and a.dtype == b.dtype, (what, k)
        same = a.view(np.uint8) == b.view(np.uint8) if a.dtype.kind == "f" else a == b
        assert bool(np.all(same)), (what, k, int(np.sum(~same)), a.size)
    assert int(ref["flags"]) == 0


_reference = {}


def _ref(monkeypatch, case):
    if case not in _reference:
        monkeypatch.setenv("MS_FREE_STAGGER", "0")
        n0 = _tickets()
        _reference[case] = _run(CASES[case])[0]
        assert _tickets() == n0  # mode 0 takes no ticket
    return _reference[case]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", list(CASES))
def test_stagger_modes_equal_the_plain_launch(ms, monkeypatch, case, mode):
    ref = _ref(monkeypatch, case)
    monkeypatch.setenv("MS_FREE_STAGGER", str(mode))
    n0 = _tickets()
    got, wgs = _run(CASES[case])
    # the staggered kernel is what ran: one ticket per workgroup of both rollout launches
    assert _tickets() - n0 == 2 * wgs
    _assert_same(ref, got, (case, mode))


def test_ticket_parity_carries_over_launches(ms, monkeypatch):
    """The staggered launch (value 3, as good as any but 0) twice in one process: the second trainer's launches start from whatever tickets the first left."""
    monkeypatch.setenv("MS_FREE_STAGGER", "3")
    a, _ = _run(CASES["three_workgroups"])
    b, _ = _run(CASES["three_workgroups"])
    _assert_same(a, b, "mode 3 twice")
    _assert_same(_ref(monkeypatch, "three_workgroups"), a, "mode 3 against 0")


def _one_round(E):
    """ms_env_rollout_act_free with n_rounds 1 and no acting after it (the trainer launches T > 1 rounds only), on
    the rings of a fresh cfg3 trainer whose round 0 has acted."""
    abi, tr_mod = _mod("abi"), _mod("trainer")
    t = tr_mod.Trainer.from_named("cfg3", n_envs=E, update_step=2, seed=2, device="cuda:0")
    assert t.fused_rollout_free
    t._prepare_acting()
    t._act_part(0, 0)
    env, e0, e1 = t.env.parts[0]
    N, C, L = t.N, t.C, t.L
    obs = dict(t._acc_out(1, e0, e1), offer=t.off_obs[1])
    rew = dict(offer=t.off.rewards[0].view(E, N, L), acceptor=t.acc.rewards[0].view(E, N, C), agent=t.agent_reward,
               auctioneer=t.auct_reward, price=t.price.rewards[0].view(E, N, L))
    b = lambda x: x.stride(0) * x.element_size()
    strides = abi.MsRoundStridesFree(b(t.acc.actions), b(t.off.actions), b(t.acc_rows), b(t.acc_owner), b(t.off_obs),
                                     b(t.off.rewards), b(t.price.rewards), b(t.acc.rewards), 0, 0, b(t.off.actions),
                                     b(t.off.logprobs), b(t.price_obs), b(t.price.actions), b(t.price.logprobs),
                                     b(t.acc.actions), b(t.acc.logprobs), 8)
    nxt, out = t._fused_next_free(1, 0)
    if t.acc_own is not None:
        strides.next_own_action, strides.next_own_logprob = b(t.acc_own[0]), b(t.acc_own[1])
    env.rollout_act_free(t.acc.actions[0].view(E, N, C), t.off.actions[0].view(E, N, L), obs, rew, nxt, out, strides,
                         1, act_after_last=False)
    torch.cuda.synchronize()
    res = {}
    _snapshot(t, res, "round")
    for k, v in env.export_state().items():
        res["state/%s" % k] = np.asarray(v)
    res["flags"] = np.asarray(t.flags())
    return res


def test_one_round_without_acting(ms, monkeypatch):
    """T = 1: the launch has no barrier after its env round and no acting; the
    round's outputs are those of the plain launch."""
    monkeypatch.setenv("MS_FREE_STAGGER", "0")
    ref = _one_round(96)
    for mode in MODES:
        monkeypatch.setenv("MS_FREE_STAGGER", str(mode))
        n0 = _tickets()
        got = _one_round(96)
        assert _tickets() - n0 == 3
        _assert_same(ref, got, ("one round", mode))
