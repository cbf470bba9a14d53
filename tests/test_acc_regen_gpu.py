"""The acceptor gradient's regenerating scan (ms_ppo_batch's regen fields, ABI 20; k_ppo_grad mode kOwnerRow).

A one-launch free-price rollout acts only for the acceptor items whose agent owns the core; the other items of
ring slots >= 1 are k_acc_common_fill's samples: a pure function of the item's Philox counter, the agent's act-time
common-row table and the owner byte. With the regen fields the gradient kernel computes those pairs (action, old
log-prob) itself and reads the owned items by core, so the fill need not run before the update. Everything here is
bit-exact: the gradient and loss terms against the ring-reading kernel on complete rings, the trainer with
MS_ACC_REGEN=1 against MS_ACC_REGEN=0, and the rings a reader gets (completed on demand) against the filled ones."""
import ctypes as ct
import importlib

import pytest
import torch

pytestmark = pytest.mark.gpu

CFG3 = ("cfg3", None)
SHAPES = [  # (shape, E, T, hand-made owners)
    (CFG3, 100, 3, False),       # E no multiple of 64 (steps straddle rounds), replica e ^ 8 absent at the end
    (CFG3, 100, 3, True),        # + a core its agent owns in no row, and one it owns in every row of a replica
    (CFG3, 64, 2, False),
    ((6, 6, 3), 50, 4, False),   # the generic shapes of the one-launch rollout's test: no draw pairing (64 % C != 0),
    ((8, 7, 2), 40, 4, False),   #   C % 4 != 0 (the per-item fill kernel)
    ((4, 9, 4), 34, 4, False),
]


def _mods():
    return [importlib.import_module("marl-scheduling_amd." + m) for m in ("trainer", "abi", "ppo", "_lib")]


def _trainer(shape, E, T, seed=5, **kw):
    tr_mod, abi, _, _ = _mods()
    if shape == CFG3:
        return tr_mod.Trainer.from_named("cfg3", n_envs=E, update_step=T, seed=seed, device="cuda:0", **kw)
    cfg = abi.make_config(*shape, free_prices=True, commercial=True, **abi.EXP4_JOBS)
    hp = tr_mod.Hyper(update_step=T, raw_k_epochs=2)
    return tr_mod.Trainer(cfg, E, arch="local", hyper=hp, seed=seed, device="cuda:0", **kw)


def _all_common_rings(tr):
    """Ring-shaped (actions, log-probs) with every item of slots >= 1 sampled as a common item: the fill run on
    owners that own nothing."""
    abi = _mods()[1]
    env, obs, fill, strides = tr._fill_args[0]
    act, lp = torch.zeros_like(tr.acc.actions_raw), torch.zeros_like(tr.acc.logprobs_raw)
    nobody = torch.zeros_like(tr.acc_owner)
    f = abi.MsFusedActFree.from_buffer_copy(fill)
    f.acc_action, f.acc_logprob = ct.c_void_p(act[1].data_ptr()), ct.c_void_p(lp[1].data_ptr())
    env.fill_common(dict(core_owner=nobody[1]), f, strides, tr.T, act_after_last=False)
    return act, lp


def _grads(tr, actions, logprobs, owner, sel, ret, regen):
    ppo = _mods()[2]
    T, E, C = tr.T, tr.E, tr.C
    g = tr.acc.group
    ep = g.fused_epoch(tr.acc_rows[:T].reshape(T * E, C, -1), actions.view(T * E, -1), logprobs.view(T * E, -1), ret,
                       sel, T, E, common_row=tr.acc_common, core_owner=owner.reshape(T * E, C), regen=regen)
    for k in ppo.ACTOR_KEYS + ppo.CRITIC_KEYS:
        getattr(g.policy, k).grad.fill_(float("nan"))
    terms = ep.launch().clone()
    torch.cuda.synchronize()
    return {k: getattr(g.policy, k).grad.clone() for k in ppo.ACTOR_KEYS + ppo.CRITIC_KEYS}, terms


@pytest.mark.parametrize("shape,E,T,hand", SHAPES)
def test_regenerating_scan_equals_ring_reads(ms, shape, E, T, hand):
    """ms_ppo_grad with the regen fields on rings whose slots >= 1 are poisoned = ms_ppo_grad reading the rings the
    fill completed: every gradient tensor and the loss terms, bit for bit, with policy != policy_old."""
    ppo = _mods()[2]
    tr = _trainer(shape, E, T, use_graph=False)
    assert tr.acc_regen and tr.fused_rollout_free
    N, C = tr.N, tr.C
    tr.rollout()  # (on its own: the rings are complete when it returns)
    actions, logprobs = tr.acc.actions.clone(), tr.acc.logprobs.clone()
    owner = tr.acc_owner[:T].clone()
    own_a, own_l = tr.acc_own[0].clone(), tr.acc_own[1].clone()
    gen = torch.Generator(device="cuda:0").manual_seed(3)
    with torch.no_grad():  # ratios away from 1
        for prm in tr.acc.group.policy.parameters():
            prm.add_(0.05 * torch.randn(prm.shape, generator=gen, device=prm.device))
    cores = [(2 * a + 1) % C for a in range(N)]
    if hand:
        # owners by hand: agent 0 owns its drawn core in no row, agent 1 owns its drawn core in every row of
        # replica 5 (and of the last replica); the by-core pairs of the items that became owned are made up, and
        # the reference rings are put together from the all-common samples and the by-core pairs
        c0, c1 = cores[0], cores[1]
        owner[:, :, c0][owner[:, :, c0] == 1] = 0
        owner[:, 5, c1] = 2
        owner[:, E - 1, c1] = 2
        own_a = torch.randint(0, tr.acc.group.policy.A, own_a.shape, generator=gen, device="cuda:0").to(torch.int8)
        own_l = -torch.rand(own_l.shape, generator=gen, device="cuda:0") * 3 - 0.01
        com_a, com_l = _all_common_rings(tr)
        agents = torch.arange(1, N + 1, device="cuda:0").view(1, 1, N, 1)
        mine = (owner.unsqueeze(2) == agents)[1:]                              # [T - 1][E][N][C]
        actions[1:] = torch.where(mine, own_a[1:].unsqueeze(2), com_a[1:].view(T - 1, E, N, C)).view(T - 1, E, N * C)
        logprobs[1:] = torch.where(mine, own_l[1:].unsqueeze(2), com_l[1:].view(T - 1, E, N, C)).view(T - 1, E, N * C)
    sel = torch.tensor([a * C + cores[a] for a in range(N)], dtype=torch.int32, device="cuda:0")
    ret = ppo.unit_returns(tr.acc.rewards, sel, tr.acc.group.gamma)
    want, want_terms = _grads(tr, actions, logprobs, owner, sel, ret, None)
    # the regenerating call: nothing of ring slots >= 1 may be read
    bad_a, bad_l = actions.clone(), logprobs.clone()
    bad_a[1:] = 1
    bad_l[1:] = -0.25
    regen = dict(tr._acc_regen_args(), own_action=own_a.view(T * E, C), own_logprob=own_l.view(T * E, C))
    got, got_terms = _grads(tr, bad_a, bad_l, owner, sel, ret, regen)
    for k in want:
        assert torch.isfinite(want[k]).all(), k
        assert torch.equal(want[k], got[k]), (k, int((want[k] != got[k]).sum()))
    assert torch.equal(want_terms, got_terms)
    # ... and the poison does change the ring-reading kernel's result (the comparison above can fail)
    other, _ = _grads(tr, bad_a, bad_l, owner, sel, ret, None)
    assert not torch.equal(other["w3"], want["w3"])
    if hand:  # the owners are what the case is about
        assert not bool((owner[:, :, cores[0]] == 1).any()) and bool((owner[:, 5, cores[1]] == 2).all())


def _rings(t):
    out = {"acc_owner": t.acc_owner, "acc_rows": t.acc_rows}
    for u in t.units():
        for k in ("actions", "logprobs", "rewards"):
            out["%s.%s" % (u.name, k)] = getattr(u, k)
    return out


@pytest.mark.parametrize("graph", [True, False])
@pytest.mark.parametrize("E", [128, 100])
def test_trainer_regen_equals_fill(ms, monkeypatch, E, graph):
    """cfg3, T = 8, three iterations with MS_ACC_REGEN 1 and 0: equal losses and weights after each; the rings read
    after iteration 2 in the regenerating trainer (completed on demand) equal the filling trainer's, and iteration 3
    is still equal."""
    ppo = _mods()[2]
    mk = lambda: _trainer(CFG3, E, 8, seed=9, use_graph=graph)
    regen = mk()
    monkeypatch.setenv("MS_ACC_REGEN", "0")
    fill = mk()
    assert regen.acc_regen and not fill.acc_regen
    for it in range(3):
        l0, l1 = regen.iteration(), fill.iteration()
        torch.cuda.synchronize()
        for k in l0:
            assert torch.equal(l0[k], l1[k]), (it, k)
        for u0, u1 in zip(regen.units(), fill.units()):
            for k in ppo.ACTOR_KEYS + ppo.CRITIC_KEYS:
                assert torch.equal(getattr(u0.group.policy, k), getattr(u1.group.policy, k)), (it, u0.name, k)
        if it == 1:
            assert regen._rings_pending  # nothing has completed them yet
            r0, r1 = _rings(regen), _rings(fill)
            assert not regen._rings_pending
            for k in r0:
                assert torch.equal(r0[k], r1[k]), k
    assert regen.flags() == 0 and fill.flags() == 0


def test_rings_survive_a_table_rebuild(ms, monkeypatch):
    """evaluate() (and anything else that may rebuild the acting tables from the updated policy_old) between
    iteration() and the first ring read: the rings still equal the filling trainer's."""
    mk = lambda: _trainer(CFG3, 128, 8, seed=3)
    regen = mk()
    monkeypatch.setenv("MS_ACC_REGEN", "0")
    fill = mk()
    for _ in range(2):
        regen.iteration(), fill.iteration()
    assert regen._rings_pending
    regen.evaluate(episodes=1, n_envs=16)
    regen._prepare_acting()  # the tables rebuilt from the new policy_old: pending rings are completed first
    r0, r1 = _rings(regen), _rings(fill)
    for k in r0:
        assert torch.equal(r0[k], r1[k]), k


def test_regen_arguments_are_checked(ms):
    """The regen fields without core_owner (or without the by-core arrays) are MS_EINVAL."""
    _, abi, ppo, lib_mod = _mods()
    tr = _trainer(CFG3, 64, 2, use_graph=False)
    tr.rollout()
    T, E, C, N = tr.T, tr.E, tr.C, tr.N
    sel = torch.arange(N, dtype=torch.int32, device="cuda:0") * C
    ret = ppo.unit_returns(tr.acc.rewards, sel, tr.acc.group.gamma)
    g = tr.acc.group
    rows = tr.acceptor_rows(0, T).reshape(T * E, N * C, -1).contiguous()
    regen = tr._acc_regen_args()

    def call(batch_edit):
        ep = g.fused_epoch(tr.acc_rows[:T].reshape(T * E, C, -1), tr.acc.actions.view(T * E, -1),
                           tr.acc.logprobs.view(T * E, -1), ret, sel, T, E, common_row=tr.acc_common,
                           core_owner=tr.acc_owner[:T].reshape(T * E, C), regen=regen)
        # (the closure's structs: cell contents of launch)
        cells = dict(zip(ep.launch.__code__.co_freevars, [c.cell_contents for c in ep.launch.__closure__]))
        batch_edit(cells["batch"])
        return ep.launch

    def no_owner(b):
        b.core_owner, b.n_cores, b.states = None, 0, ct.c_void_p(rows.data_ptr())

    def no_own_arrays(b):
        b.own_action = None

    for edit, msg in ((no_owner, "core_owner"), (no_own_arrays, "own_action")):
        with pytest.raises(lib_mod.MarlSchedError, match=msg) as ei:
            call(edit)()
        assert ei.value.code == 22  # MS_EINVAL
