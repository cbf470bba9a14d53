"""Greedy (argmax) acting, ms_policy_act_greedy / ms_act_round_greedy: the picks against a float64
restatement of ActorCritic.actor (PPOmodules.py:53-63), the first-maximum rule within and across
16-action tiles, the padding actions, the common-row and compact forms bit for bit, and the
argument checks."""
import ctypes as ct
import importlib
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SHAPES = [(8, 8, 51, 52, 25), (24, 1, 18, 20, 9), (1, 16, 27, 28, 13), (8, 3, 4, 4, 13), (2, 5, 195, 196, 97),
          (3, 2, 11, 12, 5)]


def _ppo():
    return importlib.import_module("marl-scheduling_amd.ppo")


def _cpu_weights(ppo, net):
    return {k: getattr(net, k).detach().cpu().clone() for k in ppo.ACTOR_KEYS}


def _logits(w, g, x, dtype):
    """Group g's actor logits of rows x [R, D] in dtype on the CPU (Linear-tanh-Linear-tanh-Linear)."""
    p = {k: v[g].to(dtype) for k, v in w.items()}
    h = torch.tanh(x.to(dtype) @ p["w1"].T + p["b1"])
    h = torch.tanh(h @ p["w2"].T + p["b2"])
    return h @ p["w3"].T + p["b3"]


def _obs(E, U, D, stride, seed=1):
    gen = torch.Generator().manual_seed(seed)
    obs = torch.zeros((E, U, stride), dtype=torch.int8)
    obs[..., :D] = torch.randint(-5, 13, (E, U, D), generator=gen, dtype=torch.int8)
    return obs


def check_greedy_rows(act, l64, l32, what="", max_near=0.005):
    """The near-tie rule: delta = 8 * max|f32 - f64| over the rows given (8: the MFMA's other accumulation
    order and fast_tanh_b's ~1e-7 absolute error); a row whose float64 top-2 gap is below delta is near-tied
    and may take any action within delta of the maximum, every other row takes the float64 argmax. Near-tied
    rows are at most max_near (0.5 %) of the rows (None: a closed loop's rows, many of them equal, are not
    held to it). act [R] long, l64 / l32 [R, A]. Returns (delta, near-tied rows)."""
    delta = 8.0 * float((l32.double() - l64).abs().max())
    top2 = l64.topk(2, dim=-1).values
    near = (top2[:, 0] - top2[:, 1]) < delta
    print("%s delta %.3g, smallest top-2 gap %.3g, near-tied %d of %d rows" %
          (what, delta, float((top2[:, 0] - top2[:, 1]).min()), int(near.sum()), len(act)))
    want = l64.argmax(-1)
    assert torch.equal(act[~near], want[~near])
    chosen = l64.gather(1, act.view(-1, 1)).squeeze(1)
    assert bool((chosen[near] >= top2[near, 0] - delta).all())
    if max_near is not None:
        assert int(near.sum()) <= max_near * len(act)
    return delta, int(near.sum())


@pytest.mark.parametrize("G,per_group,D,stride,A", SHAPES)
def test_greedy_matches_float64_argmax(ms, G, per_group, D, stride, A):
    ppo = _ppo()
    torch.manual_seed(0)
    net = ppo.GroupedActorCritic(G, D, A)
    w = _cpu_weights(ppo, net)
    E, U = 333, G * per_group
    obs = _obs(E, U, D, stride)
    act, lp = net.cuda().act_greedy(obs.cuda(), U)
    act, lp = act.cpu().long(), lp.cpu()
    assert int(act.min()) >= 0 and int(act.max()) < A
    l64, l32 = [], []
    for g in range(G):
        rows = obs[:, g * per_group:(g + 1) * per_group, :D].reshape(-1, D)
        l64.append(_logits(w, g, rows, torch.float64))
        l32.append(_logits(w, g, rows, torch.float32))
    ga = torch.cat([act[:, g * per_group:(g + 1) * per_group].reshape(-1) for g in range(G)])
    glp = torch.cat([lp[:, g * per_group:(g + 1) * per_group].reshape(-1) for g in range(G)])
    l64, l32 = torch.cat(l64), torch.cat(l32)
    check_greedy_rows(ga, l64, l32, "shape %s:" % ((G, per_group, D, stride, A),))
    # the chosen action's log-prob against log_softmax of the f32 restatement, at the act tolerance
    ref = torch.log_softmax(l32, -1).gather(1, ga.view(-1, 1)).squeeze(1)
    np.testing.assert_allclose(glp.numpy(), ref.numpy(), rtol=1e-5, atol=2e-6)


@pytest.mark.parametrize("rows,expect", [((3, 7, 19), 3), ((19, 23), 19)])
def test_first_maximum_within_and_across_tiles(ms, rows, expect):
    """Equal weight rows give bit-equal logits: the smallest index wins, inside a 16-action tile (3 vs 7,
    19 vs 23), across a lane's registers and lanes, and across tiles (3 vs 19)."""
    ppo = _ppo()
    torch.manual_seed(0)
    net = ppo.GroupedActorCritic(1, 51, 25)
    with torch.no_grad():
        for r in rows[1:]:
            net.w3[0, r] = net.w3[0, rows[0]]
            net.b3[0, r] = net.b3[0, rows[0]]
        net.b3[0, list(rows)] += 5.0
    obs = _obs(333, 1, 51, 52)
    act, _ = net.cuda().act_greedy(obs.cuda(), 1)
    assert torch.equal(act.cpu().long(), torch.full((333, 1), expect))


@pytest.mark.parametrize("A", [5, 13, 25, 97])
def test_padding_actions_never_win(ms, A):
    """Every logit -10, the padded accumulator rows 0: the pick must stay below A."""
    ppo = _ppo()
    torch.manual_seed(0)
    G, per_group, D, stride, E = 2, 3, 11, 12, 37
    net = ppo.GroupedActorCritic(G, D, A)
    with torch.no_grad():
        net.w3.zero_()
        net.b3.fill_(-10.0)
    obs = _obs(E, G * per_group, D, stride).cuda()
    net = net.cuda()
    act, lp = net.act_greedy(obs, G * per_group)
    assert torch.equal(act.cpu().long(), torch.zeros((E, G * per_group), dtype=torch.long))
    np.testing.assert_allclose(lp.cpu().numpy(), -math.log(A), rtol=1e-5, atol=2e-6)
    with torch.no_grad():
        net.b3[:, A - 1] = -9.0
    act, _ = net.act_greedy(obs, G * per_group)
    assert torch.equal(act.cpu().long(), torch.full((E, G * per_group), A - 1))


def _common_row(D, stride, O):
    return torch.tensor([0, -1, -1] + [-2] * (2 * O) + [0] * (stride - D), dtype=torch.int8)


@pytest.mark.parametrize("G,per_group,O,A,frac", [(8, 8, 24, 25, 0.85), (8, 8, 24, 25, 0.0), (8, 8, 24, 25, 1.0),
                                                  (1, 16, 12, 13, 0.5), (3, 2, 4, 5, 0.9), (2, 5, 96, 97, 0.8)])
def test_greedy_common_rows_bit_identical(ms, G, per_group, O, A, frac):
    """act_greedy(common_row=...) == act_greedy() bit for bit (actions and log-probs), incl. rows one byte
    off the common row."""
    ppo = _ppo()
    D = 3 + 2 * O
    stride = (D + 3) // 4 * 4
    torch.manual_seed(5)
    net = ppo.GroupedActorCritic(G, D, A).cuda()
    E, U = 1001, G * per_group
    gen = torch.Generator().manual_seed(6)
    crow = _common_row(D, stride, O)
    obs = torch.zeros((E, U, stride), dtype=torch.int8)
    obs[..., :D] = torch.randint(-5, 13, (E, U, D), generator=gen, dtype=torch.int8)
    pick = torch.rand((E, U), generator=gen) < frac
    obs[pick] = crow
    near = (torch.rand((E, U), generator=gen) < 0.02) & pick  # one byte off the common row
    col = torch.randint(0, D, (E, U), generator=gen)
    obs[near, col[near]] = 7
    dobs = obs.cuda()
    a0, l0 = net.act_greedy(dobs, U)
    a1, l1 = net.act_greedy(dobs, U, common_row=crow.cuda())
    assert torch.equal(a0, a1)
    assert torch.equal(l0.view(torch.int32), l1.view(torch.int32))


# (N, C, L, E): cfg2's and cfg3's shapes (the paired kernels under fixed and free prices) and cfg4's
GEOMETRIES = {"cfg2": (4, 4, 3, 1001), "cfg3": (8, 8, 3, 1001), "cfg4": (16, 16, 3, 101)}
COMPACT_CASES = [(geo, groups, own, free) for geo in ("cfg2", "cfg3") for groups in ("one", "agent", "unit")
                 for own in ("none", "all", "mixed") for free in (False, True)] + [("cfg4", "unit", "mixed", True)]


@pytest.mark.parametrize("geo,groups,own,free", COMPACT_CASES)
def test_act_round_greedy_equals_act_greedy(ms, geo, groups, own, free):
    """One launch on the env's compact observations == act_greedy on the offer rows, on the regenerated
    acceptor rows and (free prices) on the price_state it derives, bit for bit."""
    ppo = _ppo()
    N, C, L, E = GEOMETRIES[geo]
    O = N * L
    D_acc, D_off = 3 + 2 * O, 2 * C + 2
    s_acc, s_off = (D_acc + 3) // 4 * 4, (D_off + 3) // 4 * 4
    g_acc = dict(one=1, agent=N, unit=N * C)[groups]
    g_off = dict(one=1, agent=N, unit=N * L)[groups]
    A_price = 13
    torch.manual_seed(7)
    acc = ppo.GroupedActorCritic(g_acc, D_acc, O + 1).cuda()
    core = ppo.GroupedActorCritic(g_off, D_off, C + 1).cuda()
    price = ppo.GroupedActorCritic(g_off, 4, A_price).cuda() if free else None
    gen = torch.Generator().manual_seed(8)
    crow = _common_row(D_acc, s_acc, O)
    core_rows = torch.zeros((E, C, s_acc), dtype=torch.int8)
    core_rows[..., :D_acc] = torch.randint(-5, 13, (E, C, D_acc), generator=gen, dtype=torch.int8)
    same = torch.rand((E, C), generator=gen) < 0.1   # an owner's row that equals the common row, or is one byte off
    core_rows[same] = crow
    off1 = (torch.rand((E, C), generator=gen) < 0.5) & same
    col = torch.randint(0, D_acc, (E, C), generator=gen)
    core_rows[off1, col[off1]] = 7
    owner = dict(none=torch.zeros((E, C), dtype=torch.int8),
                 all=torch.randint(1, N + 1, (E, C), generator=gen, dtype=torch.int8),
                 mixed=torch.randint(0, N + 1, (E, C), generator=gen, dtype=torch.int8))[own]
    off_obs = _obs(E, N * L, D_off, s_off, seed=9)
    dev = "cuda"
    core_rows, owner, off_obs, crow = core_rows.to(dev), owner.to(dev), off_obs.to(dev), crow.to(dev)
    i8 = lambda *shape: torch.full(shape, 99, dtype=torch.int8, device=dev)
    out = dict(core_action=i8(E, N * L))
    if free:
        out.update(price_state=i8(E, N * L, 4), price_action=i8(E, N * L), env_price=i8(E, N * L))
    acc_action = i8(E, N * C)
    ppo.act_round_greedy(core, price, off_obs, acc, core_rows, owner, crow, C, out, acc_action)
    rows = ppo.regen_acceptor_rows(core_rows, owner, crow, N).contiguous()
    want_acc, _ = acc.act_greedy(rows, N * C)
    assert torch.equal(acc_action, want_acc)
    assert int(acc_action.min()) >= 0 and int(acc_action.max()) <= O
    want_core, _ = core.act_greedy(off_obs, N * L)
    assert torch.equal(out["core_action"], want_core)
    if free:
        a = want_core.long()
        assert bool((a == 0).any()) and bool((a > 0).any())
        idx = torch.stack([2 * a, 2 * a + 1, torch.full_like(a, 2 * C), torch.full_like(a, 2 * C + 1)], -1)
        st = torch.gather(off_obs, 2, idx)
        st[a == 0] = -5  # the dummy state of "no offer" (PPOmodules.py:327)
        assert torch.equal(out["price_state"], st)
        want_price, _ = price.act_greedy(out["price_state"], N * L)
        assert torch.equal(out["price_action"], want_price)
        env_price = torch.where(a == 0, torch.full_like(want_price, -5), want_price)
        assert torch.equal(out["env_price"], env_price)


def test_greedy_argument_checks(ms):
    """Shapes outside the kernels' range and missing outputs: MS_EINVAL with a message, nothing launched."""
    ppo = _ppo()
    lib, ptr = ms.lib, importlib.import_module("marl-scheduling_amd._lib").ptr
    torch.manual_seed(0)
    E, U, D, stride, A = 8, 4, 10, 12, 5
    net = ppo.GroupedActorCritic(1, D, A).cuda()
    obs = _obs(E, U, D, stride).cuda()
    action = torch.full((E, U), 77, dtype=torch.int8, device="cuda")
    logprob = torch.full((E, U), 7.0, device="cuda")

    def call(p, obs_p, act_p):
        return lib.ms_policy_act_greedy(ct.byref(p), obs_p, stride, E, U, U, None, act_p, ptr(logprob), None)

    def einval(rc):
        assert rc == ppo.MS_EINVAL and len(lib.ms_last_error()) > 0

    p = net.mlp_params()
    p.hidden = 32
    einval(call(p, ptr(obs), ptr(action)))
    p = net.mlp_params()
    p.n_actions = 130
    einval(call(p, ptr(obs), ptr(action)))
    p = net.mlp_params()
    einval(call(p, ptr(obs), None))
    einval(call(p, None, ptr(action)))
    # the round: acceptor output missing; price chooser without its outputs; fixed prices with one
    N, C, L = 2, 4, 2
    acc = ppo.GroupedActorCritic(1, 3 + 2 * N * L, N * L + 1).cuda()
    core = ppo.GroupedActorCritic(1, 2 * C + 2, C + 1).cuda()
    price = ppo.GroupedActorCritic(1, 4, 13).cuda()
    s_acc = 12
    core_rows = torch.zeros((E, C, s_acc), dtype=torch.int8, device="cuda")
    owner = torch.zeros((E, C), dtype=torch.int8, device="cuda")
    crow = torch.zeros(s_acc, dtype=torch.int8, device="cuda")
    off_obs = _obs(E, N * L, 2 * C + 2, 12).cuda()
    core_action = torch.full((E, N * L), 77, dtype=torch.int8, device="cuda")
    acc_action = torch.full((E, N * C), 77, dtype=torch.int8, device="cuda")
    pst = torch.full((E, N * L, 4), 77, dtype=torch.int8, device="cuda")

    def round_call(pp, core_p, price_outs, acc_p, hidden=16):
        pc, pa = core.mlp_params(), acc.mlp_params()
        pa.hidden = hidden
        return lib.ms_act_round_greedy(ct.byref(pc), ct.byref(pp) if pp is not None else None, ptr(off_obs), 12,
                                       N * L, N * L, ct.byref(pa), ptr(core_rows), ptr(owner), s_acc, N * C, N * C, C,
                                       ptr(crow), E, core_p, *price_outs, acc_p, None)

    none3 = (None, None, None)
    einval(round_call(None, ptr(core_action), none3, None))
    einval(round_call(None, None, none3, ptr(acc_action)))
    einval(round_call(price.mlp_params(), ptr(core_action), none3, ptr(acc_action)))
    einval(round_call(None, ptr(core_action), (ptr(pst), None, None), ptr(acc_action)))
    einval(round_call(None, ptr(core_action), none3, ptr(acc_action), hidden=32))
    torch.cuda.synchronize()
    for t in (action, core_action, acc_action, pst):
        assert bool((t == 77).all())
    assert bool((logprob == 7.0).all())
    # and the valid calls go through
    assert round_call(None, ptr(core_action), none3, ptr(acc_action)) == 0
    assert call(net.mlp_params(), ptr(obs), ptr(action)) == 0
    torch.cuda.synchronize()
    assert int(action.max()) < A and int(acc_action.max()) <= N * L and int(core_action.max()) <= C
