"""The learned auctioneer: Trainer(learned_auctioneer=True) adds a fourth unit type, one net of the acceptor's shape
shared by the C cores, that sells the cores nobody owns. Its rollout runs as one launch (k_env_rollout_act_auct), as
one launch per round (k_env_step_act_auct, MS_ENV_ROLLOUT=0) or as launch pairs (MS_ENV_FUSED_ACT=0: the agents'
act launch, act_compact for the auctioneer at Philox offset 8 t + 5, env.step(auctioneer=ring[t])), and the three
are compared bit for bit; the played trajectory is replayed on the C restatement (oracle/pyoracle) with the
auctioneer ring as its auctioneer actions; the sampled actions and the gradient are held against float64.

Which kernel a (shape, E) reaches is written at the top of tests/test_mixed_train_gpu.py; the cases are those."""
import ctypes as ct
import functools
import importlib

import numpy as np
import pytest
import torch

from oracle import ppo_grad_ref as pr
from oracle import pyoracle
from oracle.ppo_ref import act_reference
from tests.drivers import compare_state
from tests.test_act_buckets_gpu import ATOL, EPS, MAX_NEAR_SHARE, NEAR_U, RTOL
from tests.test_mixed_train_gpu import _JOBS, _assert_same, _environ
from tests.test_ppo_grad_parity_gpu import R_PPO, _compare

pytestmark = pytest.mark.gpu

SEED = 3
PAIRS = (dict(MS_ENV_ROLLOUT="0"), dict(MS_ENV_FUSED_ACT="0"))
SHAPE_KW = {"4x4x3": None, "6x5x2": dict(n_agents=6, n_cores=5, collection_length=2, **_JOBS),
            "4x1x3": dict(n_agents=4, n_cores=1, collection_length=3, **_JOBS)}


def _mod(name):
    return importlib.import_module("marl-scheduling_amd." + name)


def _cfg(shape):
    abi = _mod("abi")
    kw = SHAPE_KW[shape]
    return abi.named_config("cfg2") if kw is None else abi.make_config(**kw)


def _trainer(shape, E, t, env=None, auct=True, **kw):
    tr = _mod("trainer")
    kw.setdefault("use_graph", False)
    with _environ(env or {}):
        return tr.Trainer(_cfg(shape), E, arch="global", hyper=tr.Hyper(update_step=t), seed=SEED, device="cuda:0",
                          learned_auctioneer=auct, **kw)


def _state(t, losses):
    """Everything a run leaves behind: losses, the three unit types' nets, Adam state and rings, the observation
    rings, the exported env state (MT words and flags included), the counters and the episode accumulators."""
    st = {}
    for i, ls in enumerate(losses):
        for k, v in ls.items():
            st["loss%d.%s" % (i, k)] = v.clone()
    for u in t.units():
        g = u.group
        for pol_name, pol in (("policy", g.policy), ("policy_old", g.policy_old)):
            for k, p in pol.named_parameters():
                st["%s.%s.%s" % (u.name, pol_name, k)] = p.detach().clone()
        opt = g.hip_optimizer
        for i, p in enumerate(q for grp in opt.param_groups for q in grp["params"]):
            st["%s.adam%d.m" % (u.name, i)] = opt.state[p]["exp_avg"].clone()
            st["%s.adam%d.v" % (u.name, i)] = opt.state[p]["exp_avg_sq"].clone()
        st[u.name + ".adam.step"] = int(opt.step_dev)
        st[u.name + ".actions"] = u.actions.clone()
        st[u.name + ".logprobs"] = u.logprobs.clone()
        st[u.name + ".rewards"] = u.rewards.clone()
    st["off_obs"], st["acc_rows"], st["acc_owner"] = t.off_obs.clone(), t.acc_rows.clone(), t.acc_owner.clone()
    st["agent_reward"] = t.agent_reward.clone()
    st["env"] = [env.export_state() for env, _, _ in t.env.parts]
    st["counters"] = (t.rounds_done, t.rng.getstate(), int(t.rng_ctr), t.flags(), t.env.round)
    if t.metric_bufs is not None:
        st["metrics"] = [b.clone() for b in t.metric_bufs]
        st["episode_log"] = list(t.episode_log)
    return st


def _run(t, n):
    return _state(t, [t.iteration() for _ in range(n)])


# ---- 1. one launch == one launch per round == launch pairs

def _three_paths(shape, E, t, fused=True, **kw):
    a = _trainer(shape, E, t, **kw)
    assert a.fused_rollout == fused and [u.name for u in a.units()] == ["acceptor", "offer", "auctioneer"]
    want = _run(a, 2)
    for env in PAIRS:
        b = _trainer(shape, E, t, env=env, **kw)
        assert not b.fused_rollout and (env.get("MS_ENV_FUSED_ACT") != "0" or not b.fused_step)
        _assert_same(_run(b, 2), want, "%s E=%d %r" % (shape, E, env))
    assert a.flags() == 0
    return a, want


def test_three_paths_small(ms):
    """4x4x3 at E 37, T 48, episodes of 16 rounds: 16 lanes per replica, a partial last wave, 148 auctioneer items
    (both words of a draw pair), episode ends inside the rollout and an MT block crossing."""
    a, want = _three_paths("4x4x3", 37, 48, episode_length=16)
    own = want["acc_owner"][:48]
    assert bool((own == 0).any()) and bool((own > 0).any())       # items from the net and items from the table
    assert int(want["auctioneer.rewards"].abs().sum()) > 0        # the auctioneer sold something
    assert len({int(x) for x in want["auctioneer.actions"].unique()}) > 2


def test_three_paths_two_streams(ms):
    with pytest.warns(UserWarning):  # (33 * C is no multiple of 128: the parts' draws are not an unsplit run's)
        a, _ = _three_paths("4x4x3", 66, 48, episode_length=16, rollout_streams=2)
    assert len(a.env.parts) == 2


DISPATCH = [("4x4x3", 2065, "32 lanes, FixShape<4,4,3,1>"), ("4x4x3", 1025, "64 lanes, DynShape"),
            ("6x5x2", 2051, "32 lanes, DynShape")]


@pytest.mark.parametrize("shape,E,kernel", DISPATCH, ids=[d[2].split(",")[0] + "-" + d[0] for d in DISPATCH])
def test_three_paths_wide_groups(ms, shape, E, kernel):
    _three_paths(shape, E, 4)


def test_three_paths_one_core(ms):
    a, want = _three_paths("4x1x3", 33, 6)
    assert a.C == 1 and want["auctioneer.actions"].shape == (6, 33, 1)


def test_three_paths_unsupported_shape_steps_with_pairs(ms):
    """6x5x2 at 40 replicas is outside the fused kernels' range: every path is the launch pair, and still agrees."""
    a, _ = _three_paths("6x5x2", 40, 4, fused=False)
    assert not a.fused_step


def test_t1_has_no_fused_acting(ms):
    a, _ = _three_paths("4x4x3", 37, 1, fused=False)
    assert not a.fused_step


def test_three_paths_metrics(ms):
    a, want = _three_paths("4x4x3", 37, 48, episode_length=16, metrics=True)
    assert len(want["episode_log"]) == 6 and len(want["episode_log"][0]) == 37
    sold = [d["auctioneerRew"] for ep in want["episode_log"] for d in ep]
    assert any(v != 0 for v in sold)  # the learned auctioneer's reward, per replica and episode


# ---- 2. the env played what the rings say

@functools.lru_cache(maxsize=None)
def _rollout_48():
    """The 4x4x3 / E 37 / T 48 rollout (one launch), before any update: shared by the replay and parity tests and
    left unchanged."""
    t = _trainer("4x4x3", 37, 48, episode_length=16)
    assert t.fused_rollout
    t.rollout()
    torch.cuda.synchronize()
    return t


def test_rings_replay_on_the_oracle(ms):
    t = _rollout_48()
    T, E, N, C, L = t.T, t.E, t.N, t.C, t.L
    s = ms.abi.config_shape(t.cfg)
    D_acc, D_off = s["acc_obs_dim"], s["off_obs_dim"]
    base = _mod("evaluation").env_seed(SEED, 0, E)
    rows = t.acceptor_rows().cpu().numpy()        # [T + 1, E, N*C, stride]
    off = t.off_obs.cpu().numpy()
    own = t.acc_owner.cpu().numpy()
    aa, ao, au = (u.actions.cpu().numpy() for u in (t.acc, t.off, t.auct))
    ra, ro, ru = (u.rewards.cpu().numpy() for u in (t.acc, t.off, t.auct))
    agent = t.agent_reward.cpu().numpy()
    gs = t.env.parts[0][0].export_state()
    sold, owned_items, free_items = 0, 0, 0
    for e in (0, 17, 35, 36):
        env = pyoracle.OracleEnv(t.cfg, base + e)
        o = env.observe()
        assert np.array_equal(rows[0, e, :, :D_acc].reshape(N, C, D_acc), o["acceptor"])
        for r in range(T):
            free_items += int((own[r, e] == 0).sum())
            owned_items += int((own[r, e] > 0).sum())
            res = env.step(aa[r, e].reshape(N, C), ao[r, e].reshape(N, L), None, au[r, e])
            sold += int(((res["accepted"]["valid"] != 0) & (res["accepted"]["recipient"] == 0)).sum())
            o = env.observe()
            assert np.array_equal(rows[r + 1, e, :, :D_acc].reshape(N, C, D_acc), o["acceptor"]), (e, r)
            assert np.array_equal(off[r + 1, e, :, :D_off].reshape(N, L, D_off), o["offer"]), (e, r)
            assert np.array_equal(ra[r, e].reshape(N, C), res["acceptor"]), (e, r)
            assert np.array_equal(ro[r, e].reshape(N, L), res["offer"]), (e, r)
            assert np.array_equal(ru[r, e], res["auctioneer"]), (e, r)
        assert np.array_equal(agent[e], res["agent"]), e  # (one [E][N] buffer: the last round's)
        assert env.flags == 0
        compare_state({k: v[e:e + 1] for k, v in gs.items()}, [env.export_state()], 1)
    # at round 0 the auctioneer owns every core; later ownership is mixed, and it sold cores
    assert bool((own[0] == 0).all()) and owned_items > 0 and free_items > 0 and sold > 0


# ---- 3. the ring's actions and log-probs against float64 at the recomputed uniforms

def _philox2(row, off, seed):
    """ms_common.h philox2 on arrays of rows: the two output words."""
    m32 = np.uint64(0xffffffff)
    c0 = np.asarray(row, dtype=np.uint64) & m32
    c1 = np.full_like(c0, off & 0xffffffff)
    k = np.uint64(((seed & 0xffffffff) ^ (((seed >> 32) * 0x85EBCA6B) & 0xffffffff) ^
                   (((off >> 32) * 0xC2B2AE35) & 0xffffffff)) & 0xffffffff)
    for _ in range(10):
        p = np.uint64(0xD256D193) * c0
        c0, c1 = ((p >> np.uint64(32)) ^ k ^ c1) & m32, p & m32
        k = (k + np.uint64(0x9E3779B9)) & m32
    return c0, c1


def test_acting_matches_float64(ms):
    t = _rollout_48()
    ppo = _mod("ppo")
    T, E, C = t.T, t.E, t.C
    net = t.auct.group.policy_old
    D, A = net.D, net.A
    w = {k: getattr(net, k).detach().cpu()[0] for k in ppo.ACTOR_KEYS}
    own0 = (t.acc_owner[:T] == 0).to(torch.int8)
    rows = ppo.regen_acceptor_rows(t.acc_rows[:T].contiguous(), own0.contiguous(), t.acc_common, 1).cpu()
    assert rows.shape[:3] == (T, E, C)
    item = np.arange(E * C, dtype=np.uint64)
    u = np.empty((T, E * C), dtype=np.float32)
    for r in range(T):  # item i: word (i >> 6) & 1 of the draw countered by i & ~64, offset 8 t + 5 (counter 0)
        o0, o1 = _philox2(item & ~np.uint64(64), 8 * r + 5, SEED * 7919)
        word = np.where((item & np.uint64(64)) != 0, o1, o0)
        u[r] = (word >> np.uint64(8)).astype(np.float32) * np.float32(1.0 / 16777216.0)
    u = torch.from_numpy(u).view(T, E, C)
    x = rows[..., :D].reshape(T * E, C, D)
    uu = u.reshape(T * E, C)
    a64, _, p64 = act_reference({k: v.double() for k, v in w.items()}, x.double(), uu.double())
    _, _, p32 = act_reference({k: v.float() for k, v in w.items()}, x.float(), uu.float())
    cdf = torch.cumsum(p64, -1)[..., :-1]
    near = (cdf - uu.double().unsqueeze(-1)).abs().min(-1).values < NEAR_U
    share = float(near.float().mean())
    assert share <= MAX_NEAR_SHARE
    act = t.auct.actions.cpu().long().reshape(T * E, C)
    lp = t.auct.logprobs.cpu().reshape(T * E, C)
    assert int(act.min()) >= 0 and int(act.max()) < A and bool(torch.isfinite(lp).all())
    mism = act != a64
    print("AUCT|act|rows %d|near share %.4f%%|exempted %d" % (act.numel(), 100.0 * share, int(mism.sum())))
    assert not bool((mism & ~near).any()) and int(mism.sum()) <= int(near.sum())
    want = torch.log(p32.clamp(EPS, 1.0 - EPS)).gather(2, act.unsqueeze(-1)).squeeze(-1)
    same = ~mism
    np.testing.assert_allclose(lp[same].numpy(), want[same].numpy(), rtol=RTOL, atol=ATOL)
    both = own0.cpu().reshape(T * E, C).bool()
    assert bool(both.any()) and bool((~both).any())  # rows through the net's tile and rows from its table


# ---- 4. one auctioneer epoch against the float64 gradient (the owner-row path with a derived owner ring, U = C)

def test_gradient_matches_float64(ms):
    t = _trainer("4x4x3", 37, 12, episode_length=16)
    t.rollout()
    ppo = _mod("ppo")
    T, E, C = t.T, t.E, t.C
    R = T * E
    assert R % 64 != 0
    au = t.auct
    c = int(au.rewards.ne(0).sum((0, 1)).argmax())  # the core whose returns vary most
    sel = torch.tensor([c], dtype=torch.int32, device=t.device)
    epoch = t._epochs(au, sel, [1])[0]
    loss = epoch.launch().cpu().numpy()
    torch.cuda.synchronize()
    pol = au.group.policy
    grads = {k: getattr(pol, k).grad.cpu().numpy() for k in pr.KEYS}
    nets = {k: getattr(pol, k).detach().cpu().numpy() for k in pr.KEYS}
    own0 = (t.acc_owner[:T] == 0).to(torch.int8).contiguous()
    rows = ppo.regen_acceptor_rows(t.acc_rows[:T].contiguous(), own0, t.acc_common, 1).cpu()
    x = rows[:, :, c, :pol.D].reshape(1, R, pol.D).float().numpy()
    act = au.actions[:, :, c].reshape(1, R).cpu().numpy()
    olp = au.logprobs[:, :, c].reshape(1, R).cpu().numpy()
    ret = ppo.unit_returns(au.rewards, sel, au.group.gamma).reshape(1, R).cpu().numpy()
    assert float(np.abs(ret).max()) > 0 and bool(own0[:, :, c].any()) and not bool(own0[:, :, c].all())
    g64, l64 = pr.grad_ref(nets, x, act, olp, ret, eps_clip=t.hp.eps_clip)
    g32, l32 = pr.grad_ref(nets, x, act, olp, ret, eps_clip=t.hp.eps_clip, dtype=torch.float32)
    ratios = {k: _compare("auct|%s" % k, grads[k], g64[k], g32[k]) for k in pr.KEYS}
    for i, term in enumerate(("loss_min", "loss_mse", "loss_ent")):
        ratios[term] = _compare("auct|%s" % term, loss[:, i], l64[:, i], l32[:, i])
    over = {k: round(v, 3) for k, v in ratios.items() if not v <= R_PPO["C"]}
    assert not over, over


# ---- 5. graph == eager

def test_graph_equals_eager(ms):
    """Three iterations: the graph trainer runs its first eagerly, captures, and replays the third."""
    want = _run(_trainer("4x4x3", 37, 6, episode_length=16), 3)
    g = _trainer("4x4x3", 37, 6, episode_length=16, use_graph=True)
    _assert_same(_run(g, 3), want, "graph")
    assert g.graph is not None and g.update_graph is not None


# ---- 6. the agents' nets start as without the auctioneer

def test_agent_nets_start_as_in_a_plain_trainer(ms):
    a, b = _trainer("4x4x3", 8, 4), _trainer("4x4x3", 8, 4, auct=False)
    assert b.auct is None and [u.name for u in b.units()] == ["acceptor", "offer"]
    assert b.auct_frag is None and b.auct_owner0 is None  # off: nothing allocated
    for ua, ub in ((a.acc, b.acc), (a.off, b.off)):
        for pol in ("policy", "policy_old"):
            for (k, p), (_, q) in zip(getattr(ua.group, pol).named_parameters(), getattr(ub.group, pol).named_parameters()):
                assert torch.equal(p, q), (ua.name, pol, k)
    pa = dict(a.auct.group.policy.named_parameters())
    assert a.auct.group.policy.G == 1 and tuple(pa["w1"].shape) == tuple(a.acc.group.policy.w1.shape)
    assert not torch.equal(pa["w1"], a.acc.group.policy.w1)
    assert a.auct.group.K == max(round(a.hp.raw_k_epochs / a.C), 1) and a.auct.group.gamma == a.acc.group.gamma


# ---- 7. checkpoint and exact resume

def test_checkpoint_resume(ms, tmp_path):
    path = str(tmp_path / "auct.ckpt")
    a = _trainer("4x4x3", 37, 6, episode_length=16)
    want = _run(a, 2)
    b = _trainer("4x4x3", 37, 6, episode_length=16)
    first = b.iteration()
    manifest = b.save_checkpoint(path) and _mod("checkpoint").read_file(path)[0]
    assert manifest["learned_auctioneer"] is True
    c = _trainer("4x4x3", 37, 6, episode_length=16)
    c.load_checkpoint(path)
    got = _state(c, [first, c.iteration()])
    _assert_same(got, want, "resume")
    plain = _trainer("4x4x3", 37, 6, episode_length=16, auct=False)
    before = _state(plain, [])
    for load in (plain.load_checkpoint, plain.load_policy):
        with pytest.raises(ValueError, match="learned_auctioneer"):
            load(path)
    _assert_same(_state(plain, []), before, "refused load")
    plain.iteration()
    plain.save_checkpoint(path)
    assert "learned_auctioneer" not in _mod("checkpoint").read_file(path)[0]
    for load in (c.load_checkpoint, c.load_policy):
        with pytest.raises(ValueError, match="learned_auctioneer"):
            load(path)


# ---- 8. evaluate()

def _hand_eval(t, learned):
    """evaluate(mode="greedy") restated: act_round_greedy for the agents, act_greedy on the emitted auctioneer rows
    with the common row, env.step(auctioneer=...)."""
    ev, ppo = _mod("evaluation"), _mod("ppo")
    episodes, seed, env, log = ev.fresh_env(t, 1, None, "greedy", ("greedy",), None)
    E, N, C, L = env.E, t.N, t.C, t.L
    s, dev = t.env.shape, t.device
    z = lambda *shape, dtype=torch.int8: torch.zeros(shape, dtype=dtype, device=dev)
    b = dict(offer=z(E, N * L, s.off_obs_stride), core_rows=z(E, C, s.acc_obs_stride), core_owner=z(E, C),
             auctioneer=z(E, C, s.acc_obs_stride))
    acc_a, off_a, au_a = z(E, N * C), z(E, N * L), z(E, C)
    rew = dict(offer=z(E, N, L, dtype=torch.float32), acceptor=z(E, N, C, dtype=torch.int32),
               agent=z(E, N, dtype=torch.int32), auctioneer=z(E, C, dtype=torch.int32))
    obs = env.reset(b)

    def one_round(r):
        ppo.act_round_greedy(t.off.group.policy_old, None, b["offer"], t.acc.group.policy_old, b["core_rows"],
                             b["core_owner"], t.acc_common, C, dict(core_action=off_a), acc_a)
        if learned:
            t.auct.group.policy_old.act_greedy(b["auctioneer"], C, common_row=t.acc_common, action=au_a)
        env.step(acc_a.view(E, N, C), off_a.view(E, N, L), auctioneer=au_a if learned else None, obs=obs, rewards=rew,
                 events=log.events[0])

    return ev.evaluation_result("greedy", seed, E, ev.run_episodes(log, episodes, one_round))


def _same_result(a, b):
    assert a["seed"] == b["seed"] and a["n_envs"] == b["n_envs"] and len(a["episodes"]) == len(b["episodes"])
    for x, y in zip(a["episodes"], b["episodes"]):
        assert x.keys() == y.keys()
        for k in x:
            assert np.array_equal(np.asarray(x[k]), np.asarray(y[k]), equal_nan=True), k


def test_evaluate(ms):
    t = _trainer("4x4x3", 37, 6, episode_length=16)
    t.iteration()
    before = (t.env.parts[0][0].export_state(), t.rng.getstate(), int(t.rng_ctr))
    r1, r2 = t.evaluate(mode="greedy"), t.evaluate(mode="greedy")
    assert r1["auctioneer"] == "learned" and r1["mode"] == "greedy"
    _same_result(r1, r2)
    _same_result(r1, _hand_eval(t, True))
    base = t.evaluate(mode="greedy", auctioneer="hardcoded")
    assert base["auctioneer"] == "hardcoded" and base["seed"] == r1["seed"]
    _same_result(base, _hand_eval(t, False))
    assert any(not np.array_equal(np.asarray(r1["episodes"][0][k]), np.asarray(base["episodes"][0][k]))
               for k in r1["episodes"][0])  # two different auctioneers
    s1 = t.evaluate(mode="sample", seed=11)
    _same_result(s1, t.evaluate(mode="sample", seed=11))
    assert t.evaluate(mode="hardcoded")["auctioneer"] == "hardcoded"
    after = (t.env.parts[0][0].export_state(), t.rng.getstate(), int(t.rng_ctr))
    _assert_same(after, before, "training state")
    with pytest.raises(ValueError, match="learned"):
        t.evaluate(mode="hardcoded", auctioneer="learned")
    plain = _trainer("4x4x3", 8, 4, auct=False)
    with pytest.raises(ValueError, match="learned_auctioneer"):
        plain.evaluate(auctioneer="learned")
    assert "auctioneer" not in plain.evaluate(mode="greedy")


# ---- the C calls' refusals (nothing is launched: the env's round stays)

def test_c_calls_refuse(ms):
    L = _mod("_lib")
    abi = ms.abi
    t = _trainer("4x4x3", 33, 4)
    env = t.env.parts[0][0]
    assert env.auct_supported() and t.fused_rollout
    E, N, C, Ls = t.E, t.N, t.C, t.L
    obs = dict(t._acc_out(1, 0, E), offer=t._off_obs[1])
    rew = dict(offer=t.off.rewards[0].view(E, N, Ls), acceptor=t.acc.rewards[0].view(E, N, C), agent=t.agent_reward,
               auctioneer=t.auct.rewards[0])
    a, o, r, _ = env._step_structs(t.acc.actions[0].view(E, N, C), t.off.actions[0].view(E, N, Ls), None,
                                   t.auct.actions[0], obs, rew, None)
    t._prepare_acting()
    b = lambda x: x.stride(0) * x.element_size()
    st = abi.MsRoundStrides(b(t.acc.actions), b(t.off.actions), b(t.acc_rows), b(t.acc_owner), b(t._off_obs),
                            b(t.off.rewards), b(t.acc.rewards), 0, b(t.auct.rewards), b(t.off.actions),
                            b(t.off.logprobs), b(t.acc.actions), b(t.acc.logprobs), 8)
    ast = abi.MsRoundStridesAuct(b(t.auct.actions), b(t.auct.actions), b(t.auct.logprobs))

    def call(h, a=a, nxt=None, au=None, rollout=True):
        nxt = nxt or t._fused_next(1, 0)
        au = au or t._fused_next_auct(1, 0)
        if rollout:
            return L.lib.ms_env_rollout_act_auct(h, ct.byref(a), ct.byref(o), ct.byref(r), None, ct.byref(nxt),
                                                 ct.byref(au), ct.byref(st), ct.byref(ast), 4, 0, L.stream_ptr())
        return L.lib.ms_env_step_act_auct(h, ct.byref(a), ct.byref(o), ct.byref(r), None, ct.byref(nxt), ct.byref(au),
                                          L.stream_ptr())

    def refused(rc, word):
        assert rc == abi.EINVAL and word in L.lib.ms_last_error(), (rc, L.lib.ms_last_error())

    for rollout in (True, False):
        no_ring = abi.MsActions.from_buffer_copy(a)
        no_ring.auctioneer = None
        refused(call(env._h, a=no_ring, rollout=rollout), b"auctioneer")
        au = t._fused_next_auct(1, 0)
        au.auct_logprob = None
        refused(call(env._h, au=au, rollout=rollout), b"NULL auctioneer output")
        for field, value in (("n_groups", 2), ("n_actions", 17), ("in_dim", 26), ("act_frag", None)):
            au = t._fused_next_auct(1, 0)
            setattr(au.auctioneer, field, value)
            refused(call(env._h, au=au, rollout=rollout), b"auctioneer net")
        free = _mod("env").BatchedEnv(abi.named_config("cfg3"), 8, seed=1, device=t.device)
        refused(call(free._h, rollout=rollout), b"fixed-price")
    wide = _trainer("6x5x2", 40, 4)  # 4 replicas a wave, 120 acceptor items: outside the fused kernels' range
    wenv = wide.env.parts[0][0]
    assert not wenv.auct_supported() and not wide.fused_step
    wide._prepare_acting()
    refused(call(wenv._h, nxt=wide._fused_next(1, 0), au=wide._fused_next_auct(1, 0)), b"shape not supported")
    torch.cuda.synchronize()
    assert env.round == 0 and wenv.round == 0
