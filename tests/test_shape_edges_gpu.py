"""The env round and the fused rollouts at the edges of the shapes their launches choose a kernel by.

launch_env_step and the three fused launches (env_kernels.hip) pick the lanes per replica (16 / 32 / 64 from
max(N, C), widened for 1024 <= E with too few waves), FixShape or DynShape, and the fused paths by the support
predicates env_step_act_supported / env_rollout_free_supported. The other suites run these at the BASELINE shapes;
the cases here sit on the boundaries: lane counts 16|17 and 32|33, N = 1, L = 1, N = C = 64, O = 126, partial last
waves and workgroups, each term of the predicates at and just past equality, and MT19937 block crossings at small
shapes (the successor twist writes 4 * 624 B of LDS at the start of a round, the largest LDS user of a small shape).
Every comparison is bit-exact: against the C oracle, and between the fused and the two-launch device paths."""
import importlib

import numpy as np
import pytest
import torch

from tests.drivers import step_rounds_vs_oracle
from tests.replay import oracle_replay, set_mt_index
from tests.test_configs_gpu import _actions
from tests.test_rollout_free_gpu import _compare, _trainers

pytestmark = pytest.mark.gpu

JOBS = dict(priorities=[3, 10, 7], lengths=[6, 3, 2], probabilities=[0.5, 0.3, 0.2])


def _cfg(abi, N, C, L, free):
    if free:
        return abi.make_config(N, C, L, free_prices=True, commercial=True, **JOBS)
    return abi.make_config(N, C, L, fix_prices=[2, 7, 4], **JOBS)


def _stagger_mt(genv, oenvs, replicas):
    """Replica e's stream to 3 * (1 + e % 4) words before its block's end, on the device and in the oracles
    (oenvs[i] is replica replicas[i]): the replicas of a wave cross in different rounds, so after round 0 the
    refill runs for partial masks. Returns the imported MT words [E][624]."""
    st = genv.export_state()
    st["mt_index"][:] = 624 - 3 * (1 + np.arange(genv.E) % 4)
    genv.import_state(st)
    for o, e in zip(oenvs, replicas):
        o.import_state({k: v[e] for k, v in st.items()})
    return st["mt"].copy()


def _wrapped(env, mt0):
    """Every replica's current MT19937 block is no longer the imported one."""
    return bool((env.export_state()["mt"] != mt0).any(axis=1).all())


# ---- (a) ms_env_step against the oracle

STEP_CASES = [
    (1, 1, 16, 7),    # N = 1, C = 1; four replicas per wave, the last wave 3 of 4
    (2, 3, 1, 5),     # L = 1
    (16, 16, 1, 7),   # top of 16 lanes, generic kernel
    (17, 3, 2, 3),    # first 32-lane shape by N; the last wave 1 of 2
    (3, 17, 2, 3),    # ... and by C
    (32, 32, 1, 3),   # top of 32 lanes, generic kernel
    (33, 5, 2, 2),    # first 64-lane shape by N
    (5, 33, 2, 2),    # ... and by C
    (64, 64, 1, 2),   # the API's largest N and C
    (63, 2, 2, 5),    # O = 126 = MS_MAX_OFFERS: acceptor rows of 255 B, action 126 in an int8
]


@pytest.mark.parametrize("free", [False, True], ids=["fixed", "free"])
@pytest.mark.parametrize("N,C,L,E", STEP_CASES)
def test_step_at_shape_edges_vs_oracle(ms, oracle, N, C, L, E, free):
    """60 rounds of the loop of test_env_gpu.py::test_step_bit_exact_vs_oracle (observations, every reward kind
    and the events each round, the whole state incl. the 624 MT words every 20 rounds), every replica starting a
    few words before its MT block's end. The run must have executed offers, crossed a block in every replica
    and fed the largest legal action of every kind."""
    cfg = _cfg(ms.abi, N, C, L, free)
    s = ms.abi.config_shape(cfg)
    seed = 7
    genv = ms.BatchedEnv(cfg, E, seed=seed)
    oenvs = [oracle.OracleEnv(cfg, seed + e) for e in range(E)]
    mt0 = _stagger_mt(genv, oenvs, range(E))
    seen = step_rounds_vs_oracle(ms, genv, oenvs, 60, np.random.default_rng(1), state_every=20)
    assert genv.flags() == 0
    assert genv.round == 60
    assert seen["executed"] > 0
    assert _wrapped(genv, mt0)
    assert seen["acceptor"] == s["O"] and seen["core"] == C
    if free:
        assert seen["price"] == s["price_actions"] - 1


@pytest.mark.parametrize("E", [1023, 1030, 2100])
def test_step_widened_lanes_vs_oracle(ms, oracle, E):
    """6 x 6 x 3 with free prices (the generic kernel) on either side of the widening rule of lanes_per_env
    (1024 <= E and fewer than 2048 waves: double the lanes while the launch stays within 2048 waves):
      E = 1023: 16 lanes (below 1024 replicas), the last wave 3 of 4 replicas;
      E = 1030: 64 lanes (1030 waves);
      E = 2100: 32 lanes (1050 waves; 64 lanes would be 2100 > 2048).
    Replicas 0, 1, E / 2, E - 2, E - 1 against the oracle for 40 rounds."""
    cfg = _cfg(ms.abi, 6, 6, 3, True)
    s = ms.abi.config_shape(cfg)
    T, seed = 40, 13
    sample = [0, 1, E // 2, E - 2, E - 1]
    genv = ms.BatchedEnv(cfg, E, seed=seed)
    oenvs = [oracle.OracleEnv(cfg, seed + e) for e in sample]
    mt0 = _stagger_mt(genv, oenvs, sample)
    d = genv.device
    idx = torch.tensor(sample, device=d)
    bufs = genv.obs_buffers(auctioneer=True)
    g = torch.Generator(device=d)
    g.manual_seed(17)
    n_exec = 0
    for t in range(T):
        acc, off, pr = _actions(g, s, E, d)
        obs, rew, _ = genv.step(acc, off, pr, obs=bufs)
        a_np, o_np, p_np = (x.index_select(0, idx).cpu().numpy() for x in (acc, off, pr))
        gobs = {k: obs[k].index_select(0, idx).cpu().numpy() for k in ("acceptor", "offer", "auctioneer")}
        grew = {k: v.index_select(0, idx).cpu().numpy() for k, v in rew.items() if v is not None}
        for j, e in enumerate(sample):
            ores = oenvs[j].step(a_np[j], o_np[j], p_np[j])
            ob = oenvs[j].observe()
            np.testing.assert_array_equal(gobs["acceptor"][j, :, :, : s["acc_obs_dim"]], ob["acceptor"], err_msg="acc t=%d e=%d" % (t, e))
            np.testing.assert_array_equal(gobs["offer"][j, :, :, : s["off_obs_dim"]], ob["offer"], err_msg="off t=%d e=%d" % (t, e))
            np.testing.assert_array_equal(gobs["auctioneer"][j, :, : s["acc_obs_dim"]], ob["auctioneer"], err_msg="auct t=%d e=%d" % (t, e))
            for k in ("acceptor", "offer", "price", "auctioneer", "agent"):
                np.testing.assert_array_equal(grew[k][j], ores[k], err_msg="%s reward t=%d e=%d" % (k, t, e))
            n_exec += int((ores["accepted"]["valid"] == 1).sum())
    assert genv.flags() == 0
    assert n_exec > 0
    st = genv.export_state()
    for j, e in enumerate(sample):
        ost = oenvs[j].export_state()
        for k in ("round", "core_owner", "core_kind", "core_rem", "slot_kind", "slot_rem", "slot_wait", "offer_core",
                  "offer_recip", "offer_price", "liab_n", "mt_index"):
            np.testing.assert_array_equal(st[k][e], ost[k], err_msg="%s env %d" % (k, e))
        np.testing.assert_array_equal(st["mt"][e], ost["mt"], err_msg="mt env %d" % e)
    assert bool((st["mt"] != mt0).any(axis=1).all())


# ---- (b) the fused fixed-price step and rollout (ms_env_step_act, ms_env_rollout_act)

def _rings(t):
    out = {"acceptor_rows": t.acceptor_rows(), "off_obs": t.off_obs}
    for u in t.units():
        for k in ("actions", "logprobs", "rewards"):
            out["%s.%s" % (u.name, k)] = getattr(u, k)
    return out


def _global_trainer(ms, N, C, L, E, seed=9):
    tr_mod = importlib.import_module("marl-scheduling_amd.trainer")
    return tr_mod.Trainer(_cfg(ms.abi, N, C, L, False), E, arch="global",
                          hyper=tr_mod.Hyper(update_step=12, raw_k_epochs=2), seed=seed, device="cuda:0")


FUSED_CASES = [
    (2, 4, 7, 96),     # 16 lanes: epw * C = 16, O = 14 (the acting's largest), the generic kernel of cfg2's lanes
    (14, 1, 1, 99),    # 16 lanes by N, C = 1, L = 1; a last wave of 3 replicas
    (1, 4, 14, 50),    # N = 1: epw * C = 16, O = 14; a last wave of 2 replicas
    (4, 8, 3, 2100),   # 32 lanes by widening: epw * N * C = 64 and epw * C = 16, DynShape
    (4, 15, 3, 1030),  # 64 lanes by widening: 16 core actions and 32-byte offer rows (the acting's largest), N * C = 60
]


@pytest.mark.parametrize("N,C,L,E", FUSED_CASES)
def test_fused_env_act_equals_two_launches_at_shape_edges(ms, monkeypatch, N, C, L, E):
    """The three-way comparison of test_compact_variants_gpu.py::test_fused_env_act_equals_two_launches (whole
    rollout in one launch, fused per round, act launch + env launch; rings, losses and the exported env state over
    two iterations) away from 4 x 4 x 3, plus three replicas of the first rollout replayed through the C oracle.

    Shapes: the fused acting needs, besides env_step_act_supported's epw * N * C <= 64, epw * N * L <= 64 and
    epw * C <= 16 (epw = 64 / lanes), rows of one k-step and one action tile (ms_env_step_act_supported:
    acc_stride <= 32, so O <= 14; C + 1 <= 16; off_stride <= 32). 4 x 4 x 4, 16 x 1 x 1, 1 x 4 x 16, 32 x 1 x 1 and
    4 x 16 x 16 all have O >= 16 (or C = 16), so no Trainer fuses them; the cases are the nearest shapes that do
    fuse and keep the edge: O at 14 instead of 16 (2 x 4 x 7, 14 x 1 x 1, 1 x 4 x 14; with O <= 14 the term
    epw * N * L stays <= 56), 32 lanes by widening instead of by N (max(N, C) >= 17 means O >= 17 or C + 1 > 16),
    and 4 x 15 x 3 for 4 x 16 x 16 (C = 15 and off_stride = 32 are the acting's limits)."""
    tr_mod = importlib.import_module("marl-scheduling_amd.trainer")
    seed = 9
    whole = _global_trainer(ms, N, C, L, E, seed)
    monkeypatch.setenv("MS_ENV_ROLLOUT", "0")
    per_round = _global_trainer(ms, N, C, L, E, seed)
    monkeypatch.setenv("MS_ENV_FUSED_ACT", "0")
    plain = _global_trainer(ms, N, C, L, E, seed)
    assert whole.fused_rollout and per_round.fused_step and not per_round.fused_rollout and not plain.fused_step
    trs = (whole, per_round, plain)
    for it in range(2):
        for t in trs:
            t.rollout()
        torch.cuda.synchronize()
        rings = [_rings(t) for t in trs]
        for k in rings[0]:
            for r in rings[1:]:
                assert torch.equal(rings[0][k], r[k]), (it, k)
        if it == 0:
            oracle_replay(whole, (0, E // 2 + 1, E - 1), tr_mod.env_seed(seed, 0, E), whole.T)
        losses = [t.update() for t in trs]
        for k in losses[0]:
            for l in losses[1:]:
                assert torch.equal(losses[0][k], l[k]), (it, k)
    assert all(t.flags() == 0 for t in trs)
    st = [t.env.parts[0][0].export_state() for t in trs]
    for k in st[0]:
        for o in st[1:]:
            assert (st[0][k] == o[k]).all(), k


UNFUSED_CASES = [
    (4, 4, 5, 96),      # epw * N * L = 80
    (5, 4, 3, 96),      # epw * N * C = 80
    (5, 4, 2, 96),      # ... with every other term inside (O = 10)
    (3, 5, 3, 96),      # epw * C = 20, every other term inside
    (4, 16, 16, 1000),  # 16 lanes below 1024 replicas
    (4, 15, 3, 1000),   # the fused case above without the widening: epw = 4
]


@pytest.mark.parametrize("N,C,L,E", UNFUSED_CASES)
def test_shapes_just_outside_the_fused_step(ms, N, C, L, E):
    """One term past env_step_act_supported the trainer runs the act launch and the env launch of every round:
    one rollout, replayed through the C oracle."""
    tr_mod = importlib.import_module("marl-scheduling_amd.trainer")
    t = _global_trainer(ms, N, C, L, E)
    assert not t.fused_step and not t.fused_rollout
    assert not t.env.parts[0][0].fused_act_supported()
    t.rollout()
    torch.cuda.synchronize()
    assert t.flags() == 0
    oracle_replay(t, (0, E // 2 + 1, E - 1), tr_mod.env_seed(9, 0, E), t.T)


# ---- (c) the fused free-price rollout (ms_env_rollout_act_free)

def _local_trainer(ms, N, C, L, E, seed=4):
    tr_mod = importlib.import_module("marl-scheduling_amd.trainer")
    return tr_mod.Trainer(_cfg(ms.abi, N, C, L, True), E, arch="local",
                          hyper=tr_mod.Hyper(update_step=16, raw_k_epochs=2), seed=seed, device="cuda:0")


FREE_CASES = [
    (1, 1, 16, 130, "1"),  # one wave whose env slot (4 * 608 B) is shorter than an MT block: pdig behind padding
    (1, 1, 16, 130, "0"),
    (2, 1, 8, 130, "1"),   # slots of 2560 B: the tightest fit of two waves
    (8, 1, 2, 100, "1"),   # N = 8 with C = 1; a last workgroup of 4 of 32 replicas
    (8, 11, 2, 70, "1"),   # the largest C within the LDS bound at N = 8, L = 2
    (1, 15, 16, 40, "1"),  # the largest C: 16 core actions
    (1, 15, 16, 42, "1"),  # ... with a last workgroup of 2 of 4 replicas
    (3, 15, 10, 50, "1"),  # O = 30: 31 acceptor actions, acc_stride 64
]


@pytest.mark.parametrize("N,C,L,E,own", FREE_CASES)
def test_free_rollout_at_predicate_edges(ms, monkeypatch, N, C, L, E, own):
    """The one-launch rollout against the two-launch trainer (test_rollout_free_gpu.py's comparison: every ring,
    loss and weight and the env state over two iterations) at the edges of env_rollout_free_supported, and three
    replicas of the first rollout against the C oracle. Every replica starts at index 623 of its MT block: the
    first draw crosses it in round 0, and the next successor is twisted at the start of a later round of the
    launch, when the workgroup's digit table and the other waves' slots are live.
    (1 x 1 x 16 also passed before free_lds padded the table behind the twist: the 64 B the twist overran hold the
    digits of byte values -128 .. -97 of the first price-state byte, which no state holds. The layout itself is
    checked for every shape by tests/test_lds_plan.py.)"""
    tr_mod = importlib.import_module("marl-scheduling_amd.trainer")
    monkeypatch.setenv("MS_FILL_OWN", own)
    seed = 4
    trs = _trainers(monkeypatch, lambda: _local_trainer(ms, N, C, L, E, seed))
    assert (trs[0].acc_own is not None) == (own == "1")
    for t in trs:
        set_mt_index(t.env.parts[0][0], 623)
    mt0 = trs[1].env.parts[0][0].export_state()["mt"].copy()

    def after_rollout(it):
        if it == 0:
            assert _wrapped(trs[1].env.parts[0][0], mt0)
            oracle_replay(trs[0], (0, E // 2 + 1, E - 1), tr_mod.env_seed(seed, 0, E), trs[0].T, mt_index=623)

    _compare(trs, after_rollout=after_rollout)


NOT_FREE_CASES = [
    (8, 12, 2, 70),   # the LDS bound
    (1, 1, 15, 130),  # O + 1 = 16: the acceptor's actions fit one tile
    (2, 16, 4, 130),  # C = 16: 17 core actions
    (1, 1, 31, 130),  # acc_stride 68
]


@pytest.mark.parametrize("N,C,L,E", NOT_FREE_CASES)
def test_shapes_just_outside_the_free_rollout(ms, N, C, L, E):
    """One step past each term of env_rollout_free_supported: the env refuses the one-launch rollout, the trainer
    runs the two launches per round; one iteration, its rollout replayed through the C oracle."""
    tr_mod = importlib.import_module("marl-scheduling_amd.trainer")
    t = _local_trainer(ms, N, C, L, E)
    assert not t.env.parts[0][0].rollout_free_supported()
    assert not t.fused_rollout_free
    t.rollout()
    torch.cuda.synchronize()
    oracle_replay(t, (0, E // 2 + 1, E - 1), tr_mod.env_seed(4, 0, E), t.T)
    losses = t.update()
    for k, v in losses.items():
        assert torch.isfinite(v).all(), k
    assert t.flags() == 0
