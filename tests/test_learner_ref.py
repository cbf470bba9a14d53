"""oracle/learner_ref.py on the CPU: the float64 references of ms_bdqn_update, ms_dqn_grad and ms_dqn_act against
torch autograd (float64 tightly, float32 and the existing restatements oracle/bdqn_ref.py and oracle/dqn_ref.py at
the tolerances of tests/test_bdqn_gpu.py and tests/test_dqn_gpu.py), the Philox restatement against Random123's
known answers, and for every case of the tables tests/test_learner_parity_gpu.py runs: the conditions that keep it
off the discontinuities, and that the tables reach every edge they were built for."""
import numpy as np
import pytest
import torch

from oracle import learner_ref as lr
from oracle.bdqn_ref import RefBranchingQNetwork, update_policy_reference
from oracle.dqn_ref import RefDQNEntity, optimize_model_reference


def _maxabs(a):
    return float(np.abs(a).max()) if np.size(a) else 0.0


# ------------------------------------------------------------------------------------------------ Philox

def test_philox_known_answers():
    """The three philox4x32-10 vectors of Random123's kat_vectors. Neither torch nor numpy ships a published
    Philox4x32 vector to read them from (numpy's test data holds Philox4x64 vectors only), so they are written
    out in learner_ref.PHILOX_KAT; a restatement that reproduces all twelve words cannot do so by accident."""
    for ctr, key, want in lr.PHILOX_KAT:
        got = lr.philox4x32_10(*[np.array([c]) for c in ctr], *[np.array([k]) for k in key])
        assert tuple(int(g[0]) for g in got) == want


def test_u53_and_counter_layout():
    assert lr.u53(0, 0) == 0.0
    assert lr.u53(0xffffffff, 0xffffffff) == 1.0 - 2.0 ** -53
    assert lr.u53(1 << 5, 0) == 2.0 ** -27 and lr.u53(0, 1 << 6) == 2.0 ** -53
    # row in counter words 0 and 1, offset in words 2 and 3, seed in the key
    seed, off = 0x0123456789abcdef, (5 << 32) + 7
    u1, u2 = lr.dqn_act_uniforms(3, seed, off)
    o = lr.philox4x32_10([2], [0], [7], [5], [0x89abcdef], [0x01234567])
    assert u1[2] == lr.u53(o[0], o[1])[0] and u2[2] == lr.u53(o[2], o[3])[0]
    assert len({float(x) for x in u1} | {float(x) for x in u2}) == 6


# ------------------------------------------------------------------------------------------ Branching DQN

@pytest.mark.parametrize("name", list(lr.BDQN_CASES))
def test_bdqn_case_conditions_and_reference(name):
    c = lr.bdqn_case(name)
    cfg, ref = c["cfg"], c["ref"]
    B = cfg["B"]
    # the argmax rule: every near-tie row is masked, and at most a tenth of the rows are masked this way
    near = (ref["argmax_gap"] < lr.ARGMAX_GAP * ref["qn_scale"]).any(axis=1)
    assert (c["masks"][near] == 0).all()
    assert c["tie_masked"].mean() <= 0.10, c["tie_masked"].mean()
    assert np.array_equal(near, c["tie_masked"])
    # the ReLU kink: every row of q(s), both layers
    assert ref["relu_rel"].shape == (B,) and (ref["relu_rel"] >= lr.RELU_MARGIN).all(), ref["relu_rel"].min()
    assert (ref["relu_margin"] > 0).all()
    # the reference against float64 autograd, and float32 autograd at the existing tolerance
    args = (c["q"], c["t"], c["xs"], c["xn"], c["actions"], c["rewards"], c["masks"], cfg["gamma"], cfg["clip"])
    l64, g64 = lr.bdqn_update_torch(*args, dtype=torch.float64)
    l32, g32 = lr.bdqn_update_torch(*args, dtype=torch.float32)
    assert abs(l64 - ref["loss"]) <= 1e-12 * abs(ref["loss"])
    assert abs(l32 - ref["loss"]) <= 1e-5 * abs(ref["loss"])
    for k in lr.BDQN_KEYS:
        want = ref["grads"][k]
        scale = _maxabs(want)
        assert g64[k].shape == want.shape, k
        assert _maxabs(g64[k] - want) <= 1e-11 * scale, (k, _maxabs(g64[k] - want), scale)
        assert _maxabs(g32[k] - want) <= 1e-4 * scale + 1e-7 * max(1.0, cfg["wscale"] ** 3), k
    if name == "clip-small":  # more than a tenth of the elements sit on the clamp
        sat = sum(int((np.abs(ref["raw"][k]) > cfg["clip"]).sum()) for k in lr.BDQN_KEYS)
        assert sat > 0.1 * sum(ref["raw"][k].size for k in lr.BDQN_KEYS)
    if cfg["clip"] > 0:
        assert all(_maxabs(ref["grads"][k]) <= cfg["clip"] for k in lr.BDQN_KEYS)
    else:
        assert all(np.array_equal(ref["grads"][k], ref["raw"][k]) for k in lr.BDQN_KEYS)


@pytest.mark.parametrize("name", ["B128", "B33", "heads65", "n1", "ac32"])
def test_bdqn_reference_matches_update_policy_restatement(name):
    """oracle/bdqn_ref.update_policy_reference (gamma 0.99, clamp 1, then an optimiser step: SGD at lr 0 here, so
    the clamped .grad stays to be read) at the tolerances of tests/test_bdqn_gpu.py."""
    c = lr.bdqn_case(name)
    cfg, ref = c["cfg"], c["ref"]
    assert cfg["gamma"] == 0.99 and cfg["clip"] == 1.0
    nets = []
    for w in (c["q"], c["t"]):
        net = RefBranchingQNetwork(cfg["obs"], cfg["ac"], cfg["n"])
        net.load_stacked({k: torch.tensor(v) for k, v in w.items()})
        nets.append(net)
    opt = torch.optim.SGD(nets[0].parameters(), lr=0.0)
    loss = update_policy_reference(nets[0], nets[1], opt, torch.tensor(c["xs"]).float(),
                                   torch.tensor(c["actions"].astype(np.int64)), torch.tensor(c["rewards"]),
                                   torch.tensor(c["xn"]).float(), torch.tensor(c["masks"]))
    assert abs(float(loss) - ref["loss"]) <= 1e-4 * max(1.0, abs(ref["loss"]))
    got = nets[0].stacked()
    for k in lr.BDQN_KEYS:
        if k in ("wa", "ba"):
            g = torch.cat([getattr(h, "weight" if k == "wa" else "bias").grad for h in nets[0].adv_heads])
        else:
            g = got[k].grad
        want = ref["grads"][k]
        assert _maxabs(g.double().numpy() - want) <= 1e-4 * _maxabs(want) + 1e-7, k


def test_bdqn_tie_case():
    """The exact-tie case: in both branches the duplicated pair is the maximum of every row with a gap of exactly
    zero, the third value is far below, the first index is the reference's pick, and taking the other index
    would move the loss by far more than any tolerance."""
    c = lr.bdqn_tie_case()
    ref, n = c["ref"], c["cfg"]["n"]
    assert (ref["argmax_gap"] == 0.0).all()
    assert (c["third_gap"] > 1.0).all()
    for m, (j, k) in enumerate(lr.TIE["pairs"]):
        assert j < k and (c["argmax"][:, m] == j).all()
        assert np.array_equal(c["q"]["wa"][m * n + j], c["q"]["wa"][m * n + k])
        assert c["q"]["ba"][m * n + j] == c["q"]["ba"][m * n + k]
    (j0, k0), (j1, k1) = lr.TIE["pairs"]
    assert j0 // 64 != k0 // 64 and j1 // 64 == k1 // 64  # across two 64-lane strides, and within one
    assert (ref["relu_rel"] >= lr.RELU_MARGIN).all()
    assert abs(c["ref_last"]["loss"] - ref["loss"]) > 0.1 * abs(ref["loss"])


def test_bdqn_table_covers_every_edge():
    """Every path of bdqn_update_kernels.hip the table was built to cross is crossed by some case."""
    cs = [dict(lr.bdqn_case(n)["cfg"]) for n in lr.BDQN_CASES]
    for c in cs:
        c["ld"] = c["ld"] or c["obs"]
        c["act_ld"] = c["act_ld"] or c["ac"]
        c["Mn"] = c["ac"] * c["n"]
        c["Mp"] = (c["Mn"] + 1 + 63) // 64 * 64
        c["nK"] = (c["obs"] + 127) // 128
    has = lambda f: any(f(c) for c in cs)
    assert {c["B"] for c in cs} >= {1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128}
    assert {c["obs"] for c in cs} >= {1, 7, 8, 9, 31, 32, 33, 127, 128, 129, 255, 256, 257, 512, 513, 1024, 1025}
    # k_bdqn_upd_l1 / _w1 load paths: (ld & 7, obs & 3) vector or scalar, ld == obs and ld > obs; _w1's ld & 3
    for ld8 in (True, False):
        for o4 in (True, False):
            for wide in (True, False):
                if ld8 and not o4 and not wide:
                    continue  # ld == obs with ld % 8 == 0 has obs % 4 == 0
                assert has(lambda c: (c["ld"] % 8 == 0) == ld8 and (c["obs"] % 4 == 0) == o4 and (c["ld"] > c["obs"]) == wide), (ld8, o4, wide)
    assert has(lambda c: c["ld"] % 4 != 0) and has(lambda c: c["ld"] % 4 == 0 and c["obs"] % 64 == 0)
    # the partial last 32-wide k-step (every count 1 .. 4 of the last chunk) and chunk counts across the 4-unroll
    assert {min(4, (c["obs"] - (c["nK"] - 1) * 128 + 31) // 32) for c in cs} == {1, 2, 3, 4}
    assert has(lambda c: c["obs"] % 32 != 0 and c["obs"] % 8 != 0) and has(lambda c: c["obs"] % 32 == 0)
    assert {c["nK"] for c in cs} >= {1, 2, 3, 4, 5, 8, 9}
    # head rows padded to Mp: the value row last in its 64-block, first in a new one, and in between; Mp / 64
    # across the 8-unroll of k_bdqn_upd_back1
    assert {c["Mn"] + 1 for c in cs} >= {63, 64, 65, 512, 513}
    assert {c["Mp"] // 64 for c in cs} >= {1, 2, 8, 9}
    # the 64-lane strided mean and argmax
    assert {c["n"] for c in cs} >= {1, 2, 63, 64, 65, 127, 128}
    assert {c["ac"] for c in cs} >= {1, 4, 5, 32}
    assert has(lambda c: c["actions"] == "zero") and has(lambda c: c["actions"] == "last")
    assert has(lambda c: c["act_ld"] > c["ac"])
    assert has(lambda c: c["lo"] == -128 and c["hi"] == 127)
    assert {c["wscale"] for c in cs} >= {1e-3, 1.0, 1e2}
    assert {c["gamma"] for c in cs} >= {0.0, 0.99}
    assert has(lambda c: c["masks"] == "zero")
    assert has(lambda c: c["clip"] == 0.0) and has(lambda c: c["clip"] == 1.0) and has(lambda c: 0 < c["clip"] < 1)


# ---------------------------------------------------------------------------------------------------- DQN

def _grad_args(c):
    return (c["pol"], c["tgt"], c["states"], c["next_states"], c["actions"], c["rewards"], c["samples"], c["D"],
            c["upg"], c["gamma"], c["clip"])


@pytest.mark.parametrize("name", list(lr.DQN_GRAD_CASES))
def test_dqn_grad_case_conditions_and_reference(name):
    c = lr.dqn_grad_case(name)
    ref = c["ref"]
    rows = c["upg"] * c["E"] * c["B"]
    assert all(r["absd"].shape == (rows,) for r in ref)
    # both SmoothL1 branches: at least a tenth of the case's rows each (over its groups: the one-row case has one
    # row per group, one in each branch)
    ad = np.concatenate([r["absd"] for r in ref])
    assert (ad < 1).mean() >= 0.1 and (ad > 1).mean() >= 0.1, ((ad < 1).mean(), (ad > 1).mean())
    assert all(np.isfinite(r["gap"]).all() or c["A"] == 1 for r in ref)
    t64 = lr.dqn_grad_torch(*_grad_args(c), dtype=torch.float64)
    t32 = lr.dqn_grad_torch(*_grad_args(c), dtype=torch.float32)
    for g in range(c["G"]):
        assert abs(t64[g][0] - ref[g]["loss"]) <= 1e-12 * max(1.0, abs(ref[g]["loss"]))
        assert abs(t32[g][0] - ref[g]["loss"]) <= 1e-5 * max(1.0, abs(ref[g]["loss"]))
        for k in lr.DQN_KEYS:
            want = ref[g]["grads"][k]
            assert _maxabs(t64[g][1][k] - want) <= 1e-11 * _maxabs(want), (g, k)
            assert _maxabs(t32[g][1][k] - want) <= 1e-4 * _maxabs(want) + 1e-7, (g, k)
    # the groups' nets differ, and so do their results: a wrong group index shows
    assert c["G"] >= 2 and not np.array_equal(c["pol"]["w1"][0], c["pol"]["w1"][1])
    assert ref[0]["loss"] != ref[1]["loss"]


@pytest.mark.parametrize("name", ["D5", "A97", "rows513", "clip0"])
def test_dqn_reference_matches_optimize_model_restatement(name):
    """oracle/dqn_ref.optimize_model_reference (SGD at lr 0 for its optimiser, so .grad stays) at the tolerances
    of tests/test_dqn_gpu.py."""
    c = lr.dqn_grad_case(name)
    for g in range(c["G"]):
        pol = RefDQNEntity(*[torch.tensor(c["pol"][k][g]) for k in lr.DQN_KEYS])
        tgt = RefDQNEntity(*[torch.tensor(c["tgt"][k][g]) for k in lr.DQN_KEYS])
        s, s1, a, r = lr.dqn_gather(c["states"], c["next_states"], c["actions"], c["rewards"], c["samples"], c["D"],
                                    c["upg"], g)
        loss = optimize_model_reference(pol, tgt, torch.optim.SGD(pol.parameters(), lr=0.0),
                                        torch.tensor(s.astype(np.int64)), torch.tensor(a.astype(np.int64)),
                                        torch.tensor(s1.astype(np.int64)), torch.tensor(r.astype(np.int64)),
                                        c["gamma"], clip=c["clip"] > 0)
        assert abs(float(loss) - c["ref"][g]["loss"]) <= 1e-5 * max(1.0, abs(c["ref"][g]["loss"]))
        for k, p in zip(lr.DQN_KEYS, pol.params()):
            want = c["ref"][g]["grads"][k]
            assert _maxabs(p.grad.double().numpy() - want) <= 1e-4 * _maxabs(want) + 1e-7, (g, k)


@pytest.mark.parametrize("name", list(lr.DQN_ACT_CASES))
def test_dqn_act_case_conditions(name):
    c = lr.dqn_act_case(name)
    A, eps = c["A"], lr.ACT_EPS
    assert c["clear"].mean() >= 0.95
    flat = lambda x: x.reshape(-1)
    assert flat(c["clear"])[:4].all()  # the rows that carry the rule's edges are compared
    u1, u2 = c["uniforms"]
    assert u1[0] == eps and flat(c["explore"])[0] and u1[1] > eps and u1[1] == np.nextafter(eps, 1) and not flat(c["explore"])[1]
    if A > 1:  # the other branch of the rule would give another action
        assert flat(c["action"])[0] != flat(c["greedy"])[0] and int(u2[1] * A) != flat(c["greedy"])[1]
    assert flat(c["action"])[1] == flat(c["greedy"])[1]
    assert u2[2] == 1 - 2.0 ** -53 and flat(c["action"])[2] == A - 1 and flat(c["action"])[3] == 0
    assert ((u1 >= 0) & (u1 < 1) & (u2 >= 0) & (u2 < 1)).all()
    assert (flat(c["action"]) >= 0).all() and (flat(c["action"]) < A).all()
    # float32 torch agrees with the float64 argmax on the clear rows
    with torch.no_grad():
        for u in range(c["U"]):
            net = RefDQNEntity(*[torch.tensor(c["net"][k][u // c["upg"]]) for k in lr.DQN_KEYS])
            q32 = net(torch.tensor(c["obs"][:, u, :c["D"]].astype(np.int64)))
            ok = c["clear"][:, u]
            assert np.array_equal(q32.argmax(1).numpy()[ok], c["greedy"][:, u][ok])


def test_dqn_act_rule_edges():
    greedy = np.array([3, 3, 3, 3])
    act, ex = lr.dqn_act_rule(greedy, [0.4, np.nextafter(0.4, 1), 0.0, float("nan")], [0.0, 0.0, 1 - 2.0 ** -53, 0.5],
                              0.4, 7)
    assert ex.tolist() == [True, False, True, True] and act.tolist() == [0, 3, 6, 3]  # !(nan > eps) explores


def test_dqn_tables_cover_every_edge():
    gs = [lr.dqn_grad_case(n) for n in lr.DQN_GRAD_CASES]
    assert {c["D"] for c in gs} >= {1, 3, 4, 5, 60, 195, 256} and {c["A"] for c in gs} >= {1, 2, 97, 127}
    assert {c["upg"] * c["E"] * c["B"] for c in gs} >= {1, 255, 256, 257, 513}
    assert {c["upg"] for c in gs} >= {1, 3} and any(c["cap"] == 2 for c in gs) and any(c["B"] == 1 for c in gs)
    assert {c["clip"] for c in gs} >= {0.0, 1.0, float("inf")}
    assert any(c["stride"] > lr.align4(c["D"]) for c in gs)
    assert all(c["stride"] % 4 == 0 and c["stride"] >= c["D"] for c in gs)
    lds = [lr.dqn_grad_lds(c["D"], c["A"]) for c in gs]
    assert max(lds) == 154616 and sum(x > 64 * 1024 for x in lds) >= 3 and max(lds) <= 160 * 1024
    assert any(c["D"] == 256 and c["A"] == 127 for c in gs)
    acts = [lr.dqn_act_case(n) for n in lr.DQN_ACT_CASES]
    assert {c["D"] for c in acts} >= {1, 3, 4, 5, 60, 195, 256} and {c["A"] for c in acts} >= {1, 2, 97, 127}
    assert {c["E"] for c in acts} >= {1, 255, 256, 257}
    assert any(c["D"] == 256 and c["A"] == 127 for c in acts) and any(c["stride"] > lr.align4(c["D"]) for c in acts)
