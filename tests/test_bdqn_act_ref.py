"""oracle/bdqn_act_ref.py on the CPU: the float64 reference of Branching-DQN acting against torch float64
RefBranchingQNetwork (oracle/bdqn_ref.py) tightly, its float32 restatement against the same at the tolerance of
tests/test_bdqn_gpu.py, dense_rows + layer1 against layer1_compact_reference, and for every case of the tables
tests/test_bdqn_act_parity_gpu.py runs: that the float32 restatement's own argmax stays within the pick cap, that
the ownership patterns and tie cases are what their names say, and that the tables reach every edge of the launch
plan of bdqn_kernels.hip they were built for (computed from the shapes by act_plan / l1_plan)."""
import numpy as np
import pytest
import torch

from oracle import bdqn_act_ref as br
from oracle.bdqn_ref import RefBranchingQNetwork, layer1_compact_reference
from oracle.learner_ref import BDQN_KEYS, align4

PICK_CAP = 0.005  # of a case's (row, branch) entries: float32 argmax != float64 argmax


def _maxabs(a):
    return float(np.abs(a).max()) if np.size(a) else 0.0


def _cases():
    out = [("H", n) for n in br.H_CASES] + [("X", n) for n in br.X_CASES]
    out += [("L", n) for n in br.L_CASES] + [("C", n) for n in br.C_CASES] + [("T", n) for n in br.TIE_N + (5,)]
    return out


def _case(table, name):
    return br.case("%s-%s" % (table, name))


def _torch_q(c, x, dtype):
    """q of RefBranchingQNetwork on input rows x (the case's net), or from h1 where the case has no inputs: the
    layers after the first Linear, applied by hand to h1."""
    net = RefBranchingQNetwork(c["net"]["w1"].shape[1], c["A"], c["n"]).to(dtype)
    net.load_stacked({k: torch.tensor(c["net"][k]).to(dtype) for k in BDQN_KEYS})
    with torch.no_grad():
        if x is not None:
            return net(torch.tensor(x).to(dtype)).numpy().astype(np.float64)
        out = net.model[1:](torch.tensor(c["h1"]).to(dtype))
        advs = torch.stack([l(out) for l in net.adv_heads], dim=1)
        return (net.value_head(out).unsqueeze(2) + advs - advs.mean(2, keepdim=True)).numpy().astype(np.float64)


@pytest.mark.parametrize("table,name", _cases())
def test_reference_matches_the_torch_network(table, name):
    c = _case(table, name)
    ref = c["ref"]
    x = c["x"][:, :c["obs"]] if table == "X" else (c["x"] if table in "LC" else None)
    rows = c["rows"] if "rows" in c else c["E"] * c["N"]
    assert ref["q64"].shape == ref["q32"].shape == (rows, c["A"], c["n"])
    q64, q32 = _torch_q(c, x, torch.float64), _torch_q(c, x, torch.float32)
    scale = _maxabs(ref["q64"])
    assert _maxabs(q64 - ref["q64"]) <= 1e-12 * scale
    assert _maxabs(q32 - ref["q64"]) <= 1e-5 * scale           # torch float32 against the reference
    assert _maxabs(ref["q32"] - q64) <= 1e-5 * scale           # the restatement against torch float64
    # first maximum, as torch.argmax; torch's own rounding decides entries within it of a tie (the exact ties of T
    # among them: its BLAS need not sum two identical rows in the same order)
    clear = ref["gap"] > 1e-10 * scale
    assert np.array_equal(ref["pick"][clear], np.argmax(q64, axis=2)[clear]) and (clear.mean() > 0.99 or table == "T")
    assert ((ref["pick"] >= 0) & (ref["pick"] < c["n"])).all()
    # the pick cap: the float32 restatement's own argmax against the float64 one
    differ = float((ref["pick32"] != ref["pick"]).mean())
    print("BACT|%s-%s|f32 picks differ %.5f" % (table, name, differ))
    assert differ <= PICK_CAP, differ
    if table != "T":  # off the discontinuity: hardly any entry is a near tie
        assert (ref["gap"] < 1e-6 * scale).mean() <= PICK_CAP
        # every advantage is negative: a zero-padded action row past n would win the argmax if it joined it
        assert (ref["adv32"].max(axis=2) < 0).all()


@pytest.mark.parametrize("table,name", [("L", n) for n in br.L_CASES] + [("C", n) for n in br.C_CASES])
def test_dense_rows_and_layer1_match_the_compact_algebra(table, name):
    c = br.compact_case(table, name)
    D, C, N, E = c["D"], c["C"], c["N"], c["E"]
    assert c["x"].shape == (E * N, C * D) and c["x"].dtype == np.int8
    # the rule itself, element by element on a few rows
    f = br.foreign_row(D)
    assert f.tolist()[:4] == [0, -1, -1, -2] and (f[3:] == -2).all()
    for r in (0, E * N // 2, E * N - 1):
        e, a = divmod(r, N)
        for k in range(C):
            want = c["core_rows"][e, k, :D] if c["core_owner"][e, k] == a + 1 else f
            assert np.array_equal(c["x"][r, k * D:(k + 1) * D], want)
    h = layer1_compact_reference(torch.tensor(c["net"]["w1"]), torch.tensor(c["net"]["b1"]), torch.tensor(c["core_rows"]),
                                 torch.tensor(c["core_owner"]), N, D).numpy().astype(np.float64)
    scale = _maxabs(c["h64"])
    assert _maxabs(h - c["h64"]) <= 1e-5 * scale
    assert _maxabs(c["h32"] - c["h64"]) <= 1e-5 * scale
    # base: layer 1 of an agent owning nothing
    assert _maxabs(c["base32"] - c["base64"]) <= 1e-5 * _maxabs(c["base64"])
    free = ~c["owning"]
    if free.any():
        assert np.array_equal(c["h64"][free], np.broadcast_to(c["base64"], (int(free.sum()), 128)))
    # the weights the split must keep: an exact zero and two of magnitude about 2^-20
    w1 = c["net"]["w1"]
    assert w1[0, 0] == 0 and w1[1, 1] == np.float32(2.0 ** -20) and 2.0 ** -20 < -w1[2, D - 1] < 2.0 ** -19


@pytest.mark.parametrize("name", list(br.C_CASES))
def test_ownership_patterns(name):
    c = br.compact_case("C", name)
    co, N, C, E = c["core_owner"], c["N"], c["C"], c["E"]
    assert co.min() >= 0 and co.max() <= N
    own = c["owning"].reshape(E, N)
    if c["own"] == "none":
        assert (co == 0).all() and not own.any()
    elif c["own"] == "all":
        assert N <= C and own.all()
    else:
        assert own.any() and (not own.all() or E * N == 1)
        assert own[0, N - 1]
        if c["own"] == "mixed63":
            alone = own[:, 63] & (own.sum(axis=1) == 1)
            assert N == 64 and alone.sum() >= E // 3 and (~alone).sum() >= 1
    ex = c["explore"]
    assert set(np.unique(ex)) == {0, 1, 255} or E * N < 3
    assert (c["rnd"][ex != 0] >= 0).all() and (c["rnd"][ex != 0] < c["n"]).all() and (c["rnd"][ex == 0] < 0).all()


@pytest.mark.parametrize("n", br.TIE_N + (5,))
def test_tie_cases_are_exact(n):
    c = br.tie_case(n)
    ref, A = c["ref"], c["A"]
    adv32, q64 = ref["adv32"], ref["q64"]
    seen = set()
    for b in range(A):
        if c["pairs"][b] is None:  # every action of the branch bit-equal, in float32 and float64
            assert (adv32[:, b, :] == adv32[:, b, :1]).all() and (q64[:, b, :] == q64[:, b, :1]).all()
            assert c["expect"][b] == 0
            continue
        j, k = c["pairs"][b]
        assert 0 <= j < k < n and c["expect"][b] == j
        assert np.array_equal(c["net"]["wa"][b * n + j], c["net"]["wa"][b * n + k])
        assert c["net"]["ba"][b * n + j] == c["net"]["ba"][b * n + k]
        assert np.array_equal(adv32[:, b, j].view(np.int32), adv32[:, b, k].view(np.int32))
        assert (q64[:, b, j] == q64[:, b, k]).all() and (ref["gap"][:, b] == 0).all()
        third = np.sort(q64[:, b, :], axis=1)[:, -3]
        assert (q64[:, b, j] - third > 1.0).all()  # the pair is the maximum of every row, far above the rest
        assert (ref["pick"][:, b] == j).all()
        pj, pk = br.tie_position(j), br.tie_position(k)
        seen.add((pj["mt"] == pk["mt"], pj["g4"] == pk["g4"], b & 3))
        if br.TIE_PATTERNS[b // 4][0] == "first-last-tile":
            assert pj["mt"] == 0 and pk["mt"] == br.act_plan(n, 1)["nmt"] - 1
        if br.TIE_PATTERNS[b // 4][0] == "tiles":
            assert pj["g4"] > pk["g4"] and pj["mt"] < pk["mt"]
    if n > 16:
        # same lane group at different q, different lane groups, different tiles: each under all four writer groups
        for same_mt, same_g4 in ((True, True), (True, False), (False, False), (False, True)):
            assert {w for (a, b_, w) in seen if (a, b_) == (same_mt, same_g4)} == {0, 1, 2, 3}
        assert br.act_plan(n, 1)["nmt"] == (7 if n == 100 else 8)
    else:
        assert br.act_plan(n, 1)["nmt"] == 1 and A == 4


def test_tables_cover_every_edge():
    """Every path of bdqn_kernels.hip the tables were built to cross is crossed by some case."""
    H = [dict(c, **br.act_plan(c["n"], c["rows"])) for c in br.H_CASES.values()]
    has = lambda cs, f: any(f(c) for c in cs)
    # k_bdqn_act<NMT, false>: every NMT, both sides of each tile edge, the one instantiation without LDS-DMA
    assert {c["n"] for c in H} >= {1, 2, 12, 13, 15, 16, 17, 32, 33, 80, 81, 96, 97, 112, 113, 127, 128}
    assert {c["nmt"] for c in H} == {1, 2, 3, 4, 5, 6, 7, 8}
    assert {c["nmt"] for c in H if not c["glds"]} == {8} and all(c["glds"] for c in H if c["nmt"] < 8)
    assert {c["empty_groups"] for c in H if c["nmt"] == 1} >= {0, 1, 3}  # n = 16 / 13, 15 / 1, 2 ... 4
    assert has(H, lambda c: c["last_tile_full"]) and has(H, lambda c: not c["last_tile_full"])
    assert {c["A"] for c in H} >= {1, 3, 4, 5, 16, 17, 32, 127}
    assert {c["rows"] for c in H} >= {1, 15, 16, 17, 31, 32, 33, 255, 256, 257}
    assert {c["blocks"] for c in H} >= {1, 2} and has(H, lambda c: c["blocks"] == 2 and c["last_block_rows"] == 1)
    # k_bdqn_act<NMT, true>: obs around the k-step of 32, the stride below and above Kp, pad bytes present
    X = list(br.X_CASES.values())
    assert {c["obs"] for c in X} >= {1, 31, 32, 33, 64, 65, 255, 256} and all(c["rows"] == 257 for c in X)
    for obs in (1, 31, 32, 33, 64, 65, 255, 256):
        strides = {c["x_stride"] for c in X if c["obs"] == obs}
        assert strides == {align4(obs), br.pad32(obs) + 8}
    assert has(X, lambda c: c["x_stride"] < br.pad32(c["obs"])) and has(X, lambda c: c["x_stride"] > br.pad32(c["obs"]))
    assert has(X, lambda c: c["x_stride"] == br.pad32(c["obs"]))
    assert {br.pad32(c["obs"]) // 32 for c in X} >= {1, 2, 3, 8}
    assert {br.act_plan(c["n"], c["rows"])["nmt"] for c in X} >= {1, 2, 3, 5, 6, 7, 8}
    assert all(c["x_stride"] % 4 == 0 and c["x_stride"] >= c["obs"] for c in X)
    # k_bdqn_l1_cores<S>, the gather, the split and the base
    L = [dict(c, **br.l1_plan(c["D"], c["stride"], c["C"], c["E"])) for c in br.L_CASES.values()]
    assert {c["D"] for c in L} >= {4, 5, 31, 32, 33, 64, 65, 97, 129, 161, 193, 225, 255, 256}
    assert {c["S"] for c in L} == {1, 2, 3, 4, 5, 6, 7, 8}
    for D in (4, 31, 32, 33, 256):
        assert {c["stride"] for c in L if c["D"] == D} >= {align4(D), align4(D) + 8}
    assert has(L, lambda c: c["stride_over_Dp"]) and has(L, lambda c: c["stride_under_Dp"])
    assert has(L, lambda c: c["stride"] == c["Dp"]) and has(L, lambda c: c["pad"] >= 8) and has(L, lambda c: c["pad"] == 0)
    assert {c["C"] for c in L} >= {1, 3, 4, 5, 16, 17} and {c["N"] for c in L} >= {1, 2, 5, 64}
    assert {c["E"] for c in L} >= {1, 15, 16, 17, 128, 129, 144}
    assert has(L, lambda c: c["partial_tile"]) and has(L, lambda c: not c["partial_tile"])
    assert {c["chunks"] for c in L} >= {1, 2}
    assert has(L, lambda c: c["chunks"] == 1 and c["tiles"] == 8) and has(L, lambda c: c["chunks"] == 2 and c["last_chunk_tiles"] == 1)
    assert has(L, lambda c: c["last_chunk_tiles"] % 2 == 1 and c["last_chunk_tiles"] > 1 or c["tiles"] == 9)
    assert has(L, lambda c: c["tiles"] == 1) and has(L, lambda c: c["tiles"] == 2)
    assert has(L, lambda c: c["E"] == 144 and c["C"] == 17)
    # the row list of ms_bdqn_act_compact
    C = []
    for name in br.C_CASES:
        c = br.compact_case("C", name)
        rows = c["E"] * c["N"]
        ll = 1 + int(c["owning"].sum())
        C.append(dict({k: c[k] for k in ("D", "stride", "C", "N", "E", "own", "n", "A")}, rows=rows, list_len=ll,
                      **br.act_plan(c["n"], rows, ll)))
    assert all(c["A"] == c["C"] for c in C)
    assert has(C, lambda c: c["list_len"] == 1)                                   # *n_owning == 0
    assert {c["rows"] for c in C if c["own"] == "all"} >= {256, 512, 1024}
    assert all(c["list_len"] == c["rows"] + 1 for c in C if c["own"] == "all")
    assert has(C, lambda c: c["own"] == "all" and c["last_block_rows"] == 1 and c["blocks"] >= 2)  # the + 1 block
    assert {c["rows"] for c in C} >= {1, 1023, 1024, 1025, 1088}
    assert has(C, lambda c: c["N"] == 64 and c["own"] == "mixed63") and has(C, lambda c: c["N"] == 1)
    assert has(C, lambda c: c["rows"] > br.OWN_LIST_THREADS) and has(C, lambda c: c["rows"] == br.OWN_LIST_THREADS)
    # byte paths: C % 16 (k_bdqn_own_mask), C % 4 (k_bdqn_act), A % 16 (k_bdqn_common_fill, rows owning nothing)
    assert {c["A"] for c in C} >= {1, 3, 4, 5, 16, 17, 32}
    assert has(C, lambda c: c["C"] % 16 == 0) and has(C, lambda c: c["C"] % 16 != 0 and c["C"] % 4 == 0)
    assert has(C, lambda c: c["C"] % 4 != 0 and c["C"] > 4) and has(C, lambda c: c["C"] < 4)
    assert has(C, lambda c: c["A"] % 16 == 0 and c["list_len"] <= c["rows"])
    assert has(C, lambda c: c["A"] % 16 != 0 and c["list_len"] <= c["rows"])
    assert {c["nmt"] for c in C} >= {1, 2, 3, 7, 8}
    assert {br.l1_plan(c["D"], c["stride"], c["C"], c["E"])["S"] for c in C} >= {1, 2, 3}
    assert len(br.TIE_PATTERNS) == 6 and br.TIE_N == (100, 128)
