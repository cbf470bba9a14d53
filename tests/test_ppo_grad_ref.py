"""The float64 reference of the PPO gradient (oracle/ppo_grad_ref.py) and its case tables, on the CPU: the tables
reach every instantiation launch_ppo_grad can choose, every listed input, action and row-count edge and the seams of
ppo_split (from the restated dispatch and split); no case sits on a discontinuity of the loss, every case has rows on
both surrogate branches, the row redraws end within five sweeps, float32 CPU autograd of the same loss stays within
1e-4 of scale of the reference (a sanity check of the reference, not of the kernel), and the keyed cases' extra
allowance covers what the 2^-20 fixed point does to the reference's own terms."""
import numpy as np
import pytest
import torch
from torch.distributions import Categorical

from oracle import ppo_grad_ref as pr

A_CASES = pr.TABLES["A"]
B_CASES = pr.TABLES["B"]


def _inst(spec, keyed=False):
    return pr.dispatch(spec["D"], spec["A"], keyed)


def test_dispatch_restated_over_the_whole_range():
    """Every (D, A) the entry point accepts has one of the 19 instantiations ({1,2,4,8,16} x {1,2}, {2,4,8,16} x 4,
    {4,8,16} x 8 and the two single-action-tile ones); D = 256 has none."""
    assert len(set(pr.INSTANTIATIONS)) == 19
    seen = set()
    for D in range(1, 256):
        for A in range(1, 129):
            q, t, x1 = pr.dispatch(D, A)
            assert (q, t, x1) in pr.INSTANTIATIONS
            assert 16 * q > D and 16 * t >= A
            assert x1 == (A in (17, 49) and (q, t) == ((4, 2) if A == 17 else (8, 4)) and 8 * q <= D)
            seen.add((q, t, x1))
    assert seen == set(pr.INSTANTIATIONS)
    assert all(pr.dispatch(256, A) is None for A in range(1, 129))
    # the keyed passes never take a single-action tile, and reach <1, 1> and <1, 2> only
    assert {pr.dispatch(D, A, True) for D in range(1, 5) for A in range(1, 33)} == {(1, 1, False), (1, 2, False)}


def test_table_a_reaches_every_instantiation_and_edge():
    inst = {n: _inst(s) for n, s in A_CASES.items()}
    assert {v for n, v in inst.items() if n.startswith("inst-")} == set(pr.INSTANTIATIONS)
    assert sum(n.startswith("inst-") for n in A_CASES) == 19  # one each
    assert inst["inst-x1-D40-A17"] == (4, 2, True) and inst["inst-x1-D99-A49"] == (8, 4, True)
    by_a13 = {s["D"]: s for n, s in A_CASES.items() if s["A"] == 13}
    assert {1, 15, 16, 31, 32, 63, 64, 127, 128, 255} <= set(by_a13)
    assert {s["D"] % 4 for s in A_CASES.values()} == {0, 1, 2, 3}
    # stride == D (the ones byte is past the row: its dword reads 0) and whole pad dwords after D + 13
    assert any(s["stride"] == s["D"] for s in A_CASES.values())
    assert any(s["stride"] == pr.align4(s["D"] + 13) and s["stride"] - s["D"] >= 8 for s in A_CASES.values())
    for m in range(4):  # every position of the ones byte, with pad bytes behind it
        assert any(s["D"] % 4 == m and s["stride"] > s["D"] for s in A_CASES.values()), m
    assert {s["A"] for s in A_CASES.values() if s["D"] == 19} >= {1, 2, 15, 16, 17, 32, 33, 48, 49, 64, 65, 127, 128}
    # A % 16 == 1 outside the two single-action-tile shapes
    for D, A in ((19, 17), (195, 17), (40, 49)):
        assert any(s["D"] == D and s["A"] == A for s in A_CASES.values())
        assert pr.dispatch(D, A)[2] is False
    assert (A_CASES["corner"]["D"], A_CASES["corner"]["stride"], A_CASES["corner"]["A"]) == (255, 256, 128)
    for n, s in A_CASES.items():
        R = s["T"] * s["E"]
        assert 128 < R <= 640 and R % 16 != 0, n
        assert s["pad_garbage"] and s["G"] in (2, 3) and s["U"] >= 3, n
        assert pr.path(s) == "plain", n


def test_split_restated():
    for G in (1, 2, 3, 64):
        for R in list(range(1, 2100)) + [10 ** 6, 3 * 10 ** 6]:
            ct, nc = pr.split(R, G)
            tiles = (R + 15) // 16
            assert ct >= 8 and ct % 2 == 0 and nc % 4 == 0
            assert ct * nc >= tiles > ct * (nc - 4)  # every tile in a chunk, no idle block
            assert tiles * G <= pr.GRAD_WAVES * ct
    assert pr.split(1, 3) == (8, 4) and pr.split(513, 3) == (8, 8) and pr.split(1025, 3) == (8, 12)
    assert pr.split(3 * 10 ** 6, 8)[0] == 184  # chunks grow once tiles * G passes 8 * 8192


def test_table_b_reaches_the_row_count_seams():
    """Tiles of 16 rows, tile pairs of 32, chunks of 8 tiles (128 rows), blocks of 4 chunks (512 rows)."""
    for tag, inst in (("s", (2, 1, False)), ("c", (16, 8, False))):
        cases = {n: s for n, s in B_CASES.items() if n.startswith(tag + "-")}
        assert {_inst(s) for s in cases.values()} == {inst}
        rows = {s["T"] * s["E"] for s in cases.values()}
        assert rows == set(pr.B_ROWS)
        for R in pr.B_ROWS:
            shapes = {(s["T"], s["E"]) for s in cases.values() if s["T"] * s["E"] == R and s["um"] is None}
            assert (R, 1) in shapes and (1, R) in shapes
            if R in (15, 16, 32, 33, 128, 129, 511, 512, 513, 1025):
                assert any(1 < T < R for T, _ in shapes), R
        assert {s["um"] for s in cases.values()} == {None, 0, 7}  # unit_stride R and R + 7
        edges = {R: pr.split_edges(R, 3) for R in pr.B_ROWS}
        assert edges[1] == dict(tiles=1, ragged=1, odd_pair=True, chunks_used=1, chunks_idle=3, blocks=1)
        assert [edges[R]["tiles"] for R in (15, 16, 17, 31, 32, 33)] == [1, 1, 2, 2, 2, 3]
        assert [edges[R]["chunks_used"] for R in (127, 128, 129, 511, 512, 513, 1025)] == [1, 1, 2, 4, 4, 5, 9]
        assert [edges[R]["blocks"] for R in (511, 512, 513, 1025)] == [1, 1, 2, 3]
        assert {edges[R]["ragged"] for R in pr.B_ROWS} >= {0, 1, 15}
        assert {edges[R]["odd_pair"] for R in pr.B_ROWS} == {True, False}
    assert all(s["G"] == 3 and s["U"] >= 3 for s in B_CASES.values())


def test_no_instantiation_runs_two_waves_per_block():
    """GradLds::WPB is 4 for every kernel the launcher can choose (<16, 8> plain fits with 940 floats to spare), so
    the two-chunks-per-wave branch of k_ppo_grad is unreachable."""
    for q, t, _ in pr.INSTANTIATIONS:
        assert pr.grad_lds_wpb(q, t) == 4, (q, t)
        if q <= 8:  # the common-row modes
            for cm in pr.common_row_floats(t):
                assert pr.grad_lds_wpb(q, t, cm) == 4, (q, t, cm)


def test_tables_c_d_e_take_their_paths():
    C, D, E = pr.TABLES["C"], pr.TABLES["D"], pr.TABLES["E"]
    assert {s["D"]: _inst(s) for n, s in C.items() if n.startswith("O")} == {
        15: (1, 1, False), 27: (2, 1, False), 51: (4, 2, False), 99: (8, 4, True)}
    for n, s in C.items():
        R = s["T"] * s["E"]
        want = "own_scan" if n.startswith("many") else ("owner" if s["compact"] else "common")
        assert pr.path(s) == want, n
        assert s["compact"] is None or s["U"] == s["compact"][0] * s["compact"][1]
        assert n.startswith("many") == (s["G"] >= pr.OWN_MIN_GROUPS)
    rows = {s["T"] * s["E"] for n, s in C.items() if n.startswith("O")}
    assert rows == {33, 513, 1500} and 1500 > 2 * pr.COMMON_SEG  # listed rows carry over two segment ends
    assert {s["common"] for n, s in C.items() if n.startswith("O")} == {0.0, 0.5, 1.0}
    many = sorted(s["T"] * s["E"] for n, s in C.items() if n.startswith("many"))
    assert many == [33, 4 * pr.OWN_SCAN_ROWS - 1, 4 * pr.OWN_SCAN_ROWS + 1]  # mask words, the scan block's end
    assert pr.path(pr.SMALL_STRIDE) == "plain" and pr.SMALL_STRIDE["stride"] < 16
    for n, s in D.items():
        assert s["stride"] == 4 and s["D"] in (1, 2, 3, 4) and s["A"] in (13, 20), n
        assert pr.path(s) == ("keyed" if s["row_keys"] == 0 else "plain"), n
    assert {s["T"] * s["E"] for s in D.values()} >= {1, 255, 256, 257, 2000}
    assert {s["distinct"] for s in D.values()} >= {1, 3, 300}
    assert {s["scale3"] for s in E.values()} == {40.0}
    assert (4, 2, True) in {_inst(s) for s in E.values()}


def test_float32_chain_is_torch_categorical():
    """The written-out chain, in float32, is nn.Softmax -> Categorical(probs): the same log-probs and entropies
    bit for bit (the float64 reference differs from it in precision only, clamp edge included)."""
    c = pr.case("E/sat-D19-A25")
    for g in range(c["spec"]["G"]):
        p = {k: torch.as_tensor(c["nets"][k][g]) for k in pr.KEYS}
        x, a = torch.as_tensor(c["x"][g]).float(), torch.as_tensor(c["act"][g])
        pn, logits, lp, ent, _ = pr._forward(p, x, a)
        h = torch.tanh(torch.tanh(x @ p["w1"].T + p["b1"]) @ p["w2"].T + p["b2"])
        dist = Categorical(torch.nn.Softmax(dim=-1)(h @ p["w3"].T + p["b3"]))
        assert torch.equal(lp, dist.log_prob(a)) and torch.equal(ent, dist.entropy())
        assert float(pn.min()) < pr.EPS_P  # the clamp is in use


@pytest.mark.parametrize("name", list(pr.CASES))
def test_case_is_clear_of_discontinuities(name):
    c = pr.case(name)
    spec, v = c["spec"], c["rows"]
    G, R = spec["G"], spec["R"]
    assert c["sweeps"] <= pr.MAX_SWEEPS
    e = pr.EPS_CLIP
    for edge in (1 - e, 1 + e):
        assert np.abs(v["ratio"] / edge - 1).min() >= pr.KINK
    assert np.abs(v["adv"]).min() >= pr.KINK
    assert v["edge"].min() > 4.0
    sh = c["shares"]
    if R == 1:  # one row per group: one of each over the groups
        assert sh["inside"] * G >= 1 and sh["away"] * G >= 1
    else:
        assert sh["inside"] >= 0.1 and sh["away"] >= 0.1, sh
    assert (v["ratio"] < 1 - e).any() and (v["ratio"] > 1 + e).any() or R == 1
    # what the kernel reads is clean; everything else in the buffers is garbage
    assert np.isfinite(c["olp"]).all() and np.isfinite(c["ret"]).all()
    assert c["act"].min() >= 0 and c["act"].max() < spec["A"]
    buf = c["buf"]
    assert len(set(buf["uog"].tolist())) == G and not np.array_equal(buf["uog"], np.arange(G))
    assert buf["ld"] > G and np.isnan(buf["returns"][:, G:]).all() and np.isnan(buf["returns"][R:]).all()
    assert np.isnan(buf["olp"]).sum() == buf["olp"].size - G * R
    assert (buf["actions"] < 0).sum() == buf["actions"].size - G * R
    if spec["distinct"]:
        for g in range(G):
            assert len({r.tobytes() for r in c["x"][g]}) == min(spec["distinct"], R) + (spec["outlier"] and g == 0)
    if name == "D/ranks-over":
        assert min(len({r.tobytes() for r in c["x"][g]}) for g in range(G)) > pr.KEY_MAX_RANKS
    if name == "D/byte-outside":
        assert c["x"][0].max() == 100
    if spec["common"] is not None and spec["compact"] is None:
        same = (c["x"] == buf["common_row"][None, None, :spec["D"]]).all(axis=2).mean()
        assert abs(same - spec["common"]) < 0.06, same
        if spec["common"] < 1.0 and R > 100:  # rows one byte off the common row
            assert ((c["x"] != buf["common_row"][None, None, :spec["D"]]).sum(axis=2) == 1).any()
    # float32 CPU autograd against the reference
    (g64, l64), (g32, l32) = c["ref"], c["f32"]
    for k in pr.KEYS:
        assert np.abs(g32[k] - g64[k]).max() <= 1e-4 * np.abs(g64[k]).max(), k
    assert (np.abs(l32 - l64).max(axis=0) <= 1e-4 * np.abs(l64).max(axis=0)).all()


KEYED = [n for n, s in pr.TABLES["D"].items() if s["row_keys"] == 0 and s["distinct"] and not s["outlier"]]


@pytest.mark.parametrize("name", KEYED)
def test_keyed_allowance_covers_the_fixed_point(name):
    """The keyed passes see a row only through qd = d min(surr) / d ratio * ratio and dv = V - G, rounded to 2^-20.
    With the exact terms the linear form reproduces the reference; with the rounded terms it moves no gradient
    element by more than keyed_allowance, which is not idle (something moves)."""
    c = pr.case("D/" + name)
    qd, dv = pr.keyed_terms(c)
    exact = pr.keyed_grads(c, qd, dv)
    for k in pr.KEYS:
        assert np.abs(exact[k] - c["ref"][0][k]).max() <= 1e-12 * max(np.abs(c["ref"][0][k]).max(), 1e-3), k
    assert np.abs(pr.quantise(qd) - qd).max() <= 0.5 / pr.KEY_FX
    moved = pr.keyed_grads(c, pr.quantise(qd), pr.quantise(dv))
    allow = pr.keyed_allowance(c)
    used = 0.0
    for k in pr.KEYS:
        d = np.abs(moved[k] - exact[k])
        assert (d <= allow[k] + 1e-18).all(), k
        used = max(used, float((d / np.maximum(allow[k], 1e-30)).max()))
    assert 0.0 < used <= 1.0
