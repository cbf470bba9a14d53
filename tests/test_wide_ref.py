"""The float64 references of the wide nets' kernels (oracle/wide_ref.py), the restated work plan and the case
tables of tests/test_wide_parity_gpu.py, on the CPU: the restated plan's byte count is ms_wide_workspace_bytes for
every table case, for shapes where the 2^28-float cap on the split partials binds and past the 64 GiB bound; the
tables reach the seams of the plan and of the kernels' thread mappings (asserted on the restated plan); no gradient
case sits on a discontinuity of the loss; and the float32 restatement of the sampling picks the float64 action on all
but 1 % of each act case's rows, so a device that misses that cap has itself to blame."""
import ctypes as ct

import numpy as np
import pytest

from oracle import wide_ref as wr

GRAD = wr.GRAD_CASES
ACT = wr.ACT_CASES


def _family(f):
    return {n: s for n, s in GRAD.items() if s["family"] == f}


def _plan(s):
    return wr.wide_plan(s["G"], s["D"], s["A"], s["H"], s["R"])


def _lib_bytes(ms, G, D, A, H, R):
    p = ms.abi.MsMlpParams(None, None, None, None, None, None, D, H, A, G, None, 0)  # sizes only: no pointer is read
    return int(ms.lib.ms_wide_workspace_bytes(ct.byref(p), R))


def test_restated_plan_is_the_librarys(ms):
    for n, s in GRAD.items():
        want = wr.workspace_bytes(s["G"], s["D"], s["A"], s["H"], s["R"])
        assert want > 0 and want % 256 == 0
        assert _lib_bytes(ms, s["G"], s["D"], s["A"], s["H"], s["R"]) == want == _plan(s)["bytes"], n
    # the cap on the partials binds (G * total > 2^28 / 3 floats): rs falls from ceil(R / 256) to rs_mem
    for G, D, A, H, R in ((1, 8, 1 << 21, 64, 600), (1, 8, 1 << 21, 64, 1037), (3, 30, 1 << 20, 32, 1037),
                          (1, 255, 1 << 24, 64, 513), (2, 8, 3 << 20, 32, 700)):
        p = wr.wide_plan(G, D, A, H, R)
        assert G * p["total"] > (1 << 28) // 3 and p["rs_mem"] < p["rs_rows"] and p["rs"] == p["rs_mem"], (G, A)
        assert 0 < p["bytes"] <= wr.WORKSPACE_CAP
        assert _lib_bytes(ms, G, D, A, H, R) == p["bytes"], (G, D, A, H, R)
    p = wr.wide_plan(1, 8, 1 << 21, 64, 600)
    assert (p["rs_rows"], p["rs_mem"], p["rps"], p["RS"]) == (3, 1, 608, 1)
    # past the 64 GiB bound: 0 and the reason
    G, D, A, H, R = 64, 8, 1 << 24, 64, 16437
    assert wr.wide_plan(G, D, A, H, R)["bytes"] > wr.WORKSPACE_CAP and wr.workspace_bytes(G, D, A, H, R) == 0
    assert _lib_bytes(ms, G, D, A, H, R) == 0 and b"64 GiB" in ms.lib.ms_last_error()


@pytest.mark.parametrize("G,D,A,H,R", [(2, 256, 9, 32, 100), (2, 8, (1 << 24) + 1, 32, 100), (2, 0, 9, 32, 100),
                                       (2, 8, 0, 32, 100), (2, 8, 9, 48, 100), (0, 8, 9, 32, 100), (2, 8, 9, 32, 0)])
def test_no_size_for_what_the_gradient_refuses(ms, G, D, A, H, R):
    """in_dim > 255 and n_actions > 2^24 used to get a size that ms_wide_grad then refused."""
    assert wr.workspace_bytes(G, D, A, H, R) == 0
    assert _lib_bytes(ms, G, D, A, H, R) == 0
    if D == 256 or A > 1 << 24:
        assert b"in_dim must be in [1, 255], n_actions in [1, 2^24]" in ms.lib.ms_last_error()
    assert _lib_bytes(ms, 2, 255, 1 << 24, 32, 100) == wr.workspace_bytes(2, 255, 1 << 24, 32, 100) > 0  # the last accepted


def test_plan_by_hand():
    p = wr.wide_plan(2, 8, 9, 32, 1037)
    assert p["off"] == [0, 256, 288, 1312, 1344, 1632, 1641, 1897, 1929, 2953, 2985, 3017, 3018]
    assert (p["NB"], p["tiles"], p["rs"], p["rps"], p["RS"], p["last_rows"]) == (65, 65, 5, 208, 5, 205)
    # zbuf 65 * 2 * 16 * 9 floats = 74880 bytes, rec 2 * 1037 * 272 floats, part 5 * 2 * 3018, loss 2 * 65 * 3,
    # each rounded up to 256 bytes
    assert p["at"] == dict(zbuf=0, rec=75008, part=75008 + 2256640, loss=2331648 + 120832) and p["bytes"] == 2452480 + 1792
    for G in (1, 2, 3, 128, 2048, 2049, 5000):
        for R in list(range(1, 700)) + [4096, 4097, 16384, 16385, 16437, 10 ** 6]:
            q = wr.wide_plan(G, 8, 9, 32, R)
            assert q["rps"] % 16 == 0 and q["RS"] <= q["rs"] <= 64
            assert (q["RS"] - 1) * q["rps"] < R <= q["RS"] * q["rps"]  # every row in a split, no empty split
            assert 1 <= q["NB"] <= q["tiles"] and q["NB"] * G <= max(2048, G)


def test_tables_reach_the_tile_loop():
    plans = {n: _plan(s) for n, s in _family("T").items()}
    assert all(p["tiles"] > p["NB"] for p in plans.values())
    p = plans["T/G128-R595"]
    assert (p["NB"], p["tiles"], p["trips"]) == (16, 38, [2, 3])
    p = plans["T/G128-R512-H64"]
    assert (p["NB"], p["tiles"], p["trips"]) == (16, 32, [2])          # equal trips, NB > 1
    p = plans["T/G2049-R40"]
    assert (p["NB"], p["tiles"], p["trips"]) == (1, 3, [3])
    for n in ("T/G2-R16437", "T/G2-R16437-full"):
        p = plans[n]
        assert (p["NB"], p["tiles"], p["trips"]) == (1024, 1028, [1, 2])
        assert (p["rs"], p["rps"], p["RS"], p["last_rows"]) == (64, 272, 61, 117)  # rs = 64 and RS < rs
    s = GRAD["T/G2-R16437-full"]
    assert (s["D"], s["A"], s["H"]) == (30, 225, 64)
    # every case of the other families, and of the old suite's shapes, has one tile per block
    assert all(_plan(s)["trips"] == [1] for n, s in GRAD.items() if s["family"] != "T")


def test_tables_reach_the_row_split_seams():
    by_r = {s["R"]: _plan(s) for s in _family("R").values() if s["H"] == 32}
    assert set(by_r) == set(wr.R_ROWS) and set(wr.R_ROWS) >= {1, 15, 16, 17, 256, 257, 273, 288, 513, 1037}
    assert all(s["G"] == 2 for s in _family("R").values())
    assert [by_r[R]["RS"] for R in (1, 15, 16, 17, 256)] == [1] * 5
    assert (by_r[257]["RS"], by_r[257]["rps"], by_r[257]["last_rows"]) == (2, 144, 113)
    assert (by_r[288]["RS"], by_r[288]["rps"], by_r[288]["last_rows"]) == (2, 144, 144)      # the last split full
    # R = 273 has rps = 144 too, but its last split holds 129 rows: with rs = RS a last split of one row needs
    # R <= 16 rs (rs - 1) and R > 256 (rs - 1), so rs >= 16, and R = 3841 = 15 * 256 + 1 is the first
    assert (by_r[273]["RS"], by_r[273]["rps"], by_r[273]["last_rows"]) == (2, 144, 129)
    assert (by_r[3841]["rs"], by_r[3841]["RS"], by_r[3841]["rps"], by_r[3841]["last_rows"]) == (16, 16, 256, 1)
    assert not any(wr.wide_plan(2, 8, 9, 32, R)["last_rows"] == 1 for R in range(17, 3841))
    assert (by_r[1037]["RS"], by_r[1037]["last_rows"], by_r[1037]["last_rows"] % 16) == (5, 205, 13)  # a partial tile
    assert (by_r[513]["rs"], by_r[513]["RS"], by_r[513]["last_rows"]) == (3, 3, 161)
    assert any(p["RS"] < p["rs"] for p in map(_plan, GRAD.values()))
    assert any(p["rs"] == 64 for p in map(_plan, GRAD.values()))
    # no table case has the memory cap binding: that branch is checked on the CPU only (above)
    assert all(p["rs_mem"] >= p["rs_rows"] for p in map(_plan, GRAD.values()))


def test_tables_reach_the_thread_mapping_edges():
    D = _family("D")
    assert [s["D"] for s in D.values()] == list(wr.D_DIMS) == [1, 2, 84, 85, 127, 128, 254, 255]
    assert {wr.outer_phases(s["D"]) for s in D.values()} >= {1, 2, 3, 128}
    assert [wr.outer_phases(d) for d in (1, 84, 85, 127, 128, 255)] == [128, 3, 2, 2, 1, 1]
    assert (255 + 1) * wr.outer_phases(255) == wr.TPB  # every thread busy
    A = _family("A")
    assert [s["A"] for s in A.values()] == list(wr.A_COUNTS) == [1, 2, 63, 64, 65, 255, 256, 257, 513, 3000]
    assert [wr.actions_per_thread(a) for a in (255, 256, 257, 513, 3000)] == [1, 1, 2, 3, 12]
    assert [(a + 63) // 64 for a in (63, 64, 65)] == [1, 1, 2]  # k_wide_w3's blocks of 64 actions
    assert {s["G"] for s in A.values()} == {1, 3}
    assert all(s["R"] == 100 for s in list(D.values()) + list(A.values()))
    S = _family("S")
    assert {s["A"] for s in S.values()} == {25, 257} and all(s["R"] == 160 and s["scale3"] == 40.0 for s in S.values())
    for f in "RTDAS":
        assert {s["H"] for s in _family(f).values()} == {32, 64}, f
    strides = [s["stride"] - wr.up4(s["D"]) for s in GRAD.values()]
    assert set(strides) == {0, 8} and abs(strides.count(0) - strides.count(8)) <= 1
    # the act tables
    assert {s["A"] for s in ACT.values()} >= {1, 2, 9, 255, 256, 257, 513, 3000}
    assert {s["D"] for s in ACT.values()} >= {1, 8, 255}
    assert {s["E"] for s in ACT.values()} >= {1, 16, 17, 37}
    assert {s["H"] for s in ACT.values()} == {32, 64} and {s["G"] for s in ACT.values()} == {1, 3}
    assert sum(s["underflow"] > 0 for s in ACT.values()) == 2
    assert {s["stride"] - wr.up4(s["D"]) for s in ACT.values()} == {0, 8}


@pytest.mark.parametrize("name", list(GRAD))
def test_no_gradient_case_sits_on_a_discontinuity(name):
    c = wr.grad_case(name)
    s, v = c["spec"], c["rows"]
    G, D, A, R, stride = s["G"], s["D"], s["A"], s["R"], s["stride"]
    assert np.abs(v["ratio"] - (1 - wr.EPS_CLIP)).min() >= 1e-3 and np.abs(v["ratio"] - (1 + wr.EPS_CLIP)).min() >= 1e-3
    assert np.abs(v["adv"]).min() >= 1e-3
    if R >= 64:
        assert c["shares"]["live"] >= 0.1 and c["shares"]["away"] >= 0.1, c["shares"]
    if s["family"] == "S":
        assert v["edge"].min() > 4.0
        assert (v["pmax"] > 1 - wr.EPS_P).mean() > 0.2 and v["pmin"].max() < wr.EPS_P  # clamped on both sides
    elif A > 1:
        assert v["pmin"].min() >= 4 * wr.EPS_P and (1 - v["pmax"]).min() >= 4 * wr.EPS_P
    else:
        assert (v["pmin"] == 1.0).all()  # one action: p = 1, beyond the upper edge
    # the buffers: garbage where the kernel must not read, the extremes of int8 in rows it does
    st = c["states"]
    assert st.shape == (R + 3, G, stride) and (np.abs(st[:, :, D:].astype(np.int32)) == 127).all()
    assert (np.abs(st[R:].astype(np.int32)) == 127).all()
    assert ((c["actions"][R:] < 0) | (c["actions"][R:] >= A)).all() and np.isnan(c["olp"][R:]).all()
    assert (0 <= c["actions"][:R]).all() and (c["actions"][:R] < A).all() and np.isfinite(c["olp"][:R]).all()
    body = st[:R, :, :D].reshape(R * G, D)
    if R >= 2 and s["family"] != "S":
        assert (body == -128).all(axis=1).any() and (body == 127).all(axis=1).any()
    rest = body[~((body == -128).all(axis=1) | (body == 127).all(axis=1))]
    assert rest.size == 0 or (rest.min() >= -2 and rest.max() <= 12)
    # the float32 autograd stays near the reference (a check of the reference, not of the kernel)
    (g64, l64), (g32, l32) = c["ref"], c["f32"]
    for k in wr.KEYS:
        assert np.isfinite(g64[k]).all()
        assert np.abs(g32[k] - g64[k]).max() <= 1e-4 * max(np.abs(g64[k]).max(), 1e-30) + 1e-9, k
    if A == 1:
        assert all(not g64[k].any() for k in wr.ACTOR_KEYS)  # no choice, no actor gradient
    assert np.allclose(l32, l64, rtol=1e-4, atol=1e-6)


@pytest.mark.parametrize("name", list(ACT))
def test_float32_sampling_stays_within_the_cap(name):
    c = wr.act_case(name)
    s = c["spec"]
    G, D, A, E = s["G"], s["D"], s["A"], s["E"]
    differ = c["pick32"] != c["pick64"]
    assert differ.mean() <= 0.01, (int(differ.sum()), differ.size)
    # the rule of the device test holds for the restatement's own picks with R_ACT = 1
    a = c["pick32"]
    hi = np.take_along_axis(c["cdf64"], a[..., None], -1)[..., 0]
    lo = np.where(a > 0, np.take_along_axis(c["cdf64"], np.maximum(a - 1, 0)[..., None], -1)[..., 0], 0.0)
    delta = np.maximum(np.abs(c["cdf32"].astype(np.float64) - c["cdf64"]).max(-1), wr.EPS32)
    u = c["ug"].astype(np.float64)
    assert (lo - delta <= u).all() and (u <= hi + delta).all()
    # uniforms: exact 0 and 1 - 2^-24 among the rows, NaN past them; garbage pads and rows
    flat = c["u"][:E].reshape(-1)
    zeros, lasts = c["forced"]
    assert (flat[zeros] == 0.0).all() and (flat[lasts] == wr.U_LAST).all() and wr.U_LAST < 1.0
    assert float(wr.U_LAST) == 1.0 - 2.0 ** -24 and len(zeros) == len(lasts) >= 1
    assert (flat >= 0).all() and (flat < 1).all() and np.isnan(c["u"][E:]).all()
    assert (c["pick64"].T.reshape(-1)[zeros] == 0).all()
    assert (np.abs(c["obs"][:, :, D:].astype(np.int32)) == 127).all() and (np.abs(c["obs"][E:].astype(np.int32)) == 127).all()
    if E >= 2:
        body = c["obs"][:E, :, :D].reshape(E * G, D)
        assert (body == -128).all(axis=1).any() and (body == 127).all(axis=1).any()
    assert np.allclose(c["cdf64"][..., -1], 1.0, atol=1e-12)
    if s["ties"]:  # exact in both precisions, and most rows on a boundary
        assert np.array_equal(c["cdf32"], c["cdf64"]) and not differ.any()
        assert (c["cdf64"] == u[..., None]).any(-1).mean() > 0.5
    if s["underflow"]:
        k = s["underflow"]
        assert (c["p32"][..., A - k:] == 0).all() and (c["p64"][..., A - k:] > 0).all()  # 0 in float32 only
        assert (c["p32"][..., :A - k].max(-1) > 0.5).mean() > 0.5                         # near one-hot rows
