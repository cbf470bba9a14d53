"""Branching-DQN acting on the device (bdqn_kernels.hip through ms_bdqn_prepare, ms_bdqn_layer1_compact, ms_bdqn_act
and ms_bdqn_act_compact) against the float64 reference of oracle/bdqn_act_ref.py, through the C entry points (so
pitches, strides, scratch and workspace are the test's to set), at every edge of the launch plan
(tests/test_bdqn_act_ref.py proves on the CPU that the tables reach them).

Numeric outputs (base, the h1 of ms_bdqn_layer1_compact), per case and tensor:
    e_hip = max |hip - f64| <= R_L1 * max(e_f32, eps32 * max |f64|),  e_f32 = max |float32 restatement - f64|
(the products are exact, only the summation order differs from a plain float32 dot).
Picks, per (row, branch) with the device's pick a, every row held to it (no row is excused as unclear):
    max_m q64[m] - q64[a] <= R_BACT * max(max_m |q32[m] - q64[m]|, eps32 * max |q64 of the case|)
and at most 1 % of a case's picks differ from the float64 first argmax; every pick is in [0, n). The tie cases are
compared exactly. Every case prints "BACT|" lines with its figures (pytest -s); profiles/bdqn_act_parity/README.md
records them.

Around every call: the action buffer is pre-filled with a sentinel byte no pick can equal and carries a 256-byte
band behind it, h1 is pre-filled with NaN and carries a band, the scratch is passed at exactly
ms_bdqn_layer1_scratch_bytes, filled with 0xFF bytes before the first call, with a band of 256 floats behind it; a
second call on the same scratch gives the same bits; exploring rows take rand_action, whose bytes on the other rows
are out of range; rows past n_rows of h1 / x / explore / rand_action hold NaN / +-127 / 255 / out-of-range bytes."""
import ctypes as ct
import importlib

import numpy as np
import pytest
import torch

from oracle import bdqn_act_ref as br
from oracle.learner_ref import BDQN_KEYS, EPS32

pytestmark = pytest.mark.gpu

# R of the two rules above: twice the largest ratio measured on an MI355X over all cases of the tables, rounded up
# to a power of two (the condition: no more than 16); R_BACT floored at 2 (a pick made from q values each within e
# of the float64 ones can lie 2 e below the float64 maximum).
# Measured: numeric outputs 1.77 (base of L-N1; h1 0.88 at most, L-D32), picks 0.00 (no pick of any case lies below
# the float64 maximum, and none differs from the float64 first argmax): profiles/bdqn_act_parity/README.md.
R_L1 = 4.0
R_BACT = 2.0
PICK_CAP = 0.01
BAND = 256           # bytes behind the action buffer, floats behind h1 / base / the scratch
SENT = -77           # the action buffer's fill: negative, so no pick and no in-range random action equals it
SENT_F = -12345.678
WS_FILL, BAND_FILL = 0x5A, 0x3C
OK, EINVAL = 0, 22


def _L(ms):
    return importlib.import_module("marl-scheduling_amd._lib")


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _net_dev(net):
    return {k: _dev(net[k]) for k in BDQN_KEYS}


def _params(ms, netd, obs, ac, n):
    ptr = _L(ms).ptr
    return ms.abi.MsBdqnParams(*[ptr(netd[k]) for k in BDQN_KEYS], obs, ac, n)


def _with_tail(a, fill):
    """a with br.EXTRA_ROWS more rows of garbage behind it (fill: a value, or 'pm127')."""
    a = np.asarray(a)
    shape = (br.EXTRA_ROWS,) + a.shape[1:]
    if isinstance(fill, str):
        tail = np.random.default_rng(7).choice(br.PAD_BYTES, shape)
    else:
        tail = np.full(shape, fill, dtype=a.dtype)
    return _dev(np.concatenate([a, tail.astype(a.dtype)]))


def _band_f(nfloats, fill=float("nan")):
    t = torch.full((nfloats + BAND,), fill, dtype=torch.float32, device="cuda")
    t[nfloats:] = SENT_F
    return t


def _band_f_intact(t, nfloats):
    return bool((t[nfloats:] == torch.tensor(SENT_F, dtype=torch.float32)).all())


def _bytes_buf(nbytes, fill):
    t = torch.full((nbytes + 4 * BAND,), fill, dtype=torch.uint8, device="cuda")
    t[nbytes:] = BAND_FILL
    return t


def _bytes_intact(t, nbytes):
    return bool((t[nbytes:] == BAND_FILL).all())


def _ratio(num, den):
    if den > 0:
        return num / den
    return 0.0 if num == 0 else float("inf")


def _compare(tag, got, want64, got32):
    got, want64, got32 = (np.asarray(x, dtype=np.float64) for x in (got, want64, got32))
    assert got.shape == want64.shape, tag
    assert np.isfinite(got).all(), tag  # fully overwritten: no NaN left
    e_hip = float(np.abs(got - want64).max())
    e_f32 = float(np.abs(got32 - want64).max())
    floor = EPS32 * float(np.abs(want64).max())
    ratio = _ratio(e_hip, max(e_f32, floor))
    print("BACT|%s|e_hip %.3e|e_f32 %.3e|floor %.3e|ratio %.3f" % (tag, e_hip, e_f32, floor, ratio))
    assert ratio <= R_L1, (tag, e_hip, e_f32, floor, ratio)
    return ratio


def _check_picks(tag, got, ref, n, rows=None):
    """The pick rule on the greedy actions got [R, A] (rows: a mask of the rows to hold to it, default all)."""
    q64, q32 = ref["q64"], ref["q32"]
    assert got.shape == q64.shape[:2], tag
    assert ((got >= 0) & (got < n)).all(), tag
    keep = np.ones(got.shape[0], dtype=bool) if rows is None else rows
    regret = q64.max(axis=2) - np.take_along_axis(q64, got[..., None], axis=2)[..., 0]
    floor = EPS32 * float(np.abs(q64).max())
    den = np.maximum(np.abs(q32 - q64).max(axis=2), floor)
    assert (den > 0).all(), tag
    ratio = float((regret / den)[keep].max()) if keep.any() else 0.0
    differ = float((got != ref["pick"])[keep].mean()) if keep.any() else 0.0
    print("BACT|%s|picks|differ %.5f|worst regret ratio %.3f" % (tag, differ, ratio))
    assert ratio <= R_BACT, (tag, ratio)
    assert differ <= PICK_CAP, (tag, differ)
    return ratio


def _prepare(ms, qp, seg, segs, want_base):
    """ms_bdqn_prepare on a workspace of exactly ms_bdqn_workspace_bytes with a band behind it: (ws, base, nbytes)."""
    L = _L(ms)
    nb = int(L.lib.ms_bdqn_workspace_bytes(seg, segs))
    assert nb == 3 * br.BH * segs * br.pad32(seg) * 2 + segs * br.BH * 4
    ws = _bytes_buf(nb, WS_FILL)
    base = _band_f(br.BH) if want_base else None
    L.check(L.lib.ms_bdqn_prepare(ct.byref(qp), seg, segs, L.ptr(ws), nb, L.ptr(base), L.stream_ptr()))
    torch.cuda.synchronize()
    assert _bytes_intact(ws, nb)
    assert base is None or _band_f_intact(base, br.BH)
    return ws, base, nb


def _check_split(ws, w1, seg, segs):
    """The workspace's [3][128][segs][Dp] bf16 terms: hi + mid + lo == W1 exactly for k < seg, zero past it."""
    Dp = br.pad32(seg)
    cnt = 3 * br.BH * segs * Dp
    bits = ws[: 2 * cnt].cpu().numpy().view(np.uint16).astype(np.uint32) << 16
    terms = bits.view(np.float32).reshape(3, br.BH, segs, Dp).astype(np.float64)
    want = np.asarray(w1, dtype=np.float64).reshape(br.BH, segs, seg)
    assert np.array_equal(terms.sum(axis=0)[..., :seg], want)
    assert (bits.reshape(3, br.BH, segs, Dp)[..., seg:] == 0).all()
    # each term keeps eight significant bits, the later ones below the earlier
    assert (np.abs(terms[1]) <= np.abs(terms[0]) * 2.0 ** -7).all() and (np.abs(terms[2]) <= np.abs(terms[0]) * 2.0 ** -15).all()


def _act(ms, qp, A, rows, h1=None, x=None, x_stride=0, ws=None, ex=None, rnd=None):
    """ms_bdqn_act into a sentinel-filled buffer with a band: the actions [rows, A] as int64."""
    L = _L(ms)
    action = torch.full((rows * A + BAND,), SENT, dtype=torch.int8, device="cuda")
    L.check(L.lib.ms_bdqn_act(ct.byref(qp), L.ptr(h1), L.ptr(x), x_stride, L.ptr(ws), rows, L.ptr(ex), L.ptr(rnd),
                              L.ptr(action), L.stream_ptr()))
    torch.cuda.synchronize()
    a = action.cpu().numpy()
    assert (a[rows * A:] == SENT).all()
    return a[: rows * A].reshape(rows, A).astype(np.int64)


def _check_explore(got, greedy, ex, rnd, n):
    """Exploring rows take rand_action, the others the greedy pick; no out-of-range byte of rand_action shows."""
    e = ex != 0
    assert np.array_equal(got[e], rnd[e].astype(np.int64))
    assert np.array_equal(got[~e], greedy[~e])
    assert ((got >= 0) & (got < n)).all()


def _greedy_and_explore(ms, c, qp, rows, **src):
    """Greedy twice (same bits) and epsilon-greedy with the case's explore bytes: the greedy actions."""
    A, n = c["A"], c["n"]
    greedy = _act(ms, qp, A, rows, **src)
    assert ((greedy >= 0) & (greedy < n)).all()  # in range, so the sentinel is fully overwritten
    assert np.array_equal(greedy, _act(ms, qp, A, rows, **src))
    ex, rnd = _with_tail(c["explore"], 255), _with_tail(c["rnd"], -128)
    got = _act(ms, qp, A, rows, ex=ex, rnd=rnd, **src)
    _check_explore(got, greedy, c["explore"], c["rnd"], n)
    return greedy


# ------------------------------------------------------------------------------------- H: ms_bdqn_act on h1

@pytest.mark.parametrize("name", list(br.H_CASES))
def test_act_on_h1_matches_float64(ms, name):
    c = br.h_case(name)
    netd = _net_dev(c["net"])
    qp = _params(ms, netd, br.H_OBS, c["A"], c["n"])
    greedy = _greedy_and_explore(ms, c, qp, c["rows"], h1=_with_tail(c["h1"], np.float32("nan")))
    _check_picks("H-" + name, greedy, c["ref"], c["n"])


@pytest.mark.parametrize("n", br.TIE_N + (5,))
def test_act_exact_ties_take_the_first_index(ms, n):
    """Bit-equal maxima in one lane at two q, in two lane groups, in two tiles and in the first and last tile, each
    under every writer lane group; a branch of all-equal q; n = 5: the NMT = 1 scan with empty lane groups."""
    c = br.tie_case(n)
    netd = _net_dev(c["net"])
    qp = _params(ms, netd, br.H_OBS, c["A"], n)
    got = _act(ms, qp, c["A"], c["rows"], h1=_with_tail(c["h1"], np.float32("nan")))
    want = np.broadcast_to(c["expect"], got.shape)
    assert np.array_equal(got, want), np.argwhere(got != want)[:8]
    _check_picks("T-n%d" % n, got, c["ref"], n)


# ----------------------------------------------------------------------------- X: ms_bdqn_act on int8 rows

@pytest.mark.parametrize("name", list(br.X_CASES))
def test_act_on_int8_rows_matches_float64(ms, name):
    c = br.x_case(name)
    netd = _net_dev(c["net"])
    qp = _params(ms, netd, c["obs"], c["A"], c["n"])
    ws, _, _ = _prepare(ms, qp, c["obs"], 1, False)
    _check_split(ws, c["net"]["w1"], c["obs"], 1)
    greedy = _greedy_and_explore(ms, c, qp, c["rows"], x=_with_tail(c["x"], "pm127"), x_stride=c["x_stride"], ws=ws)
    _check_picks("X-" + name, greedy, c["ref"], c["n"])


# -------------------------------------------------------- L, C: the compact layer 1 and ms_bdqn_act_compact

class _Compact:
    """The device side of an L or C case: prepared workspace and base, the compact observations with garbage
    replicas behind them, and a scratch of exactly ms_bdqn_layer1_scratch_bytes filled with 0xFF."""

    def __init__(self, ms, c):
        L = _L(ms)
        self.ms, self.c, self.L = ms, c, L
        self.netd = _net_dev(c["net"])
        self.qp = _params(ms, self.netd, c["C"] * c["D"], c["A"], c["n"])
        self.ws, self.base, self.ws_bytes = _prepare(ms, self.qp, c["D"], c["C"], True)
        self.core_rows = _with_tail(c["core_rows"], "pm127")
        self.core_owner = _with_tail(c["core_owner"], 127)
        self.sb = int(L.lib.ms_bdqn_layer1_scratch_bytes(c["E"], c["C"]))
        assert self.sb > 0 and self.sb % 4 == 0
        self.scratch = _bytes_buf(self.sb, 0xFF)
        self.rows = c["E"] * c["N"]

    def shape_args(self):
        c = self.c
        return (c["E"], c["N"], c["C"], c["D"], c["stride"])

    def layer1(self):
        L = self.L
        h1 = _band_f(self.rows * br.BH)
        L.check(L.lib.ms_bdqn_layer1_compact(ct.byref(self.qp), L.ptr(self.ws), L.ptr(self.base), L.ptr(self.core_rows),
                                             L.ptr(self.core_owner), *self.shape_args(), L.ptr(self.scratch), self.sb,
                                             L.ptr(h1), L.stream_ptr()))
        torch.cuda.synchronize()
        assert _band_f_intact(h1, self.rows * br.BH) and _bytes_intact(self.scratch, self.sb)
        return h1[: self.rows * br.BH].cpu().numpy().reshape(self.rows, br.BH)

    def act_compact(self, ex=None, rnd=None):
        L, A = self.L, self.c["A"]
        action = torch.full((self.rows * A + BAND,), SENT, dtype=torch.int8, device="cuda")
        L.check(L.lib.ms_bdqn_act_compact(ct.byref(self.qp), L.ptr(self.ws), L.ptr(self.base), L.ptr(self.core_rows),
                                          L.ptr(self.core_owner), *self.shape_args(), L.ptr(self.scratch), self.sb,
                                          L.ptr(ex), L.ptr(rnd), L.ptr(action), L.stream_ptr()))
        torch.cuda.synchronize()
        a = action.cpu().numpy()
        assert (a[self.rows * A:] == SENT).all() and _bytes_intact(self.scratch, self.sb)
        return a[: self.rows * A].reshape(self.rows, A).astype(np.int64)


def _check_layer1(tag, k):
    c = k.c
    _check_split(k.ws, c["net"]["w1"], c["D"], c["C"])
    worst = _compare(tag + "|base", k.base[: br.BH].cpu().numpy(), c["base64"], c["base32"])
    h1 = k.layer1()
    assert not np.isnan(h1).any()
    worst = max(worst, _compare(tag + "|h1", h1, c["h64"], c["h32"]))
    h1b = k.layer1()  # the same scratch again
    assert np.array_equal(h1.view(np.int32), h1b.view(np.int32))
    return h1


@pytest.mark.parametrize("name", list(br.L_CASES))
def test_layer1_compact_matches_float64(ms, name):
    _check_layer1("L-" + name, _Compact(ms, br.compact_case("L", name)))


@pytest.mark.parametrize("name", list(br.C_CASES))
def test_act_compact_matches_float64_and_the_dense_route(ms, name):
    c = br.compact_case("C", name)
    k = _Compact(ms, c)
    A, n, rows = c["A"], c["n"], k.rows
    ex, rnd = _with_tail(c["explore"], 255), _with_tail(c["rnd"], -128)
    # compact first, on the 0xFF scratch: nothing of it is read before it is written
    greedy = k.act_compact()
    _check_picks("C-" + name, greedy, c["ref"], n)
    assert np.array_equal(greedy, k.act_compact())  # the list order may differ, the actions may not
    got = k.act_compact(ex, rnd)
    _check_explore(got, greedy, c["explore"], c["rnd"], n)
    assert np.array_equal(got, k.act_compact(ex, rnd))
    # the dense route: ms_bdqn_layer1_compact, then ms_bdqn_act on its h1
    h1 = _with_tail(_check_layer1("C-" + name, k), np.float32("nan"))
    dense = _act(ms, k.qp, A, rows, h1=h1)
    _check_picks("C-" + name + "|dense", dense, c["ref"], n)
    assert np.array_equal(greedy, dense)
    assert np.array_equal(got, _act(ms, k.qp, A, rows, h1=h1, ex=ex, rnd=rnd))
    if c["own"] == "none":  # one common action vector, the pick of layer 1 = base
        assert (greedy == greedy[0]).all()
        assert np.abs(c["h64"] - c["base64"]).max() == 0


# ------------------------------------------------------------------------------------------------ refusals

def _refused(rc, *outs):
    torch.cuda.synchronize()
    assert rc == EINVAL, rc
    for t, fill in outs:
        if isinstance(fill, float) and np.isnan(fill):
            assert bool(torch.isnan(t).all())
        else:
            assert bool((t == fill).all())


def test_act_refuses_bad_arguments(ms):
    """MS_EINVAL before any launch, the action buffer untouched; the same call with nothing wrong runs."""
    L = _L(ms)
    obs, A, n, rows = 40, 3, 20, 33
    rng = np.random.default_rng(3)
    net = br._net(rng, obs, A, n)
    netd = _net_dev(net)
    x = _dev(rng.integers(-5, 14, (rows, 44)).astype(np.int8))
    h1 = _dev(br._h1_rows(rng, rows))
    ex = torch.ones(rows, dtype=torch.uint8, device="cuda")
    rnd = torch.zeros((rows, A), dtype=torch.int8, device="cuda")
    qp = _params(ms, netd, obs, A, n)
    ws, _, nb = _prepare(ms, qp, obs, 1, False)
    action = torch.full((rows * 128,), SENT, dtype=torch.int8, device="cuda")

    def call(q, h, xx, stride, w, e, r):
        return L.lib.ms_bdqn_act(ct.byref(q), L.ptr(h), L.ptr(xx), stride, L.ptr(w), rows, L.ptr(e), L.ptr(r),
                                 L.ptr(action), L.stream_ptr())

    for bad_n, bad_A in ((129, A), (0, A), (n, 128)):
        _refused(call(_params(ms, netd, obs, bad_A, bad_n), h1, None, 0, None, None, None), (action, SENT))
    wide = br._net(rng, 257, A, n)
    wd = _net_dev(wide)
    x257 = torch.zeros((rows, 260), dtype=torch.int8, device="cuda")
    _refused(call(_params(ms, wd, 257, A, n), None, x257, 260, ws, None, None), (action, SENT))
    _refused(call(qp, None, x, 36, ws, None, None), (action, SENT))   # x_stride < obs
    _refused(call(qp, None, x, 42, ws, None, None), (action, SENT))   # x_stride % 4
    _refused(call(qp, None, x, 44, None, None, None), (action, SENT))  # no workspace
    _refused(call(qp, h1, None, 0, None, ex, None), (action, SENT))   # explore without rand_action
    _refused(call(qp, None, x, 44, ws, ex, None), (action, SENT))
    # the same calls with nothing wrong
    assert call(qp, h1, None, 0, None, ex, rnd) == OK
    assert call(qp, None, x, 44, ws, None, None) == OK
    assert call(_params(ms, netd, obs, A, n), h1, None, 0, None, None, None) == OK
    torch.cuda.synchronize()
    assert bool((action[: rows * A] >= 0).all()) and bool((action[rows * A:] == SENT).all())


def test_prepare_refuses_bad_arguments(ms):
    L = _L(ms)
    D, C, A, n = 9, 4, 4, 5
    rng = np.random.default_rng(4)
    netd = _net_dev(br._net(rng, C * D, A, n))
    qp = _params(ms, netd, C * D, A, n)
    nb = int(L.lib.ms_bdqn_workspace_bytes(D, C))
    ws = _bytes_buf(nb, WS_FILL)
    base = _band_f(br.BH)

    def call(seg, segs, nbytes):
        return L.lib.ms_bdqn_prepare(ct.byref(qp), seg, segs, L.ptr(ws), nbytes, L.ptr(base), L.stream_ptr())

    for seg, segs, nbytes in ((D, C - 1, nb), (D + 1, C, nb + 4096), (D, C, nb - 1)):
        _refused(call(seg, segs, nbytes), (ws[:nb], WS_FILL), (base[: br.BH], float("nan")))
    assert call(D, C, nb) == OK
    torch.cuda.synchronize()
    assert not bool(torch.isnan(base[: br.BH]).any()) and _bytes_intact(ws, nb) and _band_f_intact(base, br.BH)


def test_compact_entry_points_refuse_bad_arguments(ms):
    """ms_bdqn_layer1_compact and ms_bdqn_act_compact: MS_EINVAL with h1 and the actions untouched."""
    L = _L(ms)
    rng = np.random.default_rng(5)
    E, N, C, D, stride, n = 6, 3, 4, 9, 12, 5
    netd = _net_dev(br._net(rng, C * D, C, n))
    qp = _params(ms, netd, C * D, C, n)
    ws, base, _ = _prepare(ms, qp, D, C, True)
    # nets whose obs fits the refused acc_dim, so that only the acc_dim is wrong
    q3 = _params(ms, _net_dev(br._net(rng, C * 3, C, n)), C * 3, C, n)
    n257 = _net_dev(br._net(rng, C * 257, C, n))
    q257 = _params(ms, n257, C * 257, C, n)
    cr = torch.zeros((E + 60, C, 264), dtype=torch.int8, device="cuda")
    co = torch.zeros((E + 60, C), dtype=torch.int8, device="cuda")
    sb = int(L.lib.ms_bdqn_layer1_scratch_bytes(E + 60, C))
    scratch = _bytes_buf(sb, 0xFF)
    sb_e = int(L.lib.ms_bdqn_layer1_scratch_bytes(E, C))
    ex = torch.ones(E * 65, dtype=torch.uint8, device="cuda")
    rnd = torch.zeros((E * 65, C), dtype=torch.int8, device="cuda")
    h1 = torch.full((E * 65 * br.BH,), float("nan"), dtype=torch.float32, device="cuda")
    action = torch.full((E * 65 * C,), SENT, dtype=torch.int8, device="cuda")

    def l1(q, n_agents, acc_dim, acc_stride, nbytes, n_cores=C):
        return L.lib.ms_bdqn_layer1_compact(ct.byref(q), L.ptr(ws), L.ptr(base), L.ptr(cr), L.ptr(co), E, n_agents,
                                            n_cores, acc_dim, acc_stride, L.ptr(scratch), nbytes, L.ptr(h1),
                                            L.stream_ptr())

    def ac(q, n_agents, acc_dim, acc_stride, nbytes, e=None, r=None, n_cores=C):
        return L.lib.ms_bdqn_act_compact(ct.byref(q), L.ptr(ws), L.ptr(base), L.ptr(cr), L.ptr(co), E, n_agents,
                                         n_cores, acc_dim, acc_stride, L.ptr(scratch), nbytes, L.ptr(e), L.ptr(r),
                                         L.ptr(action), L.stream_ptr())

    bad = ((q3, N, 3, 4, sb), (q257, N, 257, 260, sb), (qp, N, D, 14, sb), (qp, N, D, 8, sb), (qp, N, D + 1, stride, sb),
           (qp, N, D, stride, sb_e - 1))
    for args in bad:
        _refused(l1(*args), (h1, float("nan")))
        _refused(ac(*args), (action, SENT))
    _refused(l1(qp, N, D, stride, sb, n_cores=C - 1), (h1, float("nan")))  # obs != n_cores * acc_dim
    _refused(ac(qp, N, D, stride, sb, n_cores=C - 1), (action, SENT))
    _refused(ac(qp, 65, D, stride, sb), (action, SENT))
    _refused(ac(qp, N, D, stride, sb, e=ex), (action, SENT))               # explore without rand_action
    for bad_n, bad_A in ((129, C), (0, C), (n, 128)):
        _refused(ac(_params(ms, netd, C * D, bad_A, bad_n), N, D, stride, sb), (action, SENT))
    assert bool((scratch[:sb] == 0xFF).all())  # no refused call touched the scratch
    # nothing wrong: the exact scratch size, and 64 agents
    assert l1(qp, N, D, stride, sb_e) == OK and ac(qp, N, D, stride, sb_e, ex, rnd) == OK
    assert ac(qp, 64, D, stride, sb) == OK
    torch.cuda.synchronize()
    assert not bool(torch.isnan(h1[: E * N * br.BH]).any()) and bool(torch.isnan(h1[E * N * br.BH:]).all())
    assert bool((action[: E * 64 * C] >= 0).all()) and bool((action[E * 64 * C:] == SENT).all())
    assert _bytes_intact(scratch, sb)
