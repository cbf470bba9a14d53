"""ms_wide_act and ms_wide_grad (wide_kernels.hip: k_wide_act; k_wide_rows, k_wide_outer, k_wide_w3, k_wide_reduce) on
the device against the float64 references of oracle/wide_ref.py, through the C entry points (so stride, pad bytes
and the workspace are the test's to set), at the seams of the work plan (several row tiles per block, the row splits)
and of the kernels' thread mappings. tests/test_wide_ref.py proves on the CPU that the tables reach them, that no
gradient case sits on a discontinuity, and that float32 sampling keeps the cap used here.

Gradient, per case and tensor and for each of the three loss terms (one launch, gradients before Adam):

    e_hip = max |hip - f64| <= R_WIDE[family] * max(e_f32, 2^-24 * max |f64|),  e_f32 = max |float32 CPU autograd - f64|

and a tensor whose float64 reference is identically zero is exactly zero. Every case also checks: outputs and loss
pre-filled with NaN are fully overwritten; the workspace is NaN-filled, passed at exactly ms_wide_workspace_bytes, and
the 256-float band after it stays intact; a second launch is bit-identical; every pad byte of the rows, and three rows
after row R - 1 of states (+-127), actions (out of range) and old log-probs (NaN) hold garbage; returns [G][R] ends
its NaN-padded buffer.

Act, per row with the device's pick a at the injected uniform u:

    cdf64[a - 1] - d <= u <= cdf64[a] + d,   d = R_ACT * max(max |cdf32 - cdf64| of the row, 2^-24)

(cdf64[-1] = 0; cdf32 the float32 restatement's sequential running sums); at most 1 % of a case's rows differ from
the float64 pick (rows that differ are held to the rule like the others); the log-prob is log(clamp(p64[a])) of the
device's own pick under R_ACT * max(e_f32, 2^-24 * max |f64|); uniforms past row E - 1 are NaN, the action and
log-prob slots past E * G keep their sentinels; a second launch is bit-identical. Some rows of every case have
u = 0 and u = 1 - 2^-24; act/ties-A4 (equal logits, exact float32 sums) has u on the boundaries themselves, where
the pick is the action after the boundary on every row.

The kernels use the hardware exp / log / rcp / tanh and their own summation orders, so the constants are measured,
not derived: twice the largest ratio over the table on an MI355X, rounded up to a power of two
(profiles/wide_parity/README.md has every case's figures). Every tensor prints a "WIDE|case|tensor|e_hip|e_f32|
floor|ratio" line (pytest -s)."""
import ctypes as ct
import importlib

import numpy as np
import pytest
import torch

from oracle import wide_ref as wr

pytestmark = pytest.mark.gpu

# Twice the largest e_hip / max(e_f32, floor) measured on an MI355X, rounded up to a power of two, per family
# (profiles/wide_parity/README.md). Measured: R 7.54 (R/R3841 loss_ent), T 9.87 (T/G2-R16437 loss_min), D 3.71
# (D/D1), A 4.85 (A/A2), S 1.62 (S/A257). The largest are loss terms of the cases with the most row tiles:
# k_wide_reduce adds the NB block partials (257 and 1024 of them) one after the other in float32; the gradients of
# those cases stay under 3.1. R_ACT: 2.41 (act/E37 logprob); the pick rule's largest miss is 0.5 of its yardstick
# (act/sat-A25, a forced u = 1 - 2^-24 row).
R_WIDE = {"R": 16.0, "T": 32.0, "D": 8.0, "A": 16.0, "S": 4.0}
R_ACT = 8.0
GUARD = 256
SENTINEL = -12345.678
ACT_SENTINEL = -77777
OK, EINVAL = 0, 22
LOSS_TERMS = ("loss_min", "loss_mse", "loss_ent")
RET_PAD = 64


def _lib():
    return importlib.import_module("marl-scheduling_amd._lib")


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _params(ms, L, w, D, H, A, G):
    actor = ms.abi.MsMlpParams(*[L.ptr(w[k]) for k in wr.ACTOR_KEYS], D, H, A, G, None, 0)
    critic = ms.abi.MsMlpParams(*[L.ptr(w[k]) for k in wr.CRITIC_KEYS], D, H, 1, G, None, 0)
    return actor, critic


def _launch_grad(ms, c, calls=2):
    """ms_wide_grad `calls` times on fresh NaN-filled outputs (the workspace kept): [(loss [G, 3], grads)] as numpy,
    after the return codes and the guard band were checked."""
    L = _lib()
    s = c["spec"]
    G, D, A, H, R, stride = (s[k] for k in ("G", "D", "A", "H", "R", "stride"))
    w = {k: _dev(v) for k, v in c["nets"].items()}
    actor, critic = _params(ms, L, w, D, H, A, G)
    states, actions, olp = _dev(c["states"]), _dev(c["actions"]), _dev(c["olp"])
    ret = torch.full((RET_PAD + G * R,), float("nan"), dtype=torch.float32, device="cuda")
    ret[RET_PAD:] = _dev(c["ret"]).reshape(-1)  # nothing of the buffer follows returns[G - 1][R - 1]
    batch = ms.abi.MsWideBatch(states=L.ptr(states), actions=L.ptr(actions), old_logprob=L.ptr(olp),
                               returns=L.ptr(ret[RET_PAD:]), stride=stride, rows=R)
    nb = int(L.lib.ms_wide_workspace_bytes(ct.byref(actor), R))
    assert nb == c["plan"]["bytes"] and nb % 4 == 0
    ws = torch.full((nb // 4 + GUARD,), float("nan"), dtype=torch.float32, device="cuda")
    ws[nb // 4:] = SENTINEL
    out = []
    for _ in range(calls):
        g = {k: torch.full_like(w[k], float("nan")) for k in wr.KEYS}
        loss = torch.full((G, 3), float("nan"), dtype=torch.float32, device="cuda")
        gr = ms.abi.MsPpoGrads(*[L.ptr(g[k]) for k in wr.KEYS], L.ptr(loss))
        L.check(L.lib.ms_wide_grad(ct.byref(actor), ct.byref(critic), ct.byref(batch), ct.c_float(wr.EPS_CLIP),
                                   L.ptr(ws), nb, ct.byref(gr), L.stream_ptr()))
        torch.cuda.synchronize()
        out.append((loss.cpu().numpy(), {k: v.cpu().numpy() for k, v in g.items()}))
    assert bool((ws[nb // 4:] == torch.tensor(SENTINEL, dtype=torch.float32)).all())  # the band after the workspace
    return out


def _same_bits(a, b):
    (la, ga), (lb, gb) = a, b
    return np.array_equal(la.view(np.int32), lb.view(np.int32)) and all(
        np.array_equal(ga[k].view(np.int32), gb[k].view(np.int32)) for k in wr.KEYS)


def _compare(tag, got, want64, got32):
    """One tensor (or one loss term): its e_hip / max(e_f32, floor), printed. inf for a nonzero value where the
    reference is identically zero."""
    got, want64, got32 = (np.asarray(x, dtype=np.float64) for x in (got, want64, got32))
    assert got.shape == want64.shape, tag
    assert np.isfinite(got).all(), tag  # NaN: not overwritten, or garbage was read
    e_hip, e_f32 = float(np.abs(got - want64).max()), float(np.abs(got32 - want64).max())
    floor = wr.EPS32 * float(np.abs(want64).max())
    if not want64.any():
        ratio = 0.0 if not got.any() else float("inf")
    else:
        ratio = e_hip / max(e_f32, floor)
    print("WIDE|%s|e_hip %.3e|e_f32 %.3e|floor %.3e|ratio %.3f" % (tag, e_hip, e_f32, floor, ratio))
    return ratio


@pytest.mark.parametrize("name", list(wr.GRAD_CASES))
def test_wide_grad_matches_float64(ms, name):
    c = wr.grad_case(name)
    first, second = _launch_grad(ms, c)
    assert _same_bits(first, second)
    loss, grads = first
    (g64, l64), (g32, l32) = c["ref"], c["f32"]
    ratios = {k: _compare("%s|%s" % (name, k), grads[k], g64[k], g32[k]) for k in wr.KEYS}
    for i, term in enumerate(LOSS_TERMS):
        ratios[term] = _compare("%s|%s" % (name, term), loss[:, i], l64[:, i], l32[:, i])
    print("WIDE|%s|worst %.3f" % (name, max(ratios.values())))
    bound = R_WIDE[c["spec"]["family"]]
    over = {k: round(v, 3) for k, v in ratios.items() if not v <= bound}  # every tensor is printed before any fails
    assert not over, (name, bound, over)


def _launch_act(ms, c, calls=2):
    L = _lib()
    s = c["spec"]
    G, D, A, H, E, stride = (s[k] for k in ("G", "D", "A", "H", "E", "stride"))
    w = {k: _dev(c["nets"][k]) for k in wr.ACTOR_KEYS}
    actor = ms.abi.MsMlpParams(*[L.ptr(w[k]) for k in wr.ACTOR_KEYS], D, H, A, G, None, 0)
    obs, u = _dev(c["obs"]), _dev(c["u"])
    out = []
    for _ in range(calls):
        action = torch.full((E * G + GUARD,), ACT_SENTINEL, dtype=torch.int32, device="cuda")
        logprob = torch.full((E * G + GUARD,), SENTINEL, dtype=torch.float32, device="cuda")
        L.check(L.lib.ms_wide_act(ct.byref(actor), L.ptr(obs), stride, E, L.ptr(u), L.ptr(action), L.ptr(logprob),
                                  L.stream_ptr()))
        torch.cuda.synchronize()
        a, lp = action.cpu().numpy(), logprob.cpu().numpy()
        assert (a[E * G:] == ACT_SENTINEL).all() and (lp[E * G:] == np.float32(SENTINEL)).all()
        out.append((a[:E * G].reshape(E, G).T.copy(), lp[:E * G].reshape(E, G).T.copy()))
    return out


@pytest.mark.parametrize("name", list(wr.ACT_CASES))
def test_wide_act_matches_float64(ms, name):
    c = wr.act_case(name)
    A = c["spec"]["A"]
    (a, lp), (a2, lp2) = _launch_act(ms, c)
    assert np.array_equal(a, a2) and np.array_equal(lp.view(np.int32), lp2.view(np.int32))
    assert a.min() >= 0 and a.max() < A and np.isfinite(lp).all()
    cdf64, u = c["cdf64"], c["ug"].astype(np.float64)
    a64 = a.astype(np.int64)
    hi = np.take_along_axis(cdf64, a64[..., None], -1)[..., 0]
    lo = np.where(a64 > 0, np.take_along_axis(cdf64, np.maximum(a64 - 1, 0)[..., None], -1)[..., 0], 0.0)
    yard = np.maximum(np.abs(c["cdf32"].astype(np.float64) - cdf64).max(-1), wr.EPS32)
    miss = np.maximum(np.maximum(lo - u, u - hi), 0.0)
    r_cdf = float((miss / yard).max())
    differ = a64 != c["pick64"]
    print("WIDE|act/%s|cdf|miss %.3e|yard %.3e|differ %d of %d|ratio %.3f"
          % (name, float(miss.max()), float(yard.max()), int(differ.sum()), differ.size, r_cdf))
    lp64 = wr.clamped_log(np.take_along_axis(c["p64"], a64[..., None], -1)[..., 0])
    p32 = np.take_along_axis(c["p32"], a64[..., None], -1)[..., 0]
    lp32 = np.log(np.clip(p32, np.float32(wr.EPS_P), np.float32(1.0 - wr.EPS_P)))
    r_lp = _compare("act/%s|logprob" % name, lp, lp64, lp32)
    assert r_cdf <= R_ACT, (name, r_cdf)
    assert differ.mean() <= 0.01, (name, int(differ.sum()), differ.size)
    assert r_lp <= R_ACT, (name, r_lp)
    zeros, _ = c["forced"]
    first_alive = (c["p32"][..., 0] > 0).T.reshape(-1)[zeros]  # u = 0 takes the first action unless its exp is 0
    assert (a.T.reshape(-1)[zeros][first_alive] == 0).all()


# (what is wrong, hidden, in_dim, n_actions, stride, rows, workspace bytes short)
REFUSALS = [("hidden 48", 48, 8, 9, 8, 40, 0), ("in_dim 0", 32, 0, 9, 8, 40, 0), ("in_dim 256", 32, 256, 9, 256, 40, 0),
            ("n_actions 0", 32, 8, 0, 8, 40, 0), ("stride < in_dim", 32, 9, 9, 8, 40, 0),
            ("stride % 4", 32, 8, 9, 10, 40, 0), ("rows 0", 32, 8, 9, 8, 0, 0), ("workspace short", 32, 8, 9, 8, 40, 1),
            ("nothing", 32, 8, 9, 8, 40, 0)]


def test_refusals_before_any_launch(ms):
    """MS_EINVAL and the sentinel-filled outputs untouched, for ms_wide_grad and (all but the workspace) ms_wide_act.
    Every buffer has the true size of the stated shape, so a refusal that is missed reads inside its allocations;
    the last entry, with nothing wrong, runs."""
    L = _lib()
    G = 2
    for what, H, D, A, stride, R, short in REFUSALS:
        rows = max(R, 1)
        shapes = dict(w1=(G, H, max(D, 1)), b1=(G, H), w2=(G, H, H), b2=(G, H), w3=(G, max(A, 1), H), b3=(G, max(A, 1)),
                      cw1=(G, H, max(D, 1)), cb1=(G, H), cw2=(G, H, H), cb2=(G, H), cw3=(G, 1, H), cb3=(G, 1))
        w = {k: torch.zeros(v, dtype=torch.float32, device="cuda") for k, v in shapes.items()}
        actor, critic = _params(ms, L, w, D, H, A, G)
        states = torch.zeros((rows, G, max(stride, D, 1)), dtype=torch.int8, device="cuda")
        actions = torch.zeros((rows, G), dtype=torch.int32, device="cuda")
        olp = torch.zeros((rows, G), dtype=torch.float32, device="cuda")
        ret = torch.zeros((G, rows), dtype=torch.float32, device="cuda")
        u = torch.full((rows, G), 0.5, dtype=torch.float32, device="cuda")
        batch = ms.abi.MsWideBatch(states=L.ptr(states), actions=L.ptr(actions), old_logprob=L.ptr(olp),
                                   returns=L.ptr(ret), stride=stride, rows=R)
        # the size of the nearest shape the entry point accepts: what a missed refusal would at most use
        need = wr.workspace_bytes(G, min(max(D, 1), 255), max(A, 1), 64, rows)
        if what in ("workspace short", "nothing"):
            assert int(L.lib.ms_wide_workspace_bytes(ct.byref(actor), R)) == wr.workspace_bytes(G, D, A, H, R) > 0
            need = wr.workspace_bytes(G, D, A, H, R)
        elif what in ("hidden 48", "in_dim 0", "in_dim 256", "n_actions 0", "rows 0"):
            assert int(L.lib.ms_wide_workspace_bytes(ct.byref(actor), R)) == 0
        ws = torch.zeros(need // 4, dtype=torch.float32, device="cuda")
        g = {k: torch.full_like(w[k], float("nan")) for k in wr.KEYS}
        loss = torch.full((G, 3), float("nan"), dtype=torch.float32, device="cuda")
        gr = ms.abi.MsPpoGrads(*[L.ptr(g[k]) for k in wr.KEYS], L.ptr(loss))
        rc = L.lib.ms_wide_grad(ct.byref(actor), ct.byref(critic), ct.byref(batch), ct.c_float(0.2), L.ptr(ws),
                                need - short, ct.byref(gr), L.stream_ptr())
        action = torch.full((rows * G,), ACT_SENTINEL, dtype=torch.int32, device="cuda")
        logprob = torch.full((rows * G,), SENTINEL, dtype=torch.float32, device="cuda")
        rc_act = L.lib.ms_wide_act(ct.byref(actor), L.ptr(states), stride, R, L.ptr(u), L.ptr(action), L.ptr(logprob),
                                   L.stream_ptr())
        torch.cuda.synchronize()
        if what == "nothing":
            assert rc == OK and not bool(torch.isnan(loss).any())
            assert not any(bool(torch.isnan(v).any()) for v in g.values())
        else:
            assert rc == EINVAL, (what, rc)
            assert bool(torch.isnan(loss).all()) and all(bool(torch.isnan(v).all()) for v in g.values()), what
        if what in ("nothing", "workspace short"):
            assert rc_act == OK and bool((action != ACT_SENTINEL).all()) and bool((logprob != SENTINEL).all())
        else:
            assert rc_act == EINVAL, (what, rc_act)
            assert bool((action == ACT_SENTINEL).all()) and bool((logprob == SENTINEL).all()), what
