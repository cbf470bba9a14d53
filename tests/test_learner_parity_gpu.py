"""ms_bdqn_update, ms_dqn_grad and ms_dqn_act on the device against the float64 references of
oracle/learner_ref.py, through the C entry points (so the row pitch, the action pitch, the stride and the
workspace are the test's to set), gradients and loss before Adam, at every tile edge of the kernels
(tests/test_learner_ref.py proves on the CPU that the tables reach them and that no case sits on a discontinuity).

Tolerance (per case and tensor, and for the loss): e_hip = max |hip - f64| <= R * max(e_f32, eps32 * max |f64|),
e_f32 = max |torch float32 CPU autograd of the same loss - f64|: the kernels' products are exact and only the f32
summation order differs from torch's, so a kernel needs no more than a small multiple of torch's own error.
Clamped values are compared (the clamp is continuous). Every case prints "LRN|" lines with its figures (pytest -s);
profiles/r15_learner_parity/README.md records them.

Every update case also checks: a second call is bit-identical, gradient tensors pre-filled with NaN are fully
overwritten, the workspace (NaN-filled, so nothing is read before it is written) is not written past
ms_bdqn_update_workspace_bytes / ms_dqn_workspace_bytes (a guard band of 256 floats, ws_bytes passed exact), and the
128-row buffers hold +-127 / NaN garbage in every row past the batch and every byte past obs / ac_dim."""
import ctypes as ct
import importlib

import numpy as np
import pytest
import torch

from oracle import learner_ref as lr

pytestmark = pytest.mark.gpu

# R of the tolerance above: twice the largest e_hip / max(e_f32, floor) measured on an MI355X over all cases of
# the family, rounded up to a power of two (the condition: no more than 16).
# Measured: Branching DQN update 3.90 (the loss of the one-row case B1; gradients 2.9 at most), DQN gradient 2.22
# (w2 of D3). Before the bias and loss row sums of both learners ran in f64 the maxima were 16.56 (bv of heads64)
# and 12.26 (the loss of rows256), all of the excess in those plain f32 running sums.
R_BDQN = 8.0
R_DQN = 8.0
GUARD = 256          # floats after the workspace
SENTINEL = -12345.678
OK, EINVAL = 0, 22


def _lib(ms):
    return importlib.import_module("marl-scheduling_amd._lib")


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _ratio(e_hip, e_f32, floor):
    den = max(e_f32, floor)
    if den > 0:
        return e_hip / den
    return 0.0 if e_hip == 0 else float("inf")


def _compare(tag, got, want64, got32, R):
    """One tensor (or the loss) under the module's rule; returns the ratio."""
    got, want64, got32 = (np.asarray(x, dtype=np.float64) for x in (got, want64, got32))
    assert got.shape == want64.shape, tag
    assert np.isfinite(got).all(), tag
    e_hip = float(np.abs(got - want64).max())
    e_f32 = float(np.abs(got32 - want64).max())
    floor = lr.EPS32 * float(np.abs(want64).max())
    ratio = _ratio(e_hip, e_f32, floor)
    print("LRN|%s|e_hip %.3e|e_f32 %.3e|floor %.3e|ratio %.3f" % (tag, e_hip, e_f32, floor, ratio))
    assert ratio <= R, (tag, e_hip, e_f32, floor, ratio)
    return ratio


def _workspace(nbytes):
    assert nbytes > 0 and nbytes % 4 == 0
    ws = torch.full((nbytes // 4 + GUARD,), float("nan"), dtype=torch.float32, device="cuda")
    ws[nbytes // 4:] = SENTINEL
    return ws


def _guard_intact(ws, nbytes):
    return bool((ws[nbytes // 4:] == torch.tensor(SENTINEL, dtype=torch.float32)).all())


# ------------------------------------------------------------------------------------------ Branching DQN

def _bdqn_params(ms, net, obs, ac, n):
    ptr = _lib(ms).ptr
    return ms.abi.MsBdqnParams(*[ptr(net[k]) for k in lr.BDQN_KEYS], obs, ac, n)


def _bdqn_buffers(c):
    """The 128-row device buffers of a case: rows past the batch and bytes past obs / ac_dim hold garbage."""
    cfg = c["cfg"]
    obs, ac, B = cfg["obs"], cfg["ac"], cfg["B"]
    ld, act_ld = cfg["ld"] or obs, cfg["act_ld"] or ac
    rng = np.random.default_rng(99)
    junk = np.array([-127, 127], dtype=np.int8)
    xs, xn = rng.choice(junk, (128, ld)), rng.choice(junk, (128, ld))
    xs[:B, :obs], xn[:B, :obs] = c["xs"], c["xn"]
    acts = rng.choice(np.array([-128, 127], dtype=np.int8), (128, act_ld))
    acts[:B, :ac] = c["actions"]
    rew, mk = np.full(128, np.nan, dtype=np.float32), np.full(128, np.nan, dtype=np.float32)
    rew[:B], mk[:B] = c["rewards"], c["masks"]
    return dict(xs=_dev(xs), xn=_dev(xn), acts=_dev(acts), rew=_dev(rew), mk=_dev(mk), ld=ld, act_ld=act_ld)


def _bdqn_update(ms, c, calls=2):
    """ms_bdqn_update `calls` times on fresh NaN-filled gradient tensors (the workspace kept): [(loss, grads)]
    as numpy, after the guard band and the return codes were checked."""
    L = _lib(ms)
    cfg = c["cfg"]
    obs, ac, n, B = cfg["obs"], cfg["ac"], cfg["n"], cfg["B"]
    q = {k: _dev(v) for k, v in c["q"].items()}
    t = {k: _dev(v) for k, v in c["t"].items()}
    qp, tp = _bdqn_params(ms, q, obs, ac, n), _bdqn_params(ms, t, obs, ac, n)
    buf = _bdqn_buffers(c)
    nb = int(L.lib.ms_bdqn_update_workspace_bytes(ct.byref(qp), B))
    ws = _workspace(nb)
    bt = ms.abi.MsBdqnBatch(L.ptr(buf["xs"]), L.ptr(buf["xn"]), buf["ld"], L.ptr(buf["acts"]), buf["act_ld"],
                            L.ptr(buf["rew"]), L.ptr(buf["mk"]), B)
    out = []
    for _ in range(calls):
        g = {k: torch.full_like(q[k], float("nan")) for k in lr.BDQN_KEYS}
        loss = torch.full((1,), float("nan"), dtype=torch.float32, device="cuda")
        gr = ms.abi.MsBdqnGrads(*[L.ptr(g[k]) for k in lr.BDQN_KEYS], L.ptr(loss))
        L.check(L.lib.ms_bdqn_update(ct.byref(qp), ct.byref(tp), ct.byref(bt), ct.c_float(cfg["gamma"]),
                                     ct.c_float(cfg["clip"]), L.ptr(ws), nb, ct.byref(gr), L.stream_ptr()))
        torch.cuda.synchronize()
        out.append((loss.cpu().numpy(), {k: v.cpu().numpy() for k, v in g.items()}))
    assert _guard_intact(ws, nb)
    return out


def _check_bdqn(ms, name, c):
    cfg, ref = c["cfg"], c["ref"]
    (l1, g1), (l2, g2) = _bdqn_update(ms, c)
    assert np.array_equal(l1.view(np.int32), l2.view(np.int32))
    for k in lr.BDQN_KEYS:
        assert not np.isnan(g1[k]).any(), k  # fully overwritten
        assert np.array_equal(g1[k].view(np.int32), g2[k].view(np.int32)), k
    l32, g32 = lr.bdqn_update_torch(c["q"], c["t"], c["xs"], c["xn"], c["actions"], c["rewards"], c["masks"],
                                    cfg["gamma"], cfg["clip"], dtype=torch.float32)
    worst = _compare("bdqn|%s|loss" % name, l1[0], ref["loss"], l32, R_BDQN)
    for k in lr.BDQN_KEYS:
        worst = max(worst, _compare("bdqn|%s|%s" % (name, k), g1[k], ref["grads"][k], g32[k], R_BDQN))
    print("LRN|bdqn|%s|worst %.3f" % (name, worst))
    return float(l1[0])


@pytest.mark.parametrize("name", list(lr.BDQN_CASES))
def test_bdqn_update_matches_float64(ms, name):
    _check_bdqn(ms, name, lr.bdqn_case(name))


def test_bdqn_update_exact_ties_take_the_first_index(ms):
    """Duplicated advantage rows in the online net (bit-equal q values in the kernel), one pair in two different
    64-lane strides of the argmax and one within a stride; the target differs by 100 between the two indices, so
    the loss shows which was taken."""
    c = lr.bdqn_tie_case()
    loss = _check_bdqn(ms, "tie", c)
    assert abs(loss - c["ref"]["loss"]) < 1e-3 * abs(loss - c["ref_last"]["loss"])


def test_bdqn_update_refuses_bad_shapes(ms):
    """ac_dim = 33, batch = 129 and ld < obs return MS_EINVAL before any launch (the outputs keep their NaN)."""
    L = _lib(ms)
    obs, n = 70, 4
    rng = np.random.default_rng(5)
    for ac, B, ld in ((33, 128, obs), (3, 129, obs), (3, 128, obs - 1)):
        net = {k: _dev(v) for k, v in lr.bdqn_net(rng, obs, ac, n).items()}
        p = _bdqn_params(ms, net, obs, ac, n)
        xs = torch.zeros((130, obs), dtype=torch.int8, device="cuda")
        acts = torch.zeros((130, ac), dtype=torch.int8, device="cuda")
        rew = torch.zeros(130, dtype=torch.float32, device="cuda")
        ws = torch.zeros(1 << 20, dtype=torch.float32, device="cuda")
        g = {k: torch.full_like(net[k], float("nan")) for k in lr.BDQN_KEYS}
        loss = torch.full((1,), float("nan"), dtype=torch.float32, device="cuda")
        bt = ms.abi.MsBdqnBatch(L.ptr(xs), L.ptr(xs), ld, L.ptr(acts), ac, L.ptr(rew), L.ptr(rew), B)
        gr = ms.abi.MsBdqnGrads(*[L.ptr(g[k]) for k in lr.BDQN_KEYS], L.ptr(loss))
        rc = L.lib.ms_bdqn_update(ct.byref(p), ct.byref(p), ct.byref(bt), ct.c_float(0.99), ct.c_float(1.0), L.ptr(ws),
                                  ws.numel() * 4, ct.byref(gr), L.stream_ptr())
        torch.cuda.synchronize()
        assert rc == EINVAL, (ac, B, ld, rc)
        assert bool(torch.isnan(loss).all()) and all(bool(torch.isnan(v).all()) for v in g.values())


# ---------------------------------------------------------------------------------------------------- DQN

def _qnet_params(ms, net, D, A, G):
    ptr = _lib(ms).ptr
    return ms.abi.MsQnetParams(*[ptr(net[k]) for k in lr.DQN_KEYS], D, lr.QH, A, G)


def _dqn_grad(ms, c, calls=2):
    L = _lib(ms)
    G, D, A = c["G"], c["D"], c["A"]
    pol = {k: _dev(v) for k, v in c["pol"].items()}
    tgt = {k: _dev(v) for k, v in c["tgt"].items()}
    pp, tp = _qnet_params(ms, pol, D, A, G), _qnet_params(ms, tgt, D, A, G)
    st, nx, acts, rew, smp = (_dev(c[k]) for k in ("states", "next_states", "actions", "rewards", "samples"))
    rows = c["upg"] * c["E"] * c["B"]
    need = int(L.lib.ms_dqn_workspace_bytes(ct.byref(pp), rows))
    assert need == 4 * G * ((rows + 255) // 256) * (lr.QH * D + lr.QH + A * lr.QH + A + 1)
    ws = _workspace(need)
    b = ms.abi.MsDqnBatch(L.ptr(st), L.ptr(nx), L.ptr(acts), L.ptr(rew), L.ptr(smp), c["stride"], G * c["upg"],
                          c["upg"], c["cap"], c["B"], c["E"], ct.c_float(c["gamma"]))
    out = []
    for _ in range(calls):
        g = {k: torch.full_like(pol[k], float("nan")) for k in lr.DQN_KEYS}
        loss = torch.full((G,), float("nan"), dtype=torch.float32, device="cuda")
        gr = ms.abi.MsQnetGrads(*[L.ptr(g[k]) for k in lr.DQN_KEYS], L.ptr(loss))
        L.check(L.lib.ms_dqn_grad(ct.byref(pp), ct.byref(tp), ct.byref(b), ct.c_float(c["clip"]), L.ptr(ws), need,
                                  ct.byref(gr), L.stream_ptr()))
        torch.cuda.synchronize()
        out.append((loss.cpu().numpy(), {k: v.cpu().numpy() for k, v in g.items()}))
    assert _guard_intact(ws, need)
    return out


@pytest.mark.parametrize("name", list(lr.DQN_GRAD_CASES))
def test_dqn_grad_matches_float64(ms, name):
    c = lr.dqn_grad_case(name)
    (l1, g1), (l2, g2) = _dqn_grad(ms, c)
    assert np.array_equal(l1.view(np.int32), l2.view(np.int32))
    for k in lr.DQN_KEYS:
        assert not np.isnan(g1[k]).any(), k
        assert np.array_equal(g1[k].view(np.int32), g2[k].view(np.int32)), k
    t32 = lr.dqn_grad_torch(c["pol"], c["tgt"], c["states"], c["next_states"], c["actions"], c["rewards"],
                            c["samples"], c["D"], c["upg"], c["gamma"], c["clip"], dtype=torch.float32)
    worst = 0.0
    for g in range(c["G"]):
        ref = c["ref"][g]
        worst = max(worst, _compare("dqn|%s|g%d|loss" % (name, g), l1[g], ref["loss"], t32[g][0], R_DQN))
        for k in lr.DQN_KEYS:
            worst = max(worst, _compare("dqn|%s|g%d|%s" % (name, g, k), g1[k][g], ref["grads"][k], t32[g][1][k], R_DQN))
    print("LRN|dqn|%s|lds %d|worst %.3f" % (name, lr.dqn_grad_lds(c["D"], c["A"]), worst))


def _dqn_act(ms, c, uniforms, seed=0, offset=0, offset_dev=None):
    L = _lib(ms)
    net = {k: _dev(v) for k, v in c["net"].items()}
    p = _qnet_params(ms, net, c["D"], c["A"], c["G"])
    obs = _dev(c["obs"])
    E, U = c["E"], c["U"]
    action = torch.full((E, U), -1, dtype=torch.int8, device="cuda")
    greedy = torch.full((E, U), -1, dtype=torch.int8, device="cuda")
    uni = None if uniforms is None else _dev(uniforms)
    L.check(L.lib.ms_dqn_act(ct.byref(p), L.ptr(obs), c["stride"], E, U, c["upg"], ct.c_double(lr.ACT_EPS), L.ptr(uni),
                             ct.c_uint64(seed), ct.c_uint64(offset), L.ptr(offset_dev), L.ptr(action), L.ptr(greedy),
                             L.stream_ptr()))
    torch.cuda.synchronize()
    return action.cpu().numpy().astype(np.int64), greedy.cpu().numpy().astype(np.int64)


@pytest.mark.parametrize("name", list(lr.DQN_ACT_CASES))
def test_dqn_act_given_uniforms(ms, name):
    """The greedy action where the float64 gap is clear, and the epsilon rule on given uniforms with its edges in
    the first four rows (u1 == eps explores, one ulp above does not, u2 = 1 - 2^-53 and u2 = 0)."""
    c = lr.dqn_act_case(name)
    action, greedy = _dqn_act(ms, c, c["uniforms"])
    clear = c["clear"]
    assert np.array_equal(greedy[clear], c["greedy"][clear])
    assert (greedy >= 0).all() and (greedy < c["A"]).all()
    ex = c["explore"]
    assert np.array_equal(action[ex], c["action"][ex])
    assert np.array_equal(action[~ex], greedy[~ex])
    assert np.array_equal(action.reshape(-1)[:4], c["action"].reshape(-1)[:4])
    a2, g2 = _dqn_act(ms, c, c["uniforms"])
    assert np.array_equal(a2, action) and np.array_equal(g2, greedy)


@pytest.mark.parametrize("name", ["D5", "A1", "corner"])
def test_dqn_act_philox_path(ms, name):
    """No uniforms: k_dqn_act draws from Philox4x32-10 with counter (row, offset + *offset_dev) and key seed;
    offset and offset_dev both nonzero with high words set, rows in a second block (E = 257)."""
    c = lr.dqn_act_case(name)
    seed, offset, odev = 0x9E3779B97F4A7C15, (3 << 32) + 11, (1 << 33) + 5
    od = torch.tensor([odev], dtype=torch.int64, device="cuda")
    action, greedy = _dqn_act(ms, c, None, seed=seed, offset=offset, offset_dev=od)
    E, U, A = c["E"], c["U"], c["A"]
    assert E > 256  # a second block of 256 replicas
    u1, u2 = lr.dqn_act_uniforms(E * U, seed, offset + odev)
    want, ex = lr.dqn_act_rule(c["greedy"].reshape(-1), u1, u2, lr.ACT_EPS, A)
    want, ex = want.reshape(E, U), ex.reshape(E, U)
    assert 0.3 < ex.mean() < 0.5  # eps 0.4
    assert np.array_equal(action[ex], want[ex])
    assert np.array_equal(action[~ex], greedy[~ex])
    assert np.array_equal(greedy[c["clear"]], c["greedy"][c["clear"]])
    # another offset draws other numbers
    a3, _ = _dqn_act(ms, c, None, seed=seed, offset=offset + 1, offset_dev=od)
    assert np.array_equal(a3, action) == (A == 1)
