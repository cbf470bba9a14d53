"""Float64 reference of ms_ppo_grad (k_ppo_grad + k_ppo_reduce), its case tables, and plain restatements of the
launcher's kernel choice and of the work split. TEST INFRASTRUCTURE ONLY, CPU only.

The loss is the one of include/marlsched.h (ms_ppo_grad's comment) and oracle/ppo_ref.py, per group:

    mean(-min(ratio * adv, clamp(ratio, 1 - eps, 1 + eps) * adv)) + 0.5 * mean((V - G)^2) - 0.01 * mean(entropy)

with adv = G - V.detach() and the chain nn.Softmax -> Categorical(probs) -> clamped logs written out (probs
renormalised, logits = log(clamp(p, 2^-23, 1 - 2^-23)), entropy = -sum(logits * p)). The clamp edge is float32's eps
in every precision: that is the function the kernel and torch's float32 Categorical compute, and a float64
Categorical would clamp at 2^-52, another function.

A case's inputs are the device buffers as the kernel addresses them ([R][U][stride] rows with unit_of_group,
unit-major rows with unit_stride, returns_ld, compact rows with core_owner / n_cores / common_row): `gather` restates
the addressing, and the reference runs on what it gathers, so garbage in everything the kernel must not read is part
of the inputs here too.

Discontinuities come from the float64 values alone: a row whose ratio is within KINK (relative) of 1 - eps or 1 + eps,
whose |adv| < KINK, or (every case, it only bites with a scaled last layer) which has an action with p or 1 - p within
a factor 4 of the clamp edge, is drawn again from default_rng((seed, g, r, sweep)), row by row. Old log-probs are the
reference's own log-prob plus N(0, 0.15) noise (variance 0.15, sigma 0.387: at sigma 0.15 only 9 % of the rows would
be clipped away, short of the 10 % every case must have), so the ratios straddle both clip edges.
"""
from __future__ import annotations

import functools

import numpy as np
import torch

KEYS = ("w1", "b1", "w2", "b2", "w3", "b3", "cw1", "cb1", "cw2", "cb2", "cw3", "cb3")
ACTOR_KEYS, CRITIC_KEYS = KEYS[:6], KEYS[6:]
EPS32 = 2.0 ** -24       # half an ulp of 1.0f: the floor of the parity rule
EPS_P = 2.0 ** -23       # Categorical's clamp edge on float32 probabilities
EPS_CLIP = 0.2
KINK = 1e-4
NOISE_SIGMA = 0.15 ** 0.5
MAX_SWEEPS = 5
SENTINEL_ROWS = 3        # rows after row R - 1 in every input
H = 16

# ---------------------------------------------------------------------------- launcher and split, restated

INSTANTIATIONS = tuple([(q, t, False) for t in (1, 2) for q in (1, 2, 4, 8, 16)] +
                       [(q, 4, False) for q in (2, 4, 8, 16)] + [(q, 8, False) for q in (4, 8, 16)] +
                       [(4, 2, True), (8, 4, True)])


def dispatch(D, A, keyed=False):
    """launch_ppo_grad's choice (NQ, NT, X1) for in_dim D and A actions, None where it has no kernel. keyed: the
    keyed passes take the call (row_keys 0, stride 4, no common row, D <= 4, A <= 32)."""
    nq, nt = D // 16 + 1, (A + 15) // 16
    if A % 16 == 1 and not keyed:
        if nt == 2 and 2 < nq <= 4:
            return (4, 2, True)
        if nt == 4 and 4 < nq <= 8:
            return (8, 4, True)
    if nt <= 1:
        rows = ((1, 1), (2, 1), (4, 1), (8, 1), (16, 1))
    elif nt <= 2:
        rows = ((1, 2), (2, 2), (4, 2), (8, 2), (16, 2))
    elif nt <= 4:
        rows = ((2, 4), (4, 4), (8, 4), (16, 4))
    else:
        rows = ((4, 8), (8, 8), (16, 8))
    for q, t in rows:
        if nq <= q and nt <= t:
            return (q, t, False)
    return None


GRAD_WAVES = 8192


def split(R, G):
    """ppo_split: (chunk_tiles, n_chunks) of R rows and G groups: tiles of 16 rows, chunks of whole tile pairs and
    at least 8 tiles, a whole number of 4-chunk blocks."""
    tiles = (R + 15) // 16
    ct = max((tiles * G + GRAD_WAVES - 1) // GRAD_WAVES, 8)
    ct = (ct + 1) & ~1
    nc = (tiles + ct - 1) // ct
    return ct, (nc + 3) // 4 * 4


def split_edges(R, G):
    """What of the split a row count exercises: tiles, the rows of the ragged last tile (0: none), whether the
    last chunk in use ends on half a tile pair, chunks that hold rows, blocks per group."""
    ct, nc = split(R, G)
    tiles = (R + 15) // 16
    used = (tiles + ct - 1) // ct
    return dict(tiles=tiles, ragged=R % 16, odd_pair=(tiles - (used - 1) * ct) % 2 == 1, chunks_used=used,
                chunks_idle=nc - used, blocks=nc // 4)


def grad_lds_wpb(NQ, NT, cm_floats=0):
    """GradLds<NQ, NT>::WPB: 4 waves per block when shared + 4 * per-wave floats fit 160 KB of LDS, else 2."""
    S1 = (NQ + 1) // 2
    W1B = 32 * S1 + 8
    XPD = 4 * NQ + 6 if NQ & 1 else 4 * NQ + 2
    shared = 2 * 3 * 16 * W1B // 2 + 2 * 256 + 256 * NT + 16 * 5 + 16 * NT + 4
    wave = 2 * 16 * 36 + (NT + 1) * 16 * 20 + 32 * XPD + cm_floats
    return 4 if shared + 4 * wave <= 40960 else 2


def common_row_floats(NT):
    """GradLds::CMF of the common-row and owner-row modes (512-row segments), and of kMaskRow."""
    return 16 * NT + 4 + 512 + 64 + 2 * 16 * NT, 1024 + 64


KEY_MAX_RANKS = 4096
KEY_FX = 2.0 ** 20
OWN_MIN_GROUPS = 64
OWN_SCAN_ROWS = 1024
COMMON_SEG = 512


def path(spec):
    """The launch path of a case: 'keyed' (which may still fall to the tiles per group), 'own_scan', 'owner',
    'common' or 'plain'."""
    D, A = spec["D"], spec["A"]
    nq, nt = D // 16 + 1, (A + 15) // 16
    has_common = spec["common"] is not None or spec["compact"] is not None
    if spec["row_keys"] == 0 and D <= 4 and A <= 32 and spec["stride"] == 4 and not has_common:
        return "keyed"
    q = dispatch(D, A)[0]
    if has_common and spec["stride"] >= 16 and q <= 8:
        if spec["compact"] is not None:
            return "own_scan" if spec["G"] >= OWN_MIN_GROUPS and D >= 16 else "owner"
        return "common"
    return "plain"


# ------------------------------------------------------------------------------------------- the reference

def _t(a, dtype):
    return torch.as_tensor(np.asarray(a), dtype=dtype)


def _lin(x, w, b):
    return x @ w.transpose(-1, -2) + b.unsqueeze(-2)


def _forward(p, x, act):
    """p the twelve tensors, x [R, D], act [R] int64 of one group, or [G, ...] of all (the groups are independent)
    -> pn [.., R, A], logits, lp [.., R], ent, V."""
    h = torch.tanh(_lin(torch.tanh(_lin(x, p["w1"], p["b1"])), p["w2"], p["b2"]))
    probs = torch.softmax(_lin(h, p["w3"], p["b3"]), dim=-1)    # nn.Softmax
    pn = probs / probs.sum(-1, keepdim=True)                     # Categorical(probs)
    logits = torch.log(pn.clamp(EPS_P, 1.0 - EPS_P))
    lp = logits.gather(-1, act.unsqueeze(-1)).squeeze(-1)
    ent = -(logits * pn).sum(-1)
    c = torch.tanh(_lin(torch.tanh(_lin(x, p["cw1"], p["cb1"])), p["cw2"], p["cb2"]))
    V = _lin(c, p["cw3"], p["cb3"]).squeeze(-1)
    return pn, logits, lp, ent, V


def _params(nets, dtype, grad, g=None):
    return {k: _t(nets[k] if g is None else nets[k][g], dtype).requires_grad_(grad) for k in KEYS}


def _group_params(nets, g, dtype, grad):
    return _params(nets, dtype, grad, g)


def grad_ref(nets, x, act, olp, ret, eps_clip=EPS_CLIP, dtype=torch.float64):
    """Autograd of the loss in `dtype` on the CPU. nets: {key: [G, ...] float32}, x [G, R, D], act [G, R],
    olp, ret [G, R] float32 -> ({key: [G, ...] float64 in torch .grad layout}, loss [G, 3] float64: mean(-min(surr)),
    mean((V - G)^2), mean(entropy)). One pass over all groups: a group's loss reads its own tensors only, so the
    gradient of the sum over the groups is each group's gradient."""
    p = _params(nets, dtype, True)
    og, rg = _t(olp, dtype), _t(ret, dtype)
    _, _, lp, ent, V = _forward(p, _t(x, dtype), _t(act, torch.int64))
    ratio = torch.exp(lp - og)
    adv = rg - V.detach()
    s1 = ratio * adv
    s2 = torch.clamp(ratio, 1 - eps_clip, 1 + eps_clip) * adv
    l_min, l_mse, l_ent = (-torch.min(s1, s2)).mean(-1), ((V - rg) ** 2).mean(-1), ent.mean(-1)
    total = (l_min + 0.5 * l_mse - 0.01 * l_ent).sum()
    gs = torch.autograd.grad(total, [p[k] for k in KEYS])
    grads = {k: v.double().numpy() for k, v in zip(KEYS, gs)}
    return grads, torch.stack([l_min, l_mse, l_ent], dim=-1).detach().double().numpy()


def _forward_values(p, x, act):
    """lp, V, ent and edge (the smallest factor between any action's p or 1 - p and the clamp edge; 1 = on it) of
    every row, float64."""
    with torch.no_grad():
        pn, _, lp, ent, V = _forward(p, _t(x, torch.float64), _t(act, torch.int64))
        both = torch.cat([pn, 1.0 - pn], dim=-1).clamp_min(1e-300)
        edge = torch.exp(torch.abs(torch.log(both / EPS_P)).min(dim=-1).values.clamp_max(700.0))
    return dict(lp=lp.numpy(), V=V.numpy(), ent=ent.numpy(), edge=edge.numpy())


def _with_olp(v, olp, ret):
    v = dict(v)
    v["ratio"] = np.exp(v["lp"] - olp.astype(np.float64))
    v["adv"] = ret.astype(np.float64) - v["V"]
    return v


def row_values(nets, x, act, olp, ret):
    """The float64 per-row values the kink rules and the tests read: lp, V, ent, edge, ratio, adv, each [G, R]."""
    return _with_olp(_forward_values(_params(nets, torch.float64, False), x, act), olp, ret)


def kink_rows(v, eps_clip=EPS_CLIP):
    """[G, R] bool: the rows the module's docstring sends back to the draw."""
    near = (np.abs(v["ratio"] / (1 - eps_clip) - 1) < KINK) | (np.abs(v["ratio"] / (1 + eps_clip) - 1) < KINK)
    return near | (np.abs(v["adv"]) < KINK) | (v["edge"] <= 4.0)


def branch_shares(v, eps_clip=EPS_CLIP):
    """Shares of the rows (all groups) on the unclipped branch (ratio inside the clip range), outside it with the
    minimum still taking ratio * adv (the gradient flows), and clipped away (no surrogate gradient)."""
    lo, hi = v["ratio"] < 1 - eps_clip, v["ratio"] > 1 + eps_clip
    away = (hi & (v["adv"] > 0)) | (lo & (v["adv"] < 0))
    inside = ~lo & ~hi
    return dict(inside=float(inside.mean()), outside_live=float((~inside & ~away).mean()), away=float(away.mean()))


# ----------------------------------------------------------------------------------- buffers and addressing

def align4(x):
    return (x + 3) // 4 * 4


def common_row(O, stride):
    """The acceptor row of a core the agent does not own (Agent.py:167-212), zero pad bytes."""
    D = 3 + 2 * O
    return np.array([0, -1, -1] + [-2] * (2 * O) + [0] * (stride - D), dtype=np.int8)


def _row_index(spec, buf, g):
    """Flat index of row (r, unit_of_group[g]) in actions / old_logprobs (and, times stride, in plain states)."""
    R, U, u = spec["R"], spec["U"], int(buf["uog"][g])
    r = np.arange(R)
    return u * buf["unit_stride"] + r if buf["unit_stride"] else r * U + u


def gather_group(spec, buf, g):
    """Group g's x [R, D] int8, act [R], olp, ret [R] float32 as ms_ppo_grad addresses them."""
    R, D, stride = spec["R"], spec["D"], spec["stride"]
    r = np.arange(R)
    i = _row_index(spec, buf, g)
    act = buf["actions"].reshape(-1)[i].astype(np.int64)
    olp = buf["olp"].reshape(-1)[i]
    ret = buf["returns"].reshape(-1)[r * buf["ld"] + g]
    if spec["compact"] is not None:
        # unit a * C + c reads core row (r, c) if core_owner[r][c] == a + 1, else the common row
        C = spec["compact"][1]
        a, c = divmod(int(buf["uog"][g]), C)
        rows = buf["states"].reshape(-1, C, stride)
        own = buf["owner"].reshape(-1, C)[r, c] == a + 1
        x = np.where(own[:, None], rows[r, c, :D], buf["common_row"][None, :D])
    else:
        x = buf["states"].reshape(-1, stride)[i, :D]
    return x, act, olp, ret


def gather(spec, buf):
    """x [G, R, D] int8, act [G, R], olp, ret [G, R] float32 over the groups."""
    per = [gather_group(spec, buf, g) for g in range(spec["G"])]
    return tuple(np.stack([p[k] for p in per]) for k in range(4))


def _junk(rng, shape):
    return rng.choice(np.array([-127, 127], dtype=np.int8), shape)


def _draw_states(spec, rng, n):
    """n rows [n, stride] of a unit some group selects: bytes < D drawn, pad bytes zero or garbage."""
    D, stride = spec["D"], spec["stride"]
    lo, hi = spec["bytes"]
    rows = _junk(rng, (n, stride)) if spec["pad_garbage"] else np.zeros((n, stride), dtype=np.int8)
    rows[:, :D] = rng.integers(lo, hi, (n, D)).astype(np.int8)
    return rows


def _one_off(rng, crow, D, n):
    """n copies of the common row with one byte changed: the first, the last (D - 1), or any."""
    rows = np.repeat(crow[None], n, axis=0)
    pos = np.where(np.arange(n) % 3 == 0, 0, np.where(np.arange(n) % 3 == 1, D - 1, rng.integers(0, D, n)))
    rows[np.arange(n), pos] += np.where(rng.random(n) < 0.5, 1, -1).astype(np.int8)
    return rows


def _mixed_rows(spec, rng, n, crow):
    """n rows of a common-row case: `common` of them the common row, a tenth of the rest one byte off it."""
    rows = _draw_states(spec, rng, n)
    pick = rng.random(n)
    share = spec["common"]
    is_c = pick < share
    off = ~is_c & (rng.random(n) < 0.1)
    rows[is_c] = crow
    rows[off] = _one_off(rng, crow, spec["D"], int(off.sum()))
    return rows


def _key_pool(spec, rng):
    D, n = spec["D"], spec["distinct"]
    lo, hi = spec["bytes"]
    seen = {}
    while len(seen) < n:
        row = rng.integers(lo, hi, D).astype(np.int8)
        seen.setdefault(row.tobytes(), row)
    pool = np.zeros((n, 4), dtype=np.int8)
    pool[:, :D] = np.stack(list(seen.values()))
    return pool


def build_inputs(spec, rng):
    """The device buffers of a case as numpy arrays: everything no group may read holds garbage (+-127 bytes,
    out-of-range action bytes, NaN), SENTINEL_ROWS rows after row R - 1 included. old_logprobs of the rows in use
    are set by case()."""
    G, U, R, D, stride, A = (spec[k] for k in ("G", "U", "R", "D", "stride", "A"))
    RP = R + SENTINEL_ROWS
    us = R + spec["um"] if spec["um"] is not None else 0
    perm = rng.permutation(U)[:G]
    if np.array_equal(perm, np.arange(G)):
        perm = perm[::-1].copy() if G > 1 else np.array([U - 1])
    buf = dict(unit_stride=us, ld=G + spec["ld_extra"], common_row=None, owner=None)
    n_rows = U * us if us else RP * U
    bad_act = np.array([-128, -3], dtype=np.int8)
    buf["actions"] = rng.choice(bad_act, n_rows)
    buf["olp"] = np.full(n_rows, np.nan, dtype=np.float32)
    buf["returns"] = np.full((RP, buf["ld"]), np.nan, dtype=np.float32)
    buf["returns"][:R, :G] = rng.standard_normal((R, G)).astype(np.float32)
    crow = None
    if spec["common"] is not None or spec["compact"] is not None:
        crow = common_row((D - 3) // 2, stride)
        buf["common_row"] = crow
    if spec["compact"] is not None:
        N, C = spec["compact"]
        assert U == N * C
        if G < U:  # selected units on distinct cores: each core row has one reader
            cores = rng.permutation(C)[:G]
            perm = rng.integers(0, N, G) * C + cores
        states = _junk(rng, (RP, C, stride))
        owner = rng.integers(0, N + 1, (RP, C)).astype(np.int8)
        owner[R:] = 127
        for g in range(G):
            a, c = divmod(int(perm[g]), C)
            if G < U:  # the share of common rows is the case's: own the core row or hand it to another owner
                own = rng.random(R) >= spec["common"]
                other = rng.integers(0, N, R)
                owner[:R, c] = np.where(own, a + 1, np.where(other >= a + 1, other + 1, other)).astype(np.int8)
            own = owner[:R, c] == a + 1
            n = int(own.sum())
            rows = _draw_states(spec, rng, n)
            kind = rng.random(n)
            rows[kind < 0.05] = crow  # an owned row that equals the common row byte for byte
            off = (kind >= 0.05) & (kind < 0.15)
            rows[off] = _one_off(rng, crow, D, int(off.sum()))
            states[:R, c][own] = rows
        buf["states"], buf["owner"] = states, owner
    else:
        states = _junk(rng, (n_rows, stride))
        pool = _key_pool(spec, rng) if spec["distinct"] else None
        for g in range(G):
            u = int(perm[g])
            i = u * us + np.arange(R) if us else np.arange(R) * U + u
            if pool is not None:
                idx = rng.integers(0, len(pool), R)
                idx[:min(R, len(pool))] = rng.permutation(len(pool))[:min(R, len(pool))]
                states[i] = pool[idx]
            elif crow is not None:
                states[i] = _mixed_rows(spec, rng, R, crow)
            else:
                states[i] = _draw_states(spec, rng, R)
        if spec["outlier"]:
            u = int(perm[0])
            states[(u * us + R // 2) if us else (R // 2) * U + u, 0] = 100
        buf["states"] = states
    buf["uog"] = perm.astype(np.int32)
    for g in range(G):
        buf["actions"][_row_index(spec, buf, g)] = rng.integers(0, A, R).astype(np.int8)
    return buf


# --------------------------------------------------------------------------------------------- case tables

BASE = dict(G=2, U=3, T=None, E=None, ld_extra=2, um=None, common=None, compact=None, row_keys=-1, distinct=None,
            outlier=False, bytes=(-5, 13), scale3=1.0, pad_garbage=False, seed=0)
_RS = ((7, 19), (11, 13), (3, 67), (1, 211), (5, 59), (17, 37), (131, 1), (23, 11), (9, 31))  # 128 < T*E <= 640


def _table_a():
    t = {}
    n = [0]

    def add(name, D, stride, A):
        T, E = _RS[n[0] % len(_RS)]
        t[name] = dict(BASE, D=D, stride=stride, A=A, T=T, E=E, G=2 + n[0] % 2, U=3 + n[0] % 3, pad_garbage=True,
                       seed=100 + n[0])
        n[0] += 1

    # one per instantiation
    for D in (9, 19, 51, 99, 195):
        for A in (9, 25):
            add("inst-D%d-A%d" % (D, A), D, align4(D + (13 if A == 25 else 0)), A)
    for D, A in ((19, 49), (51, 49), (99, 41), (195, 49)):
        add("inst-D%d-A%d" % (D, A), D, align4(D), A)
    for D in (51, 99, 195):
        add("inst-D%d-A97" % D, D, align4(D + 13), 97)
    add("inst-x1-D40-A17", 40, 40, 17)
    add("inst-x1-D99-A49", 99, 100, 49)
    # input edges at A = 13: every D mod 4 (the position of the ones byte), stride == D and whole pad dwords
    for D in (1, 2, 15, 16, 18, 31, 32, 63, 64, 127, 128, 255):
        add("D%d" % D, D, align4(D), 13)
    for D in (1, 15, 16, 30, 32, 63, 128):
        add("D%d-pad" % D, D, align4(D + 13), 13)
    for A in (1, 2, 15, 16, 17, 32, 33, 48, 49, 64, 65, 127, 128):
        add("A%d" % A, 19, 20 if A % 2 else 32, A)
    add("nox1-D195-A17", 195, 196, 17)   # (A17 above is the D = 19 one)
    add("nox1-D40-A49", 40, 40, 49)
    add("corner", 255, 256, 128)
    return t


B_ROWS = (1, 15, 16, 17, 31, 32, 33, 127, 128, 129, 511, 512, 513, 1025)
_B_BETWEEN = {15: (3, 5), 16: (4, 4), 32: (2, 16), 33: (3, 11), 128: (8, 16), 129: (3, 43), 511: (7, 73),
              512: (16, 32), 513: (27, 19), 1025: (25, 41)}


def _table_b():
    t = {}
    n = 0
    for tag, D, stride, A in (("s", 19, 20, 9), ("c", 255, 256, 128)):
        for R in B_ROWS:
            shapes = [(R, 1), (1, R)] + ([_B_BETWEEN[R]] if R in _B_BETWEEN else [])
            for T, E in shapes if R > 1 else [(1, 1)]:
                t["%s-R%d-%dx%d" % (tag, R, T, E)] = dict(BASE, D=D, stride=stride, A=A, T=T, E=E, G=3, U=4,
                                                          seed=300 + n)
                n += 1
        for R, um in ((33, 0), (33, 7), (513, 0), (513, 7), (1, 7)):
            t["%s-R%d-um%d" % (tag, R, um)] = dict(BASE, D=D, stride=stride, A=A, T=1, E=R, G=3, U=4, um=um,
                                                   seed=400 + n)
            n += 1
    # one-row cases: the first seed with one row inside the clip range and one clipped away over the groups
    t["s-R1-1x1"]["seed"] = 304
    t["c-R1-1x1"]["seed"] = 341
    t["s-R1-um7"]["seed"] = 450
    t["c-R1-um7"]["seed"] = 478
    return t


def _table_c():
    t = {}
    n = 0
    for O in (6, 12, 24, 48):
        D, A = 3 + 2 * O, O + 1
        for R, shares in ((513, (0.0, 0.5, 1.0)), (33, (0.5,)), (1500, (0.5,))):
            T, E = {513: (27, 19), 33: (3, 11), 1500: (3, 500)}[R]
            for share in shares:
                for compact in (None, (3, 4)):
                    name = "O%d-R%d-c%g-%s" % (O, R, share, "own" if compact else "row")
                    t[name] = dict(BASE, D=D, stride=align4(D), A=A, T=T, E=E, G=3, U=12 if compact else 4,
                                   common=share, compact=compact, seed=500 + n)
                    n += 1
    for R, (T, E) in ((33, (3, 11)), (4095, (5, 819)), (4097, (17, 241))):
        t["many-R%d" % R] = dict(BASE, D=51, stride=52, A=25, T=T, E=E, G=64, U=64, common=8.0 / 9, compact=(8, 8),
                                 seed=600 + n)
        n += 1
    return t


SMALL_STRIDE = dict(BASE, D=11, stride=12, A=5, T=7, E=47, G=3, U=4, common=0.5, seed=650)  # O = 4: the plain path


def _table_d():
    t = {}
    n = 0
    for D, A in ((1, 13), (2, 20), (3, 13), (4, 20)):
        for R, distinct in ((1, 1), (255, 3), (256, 300), (257, 1), (2000, 300), (2000, 3)):
            distinct = min(distinct, R, 18 ** D)
            T, E = {1: (1, 1), 255: (5, 51), 256: (16, 16), 257: (1, 257), 2000: (8, 250)}[R]
            for keys in (0, -1):
                t["D%d-A%d-R%d-k%d-%s" % (D, A, R, distinct, "keyed" if keys == 0 else "tiles")] = dict(
                    BASE, D=D, stride=4, A=A, T=T, E=E, G=3, U=4, row_keys=keys, distinct=distinct, seed=700 + n)
            n += 1
    # more distinct rows than ranks, and a byte outside the dense index: the keyed passes hand both to the tiles
    t["ranks-over"] = dict(BASE, D=4, stride=4, A=20, T=10, E=600, G=2, U=3, row_keys=0, bytes=(-8, 24), seed=790)
    t["byte-outside"] = dict(BASE, D=3, stride=4, A=13, T=5, E=51, G=3, U=4, row_keys=0, distinct=3, outlier=True,
                             seed=791)
    t["D1-A13-R1-k1-keyed"]["seed"] = t["D1-A13-R1-k1-tiles"]["seed"] = 702
    t["D2-A20-R1-k1-keyed"]["seed"] = t["D2-A20-R1-k1-tiles"]["seed"] = 708
    t["D3-A13-R1-k1-keyed"]["seed"] = t["D3-A13-R1-k1-tiles"]["seed"] = 712
    t["D4-A20-R1-k1-keyed"]["seed"] = t["D4-A20-R1-k1-tiles"]["seed"] = 720
    return t


def _table_e():
    t = {}
    for n, (D, stride, A) in enumerate(((19, 20, 25), (51, 52, 49), (34, 36, 17), (9, 12, 9))):
        t["sat-D%d-A%d" % (D, A)] = dict(BASE, D=D, stride=stride, A=A, T=9, E=37, G=2, U=3, scale3=40.0, seed=800 + n)
    return t


TABLES = dict(A=_table_a(), B=_table_b(), C=_table_c(), D=_table_d(), E=_table_e())
CASES = {"%s/%s" % (fam, name): spec for fam, t in TABLES.items() for name, spec in t.items()}
CASES["C/O4-plain"] = SMALL_STRIDE


def _linear_init(rng, out_f, in_f):
    k = 1.0 / np.sqrt(in_f)
    return (rng.uniform(-k, k, (out_f, in_f)).astype(np.float32), rng.uniform(-k, k, (out_f,)).astype(np.float32))


def draw_nets(rng, G, D, A, scale3=1.0):
    """G actor-critics [D -> 16 -> 16 -> A], [D -> 16 -> 16 -> 1], nn.Linear's init ranges, stacked over groups."""
    per = []
    for _ in range(G):
        n = {}
        for pre, out in (("", A), ("c", 1)):
            n[pre + "w1"], n[pre + "b1"] = _linear_init(rng, H, D)
            n[pre + "w2"], n[pre + "b2"] = _linear_init(rng, H, H)
            n[pre + "w3"], n[pre + "b3"] = _linear_init(rng, out, H)
        n["w3"], n["b3"] = (n["w3"] * np.float32(scale3)), (n["b3"] * np.float32(scale3))
        per.append(n)
    return {k: np.stack([n[k] for n in per]) for k in KEYS}


ROW_DRAWS = 64  # candidates of one row in one sweep


def _redraw_rows(spec, nets, buf, noise, g, rows, sweep):
    """Draw the rows `rows` of group g again: action, return, old log-prob noise, and the state bytes where the row
    is the group's own to change (plain rows outside the keyed pools). Row r takes the first of ROW_DRAWS candidates
    from default_rng((seed, g, r, sweep)) that is clear by its own float64 values (a row's rules read that row
    alone); if none is, the last, and the next sweep draws again."""
    own_state = spec["common"] is None and spec["compact"] is None and not spec["distinct"]
    idx = _row_index(spec, buf, g)
    x_now = gather_group(spec, buf, g)[0]
    n, K, D = len(rows), ROW_DRAWS, spec["D"]
    st = np.zeros((n, K, spec["stride"]), dtype=np.int8)
    xs = np.zeros((n, K, D), dtype=np.int8)
    act = np.zeros((n, K), dtype=np.int64)
    ret, nz = np.zeros((n, K), dtype=np.float32), np.zeros((n, K))
    for i, r in enumerate(rows):
        rr = np.random.default_rng((spec["seed"], g, int(r), sweep))
        for k in range(K):
            act[i, k] = rr.integers(0, spec["A"])
            ret[i, k] = np.float32(rr.standard_normal())
            nz[i, k] = rr.standard_normal() * NOISE_SIGMA
            if own_state:
                st[i, k] = _draw_states(spec, rr, 1)[0]
        xs[i] = st[i, :, :D] if own_state else x_now[r]
    flat = lambda a: a.reshape((n * K,) + a.shape[2:])
    v = _forward_values(_params(nets, torch.float64, False, g), flat(xs), flat(act))
    v = _with_olp(v, (v["lp"] + flat(nz)).astype(np.float32), flat(ret))
    clear = ~kink_rows(v).reshape(n, K)
    pick = np.where(clear.any(axis=1), clear.argmax(axis=1), K - 1)
    for i, r in enumerate(rows):
        k, j = int(pick[i]), int(idx[r])
        buf["actions"][j], buf["returns"][r, g], noise[g, r] = act[i, k], ret[i, k], nz[i, k]
        if own_state:
            buf["states"][j] = st[i, k]


def _normalise(spec):
    spec = dict(spec)
    spec["R"] = spec["T"] * spec["E"]
    return spec


def _inputs_key(spec):
    """Two cases that differ in row_keys alone share their inputs and their reference."""
    return tuple(sorted((k, v) for k, v in spec.items() if k != "row_keys"))


@functools.lru_cache(maxsize=None)
def _case(key):
    spec = _normalise(dict(key))
    G, R, D, A = spec["G"], spec["R"], spec["D"], spec["A"]
    rng = np.random.default_rng((spec["seed"], D, A, R, G))
    nets = draw_nets(rng, G, D, A, spec["scale3"])
    buf = build_inputs(spec, rng)
    noise = rng.standard_normal((G, R)) * NOISE_SIGMA
    sweeps = 0
    while True:
        x, act, _, ret = gather(spec, buf)
        v = _forward_values(_params(nets, torch.float64, False), x, act)
        olp = (v["lp"] + noise).astype(np.float32)
        v = _with_olp(v, olp, ret)
        bad = kink_rows(v)
        if not bad.any():
            break
        sweeps += 1
        if sweeps > 4 * MAX_SWEEPS:
            raise RuntimeError("rows of %r stay on a discontinuity" % (spec,))
        for g in np.nonzero(bad.any(axis=1))[0]:
            _redraw_rows(spec, nets, buf, noise, int(g), np.nonzero(bad[g])[0], sweeps)
    for g in range(G):
        buf["olp"][_row_index(spec, buf, g)] = olp[g]
    x, act, olp, ret = gather(spec, buf)
    xf = x.astype(np.float64)
    g64, l64 = grad_ref(nets, xf, act, olp, ret, dtype=torch.float64)
    g32, l32 = grad_ref(nets, xf, act, olp, ret, dtype=torch.float32)
    return dict(nets=nets, buf=buf, x=x, act=act, olp=olp, ret=ret, rows=v, sweeps=sweeps,
                shares=branch_shares(v), ref=(g64, l64), f32=(g32, l32))


def case(name):
    """dict(spec, nets, buf, x, act, olp, ret (what the kernel reads, gathered), rows (float64 per-row values),
    sweeps, shares, ref = (grads, loss) in float64, f32 = the same from float32 CPU autograd). Deterministic in the
    case's committed seed. Treat as read-only: cases are cached, and keyed / tiles pairs share one."""
    spec = _normalise(CASES[name])
    c = dict(_case(_inputs_key(CASES[name])))
    c["spec"] = spec
    return c


# ------------------------------------------------------------------------------ keyed rows: the 2^-20 sums

def keyed_terms(c):
    """Per row, the two terms k_key_scan adds to its distinct row's int64 sums: qd = d min(surr) / d ratio * ratio
    and dv = V - G, from the float64 values."""
    v, e = c["rows"], EPS_CLIP
    ratio, adv = v["ratio"], v["adv"]
    s1, s2 = ratio * adv, np.clip(ratio, 1 - e, 1 + e) * adv
    inr = ((ratio >= 1 - e) & (ratio <= 1 + e)).astype(np.float64)
    dmin = np.where(s1 < s2, adv, np.where(s2 < s1, adv * inr, 0.5 * adv + 0.5 * adv * inr))
    return dmin * ratio, -adv


def keyed_grads(c, qd, dv):
    """The gradient as the keyed passes form it, in float64: every row's derivatives enter through qd and dv only
    (the backward is linear in them): d/dtheta of mean(-qd * lp + dv * V - 0.01 * ent) with qd, dv constants."""
    nets, x, act = c["nets"], c["x"].astype(np.float64), c["act"]
    grads = {k: np.zeros(nets[k].shape, dtype=np.float64) for k in KEYS}
    for g in range(x.shape[0]):
        p = _group_params(nets, g, torch.float64, True)
        _, _, lp, ent, V = _forward(p, _t(x[g], torch.float64), _t(act[g], torch.int64))
        total = (-_t(qd[g], torch.float64) * lp + _t(dv[g], torch.float64) * V - 0.01 * ent).mean()
        for k, t in zip(KEYS, torch.autograd.grad(total, [p[k] for k in KEYS])):
            grads[k][g] = t.numpy()
    return grads


def keyed_allowance(c):
    """{key: [G, ...]} the most the 2^-20 fixed point can move each gradient element: a term is rounded to the
    nearest multiple of 2^-20 (error <= 2^-21, the integer sums are exact), and the gradient is linear in the terms,
    d grad = mean_r(-d qd_r * d lp_r / d theta) (actor) and mean_r(d dv_r * d V_r / d theta) (critic), so
    |d grad| <= 2^-21 * mean_r |d lp_r / d theta|, resp. |d V_r / d theta|, element by element."""
    from torch.func import functional_call, grad, vmap  # noqa: F401

    nets, x, act = c["nets"], c["x"].astype(np.float64), c["act"]
    out = {k: np.zeros(nets[k].shape, dtype=np.float64) for k in KEYS}

    def lp_of(p, xr, ar):
        return _forward(p, xr[None], ar[None])[2][0]

    def v_of(p, xr, ar):
        return _forward(p, xr[None], ar[None])[4][0]

    for g in range(x.shape[0]):
        p = _group_params(nets, g, torch.float64, False)
        xs, as_ = _t(x[g], torch.float64), _t(act[g], torch.int64)
        jl = vmap(grad(lp_of), in_dims=(None, 0, 0))(p, xs, as_)
        jv = vmap(grad(v_of), in_dims=(None, 0, 0))(p, xs, as_)
        for k in ACTOR_KEYS:
            out[k][g] = jl[k].abs().mean(0).numpy() / (2 * KEY_FX)
        for k in CRITIC_KEYS:
            out[k][g] = jv[k].abs().mean(0).numpy() / (2 * KEY_FX)
    return out


def quantise(t):
    """__float2ll_rn(t * 2^20) / 2^20."""
    return np.rint(t * KEY_FX) / KEY_FX
