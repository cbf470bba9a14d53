"""Float64 references of the wide nets' kernels (wide_kernels.hip: ms_wide_act, ms_wide_grad), a plain restatement
of ms_wide_grad's work plan (capi.cpp's wide_plan), and the case tables of tests/test_wide_ref.py (CPU) and
tests/test_wide_parity_gpu.py. TEST INFRASTRUCTURE ONLY, CPU only: nothing here imports a device.

The gradient is that of oracle/ppo_grad_ref.py's loss (its grad_ref is shape-generic and reused), per group:

    mean(-min(ratio * adv, clamp(ratio, 1 - eps, 1 + eps) * adv)) + 0.5 * mean((V - G)^2) - 0.01 * mean(entropy)

through nn.Softmax -> Categorical(probs)'s p / sum(p) -> log(clamp(p, 2^-23, 1 - 2^-23)), the clamp edge float32's
eps in every precision (the function the kernel states in its header comment), for tanh MLPs of 32 or 64 hidden units.

The act reference gives, per row, the float64 probabilities and their running sums (the CDF), the inverse-CDF pick
at a uniform u (the number of running sums <= u, at most A - 1), and the same from a float32 restatement whose CDF
is summed sequentially: its distance from the float64 CDF is the yardstick of the device's pick.

A gradient case's inputs are the device buffers as ms_wide_grad addresses them: states [R + 3][G][stride] int8,
actions and old log-probs [R + 3][G], returns [G][R]. Everything the kernel must not read holds garbage: every pad
byte (+-127), and three rows after row R - 1 of states (+-127), actions (out of range) and old log-probs (NaN).
Rows on a discontinuity of the loss (ratio within KINK of 1 +- eps_clip, |adv| < KINK, a probability within a factor
4 of a clamp edge) are drawn again, sweep by sweep, from default_rng((seed, sweep)). Old log-probs are the reference's
own log-prob plus N(0, 0.15) noise, so the ratios straddle both clip edges.
"""
from __future__ import annotations

import functools

import numpy as np
import torch

from oracle import ppo_grad_ref as pr

KEYS, ACTOR_KEYS, CRITIC_KEYS = pr.KEYS, pr.ACTOR_KEYS, pr.CRITIC_KEYS
EPS32 = pr.EPS32          # 2^-24: the floor of the parity rule
EPS_P = pr.EPS_P          # 2^-23: Categorical's clamp edge on float32 probabilities
EPS_CLIP = 0.2
KINK = 1e-3
NOISE_SIGMA = pr.NOISE_SIGMA
MAX_SWEEPS = 400
SENTINEL_ROWS = 3
U_LAST = np.float32(1.0 - 2.0 ** -24)  # the largest float32 below 1

TPB, TILE = 256, 16       # kWideThreads, kWideRowsPerTile
STATS = 16                # kWideStats
WORKSPACE_CAP = 64 << 30  # kWideWorkspaceCap


def up4(n):
    return (n + 3) & ~3


def _align256(n):
    return (n + 255) & ~255


# ------------------------------------------------------------------------------------------ the plan, restated

def seg_counts(D, A, H):
    """Floats of one group's twelve gradient tensors, in ms_ppo_grads order."""
    return [H * D, H, H * H, H, A * H, A, H * D, H, H * H, H, H, 1]


def wide_plan(G, D, A, H, R):
    """capi.cpp's wide_plan: k_wide_rows runs NB blocks per group over ceil(R / 16) row tiles (block b takes tiles
    b, b + NB, ...); k_wide_outer / k_wide_w3 reduce RS row splits of rps rows each; the workspace holds
    zbuf [G][NB][16][A], rec [G][R][8H + 16], part [RS][G][total] and loss [G][NB][3] floats, each 256-byte aligned."""
    off = [0]
    for c in seg_counts(D, A, H):
        off.append(off[-1] + c)
    total = off[-1]
    tiles = (R + 15) // 16
    NB = min(tiles, max(1, 2048 // G))
    rs_rows = min(64, max(1, (R + 255) // 256))
    rs_mem = max(1, (1 << 28) // (G * total))
    rs = min(rs_rows, rs_mem)
    rps = ((R + rs - 1) // rs + 15) // 16 * 16
    RS = (R + rps - 1) // rps
    RW = 8 * H + STATS
    o = 0
    at = {}
    for name, floats in (("zbuf", G * NB * 16 * A), ("rec", G * R * RW), ("part", RS * G * total), ("loss", G * NB * 3)):
        at[name] = o
        o += _align256(4 * floats)
    trips = sorted({(tiles - b + NB - 1) // NB for b in range(NB)})
    return dict(NB=NB, tiles=tiles, trips=trips, rs_rows=rs_rows, rs_mem=rs_mem, rs=rs, rps=rps, RS=RS,
                last_rows=R - (RS - 1) * rps, off=off, total=total, at=at, bytes=o)


def workspace_bytes(G, D, A, H, R):
    """ms_wide_workspace_bytes: the plan's byte count, 0 for what ms_wide_grad refuses."""
    if R < 1 or G < 1 or not 1 <= D <= 255 or not 1 <= A <= 1 << 24 or H not in (32, 64):
        return 0
    b = wide_plan(G, D, A, H, R)["bytes"]
    return b if b <= WORKSPACE_CAP else 0


def outer_phases(N):
    """k_wide_outer: row phases per column of a job with N input columns (and the bias column)."""
    return TPB // (N + 1)


def actions_per_thread(A):
    """chunk_of: contiguous actions per thread."""
    return (A + TPB - 1) // TPB


# ------------------------------------------------------------------------------------------------- the nets

def _linear_init(rng, out_f, in_f):
    k = 1.0 / np.sqrt(in_f)
    return (rng.uniform(-k, k, (out_f, in_f)).astype(np.float32), rng.uniform(-k, k, (out_f,)).astype(np.float32))


def draw_nets(rng, G, D, A, H, scale3=1.0):
    """G actor-critics [D -> H -> H -> A], [D -> H -> H -> 1], nn.Linear's init ranges, stacked over the groups."""
    per = []
    for _ in range(G):
        n = {}
        for pre, out in (("", A), ("c", 1)):
            n[pre + "w1"], n[pre + "b1"] = _linear_init(rng, H, D)
            n[pre + "w2"], n[pre + "b2"] = _linear_init(rng, H, H)
            n[pre + "w3"], n[pre + "b3"] = _linear_init(rng, out, H)
        n["w3"], n["b3"] = n["w3"] * np.float32(scale3), n["b3"] * np.float32(scale3)
        per.append(n)
    return {k: np.stack([n[k] for n in per]) for k in KEYS}


def _junk(rng, shape):
    return rng.choice(np.array([-127, 127], dtype=np.int8), shape)


def _draw_rows(rng, shape, D):
    """int8 rows [..., stride]: bytes < D in [-2, 12], garbage in every pad byte."""
    rows = _junk(rng, shape)
    rows[..., :D] = rng.integers(-2, 13, shape[:-1] + (D,)).astype(np.int8)
    return rows


def _extreme_rows(n):
    """(rows at -128, rows at 127) among n rows: two of each from 8 rows on, one of each from 2, none for one."""
    if n < 2:
        return [], []
    if n < 8:
        return [0], [n - 1]
    return [n // 5, n // 2], [n // 3, n - 2]


# ------------------------------------------------------------------------------------------- gradient cases

GBASE = dict(G=2, D=8, A=9, H=32, scale3=1.0)
R_ROWS = (1, 15, 16, 17, 256, 257, 273, 288, 513, 1037, 3841)
D_DIMS = (1, 2, 84, 85, 127, 128, 254, 255)
A_COUNTS = (1, 2, 63, 64, 65, 255, 256, 257, 513, 3000)


def _grad_tables():
    t = {}
    n = [0]

    def add(name, **kw):
        s = dict(GBASE, **kw)
        s["stride"] = up4(s["D"]) + (8 if n[0] % 2 else 0)
        s.setdefault("seed", 1000 + n[0])
        s["family"] = name[0]
        t[name] = s
        n[0] += 1

    # R: the row plan. 288 = two full splits of 144; 1037 = five splits of 208, the last of 205 rows (a partial
    # tile); 3841 = sixteen splits of 256, the last of one row (the smallest R with such a split: see the README)
    for R in R_ROWS:
        add("R/R%d" % R, R=R)
    for R in (273, 1037):
        add("R/R%d-H64" % R, R=R, H=64)
    # T: the tile loop of k_wide_rows
    add("T/G128-R595", G=128, R=595)                       # NB 16, 38 tiles: trips 3 and 2
    add("T/G128-R512-H64", G=128, R=512, H=64)             # NB 16, 32 tiles: two trips each
    add("T/G2049-R40", G=2049, R=40)                       # NB 1: one block, three trips
    add("T/G2-R16437", G=2, R=16437)                       # NB 1024, four blocks with two tiles; rs 64, RS 61
    add("T/G2-R16437-full", G=2, R=16437, D=30, A=225, H=64)  # cfg1's fully aggregated net
    for i, D in enumerate(D_DIMS):
        add("D/D%d" % D, D=D, R=100, H=(32, 64)[i % 2])
    for i, A in enumerate(A_COUNTS):
        add("A/A%d" % A, A=A, R=100, H=(32, 64)[i % 2], G=(1, 3)[(i // 2) % 2])
    # S: near one-hot softmaxes. Most rows have some probability within a factor 4 of a clamp edge and are drawn
    # again (a quarter of the draws is clear at A = 25, one in 25 at A = 257, with these seeds: the best of 600)
    add("S/A25", D=22, A=25, R=160, scale3=40.0, seed=3069)
    add("S/A257", A=257, R=160, H=64, scale3=40.0, seed=3168)
    return t


GRAD_CASES = _grad_tables()


def _row_values(nets, x, act):
    """Float64 per-row values of all groups: lp, V, pmin, pmax (the smallest and largest renormalised probability),
    edge (the smallest factor between any action's p or 1 - p and the clamp edge; 1 = on it)."""
    with torch.no_grad():
        p = {k: torch.as_tensor(nets[k], dtype=torch.float64) for k in KEYS}
        pn, _, lp, _, V = pr._forward(p, torch.as_tensor(x, dtype=torch.float64), torch.as_tensor(act, dtype=torch.int64))
        both = torch.cat([pn, 1.0 - pn], dim=-1).clamp_min(1e-300)
        edge = torch.exp(torch.abs(torch.log(both / EPS_P)).min(dim=-1).values.clamp_max(700.0))
        return dict(lp=lp.numpy(), V=V.numpy(), pmin=pn.min(-1).values.numpy(), pmax=pn.max(-1).values.numpy(),
                    edge=edge.numpy())


def kinks(v, saturated, A):
    """([G, R] bool rows on a discontinuity, [G, R] bool those among them whose state is the cause)."""
    near = (np.abs(v["ratio"] - (1 - EPS_CLIP)) < KINK) | (np.abs(v["ratio"] - (1 + EPS_CLIP)) < KINK)
    if saturated:
        prob = v["edge"] <= 4.0
    else:  # every probability inside the clamp range by a factor 4 (a single action has p = 1: beyond the edge)
        prob = (v["pmin"] < 4 * EPS_P) | ((1 - v["pmax"] < 4 * EPS_P) & (A > 1))
    return near | (np.abs(v["adv"]) < KINK) | prob, prob


def branch_shares(v):
    """Shares of the rows whose minimum is the unclipped surrogate (the ratio's gradient flows) and of those
    clipped away."""
    lo, hi = v["ratio"] < 1 - EPS_CLIP, v["ratio"] > 1 + EPS_CLIP
    away = (hi & (v["adv"] > 0)) | (lo & (v["adv"] < 0))
    return dict(live=float((~away).mean()), away=float(away.mean()))


@functools.lru_cache(maxsize=None)
def grad_case(name):
    """dict(spec, nets, states [R + 3, G, stride] int8, actions [R + 3, G] int32, olp [R + 3, G] float32,
    ret [G, R] float32, x [G, R, D] / act [G, R] / olp_g [G, R] (what the kernel reads), rows (float64 per-row
    values with ratio and adv), sweeps, shares, plan, ref = (grads, loss [G, 3]) in float64, f32 = the same from
    float32 CPU autograd). Deterministic in the case's seed; cached, read-only."""
    spec = GRAD_CASES[name]
    G, D, A, H, R, stride = (spec[k] for k in ("G", "D", "A", "H", "R", "stride"))
    rng = np.random.default_rng((spec["seed"], G, D, A, H, R))
    nets = draw_nets(rng, G, D, A, H, spec["scale3"])
    RP = R + SENTINEL_ROWS
    states = _draw_rows(rng, (RP, G, stride), D)
    states[R:] = _junk(rng, (SENTINEL_ROWS, G, stride))
    lo_rows, hi_rows = _extreme_rows(R)
    for i, r in enumerate(lo_rows):
        states[r, i % G, :D] = -128
    for i, r in enumerate(hi_rows):
        states[r, (i + 1) % G, :D] = 127
    actions = rng.integers(0, A, (RP, G)).astype(np.int32)
    actions[R:] = rng.choice(np.array([-7, A + 5], dtype=np.int32), (SENTINEL_ROWS, G))
    ret = rng.standard_normal((G, R)).astype(np.float32)
    noise = rng.standard_normal((G, R)) * NOISE_SIGMA
    saturated = spec["family"] == "S"
    sweeps = 0
    while True:
        x = np.ascontiguousarray(states[:R, :, :D].transpose(1, 0, 2))
        act = np.ascontiguousarray(actions[:R].T).astype(np.int64)
        v = _row_values(nets, x, act)
        olp_g = (v["lp"] + noise).astype(np.float32)
        v["ratio"] = np.exp(v["lp"] - olp_g.astype(np.float64))
        v["adv"] = ret.astype(np.float64) - v["V"]
        bad, by_state = kinks(v, saturated, A)
        if not bad.any():
            break
        sweeps += 1
        if sweeps > MAX_SWEEPS:
            raise RuntimeError("rows of %s stay on a discontinuity" % name)
        rr = np.random.default_rng((spec["seed"], sweeps))
        g_i, r_i = np.nonzero(bad)
        actions[r_i, g_i] = rr.integers(0, A, len(g_i))
        ret[g_i, r_i] = rr.standard_normal(len(g_i)).astype(np.float32)
        noise[g_i, r_i] = rr.standard_normal(len(g_i)) * NOISE_SIGMA
        g_s, r_s = np.nonzero(by_state)
        if len(g_s):
            states[r_s, g_s] = _draw_rows(rr, (len(g_s), stride), D)
    olp = np.full((RP, G), np.nan, dtype=np.float32)
    olp[:R] = olp_g.T
    xf = x.astype(np.float64)
    ref = pr.grad_ref(nets, xf, act, olp_g, ret, EPS_CLIP, torch.float64)
    f32 = pr.grad_ref(nets, xf, act, olp_g, ret, EPS_CLIP, torch.float32)
    return dict(spec=spec, nets=nets, states=states, actions=actions, olp=olp, ret=ret, x=x, act=act, olp_g=olp_g,
                rows=v, sweeps=sweeps, shares=branch_shares(v), plan=wide_plan(G, D, A, H, R), ref=ref, f32=f32,
                extreme=(lo_rows, hi_rows))


# ------------------------------------------------------------------------------------------------ act cases

ABASE = dict(G=3, D=8, A=9, H=32, E=37, scale3=1.0, underflow=0, ties=False)


def _act_tables():
    t = {}
    n = [0]

    def add(name, **kw):
        s = dict(ABASE, **kw)
        s["stride"] = up4(s["D"]) + (8 if n[0] % 2 else 0)
        s["seed"] = 2000 + n[0]
        t[name] = s
        n[0] += 1

    for i, A in enumerate((1, 2, 9, 255, 256, 257, 513, 3000)):
        add("A%d" % A, A=A, H=(32, 64)[i % 2], G=(1, 3)[(i // 2) % 2])
    for i, D in enumerate((1, 8, 255)):
        add("D%d" % D, D=D, H=(64, 32)[i % 2], A=25)
    for i, E in enumerate((1, 16, 17, 37)):
        add("E%d" % E, E=E, H=(32, 64)[i % 2], G=(3, 1)[i % 2])
    # near one-hot rows whose trailing actions' exp(z - max) is 0 in float32 (b3 lowered by 300 there)
    # (333 rows x 3 groups: the forced u = 1 - 2^-24 rows end on an action the float64 CDF has already passed, and
    # must stay under the 1 % of rows that may differ)
    add("sat-A25", D=22, A=25, E=333, scale3=40.0, underflow=6)
    add("sat-A600", A=600, H=64, E=333, scale3=40.0, underflow=90)
    # a zero last layer: four equal logits, exp(0) = 1 and every running sum exact in float32, every u a multiple
    # of 1/4. u on a boundary takes the action after it (the running sums <= u are counted), with no rounding to
    # hide behind: every pick is the float64 pick
    add("ties-A4", A=4, scale3=0.0, ties=True)
    return t


ACT_CASES = _act_tables()


def _act_forward(nets, x, dtype):
    """[G, E, A] softmax -> renormalised probabilities in `dtype` (torch on the CPU)."""
    with torch.no_grad():
        p = {k: torch.as_tensor(nets[k], dtype=dtype) for k in ACTOR_KEYS}
        h = torch.tanh(pr._lin(torch.tanh(pr._lin(torch.as_tensor(x, dtype=dtype), p["w1"], p["b1"])), p["w2"], p["b2"]))
        probs = torch.softmax(pr._lin(h, p["w3"], p["b3"]), dim=-1)
        return (probs / probs.sum(-1, keepdim=True)).numpy()


def pick(cdf, u):
    """The inverse-CDF sample: the number of running sums <= u, at most A - 1. cdf [..., A], u [...]."""
    return np.minimum((cdf <= u[..., None]).sum(-1), cdf.shape[-1] - 1)


def clamped_log(p):
    return np.log(np.clip(p, EPS_P, 1.0 - EPS_P))


@functools.lru_cache(maxsize=None)
def act_case(name):
    """dict(spec, nets (actor tensors only meaningful), obs [E + 3, G, stride] int8, u [E + 3, G] float32 (NaN past
    row E - 1), p64 / cdf64 [G, E, A], pick64 [G, E], p32 (float32 restatement), cdf32 (its sequential float32 running
    sums), pick32 [G, E], forced = flat rows (e * G + g) whose u is exactly 0 or 1 - 2^-24)."""
    spec = ACT_CASES[name]
    G, D, A, H, E, stride = (spec[k] for k in ("G", "D", "A", "H", "E", "stride"))
    rng = np.random.default_rng((spec["seed"], G, D, A, H, E))
    nets = draw_nets(rng, G, D, A, H, spec["scale3"])
    if spec["underflow"]:
        nets["b3"][:, A - spec["underflow"]:] -= np.float32(300.0)
    EP = E + SENTINEL_ROWS
    obs = _draw_rows(rng, (EP, G, stride), D)
    obs[E:] = _junk(rng, (SENTINEL_ROWS, G, stride))
    lo_rows, hi_rows = _extreme_rows(E)
    for i, r in enumerate(lo_rows):
        obs[r, i % G, :D] = -128
    for i, r in enumerate(hi_rows):
        obs[r, (i + 1) % G, :D] = 127
    u = np.full((EP, G), np.nan, dtype=np.float32)
    u[:E] = rng.random((E, G), dtype=np.float32)
    if spec["ties"]:
        u[:E] = rng.integers(0, A, (E, G)).astype(np.float32) / np.float32(A)
    n = E * G
    zeros = [0] if n < 8 else [0, n // 2, n - 3]
    lasts = [1] if n < 8 else [1, n // 2 + 1, n - 1]
    if n < 2:
        raise ValueError("an act case needs two rows for the forced uniforms")
    flat = u[:E].reshape(-1)
    flat[zeros] = 0.0
    flat[lasts] = U_LAST
    x = np.ascontiguousarray(obs[:E, :, :D].transpose(1, 0, 2)).astype(np.float64)
    ug = np.ascontiguousarray(u[:E].T)
    p64 = _act_forward(nets, x, torch.float64)
    cdf64 = np.cumsum(p64, axis=-1)
    p32 = _act_forward(nets, x, torch.float32)
    cdf32 = np.cumsum(p32, axis=-1, dtype=np.float32)  # sequential float32 running sums
    return dict(spec=spec, nets=nets, obs=obs, u=u, ug=ug, p64=p64, cdf64=cdf64, pick64=pick(cdf64, ug.astype(np.float64)),
                p32=p32, cdf32=cdf32, pick32=pick(cdf32, ug), forced=(zeros, lasts), extreme=(lo_rows, hi_rows))
