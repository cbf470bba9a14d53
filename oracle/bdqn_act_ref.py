"""Float64 reference of Branching-DQN acting (BranchingDQNModules.py:75-123; bdqn_kernels.hip through
ms_bdqn_prepare, ms_bdqn_layer1_compact, ms_bdqn_act and ms_bdqn_act_compact), a plain float32 restatement of the
same arithmetic (the yardstick the GPU tolerances are measured against), and the case tables the CPU and GPU tests
share (tests/test_bdqn_act_ref.py, tests/test_bdqn_act_parity_gpu.py). numpy only, no device.

Acting has one discontinuity, the argmax. The GPU test does not excuse rows near it: a pick is judged by its regret
in the float64 q (how far below the float64 maximum the picked action's float64 q lies), which is continuous in the
kernel's rounding error. The tie cases make q bit-equal on purpose and expect the first index.

Tables (the plan functions below restate the launch plan of bdqn_kernels.hip from the shapes alone):
  H  ms_bdqn_act on given h1 [rows][128]: every NMT = ceil(n / 16) of k_bdqn_act, both sides of each tile edge, row
     counts around the 16-row tile and the 256-row block;
  X  ms_bdqn_act on int8 rows (layer 1 in the kernel): obs around the 32-input k-step, the stride below and above Kp;
  L  ms_bdqn_prepare + ms_bdqn_layer1_compact: every S = Dp / 32 of k_bdqn_l1_cores, replica counts around the
     16-replica tile and the 8-tile chunk, core counts around the vector reads, N 1 and 64;
  C  ms_bdqn_act_compact: ownership patterns none / all / mixed, list lengths around the 256-row block of
     k_bdqn_act and the 1024-row block of k_bdqn_own_list, A = C on both copy paths of k_bdqn_common_fill;
  T  exact ties.
"""
from __future__ import annotations

import functools

import numpy as np

from oracle.learner_ref import BDQN_KEYS, BH, EPS32, align4, bdqn_net

L1_TILES_PER_WAVE = 8    # kL1TilesPerWave
ACT_ROWS_PER_BLOCK = 256  # 16 * kActWaves * kActTiles
OWN_LIST_THREADS = 1024  # kOwnListThreads
H_OBS = 40               # inputs of the net whose layer 1 gives the H and T cases their h1 rows
PAD_BYTES = np.array([-127, 127], dtype=np.int8)
BA_SHIFT = 4.0            # see _net
TIE_RAISE = 12.0          # the tie pairs' bias above the others: the pair is every row's maximum


def pad32(x):
    return (x + 31) // 32 * 32


def foreign_row(D):
    """The foreign acceptor row F (Agent.py:167-212; foreign() of bdqn_kernels.hip): [0, -1, -1, -2, ...]."""
    f = np.full(D, -2, dtype=np.int8)
    f[0:1] = 0
    f[1:3] = -1
    return f


def dense_rows(core_rows, core_owner, N, D):
    """The aggregated acceptor rows [E * N, C * D] int8: agent a's row is R_c[:D] on the cores with owner == a + 1
    and the foreign row elsewhere (k_regen_agent_rows). core_rows [E, C, stride], core_owner [E, C]."""
    cr = np.asarray(core_rows)[:, :, :D]
    co = np.asarray(core_owner)
    E, C = co.shape
    own = co[:, None, :] == (np.arange(N)[None, :, None] + 1)                          # [E, N, C]
    rows = np.where(own[..., None], cr[:, None, :, :], foreign_row(D)[None, None, None, :])
    return rows.reshape(E * N, C * D).astype(np.int8)


def layer1(net, x):
    """W1 x + b1 of int8 rows x [R, obs]: (float64, plain float32 dot)."""
    x = np.asarray(x)
    w1, b1 = np.asarray(net["w1"]), np.asarray(net["b1"])
    h64 = x.astype(np.float64) @ w1.astype(np.float64).T + b1.astype(np.float64)
    h32 = x.astype(np.float32) @ w1.astype(np.float32).T + b1.astype(np.float32)
    return h64, h32


def _q(net, h, dt, ac, n):
    w = {k: np.asarray(net[k], dtype=dt) for k in BDQN_KEYS}
    o1 = np.maximum(np.asarray(h, dtype=dt), 0)
    o2 = np.maximum(o1 @ w["w2"].T + w["b2"], 0)
    v = o2 @ w["wv"].reshape(-1) + w["bv"].reshape(())
    # einsum's own loop, not BLAS: every output element is summed in the same order wherever its row of Wa sits, so
    # identical rows of Wa give bit-equal advantages on any machine (the tie cases rely on it)
    adv = (np.einsum("rk,mk->rm", o2, w["wa"], optimize=False) + w["ba"]).reshape(o1.shape[0], ac, n)
    q = (v[:, None, None] + adv) - adv.mean(axis=2, keepdims=True)
    assert q.dtype == dt
    return q, adv


def q_values(net, h1, h1_32=None):
    """q[r, b, m] = value + adv - mean(adv) after the two ReLUs (BranchingDQNModules.py:88-101) on layer-1
    pre-activations h1 [R, 128], in float64 and in float32 (h1_32: the float32 path's own layer 1, else h1 rounded).
    dict(q64, q32, adv32, pick = first argmax of q64 [R, ac], pick32, gap = top-1 minus top-2 of q64)."""
    wa = np.asarray(net["wa"])
    ba = np.asarray(net["ba"])
    ac_n = wa.shape[0]
    n = int(net["n"]) if "n" in net else None
    assert n is not None and ac_n % n == 0 and ba.shape == (ac_n,)
    ac = ac_n // n
    q64, _ = _q(net, np.asarray(h1, dtype=np.float64), np.float64, ac, n)
    q32, adv32 = _q(net, np.asarray(h1 if h1_32 is None else h1_32, dtype=np.float32), np.float32, ac, n)
    if n > 1:
        s = np.sort(q64, axis=2)
        gap = s[..., -1] - s[..., -2]
    else:
        gap = np.full(q64.shape[:2], np.inf)
    return dict(q64=q64, q32=q32, adv32=adv32, pick=np.argmax(q64, axis=2), pick32=np.argmax(q32, axis=2), gap=gap)


def base_ref(net, D, C):
    """base = b1 + sum_c W1_c F [128]: (float64, float32)."""
    h64, h32 = layer1(net, np.tile(foreign_row(D), C)[None, :])
    return h64[0], h32[0]


def _net(rng, obs, ac, n):
    """bdqn_net's weights with every advantage bias lowered by BA_SHIFT, more than the advantages' spread (about
    3.5 at most over the tables): all advantages are negative then, so a zero-padded action row past n, were it to
    join the argmax, would win it (tests/test_bdqn_gpu.py lowers them by 0.5, which only small n notice)."""
    net = bdqn_net(rng, obs, ac, n)
    net["ba"] = (net["ba"] - np.float32(BA_SHIFT)).astype(np.float32)
    net["n"] = n
    return net


# ------------------------------------------------------------------------------------- the launch plan, restated

def act_plan(n, rows, list_len=None):
    """k_bdqn_act's instantiation and grid for branch width n: NMT, whether the next branch's rows come by LDS-DMA
    (GLDS), the lane groups of an NMT = 1 kernel that hold no action, and the blocks (list_len: 1 + rows owning)."""
    nmt = (n + 15) // 16
    rw = 16 * nmt
    glds = 3 * rw * 136 * 2 + rw * 4 + rw * BH * 4 <= 160 * 1024
    length = rows if list_len is None else list_len
    return dict(nmt=nmt, glds=glds, empty_groups=sum(1 for g4 in range(4) if nmt == 1 and 4 * g4 >= n),
                last_tile_full=n % 16 == 0, blocks=(length + ACT_ROWS_PER_BLOCK - 1) // ACT_ROWS_PER_BLOCK,
                last_block_rows=(length - 1) % ACT_ROWS_PER_BLOCK + 1)


def l1_plan(D, stride, C, E):
    """k_bdqn_l1_cores's instantiation S, replica tiles, chunks of 8 tiles per wave, and the tile count of the
    last chunk (odd: the second accumulator of the last pair idles)."""
    tiles = (E + 15) // 16
    chunks = (tiles + L1_TILES_PER_WAVE - 1) // L1_TILES_PER_WAVE
    return dict(S=pad32(D) // 32, Dp=pad32(D), tiles=tiles, chunks=chunks,
                last_chunk_tiles=tiles - (chunks - 1) * L1_TILES_PER_WAVE, partial_tile=E % 16 != 0,
                stride_over_Dp=stride > pad32(D), stride_under_Dp=stride < pad32(D), pad=stride - D)


# ---------------------------------------------------------------------------------------------------- tables

def _h_table():
    t = {}
    for n in (1, 2, 12, 13, 15, 16, 17, 32, 33, 48, 49, 64, 65, 80, 81, 96, 97, 112, 113, 127, 128):  # 48 .. 65: NMT 4
        t["n%d" % n] = dict(n=n, A=3, rows=300)  # a full block of 256 rows and 44 of the next
    for A, n in ((1, 5), (4, 9), (5, 20), (16, 3), (17, 7), (32, 6), (127, 4)):
        t["A%d" % A] = dict(n=n, A=A, rows=70)
    for rows in (1, 15, 16, 17, 31, 32, 33, 255, 256, 257):
        t["rows%d" % rows] = dict(n=50, A=3, rows=rows)
    return t


def _x_table():
    t = {}
    ns = (5, 16, 17, 40, 70, 90, 100, 128)
    for i, obs in enumerate((1, 31, 32, 33, 64, 65, 255, 256)):
        t["obs%d" % obs] = dict(obs=obs, x_stride=align4(obs), n=ns[i], A=3, rows=257)
        t["obs%d-wide" % obs] = dict(obs=obs, x_stride=pad32(obs) + 8, n=ns[(i + 3) % 8], A=3, rows=257)
    return t


def _l_table():
    t = {}

    def add(name, D, wide, C, N, E, own="mixed", n=3):
        assert name not in t
        t[name] = dict(D=D, stride=align4(D) + (8 if wide else 0), C=C, N=N, E=E, own=own, n=n)

    Cs, Ns, Es = (3, 4, 5, 1, 16, 17), (5, 2, 1, 64), (17, 16, 15, 1, 128, 129, 144)
    for i, D in enumerate((4, 5, 31, 32, 33, 64, 65, 97, 129, 161, 193, 225, 255, 256)):
        big = D > 128
        add("D%d" % D, D, i % 2 == 1, Cs[i % 3] if big else Cs[i % 6], Ns[i % 3] if big else Ns[i % 4], Es[i % 7])
    for D, wide in ((4, True), (31, True), (32, False), (33, True), (256, False)):  # the other stride at a Dp edge
        add("D%d-s" % D, D, wide, 3, 2, 33)
    for C in (1, 3, 4, 5, 16, 17):
        add("C%d" % C, 9, C % 2 == 0, C, 5, 40)
    for N in (1, 2, 5, 64):
        add("N%d" % N, 9, False, 4, N, 20)
    for E in (1, 15, 16, 17, 128, 129, 144):
        add("E%d" % E, 13, E % 2 == 0, 17 if E == 144 else 3, 2, E)
    return t


def _c_table():
    t = {}

    def add(name, D, wide, C, N, E, own, n):
        assert name not in t
        t[name] = dict(D=D, stride=align4(D) + (8 if wide else 0), C=C, N=N, E=E, own=own, n=n)

    # none: every owner 0, the whole result from the common row; A = C on both copy paths of the fill
    add("none-C16", 33, False, 16, 5, 17, "none", 7)
    add("none-C3", 9, True, 3, 2, 129, "none", 97)
    add("none-N64", 5, False, 4, 64, 16, "none", 20)
    # all: every agent owns a core, the list holds rows + 1 entries
    add("all-256", 5, False, 4, 4, 64, "all", 20)
    add("all-512", 4, True, 17, 16, 32, "all", 7)
    add("all-1024", 7, False, 32, 32, 32, "all", 13)
    add("all-N1", 9, False, 1, 1, 1, "all", 5)
    # mixed, list lengths around the 1024-row block of k_bdqn_own_list
    add("mixed-1023", 31, True, 5, 31, 33, "mixed", 17)
    add("mixed-1024", 5, False, 16, 64, 16, "mixed63", 33)
    add("mixed-1025", 9, False, 3, 25, 41, "mixed", 128)
    add("mixed-1088", 4, False, 32, 64, 17, "mixed63", 6)
    add("mixed-C1", 65, False, 1, 2, 40, "mixed", 16)
    add("mixed-C17", 13, False, 17, 5, 144, "mixed", 3)
    add("mixed-C4", 64, True, 4, 5, 30, "mixed", 113)
    return t


H_CASES, X_CASES, L_CASES, C_CASES = _h_table(), _x_table(), _l_table(), _c_table()
EXTRA_ROWS = 40  # rows past n_rows the GPU test appends to h1 / x / explore / rand_action, all garbage


def _h1_rows(rng, rows):
    """Layer-1 pre-activations as a net gives them (both signs around the ReLU), as the f32 the kernel receives."""
    w1 = rng.uniform(-1, 1, (BH, H_OBS)) / np.sqrt(H_OBS)
    b1 = rng.uniform(-1, 1, BH) / np.sqrt(H_OBS)
    x = rng.integers(-5, 14, (rows, H_OBS)).astype(np.float64)
    return (x @ w1.T + b1).astype(np.float32)


def _explore(rng, rows, A, n):
    """explore bytes in {0, 1, 255}; rand_action in range on exploring rows and out of range (negative bytes, which
    no pick can equal) on the others."""
    ex = rng.choice(np.array([0, 0, 1, 255], dtype=np.uint8), rows)
    ex[: min(3, rows)] = np.array([1, 0, 255], dtype=np.uint8)[: min(3, rows)]
    rnd = rng.integers(-128, 0, (rows, A)).astype(np.int8)
    rnd[ex != 0] = rng.integers(0, n, (int((ex != 0).sum()), A)).astype(np.int8)
    return ex, rnd


@functools.lru_cache(maxsize=None)
def h_case(name):
    """dict(n, A, rows, net, h1 [rows, 128] f32, explore, rnd, ref = q_values(net, h1))."""
    c = dict(H_CASES[name])
    n, A, rows = c["n"], c["A"], c["rows"]
    rng = np.random.default_rng((11, n, A, rows))
    net = _net(rng, H_OBS, A, n)
    h1 = _h1_rows(rng, rows)
    ex, rnd = _explore(rng, rows, A, n)
    return dict(c, net=net, h1=h1, explore=ex, rnd=rnd, ref=q_values(net, h1))


@functools.lru_cache(maxsize=None)
def x_case(name):
    """dict(obs, x_stride, n, A, rows, net, x [rows, x_stride] int8 with +-127 in every byte past obs, explore,
    rnd, h64, h32, ref)."""
    c = dict(X_CASES[name])
    obs, xs, n, A, rows = c["obs"], c["x_stride"], c["n"], c["A"], c["rows"]
    rng = np.random.default_rng((12, obs, xs, n))
    net = _net(rng, obs, A, n)
    x = rng.choice(PAD_BYTES, (rows, xs))
    x[:, :obs] = rng.integers(-5, 14, (rows, obs))
    ex, rnd = _explore(rng, rows, A, n)
    h64, h32 = layer1(net, x[:, :obs])
    return dict(c, net=net, x=x, explore=ex, rnd=rnd, h64=h64, h32=h32, ref=q_values(net, h64, h32))


def _owners(rng, pattern, E, C, N):
    if pattern == "none":
        return np.zeros((E, C), dtype=np.int8)
    if pattern == "all":  # every agent owns at least one core (N <= C), the other cores anyone's or nobody's
        assert N <= C
        own = rng.integers(0, N + 1, (E, C))
        for e in range(E):
            own[e, rng.permutation(C)[:N]] = np.arange(1, N + 1)
        return own.astype(np.int8)
    own = np.where(rng.random((E, C)) < 0.5, 0, rng.integers(1, N + 1, (E, C)))
    if pattern == "mixed63":  # every third replica: agent 63 (bit 63 of the mask) owns one core, nobody else any
        assert N == 64
        for e in range(0, E, 3):
            own[e] = 0
            own[e, rng.integers(0, C)] = 64
    own[0, 0] = N  # some core is owned, and by the last agent
    return own.astype(np.int8)


@functools.lru_cache(maxsize=None)
def compact_case(table, name):
    """An L or C case: dict(D, stride, C, N, E, own, n, A = C, net (obs = C * D; W1 holds an exact zero and two
    weights of magnitude about 2^-20), core_rows [E, C, stride] int8 (+-127 past D), core_owner [E, C] int8, x =
    dense_rows, h64, h32, base64, base32, owning [E * N] bool, explore, rnd, ref = q_values on layer1(x))."""
    c = dict((L_CASES if table == "L" else C_CASES)[name])
    D, stride, C, N, E, n = c["D"], c["stride"], c["C"], c["N"], c["E"], c["n"]
    rng = np.random.default_rng((13 if table == "L" else 14, D, stride, C, N, E, n))
    net = _net(rng, C * D, C, n)
    net["w1"][0, 0] = 0.0
    net["w1"][1, 1] = np.float32(2.0 ** -20)
    net["w1"][2, D - 1] = np.float32(-1.2345 * 2.0 ** -20)
    cr = rng.choice(PAD_BYTES, (E, C, stride))
    cr[:, :, :D] = rng.integers(-5, 14, (E, C, D))
    co = _owners(rng, c["own"], E, C, N)
    x = dense_rows(cr, co, N, D)
    h64, h32 = layer1(net, x)
    b64, b32 = base_ref(net, D, C)
    owning = (co[:, None, :] == (np.arange(N)[None, :, None] + 1)).any(axis=2).reshape(-1)
    ex, rnd = _explore(rng, E * N, C, n)
    return dict(c, A=C, net=net, core_rows=cr, core_owner=co, x=x, h64=h64, h32=h32, base64=b64, base32=b32,
                owning=owning, explore=ex, rnd=rnd, ref=q_values(net, h64, h32))


# ------------------------------------------------------------------------------------------------ exact ties
# Lane (j, g4) of k_bdqn_act holds actions 16 mt + 4 g4 + q of its row: a lane scans (mt, q) in increasing index,
# then two __shfl_xor rounds join the four lane groups. Pairs (first, second) of equal maxima by where they sit;
# `last` is the branch's last action n - 1. Every pattern fills four consecutive branches, since lane group b & 3
# writes branch b and a wrong join leaves different lane groups with different answers.
TIE_N = (100, 128)
TIE_PATTERNS = (
    ("same-lane-q", lambda n: (36, 38)),        # mt 2, g4 1, q 0 and 2
    ("lane-groups", lambda n: (49, 57)),        # mt 3, g4 0 and 2
    ("tiles", lambda n: (28, 64)),              # mt 1 g4 3 against mt 4 g4 0: the smaller index in the higher group
    ("same-lane-tiles", lambda n: (5, 53)),     # g4 1 q 1, mt 0 and 3
    ("first-last-tile", lambda n: (2, n - 1)),  # mt 0 against the last (partial at n = 100) tile
    ("zero", None),                             # Wa = 0 and ba constant (negative): every q equal, the pick is 0
)


def tie_position(m):
    return dict(mt=m // 16, g4=(m % 16) // 4, q=m % 4)


@functools.lru_cache(maxsize=None)
def tie_case(n):
    """ms_bdqn_act on h1 with exact ties: branch b carries pattern b // 4. dict(n, A, rows, net, h1, expect [A]
    (the first index of the pair, or 0), pairs [A] ((j, k) or None), ref). n = 5: four all-equal branches."""
    pats = TIE_PATTERNS if n > 16 else (("zero", None),)
    A, rows = 4 * len(pats), 70
    rng = np.random.default_rng((15, n))
    net = _net(rng, H_OBS, A, n)
    expect, pairs = [], []
    for b in range(A):
        pos = pats[b // 4][1]
        if pos is None:
            net["wa"][b * n:(b + 1) * n] = 0.0
            net["ba"][b * n:(b + 1) * n] = np.float32(-0.3)
            expect.append(0)
            pairs.append(None)
            continue
        j, k = pos(n)
        net["wa"][b * n + k] = net["wa"][b * n + j]
        net["ba"][b * n + j] += np.float32(TIE_RAISE)
        net["ba"][b * n + k] = net["ba"][b * n + j]
        expect.append(j)
        pairs.append((j, k))
    h1 = _h1_rows(rng, rows)
    return dict(n=n, A=A, rows=rows, net=net, h1=h1, expect=np.array(expect), pairs=tuple(pairs), ref=q_values(net, h1))


def case(name):
    """A case by its printed name: "H-n17", "X-obs31-wide", "L-D5", "C-none-C3", "T-100" (ties at n = 100)."""
    table, key = name.split("-", 1)
    if table == "H":
        return h_case(key)
    if table == "X":
        return x_case(key)
    if table == "T":
        return tie_case(int(key))
    return compact_case(table, key)
