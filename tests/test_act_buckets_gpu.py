"""The acting kernels at every instantiation their launchers dispatch (policy_kernels.hip: dispatch_act,
greedy_kernels.hip: dispatch_greedy, ms_act_kernels.h: act_bucket): S1 = bucket(ceil(stride / 32)) layer-1
k-steps times NT = bucket(ceil(A / 16)) action tiles, buckets {1, 2, 4, 8}. One shape table (TABLE) holds an
interior point of each of the 16 (S1, NT) pairs and the edges of every bucket; each case is one shape, so a
failure names its bucket. Sampling (ms_policy_act) and greedy (ms_policy_act_greedy) are held against float64
and float32 CPU restatements (oracle.ppo_ref.act_reference, tests.test_greedy_gpu), the derived forms
(common row, ms_act_prepare's fragments, compact rows) against the plain kernel bit for bit, the two-net offer
kernel (ms_offer_act_free) at each of its (NT, NT2) variants, and three edges of the sampling code are forced:
garbage in the bytes between D and stride (they must meet zero weights), u * S at the rounded total (the last
action with nonzero probability) and A = 1. The PPO gradient dispatch, the act rounds and the fused env rollouts
are not covered here.

Every case prints one "ACTB|" line of figures (pytest -s); profiles/r14_act_buckets/README.md records them."""
import copy
import functools
import importlib

import numpy as np
import pytest
import torch

from oracle.ppo_ref import act_reference
from tests.test_greedy_gpu import _logits, _obs, check_greedy_rows

gpu = pytest.mark.gpu

EPS = float(torch.finfo(torch.float32).eps)  # Categorical's clamp of the probabilities (Head::clamped_log)
RTOL, ATOL = 1e-5, 2e-6                      # the project's log-prob tolerance (test_act_kernel_matches_reference)
NEAR_U = 1e-5                                # u this close to a float64 CDF boundary: either neighbour may be picked
MAX_NEAR_SHARE = 0.01                        # of a case's rows, from the reference alone


def act_bucket(n):
    """ms_act_kernels.h: 'the kernels are built for 1, 2, 4 or 8 layer-1 k-steps (32 row bytes each) and 16-action
    tiles: the bucket a count falls in, 0 beyond 8 (not built)'."""
    return 1 if n <= 1 else 2 if n <= 2 else 4 if n <= 4 else 8 if n <= 8 else 0


def s1_of(stride):
    return act_bucket((stride + 31) // 32)


def nt_of(n_actions):
    return act_bucket((n_actions + 15) // 16)


# ---- the shape table: (D, stride, A)
INTERIOR = [(s - 1, s, A) for s in (20, 52, 100, 196) for A in (9, 25, 49, 97)]
A_EDGE_VALUES = (1, 2, 16, 17, 32, 33, 48, 64, 65, 112, 127)
A_EDGES = [(s - 1, s, A) for s in (12, 132) for A in A_EDGE_VALUES]
STRIDE_EDGES = [(D, s, 13) for D, s in ((1, 4), (4, 4), (30, 32), (32, 32), (33, 36), (64, 64), (65, 68), (126, 128),
                                        (128, 128), (129, 132), (253, 256), (256, 256))]
CORNER = [(256, 256, 127)]
TABLE = INTERIOR + A_EDGES + STRIDE_EDGES + CORNER


def shape_id(shape):
    D, stride, A = shape
    return "s%d-nt%d-D%dx%d-A%d" % (s1_of(stride), nt_of(A), D, stride, A)


def ids(shapes):
    return [shape_id(s) for s in shapes]


# (E, G, units per group): rows per group 201, 101, 131, 166, 485, 213, none a multiple of 16, so every group
# ends in a partial tile; at these sizes a wave of k_act takes one tile (an odd count: run2's unpaired tile)
SIZES = [(67, 1, 3), (101, 3, 1), (131, 1, 1), (83, 3, 2), (97, 1, 5), (71, 3, 3)]

# Shapes wider than 196 bytes whose log-probs need more than RTOL / ATOL: the allowance is max|lp32 - lp64| of
# the two CPU restatements at that shape (the reference's own error), added to ATOL. None was needed.
WIDE_ALLOW = {}


def test_table_reaches_every_bucket():
    """A fact about TABLE, not about the kernels: every (S1, NT) in {1, 2, 4, 8}^2 is reached, by an interior
    point and by the edges of each bucket, within what check_mlp admits."""
    assert len(set(TABLE)) == len(TABLE)
    for D, stride, A in TABLE:
        assert 1 <= D <= stride <= 256 and stride % 4 == 0 and 1 <= A <= 127
        assert s1_of(stride) in (1, 2, 4, 8) and nt_of(A) in (1, 2, 4, 8)
    want = {(s, n) for s in (1, 2, 4, 8) for n in (1, 2, 4, 8)}
    assert {(s1_of(s), nt_of(A)) for _, s, A in INTERIOR} == want and len(INTERIOR) == 16
    assert {(s1_of(s), nt_of(A)) for _, s, A in TABLE} == want
    # both sides of every bucket edge
    assert [nt_of(A) for A in A_EDGE_VALUES] == [1, 1, 1, 2, 2, 4, 4, 4, 8, 8, 8]
    assert [s1_of(s) for _, s, _ in STRIDE_EDGES] == [1, 1, 1, 1, 2, 2, 4, 4, 4, 8, 8, 8]
    # a wholly padded tile: A = 33..48 inside NT = 4, A = 65..112 inside NT = 8
    assert any(33 <= A <= 48 for _, _, A in A_EDGES) and any(65 <= A <= 112 for _, _, A in A_EDGES)
    for E, G, pg in SIZES:
        assert (E * pg) % 16 != 0 and E * G * pg <= 4000


def _ppo():
    return importlib.import_module("marl-scheduling_amd.ppo")


def _grouped(fn, G, pg):
    """fn(g, slice of group g's units) -> [E, pg, ...]; the groups side by side as [E, U, ...]."""
    return torch.cat([fn(g, slice(g * pg, (g + 1) * pg)) for g in range(G)], 1)


def _probs(w, obs, u, G, pg, D, dtype):
    """act_reference in dtype on every group's rows: (action [E, U], probabilities [E, U, A])."""
    out = []
    for g in range(G):
        sl = slice(g * pg, (g + 1) * pg)
        flat = {k: v[g].to(dtype) for k, v in w.items()}
        a, _, p = act_reference(flat, obs[:, sl, :D].to(dtype), u[:, sl].to(dtype))
        out.append((a, p))
    return torch.cat([a for a, _ in out], 1), torch.cat([p for _, p in out], 1)


def _clamped_log(p):
    return torch.log(p.clamp(EPS, 1.0 - EPS))


class Case:
    """One table shape's net, rows and uniforms, and the CPU restatements of both (computed once, shared by
    the sampling and the greedy tests, never written to)."""

    def __init__(self, shape):
        ppo = _ppo()
        self.shape = shape
        D, stride, A = shape
        i = TABLE.index(shape)
        self.E, self.G, self.pg = SIZES[i % len(SIZES)]
        self.U = self.G * self.pg
        torch.manual_seed(100 + i)
        net = ppo.GroupedActorCritic(self.G, D, A)
        with torch.no_grad():  # a default head is near-uniform: sharper distributions
            net.w3.mul_(4.0)
            net.b3.mul_(4.0)
        self.net = net
        self.w = {k: getattr(net, k).detach().clone() for k in ppo.ACTOR_KEYS}
        self.obs = _obs(self.E, self.U, D, stride, seed=200 + i)
        # (seeds chosen on the CPU: every case's share of near-boundary rows is within MAX_NEAR_SHARE)
        self.u = torch.rand((self.E, self.U), generator=torch.Generator().manual_seed(310 + i))
        self.a64, self.p64 = _probs(self.w, self.obs, self.u, self.G, self.pg, D, torch.float64)
        _, self.p32 = _probs(self.w, self.obs, self.u, self.G, self.pg, D, torch.float32)
        self.lp32 = _clamped_log(self.p32)                      # [E, U, A] f32: what the kernel returns for a
        self.lp64 = _clamped_log(self.p64)
        cdf = torch.cumsum(self.p64, -1)[..., :-1]              # the A - 1 boundaries between actions
        gap = (cdf - self.u.double().unsqueeze(-1)).abs()
        self.near = gap.min(-1).values < NEAR_U if A > 1 else torch.zeros_like(self.u, dtype=torch.bool)
        # the restatements' own disagreement on the reference pick's log-prob
        at = self.a64.unsqueeze(-1)
        self.lp_gap = float((self.lp32.double().gather(2, at) - self.lp64.gather(2, at)).abs().max())
        self.l64 = _grouped(lambda g, sl: _logits(self.w, g, self.obs[:, sl, :D], torch.float64), self.G, self.pg)
        self.l32 = _grouped(lambda g, sl: _logits(self.w, g, self.obs[:, sl, :D], torch.float32), self.G, self.pg)

    def device_net(self):
        return copy.deepcopy(self.net).cuda()

    def garbage_obs(self):
        """The rows with bytes D..stride-1 alternating 127, -128 (None: no such bytes)."""
        D, stride, _ = self.shape
        if stride == D:
            return None
        obs = self.obs.clone()
        obs[..., D:] = torch.tensor([127, -128] * 2, dtype=torch.int8)[:stride - D]
        return obs


@functools.lru_cache(maxsize=None)
def _case(shape):
    return Case(shape)


def _bits(x):
    return x.view(torch.int32)


def _assert_same(a0, l0, a1, l1):
    assert torch.equal(a0, a1)
    assert torch.equal(_bits(l0), _bits(l1))


def _check_range(act, lp, A):
    assert int(act.min()) >= 0 and int(act.max()) < A
    assert bool(torch.isfinite(lp).all()) and float(lp.max()) <= 0.0


# ---- 2. sampling against the float64 restatement
@gpu
@pytest.mark.parametrize("shape", TABLE, ids=ids(TABLE))
def test_act_matches_float64(ms, shape):
    D, stride, A = shape
    c = _case(shape)
    n_rows = c.E * c.U
    # the exemption's cap comes from the reference alone
    share = float(c.near.float().mean())
    assert share <= MAX_NEAR_SHARE
    net = c.device_net()
    dobs, du = c.obs.cuda(), c.u.cuda()
    act_d, lp_d = net.act(dobs, c.U, seed=0, offset=0, uniforms=du)
    act, lp = act_d.cpu().long(), lp_d.cpu()
    _check_range(act, lp, A)
    mism = act != c.a64
    print("ACTB|act|%s|rows %d|near share %.4f%%|exempted %d|lp32-lp64 gap %.3g" %
          (shape_id(shape), n_rows, 100.0 * share, int(mism.sum()), c.lp_gap))
    assert not bool((mism & ~c.near).any())
    assert int(mism.sum()) <= int(c.near.sum())
    same = ~mism
    want = c.lp32.gather(2, act.unsqueeze(-1)).squeeze(-1)
    np.testing.assert_allclose(lp[same].numpy(), want[same].numpy(), rtol=RTOL, atol=ATOL + WIDE_ALLOW.get(shape, 0.0))
    # bytes D..stride-1 meet zero weights (W1Split::load): garbage there changes nothing, bit for bit
    gobs = c.garbage_obs()
    if gobs is not None:
        gobs = gobs.cuda()
        a2, l2 = net.act(gobs, c.U, seed=0, offset=0, uniforms=du)
        _assert_same(act_d, lp_d, a2, l2)
        g0, gl0 = net.act_greedy(dobs, c.U)
        g1, gl1 = net.act_greedy(gobs, c.U)
        _assert_same(g0, gl0, g1, gl1)


@gpu
@pytest.mark.parametrize("shape", INTERIOR, ids=ids(INTERIOR))
def test_act_philox_path(ms, shape):
    """uniforms=None: the kernel's own Philox draws. Deterministic in (seed, offset), another offset draws
    anew, and a row's log-prob is the restated log p[a] of whatever action it drew; where the draw picks the
    action the external uniform picked, the same row gives the same bits."""
    D, stride, A = shape
    c = _case(shape)
    net = c.device_net()
    dobs = c.obs.cuda()
    a0, l0 = net.act(dobs, c.U, seed=3, offset=11)
    a1, l1 = net.act(dobs, c.U, seed=3, offset=11)
    _assert_same(a0, l0, a1, l1)
    a2, _ = net.act(dobs, c.U, seed=3, offset=12)
    assert not torch.equal(a0, a2)
    act, lp = a0.cpu().long(), l0.cpu()
    _check_range(act, lp, A)
    want = c.lp32.gather(2, act.unsqueeze(-1)).squeeze(-1)
    np.testing.assert_allclose(lp.numpy(), want.numpy(), rtol=RTOL, atol=ATOL + WIDE_ALLOW.get(shape, 0.0))
    ae, le = net.act(dobs, c.U, seed=0, offset=0, uniforms=c.u.cuda())
    both = a0 == ae
    assert int(both.sum()) > 0
    assert torch.equal(_bits(l0)[both], _bits(le)[both])


# ---- 3. sampling edges: zero-probability actions at both ends, u at 0 and at the top, A = 1
EDGE_SHAPES = [(D, s, A) for D, s in ((11, 12), (100, 100)) for A in (1, 5, 17, 33, 65, 127)]
EDGE_U = (0.0, 2.0 ** -24, 0.5, 1.0 - 2.0 ** -24)


@gpu
@pytest.mark.parametrize("shape", EDGE_SHAPES, ids=ids(EDGE_SHAPES))
def test_sampling_edges(ms, shape):
    """The first k0 and the last k1 actions 200 below the rest: their f32 numerators are exactly 0. A pick
    always has nonzero probability and stays below A (15 padded lanes in the last tile at A = 16 (NT - 1) + 1);
    u = 0 picks the first live action, u = 1 - 2^-24 the last one (u * S at or past the rounded total takes
    Head::last_nonzero, not act_reference's clamp to A - 1). Rows of 16 bytes and more repeat every draw through
    the common row's sampling table (act(common_row=...)), bit for bit."""
    ppo = _ppo()
    D, stride, A = shape
    i = EDGE_SHAPES.index(shape)
    E, G, pg = SIZES[i % len(SIZES)]
    U = G * pg
    torch.manual_seed(400 + i)
    net = ppo.GroupedActorCritic(G, D, A)
    w = {k: getattr(net, k).detach().clone() for k in ppo.ACTOR_KEYS}
    obs = _obs(E, U, D, stride, seed=500 + i)
    dobs = obs.cuda()
    net = net.cuda()
    # the same edges through the common row's sampling table (Head::table's running sums and last nonzero
    # action, k_act_common's scan): every other replica's rows equal one row
    crow = obs[0, 0].clone().cuda()
    cobs = obs.clone()
    cobs[::2] = obs[0, 0]
    cobs = cobs.cuda()
    for k0 in (0, 1, 3):
        for k1 in (0, 1, 3):
            if k0 + k1 >= A:
                continue
            b3 = w["b3"].clone()
            b3[:, :k0] -= 200.0
            b3[:, A - k1:] -= 200.0
            with torch.no_grad():
                net.b3.copy_(b3)
            wk = dict(w, b3=b3)
            _, p32 = _probs(wk, obs, torch.zeros((E, U)), G, pg, D, torch.float32)
            live = torch.zeros(A, dtype=torch.bool)
            live[k0:A - k1] = True
            assert bool((p32[..., live] > 0).all()) and bool((p32[..., ~live] == 0).all())
            # the ends are no rounding matter: the first and the last live action have real mass
            assert float(p32[..., k0].min()) > 1e-4 and float(p32[..., A - k1 - 1].min()) > 1e-4
            lp32 = _clamped_log(p32)
            for uv in EDGE_U:
                u = torch.full((E, U), uv, dtype=torch.float32)
                assert float(u[0, 0]) == uv
                act, lp = net.act(dobs, U, seed=0, offset=0, uniforms=u.cuda())
                act, lp = act.cpu().long(), lp.cpu()
                what = "%s k0=%d k1=%d u=%r" % (shape_id(shape), k0, k1, uv)
                assert int(act.min()) >= 0 and int(act.max()) < A, what
                assert bool(live[act].all()), what
                assert bool((p32.gather(2, act.unsqueeze(-1)) > 0).all()), what
                if uv == 0.0:
                    assert bool((act == k0).all()), what
                if uv == EDGE_U[-1]:
                    assert bool((act == A - k1 - 1).all()), what
                assert bool(torch.isfinite(lp).all()) and float(lp.max()) <= 0.0, what
                want = lp32.gather(2, act.unsqueeze(-1)).squeeze(-1)
                np.testing.assert_allclose(lp.numpy(), want.numpy(), rtol=RTOL, atol=ATOL, err_msg=what)
                if A == 1:
                    assert bool((act == 0).all())
                    np.testing.assert_allclose(lp.numpy(), np.log(1.0 - 2.0 ** -23), rtol=0, atol=ATOL)
                if stride >= 16:
                    ca, cl = net.act(cobs, U, seed=0, offset=0, uniforms=u.cuda())
                    assert int(ca.min()) >= 0 and int(ca.max()) < A and bool(live[ca.cpu().long()].all()), what
                    ta, tl = net.act(cobs, U, seed=0, offset=0, uniforms=u.cuda(), common_row=crow)
                    assert torch.equal(ca, ta) and torch.equal(_bits(cl), _bits(tl)), what
    print("ACTB|edges|%s|rows %d" % (shape_id(shape), E * U))


# ---- 4. the derived forms, bit for bit, at every bucket
BIT_SHAPES = (INTERIOR + [(s - 1, s, A) for s in (12, 132) for A in (17, 33, 65)] +
              [(33, 36, 13), (65, 68, 13), (129, 132, 13)])


@gpu
@pytest.mark.parametrize("ext_u", [False, True], ids=["philox", "extu"])
@pytest.mark.parametrize("shape", BIT_SHAPES, ids=ids(BIT_SHAPES))
def test_derived_forms_bit_identical(ms, shape, ext_u):
    """act(common_row=...), acting on ms_act_prepare's fragments (made with and without the common row's
    table), act_compact on (core rows, owners) and act_greedy(common_row=...) against the plain kernels, with
    an arbitrary common row (not the acceptor's, so S1 and NT vary independently). Rows of fewer than 16
    bytes have no common-row kernel: act takes the plain one, act_compact refuses them."""
    ppo = _ppo()
    lib_mod = importlib.import_module("marl-scheduling_amd._lib")
    D, stride, A = shape
    i = BIT_SHAPES.index(shape)
    N, C = 3, 2 + i % 2
    G = 1 if (i // 2) % 2 == 0 else 3  # G = 3: a group is one agent's C acceptors (S == C)
    U = N * C
    E = (67, 101, 131)[i % 3]
    assert (E * U // G) % 16 != 0
    torch.manual_seed(600 + i)
    net = ppo.GroupedActorCritic(G, D, A)
    with torch.no_grad():
        net.w3.mul_(4.0)
        net.b3.mul_(4.0)
    net = net.cuda()
    gen = torch.Generator().manual_seed(700 + i)
    crow = torch.zeros(stride, dtype=torch.int8)
    crow[:D] = torch.randint(-5, 13, (D,), generator=gen, dtype=torch.int8)
    obs = torch.zeros((E, U, stride), dtype=torch.int8)
    obs[..., :D] = torch.randint(-5, 13, (E, U, D), generator=gen, dtype=torch.int8)
    pick = torch.rand((E, U), generator=gen) < 0.85
    obs[pick] = crow
    off1 = (torch.rand((E, U), generator=gen) < 0.02) & pick  # one byte off the common row
    col = torch.randint(0, D, (E, U), generator=gen)
    obs[off1, col[off1]] = crow[col[off1]] + 1
    assert int(off1.sum()) > 0 and not bool((obs[off1] == crow).all(-1).any())
    u = torch.rand((E, U), generator=gen).cuda() if ext_u else None
    dobs, dcrow = obs.cuda(), crow.cuda()
    kw = dict(seed=3, offset=11, uniforms=u)
    a0, l0 = net.act(dobs, U, **kw)
    _check_range(a0.cpu().long(), l0.cpu(), A)
    _assert_same(a0, l0, *net.act(dobs, U, common_row=dcrow, **kw))
    frag_c = ppo.ActFrag(net, stride, dcrow)  # with the common row's table
    frag_c.build(net)
    frag_p = ppo.ActFrag(net, stride)         # without: the common-row kernel makes its table itself
    frag_p.build(net)
    for frag in (frag_c, frag_p):
        _assert_same(a0, l0, *net.act(dobs, U, frag=frag, **kw))
        _assert_same(a0, l0, *net.act(dobs, U, common_row=dcrow, frag=frag, **kw))
    g0, gl0 = net.act_greedy(dobs, U)
    _assert_same(g0, gl0, *net.act_greedy(dobs, U, common_row=dcrow))
    # compact rows: owners include the auctioneer (0); some owned rows equal the common row or are one byte off
    rows = torch.zeros((E, C, stride), dtype=torch.int8)
    rows[..., :D] = torch.randint(-5, 13, (E, C, D), generator=gen, dtype=torch.int8)
    same = torch.rand((E, C), generator=gen) < 0.1
    rows[same] = crow
    off1 = (torch.rand((E, C), generator=gen) < 0.5) & same
    col = torch.randint(0, D, (E, C), generator=gen)
    rows[off1, col[off1]] = crow[col[off1]] + 1
    owner = torch.randint(0, N + 1, (E, C), generator=gen, dtype=torch.int8)
    assert bool((owner == 0).any())
    rows, owner = rows.cuda(), owner.cuda()
    if stride < 16:
        with pytest.raises(lib_mod.MarlSchedError) as err:
            net.act_compact(rows, owner, U, 3, 11, dcrow, uniforms=u)
        assert err.value.code == ppo.MS_EINVAL
        return
    full = ppo.regen_acceptor_rows(rows, owner, dcrow, N).contiguous()
    assert full.shape == (E, U, stride)
    c0, cl0 = net.act(full, U, **kw)
    _assert_same(c0, cl0, *net.act(full, U, common_row=dcrow, **kw))
    for frag in (None, frag_c, frag_p):
        _assert_same(c0, cl0, *net.act_compact(rows, owner, U, 3, 11, dcrow, uniforms=u, frag=frag))


# ---- 5. greedy against float64
@gpu
@pytest.mark.parametrize("shape", TABLE, ids=ids(TABLE))
def test_greedy_matches_float64(ms, shape):
    D, stride, A = shape
    c = _case(shape)
    act, lp = c.device_net().act_greedy(c.obs.cuda(), c.U)
    act, lp = act.cpu().long().reshape(-1), lp.cpu().reshape(-1)
    assert int(act.min()) >= 0 and int(act.max()) < A
    l64, l32 = c.l64.reshape(-1, A), c.l32.reshape(-1, A)
    if A == 1:  # no second logit to tie with
        assert bool((act == 0).all())
        near = 0
    else:
        _, near = check_greedy_rows(act, l64, l32, shape_id(shape) + ":")
    print("ACTB|greedy|%s|rows %d|near-tied %d" % (shape_id(shape), len(act), near))
    ref = torch.log_softmax(l32, -1).gather(1, act.view(-1, 1)).squeeze(1)
    np.testing.assert_allclose(lp.numpy(), ref.numpy(), rtol=RTOL, atol=ATOL)


@gpu
@pytest.mark.parametrize("A", [17, 33, 48, 65, 112, 127])
@pytest.mark.parametrize("stride", [12, 132])
def test_greedy_padding_actions_never_win(ms, stride, A):
    """Every logit -10, the padded accumulator rows 0 (a whole tile of them at A = 33, 48, 65, 112): the pick
    is 0; b3[A - 1] raised: the pick is A - 1, the last real action beside the padding."""
    ppo = _ppo()
    torch.manual_seed(0)
    G, per_group, D, E = 2, 3, stride - 1, 37
    net = ppo.GroupedActorCritic(G, D, A)
    with torch.no_grad():
        net.w3.zero_()
        net.b3.fill_(-10.0)
    obs = _obs(E, G * per_group, D, stride).cuda()
    net = net.cuda()
    act, lp = net.act_greedy(obs, G * per_group)
    assert torch.equal(act.cpu().long(), torch.zeros((E, G * per_group), dtype=torch.long))
    np.testing.assert_allclose(lp.cpu().numpy(), -np.log(A), rtol=RTOL, atol=ATOL)
    with torch.no_grad():
        net.b3[:, A - 1] = -9.0
    act, _ = net.act_greedy(obs, G * per_group)
    assert torch.equal(act.cpu().long(), torch.full((E, G * per_group), A - 1))


# ---- 6. the two-net offer kernel at each (NT, NT2) variant
# (C, A2): k_act<S1, NT, NT2> of dispatch_act; 3 to 8 price tiles share <4, 8> whatever the core chooser's NT
OFFER_CASES = [(2, 5), (2, 20), (16, 11), (16, 30), (40, 13), (40, 20), (16, 40), (40, 100), (8, 127)]


def _offer_out(E, U, fill=None):
    dev = "cuda"
    mk = (lambda shape, dt: torch.empty(shape, dtype=dt, device=dev)) if fill is None else \
        (lambda shape, dt: torch.full(shape, fill, dtype=dt, device=dev))
    return dict(core_action=mk((E, U), torch.int8), core_logprob=mk((E, U), torch.float32),
                price_state=mk((E, U, 4), torch.int8), price_action=mk((E, U), torch.int8),
                price_logprob=mk((E, U), torch.float32), env_price=mk((E, U), torch.int8))


@gpu
@pytest.mark.parametrize("C,A2", OFFER_CASES, ids=["C%d-A2_%d-nt%d-nt2_%d" % (C, A2, nt_of(C + 1), nt_of(A2))
                                                   for C, A2 in OFFER_CASES])
def test_offer_act_free_variants(ms, C, A2):
    """FreePriceOfferPPO.selectAction fused (PPOmodules.py:312-332) against act_reference, as
    test_offer_act_free_matches_reference holds it, at every two-net instantiation; and garbage in the row's
    padding bytes changes no output."""
    ppo = _ppo()
    i = OFFER_CASES.index((C, A2))
    G, per_group = ((1, 3), (3, 1), (3, 2))[i % 3]
    torch.manual_seed(800 + i)
    D, A = 2 * C + 2, C + 1
    stride = (D + 3) & ~3
    assert stride > D
    core = ppo.GroupedActorCritic(G, D, A)
    price = ppo.GroupedActorCritic(G, 4, A2)
    E, U = 67, G * per_group
    gen = torch.Generator().manual_seed(900 + i)
    obs = torch.zeros((E, U, stride), dtype=torch.int8)
    obs[..., :D] = torch.randint(-1, 13, (E, U, D), generator=gen, dtype=torch.int8)
    u = torch.rand((2, E, U), generator=gen)
    cf = {k: getattr(core, k).detach().clone() for k in ppo.ACTOR_KEYS}
    pf = {k: getattr(price, k).detach().clone() for k in ppo.ACTOR_KEYS}
    core, price = core.cuda(), price.cuda()
    dout = _offer_out(E, U)
    ppo.offer_act_free(core, price, obs.cuda(), C, 0, 0, dout, uniforms=u.cuda())
    out = {k: v.cpu() for k, v in dout.items()}
    assert int(out["core_action"].min()) >= 0 and int(out["core_action"].max()) < A
    assert int(out["price_action"].min()) >= 0 and int(out["price_action"].max()) < A2
    for g in range(G):
        sl = slice(g * per_group, (g + 1) * per_group)
        x = obs[:, sl, :D].float()
        ra, rlp, _ = act_reference({k: v[g] for k, v in cf.items()}, x, u[0][:, sl])
        ga = out["core_action"][:, sl].long()
        ok = ga == ra
        assert ok.float().mean() > 0.999
        np.testing.assert_allclose(out["core_logprob"][:, sl][ok].numpy(), rlp[ok].numpy(), rtol=RTOL, atol=ATOL)
        # the price chooser's input from the device's own core action
        idx = (2 * ga).unsqueeze(-1) + torch.arange(2)
        pin = torch.cat((torch.gather(x, 2, idx), x[..., 2 * C:2 * C + 2]), -1)
        pin = torch.where((ga == 0).unsqueeze(-1), torch.full_like(pin, -5.0), pin)
        assert torch.equal(out["price_state"][:, sl].float(), pin)
        pa, plp, _ = act_reference({k: v[g] for k, v in pf.items()}, pin, u[1][:, sl])
        gp = out["price_action"][:, sl].long()
        okp = gp == pa
        assert okp.float().mean() > 0.999
        np.testing.assert_allclose(out["price_logprob"][:, sl][okp].numpy(), plp[okp].numpy(), rtol=RTOL, atol=ATOL)
        want_env = torch.where(ga == 0, torch.full_like(gp, -5), gp)
        assert torch.equal(out["env_price"][:, sl].long(), want_env)
    gobs = obs.clone()
    gobs[..., D:] = torch.tensor([127, -128] * 2, dtype=torch.int8)[:stride - D]
    dout2 = _offer_out(E, U)
    ppo.offer_act_free(core, price, gobs.cuda(), C, 0, 0, dout2, uniforms=u.cuda())
    for k in dout:
        a, b = dout[k], dout2[k]
        assert torch.equal(_bits(a), _bits(b)) if a.dtype == torch.float32 else torch.equal(a, b), k


@gpu
def test_offer_act_free_refuses_wide_core_chooser(ms):
    """The two-net kernel has no NT = 8 core chooser: C = 64 (MS_MAX_CORES, A = 65) with a price chooser is
    MS_EINVAL with a message, and nothing is launched."""
    ppo = _ppo()
    lib_mod = importlib.import_module("marl-scheduling_amd._lib")
    C, A2, E, U = 64, 13, 5, 2
    D, A = 2 * C + 2, C + 1
    stride = (D + 3) & ~3
    assert nt_of(A) == 8
    torch.manual_seed(0)
    core = ppo.GroupedActorCritic(1, D, A).cuda()
    price = ppo.GroupedActorCritic(1, 4, A2).cuda()
    obs = _obs(E, U, D, stride).cuda()
    out = _offer_out(E, U, fill=77)
    u = torch.rand((2, E, U)).cuda()
    with pytest.raises(lib_mod.MarlSchedError) as err:
        ppo.offer_act_free(core, price, obs, C, 0, 0, out, uniforms=u)
    assert err.value.code == ppo.MS_EINVAL and len(ms.lib.ms_last_error()) > 0
    torch.cuda.synchronize()
    for k, v in out.items():
        assert bool((v == 77).all()), k
    # the core chooser alone is built at this shape
    act, lp = core.act(obs, U, seed=0, offset=0, uniforms=u[0].contiguous())
    _check_range(act.cpu().long(), lp.cpu(), A)
