"""Argmax acting of the aggregated agents' nets (ms_wide_act_greedy / k_wide_greedy, wide_kernels.hip): the picks
against a float64 restatement of the actor under the near-tie rule of tests/test_greedy_gpu.py, the log-prob at
k_wide_act's tolerance, the first-maximum rule at exactly equal logits (inside a thread's chunk, across the lanes of
a wave, across the waves), the action range under NaN logits, tail rows, refused shapes and run-to-run equality.

The float64 test first checks, on the CPU, that the float32 and float64 restatements alone stay inside the near-tie
cap with the seeds used (so a failure of the cap is the kernel's)."""
import ctypes as ct
import importlib

import pytest
import torch

from tests.test_greedy_gpu import _logits, check_greedy_rows
from tests.test_wide_gpu import SHAPES as ACT_SHAPES
from tests.test_wide_gpu import _group, _rows

pytestmark = pytest.mark.gpu

# (G, D, A, H): k_wide_act's test shapes, plus one action per thread (256) and one thread with two (257)
SHAPES = ACT_SHAPES + [(1, 8, 256, 32), (1, 8, 257, 32)]
# rows per group: not a multiple of the 16-row tile; and once each a single row, a full tile, a tile and a row
CASES = [(s, 417) for s in SHAPES] + [(SHAPES[0], 1), (SHAPES[0], 16), (SHAPES[0], 17)]
W_SEED, X_SEED = 1, 2
EPS = 1.1920928955078125e-07  # torch.finfo(float32).eps: the probability clamp of k_wide_act
KEYS = ("w1", "b1", "w2", "b2", "w3", "b3")


def _ppo():
    return importlib.import_module("marl-scheduling_amd.ppo")


def _cpu_weights(G, D, A, H):
    """The actor weights _group(G, D, A, H, W_SEED) starts from, made on the CPU (PPOGroup builds its policy with
    this constructor on torch's CPU generator)."""
    torch.manual_seed(W_SEED)
    net = _ppo().GroupedActorCritic(G, D, A, H)
    return {k: getattr(net, k).detach().clone() for k in KEYS}


def _restate(w, x, D):
    """(l64, l32) [G * R, A]: the logits of rows x [R, G, stride], group by group."""
    G = x.shape[1]
    l64 = torch.cat([_logits(w, g, x[:, g, :D], torch.float64) for g in range(G)])
    l32 = torch.cat([_logits(w, g, x[:, g, :D], torch.float32) for g in range(G)])
    return l64, l32


@pytest.mark.parametrize("shape,R", CASES)
def test_greedy_matches_float64_argmax(ms, shape, R):
    G, D, A, H = shape
    # before any launch, on the CPU: the restatements alone (the f32 one's own argmax as the action) pass the rule,
    # cap included, with these seeds; a failure of the cap below is then the kernel's
    w = _cpu_weights(G, D, A, H)
    x = _rows(R, G, D, X_SEED)
    l64, l32 = _restate(w, x, D)
    check_greedy_rows(l32.argmax(-1), l64, l32, "restatement %s x %d:" % (shape, R))
    grp = _group(G, D, A, H, W_SEED)
    for k, v in w.items():
        assert torch.equal(v, getattr(grp.policy_old, k).detach().cpu()), k
    a, lp = grp.wide_act_greedy(x.cuda())
    assert a.shape == (R, G) and a.dtype == torch.int32 and lp.shape == (R, G) and lp.dtype == torch.float32
    a, lp = a.cpu().long(), lp.cpu()
    assert int(a.min()) >= 0 and int(a.max()) < A
    act = a.T.reshape(-1)  # group-major, as _restate's rows
    check_greedy_rows(act, l64, l32, "shape %s x %d:" % (shape, R))
    p = torch.softmax(l64, -1).gather(1, act.view(-1, 1)).squeeze(1)
    want = torch.log(p.clamp(EPS, 1.0 - EPS))
    err = float((lp.T.reshape(-1).double() - want).abs().max())
    print("log-prob max abs error %.3g" % err)
    assert err < 2e-5
    # without the log-prob: the same actions, a given tensor left as it was
    keep = torch.full((R, G), -7.5, dtype=torch.float32, device="cuda")
    a2, lp2 = grp.wide_act_greedy(x.cuda(), logprob=keep, want_logprob=False)
    assert torch.equal(a2.cpu().long(), a) and lp2 is keep
    assert torch.equal(keep.cpu(), torch.full((R, G), -7.5))
    assert grp.wide_act_greedy(x.cuda(), want_logprob=False)[1] is None


def _tied_group(A, hot, H=32, G=2, D=8):
    """Every logit exactly -1 except exactly 1 at the actions in `hot` (w3 = 0, so the logit is b3)."""
    grp = _group(G, D, A, H, W_SEED)
    with torch.no_grad():
        grp.policy.w3.zero_()
        grp.policy.b3.fill_(-1.0)
        for i in hot:
            grp.policy.b3[:, i] = 1.0
    grp.sync_old()
    return grp


# A = 3000: 12 actions a thread, 768 a wave; A = 257: two a thread (threads from 129 on hold none); A = 256: one
TIES = [(3000, 5, 7, "one thread's chunk"), (3000, 5, 100, "two lanes of a wave"), (3000, 5, 2999, "two waves"),
        (3000, 767, 768, "the last lane of a wave and the first of the next"), (3000, 2998, 2999, "the last chunk"),
        (257, 2, 3, "one thread's chunk"), (257, 2, 100, "two lanes of a wave"), (257, 2, 256, "two waves"),
        (256, 3, 40, "two lanes of a wave"), (256, 3, 255, "two waves"), (25, 4, 24, "two lanes, most threads empty")]


@pytest.mark.parametrize("A,i,j,where", TIES)
def test_first_maximum_at_exactly_equal_logits(ms, A, i, j, where):
    grp = _tied_group(A, (i, j))
    x = _rows(37, 2, 8, X_SEED).cuda()
    a, lp = grp.wide_act_greedy(x)
    assert torch.equal(a.cpu(), torch.full((37, 2), i, dtype=torch.int32)), where
    # p = e^2 / (2 e^2 + (A - 2))
    want = torch.log(torch.tensor(1.0, dtype=torch.float64) / (2.0 + (A - 2) * torch.exp(torch.tensor(-2.0).double())))
    assert float((lp.cpu().double() - want).abs().max()) < 2e-5


@pytest.mark.parametrize("A", [9, 256, 257, 3000])
def test_all_logits_equal_gives_action_zero(ms, A):
    grp = _tied_group(A, ())
    a, _ = grp.wide_act_greedy(_rows(37, 2, 8, X_SEED).cuda())
    assert torch.equal(a.cpu(), torch.zeros((37, 2), dtype=torch.int32))


@pytest.mark.parametrize("A", [9, 25, 256, 257, 3000])
@pytest.mark.parametrize("nan_all", [False, True])
def test_actions_stay_in_range_under_nan_logits(ms, A, nan_all):
    grp = _group(2, 8, A, 32, W_SEED)
    with torch.no_grad():
        if nan_all:
            grp.policy.b3.fill_(float("nan"))
        else:
            grp.policy.b3[:, 0] = float("nan")
    grp.sync_old()
    a, _ = grp.wide_act_greedy(_rows(37, 2, 8, X_SEED).cuda())
    a = a.cpu()
    assert int(a.min()) >= 0 and int(a.max()) < A
    a2, lp2 = grp.wide_act_greedy(_rows(37, 2, 8, X_SEED).cuda(), want_logprob=False)
    assert torch.equal(a2.cpu(), a) and lp2 is None


@pytest.mark.parametrize("shape", [(2, 22, 25, 32), (3, 37, 700, 64), (2, 50, 3000, 32)])
def test_two_calls_give_equal_bytes(ms, shape):
    G, D, A, H = shape
    grp = _group(G, D, A, H, W_SEED)
    x = _rows(417, G, D, X_SEED).cuda()
    a1, lp1 = grp.wide_act_greedy(x)
    a2, lp2 = grp.wide_act_greedy(x)
    assert torch.equal(a1.view(torch.uint8), a2.view(torch.uint8))
    assert torch.equal(lp1.view(torch.uint8), lp2.view(torch.uint8))


def test_rows_beyond_n_rows_are_not_written(ms):
    """The C call on n_rows = 21 (a tile and five rows) with room for 32: the last tile's other rows keep their bytes."""
    G, D, A, H = 2, 22, 25, 32
    grp = _group(G, D, A, H, W_SEED)
    x = _rows(32, G, D, X_SEED).cuda()
    act = torch.full((32, G), -7, dtype=torch.int32, device="cuda")
    lp = torch.full((32, G), -7.5, dtype=torch.float32, device="cuda")
    ptr = lambda t: ct.c_void_p(t.data_ptr())
    rc = ms.lib.ms_wide_act_greedy(ct.byref(grp.policy_old.mlp_params()), ptr(x), x.shape[2], 21, ptr(act), ptr(lp),
                                   ct.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0
    want_a, want_lp = grp.wide_act_greedy(x[:21].contiguous())
    assert torch.equal(act[:21], want_a) and torch.equal(lp[:21], want_lp)
    assert bool((act[21:] == -7).all()) and bool((lp[21:] == -7.5).all())


def test_shapes_the_sampling_launcher_refuses_are_refused(ms):
    grp = _group(2, 8, 9, 32, W_SEED)
    x = _rows(5, 2, 8, X_SEED).cuda()
    act = torch.full((5, 2), -7, dtype=torch.int32, device="cuda")
    ptr = lambda t: ct.c_void_p(t.data_ptr())
    u = torch.rand((5, 2), device="cuda")
    lp = torch.zeros((5, 2), device="cuda")
    for field, value in (("hidden", 16), ("hidden", 48), ("in_dim", 256), ("n_actions", 0)):
        p = grp.policy_old.mlp_params()
        setattr(p, field, value)
        rc_sample = ms.lib.ms_wide_act(ct.byref(p), ptr(x), 8, 5, ptr(u), ptr(act), ptr(lp), None)
        rc = ms.lib.ms_wide_act_greedy(ct.byref(p), ptr(x), 8, 5, ptr(act), None, None)
        assert rc == rc_sample != 0, (field, value)
    p = grp.policy_old.mlp_params()
    for stride, rows in ((6, 5), (4, 5), (8, 0)):  # not a multiple of 4, below in_dim, no rows
        assert ms.lib.ms_wide_act_greedy(ct.byref(p), ptr(x), stride, rows, ptr(act), None, None) != 0
    assert ms.lib.ms_wide_act_greedy(ct.byref(p), ptr(x), 8, 5, None, None, None) != 0
    torch.cuda.synchronize()
    assert bool((act == -7).all())  # nothing was launched
