"""ms_policy_evaluate (GroupedActorCritic.evaluate_hip): log-prob of a given action, state value and entropy
against a float64 CPU restatement of ActorCritic.evaluate (PPOmodules.py:65-72), both probability clamps,
agreement with the log-probs ms_policy_act writes, the optional outputs and the argument checks.

The bound of every comparison with float64 is derived per shape and per output: 8 x the largest
|f32 CPU restatement - float64| over the rows (the greedy test's rule and factor: the MFMA's other accumulation
order and fast_tanh_b's ~1e-7 absolute error)."""
import ctypes as ct
import functools
import importlib
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

# (G, per_group, D, stride, A): tests/test_greedy_gpu.py's list, then A on a tile edge and one past it
SHAPES = [(8, 8, 51, 52, 25), (24, 1, 18, 20, 9), (1, 16, 27, 28, 13), (8, 3, 4, 4, 13), (2, 5, 195, 196, 97),
          (3, 2, 11, 12, 5), (1, 1, 11, 12, 16), (2, 3, 27, 28, 17)]
EPS = float(torch.finfo(torch.float32).eps)
OUTPUTS = ("logprob", "value", "entropy")


def _ppo():
    return importlib.import_module("marl-scheduling_amd.ppo")


def _mlp(p, x):
    h = torch.tanh(x @ p[0].T + p[1])
    h = torch.tanh(h @ p[2].T + p[3])
    return h @ p[4].T + p[5]


def _restate(ppo, w, obs, acts, G, per_group, D, dtype):
    """ActorCritic.evaluate on the CPU in dtype: (logprob, value, entropy, p[a]) each [E, U]."""
    E, U = acts.shape
    out = [torch.empty((E, U), dtype=dtype) for _ in range(4)]
    for g in range(G):
        cols = slice(g * per_group, (g + 1) * per_group)
        x = obs[:, cols, :D].reshape(-1, D).to(dtype)
        a = acts[:, cols].reshape(-1, 1).long()
        p = torch.softmax(_mlp([w[k][g].to(dtype) for k in ppo.ACTOR_KEYS], x), -1)
        p = p / p.sum(-1, keepdim=True)  # Categorical(probs)
        logp = torch.log(p.clamp(EPS, 1 - EPS))  # Categorical.logits
        v = _mlp([w[k][g].to(dtype) for k in ppo.CRITIC_KEYS], x).squeeze(-1)
        for o, val in zip(out, (logp.gather(1, a).squeeze(1), v, -(logp * p).sum(-1), p.gather(1, a).squeeze(1))):
            o[:, cols] = val.view(E, per_group)
    return out


@functools.lru_cache(maxsize=None)
def _case(shape, E, scale):
    """One shape's net, inputs, float64 reference and bounds, computed once and shared by the tests."""
    G, per_group, D, stride, A = shape
    ppo = _ppo()
    torch.manual_seed(0)
    net = ppo.GroupedActorCritic(G, D, A)
    with torch.no_grad():
        net.w3.mul_(scale)
        net.b3.mul_(scale)
    w = {k: getattr(net, k).detach().clone() for k in ppo.ACTOR_KEYS + ppo.CRITIC_KEYS}
    U = G * per_group
    gen = torch.Generator().manual_seed(1)
    obs = torch.zeros((E, U, stride), dtype=torch.int8)
    obs[..., :D] = torch.randint(-5, 13, (E, U, D), generator=gen, dtype=torch.int8)
    acts = torch.randint(0, A, (E, U), generator=gen, dtype=torch.int8)
    r64 = _restate(ppo, w, obs, acts, G, per_group, D, torch.float64)
    r32 = _restate(ppo, w, obs, acts, G, per_group, D, torch.float32)
    bound = {n: 8.0 * float((r32[i].double() - r64[i]).abs().max()) for i, n in enumerate(OUTPUTS)}
    return dict(net=net.cuda(), obs=obs.cuda(), acts=acts.cuda(), U=U, ref=dict(zip(OUTPUTS, r64[:3])), pa=r64[3],
                bound=bound)


def _check_against_float64(c, what):
    got = dict(zip(OUTPUTS, c["net"].evaluate_hip(c["obs"], c["acts"], c["U"])))
    for n in OUTPUTS:
        g = got[n].cpu()
        assert bool(torch.isfinite(g).all()), n
        err = float((g.double() - c["ref"][n]).abs().max())
        print("%s %s: bound %.3g, largest error %.3g" % (what, n, c["bound"][n], err))
    for n in OUTPUTS:
        assert float((got[n].cpu().double() - c["ref"][n]).abs().max()) <= c["bound"][n], n
    return got


@pytest.mark.parametrize("shape,E", [(s, 333) for s in SHAPES] + [(SHAPES[0], 1)])
def test_matches_float64(ms, shape, E):
    c = _case(shape, E, 1.0)
    # at this scale no row touches either clamp
    assert float(c["pa"].min()) > EPS and float(c["pa"].max()) < 1 - EPS
    _check_against_float64(c, "shape %s E %d" % (shape, E))


@pytest.mark.parametrize("shape", SHAPES)
def test_both_clamps(ms, shape):
    """w3 and b3 times 64: the taken action's probability is below eps on most rows and above 1 - eps on some."""
    c = _case(shape, 333, 64.0)
    low, high = c["pa"] < EPS, c["pa"] > 1 - EPS
    print("shape %s: p[a] < eps on %.1f %% of the rows, > 1 - eps on %.1f %%" %
          (shape, 100 * float(low.double().mean()), 100 * float(high.double().mean())))
    assert int(low.sum()) > 0 and int(high.sum()) > 0
    got = _check_against_float64(c, "shape %s x64" % (shape,))
    lp = got["logprob"].cpu().double()
    deep = c["pa"] < EPS / 2
    assert int(deep.sum()) > 0
    assert float((lp[deep] - math.log(EPS)).abs().max()) <= c["bound"]["logprob"]


@pytest.mark.parametrize("shape", [SHAPES[0], SHAPES[7]])
def test_reproduces_the_acting_logprobs(ms, shape):
    """evaluate_hip on the rows and actions ms_policy_act sampled gives the log-probs it wrote."""
    c = _case(shape, 333, 1.0)
    act, lp_act = c["net"].act(c["obs"], c["U"], seed=11, offset=5)
    lp, _, _ = c["net"].evaluate_hip(c["obs"], act, c["U"], want=("logprob",))
    diff = (lp.double() - lp_act.double()).abs()
    print("shape %s: bound %.3g, largest |evaluate - act| %.3g, bit-equal rows %d of %d" %
          (shape, c["bound"]["logprob"], float(diff.max()), int((lp == lp_act).sum()), lp.numel()))
    assert float(diff.max()) <= c["bound"]["logprob"]


def test_each_output_alone_equals_all_three(ms):
    c = _case(SHAPES[0], 333, 1.0)
    net, obs, acts, U = c["net"], c["obs"], c["acts"], c["U"]
    full = dict(zip(OUTPUTS, net.evaluate_hip(obs, acts, U)))
    for i, n in enumerate(OUTPUTS):
        alone = net.evaluate_hip(obs, acts if n == "logprob" else None, U, want=(n,))
        assert all(alone[j] is None for j in range(3) if j != i)
        assert torch.equal(alone[i], full[n]), n


def test_critic_is_optional_without_value(ms):
    ppo = _ppo()
    c = _case(SHAPES[5], 333, 1.0)
    net, obs, acts, U = c["net"], c["obs"], c["acts"], c["U"]
    E, _, stride = obs.shape
    full = net.evaluate_hip(obs, acts, U)
    lp = torch.empty((E, U), dtype=torch.float32, device="cuda")
    ent = torch.empty_like(lp)
    p = net.mlp_params()
    ms.check(ms.lib.ms_policy_evaluate(ct.byref(p), None, ppo.ptr(obs), stride, E, U, U // net.G, ppo.ptr(acts),
                                       ppo.ptr(lp), None, ppo.ptr(ent), None))
    assert torch.equal(lp, full[0]) and torch.equal(ent, full[2])


def test_invalid_arguments_launch_nothing(ms):
    """Every MS_EINVAL case returns with a message and leaves the outputs and the canaries around them alone."""
    ppo = _ppo()
    lib, ptr = ms.lib, ppo.ptr
    c = _case(SHAPES[5], 333, 1.0)
    net, obs, acts, U = c["net"], c["obs"], c["acts"], c["U"]
    E, _, stride = obs.shape
    n = E * U
    guard = torch.full((5 * n,), 7.0, device="cuda")  # [canary][logprob][value][entropy][canary]
    lp, val, ent = guard[n:2 * n], guard[2 * n:3 * n], guard[3 * n:4 * n]

    def call(p=None, cr=None, stride_=stride, per_group=U // net.G, acts_=acts, lp_=lp, val_=val, ent_=ent,
             with_critic=True):
        p = net.mlp_params() if p is None else p
        cr = net.critic_mlp_params() if cr is None else cr
        return lib.ms_policy_evaluate(ct.byref(p), ct.byref(cr) if with_critic else None, ptr(obs), stride_, E, U,
                                      per_group, ptr(acts_) if acts_ is not None else None, ptr(lp_) if lp_ is not None
                                      else None, ptr(val_) if val_ is not None else None, ptr(ent_), None)

    def bad(**kw):
        p, cr = net.mlp_params(), net.critic_mlp_params()
        for k, v in kw.items():
            setattr(p if k[0] == "a" else cr, k[2:], v)
        return dict(p=p, cr=cr)

    cases = dict(
        hidden=bad(a_hidden=32), critic_hidden=bad(c_hidden=32), actions_128=bad(a_n_actions=128),
        stride_over_256=dict(stride_=260), stride_not_dwords=dict(stride_=stride + 2),
        units=dict(per_group=U // net.G + 1), critic_in_dim=bad(c_in_dim=net.D - 1),
        critic_groups=bad(c_n_groups=net.G + 1), logprob_without_actions=dict(acts_=None),
        value_without_critic=dict(with_critic=False))
    for name, kw in cases.items():
        rc = call(**kw)
        assert rc == ppo.MS_EINVAL, name
        assert len(lib.ms_last_error()) > 0, name
    torch.cuda.synchronize()
    assert bool((guard == 7.0).all())
    assert call() == 0  # the same call with nothing wrong writes the three outputs, and only them
    torch.cuda.synchronize()
    assert bool((guard[:n] == 7.0).all()) and bool((guard[4 * n:] == 7.0).all())
    full = net.evaluate_hip(obs, acts, U)
    assert all(torch.equal(a, b.view(-1)) for a, b in zip((lp, val, ent), full))


def test_action_outside_the_range_gives_nan_logprob(ms):
    """An action byte outside [0, A) is compared, never used as an index: that row's logprob is NaN, its value and
    entropy and every other row are what they are without it, bit for bit."""
    c = _case(SHAPES[7], 333, 1.0)
    net, obs, U = c["net"], c["obs"], c["U"]
    A = net.A
    full = net.evaluate_hip(obs, c["acts"], U)
    acts = c["acts"].clone()
    flat = acts.view(-1)
    where = torch.tensor([0, 5, 17, flat.numel() - 1], device="cuda")
    flat[where] = torch.tensor([A, 127, -1, -128], dtype=torch.int8, device="cuda")
    lp, v, ent = net.evaluate_hip(obs, acts, U)
    torch.cuda.synchronize()
    mask = torch.zeros_like(flat, dtype=torch.bool)
    mask[where] = True
    assert bool(torch.isnan(lp.view(-1)[mask]).all())
    assert torch.equal(lp.view(-1)[~mask], full[0].view(-1)[~mask])
    assert torch.equal(v, full[1]) and torch.equal(ent, full[2])
