"""The float64 references of the returns and Adam kernels (oracle/update_ref.py) against the references the suite
already trusts (RefPPO.returns, torch.optim.Adam on the CPU), and the numpy restatements of the kernels' operation
order against the error bounds the device tests (tests/test_returns_adam_gpu.py) hold the kernels to: the
bounds can be met by a correct f32 kernel, and the magnitude limit of the one-pass variance is where they stop
being met."""
import math

import numpy as np
import pytest
import torch

from oracle import update_ref as ur
from oracle.ppo_ref import RefPPO

# gamma of the named configs (trainer.py: acceptor -((1 - maxLen) / maxLen) + 0.04 with maxLen 6 for cfg1, cfg2, cfg4
# and cfg5, 0.95 for cfg3; every offer unit 0.5) between the two ends of the range
GAMMAS = (0.0, 0.5, -((1 - 6) / 6) + 0.04, 0.95, 1.0)
LENGTHS = (1, 2, 15, 16, 17, 31, 32, 33, 199, 200, 201)
# the largest per-round reward of the named configs: reward_multiplier (1) times the highest job priority (12,
# abi.EXP4_JOBS; 10 in abi.README_JOBS), paid to the acceptor unit that owns the core when the job ends
MAG = 12


_ratio = ur.bound_ratio


@pytest.mark.parametrize("T", LENGTHS)
def test_returns_ref_matches_ref_ppo(T):
    """returns_ref against RefPPO.returns (torch f32) at the tolerance of the device tests that compare with
    RefPPO, on every shared family at the rewards the env can emit. The family at the magnitude limit has no
    part in it: there torch's own f32 mean is off by up to 1/4 in a sequence whose std is 1/2 and its f32 std
    errs on top (measured: RefPPO 0.61 away from float64, 1.26 times returns_bound, at T = 15, gamma = 0), so no
    f32 computation can agree with float64 to 1e-5; the float64 reference alone judges the kernels there."""
    for gamma in GAMMAS:
        ref_ppo = RefPPO(4, 3, 0.1, 0.1, gamma, 0.2, 1)
        for name, fam in ur.returns_families(T, 3, 11 + T, MAG).items():
            if name == "limit":
                continue
            for scale in (1, 0.5):
                for m in range(fam.shape[1]):
                    seq = [int(x) * scale for x in fam[:, m]]
                    want = ref_ppo.returns(seq).numpy()
                    got, mean64, sd64 = ur.returns_ref(seq, gamma)
                    if T == 1:
                        assert np.isnan(got).all() and np.isnan(want).all() and np.isnan(sd64)
                    else:
                        np.testing.assert_allclose(got, want, rtol=1e-5, atol=2e-6, err_msg="%s %r" % (name, gamma))


@pytest.mark.parametrize("T", LENGTHS)
def test_returns_ref_many_is_returns_ref(T):
    """The vectorised reference the device tests use is the per-sequence one: the same f32 scan values bit for
    bit, the normalised values to float64 rounding (only the order of the sums differs)."""
    for gamma in GAMMAS:
        for name, fam in ur.returns_families(T, 5, 3 * T, MAG).items():
            many, mean, sd = ur.returns_ref_many(fam, gamma)
            for m in range(fam.shape[1]):
                one, mean1, sd1 = ur.returns_ref(fam[:, m], gamma)
                np.testing.assert_allclose(many[:, m], one, rtol=1e-9, atol=1e-12, err_msg=name)
                np.testing.assert_allclose([mean[m], sd[m]], [mean1, sd1], rtol=1e-12, atol=0)


@pytest.mark.parametrize("one_pass", [True, False])
@pytest.mark.parametrize("T", LENGTHS)
def test_returns_emulation_within_bound(T, one_pass, record_property):
    """A correct kernel can meet returns_bound: the restatement of either kernel's operation order does, on every
    family (the magnitude limit included), gamma and reward type, and gives exact zeros where the device tests ask
    for them. Observed: at most 0.97 of the bound (T = 201)."""
    worst = 0.0
    for gamma in GAMMAS:
        for name, fam in ur.returns_families(T, 400, 5 + T, MAG).items():
            for scale in (1, 0.5):
                r = fam * scale
                got = ur.returns_emul(r, gamma, one_pass=one_pass)
                if T == 1:
                    assert np.isnan(got).all()
                    continue
                ref, mean64, sd64 = ur.returns_ref_many(r, gamma)
                ratio = _ratio(np.abs(got.astype(np.float64) - ref), ur.returns_bound(ref, mean64, sd64))
                worst = max(worst, ratio)
                assert ratio <= 1.0, (name, gamma, scale, ratio)
                if name == "zero" or (name == "const" and gamma == 0.0):
                    assert (got == 0.0).all(), (name, gamma)
    record_property("worst_ratio", worst)
    print("T=%d one_pass=%s worst ratio %.3f" % (T, one_pass, worst))


def test_unit_returns_magnitude_limit():
    """The magnitude contract of ms_unit_returns (include/marlsched.h): |reward| <= 2^22.

    The one-pass sum of squared deviations ss - 2*m*s + T*m*m cancels three float64 numbers of about T*reward^2.
    While every partial sum of squares stays below 2^53 (integers up to 2^22 over 200 rounds: 200 * 2^44 < 2^52)
    the sums are exact and only the two products with the f32 mean round, an error of about 1 against a sum of
    deviations of T/4. One power of two further the squares no longer add exactly and the result is noise.

    Found with returns_emul on `mag - {0, 1}`, 2000 sequences per cell, every length of LENGTHS and gamma of
    GAMMAS: the worst error is 0.94 of returns_bound at each of 2^18 .. 2^22 (at T = 33, gamma = 1, which no
    cancellation touches) and 4.9e6 times the bound at 2^23 (T = 200, gamma = 0: the variance comes out as 0).
    The two-pass kernel (k_returns) has no such limit. 2^22 is 3.5e5 times the largest reward of the named
    configs."""
    lim = ur.UNIT_RETURNS_MAX_ABS_REWARD
    assert lim == 2.0 ** 22
    beyond = 0.0
    for T in LENGTHS[1:]:
        for gamma in GAMMAS:
            r = ur.returns_families(T, 2000, 7, MAG, lim)["limit"]
            ref, mean64, sd64 = ur.returns_ref_many(r, gamma)
            got = ur.returns_emul(r, gamma, one_pass=True).astype(np.float64)
            assert _ratio(np.abs(got - ref), ur.returns_bound(ref, mean64, sd64)) <= 1.0, (T, gamma)
            r2 = ur.returns_families(T, 2000, 7, MAG, 2 * lim)["limit"]
            ref2, mean2, sd2 = ur.returns_ref_many(r2, gamma)
            bound2 = ur.returns_bound(ref2, mean2, sd2)
            two = ur.returns_emul(r2, gamma, one_pass=False).astype(np.float64)
            assert _ratio(np.abs(two - ref2), bound2) <= 1.0, (T, gamma)
            one = ur.returns_emul(r2, gamma, one_pass=True).astype(np.float64)
            beyond = max(beyond, _ratio(np.abs(one - ref2), bound2))
    assert beyond > 1.0  # the limit is not a loose one: twice as far the one-pass formula leaves the bound


def test_adam_ref_matches_torch_adam():
    """adam_ref, re-synced to torch's f32 state before every step, against torch.optim.Adam on the CPU with the
    actor / critic learning-rate groups of PPO.__init__ (PPOmodules.py:100-105), steps 1..8, at the tolerance
    test_hip_adam_matches_torch_adam holds the device step to."""
    gen = torch.Generator().manual_seed(3)
    shapes = [(8, 16, 51), (8, 16), (8, 25, 16), (8, 1, 16), (8, 1)]
    ps = [torch.randn(s, generator=gen).requires_grad_(True) for s in shapes]
    lrs = [0.003] * 3 + [0.01] * 2
    opt = torch.optim.Adam([{"params": ps[:3], "lr": 0.003}, {"params": ps[3:], "lr": 0.01}])
    for step in range(1, 9):
        before = []
        for p, s in zip(ps, shapes):
            p.grad = torch.randn(s, generator=gen) * (10.0 ** (step - 4))
            st = opt.state.get(p, {})
            m = st["exp_avg"].numpy().copy() if st else np.zeros(s, dtype=np.float32)
            v = st["exp_avg_sq"].numpy().copy() if st else np.zeros(s, dtype=np.float32)
            before.append((p.detach().numpy().copy(), p.grad.numpy().copy(), m, v))
        opt.step()
        for p, lr, (p0, g, m0, v0) in zip(ps, lrs, before):
            m64, v64, den64, u64, p64 = ur.adam_ref(p0, g, m0, v0, lr, step)
            np.testing.assert_allclose(p.detach().numpy(), p64, rtol=2e-6, atol=1e-7, err_msg="step %d" % step)
            np.testing.assert_allclose(opt.state[p]["exp_avg_sq"].numpy(), v64, rtol=2e-6, atol=0)
            # the first moment cancels (m + w * (g - m)): no relative tolerance fits it, its derived bound does
            bm = ur.adam_bounds(p0, g, m0, v0, lr, step)[0]
            assert (np.abs(opt.state[p]["exp_avg"].numpy() - m64) <= bm).all()


ADAM_STEPS, ADAM_SCALES, adam_case = ur.ADAM_STEPS, ur.ADAM_SCALES, ur.adam_case


@pytest.mark.parametrize("fma", [False, True])
def test_adam_emulation_within_bounds(fma):
    """A correct kernel can meet adam_bounds: k_adam's statements in numpy f32, with and without fused
    multiply-adds, do at every step count and gradient scale of the device tests, and leave elements with a zero
    gradient and zero moments exactly where they were. Observed: at most 0.7 of a bound."""
    worst = [0.0, 0.0, 0.0]
    for step in ADAM_STEPS:
        for i, scale in enumerate(ADAM_SCALES):
            for lr in (0.003, 0.01, 1e-4):
                p, g, m, v = adam_case(4096, 100 * i + step % 97, scale)
                p1, m1, v1 = ur.adam_emul(p, g, m, v, lr, step, fma=fma)
                m64, v64, den64, u64, p64 = ur.adam_ref(p, g, m, v, lr, step)
                for k, (got, ref, b) in enumerate(zip((m1, v1, p1), (m64, v64, p64),
                                                      ur.adam_bounds(p, g, m, v, lr, step))):
                    ratio = _ratio(np.abs(got.astype(np.float64) - ref), b)
                    worst[k] = max(worst[k], ratio)
                    assert ratio <= 1.0, ("mvp"[k], step, scale, lr, ratio)
                still = (g == 0) & (m == 0) & (v == 0)
                assert still.any() and (p1[still] == p[still]).all() and (m1[still] == 0).all()
                assert np.isfinite(p1).all()
    print("fma=%s worst ratios m %.3f v %.3f p %.3f" % (fma, *worst))


def test_adam_scalars_at_large_steps():
    """At step 10^7 both beta^step underflow to 0 in float64 and the corrections are exactly 1."""
    k = ur.adam_scalars(0.003, 10 ** 7)
    assert k["bc2_sqrt"] == 1.0 and k["ns"] == -float(np.float32(0.003))
    k1 = ur.adam_scalars(0.003, 1)
    assert k1["ns"] == float(np.float32(-(0.003 / (1.0 - 0.9)))) and k1["bc2_sqrt"] == float(np.float32(math.sqrt(1.0 - 0.999)))
