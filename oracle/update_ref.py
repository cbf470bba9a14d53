"""Float64 references of the update path's two elementwise halves: the normalised Monte-Carlo returns
(PPOmodules.py:128-137; ms_discounted_returns, ms_unit_returns) and one Adam step (torch.optim.Adam's foreach
step; ms_adam_step, ms_adam_step_dev, ms_adam_step_dev_masked), with the error bounds a correct f32 kernel
stays inside, and numpy restatements of the kernels' own operation order that show on the CPU that the bounds
can be met (tests/test_update_ref.py). Plain numpy: no torch, no device.
"""
from __future__ import annotations

import math

import numpy as np

EPS32 = 2.0 ** -24  # unit roundoff of f32

# |reward| up to which ms_unit_returns' one-pass variance keeps returns_bound (include/marlsched.h): the largest
# power of two at which returns_emul holds it at every gamma of tests/test_update_ref.py (there: how it was found)
UNIT_RETURNS_MAX_ABS_REWARD = 2.0 ** 22


def bound_ratio(err, bound):
    """max err / bound over the arrays; a zero bound asks for a zero error (inf otherwise), a NaN error gives NaN,
    which no comparison accepts."""
    err, bound = np.asarray(err, dtype=np.float64), np.asarray(bound, dtype=np.float64)
    pos = bound > 0
    r = np.where(pos, err / np.where(pos, bound, 1.0), np.where(err == 0, 0.0, np.where(np.isnan(err), np.nan, np.inf)))
    return float(np.max(r)) if r.size else 0.0


# ---------------------------------------------------------------------------------------------- returns

def returns_ref(rewards_1d, gamma):
    """One sequence. The scan in Python floats as PPO.update runs it (g = r + gamma*g from the last round
    back), each value rounded to f32 (torch.tensor(..., dtype=float32)), then mean, unbiased std and
    (f - mean) / (std + 1e-7) in float64 on those f32 values. Returns (normalised [T] f64, mean64, sd64);
    T == 1 has no unbiased std: sd64 and every value are NaN, as torch's std() of one sample gives."""
    g = 0
    out = []
    for r in reversed([x.item() if hasattr(x, "item") else x for x in rewards_1d]):
        g = r + (gamma * g)
        out.append(g)
    f = np.array(out[::-1], dtype=np.float64).astype(np.float32).astype(np.float64)
    T = f.shape[0]
    mean64 = float(f.sum() / T)
    sd64 = math.sqrt(float(((f - mean64) ** 2).sum()) / (T - 1)) if T > 1 else float("nan")
    return (f - mean64) / (sd64 + 1e-7), mean64, sd64


def returns_scan(rewards_tm, gamma):
    """The f32 values of the scan for many sequences at once: rewards [T, ...] -> [T, ...] f32. numpy's
    float64 multiply and add are the two roundings of Python's r + gamma*g."""
    r = np.asarray(rewards_tm).astype(np.float64)
    f = np.empty(r.shape, dtype=np.float32)
    g = np.zeros(r.shape[1:], dtype=np.float64)
    gm = np.float64(gamma)
    for t in range(r.shape[0] - 1, -1, -1):
        g = r[t] + gm * g
        f[t] = g.astype(np.float32)
    return f


def returns_ref_many(rewards_tm, gamma):
    """returns_ref of every sequence of rewards [T, ...] (time first): (normalised [T, ...] f64, mean64 [...],
    sd64 [...]). The same numbers as returns_ref column by column up to the order of the float64 sums."""
    f = returns_scan(rewards_tm, gamma).astype(np.float64)
    T = f.shape[0]
    mean64 = f.sum(axis=0) / T
    with np.errstate(invalid="ignore", divide="ignore"):
        sd64 = np.sqrt(((f - mean64) ** 2).sum(axis=0) / (T - 1)) if T > 1 else np.full(f.shape[1:], np.nan)
        return (f - mean64) / (sd64 + 1e-7), mean64, sd64


def returns_bound(ref, mean64, sd64):
    """|got - ref| of a correct f32 kernel: the subtraction, the division and the f32 std + 1e-7 round once each
    (3 roundings relative to the value), and the mean is rounded to f32 before it is subtracted, which moves
    every value by up to eps*|mean| / (sd + 1e-7) / 2 (torch's f32 mean does the same). Factor 2 on both."""
    return 2 * EPS32 * (3 * np.abs(ref) + 0.5 * np.abs(mean64) / (sd64 + 1e-7))


def returns_emul(rewards_tm, gamma, one_pass=True):
    """The returns kernels' arithmetic restated in numpy for rewards [T, ...]: float64 scan, f32 values, float64
    sums taken from the last round back, f32 mean, then the sum of squared deviations either from the same
    pass's sums as ss - 2*m*s + T*m*m (one_pass: k_unit_returns, k_unit_returns_reg) or by a second pass
    (k_returns), f32 std, f32 std + 1e-7f, f32 subtraction and division. No fused multiply-add (the compiler may
    fuse some of the float64 products, which only removes roundings). Returns [T, ...] f32."""
    f = returns_scan(rewards_tm, gamma)
    T = f.shape[0]
    fd = f.astype(np.float64)
    s = np.zeros(f.shape[1:], dtype=np.float64)
    ss = np.zeros(f.shape[1:], dtype=np.float64)
    for t in range(T - 1, -1, -1):
        s = s + fd[t]
        ss = ss + fd[t] * fd[t]
    mean = (s / T).astype(np.float32)
    md = mean.astype(np.float64)
    if one_pass:
        v = ss - 2.0 * md * s + np.float64(T) * md * md
        v = np.where(v > 0.0, v, 0.0)
    else:
        v = np.zeros(f.shape[1:], dtype=np.float64)
        for t in range(T):
            d = fd[t] - md
            v = v + d * d
    with np.errstate(invalid="ignore", divide="ignore"):
        sd = np.sqrt(v / (T - 1)).astype(np.float32) if T > 1 else np.full(f.shape[1:], np.nan, dtype=np.float32)
        den = sd + np.float32(1e-7)
        return (f - mean) / den


def returns_families(T, M, seed, mag, limit=UNIT_RETURNS_MAX_ABS_REWARD):
    """The reward sequences the returns tests share, {name: [T, M] int64}, every value an integer below 2^31 (the
    tests feed them as int32, as f32, or halved as f32): random small integers; all zero; a constant; one
    non-zero reward in the first round, one in the last; `mag` minus 0 or 1 at random (a large offset under a
    variance of 1/4); the same at `limit`."""
    rng = np.random.default_rng(seed)
    first = np.zeros((T, M), dtype=np.int64)
    first[0] = rng.integers(1, 13, M)
    last = np.zeros((T, M), dtype=np.int64)
    last[T - 1] = rng.integers(1, 13, M)
    return dict(
        small=rng.integers(-20, 30, (T, M)),
        zero=np.zeros((T, M), dtype=np.int64),
        const=np.broadcast_to(rng.integers(1, 13, M), (T, M)).copy(),
        first=first,
        last=last,
        offset=int(mag) - rng.integers(0, 2, (T, M)),
        limit=int(limit) - rng.integers(0, 2, (T, M)),
    )


# ------------------------------------------------------------------------------------------------- Adam

def adam_scalars(lr, step, betas=(0.9, 0.999), eps=1e-8):
    """The scalars torch.optim.Adam's foreach step hands to its f32 ops, each rounded to f32, as float64:
    dict(w1 = 1 - beta1, beta2, one_m_beta2, eps, ns = -(lr / bc1), bc2_sqrt). bc1, bc2 in Python floats."""
    b1, b2 = float(betas[0]), float(betas[1])
    bc1 = 1.0 - b1 ** step
    bc2 = 1.0 - b2 ** step
    f32 = lambda x: float(np.float32(x))
    return dict(w1=f32(1.0 - b1), beta2=f32(b2), one_m_beta2=f32(1.0 - b2), eps=f32(eps),
                ns=f32((lr / bc1) * -1.0), bc2_sqrt=f32(math.sqrt(bc2)))


def adam_ref(p, g, m, v, lr, step, betas=(0.9, 0.999), eps=1e-8):
    """Step number `step` (>= 1) in float64 from the f32 state before it (p, g, m, v: arrays of one shape; call
    it again with the kernel's own f32 state for the next step, so nothing drifts). Returns (m64, v64, den64,
    u64, p64): the new moments, sqrt(v64) / sqrt(bc2) + eps, the update ns * m64 / den64, and p + u64."""
    k = adam_scalars(lr, step, betas, eps)
    p, g, m, v = (np.asarray(x).astype(np.float64) for x in (p, g, m, v))
    m64 = m + k["w1"] * (g - m)
    v64 = v * k["beta2"] + k["one_m_beta2"] * (g * g)
    den64 = np.sqrt(v64) / k["bc2_sqrt"] + k["eps"]
    u64 = k["ns"] * m64 / den64
    return m64, v64, den64, u64, p + u64


def adam_bounds(p, g, m, v, lr, step, betas=(0.9, 0.999), eps=1e-8):
    """(bound_m, bound_v, bound_p) on |kernel - adam_ref| of a correct f32 kernel, each twice its rounding count.
    m: g - m and the lerp's product and sum round relative to at most |m_old| + |g| (2 roundings). v: the two
    products and the sum (for |g| >= 1e-15 or 0, so that g*g is a normal f32 or exactly 0; 2 roundings relative to
    v64). p: the final sum rounds relative to p64, the update carries sqrt, the two divisions, the + eps and the
    product (4 roundings relative to u64, v's error entering at half weight under the root), and m's error
    comes through scaled by |ns| / den64."""
    k = adam_scalars(lr, step, betas, eps)
    m64, v64, den64, u64, p64 = adam_ref(p, g, m, v, lr, step, betas, eps)
    mg = np.abs(np.asarray(m).astype(np.float64)) + np.abs(np.asarray(g).astype(np.float64))
    bm = 4 * EPS32 * mg
    bv = 4 * EPS32 * np.abs(v64)
    bp = 2 * EPS32 * np.abs(p64) + 8 * EPS32 * np.abs(u64) + abs(k["ns"]) * 4 * EPS32 * mg / den64
    return bm, bv, bp


def adam_emul(p, g, m, v, lr, step, betas=(0.9, 0.999), eps=1e-8, fma=False):
    """k_adam's statements in numpy f32, one rounding per operation: m += w1 * (g - m); v *= beta2;
    v += one_m_beta2 * (g * g); den = sqrt(v) / bc2_sqrt + eps; p += ns * (m / den). fma: the three
    multiply-adds each round once (the product exact in float64, the sum rounded to f32), which is what the
    compiler makes of them. Returns (p, m, v) f32."""
    k = {n: np.float32(x) for n, x in adam_scalars(lr, step, betas, eps).items()}
    p, g, m, v = (np.asarray(x).astype(np.float32) for x in (p, g, m, v))

    def muladd(a, b, c):
        if fma:
            return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)
        return (a * b).astype(np.float32) + c

    with np.errstate(over="ignore", invalid="ignore", divide="ignore", under="ignore"):
        m = muladd(k["w1"], g - m, m)
        v = v * k["beta2"]
        v = muladd(k["one_m_beta2"], g * g, v)
        den = np.sqrt(v) / k["bc2_sqrt"] + k["eps"]
        p = muladd(k["ns"], m / den, p)
    return p.astype(np.float32), m.astype(np.float32), v.astype(np.float32)


ADAM_STEPS = (1, 2, 7, 1000, 100000, 10 ** 7)
ADAM_SCALES = (1e-12, 1e-9, 1e-6, 1e-3, 1.0, 1e3)


def adam_case(n, seed, scale):
    """The Adam inputs the tests share, (p, g, m, v) f32 of n elements: gradients of size `scale` (a number, or n
    of them), none smaller than 1e-15 (so g*g is a normal f32), a tenth of the elements with an exactly zero
    gradient and zero moments, the other moments what earlier gradients of that size leave. The last element
    is never one of the zeros."""
    rng = np.random.default_rng(seed)
    scale = np.broadcast_to(np.asarray(scale, dtype=np.float64), (n,))
    p = rng.standard_normal(n).astype(np.float32)
    sign = np.where(rng.random(n) < 0.5, -1.0, 1.0)
    g = (sign * np.maximum(np.abs(rng.standard_normal(n)) * scale, 1e-15)).astype(np.float32)
    m = (rng.standard_normal(n) * scale * 0.5).astype(np.float32)
    v = ((rng.standard_normal(n) * scale) ** 2 * rng.random(n)).astype(np.float32)
    v = np.where(v < 1e-30, np.float32(0), v).astype(np.float32)
    zero = rng.random(n) < 0.1
    zero[n - 1] = False
    for x in (g, m, v):
        x[zero] = 0
    return p, g, m, v
