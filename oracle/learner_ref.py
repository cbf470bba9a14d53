"""Float64 references of the two learners outside PPO: BranchingDQN.update_policy (BranchingDQNModules.py:125-164;
ms_bdqn_update) and the DQN unit's optimize_model and selectAction (DQNmodules.py:56-70, 97-154; ms_dqn_grad,
ms_dqn_act), the Philox4x32-10 stream ms_dqn_act draws from, and the case tables the CPU and GPU tests share
(tests/test_learner_ref.py, tests/test_learner_parity_gpu.py). numpy float64 for the references, torch only for
the autograd cross-checks (float64) and the float32 baseline the tolerance is measured against. No device.

A reference takes its discontinuities (argmax, ReLU mask, SmoothL1 branch, epsilon rule) from its own float64
values alone; the case builders below steer the inputs away from them, from the reference alone:
  - a row whose double-DQN argmax is within ARGMAX_GAP of a tie in any branch gets masks[b] = 0 (an episode end:
    the next-state term vanishes and the argmax no longer matters);
  - a row of q(s) with a pre-activation within RELU_MARGIN of the ReLU kink is drawn again (see bdqn_case).
"""
from __future__ import annotations

import functools

import numpy as np

EPS32 = 2.0 ** -24  # unit roundoff of f32
BH = 128            # BranchingQNetwork hidden width
QH = 16             # DQNEntity hidden width
ARGMAX_GAP = 1e-4   # of max |q(s')|
RELU_MARGIN = 1e-4  # of max |pre-activation| of the layer
BDQN_KEYS = ("w1", "b1", "w2", "b2", "wv", "bv", "wa", "ba")
DQN_KEYS = ("w1", "b1", "w2", "b2")


def f32(x):
    """The float64 value of x rounded to f32 (a scalar the kernel receives as float)."""
    return float(np.float32(x))


# ------------------------------------------------------------------------------------------ Branching DQN

def _bdqn_forward(net, x, ac, n):
    """x [B, obs] f64 -> dict(pre1, o1, pre2, o2, v [B], adv [B, ac, n], q [B, ac, n]) in float64."""
    w = {k: np.asarray(net[k], dtype=np.float64) for k in BDQN_KEYS}
    pre1 = x @ w["w1"].T + w["b1"]
    o1 = np.maximum(pre1, 0.0)
    pre2 = o1 @ w["w2"].T + w["b2"]
    o2 = np.maximum(pre2, 0.0)
    v = o2 @ w["wv"].reshape(-1) + w["bv"].reshape(())
    adv = (o2 @ w["wa"].T + w["ba"]).reshape(x.shape[0], ac, n)
    q = v[:, None, None] + adv - adv.mean(axis=2, keepdims=True)
    return dict(pre1=pre1, o1=o1, pre2=pre2, o2=o2, v=v, adv=adv, q=q)


def _top2_gap(q):
    """Top-1 minus top-2 along the last axis (inf where it has one entry)."""
    if q.shape[-1] < 2:
        return np.full(q.shape[:-1], np.inf)
    s = np.sort(q, axis=-1)
    return s[..., -1] - s[..., -2]


def _argmax(q, last=False):
    """First (torch.argmax) or last maximal index along the last axis."""
    if not last:
        return np.argmax(q, axis=-1)
    return q.shape[-1] - 1 - np.argmax(q[..., ::-1], axis=-1)


def bdqn_update_ref(q, t, xs, xn, actions, rewards, masks, gamma, clip, argmax_last=False):
    """update_policy on a drawn batch in float64. q, t: dicts of the stacked f32 weights (w1 [128, obs], b1, w2,
    b2, wv [1, 128], bv [1], wa [ac * n, 128], ba); xs, xn [B, obs] int8; actions [B, ac] (clamped to 0 .. n - 1
    as the kernel documents); rewards, masks [B]; gamma and clip as the kernel's f32 receives them (clip <= 0: no
    clamp). Returns dict(loss, grads = the eight clamped gradients, raw = the unclamped ones, argmax_gap [B, ac]
    = top-1 minus top-2 of the online q(s'), relu_margin [B] = the smallest |pre-activation| of layers 1 and 2 of
    q(s), pre_scale = (max |pre1|, max |pre2|) of q(s), qn_scale = max |q(s')|, relu_rel [B] = the row's smallest
    |pre| / its layer's scale). argmax_last: ties go to the larger index (what a wrong kernel would do)."""
    ac = int(np.asarray(actions).shape[1])
    n = int(np.asarray(q["wa"]).shape[0]) // ac
    xs = np.asarray(xs).astype(np.float64)
    xn = np.asarray(xn).astype(np.float64)
    B = xs.shape[0]
    act = np.clip(np.asarray(actions).astype(np.int64), 0, n - 1)
    r = np.asarray(rewards, dtype=np.float64)
    mk = np.asarray(masks, dtype=np.float64)
    g32 = f32(gamma)
    fs, fn, ft = _bdqn_forward(q, xs, ac, n), _bdqn_forward(q, xn, ac, n), _bdqn_forward(t, xn, ac, n)
    am = _argmax(fn["q"], last=argmax_last)                                   # [B, ac]
    tq = np.take_along_axis(ft["q"], am[..., None], axis=2)[..., 0]           # [B, ac]
    expected = r + tq.mean(axis=1) * g32 * mk                                 # [B]
    cur = np.take_along_axis(fs["q"], act[..., None], axis=2)[..., 0]         # [B, ac]
    e = expected[:, None] - cur
    loss = float((e * e).sum() / (B * ac))
    # backward: d loss / d cur, through q = v + adv - mean(adv), the heads, and both ReLU layers
    dcur = -2.0 * e / (B * ac)
    dqv = np.zeros((B, ac, n))
    np.put_along_axis(dqv, act[..., None], dcur[..., None], axis=2)
    dadv = (dqv - dqv.sum(axis=2, keepdims=True) / n).reshape(B, ac * n)
    dv = dcur.sum(axis=1)
    w = {k: np.asarray(q[k], dtype=np.float64) for k in BDQN_KEYS}
    do2 = dadv @ w["wa"] + dv[:, None] * w["wv"].reshape(1, -1)
    dpre2 = do2 * (fs["pre2"] > 0)
    dpre1 = (dpre2 @ w["w2"]) * (fs["pre1"] > 0)
    raw = dict(w1=dpre1.T @ xs, b1=dpre1.sum(0), w2=dpre2.T @ fs["o1"], b2=dpre2.sum(0),
               wv=(dv @ fs["o2"]).reshape(1, -1), bv=dv.sum().reshape(1), wa=dadv.T @ fs["o2"], ba=dadv.sum(0))
    c32 = f32(clip)
    grads = {k: (np.clip(g, -c32, c32) if c32 > 0 else g.copy()) for k, g in raw.items()}
    s1, s2 = float(np.abs(fs["pre1"]).max()), float(np.abs(fs["pre2"]).max())
    m1, m2 = np.abs(fs["pre1"]).min(axis=1), np.abs(fs["pre2"]).min(axis=1)
    return dict(loss=loss, grads=grads, raw=raw, argmax_gap=_top2_gap(fn["q"]), relu_margin=np.minimum(m1, m2),
                pre_scale=(s1, s2), qn_scale=float(np.abs(fn["q"]).max()),
                relu_rel=np.minimum(m1 / (s1 if s1 > 0 else 1.0), m2 / (s2 if s2 > 0 else 1.0)))


def bdqn_update_torch(q, t, xs, xn, actions, rewards, masks, gamma, clip, dtype):
    """The same loss through torch CPU autograd in `dtype` (float64: cross-check of bdqn_update_ref; float32:
    torch's own rounding on the same inputs, the yardstick of the GPU tolerance). Returns (loss, clamped grads)."""
    import torch

    ac = int(np.asarray(actions).shape[1])
    n = int(np.asarray(q["wa"]).shape[0]) // ac
    tw = lambda net, grad: {k: torch.tensor(np.asarray(net[k]), dtype=dtype, requires_grad=grad) for k in BDQN_KEYS}
    qw, twt = tw(q, True), tw(t, False)

    def fwd(w, x):
        o = torch.relu(torch.nn.functional.linear(x, w["w1"], w["b1"]))
        o = torch.relu(torch.nn.functional.linear(o, w["w2"], w["b2"]))
        v = torch.nn.functional.linear(o, w["wv"], w["bv"])
        adv = torch.nn.functional.linear(o, w["wa"], w["ba"]).view(x.shape[0], ac, n)
        return v.unsqueeze(2) + adv - adv.mean(2, keepdim=True)

    s = torch.tensor(np.asarray(xs)).to(dtype)
    s1 = torch.tensor(np.asarray(xn)).to(dtype)
    a = torch.tensor(np.clip(np.asarray(actions).astype(np.int64), 0, n - 1))
    r = torch.tensor(np.asarray(rewards, dtype=np.float64)).to(dtype).view(-1, 1)
    m = torch.tensor(np.asarray(masks, dtype=np.float64)).to(dtype).view(-1, 1)
    cur = fwd(qw, s).gather(2, a.unsqueeze(2)).squeeze(-1)
    with torch.no_grad():
        am = torch.argmax(fwd(qw, s1), dim=2)
        mx = fwd(twt, s1).gather(2, am.unsqueeze(2)).squeeze(-1).mean(1, keepdim=True)
    expected = r + mx * torch.tensor(f32(gamma), dtype=dtype) * m
    loss = ((expected - cur) ** 2).mean()
    gr = torch.autograd.grad(loss, [qw[k] for k in BDQN_KEYS])
    c32 = f32(clip)
    out = {k: (g.clamp(-c32, c32) if c32 > 0 else g).double().numpy() for k, g in zip(BDQN_KEYS, gr)}
    return float(loss.detach()), out


# base of the update table and the axes varied one at a time around it (issue: part 3)
BDQN_BASE = dict(obs=70, ac=3, n=33, B=128, ld=None, act_ld=None, lo=-5, hi=12, wscale=1.0, gamma=0.99, clip=1.0,
                 masks="rand", actions="rand", seed=1)


def _bdqn_table():
    t = {}

    def add(name, **kw):
        assert name not in t
        t[name] = dict(BDQN_BASE, **kw)

    for B in (1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128):
        add("B%d" % B, B=B)
    for obs in (1, 7, 8, 9, 31, 32, 33, 127, 128, 129, 255, 256, 257, 512, 513, 1024, 1025):
        add("obs%d" % obs, obs=obs)
    for ac, n in ((2, 31), (7, 9), (2, 32), (16, 32), (7, 73)):  # head rows 63, 64, 65, 513 (Mp 576), 512 (Mp 512)
        add("heads%d" % (ac * n + 1), ac=ac, n=n)
    for n in (1, 2, 63, 64, 65, 127, 128):
        add("n%d" % n, n=n)
    for ac in (1, 4, 5, 32):
        add("ac%d" % ac, ac=ac)
    add("act-zero", actions="zero")
    add("act-last", actions="last")
    # ld == obs and ld > obs, ld % 8 zero and not, obs % 4 zero and not (ld == obs with ld % 8 == 0 forces obs % 4 == 0)
    for obs, ld in ((72, 72), (68, 68), (72, 80), (72, 76), (68, 72), (70, 80), (70, 75), (70, 71)):
        add("obs%d-ld%d" % (obs, ld), obs=obs, ld=ld)
    add("act-ld8", act_ld=8)
    add("full-range", lo=-128, hi=127)
    add("w1e-3", wscale=1e-3, clip=0.0)
    add("w1e2", wscale=1e2, clip=0.0)
    add("gamma0", gamma=0.0)
    add("mask0", masks="zero")
    add("clip0", clip=0.0)
    add("clip-small", clip=None)  # chosen by bdqn_case: the median |unclamped gradient| of w2
    return t


BDQN_CASES = _bdqn_table()
MAX_ROW_DRAWS = 200


def _linear_init(rng, out_f, in_f):
    k = 1.0 / np.sqrt(in_f)
    return (rng.uniform(-k, k, (out_f, in_f)).astype(np.float32), rng.uniform(-k, k, (out_f,)).astype(np.float32))


def bdqn_net(rng, obs, ac, n, scale=1.0):
    """One BranchingQNetwork's stacked f32 weights, nn.Linear's init ranges, times scale."""
    w1, b1 = _linear_init(rng, BH, obs)
    w2, b2 = _linear_init(rng, BH, BH)
    wv, bv = _linear_init(rng, 1, BH)
    wa, ba = _linear_init(rng, ac * n, BH)
    net = dict(w1=w1, b1=b1, w2=w2, b2=b2, wv=wv, bv=bv, wa=wa, ba=ba)
    return {k: (v.astype(np.float64) * scale).astype(np.float32) for k, v in net.items()}


def _redraw_kink_rows(q, xs, B, lo, hi, ac, n, seed):
    """Draw again, one row at a time, every row of xs[:B] whose q(s) has a pre-activation within 2 * RELU_MARGIN
    of zero (relative to its layer's largest). A whole-case seed search cannot do this: a 128-row case has 32768
    pre-activations and about ten of them land inside the margin at any seed, so no seed would be found; a row
    has 256 and is clear nine times in ten. The draw of row b, attempt k, is default_rng((seed, b, k))."""
    obs = xs.shape[1]
    for sweep in range(MAX_ROW_DRAWS):
        f = _bdqn_forward(q, xs[:B].astype(np.float64), ac, n)
        s1, s2 = np.abs(f["pre1"]).max(), np.abs(f["pre2"]).max()
        bad = (np.abs(f["pre1"]).min(axis=1) < 2 * RELU_MARGIN * s1) | (np.abs(f["pre2"]).min(axis=1) < 2 * RELU_MARGIN * s2)
        if not bad.any():
            return sweep
        for b in np.nonzero(bad)[0]:
            xs[b] = np.random.default_rng((seed, int(b), sweep + 1)).integers(lo, hi + 1, obs).astype(np.int8)
    raise RuntimeError("no draw of some row clears the ReLU margin")


@functools.lru_cache(maxsize=None)
def bdqn_case(name):
    """The inputs and the float64 reference of one table case: dict(cfg, q, t, xs, xn [B, obs] int8, actions
    [B, ac] int8, rewards, masks [B] f32, terminal [B] bool (the random episode ends), tie_masked [B] bool (rows
    masked by the argmax rule), ref = bdqn_update_ref(...)). Deterministic in the case's committed seed."""
    cfg = dict(BDQN_CASES[name])
    obs, ac, n, B, seed = cfg["obs"], cfg["ac"], cfg["n"], cfg["B"], cfg["seed"]
    rng = np.random.default_rng((seed, obs, ac, n, B))
    q = bdqn_net(rng, obs, ac, n, cfg["wscale"])
    t = bdqn_net(rng, obs, ac, n, cfg["wscale"])  # a target net of its own draw
    xs = rng.integers(cfg["lo"], cfg["hi"] + 1, (B, obs)).astype(np.int8)
    xn = rng.integers(cfg["lo"], cfg["hi"] + 1, (B, obs)).astype(np.int8)
    if cfg["actions"] == "zero":
        actions = np.zeros((B, ac), dtype=np.int8)
    elif cfg["actions"] == "last":
        actions = np.full((B, ac), n - 1, dtype=np.int8)
    else:
        actions = rng.integers(0, n, (B, ac)).astype(np.int8)
    rewards = rng.integers(-30, 30, B).astype(np.float32)
    terminal = rng.random(B) < 0.1
    masks = np.zeros(B, dtype=np.float32) if cfg["masks"] == "zero" else (~terminal).astype(np.float32)
    cfg["row_sweeps"] = _redraw_kink_rows(q, xs, B, cfg["lo"], cfg["hi"], ac, n, seed)
    ref = bdqn_update_ref(q, t, xs, xn, actions, rewards, masks, cfg["gamma"], 0.0)
    tie = (ref["argmax_gap"] < ARGMAX_GAP * ref["qn_scale"]).any(axis=1)
    masks[tie] = 0.0
    if cfg["clip"] is None:  # a clamp that about half of w2's gradient elements reach
        ref = bdqn_update_ref(q, t, xs, xn, actions, rewards, masks, cfg["gamma"], 0.0)
        cfg["clip"] = f32(np.median(np.abs(ref["raw"]["w2"][ref["raw"]["w2"] != 0])))
    ref = bdqn_update_ref(q, t, xs, xn, actions, rewards, masks, cfg["gamma"], cfg["clip"])
    return dict(cfg=cfg, q=q, t=t, xs=xs, xn=xn, actions=actions, rewards=rewards, masks=masks, terminal=terminal,
                tie_masked=tie, ref=ref)


TIE = dict(obs=70, ac=2, n=100, B=64, pairs=((3, 67), (5, 40)), seed=3)  # (j, k) of branch 0: lanes 3 of strides 0
# and 1 of the kernel's 64-lane strided argmax; of branch 1: two lanes of stride 0


@functools.lru_cache(maxsize=None)
def bdqn_tie_case():
    """Exact ties on purpose: in branch m the online net's advantage rows j and k are copies (weights and bias),
    raised above the others, so q(s')[j] == q(s')[k] bit for bit in any arithmetic and they are the maximum; the
    target net differs by 100 between j and k. The first index must win. masks are all 1. Returns the case with
    ref (first index) and ref_last (ties to the larger index: what the loss would be then)."""
    c = TIE
    obs, ac, n, B = c["obs"], c["ac"], c["n"], c["B"]
    rng = np.random.default_rng((c["seed"], obs, ac, n, B))
    q, t = bdqn_net(rng, obs, ac, n), bdqn_net(rng, obs, ac, n)
    for m, (j, k) in enumerate(c["pairs"]):
        q["wa"][m * n + k] = q["wa"][m * n + j]
        q["ba"][m * n + j] += 5.0
        q["ba"][m * n + k] = q["ba"][m * n + j]
        t["ba"][m * n + j] += 50.0
        t["ba"][m * n + k] -= 50.0
    xs = rng.integers(-5, 13, (B, obs)).astype(np.int8)
    xn = rng.integers(-5, 13, (B, obs)).astype(np.int8)
    actions = rng.integers(0, n, (B, ac)).astype(np.int8)
    rewards = rng.integers(-30, 30, B).astype(np.float32)
    masks = np.ones(B, dtype=np.float32)
    sweeps = _redraw_kink_rows(q, xs, B, -5, 12, ac, n, c["seed"])
    cfg = dict(BDQN_BASE, obs=obs, ac=ac, n=n, B=B, clip=0.0, row_sweeps=sweeps)
    ref = bdqn_update_ref(q, t, xs, xn, actions, rewards, masks, cfg["gamma"], cfg["clip"])
    ref_last = bdqn_update_ref(q, t, xs, xn, actions, rewards, masks, cfg["gamma"], cfg["clip"], argmax_last=True)
    qn = _bdqn_forward(q, xn.astype(np.float64), ac, n)["q"]
    third = np.sort(qn, axis=2)[..., -3]
    return dict(cfg=cfg, q=q, t=t, xs=xs, xn=xn, actions=actions, rewards=rewards, masks=masks, ref=ref,
                ref_last=ref_last, third_gap=qn.max(axis=2) - third, argmax=_argmax(qn))


# ---------------------------------------------------------------------------------------------------- DQN

def _dqn_q(net, g, x):
    """Q [R, A] of group g's net on rows x [R, D] f64, and the hidden layer [R, 16]."""
    w1, b1, w2, b2 = (np.asarray(net[k][g], dtype=np.float64) for k in DQN_KEYS)
    h = np.tanh(x @ w1.T + b1)
    return h @ w2.T + b2, h


def dqn_gather(states, next_states, actions, rewards, samples, D, upg, g):
    """The rows of group g in the kernel's order ((e * upg + j) * B + b): states / next_states [E, U, cap, stride]
    int8, actions / rewards [E, U, cap], samples [E, U, B] -> (s [R, D], s1 [R, D], a [R], r [R])."""
    E, U, B = samples.shape
    units = np.arange(g * upg, (g + 1) * upg)
    idx = np.asarray(samples)[:, units].astype(np.int64)                       # [E, upg, B]
    ei = np.arange(E)[:, None, None]
    ui = units[None, :, None]
    s = np.asarray(states)[ei, ui, idx][..., :D].reshape(-1, D)
    s1 = np.asarray(next_states)[ei, ui, idx][..., :D].reshape(-1, D)
    return s, s1, np.asarray(actions)[ei, ui, idx].reshape(-1), np.asarray(rewards)[ei, ui, idx].reshape(-1)


def dqn_grad_ref(pol, tgt, states, next_states, actions, rewards, samples, D, upg, gamma, clip):
    """optimize_model of every group in float64: SmoothL1 (beta 1) of Q(s)[a] against r + gamma * max Q_t(s'),
    mean over the group's upg * E * B rows; clip > 0 clamps (inf: a clamp that moves nothing), clip <= 0 does
    not. pol / tgt: dicts of [G, ...] f32 arrays. Returns a list per group of dict(loss, grads (clamped), raw,
    absd [R] = |Q(s)[a] - expected|, gap [R] = top-2 gap of the target's max (recorded only: the max value is
    continuous in the Q-values))."""
    G = np.asarray(pol["w1"]).shape[0]
    g32, c32 = f32(gamma), float(np.float32(clip))
    out = []
    for g in range(G):
        s, s1, a, r = dqn_gather(states, next_states, actions, rewards, samples, D, upg, g)
        s, s1, a, r = s.astype(np.float64), s1.astype(np.float64), a.astype(np.int64), r.astype(np.float64)
        R = s.shape[0]
        qv, h = _dqn_q(pol, g, s)
        qt, _ = _dqn_q(tgt, g, s1)
        y = qt.max(axis=1) * g32 + r
        d = qv[np.arange(R), a] - y
        ad = np.abs(d)
        loss = float(np.where(ad < 1.0, 0.5 * d * d, ad - 0.5).sum() / R)
        gd = np.where(ad < 1.0, d, np.sign(d)) / R
        dq = np.zeros_like(qv)
        dq[np.arange(R), a] = gd
        w2 = np.asarray(pol["w2"][g], dtype=np.float64)
        dpre = (dq @ w2) * (1.0 - h * h)
        raw = dict(w1=dpre.T @ s, b1=dpre.sum(0), w2=dq.T @ h, b2=dq.sum(0))
        grads = {k: (np.clip(v, -c32, c32) if c32 > 0 else v.copy()) for k, v in raw.items()}
        out.append(dict(loss=loss, grads=grads, raw=raw, absd=ad, gap=_top2_gap(qt)))
    return out


def dqn_grad_torch(pol, tgt, states, next_states, actions, rewards, samples, D, upg, gamma, clip, dtype):
    """The same per group through torch CPU autograd in `dtype`: [(loss, clamped grads)]."""
    import torch

    G = np.asarray(pol["w1"]).shape[0]
    c32 = float(np.float32(clip))
    out = []
    for g in range(G):
        s, s1, a, r = dqn_gather(states, next_states, actions, rewards, samples, D, upg, g)
        w = [torch.tensor(np.asarray(pol[k][g]), dtype=dtype, requires_grad=True) for k in DQN_KEYS]
        wt = [torch.tensor(np.asarray(tgt[k][g]), dtype=dtype) for k in DQN_KEYS]
        net = lambda p, x: torch.nn.functional.linear(torch.tanh(torch.nn.functional.linear(x, p[0], p[1])), p[2], p[3])
        qsa = net(w, torch.tensor(s).to(dtype)).gather(1, torch.tensor(a.astype(np.int64)).view(-1, 1))
        nxt = net(wt, torch.tensor(s1).to(dtype)).max(1)[0].detach()
        y = nxt * torch.tensor(f32(gamma), dtype=dtype) + torch.tensor(r.astype(np.float64)).to(dtype)
        loss = torch.nn.SmoothL1Loss()(qsa, y.unsqueeze(1))
        gr = torch.autograd.grad(loss, w)
        out.append((float(loss), {k: (v.clamp(-c32, c32) if c32 > 0 else v).double().numpy()
                                  for k, v in zip(DQN_KEYS, gr)}))
    return out


def dqn_act_ref(net, obs, D, upg):
    """selectAction's greedy half in float64 for obs [E, U, stride] int8, unit u in group u // upg: (Q [E, U, A],
    the first argmax [E, U], the top-2 gap [E, U] (inf at A = 1))."""
    obs = np.asarray(obs)
    E, U, _ = obs.shape
    A = np.asarray(net["w2"]).shape[1]
    Q = np.empty((E, U, A))
    for u in range(U):
        Q[:, u], _ = _dqn_q(net, u // upg, obs[:, u, :D].astype(np.float64))
    return Q, np.argmax(Q, axis=2), _top2_gap(Q)


def dqn_act_rule(greedy, u1, u2, eps, A):
    """The epsilon rule as k_dqn_act documents it: a row explores unless u1 > eps (so u1 == eps explores), and
    an exploring row takes min(int(u2 * A), A - 1) (u2 * A in float64 may round up to A)."""
    u1, u2 = np.asarray(u1, dtype=np.float64), np.asarray(u2, dtype=np.float64)
    explore = ~(u1 > eps)
    rnd = np.minimum((u2 * float(A)).astype(np.int64), A - 1)
    return np.where(explore, rnd, greedy), explore


def dqn_clear(Q, gap):
    """Rows whose greedy action is compared: the float64 gap exceeds 1e-5 * (1 + |q|) (tests/test_dqn_gpu.py)."""
    return gap > 1e-5 * (1.0 + np.abs(Q.max(axis=2)))


def dqn_nets(rng, G, D, A):
    w = dict(w1=[], b1=[], w2=[], b2=[])
    for _ in range(G):
        w1, b1 = _linear_init(rng, QH, D)
        w2, b2 = _linear_init(rng, A, QH)
        for k, v in zip(DQN_KEYS, (w1, b1, w2, b2)):
            w[k].append(v)
    return {k: np.stack(v) for k, v in w.items()}


def align4(x):
    return (x + 3) // 4 * 4


def dqn_grad_lds(D, A):
    """ms_dqn_grad's dynamic LDS in bytes (dqn_kernels.hip dqn_grad_lds, capi.cpp dqn_xpitch)."""
    xpitch = 4 * (((D + 3) // 4) | 1)
    wfl = QH * D + QH + A * QH + A
    return 4 * (2 * wfl + 2 * 256 * (QH + 1) + 2 * 256) + 4 * 256 + 256 * xpitch


# gradient table: name -> (G, upg, D, stride, A, E, cap, B, clip, seed); rows per group = upg * E * B
def _dqn_grad_table():
    t = {}
    inf = float("inf")
    for D in (1, 3, 4, 5, 60, 195, 256):
        t["D%d" % D] = (2, 1, D, align4(D), 5, 7, 6, 10, 1.0, 1)
    for A in (1, 2, 97, 127):
        t["A%d" % A] = (2, 1, 11, 12, A, 7, 6, 10, 1.0, 1)
    # cap 2 and B 1 too; seed 2: the first whose two rows (one per group) lie one in each SmoothL1 branch
    t["rows1"] = (2, 1, 11, 12, 5, 1, 2, 1, 1.0, 2)
    t["rows255"] = (2, 3, 11, 12, 5, 85, 3, 1, 1.0, 1)
    t["rows256"] = (2, 1, 11, 12, 5, 32, 3, 8, 1.0, 1)
    t["rows257"] = (2, 1, 11, 12, 5, 257, 2, 1, 1.0, 1)
    t["rows513"] = (3, 3, 11, 12, 5, 19, 4, 9, 1.0, 1)
    t["clip0"] = (2, 1, 11, 12, 5, 7, 6, 10, 0.0, 1)
    t["clip-inf"] = (2, 1, 11, 12, 5, 7, 6, 10, inf, 1)
    t["stride"] = (2, 2, 11, 24, 5, 7, 6, 10, 1.0, 1)     # stride > D, garbage in the padding
    t["corner"] = (2, 1, 256, 256, 127, 30, 4, 10, 1.0, 1)  # the LDS maximum, 154616 B
    return t


DQN_GRAD_CASES = _dqn_grad_table()


@functools.lru_cache(maxsize=None)
def dqn_grad_case(name):
    """Inputs and float64 reference of one gradient case. Rewards mix {-1, 0, 1} with +-20 so that both SmoothL1
    branches are taken; the bytes D .. stride - 1 hold +-127 garbage."""
    G, upg, D, stride, A, E, cap, B, clip, seed = DQN_GRAD_CASES[name]
    rng = np.random.default_rng((seed, G, upg, D, A, E, cap, B))
    pol, tgt = dqn_nets(rng, G, D, A), dqn_nets(rng, G, D, A)
    U = G * upg
    st = rng.choice(np.array([-127, 127], dtype=np.int8), (E, U, cap, stride))
    nx = rng.choice(np.array([-127, 127], dtype=np.int8), (E, U, cap, stride))
    st[..., :D] = rng.integers(-5, 13, (E, U, cap, D))
    nx[..., :D] = rng.integers(-5, 13, (E, U, cap, D))
    acts = rng.integers(0, A, (E, U, cap)).astype(np.int8)
    small = rng.integers(-1, 2, (E, U, cap))
    big = rng.choice(np.array([-20, 20]), (E, U, cap))
    rew = np.where(rng.random((E, U, cap)) < 0.5, small, big).astype(np.float32)
    samples = rng.integers(0, cap, (E, U, B)).astype(np.int32)
    gamma = 0.84
    ref = dqn_grad_ref(pol, tgt, st, nx, acts, rew, samples, D, upg, gamma, clip)
    return dict(G=G, upg=upg, D=D, stride=stride, A=A, E=E, cap=cap, B=B, clip=clip, gamma=gamma, pol=pol, tgt=tgt,
                states=st, next_states=nx, actions=acts, rewards=rew, samples=samples, ref=ref)


# act table: name -> (G, upg, D, stride, A, E, seed)
def _dqn_act_table():
    t = {}
    Es = (1, 255, 256, 257)
    for i, D in enumerate((1, 3, 4, 5, 60, 195, 256)):
        t["D%d" % D] = (2, 2, D, align4(D) + (4 if D in (3, 60) else 0), 5, Es[i % 4], 1)
    for i, A in enumerate((1, 2, 97, 127)):
        t["A%d" % A] = (2, 2, 11, 12, A, Es[(i + 3) % 4], 1)
    t["corner"] = (2, 2, 256, 256, 127, 257, 1)
    return t


DQN_ACT_CASES = _dqn_act_table()
ACT_EPS = 0.4


@functools.lru_cache(maxsize=None)
def dqn_act_case(name):
    """Inputs and float64 reference of one act case with given uniforms. The first four rows carry the edges of
    the epsilon rule: row 0 u1 == eps (explores), row 1 u1 one ulp above eps (greedy), row 2 u2 = 1 - 2^-53
    (u2 * A may round to A: the clamp), row 3 u2 = 0; rows 0 and 1 get a u2 whose action is not the greedy one,
    so that the wrong branch shows."""
    G, upg, D, stride, A, E, seed = DQN_ACT_CASES[name]
    rng = np.random.default_rng((seed, G, upg, D, A, E))
    net = dqn_nets(rng, G, D, A)
    U = G * upg
    obs = rng.choice(np.array([-127, 127], dtype=np.int8), (E, U, stride))
    obs[..., :D] = rng.integers(-5, 13, (E, U, D))
    uni = rng.random((2, E * U))
    Q, greedy, gap = dqn_act_ref(net, obs, D, upg)
    gflat = greedy.reshape(-1)
    other = lambda r: (((int(gflat[r]) + 1) % A) + 0.5) / A
    uni[0, 0], uni[1, 0] = ACT_EPS, other(0)
    uni[0, 1], uni[1, 1] = np.nextafter(ACT_EPS, 1.0), other(1)
    uni[0, 2], uni[1, 2] = 0.0, 1.0 - 2.0 ** -53
    uni[0, 3], uni[1, 3] = 0.25, 0.0
    action, explore = dqn_act_rule(gflat, uni[0], uni[1], ACT_EPS, A)
    return dict(G=G, upg=upg, D=D, stride=stride, A=A, E=E, U=U, net=net, obs=obs, uniforms=uni, Q=Q, greedy=greedy,
                gap=gap, clear=dqn_clear(Q, gap), action=action.reshape(E, U), explore=explore.reshape(E, U))


# --------------------------------------------------------------------------------------- Philox4x32-10

PHILOX_M0, PHILOX_M1 = 0xD2511F53, 0xCD9E8D57
PHILOX_W0, PHILOX_W1 = 0x9E3779B9, 0xBB67AE85
# Random123's known-answer vectors of philox4x32-10 (Salmon et al., SC'11; the kat_vectors file of the
# Random123 distribution): (counter, key, output)
PHILOX_KAT = (
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
     (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
)


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Ten rounds of Philox4x32 on arrays of 32-bit words (held in uint64): four output words."""
    m32 = np.uint64(0xffffffff)
    c0, c1, c2, c3, k0, k1 = (np.asarray(x, dtype=np.uint64) & m32 for x in (c0, c1, c2, c3, k0, k1))
    sh = np.uint64(32)
    for _ in range(10):
        p0 = np.uint64(PHILOX_M0) * c0
        p1 = np.uint64(PHILOX_M1) * c2
        c0, c1, c2, c3 = (p1 >> sh) ^ c1 ^ k0, p1 & m32, (p0 >> sh) ^ c3 ^ k1, p0 & m32
        k0 = (k0 + np.uint64(PHILOX_W0)) & m32
        k1 = (k1 + np.uint64(PHILOX_W1)) & m32
    return c0, c1, c2, c3


def u53(a, b):
    """random.random()'s 53-bit double in [0, 1) from two 32-bit words."""
    a, b = np.asarray(a, dtype=np.uint64), np.asarray(b, dtype=np.uint64)
    return ((a >> np.uint64(5)).astype(np.float64) * 67108864.0 + (b >> np.uint64(6)).astype(np.float64)) / 9007199254740992.0


def dqn_act_uniforms(rows, seed, offset):
    """The (u1, u2) k_dqn_act draws for rows 0 .. rows - 1: counter (row lo, row hi, off lo, off hi), key (seed
    lo, seed hi), off = offset + *offset_dev mod 2^64."""
    r = np.arange(rows, dtype=np.uint64)
    off = np.uint64(offset % (1 << 64))
    sd = np.uint64(seed % (1 << 64))
    s32 = np.uint64(32)
    full = lambda v: np.full(rows, v, dtype=np.uint64)
    o = philox4x32_10(r, r >> s32, full(off), full(off >> s32), full(sd), full(sd >> s32))
    return u53(o[0], o[1]), u53(o[2], o[3])
