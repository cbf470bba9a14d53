"""Trainer(diagnostics=k) / Trainer.update_diagnostics(): training is unchanged bit for bit, the reported values
equal a float64 CPU recomputation from the trainer's own rings, draws and weights, a policy that did not move
reports so, and the call order is checked.

Bounds: the per-row bound of an output is the kernel test's, 8 x the largest |f32 CPU restatement - float64|
over the rows reduced (tests/test_evaluate_kernel_gpu.py); a mean of per-row values takes the bound itself, a
function of them the bound times the largest |derivative| over the rows."""
import functools
import importlib
import math

import pytest
import torch

from tests.test_evaluate_kernel_gpu import OUTPUTS, _restate

pytestmark = pytest.mark.gpu

E, T, SEED = 64, 8, 3


def _mod(name):
    return importlib.import_module("marl-scheduling_amd." + name)


def _make(name, k, **hyper):
    tr, abi = _mod("trainer"), _mod("abi")
    if name == "divided":
        return tr.Trainer(abi.make_config(3, 2, 2, **abi.README_JOBS), E, arch="divided",
                          hyper=tr.Hyper(update_step=T, **hyper), seed=SEED, diagnostics=k)
    if name == "mixed":  # locally shared nets, so that agent 0's groups are frozen
        return tr.Trainer.from_named("cfg2", n_envs=E, update_step=T, seed=SEED, arch="local", hardcoded_agents=[0],
                                     diagnostics=k)
    if hyper:  # from_named's cfg3 with other learning rates (trainPPOExperiment4.py:96-98)
        hp = tr.Hyper(update_step=T, raw_k_epochs=2, acceptor_gamma=-((1 - 5) / 5) + 0.15, **hyper)
        return tr.Trainer(abi.named_config(name), E, arch="local", hyper=hp, seed=SEED, diagnostics=k)
    return tr.Trainer.from_named(name, n_envs=E, update_step=T, seed=SEED, diagnostics=k)


def _state(t, losses):
    st = {}
    for i, ls in enumerate(losses):
        for k, v in ls.items():
            st["loss%d.%s" % (i, k)] = v.clone()
    for u in t.units():
        g = u.group
        for pol_name, pol in (("policy", g.policy), ("policy_old", g.policy_old)):
            for k, p in pol.named_parameters():
                st["%s.%s.%s" % (u.name, pol_name, k)] = p.detach().clone()
        opt = g.hip_optimizer
        for i, p in enumerate(q for grp in opt.param_groups for q in grp["params"]):
            st["%s.adam%d.m" % (u.name, i)] = opt.state[p]["exp_avg"].clone()
            st["%s.adam%d.v" % (u.name, i)] = opt.state[p]["exp_avg_sq"].clone()
        st[u.name + ".adam.step"] = int(opt.step_dev)
        st[u.name + ".actions"] = u.actions.clone()
        st[u.name + ".logprobs"] = u.logprobs.clone()
        st[u.name + ".rewards"] = u.rewards.clone()
    st["env"] = [env.snapshot().clone() for env, _, _ in t.env.parts]
    st["counters"] = (t.rounds_done, t.rng.getstate(), int(t.rng_ctr), t.flags(), t.env.round)
    return st


def _assert_same(a, b, what=""):
    if isinstance(a, dict):
        assert a.keys() == b.keys(), what
        for k in a:
            _assert_same(a[k], b[k], "%s.%s" % (what, k))
    elif isinstance(a, (list, tuple)):
        assert len(a) == len(b), what
        for i, (x, y) in enumerate(zip(a, b)):
            _assert_same(x, y, "%s[%d]" % (what, i))
    elif isinstance(a, torch.Tensor):
        assert torch.equal(a, b) or (a.is_floating_point() and torch.equal(a.isnan(), b.isnan()) and
                                     torch.equal(a.nan_to_num(0.0), b.nan_to_num(0.0))), what
    else:
        assert a == b, what


@functools.lru_cache(maxsize=None)
def _run(name, k, iters):
    t = _make(name, k)
    losses = [t.iteration() for _ in range(iters)]
    return t, losses


@pytest.mark.parametrize("name", ["cfg2", "cfg3", "divided", "mixed"])
def test_training_is_unchanged(ms, name):
    with_d, losses_d = _run(name, 3, 3)
    plain, losses_p = _run(name, 0, 3)
    assert len(with_d.diagnostics_log) == 3 and with_d.diagnostics_log[0]["slots"] == [1, 4, 6]
    _assert_same(_state(with_d, losses_d), _state(plain, losses_p), name)
    assert plain.diagnostics_log == [] and plain._diag is None and plain._diag_slot0 is None
    if name == "mixed":
        for d in with_d.diagnostics_log:
            for unit in ("acceptor", "offer"):
                for vals in d[unit].values():
                    assert vals[0] is None and all(v is not None for v in vals[1:])


def _reference(t, slots):
    """The diagnostics recomputed on the CPU in float64 from the trainer's rings, its draws and policy's weights,
    with the per-row bounds; Gt is the update's own input (unit_returns of the reward ring, f32)."""
    ppo = _mod("ppo")
    eps = t.hp.eps_clip
    out = {}
    for u in t.units():
        pol = u.group.policy
        G, D = pol.G, pol.D
        w = {k: getattr(pol, k).detach().cpu() for k in ppo.ACTOR_KEYS + ppo.CRITIC_KEYS}
        draws = t._last_draws[u.name]
        if u is t.acc:
            src = t.acceptor_rows(0, T)
        else:
            src = (t.off_obs if u is t.off else t.price_obs)[:T]
        k0 = t._diag_slot0
        if 0 in slots and u is not t.price:  # the rings' slot 0 now holds the carried last observation
            src = src.clone()
            src[0] = k0["off"] if u is t.off else ppo.regen_acceptor_rows(
                k0["acc_rows"][None], k0["acc_owner"][None], t.acc_common, t.N)[0]
        src, actions, logprobs = src.cpu(), u.actions.cpu(), u.logprobs.cpu()
        flat = torch.tensor([x for d in draws for x in d], dtype=torch.int32, device=t.device)
        ret = ppo.unit_returns(u.rewards, flat, u.group.gamma).cpu()
        obs, act, old, gt = [], [], [], []
        for d, sel in enumerate(draws):
            for s in slots:
                obs.append(src[s][:, sel])
                act.append(actions[s][:, sel])
                old.append(logprobs[s][:, sel])
                gt.append(ret[s][:, d * G:(d + 1) * G])
        obs, act, old, gt = torch.cat(obs), torch.cat(act), torch.cat(old).double(), torch.cat(gt).double()
        r64 = _restate(ppo, w, obs, act, G, 1, D, torch.float64)
        r32 = _restate(ppo, w, obs, act, G, 1, D, torch.float32)
        bound = {n: 8.0 * float((r32[i].double() - r64[i]).abs().max()) for i, n in enumerate(OUTPUTS)}
        lp, v, ent = r64[:3]
        lr = lp - old
        ratio = lr.exp()
        var_gt = gt.var(0, unbiased=False)
        ev = torch.where(var_gt > 0, 1 - (gt - v).var(0, unbiased=False) / var_gt, torch.full_like(var_gt, math.nan))
        b_lp, b_v = bound["logprob"], bound["value"]
        # rows whose ratio the log-prob bound can carry over a clip edge
        near = ((ratio - (1 - eps)).abs() <= ratio * math.expm1(b_lp)) | \
               ((ratio - (1 + eps)).abs() <= ratio * math.expm1(b_lp))
        sd_d = (gt - v).var(0, unbiased=False).sqrt()
        out[u.name] = dict(
            rows=obs.shape[0], near=near.sum(0),
            values=dict(approx_kl=(-lr).mean(0), approx_kl_k3=(ratio - 1 - lr).mean(0),
                        clip_fraction=((ratio < 1 - eps) | (ratio > 1 + eps)).double().mean(0),
                        ratio_max=ratio.max(0).values, entropy=ent.mean(0), value_mse=((v - gt) ** 2).mean(0),
                        explained_variance=ev),
            # first-order propagation of the per-row bounds (plus the second-order term where the first vanishes)
            tol=dict(approx_kl=b_lp, approx_kl_k3=b_lp * float((ratio - 1).abs().max()) + b_lp ** 2,
                     ratio_max=b_lp * float(ratio.max()) + b_lp ** 2, entropy=bound["entropy"],
                     value_mse=b_v * 2 * float((v - gt).abs().max()) + b_v ** 2,
                     explained_variance=(2 * b_v * sd_d + b_v ** 2) / var_gt),
            bound=bound)
    return out


@pytest.mark.parametrize("name", ["cfg2", "cfg3"])
def test_values_match_float64(ms, name):
    t, _ = _run(name, 3, 1)
    got = t.diagnostics_log[-1]
    assert got["slots"] == [1, 4, 6]
    ref = _reference(t, got["slots"])
    for u in t.units():
        r, g = ref[u.name], got[u.name]
        G = u.group.policy.G
        n_draws = len(t._last_draws[u.name])
        assert r["rows"] == n_draws * 3 * E and g["rows"] == [r["rows"]] * G
        print("%s %s: rows %d, per-row bounds %s" % (name, u.name, r["rows"], r["bound"]))
        for n, want in r["values"].items():
            have = torch.tensor([math.nan if x is None else x for x in g[n]], dtype=torch.float64)
            if n == "clip_fraction":
                print("  clip_fraction %s (reference %s), rows near an edge %s" %
                      (have.tolist(), want.tolist(), r["near"].tolist()))
                assert bool((r["near"] <= 0.01 * r["rows"]).all())
                assert bool(((have - want).abs() * r["rows"] <= r["near"] + 1e-9).all())
                continue
            tol = r["tol"][n]
            tol = tol if isinstance(tol, torch.Tensor) else torch.full_like(want, tol)
            print("  %s: largest error %.3g, bound %.3g" % (n, float((have - want).abs().nan_to_num(0).max()),
                                                         float(tol.nan_to_num(0).max())))
            assert torch.equal(have.isnan(), want.isnan()), n
            assert bool(((have - want).abs().nan_to_num(0) <= tol.nan_to_num(0)).all()), n


def test_policy_that_did_not_move(ms):
    """Zero learning rates: the update leaves the weights, so the evaluation is of the policy that acted."""
    t = _make("cfg3", T, lr_actor=0.0, lr_critic=0.0)
    for _ in range(2):
        t.iteration()
    got = t.diagnostics_log[-1]
    assert got["slots"] == list(range(T))
    ref = _reference_bounds_only(t, got["slots"])
    for u in t.units():
        g, b = got[u.name], ref[u.name]["logprob"]
        print("%s: log-prob bound %.3g, |approx_kl| %.3g, k3 %.3g, |ratio_max - 1| %.3g" %
              (u.name, b, max(abs(x) for x in g["approx_kl"]), max(g["approx_kl_k3"]),
               max(abs(x - 1) for x in g["ratio_max"])))
        assert g["clip_fraction"] == [0.0] * len(g["clip_fraction"])
        assert all(abs(x) <= b for x in g["approx_kl"])
        assert all(0 <= x <= b for x in g["approx_kl_k3"])
        assert all(abs(x - 1) <= b * math.exp(b) for x in g["ratio_max"])
        # every slot and every draw is evaluated: the rows of the update's own entropy term (all epochs alike)
        want = u.group.last_terms[:, :, 2].double().mean(0).cpu()
        have = torch.tensor(g["entropy"], dtype=torch.float64)
        print("  entropy %s, the update's %s" % (have.tolist(), want.tolist()))
        assert bool(((have - want).abs() <= 1e-5 * want.abs()).all())


def _reference_bounds_only(t, slots):
    return {name: r["bound"] for name, r in _reference(t, slots).items()}


def test_call_order(ms):
    t = _make("cfg2", 2)
    with pytest.raises(RuntimeError):
        t.update_diagnostics()
    t.rollout()
    with pytest.raises(RuntimeError):
        t.update_diagnostics()
    t.update()
    d = t.update_diagnostics()
    assert d["slots"] == [2, 6] and t.diagnostics_log == []  # (iteration() keeps the log, a direct call does not)
    assert t.update_diagnostics(slots=[3])["slots"] == [3]
    with pytest.raises(ValueError):
        t.update_diagnostics(slots=[0])  # the carry overwrote slot 0 and no copy was asked for
    t.rollout()
    with pytest.raises(RuntimeError):
        t.update_diagnostics()


def test_off_allocates_and_launches_nothing(ms):
    t, _ = _run("cfg2", 0, 3)
    assert t.diagnostics == 0 and t.diagnostics_slots == [] and t.diagnostics_log == []
    assert t._diag is None and t._diag_slot0 is None and t.diagnostics_bytes() == 0
