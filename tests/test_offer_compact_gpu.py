"""Compact offer observations in the one-launch free-price rollout and the fused update (Trainer.off_compact).

A round's N*L offer rows are the replica's template (the cores' (prio, rem) pairs, Agent.py:126-134) with the slot's
pair at bytes 2C, 2C + 1. By default the one-launch rollout (ms_env_rollout_act_free_compact) writes the template and
the pairs of every round and the offer rows of the last round only, the offer gradient reads the compact rings
(ms_ppo_grad_offer_compact), and Trainer.off_obs expands ring slots 1..T-1 at its first read. MS_OFF_COMPACT=0 is
the trainer that writes and reads the rows. Nothing may change: every comparison here is bit for bit."""
import importlib

import pytest
import torch

pytestmark = pytest.mark.gpu

CFG3 = (8, 8, 3)
# cfg3: C = 8, the pair in a dword of its own (shift 0), 2C + 2 = 18 no multiple of 4 (two zero tail bytes);
# 8 x 7 x 2: odd C, the pair in the upper half of a template dword (shift 16), 2C + 2 = 16 a multiple of 4;
# 5 x 5 x 5: odd C again with an odd N * L = 25 (pairs stored one by one, no dword copies), rows of 12 bytes
SHAPES = [CFG3, (8, 7, 2), (5, 5, 5)]


def _mods():
    return (importlib.import_module("marl-scheduling_amd.trainer"), importlib.import_module("marl-scheduling_amd.abi"),
            importlib.import_module("marl-scheduling_amd.ppo"))


def _trainer(shape, E, T, seed=5, **kw):
    tr_mod, abi, _ = _mods()
    if shape == CFG3:
        return tr_mod.Trainer.from_named("cfg3", n_envs=E, update_step=T, seed=seed, device="cuda:0", **kw)
    cfg = abi.make_config(*shape, free_prices=True, commercial=True, **abi.EXP4_JOBS)
    hp = tr_mod.Hyper(update_step=T, raw_k_epochs=2)
    return tr_mod.Trainer(cfg, E, arch="local", hyper=hp, seed=seed, device="cuda:0", **kw)


def _pair(monkeypatch, mk):
    """(compact trainer, MS_OFF_COMPACT=0 trainer) of one construction."""
    compact = mk()
    monkeypatch.setenv("MS_OFF_COMPACT", "0")
    rows = mk()
    monkeypatch.delenv("MS_OFF_COMPACT")
    assert compact.off_compact and compact.fused_rollout_free and rows.fused_rollout_free and not rows.off_compact
    return compact, rows


def _rings(t):
    out = {"acc_rows": t.acc_rows, "acc_owner": t.acc_owner, "off_obs": t.off_obs, "env_price": t.env_price,
           "price_obs": t.price_obs, "agent_reward": t.agent_reward, "auct_reward": t.auct_reward}
    for u in t.units():
        for k in ("actions", "logprobs", "rewards"):
            out["%s.%s" % (u.name, k)] = getattr(u, k)
    return out


def _same_weights(a, b):
    ppo = _mods()[2]
    for u0, u1 in zip(a.units(), b.units()):
        for k in ppo.ACTOR_KEYS + ppo.CRITIC_KEYS:
            assert torch.equal(getattr(u0.group.policy, k), getattr(u1.group.policy, k)), (u0.name, k)


@pytest.mark.parametrize("E", [7, 33, 64])
@pytest.mark.parametrize("shape", SHAPES)
def test_compact_rollout_equals_row_rollout(ms, monkeypatch, shape, E):
    """rollout() with T = 2 and T = 5, twice with an update between (the second from the carried slot 0, compressed
    by the rollout): every ring of the compact trainer, off_obs included, equals the row-writing trainer's, and the
    compact rings hold the template and the pairs cut out of that trainer's rows. E = 7: less than a wave's four
    replicas twice over; 33: a partial last workgroup (4 N replicas each); 64."""
    C = shape[1]
    for T in (2, 5):
        compact, rows = _pair(monkeypatch, lambda: _trainer(shape, E, T, use_graph=False))
        for it in range(2):
            compact.rollout()
            rows.rollout()
            torch.cuda.synchronize()
            raw = compact._off_obs.clone()  # before anything reads the property
            r0, r1 = _rings(compact), _rings(rows)
            for k in r0:
                assert torch.equal(r0[k], r1[k]), (T, it, k)
            assert torch.equal(raw[0], r1["off_obs"][0]) and torch.equal(raw[T], r1["off_obs"][T])
            ref = r1["off_obs"]  # [T + 1, E, N*L, stride]
            tmpl = ref[:, :, 0].clone()
            tmpl[..., 2 * C: 2 * C + 2] = 0
            pair = ref[..., 2 * C: 2 * C + 2].contiguous().view(torch.int16).squeeze(-1)
            assert torch.equal(compact.off_tmpl, tmpl), (T, it)
            assert torch.equal(compact.off_pair, pair), (T, it)
            l0, l1 = compact.update(), rows.update()
            for k in l0:
                assert torch.equal(l0[k], l1[k]), (T, it, k)
        _same_weights(compact, rows)
        assert compact.flags() == 0 and rows.flags() == 0


def test_update_reads_no_stale_rows(ms, monkeypatch):
    """After a compact rollout the rows of ring slots 1..T-1 are whatever the ring held: filled with 0x55, update()
    gives the losses and weights of the unpoisoned run, and off_obs read afterwards is the completed ring."""
    T = 5
    poisoned, rows = _pair(monkeypatch, lambda: _trainer(CFG3, 64, T, use_graph=False))
    clean = _trainer(CFG3, 64, T, use_graph=False)
    for t in (poisoned, clean, rows):
        t.rollout()
    poisoned._off_obs[1:T].fill_(0x55)
    losses = [t.update() for t in (poisoned, clean, rows)]
    torch.cuda.synchronize()
    for k in losses[0]:
        assert torch.equal(losses[0][k], losses[1][k]) and torch.equal(losses[0][k], losses[2][k]), k
    _same_weights(poisoned, clean)
    _same_weights(poisoned, rows)
    # (the carry copied slot T over slot 0; slots 1..T-1 are expanded now)
    assert torch.equal(poisoned.off_obs, rows.off_obs) and torch.equal(clean.off_obs, rows.off_obs)


def test_iterations_graph_eager_and_rows(ms, monkeypatch):
    """Three iteration()s (eager, captured, replayed): the compact trainer under HIP graphs, the compact trainer
    without, and the row-writing trainer give equal losses, weights and last observations."""
    T = 5
    graph, rows = _pair(monkeypatch, lambda: _trainer(CFG3, 64, T))
    eager = _trainer(CFG3, 64, T, use_graph=False)
    assert graph.use_graph and eager.off_compact
    for it in range(3):
        ls = [t.iteration() for t in (graph, eager, rows)]
        torch.cuda.synchronize()
        for k in ls[0]:
            assert torch.equal(ls[0][k], ls[1][k]) and torch.equal(ls[0][k], ls[2][k]), (it, k)
        assert torch.equal(graph.off_obs[T], rows.off_obs[T]) and torch.equal(eager.off_obs[T], rows.off_obs[T]), it
    _same_weights(graph, rows)
    _same_weights(eager, rows)
    assert torch.equal(graph.off_obs, rows.off_obs)


def test_checkpoint_resume_of_compact_trainer(ms, tmp_path):
    """A checkpoint saved after iteration 2 and resumed in a fresh trainer runs iteration 3 as the uninterrupted
    trainer does: the loaded slot 0 holds rows, which the next rollout compresses."""
    T = 5
    tr = _trainer(CFG3, 64, T)
    assert tr.off_compact
    for _ in range(2):
        tr.iteration()
    path = str(tmp_path / "ck.pt")
    tr.save_checkpoint(path)
    want = tr.iteration()
    resumed = _trainer(CFG3, 64, T)
    resumed.load_checkpoint(path)
    got = resumed.iteration()
    torch.cuda.synchronize()
    for k in want:
        assert torch.equal(want[k], got[k]), k
    _same_weights(tr, resumed)
    assert torch.equal(tr.off_obs[T], resumed.off_obs[T])
    assert torch.equal(tr.off_obs[1:T], resumed.off_obs[1:T])
