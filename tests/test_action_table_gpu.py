"""ms_action_table (ppo.action_table) against numpy on the same bytes: every quantity is an integer, so equality is
exact. Cases are (E, T, U, A, K): replicas, rounds, units per row, actions, keys."""
import ctypes as ct
import importlib

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _ppo():
    return importlib.import_module("marl-scheduling_amd.ppo")


def _dev(x):
    return torch.as_tensor(np.ascontiguousarray(x), device="cuda")


def ref_table(actions, keys, A, K, n_slots, upb=1, round0=0, ep_len=1 << 30, key_min=0):
    """(counts [n_slots][U / upb][K][A], skipped, bad) of actions / keys [T][E][U]."""
    T, E, U = actions.shape
    a = actions.reshape(T * E, U).astype(np.int64)
    k = keys.reshape(T * E, U).astype(np.int64) - key_min
    keyed = (k >= 0) & (k < K)
    ok = keyed & (a >= 0) & (a < A)
    slot = np.repeat(((round0 + np.arange(T)) // ep_len) % n_slots, E)
    slot = np.broadcast_to(slot[:, None], a.shape)
    bin_ = np.broadcast_to((np.arange(U) // upb)[None, :], a.shape)
    counts = np.zeros((n_slots, U // upb, K, A), dtype=np.int64)
    np.add.at(counts, (slot[ok], bin_[ok], k[ok], a[ok]), 1)
    return counts, int((~keyed).sum()), int((keyed & ~ok).sum())


def run(actions, keys, U, A, K, n_slots, upb=1, round0=0, ep_len=1 << 30, key_min=0, counts=None):
    if counts is None:
        counts = torch.zeros((n_slots, U // upb, K, A), dtype=torch.int64, device="cuda")
    skipped = torch.zeros(1, dtype=torch.int64, device="cuda")
    bad = torch.zeros(1, dtype=torch.int64, device="cuda")
    _ppo().action_table(actions, keys, counts, round0, ep_len, units_per_bin=upb, key_min=key_min, skipped=skipped,
                        bad=bad)
    return counts.cpu().numpy(), int(skipped), int(bad)


def _random(E, T, U, A, K, seed=0):
    rng = np.random.default_rng(seed)
    return rng.integers(0, A, (T, E, U)).astype(np.int8), rng.integers(0, K, (T, E, U)).astype(np.int8)


@pytest.mark.parametrize("E,T,U,A,K", [(1, 1, 1, 1, 1), (65, 3, 5, 9, 13), (300, 2, 24, 9, 13), (33, 2, 40, 5, 3)])
def test_per_unit_tables(ms, E, T, U, A, K):
    """The minimal call; a wave's tail with an odd unit count (byte loads); more than one workgroup's rows with
    word loads; more columns than a lane holds at a time."""
    a, k = _random(E, T, U, A, K)
    got, skipped, bad = run(_dev(a), _dev(k), U, A, K, 1)
    want, _, _ = ref_table(a, k, A, K, 1)
    assert np.array_equal(got, want) and skipped == 0 and bad == 0 and got.sum() == E * T * U


def test_widest_actions_and_keys_in_one_bin(ms):
    E, T, U = 130, 2, 3
    for A, K in ((64, 64), (64, 3), (3, 64)):
        a, k = _random(E, T, U, A, K, seed=1)
        got, skipped, bad = run(_dev(a), _dev(k), U, A, K, 1, upb=U)
        want, _, _ = ref_table(a, k, A, K, 1, upb=U)
        assert got.shape == (1, 1, K, A) and np.array_equal(got, want) and skipped == 0 and bad == 0


@pytest.mark.parametrize("upb", [1, 4, 24])
def test_units_per_bin(ms, upb):
    """A table per unit, per agent (L = 4) and one pooled table."""
    E, T, U, A, K = 70, 2, 24, 5, 4
    a, k = _random(E, T, U, A, K, seed=2)
    got, _, _ = run(_dev(a), _dev(k), U, A, K, 1, upb=upb)
    want, _, _ = ref_table(a, k, A, K, 1, upb=upb)
    assert got.shape[1] == U // upb and np.array_equal(got, want) and got.sum() == E * T * U


@pytest.mark.parametrize("n_slots", [4, 2])
def test_episode_split_and_slot_wrap(ms, n_slots):
    """Rounds 2 .. 8 of episodes of 3 rounds: episodes 0 (one round), 1, 2 (three rounds each); with two slots
    episodes 0 and 2 share slot 0 and their counts add."""
    E, T, U, A, K = 64, 7, 24, 9, 6
    a, k = _random(E, T, U, A, K, seed=3)
    got, _, _ = run(_dev(a), _dev(k), U, A, K, n_slots, upb=4, round0=2, ep_len=3)
    want, _, _ = ref_table(a, k, A, K, n_slots, upb=4, round0=2, ep_len=3)
    assert np.array_equal(got, want)
    per_slot = got.sum(axis=(1, 2, 3)) // (E * U)
    assert list(per_slot) == ([1, 3, 3, 0] if n_slots == 4 else [4, 3])


def test_strided_key_views(ms):
    """Keys as byte 2 of a [..][U][4] state (unit stride 4, offset 2), as the first byte of int16 pairs (unit stride
    2) and as byte 2C of rows of 12 bytes (unit stride 12, offset 6); key_min != 0."""
    E, T, U, A, K = 65, 3, 8, 9, 13
    a, k = _random(E, T, U, A, K, seed=4)
    want, _, _ = ref_table(a, k, A, K, 2, upb=4, round0=1, ep_len=2)
    rng = np.random.default_rng(5)
    for width, at in ((4, 2), (2, 0), (12, 6)):
        rows = rng.integers(-128, 128, (T, E, U, width)).astype(np.int8)
        rows[..., at] = k
        view = _dev(rows)[..., at]
        assert view.stride(2) == width and view.storage_offset() == at
        got, skipped, bad = run(_dev(a), view, U, A, K, 2, upb=4, round0=1, ep_len=2)
        assert np.array_equal(got, want) and skipped == 0 and bad == 0
    pair = _dev((k.astype(np.int16) & 0xff) | (rng.integers(0, 100, k.shape).astype(np.int16) << 8))
    view = pair.view(torch.int8).view(T, E, U, 2)[..., 0]
    got, _, _ = run(_dev(a), view, U, A, K, 2, upb=4, round0=1, ep_len=2)
    assert np.array_equal(got, want)
    got, skipped, _ = run(_dev(a), _dev((k - 5).astype(np.int8)), U, A, K, 2, upb=4, round0=1, ep_len=2, key_min=-5)
    assert np.array_equal(got, want) and skipped == 0


def test_unit_major_strides_equal_row_major(ms):
    E, T, U, A, K = 65, 3, 5, 9, 13
    a, k = _random(E, T, U, A, K, seed=6)
    view = _dev(a.transpose(2, 0, 1)).permute(1, 2, 0)  # stored [U][T][E], seen [T][E][U]
    kview = _dev(k.transpose(2, 0, 1)).permute(1, 2, 0)
    assert not view.is_contiguous()
    got_um, _, _ = run(view, kview, U, A, K, 2, round0=1, ep_len=2)
    got_mixed, _, _ = run(view, _dev(k), U, A, K, 2, round0=1, ep_len=2)
    got_rm, _, _ = run(_dev(a), _dev(k), U, A, K, 2, round0=1, ep_len=2)
    want, _, _ = ref_table(a, k, A, K, 2, round0=1, ep_len=2)
    assert np.array_equal(got_um, got_rm) and np.array_equal(got_mixed, got_rm) and np.array_equal(got_rm, want)


def test_contention_one_pair_everywhere(ms):
    """A converged policy on jobs of one priority: every lane of every wave on one counter per column."""
    E, T, U, A, K = 4096, 2, 24, 9, 13
    a, k = np.full((T, E, U), 7, dtype=np.int8), np.full((T, E, U), 12, dtype=np.int8)
    got, skipped, bad = run(_dev(a), _dev(k), U, A, K, 1, upb=4)
    assert skipped == 0 and bad == 0 and got.sum() == E * T * U
    assert np.array_equal(got[0, :, 12, 7], np.full(U // 4, E * T * 4))
    again, _, _ = run(_dev(a), _dev(k), U, A, K, 1, upb=4)
    assert np.array_equal(again, got)  # integer sums: the same from run to run


def test_keys_out_of_range_are_skipped_and_their_actions_not_examined(ms):
    E, T, U, A, K = 65, 3, 8, 9, 13
    rng = np.random.default_rng(7)
    a, k = _random(E, T, U, A, K, seed=8)
    hit = rng.random(a.shape) < 0.2
    k[hit] = rng.choice(np.array([-5, -2, -1, K], dtype=np.int8), hit.sum())
    a[hit] = 127
    got, skipped, bad = run(_dev(a), _dev(k), U, A, K, 2, upb=4, ep_len=2)
    want, want_skipped, _ = ref_table(a, k, A, K, 2, upb=4, ep_len=2)
    assert np.array_equal(got, want) and skipped == want_skipped == hit.sum() and bad == 0
    assert got.sum() + skipped + bad == E * T * U


def test_actions_out_of_range_are_bad_not_binned(ms):
    E, T, U, A, K = 65, 3, 8, 9, 13
    rng = np.random.default_rng(9)
    a, k = _random(E, T, U, A, K, seed=10)
    hit = rng.random(a.shape) < 0.1
    a[hit] = rng.choice(np.array([-1, A], dtype=np.int8), hit.sum())
    skip = ~hit & (rng.random(a.shape) < 0.1)
    k[skip] = -1
    got, skipped, bad = run(_dev(a), _dev(k), U, A, K, 1, upb=8)
    want, want_skipped, want_bad = ref_table(a, k, A, K, 1, upb=8)
    assert np.array_equal(got, want) and bad == want_bad == hit.sum() and skipped == want_skipped == skip.sum()
    assert got.sum() + skipped + bad == E * T * U


def test_accumulation(ms):
    E, T, U, A, K = 65, 3, 5, 9, 13
    (a, k), (b, kb) = _random(E, T, U, A, K, seed=11), _random(E, T, U, A, K, seed=12)
    counts = torch.zeros((2, U, K, A), dtype=torch.int64, device="cuda")
    run(_dev(a), _dev(k), U, A, K, 2, round0=0, ep_len=2, counts=counts)
    got, _, _ = run(_dev(b), _dev(kb), U, A, K, 2, round0=3, ep_len=2, counts=counts)
    want = ref_table(a, k, A, K, 2, 1, 0, 2)[0] + ref_table(b, kb, A, K, 2, 1, 3, 2)[0]
    assert np.array_equal(got, want)


def _raw(ms, a, k, c, **over):
    g = ms.abi.MsActionTableArgs()
    T, E, U = a.shape
    g.actions, g.row_stride, g.unit_stride = ms._lib.ptr(a), U, 1
    g.keys, g.key_row_stride, g.key_unit_stride = ms._lib.ptr(k), U, 1
    g.n_units, g.units_per_bin, g.n_keys, g.key_min, g.n_actions = U, 1, 3, 0, 5
    g.n_envs, g.n_rounds, g.episode_length, g.n_slots, g.counts = E, T, 4, 1, ms._lib.ptr(c)
    for name, v in over.items():
        setattr(g, name, v)
    return ms.lib.ms_action_table(ct.byref(g), None)


def test_unsupported_shapes_are_refused(ms):
    a, k = (_dev(x) for x in _random(4, 2, 3, 5, 3))
    counts = torch.full((16384 + 64 * 65 * 3,), 5, dtype=torch.int64, device="cuda")
    assert _raw(ms, a, k, torch.zeros(3 * 3 * 5, dtype=torch.int64, device="cuda")) == 0  # (the helper's call is valid)
    for over, word in ((dict(n_actions=65), b"n_actions"), (dict(n_keys=65), b"n_keys"),
                       (dict(units_per_bin=2), b"units_per_bin"), (dict(units_per_bin=0), b"units_per_bin"),
                       (dict(actions=None), b"NULL"), (dict(keys=None), b"NULL"), (dict(counts=None), b"NULL"),
                       (dict(n_slots=0), b"n_slots"), (dict(n_rounds=0), b"n_rounds"),
                       (dict(key_unit_stride=0), b"stride"), (dict(key_min=-129), b"key_min")):
        assert _raw(ms, a, k, counts, **over) == 22  # MS_EINVAL
        assert word in ms.lib.ms_last_error()
    # the counter budget's edge (A, K <= 64, so 16383 = 3 * 43 * 127 needs 127 bins): 127 bins x 43 keys x 3 actions
    # = 16383 is taken, 128 bins x 64 keys x 2 actions = 16384 is refused
    a127, k127 = (_dev(x) for x in _random(4, 2, 127, 3, 43, seed=1))
    ok_counts = torch.zeros(16383, dtype=torch.int64, device="cuda")
    assert _raw(ms, a127, k127, ok_counts, n_keys=43, n_actions=3) == 0
    want, _, _ = ref_table(a127.cpu().numpy(), k127.cpu().numpy(), 3, 43, 1, ep_len=4)
    assert np.array_equal(ok_counts.cpu().numpy().reshape(want.shape), want)
    a128, k128 = (_dev(x) for x in _random(4, 2, 128, 2, 64, seed=2))
    assert _raw(ms, a128, k128, counts, n_keys=64, n_actions=2) == 22 and b"do not fit" in ms.lib.ms_last_error()
    torch.cuda.synchronize()
    assert int((counts != 5).sum()) == 0
