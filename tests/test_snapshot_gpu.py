"""BatchedEnv.snapshot / restore (ms_env_snapshot / ms_env_restore): the packed state restores into another env
exactly (against the CPU oracle, through further rounds), is as small as documented, and a snapshot that does
not fit or was damaged is refused with code 22 and leaves the target as it was."""
import numpy as np
import pytest
import torch

from tests.drivers import STATE_KEYS, compare_state, step_rounds_vs_oracle

pytestmark = pytest.mark.gpu

MT_WORDS = 624
A16 = lambda x: (x + 15) & ~15


def _cfg(ms, name, **kw):
    if name == "3x5x2":  # tests/test_oracle.py's small_free_commercial with five cores
        return ms.abi.make_config(n_agents=3, n_cores=5, collection_length=2, priorities=[2, 4, 8], lengths=[5, 5, 5],
                                  probabilities=[0.5, 0.25, 0.25], free_prices=True, commercial=True, **kw)
    assert not kw
    return ms.abi.named_config(name)


def _header(snap):
    h = snap[:64].cpu().numpy()
    return dict(magic=bytes(h[:4]), version=int(h[4:8].view("<u4")[0]), E=int(h[8:16].view("<i8")[0]),
                dims=tuple(int(x) for x in h[16:40].view("<i4")), n_liab=int(h[40:48].view("<i8")[0]),
                total=int(h[48:56].view("<u8")[0]))


def _layout(env, n_liab):
    """Section offsets as marlsched.h documents them."""
    E, rb = env.E, env.shape.env_record_bytes
    o_recs = A16(64 + len(bytes(env.cfg)))
    o_mt = o_recs + E * rb
    o_off = o_mt + E * 4 * MT_WORDS
    o_liab = o_off + A16(8 * (E + 1))
    return dict(o_recs=o_recs, o_mt=o_mt, o_off=o_off, o_liab=o_liab, total=o_liab + A16(8 * n_liab))


def _state_equal(a, b):
    assert a.keys() == b.keys()
    for k in a:
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)


def _other_env(ms, oracle, cfg, E, seed):
    """An env of another seed, 7 rounds in with actions of its own: every array of it differs."""
    env = ms.BatchedEnv(cfg, E, seed=seed)
    step_rounds_vs_oracle(ms, env, [oracle.OracleEnv(cfg, seed + e) for e in range(E)], 7, np.random.default_rng(99),
                          state_every=100, accept_bias=0.4)
    return env


@pytest.mark.parametrize("name,E", [("3x5x2", 37), ("3x5x2", 1), ("cfg1", 37), ("cfg1", 1), ("cfg3", 37), ("cfg3", 1),
                                    ("cfg4", 5)])
def test_round_trip_against_oracle(ms, oracle, name, E):
    cfg = _cfg(ms, name)
    seed = 100
    A = ms.BatchedEnv(cfg, E, seed=seed)
    oenvs = [oracle.OracleEnv(cfg, seed + e) for e in range(E)]
    rng = np.random.default_rng(1)
    step_rounds_vs_oracle(ms, A, oenvs, 2, rng, state_every=1)
    # the odd replicas get a state of their own: by the ABI their current block is then half 0, while the even
    # ones crossed into half 1 at their first draw (a seeded stream starts at mti = 624)
    for e in range(1, E, 2):
        words = np.random.default_rng(1000 + e).integers(0, 2 ** 32, MT_WORDS, dtype=np.uint64).astype(np.uint32)
        A.set_rng_state(words.tolist(), 300, env_index=e)
        st = oenvs[e].export_state()
        st["mt"], st["mt_index"] = words, 300
        oenvs[e].import_state(st)
    step_rounds_vs_oracle(ms, A, oenvs, 22, rng, state_every=4)
    want = A.export_state()
    # no replica crossed into another block since: both halves are present as current ones
    assert all(300 < want["mt_index"][e] < MT_WORDS for e in range(1, E, 2))
    assert all(0 < want["mt_index"][e] < MT_WORDS for e in range(0, E, 2))
    # the chains are neither all empty nor all alike
    assert want["liab_n"].max() >= 2 and want["liab_n"].min() == 0
    snap = A.snapshot()
    assert snap.dtype == torch.uint8 and snap.is_cuda and snap.dim() == 1
    h = _header(snap)
    n_liab = int(want["liab_n"].sum())
    assert h["n_liab"] == n_liab and n_liab > 0
    assert h["magic"] == b"MSSP" and h["version"] == 1 and h["E"] == E and h["total"] == snap.numel()
    assert h["dims"] == (A.N, A.C, A.L, A.shape.liability_cap, A.shape.env_record_bytes, len(bytes(cfg)))
    assert snap.numel() == A.snapshot_bytes(n_liab) == _layout(A, n_liab)["total"]
    assert torch.equal(A.snapshot(), snap)  # a function of the state
    _state_equal(A.export_state(), want)    # taking it changed nothing
    B = _other_env(ms, oracle, cfg, E, seed=777)
    B.restore(snap)
    assert B.round == int(want["round"][0]) == A.round and B.flags() == 0
    got = B.export_state()
    compare_state(got, [o.export_state() for o in oenvs], E)
    for k in STATE_KEYS + ("mt", "liab", "flags"):
        np.testing.assert_array_equal(got[k], want[k], err_msg=k)
    # ... and B goes on as A would have: observations, rewards, events and the state after every round
    seen = step_rounds_vs_oracle(ms, B, oenvs, 16, rng, state_every=1)
    assert seen["executed"] > 0 and B.flags() == 0 and B.round == int(want["round"][0]) + 16


def test_fresh_env(ms, oracle):
    """A snapshot at round 0 (mti = 624, every chain empty) restores and steps like a fresh env of that seed;
    a CPU tensor is accepted."""
    cfg = _cfg(ms, "cfg3")
    E, seed = 6, 31
    fresh = ms.BatchedEnv(cfg, E, seed=seed)
    want = fresh.export_state()
    snap = fresh.snapshot()
    assert _header(snap)["n_liab"] == 0 and snap.numel() == _layout(fresh, 0)["total"]
    B = _other_env(ms, oracle, cfg, E, seed=500)
    B.restore(snap.cpu())
    st = B.export_state()
    assert (st["mt_index"] == MT_WORDS).all() and (st["liab_n"] == 0).all()
    _state_equal(st, want)
    seen = step_rounds_vs_oracle(ms, B, [oracle.OracleEnv(cfg, seed + e) for e in range(E)], 6, np.random.default_rng(3),
                                 state_every=1)
    assert seen["executed"] > 0


def _with_chain(env, e, core, n, flags=0):
    """env's exported state with replica e's `core` holding n valid entries (and its last core none)."""
    st = env.export_state()
    st["liab_n"][e, core] = n
    st["liab_n"][e, -1] = 0
    for q in range(n):
        st["liab"][e, core, q] = (1 + q % env.N, q % (env.N + 1), q - 2, 1 + q, 5 + q)
    st["flags"][e] = flags
    return st


def test_full_chain(ms):
    cfg = _cfg(ms, "3x5x2", liability_cap=4)
    A = ms.BatchedEnv(cfg, 3, seed=9)
    A.import_state(_with_chain(A, 1, 0, 4))
    want = A.export_state()
    assert want["liab_n"][1, 0] == 4 == A.shape.liability_cap and want["liab_n"][1, -1] == 0
    snap = A.snapshot()
    assert _header(snap)["n_liab"] == 4
    B = ms.BatchedEnv(cfg, 3, seed=10)
    B.restore(snap)
    _state_equal(B.export_state(), want)


def test_sticky_flag(ms):
    cfg = _cfg(ms, "3x5x2")
    A = ms.BatchedEnv(cfg, 4, seed=9)
    A.import_state(_with_chain(A, 2, 1, 1, flags=ms.abi.FLAG_LIABILITY_OVERFLOW))
    snap = A.snapshot()
    B = ms.BatchedEnv(cfg, 4, seed=9)
    assert B.flags() == 0
    B.restore(snap)
    assert B.flags() & ms.abi.FLAG_LIABILITY_OVERFLOW
    z = lambda *s: torch.zeros(s, dtype=torch.int8, device=B.device)
    with pytest.raises(ms.MarlSchedError) as exc:
        B.step(z(4, B.N, B.C), z(4, B.N, B.L), z(4, B.N, B.L))
    assert exc.value.code == ms.abi.EOVERFLOW == 75
    # a clean snapshot clears the word again
    B.restore(ms.BatchedEnv(cfg, 4, seed=9).snapshot())
    assert B.flags() == 0
    B.step(z(4, B.N, B.C), z(4, B.N, B.L), z(4, B.N, B.L))


def test_size_and_out_buffer(ms, oracle):
    cfg = _cfg(ms, "cfg3")
    E = 37
    A = _other_env(ms, oracle, cfg, E, seed=40)
    n_liab = int(A.export_state()["liab_n"].sum())
    snap = A.snapshot()
    s = A.shape
    assert snap.numel() == (A16(64 + len(bytes(cfg))) + E * (s.env_record_bytes + 2496) + A16(8 * (E + 1)) +
                            A16(8 * n_liab))
    assert snap.numel() < E * (s.env_record_bytes + 2 * 2496 + A.C * s.liability_cap * 8)
    big = torch.full((snap.numel() + 4096,), 0xAB, dtype=torch.uint8, device=A.device)
    view = A.snapshot(out=big)
    assert view.data_ptr() == big.data_ptr() and torch.equal(view, snap)
    assert (big[snap.numel():] == 0xAB).all()  # nothing written behind the snapshot
    small = torch.zeros(snap.numel() - 16, dtype=torch.uint8, device=A.device)
    with pytest.raises(ms.MarlSchedError) as exc:
        A.snapshot(out=small)
    assert exc.value.code == 22


def _rec_offsets(env):
    """Byte offsets inside a record (ms_layout.h): header 16 B, then core_owner, core_kind, core_rem, liab_n."""
    c4 = (env.C + 3) & ~3
    return dict(mti=8, core_owner=16, core_kind=16 + c4, core_rem=16 + 2 * c4, liab_n=16 + 3 * c4)


def test_refusals_leave_the_env_untouched(ms, oracle):
    cfg = _cfg(ms, "3x5x2")
    E = 37
    target = _other_env(ms, oracle, cfg, E, seed=60)
    before = target.export_state()
    src = _other_env(ms, oracle, cfg, E, seed=61)
    good = src.snapshot()
    n_liab = _header(good)["n_liab"]
    lay, ro, rb = _layout(src, n_liab), _rec_offsets(src), src.shape.env_record_bytes
    assert n_liab > 8

    def edited(fn):
        h = good.cpu().numpy().copy()
        fn(h, h[lay["o_off"]: lay["o_off"] + 8 * (E + 1)].view("<u8"))
        return torch.from_numpy(h)

    rec = lambda h, e, field, i=0: lay["o_recs"] + e * rb + ro[field] + i

    def set_u8(e, field, i, v):
        def fn(h, off):
            h[rec(h, e, field, i)] = v
        return fn

    def set_mti(h, off):
        h[rec(h, 4, "mti"): rec(h, 4, "mti") + 4].view("<i4")[0] = 700

    def off_beyond(h, off):
        off[3] = n_liab + 5

    def off_decreasing(h, off):
        assert off[2] + 1 <= n_liab
        off[1] = off[2] + 1

    def off_huge(h, off):
        off[5] = 1 << 62

    def off_shifted(h, off):
        off[:] += 1

    other_prio = _cfg(ms, "3x5x2")
    other_prio.job_priority[1] = 5
    cases = [
        ("another shape", ms.BatchedEnv(_cfg(ms, "cfg1"), E, seed=1).snapshot(), "shape"),
        ("another E", ms.BatchedEnv(cfg, E + 1, seed=1).snapshot(), "replicas"),
        ("other job priorities", ms.BatchedEnv(other_prio, E, seed=1).snapshot(), "configuration"),
        ("one byte short", good[:-1], "bytes"),
        ("sixteen bytes long", torch.cat([good, good[:16]]), "bytes"),
        ("header only", good[:64].clone(), "bytes"),
        ("core_kind 9", edited(set_u8(2, "core_kind", 0, 9)), "env 2: bad core kind"),
        ("liab_n cap + 1", edited(set_u8(3, "liab_n", 1, src.shape.liability_cap + 1)), "env 3: liability chain too long"),
        ("owner N + 1", edited(set_u8(36, "core_owner", 4, src.N + 1)), "env 36: bad core owner"),
        ("mti 700", edited(set_mti), "env 4: mt_index"),
        ("liab_off beyond n_liab", edited(off_beyond), "bad liab_off"),
        ("liab_off decreasing", edited(off_decreasing), "liab_off"),
        ("liab_off huge", edited(off_huge), "bad liab_off"),
        ("liab_off not from 0", edited(off_shifted), "env 0: bad liab_off"),
        ("not a snapshot", torch.zeros(good.numel(), dtype=torch.uint8), "magic"),
    ]
    for what, snap, msg in cases:
        with pytest.raises(ms.MarlSchedError) as exc:
            target.restore(snap)
        assert exc.value.code == 22, what
        assert msg in str(exc.value), (what, str(exc.value))
        _state_equal(target.export_state(), before)
    # the target still steps, and the unedited snapshot still restores
    assert target.flags() == 0
    target.restore(good)
    _state_equal(target.export_state(), src.export_state())
