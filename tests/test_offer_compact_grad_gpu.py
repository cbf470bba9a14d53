"""The offer gradient on compact offer rows (ms_ppo_grad_offer_compact, k_ppo_grad's kOffCompact bit).

The N*L offer rows of a replica and round share every byte but the slot's (prio, rem) pair at bytes 2C, 2C + 1
(Agent.py:126-134), so the one-launch free-price rollout stores a template per replica and a pair per row. The
gradient kernel's compact mode loads a lane's dwords from the template and ORs the pair into the dword that holds it:
the same dwords the rows would have given, so every gradient tensor and loss term must equal ms_ppo_grad on the
expanded rows bit for bit. ms_offer_compress / ms_offer_expand are each other's inverse on such rows."""
import importlib

import pytest
import torch

pytestmark = pytest.mark.gpu

N, L, G = 8, 3, 8
U = N * L


def _chunk_tiles(R, groups):
    """capi.cpp's ppo_split: 16-row tiles per wave chunk."""
    tiles = (R + 15) // 16
    ct = max(8, -(-tiles * groups // 8192))
    return (ct + 1) & ~1


def _batch(R, C, seed):
    """Random templates [R, stride] (zero tail), pairs [R, U], actions, old log-probs, returns for G groups."""
    D = 2 * C + 2
    stride = (D + 3) & ~3
    gen = torch.Generator().manual_seed(seed)
    tmpl = torch.zeros((R, stride), dtype=torch.int8)
    tmpl[:, : 2 * C] = torch.randint(-1, 13, (R, 2 * C), generator=gen, dtype=torch.int8)
    pair_bytes = torch.randint(-1, 13, (R, U, 2), generator=gen, dtype=torch.int8)
    pair = pair_bytes.contiguous().view(torch.int16).reshape(R, U)
    rows = tmpl.unsqueeze(1).repeat(1, U, 1)
    rows[:, :, 2 * C: 2 * C + 2] = pair_bytes
    actions = torch.randint(0, C + 1, (R, U), generator=gen, dtype=torch.int8)
    old_lp = -torch.rand((R, U), generator=gen) * 3 - 0.05
    ret = torch.randn((R, 1, G), generator=gen)
    return [x.cuda() for x in (tmpl, pair, rows.contiguous(), actions, old_lp, ret)]


@pytest.mark.parametrize("C", [8, 7, 5])
def test_compress_expand_round_trip(ms, C):
    """Rows -> (template, pairs) -> rows, R = 33 records; C 8: the pair in a dword of its own, 7 and 5: the pair in
    the upper half of the last template dword."""
    ppo = importlib.import_module("marl-scheduling_amd.ppo")
    tmpl, pair, rows, *_ = _batch(33, C, 1)
    t2, p2 = torch.full_like(tmpl, 0x55), torch.full_like(pair, 0x5555)
    ppo.offer_compress(rows, 2 * C + 2, t2, p2)
    assert torch.equal(t2, tmpl) and torch.equal(p2, pair)
    r2 = torch.full_like(rows, 0x55)
    ppo.offer_expand(tmpl, pair, 2 * C + 2, r2)
    torch.cuda.synchronize()
    assert torch.equal(r2, rows)


@pytest.mark.parametrize("C", [8, 7, 5])
@pytest.mark.parametrize("R", [1, 15, 16, 17, 33, "chunk+1"])
def test_compact_gradient_equals_row_gradient(ms, C, R):
    """ms_ppo_grad_offer_compact = ms_ppo_grad on the expanded rows: all twelve gradient tensors and the loss terms,
    bit for bit. R around the 16-row tile, a tile pair, and one row past a wave chunk (16 * chunk_tiles + 1: a second
    chunk of one row); G = 8 groups whose units include unit 0 and unit N*L - 1; C = 8 (D 18: <2, 1>, pair at dword
    4, shift 0), C = 7 (D 16: <2, 1>, shift 16), C = 5 (D 12: <1, 1>, shift 16)."""
    ppo = importlib.import_module("marl-scheduling_amd.ppo")
    if R == "chunk+1":
        R = 16 * _chunk_tiles(129, G) + 1
        assert _chunk_tiles(R, G) * 16 + 1 == R
    D, A = 2 * C + 2, C + 1
    tmpl, pair, rows, actions, old_lp, ret = _batch(R, C, 10 * C + (R % 7))
    sel = torch.tensor([0, 4, 7, 11, 12, 16, 20, U - 1], dtype=torch.int32, device="cuda")
    torch.manual_seed(5)
    grp = ppo.PPOGroup(G, D, A, 0.003, 0.01, 0.9, 0.2, 1, device="cuda")
    keys = ppo.ACTOR_KEYS + ppo.CRITIC_KEYS
    out = []
    for compact in (False, True):
        if compact:
            ep = grp.fused_epoch(None, actions, old_lp, ret, sel, R, 1, off_compact=(tmpl, pair))
        else:
            ep = grp.fused_epoch(rows, actions, old_lp, ret, sel, R, 1)
        for k in keys:
            getattr(grp.policy, k).grad.fill_(float("nan"))
        terms = ep.launch().clone()
        torch.cuda.synchronize()
        out.append(({k: getattr(grp.policy, k).grad.clone() for k in keys}, terms))
    (g0, t0), (g1, t1) = out
    assert torch.isfinite(t0).all() and torch.equal(t0, t1)
    for k in keys:
        assert torch.isfinite(g0[k]).all() and torch.equal(g0[k], g1[k]), k
