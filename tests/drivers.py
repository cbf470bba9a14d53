"""Synthetic action drivers shared by parity tests (test infrastructure)."""
import numpy as np
import torch


def random_actions(rng: np.random.Generator, obs_acc_counts, N, C, L, O, free, max_price, accept_bias=0.6):
    """Actions like a policy would emit them.

    obs_acc_counts[a][c] = number of real offers in acceptor (a, c)'s observation.
    Acceptors pick a real offer with probability accept_bias, else uniform in [0, O].
    Offer units pick a core action uniformly in [0, C]; with free prices the price
    follows FreePriceOfferPPO.selectAction (PPOmodules.py:312-332): -5 when the
    core chooser picked action 0, else uniform in [0, max_price].
    """
    acc = rng.integers(0, O + 1, size=(N, C))
    pick = rng.random((N, C)) < accept_bias
    for a in range(N):
        for c in range(C):
            n = int(obs_acc_counts[a][c])
            if pick[a, c] and n > 0:
                acc[a, c] = rng.integers(0, n)
    off = rng.integers(0, C + 1, size=(N, L))
    price = None
    if free:
        price = rng.integers(0, max_price + 1, size=(N, L))
        price[off == 0] = -5
    return acc.astype(np.int32), off.astype(np.int32), None if price is None else price.astype(np.int32)


def offer_counts_from_obs(acc_obs, O):
    """Number of non-pad (price, necT) pairs in each acceptor observation row."""
    pairs = np.asarray(acc_obs)[..., 3:3 + 2 * O].reshape(acc_obs.shape[:-1] + (O, 2))
    return (pairs[..., 1] != -2).sum(-1)


STATE_KEYS = ("round", "core_owner", "core_kind", "core_rem", "core_birth", "slot_kind", "slot_rem", "slot_wait",
              "slot_birth", "offer_core", "offer_recip", "offer_price", "liab_n", "mt_index")


def compare_state(gs, os_list, E):
    """The exported device state of replicas 0..E-1 against the oracles' (every field, the live liability
    entries and all 624 MT19937 words)."""
    for e in range(E):
        o = os_list[e]
        for k in STATE_KEYS:
            np.testing.assert_array_equal(gs[k][e], o[k], err_msg="%s env %d" % (k, e))
        np.testing.assert_array_equal(gs["mt"][e], o["mt"], err_msg="mt env %d" % e)
        for c in range(gs["liab_n"].shape[1]):
            n = gs["liab_n"][e, c]
            np.testing.assert_array_equal(gs["liab"][e, c, :n], o["liab"][c, :n])


def step_rounds_vs_oracle(ms, genv, oenvs, T, rng, state_every, accept_bias=0.7):
    """T rounds of ms_env_step on genv beside one OracleEnv per replica, fed the same random_actions: the
    observations (pad bytes zero), every reward kind and the accepted / terminated events after every round, the
    whole state every state_every rounds and after the last. Returns what the run exercised: the number of
    executed offers and the largest acceptor, core and price action fed."""
    cfg = genv.cfg
    s = ms.abi.config_shape(cfg)
    N, C, L, O = s["N"], s["C"], s["L"], s["O"]
    E = genv.E
    dev = genv.device
    genv.reset(genv.obs_buffers(auctioneer=True))
    oobs = [o.observe() for o in oenvs]
    free = bool(cfg.free_prices)
    seen = dict(executed=0, acceptor=-1, core=-1, price=-1)
    for t in range(T):
        acts = [random_actions(rng, offer_counts_from_obs(oobs[e]["acceptor"], O), N, C, L, O, free,
                               s["price_actions"] - 1, accept_bias=accept_bias) for e in range(E)]
        acc = torch.tensor(np.stack([a[0] for a in acts]), dtype=torch.int8, device=dev)
        off = torch.tensor(np.stack([a[1] for a in acts]), dtype=torch.int8, device=dev)
        pr = torch.tensor(np.stack([a[2] for a in acts]), dtype=torch.int8, device=dev) if free else None
        seen["acceptor"] = max(seen["acceptor"], int(acc.max()))
        seen["core"] = max(seen["core"], int(off.max()))
        if free:
            seen["price"] = max(seen["price"], int(pr.max()))
        ev = genv.event_buffers()
        gobs, grew, gev = genv.step(acc, off, pr, obs=genv.obs_buffers(auctioneer=True), events=ev)
        ores = [oenvs[e].step(*acts[e]) for e in range(E)]
        oobs = [o.observe() for o in oenvs]
        ga = gobs["acceptor"].cpu().numpy()
        gof = gobs["offer"].cpu().numpy()
        gau = gobs["auctioneer"].cpu().numpy()
        grew = {k: v.cpu().numpy() for k, v in grew.items() if v is not None}
        for e in range(E):
            np.testing.assert_array_equal(ga[e, :, :, : s["acc_obs_dim"]], oobs[e]["acceptor"], err_msg="acc obs t=%d e=%d" % (t, e))
            assert (ga[e, :, :, s["acc_obs_dim"]:] == 0).all()
            np.testing.assert_array_equal(gof[e, :, :, : s["off_obs_dim"]], oobs[e]["offer"], err_msg="off obs t=%d e=%d" % (t, e))
            np.testing.assert_array_equal(gau[e, :, : s["acc_obs_dim"]], oobs[e]["auctioneer"], err_msg="auct obs t=%d" % t)
            np.testing.assert_array_equal(grew["acceptor"][e], ores[e]["acceptor"], err_msg="acc rew t=%d e=%d" % (t, e))
            np.testing.assert_array_equal(grew["offer"][e], ores[e]["offer"])
            if free:
                np.testing.assert_array_equal(grew["price"][e], ores[e]["price"])
            np.testing.assert_array_equal(grew["auctioneer"][e], ores[e]["auctioneer"])
            np.testing.assert_array_equal(grew["agent"][e], ores[e]["agent"])
            gacc = ms.decode_accepted(gev["accepted"][e])
            gterm = ms.decode_terminated(gev["terminated"][e])
            for f in ("valid", "offerer", "recipient", "slot", "price", "nec_time", "prio", "kind", "order", "round"):
                np.testing.assert_array_equal(gacc[f][gacc["valid"] == 1], ores[e]["accepted"][f][ores[e]["accepted"]["valid"] == 1])
            np.testing.assert_array_equal(gacc["valid"], ores[e]["accepted"]["valid"])
            for f in ("valid", "owner", "prio", "init_len", "dwell"):
                np.testing.assert_array_equal(gterm[f], ores[e]["terminated"][f])
            seen["executed"] += int((ores[e]["accepted"]["valid"] == 1).sum())
        if t % state_every == 0 or t == T - 1:
            compare_state(genv.export_state(), [o.export_state() for o in oenvs], E)
    return seen
