"""Host side of the learned auctioneer (Trainer(learned_auctioneer=True)), no device: the new entry points are
declared, exported and found by name with the ABI version unchanged, the ctypes structs have the C compiler's
layout, the calls refuse NULL arguments, Trainer refuses the combinations it cannot run before it touches a device,
the auctioneer's cores are drawn after the agents' sub-units, and the checkpoint manifest carries the field only
when the feature is on."""
import ctypes as ct
import importlib
import os
import random
import re
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("ms_env_auct_supported", "ms_env_step_act_auct", "ms_env_rollout_act_auct")
N, C, L = 4, 4, 3


def _header():
    with open(os.path.join(REPO, "include", "marlsched.h")) as f:
        return f.read()


def _mod(name):
    return importlib.import_module("marl-scheduling_amd." + name)


def test_exports_exist_and_abi_is_still_24(ms):
    header = _header()
    assert int(re.search(r"#define\s+MS_ABI_VERSION\s+(\d+)", header).group(1)) == 24
    assert ms._lib.ABI_VERSION == 24 and int(ms.lib.ms_abi_version()) == 24
    lib = ct.CDLL(ms.LIB_PATH)
    for name in NAMES:
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert name in ms._lib.EXPORTED and hasattr(lib, name) and ms._lib.has(name)
    assert re.search(r"ms_env_rollout_act_auct\s*\([^;]*const\s+ms_fused_act_auct\s*\*\s*auct,\s*const\s+"
                     r"ms_round_strides\s*\*\s*strides,\s*const\s+ms_round_strides_auct\s*\*\s*astrides,", header)


PROBE = r"""
#include <cstddef>
#include <cstdio>
#include "marlsched.h"
int main() {
    printf("%zu %zu %zu %zu %zu\n", sizeof(ms_fused_act_auct), offsetof(ms_fused_act_auct, auctioneer),
           offsetof(ms_fused_act_auct, auct_offset), offsetof(ms_fused_act_auct, auct_action),
           offsetof(ms_fused_act_auct, auct_logprob));
    printf("%zu %zu %zu %zu\n", sizeof(ms_round_strides_auct), offsetof(ms_round_strides_auct, auctioneer_action),
           offsetof(ms_round_strides_auct, next_auct_action), offsetof(ms_round_strides_auct, next_auct_logprob));
    printf("%zu %zu %zu %zu\n", sizeof(ms_mlp_params), sizeof(ms_fused_act), sizeof(ms_round_strides),
           sizeof(ms_actions));
    return 0;
}
"""


def test_struct_layouts_match_the_compiler(ms, tmp_path):
    cxx = next((c for c in (os.environ.get("CXX"), "c++", "g++", "clang++") if c and shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no C++ compiler")
    src, exe = tmp_path / "probe.cpp", tmp_path / "probe"
    src.write_text(PROBE)
    subprocess.run([cxx, "-std=c++17", "-I", os.path.join(REPO, "include"), "-o", str(exe), str(src)], check=True)
    rows = [[int(x) for x in line.split()]
            for line in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines()]
    A, S = ms.abi.MsFusedActAuct, ms.abi.MsRoundStridesAuct
    assert rows[0] == [ct.sizeof(A), A.auctioneer.offset, A.auct_offset.offset, A.auct_action.offset,
                       A.auct_logprob.offset]
    assert rows[1] == [ct.sizeof(S), S.auctioneer_action.offset, S.next_auct_action.offset,
                       S.next_auct_logprob.offset]
    # the structs that were there before keep their layout
    assert rows[2] == [ct.sizeof(ms.abi.MsMlpParams), ct.sizeof(ms.abi.MsFusedAct), ct.sizeof(ms.abi.MsRoundStrides),
                       ct.sizeof(ms.abi.MsActions)]
    assert rows[2] == [80, 232, 112, 32]


def test_signatures(ms):
    P, abi = ct.c_void_p, ms.abi
    head = [P, ct.POINTER(abi.MsActions), ct.POINTER(abi.MsObsOut), ct.POINTER(abi.MsRewardOut),
            ct.POINTER(abi.MsEventOut), ct.POINTER(abi.MsFusedAct), ct.POINTER(abi.MsFusedActAuct)]
    assert list(ms.lib.ms_env_step_act_auct.argtypes) == head + [P]
    assert list(ms.lib.ms_env_rollout_act_auct.argtypes) == head + [
        ct.POINTER(abi.MsRoundStrides), ct.POINTER(abi.MsRoundStridesAuct), ct.c_int32, ct.c_int32, P]
    assert list(ms.lib.ms_env_auct_supported.argtypes) == [P]


def test_null_arguments_are_refused(ms):
    """Without an env nothing can launch: MS_EINVAL and a message that names the call."""
    abi = ms.abi
    a, o, r = abi.MsActions(), abi.MsObsOut(), abi.MsRewardOut()
    nxt, au = abi.MsFusedAct(), abi.MsFusedActAuct()
    st, ast = abi.MsRoundStrides(), abi.MsRoundStridesAuct()
    assert ms.lib.ms_env_auct_supported(None) == 0
    rc = ms.lib.ms_env_step_act_auct(None, ct.byref(a), ct.byref(o), ct.byref(r), None, ct.byref(nxt), ct.byref(au),
                                     None)
    assert rc == abi.EINVAL and b"ms_env_step_act_auct" in ms.lib.ms_last_error()
    rc = ms.lib.ms_env_rollout_act_auct(None, ct.byref(a), ct.byref(o), ct.byref(r), None, ct.byref(nxt),
                                        ct.byref(au), ct.byref(st), ct.byref(ast), 4, 0, None)
    assert rc == abi.EINVAL and b"ms_env_rollout_act_auct" in ms.lib.ms_last_error()
    rc = ms.lib.ms_env_rollout_act_auct(None, ct.byref(a), ct.byref(o), ct.byref(r), None, ct.byref(nxt),
                                        ct.byref(au), ct.byref(st), None, 4, 0, None)
    assert rc == abi.EINVAL and b"strides" in ms.lib.ms_last_error()
    rc = ms.lib.ms_env_rollout_act_auct(None, ct.byref(a), ct.byref(o), ct.byref(r), None, ct.byref(nxt),
                                        ct.byref(au), ct.byref(st), ct.byref(ast), 0, 0, None)
    assert rc == abi.EINVAL and b"n_rounds" in ms.lib.ms_last_error()


REFUSED = [
    ("free prices", dict(free=True), "fixed prices"),
    ("compact=False", dict(compact=False), "compact"),
    ("hardcoded_agents", dict(hardcoded_agents=[0]), "hardcoded_agents"),
    ("empty hardcoded_agents", dict(hardcoded_agents=[]), "hardcoded_agents"),
    ("world_size", dict(world_size=2), "world_size"),
    ("diagnostics", dict(diagnostics=1), "diagnostics"),
]


@pytest.mark.parametrize("what,kw,reason", REFUSED, ids=[r[0] for r in REFUSED])
def test_trainer_refuses(ms, what, kw, reason):
    """Each refused combination is a ValueError that names the reason, raised before a device is touched (this
    test runs without one)."""
    tr = _mod("trainer")
    kw = dict(kw)
    cfg = ms.abi.named_config("cfg3" if kw.pop("free", False) else "cfg2")
    assert bool(cfg.free_prices) == (what == "free prices")
    with pytest.raises(ValueError, match=reason):
        tr.Trainer(cfg, 8, arch="global", hyper=tr.Hyper(update_step=4), seed=1, learned_auctioneer=True, **kw)


def _bare(arch, auct, seed=5):
    tr = _mod("trainer")
    t = tr.Trainer.__new__(tr.Trainer)
    t.N, t.C, t.L, t.hp, t.arch, t.rng, t.device = N, C, L, tr.Hyper(), arch, random.Random(seed), "cpu"
    t.hardcoded, t.hc_mask, t.learned = None, 0, list(range(N))
    t.auct = object() if auct else None
    return t


@pytest.mark.parametrize("arch", ["global", "local", "divided"])
def test_auctioneer_cores_are_drawn_after_the_agents_sub_units(ms, arch):
    """centralisation_sample cores, randint(0, C - 1) each, from the trainer's generator after the offer draws: the
    agents' selections are those of a trainer without the auctioneer that made the same calls before."""
    t, plain, mirror = _bare(arch, True), _bare(arch, False), random.Random(5)
    cs = t.hp.centralisation_sample
    for _ in range(50):
        sel = {k: [x.tolist() for x in v] for k, v in t._draws(device="cpu").items()}
        want = {k: [x.tolist() for x in v] for k, v in plain._draws(device="cpu").items()}
        assert "auctioneer" not in want
        cores = [[plain.rng.randint(0, C - 1)] for _ in range(cs)]  # (keeps the two generators in step)
        assert sel.pop("auctioneer") == cores and sel == want
        assert t._last_draws["auctioneer"] == cores
    assert t.rng.getstate() == plain.rng.getstate() != mirror.getstate()


def test_manifest_field_only_when_on(ms):
    ck, tr = _mod("checkpoint"), _mod("trainer")
    cfg = ms.abi.named_config("cfg2")
    base = ck.make_manifest(cfg, "global", 8, 4, tr.Hyper(), 1)
    assert "learned_auctioneer" not in base
    assert ck.make_manifest(cfg, "global", 8, 4, tr.Hyper(), 1, learned_auctioneer=False).keys() == base.keys()
    on = ck.make_manifest(cfg, "global", 8, 4, tr.Hyper(), 1, learned_auctioneer=True)
    assert on["learned_auctioneer"] is True and list(on)[:-1] == list(base)
    assert [f.name for f in __import__("dataclasses").fields(tr.Hyper)] == [
        "lr_actor", "lr_critic", "eps_clip", "acceptor_gamma", "offer_gamma", "raw_k_epochs", "centralisation_sample",
        "update_step", "extra"]  # Hyper's fields are the manifest: the feature adds none
    ck.compare_manifest(on, dict(on))
    for want, got in ((on, base), (base, on)):
        with pytest.raises(ValueError, match="learned_auctioneer"):
            ck._check_auctioneer(want, got)
        with pytest.raises(ValueError):
            ck.compare_manifest(want, got)
    ck._check_auctioneer(on, dict(on))
    ck._check_auctioneer(base, dict(base))
