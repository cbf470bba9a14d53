"""The LDS plan of the one-launch free-price rollout (ms_layout.h free_lds) checked on the host for every shape
the config check accepts (tests/lds_plan_check.cpp, compiled with the system C++ compiler: the header needs no HIP).

A wave of k_env_rollout_act_free twists an MT19937 block (4 * 624 B) at the start of its env slot while the
other waves' slots and the act area behind the slots are live. 1 x 1 x 16 has a slot of 4 * 608 = 2432 B: its
twist used to run 64 B into the price-key digit table. The program checks, for every shape, that each wave's
twist stays in bytes nothing else uses, that the act areas do not overlap and that the 160 KiB budget is what
free_rollout_lds_ok tests; env_rollout_free_supported and the kernel read the same header."""
import os
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    cxx = next((c for c in (os.environ.get("CXX"), "c++", "g++", "clang++") if c and shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no C++ compiler")
    exe = str(tmp_path_factory.mktemp("lds_plan") / "lds_plan_check")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-o", exe, os.path.join(REPO, "tests", "lds_plan_check.cpp")])
    r = subprocess.run([exe], stdout=subprocess.PIPE, universal_newlines=True)
    return r.returncode, r.stdout.splitlines()


def test_every_shape_keeps_the_twist_out_of_live_lds(plan):
    rc, lines = plan
    fails = [l for l in lines if l.startswith("FAIL")]
    assert not fails, "\n".join(fails[:20])
    assert rc == 0
    n_shape, n_supported = (int(x) for x in next(l for l in lines if l.startswith("count")).split()[1:])
    # the enumeration is not empty, and the LDS budget refuses some shapes that pass the shape terms
    assert 0 < n_supported < n_shape


def test_layout_of_the_shipped_shapes(plan):
    """8 x 8 x 3 (cfg3, the benchmark's kernel): the plan of the header before the padding, byte for byte.
    1 x 1 x 16: pdig starts where the one wave's twist ends."""
    _, lines = plan
    lds = {tuple(int(x) for x in l.split()[1:4]): [int(x) for x in l.split()[4:]] for l in lines if l.startswith("lds")}
    assert lds[(8, 8, 3)] == [66560, 68608, 73216, 75264, 75296]  # pdig, list, accx, pace, total
    assert lds[(1, 1, 16)][0] == 4 * 624
