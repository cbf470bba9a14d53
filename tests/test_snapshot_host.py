"""The packed env snapshot's section offsets and per-replica check (ms_snapshot.h) on the host
(tests/snapshot_check.cpp, compiled with the system C++ compiler: the header needs no HIP), plain and under
-fsanitize=address,undefined. The validate kernel and ms_env_restore apply the same functions."""
import os
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build_and_run(tmp_path_factory, name, flags):
    cxx = next((c for c in (os.environ.get("CXX"), "c++", "g++", "clang++") if c and shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no C++ compiler")
    exe = str(tmp_path_factory.mktemp(name) / "snapshot_check")
    cmd = [cxx, "-std=c++17", "-O1", "-g", *flags, "-o", exe, os.path.join(REPO, "tests", "snapshot_check.cpp")]
    # the sanitizer runtimes linked into the program where the compiler knows the flags (gcc): the program then
    # runs whatever else the process environment makes the loader bring in first
    static = ["-static-libasan", "-static-libubsan"] if flags else []
    if subprocess.call(cmd + static, stderr=subprocess.DEVNULL) != 0:
        subprocess.check_call(cmd)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True, env=env)
    return r.returncode, r.stdout.splitlines(), r.stderr


@pytest.fixture(scope="module")
def plain(tmp_path_factory):
    return _build_and_run(tmp_path_factory, "snapshot_plain", [])


@pytest.fixture(scope="module")
def sanitized(tmp_path_factory):
    return _build_and_run(tmp_path_factory, "snapshot_san", ["-fsanitize=address,undefined", "-fno-omit-frame-pointer"])


def _no_failures(run):
    rc, lines, err = run
    fails = [l for l in lines if l.startswith("FAIL")]
    assert not fails, "\n".join(fails[:20])
    assert rc == 0, err[-2000:]
    n_layouts, n_replicas = (int(x) for x in next(l for l in lines if l.startswith("checked")).split()[1:])
    # 8 shapes x 7 E x 5 counts; the valid replicas and at least one per invariant of ms_env_import's loop
    assert n_layouts == 280 and n_replicas >= 4 + 14


def test_layout_and_replica_check(plain):
    _no_failures(plain)


def test_layout_and_replica_check_sanitized(sanitized):
    """The same program under AddressSanitizer and UBSan: the check reads nothing beyond the record and the
    `count` entries it is given, whatever liab_n claims."""
    _no_failures(sanitized)
    assert "Sanitizer" not in sanitized[2] and "runtime error" not in sanitized[2]


def test_cfg3_offsets(plain):
    """8 x 8 x 3 (cfg3) at E = 16384 with 19 entries per replica: the sections byte for byte. 320-byte records
    behind the 64-byte header and the 408-byte config; about 49 MB against 221 MB of device state."""
    _, lines, _ = plain
    v = [int(x) for x in next(l for l in lines if l.startswith("layout 8 8 3 16384")).split()[6:]]
    E, n = 16384, 19 * 16384
    o_cfg, o_recs, o_mt, o_off, o_liab, total = v
    assert (o_cfg, o_recs) == (64, 480)
    assert o_mt == 480 + E * 320 and o_off == o_mt + E * 2496
    assert o_liab == o_off + 8 * (E + 1) + 8 and total == o_liab + 8 * n
    assert total < 0.23 * E * (320 + 2 * 2496 + 8 * 128 * 8)
