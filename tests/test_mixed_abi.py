"""ABI 23 (mixed populations): the header declares ms_env_step_mixed and ms_mixed, the versions agree and
abi.MsMixed has the header's layout (no device needed)."""
import ctypes as ct
import os
import re

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    with open(os.path.join(REPO, "include", "marlsched.h")) as f:
        return f.read()


def test_header_declares_mixed_step(ms):
    src = _header()
    assert re.search(r"\bint\s+ms_env_step_mixed\s*\(\s*ms_env\s*\*\s*env,\s*const\s+ms_actions\s*\*\s*act,\s*"
                     r"const\s+ms_mixed\s*\*\s*mix,", src)
    assert re.search(r"typedef\s+struct\s+ms_mixed\s*\{", src)
    assert "ms_env_step_mixed" in ms._lib.EXPORTED
    assert hasattr(ct.CDLL(ms.LIB_PATH), "ms_env_step_mixed") and ms._lib.has("ms_env_step_mixed")


def test_abi_version(ms):
    version = int(re.search(r"#define\s+MS_ABI_VERSION\s+(\d+)", _header()).group(1))
    assert version == ms._lib.ABI_VERSION == ms._lib.ABI_LOADED and version >= 23


def test_ms_mixed_layout(ms):
    body = re.search(r"typedef\s+struct\s+ms_mixed\s*\{(.*?)\}\s*ms_mixed\s*;", _header(), re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [re.match(r"\s*(.*?)\s*(\w+)$", d.strip()).groups() for d in body.split(";") if d.strip()]
    assert fields == [("uint64_t", "hardcoded_agents"), ("int8_t*", "acceptor_taken"), ("int8_t*", "offer_core_taken")]
    # the C layout of those declarations: a uint64_t and two pointers, each 8 bytes and 8-aligned
    M = ms.abi.MsMixed
    assert [name for name, _ in M._fields_] == [name for _, name in fields]
    assert ct.sizeof(M) == 24
    assert [getattr(M, name).offset for name, _ in M._fields_] == [0, 8, 16]
    assert [getattr(M, name).size for name, _ in M._fields_] == [8, 8, 8]
