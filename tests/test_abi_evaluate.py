"""ms_policy_evaluate at the C boundary without a device: _lib.py's signature against the declaration in
include/marlsched.h, and the ABI version on both sides."""
import ctypes as ct
import os
import re

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

C_TYPES = {"int32_t": ct.c_int32, "int64_t": ct.c_int64, "uint64_t": ct.c_uint64, "int": ct.c_int}


def _header():
    with open(os.path.join(REPO, "include", "marlsched.h")) as f:
        return f.read()


def _ctype(decl, ms):
    """The ctypes type _lib.py should give a C parameter declaration."""
    decl = decl.strip()
    if "*" in decl:
        base = decl.replace("const", "").split("*")[0].strip()
        return ct.POINTER(ms.abi.MsMlpParams) if base == "ms_mlp_params" else ct.c_void_p
    return C_TYPES[decl.rsplit(" ", 1)[0].strip()]


def test_abi_version_matches_header(ms):
    want = int(re.search(r"#define\s+MS_ABI_VERSION\s+(\d+)", _header()).group(1))
    assert ms._lib.ABI_VERSION == want
    assert int(ms.lib.ms_abi_version()) == want


def test_evaluate_signature_matches_header(ms):
    m = re.search(r"\bint\s+ms_policy_evaluate\s*\(([^)]*)\)\s*;", _header())
    assert m, "ms_policy_evaluate is not declared"
    params = [p for p in re.sub(r"\s+", " ", m.group(1)).split(",")]
    names = [re.findall(r"[A-Za-z_][A-Za-z0-9_]*", p)[-1] for p in params]
    assert names == ["actor", "critic", "obs", "obs_stride", "n_envs", "n_units", "units_per_group", "actions",
                     "logprob", "value", "entropy", "stream"]
    fn = ms.lib.ms_policy_evaluate
    assert fn.restype is ct.c_int
    assert list(fn.argtypes) == [_ctype(p, ms) for p in params]
    assert ms._lib.has("ms_policy_evaluate") and "ms_policy_evaluate" in ms._lib.EXPORTED


def test_lenient_set_takes_abi_24():
    """An ABI 24 library built before ms_policy_evaluate loads (the entry point is optional, found with has()), and
    24 is in the set MARLSCHED_LENIENT_ABI=1 accepts (read from the source: the set is local to the loader)."""
    with open(os.path.join(REPO, "marl-scheduling_amd", "_lib.py")) as f:
        src = f.read()
    m = re.search(r"MARLSCHED_LENIENT_ABI\"\)\s*==\s*\"1\"\s*and\s*version\s+in\s*\(([^)]*)\)", src)
    assert m and 24 in [int(x) for x in m.group(1).split(",")]
