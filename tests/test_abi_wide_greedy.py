"""ms_wide_act_greedy at the C boundary without a device: _lib.py's signature and abi.py's parameter struct
against the declarations in include/marlsched.h, the export list, the launcher's single declaration, and the ABI
version on both sides (unchanged: the entry point is optional, found with has())."""
import ctypes as ct
import os
import re

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

C_TYPES = {"int32_t": ct.c_int32, "int64_t": ct.c_int64}


def _read(*parts):
    with open(os.path.join(REPO, *parts)) as f:
        return f.read()


def _header():
    return _read("include", "marlsched.h")


def _params(name):
    m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, _header())
    assert m, "%s is not declared" % name
    return [re.sub(r"\s+", " ", p).strip() for p in m.group(1).split(",")]


def test_abi_version_is_still_24(ms):
    want = int(re.search(r"#define\s+MS_ABI_VERSION\s+(\d+)", _header()).group(1))
    assert want == 24 and ms._lib.ABI_VERSION == 24 and int(ms.lib.ms_abi_version()) == 24


def test_signature_matches_header(ms):
    assert _params("ms_wide_act_greedy") == [
        "const ms_mlp_params* actor", "const int8_t* obs", "int32_t obs_stride", "int64_t n_rows", "int32_t* action",
        "float* logprob", "void* stream"]
    fn = ms.lib.ms_wide_act_greedy
    assert fn.restype is ct.c_int
    want = [ct.POINTER(ms.abi.MsMlpParams) if p.startswith("const ms_mlp_params*")
            else ct.c_void_p if "*" in p else C_TYPES[p.split(" ")[0]] for p in _params("ms_wide_act_greedy")]
    assert list(fn.argtypes) == want
    # ms_wide_act's arguments without the uniforms, in its order
    sample = _params("ms_wide_act")
    assert [p for p in sample if p != "const float* uniforms"] == _params("ms_wide_act_greedy")


def test_declared_next_to_ms_wide_act():
    h = _header()
    assert h.index("int ms_wide_act(") < h.index("int ms_wide_act_greedy(") < h.index("typedef struct ms_wide_batch")


def test_name_is_exported_and_optional(ms):
    assert "ms_wide_act_greedy" in ms._lib.EXPORTED and ms._lib.has("ms_wide_act_greedy")
    assert hasattr(ct.CDLL(ms.LIB_PATH), "ms_wide_act_greedy")
    src = _read("marl-scheduling_amd", "_lib.py")
    optional = src[src.index("optional = {"):src.index("sig.update(")]
    assert '"ms_wide_act_greedy"' in optional


def test_param_struct_matches_header(ms):
    body = re.search(r"typedef struct ms_mlp_params \{(.*?)\} ms_mlp_params;", _header(), re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = []
    for decl in body.split(";"):
        decl = " ".join(decl.split())
        if not decl:
            continue
        if "*" in decl:
            names += [n.strip().lstrip("*") for n in decl.split("*", 1)[1].split(",")]
        else:
            names += [n.strip() for n in decl.split(" ", 1)[1].split(",")]
    assert names == [n for n, _ in ms.abi.MsMlpParams._fields_]


def test_launcher_and_args_declared_once():
    hdr = _read("marl-scheduling_amd", "csrc", "ms_wide.h")
    assert len(re.findall(r"\bstruct WideGreedy\b", hdr)) == 1
    assert len(re.findall(r"hipError_t launch_wide_greedy\(", hdr)) == 1
    for unit in ("capi.cpp", "wide_kernels.hip"):
        src = _read("marl-scheduling_amd", "csrc", unit)
        assert "struct WideGreedy" not in src
        assert len(re.findall(r"hipError_t\s+launch_wide_greedy\(", src)) == (1 if unit.endswith(".hip") else 0)


def test_wrapper_signature(ms):
    import importlib
    import inspect
    ppo = importlib.import_module("marl-scheduling_amd.ppo")
    sig = inspect.signature(ppo.PPOGroup.wide_act_greedy)
    assert list(sig.parameters) == ["self", "obs_i8", "action", "logprob", "want_logprob", "stream"]
    assert sig.parameters["want_logprob"].default is True
