"""ms_action_table at the C boundary without a device: _lib.py's signature and abi.py's struct against the
declarations in include/marlsched.h, the export list, and the ABI version on both sides (unchanged: the entry point
is optional, found with has())."""
import ctypes as ct
import os
import re

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

C_TYPES = {"int32_t": ct.c_int32, "int64_t": ct.c_int64}


def _header():
    with open(os.path.join(REPO, "include", "marlsched.h")) as f:
        return f.read()


def test_abi_version_is_still_24(ms):
    want = int(re.search(r"#define\s+MS_ABI_VERSION\s+(\d+)", _header()).group(1))
    assert want == 24 and ms._lib.ABI_VERSION == 24 and int(ms.lib.ms_abi_version()) == 24


def test_signature_matches_header(ms):
    m = re.search(r"\bint\s+ms_action_table\s*\(([^)]*)\)\s*;", _header())
    assert m, "ms_action_table is not declared"
    params = [re.sub(r"\s+", " ", p).strip() for p in m.group(1).split(",")]
    assert params == ["const ms_action_table_args* args", "void* stream"]
    fn = ms.lib.ms_action_table
    assert fn.restype is ct.c_int
    assert list(fn.argtypes) == [ct.POINTER(ms.abi.MsActionTableArgs), ct.c_void_p]


def test_name_is_exported(ms):
    assert "ms_action_table" in ms._lib.EXPORTED and ms._lib.has("ms_action_table")
    assert hasattr(ct.CDLL(ms.LIB_PATH), "ms_action_table")


def test_struct_matches_header(ms):
    body = re.search(r"typedef struct ms_action_table_args \{(.*?)\} ms_action_table_args;", _header(), re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in body.split(";"):
        decl = " ".join(decl.split())
        if not decl:
            continue
        if "*" in decl:
            fields.append((decl.rsplit("*", 1)[1].strip(), ct.c_void_p))
            continue
        ctype, names = decl.split(" ", 1)
        fields += [(n.strip(), C_TYPES[ctype]) for n in names.split(",")]
    assert fields == list(ms.abi.MsActionTableArgs._fields_)
    # the histogram's struct and constants are as they were: the table has its own struct and no MS_HIST_* name
    assert set(re.findall(r"#define\s+MS_HIST_(\w+)", _header())) == {"ALL", "GATED", "OWNER"}
