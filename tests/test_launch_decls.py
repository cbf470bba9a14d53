"""Every host function that crosses a translation unit of csrc/ is declared once, in a header (text only: no
library, no device). A prototype written into the calling file is checked against its definition by the linker's
mangled name alone, which two swapped neighbours of one type pass."""
import glob
import os
import re

CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "marl-scheduling_amd", "csrc")
CROSS = r"(?:launch_\w+|dispatch_\w+|act_frag_bytes|acc_common_tables|ppo_pa\w+)"
# a function head at column 0: specifiers and return type, name, parameter list, then `{` or `;`
HEAD = r"^(\w[\w:<>*& ]*?[ *&])(%s)\(([^;{}]*?)\)\s*(\{|;)"


def _read(pattern):
    return {os.path.basename(p): open(p).read() for p in sorted(glob.glob(os.path.join(CSRC, pattern)))}


def _heads(text, name=r"\w+"):
    return [(m.group(1), m.group(2), m.group(4)) for m in re.finditer(HEAD % name, text, re.M)]


def test_cross_unit_functions_are_declared_once_in_a_header():
    headers = _read("*.h")
    defined = [(unit, name) for unit, text in _read("*.hip").items()
               for spec, name, end in _heads(text, CROSS) if end == "{" and "static" not in spec.split()]
    assert len(defined) >= 35 and ("policy_kernels.hip", "dispatch_act") in defined  # the pattern still finds them
    for unit, name in defined:
        where = [h for h, text in headers.items() for _, _, end in _heads(text, name) if end == ";"]
        assert len(where) == 1, f"{name} ({unit}) is declared in {where or 'no header'}: exactly one header must"


def test_no_unit_declares_a_function_it_does_not_define():
    for unit, text in {**_read("*.hip"), **_read("*.cpp")}.items():
        heads = _heads(text)
        defined = {name for _, name, end in heads if end == "{"}
        foreign = sorted({name for _, name, end in heads if end == ";"} - defined)
        assert not foreign, f"{unit} declares {foreign} without defining them: the declarations belong in a header"
