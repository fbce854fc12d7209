"""CPU suite: the workspace-poisoning test hook (include/summertts_hip.h STS_DBG_POISON, sts_profile.poison_bytes) as the header
declares it and the Python binding mirrors it.  No compiler and no GPU needed: the header's struct is laid out from its parsed field list."""
import ctypes as C
import os
import re

import pytest

from conftest import ROOT
from summertts_amd import engine

HEADER = os.path.join(ROOT, "include", "summertts_hip.h")
CTYPES_OF = {"float": C.c_float, "double": C.c_double, "int32_t": C.c_int32, "int64_t": C.c_int64}


def _struct_fields(name):
    src = open(HEADER).read()
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), src, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    out = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            ctype, names = decl.split(None, 1)
            out += [(n.strip(), CTYPES_OF[ctype]) for n in names.split(",")]
    return out


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(engine.LIB_PATH):
        engine.build_library()
    return engine.load_library()


def test_header_declares_the_poison_key():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert re.search(r"\bSTS_DBG_POISON\s*=\s*18\b", src)
    # the key must not collide with any other test hook
    keys = [int(v) for v in re.findall(r"\bSTS_DBG_[A-Z0-9_]+\s*=\s*(\d+)", src)]
    assert keys.count(18) == 1 and len(keys) == len(set(keys)), keys


def test_abi_version_counts_the_poison_field(lib):
    assert lib.sts_abi_version() >= 12
    assert re.search(r"#define STS_ABI_VERSION (\d+)", open(HEADER).read()).group(1) == str(lib.sts_abi_version())


def test_profile_mirror_ends_in_poison_bytes_and_has_the_header_size():
    fields = _struct_fields("sts_profile")
    assert fields[-1] == ("poison_bytes", C.c_int64)
    assert [(n, t) for n, t in engine.Profile._fields_] == fields

    class HeaderLayout(C.Structure):          # the C layout of the header's field list (natural alignment, as the C compiler lays it out)
        _fields_ = fields
    assert C.sizeof(engine.Profile) == C.sizeof(HeaderLayout)
    assert engine.Profile.poison_bytes.offset == HeaderLayout.poison_bytes.offset
    assert engine.Profile.poison_bytes.offset + 8 <= C.sizeof(engine.Profile)

