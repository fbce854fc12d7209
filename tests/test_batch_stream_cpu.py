"""Batched streaming, host side: the ABI revision, the header's declarations of sts_infer_ids_batch_stream / sts_pool_submit_stream /
sts_batch_chunk_cb, the library's exports, and the Python argtypes against the header's prototypes."""
import ctypes as C
import os
import re

from summertts_amd import engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "summertts_hip.h")
NEW = ("sts_infer_ids_batch_stream", "sts_pool_submit_stream")


def _header():
    return re.sub(r"/\*.*?\*/", " ", open(HDR).read(), flags=re.S)


def _params(decl):
    """'int32_t a, const float* b, ...' -> the C types without the parameter names"""
    out = []
    for p in decl.split(","):
        p = " ".join(p.replace("*", " * ").split())
        m = re.match(r"^(.*?)\s*([A-Za-z_]\w*)$", p)
        t = m.group(1) if m and m.group(1) and not m.group(1).endswith(("const", "struct")) else p
        out.append(t.replace(" *", "*").strip())
    return out


def _ctype(t):
    if "*" in t:
        return C.c_void_p
    return {"int32_t": C.c_int32, "int64_t": C.c_int64, "uint64_t": C.c_uint64, "float": C.c_float, "int": C.c_int,
            "sts_chunk_cb": engine.CHUNK_CB, "sts_batch_chunk_cb": engine.BATCH_CHUNK_CB}[t]


def test_abi_version_is_10():
    assert engine.load_library().sts_abi_version() >= 10


def test_header_declares_and_library_exports():
    hdr = _header()
    lib = engine.load_library()
    for s in NEW:
        assert re.search(r"\b" + s + r"\s*\(", hdr), s
        assert s in engine.EXPORTED_SYMBOLS and hasattr(lib, s), s
    assert re.search(r"typedef\s+int\s*\(\s*\*\s*sts_batch_chunk_cb\s*\)", hdr)
    assert re.search(r"\bSTS_DBG_STREAM_RETRY_STEP\s*=\s*16\b", hdr)


def test_python_callbacks_match_the_header():
    hdr = _header()
    for name, proto in (("sts_chunk_cb", engine.CHUNK_CB), ("sts_batch_chunk_cb", engine.BATCH_CHUNK_CB)):
        m = re.search(r"typedef\s+int\s*\(\s*\*\s*" + name + r"\s*\)\s*\(([^)]*)\)", hdr)
        assert m, name
        assert proto._restype_ is C.c_int
        assert list(proto._argtypes_) == [C.POINTER(C.c_int16) if t == "const int16_t*" else _ctype(t) for t in _params(m.group(1))], name


def test_python_argtypes_match_the_header():
    """The ctypes argtypes (summertts_amd/engine.py load_library) of the two new entry points name the header's parameter types in the
    header's order (pointers as c_void_p, the callbacks as engine.CHUNK_CB / BATCH_CHUNK_CB), and the return types agree."""
    hdr = _header()
    lib = engine.load_library()
    for s in NEW:
        m = re.search(r"\b(int|int64_t)\s+" + s + r"\s*\(([^)]*)\)\s*;", hdr)
        assert m, s
        want = [_ctype(t) for t in _params(m.group(2))]
        fn = getattr(lib, s)
        assert list(fn.argtypes) == want, s
        assert fn.restype is {"int": C.c_int, "int64_t": C.c_int64}[m.group(1)], s
