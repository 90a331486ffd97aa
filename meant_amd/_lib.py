"""ctypes binding of libmeant_hip.so, derived at import from include/meant_hip.h.

The header is the only declaration of the C ABI.  The compiler checks every `extern "C"` definition against it; this module reads the
same file for every signature (SIGNATURES) and every enumerator (F32, EPI_GELU, MASK_U8, ERR_ARG, KV_LIST_HDR, ...: the header's names
without their MEANT_ prefix).  A new entry point is bound by declaring it there and defining it: nothing is added here.

The product path has exactly one backend.  If the shared library or the header is missing, or the header holds something this module
cannot bind, the import raises: there is no CPU or PyTorch-eager fallback (by design -- see DESIGN.md) and no type is guessed.
"""
from __future__ import annotations

import ctypes as C
import os
import re

# torch first: its bundled HIP runtime carries the soname libamdhip64.so.7 that the library links against, so the dlopen below
# binds to the runtime torch drives the GPU with.  Loaded the other way round, the process maps a second HIP / HSA runtime and
# the library's launches find no device.
import torch  # noqa: F401

_HERE = os.path.dirname(os.path.abspath(__file__))
# MEANT_LIB_PATH: load another build of the same ABI (A/B measurements of one kernel against an older build)
LIB_PATH = os.environ.get("MEANT_LIB_PATH") or os.path.join(_HERE, "libmeant_hip.so")
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "meant_hip.h")


class MeantLibraryMissing(ImportError):
    pass


class MeantHeaderError(ImportError):
    pass


_VALUE_TYPES = {"int": C.c_int, "int32_t": C.c_int32, "uint32_t": C.c_uint32, "int64_t": C.c_int64, "uint64_t": C.c_uint64,
                "size_t": C.c_size_t, "float": C.c_float}


def _ctype(text, fn):
    """the ctypes type of one C type as the header spells it.  Callers hand device addresses over as Python ints (`t.data_ptr() + n`),
    which a typed POINTER would refuse: every pointer but `const char*` is c_void_p.  A type outside the table stops the import."""
    words = text.replace("*", " * ").split()
    if "*" in words:
        return C.c_char_p if words == ["const", "char", "*"] else C.c_void_p
    if " ".join(words) not in _VALUE_TYPES:
        raise MeantHeaderError(f"{fn}: no ctypes type for the C type `{' '.join(words)}`")
    return _VALUE_TYPES[" ".join(words)]


def parse_header(src):
    """({function: (restype, [argtypes])}, {enumerator: value}) of the text of a C header as regular as include/meant_hip.h.  With the
    comments, the preprocessor lines, the enums and the extern "C" wrapper taken out, every statement left has to be a declaration
    `ret meant_name(type name, ...);` of known types, or the header is refused: a declaration is never skipped."""
    src = re.sub(r"/\*.*?\*/|//[^\n]*|^[ \t]*#[^\n]*", " ", src, flags=re.S | re.M)
    constants, signatures = {}, {}

    def enum(m):
        for item in m.group(1).split(","):
            e = re.fullmatch(r"\s*(\w+)\s*=\s*(-?\d+)\s*", item)
            if not e:
                raise MeantHeaderError(f"enumerator `{item.strip()}`: expected `NAME = integer`")
            constants[e.group(1)] = int(e.group(2))
        return ""
    src = re.sub(r"\benum\b[^{;]*\{([^}]*)\}\s*;", enum, src)
    src = re.sub(r'extern\s+"C"\s*\{(.*)\}', r"\1", src, flags=re.S)
    for stmt in filter(None, (s.strip() for s in src.split(";"))):
        m = re.fullmatch(r"([\w\s*]+?)\b(meant_\w+)\s*\(([^()]*)\)", stmt)
        if not m:
            raise MeantHeaderError(f"not a declaration of a meant_* function: `{' '.join(stmt.split())[:80]}`")
        ret, fn, params = m.groups()
        argtypes = []
        for p in [] if params.strip() == "void" else params.split(","):
            named = re.fullmatch(r"(.*[\s*])\w+", p.strip(), flags=re.S)
            if not named:
                raise MeantHeaderError(f"{fn}: parameter `{p.strip()}` is not `type name`")
            argtypes.append(_ctype(named.group(1), fn))
        signatures[fn] = (None if ret.split() == ["void"] else _ctype(ret, fn), argtypes)
    return signatures, constants


if not os.path.exists(HEADER_PATH):
    raise MeantHeaderError(f"{HEADER_PATH} not found: the signatures of libmeant_hip.so are read from it (include/ travels with "
                           f"meant_amd/).  There is no second copy of them to fall back to.")
with open(HEADER_PATH) as _f:
    # name -> (restype, argtypes) of every entry point; every enumerator of the header under its full name
    SIGNATURES, CONSTANTS = parse_header(_f.read())
# F32, BF16 | RAW_F32 .. RAW_U8 | MASK_F32 .. MASK_I32 | OK, ERR_ARG .. ERR_WORKSPACE | EPI_NONE .. EPI_SIGMOID | KV_LIST_HDR
globals().update({name.removeprefix("MEANT_"): value for name, value in CONSTANTS.items()})


def _load():
    if not os.path.exists(LIB_PATH):
        raise MeantLibraryMissing(
            f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            f"(or `make -C meant_amd/csrc`).  meant_amd has no CPU / eager fallback.")
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)          # AttributeError here == header and library out of sync
        fn.restype = res
        fn.argtypes = args
    return lib


lib = _load()


def set_option(name: str, value: int) -> None:
    check(lib.meant_set_option(name.encode(), int(value)), "set_option")


def get_option(name: str) -> int:
    v = C.c_int(0)
    check(lib.meant_get_option(name.encode(), C.byref(v)), "get_option")
    return v.value


def route_count(route: str) -> int:
    n = lib.meant_route_count(route.encode())
    if n < 0:
        raise KeyError(route)
    return n


def route_reset() -> None:
    lib.meant_route_reset()


class MeantHipError(RuntimeError):
    pass


def check(rc: int, what: str = "") -> None:
    if rc != 0:
        msg = lib.meant_last_error().decode("utf-8", "replace")
        raise MeantHipError(f"{what or 'libmeant_hip'} failed (status {rc}): {msg}")
