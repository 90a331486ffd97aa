"""CPU-side checks of the binding that meant_amd/_lib.py derives from include/meant_hip.h: the parser on a synthetic header, argument
lists typed by hand here against the derived ones, the loaded library's prototypes, and the header's constants as Python names."""
import ctypes as C
import os
import shutil
import subprocess
import sys

import pytest
import torch

_p, _i, _i64, _f, _u64, _sz, _u32, _s = C.c_void_p, C.c_int, C.c_int64, C.c_float, C.c_uint64, C.c_size_t, C.c_uint32, C.c_char_p

SYNTHETIC = """
/* a comment with a declaration in it: int meant_fake(int x); and meant_other(rows, d) */
#ifndef SYNTHETIC_H
#define SYNTHETIC_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif
enum meant_kind { MEANT_A = 0, MEANT_B = 7 };   // int meant_fake2(void);
enum meant_code {
  MEANT_FINE = 0,
  MEANT_BAD = -3   /* worse; than fine */
};
int meant_zero(void);
const char* meant_text(void);
size_t meant_bytes(int64_t rows, int32_t d);
int meant_three_lines(const void* x, const float *scale, float* y,
                      int64_t rows, uint64_t seed /* a, b; c */,
                      uint32_t t, float eps, const char* name, const int64_t* ids, void* stream);
void meant_nothing(int flag);
#ifdef __cplusplus
}
#endif
#endif
"""


def test_parser_on_a_synthetic_header():
    """a declaration over three lines, comments that hold declarations and semicolons, (void), a `const char*` and a size_t return,
    the star on either side of the space, a void return: exactly this dict and nothing else"""
    from meant_amd import _lib
    sigs, consts = _lib.parse_header(SYNTHETIC)
    assert sigs == {
        "meant_zero": (_i, []),
        "meant_text": (_s, []),
        "meant_bytes": (_sz, [_i64, C.c_int32]),
        "meant_three_lines": (_i, [_p, _p, _p, _i64, _u64, _u32, _f, _s, _p, _p]),
        "meant_nothing": (None, [_i]),
    }
    assert consts == {"MEANT_A": 0, "MEANT_B": 7, "MEANT_FINE": 0, "MEANT_BAD": -3}


@pytest.mark.parametrize("decl,named", [
    ("int meant_takes_double(const void* x, double eps);", "meant_takes_double"),
    ("int meant_takes_struct(struct meant_cfg cfg, int n);", "meant_takes_struct"),
    ("double meant_returns_double(int n);", "meant_returns_double"),
    ("int meant_unnamed(int64_t, int n);", "meant_unnamed"),
    ("int meant_void_value(void x);", "meant_void_value"),
    ("int meant_callback(void (*fn)(int), int n);", "meant_callback"),
    ("int other_prefix(int n);", "other_prefix"),
    ("enum meant_kind { MEANT_IMPLICIT };", "MEANT_IMPLICIT"),
])
def test_parser_refuses_what_it_cannot_bind(decl, named):
    """a type outside the table, an unnamed parameter or a statement that is no meant_* declaration stops the parse with an ImportError
    that names it: no type is guessed and no declaration skipped"""
    from meant_amd import _lib
    with pytest.raises(ImportError, match=named):
        _lib.parse_header("int meant_before(int n);\n" + decl + "\nint meant_after(int n);\n")


def test_hand_typed_signatures_match_the_derived_ones():
    """argument lists typed here by hand from the header, one entry point per kind of list; together they hold every type the ABI
    uses.  meant_get_option's `int*` is a c_void_p like every other pointer (it takes the byref() that get_option passes)"""
    from meant_amd import _lib
    pins = {
        "meant_version": (_i, []),
        "meant_last_error": (_s, []),
        "meant_route_reset": (None, []),
        "meant_set_option": (_i, [_s, _i]),
        "meant_get_option": (_i, [_s, _p]),
        "meant_rmsnorm_bwd_ws": (_sz, [_i64, _i64]),
        "meant_linear_bwd_dw_rows": (_i, [_p, _i64, _p, _i64, _p, _p, _p, _p, _i64, _i64, _i64, _i, _p, _sz, _p]),
        "meant_gemm_f32_strided": (_i, [_p, _p, _p, _i64, _i64, _i64, _i64, _i64, _p, _p, _p, _f, _i, _p]),
        "meant_mlm_mask": (_i, [_p, _p, _i, _p, _i64, _i64, _p, _i, _i64, _i64, _u64, _u32, _u32, _u32, _i64, _i64, _i64, _p, _p, _p]),
        "meant_rmsnorm_bwd_chain": (_i, [_p, _i, _p, _p, _p, _p, _p, _i64, _i64, _i64, _f, _f, _u64, _p, _p, _p, _f, _i64, _p, _p, _i, _p, _sz, _p]),
        "meant_mim_l1_fwd": (_i, [_p, _i, _p, _i, _f, _f, _i64, _i, _i, _i, _i, _u64, _u32, _p, _i64, _i64, _f, _i, _p, _p, _p, _sz, _p]),
    }
    assert len(pins["meant_rmsnorm_bwd_chain"][1]) == 24 and len(pins["meant_mim_l1_fwd"][1]) == 23
    for name, want in pins.items():
        assert _lib.SIGNATURES[name] == want, name
    assert _p.from_param(C.byref(C.c_int())) is not None
    assert _lib.get_option("nt_pp") == 1                 # through the c_void_p: a pure host call


def test_loaded_library_carries_the_derived_prototypes():
    from meant_amd import _lib
    assert len(_lib.SIGNATURES) >= 96
    for name, (res, args) in _lib.SIGNATURES.items():
        fn = getattr(_lib.lib, name)
        assert fn.restype is res and list(fn.argtypes) == args, name
    with pytest.raises(TypeError):
        _lib.lib.meant_rmsnorm_bwd_ws(1)                 # one argument too few: refused before anything is called
    assert _lib.lib.meant_rmsnorm_bwd_ws(1, 8) >= 0


def test_header_constants_are_the_python_names():
    from meant_amd import _lib, ops
    assert (_lib.F32, _lib.BF16) == (0, 1)
    assert (_lib.RAW_F32, _lib.RAW_BF16, _lib.RAW_F64, _lib.RAW_U8) == (0, 1, 2, 3)
    assert (_lib.EPI_NONE, _lib.EPI_GELU, _lib.EPI_RESIDUAL, _lib.EPI_SIGMOID) == (0, 1, 2, 4)
    assert (_lib.MASK_F32, _lib.MASK_BF16, _lib.MASK_I64, _lib.MASK_U8, _lib.MASK_I32) == (0, 1, 2, 3, 4)
    assert (_lib.OK, _lib.ERR_ARG, _lib.ERR_UNSUPPORTED, _lib.ERR_LAUNCH, _lib.ERR_WORKSPACE) == (0, -1, -2, -3, -4)
    assert _lib.CONSTANTS["MEANT_ERR_WORKSPACE"] == -4
    assert ops._MASK_DTYPES[torch.bool] == _lib.MASK_U8 == ops._MASK_DTYPES[torch.uint8]
    assert ops._MASK_DTYPES == {torch.float32: 0, torch.bfloat16: 1, torch.int64: 2, torch.uint8: 3, torch.bool: 3, torch.int32: 4}


def test_kv_list_header_has_one_value():
    """the header length of the meant_kv_live_rows buffer, as the binding, ops and the library's own size query see it"""
    from meant_amd import _lib, ops
    assert ops.KV_LIST_HEADER == _lib.KV_LIST_HDR == 64
    # G = 1, S = 256: nblk = 4 blocks, npan = 1 panel; header + blocks + live panels + dead panels + nblk words of scratch
    assert _lib.lib.meant_kv_live_rows_ws(1, 256) == (64 + 2 * 4 + 2 * 1) * 4


def test_import_without_the_header_raises(tmp_path):
    """_lib.py on its own, with the built library but no include/ beside it: an ImportError that names the header, no fallback"""
    from meant_amd import _lib
    os.makedirs(tmp_path / "pkg")
    shutil.copy(_lib.__file__, tmp_path / "pkg" / "_lib.py")
    out = subprocess.run([sys.executable, "-c", "import _lib"], cwd=tmp_path / "pkg", env=dict(os.environ, MEANT_LIB_PATH=_lib.LIB_PATH),
                         capture_output=True, text=True)
    assert out.returncode != 0
    assert "MeantHeaderError" in out.stderr and "meant_hip.h not found" in out.stderr, out.stderr[-500:]
