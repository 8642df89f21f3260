"""CPU: the C ABI of the multi-leg stacking entry point (genie_stack_windows_legs) -- declared in the header, bound in `_lib.SYMBOLS`
with the header's argument types, exported by the built library -- and the one leg limit the day's passes share."""
import ctypes
import os
import re

from genie_amd import _lib, engine, postproc


def test_stack_legs_symbol_is_declared_bound_and_exported():
    header = open(os.path.join(_lib.INCLUDE, "genie_hip.h")).read()
    m = re.search(r"\bint\s+genie_stack_windows_legs\s*\(([^)]*)\)\s*;", header)
    assert m, "genie_stack_windows_legs is not declared in genie_hip.h"
    declared = [" ".join(a.split()) for a in m.group(1).split(",")]
    assert declared == ["const float* const* x_legs", "int n_legs", "const int32_t* cols", "int n_windows", "int64_t n_query",
                        "int n_offsets", "float scale", "float* out", "int64_t n_cols", "int64_t c_min", "int64_t c_max", "void* stream"]
    bound = {name: (res, args) for name, res, args in _lib.SYMBOLS}
    assert "genie_stack_windows_legs" in bound, "genie_stack_windows_legs is not in _lib.SYMBOLS"
    P, I, L, F = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_float
    assert bound["genie_stack_windows_legs"] == (I, [P, I, P, I, L, I, F, P, L, L, L, P])
    assert getattr(_lib.load(), "genie_stack_windows_legs").restype is not None


def test_one_leg_limit_for_the_days_passes():
    assert engine.STACK_MAX_LEGS == postproc.REFINE_SELECT_MAX_LEGS == 32
