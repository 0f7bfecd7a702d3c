"""gprc_gpr_extend on a CPU-only box: argument checks that precede every HIP call, the packed-layout identity the extend
relies on (the trailing panels of a packed matrix are a packed matrix of their own), and the R binding's registration."""
import ctypes as C
import os
import re

import pytest

from conftest import ROOT
from gprc_amd import _native as nat


def test_extend_of_a_null_model_is_refused_without_a_device():
    lib = nat.lib()
    x = (C.c_double * 4)(0.0, 1.0, 2.0, 3.0)
    y = (C.c_double * 4)(0.0, 1.0, 2.0, 3.0)
    assert lib.gprc_gpr_extend(None, C.cast(x, C.c_void_p), 4, C.cast(y, C.c_void_p)) == nat.ERR_ARG
    assert nat.last_error().startswith("extend:")


@pytest.mark.parametrize("n_pad", [512, 1024, 4096, 16896, 66560])
def test_trailing_panels_are_a_packed_matrix_of_their_own(n_pad):
    """offset(n_pad, p0 + k) - offset(n_pad, p0) == offset(n_pad - p0 NB, k) and the leading dimensions agree: the extend
    factors the tail as a sub-view at packed + offset(n_pad, p0) (winv at n0 * 128, inv at p0 NB NB)."""
    lib = nat.lib()
    NB = lib.gprc_panel_width()
    assert lib.gprc_pad(n_pad) == n_pad and n_pad % NB == 0
    P = lib.gprc_panel_count(n_pad)
    for p0 in sorted({0, 1, P // 2, P - 1}):
        sub = n_pad - p0 * NB
        assert lib.gprc_pad(sub) == sub
        base = lib.gprc_panel_offset(n_pad, p0)
        for k in range(P - p0 + 1):
            assert lib.gprc_panel_offset(n_pad, p0 + k) - base == lib.gprc_panel_offset(sub, k)
            if k < P - p0:
                assert lib.gprc_panel_elems(n_pad, p0 + k) == lib.gprc_panel_elems(sub, k)
        assert lib.gprc_packed_size(n_pad) - base == lib.gprc_packed_size(sub)
        assert lib.gprc_winv_size(n_pad) - p0 * NB * 128 == lib.gprc_winv_size(sub)
        assert lib.gprc_solve_inv_size(n_pad) - p0 * NB * NB == lib.gprc_solve_inv_size(sub)


def test_r_binding_registers_and_calls_the_extend():
    shim = open(os.path.join(ROOT, "gaussian-process-regression_amd", "r", "src", "gprc_call_shim.c")).read()
    assert re.search(r'\{"gprc_R_gpr_extend", \(DL_FUNC\)&gprc_R_gpr_extend, 3\}', shim)
    assert re.search(r"SEXP gprc_R_gpr_extend\(SEXP [a-z_A-Z]+, SEXP [a-z_A-Z]+, SEXP [a-z_A-Z]+\)", shim)
    assert "gprc_gpr_extend(" in shim
    native_r = open(os.path.join(ROOT, "gaussian-process-regression_amd", "r", "R", "native.R")).read()
    assert re.search(r"\.gpr_add_data_native <- function\(private, X_new, y_new\)", native_r)
    assert ".Call(gprc_R_gpr_extend," in native_r


def test_python_binding_declares_the_extend():
    res, args = nat.PROTOTYPES["gprc_gpr_extend"]
    assert res is C.c_int and len(args) == 4
    from gprc_amd import GPR, GPR_sqrexp
    assert callable(GPR.add_data) and GPR_sqrexp.add_data is GPR.add_data
