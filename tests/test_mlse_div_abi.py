"""Two-antenna receive diversity in the C-ABI: its three entry points exported by libtrxsig.so and libtrxsig_tune.so, declared in
the headers and typed in the binding's table, refused with TRXSIG_EINVAL for a NULL context before anything touches a device;
the contract's words in the header; the kernel file in the Makefile; the binding's methods.  No GPU needed (the refusals that
need a live context are in tests/test_gpu_mlse_div.py and tests/test_gpu_mlse_div_group.py)."""
import ctypes

import pytest

import mlse_abi as abi

SYMBOLS = {"trxsig_mlse_div_batch": "trxsig.h", "trxsig_mlse_div_normal_batch": "trxsig.h", "trxsig_trxgroup_combine_div": "trxsig_trxgroup.h"}


@pytest.mark.parametrize("name", abi.LIBS)
def test_diversity_in_the_abi(name):
    lib = abi.exported_and_declared(name, SYMBOLS)
    vp, i32, f32 = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
    lib.trxsig_mlse_div_batch.argtypes = [vp, vp, vp, vp, vp, vp, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp, i32, i32]
    lib.trxsig_mlse_div_normal_batch.argtypes = [vp, vp, vp, vp, vp, vp, i32, i32, f32, f32, vp, vp, vp, vp, vp, vp, vp, vp, vp, i32, i32]
    lib.trxsig_trxgroup_combine_div.argtypes = [vp] * 8
    x = (ctypes.c_float * 16)()
    for nsoft, tsc in ((148, 0), (149, 0), (148, 8), (148, -1), (0, 0)):
        assert lib.trxsig_mlse_div_batch(None, x, x, x, x, x, 1, tsc, x, x, None, None, None, None, x, None, nsoft, 160) == -1      # TRXSIG_EINVAL
        assert lib.trxsig_mlse_div_normal_batch(None, x, x, x, x, x, 1, tsc, 3.0, -1.0, x, x, x, None, x, None, None, x, None, nsoft, 160) == -1
    assert lib.trxsig_mlse_div_batch(None, None, None, None, None, None, 0, 0, None, None, None, None, None, None, None, None, 0, 0) == -1
    assert lib.trxsig_trxgroup_combine_div(None, x, None, x, None, None, None, x) == -1
    abi.table_stays(lib)


def test_header_states_the_contract():
    h = abi.read("include", "trxsig.h")
    for word in ("p[d] = (c_0.re*c_0.re + c_0.im*c_0.im) + (c_1.re*c_1.re + c_1.im*c_1.im)",
                 "gamma = (dr_0*dr_0 + di_0*di_0) + (dr_1*dr_1 + di_1*di_1)", "d_primary", "same noise power",
                 "sel = 1 if v_1 && (!v_0 || n_1 > n_0)", "sel = 0 if v_0", "sel = 2", "ONE window w", "tests/mlse_div_model.py",
                 "tests/mlse_div_ref.py", "B x 2 x 5"):
        assert word in h, word
    g = abi.read("include", "trxsig_trxgroup.h")
    for word in ("1 if v_1 && (!v_0 || n_1 > n_0)", "TRXSIG_TSCLEG_DEMOD is the cheaper choice", "TRXSIG_TSCLEG_EQUALIZE", "fused source",
                 "valid until g0's next pull or combine"):
        assert word in g, word


def test_python_binding():
    m, _abi = abi.binding(SYMBOLS, TrxSig=("mlse_div", "mlse_div_normal"), TrxGroup=("combine_div",))
    assert len(_abi.SIGNATURES["trxsig_mlse_div_batch"][1]) == 18 and len(_abi.SIGNATURES["trxsig_mlse_div_normal_batch"][1]) == 21
    assert len(_abi.SIGNATURES["trxsig_trxgroup_combine_div"][1]) == 8


def test_kernel_file_is_built_and_audited():
    assert abi.kernel_file("trxsig_mlse_div")


def test_documents_name_the_stage():
    abi.documents_name("trxsig_mlse_div_batch", "trxsig_trxgroup_combine_div")
