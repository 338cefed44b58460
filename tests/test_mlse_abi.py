"""The sequence equaliser in the C-ABI: its two entry points exported by libtrxsig.so and libtrxsig_tune.so, declared in
include/trxsig.h and typed in the binding's table, refused with TRXSIG_EINVAL for a NULL context before anything touches a
device; TRXSIG_TSCLEG_MLSE in the header and the binding; the contract's parts in the header.  No GPU needed (the refusals that
need a live context -- nsoft > 148, tsc outside 0..7, NULL arrays -- are in tests/test_gpu_mlse.py)."""
import ctypes
import re

import pytest

import mlse_abi as abi

SYMBOLS = {"trxsig_mlse_batch": "trxsig.h", "trxsig_mlse_normal_batch": "trxsig.h"}


@pytest.mark.parametrize("name", abi.LIBS)
def test_mlse_in_the_abi(name):
    lib = abi.exported_and_declared(name, SYMBOLS)
    vp, i32, f32 = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
    lib.trxsig_mlse_batch.argtypes = [vp, vp, vp, vp, i32, i32, vp, vp, vp, vp, vp, vp, vp, i32, i32]
    lib.trxsig_mlse_normal_batch.argtypes = [vp, vp, vp, vp, i32, i32, f32, f32, vp, vp, vp, vp, vp, vp, vp, vp, i32, i32]
    x = (ctypes.c_float * 16)()
    for nsoft, tsc in ((148, 0), (149, 0), (148, 8), (148, -1), (0, 0)):
        assert lib.trxsig_mlse_batch(None, x, x, x, 1, tsc, x, x, None, None, None, x, None, nsoft, 160) == -1           # TRXSIG_EINVAL
        assert lib.trxsig_mlse_normal_batch(None, x, x, x, 1, tsc, 3.0, -1.0, x, x, x, None, None, None, x, None, nsoft, 160) == -1
    assert lib.trxsig_mlse_batch(None, None, None, None, 0, 0, None, None, None, None, None, None, None, 0, 0) == -1
    abi.table_stays(lib)


def test_header_states_the_contract():
    h = abi.read("include", "trxsig.h")
    for word in ("0.0625f", "strict >", "fabsf(v) < 0x1p30f", "E == 0", "8.0f * E", "tests/mlse_model.py", "length/sps < 148",
                 "a[145..147] = -1", "a[0..2] = -1", "g[k] = h[4-k]"):
        assert word in h, word
    assert re.search(r"TRXSIG_TSCLEG_MLSE\s*=\s*2\b", abi.read("include", "trxsig_transceiver.h"))
    assert "TRXSIG_TSCLEG_MLSE" in abi.read("include", "trxsig_trxgroup.h")


def test_python_binding():
    m, _abi = abi.binding(SYMBOLS, TrxSig=("mlse", "mlse_normal"))
    assert len(_abi.SIGNATURES["trxsig_mlse_batch"][1]) == 15 and len(_abi.SIGNATURES["trxsig_mlse_normal_batch"][1]) == 18
    assert (m.TSCLEG_EQUALIZE, m.TSCLEG_DEMOD, m.TSCLEG_MLSE) == (0, 1, 2)


def test_kernel_file_is_built_and_audited():
    assert abi.kernel_file("trxsig_mlse")


def test_documents_name_the_stage():
    abi.documents_name("trxsig_mlse_batch")
