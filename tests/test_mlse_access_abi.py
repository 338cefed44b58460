"""The access-burst sequence equaliser in the C-ABI: its entry points exported by libtrxsig.so and libtrxsig_tune.so, declared in the
headers and typed in the binding's table, refused with TRXSIG_EINVAL for a NULL context (nsoft > 148 among the calls) before
anything touches a device; the library's least-squares table equal to the model's word for word; the committed table header equal
to what its generator writes; the contract's key formulas in the header; the kernel file in the Makefile; the binding's methods.
No GPU needed (the refusals that need a live context are checked on one in tests/test_gpu_mlse_access.py and
tests/test_gpu_mlse_access_group.py)."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import mlse_abi as abi
import mlse_access_model as model

ROOT = abi.ROOT
SYMBOLS = {"trxsig_mlse_access_batch": "trxsig.h", "trxsig_mlse_rach_batch": "trxsig.h", "trxsig_mlse_access_pinv_host": "trxsig.h",
           "trxsig_trxgroup_set_rach_leg": "trxsig_trxgroup.h"}


@pytest.mark.parametrize("name", abi.LIBS)
def test_access_equaliser_in_the_abi(name):
    lib = abi.exported_and_declared(name, SYMBOLS)
    vp, i32, f32 = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
    lib.trxsig_mlse_access_batch.argtypes = [vp, vp, vp, vp, i32, vp, vp, vp, vp, vp, vp, vp, i32, i32]
    lib.trxsig_mlse_rach_batch.argtypes = [vp, vp, vp, vp, i32, f32, f32, vp, vp, vp, vp, vp, vp, vp, vp, i32, i32]
    lib.trxsig_mlse_access_pinv_host.argtypes = [vp]
    lib.trxsig_trxgroup_set_rach_leg.argtypes = [vp, i32]
    x = (ctypes.c_float * 16)()
    for nsoft in (148, 149, 0, -1):
        assert lib.trxsig_mlse_access_batch(None, x, x, x, 1, x, x, None, None, None, x, None, nsoft, 160) == -1
        assert lib.trxsig_mlse_rach_batch(None, x, x, x, 1, 5.0, -1.0, x, x, x, None, None, None, x, None, nsoft, 160) == -1
    assert lib.trxsig_mlse_access_batch(None, None, None, None, 0, None, None, None, None, None, None, None, 0, 0) == -1
    assert lib.trxsig_mlse_access_pinv_host(None) == -1
    for leg in (0, 1, 2):
        assert lib.trxsig_trxgroup_set_rach_leg(None, leg) == -1
    # the table, word for word
    out = np.full((9, 41), np.nan, np.float32)
    assert lib.trxsig_mlse_access_pinv_host(out.ctypes.data) == 0
    assert out.tobytes() == model.pinv_table().tobytes()
    abi.table_stays(lib)


def test_committed_table_is_the_generated_one():
    """csrc/trxsig_mlse_access_tab.h is what tools/gen_mlse_access_tab.py writes from the exact integers (hexadecimal float literals:
    the words themselves)."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_mlse_access_tab.py"), "--check"], cwd=ROOT)
    assert r.returncode == 0
    text = open(os.path.join(ROOT, "openbts-ttsou_amd", "csrc", "trxsig_mlse_access_tab.h")).read()
    words = re.findall(r"-?0x1\.[0-9a-f]+p[-+]\d+f", text)
    assert len(words) == 9 * 41
    got = np.array([float.fromhex(w[:-1]) for w in words], np.float64)
    assert np.array_equal(got.astype(np.float32), model.pinv_table().ravel()) and np.array_equal(got, model.pinv_table().ravel().astype(np.float64))


def test_headers_state_the_contract():
    h = abi.read("include", "trxsig.h")
    for word in ("y[n] = sum_{d=-4..4} c[d] a[n-d]", "A[n-4][d+4] = a[n-d]", "N = adj(G) A^T", "P32[d+4][j] = (float)((double)N[d+4][j] / (double)det)",
                 "c[d].re = sum_{j=0..40} P32[d+4][j] * y[4+j].re", "|P32| < 0.04", "m = 49 + i on y[m+w]", "a[48], a[47], a[46], a[45]",
                 "for i >= 36 a", "clamp(0.5f + (M_0 - M_1) / (8.0f * E), 0, 1) for m = 49..87", "Positions 0..48 and 88..147",
                 "fabsf(v) < 0x1p30f", "(2 Q + 80 P) / (8 E)", "tests/mlse_access_model.py", "tests/mlse_access_ref.py", "d_win = 2",
                 "TRXSIG_K_COUNT = 15", "#define TRXSIG_ABI_VERSION 2"):
        assert word in h, word
    g = abi.read("include", "trxsig_trxgroup.h")
    for word in ("trxsig_trxgroup_set_rach_leg", "TRXSIG_RACHLEG_DEMOD = 0", "TRXSIG_RACHLEG_MLSE = 1", "trxsig_mlse_access_batch", "push / pop"):
        assert word in g, word
    c = abi.read("openbts-ttsou_amd", "csrc", "trxsig_ctx.h")
    assert "int trx_ctx_mlse(" in c and "need_mask" in c


def test_python_binding():
    m, _abi = abi.binding(SYMBOLS, TrxSig=("mlse_access", "mlse_rach", "mlse_access_pinv"), TrxGroup=("set_rach_leg",))
    assert len(_abi.SIGNATURES["trxsig_mlse_access_batch"][1]) == 14 and len(_abi.SIGNATURES["trxsig_mlse_rach_batch"][1]) == 17
    assert _abi.SIGNATURES["trxsig_mlse_rach_batch"][1][5] is ctypes.c_float and len(_abi.SIGNATURES["trxsig_trxgroup_set_rach_leg"][1]) == 2
    assert (m.RACHLEG_DEMOD, m.RACHLEG_MLSE) == (0, 1)
    assert "rach_leg" not in abi.read("include", "trxsig_transceiver.h")      # the one-burst object does not get the setter


def test_kernel_file_is_built():
    src = abi.kernel_file("trxsig_mlse_access")
    assert "k_mlse_access" in src and "amdgpu_waves_per_eu(4)" in src and "trxsig_mlse_dev.h" in src and "trxsig_mlse_access_tab.h" in src
    for call in ("mlse_symbols<SPS>(", "mlse_ls_tap<TRX_MLSE_ACCESS_NROW>(", "mlse_window(", "mlse_trellis<TRX_MLSE_ACC_STEPS>(", "#pragma unroll 1"):
        assert call in src, call


def test_documents_name_the_stage():
    abi.documents_name("trxsig_mlse_access_batch", "trxsig_trxgroup_set_rach_leg", "mlse_access_bench", "k_mlse_access")
