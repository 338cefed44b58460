"""The synchronisation-burst sequence equaliser in the C-ABI: its entry points exported by libtrxsig.so and libtrxsig_tune.so,
declared in the headers and typed in the binding's table, refused with TRXSIG_EINVAL for a NULL context or object (nsoft > 148 and
a leg that is none among the calls) before anything touches a device; the library's least-squares table equal to the model's word
for word; the committed table header equal to what its generator writes, the two start states in it equal to the model's
derivation; the contract's key formulas in the headers; the kernel file in the Makefile; the binding's methods.  No GPU needed (the
refusals that need a live context or object are checked on one in tests/test_gpu_mlse_sch.py and tests/test_gpu_l1acq_mlse.py)."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import mlse_abi as abi
import mlse_sch_model as model

ROOT = abi.ROOT
SYMBOLS = {"trxsig_mlse_sch_batch": "trxsig.h", "trxsig_mlse_sch_pinv_host": "trxsig.h", "trxsig_l1acq_set_sch_leg": "trxsig_l1acq.h",
           "trxsig_l1acq_sch_channel": "trxsig_l1acq.h"}


@pytest.mark.parametrize("name", abi.LIBS)
def test_sch_equaliser_in_the_abi(name):
    lib = abi.exported_and_declared(name, SYMBOLS)
    vp, i32 = ctypes.c_void_p, ctypes.c_int
    lib.trxsig_mlse_sch_batch.argtypes = [vp, vp, vp, vp, i32, vp, vp, vp, vp, vp, vp, vp, i32, i32]
    lib.trxsig_mlse_sch_pinv_host.argtypes = [vp]
    lib.trxsig_l1acq_set_sch_leg.argtypes = [vp, i32]
    lib.trxsig_l1acq_sch_channel.argtypes = [vp, vp, vp]
    x = (ctypes.c_float * 16)()
    for nsoft in (148, 149, 0, -1):
        assert lib.trxsig_mlse_sch_batch(None, x, x, x, 1, x, x, None, None, None, x, None, nsoft, 160) == -1
    assert lib.trxsig_mlse_sch_batch(None, None, None, None, 0, None, None, None, None, None, None, None, 0, 0) == -1
    assert lib.trxsig_mlse_sch_pinv_host(None) == -1
    for leg in (0, 1, 2, -1):
        assert lib.trxsig_l1acq_set_sch_leg(None, leg) == -1
    assert lib.trxsig_l1acq_sch_channel(None, x, x) == -1
    # the table, word for word
    out = np.full((9, 56), np.nan, np.float32)
    assert lib.trxsig_mlse_sch_pinv_host(out.ctypes.data) == 0
    assert out.tobytes() == model.pinv_table().tobytes()
    abi.table_stays(lib)


def test_committed_table_is_the_generated_one():
    """csrc/trxsig_mlse_sch_tab.h is what tools/gen_mlse_sch_tab.py writes from the exact integers (hexadecimal float literals:
    the words themselves), and the two start states the kernel carries are the model's derivation from the training sequence."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_mlse_sch_tab.py"), "--check"], cwd=ROOT)
    assert r.returncode == 0
    text = open(os.path.join(ROOT, "openbts-ttsou_amd", "csrc", "trxsig_mlse_sch_tab.h")).read()
    words = re.findall(r"-?0x1\.[0-9a-f]+p[-+]\d+f", text)
    assert len(words) == 9 * 56
    got = np.array([float.fromhex(w[:-1]) for w in words], np.float64)
    assert np.array_equal(got.astype(np.float32), model.pinv_table().ravel()) and np.array_equal(got, model.pinv_table().ravel().astype(np.float64))
    consts = dict(re.findall(r"^#define (TRX_MLSE_SCH_\w+) (\d+)", text, re.M))
    assert (int(consts["TRX_MLSE_SCH_START_RIGHT"]), int(consts["TRX_MLSE_SCH_START_LEFT"])) == (model.START_RIGHT, model.START_LEFT) == (11, 13)
    assert (int(consts["TRX_MLSE_SCH_NTAP"]), int(consts["TRX_MLSE_SCH_NROW"]), int(consts["TRX_MLSE_SCH_ROW0"])) == (9, 56, 46)
    src = open(os.path.join(ROOT, "openbts-ttsou_amd", "csrc", "trxsig_mlse_sch.hip")).read()
    assert "left ? TRX_MLSE_SCH_START_LEFT : TRX_MLSE_SCH_START_RIGHT" in src        # the kernel carries these two and no others


def test_headers_state_the_contract():
    h = abi.read("include", "trxsig.h")
    for word in ("y[n] = sum_{d=-4..4} c[d] a[n-d]", "A[n-46][d+4] = a[n-d]", "N = adj(G) A^T", "P32[d+4][j] = (float)((double)N[d+4][j] / (double)det)",
                 "c[d].re = sum_{j=0..55} P32[d+4][j] * y[46+j].re", "|P32| < 0.0253", "steps m = 106..147 on y[m+w]", "a[105], a[104], a[103], a[102]",
                 "steps m = 41..0 on y[m+4+w]", "a[42],", "a[43], a[44], a[45]", "g[k] = h[4-k]", "for m = 0..41 and 106..147", "Positions 42..105",
                 "fabsf(v) < 0x1p30f", "(2 Q + 86 P) / (8 E)", "S1 <= 1.0001", "tests/mlse_sch_model.py", "tests/mlse_sch_ref.py",
                 "the six tail bits come out as exactly 0", "TRXSIG_K_COUNT = 15", "#define TRXSIG_ABI_VERSION 2"):
        assert word in h, word
    g = abi.read("include", "trxsig_l1acq.h")
    for word in ("trxsig_l1acq_set_sch_leg", "TRXSIG_SCHLEG_DEMOD = 0", "TRXSIG_SCHLEG_MLSE = 1", "trxsig_mlse_sch_batch", "trxsig_l1acq_sch_channel",
                 "byte for byte"):
        assert word in g, word
    assert "d_chan" not in re.search(r"typedef struct \{(.*?)\} trxsig_l1acq_out;", g, re.S).group(1)       # the out structure is as it was
    assert "int trx_ctx_mlse(" in abi.read("openbts-ttsou_amd", "csrc", "trxsig_ctx.h")


def test_python_binding():
    m, _abi = abi.binding(SYMBOLS, TrxSig=("mlse_sch", "mlse_sch_pinv"), L1Acq=("set_sch_leg", "sch_channel"))
    assert _abi.SIGNATURES["trxsig_mlse_sch_batch"] == _abi.SIGNATURES["trxsig_mlse_access_batch"]      # the same argument list, no tsc
    assert len(_abi.SIGNATURES["trxsig_l1acq_set_sch_leg"][1]) == 2 and len(_abi.SIGNATURES["trxsig_l1acq_sch_channel"][1]) == 3
    assert (m.SCHLEG_DEMOD, m.SCHLEG_MLSE) == (0, 1)
    assert [f[0] for f in _abi.L1AcqOut._fields_][-3:] == ["d_ok", "d_bsic", "d_rfn"] and len(_abi.L1AcqOut._fields_) == 17


def test_kernel_file_is_built():
    src = abi.kernel_file("trxsig_mlse_sch")
    assert "k_mlse_sch" in src and "amdgpu_waves_per_eu(4)" in src and "trxsig_mlse_dev.h" in src and "trxsig_mlse_sch_tab.h" in src
    for call in ("mlse_symbols<SPS>(", "mlse_ls_tap<TRX_MLSE_SCH_NROW>(", "mlse_window(", "mlse_trellis<TRX_MLSE_SCH_STEPS>(", "#pragma unroll 1"):
        assert call in src, call
    acq = abi.read("openbts-ttsou_amd", "csrc", "trxsig_l1acq.cpp")
    assert "trx_launch_mlse_sch" in acq and "trx_launch_demod" in acq


def test_documents_name_the_stage():
    abi.documents_name("trxsig_mlse_sch_batch", "trxsig_l1acq_set_sch_leg", "mlse_sch_bench", "k_mlse_sch")
