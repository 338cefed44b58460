"""The fit detector in the C-ABI: its entry points exported by libtrxsig.so and libtrxsig_tune.so, declared in the headers and typed
in the binding's table, refused with TRXSIG_EINVAL for a NULL context or object before anything touches a device; the kernel's
copy of the extended training sequence equal to the model's; the contract's key formulas and the measured threshold in the
headers; the kernel file in the Makefile; the binding's methods.  No GPU needed (the refusals that need a live context or object
are checked on one in tests/test_gpu_sch_fit.py and tests/test_gpu_l1acq_fit.py)."""
import ctypes
import re

import pytest

import mlse_abi as abi
import mlse_sch_model as sch_model

SYMBOLS = {"trxsig_sch_fit_batch": "trxsig.h", "trxsig_l1acq_set_sch_detector": "trxsig_l1acq.h", "trxsig_l1acq_sch_fit": "trxsig_l1acq.h"}


@pytest.mark.parametrize("name", abi.LIBS)
def test_fit_detector_in_the_abi(name):
    lib = abi.exported_and_declared(name, SYMBOLS)
    vp, i32 = ctypes.c_void_p, ctypes.c_int
    lib.trxsig_sch_fit_batch.argtypes = [vp, vp, vp, vp, i32, vp, vp, vp, vp, vp, vp, vp, vp]
    lib.trxsig_l1acq_set_sch_detector.argtypes = [vp, i32]
    lib.trxsig_l1acq_sch_fit.argtypes = [vp, vp, vp]
    x = (ctypes.c_float * 16)()
    assert lib.trxsig_sch_fit_batch(None, x, x, x, 1, x, x, None, x, x, x, x, x) == -1
    assert lib.trxsig_sch_fit_batch(None, None, None, None, 0, None, None, None, None, None, None, None, None) == -1
    for det in (0, 1, 2, -1):
        assert lib.trxsig_l1acq_set_sch_detector(None, det) == -1
    assert lib.trxsig_l1acq_sch_fit(None, x, x) == -1
    abi.table_stays(lib)


def test_kernel_carries_the_training_sequence():
    src = abi.read("openbts-ttsou_amd", "csrc", "trxsig_sch_fit.hip")
    bits = re.search(r'const char \*x = "([01]{64})";', src).group(1)
    assert [int(b) for b in bits] == sch_model.XTS.tolist()
    assert "(x[t] == '1') << t" in src and "kSchFitXts >> (t0 - k)" in src and "(TRX_MLSE_SCH_ROW0 - 42) - w" in src


def test_headers_state_the_contract():
    h = abi.read("include", "trxsig.h")
    for word in ("trxsig_sch_fit_batch", "q = sqrtf((51.0f * E) / R)", "Z[n] = h[0] a[n - w], then + h[1] a[n - w - 1]", "r[n] = y[n] - Z[n]",
                 "the pairwise tree over e[0..63] with e[56..63] = 0", "gives +inf and stays", "q = 0 where the result is a NaN",
                 "step 2 of trxsig_mlse_sch_batch, word for word", "tests/sch_fit_model.py", "tests/sch_fit_ref.py", "g_k = k u / (1 - k u)",
                 "sqrt((1 + g_8) / (1 - bR / R)) (1 + u) - 1", "TRXSIG_K_COUNT = 15", "#define TRXSIG_ABI_VERSION 2"):
        assert word in h, word
    g = abi.read("include", "trxsig_l1acq.h")
    for word in ("trxsig_l1acq_set_sch_detector", "TRXSIG_SCHDET_VALLEY = 0", "TRXSIG_SCHDET_FIT = 1", "trxsig_l1acq_sch_fit", "CANDIDATE",
                 "CARRY q, THE METRIC OF THE ACTIVE DETECTOR", "#define TRXSIG_L1ACQ_SCH_FIT_THRESH 1.4f", "independent of trxsig_l1acq_set_sch_leg"):
        assert word in g, word
    out = re.search(r"typedef struct \{(.*?)\} trxsig_l1acq_out;", g, re.S).group(1)
    assert "d_q" not in out and "d_R" not in out                # the out structure is as it was


def test_python_binding():
    m, _abi = abi.binding(SYMBOLS, TrxSig=("sch_fit",), L1Acq=("set_sch_detector", "sch_fit"))
    assert len(_abi.SIGNATURES["trxsig_sch_fit_batch"][1]) == 13
    assert _abi.SIGNATURES["trxsig_sch_fit_batch"][1][:8] == _abi.SIGNATURES["trxsig_mlse_sch_batch"][1][:8]      # the same inputs
    assert _abi.SIGNATURES["trxsig_l1acq_set_sch_detector"] == _abi.SIGNATURES["trxsig_l1acq_set_sch_leg"]
    assert _abi.SIGNATURES["trxsig_l1acq_sch_fit"] == _abi.SIGNATURES["trxsig_l1acq_sch_channel"]
    assert (m.SCHDET_VALLEY, m.SCHDET_FIT) == (0, 1) and m.ACQ_SCH_FIT_THRESH == 1.4
    assert len(_abi.L1AcqOut._fields_) == 17


def test_kernel_file_is_built():
    src = abi.kernel_file("trxsig_sch_fit")
    assert "k_sch_fit" in src and "amdgpu_waves_per_eu(4)" in src and "trxsig_mlse_dev.h" in src and "trxsig_mlse_sch_tab.h" in src
    dev = abi.read("openbts-ttsou_amd", "csrc", "trxsig_mlse_dev.h")
    assert "demod_core<SPS, true, 148>" in dev and "mlse_symbols<SPS>(" in src and "#pragma unroll 1" in src      # the symbols step is the shared one
    assert "mlse_ls_tap<TRX_MLSE_SCH_NROW>(" in src and "mlse_window(" in src
    acq = abi.read("openbts-ttsou_amd", "csrc", "trxsig_l1acq.cpp")
    assert "trx_launch_sch_fit" in acq and "trx_launch_l1acq_verdict" in acq and "trx_launch_l1acq_fit_verdict" in acq


def test_documents_name_the_stage():
    abi.documents_name("trxsig_sch_fit_batch", "trxsig_l1acq_set_sch_detector", "sch_fit_bench", "k_sch_fit")
