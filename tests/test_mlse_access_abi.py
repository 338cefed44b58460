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

import _pkg
import mlse_access_model as model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = {"trxsig_mlse_access_batch": "trxsig.h", "trxsig_mlse_rach_batch": "trxsig.h", "trxsig_mlse_access_pinv_host": "trxsig.h",
           "trxsig_trxgroup_set_rach_leg": "trxsig_trxgroup.h"}


@pytest.mark.parametrize("name", ["libtrxsig.so", "libtrxsig_tune.so"])
def test_access_equaliser_in_the_abi(name):
    lib = ctypes.CDLL(os.path.join(ROOT, "openbts-ttsou_amd", name))
    for s, header in SYMBOLS.items():
        assert hasattr(lib, s), s
        assert re.search(r"\bint\s+%s\(" % s, open(os.path.join(ROOT, "include", header)).read()), s
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
    # the new kernel has no profiler id: the table (ABI 2) stays where it was
    assert lib.trxsig_kernel_count() == 28
    assert lib.trxsig_abi_version() == 2


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
    h = open(os.path.join(ROOT, "include", "trxsig.h")).read()
    for word in ("y[n] = sum_{d=-4..4} c[d] a[n-d]", "A[n-4][d+4] = a[n-d]", "N = adj(G) A^T", "P32[d+4][j] = (float)((double)N[d+4][j] / (double)det)",
                 "c[d].re = sum_{j=0..40} P32[d+4][j] * y[4+j].re", "|P32| < 0.04", "m = 49 + i on y[m+w]", "a[48], a[47], a[46], a[45]",
                 "for i >= 36 a", "clamp(0.5f + (M_0 - M_1) / (8.0f * E), 0, 1) for m = 49..87", "Positions 0..48 and 88..147",
                 "fabsf(v) < 0x1p30f", "(2 Q + 80 P) / (8 E)", "tests/mlse_access_model.py", "tests/mlse_access_ref.py", "d_win = 2",
                 "TRXSIG_K_COUNT = 15", "#define TRXSIG_ABI_VERSION 2"):
        assert word in h, word
    g = open(os.path.join(ROOT, "include", "trxsig_trxgroup.h")).read()
    for word in ("trxsig_trxgroup_set_rach_leg", "TRXSIG_RACHLEG_DEMOD = 0", "TRXSIG_RACHLEG_MLSE = 1", "trxsig_mlse_access_batch", "push / pop"):
        assert word in g, word
    c = open(os.path.join(ROOT, "openbts-ttsou_amd", "csrc", "trxsig_ctx.h")).read()
    assert "trx_ctx_mlse_access_masked" in c and "need_mask" in c


def test_python_binding():
    m = _pkg.load()
    from openbts_ttsou_amd import _abi
    for name in SYMBOLS:
        assert name in _abi.SIGNATURES, name
    assert len(_abi.SIGNATURES["trxsig_mlse_access_batch"][1]) == 14 and len(_abi.SIGNATURES["trxsig_mlse_rach_batch"][1]) == 17
    assert _abi.SIGNATURES["trxsig_mlse_rach_batch"][1][5] is ctypes.c_float and len(_abi.SIGNATURES["trxsig_trxgroup_set_rach_leg"][1]) == 2
    for name in ("mlse_access", "mlse_rach", "mlse_access_pinv"):
        assert callable(getattr(m.TrxSig, name, None)), name
    assert callable(getattr(m.TrxGroup, "set_rach_leg", None))
    assert (m.RACHLEG_DEMOD, m.RACHLEG_MLSE) == (0, 1)
    assert "rach_leg" not in open(os.path.join(ROOT, "include", "trxsig_transceiver.h")).read()      # the one-burst object does not get the setter


def test_kernel_file_is_built():
    mk = open(os.path.join(ROOT, "openbts-ttsou_amd", "csrc", "Makefile")).read()
    assert re.search(r"^KERNELS\s*:=.*\btrxsig_mlse_access\b", mk, re.M)
    src = open(os.path.join(ROOT, "openbts-ttsou_amd", "csrc", "trxsig_mlse_access.hip")).read()
    assert "k_mlse_access" in src and "amdgpu_waves_per_eu(4)" in src and "trxsig_mlse_dev.h" in src and "trxsig_mlse_access_tab.h" in src
    for call in ("mlse_symbols<SPS>(", "mlse_ls_tap<TRX_MLSE_ACCESS_NROW>(", "mlse_window(", "mlse_trellis<TRX_MLSE_ACC_STEPS>(", "#pragma unroll 1"):
        assert call in src, call


def test_documents_name_the_stage():
    for doc in ("DESIGN.md", "README.md"):
        text = open(os.path.join(ROOT, doc)).read()
        for word in ("trxsig_mlse_access_batch", "trxsig_trxgroup_set_rach_leg", "mlse_access_bench", "k_mlse_access"):
            assert word in text, (doc, word)
