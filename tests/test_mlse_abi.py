"""The sequence equaliser in the C-ABI: its two entry points exported by libtrxsig.so and libtrxsig_tune.so, declared in
include/trxsig.h and typed in the binding's table, refused with TRXSIG_EINVAL for a NULL context before anything touches a
device; TRXSIG_TSCLEG_MLSE in the header and the binding; the contract's parts in the header.  No GPU needed (the refusals that
need a live context -- nsoft > 148, tsc outside 0..7, NULL arrays -- are in tests/test_gpu_mlse.py)."""
import ctypes
import os
import re

import pytest

import _pkg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["trxsig_mlse_batch", "trxsig_mlse_normal_batch"]


@pytest.mark.parametrize("name", ["libtrxsig.so", "libtrxsig_tune.so"])
def test_mlse_in_the_abi(name):
    lib = ctypes.CDLL(os.path.join(ROOT, "openbts-ttsou_amd", name))
    h = open(os.path.join(ROOT, "include", "trxsig.h")).read()
    for s in SYMBOLS:
        assert hasattr(lib, s), s
        assert re.search(r"\bint\s+%s\(" % s, h), s
    vp, i32, f32 = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
    lib.trxsig_mlse_batch.argtypes = [vp, vp, vp, vp, i32, i32, vp, vp, vp, vp, vp, vp, vp, i32, i32]
    lib.trxsig_mlse_normal_batch.argtypes = [vp, vp, vp, vp, i32, i32, f32, f32, vp, vp, vp, vp, vp, vp, vp, vp, i32, i32]
    x = (ctypes.c_float * 16)()
    for nsoft, tsc in ((148, 0), (149, 0), (148, 8), (148, -1), (0, 0)):
        assert lib.trxsig_mlse_batch(None, x, x, x, 1, tsc, x, x, None, None, None, x, None, nsoft, 160) == -1           # TRXSIG_EINVAL
        assert lib.trxsig_mlse_normal_batch(None, x, x, x, 1, tsc, 3.0, -1.0, x, x, x, None, None, None, x, None, nsoft, 160) == -1
    assert lib.trxsig_mlse_batch(None, None, None, None, 0, 0, None, None, None, None, None, None, None, 0, 0) == -1
    # the new kernel has no profiler id: the table (ABI 2) stays where it was
    assert lib.trxsig_kernel_count() == 28
    assert lib.trxsig_abi_version() == 2


def test_header_states_the_contract():
    h = open(os.path.join(ROOT, "include", "trxsig.h")).read()
    for word in ("0.0625f", "strict >", "fabsf(v) < 0x1p30f", "E == 0", "8.0f * E", "tests/mlse_model.py", "length/sps < 148",
                 "a[145..147] = -1", "a[0..2] = -1", "g[k] = h[4-k]"):
        assert word in h, word
    t = open(os.path.join(ROOT, "include", "trxsig_transceiver.h")).read()
    assert re.search(r"TRXSIG_TSCLEG_MLSE\s*=\s*2\b", t)
    assert "TRXSIG_TSCLEG_MLSE" in open(os.path.join(ROOT, "include", "trxsig_trxgroup.h")).read()


def test_python_binding():
    m = _pkg.load()
    from openbts_ttsou_amd import _abi
    for name in SYMBOLS:
        assert name in _abi.SIGNATURES, name
    assert len(_abi.SIGNATURES["trxsig_mlse_batch"][1]) == 15 and len(_abi.SIGNATURES["trxsig_mlse_normal_batch"][1]) == 18
    assert callable(getattr(m.TrxSig, "mlse", None)) and callable(getattr(m.TrxSig, "mlse_normal", None))
    assert (m.TSCLEG_EQUALIZE, m.TSCLEG_DEMOD, m.TSCLEG_MLSE) == (0, 1, 2)


def test_kernel_file_is_built_and_audited():
    mk = open(os.path.join(ROOT, "openbts-ttsou_amd", "csrc", "Makefile")).read()
    assert re.search(r"^KERNELS\s*:=.*\btrxsig_mlse\b", mk, re.M)
    assert os.path.exists(os.path.join(ROOT, "openbts-ttsou_amd", "csrc", "trxsig_mlse.hip"))


def test_documents_name_the_stage():
    for doc in ("DESIGN.md", "README.md"):
        assert "trxsig_mlse_batch" in open(os.path.join(ROOT, doc)).read(), doc
