"""The fading-tap generator in the C-ABI: its four entry points exported by libtrxsig.so, declared in include/trxsig_air.h and
typed in the binding's table, refused with TRXSIG_EINVAL for a NULL object before anything touches a device; the contract's
parts in the header; the binding's methods.  No GPU needed (the refusals that need a live object are in
tests/test_gpu_air_fade.py)."""
import ctypes
import os
import re

import _pkg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["fade_profile", "fade_columns", "fade", "fade_params"]


def test_fade_in_the_abi():
    lib = ctypes.CDLL(os.path.join(ROOT, "openbts-ttsou_amd", "libtrxsig.so"))
    h = open(os.path.join(ROOT, "include", "trxsig_air.h")).read()
    for s in SYMBOLS:
        assert hasattr(lib, "trxsig_air_" + s), s
        assert re.search(r"\bint\s+trxsig_air_%s\(" % s, h), s
    vp, i32, u64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_uint64
    lib.trxsig_air_fade_profile.argtypes = [vp, i32, vp, vp, vp, vp, i32, i32, i32]
    lib.trxsig_air_fade_columns.argtypes = [vp, i32, vp]
    lib.trxsig_air_fade.argtypes = [vp, i32, i32, i32, u64, vp, i32, vp, vp]
    lib.trxsig_air_fade_params.argtypes = [vp, u64, i32, vp, vp, vp]
    d, p = (ctypes.c_int32 * 1)(0), (ctypes.c_float * 1)(1.0)
    assert lib.trxsig_air_fade_profile(None, 1, d, p, None, None, 1, 1, 0) == -1           # TRXSIG_EINVAL
    assert lib.trxsig_air_fade_profile(None, 1, None, None, None, None, 1, 1, 0) == -1
    assert lib.trxsig_air_fade_columns(None, 1, d) == -1 and lib.trxsig_air_fade_columns(None, 1, None) == -1
    assert lib.trxsig_air_fade(None, 0, 1, 1, 0, None, 1, None, None) == -1
    assert lib.trxsig_air_fade_params(None, 0, 1, None, None, None) == -1
    # the new kernels have no profiler id: the table (ABI 2) stays where it was
    assert lib.trxsig_kernel_count() == 28
    for word in ("TRXSIG_AIR_FADE_MAX_PATHS 12", "TRXSIG_AIR_FADE_MAX_SINUSOIDS 32", "TRXSIG_AIR_FADE_MAX_COLUMNS 1024", "(s, p, l, 2)",
                 "Out of scope", "Error bound", "hyperframe's wrap"):
        assert word in h, word


def test_python_binding():
    m = _pkg.load()
    from openbts_ttsou_amd import _abi
    for name in SYMBOLS:
        assert callable(getattr(m.Air, name, None)), name
        assert "trxsig_air_" + name in _abi.SIGNATURES, name
    assert _abi.SIGNATURES["trxsig_air_fade"][1][4] is ctypes.c_uint64


def test_documents_name_the_stage():
    for doc in ("DESIGN.md", "README.md"):
        assert "trxsig_air_fade" in open(os.path.join(ROOT, doc)).read(), doc
