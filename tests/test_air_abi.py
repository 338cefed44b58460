"""trxsig_air in the C-ABI: every entry point exported by libtrxsig.so and declared in include/trxsig_air.h, refused with
TRXSIG_EINVAL for a NULL object or context before anything touches a device, the parameter records' layout, and the binding
Air.  No GPU needed (the refusals that need a live object -- frames, strides, overlap, lengths -- are in tests/test_gpu_air.py)."""
import ctypes
import os
import re

import _pkg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["create", "destroy", "cells", "stream"]


def test_air_in_the_abi():
    lib = ctypes.CDLL(os.path.join(ROOT, "openbts-ttsou_amd", "libtrxsig.so"))
    h = open(os.path.join(ROOT, "include", "trxsig_air.h")).read()
    for s in SYMBOLS:
        assert hasattr(lib, "trxsig_air_" + s), s
        assert re.search(r"\b(int|void)\s+trxsig_air_%s\(" % s, h), s
    vp, i32, i64, u64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_uint64
    lib.trxsig_air_create.argtypes = [ctypes.POINTER(vp), vp, i32]
    out = vp()
    assert lib.trxsig_air_create(None, None, 4) == -1           # TRXSIG_EINVAL
    for taps in (0, 1, 32, 33, -1):
        assert lib.trxsig_air_create(ctypes.byref(out), None, taps) == -1 and not out.value
    lib.trxsig_air_cells.argtypes = [vp, i32, i32, i32, u64, vp, i64, i64, vp, vp, i64, i64, i32]
    lib.trxsig_air_stream.argtypes = [vp, i32, u64, vp, i64, i64, i32, vp, i32, vp, i64]
    assert lib.trxsig_air_cells(None, 0, 1, 1, 0, None, 0, 0, None, None, 0, 0, 0) == -1
    assert lib.trxsig_air_stream(None, 1, 0, None, 0, 0, 1, None, 1, None, 0) == -1
    lib.trxsig_air_destroy.argtypes = [vp]; lib.trxsig_air_destroy.restype = None
    lib.trxsig_air_destroy(None)
    # the new kernels have no profiler id: the table (ABI 2) stays where it was
    assert lib.trxsig_kernel_count() == 28
    assert re.search(r"#define TRXSIG_AIR_MAX_TAPS 32\b", h)


def test_python_binding():
    m = _pkg.load()
    for name in ("cells", "stream", "destroy"):
        assert callable(getattr(m.Air, name, None)), name
    p = ctypes.sizeof(ctypes.c_void_p)
    assert ctypes.sizeof(m.AirCellParams) == 5 * p and m.AirCellParams.d_step.offset == 2 * p
    assert ctypes.sizeof(m.AirStreamParams) == 9 * p and m.AirStreamParams.d_arfcn.offset == p
    assert m.AIR_MAX_TAPS == 32


def test_documents_name_the_object():
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "trxsig_air" in design and "trxsig_air" in open(os.path.join(ROOT, "README.md")).read()
    assert "trxsig_air" in open(os.path.join(ROOT, "include", "trxsig_l1ms.h")).read() or "trxsig_air" in design
