"""trxsig_l1ms in the C-ABI: every entry point exported by libtrxsig.so and declared in include/trxsig_l1ms.h, refused with
TRXSIG_EINVAL for NULL objects before anything touches a device, and bound as L1Ms.  No GPU needed."""
import ctypes
import os
import re

import _pkg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["create", "destroy", "channels", "channel", "open", "close", "set_phy", "grid", "encode", "radiate", "state"]


def test_l1ms_in_the_abi():
    lib = ctypes.CDLL(os.path.join(ROOT, "openbts-ttsou_amd", "libtrxsig.so"))
    h = open(os.path.join(ROOT, "include", "trxsig_l1ms.h")).read()
    for s in SYMBOLS:
        assert hasattr(lib, "trxsig_l1ms_" + s), s
        assert re.search(r"\b(int|void) trxsig_l1ms_%s\(" % s, h), s
    vp = ctypes.c_void_p
    lib.trxsig_l1ms_create.argtypes = [ctypes.POINTER(vp), vp, ctypes.c_int, vp, ctypes.c_int, ctypes.c_int]
    out = vp()
    assert lib.trxsig_l1ms_create(None, None, 1, None, 0, 900) == -1   # TRXSIG_EINVAL
    assert lib.trxsig_l1ms_create(ctypes.byref(out), None, 1, None, 0, 900) == -1 and not out.value
    lib.trxsig_l1ms_encode.argtypes = [vp, ctypes.c_int, ctypes.c_int, vp, vp, vp]
    lib.trxsig_l1ms_radiate.argtypes = [vp, vp, vp, ctypes.c_int64, ctypes.c_int64]
    assert lib.trxsig_l1ms_encode(None, 0, 1, None, None, None) == -1
    assert lib.trxsig_l1ms_radiate(None, None, None, 0, 0) == -1
    assert "TRXSIG_L1MS_STATE_BYTES 160" in h
    # no kernel id was added: the profiler's table (ABI 2) stays where it was
    assert lib.trxsig_kernel_count() == 28


def test_python_binding():
    m = _pkg.load()
    for name in ("encode", "radiate", "collect", "set_phy", "grid", "open", "close", "state"):
        assert callable(getattr(m.L1Ms, name, None)), name
    assert (m.L1MS_NONE, m.L1MS_TCH, m.L1MS_XCCH, m.L1MS_ACCESS) == (0, 1, 2, 3) and m.L1MS_STATE_BYTES == 160
