"""trxsig_l1msrx in the C-ABI: every entry point exported by libtrxsig.so and declared in include/trxsig_l1msrx.h (and
trxsig_l1ms_follow in include/trxsig_l1ms.h), refused with TRXSIG_EINVAL for NULL objects before anything touches a device, the
class and kind numbers, and the binding L1MsRx / L1Ms.follow.  No GPU needed."""
import ctypes
import os
import re

import _pkg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["create", "destroy", "channels", "channel", "open", "close", "decode", "state"]


def enum_values(text):
    out = {}
    for body in re.findall(r"enum\s*\{([^}]*)\}", text):
        for name, val in re.findall(r"(TRXSIG_L1_\w+)\s*=\s*(\d+)", body):
            out[name] = int(val)
    return out


def test_l1msrx_in_the_abi():
    lib = ctypes.CDLL(os.path.join(ROOT, "openbts-ttsou_amd", "libtrxsig.so"))
    h = open(os.path.join(ROOT, "include", "trxsig_l1msrx.h")).read()
    for s in SYMBOLS:
        assert hasattr(lib, "trxsig_l1msrx_" + s), s
        assert re.search(r"\b(int|void) trxsig_l1msrx_%s\(" % s, h), s
    hm = open(os.path.join(ROOT, "include", "trxsig_l1ms.h")).read()
    assert hasattr(lib, "trxsig_l1ms_follow") and re.search(r"\bint trxsig_l1ms_follow\(", hm)
    vp, i32 = ctypes.c_void_p, ctypes.c_int
    lib.trxsig_l1msrx_create.argtypes = [ctypes.POINTER(vp), vp, i32, vp, i32, i32]
    out = vp()
    assert lib.trxsig_l1msrx_create(None, None, 1, None, 0, 900) == -1   # TRXSIG_EINVAL
    assert lib.trxsig_l1msrx_create(ctypes.byref(out), None, 1, None, 0, 900) == -1 and not out.value
    lib.trxsig_l1msrx_decode.argtypes = [vp, vp, i32, i32, vp]
    lib.trxsig_l1msrx_open.argtypes = lib.trxsig_l1msrx_close.argtypes = [vp, i32, i32]
    lib.trxsig_l1msrx_channels.argtypes = [vp, i32]
    lib.trxsig_l1msrx_channel.argtypes = [vp, i32, i32, vp, vp, vp, vp]
    lib.trxsig_l1msrx_state.argtypes = [vp, i32, vp]
    lib.trxsig_l1ms_follow.argtypes = [vp, vp]
    assert lib.trxsig_l1msrx_decode(None, None, 0, 1, None) == -1
    assert lib.trxsig_l1msrx_open(None, 0, 0) == -1 and lib.trxsig_l1msrx_close(None, 0, 0) == -1
    assert lib.trxsig_l1msrx_channels(None, 0) == -1 and lib.trxsig_l1msrx_channel(None, 0, 0, None, None, None, None) == -1
    assert lib.trxsig_l1msrx_state(None, 0, None) == -1
    assert lib.trxsig_l1ms_follow(None, None) == -1
    lib.trxsig_l1msrx_destroy.argtypes = [vp]; lib.trxsig_l1msrx_destroy.restype = None
    lib.trxsig_l1msrx_destroy(None)
    # no kernel id was added: the profiler's table (ABI 2) stays where it was
    assert lib.trxsig_kernel_count() == 28


def test_class_and_kind_numbers():
    inc = os.path.join(ROOT, "include")
    e = {}
    for f in ("trxsig_l1rx.h", "trxsig_l1tx.h", "trxsig_l1msrx.h"):
        e.update(enum_values(open(os.path.join(inc, f)).read()))
    assert (e["TRXSIG_L1_TCH"], e["TRXSIG_L1_XCCH"], e["TRXSIG_L1_RACH"], e["TRXSIG_L1_CCCH"]) == (0, 1, 2, 3)
    assert (e["TRXSIG_L1_BCCH"], e["TRXSIG_L1_SCH"], e["TRXSIG_L1_FCCH"]) == (4, 5, 6)
    assert [e["TRXSIG_L1_" + k] for k in ("TCHF", "SACCH_TF", "SDCCH8", "SACCH_C8", "SDCCH4", "SACCH_C4", "RACH_C5", "CCCH_C5")] == \
        list(range(8))
    assert (e["TRXSIG_L1_BCCH_C5"], e["TRXSIG_L1_SCH_C5"], e["TRXSIG_L1_FCCH_C5"]) == (8, 9, 10)


def test_python_binding():
    m = _pkg.load()
    for name in ("decode", "collect", "open", "close", "channels", "channel", "state", "destroy"):
        assert callable(getattr(m.L1MsRx, name, None)), name
    assert callable(getattr(m.L1Ms, "follow", None))
    assert (m.L1_BCCH, m.L1_SCH, m.L1_FCCH) == (4, 5, 6) and (m.L1_BCCH_C5, m.L1_SCH_C5, m.L1_FCCH_C5) == (8, 9, 10)
    assert ctypes.sizeof(m.L1MsRxOut) == 8 * 4 + 36 * ctypes.sizeof(ctypes.c_void_p)
