"""trxsig_l1acq in the C-ABI: every entry point exported by libtrxsig.so and declared in include/trxsig_l1acq.h (and
trxsig_fec_sch_decode_batch in include/trxsig.h), refused with TRXSIG_EINVAL for NULL objects before anything touches a device,
the state bits, and the binding L1Acq / TrxSig.fec_sch_decode.  No GPU needed."""
import ctypes
import os
import re

import _pkg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["create", "destroy", "search", "detect_sch_batch", "sequence"]


def test_l1acq_in_the_abi():
    lib = ctypes.CDLL(os.path.join(ROOT, "openbts-ttsou_amd", "libtrxsig.so"))
    h = open(os.path.join(ROOT, "include", "trxsig_l1acq.h")).read()
    for s in SYMBOLS:
        assert hasattr(lib, "trxsig_l1acq_" + s), s
        assert re.search(r"\b(int|void)\s+trxsig_l1acq_%s\(" % s, h), s
    ht = open(os.path.join(ROOT, "include", "trxsig.h")).read()
    assert hasattr(lib, "trxsig_fec_sch_decode_batch") and re.search(r"\bint trxsig_fec_sch_decode_batch\(", ht)
    vp, i32, f32 = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
    lib.trxsig_l1acq_create.argtypes = [ctypes.POINTER(vp), vp, i32, i32]
    out = vp()
    assert lib.trxsig_l1acq_create(None, None, 1, 1000) == -1   # TRXSIG_EINVAL
    assert lib.trxsig_l1acq_create(ctypes.byref(out), None, 1, 1000) == -1 and not out.value
    lib.trxsig_l1acq_search.argtypes = [vp, vp, ctypes.c_int64, i32, i32, f32, f32, vp]
    lib.trxsig_l1acq_detect_sch_batch.argtypes = [vp, vp, vp, vp, i32, vp, f32, vp, vp, vp, vp, vp, vp, i32]
    lib.trxsig_l1acq_sequence.argtypes = [vp, vp, vp, vp]
    lib.trxsig_fec_sch_decode_batch.argtypes = [vp, vp, i32, i32, vp, vp, vp]
    assert lib.trxsig_l1acq_search(None, None, 0, 0, 0, 0.5, 8.0, None) == -1
    assert lib.trxsig_l1acq_detect_sch_batch(None, None, None, None, 0, None, 8.0, None, None, None, None, None, None, 148) == -1
    assert lib.trxsig_l1acq_sequence(None, None, None, None) == -1
    assert lib.trxsig_fec_sch_decode_batch(None, None, 148, 0, None, None, None) == -1
    lib.trxsig_l1acq_destroy.argtypes = [vp]; lib.trxsig_l1acq_destroy.restype = None
    lib.trxsig_l1acq_destroy(None)
    # the new kernels have no profiler id: the table (ABI 2) stays where it was
    assert lib.trxsig_kernel_count() == 28


def test_state_bits_and_thresholds():
    h = open(os.path.join(ROOT, "include", "trxsig_l1acq.h")).read()
    e = {n: int(v) for n, v in re.findall(r"(TRXSIG_ACQ_\w+)\s*=\s*(\d+)", h)}
    assert (e["TRXSIG_ACQ_FCCH"], e["TRXSIG_ACQ_WINDOW"], e["TRXSIG_ACQ_SCH"], e["TRXSIG_ACQ_DECODED"]) == (1, 2, 4, 8)
    assert re.search(r"#define TRXSIG_L1ACQ_FCCH_THRESH 0\.5f", h) and re.search(r"#define TRXSIG_L1ACQ_SCH_THRESH 8\.0f", h)
    assert "Not here: acquisition" not in open(os.path.join(ROOT, "include", "trxsig_l1msrx.h")).read()


def test_python_binding():
    m = _pkg.load()
    for name in ("search", "detect_sch", "sequence", "collect", "destroy"):
        assert callable(getattr(m.L1Acq, name, None)), name
    assert callable(getattr(m.TrxSig, "fec_sch_decode", None))
    assert (m.ACQ_FCCH, m.ACQ_WINDOW, m.ACQ_SCH, m.ACQ_DECODED) == (1, 2, 4, 8)
    assert ctypes.sizeof(m.L1AcqOut) == 2 * 4 + 15 * ctypes.sizeof(ctypes.c_void_p)
