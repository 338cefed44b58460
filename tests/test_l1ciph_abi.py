"""trxsig_l1ciph in the C-ABI: every entry point exported by libtrxsig.so (and the tuning build) and declared in
include/trxsig_l1ciph.h, refused with TRXSIG_EINVAL for a NULL object, context or plan before anything touches a device, the
constants, and the binding L1Ciph.  No GPU needed (the refusals that need a live object are in tests/test_gpu_l1ciph.py)."""
import ctypes
import os
import re

import _pkg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["create", "destroy", "channels", "channel", "set", "state", "bits", "soft"]


def test_l1ciph_in_the_abi():
    h = open(os.path.join(ROOT, "include", "trxsig_l1ciph.h")).read()
    assert '#include "trxsig_l1ms.h"' in h
    for so in ("libtrxsig.so", "libtrxsig_tune.so"):
        lib = ctypes.CDLL(os.path.join(ROOT, "openbts-ttsou_amd", so))
        for s in SYMBOLS:
            assert hasattr(lib, "trxsig_l1ciph_" + s), (so, s)
            assert re.search(r"\b(int|void)\s+trxsig_l1ciph_%s\(" % s, h), s
        assert hasattr(lib, "trxsig_a5_1_blocks_batch") and re.search(r"\bint\s+trxsig_a5_1_blocks_batch\(", h)
        # the new kernels have no profiler id: the table (ABI 2) stays where it was
        assert lib.trxsig_kernel_count() == 28
    vp, i32, u32 = ctypes.c_void_p, ctypes.c_int, ctypes.c_uint32
    lib.trxsig_l1ciph_create.argtypes = [ctypes.POINTER(vp), vp, i32, vp]
    out = vp()
    comb = (ctypes.c_uint8 * 8)(5, 7, 1, 0, 0, 0, 0, 0)
    assert lib.trxsig_l1ciph_create(None, None, 1, comb) == -1                               # TRXSIG_EINVAL
    assert lib.trxsig_l1ciph_create(ctypes.byref(out), None, 1, comb) == -1 and not out.value
    assert lib.trxsig_l1ciph_create(ctypes.byref(out), None, 1, None) == -1 and not out.value
    lib.trxsig_a5_1_blocks_batch.argtypes = [vp, i32, vp, vp, vp, vp]
    assert lib.trxsig_a5_1_blocks_batch(None, 0, None, None, None, None) == -1
    lib.trxsig_l1ciph_channels.argtypes = [vp, i32]
    lib.trxsig_l1ciph_channel.argtypes = [vp, i32, i32, vp, vp, vp, vp]
    lib.trxsig_l1ciph_set.argtypes = [vp, i32, i32, i32, vp]
    lib.trxsig_l1ciph_state.argtypes = [vp, i32, vp]
    lib.trxsig_l1ciph_bits.argtypes = [vp, i32, i32, i32, vp, vp, u32]
    lib.trxsig_l1ciph_soft.argtypes = [vp, i32, vp, i32]
    assert lib.trxsig_l1ciph_channels(None, 0) == -1 and lib.trxsig_l1ciph_channel(None, 0, 0, None, None, None, None) == -1
    assert lib.trxsig_l1ciph_set(None, 0, 0, 1, comb) == -1 and lib.trxsig_l1ciph_state(None, 0, None) == -1
    assert lib.trxsig_l1ciph_bits(None, 0, 0, 1, None, None, 0) == -1 and lib.trxsig_l1ciph_soft(None, 0, None, 0) == -1
    lib.trxsig_l1ciph_destroy.argtypes = [vp]; lib.trxsig_l1ciph_destroy.restype = None
    lib.trxsig_l1ciph_destroy(None)
    assert re.search(r"TRXSIG_A5_OFF = 0\b", h) and re.search(r"TRXSIG_A5_1 = 1\b", h)
    assert re.search(r"#define TRXSIG_L1CIPH_STATE_BYTES 16\b", h)
    # A5/1 is stated once, in the device header the host side and the kernels both include
    csrc = os.path.join(ROOT, "openbts-ttsou_amd", "csrc")
    defs = [f for f in os.listdir(csrc) if f.endswith((".hip", ".h", ".cpp")) and "uint32_t a5_clock_maj(TrxA5 &s) {" in open(os.path.join(csrc, f)).read()]
    assert defs == ["trxsig_a5_dev.h"]
    for f in ("trxsig_l1ciph.hip", "trxsig_l1ciph.cpp"):
        assert '#include "trxsig_a5_dev.h"' in open(os.path.join(csrc, f)).read()


def test_python_binding():
    m = _pkg.load()
    for name in ("channels", "channel", "set", "state", "bits", "soft", "collect", "destroy"):
        assert callable(getattr(m.L1Ciph, name, None)), name
    assert callable(m.a5_1_blocks)
    assert (m.A5_OFF, m.A5_1, m.L1CIPH_STATE_BYTES) == (0, 1, 16)
    # the masks the two callers pass
    assert (1 << m.L1TX_XCCH | 1 << m.L1TX_TCH, 1 << m.L1MS_TCH | 1 << m.L1MS_XCCH) == (0x60, 0x06)


def test_documents_name_the_object():
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    readme = open(os.path.join(ROOT, "README.md")).read()
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "trxsig_l1ciph" in design and "k_l1ciph_bits" in design and "k_l1ciph_soft" in design
    assert "trxsig_l1ciph" in readme and "l1ciph_bench" in readme
    assert "trxsig_l1ciph_bits" in integration and "trxsig_l1ciph_soft" in integration
