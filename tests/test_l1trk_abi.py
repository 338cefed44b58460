"""trxsig_l1trk in the C-ABI: every entry point exported by libtrxsig.so (and the tuning build) and declared in
include/trxsig_l1trk.h, refused with TRXSIG_EINVAL for a NULL object, context or plan before anything touches a device, the
records' layout, and the binding L1Trk.  No GPU needed (the refusals that need a live object are in tests/test_gpu_l1trk.py)."""
import ctypes
import os
import re

import _pkg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["create", "destroy", "seed", "set", "state", "slice", "update"]


def test_l1trk_in_the_abi():
    h = open(os.path.join(ROOT, "include", "trxsig_l1trk.h")).read()
    for so in ("libtrxsig.so", "libtrxsig_tune.so"):
        lib = ctypes.CDLL(os.path.join(ROOT, "openbts-ttsou_amd", so))
        for s in SYMBOLS:
            assert hasattr(lib, "trxsig_l1trk_" + s), (so, s)
            assert re.search(r"\b(int|void)\s+trxsig_l1trk_%s\(" % s, h), s
        # the new kernels have no profiler id: the table (ABI 2) stays where it was
        assert lib.trxsig_kernel_count() == 28
    vp, i32, i64, u32, f32 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_uint32, ctypes.c_float
    lib.trxsig_l1trk_create.argtypes = [ctypes.POINTER(vp), vp, i32, i32, vp, vp, i32, i32, i32, f32]
    out = vp()
    phone, c0 = (ctypes.c_int32 * 2)(0, 0), (ctypes.c_int32 * 1)(0)
    assert lib.trxsig_l1trk_create(None, None, 1, 2, phone, c0, 17, 1, 512, 0.5) == -1       # TRXSIG_EINVAL
    assert lib.trxsig_l1trk_create(ctypes.byref(out), None, 1, 2, phone, c0, 17, 1, 512, 0.5) == -1 and not out.value
    lib.trxsig_l1trk_seed.argtypes = [vp, vp, vp]
    lib.trxsig_l1trk_set.argtypes = [vp, i32, i32, i32, i64, u32, u32]
    lib.trxsig_l1trk_state.argtypes = [vp, vp]
    lib.trxsig_l1trk_slice.argtypes = [vp, vp, i64, i64, i32, i32, i32, vp, i64, i64, vp]
    lib.trxsig_l1trk_update.argtypes = [vp, vp, i32, vp]
    assert lib.trxsig_l1trk_seed(None, None, None) == -1 and lib.trxsig_l1trk_set(None, 0, 1, 0, 0, 0, 0) == -1
    assert lib.trxsig_l1trk_state(None, None) == -1
    assert lib.trxsig_l1trk_slice(None, None, 0, 0, 1, 0, 1, None, 0, 0, None) == -1
    assert lib.trxsig_l1trk_update(None, None, 0, None) == -1
    lib.trxsig_l1trk_destroy.argtypes = [vp]; lib.trxsig_l1trk_destroy.restype = None
    lib.trxsig_l1trk_destroy(None)
    assert re.search(r"TRXSIG_TRK_CLIPPED = 1\b", h) and re.search(r"TRXSIG_TRK_UNLOCKED = 2\b", h)
    assert re.search(r"#define TRXSIG_L1TRK_MAX_FRAMES 65536\b", h) and re.search(r"#define TRXSIG_L1TRK_MAX_GATE \(1 << 24\)", h)
    # the arctangent is shared, not copied: one definition, in the device header both kernel files include
    csrc = os.path.join(ROOT, "openbts-ttsou_amd", "csrc")
    defs = [f for f in os.listdir(csrc) if f.endswith((".hip", ".h", ".cpp")) and "float acq_atan2(float y, float x) {" in open(os.path.join(csrc, f)).read()]
    assert defs == ["trxsig_l1acq_dev.h"]
    for f in ("trxsig_l1acq.hip", "trxsig_l1trk.hip"):
        assert '#include "trxsig_l1acq_dev.h"' in open(os.path.join(csrc, f)).read()


def test_python_binding():
    m = _pkg.load()
    for name in ("seed", "set", "state", "slice", "update", "collect", "destroy"):
        assert callable(getattr(m.L1Trk, name, None)), name
    p = ctypes.sizeof(ctypes.c_void_p)
    assert ctypes.sizeof(m.L1TrkView) == 12 * p and m.L1TrkView.d_fn.offset == p and m.L1TrkView.d_afc_delta.offset == 11 * p
    assert ctypes.sizeof(m.L1TrkMeas) == 16 + 5 * p and m.L1TrkMeas.d_status.offset == 16 and m.L1TrkMeas.fcch_stride.offset == 12
    assert (m.TRK_CLIPPED, m.TRK_UNLOCKED, m.TRK_MAX_FRAMES, m.TRK_MAX_GATE) == (1, 2, 65536, 1 << 24)


def test_documents_name_the_object():
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert "trxsig_l1trk" in design and "k_l1trk_slice" in design and "trxsig_l1trk" in readme and "l1trk_bench" in readme
    assert "l1acq -> l1trk -> " in readme.replace("→", "->")
