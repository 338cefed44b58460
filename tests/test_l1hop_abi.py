"""trxsig_l1hop in the C-ABI: every entry point exported by libtrxsig.so (and the tuning build) and declared in
include/trxsig_l1hop.h, refused with TRXSIG_EINVAL for a NULL object, context or plan before anything touches a device; the
header compiles as C; the binding L1Hop; the documents.  No GPU needed (the refusals that need a live object are in
tests/test_gpu_l1hop.py)."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest

import _pkg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["create", "destroy", "groups", "members", "map", "bits", "cells", "result"]


def test_l1hop_in_the_abi():
    h = open(os.path.join(ROOT, "include", "trxsig_l1hop.h")).read()
    assert '#include "trxsig_l1ms.h"' in h
    for so in ("libtrxsig.so", "libtrxsig_tune.so"):
        lib = ctypes.CDLL(os.path.join(ROOT, "openbts-ttsou_amd", so))
        for s in SYMBOLS:
            assert hasattr(lib, "trxsig_l1hop_" + s), (so, s)
            assert re.search(r"\b(int|void)\s+trxsig_l1hop_%s\(" % s, h), s
        assert hasattr(lib, "trxsig_hop_mai_batch") and re.search(r"\bint\s+trxsig_hop_mai_batch\(", h)
        # the new kernels have no profiler id: the table (ABI 2) stays where it was
        assert lib.trxsig_kernel_count() == 28
    vp, i32, i64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64
    lib.trxsig_l1hop_create.argtypes = [ctypes.POINTER(vp), vp, i32, vp, vp, i32, vp, i32]
    out = vp()
    comb = (ctypes.c_uint8 * 8)(5, 7, 1, 0, 0, 0, 0, 0)
    group = (ctypes.c_int8 * 8)(-1, 0, -1, -1, -1, -1, -1, -1)
    hsn = (ctypes.c_uint8 * 1)(3)
    assert lib.trxsig_l1hop_create(None, None, 1, comb, group, 1, hsn, 8) == -1               # TRXSIG_EINVAL
    assert lib.trxsig_l1hop_create(ctypes.byref(out), None, 1, comb, group, 1, hsn, 8) == -1 and not out.value
    lib.trxsig_hop_mai_batch.argtypes = [vp, i32, vp, vp, vp, vp, vp]
    assert lib.trxsig_hop_mai_batch(None, 0, None, None, None, None, None) == -1
    lib.trxsig_l1hop_groups.argtypes = [vp]
    lib.trxsig_l1hop_members.argtypes = [vp, i32, i32, vp]
    lib.trxsig_l1hop_map.argtypes = [vp, i32, i32, vp]
    lib.trxsig_l1hop_bits.argtypes = [vp, i32, i32, i32, vp, vp]
    lib.trxsig_l1hop_cells.argtypes = [vp, i32, i32, i32, vp, i64, i64, vp, i64, i64]
    lib.trxsig_l1hop_result.argtypes = [vp, i32, vp, vp]
    assert lib.trxsig_l1hop_groups(None) == -1 and lib.trxsig_l1hop_members(None, 0, 0, None) == -1
    assert lib.trxsig_l1hop_map(None, 0, 1, None) == -1 and lib.trxsig_l1hop_bits(None, 1, 0, 1, None, None) == -1
    assert lib.trxsig_l1hop_cells(None, 1, 0, 1, None, 0, 0, None, 0, 0) == -1 and lib.trxsig_l1hop_result(None, 0, None, None) == -1
    lib.trxsig_l1hop_destroy.argtypes = [vp]; lib.trxsig_l1hop_destroy.restype = None
    lib.trxsig_l1hop_destroy(None)
    assert re.search(r"#define TRXSIG_L1HOP_MAX_N 64\b", h)
    # the header states the algorithm, the table's checks and the known answers, and what they pin
    for text in ("RNTABLE", "0xED53E222", "7446", "2 0 3 2 3 3 2 0 1 1 2 3 1 1 1 3 3 1 0 0", "47 41 7 57 45 9 6 52 35 34 35 11",
                 "NOT THE STANDARD"):
        assert text in h, text
    # the sequence is stated once, in the device header the host side and the kernels both include
    csrc = os.path.join(ROOT, "openbts-ttsou_amd", "csrc")
    defs = [f for f in os.listdir(csrc) if f.endswith((".hip", ".h", ".cpp")) and "inline int hop_s(" in open(os.path.join(csrc, f)).read()]
    assert defs == ["trxsig_hop_dev.h"]
    for f in ("trxsig_l1hop.hip", "trxsig_l1hop.cpp"):
        assert '#include "trxsig_hop_dev.h"' in open(os.path.join(csrc, f)).read()
    mk = open(os.path.join(csrc, "Makefile")).read()
    assert re.search(r"^KERNELS := .*\btrxsig_l1hop\b", mk, re.M) and re.search(r"^HOSTSRC := .*\btrxsig_l1hop_host\b", mk, re.M)
    assert re.search(r"^HDRS .*include/trxsig_l1hop\.h", mk, re.M)


def test_header_compiles_as_c(tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    if cc is None:
        pytest.fail("no C compiler to check the header with")
    src = tmp_path / "hop.c"
    src.write_text('#include "trxsig_l1hop.h"\nint use(trxsig_l1hop *h) { return trxsig_l1hop_groups(h) + TRXSIG_L1HOP_MAX_N; }\n')
    r = subprocess.run([cc, "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o",
                        str(tmp_path / "hop.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_python_binding():
    m = _pkg.load()
    for name in ("map", "bits", "cells", "result", "groups", "members", "destroy"):
        assert callable(getattr(m.L1Hop, name, None)), name
    assert callable(m.hop_mai) and m.L1HOP_MAX_N == 64


def test_documents_name_the_object():
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    readme = open(os.path.join(ROOT, "README.md")).read()
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "trxsig_l1hop" in design and all(k in design for k in ("k_hop_mai", "k_hop_bits", "k_hop_cells", "k_hop_result"))
    assert "trxsig_l1hop" in readme and "l1hop_bench" in readme
    assert all(k in integration for k in ("trxsig_l1hop_bits", "trxsig_l1hop_cells", "trxsig_l1hop_result"))
