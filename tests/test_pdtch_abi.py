"""The GPRS packet data block coders in the C-ABI: the entry points exported by libtrxsig.so (and the tuning build) and
declared in include/trxsig.h, refused with TRXSIG_EINVAL for a NULL context before anything touches a device;
trxsig_pdch_map_host over the 52-multiframe and at a negative frame number; the header's statement; the binding; the
documents.  No GPU needed (the refusals that need a live context are in tests/test_gpu_pdtch.py)."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest

import _pkg
import pdtch_model as pm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "trxsig.h")
vp, i32, i64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64


def libs():
    for so in ("libtrxsig.so", "libtrxsig_tune.so"):
        lib = ctypes.CDLL(os.path.join(ROOT, "openbts-ttsou_amd", so))
        lib.trxsig_fec_pdtch_encode_batch.argtypes = [vp, vp, vp, vp, i32, vp]
        lib.trxsig_fec_pdtch_decode_batch.argtypes = [vp, vp, i32, i64, vp, i32, i32, i32, vp, vp, vp, vp, vp]
        lib.trxsig_pdch_map_host.argtypes = [ctypes.c_int32, ctypes.POINTER(i32), ctypes.POINTER(i32)]
        yield so, lib


def test_pdtch_in_the_abi():
    h = open(HEADER).read()
    for so, lib in libs():
        for s in ("trxsig_fec_pdtch_encode_batch", "trxsig_fec_pdtch_decode_batch", "trxsig_pdch_map_host"):
            assert hasattr(lib, s), (so, s)
            assert re.search(r"\bint\s+%s\(" % s, h), s
        # the new kernels are booked under TRXSIG_K_FEC: the profiler's table (ABI 2) stays where it was
        assert lib.trxsig_kernel_count() == 28
        buf = (ctypes.c_uint8 * 4096)()
        assert lib.trxsig_fec_pdtch_encode_batch(None, buf, buf, buf, 1, buf) == -1            # TRXSIG_EINVAL
        assert lib.trxsig_fec_pdtch_encode_batch(None, None, None, None, 0, None) == -1
        assert lib.trxsig_fec_pdtch_decode_batch(None, buf, 148, 4, None, 1, 0, -1, buf, None, None, None, None) == -1
        assert lib.trxsig_fec_pdtch_decode_batch(None, None, 148, 0, None, 0, 0, -1, None, None, None, None, None) == -1


def test_pdch_map_host():
    for so, lib in libs():
        block, burst = i32(7), i32(7)
        for fn in range(52):
            for base in (0, 52, 52 * 51 * 26 * 2047):
                assert lib.trxsig_pdch_map_host(base + fn, ctypes.byref(block), ctypes.byref(burst)) == 0
                assert (block.value, burst.value) == pm.pdch_map(fn), (so, fn)
        block.value = burst.value = 7
        assert lib.trxsig_pdch_map_host(-1, ctypes.byref(block), ctypes.byref(burst)) == -1
        assert lib.trxsig_pdch_map_host(-52, ctypes.byref(block), ctypes.byref(burst)) == -1
        assert (block.value, burst.value) == (7, 7)                                              # nothing written
        assert lib.trxsig_pdch_map_host(0, None, ctypes.byref(burst)) == -1
        assert lib.trxsig_pdch_map_host(0, ctypes.byref(block), None) == -1


def test_header_states_the_coders():
    h = open(HEADER).read()
    flat = " ".join(h.split())
    for cs, name in enumerate(("TRXSIG_CS1", "TRXSIG_CS2", "TRXSIG_CS3", "TRXSIG_CS4")):
        assert re.search(r"\b%s = %d\b" % (name, cs), h)
    assert re.search(r"#define TRXSIG_PDTCH_BLOCK_BYTES %d\b" % pm.BLOCK_BYTES, h)
    assert " ".join(pm.USF6) in flat and " ".join(pm.USF12) in flat
    for cs, word in enumerate(pm.FLAGS):
        assert "CS-%d %s" % (cs + 1, word) in flat
    for text in ("184 / 271 / 315 / 431", "D^16 + D^12 + D^5 + 1", "Parity(0x11021, 16, K)", "C(3 + 4j)", "j = 9 mod 12",
                 "C(3 + 6j) and C(5 + 6j)", "j = 2..111", "q(2B) is bit 87 and q(2B + 1) bit 60 of burst B",
                 "NOT CHECKED AGAINST THE STANDARD", "ties to the lower scheme", "ties to the first row", "exactly 0.5"):
        assert text in flat, text


def test_header_compiles_as_c(tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    if cc is None:
        pytest.fail("no C compiler to check the header with")
    src = tmp_path / "pd.c"
    src.write_text('#include "trxsig.h"\nint use(trxsig_ctx *c, uint8_t *p, int *b) {\n'
                   "  return trxsig_fec_pdtch_encode_batch(c, p, p, p, TRXSIG_CS4, p) + trxsig_pdch_map_host(0, b, b) +\n"
                   "         trxsig_fec_pdtch_decode_batch(c, 0, 148, 0, 0, 0, 0, -1, p, p, p, p, p) + TRXSIG_PDTCH_BLOCK_BYTES;\n}\n")
    r = subprocess.run([cc, "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o",
                        str(tmp_path / "pd.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_python_binding():
    m = _pkg.load()
    assert callable(m.TrxSig.pdtch_encode) and callable(m.TrxSig.pdtch_decode)
    assert (m.CS1, m.CS2, m.CS3, m.CS4) == (0, 1, 2, 3) and m.PDTCH_BLOCK_BYTES == 54
    assert [m.pdch_map(fn) for fn in range(52)] == [pm.pdch_map(fn) for fn in range(52)]
    with pytest.raises(m.TrxSigError):
        m.pdch_map(-1)
    from openbts_ttsou_amd import _abi
    for s in ("trxsig_fec_pdtch_encode_batch", "trxsig_fec_pdtch_decode_batch", "trxsig_pdch_map_host"):
        assert s in _abi.SIGNATURES


def test_kernels_share_the_trellis():
    """One fec_trellis in the file the new kernels live in, and the parity table generated, not typed in."""
    src = open(os.path.join(ROOT, "openbts-ttsou_amd", "csrc", "trxsig_fec.hip")).read()
    assert len(re.findall(r"unsigned fec_trellis\(", src)) == 1 and src.count("fec_trellis(") >= 4
    assert "k_fec_pdtch_encode" in src and "k_fec_pdtch_decode" in src
    assert re.search(r"struct PdPar \{.*?constexpr PdPar\(\)", src, re.S)


def test_documents_name_the_coders():
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert all(k in design for k in ("k_fec_pdtch_encode", "k_fec_pdtch_decode", "trxsig_fec_pdtch_decode_batch", "pdtch_bench"))
    assert "trxsig_fec_pdtch_encode_batch" in readme and "pdtch_bench" in readme
