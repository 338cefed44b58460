"""The access burst's coders in the C-ABI: the entry points exported by libtrxsig.so (and the tuning build) and declared in
include/trxsig.h, refused with TRXSIG_EINVAL for a NULL context before anything touches a device; the header's statement and
its constants; the header as C99; the binding; one copy of the coder and of the trellis; the documents.  No GPU needed (the
refusals that need a live context are in tests/test_gpu_access.py)."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest

import _pkg
import access_model as am

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "trxsig.h")
CSRC = os.path.join(ROOT, "openbts-ttsou_amd", "csrc")
vp, i32, i64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64
NAMES = ("trxsig_fec_access_encode_batch", "trxsig_fec_access_decode_batch")


def libs():
    for so in ("libtrxsig.so", "libtrxsig_tune.so"):
        lib = ctypes.CDLL(os.path.join(ROOT, "openbts-ttsou_amd", so))
        lib.trxsig_fec_access_encode_batch.argtypes = [vp, vp, vp, vp, i32, vp]
        lib.trxsig_fec_access_decode_batch.argtypes = [vp, vp, i32, i64, vp, i32, i32, i32, i32, vp, vp, vp, vp]
        yield so, lib


def test_access_in_the_abi():
    h = open(HEADER).read()
    for so, lib in libs():
        for s in NAMES:
            assert hasattr(lib, s), (so, s)
            assert re.search(r"\bint\s+%s\(" % s, h), s
        # the new kernels are booked under TRXSIG_K_FEC: the profiler's table and the ABI version stay where they were
        assert lib.trxsig_kernel_count() == 28 and lib.trxsig_abi_version() == 2
        buf = (ctypes.c_uint8 * 4096)()
        assert lib.trxsig_fec_access_encode_batch(None, buf, buf, buf, 1, buf) == -1              # TRXSIG_EINVAL
        assert lib.trxsig_fec_access_encode_batch(None, None, None, None, 0, None) == -1
        assert lib.trxsig_fec_access_decode_batch(None, buf, 148, 4, None, 1, 0, -1, 0, buf, None, None, None) == -1
        assert lib.trxsig_fec_access_decode_batch(None, None, 148, 0, None, 0, 0, 0, 0, None, None, None, None) == -1


def test_header_states_the_coders():
    h = open(HEADER).read()
    flat = " ".join(h.split())
    assert re.search(r"\bTRXSIG_ACCESS_8 = %d\b" % am.ACCESS_8, h) and re.search(r"\bTRXSIG_ACCESS_11 = %d\b" % am.ACCESS_11, h)
    assert re.search(r"#define TRXSIG_ACCESS_MAX_BURSTS 16777216\b", h)
    assert "C(%s) and C(%d) are not sent" % ("), C(".join(map(str, am.DELETED[:-1])), am.DELETED[-1]) in flat
    for text in ("GSM 05.03 5.3.2", "NOT CHECKED AGAINST THE STANDARD", "d(0..10)", "u(0..20)", "C(0..41)", "exactly 0.5F",
                 "ties to the lower scheme", "Parity(0x6f, 6, 8)", "trxsig_fec_rach_decode_batch returns", "trxsig_l1ms_encode writes",
                 "k_fec_access_encode, k_fec_access_decode", "TRXSIG_K_FEC", "all-zero row", "n == 0 is a no-op"):
        assert text in flat, text


def test_header_compiles_as_c(tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    if cc is None:
        pytest.fail("no C compiler to check the header with")
    src = tmp_path / "acc.c"
    src.write_text('#include "trxsig.h"\nint use(trxsig_ctx *c, uint16_t *r, uint8_t *p) {\n'
                   "  return trxsig_fec_access_encode_batch(c, r, p, p, TRXSIG_ACCESS_11, p) + TRXSIG_ACCESS_8 +\n"
                   "         trxsig_fec_access_decode_batch(c, 0, 148, 0, 0, 0, 0, -1, 63, r, p, p, p) + TRXSIG_ACCESS_MAX_BURSTS;\n}\n")
    r = subprocess.run([cc, "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o",
                        str(tmp_path / "acc.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_python_binding():
    m = _pkg.load()
    assert callable(m.TrxSig.access_encode) and callable(m.TrxSig.access_decode)
    assert (m.ACCESS_8, m.ACCESS_11) == (0, 1)
    from openbts_ttsou_amd import _abi
    for s in NAMES:
        assert s in _abi.SIGNATURES


def test_one_coder_one_trellis():
    """The kernels share the file's one fec_trellis; the access coder exists once, in trxsig_fec_enc.h, where rach_e36 -- what the
    two multiplexers call -- is its 8-bit case; the deleted positions are written once each way."""
    fec = open(os.path.join(CSRC, "trxsig_fec.hip")).read()
    enc = open(os.path.join(CSRC, "trxsig_fec_enc.h")).read()
    assert len(re.findall(r"unsigned fec_trellis\(", fec)) == 1 and fec.count("fec_trellis(") >= 6
    assert "k_fec_access_encode" in fec and "k_fec_access_decode" in fec
    assert len(re.findall(r"unsigned long long access_coder\(", enc)) == 1 and "access_coder" not in fec
    assert re.search(r"rach_e36\(unsigned ra, unsigned bsic\) \{ return access_coder<8>\(ra, bsic\); \}", enc)
    assert fec.count("access_e36(") == 1 and fec.count("access_cindex(") == 1 and "0x19" not in fec
    for name in ("trxsig_l1ms.hip", "trxsig_l1tx.hip"):
        assert "access_coder" not in open(os.path.join(CSRC, name)).read()


def test_documents_name_the_coders():
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert "The access burst's two coders" in design
    assert all(k in design for k in ("k_fec_access_encode", "k_fec_access_decode", "trxsig_fec_access_decode_batch", "l1pacc_bench"))
    assert "trxsig_fec_access_decode_batch" in readme and "l1pacc_bench" in readme and "from memory" in readme
    assert "trxsig_fec_access_decode_batch" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
