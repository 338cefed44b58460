"""Packet data channels through L1 in the C-ABI: the entry points exported by libtrxsig.so (and the tuning build) and declared in
include/trxsig_l1pdch.h, the enum values, the refusals that need no device, the header's statement, the binding and its
structures against the C compiler's layout, the documents.  No GPU needed (the refusals that need a live context are the last
test of tests/test_gpu_l1pdch.py)."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest

import _pkg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
HEADER = os.path.join(INCLUDE, "trxsig_l1pdch.h")
ENTRY = ("create", "destroy", "channels", "channel", "grid", "state", "encode", "decode")
vp, i32 = ctypes.c_void_p, ctypes.c_int


def test_l1pdch_in_the_abi():
    h = open(HEADER).read()
    for so in ("libtrxsig.so", "libtrxsig_tune.so"):
        lib = ctypes.CDLL(os.path.join(ROOT, "openbts-ttsou_amd", so))
        for s in ENTRY:
            assert hasattr(lib, "trxsig_l1pdch_" + s), (so, s)
            assert re.search(r"\b(int|void)\s+trxsig_l1pdch_%s\(" % s, h), s
        assert lib.trxsig_kernel_count() == 28 and lib.trxsig_abi_version() == 2      # booked under TRXSIG_K_FEC: no new row
        lib.trxsig_l1pdch_create.argtypes = [ctypes.POINTER(vp), vp, i32, vp, i32, i32]
        out = vp(7)
        comb = (ctypes.c_uint8 * 8)(0, 13, 1, 7, 0, 0, 0, 13)
        bad = (ctypes.c_uint8 * 8)(0, 13, 2, 7, 0, 0, 0, 13)
        # the create-time refusals, each TRXSIG_EINVAL with nothing made: no context; combination 2; dir 2; n_arfcn 0
        for args in ((1, comb, 5, 0), (1, bad, 5, 0), (1, comb, 5, 2), (0, comb, 5, 0)):
            out.value = 7
            assert lib.trxsig_l1pdch_create(ctypes.byref(out), None, *args) == -1
        assert lib.trxsig_l1pdch_create(None, None, 1, comb, 5, 0) == -1
        for f in ("channels", "grid", "state", "encode", "decode"):
            getattr(lib, "trxsig_l1pdch_" + f).argtypes = None
        assert lib.trxsig_l1pdch_channels(None, 0) == -1 and lib.trxsig_l1pdch_grid(None, 0, 4, None, None) == -1
        assert lib.trxsig_l1pdch_state(None, 0, None) == -1
        assert lib.trxsig_l1pdch_encode(None, 0, 4, None, None, None, None) == -1
        assert lib.trxsig_l1pdch_decode(None, None, 0, 1, -1, None, None) == -1
        lib.trxsig_l1pdch_destroy.argtypes = [vp]
        lib.trxsig_l1pdch_destroy(None)


def enum_values(text):
    out = {}
    for body in re.findall(r"enum\s*\{([^}]*)\}", re.sub(r"/\*.*?\*/", " ", text, flags=re.S)):
        for name, val in re.findall(r"(\w+)\s*=\s*(-?\d+)", body):
            out[name] = int(val)
    return out


def test_enum_values():
    e = enum_values(open(HEADER).read())
    assert (e["TRXSIG_L1PDCH_DOWN"], e["TRXSIG_L1PDCH_UP"]) == (0, 1)
    assert (e["TRXSIG_L1PDCH_PDTCH"], e["TRXSIG_L1PDCH_PTCCH"]) == (0, 1)
    assert e["TRXSIG_L1TX_PDCH"] == 8 and e["TRXSIG_L1PDCH_COMB"] == 13
    tx = {k: v for k, v in enum_values(open(os.path.join(INCLUDE, "trxsig_l1tx.h")).read()).items() if k.startswith("TRXSIG_L1TX_")}
    assert len(tx) == 8 and e["TRXSIG_L1TX_PDCH"] not in tx.values() and "TRXSIG_L1TX_PDCH" not in tx


def test_header_states_the_object():
    flat = " ".join(open(HEADER).read().split())
    for text in ("NOT CHECKED AGAINST THE STANDARD", "written from memory of GSM 05.02", "FN mod 104 = 12, 38, 64, 90",
                 "12 * (FN / 52) + B", "12 * 52224", "13 marks a packet data channel", "bsic & 7", "trxsig_trxgroup_add_l1tx",
                 "until that object's next encode", "neither reads nor clears", "missing bursts at 0.5", "TRXSIG_K_FEC",
                 "PTCCH/U and PRACH", "timing-advance", "USF gating", "dummy control blocks", "RLC/MAC", "EGPRS", "hopping or ciphering"):
        assert text in flat, text
    assert re.search(r"#define TRXSIG_L1PDCH_STATE_BYTES 3104\b", flat) and re.search(r"#define TRXSIG_L1PDCH_RING 32\b", flat)


def test_header_compiles_as_c(tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    if cc is None:
        pytest.fail("no C compiler to check the header with")
    src = tmp_path / "pd.c"
    src.write_text('#include "trxsig_l1pdch.h"\nint use(trxsig_l1pdch *p, trxsig_l1pdch_in *i, trxsig_l1pdch_out *o, trxsig_l1pdch_dec *d,\n'
                   "        const trxsig_trxgroup_result *r) {\n"
                   "  return trxsig_l1pdch_encode(p, 0, 4, i, 0, 0, o) + trxsig_l1pdch_decode(p, r, 0, 1, -1, p, d) + TRXSIG_L1TX_PDCH +\n"
                   "         TRXSIG_L1PDCH_STATE_BYTES;\n}\n")
    r = subprocess.run([cc, "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", INCLUDE, "-c", str(src), "-o", str(tmp_path / "pd.o")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_python_binding_and_structures(tmp_path):
    m = _pkg.load()
    from openbts_ttsou_amd import _abi, _abi_l1pdch
    for s in ENTRY:
        assert "trxsig_l1pdch_" + s in _abi.SIGNATURES
    for name in ("destroy", "channels", "channel", "grid", "state", "encode", "decode", "collect", "collect_decode", "states", "circuit_plan"):
        assert callable(getattr(m.L1Pdch, name)), name
    assert issubclass(m.L1Pdch, m._Object) and not hasattr(m.L1Pdch, "open") and not hasattr(m.L1Pdch, "close")
    assert (m.L1PDCH_DOWN, m.L1PDCH_UP, m.L1PDCH_PDTCH, m.L1PDCH_PTCCH, m.L1PDCH_COMB, m.L1TX_PDCH) == (0, 1, 0, 1, 13, 8)
    assert (m.L1PDCH_STATE_BYTES, m.L1PDCH_RING) == (3104, 32)
    assert m.L1TX_PDCH not in (m.L1TX_NONE, m.L1TX_FCCH, m.L1TX_SCH, m.L1TX_BCCH, m.L1TX_CCCH, m.L1TX_XCCH, m.L1TX_TCH, m.L1TX_IDLE)
    # the three structures against the C compiler's layout, as tests/test_binding_abi.py holds _abi's own
    structs = [_abi_l1pdch.L1PdchIn, _abi_l1pdch.L1PdchOut, _abi_l1pdch.L1PdchDec]
    assert all(getattr(m, s.__name__) is s for s in structs)
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler to lay the structures out with")
    lines = ["#include <cstddef>", "#include <cstdio>", '#include "trxsig_l1pdch.h"', "int main() {"]
    want = {}
    for s in structs:
        lines.append('  std::printf("%s %%zu\\n", sizeof(%s));' % (s.__name__, s._c_name_))
        want[s.__name__] = str(ctypes.sizeof(s))
        for field, _ in s._fields_:
            lines.append('  std::printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (s.__name__, field, s._c_name_, field))
            want["%s.%s" % (s.__name__, field)] = str(getattr(s, field).offset)
    src, exe = tmp_path / "layout.cpp", tmp_path / "layout"
    src.write_text("\n".join(lines + ["  return 0;", "}"]) + "\n")
    subprocess.check_call([cxx, "-std=c++17", "-I", INCLUDE, "-o", str(exe), str(src)])
    assert dict(line.split() for line in subprocess.check_output([str(exe)]).decode().splitlines()) == want


def test_one_copy_of_the_coder():
    """The object's kernel file holds no coder of its own: the host runs trxsig_fec.hip's launches between its kernels."""
    csrc = os.path.join(ROOT, "openbts-ttsou_amd", "csrc")
    hip = open(os.path.join(csrc, "trxsig_l1pdch.hip")).read()
    host = open(os.path.join(csrc, "trxsig_l1pdch.cpp")).read()
    for k in ("k_l1pdch_stage", "k_l1pdch_mux", "k_l1pdch_commit", "k_l1pdch_demux", "k_l1pdch_fold"):
        assert re.search(r"__global__[^\n]*\b%s\(" % k, hip), k
    assert not re.search(r"kGen|fec_trellis|pd_cindex|kPdUsf|PdPar", hip)
    assert "trx_launch_fec_pdtch_encode(" in host and "trx_launch_fec_pdtch_decode(" in host
    assert not re.search(r"hipStreamSynchronize|hipDeviceSynchronize|hipMemcpy\(", host)
    assert "TRXSIG_K_FEC" in hip and not re.search(r"TRXSIG_K_(?!FEC\b)\w+", hip)


def test_documents_name_the_object():
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    readme = open(os.path.join(ROOT, "README.md")).read()
    integ = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "Packet data channels through L1" in design
    assert all(k in design for k in ("k_l1pdch_stage", "k_l1pdch_mux", "k_l1pdch_commit", "k_l1pdch_demux", "k_l1pdch_fold",
                                     "trxsig_l1pdch_decode", "l1pdch_bench"))
    assert "trxsig_l1pdch" in readme and "l1pdch_bench" in readme
    assert re.search(r"SETSLOT[^\n]*\b1\b[^\n]*PDCH|PDCH[^\n]*SETSLOT[^\n]*\b1\b", integ)
