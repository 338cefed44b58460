"""Packet access through L1 in the C-ABI: the entry points exported by libtrxsig.so (and the tuning build) and declared in
include/trxsig_l1pacc.h, the enum values, the refusals that need no device, the header's statement and its record size, the
header as C99, the binding and its structures against the C compiler's layout, no coder and no synchronise of the object's own,
the documents.  No GPU needed (the refusals that need a live context are the last test of tests/test_gpu_l1pacc.py)."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest

import _pkg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
HEADER = os.path.join(INCLUDE, "trxsig_l1pacc.h")
ENTRY = ("create", "destroy", "channels", "channel", "grid", "state", "encode", "detect", "ta_message", "ta_read")
vp, i32 = ctypes.c_void_p, ctypes.c_int


def test_l1pacc_in_the_abi():
    h = open(HEADER).read()
    for so in ("libtrxsig.so", "libtrxsig_tune.so"):
        lib = ctypes.CDLL(os.path.join(ROOT, "openbts-ttsou_amd", so))
        for s in ENTRY:
            assert hasattr(lib, "trxsig_l1pacc_" + s), (so, s)
            assert re.search(r"\b(int|void)\s+trxsig_l1pacc_%s\(" % s, h), s
        assert lib.trxsig_kernel_count() == 28 and lib.trxsig_abi_version() == 2      # booked under TRXSIG_K_FEC: no new row
        lib.trxsig_l1pacc_create.argtypes = [ctypes.POINTER(vp), vp, i32, vp, i32]
        out = vp(7)
        comb = (ctypes.c_uint8 * 8)(0, 13, 1, 7, 0, 0, 0, 13)
        assert lib.trxsig_l1pacc_create(ctypes.byref(out), None, 1, comb, 5) == -1   # TRXSIG_EINVAL: no context
        assert lib.trxsig_l1pacc_create(None, None, 1, comb, 5) == -1
        assert lib.trxsig_l1pacc_channels(None) == -1 and lib.trxsig_l1pacc_channel(None, 0, None, None) == -1
        assert lib.trxsig_l1pacc_grid(None, 0, 4, None) == -1 and lib.trxsig_l1pacc_state(None, None) == -1
        assert lib.trxsig_l1pacc_encode(None, 0, 4, None, None, None, None) == -1
        lib.trxsig_l1pacc_detect.argtypes = [vp, vp, ctypes.c_int64, ctypes.c_int64, i32, i32, vp, i32, i32, ctypes.c_float, ctypes.c_float, i32, vp]
        assert lib.trxsig_l1pacc_detect(None, None, 1280, 640, 0, 4, None, -1, 0, 5.0, -1.0, 1, None) == -1
        assert lib.trxsig_l1pacc_ta_message(None, None, None, 1) == -1 and lib.trxsig_l1pacc_ta_read(None, None, None) == -1
        lib.trxsig_l1pacc_destroy.argtypes = [vp]
        lib.trxsig_l1pacc_destroy(None)


def enum_values(text):
    out = {}
    for body in re.findall(r"enum\s*\{([^}]*)\}", re.sub(r"/\*.*?\*/", " ", text, flags=re.S)):
        for name, val in re.findall(r"(\w+)\s*=\s*(-?\d+)", body):
            out[name] = int(val)
    return out


def test_enum_values_and_record_size():
    text = open(HEADER).read()
    e = enum_values(text)
    assert e["TRXSIG_L1TX_PACC"] == 9
    assert (e["TRXSIG_L1PACC_NONE"], e["TRXSIG_L1PACC_PTCCH"], e["TRXSIG_L1PACC_PRACH"]) == (0, 1, 2)
    taken = {k: v for name in ("trxsig_l1tx.h", "trxsig_l1pdch.h") for k, v in enum_values(open(os.path.join(INCLUDE, name)).read()).items()
             if k.startswith("TRXSIG_L1TX_")}
    assert len(taken) == 9 and e["TRXSIG_L1TX_PACC"] not in taken.values()
    assert re.search(r"#define TRXSIG_L1PACC_STATE_BYTES 144\b", text)
    dev = open(os.path.join(ROOT, "openbts-ttsou_amd", "csrc", "trxsig_l1pacc_dev.h")).read()
    assert 'static_assert(sizeof(TrxL1paccChan) == 144, "TRXSIG_L1PACC_STATE_BYTES")' in dev


def test_header_states_the_object():
    flat = " ".join(open(HEADER).read().split())
    for text in ("NOT CHECKED AGAINST THE STANDARD", "FROM MEMORY of GSM 05.02 / 03.64", "FN mod 416 = 12 + 26 n", "FN mod 52 = 12 or 38",
                 "USF = FREE", "THE OCTET LAYOUT IS FROM MEMORY", "0x7F", "0x2B", "t < 0 ? 0 : min(63, (int)(t + 0.5F))", "toa / (float)sps",
                 "timing advance 0", "HOST array", "fit int32", "trxsig_detect_demod_rach_batch", "trxsig_mlse_rach_batch",
                 "k_fec_access_decode", "one fold kernel", "equals any split", "nothing synchronises or reads back", "TRXSIG_K_FEC",
                 "the group's classifier", "device-resident PRACH marks", "USF scheduling and RLC/MAC", "EGPRS training sequences",
                 "two antennas", "PACKET CHANNEL REQUEST"):
        assert text in flat, text
    pd = " ".join(open(os.path.join(INCLUDE, "trxsig_l1pdch.h")).read().split())
    assert "PTCCH/U and PRACH" in pd and "timing-advance" in pd and "RLC/MAC" in pd        # that header loses none of its own


def test_header_compiles_as_c(tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    if cc is None:
        pytest.fail("no C compiler to check the header with")
    src = tmp_path / "pa.c"
    src.write_text('#include "trxsig_l1pacc.h"\nint use(trxsig_l1pacc *p, trxsig_l1pacc_in *i, trxsig_l1pacc_out *o, trxsig_l1pacc_det *d,\n'
                   "        const trxsig_l1pdch_dec *r, const trxsig_c32 *x, uint8_t *b) {\n"
                   "  return trxsig_l1pacc_encode(p, 0, 4, i, 0, 0, o) + TRXSIG_L1TX_PACC + TRXSIG_L1PACC_STATE_BYTES + TRXSIG_L1PACC_PRACH +\n"
                   "         trxsig_l1pacc_detect(p, x, 1280, 640, 0, 4, b, -1, TRXSIG_RACHLEG_MLSE, 5.0f, -1.0f, 1, d) +\n"
                   "         trxsig_l1pacc_ta_message(p, b, b, 1) + trxsig_l1pacc_ta_read(p, r, b) + i->fmt;\n}\n")
    r = subprocess.run([cc, "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", INCLUDE, "-c", str(src), "-o", str(tmp_path / "pa.o")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_python_binding_and_structures(tmp_path):
    m = _pkg.load()
    from openbts_ttsou_amd import _abi, _abi_l1pacc
    for s in ENTRY:
        assert "trxsig_l1pacc_" + s in _abi.SIGNATURES
    for name in ("destroy", "channels", "channel", "grid", "state", "encode", "detect", "ta_message", "ta_read", "collect", "states"):
        assert callable(getattr(m.L1Pacc, name)), name
    assert issubclass(m.L1Pacc, m._Object) and callable(m.TrxSig.access_encode) and callable(m.TrxSig.access_decode)
    assert (m.L1TX_PACC, m.L1PACC_NONE, m.L1PACC_PTCCH, m.L1PACC_PRACH, m.L1PACC_STATE_BYTES) == (9, 0, 1, 2, 144)
    structs = [_abi_l1pacc.L1PaccIn, _abi_l1pacc.L1PaccOut, _abi_l1pacc.L1PaccDet]
    assert all(getattr(m, s.__name__) is s for s in structs)
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler to lay the structures out with")
    lines = ["#include <cstddef>", "#include <cstdio>", '#include "trxsig_l1pacc.h"', "int main() {"]
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
    # no signature typed outside _abi.py
    for name in ("_abi_l1pacc.py", "__init__.py"):
        assert not re.search(r"\.(argtypes|restype)\s*=[^=]", open(os.path.join(ROOT, "openbts-ttsou_amd", name)).read()), name


def test_no_coder_and_no_synchronise_of_its_own():
    """The object's kernel file holds no coder, trellis or detector: the host runs trxsig_fec.hip's launches and the C ABI's
    detector calls between its kernels, and waits for nothing."""
    csrc = os.path.join(ROOT, "openbts-ttsou_amd", "csrc")
    hip = open(os.path.join(csrc, "trxsig_l1pacc.hip")).read()
    host = open(os.path.join(csrc, "trxsig_l1pacc_host.cpp")).read()
    for k in ("k_l1pacc_stage", "k_l1pacc_mux", "k_l1pacc_fold", "k_l1pacc_message", "k_l1pacc_read"):
        assert re.search(r"__global__[^\n]*\b%s\(" % k, hip), k
    assert len(re.findall(r"__global__", hip)) == 5
    assert not re.search(r"kGen|fec_trellis|access_coder|access_e36|rach_e36|access_cindex|trxsig_fec_enc\.h", hip)
    assert "trx_launch_fec_access_encode(" in host and "trx_launch_fec_access_decode(" in host
    assert "trxsig_detect_demod_rach_batch(" in host and "trxsig_mlse_rach_batch(" in host
    assert not re.search(r"hipStreamSynchronize|hipDeviceSynchronize|hipMemcpy\(|hipMemcpyDtoH|hipMemcpyAsync", host)
    assert "TRXSIG_K_FEC" in hip and not re.search(r"TRXSIG_K_(?!FEC\b)\w+", hip)
    mk = open(os.path.join(csrc, "Makefile")).read()
    assert re.search(r"^KERNELS := .*\btrxsig_l1pacc\b", mk, re.M) and re.search(r"^HOSTSRC := .*\btrxsig_l1pacc_host\b", mk, re.M)


def test_documents_name_the_object():
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    readme = open(os.path.join(ROOT, "README.md")).read()
    integ = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "Packet access on the PDCH" in design
    assert all(k in design for k in ("trxsig_l1pacc", "k_l1pacc_stage", "k_l1pacc_mux", "k_l1pacc_fold", "k_l1pacc_message", "k_l1pacc_read",
                                     "trxsig_l1pacc_detect", "l1pacc_bench"))
    assert "trxsig_l1pacc" in readme and "l1pacc_bench" in readme and "from memory" in readme
    assert "trxsig_l1pacc_detect" in integ and "trxsig_trxgroup_pull" in integ
