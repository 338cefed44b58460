"""The Python binding against the C headers (no GPU; needs the built libraries, like the other test_*_abi.py).

The binding declares every entry point of include/trxsig*.h once, in _abi.SIGNATURES, and every structure it passes once, in
_abi.py.  Here the table is held against the headers' prototypes (names, parameter count, parameter classes, return class),
every entry is resolved in both libraries, the structures are held against the layout the C compiler gives them, and the
package is searched for a second place where a signature or the device-to-host round trip is written."""
import copy
import ctypes as C
import glob
import os
import re
import shutil
import subprocess

import pytest

import _pkg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
PKG_DIR = os.path.join(ROOT, "openbts-ttsou_amd")

_SCALARS = {"int": "i32", "int32_t": "i32", "unsigned": "u32", "unsigned int": "u32", "uint32_t": "u32", "int64_t": "i64",
            "uint64_t": "u64", "float": "f32", "double": "f64", "size_t": "size", "trxsig_c32": "C32", "void": None}


def _c_class(decl, is_return=False):
    """One parameter declaration (or a return type) of a prototype -> its class."""
    if "*" in decl or "[" in decl:
        return "ptr"
    words = [w for w in re.findall(r"\w+", decl) if w not in ("const", "struct")]
    if not is_return and len(words) > 1 and " ".join(words[:-1]) in _SCALARS:
        words = words[:-1]                                  # the parameter's name
    return _SCALARS[" ".join(words)]                        # (a type this parser does not know is a KeyError: extend it, knowingly)


def header_prototypes():
    """{name: (return class, [parameter classes])} of every trxsig_* prototype of include/trxsig*.h (not the C++ facade)."""
    protos = {}
    for path in sorted(glob.glob(os.path.join(INCLUDE, "trxsig*.h"))):
        text = open(path).read()
        text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
        text = re.sub(r"//[^\n]*", " ", text)
        text = re.sub(r"^\s*#.*$", " ", text, flags=re.M)
        for m in re.finditer(r"([\w\s\*]+?)\b(trxsig_\w+)\s*\(([^()]*)\)\s*;", text):
            ret, name, params = m.groups()
            if "typedef" in ret:
                continue
            params = [p for p in params.split(",") if p.strip()]
            if [p.strip() for p in params] == ["void"]:
                params = []
            assert name not in protos, "%s is declared twice" % name
            protos[name] = (_c_class(ret, True), [_c_class(p) for p in params])
    return protos


_CTYPES = {C.c_int: "i32", C.c_uint: "u32", C.c_int64: "i64", C.c_uint64: "u64", C.c_float: "f32", C.c_double: "f64"}


def _ctypes_class(t, abi):
    """A restype or argtype of the table -> its class.  ctypes has one type for size_t and uint64_t where both are 64 bits wide,
    so a table entry of either reads u64 (compare() holds the header's `size` against that)."""
    if t is None:
        return None
    if t is abi.C32:
        return "C32"
    if t in (C.c_void_p, C.c_char_p) or hasattr(t, "contents"):   # (contents: a POINTER(...) type)
        return "ptr"
    return _CTYPES[t]


def compare(protos, table, abi):
    """Every disagreement between the headers' prototypes and a signature table, as a list of strings."""
    bad = ["%s: declared in a header, not in the table" % n for n in sorted(set(protos) - set(table))]
    bad += ["%s: in the table, declared in no header" % n for n in sorted(set(table) - set(protos))]
    for name in sorted(set(protos) & set(table)):
        ret, params = protos[name]
        restype, argtypes = table[name]
        size = _CTYPES[C.c_size_t]
        want, want_ret = [size if p == "size" else p for p in params], size if ret == "size" else ret
        if len(argtypes) != len(want):
            bad.append("%s: %d parameters in the header, %d in the table" % (name, len(want), len(argtypes)))
        else:
            got = [_ctypes_class(t, abi) for t in argtypes]
            bad += ["%s: parameter %d is %s in the header, %s in the table" % (name, i, w, g)
                    for i, (w, g) in enumerate(zip(want, got)) if w != g]
        if _ctypes_class(restype, abi) != want_ret:
            bad.append("%s: returns %s in the header, %s in the table" % (name, want_ret, _ctypes_class(restype, abi)))
    return bad


@pytest.fixture(scope="module")
def abi():
    _pkg.load()
    from openbts_ttsou_amd import _abi
    return _abi


def test_table_agrees_with_the_headers(abi):
    protos = header_prototypes()
    assert len(protos) >= 232                               # what the headers held when this test was written
    assert "trxsig_create" in protos and not any(n.startswith("sigProc") for n in protos)
    assert compare(protos, abi.SIGNATURES, abi) == []


def test_the_comparer_can_fail(abi):
    """One i64 turned into i32, one parameter dropped, one restype taken from a pointer-returning function, one entry missing
    and one too many: each is reported, and nothing else is."""
    protos = header_prototypes()
    t = copy.deepcopy(dict(abi.SIGNATURES))
    r, a = t["trxsig_resample_batch"]
    assert a[3] is C.c_int64
    t["trxsig_resample_batch"] = (r, a[:3] + [C.c_int] + a[4:])
    r, a = t["trxsig_l1hop_groups"]
    t["trxsig_l1hop_groups"] = (r, a[:-1])
    r, a = t["trxsig_tables_device"]
    assert r is C.c_void_p
    t["trxsig_tables_device"] = (C.c_int, a)                # what ctypes assumes where no restype is set
    del t["trxsig_air_cells"]
    t["trxsig_no_such_call"] = (C.c_int, [])
    bad = compare(protos, t, abi)
    assert len(bad) == 5, bad
    text = "\n".join(bad)
    assert "trxsig_resample_batch: parameter 3 is i64 in the header, i32 in the table" in text
    assert "trxsig_l1hop_groups: 1 parameters in the header, 0 in the table" in text
    assert "trxsig_tables_device: returns ptr in the header, i32 in the table" in text
    assert "trxsig_air_cells: declared in a header, not in the table" in text
    assert "trxsig_no_such_call: in the table, declared in no header" in text


def test_every_entry_resolves_in_both_libraries(abi):
    pkg = _pkg.load()
    for path in (pkg.LIB_PATH, pkg.TUNE_LIB_PATH):
        lib = C.CDLL(path)                                  # a handle of its own: nothing is typed on the package's
        missing = [n for n in abi.SIGNATURES if not hasattr(lib, n)]
        assert not missing, (path, missing)
    # and what bind() says of a library that lacks one
    with pytest.raises(pkg.TrxSigError, match=r"libc.*trxsig_abi_version"):
        abi.bind(C.CDLL("libc.so.6"), "libc.so.6")
    # what _load returns is typed throughout: a 64-bit address survives a call that no constructor has run before
    for L in (pkg._load(pkg.LIB_PATH), pkg._load(pkg.TUNE_LIB_PATH)):
        for name, (restype, argtypes) in abi.SIGNATURES.items():
            f = getattr(L, name)
            assert f.restype is restype and list(f.argtypes) == list(argtypes), name


def _structures(abi):
    return [v for v in vars(abi).values() if isinstance(v, type) and issubclass(v, C.Structure) and v is not C.Structure]


def test_structures_have_the_compilers_layout(abi, tmp_path):
    structs = _structures(abi)
    assert {s.__name__ for s in structs} == {"C32", "TrxGroupResult", "L1RxOut", "L1TxIn", "L1TxOut", "L1MsIn", "L1MsOut", "L1MsAir",
                                              "L1MsRxOut", "L1AcqOut", "AirCellParams", "AirStreamParams", "L1TrkView", "L1TrkMeas"}
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler to lay the structures out with")
    headers = sorted(os.path.basename(p) for p in glob.glob(os.path.join(INCLUDE, "trxsig*.h")))
    lines = ["#include <cstddef>", "#include <cstdio>"] + ['#include "%s"' % h for h in headers] + ["int main() {"]
    for s in structs:
        lines.append('  std::printf("%s %%zu\\n", sizeof(%s));' % (s.__name__, s._c_name_))
        for field, _ in s._fields_:
            lines.append('  std::printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (s.__name__, field, s._c_name_, field))
    lines += ["  return 0;", "}"]
    src, exe = tmp_path / "layout.cpp", tmp_path / "layout"
    src.write_text("\n".join(lines) + "\n")
    subprocess.check_call([cxx, "-std=c++17", "-I", INCLUDE, "-o", str(exe), str(src)])
    got = dict(line.split() for line in subprocess.check_output([str(exe)]).decode().splitlines())
    want = {}
    for s in structs:
        want[s.__name__] = str(C.sizeof(s))
        for field, _ in s._fields_:
            want["%s.%s" % (s.__name__, field)] = str(getattr(s, field).offset)
    assert got == want


PUBLIC = {
    "TrxHost": "close control expected_corr_type pull_radio_vector encode_rx_datagram decode_tx_datagram add_radio_vector "
               "push_radio_vector energy_threshold filler_modulus queue_size create_lpf",
    "TrxGroup": "close control expected_corr_type pull pull_bursts pull_rxfe add_bursts tx_staging add_staged add_l1tx push push_txbe "
                "tx_queue_size pull_host collect set_pipelined set_beside_rows set_split_rows sync energy_threshold",
    "L1Rx": "destroy channels channel open close decode state collect",
    "L1Tx": "destroy channels channel open close set_si grid encode state collect datagrams",
    "L1Ms": "destroy channels channel open close set_phy grid encode radiate follow state collect",
    "L1MsRx": "destroy channels channel open close decode state collect",
    "L1Acq": "destroy sequence search detect_sch collect",
    "Air": "destroy cells stream",
    "L1Trk": "destroy seed set slice update state collect",
    "L1Ciph": "destroy channels channel set state bits soft collect",
    "L1Hop": "destroy groups members map bits cells result",
    "RxFrontEnd": "set_shared_filter push_wideband close push_chunk pop_raw pop_bursts push_detect_demod pending",
    "TxBackEnd": "close push_bursts pop_samples pending",
}


def test_one_place():
    sources = {p: open(p).read() for p in glob.glob(os.path.join(PKG_DIR, "*.py"))}
    assert os.path.join(PKG_DIR, "_abi.py") in sources and len(sources) >= 5
    for path, text in sources.items():
        if os.path.basename(path) != "_abi.py":
            assert not re.search(r"\.(argtypes|restype)\s*=[^=]", text), path
        assert "def get(" not in text, path
    assert [os.path.basename(p) for p, text in sources.items() if re.search(r"^\s*def _to_host\(", text, re.M)] == ["__init__.py"]
    assert sum(len(re.findall(r"^\s*def _to_host\(", text, re.M)) for text in sources.values()) == 1
    pkg = _pkg.load()
    from openbts_ttsou_amd import frontend
    for cls, names in PUBLIC.items():
        c = getattr(pkg, cls, None) or getattr(frontend, cls)
        for name in names.split():
            member = getattr(c, name, None)
            assert callable(member) or isinstance(member, property), (cls, name)
    assert isinstance(pkg.TrxHost.energy_threshold, property)
    assert not hasattr(pkg.L1Ciph, "open") and not hasattr(pkg.L1Hop, "channels")   # (and nothing that the C API lacks)
    assert frontend._DevView is pkg._DevView
    for s in ("C32", "TrxGroupResult", "L1RxOut", "L1TxIn", "L1TxOut", "L1MsIn", "L1MsOut", "L1MsAir", "L1MsRxOut", "L1AcqOut",
              "AirCellParams", "AirStreamParams", "L1TrkView", "L1TrkMeas", "TrxSigError"):
        assert hasattr(pkg, s), s
