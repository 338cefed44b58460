"""The structures of include/trxsig_l1pdch.h as ctypes sees them.  They live beside _abi.py, whose own set of structures
tests/test_binding_abi.py pins by name; tests/test_l1pdch_abi.py holds these against the C compiler's layout the same way.  The
entry points that take them are declared in _abi.SIGNATURES like every other, with plain pointers."""
import ctypes as C

from ._abi import _fields


class L1PdchIn(C.Structure):
    _c_name_ = "trxsig_l1pdch_in"
    _fields_ = _fields((), ("d_pdtch_kind", "d_pdtch_cs", "d_pdtch_payload", "d_ptcch_kind", "d_ptcch_payload"))


class L1PdchOut(C.Structure):
    _c_name_ = "trxsig_l1pdch_out"
    _fields_ = _fields(("n_arfcn", "n_frames"), ("d_bits", "d_what"))


class L1PdchDec(C.Structure):
    _c_name_ = "trxsig_l1pdch_dec"
    _fields_ = _fields(("n_pdtch", "n_ptcch", "nb_pdtch", "nb_ptcch"),
                       ("d_pdtch_payload", "d_pdtch_cs", "d_pdtch_cs_dist", "d_pdtch_ok", "d_pdtch_usf", "d_pdtch_nb",
                        "d_pdtch_granted", "d_pdtch_fn", "d_ptcch_payload", "d_ptcch_cs", "d_ptcch_cs_dist", "d_ptcch_ok",
                        "d_ptcch_usf", "d_ptcch_nb", "d_ptcch_granted", "d_ptcch_fn", "d_pdtch_rssi", "d_pdtch_timing",
                        "d_ptcch_rssi", "d_ptcch_timing"))
