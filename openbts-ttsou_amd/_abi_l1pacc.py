"""The structures of include/trxsig_l1pacc.h as ctypes sees them.  They live beside _abi.py and _abi_l1pdch.py, whose own sets of
structures are pinned by name; tests/test_l1pacc_abi.py holds these against the C compiler's layout the same way.  The entry
points that take them are declared in _abi.SIGNATURES like every other, with plain pointers."""
import ctypes as C

from ._abi import _fields


class L1PaccIn(C.Structure):
    _c_name_ = "trxsig_l1pacc_in"
    _fields_ = _fields(("fmt",), ("d_ptcch_kind", "d_ptcch_ra", "d_prach_kind", "d_prach_ra"))


class L1PaccOut(C.Structure):
    _c_name_ = "trxsig_l1pacc_out"
    _fields_ = _fields(("n_arfcn", "n_frames"), ("d_bits", "d_what"))


class L1PaccDet(C.Structure):
    _c_name_ = "trxsig_l1pacc_det"
    _fields_ = _fields(("n_pdch", "n_frames"), ("d_kind", "d_tai", "d_det", "d_fmt", "d_ok", "d_ra", "d_amp", "d_toa", "d_avgpwr", "d_ta"))
