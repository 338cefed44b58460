"""trxsig_trxgroup_add_l1tx in the C-ABI: exported by libtrxsig.so, declared in include/trxsig_l1tx.h, bound as TrxGroup.add_l1tx,
its kernel known to the profiler, and refused with TRXSIG_EINVAL for NULL objects before anything touches a device.  No GPU needed."""
import ctypes
import os
import re

import _pkg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_add_l1tx_in_the_abi():
    so = os.path.join(ROOT, "openbts-ttsou_amd", "libtrxsig.so")
    lib = ctypes.CDLL(so)
    assert hasattr(lib, "trxsig_trxgroup_add_l1tx")
    h = open(os.path.join(ROOT, "include", "trxsig_l1tx.h")).read()
    assert re.search(r"int trxsig_trxgroup_add_l1tx\(trxsig_trxgroup \*g, trxsig_l1tx \*l1\);", h)
    lib.trxsig_trxgroup_add_l1tx.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
    assert lib.trxsig_trxgroup_add_l1tx(None, None) == -1   # TRXSIG_EINVAL
    # the arrival kernel has a profiler id behind the earlier ones, and TRXSIG_K_COUNT (ABI 2) stays where it was
    t = open(os.path.join(ROOT, "include", "trxsig.h")).read()
    assert "TRXSIG_K_GROUP_TX_GRID = 27" in t and "TRXSIG_K_COUNT = 15" in t
    lib.trxsig_kernel_name.restype = ctypes.c_char_p
    assert lib.trxsig_kernel_count() == 28
    assert lib.trxsig_kernel_name(27) == b"k_group_tx_arrive_grid"


def test_python_binding():
    m = _pkg.load()
    assert callable(getattr(m.TrxGroup, "add_l1tx", None))
