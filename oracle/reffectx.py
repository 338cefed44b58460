"""ctypes binding for oracle/_ref/libref_fec_tx.so (the REAL reference BitVector / ViterbiR2O4 / Parity code and
GSM::Time under the re-enacted downlink encoder flows, compiled in place by `make -C oracle -f fec_tx.mk ref`) --
TEST INFRASTRUCTURE ONLY.  Used to pin oracle/fec_tx_oracle.c and to generate tests/golden/fec_tx.npz."""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_PATH = os.path.join(_HERE, "_ref", "libref_fec_tx.so")
u8p = np.ctypeslib.ndpointer(dtype=np.uint8, flags="C_CONTIGUOUS")
u32p = np.ctypeslib.ndpointer(dtype=np.uint32, flags="C_CONTIGUOUS")


def available():
    return os.path.exists(_PATH)


class RefFecTx:
    def __init__(self):
        self.lib = L = C.CDLL(_PATH)
        L.reffec_tch_dispatch.argtypes = [C.c_int, u8p, u8p, u8p, u8p, u8p]
        L.reffec_sch_encode.argtypes = [u32p, u8p, C.c_int, u8p, u8p]

    def tch_dispatch(self, kind, payload, tsc26, filler456):
        """A fresh TCHFACCHL1Encoder, dispatch() once per block: kind[n], payload[n, 33] -> bits[n, 4, 148]."""
        kind = np.ascontiguousarray(kind, np.uint8)
        bits = np.zeros((len(kind), 4, 148), np.uint8)
        self.lib.reffec_tch_dispatch(len(kind), kind, np.ascontiguousarray(payload, np.uint8).reshape(len(kind), 33),
                                     np.ascontiguousarray(tsc26, np.uint8), np.ascontiguousarray(filler456, np.uint8), bits)
        return bits

    def sch_encode(self, fn, bsic, xts64):
        fn = np.ascontiguousarray(fn, np.uint32)
        bits = np.zeros((len(fn), 148), np.uint8)
        self.lib.reffec_sch_encode(fn, np.ascontiguousarray(bsic, np.uint8), len(fn), np.ascontiguousarray(xts64, np.uint8), bits)
        return bits
