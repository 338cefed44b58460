"""ctypes binding for oracle/libfec_tx_oracle.so (the CPU restatement of the downlink L1 encoders of traffic and sync
channels, built by `make -C oracle -f fec_tx.mk oracle`) -- TEST INFRASTRUCTURE ONLY."""
import ctypes as C
import os

import numpy as np

import fecbind

_HERE = os.path.dirname(os.path.abspath(__file__))
u8p = np.ctypeslib.ndpointer(dtype=np.uint8, flags="C_CONTIGUOUS")
u32p = np.ctypeslib.ndpointer(dtype=np.uint32, flags="C_CONTIGUOUS")
# GSM 05.02 5.2.3 training sequences and the 5.2.5 SCH extended training sequence (public constants of the standard)
TSC = ["00100101110000100010010111", "00101101110111100010110111", "01000011101110100100001110", "01000111101101000100011110",
       "00011010111001000001101011", "01001110101100000100111010", "10100111110110001010011111", "11101111000100101110111100"]
XTS = "1011100101100010000001000000111100101101010001010111011000011011"
TSC_BITS = np.array([[int(ch) for ch in t] for t in TSC], np.uint8)
XTS_BITS = np.array([int(ch) for ch in XTS], np.uint8)


class FecTxOracle(fecbind.FecOracle):
    """The encoders, beside fecbind.FecOracle's coder / parity / decoder helpers."""

    def __init__(self):
        super().__init__()
        self.txlib = L = C.CDLL(os.environ.get("FEC_TX_ORACLE_LIB", os.path.join(_HERE, "libfec_tx_oracle.so")))
        L.fo_tch_encode_stream.argtypes = [C.c_int, C.c_int, u8p, u8p, u8p, u8p, u8p, u8p, u8p, C.c_int]
        L.fo_sch_encode.argtypes = [u32p, u8p, C.c_int, u8p, u8p]

    def tch_encode_stream(self, kind, payload, tsc, filler, state=None, nthreads=8):
        """kind[S, n], payload[S, n, 33], tsc[S], filler[456], state[S, 32] (None: fresh encoders) ->
        (bits[S, n, 4, 148], new state[S, 32]); the literal TCHFACCHL1Encoder::dispatch."""
        kind = np.ascontiguousarray(kind, np.uint8)
        S, n = kind.shape
        payload = np.ascontiguousarray(payload, np.uint8).reshape(S, n, 33)
        st = np.zeros((S, 32), np.uint8) if state is None else np.array(state, np.uint8).reshape(S, 32)
        bits = np.zeros((S, n, 4, 148), np.uint8)
        self.txlib.fo_tch_encode_stream(S, n, kind, payload, np.ascontiguousarray(tsc, np.uint8), TSC_BITS,
                                      np.ascontiguousarray(filler, np.uint8), st, bits, nthreads)
        return bits, st

    def sch_encode(self, fn, bsic):
        fn = np.ascontiguousarray(fn, np.uint32)
        bits = np.zeros((len(fn), 148), np.uint8)
        self.txlib.fo_sch_encode(fn, np.ascontiguousarray(bsic, np.uint8), len(fn), XTS_BITS, bits)
        return bits
