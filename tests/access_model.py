"""The access burst's two coders as include/trxsig.h states them (trxsig_fec_access_encode_batch / _decode_batch), in numpy --
TEST INFRASTRUCTURE ONLY.  The rate-1/2 coder, the Viterbi decoder, the parity register and the UDP hop are the oracle's
(oracle/fecbind.py: encode, viterbi_decode, parity, wire), called, not rewritten, as tests/pdtch_model.py calls them; what is
stated here is the two formats' bit order, the BSIC colouring, the 11-bit format's six deleted coder outputs and the rule that
chooses between the two hypotheses.

The 8-bit format is the reference's RACH coder (GSM 05.03 4.6).  The 11-bit format (GSM 05.03 5.3.2) is written from memory
(the header says so); tests/test_access_model.py pins what follows from it."""
import functools

import numpy as np

import fecbind

ACCESS_8, ACCESS_11 = 0, 1
ND = (8, 11)                                                # data bits d(0..ND-1), LSB of the word first
NU = (18, 21)                                               # d, six parity bits, four zero tail bits
DELETED = (0, 2, 5, 37, 39, 41)                             # the 11-bit format's coder outputs that are not sent
HEAD = np.array([int(ch) for ch in "00111010" "01001011011111111001100110101010001111000"], np.uint8)   # GSM 05.02 5.2.7
E0, E1 = 49, 85                                             # the 36 coded bits' place in the burst


@functools.lru_cache(maxsize=None)
def keep_mask(deleted=DELETED):
    """True where C(i) of the 11-bit format's 42 coder outputs is sent.  Shared: read, never written."""
    keep = np.ones(42, bool)
    keep[list(deleted)] = False
    keep.flags.writeable = False
    return keep


def coder_input(o, word, fmt, bsic, colour=True, reverse=False):
    """u(0..NU-1): d LSB first, p = ~(bsic ^ parity6(d)) MSB first, 0000.  (colour / reverse: the mutants of the model's test.)"""
    nd = ND[fmt]
    d = np.array([(word >> i) & 1 for i in range(nd)], np.uint8)
    if reverse:
        d = d[::-1].copy()
    p = ~((bsic if colour else 0) ^ o.parity(fecbind.RACH_POLY, 6, d)) & 0x3F
    return np.concatenate([d, np.array([(p >> (5 - i)) & 1 for i in range(6)], np.uint8), np.zeros(4, np.uint8)])


def e36(o, word, fmt, bsic, deleted=DELETED, **mutant):
    c = o.encode(coder_input(o, word, fmt, bsic, **mutant))
    return c if fmt == ACCESS_8 else c[keep_mask(tuple(deleted))]


def fits(word, fmt, bsic):
    return fmt <= 1 and bsic <= 63 and word < (1 << ND[fmt])


def encode(o, ra, fmt, bsic):
    """ra [n] (uint16), fmt [n], bsic [n] -> bits [n, 148]; a row that the encoder refuses is all zero."""
    out = np.zeros((len(ra), 148), np.uint8)
    for i in range(len(ra)):
        if fits(int(ra[i]), int(fmt[i]), int(bsic[i])):
            out[i, :E0] = HEAD
            out[i, E0:E1] = e36(o, int(ra[i]), int(fmt[i]), int(bsic[i]))
    return out


def hypothesis(o, v36, fmt):
    """v36: the 36 values as the decoder sees them -> (ra, tail_ok, bsic) of one format."""
    nd, nu = ND[fmt], NU[fmt]
    v36 = np.asarray(v36, np.float32)
    if fmt == ACCESS_8:
        full = v36
    else:
        full = np.full(42, 0.5, np.float32)                 # a deleted position reads exactly 0.5
        full[keep_mask()] = v36
    u = o.viterbi_decode(np.ascontiguousarray(full), nu)
    sent = int("".join(map(str, u[nd:nd + 6])), 2)
    bsic = (~sent ^ o.parity(fecbind.RACH_POLY, 6, u[:nd])) & 0x3F
    ra = sum(int(u[i]) << i for i in range(nd))
    return ra, int(not u[nd + 6:].any()), bsic


def decode_row(o, v36, fmt, bsic=0):
    """-> (ra, fmt, tail_ok, bsic).  fmt -1: the 11-bit hypothesis only if it holds (tail zero, the parity gives `bsic`) and
    the 8-bit one does not; the 8-bit one otherwise."""
    if fmt >= 0:
        ra, t, b = hypothesis(o, v36, fmt)
        return ra, fmt, t, b
    h8, h11 = hypothesis(o, v36, ACCESS_8), hypothesis(o, v36, ACCESS_11)
    holds = lambda h: bool(h[1]) and h[2] == bsic
    f = ACCESS_11 if holds(h11) and not holds(h8) else ACCESS_8
    ra, t, b = h11 if f else h8
    return ra, f, t, b


def decode(o, soft, index, n, wire=False, fmt=0, bsic=0):
    """soft [n_rows, >= 85]; index [n] (None: rows 0..n-1), an index outside [0, n_rows) = a missing burst, 0.5 throughout.
    -> ra [n] uint16, fmt [n], tail_ok [n], bsic [n] (uint8)"""
    soft = np.asarray(soft, np.float32)
    n_rows = soft.shape[0]
    if index is None:
        index = np.arange(n)
    ra = np.zeros(n, np.uint16)
    f, t, b = (np.zeros(n, np.uint8) for _ in range(3))
    for k in range(n):
        i = int(index[k])
        v = np.full(36, 0.5, np.float32)
        if 0 <= i < n_rows:
            v = o.wire(soft[i, E0:E1]) if wire else soft[i, E0:E1]
        ra[k], f[k], t[k], b[k] = decode_row(o, v, fmt, bsic)
    return ra, f, t, b


@functools.lru_cache(maxsize=None)
def min_weight(deleted=DELETED):
    """The smallest weight among the punctured code's 2^11 - 1 nonzero words.  The code is linear once the constant that the
    inverted, coloured parity adds is taken out: the word of d XOR the word of d = 0 (BSIC 0)."""
    o = fecbind.FecOracle()
    zero = e36(o, 0, ACCESS_11, 0, deleted)
    return min(int((e36(o, w, ACCESS_11, 0, deleted) ^ zero).sum()) for w in range(1, 2048))
