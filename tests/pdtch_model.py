"""The GPRS packet data block coders CS-1..CS-4 (GSM 05.03 5.1) as include/trxsig.h states them, in numpy -- TEST
INFRASTRUCTURE ONLY.  The rate-1/2 coder, the Viterbi decoder, the parity and syndrome registers and the UDP hop are the
oracle's (oracle/fecbind.py: encode, viterbi_decode, parity, syndrome, wire), called, not rewritten; what is stated here is what
the packet channel adds: the payload convention, the 16-bit block check, the USF pre-coding, the puncturing, the stealing-flag
words and their vote.

The constants are written from memory of GSM 05.03 (the header says so); tests/test_pdtch_model.py pins what follows from them.
"""
import functools

import numpy as np

CS1, CS2, CS3, CS4 = 0, 1, 2, 3
K = (184, 271, 315, 431)                                    # information bits d(0..K-1)
OCTETS = (23, 34, 40, 54)
BLOCK_BYTES = 54                                            # TRXSIG_PDTCH_BLOCK_BYTES: the row pitch of a payload array
NU = (228, 294, 338, 456)                                   # bits into the coder (CS-4: the code word itself)
POLY16, POLY_FIRE = 0x11021, 0x10004820009                  # g(D) = D^16 + D^12 + D^5 + 1; XCCH's Fire code

# rows indexed by the string d(0) d(1) d(2); the first character is the first bit sent
USF6 = ("000000", "001011", "010110", "011101", "100101", "101110", "110011", "111000")
USF12 = ("000000000000", "000011011101", "001101110110", "001110101011", "110100001011", "110111010110", "111001111101",
         "111010100000")
# q(0..7): q(2B) is bit 87 and q(2B+1) bit 60 of burst B, the order XCCH's interleaver places its eight flags in
FLAGS = ("11111111", "11001000", "00100001", "00010110")


def _bits(s):
    return np.array([int(ch) for ch in s], np.uint8)


USF6_BITS = np.stack([_bits(s) for s in USF6])
USF12_BITS = np.stack([_bits(s) for s in USF12])
FLAG_BITS = np.stack([_bits(s) for s in FLAGS])
FLAG_POS = tuple((i >> 1, 60 if i & 1 else 87) for i in range(8))   # (burst, bit) of q(i)


@functools.lru_cache(maxsize=None)
def keep_mask(cs):
    """True where a coder output bit C(i) is sent (CS-2: 588 -> 456, CS-3: 676 -> 456).  Shared: read, never written."""
    if cs == CS2:
        keep = np.ones(588, bool)
        for j in range(3, 147):
            if j % 12 != 9:
                keep[3 + 4 * j] = False
    elif cs == CS3:
        keep = np.ones(676, bool)
        for j in range(2, 112):
            keep[3 + 6 * j] = keep[5 + 6 * j] = False
    else:
        raise ValueError("CS-1 and CS-4 are not punctured")
    keep.flags.writeable = False
    return keep


_K456 = np.arange(456)
_J = 2 * ((49 * _K456) % 57) + ((_K456 % 8) // 4)           # GSM 05.03 4.1.4, as the XCCH coder
C_BURST = _K456 % 4
C_POS = np.where(_J < 57, 3 + _J, 88 + (_J - 57))


def payload_bits(block, cs):
    """d(0..K-1): d(k) is bit k mod 8 of octet k / 8, counted from the least significant bit."""
    b = np.asarray(block, np.uint8)
    k = np.arange(K[cs])
    return ((b[k >> 3] >> (k & 7)) & 1).astype(np.uint8)


def payload_octets(d):
    """The 54-octet row of d(0..K-1): spare high bits and the octets past the scheme's size are 0."""
    out = np.zeros(BLOCK_BYTES, np.uint8)
    for k in np.flatnonzero(d):
        out[k >> 3] |= 1 << (k & 7)
    return out


def usf_of(d):
    return int(d[0]) | int(d[1]) << 1 | int(d[2]) << 2


def block_check(o, d):
    """p(0..15): the inverted parity word of Parity(0x11021, 16, K), most significant bit first."""
    pw = ~o.parity(POLY16, 16, d) & 0xFFFF
    return np.array([(pw >> (15 - k)) & 1 for k in range(16)], np.uint8)


def check_ok(o, d, p):
    sent = int("".join(map(str, p)), 2)
    return (o.parity(POLY16, 16, d) ^ sent) == 0xFFFF


def coder_input(o, block, cs):
    """u' (CS-1: u), the bits the rate-1/2 coder takes; for CS-4 the code word."""
    d = payload_bits(block, cs)
    if cs == CS1:
        pw = ~o.parity(POLY_FIRE, 40, d) & ((1 << 40) - 1)
        p = np.array([(pw >> (39 - k)) & 1 for k in range(40)], np.uint8)
        return np.concatenate([d, p, np.zeros(4, np.uint8)])
    row = 4 * int(d[0]) + 2 * int(d[1]) + int(d[2])
    pre = USF12_BITS[row] if cs == CS4 else USF6_BITS[row]
    tail = np.zeros(0 if cs == CS4 else 4, np.uint8)
    return np.concatenate([pre, d[3:], block_check(o, d), tail])


def code_word(o, block, cs):
    u = coder_input(o, block, cs)
    assert len(u) == NU[cs]
    if cs == CS4:
        return u
    c = o.encode(u)
    return c if cs == CS1 else c[keep_mask(cs)]


def encode(o, blocks, cs, tsc, tsc_bits):
    """blocks [n, 54], cs [n], tsc [n] -> bits [n, 4, 148]; a cs above 3 or a tsc above 7 gives four all-zero bursts."""
    n = len(cs)
    out = np.zeros((n, 4, 148), np.uint8)
    for i in range(n):
        if cs[i] > 3 or tsc[i] > 7:
            continue
        out[i, :, 61:87] = tsc_bits[tsc[i]]
        out[i, C_BURST, C_POS] = code_word(o, blocks[i], int(cs[i]))
        for q, (b, pos) in enumerate(FLAG_POS):
            out[i, b, pos] = FLAG_BITS[cs[i]][q]
    return out


def vote(hard8):
    """(scheme, distance): the nearest flag word, ties to the lower scheme."""
    dist = (FLAG_BITS != np.asarray(hard8, np.uint8)).sum(axis=1)
    cs = int(np.argmin(dist))
    return cs, int(dist[cs])


def nearest_row(table, bits):
    return int(np.argmin((table != np.asarray(bits, np.uint8)).sum(axis=1)))   # ties to the first row


def decode_block(o, v4, cs_force=-1):
    """v4 [4, 148] float32: the block's bursts as the decoder sees them (after the UDP hop; a missing burst is all 0.5).
    -> dict(block [54], cs, dist, ok, usf)"""
    v4 = np.asarray(v4, np.float32)
    hard = np.array([v4[b, pos] > np.float32(0.5) for b, pos in FLAG_POS], np.uint8)
    cs, dist = vote(hard)
    if cs_force >= 0:
        cs, dist = cs_force, int((FLAG_BITS[cs_force] != hard).sum())
    c = np.ascontiguousarray(v4[C_BURST, C_POS])
    if cs == CS1:
        u = o.viterbi_decode(c, 228)
        d = u[:184]
        dp = u[:224].copy()
        dp[184:] ^= 1
        ok = o.syndrome(POLY_FIRE, 40, dp) == 0
        return dict(block=payload_octets(d), cs=cs, dist=dist, ok=int(ok), usf=usf_of(d))
    if cs == CS4:
        u = (c > np.float32(0.5)).astype(np.uint8)
        pre, table = 12, USF12_BITS
    else:
        full = np.full(2 * NU[cs], 0.5, np.float32)         # a deleted position reads exactly 0.5
        full[keep_mask(cs)] = c
        u = o.viterbi_decode(full, NU[cs])
        pre, table = 6, USF6_BITS
    row = nearest_row(table, u[:pre])
    d = np.concatenate([np.array([row >> 2 & 1, row >> 1 & 1, row & 1], np.uint8), u[pre:pre + K[cs] - 3]])
    p = u[pre + K[cs] - 3:pre + K[cs] + 13]
    return dict(block=payload_octets(d), cs=cs, dist=dist, ok=int(check_ok(o, d, p)), usf=usf_of(d))


def decode(o, soft, index, n_blocks, wire=False, cs_force=-1):
    """soft [n_rows, >= 148]; index [n_blocks, 4] (None: rows 4k..4k+3), an index outside [0, n_rows) = a missing burst.
    -> blocks [n, 54], cs [n], dist [n], ok [n], usf [n] (uint8)"""
    soft = np.asarray(soft, np.float32)
    n_rows = soft.shape[0]
    if index is None:
        index = np.arange(4 * n_blocks).reshape(n_blocks, 4)
    blocks = np.zeros((n_blocks, BLOCK_BYTES), np.uint8)
    cs, dist, ok, usf = (np.zeros(n_blocks, np.uint8) for _ in range(4))
    for k in range(n_blocks):
        v4 = np.full((4, 148), 0.5, np.float32)
        for t in range(4):
            i = int(index[k][t])
            if 0 <= i < n_rows:
                v4[t] = o.wire(soft[i, :148]) if wire else soft[i, :148]
        r = decode_block(o, v4, cs_force)
        blocks[k], cs[k], dist[k], ok[k], usf[k] = r["block"], r["cs"], r["dist"], r["ok"], r["usf"]
    return blocks, cs, dist, ok, usf


def random_blocks(rng, cs):
    """Random payloads [n, 54] for the schemes cs [n] that the decoder returns unchanged: spare bits and octets zero."""
    cs = np.asarray(cs)
    blocks = rng.integers(0, 256, (len(cs), BLOCK_BYTES)).astype(np.uint8)
    for i, s in enumerate(cs):
        if s <= 3:
            blocks[i] = payload_octets(payload_bits(blocks[i], int(s)))
    return blocks


def pdch_map(fn):
    """(block, burst) of frame fn in the 52-multiframe: B0..B11 of four frames each; 12 and 38 (PTCCH), 25 and 51 (idle)
    give (-1, -1)."""
    r = fn % 52
    if r % 13 == 12:
        return -1, -1
    r -= r // 13
    return r >> 2, r & 3
