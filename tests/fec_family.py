"""An adversarial family of soft words for the FEC decoders (fec_trellis in csrc/trxsig_fec.hip, behind k_fec_viterbi and
k_fec_rx_stream), and a numpy float32 trellis with switchable mutants that proves -- on the CPU alone -- that the family
sees the three decisions the kernel's contract rests on.  No GPU and no native library here.

The decisions (SoftVector::decode with ViterbiR2O4::step, CommonLibs/BitVector.cpp:336-402 and 449-524, "bv:"):
  prune      a survivor keeps candidate A only when cost A < cost B, so a tie takes B, the 1-prefix one (bv:371-379)
  first min  the output bit comes from the FIRST survivor that holds the minimum cost (bv:382-393); with all sixteen costs
             NaN no survivor is ever skipped (`thisCost >= minCost` is false) and the scan ends on survivor 15
  add order  cost + (second-bit cost + first-bit cost), one rounded float32 add each (bv:365)
Uniform random soft values never tie after the first few steps, so they cannot tell a decoder that gets any of the three
wrong from one that gets them right.  The members below tie at a third of their steps or more.

decode(soft, nout, rule) is the trellis, vectorised over the words of a batch:
  "ref"      the reference
  "le"       mutant: A wins a tie
  "lastmin"  mutant: the last minimum
  "assoc"    mutant: (cost + second) + first
  "rowleak"  the kernel before its NaN fix: the first survivor EQUAL to fmin of the sixteen, else (none is: all NaN)
             survivor 0 of the next word of the batch (0 after the last word)

Members (family(); each a Member: soft [B, n] float32, nout = n / 2, the entry points that take words of that length;
B = 64 unless noted):
  alphabet   at every nout of LENGTHS (18 too, for RACH): garbage from {0, .25, .5, .75, 1}; code words at .25 / .75 with
             20 % of the positions flipped; hard 0 / 1 code words with 12 % flipped.  LENGTHS puts steps = nout + 24 on and
             around the kernel's 64-step table refill (39, 40, 41; 104, 105), at the channels' own lengths (39, 189, 228) and
             at the limit of the 32-bits-per-lane output word (512).
  edges      every position from EDGES: 0.5 and its neighbours, 0.01 / 0.99 and the neighbours where the `< 0.01F` clamps
             (bv:484-485) switch, 0, 1, -0.0, a subnormal, values outside [0, 1] up to +-Inf.  All give finite costs.
  nan        one NaN per word, either sign, at position 0, an odd position, the last position, the positions of steps 23 and
             24 (the deferral boundary) and 63 and 64 (a table refill), a late one inside class 1 of a TCH block -- on alphabet
             garbage (nan_garbage) and on a clean 0.1 / 0.9 code word (nan_clean: `sent` holds the bits, `nan_pos` the
             positions), whose output before step(NaN) - 24 must still be the sent bits.
  isolation  batches in which a NaN word sits in row 0, 1, 2, 3 of a four-row wave in turn, or is the last live word of a
             ragged batch (the next row is dead).  `soft` and `alt` hold the same NaN words with different neighbours; `groups`
             lists the batches as slices; `nan_rows` marks the NaN words.  A NaN word's output must be the same in both.
  wire       for the UDP hop's quantisation, values in [0, 1] only: both float32 neighbours of every tie (2k + 1) / 510 of
             round(x * 255.0), k = 0 .. 254 (k = 127 is 0.5, the one representable tie: 0.5 +- 1 ulp and 0.5 itself), and 0, 1.

Helper module, no tests here: tests/test_fec_family.py proves the family, tests/test_gpu_fec_family.py grades the kernels."""
import functools

import numpy as np

F32 = np.float32
DEFERRAL = 24
LENGTHS = (1, 2, 39, 40, 41, 104, 105, 189, 228, 512)          # nout
CHANNEL_NOUT = {18: ("viterbi", "rach"), 39: ("viterbi", "sch"), 228: ("viterbi", "xcch", "tch", "stream")}
B_WORDS = 64

_inf = F32(np.inf)
EDGES = np.array([0.5, np.nextafter(F32(0.5), F32(0)), np.nextafter(F32(0.5), F32(1)),
                  0.01, np.nextafter(F32(0.01), F32(0)), 0.99, np.nextafter(F32(0.99), F32(1)),
                  0.0, 1.0, -0.0, 1e-42, -3.5, 7.0, 1e30, _inf, -_inf], F32)
ALPHABET = np.array([0.0, 0.25, 0.5, 0.75, 1.0], F32)
_k = np.arange(255, dtype=np.float64)
_tie = ((2 * _k + 1) / 510.0).astype(F32)                      # the nearest float32: one neighbour; the other lies across the tie
_lo = np.where(_tie.astype(np.float64) * 510.0 < 2 * _k + 1, _tie, np.nextafter(_tie, F32(0)))
WIRE_VALUES = np.concatenate([_lo, np.nextafter(_lo, F32(1)), F32([0.0, 1.0, 0.5])]).astype(F32)
WIRE_VALUES[127], WIRE_VALUES[255 + 127] = np.nextafter(F32(0.5), F32(0)), np.nextafter(F32(0.5), F32(1))   # 127.5 / 255 IS 0.5


def _parity5(x):
    x = x & 31
    x = x ^ (x >> 1) ^ (x >> 2) ^ (x >> 3) ^ (x >> 4)
    return x & 1


# generator table (bv:306-330): the coder's output for the 5-bit input history, 0x19 in bit 1 and 0x1b in bit 0
GEN = ((_parity5(np.arange(32) & 0x19) << 1) | _parity5(np.arange(32) & 0x1b)).astype(np.uint32)


def encode(bits):
    """BitVector::encode (bv:217-239) on [B, k] bits -> [B, 2k]."""
    bits = np.asarray(bits, np.uint32)
    out = np.zeros((bits.shape[0], 2 * bits.shape[1]), np.uint8)
    acc = np.zeros(bits.shape[0], np.uint32)
    for i in range(bits.shape[1]):
        acc = ((acc << 1) | bits[:, i]) & 31
        g = GEN[acc]
        out[:, 2 * i], out[:, 2 * i + 1] = g >> 1, g & 1
    return out


def decode(soft, nout, rule="ref"):
    """SoftVector::decode on every word of soft [B, n] float32 -> [B, nout] bits, all arithmetic in float32."""
    assert rule in ("ref", "le", "lastmin", "assoc", "rowleak")
    soft = np.asarray(soft, F32)
    B, n = soft.shape
    steps = nout + DEFERRAL
    with np.errstate(all="ignore"):
        hard = soft > F32(0.5)                                 # sliced() (bv:424-433); false for a NaN
        p = np.where(hard, F32(1.0) - soft, soft).astype(F32)  # bv:467-478
        ip = (F32(1.0) - p).astype(F32)
        p = np.where(p < F32(0.01), F32(0.01), p)
        ip = np.where(ip < F32(0.01), F32(0.01), ip)
        match, mismatch = (F32(0.25) / ip).astype(F32), (F32(0.25) / p).astype(F32)
    k = np.full((2, B, max(2 * steps, n)), 0.5, F32)           # k[c]: the cost of coder bit c; past the data: unknowns
    k[0, :, :n] = np.where(hard, mismatch, match)
    k[1, :, :n] = np.where(hard, match, mismatch)
    s = np.arange(16)
    pa, pb, low = s >> 1, 8 + (s >> 1), (s & 1).astype(np.uint32)
    rows = np.arange(B)[:, None]
    cost = np.zeros((B, 16), F32)
    ist = np.zeros((B, 16), np.uint32)
    out = np.zeros((B, nout), np.uint8)
    with np.errstate(invalid="ignore"):
        for t in range(steps):
            cand = []
            for prev in (pa, pb):                              # branchCandidates + getSoftCostMetrics (bv:334-368)
                i = (ist[:, prev] << np.uint32(1)) | low
                g = GEN[i & np.uint32(31)]
                first, second = k[g >> 1, rows, 2 * t], k[g & 1, rows, 2 * t + 1]
                c0 = cost[:, prev]
                c = (c0 + second) + first if rule == "assoc" else c0 + (second + first)
                cand.append((c.astype(F32), i))
            (ca, ia), (cb, ib) = cand
            take = ca <= cb if rule == "le" else ca < cb       # pruneCandidates (bv:371-379)
            cost, ist = np.where(take, ca, cb), np.where(take, ia, ib)
            if t < DEFERRAL:
                continue
            bit = (ist >> np.uint32(DEFERRAL)) & np.uint32(1)
            if rule == "rowleak":
                mc = np.fmin.reduce(cost, axis=1)
                eq = cost == mc[:, None]
                nxt = np.concatenate([bit[1:, 0], np.zeros(1, np.uint32)])
                ob = np.where(eq.any(axis=1), bit[np.arange(B), eq.argmax(axis=1)], nxt)
            else:
                mi, mc = np.zeros(B, np.int64), cost[:, 0].copy()      # minCost (bv:382-393)
                for j in range(1, 16):
                    skip = cost[:, j] > mc if rule == "lastmin" else cost[:, j] >= mc
                    mi, mc = np.where(skip, mi, j), np.where(skip, mc, cost[:, j])
                ob = bit[np.arange(B), mi]
            out[:, t - DEFERRAL] = ob
    return out


class Member:
    def __init__(self, name, cls, soft, entries, **extra):
        self.name, self.cls, self.soft, self.entries = name, cls, np.ascontiguousarray(soft, F32), tuple(entries)
        self.n = self.soft.shape[1]
        self.nout = self.n // 2
        self.has_nan = bool(np.isnan(self.soft).any())
        self.sent = self.nan_pos = self.alt = self.groups = self.nan_rows = None
        self.__dict__.update(extra)
        self.soft.setflags(write=False)

    def __repr__(self):
        return "<%s %s>" % (self.name, "x".join(map(str, self.soft.shape)))


def _entries(nout):
    return CHANNEL_NOUT.get(nout, ("viterbi",))


def _sent(rng, B, nout):
    u = rng.integers(0, 2, (B, nout)).astype(np.uint8)
    if nout > 8:
        u[:, -4:] = 0                                          # tail bits
    return u


def _flip(rng, c, share):
    return c ^ (rng.random(c.shape) < share).astype(np.uint8)


def alphabet_members(rng, nout, B=B_WORDS, tag=None):
    tag = tag or "n%d" % nout
    e = _entries(nout)
    garbage = ALPHABET[rng.integers(0, 5, (B, 2 * nout))]
    quarter = F32(0.25) + F32(0.5) * _flip(rng, encode(_sent(rng, B, nout)), 0.20).astype(F32)
    hard = _flip(rng, encode(_sent(rng, B, nout)), 0.12).astype(F32)
    return [Member("alphabet_garbage_" + tag, "alphabet", garbage, e), Member("alphabet_quarter_" + tag, "alphabet", quarter, e),
            Member("alphabet_hard_" + tag, "alphabet", hard, e)]


def edge_member(rng, nout, B=B_WORDS):
    soft = EDGES[rng.integers(0, len(EDGES), (B, 2 * nout))]
    soft.ravel()[:len(EDGES)] = EDGES                          # every edge at least once
    return Member("edges_n%d" % nout, "edges", soft, _entries(nout))


def nan_positions(n):
    """Where a word of n values gets its NaN: position 0, an odd one, the last, steps 23 | 24 and 63 | 64, late in class 1."""
    pos = [0, 1, 7, n - 1, n - 2, 46, 47, 48, 49, 126, 127, 128, 129, 301, 376]
    return [p for p in pos if 0 <= p < n]


def _plant_nan(soft, pos):
    nan = np.array([0x7FC00000, 0xFFC00000, 0x7F800001, 0xFFFFFFFF], np.uint32).view(F32)    # either sign, quiet and not
    where = np.array([pos[i % len(pos)] for i in range(len(soft))])
    soft[np.arange(len(soft)), where] = nan[(np.arange(len(soft)) // len(pos)) % 4]
    return where


def nan_members(rng, nout, B=B_WORDS):
    e, n = _entries(nout), 2 * nout
    garbage = ALPHABET[rng.integers(0, 5, (B, n))]
    gpos = _plant_nan(garbage, nan_positions(n))
    sent = _sent(rng, B, nout)
    clean = F32(0.1) + F32(0.8) * encode(sent).astype(F32)
    cpos = _plant_nan(clean, nan_positions(n))
    return [Member("nan_garbage_n%d" % nout, "nan", garbage, e, nan_pos=gpos),
            Member("nan_clean_n%d" % nout, "nan", clean, e, nan_pos=cpos, sent=sent)]


def isolation_member(rng, nout):
    """Rows 0..3 of a wave in turn (two waves: words r and 4 + r carry the NaN), then ragged batches of 5, 6, 7 words whose
    last word carries it."""
    n = 2 * nout
    sizes = [8, 8, 8, 8, 5, 6, 7]
    marks = [(r, 4 + r) for r in range(4)] + [(4,), (5,), (6,)]
    pos = nan_positions(n)
    a, b, rows, groups, at = [], [], [], [], 0
    for g, (sz, mk) in enumerate(zip(sizes, marks)):
        wa, wb = ALPHABET[rng.integers(0, 5, (sz, n))], EDGES[rng.integers(0, len(EDGES), (sz, n))]
        mask = np.zeros(sz, bool)
        mask[list(mk)] = True
        wb[mask] = wa[mask]
        for j, w in enumerate(mk):
            p = pos[(2 * g + j) % len(pos)]
            wa[w, p] = wb[w, p] = F32(np.nan) if j == 0 else -F32(np.nan)
        a.append(wa); b.append(wb); rows.append(mask)
        groups.append(slice(at, at + sz))
        at += sz
    alt = np.concatenate(b).astype(F32)
    alt.setflags(write=False)
    return Member("isolation_n%d" % nout, "isolation", np.concatenate(a), _entries(nout), alt=alt,
                  groups=groups, nan_rows=np.concatenate(rows))


def wire_member(rng, nout, B=B_WORDS):
    soft = WIRE_VALUES[rng.integers(0, len(WIRE_VALUES), (B, 2 * nout))]
    flat = soft.ravel()
    flat[rng.permutation(flat.size)[:len(WIRE_VALUES)]] = WIRE_VALUES      # every value at least once
    return Member("wire_n%d" % nout, "wire", soft, _entries(nout))


@functools.lru_cache(maxsize=None)
def family():
    """All members, seeded: the same words everywhere."""
    rng = np.random.default_rng(20261019)
    out = []
    for nout in sorted(set(LENGTHS) | set(CHANNEL_NOUT)):
        out += alphabet_members(rng, nout)
    for nout in sorted(CHANNEL_NOUT):
        out.append(edge_member(rng, nout))
        out += nan_members(rng, nout)
        out.append(isolation_member(rng, nout))
        out.append(wire_member(rng, nout))
    return tuple(out)


def members(cls=None, entry=None, nout=None):
    """Members by class, entry point and length.  "lengths" names the alphabet members at the lengths of LENGTHS."""
    def of_class(m):
        return cls is None or (m.cls == "alphabet" and m.nout in LENGTHS if cls == "lengths" else m.cls == cls)
    return [m for m in family() if of_class(m) and (entry is None or entry in m.entries) and (nout is None or m.nout == nout)]


def clean_prefix(m):
    """Per word of a member with `sent` and `nan_pos`: the number of leading output bits that no NaN cost has touched --
    output op is taken at step op + 24, and the NaN enters at step nan_pos // 2."""
    return np.clip(m.nan_pos // 2 - DEFERRAL, 0, m.nout)
