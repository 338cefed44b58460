"""Downlink L1 encode, CPU side: the literal TCHFACCHL1Encoder::dispatch / SCHL1Encoder::generate restatement in
oracle/fec_tx_oracle.c against (1) the golden streams and bursts captured from the real reference's encoder steps and
(2) that reference itself on random streams (live where oracle/_ref/libref_fec_tx.so is built, replayed from
tests/golden/ref_calls/ elsewhere); a numpy check that the closed form the GPU kernel uses -- burst b of block m carries
c_m[k], k = b mod 8, at the even e-bit positions and c_{m-1}[k], k = b+4 mod 8, at the odd ones -- equals the literal
dispatch(); and the SCH field hazards (T3 = 0, the 25-bit LSB8MSB)."""
import numpy as np
import pytest

import fectxbind
from ref_replay import refs  # noqa: F401  (fixture)

H = 26 * 51 * 2048


@pytest.fixture(scope="module")
def o():
    return fectxbind.FecTxOracle()


def j_of(k):
    return 2 * ((49 * k) % 57) + ((k % 8) // 4)


def test_golden_tch_streams(o, golden):
    g = golden("fec_tx.npz")
    assert np.array_equal(g["tsc_bits"], fectxbind.TSC_BITS) and np.array_equal(g["xts"], fectxbind.XTS_BITS)
    kind, pl, tsc, filler = g["tch_kind"], g["tch_payload"], g["tch_tsc"], g["filler"]
    bits, st = o.tch_encode_stream(kind, pl, tsc, filler)
    assert np.array_equal(bits, g["tch_bits"])
    k = int(g["tch_split"])
    b1, s1 = o.tch_encode_stream(kind[:, :k], pl[:, :k], tsc, filler)
    b2, s2 = o.tch_encode_stream(kind[:, k:], pl[:, k:], tsc, filler, state=s1)
    assert np.array_equal(np.concatenate([b1, b2], axis=1), g["tch_bits"]) and np.array_equal(s2, st)
    # the layout: zero tails, the channel's training sequence, Hu = this block stolen, Hl = the previous one
    b = g["tch_bits"]
    assert not b[..., :3].any() and not b[..., 145:].any()
    assert np.array_equal(b[..., 61:87], np.broadcast_to(fectxbind.TSC_BITS[tsc][:, None, None, :], b[..., 61:87].shape))
    fa = kind == 2
    assert np.array_equal(b[..., 87], np.repeat(fa[..., None], 4, axis=2).astype(np.uint8))
    prev = np.concatenate([np.zeros((len(kind), 1), bool), fa[:, :-1]], axis=1)
    assert np.array_equal(b[..., 60], np.repeat(prev[..., None], 4, axis=2).astype(np.uint8))


def test_golden_sch(o, golden):
    g = golden("fec_tx.npz")
    assert np.array_equal(o.sch_encode(g["sch_fn"], g["sch_bsic"]), g["sch_bits"])
    t3 = g["sch_fn"] % 51
    assert set([0, 1, 11, 21, 31, 41, 50]) <= set(t3.tolist()) and H - 1 in g["sch_fn"]
    assert {0, 63} <= set(g["sch_bsic"].tolist())


def test_random_vs_reference(o, refs):
    """The oracle's streams and SCH bursts against the reference's, on random inputs with the reference's filler."""
    import reffectx
    r = refs._open(reffectx.available, reffectx.RefFecTx, "fectx", None)   # live or replayed, as refs.fec()
    rng = np.random.default_rng(2026)
    filler = rng.integers(0, 2, 456).astype(np.uint8)
    for it in range(24):
        n = int(rng.integers(1, 60))
        kind = rng.integers(0, 3, n).astype(np.uint8)
        if it % 3 == 0:
            kind[: n // 2] = 2                                       # a FACCH run, then whatever follows
        pl = rng.integers(0, 256, (n, 33)).astype(np.uint8)
        tsc = int(rng.integers(0, 8))
        want = r.tch_dispatch(kind, pl, fectxbind.TSC_BITS[tsc], filler)
        got, _ = o.tch_encode_stream(kind[None], pl[None], [tsc], filler)
        assert np.array_equal(got[0], want), it
    fn = rng.integers(0, H, 600).astype(np.uint32)
    fn[:8] = [0, 1, 51, 102, 1326, H - 1, H - 51, 50]
    bsic = rng.integers(0, 64, 600).astype(np.uint8)
    assert np.array_equal(o.sch_encode(fn, bsic), r.sch_encode(fn, bsic, fectxbind.XTS_BITS))


def test_closed_form_equals_dispatch(o):
    """The closed form (no mI[], no mOffset) equals the literal dispatch() over random streams: from the c[] of every
    block, burst b of block m takes c_m[k] (k = b mod 8) at even j and c_{m-1}[k] (k = b+4 mod 8, zero for m = 0) at odd j."""
    rng = np.random.default_rng(8)
    K = np.arange(456)
    J = j_of(K)
    for it in range(12):
        n = int(rng.integers(1, 40))
        kind = rng.integers(0, 3, n).astype(np.uint8)
        pl = rng.integers(0, 256, (n, 33)).astype(np.uint8)
        filler = rng.integers(0, 2, 456).astype(np.uint8)
        bits, _ = o.tch_encode_stream(kind[None], pl[None], [1], filler)
        # each block's c[] on its own: a one-block stream from a fresh state puts c[k], k mod 8 < 4, in its bursts
        # and leaves the odd half c[k], k mod 8 >= 4, in the state
        c = np.zeros((n, 456), np.uint8)
        for m in range(n):
            b1, st = o.tch_encode_stream(kind[None, m:m + 1], pl[None, m:m + 1], [1], filler)
            e = np.concatenate([b1[0, 0, :, 3:60], b1[0, 0, :, 88:145]], axis=1)
            lo = K % 8 < 4
            c[m, lo] = e[K[lo] % 8, J[lo]]
            i = 4 * (K[~lo] // 8) + K[~lo] % 8 - 4
            c[m, ~lo] = (st[0, i // 8] >> (i % 8)) & 1
        for m in range(n):
            e = np.zeros((4, 114), np.uint8)
            for b in range(4):
                ke = K[K % 8 == b]
                e[b, J[ke]] = c[m, ke]
                ko = K[K % 8 == b + 4]
                e[b, J[ko]] = c[m - 1, ko] if m > 0 else 0
            assert np.array_equal(np.concatenate([bits[0, m, :, 3:60], bits[0, m, :, 88:145]], axis=1), e), (it, m)


def test_sch_field_hazards(o):
    """T3 = 0: T3' = (0u - 1) / 10 = 429496729, whose low 3 bits are 1; LSB8MSB on 25 bits reverses the first three
    octets and leaves bit 24.  Checked by decoding the oracle's own bursts bit by bit."""
    assert ((0 - 1) % (1 << 32)) // 10 & 7 == 1
    assert np.array_equal(o.lsb8msb(np.arange(25, dtype=np.uint8) % 2 + 0)[24:], [0])
    b = np.arange(25, dtype=np.uint8)
    want = np.concatenate([b[7::-1], b[15:7:-1], b[23:15:-1], b[24:]])
    assert np.array_equal(o.lsb8msb(b), want)

    def fields(burst):
        e = np.concatenate([burst[3:42], burst[106:145]]).astype(np.float32)
        u = o.viterbi_decode(e, 39)
        d = o.lsb8msb(u[:25])
        v = int("".join(map(str, d)), 2)
        par_ok = (o.parity(0x0575, 10, u[:25]) ^ int("".join(map(str, u[25:35])), 2)) == 0x3ff
        return v >> 19, (v >> 8) & 2047, (v >> 3) & 31, v & 7, par_ok and not u[35:].any()

    for fn, bsic in ((0, 5), (51 * 7, 63), (51 * 7 + 1, 0), (H - 1, 33), (1326 * 2047 + 40, 17)):
        bs, t1, t2, t3p, ok = fields(o.sch_encode([fn], [bsic])[0])
        assert ok and bs == bsic and t1 == (fn // 1326) % 2048 and t2 == fn % 26
        assert t3p == (((fn % 51) - 1) % (1 << 32)) // 10 & 7
    assert fields(o.sch_encode([0], [0])[0])[3] == 1
    assert not o.sch_encode([H, 5], [1, 64]).any()
    z = o.sch_encode([100], [9])[0]
    assert np.array_equal(z[42:106], fectxbind.XTS_BITS) and not z[:3].any() and not z[145:].any()


def test_bad_inputs(o):
    """A TSC above 7: zero bursts and the state untouched; a kind above 2: an all-zero c[] that is not stolen."""
    rng = np.random.default_rng(4)
    kind = rng.integers(0, 3, (3, 5)).astype(np.uint8)
    kind[0, 1] = 9
    pl = rng.integers(0, 256, (3, 5, 33)).astype(np.uint8)
    st0 = rng.integers(0, 256, (3, 32)).astype(np.uint8)
    bits, st = o.tch_encode_stream(kind, pl, [1, 8, 200], np.ones(456, np.uint8), state=st0)
    assert not bits[1:].any() and np.array_equal(st[1:], st0[1:])
    assert not bits[0, 1, :, 87].any() and not bits[0, 2, :, 60].any()
    e = np.concatenate([bits[0, 1, :, 3:60], bits[0, 1, :, 88:145]], axis=1)
    assert not e[:, 0::2].any()                                     # the even positions carry block 1's (zero) c[]
