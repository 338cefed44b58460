"""The GPRS packet data block coders' statement (tests/pdtch_model.py, include/trxsig.h) on the CPU: what follows from its
constants -- the counts, the codes' linearity and distances --, CS-1 against the XCCH coder and decoder of the oracle, the
round trip on every scheme, the flag vote, missing bursts, random input, and a block-error table over the oracle's modulator
and demodulator (printed, not asserted).  No GPU."""
import itertools

import numpy as np
import pytest

import fecbind
import fectxbind
import pdtch_model as pm


@pytest.fixture(scope="module")
def o():
    return fecbind.FecOracle()


def soft_of(bits):
    return np.ascontiguousarray(bits, np.float32).reshape(-1, 148)


def test_counts_close():
    assert pm.keep_mask(pm.CS2).size == 588 and int((~pm.keep_mask(pm.CS2)).sum()) == 132 and 588 - 132 == 456
    assert pm.keep_mask(pm.CS3).size == 676 and int((~pm.keep_mask(pm.CS3)).sum()) == 220 and 676 - 220 == 456
    assert 12 + 428 + 16 == 456
    assert 6 + (271 - 3) + 16 + 4 == 294 and 6 + (315 - 3) + 16 + 4 == 338 and 184 + 40 + 4 == 228
    assert [(k + 7) // 8 for k in pm.K] == list(pm.OCTETS) and max(pm.OCTETS) == pm.BLOCK_BYTES
    # every code-word position lands on one e-bit of one burst, and the flags and the midamble are not among them
    where = set(zip(pm.C_BURST.tolist(), pm.C_POS.tolist()))
    assert len(where) == 456 and all(3 <= p < 60 or 88 <= p < 145 for _, p in where)
    assert len(set(pm.FLAG_POS)) == 8 and pm.FLAG_POS[:3] == ((0, 87), (0, 60), (1, 87))


def _min_distance(words):
    return min(int((a != b).sum()) for a, b in itertools.combinations(words, 2))


def test_tables_are_linear_codes():
    for table, dmin in ((pm.USF6_BITS, 3), (pm.USF12_BITS, 5)):
        for a in range(8):
            for b in range(8):
                assert np.array_equal(table[a] ^ table[b], table[a ^ b])      # linear in the row index: a group code
        assert _min_distance(table) == dmin
    assert [s[:3] for s in pm.USF6] == ["%d%d%d" % (r >> 2, r >> 1 & 1, r & 1) for r in range(8)]   # CS-2/3: systematic
    assert _min_distance(pm.FLAG_BITS) >= 5


def test_cs1_is_xcch(o):
    rng = np.random.default_rng(1)
    for i in range(12):
        tsc = i % 8
        blocks = pm.random_blocks(rng, [pm.CS1])
        got = pm.encode(o, blocks, np.array([pm.CS1]), np.array([tsc]), fectxbind.TSC_BITS)[0]
        assert np.array_equal(got, o.xcch_encode(blocks[0, :23], fectxbind.TSC_BITS[tsc])), i
        # the decoder: noisy soft values, both outcomes
        sigma = (0.1, 0.45, 0.6)[i % 3]
        v = (got.astype(np.float32) + rng.normal(0, sigma, got.shape)).astype(np.float32)
        r = pm.decode_block(o, v, cs_force=pm.CS1)
        x = o.xcch_decode(np.concatenate([v[:, 3:60], v[:, 88:145]], axis=1))
        assert r["ok"] == int(x["ok"]) and np.array_equal(np.packbits(x["d"]), r["block"][:23]) and not r["block"][23:].any(), i


@pytest.mark.parametrize("cs", [pm.CS1, pm.CS2, pm.CS3, pm.CS4])
def test_round_trip(o, cs):
    rng = np.random.default_rng(10 + cs)
    n = 16
    blocks = pm.random_blocks(rng, [cs] * n)
    for i in range(8):                                      # all eight USFs
        blocks[i, 0] = (blocks[i, 0] & 0xF8) | i
    tsc = rng.integers(0, 8, n)
    bits = pm.encode(o, blocks, np.full(n, cs), tsc, fectxbind.TSC_BITS)
    assert np.array_equal(bits[:, :, 61:87], fectxbind.TSC_BITS[tsc][:, None, :].repeat(4, axis=1))
    assert not bits[:, :, :3].any() and not bits[:, :, 145:].any()
    for wire in (False, True):
        got, gcs, dist, ok, usf = pm.decode(o, soft_of(bits), None, n, wire=wire)
        assert np.array_equal(got, blocks) and (gcs == cs).all() and not dist.any() and ok.all()
        assert np.array_equal(usf, blocks[:, 0] & 7)
    assert float(o.wire1(0.5)) == 0.5                       # a missing or deleted value is 0.5 on either side of the UDP hop
    # spare bits and octets past the scheme's size are ignored on encode
    dirty = blocks.copy()
    dirty[:, pm.OCTETS[cs]:] = 0xFF
    if pm.K[cs] % 8:
        dirty[:, pm.OCTETS[cs] - 1] |= (0xFF << (pm.K[cs] % 8)) & 0xFF
    assert np.array_equal(pm.encode(o, dirty, np.full(n, cs), tsc, fectxbind.TSC_BITS), bits)


def test_bad_scheme_or_tsc_is_zero(o):
    rng = np.random.default_rng(2)
    blocks = pm.random_blocks(rng, [1, 4, 2, 255])
    bits = pm.encode(o, blocks, np.array([1, 4, 2, 255]), np.array([0, 0, 8, 0]), fectxbind.TSC_BITS)
    assert bits[0].any() and not bits[1:].any()


def test_vote_with_flipped_flags():
    for cs in range(4):
        for flips in range(3):
            for which in itertools.combinations(range(8), flips):
                h = pm.FLAG_BITS[cs].copy()
                h[list(which)] ^= 1
                assert pm.vote(h) == (cs, flips)
    assert pm.vote(np.zeros(8, np.uint8)) == (pm.CS3, 2)    # all flags unknown (0.5 slices to 0)
    # a tie goes to the lower scheme: CS-1 and CS-3 differ in six places, three flips towards CS-3 leave 3 and 3
    h = pm.FLAG_BITS[pm.CS1].copy()
    h[[0, 1, 3]] ^= 1
    assert pm.vote(h) == (pm.CS1, 3) and (pm.FLAG_BITS[pm.CS3] != h).sum() == 3


def test_one_burst_missing(o, capsys):
    """CS-4 has no redundancy: a missing burst must fail its check (seeds checked here: none passes by the 2^-16 chance).
    CS-1..3 are reported."""
    rng = np.random.default_rng(77)
    passed = np.zeros((4, 4), int)
    trials = 6
    for cs in range(4):
        blocks = pm.random_blocks(rng, [cs] * trials)
        bits = pm.encode(o, blocks, np.full(trials, cs), np.zeros(trials, int), fectxbind.TSC_BITS)
        for miss in range(4):
            index = np.arange(4 * trials).reshape(trials, 4).copy()
            index[:, miss] = (-1, 4 * trials, -7, 1 << 30, -1, 4 * trials)     # outside [0, n_rows) either way
            got, gcs, dist, ok, usf = pm.decode(o, soft_of(bits), index, trials, cs_force=cs)
            passed[cs, miss] = int((ok.astype(bool) & (got == blocks).all(axis=1)).sum())
            if cs == pm.CS4:
                assert not ok.any(), miss
    with capsys.disabled():
        print("\nblocks recovered of %d with burst t missing (rows CS-1..CS-4, columns t = 0..3):\n%s" % (trials, passed))


def test_random_soft_is_not_accepted(o):
    rng = np.random.default_rng(5)
    n = 24
    soft = rng.random((4 * n, 148)).astype(np.float32)
    for cs in range(4):
        assert not pm.decode(o, soft, None, n, cs_force=cs)[3].any(), cs       # (seed checked: no 2^-16 / 2^-40 accident)
    blocks, cs, dist, ok, usf = pm.decode(o, soft, None, n)
    assert not ok.any() and (cs <= 3).all()


def test_pdch_map():
    blocks = [pm.pdch_map(fn) for fn in range(52)]
    assert [fn for fn in range(52) if blocks[fn] == (-1, -1)] == [12, 25, 38, 51]
    assert [b for b in blocks if b[0] >= 0] == [(k, t) for k in range(12) for t in range(4)]
    assert pm.pdch_map(52 * 1000 + 13) == (3, 0)


def test_block_error_table(o, capsys):
    """Block error rate against SNR per scheme through the oracle's modulator, detector and demodulator.  Printed."""
    import oraclebind
    sps, tsc, n = 4, 2, 12
    so = oraclebind.Oracle(sps)
    rng = np.random.default_rng(9)
    lines = []
    mod = {}
    for cs in range(4):
        blocks = pm.random_blocks(rng, [cs] * n)
        bits = pm.encode(o, blocks, np.full(n, cs), np.full(n, tsc), fectxbind.TSC_BITS).reshape(4 * n, 148)
        mod[cs] = (blocks, [so.modulate(b, 8) for b in bits])
    for snr_db in (0, 3, 6, 9, 12):
        sigma = np.sqrt(0.5 * 10 ** (-snr_db / 10.0))       # unit-power GMSK, complex noise of variance 2 sigma^2
        row = []
        for cs in range(4):
            blocks, bursts = mod[cs]
            x = np.concatenate(bursts)
            x = (x + sigma * (rng.standard_normal(x.size) + 1j * rng.standard_normal(x.size))).astype(np.complex64)
            length = np.array([len(b) for b in bursts], np.int32)
            off = np.concatenate([[0], np.cumsum(length)[:-1]]).astype(np.int32)
            det, amp, toa, soft = so.normal_batch(x, off, length, tsc, nthreads=4)
            soft[~det.astype(bool)] = 0.5
            got, gcs, dist, ok, usf = pm.decode(o, soft, None, n, wire=True)
            good = ok.astype(bool) & (gcs == cs) & (got == blocks).all(axis=1)
            row.append(1.0 - good.mean())
        lines.append("%5d dB   %s" % (snr_db, "   ".join("%5.2f" % r for r in row)))
    with capsys.disabled():
        print("\nblock error rate, %d blocks a cell (columns CS-1..CS-4):\n%s" % (n, "\n".join(lines)))
