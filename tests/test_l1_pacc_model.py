"""tests/l1_pacc_model.py against what include/trxsig_l1pacc.h states, without a GPU: the PTCCH/U frames, split equals whole
across FN mod 416 = 0 and across the hyperframe wrap, the timing-advance message through the CS-1 coder and back, and the
closed-loop inputs of tests/test_gpu_l1pacc.py through the oracle's modulator, detectRACHBurst and demodulator: every burst
sent is detected, ok, with its word and TA = round(delay)."""
import numpy as np
import pytest

import access_model as am
import fecbind
import fectxbind
import l1_pacc_model as lp
import oraclebind
import pdtch_model as pm


@pytest.fixture(scope="module")
def fo():
    return fecbind.FecOracle()


def test_ptcch_frames_are_12_plus_26_n():
    got = [(fn, lp.tai_of(fn)) for fn in range(832) if lp.tai_of(fn) >= 0]
    assert got == [(416 * m + 12 + 26 * n, n) for m in range(2) for n in range(16)]
    assert {fn % 52 for fn, _ in got} == {12, 38}            # the frames trxsig_l1pdch.h gives to PTCCH/D on the downlink
    assert all(pm.pdch_map(fn) == (-1, -1) for fn, _ in got)
    assert lp.tai_of(lp.HYPERFRAME + 12) == lp.tai_of(12) == 0 and lp.HYPERFRAME % 416 == 0


def test_blocks_follow_the_decoders_rule():
    assert lp.blocks(0, 52) == (0, 12) and lp.blocks(3, 2) == (0, 2) and lp.blocks(12, 1) == (0, 0) and lp.blocks(11, 3) == (2, 2)
    assert lp.blocks(25, 1)[1] == 0 and lp.blocks(50, 4) == (11, 2)


def fake_results(rng, fo, occ, fmt):
    """A detector's results for a list of occasions: most detected, clean bursts of random words at random arrival times, some
    of another cell, some noise."""
    n = len(occ)
    det = (rng.random(n) < 0.8).astype(np.uint8)
    soft = rng.random((n, 148)).astype(np.float32)
    for i in range(n):
        if rng.random() < 0.8:
            soft[i] = am.encode(fo, [int(rng.integers(0, 256))], [0], [lp.BSIC if rng.random() < 0.85 else 5])[0]
    toa = (rng.random(n) * 300 - 20).astype(np.float32)
    return det, (rng.random(n) + 1j * rng.random(n)).astype(np.complex64), toa, rng.random(n).astype(np.float32), soft


@pytest.mark.parametrize("fn,F,cuts", [(390, 130, (1, 13, 26, 52, 77)), (lp.HYPERFRAME - 40, 130, (1, 39, 40, 41, 100)),
                                        (403, 900, (9, 425, 426, 841))])
def test_split_equals_whole(fo, fn, F, cuts):
    """The dense outputs and the table of one call equal those of its pieces, with the same detector results per frame.  The
    third case holds two measurements of every TAI: the later one stays."""
    rng = np.random.default_rng(fn % 1000)
    n = len(lp.pdchs(lp.COMB))
    _, nb = lp.blocks(fn, F)
    prach = (rng.random((n, nb)) < 0.4).astype(np.uint8)
    occ = lp.cell_list(lp.COMB, fn, F, prach, 4, 1280, 640)
    res = fake_results(rng, fo, occ, 0)
    whole_t = lp.Table(n)
    whole = lp.fold(fo, whole_t, lp.COMB, lp.BSIC, fn, F, prach, 4, occ, *res, 0, True)
    assert whole["ok"].sum() > 5 and whole_t.valid.sum() > 5 and (whole["kind"] == lp.PRACH).any()
    t = lp.Table(n)
    parts = []
    blk0 = lp.blocks(fn, F)[0]
    for a, b in zip((0,) + cuts, cuts + (F,)):
        b0, nbp = lp.blocks((fn + a) % lp.HYPERFRAME, b - a)
        first = lp.block_of(fn + a + next((k for k in range(b - a) if lp.block_of(fn + a + k)[0] >= 0), 0))[0]
        pp = prach[:, first - blk0:first - blk0 + nbp] if nbp else None
        po = lp.cell_list(lp.COMB, (fn + a) % lp.HYPERFRAME, b - a, pp, 4, 1280, 640)
        pick = [i for i, o in enumerate(occ) if a <= o[1] < b]
        assert [(o[0], o[1] - a, o[2]) for o in (occ[i] for i in pick)] == [(o[0], o[1], o[2]) for o in po]
        sub = [np.asarray(x)[pick] for x in res]
        parts.append(lp.fold(fo, t, lp.COMB, lp.BSIC, (fn + a) % lp.HYPERFRAME, b - a, pp, 4, po, *sub, 0, True))
    for key in whole:
        assert np.array_equal(np.concatenate([p[key] for p in parts], axis=1), whole[key]), key
    assert t.same(dict(ta=whole_t.ta, fn=whole_t.fn, valid=whole_t.valid))
    assert (whole_t.fn[whole_t.valid != 0] < lp.HYPERFRAME).all()


def test_ta_formula():
    assert [lp.ta_of(x, 4) for x in (-3.0, 0.0, 1.9, 2.0, 6.1, 251.9, 252.0, 400.0)] == [0, 0, 0, 1, 2, 63, 63, 63]
    assert lp.ta_of(np.float32(13.0), 1) == 13 and lp.ta_of(np.float32(12.5), 1) == 13 and lp.ta_of(np.float32(12.49), 1) == 12


def test_message_through_cs1_and_back(fo):
    """ta_message -> the CS-1 coder and decoder of tests/pdtch_model.py -> ta_read is the identity on the table."""
    rng = np.random.default_rng(3)
    t = lp.Table(3)
    t.valid[:] = rng.random((3, 16)) < 0.6
    t.ta[:] = rng.integers(0, 64, (3, 16)) * t.valid
    kind, payload = t.message(2)
    assert kind.all() and (payload[:, :, 16:] == 0x2B).all() and not (payload[:, :, :16] & 0x80).any()
    want = np.where(t.valid != 0, t.ta, 99).astype(np.uint8)   # a TAI without a value stays as it was
    back, ok = np.zeros((3, 2, 23), np.uint8), np.zeros((3, 2), np.uint8)
    for g in range(3):
        for b in range(2):
            block = np.zeros((1, pm.BLOCK_BYTES), np.uint8)
            block[0, :23] = payload[g, b]
            bits = pm.encode(fo, block, [pm.CS1], [lp.BSIC & 7], fectxbind.TSC_BITS)
            blk, cs, _, k, _ = pm.decode(fo, bits[0].astype(np.float32), None, 1, wire=True, cs_force=0)
            back[g, b], ok[g, b] = blk[0, :23], k[0]
    assert ok.all()
    before = np.full((3, 16), 99, np.uint8)
    assert np.array_equal(lp.ta_read(before, back, ok), want)
    ok[1] = 0
    got = lp.ta_read(before, back, ok)
    assert (got[1] == 99).all() and np.array_equal(got[0], want[0])       # unchanged where no block came with ok


@pytest.mark.parametrize("sps", [1, 4])
@pytest.mark.parametrize("fmt", [0, 1])
def test_closed_loop_on_the_cpu(fo, sps, fmt):
    """The GPU test's closed-loop inputs (same seed, plan, words, delays of 0..20 symbols whole and fractional, amplitude 1000, no
    noise) through the oracle's modulator, detectRACHBurst and demodulator: every burst sent is detected and ok with its word
    and TA = round(delay); every marked block the handsets left empty gives det == 0."""
    fn, F = 403, 130
    so = oraclebind.Oracle(sps)
    s = lp.scenario(11, fn, F, fmt)
    cells, ss, sa = lp.cells_cpu(fo, so, s, fn, F, fmt)
    t = lp.Table(3)
    r = lp.detect(fo, so, t, lp.COMB, lp.BSIC, cells, ss, sa, fn, F, s["prach"], fmt, True)
    sent = lp.sent_bursts(s, fn, F)
    assert len(sent) >= 20
    for g, k, ra, delay in sent:
        assert (r["det"][g, k], r["ok"][g, k], r["fmt"][g, k], r["ra"][g, k]) == (1, 1, fmt, ra), (g, k, delay)
        assert r["ta"][g, k] == int(np.floor(delay + 0.5)), (g, k, delay, r["toa"][g, k])
    here = {(g, k) for g, k, _, _ in sent}
    empty = [(g, k) for g in range(3) for k in range(F) if r["kind"][g, k] and (g, k) not in here]
    assert len(empty) >= 10 and not any(r["det"][g, k] for g, k in empty)
    assert t.valid.sum() == sum(1 for g, k, _, _ in sent if lp.tai_of(fn + k) >= 0)
