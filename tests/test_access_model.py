"""tests/access_model.py against what include/trxsig.h states of the access burst's two coders, without a GPU: the bit
counts, the 8-bit format against the mobile-side model's access burst, every 11-bit word through its own decoder, the punctured
code's minimum weight (computed here, written in the header), single-bit flips, the rule that chooses between the two formats,
and three mutants of the 11-bit coder that the pinned vectors catch.

The 11-bit format's six deleted positions and its bit order are from memory of GSM 05.03 5.3.2: what pins them here is this
project's own statement, the vectors below, not the standard."""
import os
import re

import numpy as np
import pytest

import access_model as am
import fecbind
import l1_ms_model as mm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BSICS = (0, 21, 43, 63)

# e(0..35) of (word, format, BSIC), the first character the first bit sent: written down from access_model.e36 when the format
# was stated, so that a later change of a deleted position, of the colouring or of the bit order shows.
VECTORS = {
    (0x000, 1, 0): "000000000000000000011101001101001001",
    (0x555, 1, 0x2B): "111100010001000100010110010111011110",
    (0x7FF, 1, 63): "101011010101010101010100100000001011",
    (0x123, 1, 7): "100110000010000100011000100000101101",
    (0x6B4, 1, 50): "001011101100001000101011001000011000",
    (0xA5, 0, 0x2B): "110111101100101101100010100001111111",
}


@pytest.fixture(scope="module")
def o():
    return fecbind.FecOracle()


def text(bits):
    return "".join(map(str, bits))


def test_counts_close(o):
    u = am.coder_input(o, 0x5A5, am.ACCESS_11, 9)
    assert len(u) == 21 and len(o.encode(u)) == 42 and len(am.e36(o, 0x5A5, am.ACCESS_11, 9)) == 36
    assert am.keep_mask().size == 42 and int((~am.keep_mask()).sum()) == 6 and 11 + 6 + 4 == 21
    assert sorted(np.flatnonzero(~am.keep_mask())) == [0, 2, 5, 37, 39, 41]
    assert len(am.coder_input(o, 0xA5, am.ACCESS_8, 9)) == 18 and len(am.e36(o, 0xA5, am.ACCESS_8, 9)) == 36


def test_format_0_is_the_access_burst_of_the_handset_model(o):
    for bsic in (0, 21, 63):
        ra = np.arange(256, dtype=np.uint16)
        bits = am.encode(o, ra, np.zeros(256, np.uint8), np.full(256, bsic, np.uint8))
        for r in range(256):
            assert np.array_equal(bits[r], mm.access_burst(o, r, bsic)), (r, bsic)


def test_pinned_vectors(o):
    for (word, fmt, bsic), want in VECTORS.items():
        assert text(am.e36(o, word, fmt, bsic)) == want, (word, fmt, bsic)


def test_every_word_comes_back(o):
    for bsic in BSICS:
        for w in range(2048):
            assert am.hypothesis(o, am.e36(o, w, am.ACCESS_11, bsic).astype(np.float32), am.ACCESS_11) == (w, 1, bsic), (w, bsic)
    soft = am.encode(o, np.arange(2048, dtype=np.uint16), np.ones(2048, np.uint8), np.full(2048, 17, np.uint8)).astype(np.float32)
    ra, f, t, b = am.decode(o, soft, None, 2048, wire=True, fmt=1)
    assert np.array_equal(ra, np.arange(2048)) and f.all() and t.all() and (b == 17).all()


def test_minimum_weight_is_the_headers():
    h = " ".join(open(os.path.join(ROOT, "include", "trxsig.h")).read().split())
    m = re.search(r"minimum weight over its 2\^11 - 1 nonzero words is (\d+)", h)
    assert m, "the header no longer states the minimum weight"
    assert am.min_weight() == int(m.group(1)) == 7


def test_single_bit_flips(o):
    """Every single-bit flip of a clean 11-bit burst is corrected: the word and the parity's BSIC come back for all 36 positions
    of all 2048 words.  The four tail bits are another matter, and not this format's alone: SoftVector::decode does not end its
    trellis in the zero state, it reads the last bits off the cheapest survivor, so a flip among the last coded bits comes out
    as a nonzero tail bit -- e(31..35) here (the last three steps have one sent bit each), e(34..35) in the 8-bit format, the
    reference's own.  Both sets are pinned exactly."""
    for fmt, n_words, lost in ((am.ACCESS_11, 2048, {31, 32, 33, 34, 35}), (am.ACCESS_8, 256, {34, 35})):
        for w in range(n_words):
            e = am.e36(o, w, fmt, 5).astype(np.float32)
            for k in range(36):
                v = e.copy()
                v[k] = 1 - v[k]
                ra, tail_ok, bsic = am.hypothesis(o, v, fmt)
                assert (ra, bsic) == (w, 5), (fmt, w, k)
                assert tail_ok == (k not in lost), (fmt, w, k)


def test_either_mode_on_clean_bursts(o):
    """Clean bursts of either format come back as what they are, for every word and four BSICs -- but for the 11-bit words whose
    36 bits also pass as an 8-bit burst of the cell (tail zero, parity right: ten bits, so about one word in 2^10): the rule
    gives those to the 8-bit format, as the header says.  They are counted, and each is shown to be such a word."""
    aliased = []
    for bsic in BSICS:
        for w in range(256):
            assert am.decode_row(o, am.e36(o, w, am.ACCESS_8, bsic).astype(np.float32), -1, bsic) == (w, 0, 1, bsic), (w, bsic)
        for w in range(2048):
            v = am.e36(o, w, am.ACCESS_11, bsic).astype(np.float32)
            got = am.decode_row(o, v, -1, bsic)
            if got != (w, 1, 1, bsic):
                _, t8, b8 = am.hypothesis(o, v, am.ACCESS_8)
                assert t8 and b8 == bsic and got[1] == 0, (w, bsic)
                aliased.append((bsic, w))
    assert aliased == [(21, 616), (43, 1384), (63, 0)]       # 3 of 8192
    # another cell's burst, or noise, is not taken for either format's: the result is the 8-bit hypothesis, not ok
    v = am.e36(o, 0x321, am.ACCESS_11, 12).astype(np.float32)
    ra, f, t, b = am.decode_row(o, v, -1, 13)
    assert f == 0 and not (t and b == 13)


def test_refused_rows_are_zero(o):
    ra = np.array([255, 256, 2047, 2048, 7, 7, 7], np.uint16)
    fmt = np.array([0, 0, 1, 1, 2, 0, 255], np.uint8)
    bsic = np.array([0, 0, 63, 63, 0, 64, 0], np.uint8)
    bits = am.encode(o, ra, fmt, bsic)
    assert [bool(r.any()) for r in bits] == [True, False, True, False, False, False, False]
    assert np.array_equal(bits[0, :49], am.HEAD) and not bits[:, 85:].any()


@pytest.mark.parametrize("mutant", ["puncture", "colour", "order"])
def test_mutants_are_caught(o, mutant):
    """A deleted position moved by one, a parity that is not coloured with the BSIC, d sent most significant bit first: each
    changes a pinned vector.  (The first would pass any test that only decodes what it encoded: one wrong bit is corrected.)"""
    kw = dict(puncture=dict(deleted=(0, 2, 6, 37, 39, 41)), colour=dict(colour=False), order=dict(reverse=True))[mutant]
    changed = [k for k, want in VECTORS.items() if k[1] == 1 and text(am.e36(o, k[0], 1, k[2], **kw)) != want]
    assert changed, mutant
    if mutant == "puncture":
        # (C(0) and C(1) are both d(0), and with zero tail bits C(36) = C(37), C(38) = C(39), C(40) = C(41): deleting the other
        #  bit of one of those four pairs is the same code, so only moves of C(2) and C(5) can show)
        for d in ((0, 1, 5, 37, 39, 41), (0, 3, 5, 37, 39, 41), (0, 2, 4, 37, 39, 41)):
            assert any(text(am.e36(o, k[0], 1, k[2], deleted=d)) != want for k, want in VECTORS.items() if k[1] == 1), d
