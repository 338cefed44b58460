"""Proof, on the CPU, that the soft-bit family of tests/fec_family.py is what it claims: its numpy trellis is the oracle's,
the oracle is the real reference on every word (NaN and Inf included; live where oracle/_ref/libref_fec.so is built, replayed
from tests/golden/ref_calls/ elsewhere), each mutant of the three decisions changes at least half the words of the members
meant to catch it (a quantiser that rounds its product too early among them), the kernel's rule before its NaN fix differs from the reference on every NaN member and on no other, and
a clean code word with one NaN still decodes to the sent bits ahead of the NaN."""
import numpy as np
import pytest

import fec_family as ff
import fecbind
from ref_replay import refs  # noqa: F401  (fixture)


@pytest.fixture(scope="module")
def o():
    return fecbind.FecOracle()


@pytest.fixture(scope="module")
def oracle_bits(o):
    """The oracle's output for every word of the family, computed once: name -> [B, nout] (and name + "/alt")."""
    out = {}
    for m in ff.family():
        out[m.name] = np.stack([o.viterbi_decode(w, m.nout) for w in m.soft])
        if m.alt is not None:
            out[m.name + "/alt"] = np.stack([o.viterbi_decode(w, m.nout) for w in m.alt])
    return out


@pytest.fixture(scope="module")
def model_bits():
    cache = {}

    def get(m, rule):
        if (m.name, rule) not in cache:
            cache[m.name, rule] = ff.decode(m.soft, m.nout, rule)
        return cache[m.name, rule]
    return get


def test_family_is_as_described():
    fam = ff.family()
    assert len({m.name for m in fam}) == len(fam)
    assert 2000 <= sum(len(m.soft) for m in fam) <= 5000
    assert {m.nout for m in ff.members("alphabet")} == set(ff.LENGTHS) | {18}
    for entry, nout in (("rach", 18), ("sch", 39), ("xcch", 228), ("tch", 228), ("stream", 228)):
        assert {m.cls for m in ff.members(entry=entry)} == {"alphabet", "edges", "nan", "isolation", "wire"}, entry
        assert {m.nout for m in ff.members(entry=entry)} == {nout}
    for m in fam:
        assert m.soft.dtype == np.float32 and m.soft.shape[1] == 2 * m.nout and "viterbi" in m.entries
        assert m.has_nan == (m.cls in ("nan", "isolation")), m
    for m in ff.members("edges"):
        assert all((m.soft.view(np.uint32) == e.view(np.uint32)).any() for e in ff.EDGES), m      # -0.0 by its bits
        assert set(np.unique(m.soft.view(np.uint32))) <= set(ff.EDGES.view(np.uint32))
    for m in ff.members("nan"):
        assert (np.isnan(m.soft).sum(axis=1) == 1).all() and np.isnan(m.soft[np.arange(len(m.soft)), m.nan_pos]).all()
        assert set(ff.nan_positions(m.n)) == set(m.nan_pos)
        assert {0, 1, m.n - 1} <= set(m.nan_pos) and np.signbit(m.soft[np.isnan(m.soft)]).any() \
            and not np.signbit(m.soft[np.isnan(m.soft)]).all()
    for m in ff.members("nan", nout=228):
        assert {p // 2 for p in m.nan_pos} >= {23, 24, 63, 64}
    for m in ff.members("isolation"):
        assert np.array_equal(np.isnan(m.soft).any(axis=1), m.nan_rows) and np.array_equal(np.isnan(m.alt).any(axis=1), m.nan_rows)
        same = (m.soft.view(np.uint32) == m.alt.view(np.uint32)).all(axis=1)
        assert np.array_equal(same, m.nan_rows)                                 # the NaN words alone are shared
        assert {i % 4 for g in m.groups for i in np.flatnonzero(m.nan_rows[g])} == {0, 1, 2, 3}       # every row of a wave
        assert [g.stop - g.start for g in m.groups if m.nan_rows[g][-1]] == [8, 5, 6, 7]        # a NaN word ends the ragged ones
    w = ff.WIRE_VALUES
    assert w.min() == 0 and w.max() == 1 and len(w) == 513 and len(set(w)) == 513
    lo, hi = w[:255].astype(np.float64), w[255:510].astype(np.float64)
    k = np.arange(255)
    assert (lo * 510 < 2 * k + 1).all() and (hi * 510 > 2 * k + 1).all()      # on either side of every tie of round(x * 255)
    assert np.array_equal(np.flatnonzero(np.nextafter(w[:255], np.float32(1)) != w[255:510]), [127])   # 0.5 lies between those two
    assert np.array_equal(np.round(lo * 255.0), k) and np.array_equal(np.round(hi * 255.0), k + 1)
    for m in ff.members("wire"):
        assert set(np.unique(m.soft)) == set(w)


def test_model_is_the_oracle(oracle_bits, model_bits):
    for m in ff.family():
        assert np.array_equal(model_bits(m, "ref"), oracle_bits[m.name]), m
        if m.alt is not None:
            assert np.array_equal(ff.decode(m.alt, m.nout), oracle_bits[m.name + "/alt"]), m


def test_oracle_is_the_reference(o, oracle_bits, refs):
    r = refs.fec()
    for m in ff.family():
        for name, words in ((m.name, m.soft),) + (((m.name + "/alt", m.alt),) if m.alt is not None else ()):
            want = oracle_bits[name]
            for i, w in enumerate(words):
                assert np.array_equal(r.soft_decode(w, m.nout), want[i]), (name, i)


def share(a, b):
    return float((a != b).any(axis=1).mean())


def test_mutants_change_half_the_words(model_bits):
    """A condition on the family, not a measurement of it.  At the channels' code-word lengths (189 and 228 outputs) and
    above, each of the three alphabet members must see `le` and `lastmin` in at least half its words, and the two with
    inexact costs (the garbage and .25 / .75, whose 0.25 / 0.75 = 1 / 3 is rounded) must see `assoc`; hard 0 / 1 words have
    the costs 25 and 0.25 / 0.99 only, whose sums stay exact too often for the order of the adds to show.  A shorter word has
    fewer steps at which to differ, so below 189 the shares are printed and not demanded."""
    seen = 0
    for m in ff.members("alphabet"):
        ref = model_bits(m, "ref")
        for rule in ("le", "lastmin", "assoc"):
            sh = share(model_bits(m, rule), ref)
            print("%-28s %-8s changes %.3f of the words" % (m.name, rule, sh))
            if m.nout >= 189 and (rule != "assoc" or "hard" not in m.name):
                seen += 1
                assert sh >= 0.5, (m.name, rule, sh)
    assert seen == 3 * 8


def test_wire_member_sees_a_wrong_quantiser(o):
    """The hop's conversion is round((double) v * 255.0).  One that rounds the product to float32 first moves the values
    next to a tie across it -- a quarter of the member's values -- and, at XCCH / TCH length, changes the decode of at
    least half its words (at RACH and SCH length a word has too few steps: printed only)."""
    for m in ff.members("wire"):
        good = o.wire(m.soft)
        prod = (m.soft * np.float32(255.0)).astype(np.float32)
        bad = (np.floor(prod.astype(np.float64) + 0.5) / 256.0).astype(np.float32)
        assert 0.2 < (good != bad).mean() < 0.3, m
        sh = share(ff.decode(good, m.nout), ff.decode(bad, m.nout))
        print("%-12s a float32 product changes %.3f of the words" % (m.name, sh))
        if m.nout == 228:
            assert sh >= 0.5, (m, sh)


def test_row_leak_shows_on_every_nan_member_and_on_no_other(model_bits):
    for m in ff.family():
        got, ref = model_bits(m, "rowleak"), model_bits(m, "ref")
        if not m.has_nan:
            assert np.array_equal(got, ref), m
            continue
        words = np.isnan(m.soft).any(axis=1)
        diff = (got != ref).any(axis=1)
        print("%-24s row leak changes %.3f of the NaN words, %.1f bits each" % (m.name, diff[words].mean(), (got != ref).sum() / max(diff.sum(), 1)))
        assert diff[words].any() and not diff[~words].any(), m
    for m in ff.members("isolation"):                                           # and the leak is the neighbour's: alt differs
        a, b = ff.decode(m.soft, m.nout, "rowleak"), ff.decode(m.alt, m.nout, "rowleak")
        assert (a[m.nan_rows] != b[m.nan_rows]).any(), m
        assert np.array_equal(ff.decode(m.soft, m.nout)[m.nan_rows], ff.decode(m.alt, m.nout)[m.nan_rows])


def test_clean_word_with_a_nan_decodes_up_to_it(oracle_bits):
    for m in ff.members("nan"):
        if m.sent is None:
            continue
        keep = ff.clean_prefix(m)
        got = oracle_bits[m.name]
        col = np.arange(m.nout)[None, :]
        before = col < keep[:, None]
        assert np.array_equal(got[before], m.sent[before]), m
        if m.nout == 228:
            assert before.sum() > 20 * len(keep) and (keep == 0).any() and (keep > 100).any()
            late = (m.nan_pos // 2 < m.nout - 40)                               # and the NaN does ruin what follows it
            assert (got[late] != m.sent[late]).any(axis=1).mean() > 0.9
