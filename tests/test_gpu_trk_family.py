"""GPU tests of the tracking receiver (include/trxsig_l1trk.h) on the adversarial family of tests/trk_family.py, at sps 1, 2 and 4
-- what tests/test_gpu_l1trk.py's 3 columns, 12 frames and 4 2^-24 tolerance cannot see.  Every member goes through
test_gpu_l1trk.Rig.slice first: cells, guard words, status, anchors and the untouched streams word for word against the model.

  loops       k_l1trk_slice's grid-stride loop goes round two and three times, and one workgroup meets two frequency bursts: the
              records against float32 terms summed exactly, within the any-order float64 bound n 2^-53 sum |term|
  lattice     cells on which that sum is exact in any order: C, E and ok with ==, the threshold strict, the border Re C == 0
  overflow    a float32 term that overflows or underflows decides ok as the header says, not as the exact sum would
  nonfinite   NaN (either sign, either component) and Inf samples inside the streams: the cells' words, the records' classes
  capacity    every record of the capacity, across the multiframe, and a call whose first frequency burst is its frame 10
  phones      200 phones on 3 columns: seed's blocks of 64, the anchor loop of the slice, update on phones without columns
  update      llrint ties, adj at exact halves, the 2^24 gate, 60 rows at -2^24, afc_shift 0 and 8, 8 and 72 slots

tests/test_trk_family.py proves on the CPU that the family is what it claims."""
import numpy as np
import pytest

import _pkg
import l1_trk_model as ltm
import trk_family as tf
from test_gpu_l1trk import GUARD, Layout, Rig, dev, group_result, same_state, words

pytestmark = pytest.mark.gpu
F32 = np.float32


@pytest.fixture(scope="module")
def pkg():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return _pkg.load()


@pytest.fixture(scope="module")
def rigs(pkg):
    made = {}

    def get(sps):
        if sps not in made:
            made[sps] = Rig(pkg, sps)
        return made[sps]
    yield get
    for r in made.values():
        r.ctx.close()


@pytest.fixture(scope="module", params=tf.SPS)
def rig(request, rigs):
    return rigs(request.param)


def pair(rig, mb, **kw):
    """the device's object and the model with fcch_exact's records, both at the member's anchors"""
    trk, m = rig.pair(max_frames=mb["max_frames"], phone=mb["phone"], c0=mb["c0"], **dict(mb["kw"], **kw))
    m = tf.ExactTrk(m)
    tf.apply(mb, trk, m)
    return trk, m


def run(rig, mb, **kw):
    trk, m = pair(rig, mb, **kw)
    g, rec = rig.slice(trk, m, mb["x"], mb["n0"], mb["fn"], mb["F"])
    return trk, m, g, rec


def grade(g, rec, c0):
    """every record against fcch_exact within the summation bound; returns the worst |dC| / bound"""
    worst = 0.0
    for p, rs in enumerate(rec):
        assert len(rs) == (g["n_fcch"] if c0[p] >= 0 else 0)
        if c0[p] < 0:                                          # no records: the entries stay zero
            assert not g["fcch_c"][p].any() and not g["fcch_e"][p].any() and not g["fcch_ok"][p].any()
        for j, r in enumerate(rs):
            C, E = complex(g["fcch_c"][p, j]), float(g["fcch_e"][p, j])
            assert int(g["fcch_fn"][p, j]) == r["fn"] and r["finite"]
            dc, de = tf.record_error(r, C, E)
            assert dc <= r["bound_c"] and de <= r["bound_e"] and bool(g["fcch_ok"][p, j]) == r["ok"], (p, j, dc, r["bound_c"], de, r["bound_e"], r["ok"])
            if r["bound_c"]:
                worst = max(worst, dc / r["bound_c"], de / r["bound_e"])
    return worst


def check_promise(mb, g, rec):
    for p, want in enumerate(mb["promise"]):
        if want is not None:
            assert [r["ok"] for r in rec[p]] == want == [bool(v) for v in g["fcch_ok"][p]], p


# ---- the grid-stride loop -----------------------------------------------------------------------------------------------
def test_loop_reuse(rig):
    sps = rig.sps
    mb = tf.loop_reuse(sps)
    trk, m, g, rec = run(rig, mb)
    assert g["n_fcch"] == 2
    worst = grade(g, rec, mb["c0"])
    check_promise(mb, g, rec)
    print("sps %d loop_reuse: worst |dC| / bound %.3e" % (sps, worst))
    trk.destroy()
    # the same as two calls of 6 and 5 frames on a fresh object: one record each (frame 10 is frame 4 of the second call)
    trk2, m2 = pair(rig, mb)
    g1, rec1 = rig.slice(trk2, m2, mb["x"], mb["n0"], mb["fn"], 6)
    assert g1["n_fcch"] == 1
    grade(g1, rec1, mb["c0"])
    first = (g1["fcch_c"].copy(), g1["fcch_e"].copy(), g1["fcch_ok"].copy())
    g2, rec2 = rig.slice(trk2, m2, mb["x"], mb["n0"], mb["fn"] + 6, 5)
    assert g2["n_fcch"] == 1 and all(int(v) == mb["fn"] + 10 for p, v in enumerate(g2["fcch_fn"][:, 0]) if mb["c0"][p] >= 0)
    grade(g2, rec2, mb["c0"])
    for key in ("fn", "pos", "phase", "step", "locked"):       # the anchors: bit for bit
        assert np.array_equal(g[key], g2[key]), key
    # a record is its cell's alone: the split gives the whole call's, bit for bit (the same workgroup shape sums it)
    assert np.array_equal(first[0][:, 0], g["fcch_c"][:, 0]) and np.array_equal(first[1][:, 0], g["fcch_e"][:, 0])
    assert np.array_equal(g2["fcch_c"][:, 0], g["fcch_c"][:, 1]) and np.array_equal(g2["fcch_e"][:, 0], g["fcch_e"][:, 1])
    assert np.array_equal(first[2][:, 0], g["fcch_ok"][:, 0]) and np.array_equal(g2["fcch_ok"][:, 0], g["fcch_ok"][:, 1])
    trk2.destroy()


def test_loop_three(rigs):
    rig = rigs(1)
    mb = tf.loop_three()
    trk, m, g, rec = run(rig, mb)
    assert g["n_fcch"] == 2
    worst = grade(g, rec, mb["c0"])
    check_promise(mb, g, rec)
    print("sps 1 loop_three: worst |dC| / bound %.3e" % worst)
    trk.destroy()


# ---- records with == ----------------------------------------------------------------------------------------------------
def test_lattice(rig):
    sps = rig.sps
    for mb in tf.lattice(sps):
        for thresh in [0.5] + [t for pr in mb["pairs"] for t in pr]:
            trk, m, g, rec = run(rig, mb, fcch_thresh=float(thresh))
            r = rec[0][0]
            C, E, ok = complex(g["fcch_c"][0, 0]), float(g["fcch_e"][0, 0]), bool(g["fcch_ok"][0, 0])
            print("sps %d %-20s thresh %.9g: C %s (%s) E %r (%r) ok %d (%d)" % (sps, mb["name"], thresh, C, r["C"], E, r["E"], ok, r["ok"]))
            assert C == r["C"] == mb["expect"]["C"] and E == r["E"] == mb["expect"]["E"] and ok == r["ok"], (mb["name"], thresh)
            trk.destroy()
        for lo, hi in mb["pairs"]:                             # (what the rows above were held to)
            assert tf.fcch_exact(mb["cell"], sps, lo)["ok"] and not tf.fcch_exact(mb["cell"], sps, hi)["ok"]


def test_overflow(rig):
    for mb in tf.overflow(rig.sps):
        trk, m, g, rec = run(rig, mb)
        E, ok = float(g["fcch_e"][0, 0]), int(g["fcch_ok"][0, 0])
        print("sps %d overflow %s: C %s E %r ok %d" % (rig.sps, mb["name"], g["fcch_c"][0, 0], E, ok))
        assert E == mb["expect"]["E"] == rec[0][0]["E"] and not np.signbit(E) and ok == 0 and not rec[0][0]["ok"]
        trk.destroy()


# ---- NaN and Inf inside a stream ----------------------------------------------------------------------------------------
def slice_words(rig, trk, m, mb):
    """Rig.slice's comparison, but counting: (words that differ, all words, the first difference)"""
    x, sps = mb["x"], rig.sps
    n_cols, n = x.shape
    lay = Layout(n_cols, 8 * mb["F"], sps, "col-major")
    d_x = dev(np.array(x).view(F32))
    d_cells = dev(np.full(lay.total, GUARD, np.complex64).view(F32))
    trk.slice(d_x.data_ptr(), n, mb["n0"], n, mb["fn"], mb["F"], d_cells.data_ptr() + 8 * lay.lead, lay.slot, lay.col)
    cells, status, rec = m.slice(x, mb["n0"], mb["fn"], mb["F"])
    g = trk.collect()
    got = d_cells.cpu().numpy().view(np.complex64).ravel()
    want = lay.pack(cells)
    bad = np.flatnonzero(words(got) != words(want))
    first = None if not len(bad) else (int(bad[0]), got[bad[0] // 2], words(got)[bad[0]], want[bad[0] // 2], words(want)[bad[0]])
    return len(bad), 2 * len(want), first, g, rec


def test_nonfinite(rig):
    sps = rig.sps
    total = 0
    for variant in range(8):
        mb = tf.nonfinite(rig.o, variant)
        trk, m = pair(rig, mb)
        n_bad, n_all, first, g, rec = slice_words(rig, trk, m, mb)
        total += n_bad
        print("sps %d nonfinite %d: %d words differ of %d" % (sps, variant, n_bad, n_all))
        if first:
            print("first at word %d: got %r (%#010x) want %r (%#010x)" % first)
        trk.destroy()
    print("sps %d nonfinite: %d words differ in all" % (sps, total))
    assert total == 0
    for variant in range(8):                                   # and through the rig: guards, status, anchors, streams; the records
        mb = tf.nonfinite(rig.o, variant)
        trk, m, g, rec = run(rig, mb)
        for p in range(2):
            r = rec[p][0]
            C, E = complex(g["fcch_c"][p, 0]), float(g["fcch_e"][p, 0])
            assert not r["finite"] and g["fcch_ok"][p, 0] == 0
            for got, want in ((C.real, r["C"].real), (C.imag, r["C"].imag), (E, r["E"])):
                assert np.isnan(got) == np.isnan(want) and np.isinf(got) == np.isinf(want), (variant, p, C, E, r["C"], r["E"])
                assert np.isnan(want) or np.signbit(got) == np.signbit(want)
        trk.destroy()


# ---- the records' capacity ----------------------------------------------------------------------------------------------
def step_error(g, m, p):
    return ((int(g["step"][p]) - m.step[p] + (1 << 31)) & ltm.M32) - (1 << 31)


def afc_bound(sps, rec_p):
    """|delta - the model's|: acq_atan2's 2e-6 plus the sum's relative bound, in 2^-32 turn per sample, plus the rounding"""
    good = [r for r in rec_p if r["ok"]]
    rel = sum(r["bound_c"] for r in good) / abs(sum(r["C"] for r in good))
    return int((2.0 ** 32 / (2 * np.pi * sps)) * (2e-6 + rel)) + 1


def test_capacity(rigs):
    rig = rigs(1)
    for mb in tf.capacity():
        trk, m, g, rec = run(rig, mb, afc_shift=2)
        n = len(mb["frames"])
        assert g["n_fcch"] == n == len(rec[0]) and trk.meas.fcch_stride == mb["cap"] and (n == mb["cap"] or mb["max_frames"] == 21)
        grade(g, rec, mb["c0"])
        assert [int(v) for v in g["fcch_fn"][0]] == [(mb["fn"] + f) % ltm.HYPER for f in mb["frames"]] and g["fcch_ok"][0].all()
        E = g["fcch_e"][0]
        assert (E[1:] > 1.3 * E[:-1]).all()                    # burst j has amplitude j + 1: in order
        res, keep, (row, valid, toa) = group_result(rig.pkg, [(3, 0, 0, 0.0)], 8 * mb["F"], 1)
        trk.update(res, mb["fn"])
        did = m.update(row, valid, toa, mb["fn"])
        g = trk.collect()
        bound = afc_bound(1, rec[0])
        print("capacity %d: afc_n %d delta %d (model %d, bound %d)" % (mb["max_frames"], g["afc_n"][0], g["afc_delta"][0], did[0]["delta"], bound))
        assert int(g["afc_n"][0]) == n == did[0]["K"] and g["toa_n"][0] == 0 and g["quiet"][0] == 0 == m.quiet[0]
        assert abs(int(g["afc_delta"][0]) - did[0]["delta"]) <= bound and abs(step_error(g, m, 0)) <= (bound >> 2) + 1
        trk.destroy()


# ---- many phones --------------------------------------------------------------------------------------------------------
def test_many_phones(rig):
    pkg, sps = rig.pkg, rig.sps
    mb = tf.many_phones(sps)
    trk, m = pair(rig, mb)
    same_state(trk.collect(), m)
    acq = mb["acq"]
    keep = {k: dev(v) for k, v in acq.items()}
    out = pkg.L1AcqOut(n_streams=5, soft_stride=148, d_state=keep["state"].data_ptr(), d_sch_w0=keep["sch_w0"].data_ptr(),
                       d_sch_toa=keep["sch_toa"].data_ptr(), d_omega=keep["omega"].data_ptr(), d_rfn=keep["rfn"].data_ptr())
    trk.seed(out, dev(np.ascontiguousarray(mb["src"], np.int32)))
    m.seed(acq, [int(s) for s in mb["src"]])
    g = trk.collect()
    same_state(g, m)
    assert [int(g["locked"][p]) for p in (63, 64, 127, 128, 199)] == [1, 1, 1, 0, 1] and int(g["fn"][199]) == 0
    before = {p: (m.fn[p], m.pos[p], m.phase[p]) for p in range(200)}
    assert len({m.fn[p] for p in range(200)}) > 50             # the anchors stand on many frames: each is moved by its own distance
    g, rec = rig.slice(trk, m, mb["x"], mb["n0"], mb["fn"], 1)   # (same_state over all 200 inside)
    assert list(g["status"]) == [0, 0, 0]
    for p in range(200):                                       # the anchors of phones without columns moved, unlocked ones did not
        assert m.fn[p] == mb["fn"] + 1 if m.locked[p] else (m.fn[p], m.pos[p], m.phase[p]) == before[p], p
    res, keep2, (row, valid, toa) = group_result(pkg, [(1, 0, 1, 0.25), (5, 1, 1, -0.5), (2, 2, 1, 0.75)], 8, 3)
    quiet = list(m.quiet)
    trk.update(res, mb["fn"])
    m.update(row, valid, toa, mb["fn"])
    g = trk.collect()
    same_state(g, m)
    for p in range(200):
        if p in (0, 199):
            assert (int(g["toa_n"][p]), int(g["quiet"][p])) == ((2, 0) if p == 0 else (1, 0))
        elif m.locked[p]:
            assert g["toa_n"][p] == 0 and g["afc_n"][p] == 0 and g["quiet"][p] == quiet[p] + 1 == 1, p
        else:
            assert g["toa_n"][p] == 0 and g["afc_n"][p] == 0 and g["quiet"][p] == quiet[p], p
    trk.destroy()


# ---- update's integer rules ---------------------------------------------------------------------------------------------
def test_update_edges(rig):
    pkg, sps = rig.pkg, rig.sps
    fn = 51 * 555 + 41                                         # frame 41, then 42 .. 50 of the multiframe
    ue9 = tf.update_edges(sps, 9)
    trk, m = rig.pair(max_frames=9, phone=ue9["phone"], c0=ue9["c0"], toa_gate=1 << 24)
    rng = np.random.default_rng(8300 + sps)
    for p in range(m.P):
        a = (p, 1, fn, int(rng.integers(-10 ** 9, 10 ** 9)), int(rng.integers(0, 1 << 32)), int(rng.integers(0, 1 << 32)))
        trk.set(*a); m.set(*a)
    for F in (1, 9):                                           # 8 slots, then 72, on the one object
        ue = tf.update_edges(sps, F)
        rig.slice(trk, m, np.zeros((ue["n_cols"], 64), np.complex64), 0, fn, F)
        res, keep, (row, valid, toa) = group_result(pkg, ue["rows"], ue["T"], ue["n_cols"])
        trk.update(res, fn)
        did = m.update(row, valid, toa, fn)
        g = trk.collect()
        for p, e in enumerate(ue["expect"]):
            got = dict(S=int(g["toa_sum"][p]), N=int(g["toa_n"][p]), adj=int(g["adj"][p]), K=int(g["afc_n"][p]), delta=int(g["afc_delta"][p]))
            assert got == did[p] and all(got[k] == e[k] for k in e), (sps, F, p, got, did[p], e)
        same_state(g, m)                                       # pos, phase (adj * step modulo 2^32), step, quiet
        assert g["quiet"][-1] == 1 + (F == 9) and not g["quiet"][:-1].any()
        fn = (fn + F) % ltm.HYPER
    trk.destroy()
    mb = tf.afc_case(sps)
    for shift in (0, 8):
        trk, m, g, rec = run(rig, mb, afc_shift=shift)
        grade(g, rec, mb["c0"])
        res, keep, (row, valid, toa) = group_result(pkg, [(3, 0, 0, 0.0)], 8, 2)
        trk.update(res, mb["fn"])
        did = m.update(row, valid, toa, mb["fn"])
        g = trk.collect()
        for p in range(2):
            bound = afc_bound(sps, rec[p])
            delta, err = int(g["afc_delta"][p]), step_error(g, m, p)
            print("sps %d afc_shift %d phone %d: delta %d (model %d, bound %d) step error %d" % (sps, shift, p, delta, did[p]["delta"], bound, err))
            assert g["afc_n"][p] == 1 and np.sign(delta) == mb["sign"][p] == np.sign(did[p]["delta"])
            assert abs(delta - did[p]["delta"]) <= bound and abs(err) <= (bound >> shift) + 1
        assert [int(v) for v in g["pos"]] == m.pos and [int(v) for v in g["phase"]] == m.phase and list(g["quiet"]) == [0, 0]
        trk.destroy()
