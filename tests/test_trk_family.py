"""The tracking family of tests/trk_family.py is what it claims to be (no GPU), on the model alone: the loop members exceed one
round of the slice kernel's grid, the lattice cells are exact in float64 in any order and not in float32, the thresholds
straddle, the overflow cells are where the float64 model and the header disagree, the capacity members fill their records,
and update's promised sums, moves and signs come out of TrkModel.update.  This is what makes a failure of
tests/test_gpu_trk_family.py the kernel's and nobody else's."""
import math

import numpy as np
import pytest

import acq_family as af
import l1_trk_model as ltm
import trk_family as tf

F32 = np.float32


@pytest.fixture(scope="module", params=tf.SPS)
def sps(request):
    return request.param


def model(sps, mb, **kw):
    m = tf.ExactTrk(ltm.TrkModel(af.oracle(sps), mb["phone"], mb["c0"], **dict(mb["kw"], **kw)))
    tf.apply(mb, m)
    return m


def run(sps, mb, **kw):
    m = model(sps, mb, **kw)
    cells, status, rec = m.slice(mb["x"], mb["n0"], mb["fn"], mb["F"])
    return m, cells, status, rec


def test_loops_exceed_one_round():
    """the grid rule (also asserted where the members are built), and on the model at sps 1 the records the members promise"""
    assert tf.grid_x(3, 12) == 96                              # tests/test_gpu_l1trk.py's shapes: a cell per workgroup, no loop
    for n_cols, rounds in ((204, 2), (400, 3)):
        mb = tf.loop_member(1, n_cols)
        gx, rows = tf.grid_x(n_cols, mb["F"]), 8 * mb["F"]
        assert gx == tf.TRK_WG // n_cols == mb["gx"] and 8 * mb["F"] > gx and 80 % gx == 0
        assert [t for t in range(0, rows, gx)] == ([0, 80] if rounds == 2 else [0, 40, 80])     # workgroup 0's cells
        assert len([w for w in range(gx) if w + (rounds - 1) * gx < rows]) == 8                 # workgroups 0 .. 7 go round `rounds` times
        P = len(mb["c0"])
        assert sum(c < 0 for c in mb["c0"]) >= 5 and len(mb["unlocked"]) == 2 and len({a[3] - mb["n0"] for a in mb["anchors"]}) > 30
        if n_cols == 400:
            continue                                           # (the same construction; the GPU test runs its model)
        m, cells, status, rec = run(1, mb)
        for p in range(P):
            if mb["c0"][p] < 0:
                assert rec[p] == [] and mb["promise"][p] is None
            else:
                assert [r["ok"] for r in rec[p]] == mb["promise"][p] and [r["fn"] for r in rec[p]] == [mb["fn"], mb["fn"] + 10]
                for r in rec[p]:                               # placed away from the threshold
                    q = abs(r["C"]) ** 2 / r["E"] ** 2 if r["E"] else 0.0
                    assert (q > 0.9) if r["ok"] else (r["C"].real <= 0 or q < 0.1), (p, r["C"], r["E"])
        assert status == [tf.ltm.UNLOCKED if mb["phone"][c] in mb["unlocked"] else 0 for c in range(n_cols)]


def test_lattice_is_exact(sps):
    L = 142 * sps
    for mb in tf.lattice(sps):
        m, cells, status, rec = run(sps, mb)
        assert np.array_equal(cells[0][0], mb["cell"]) and status == [0], mb["name"]       # expjLookup(0) is exactly (1, 0)
        r = rec[0][0]
        y = mb["cell"].astype(np.complex128)
        n = 3 * sps + np.arange(L)
        d = y[n + sps] * np.conj(y[n]) * -1j
        e = 0.5 * (np.abs(y[n]) ** 2 + np.abs(y[n + sps]) ** 2)
        assert np.array_equal(r["terms"][0], d.real) and np.array_equal(r["terms"][1], d.imag) and np.array_equal(r["terms"][2], e)
        assert tf.lattice_check(r["terms"])
        for v in r["terms"]:                                   # any order: the same float64 sum
            assert math.fsum(v) == float(np.sum(v)) == float(np.sum(v[::-1])) == float(np.sum(np.sort(v)))
        e = mb["expect"]
        assert r["C"] == e["C"] and r["E"] == e["E"] and r["ok"] == e["ok"] and r["finite"], (mb["name"], r["C"], r["E"])
    by = {mb["name"]: mb for mb in tf.lattice(sps)}
    assert by["plateau"]["expect"]["C"] == by["plateau"]["expect"]["E"] == L
    assert [by["border " + k]["expect"]["C"] for k in ("constant", "alternating", "reversed tone")] == [-1j * L, 1j * L, -L]


def test_mixed_catches_a_float32_sum(sps):
    mb = [mb for mb in tf.lattice(sps) if mb["name"] == "mixed"][0]
    r = run(sps, mb)[3][0][0]
    for v, exact in ((r["terms"][0], r["C"].real), (r["terms"][2], r["E"])):
        for order in (v, v[::-1]):
            acc = F32(0)
            for t in order.astype(F32):
                acc = F32(acc + t)
            assert float(acc) != exact
        assert float(F32(exact)) != exact                      # no float32 holds the sum at all


def test_thresholds_straddle(sps):
    by = {mb["name"]: mb for mb in tf.lattice(sps)}
    for name in ("plateau", "mixed", "threshold"):
        mb = by[name]
        C, E = mb["expect"]["C"], mb["expect"]["E"]
        q = (C.real * C.real + C.imag * C.imag) / (E * E)
        (lo, hi), = mb["pairs"]
        assert lo.dtype == hi.dtype == F32 and np.nextafter(lo, F32(np.inf)) == hi and float(lo) < q <= float(hi), name
        assert run(sps, mb, fcch_thresh=lo)[3][0][0]["ok"] is True and run(sps, mb, fcch_thresh=hi)[3][0][0]["ok"] is False
    assert by["plateau"]["pairs"][0] == (np.nextafter(F32(1), F32(0)), F32(1))                 # refused at 1.0: strict >


def test_overflow_is_where_the_definitions_disagree(sps):
    big, small = tf.overflow(sps)
    m, cells, status, rec = run(sps, big)
    r = rec[0][0]
    assert np.array_equal(cells[0][0], big["cell"]) and np.isfinite(cells[0][0].view(F32)).all()
    assert not r["finite"] and not r["ok"] and r["E"] == math.inf == big["expect"]["E"]
    f64 = m.fcch(cells[0][0])
    assert f64["ok"] and np.isfinite(f64["E"])                 # the float64 model accepts it: why the member exists
    m, cells, status, rec = run(sps, small)
    r = rec[0][0]
    assert np.array_equal(cells[0][0], small["cell"]) and cells[0][0].all()
    assert r["finite"] and not r["ok"] and r["E"] == 0.0 and r["C"] == 0
    f64 = m.fcch(cells[0][0])
    assert f64["ok"] and f64["E"] > 0


def test_nonfinite_places(sps):
    o = af.oracle(sps)
    for variant in range(8):
        mb = tf.nonfinite(o, variant)
        bad = ~np.isfinite(mb["x"].view(F32).reshape(2, -1, 2))
        assert bad.sum() == 50 and not (bad[..., 0] & bad[..., 1]).any()       # 25 a column, one component each
        if variant:
            continue
        m, cells, status, rec = run(sps, mb)
        for c, t, i, kind in mb["places"]:
            v = cells[c][t][i]
            if tf.KINDS[kind][0] & 0x007fffff:                 # a NaN: both components, with the sample's sign in both
                w = np.array([v], np.complex64).view(np.uint32)
                assert (w & 0x7fffffff == 0x7fc00000).all(), (c, t, i, w)
            else:
                assert np.isinf(v.real) and np.isinf(v.imag)
        assert sum(int((~np.isfinite(np.asarray(cells[c][t]).view(F32))).sum()) for c in range(2) for t in range(16)) == 100
        for p in range(2):
            assert not rec[p][0]["finite"] and not rec[p][0]["ok"]


def test_capacity_fills():
    for mb, filled in zip(tf.capacity(), (6, 5, 2)):
        m, cells, status, rec = run(1, mb, afc_shift=2)
        assert len(rec[0]) == filled == len(mb["frames"]) and mb["cap"] == mb["max_frames"] // 10 + 1 and status == [0]
        assert (filled == mb["cap"]) == (mb["max_frames"] != 21)
        assert [r["fn"] for r in rec[0]] == [(mb["fn"] + f) % ltm.HYPER for f in mb["frames"]] and all(r["ok"] for r in rec[0])
        E = [r["E"] for r in rec[0]]
        assert all(b > 1.3 * a for a, b in zip(E, E[1:]))      # no two alike: a permutation shows


def test_many_phones_classes():
    mb = tf.many_phones(1)
    m = model(1, mb)
    before = [(m.locked[p], m.fn[p], m.pos[p], m.step[p], m.phase[p]) for p in range(200)]
    m.seed(mb["acq"], mb["src"])
    after = [(m.locked[p], m.fn[p], m.pos[p], m.step[p], m.phase[p]) for p in range(200)]
    assert after[64] == before[64] and after[127] == before[127] and before[64][0] == before[127][0] == 1
    assert after[128][0] == 0 and after[128][1:] == before[128][1:] and before[128][0] == 1
    assert after[63] == (1, 78, 5013 + 1250, int(np.rint(float(F32(0.03)) * ltm.K_TURN)), 0)
    assert after[199][:3] == (1, 0, 20000 + 1250) and abs(after[199][3] - (1 << 31)) < 100
    assert all(not before[p][0] for p in mb["unlocked"]) and {int(s) for s in mb["src"]} == {-9, -1, 0, 1, 2, 3, 4, 5}
    cells, status, rec = m.slice(mb["x"], mb["n0"], mb["fn"], 1)
    assert status == [0, 0, 0] and len(rec[0]) == len(rec[199]) == 0


def test_update_edges_promises(sps):
    for F in (1, 9):
        ue = tf.update_edges(sps, F)
        m = ltm.TrkModel(af.oracle(sps), ue["phone"], ue["c0"], toa_gate=1 << 24)
        for p in range(m.P):
            m.set(p, 1, 42, 0, 0x1234567 * (p + 1), 99 * p)
        m.slice(np.zeros((ue["n_cols"], 64), np.complex64), 0, 42, F)
        row = np.full((ue["T"], ue["n_cols"]), -1, np.int32)
        toa = np.array([r[3] for r in ue["rows"]], F32)
        for i, (t, c, v, d) in enumerate(ue["rows"]):
            row[t, c] = i
        pos = list(m.pos)
        did = m.update(row, np.ones(len(toa), np.uint8), toa, 42)
        for p, e in enumerate(ue["expect"]):
            assert all(did[p][k] == e[k] for k in e), (sps, F, p, did[p], e)
            assert m.pos[p] - pos[p] == did[p]["adj"] and m.quiet[p] == (did[p]["N"] == 0)
        assert [e["adj"] for e in ue["expect"][8:12]] == [-1, 0, 1, 2] and did[-1] == dict(S=0, N=0, adj=0, K=0, delta=0)
        assert did[-2]["N"] == (60 if F == 9 else 8) and any(t >= 64 for t, _, _, _ in ue["rows"]) == (F == 9)
    mb = tf.afc_case(sps)
    for shift in (0, 8):
        m, cells, status, rec = run(sps, mb, afc_shift=shift)
        step = list(m.step)
        did = m.update(np.full((8, 2), -1, np.int32), np.zeros(1, np.uint8), np.zeros(1, F32), mb["fn"])
        for p in range(2):
            assert did[p]["K"] == 1 and np.sign(did[p]["delta"]) == mb["sign"][p] and abs(did[p]["delta"]) > 1 << 18
            assert m.step[p] == (step[p] + (did[p]["delta"] >> shift)) & ltm.M32


def test_terms32_agree_with_the_float64_model(sps):
    rng = np.random.default_rng(8200 + sps)
    m = ltm.TrkModel(af.oracle(sps), [0], [0])
    for amp in (1e-3, 1.0, 1e4):
        y = tf.noise32(rng, 157 * sps, amp)
        f64, ex = m.fcch(y), tf.fcch_exact(y, sps, 0.5)
        assert abs(ex["C"] - f64["C"]) <= f64["bound_c"] and abs(ex["E"] - f64["E"]) <= f64["bound_e"] and ex["ok"] == f64["ok"]
        assert ex["bound_c"] < 1e-6 * f64["bound_c"] and ex["bound_e"] < 1e-6 * f64["bound_e"]     # the sharper grading
