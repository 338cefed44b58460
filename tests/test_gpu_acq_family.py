"""GPU tests of mobile-side acquisition (include/trxsig_l1acq.h) on the adversarial family of tests/acq_family.py, at sps 1, 2
and 4 -- what tests/test_gpu_l1acq.py's tolerance cannot see:

  ties        lattice streams, on which every float32 sum of stage 1 is exact in any order, so k, m, C and E are compared with ==:
              the smallest k of the largest m through a thread's loop, a wave's lanes, the merge of the waves and the pick's lane
              loop and shuffle tree; m > fcch_thresh at equality; the half-plane border Re C == 0
  angles      63 tones round the circle: every branch of the kernel's atan2, both half planes
  sps 2       the template instance nothing else runs: every test here, and the 16 truth cases
  range       offsets of +-0.2 and +-0.24 cycle / symbol (a phase chain of 260 rad in the shift), neighbours 60 and 90 dB up
  boundaries  state bit 2 at w0 + 172 sps == N and one sample short of it; detect_sch batches of 63, 64, 65 and 257 windows into
              arrays one row longer
  reuse       one object through a large search, smaller ones, a workspace growth, long windows and then short ones in the same
              rows, and the first search again: everything equals what a fresh object answers

tests/test_acq_family.py proves on the CPU that the family is what it claims; the tolerances are the header's."""
import numpy as np
import pytest

import _pkg
import acq_family as af
import l1_acq_model as am
from test_gpu_l1acq import Rig, check_stage1, check_stage2, dev

pytestmark = pytest.mark.gpu
F32 = np.float32


@pytest.fixture(scope="module")
def pkg():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return _pkg.load()


@pytest.fixture(scope="module")
def tx():
    return af.fec_tx()


@pytest.fixture(scope="module", params=af.SPS)
def rig(request, pkg):
    return Rig(pkg, request.param)


STAGE1 = ("fcch_k", "fcch_metric", "fcch_c", "fcch_e", "arg", "omega")


def same(a, b, what, keys=None):
    for key in keys or a:
        assert np.array_equal(a[key], b[key]), (what, key, a[key], b[key])


# ---- stage 1 with == -------------------------------------------------------------------------------------------------------
def test_lattice_exact(rig):
    sps = rig.sps
    members = af.lattice_members(sps)
    g = rig.search([mb["x"] for mb in members])                # one call carries them all
    bad = []
    for i, mb in enumerate(members):
        lm = mb["model"]
        k, m, C, E, arg = int(g["fcch_k"][i]), g["fcch_metric"][i], g["fcch_c"][i], g["fcch_e"][i], g["arg"][i]
        want = np.arctan2(float(lm["C"].imag), float(lm["C"].real))
        ok = (k == lm["k"] and m == lm["m"] and C == lm["C"] and E == lm["E"] and abs(float(arg) - want) <= 2e-6
              and g["omega"][i] == F32(-arg / F32(sps)) and bool(g["state"][i] & 1) == bool(lm["m"] > 0.5))
        print("sps %d %-40s k %6d (%6d)  m %.8f (%.8f)  C %s (%s)  E %s (%s)  arg %.7f (%.7f)  state %d%s"
              % (sps, mb["name"], k, lm["k"], m, lm["m"], C, lm["C"], E, lm["E"], arg, want, g["state"][i], "" if ok else "   <-- WRONG"))
        if not ok:
            bad.append(mb["name"])
    assert not bad, (sps, bad)


def test_threshold_is_strict(rig):
    """state bit 1 iff m > fcch_thresh: clear at fcch_thresh == m, set one float32 step below"""
    sps = rig.sps
    for mb in af.exact_m_members(sps):
        m = mb["model"]["m"]
        at, below = rig.search([mb["x"]], fcch_thresh=float(m)), rig.search([mb["x"]], fcch_thresh=float(np.nextafter(m, F32(0))))
        what = (sps, mb["name"], m, at["state"][0], below["state"][0])
        assert at["fcch_metric"][0] == m and below["fcch_metric"][0] == m and at["fcch_k"][0] == mb["model"]["k"], what
        assert at["state"][0] == 0 and not at["soft"].any(), what
        assert below["state"][0] & 1, what


def test_every_angle(rig):
    sps = rig.sps
    L = am.fcch_len(sps)
    th, xs = af.angle_sweep(sps)
    g = rig.search(xs)
    for i, (t, x) in enumerate(zip(th, xs)):
        what = "sps %d theta %+.4f" % (sps, t)
        k, m64 = check_stage1(g, i, x, sps, what)
        C64, E64, _ = am.fcch_metric64(x, sps)
        arg = float(g["arg"][i])
        # the header's bound on C turned into an angle, plus the header's bound on the angle
        bound = 2 * (L + 8) * 2.0 ** -24 * E64[k] / abs(C64[k]) + 2e-6
        print("%s: arg %+.7f, angle(C64[k]) %+.7f, |d| %.2e (bound %.2e)" % (what, arg, np.angle(C64[k]), abs(arg - np.angle(C64[k])), bound))
        assert abs(arg - np.angle(C64[k])) <= bound, what
        if abs(t) > np.pi / 2:
            assert k == 0 and g["fcch_metric"][i] == 0 and g["state"][i] == 0, what
        else:
            assert g["fcch_metric"][i] > 0.99 and g["state"][i] & 1, what


# ---- far offsets, dynamic range, sps 2 ---------------------------------------------------------------------------------------
def test_far_offsets_and_dynamic_range(rig, tx):
    sps = rig.sps
    far = af.far_offset(sps)
    g = rig.search([x for _, x in far])
    for i, (f, x) in enumerate(far):
        what = "sps %d f %+.2f" % (sps, f)
        check_stage1(g, i, x, sps, what)
        check_stage2(rig, tx, g, i, x, what)
        assert g["state"][i] == af.FAR_OFFSET_STATE[(sps, f)], (what, g["state"][i])
        assert abs(float(g["arg"][i]) / (2 * np.pi) - f) <= 2e-3, (what, g["arg"][i])
    dyn = af.dynamic_range(sps)
    g = rig.search([x for _, x in dyn])
    for i, (db, x) in enumerate(dyn):
        what = "sps %d neighbours %d dB up" % (sps, db)
        check_stage1(g, i, x, sps, what)
        check_stage2(rig, tx, g, i, x, what)
        assert g["fcch_metric"][i] > 0.9 and g["state"][i] & 1, what


def test_truth_at_sps2(pkg, tx):
    """tests/test_gpu_l1acq.py's truth test at the sps it leaves out"""
    sps = 2
    rig = Rig(pkg, sps)
    cases = am.truth_cases(sps)
    built = [am.truth_stream(rig.o, tx, c) for c in cases]
    g = rig.search([x for x, _ in built])
    assert len(cases) == 16 and af.TRUTH2_STATE15 == 16       # the model reaches state 15 on every one
    worst_t = worst_f = 0.0
    for i, (case, (x, sch)) in enumerate(zip(cases, built)):
        check_stage1(g, i, x, sps, "sps 2 truth %d" % i)
        r = check_stage2(rig, tx, g, i, x, "sps 2 truth %d" % i)
        assert g["state"][i] == 15 and r["state"] == 15, (i, case, g["state"][i])
        at = int(g["sch_w0"][i]) + float(g["sch_toa"][i])
        fn, true = min(sch, key=lambda s: abs(s[1] - at))
        assert (int(g["bsic"][i]), int(g["rfn"][i])) == (case["bsic"], fn), (i, case)
        worst_t = max(worst_t, abs(at - true))
        worst_f = max(worst_f, abs(float(g["arg"][i]) / (2 * np.pi) - case["f"]))
    print("sps 2: worst timing error %.3f sample, worst frequency error %.2e cycle / symbol" % (worst_t, worst_f))
    assert worst_t <= 0.25 and worst_f <= 2e-3


# ---- boundaries --------------------------------------------------------------------------------------------------------------
def test_window_boundary(rig, tx):
    """state bit 2 iff [w0, w0 + 172 sps) lies inside the stream: the stream that ends with the window's last sample, and the one
    that ends one sample earlier"""
    sps = rig.sps
    x = af.far_offset(sps)[1][1]
    whole = rig.search([x])
    end = int(whole["sch_w0"][0]) + 172 * sps
    assert whole["state"][0] == 15 and end < len(x)
    fits, short = rig.search([x[:end]]), rig.search([x[:end - 1]])
    r = check_stage2(rig, tx, fits, 0, x[:end], "sps %d the window ends the stream" % sps)
    assert fits["state"][0] & 2 and r["state"] == 15
    same(fits, whole, "the window ends the stream")            # the same window: the same everything
    assert short["state"][0] == 1 and not short["soft"].any() and short["sch_ptm"][0] == 0 and short["sch_amp"][0] == 0
    same(short, whole, "one sample short", STAGE1 + ("sch_w0",))


def detect(rig, acq, dX, off, ln, om, extra=0):
    """detect_sch into arrays of len(off) + extra rows and 150 columns, all pre-filled with 7 -> host arrays"""
    import torch
    R = len(off) + extra
    flags, hard = torch.full((R,), 7, dtype=torch.uint8).cuda(), torch.full((R, 150), 7, dtype=torch.uint8).cuda()
    amp, toa, ptm, soft = (torch.full(s, 7.0).cuda() for s in ((R, 2), (R,), (R,), (R, 150)))
    acq.detect_sch(dX, dev(np.asarray(off, np.int32)), dev(np.asarray(ln, np.int32)), flags, amp, toa, soft,
                   omega=dev(np.asarray(om, np.float32)), ptm=ptm, hard=hard)
    rig.ctx.synchronize()
    return dict(flags=flags.cpu().numpy(), amp=amp.cpu().numpy().view(np.complex64).ravel(), toa=toa.cpu().numpy(),
                ptm=ptm.cpu().numpy(), soft=soft.cpu().numpy(), hard=hard.cpu().numpy())


def test_detect_sch_partial_blocks(rig, tx):
    """batches that end inside, at the end of and just past a 64-thread block of the verdict: rows below B equal the model, row B
    and the columns past 148 are not touched"""
    sps, pkg = rig.sps, rig.pkg
    rng = np.random.default_rng(5100 + sps)
    clean, slots = am.build_stream(rig.o, tx, rng, 10, 2, 33, extra_slots=2)
    f = 0.04
    x = am.impair(clean, rng, sps, 0, 3, f, 0.7 + 0.2j, 20.0)
    x0 = am.impair(clean, rng, sps, 0, 5, 0.0, 1.1j, 20.0)     # no offset: the window whose shift is zero
    X = np.concatenate([x, x0])
    s = am.first(slots, "sch")[1]
    om = F32(-2 * np.pi * f / sps)
    five = [(s - 12 * sps, 172 * sps, om),                     # detected
            (s + 300 * sps, 172 * sps, om),                    # no SCH: below the threshold
            (s + 40 * sps, 2 * sps, om),                       # bogus: numRms < 2
            (s, 256 * sps + 1, om),                            # bad length
            (len(x) + s - 12 * sps, 172 * sps, F32(0))]        # unshifted
    model = [rig.det.detect(X[o:o + n], w) for o, n, w in five]   # once per distinct window
    assert [int(m["flags"]) for m in model] == [2, 0, 0, 128, 2]
    assert model[1]["ptm"] > 0 and model[2]["ptm"] == 0 and model[3]["ptm"] == 0
    dX = dev(X.view(np.float32))
    for B in (63, 64, 65, 257):
        pick = (np.arange(B) * 3 + B) % 5
        acq = pkg.L1Acq(rig.ctx, 1, 1000)
        got = detect(rig, acq, dX, [five[p][0] for p in pick], [five[p][1] for p in pick], [five[p][2] for p in pick], extra=1)
        acq.destroy()
        for b, p in enumerate(pick):
            m, what = model[p], "sps %d B %d row %d (window %d)" % (sps, B, b, p)
            assert got["flags"][b] == m["flags"] and got["amp"][b] == m["amp"] and got["toa"][b] == m["toa"] and got["ptm"][b] == m["ptm"], \
                (what, got["flags"][b], m["flags"], got["amp"][b], m["amp"], got["toa"][b], m["toa"], got["ptm"][b], m["ptm"])
            assert np.array_equal(got["soft"][b, :148], m["soft"]), what
            assert np.array_equal(got["hard"][b, :148], (m["soft"] > 0.5).astype(np.uint8)), what
        assert got["flags"][B] == 7 and got["amp"][B] == 7 + 7j and got["toa"][B] == 7 and got["ptm"][B] == 7, (sps, B)
        assert (got["soft"][B] == 7).all() and (got["hard"][B] == 7).all(), (sps, B)
        assert (got["soft"][:, 148:] == 7).all() and (got["hard"][:, 148:] == 7).all(), (sps, B)


# ---- reuse -------------------------------------------------------------------------------------------------------------------
def test_reuse_equals_fresh(rig, tx):
    """One object through: a search over the 16 truth streams; a search over two shorter streams (one found, one without a
    frequency burst) and one over streams too short for a window (one search has one length, so they are two calls); detect_sch
    on 2 max_streams + 1 windows of 256 sps, which makes the workspace grow; the same rows again with windows of 150 sps + 1;
    the first search again.  Every array equals what a fresh object answers."""
    sps, pkg = rig.sps, rig.pkg
    L = am.fcch_len(sps)
    cases = am.truth_cases(sps)
    built = [am.truth_stream(rig.o, tx, c) for c in cases]
    streams = [x for x, _ in built]
    acq = pkg.L1Acq(rig.ctx, len(streams), len(streams[0]))
    first = rig.search(streams, acq=acq)
    same(first, rig.search(streams), "the first search")
    assert (first["state"] == 15).all()

    found = af.far_offset(sps)[0][1]
    quiet = [x for name, x in am.negative_streams(rig.o, tx, sps) if name == "no_fcch"][0]
    n = min(len(found), len(quiet))
    pair = [found[:n], quiet[:n]]
    fresh = rig.search(pair)
    assert fresh["state"].tolist() == [15, 0] and not fresh["soft"][1].any()
    same(rig.search(pair, acq=acq), fresh, "two shorter streams after sixteen long ones")
    rng = np.random.default_rng(5200 + sps)
    tiny = [(rng.standard_normal(L + sps - 1) + 1j * rng.standard_normal(L + sps - 1)).astype(np.complex64) for _ in range(3)]
    fresh = rig.search(tiny)
    assert (fresh["fcch_k"] == -1).all() and not fresh["state"].any() and not fresh["soft"].any()
    same(rig.search(tiny, acq=acq), fresh, "streams without a window after streams with one")

    x, sch = built[0]
    dX = dev(x.view(np.float32))
    B = 2 * len(streams) + 1
    at = int(round(sch[0][1]))
    off = (np.arange(B) * 977 * sps) % (len(x) - 256 * sps)
    off[0], off[B - 1] = at - 40 * sps, int(round(sch[1][1])) - 100 * sps
    om = np.full(B, -2 * np.pi * cases[0]["f"] / sps, np.float32)
    other = pkg.L1Acq(rig.ctx, 1, 1000)
    long_ = detect(rig, acq, dX, off, np.full(B, 256 * sps), om)
    same(long_, detect(rig, other, dX, off, np.full(B, 256 * sps), om), "long windows after a growth")
    assert long_["flags"][0] == 2 and long_["flags"][B - 1] == 2 and (long_["flags"] == 0).sum() >= B // 2
    off[0], off[B - 1] = at - 1, int(round(sch[1][1])) - 1
    short = detect(rig, acq, dX, off, np.full(B, 150 * sps + 1), om)
    other.destroy()
    other = pkg.L1Acq(rig.ctx, 1, 1000)
    same(short, detect(rig, other, dX, off, np.full(B, 150 * sps + 1), om), "short windows in rows that long ones filled")
    other.destroy()
    assert short["flags"][0] == 2 and short["flags"][B - 1] == 2
    m = rig.det.detect(x[off[0]:off[0] + 150 * sps + 1], om[0])
    assert short["ptm"][0] == m["ptm"] and short["toa"][0] == m["toa"] and np.array_equal(short["soft"][0, :148], m["soft"])

    same(rig.search(streams, acq=acq), first, "the first search again")
    acq.destroy()
