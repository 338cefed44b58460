"""GPU parity of detectRACHBurst + demodulateBurst on the adversarial access-burst family of tests/rach_family.py: far and
near ties of the correlation maximum, chosen far-contender counts on both sides of the detector's limits (6: two bursts share
the exact pass; 38: the wave works alone), peaks at both ends of the window, truncated and empty valleys, flat inputs, extreme
scales and ragged / refused lengths beside good bursts.  Every comparison is IEEE == against the CPU oracle (flags, amplitude,
TOA, avgPwr, 148 soft bits, hard bits); tests/test_rach_family.py proves on the CPU that the family holds what it claims."""
import functools

import numpy as np
import pytest

import _pkg
import rach_family as rf
from test_gpu_soft_tolerance import grade
from util import GpuBatch, assert_veq

pytestmark = pytest.mark.gpu

SPS = (1, 2, 4)
F_ENERGY, F_DETECT, F_BADLEN = 1, 2, 128


@pytest.fixture(scope="module")
def pkg():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    p = _pkg.load()
    assert (p.F_ENERGY, p.F_DETECT, p.F_BADLEN) == (F_ENERGY, F_DETECT, F_BADLEN)
    return p


def make_ctx(pkg, monkeypatch, sps, route):
    """Routes 1 and 2 from the product library, route 0 (exact at every lag) from the tuning build."""
    monkeypatch.setenv("TRXSIG_RACH_VARIANT", str(route))
    t = pkg.TrxSig(sps, 0, tuning=(route == 0))
    t.use_torch_stream()
    return t


@functools.lru_cache(maxsize=None)
def expected(sps, thresh=5.0, energy_thresh=-1.0):
    """What the library must answer for the whole family, per burst, from the oracle: the status byte, amp, TOA, avgPwr over the
    first 20 * sps samples (energyDetect's window for access bursts, include/trxsig.h), soft and hard bits.  A refused burst:
    F_BADLEN and zeros; a burst under the energy gate: no flag, its avgPwr, zeros otherwise (the correlator is not run).
    Soft bits past a short burst's last symbol are outside the library's contract (nsoft <= length / sps) and are masked."""
    info = rf.family_info(sps)
    o = rf.oracle(sps)
    x, off, length, acc = info["x"], info["off"], info["length"], info["accepted"]
    B = len(off)
    e = dict(flags=np.zeros(B, np.uint8), amp=np.zeros(B, np.complex64), toa=np.zeros(B, np.float32),
             pwr=np.zeros(B, np.float32), soft=np.zeros((B, 148), np.float32), valid=np.zeros((B, 148), bool))
    e["flags"][~acc] = F_BADLEN
    run = []
    for i in np.flatnonzero(acc):
        passed, e["pwr"][i] = o.energy_detect(x[off[i]:off[i] + length[i]], 20 * sps, max(energy_thresh, 0.0))
        if energy_thresh < 0.0 or passed:
            e["flags"][i] = F_ENERGY
            run.append(i)
    run = np.array(run)
    ok, amp, toa, soft = o.rach_batch(x, off[run], length[run], thresh=thresh, nthreads=8)
    e["flags"][run] |= (ok.astype(np.uint8) * F_DETECT)
    e["amp"][run] = amp; e["toa"][run] = toa; e["soft"][run] = soft
    e["valid"][:] = np.arange(148)[None, :] < (length // sps)[:, None]
    e["soft"][~e["valid"]] = 0
    e["hard"] = (e["soft"] > 0.5).astype(np.uint8)
    for v in e.values():
        v.setflags(write=False)
    return e


def run(t, x, off, length, **kw):
    gb = GpuBatch(x, off, length, nsoft=148, stride=148)
    kw.setdefault("energy_thresh", -1.0)
    t.detect_demod_rach(gb.x, gb.off, gb.len, gb.flags, gb.amp, gb.toa, gb.soft, avgpwr=gb.pwr, hard=gb.hard, **kw)
    return gb.results()


def check(r, e, what, sel=None, soft=True):
    """r: the library's results for the bursts `sel` of the family (default: all, in order); e: expected(...)."""
    sel = np.arange(len(e["flags"])) if sel is None else np.asarray(sel)
    assert_veq(r["flags"], e["flags"][sel], what + ": status byte")
    assert_veq(r["amp"], e["amp"][sel], what + ": amp")
    assert_veq(r["toa"], e["toa"][sel], what + ": toa")
    assert_veq(r["pwr"], e["pwr"][sel], what + ": avgPwr")
    v = e["valid"][sel]
    if soft:
        assert_veq(np.where(v, r["soft"], 0), e["soft"][sel], what + ": soft bits")
    assert_veq(np.where(v, r["hard"], 0), e["hard"][sel], what + ": hard bits")
    quiet = (e["flags"][sel] & F_DETECT) == 0                   # not detected (refused and gated included): zeros, all 148
    assert not r["soft"][quiet].any() and not r["hard"][quiet].any(), what + ": an undetected burst has soft bits"


def same(a, b, what):
    for k in ("flags", "amp", "toa", "pwr", "soft", "hard"):
        assert_veq(a[k], b[k], what + ": " + k)


@pytest.mark.parametrize("sps", SPS)
@pytest.mark.parametrize("route", [0, 1, 2])
def test_family_on_every_route(pkg, monkeypatch, sps, route):
    x, off, length, cls = rf.family(sps)
    r = run(make_ctx(pkg, monkeypatch, sps, route), x, off, length)
    check(r, expected(sps), "route %d sps %d" % (route, sps))
    assert ((r["flags"] & F_DETECT) != 0).sum() > 40            # (the family is not a batch of misses)


def _beside(info, heavy_first):
    """A permutation of the family that puts every burst that cannot share its workgroup's exact pass (7 or more far contenders,
    the exact-everywhere kinds, the refused ones) at an even (heavy_first) or odd index, beside an ordinary burst."""
    cls, facts, acc = info["cls"], info["facts"], info["accepted"]
    heavy, ordinary = [], []
    for i in range(len(cls)):
        f = facts[i]
        if not acc[i] or cls[i] in ("contend_many", "flat") or len(f["far"]) > rf.PAIR_LIMIT or f["argmax"] < 0:
            heavy.append(i)
        else:
            ordinary.append(i)
    assert len(heavy) >= 30 and len(ordinary) >= len(heavy)
    perm = []
    for h, o in zip(heavy, ordinary):
        perm += [h, o] if heavy_first else [o, h]
    perm += ordinary[len(heavy):]
    assert sorted(perm) == list(range(len(cls)))
    return np.array(perm)


@pytest.mark.parametrize("sps", SPS)
@pytest.mark.parametrize("route", [1, 2])
def test_position_independence(pkg, monkeypatch, sps, route):
    """A burst's neighbour decides which code computes it (route 2's paired exact pass): per-burst results are the same, and the
    oracle's, as built, beside a burst that breaks the pairing (at either index), in a batch of odd length and alone."""
    info = rf.family_info(sps)
    x, off, length = info["x"], info["off"], info["length"]
    B = len(off)
    e = expected(sps)
    t = make_ctx(pkg, monkeypatch, sps, route)
    base = run(t, x, off, length)
    check(base, e, "as built")
    for first in (True, False):
        perm = _beside(info, first)
        r = run(t, x, off[perm], length[perm])
        check(r, e, "heavy bursts at %s indices" % ("even" if first else "odd"), sel=perm)
        same(r, {k: v[perm] for k, v in base.items()}, "permuted against as built")
    for odd in (B - 1 if B % 2 == 0 else B - 2, 3):
        r = run(t, x, off[:odd], length[:odd])
        check(r, e, "B = %d" % odd, sel=np.arange(odd))
        same(r, {k: v[:odd] for k, v in base.items()}, "odd B against as built")
    cls = info["cls"]
    alone = [int(np.flatnonzero(cls == c)[k]) for c, k in (("far_tie", 6), ("near_tie", 2), ("contend_k", 6), ("contend_k", 12),
                                                          ("contend_many", 0), ("flat", 0), ("edge_late", 9), ("edge_early", 6))]
    alone.append(int(np.flatnonzero(~info["accepted"])[0]))
    for i in alone:
        r = run(t, x, off[i:i + 1], length[i:i + 1])
        check(r, e, "B = 1, member %d (%s)" % (i, cls[i]), sel=[i])


@pytest.mark.parametrize("sps", SPS)
@pytest.mark.parametrize("route", [1, 2])
def test_thresholds(pkg, monkeypatch, sps, route):
    """rach_decide judges the detect flag from an approximate valley unless the threshold falls inside its error bar: the whole
    family at thresholds from 1 to 100, and thresholds ON members' own peak-to-valley ratios (and one ulp either side)."""
    info = rf.family_info(sps)
    x, off, length, cls, facts = info["x"], info["off"], info["length"], info["cls"], info["facts"]
    t = make_ctx(pkg, monkeypatch, sps, route)
    o = rf.oracle(sps)
    seen = set()
    for thr in (1.0, 5.0, 13.0, 30.0, 100.0):
        e = expected(sps, thr)
        check(run(t, x, off, length, detect_thresh=thr), e, "threshold %g" % thr)
        seen.add(int(((e["flags"] & F_DETECT) != 0).sum()))
    assert len(seen) >= 3, "the family does not spread over the thresholds: %r" % (seen,)

    def live(i):
        return facts[i] is not None and facts[i]["peak_to_mean"] > 0
    pick = []
    tr = [i for i in np.flatnonzero(cls == "edge_late") if live(i) and 2 <= facts[i]["num_samples"] < facts[i]["full"]]
    assert len(tr) >= 3
    pick += [int(i) for i in tr[:3]]
    later = []
    for _, i0, cnt, lags in [s for s in info["sweeps"] if s[0] == "far_tie"]:
        for lag in lags:                                        # both sides of the flip, where that side has a valley at all
            side = [i for i in range(i0, i0 + cnt) if facts[i]["argmax"] == lag and live(i)]
            side = side[-1:] if lag == lags[0] else side[:1]    # the member next to the flip
            pick += side
            later += [lag == lags[1]] * len(side)
    assert later.count(True) >= 2 and later.count(False) >= 2
    pools = [[int(i) for i in np.flatnonzero(cls == c) if live(i) and i not in pick] for c in rf.CLASSES + ("noisy",)]
    k = 0
    while len(pick) < 24:
        pool = pools[k % len(pools)]
        if pool:
            pick.append(pool.pop(len(pool) // 2))
        k += 1
    assert len(pick) == 24 and len({cls[i] for i in pick}) >= 8
    for i in pick:
        xi = x[off[i]:off[i] + length[i]]
        p = np.float32(facts[i]["peak_to_mean"])
        for thr in (p, np.nextafter(p, np.float32(0)), np.nextafter(p, np.float32(1e30))):
            r = run(t, xi, [0], [length[i]], detect_thresh=float(thr))
            want = o.detect_rach(xi, thresh=float(thr))["ok"]
            assert bool(r["flags"][0] & F_DETECT) == want, (i, cls[i], float(thr))
            assert want == (p > thr)


@pytest.mark.parametrize("sps", SPS)
def test_energy_gate(pkg, monkeypatch, sps):
    """energyDetect over the first 20 * sps samples with a threshold between the family's energies: flag and avgPwr are the
    oracle's, a gated burst reports zeros, and its ungated neighbour in the workgroup is untouched."""
    info = rf.family_info(sps)
    x, off, length, acc = info["x"], info["off"], info["length"], info["accepted"]
    pw = np.unique(expected(sps)["pwr"][acc])
    pw = pw[pw > 0]
    mid = np.arange(len(pw) // 4, 3 * len(pw) // 4)             # the widest gap between neighbours in the middle half
    k = int(mid[np.argmax(pw[mid + 1].astype(np.float64) / pw[mid])])
    a, b = float(pw[k]), float(pw[k + 1])
    thr = float(np.float32(0.5 * (np.sqrt(a) + np.sqrt(b))))
    assert np.float32(a) < np.float32(thr) * np.float32(thr) < np.float32(b)
    e = expected(sps, 5.0, thr)
    gated = acc & (e["flags"] == 0)
    assert gated.sum() >= 30 and (acc & ~gated).sum() >= 30
    t = make_ctx(pkg, monkeypatch, sps, 2)
    r = run(t, x, off, length, energy_thresh=thr)
    check(r, e, "energy gate at %g" % thr)
    assert not r["amp"][gated].any() and not r["toa"][gated].any() and not r["soft"][gated].any()
    free = run(t, x, off, length)
    idx = np.arange(len(off))
    beside = acc & ~gated & (gated | ~acc)[np.minimum(idx ^ 1, len(off) - 1)]
    assert beside.sum() >= 10
    same({k: v[beside] for k, v in r.items()}, {k: v[beside] for k, v in free.items()}, "ungated beside gated")
    check(run(make_ctx(pkg, monkeypatch, sps, 1), x, off, length, energy_thresh=thr), e, "energy gate, route 1")


@pytest.mark.parametrize("sps", SPS)
def test_refusals(pkg, monkeypatch, sps):
    info = rf.family_info(sps)
    x, off, length, acc = info["x"], info["off"], info["length"], info["accepted"]
    e = expected(sps)
    for route in (1, 2):
        r = run(make_ctx(pkg, monkeypatch, sps, route), x, off, length)
        bad = np.flatnonzero(~acc)
        assert len(bad) >= 5
        assert_veq(r["flags"][bad], np.full(len(bad), F_BADLEN, np.uint8), "refused")
        for k in ("amp", "toa", "pwr", "soft", "hard"):
            assert not r[k][bad].any(), k
        partner = np.array([i ^ 1 for i in bad if (i ^ 1) < len(off) and acc[i ^ 1]])
        assert len(partner) >= 3
        check({k: v[partner] for k, v in r.items()}, e, "partners of refused bursts", sel=partner)


@pytest.mark.parametrize("sps", SPS)
def test_tolerance_mode(pkg, monkeypatch, sps):
    """TRXSIG_SOFT_TOLERANCE changes the demodulator only: flags, amp, TOA and hard bits are the exact mode's, soft bits pass the
    parity contract."""
    x, off, length, cls = rf.family(sps)
    e = expected(sps)
    t = make_ctx(pkg, monkeypatch, sps, 2)
    t.set_soft_mode(pkg.SOFT_TOLERANCE)
    assert t.soft_mode() == pkg.SOFT_TOLERANCE
    r = run(t, x, off, length)
    check(r, e, "tolerance mode", soft=False)
    det = (e["flags"] & F_DETECT) != 0
    assert det.sum() > 40
    err, frac = grade(np.where(e["valid"], r["soft"], 0)[det], e["soft"][det], "tolerance-mode soft bits")
    print("tolerance mode sps %d: max soft error %.3g, %.0f %% of values not identical" % (sps, err, 100 * frac))
