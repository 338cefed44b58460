"""The access-burst family of tests/rach_family.py is what it claims to be (no GPU): per class, enough members whose facts --
taken from the CPU oracle alone -- satisfy the class's condition, and every sweep crosses its flip.  This is what keeps
tests/test_gpu_rach_family.py from silently not exercising a branch of the device detector: the counts below are conditions on
the construction, not observations of it."""
import numpy as np
import pytest

import rach_family as rf


@pytest.fixture(scope="module", params=[1, 2, 4])
def info(request):
    return rf.family_info(request.param)


def _members(info, cls):
    return [i for i in range(len(info["cls"])) if info["cls"][i] == cls]


def test_census(info):
    c = rf.census(info)
    print("\nclass: members / satisfying  " + "  ".join("%s %d/%d" % (k, v[0], v[1]) for k, v in c.items()))
    assert len(info["off"]) < 600
    for cls in rf.CLASSES:
        assert c[cls][1] >= (4 if cls == "half_sample" else 8), (cls, c[cls])
    assert np.isfinite(info["x"].view(np.float32)).all()
    assert len(info["off"]) - info["noisy_from"] >= 40          # the noisy second and third copies are there


def test_sweeps_cross_the_flip(info):
    seen = set()
    for cls, i0, cnt, lags in info["sweeps"]:
        fs = [info["facts"][i] for i in range(i0, i0 + cnt)]
        assert cnt == 13
        assert {f["argmax"] for f in fs} == set(lags), (cls, lags, [f["argmax"] for f in fs])
        if cls == "far_tie":
            assert min(f["top2_gap"] for f in fs) <= 1e-6, (cls, lags)
            assert all({f["argmax"], f["second"]} == set(lags) for f in fs if f["top2_gap"] <= 1e-6)
            assert abs(lags[1] - lags[0]) > rf.NB_LO
        else:
            assert lags[1] == lags[0] + 1
        seen.add(cls)
    assert seen == {"far_tie", "half_sample"}
    assert sum(1 for s in info["sweeps"] if s[0] == "far_tie") == 3


def test_near_ties_lie_inside_the_neighbourhood(info):
    fs = [info["facts"][i] for i in _members(info, "near_tie")]
    ok = [f for f in fs if f["top2_gap"] <= 1e-6 and 2 <= f["top2_dist"] <= 12]
    assert len(ok) >= 8
    assert len({f["top2_dist"] for f in ok}) >= 3               # several distances, the largest one included
    assert max(f["top2_dist"] for f in ok) == 12
    assert len({f["argmax"] < f["second"] for f in ok}) == 2    # the earlier and the later peak both win somewhere


def test_contender_counts(info):
    got = {}
    for i in _members(info, "contend_k"):
        if len(info["facts"][i]["far"]) == info["design"][i]:
            got[info["design"][i]] = got.get(info["design"][i], 0) + 1
    for k in (1, 2, 6, 7, 8, rf.ALONE_LIMIT):                   # both sides of the pairing limit, and the last count a wave takes alone
        assert got.get(k, 0) >= 1, (k, got)
    many = [len(info["facts"][i]["far"]) for i in _members(info, "contend_many")]
    assert sum(1 for m in many if m > rf.ALONE_LIMIT) >= 8
    assert rf.ALONE_LIMIT + 1 in many                           # ... and the first count that takes the exact-everywhere route
    # the designed counts are exact, not lower bounds: nothing else within 2 % of the maximum (5 x RACH_DELTA)
    assert sum(1 for i in _members(info, "contend_k") if info["facts"][i]["far_loose"] == info["design"][i]) >= 8


def test_edges(info):
    early = [info["facts"][i] for i in _members(info, "edge_early")]
    assert sum(1 for f in early if 0 <= f["argmax"] <= 11) >= 8
    assert any(f["argmax"] == 0 for f in early) and any(f["argmax"] == 11 for f in early)
    late = [info["facts"][i] for i in _members(info, "edge_late")]
    kinds = dict(full=sum(1 for f in late if f["num_samples"] == f["full"]),
                 truncated=sum(1 for f in late if 2 <= f["num_samples"] < f["full"]),
                 none=sum(1 for f in late if f["num_samples"] < 2),
                 at_end=sum(1 for f in late if f["n"] - 12 <= f["argmax"] <= f["n"] - 2))
    assert all(v >= 2 for v in kinds.values()), kinds
    assert kinds["truncated"] + kinds["none"] >= 8 and kinds["at_end"] >= 8, kinds


def test_scale_and_ragged(info):
    sps = info["sps"]
    sc = [info["facts"][i] for i in _members(info, "scale")]
    assert all(f["finite"] for f in sc)
    assert any(f["ok"] for f in sc)                             # the large scale is detected like any burst
    rg = _members(info, "ragged")
    lo, hi = rf.length_limits()
    ln = {int(info["length"][i]) for i in rg}
    for n in (lo * sps - 1, lo * sps + 1, hi * sps - 1, hi * sps + 1, lo * sps, hi * sps):
        assert n in ln, n
    acc = info["accepted"]
    assert sum(1 for i in rg if not acc[i]) >= 4 and sum(1 for i in rg if acc[i]) >= 4
    assert any(info["off"][i] < 0 for i in rg)
    assert any(acc[i] and (info["off"][i] & 1) for i in rg)
    assert any(acc[i] and info["length"][i] < 148 * sps for i in rg)
    other = [i for i in range(len(acc)) if info["cls"][i] != "ragged"]
    g, length, _ = rf.synth.burst_lengths(len(acc), sps)
    assert np.array_equal(info["length"][other], length[other])   # everything else: the usual 157 / 156 / 156 / 156 symbols
    assert acc[other].all()
