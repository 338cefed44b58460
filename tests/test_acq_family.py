"""The acquisition family of tests/acq_family.py is what it claims to be (no GPU): the lattice members are lattice streams whose
exact answer every model of stage 1 agrees on bit for bit, the tie plateaus lie in the tiles, waves and lanes they are meant
for, the angle sweep keeps clear of the half-plane border by more than the kernel's error, and the states the CPU model reaches
on the far offsets and the sps-2 truth cases are the ones recorded in acq_family's docstring.  This is what makes a failure of
tests/test_gpu_acq_family.py the kernel's and nobody else's."""
import numpy as np
import pytest

import acq_family as af
import l1_acq_model as am

F32 = np.float32


@pytest.fixture(scope="module", params=af.SPS)
def sps(request):
    return request.param


def test_lattice_models_agree(sps):
    """lattice_model == the float64 metric at every k (C, E, and m formed in float32 from them) == the float32 segment emulation
    == (amplitudes 0 and 1) the differenced running sum, and the members' promises hold"""
    L = am.fcch_len(sps)
    members = af.lattice_members(sps)
    assert len(members) == 1 + 13 + 2 * len(af.TWIN) + 3 + 1
    for mb in members:
        x, lm, what = mb["x"], mb["model"], (sps, mb["name"])
        C64, E64, m64 = am.fcch_metric64(x, sps)
        assert len(x) == af.N_LATTICE and C64.shape == lm["m_all"].shape
        assert np.array_equal(C64, lm["C_all"]) and np.array_equal(E64, lm["E_all"]), what
        assert np.array_equal(af.metric32(C64.astype(np.complex64), E64.astype(F32)), lm["m_all"]), what
        assert np.array_equal(am.fcch_metric32_segments(x, sps), lm["m_all"]), what
        if mb["unit"]:
            assert np.array_equal(am.fcch_metric32_segments(x, sps, running=True), lm["m_all"]), what
        assert lm["k"] == int(np.argmax(lm["m_all"])) and not (lm["m_all"][:lm["k"]] == lm["m"]).any(), what
        e = mb["expect"]
        for key in ("k", "m", "C", "E"):
            assert key not in e or lm[key] == e[key], (what, key, lm[key], e[key])
        if "arg" in e:
            assert abs(np.arctan2(float(lm["C"].imag), float(lm["C"].real)) - e["arg"]) < 1e-12, what
    n_tiles = (af.N_LATTICE - sps - L + 1 + af.W - 1) // af.W
    assert n_tiles == (70 if sps == 4 else 71) and n_tiles > 64 + 3


def test_plateaus_lie_where_the_members_say(sps):
    L = am.fcch_len(sps)
    by = {mb["name"]: mb for mb in af.lattice_members(sps)}
    m = by["plateau"]["model"]["m_all"]
    assert (m == 1.0).all()                                    # every window ties: k = 0 is the tie rule's alone
    for P in af.late_positions(sps):
        m = by["late_plateau %d" % P]["model"]["m_all"]
        assert (m[:P] < 1.0).all() and (m[P:] == 1.0).all() and (m[max(0, P - L + 1):P] > 0).all(), P
    for mb in by.values():
        m = mb["model"]["m_all"]
        if mb["name"].startswith("border"):
            assert not m.any()
        if "runs" not in mb:
            continue
        at, pl = mb["runs"], mb["plateaus"]
        assert pl == [(p, p) for p in at] and [p // af.W for p in at] == mb["tiles"], mb["name"]
        rest = m.copy()
        rest[at] = 0
        assert rest.max() < 1.0 and mb["model"]["k"] == at[0], mb["name"]
        idx = [p % af.W for p in at]
        if "waves 0 and 2" in mb["name"]:
            assert [(i % 256) // 64 for i in idx] == [0, 2]
        if "one thread" in mb["name"]:
            assert idx[0] % 256 == idx[1] % 256 and idx[0] != idx[1]
        if "tiles 3 and 67" in mb["name"]:
            assert mb["tiles"][1] == mb["tiles"][0] + 64       # one lane of the pick sees both, the earlier one first
        if "tiles 63 and 64" in mb["name"]:
            assert mb["tiles"] == [63, 64]                     # lane 63 holds the winner, lane 0 the later tie
        if "tile boundary" in mb["name"]:
            assert idx[0] + L > af.W                           # the window needs the halo segment
        if "segment boundary" in mb["name"]:
            assert 0 < idx[0] < L < idx[0] + L and 2 * L <= af.W   # suffix of segment 0, prefix of segment 1, both the tile's own
    thr = by["threshold"]["model"]
    assert 0.5 < thr["m"] < 1.0 and np.sort(thr["m_all"])[-2] < thr["m"]
    assert [mb["name"] for mb in af.exact_m_members(sps)] == ["plateau", "threshold"]


def test_angle_sweep(sps):
    th, xs = af.angle_sweep(sps)                               # the generator asserts the guard for all 63
    assert len(th) == len(xs) == 63 and len(set(np.round(th, 6))) == 63
    assert min(abs(abs(th) - np.pi / 2)) > 0.009 and th.min() > -np.pi and th.max() < np.pi
    octants = {int(np.floor(t / (np.pi / 4))) for t in th}
    assert octants == set(range(-4, 4))
    inside = 0
    for t, x in zip(th, xs):
        C, E, _ = am.fcch_metric64(x, sps)
        assert (np.abs(C.real) > af.sweep_guard(sps) * E).all(), t
        f = am.fcch_search64(x, sps)
        if abs(t) < np.pi / 2:
            assert f["m"] > 0.99 and abs(f["arg"] - t) < 1e-3, (t, f["m"], f["arg"])
            inside += 1
        else:
            assert f["k"] == 0 and f["m"] == 0 and abs(np.angle(np.exp(1j * (f["arg"] - t)))) < 1e-3, (t, f)
    assert 25 <= inside <= 38


def test_far_offsets_and_dynamic_range(sps):
    """the states the model reaches on its own k are the recorded ones; none is demanded that it does not reach"""
    det, tx = am.SchDetector(af.oracle(sps)), af.fec_tx()
    far = af.far_offset(sps)
    assert [f for f, _ in far] == list(af.FAR_F) and len({len(x) for _, x in far}) == 1
    for f, x in far:
        r = am.search_model(det, tx, x)
        assert r["state"] == af.FAR_OFFSET_STATE[(sps, f)], (sps, f, r["state"])
        assert abs(r["fcch"]["arg"] / (2 * np.pi) - f) <= 2e-3 and r["fcch"]["C"].real > 0, (sps, f, r["fcch"])
    dyn = af.dynamic_range(sps)                                # the generator asserts the float32 scheme against float64
    assert [db for db, _ in dyn] == [60, 90] and len({len(x) for _, x in dyn}) == 1
    for db, x in dyn:
        loud = np.abs(x).max()
        assert 0.5 * 10 ** (db / 20) < loud < 2 * 10 ** (db / 20) and am.fcch_search64(x, sps)["found"], (db, loud)


def test_truth_at_sps2():
    """am.truth_cases(2): all 16 reach state 15 on the model (TRUTH2_STATE15)"""
    det, tx = am.SchDetector(af.oracle(2)), af.fec_tx()
    states = [am.search_model(det, tx, am.truth_stream(af.oracle(2), tx, c)[0])["state"] for c in am.truth_cases(2)]
    assert len(states) == 16 and states.count(15) == af.TRUTH2_STATE15, states
