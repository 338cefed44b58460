"""The edge-of-range family (tests/mlse_edge_family.py) does reach its cases -- on the four float32 models, no GPU: the scale
identity where every square is a normal number, equalised bursts where they are subnormal, exact ties between windows resolved
towards the first scanned, E == 0 by underflow of nonzero taps, the 2^30 guard from both sides, IRC's identity set with E > 0, every
ordered pair of burst states within a wave, and what each boundary covariance set does.  These are conditions on the family: if a
generator changes and one fails, choose other base bursts; do not loosen it.  tests/test_gpu_mlse_edge.py holds the kernels to
the same families."""
import numpy as np
import pytest

import mlse_edge_family as ef
import mlse_irc_model as im
from mlse_edge_family import PAYLOAD, TRELLIS, assert_scale_identity, copies

F = np.float32


def kinds_of(f):
    """fell back / equalised with subnormal squares / equalised near 2^29 / ordinary, per burst of a ladder."""
    w, k = f["want"]["win"], f["k"]
    return np.where(w == 1, "fell back", np.where(k <= -60, "subnormal", np.where(k >= 28, "large", "plain")))


@pytest.mark.parametrize("sps", [1, 2, 4])
@pytest.mark.parametrize("kernel", ef.KERNELS)
def test_ladder_reaches_its_cases(kernel, sps):
    f = ef.ladder(kernel, sps)
    want, k, base = f["want"], f["k"], f["base"]
    B = len(k)
    assert 24 <= B <= 36 and B % 2 == 1 and set(k.tolist()) == set(ef.KS) and not np.isnan(want["soft"]).any()
    assert all(((k == kk) & (base == i)).sum() >= 1 for kk in ef.KS for i in range(3))
    pay = PAYLOAD[kernel]
    z = copies(f, 0)
    # the scale identity, where no square leaves the normal range
    for kk in (-50, 28):
        assert_scale_identity(kernel, want, f, kk)
    # subnormal squares: still equalised, other words, the same decisions
    a = copies(f, -66)
    assert np.all(want["win"][a] <= 0)
    assert np.array_equal(want["hard"][a][:, pay], want["hard"][z][:, pay])
    assert want["soft"][copies(f, -72)][:, pay].tobytes() != want["soft"][z][:, pay].tobytes()
    # exact ties between windows, resolved towards the first scanned (w = 0 first)
    Ew = ef.window_energies(f)
    top = Ew.max(axis=1, keepdims=True)
    tied = (Ew == top).sum(axis=1)
    first = np.argmax(Ew == top, axis=1)
    a = np.flatnonzero(k == -74)
    assert np.all(want["win"][a] <= 0)
    assert 2 * (tied[a] >= 2).sum() >= len(a), tied[a]
    eq = want["win"] <= 0
    assert np.array_equal(-want["win"][eq], first[eq])
    assert (first[a] < first[copies(f, 0)][base[a]]).any()             # ... which is another window than at scale 1
    # E == 0 by underflow of nonzero taps
    a = np.flatnonzero(k == -75)
    nonzero = np.abs(want["y"][a]).reshape(len(a), -1).max(axis=1) > 0
    gone = [i for i in range(3) if np.all((want["win"][a] == 1)[base[a] == i]) and np.all(nonzero[base[a] == i])]
    assert 2 * len(gone) >= 3, (want["win"][a], base[a])
    assert not want["chan"][a][want["win"][a] == 1].any()
    # the guard, from both sides
    a = np.flatnonzero(k == 29)
    assert (want["win"][a] == 1).any() and (want["win"][a] <= 0).any()
    for b in a[want["win"][a] <= 0]:
        i = copies(f, 0)[base[b]]
        assert want["soft"][b][TRELLIS[kernel]].tobytes() == want["soft"][i][TRELLIS[kernel]].tobytes()
    a = np.flatnonzero(k == 28)
    comp = np.abs(np.ascontiguousarray(want["y"][a]).view(F))
    assert np.all(want["win"][a] <= 0) and comp.max() >= 2.0 ** 29 and comp.max() < 2.0 ** 30
    # within a wave: an equalised burst beside one that fell back, a subnormal one beside a large one
    kind = kinds_of(f)
    pairs = {(kind[b], kind[b + 1]) for b in range(0, B - 1, 2)} | {(kind[b + 1], kind[b]) for b in range(0, B - 1, 2)}
    assert ("fell back", "plain") in pairs and ("subnormal", "large") in pairs
    if kernel == "access":                                     # four bursts a wave: each row position sees each kind
        for pos in range(4):
            assert set(kind[pos::4].tolist()) == {"fell back", "subnormal", "large", "plain"}, (pos, kind[pos::4])
    if kernel == "irc":
        ident = eq & np.all(want["cov"] == im.IDENTITY, axis=1)
        E = Ew.max(axis=1)
        assert (ident & (E > 0) & (k <= -73)).any()            # !(tt > 0) with E > 0: the residual sums underflow before the taps do
        assert (eq & ~np.all(want["cov"] == im.IDENTITY, axis=1) & (k <= -72)).any()     # ... and an estimated set out of subnormal sums


@pytest.mark.parametrize("sps", [1, 2, 4])
@pytest.mark.parametrize("kernel", ef.KERNELS)
def test_geometry_reaches_its_cases(kernel, sps):
    f = ef.geometry(kernel, sps)
    want, state = f["want"], f["state"]
    B = len(state)
    assert B < 40 and B % 2 == 1
    got = np.where(want["win"] <= 0, ef.EQ, want["win"])
    assert np.array_equal(got, state), list(zip(f["name"], state, want["win"]))
    names = set(f["name"])
    assert {"91 symbols", "92 symbols", "147 symbols", "148 symbols", "157 symbols", "158 symbols", "TOA 4096", "TOA -4096", "TOA past 4096",
            "TOA past -4096", "TOA NaN", "offset -1"} <= names
    assert sps == 1 or (f["length"] % sps != 0).sum() >= 2
    per = 4 if kernel == "access" else 2
    pairs = set()
    for b0 in range(0, B, per):
        wave = state[b0:b0 + per]
        pairs |= {(wave[i], wave[j]) for i in range(len(wave)) for j in range(i + 1, len(wave))}
    assert len(pairs) == 9, pairs
    # a burst delayed by 4096 symbols is all zeros: E == 0; no sample of an offset -1 burst is reachable without leaving the view's front
    for i, name in enumerate(f["name"]):
        if name.startswith("TOA ") and state[i] == ef.FB:
            assert not want["y"][i].any()
    offs = [f[ok] for _, ok in ef.antennas(f)]
    neg = np.flatnonzero(np.array(f["name"]) == "offset -1")
    assert len(neg) >= 2 and all(o[o >= 0].min() >= ef.GUARD for o in offs)
    if len(offs) == 1:
        assert np.all(offs[0][neg] == -1)
    else:                                                      # the negative offset is the non-primary antenna's alone
        for i in neg:
            assert offs[f["primary"][i]][i] >= 0 and offs[1 - f["primary"][i]][i] == -1
    for xk, ok in ef.antennas(f):                              # every enabled burst lies inside its array
        on = f[ok] >= 0
        assert np.all(f[ok][on] + f["length"][on] <= len(f[xk]))


@pytest.mark.parametrize("sps", [1, 4])
def test_irc_sets_do_what_their_comments_say(sps):
    f = ef.irc_set_batch(sps)
    want = f["want"]
    assert np.all(want["win"] <= 0) and not np.isnan(want["soft"]).any()
    for i, (row, accepted) in enumerate(ef.irc_sets()):
        expect = np.array(row, F) if accepted else im.IDENTITY
        assert np.array_equal(want["cov"][i], expect), (row, accepted, want["cov"][i])
    assert f["accepted"].sum() >= 6 and (~f["accepted"]).sum() >= 5


@pytest.mark.parametrize("sps", [1, 4])
def test_estimated_set_cases(sps):
    """The same samples on both antennas at loading 0: A == Bv == xr == 0.5, det == 0, the identity set; at loading 2^-20 the set is
    used; antenna 1 twice antenna 0 is decided by rounding, burst by burst."""
    for name, f, loading, identity in ef.estimated_set_cases(sps):
        want = ef.model(dict(f, loading=loading))
        eq = want["win"] <= 0
        assert eq.sum() >= len(eq) - 1
        ident = np.all(want["cov"] == im.IDENTITY, axis=1)
        S = want["sums"]
        if name.startswith("copy"):
            assert np.array_equal(S[:, 0], S[:, 1]) and np.array_equal(S[:, 0], S[:, 2]) and not S[:, 3].any()
        if identity is not None:
            assert np.all(ident[eq] == identity), (name, want["cov"])
        if identity is False:
            assert np.all(want["det"][eq] > 0) and np.all(want["det"][eq] < 2.0 ** -18)
