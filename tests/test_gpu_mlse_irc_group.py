"""Two Transceiver groups, one per receive antenna, joined by trxsig_trxgroup_combine_irc: 2 ARFCNs x 16 slots at sps 4, a training
sequence per ARFCN, one access-burst slot, independent multipath per antenna and a co-channel handset (another training
sequence, its own channel per antenna) on most cells; cells where antenna 0 is silent, where antenna 1 is, where both are.  The
training-sequence rows equal the IRC model (tests/mlse_irc_model.py) row by row with the selected amp and TOA and loading 1/64 --
soft bits, taps, window and the set; access-burst rows are the selected pull's; everything else of the result is
trxsig_trxgroup_combine_div's bytes; neither group's own result or state is touched; combine_div on the same pulls, before and
after, gives identical bytes; combine_irc's refusals are combine_div's, and the loading's."""
import numpy as np
import pytest

import mlse_family
import mlse_irc_model as im
import oraclebind
import synth
import transceiver_model as tm
from mlse_combine import CELL, FN0, PROFILES, S, SPS, T, TSCS, aux, aux_host, combination, fetch, make_cells, make_group, to_dev
from mlse_run import canaries, pkg  # noqa: F401  (pkg: the fixture)
from util import assert_veq

pytestmark = pytest.mark.gpu

ITSC = 7
SILENT0, SILENT1, SILENT_BOTH = [(3, 0), (6, 1)], [(4, 1), (10, 0)], [(5, 1)]


@pytest.fixture(scope="module")
def cells():
    """(x [2 antennas][T][S][CELL] complex64, ctype [T][S]): independent multipath per antenna and an interferer on most cells."""
    def received(rng, o, s, t, a, n):
        si = o.modulate(synth.normal_bits(rng, 1, ITSC)[0].astype(np.int8), 9)
        out = []
        for ant in (0, 1):
            own = mlse_family.channel(rng, s, SPS, PROFILES[(t + a + ant) % 3], 22.0)[:n]
            other = mlse_family.channel(rng, si, SPS, PROFILES[(t + ant) % 2 * 2], None)[:n]
            ci_db = (6.0, 3.0, 10.0)[(t + a) % 3]
            out.append(own + (0.0 if (t + a) % 5 == 0 else 10.0 ** (-ci_db / 20.0)) * other)
        return out
    return make_cells(53, received, SILENT0 + SILENT_BOTH, SILENT1 + SILENT_BOTH)


@pytest.fixture(scope="module")
def run(pkg, cells):
    """The two pulls; combine_div, combine_irc, combine_div again, combine_irc without its optional outputs; two groups that never
    combined."""
    import torch
    x, _ = cells
    ctx = pkg.TrxSig(SPS, 0)
    ctx.use_torch_stream()
    legs = (pkg.TSCLEG_MLSE, pkg.TSCLEG_DEMOD)                # either leg is accepted
    dx = [to_dev(x[0]), to_dev(x[1])]
    out = {}
    for k in (0, 1):
        g = make_group(pkg, ctx, legs[k])
        res = g.pull(dx[k], S * CELL, CELL, FN0, 0, T)
        g.sync(); torch.cuda.synchronize()
        out["alone%d" % k] = dict(fetch(pkg, ctx, res), collect=g.collect())
        g.close()
    g0, g1 = make_group(pkg, ctx, legs[0]), make_group(pkg, ctx, legs[1])
    r0 = g0.pull(dx[0], S * CELL, CELL, FN0, 0, T)
    r1 = g1.pull(dx[1], S * CELL, CELL, FN0, 0, T)
    R = r0.n_rows
    for name in ("div_before", "irc", "div_after"):
        a = aux(R)
        if name == "irc":
            cov = canaries(R, (2, 5), cov=True)["cov"]         # [R + 1, 4]: a guard row behind
            rc = g0.combine_irc(dx[0], g1, dx[1], cov=cov, **a)
        else:
            rc = g0.combine_div(dx[0], g1, dx[1], **a)
        torch.cuda.synchronize()
        out[name] = dict(fetch(pkg, ctx, rc), **aux_host(a, R))
    out["irc"]["cov"] = cov.cpu().numpy()
    bare = g0.combine_irc(dx[0], g1, dx[1])                   # the optional outputs left out: the same result
    torch.cuda.synchronize()
    out["bare"] = fetch(pkg, ctx, bare)
    out["g0"] = dict(fetch(pkg, ctx, r0), collect=g0.collect())
    out["g1"] = dict(fetch(pkg, ctx, r1), collect=g1.collect())
    g0.close(); g1.close(); ctx.close()
    return out


def test_groups_are_untouched_by_the_combine(run):
    for k in (0, 1):
        a, g = run["alone%d" % k], run["g%d" % k]
        for key in ("row", "valid", "flags", "amp", "toa", "avgpwr", "threshold"):
            assert a[key].tobytes() == g[key].tobytes(), (k, key)
        v = a["valid"] != 0
        assert a["soft"][v].tobytes() == g["soft"][v].tobytes(), k
        for key in ("valid", "rssi", "timing", "threshold", "soft"):
            assert a["collect"][key].tobytes() == g["collect"][key].tobytes(), (k, "collect " + key)


def test_combine_div_is_unchanged_around_it(run):
    """combine_div on the same pulls before and after combine_irc: identical bytes, every output."""
    for key in run["div_before"]:
        assert run["div_before"][key].tobytes() == run["div_after"][key].tobytes(), key


def test_all_but_the_soft_rows_is_combine_divs(run):
    c, d = run["irc"], run["div_before"]
    for key in ("row", "valid", "flags", "amp", "toa", "avgpwr", "threshold", "sel"):
        assert c[key].tobytes() == d[key].tobytes(), key
    assert set(c["sel"].tolist()) == {0, 1, 2}
    for key in run["bare"]:
        assert run["bare"][key].tobytes() == c[key].tobytes(), "without d_sel / d_cov / d_chan / d_win: " + key
    assert np.all(c["cov"][-1] == -5.0), "d_cov written past the rows"


def test_combined_soft_rows(run, cells):
    x, ctype = cells
    c, g0, g1 = run["irc"], run["g0"], run["g1"]
    sel = c["sel"]
    o = oraclebind.Oracle(SPS)
    n_tsc = n_rach = n_zero = n_set = n_diff = 0
    for t in range(T):
        n = (156 + (t % 8 % 4 == 0)) * SPS
        for a in range(S):
            r = c["row"][t, a]
            assert r >= 0
            if ctype[t, a] == tm.RACH:
                assert c["valid"][r]
                src = g1 if sel[r] == 1 else g0
                assert c["soft"][r].tobytes() == src["soft"][r].tobytes()
                assert c["win"][r] == 2 and not c["chan"][r].any() and not c["cov"][r].any()
                n_rach += 1
            elif not c["valid"][r]:
                assert not c["soft"][r].any() and not c["cov"][r].any() and c["win"][r] == 2
                n_zero += 1
            else:
                zero = np.array([0], np.int32)
                want = im.mlse_irc_batch(SPS, x[0, t, a], zero, x[1, t, a], zero, np.array([n], np.int32), TSCS[a], c["amp"][r:r + 1],
                                         c["toa"][r:r + 1], primary=sel[r:r + 1], oracle=o)
                assert want["win"][0] <= 0
                assert_veq(c["soft"][r, :148], want["soft"][0], "slot %d ARFCN %d" % (t, a))
                assert c["win"][r] == want["win"][0]
                assert_veq(c["chan"][r].ravel(), want["chan"][0].ravel(), "taps, slot %d ARFCN %d" % (t, a))
                assert_veq(c["cov"][r], want["cov"][0], "set, slot %d ARFCN %d" % (t, a))
                n_set += int(np.abs(want["cov"][0, 2:]).max() > 0.05)
                n_diff += int(c["soft"][r].tobytes() != run["div_before"]["soft"][r].tobytes())
                n_tsc += 1
    assert n_tsc >= 26 and n_rach == 2 and n_zero >= 1 and n_set >= 12 and n_diff >= 24      # (and it is not combine_div's result)


def test_refusals(pkg, cells):
    """combine_div's refusals, each tried on combine_div and on combine_irc with the same groups: different contexts, ARFCN counts,
    rows (slot types), class bases (training sequences), burst lengths, times; no pull; the same group twice; a NULL sample pointer;
    the equalising leg.  And the loading: -1, 17 and NaN are refused, 0 and 16 accepted."""
    import torch
    x, _ = cells
    ctx = pkg.TrxSig(SPS, 0); ctx.use_torch_stream()
    other = pkg.TrxSig(SPS, 0); other.use_torch_stream()
    dx = [to_dev(x[0]), to_dev(x[1])]

    def pulled(g, k=1, fn=FN0, burst_len=0, n_arfcn=S):
        g.pull(dx[k], n_arfcn * CELL, CELL, fn, 0, T, burst_len=burst_len)
        return g
    g0 = pulled(make_group(pkg, ctx, pkg.TSCLEG_DEMOD), k=0)
    cases = [
        ("different contexts", pulled(make_group(pkg, other, pkg.TSCLEG_DEMOD))),
        ("ARFCN counts", pulled(make_group(pkg, ctx, pkg.TSCLEG_DEMOD, tscs=(2,), n_arfcn=1), n_arfcn=1)),
        ("rows differ", pulled(make_group(pkg, ctx, pkg.TSCLEG_DEMOD, comb=lambda a, tn: 0 if (a, tn) == (1, 3) else combination(a, tn)))),
        ("rows differ", pulled(make_group(pkg, ctx, pkg.TSCLEG_DEMOD, tscs=(2, 6)))),
        ("different lengths", pulled(make_group(pkg, ctx, pkg.TSCLEG_DEMOD), burst_len=156 * SPS)),
        ("different times", pulled(make_group(pkg, ctx, pkg.TSCLEG_DEMOD), fn=FN0 + 1)),
        ("no pull", make_group(pkg, ctx, pkg.TSCLEG_DEMOD)),
    ]
    for what, g1 in cases:
        for call, name in ((g0.combine_div, "combine_div"), (g0.combine_irc, "combine_irc")):
            with pytest.raises(pkg.TrxSigError, match="trxsig_trxgroup_%s: .*%s" % (name, what)):
                call(dx[0], g1, dx[1])
        with pytest.raises(pkg.TrxSigError):
            g1.combine_irc(dx[1], g0, dx[0])
    with pytest.raises(pkg.TrxSigError):
        g0.combine_irc(dx[0], g0, dx[0])
    with pytest.raises(pkg.TrxSigError):
        g0.combine_irc(None, cases[-1][1], dx[1])
    good = pulled(make_group(pkg, ctx, pkg.TSCLEG_MLSE))
    for loading in (-1.0, 17.0, float("nan")):
        with pytest.raises(pkg.TrxSigError, match="loading"):
            g0.combine_irc(dx[0], good, dx[1], loading=loading)
    for loading in (0.0, 16.0, pkg.IRC_LOADING):
        assert g0.combine_irc(dx[0], good, dx[1], loading=loading).n_rows == T * S
    torch.cuda.synchronize()
    for g in [good] + [c[1] for c in cases]:
        g.close()
    g0.close(); ctx.close(); other.close()
    c1 = pkg.TrxSig(1, 0); c1.use_torch_stream()
    z = torch.zeros(T * S * 160 * 2, dtype=torch.float32, device="cuda:0")
    ge, gd = pkg.TrxGroup(c1, S, tsc_leg=pkg.TSCLEG_EQUALIZE), pkg.TrxGroup(c1, S, tsc_leg=pkg.TSCLEG_DEMOD)
    for a, b in ((ge, gd), (gd, ge)):
        with pytest.raises(pkg.TrxSigError, match="TRXSIG_TSCLEG_EQUALIZE"):
            a.combine_irc(z, b, z)
    ge.close(); gd.close(); c1.close()
