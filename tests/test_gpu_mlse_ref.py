"""The sequence equaliser's kernel (trxsig_mlse_batch, csrc/trxsig_mlse.hip) graded directly against the float64 reference
(tests/mlse_ref.py) on the family of tests/mlse_ref_family.py, each batch at its own rate: the soft bits within the reference's
a-priori bound, exact clamps, equal hard bits outside the margin -- the reference run on the kernel's OWN taps and window, so the
trellis grade does not lean on the estimator -- then the kernel's taps and window against the float64 estimator, and a few family
bursts through the Transceiver group's TRXSIG_TSCLEG_MLSE leg.  tests/test_mlse_ref.py does the same for the float32 model on the
CPU and shows, with six mutants, that the comparison can fail."""
import numpy as np
import pytest

import mlse_family
import mlse_model
import mlse_ref as ref
import mlse_ref_family as fam
import oraclebind
import transceiver_model as tm
from mlse_run import ctx, pkg, run_mlse  # noqa: F401  (the fixtures)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def runs(ctx):
    """Every batch of the family through the kernel, once: {sps: [(batch, outputs), ...]}."""
    return {sps: [(f, run_mlse(ctx[sps], f)) for f in fam.batches(sps)] for sps in (1, 2, 4)}


@pytest.mark.parametrize("sps", [1, 2, 4])
def test_kernel_within_the_bound(runs, sps):
    """The three conditions of tests/test_mlse_ref.py on the kernel's soft and hard bits, the reference fed the symbols of the model
    (the oracle's, graded elsewhere) and the kernel's own d_chan and d_win; the same cap on the positions kept out of the hard-bit
    comparison, the same rule for the named edge symbols.  The worst error / bound ratio is printed per group."""
    tally = ref.Tally(mlse_family.PAYLOAD)
    for f, got in runs[sps]:
        assert np.all((got["win"] >= -4) & (got["win"] <= 0)), "sps %d tsc %d: a family burst was not equalised" % (sps, f["tsc"])
        assert np.all(got["soft"][:, 148:] == -1.0) and np.all(got["hard"][:, 148:] == 255)
        named = fam.named_edges(f)
        g = ref.check(got["soft"], got["hard"], f["want"]["y"], got["win"], got["chan"], f["tsc"], "kernel, sps %d tsc %d" % (sps, f["tsc"]),
                      named=named)
        tally.add(g, f["snr"], f["group"], named)
    tally.report("kernel (GPU), sps %d" % sps)
    tally.assert_cap("kernel, sps %d" % sps)


@pytest.mark.parametrize("sps", [1, 2, 4])
def test_kernel_estimator_within_its_bounds(runs, sps):
    """d_chan against the float64 correlations of the window d_win names, |c - c64| <= 16 u Ymax per component, and that window's
    E64 >= max E64 - tolE (mlse_ref's docstring derives both)."""
    worst_c = worst_E = 0.0
    for f, got in runs[sps]:
        w = got["win"].astype(np.int64)
        assert np.all((w >= -4) & (w <= 0))
        e = ref.estimate64(f["want"]["y"], f["tsc"])
        rows = np.arange(len(w))[:, None]
        c64 = e["c"][rows, (w + 4)[:, None] + np.arange(5)[None, :]]
        err = np.maximum(np.abs(got["chan"].real - c64.real), np.abs(got["chan"].imag - c64.imag)).max(axis=1)
        assert np.all(err <= e["tol_c"]), (sps, f["tsc"], float((err / e["tol_c"]).max()))
        gap = e["E"].max(axis=1) - e["E"][np.arange(len(w)), -w]
        assert np.all(gap <= e["tol_E"]), (sps, f["tsc"])
        worst_c = max(worst_c, float((err / e["tol_c"]).max())); worst_E = max(worst_E, float((gap / e["tol_E"]).max()))
    print("kernel estimator (GPU), sps %d: worst |c - c64| / (16 u Ymax) = %.3f, worst window gap / tolE = %.3g" % (sps, worst_c, worst_E))


def test_group_leg_within_the_bound(pkg):
    """The leg in place: the distinct sps-4 bursts of the family's training sequence 2 (the lone tap and the two-tap, equal and
    ascending channels, with and without noise) in eight slots of one ARFCN of a Transceiver group on TRXSIG_TSCLEG_MLSE.  The group
    hands back no taps, so the reference runs on the float32 estimate (mlse_model.estimate, which the kernel equals and which is
    graded against the float64 estimator above) of the symbols at the group's own amplitude and TOA; the soft bits of the rows and
    of collect() meet the three conditions."""
    import torch
    sps, tsc, T, fn0 = 4, 2, 8, 101
    cell = 160 * sps
    f = [b for b in fam.batches(sps) if b["tsc"] == tsc][0]
    distinct = [int(np.flatnonzero(f["group"] == "lone")[0])] + np.flatnonzero(f["group"] == "channels").tolist()
    assert len(distinct) == 7
    x = np.zeros((T, 1, cell), np.complex64)
    for t in range(T):
        b = distinct[t % len(distinct)]
        n = min(int(f["length"][b]), (156 + (t % 4 == 0)) * sps)
        x[t, 0, :n] = f["x"][f["off"][b]:f["off"][b] + n]
    c = pkg.TrxSig(sps, 0)
    c.use_torch_stream()
    g = pkg.TrxGroup(c, 1, tsc_leg=pkg.TSCLEG_MLSE, start=(fn0, 0))
    for cmd in ["CMD RXTUNE 890000", "CMD TXTUNE 935000", "CMD SETTSC %d" % tsc] + ["CMD SETSLOT %d %d" % (tn, tm.I) for tn in range(8)] + ["CMD POWERON"]:
        g.control(0, cmd)
    dx = torch.from_numpy(x.view(np.float32).reshape(-1)).to("cuda:0")
    res = g.pull(dx, cell, cell, fn0, 0, T)
    g.sync()
    torch.cuda.synchronize()
    R = res.n_rows
    row = pkg._to_host(c, res.d_row, (T, 1), "<i4")
    valid = pkg._to_host(c, res.d_valid, (R,), "|u1")
    amp = pkg._to_host(c, res.d_amp, (R, 2), "<f4").view(np.complex64).ravel()
    toa = pkg._to_host(c, res.d_toa, (R,), "<f4")
    soft = pkg._to_host(c, res.d_soft, (R, res.soft_stride), "<f4")
    col = g.collect()
    g.close(); c.close()
    o = oraclebind.Oracle(sps)
    ys, rows, slots = [], [], []
    for t in range(T):
        r = row[t, 0]
        assert r >= 0
        if valid[r]:
            ys.append(mlse_model.symbols(o, x[t, 0, :(156 + (t % 4 == 0)) * sps], amp[r], toa[r])); rows.append(r); slots.append(t)
    assert len(rows) >= 5, "the group accepted %d of %d bursts" % (len(rows), T)
    y = np.stack(ys)
    _, w, h, E = mlse_model.estimate(y, mlse_model.tsc_symbols(tsc))
    assert np.all(E != 0) and np.abs(y.view(np.float32)).max() < 2.0 ** 30       # (none of them falls back)
    for what, s in (("rows", soft[rows][:, :148]), ("collect", col["soft"][slots, 0][:, :148])):
        gr = ref.check(s, s > np.float32(0.5), y, w, h, tsc, "group leg, " + what)
        print("group leg (GPU), %s: %d bursts, worst |soft - clamp(soft64)| / bound = %.4f" % (what, len(rows), gr["ratio"].max()))
