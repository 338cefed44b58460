"""The synchronisation-burst sequence equaliser's kernel (k_mlse_sch, csrc/trxsig_mlse_sch.hip) graded directly by the float64
reference (tests/mlse_sch_ref.py): its own soft and hard bits, windows and taps, with no model between -- |soft - clamp(soft64)|
within the a-priori bound, exact clamps beyond it (the six tail bits exactly 0), equal hard bits outside it; its taps within the
estimator's bound of the float64 least-squares solution (which uses no table) and its window within tolE of the best one."""
import numpy as np
import pytest

import mlse_sch_family as family
import mlse_sch_model as model
import mlse_sch_ref as ref
from mlse_run import dev, pkg  # noqa: F401  (the fixtures)
from util import GpuBatch

pytestmark = pytest.mark.gpu
B_ALL = 37


@pytest.mark.parametrize("sps", [1, 2, 4])
def test_kernel_within_the_reference_bounds(pkg, sps):
    """37 bursts (clean, 15 dB, 12 dB, 8 dB; three profiles; delays up to 8 symbols): no bad_soft, bad_clamp or bad_hard, at most
    0.5 % of the coded positions outside the hard-bit comparison; |taps - c64| <= tol_c; window gap <= tolE.
    Measured on an MI355X (sps 1 / 2 / 4): worst |soft - clamp(soft64)| / bound 0.0015 / 0.0017 / 0.0013, worst |taps - c64| / tol_c
    0.035 / 0.065 / 0.056 (the model's figures: the kernel equals it word for word)."""
    import torch
    f = family.mixed_batch(sps, B_ALL, 6100 + sps)
    t = pkg.TrxSig(sps, 0)
    t.use_torch_stream()
    gb = GpuBatch(f["x"], f["off"], f["length"], nsoft=148, stride=148)
    chan = torch.zeros((B_ALL, 5, 2), dtype=torch.float32, device="cuda:0"); win = torch.full((B_ALL,), 9, dtype=torch.int32, device="cuda:0")
    t.mlse_sch(gb.x, gb.off, gb.len, dev(f["amp"]), dev(f["toa"]), gb.soft, chan=chan, win=win, hard=gb.hard, nsoft=148, soft_stride=148)
    r = gb.results()
    chan = chan.cpu().numpy().reshape(B_ALL, 10).view(np.complex64); win = win.cpu().numpy()
    t.close()
    eq = win <= 0
    assert eq.sum() >= B_ALL - 2
    y = f["want"]["y"]                                         # (the symbols are the oracle's: the kernel hands none out)
    g = ref.check(r["soft"][eq], r["hard"][eq], y[eq], win[eq], chan[eq], "kernel, sps %d" % sps)
    assert np.all(r["soft"][eq][:, [0, 1, 2, 145, 146, 147]] == 0.0)
    ex = int(g["excluded"][:, family.CODED].sum())
    assert ex <= 0.005 * eq.sum() * 78
    e = ref.estimate64(y[eq], model.pinv_table())
    w = win[eq]
    rows = np.arange(len(w))[:, None]
    idx = (w + 4)[:, None] + np.arange(5)[None, :]
    c64, tol = e["c"][rows, idx], e["tol_c"][rows, idx]
    err = np.maximum(np.abs(chan[eq].real - c64.real), np.abs(chan[eq].imag - c64.imag))
    gap = e["E"].max(axis=1) - e["E"][np.arange(len(w)), -w]
    print("k_mlse_sch, sps %d: worst |soft - clamp(soft64)| / bound = %.4f, worst |taps - c64| / tol_c = %.4f, worst window gap / tolE = %.3g, "
          "%d of %d coded positions inside the margin" % (sps, g["ratio"].max(), (err / tol).max(), (gap / e["tol_E"]).max(), ex, eq.sum() * 78))
    assert np.all(err <= tol) and np.all(gap <= e["tol_E"])
