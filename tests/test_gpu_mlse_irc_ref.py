"""The interference-rejection equaliser's kernel (k_mlse_irc, csrc/trxsig_mlse_irc.hip) graded directly by the float64 reference
(tests/mlse_irc_ref.py) on the graded family with interferers (tests/mlse_irc_family.py): its own soft and hard bits, windows, taps
and sets, with no model between -- |soft - clamp(soft64)| within the a-priori bound, exact clamps beyond it, equal hard bits
outside it.  The residual sums are not an output of the kernel; what it reports of them is the set, which is held to the sums'
bound through the four divisions (a set from sums within their bound lies within the propagated bound of the float64 set)."""
import numpy as np
import pytest

import mlse_family
import mlse_irc_family as ifam
import mlse_irc_model as im
import mlse_irc_ref as iref
import mlse_ref
from mlse_run import dev, pkg  # noqa: F401  (the fixtures)
from util import GpuBatch

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("sps", [1, 4])
def test_kernel_within_the_reference_bounds(pkg, sps):
    """72 bursts at sps 1 (24 at sps 4; clean, 15 dB, 8 dB; independent channels per antenna, an interferer on five of six): no
    bad_soft, bad_clamp or bad_hard, at most 0.5 % of a noise level's payload positions outside the hard-bit comparison.  The set
    the kernel reports: tt64 = S00_64 + S11_64; each of S/tt is off from S64/tt64 by at most (b_S + |S64| (b_00 + b_11) / tt64) / tt64
    plus three roundings, 3 u |S/tt| (tt's own addition, the division, the loading's addition) -- b the sums' bounds of
    mlse_irc_ref.sums64.
    Measured on an MI355X (sps 1 / sps 4): worst |soft - clamp(soft64)| / bound 0.0042 / 0.0035 (the model's figures: the kernel
    equals it word for word); worst |set - set64| / bound 0.044 / 0.035."""
    import torch
    f = ifam.graded_batch(sps, per=24 if sps == 1 else 8)
    B = len(f["off0"])
    t = pkg.TrxSig(sps, 0)
    t.use_torch_stream()
    gb = GpuBatch(f["x0"], f["off0"], f["length"], nsoft=148, stride=148)
    chan = torch.zeros((B, 2, 5, 2), dtype=torch.float32, device="cuda:0"); win = torch.zeros(B, dtype=torch.int32, device="cuda:0")
    cov = torch.zeros((B, 4), dtype=torch.float32, device="cuda:0")
    t.mlse_irc(gb.x, gb.off, dev(f["x1"]), dev(f["off1"]), gb.len, f["tsc"], dev(f["amp"]), dev(f["toa"]), gb.soft, primary=dev(f["primary"]),
               cov=cov, chan=chan, win=win, hard=gb.hard, nsoft=148, soft_stride=148)
    r = gb.results()
    chan = chan.cpu().numpy().reshape(B, 2, 10).view(np.complex64); win = win.cpu().numpy(); cov = cov.cpu().numpy()
    t.close()
    eq = win <= 0
    assert eq.sum() >= B - 2
    y = f["want"]["y"]
    ident = np.all(cov == im.IDENTITY, axis=1)
    assert (eq & ~ident).sum() >= B - 4
    g = iref.check(r["soft"][eq], r["hard"][eq], y[eq], win[eq], chan[eq], cov[eq], f["tsc"], "kernel, sps %d" % sps)
    tally = mlse_ref.Tally(mlse_family.PAYLOAD)
    tally.add(g, f["snr"][eq], f["group"][eq])
    tally.report("k_mlse_irc, sps %d" % sps)
    tally.assert_cap("k_mlse_irc, sps %d" % sps)
    use = eq & ~ident
    s = iref.sums64(y[use], win[use], chan[use], f["tsc"])
    S, b = s["sums"], s["bound"]
    tt = S[:, 0] + S[:, 1]
    lam = np.float64(im.LOADING)
    want = np.stack([S[:, 0] / tt + lam, S[:, 1] / tt + lam, S[:, 2] / tt, S[:, 3] / tt], axis=1)
    tol = (b + np.abs(S) * ((b[:, 0] + b[:, 1]) / tt)[:, None]) / tt[:, None] * mlse_ref.SLACK + 3.0 * mlse_ref.U * np.abs(want)
    err = np.abs(cov[use].astype(np.float64) - want)
    print("k_mlse_irc, sps %d: worst |soft - clamp(soft64)| / bound = %.4f, worst |set - set64| / bound = %.4f" % (sps, g["ratio"].max(), (err / tol).max()))
    assert np.all(err <= tol)
