"""The float32 model of the fit detector for synchronisation bursts (trxsig_sch_fit_batch, csrc/trxsig_sch_fit.hip; trxsig_l1acq's
TRXSIG_SCHDET_FIT): the algorithm of include/trxsig.h restated in numpy float32, operation by operation, vectorised over bursts.
The kernel must equal it word for word.

The symbols, the nine taps, the window and E are tests/mlse_sch_model.py's and tests/mlse_core.py's, called, not copied.  What is
new here is the residual of that fit on the 56 rows whose symbols are all known, its sum R in the kernel's reduction order, and
q = sqrtf((51 E) / R).  Every arithmetic step below is ONE float32 operation on float32 arrays, in the order the header states.

FitSchDetector is tests/l1_acq_model.py's SCH detector with the fit verdict (TRXSIG_SCHDET_FIT), on either leg; it goes into
l1_acq_model.search_model unchanged."""
import numpy as np

import l1_acq_model as am
import mlse_core as core
import mlse_sch_model as sm
from mlse_core import F, WIN_FELL_BACK, WIN_SKIPPED
NDOF = 51                                                     # 56 rows less 5 taps
A_SIGN = np.zeros(148, np.int64)                              # a[n] = 2 bit - 1 on the extended training sequence, 0 elsewhere
A_SIGN[sm.XTS0:sm.XTS0 + sm.NXTS] = 2 * sm.XTS - 1


def row_energies(y, w, h, sign_shift=0, window_shift=0):
    """Step 3 on symbols y [B, 148], windows w [B] and taps h [B, 5]: e [B, 56] float32, e[n - 46] = |y[n] - Z[n]|^2 with
    Z[n] = h[0] a[n - w], + h[1] a[n - w - 1], .. in this order.  sign_shift / window_shift: the mutants of
    tests/test_sch_fit_model.py (a taken from n - w - k + sign_shift; the window w + window_shift for the signs)."""
    B = y.shape[0]
    yr, yi = y.real.astype(F), y.imag.astype(F)
    hr, hi = h.real.astype(F), h.imag.astype(F)
    n = np.arange(sm.ROW0, sm.ROW0 + sm.NROW)
    ww = (np.asarray(w, np.int64) + window_shift)[:, None]
    zr = zi = None
    for k in range(5):
        a = A_SIGN[n[None, :] - ww - k + sign_shift].astype(F)                  # [B, 56], +-1 (0 only for a mutant off the sequence)
        tr, ti = hr[:, k, None] * a, hi[:, k, None] * a                         # sign flips: exact
        zr, zi = (tr, ti) if zr is None else (zr + tr, zi + ti)
    dr = yr[:, sm.ROW0:sm.ROW0 + sm.NROW] - zr
    di = yi[:, sm.ROW0:sm.ROW0 + sm.NROW] - zi
    return (dr * dr + di * di).astype(F)


def tree(e, drop_last=False):
    """Step 4: the pairwise tree over e[0..63], e[56..63] = 0 (the 64 lanes of a wave), [B, 56] -> [B]."""
    B = e.shape[0]
    v = np.zeros((B, 64), F)
    v[:, :sm.NROW] = e
    if drop_last:
        v[:, sm.NROW - 1] = 0                                 # the mutant: row 101 dropped
    while v.shape[1] > 1:
        v = (v[:, 0::2] + v[:, 1::2]).astype(F)
    return v[:, 0]


def quality(E, R):
    """Step 5: q = sqrtf((51.0f * E) / R); +inf stays, a NaN becomes 0."""
    with np.errstate(all="ignore"):
        q = np.sqrt((F(NDOF) * E.astype(F)) / R.astype(F)).astype(F)
    return np.where(np.isnan(q), F(0), q).astype(F)


def fit(y, **mutant):
    """Steps 2-6 on symbols y [B, 148]: dict(chan9 [B, 9], win [B] (w, or 1 = fell back), E, R, q [B])."""
    y = np.ascontiguousarray(y, np.complex64)
    drop_last = mutant.pop("drop_last", False)
    fine, ys = core.usable(y)
    with np.errstate(all="ignore"):
        c, w, h, E = sm.estimate(ys)
        ok = fine & (E != 0)
        R = tree(row_energies(ys, w, h, **mutant), drop_last)
        q = quality(E, R)
    z = F(0)
    return dict(chan9=np.where(ok[:, None], c, 0).astype(np.complex64), win=np.where(ok, w, WIN_FELL_BACK).astype(np.int32),
                E=np.where(ok, E, z).astype(F), R=np.where(ok, R, z).astype(F), q=np.where(ok, q, z).astype(F), h=h, w=w)


def fit_batch(sps, x, off, length, amp, toa, enable=None, oracle=None, **mutant):
    """trxsig_sch_fit_batch on packed bursts: dict(chan9 [B, 9], win, E, R, q [B], y [B, 148])."""
    y, state = core.burst_symbols(sps, [x], [off], length, amp, toa, enable, oracle)
    y = y[:, 0]
    r = fit(y, **mutant)
    out_ = state != 0
    r["chan9"][out_] = 0; r["E"][out_] = 0; r["R"][out_] = 0; r["q"][out_] = 0
    r["win"][out_] = state[out_]
    r["y"] = y
    return r


# ---- acquisition with the fit verdict ----------------------------------------------------------------------------------------------
class FitSchDetector(am.SchDetector):
    """tests/l1_acq_model.py's SCH detector under TRXSIG_SCHDET_FIT (include/trxsig_l1acq.h): steps 1 to 3 unchanged, the geometry
    gate in the valley rule's place, q on the candidate's segment, detected iff q > thresh; ptm reports q.  mlse: step 7 on
    TRXSIG_SCHLEG_MLSE (the result then carries chan and win as tests/mlse_sch_family.MlseSchDetector's does)."""

    def __init__(self, o, mlse=False):
        super().__init__(o)
        self.mlse = mlse

    def detect(self, x, omega, thresh):
        o, sps = self.o, self.sps
        x = np.asarray(x, np.complex64)
        n = len(x)
        out = dict(flags=0, amp=np.complex64(0), toa=F(0), ptm=F(0), soft=np.zeros(148, F), chan=np.zeros(5, np.complex64),
                   win=WIN_SKIPPED, R=F(0), candidate=False)
        if n <= 0 or n > 256 * sps:
            out["flags"] = 128
            return out
        y = x if omega is None else o.frequency_shift(x, F(omega), 0.0)[0]
        peak, toa, _ = o.peak_detect(o.correlate(y, self.seq))
        toa = F(toa)
        inside = bool(toa >= 0 and toa <= F(n))
        with np.errstate(all="ignore"):
            amp = am._cdiv(peak, self.gain) if inside else np.complex64(0)
        toa_b = F(F(toa - self.toa) - F(42 * sps))
        out.update(amp=amp, toa=toa_b)
        if not (inside and np.isfinite(amp.real) and np.isfinite(amp.imag) and amp != 0):
            return out
        fl0 = np.floor(toa_b)
        if not (fl0 >= 0 and int(fl0) + 148 * sps <= n):
            return out
        i0 = int(fl0)
        nd = min(156 * sps, ((n - i0) // sps) * sps)
        seg = np.ascontiguousarray(y[i0:i0 + nd])
        rest = F(toa_b - F(fl0))
        r = fit_batch(sps, seg, np.array([0]), np.array([nd]), np.array([amp], np.complex64), np.array([rest], F), oracle=o)
        out.update(candidate=True, ptm=F(r["q"][0]), R=F(r["R"][0]))
        if r["q"][0] > F(thresh):
            out["flags"] = 2
            if self.mlse:
                m = sm.sch_batch(sps, seg, np.array([0]), np.array([nd]), np.array([amp], np.complex64), np.array([rest], F), oracle=o)
                out.update(soft=m["soft"][0], chan=m["chan"][0], win=int(m["win"][0]))
            else:
                out["soft"] = o.demodulate(seg, amp, rest)[:148].astype(F)
        return out
