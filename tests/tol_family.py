"""Inputs and grading for the tolerance-mode demodulator (TRXSIG_SOFT_TOLERANCE, csrc/trxsig_demod.h fused_demod_tol_ex).

The parity contract for soft bits: |soft - ref| <= 1e-6 or <= 1e-4 |ref| (ref: the reference's soft bit on the [0, 1] scale).
It cannot be proved for rearranged float32 arithmetic (the reference's own rounding error is far above 1e-6), so the tests check
it on stated families of inputs, one of them built to defeat it:

  adversarial_batch: unit-magnitude amplitude of random phase, TOA = -(k + f/512) with f in [200, 312) (the taps' largest
  values); outputs m whose 21-sample windows are disjoint get window samples s_j L p, s_j = sign(tap_j) (+1 before the centre,
  -1 after it), p = conj(rev[m] inv) at unit inf-norm, L = (0.9 .. 1) Z_target / |inv|_1 -- so the fused multiply-add chain
  carries partial sums of about S/2 L |rev inv| and then cancels them -- and a centre sample that steers the output into the
  low band, Re(rev inv sum tap x) = -1 + 2 U(1e-4, 0.01), where the contract's absolute floor of 1e-6 is all there is.  The
  samples outside the windows carry random signs at up to 0.9 L, which keeps the other outputs out of the slicer's guard band
  (a burst with one output there goes to the exact code whole).

Helper module, no tests here.
"""
import numpy as np

ZMAX = 4.0                  # TRX_TOL_ZMAX (csrc/trxsig_demod.h)
GUARANTEE = 9.2e-6          # |soft' - soft| <= GUARANTEE * Z for every burst the fast form takes (derivation: trxsig_demod.h)
FLOOR, REL = 1e-6, 1e-4     # the contract: absolute floor, relative bound


def allowance(ref):
    return np.maximum(FLOOR, REL * np.abs(np.asarray(ref, np.float64)))


def contract_ratio(soft, ref):
    """err / allowance per value (<= 1 where the contract holds)."""
    soft = np.asarray(soft, np.float64); ref = np.asarray(ref, np.float64)
    return np.abs(soft - ref) / allowance(ref)


def inv_of(amp):
    """((complex)1.0)/amp as Complex.h forms it in float32 (the value the kernels use)."""
    a = np.asarray(amp, np.complex64)
    ar, ai = a.real.astype(np.float32), a.imag.astype(np.float32)
    with np.errstate(all="ignore"):
        n2 = (ai * ai + ar * ar).astype(np.float32)
        cr, ci = (ar / n2).astype(np.float32), (-ai / n2).astype(np.float32)
        return (np.float32(1) * cr - np.float32(0) * ci) + 1j * (np.float32(1) * ci + np.float32(0) * cr).astype(np.float32)


def z_of(x, off, length, amp):
    """Z = max|x|_inf * |1/amp|_1 per burst, in float32 as the kernel forms it."""
    inv = inv_of(amp)
    inv1 = (np.abs(inv.real).astype(np.float32) + np.abs(inv.imag).astype(np.float32)).astype(np.float32)
    xm = np.array([max(np.abs(x[o:o + n].real).max(), np.abs(x[o:o + n].imag).max()) for o, n in zip(off, length)], np.float32)
    return (xm * inv1).astype(np.float32)


def spacing(sps):
    """Output spacing that keeps the 21-sample windows of the chosen outputs disjoint."""
    return -(-21 // sps)


def adversarial_batch(tables, sps, B, z_target, seed):
    """B bursts of 156 * sps samples (module docstring).  Returns x, off, length, amp, toa, steered (bool [B, 148]: the outputs
    steered into the low band)."""
    rng = np.random.default_rng(seed)
    N = 156 * sps
    grid = np.asarray(tables["sinc_grid"], np.float32)
    rev = np.asarray(tables["rev"], np.complex64)
    amp = np.exp(2j * np.pi * rng.uniform(size=B)).astype(np.complex64)
    inv = inv_of(amp).astype(np.complex128)
    inv1 = np.abs(inv.real) + np.abs(inv.imag)
    k = rng.integers(0, 3, B)
    f = rng.integers(200, 312, B)
    toa = (-(k + f / 512.0)).astype(np.float32)
    x = np.zeros((B, N), np.complex64)
    steered = np.zeros((B, 148), bool)
    D = spacing(sps)
    j = np.arange(21)
    for b in range(B):
        tp = grid[f[b], :21].astype(np.float64)
        s = np.sign(tp) * np.where(j < 10, 1.0, -1.0)
        s[10] = 0.0
        m_lo = -(-(10 + k[b]) // sps)                         # t - 10 >= 0
        m = m_lo + rng.integers(0, D) + D * np.arange(148)
        t = sps * m - k[b]
        keep = (m < 148) & (t + 10 < N)
        m, t = m[keep], t[keep]
        w = rev[sps * m].astype(np.complex128) * inv[b]       # [M]
        p = np.conj(w)
        p /= np.maximum(np.abs(p.real), np.abs(p.imag))
        L = rng.uniform(0.9, 1.0, len(m)) * z_target / inv1[b]
        win = s[None, :] * (L[:, None] * p[:, None])          # [M, 21]: sample t + 10 - j
        target = -1.0 + 2.0 * rng.uniform(1e-4, 0.01, len(m))
        rest = (w * (win * tp[None, :]).sum(axis=1)).real
        win[:, 10] = (target - rest) / (tp[10] * np.abs(w) ** 2) * np.conj(w)
        # every other sample: random signs at most 0.9 L, so that no output outside the windows sits in the guard band
        fill = 0.9 * z_target / inv1[b] * rng.uniform(0.5, 1.0, (2, N)) * rng.choice([-1.0, 1.0], (2, N))
        x[b] = (fill[0] + 1j * fill[1]).astype(np.complex64)
        idx = t[:, None] + 10 - j[None, :]
        x[b, idx] = win.astype(np.complex64)
        steered[b, m] = True
    off = (np.arange(B) * N).astype(np.int32)
    length = np.full(B, N, np.int32)
    return x.ravel(), off, length, amp, toa, steered


def realistic_batch(sps, B, seed, sigmas, zmax=ZMAX, grid_toa=True):
    """synth.normal_batch bursts with the oracle's amp / TOA, the amplitude scaled down by a factor in (0.15, 1] per burst so that
    Z covers (0, zmax], and (grid_toa) the TOA moved by up to half a sample on the 1/512 grid so that every fraction occurs.
    Returns x, off, length, amp, toa (detected bursts only)."""
    import oraclebind
    import synth
    rng = np.random.default_rng(seed)
    tsc = int(rng.integers(0, 8))
    x, off, length, _ = synth.normal_batch(sps, B, tsc, seed=seed, sigmas=sigmas)
    ok, amp, toa, _ = oraclebind.Oracle(sps).normal_batch(x, off, length, tsc, nsoft=148, nthreads=8)
    sel = np.flatnonzero(ok.astype(bool))
    off, length, amp, toa = off[sel], length[sel], amp[sel], toa[sel]
    z1 = z_of(x, off, length, amp).astype(np.float64)
    lo = np.clip(np.maximum(0.15, z1 / zmax * (1 + 1e-6)), None, 1.0)
    scale = rng.uniform(lo, 1.0)                               # Z / scale: from Z up to min(Z / 0.15, zmax)
    amp = (amp * scale).astype(np.complex64)
    if grid_toa:
        toa = (toa + (rng.integers(0, 512, len(sel)) - 256) / 512.0).astype(np.float32)
    return x, off, length, amp, toa
