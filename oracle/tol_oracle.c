/*
 * oracle/tol_oracle.c -- TEST INFRASTRUCTURE ONLY (see tol_oracle.h).
 *
 * Restates fused_demod_tol_ex (openbts-ttsou_amd/csrc/trxsig_demod.h) for one burst, operation by
 * operation: every fused multiply-add of the kernel is an explicit fmaf (correctly rounded, as
 * v_fma_f32 is), every other product and sum is a separately rounded float operation (built with
 * -ffp-contract=off, oracle/Makefile).  What it restates, in the kernel's order:
 *   - inv = ((complex)1.0) / amp as Complex.h forms it (cinv, then the product with 1 + 0i);
 *   - Z = max|x|_inf * (|inv.r| + |inv.i|) over the whole burst (a NaN sample is passed over);
 *   - eligibility: TOA on the 1/512 grid, max|x| and |inv|_1 in [1e-15, 1e15], Z <= zmax;
 *   - the filter threshold |frac| > 1e-2 (else output m is sample sps * m - intOffset itself);
 *   - the 21-tap chain, taps j = 0..20 ascending, y = fma(x, tap, y) from 0, per component;
 *   - a = fma(c, inv.r, -(d * inv.i)), b = fma(c, inv.i, d * inv.r), re = fma(a, y.r, -(b * y.i));
 *   - the slicer fma(re, 0.5, 0.5) clamped to [0, 1]; 0.5 where the output lies outside the burst;
 *   - the guard: a valid output with !(|re| > fma(Z, 2^-15, 2^-22)) hands the whole burst over.
 * Nothing here comes from the reference; the value-exact form it hands over to is so_demodulate.
 */
#include "tol_oracle.h"

#include <math.h>
#include <string.h>
#ifdef _OPENMP
#include <omp.h>
#endif

int so_demod_tol(const so_c32 *x, int n, int sps, so_c32 amp, float toa, const float *sinc_grid,
                 int row, const so_c32 *rev, float zmax, int nsoft, float *soft)
{
  /* the burst geometry / TOA gate every call site applies (k_demod additionally sends an odd offset or length to its other,
     exact path; k_normal_fused does not) */
  if (!(n >= 92 * sps && n <= 157 * sps && n % sps == 0 && fabsf(toa) <= 4096.0f)) return -1;
  if (nsoft < 0 || nsoft > 148) return -1;
  /* ((complex)1.0)/channel: Complex.h:85 and :154-160, each operation rounded */
  const float n2 = amp.i * amp.i + amp.r * amp.r;
  const float cr = amp.r / n2, ci = -amp.i / n2;
  so_c32 inv;
  inv.r = 1.0f * cr - 0.0f * ci;
  inv.i = 1.0f * ci + 0.0f * cr;
  const float delay = -toa;
  const int io = (int)floorf(delay);
  const float frac = delay - (float)io;
  const int filt = fabs((double)frac) > 1e-2;
  const float f512 = frac * 512.0f;
  const int f = (int)f512;
  float xm = 0.0f;
  for (int k = 0; k < n; k++) xm = fmaxf(xm, fmaxf(fabsf(x[k].r), fabsf(x[k].i)));
  const float inv1 = fabsf(inv.r) + fabsf(inv.i);
  const float Z = xm * inv1;
  const int eligible = (f < 512) && ((float)f == f512) && (xm >= 1e-15f) && (xm <= 1e15f) && (inv1 >= 1e-15f) &&
                       (inv1 <= 1e15f) && (Z <= zmax);
  if (!eligible) return 0;
  const float *tp = sinc_grid + (size_t)row * f;
  const float guard = fmaf(Z, 3.0517578125e-05f, 2.384185791015625e-07f);
  float sv[148];
  for (int m = 0; m < nsoft; m++) {
    const int t = sps * m - io;
    const int in_range = t >= 0 && t < n;
    float yr = 0.0f, yi = 0.0f;
    if (filt) {
      for (int j = 0; j < 21; j++) {
        const int k = t + 10 - j;
        const float xr = (k >= 0 && k < n) ? x[k].r : 0.0f, xi = (k >= 0 && k < n) ? x[k].i : 0.0f;
        yr = fmaf(xr, tp[j], yr);
        yi = fmaf(xi, tp[j], yi);
      }
    } else if (in_range) {
      yr = x[t].r; yi = x[t].i;
    }
    const so_c32 rv = rev[sps * m];
    const float a = fmaf(rv.r, inv.r, -(rv.i * inv.i));
    const float b = fmaf(rv.r, inv.i, rv.i * inv.r);
    const float re = fmaf(a, yr, -(b * yi));
    float s = fmaf(re, 0.5f, 0.5f);
    s = fminf(fmaxf(s, 0.0f), 1.0f);
    sv[m] = in_range ? s : 0.5f;
    if (in_range && !(fabsf(re) > guard)) return 0;
  }
  memcpy(soft, sv, sizeof(float) * (size_t)nsoft);
  return 1;
}

void so_demod_tol_batch(const so_c32 *x, const int *off, const int *len, int B, int sps, const so_c32 *amp,
                        const float *toa, const float *sinc_grid, int row, const so_c32 *rev, float zmax,
                        signed char *taken, float *soft, int nsoft, int nthreads)
{
#ifdef _OPENMP
  if (nthreads < 1) nthreads = 1;
#pragma omp parallel for num_threads(nthreads) schedule(static)
#endif
  for (int i = 0; i < B; i++)
    taken[i] = (signed char)so_demod_tol(x + off[i], len[i], sps, amp[i], toa[i], sinc_grid, row, rev, zmax, nsoft,
                                         soft + (size_t)i * nsoft);
  (void)nthreads;
}

void so_demod_batch(const so_ctx *c, const so_c32 *x, const int *off, const int *len, int B, const so_c32 *amp,
                    const float *toa, float *soft, int nsoft, int nthreads)
{
#ifdef _OPENMP
  if (nthreads < 1) nthreads = 1;
#pragma omp parallel for num_threads(nthreads) schedule(static)
#endif
  for (int i = 0; i < B; i++) {
    float s[157 + 4];
    if (len[i] > 157 * c->sps) { memset(soft + (size_t)i * nsoft, 0, sizeof(float) * (size_t)nsoft); continue; }
    const int ns = so_demodulate(c, x + off[i], len[i], amp[i], toa[i], s);
    for (int k = 0; k < nsoft; k++) soft[(size_t)i * nsoft + k] = k < ns ? s[k] : 0.0f;
  }
  (void)nthreads;
}
