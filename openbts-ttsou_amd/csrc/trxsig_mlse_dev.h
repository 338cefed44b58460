// trxsig_mlse_dev.h -- device code the sequence-equaliser kernels share (k_mlse, trxsig_mlse.hip; k_mlse_div,
// trxsig_mlse_div.hip; k_mlse_irc, trxsig_mlse_irc.hip): the row permute, the expected values of a branch, its metric, the
// whitening of the second antenna and the demodulator's slicer.
// Numerical contract as everywhere: one float32 operation at a time, nothing fused (-ffp-contract=off).
#pragma once
#include "trxsig_demod.h"

namespace {

#define TRX_MLSE_WAVES 4                                    /* waves per workgroup: eight bursts */
#define TRX_MLSE_NY 152                                     /* symbols kept per burst (148, padded to a multiple of 8) */
#define TRX_MLSE_INF __builtin_inff()

__device__ __forceinline__ float bperm(int byte_addr, float v) {
  return __int_as_float(__builtin_amdgcn_ds_bpermute(byte_addr, __float_as_int(v)));
}
__device__ __forceinline__ float sgn(float v, int plus) { return plus ? v : -v; }
// Z[x] = sum_k g[k] * (+-1): starts from g[0] * (+-1), adds k = 1..4 in order; the sign is bit k of x (the flips are exact)
__device__ __forceinline__ cx mlse_expected(const cx (&g)[5], int x) {
  cx z = mk(sgn(g[0].r, x & 1), sgn(g[0].i, x & 1));
#pragma unroll
  for (int k = 1; k < 5; k++) z = cadd(z, mk(sgn(g[k].r, (x >> k) & 1), sgn(g[k].i, (x >> k) & 1)));
  return z;
}
__device__ __forceinline__ float mlse_gamma(cx y, cx z) {
  const float dr = y.r - z.r, di = y.i - z.i;
  return dr * dr + di * di;
}
// k_mlse_irc's whitening of antenna 1 (trxsig_mlse_irc.hip; the LDL form, no square root): A v1 - conj(x) v0, x = xr + i xi, as
// A*v1.re - (xr*v0.re + xi*v0.im) and A*v1.im - (xr*v0.im - xi*v0.re), one float32 operation at a time
__device__ __forceinline__ cx mlse_whiten(float A, float xr, float xi, cx v0, cx v1) {
  return mk(A * v1.r - (xr * v0.r + xi * v0.i), A * v1.i - (xr * v0.i - xi * v0.r));
}
// the demodulator's slicer on a symbol (vectorSlicer, sigProcLib.cpp:513-515; see demod_core)
__device__ __forceinline__ float mlse_slice(float re) {
  float sv = (re + 1.0F) * 0.5F;
  if (sv > 1.0f) sv = 1.0f;
  if (sv < 0.0f) sv = 0.0f;
  return sv;
}

}  // namespace
