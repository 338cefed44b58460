// trxsig_mlse_dev.h -- device code the six sequence-equaliser kernels share (k_mlse, trxsig_mlse.hip; k_mlse_div,
// trxsig_mlse_div.hip; k_mlse_irc, trxsig_mlse_irc.hip; k_mlse_access, trxsig_mlse_access.hip; k_mlse_sch, trxsig_mlse_sch.hip;
// k_sch_fit, trxsig_sch_fit.hip), each step once:
//   mlse_enabled, mlse_symbols, mlse_zero     a burst's test, its 148 rotated symbols in LDS (all six)
//   mlse_corr_tap, mlse_ls_tap                one tap of the estimate: midamble correlation / a row of a least-squares table
//   mlse_window, mlse_window2                 the best five of nine taps, for one antenna / one window for two
//   mlse_trellis, mlse_trellis2               a row's forward and backward pass, one antenna / two (summed or whitened metric)
//   mlse_soft_out, mlse_put, mlse_fall_back   the soft and hard bits out
//   bperm, sgn, mlse_expected, mlse_gamma, mlse_whiten, mlse_slice: the small pieces under them
//   mlse_launch                               the six launchers' host side: guard, grid, sps dispatch (arguments: TrxMlseArgs, trxsig_launch.h)
// A kernel keeps what is its own: its LDS, the loop over its bursts, which symbols its estimate reads, the start state and the map
// from trellis step to symbol.  Numerical contract as everywhere: one float32 operation at a time, nothing fused
// (-ffp-contract=off); every operand order and association order below is part of it.
#pragma once
#include <type_traits>

#include "trxsig_demod.h"

namespace {

#define TRX_MLSE_WAVES 4                                    /* waves per workgroup: eight bursts */
#define TRX_MLSE_NY 152                                     /* symbols kept per burst (148, padded to a multiple of 8) */
#define TRX_MLSE_INF __builtin_inff()

// a launcher's body: nothing to do without bursts, nsoft inside 0..148 where the kind has soft bits (SOFT), a workgroup per PER
// bursts; go(S, grid, block) launches the instantiation for decltype(S)::value samples per symbol
template <int PER, bool SOFT, class Go>
hipError_t mlse_launch(int sps, const TrxMlseArgs &a, Go go) {
  if (a.B <= 0) return hipSuccess;
  if (SOFT && (a.nsoft < 0 || a.nsoft > 148)) return hipErrorInvalidValue;
  const dim3 grid((a.B + PER - 1) / PER), block(64 * TRX_MLSE_WAVES);
  switch (sps) {
    case 1: go(std::integral_constant<int, 1>(), grid, block); break;
    case 2: go(std::integral_constant<int, 2>(), grid, block); break;
    case 4: go(std::integral_constant<int, 4>(), grid, block); break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

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

// ---- 1. symbols ----
// k_demod's test on a burst descriptor, and the caller's flags: all bits of need_mask, or any bit where need_mask is 0
template <int SPS>
__device__ __forceinline__ bool mlse_enabled(int off, int N, float toa, const uint8_t *flags, int need_mask, int b) {
  bool enabled = (off >= 0) && (N >= 92 * SPS) && (N <= 157 * SPS) && (N % SPS == 0) && (fabsf(toa) <= 4096.0f);
  if (flags) enabled = enabled && (need_mask ? ((flags[b] & need_mask) == need_mask) : (flags[b] != 0));
  return enabled;
}
// a burst that is not enabled: its trellis rows run on zeros, and nothing of theirs is stored
__device__ __forceinline__ void mlse_zero(cx *Y, int lane) {
  for (int m = lane; m < TRX_MLSE_NY; m += 64) Y[m] = mk(0, 0);
}
// The whole wave forms one enabled burst's symbols with k_demod's own code (demod_core, RAW form: scaleVector(1/amp),
// delayVector(-TOA) at the decimated instants) through the wave's staging area `stage`, rotates the 148 outputs by rev[sps m] and
// keeps them, complex, in Y[0..151].  Returns whether the burst has to fall back to the demodulator's soft bits: a symbol that is
// not below 2^30 in magnitude (any lane's), or fewer than 148 symbols.  Wave-uniform arguments, wave-uniform result.
template <int SPS>
__device__ __forceinline__ bool mlse_symbols(const TrxTables *T, cx *stage, const void *samples, int off, int N, const cx &amp, float toa,
                                             int lane, cx *Y) {
  constexpr int NLD = (157 * SPS / 2 + 63) / 64;
  const bool wide = (off & 1) == 0;                         // (per antenna: the two offsets of a burst may differ in parity)
  float4 v[NLD];
#pragma unroll
  for (int i = 0; i < NLD; i++) v[i] = make_float4(0, 0, 0, 0);
  if (wide) {
#pragma unroll
    for (int i = 0; i < NLD; i++) {
      const int q = lane + 64 * i;
      if (q < N / 2) v[i] = SmpC32::ld2(samples, off, q);
    }
  }
  wave_lds_fence();                                         // the staging area's readers of the burst before are done
  demod_core<SPS, true, 148>(T, stage, samples, off, N, wide, v, amp, toa, lane, nullptr, nullptr, Y, 148);
  wave_lds_fence();
  // GMSKReverseRotate at the decimated instants, both parts kept: the reference's complex product with rev[sps m]
  bool bad = false;
  const cx *rev = T->rev;
  for (int m = lane; m < TRX_MLSE_NY; m += 64) {
    cx y = mk(0, 0);
    if (m < 148 && m < N / SPS) {                          // (a short burst's symbols past its end are zeros: demodulateBurst has none there)
      y = cmul(Y[m], rev[SPS * m]);
      bad = bad || !(fabsf(y.r) < 0x1p30f) || !(fabsf(y.i) < 0x1p30f);
    }
    Y[m] = y;
  }
  return __builtin_amdgcn_ballot_w64(bad) != 0 || N / SPS < 148;
}

// ---- 2. the estimate ----
// c[d] of a normal burst: the midamble's 16 middle symbols (training bits 5..20) against y[66 + d .. 81 + d], sign flips, then 1/16
__device__ __forceinline__ cx mlse_corr_tap(unsigned tsc_bits, int d, const cx *Y) {
  cx acc = mk(0, 0);
#pragma unroll
  for (int i = 0; i < 16; i++) {
    const cx y = Y[66 + i + d];
    const int plus = (tsc_bits >> (5 + i)) & 1;
    acc = cadd(acc, mk(sgn(y.r, plus), sgn(y.i, plus)));
  }
  return cmulr(acc, 0.0625f);
}
// one tap of a least-squares estimate: a row of NROW table words against y[row0 .. row0 + NROW - 1], from 0 in ascending order.
// The table is in constant memory and read by plain global loads, each lane its own row: read once per wave, L2- and L1-resident for
// the whole launch, independent of everything before them and so in flight while the symbols are still being computed.
template <int NROW>
__device__ __forceinline__ cx mlse_ls_tap(const float *row, const cx *Y, int row0) {
  float ar = 0.0f, ai = 0.0f;
#pragma unroll
  for (int i = 0; i < NROW; i++) {
    const cx y = Y[row0 + i];
    const float pk = row[i];
    ar = ar + pk * y.r;
    ai = ai + pk * y.i;
  }
  return mk(ar, ai);
}
// The window: the five consecutive taps of c[-4..4] with the most energy, w = 0, -1 .. -4 the first of them; w = 0 unless an
// earlier window has strictly more (a later q only on a strict >).  NA antennas share one window, chosen on the summed tap powers,
// antenna 0's first.  Antenna a's nine taps are at c9[9 a .. 9 a + 8] (LDS, written by lanes 0..8 before a fence; every lane picks
// for itself); h[a] takes its five.  Returns E, the window's energy.
// (How this is written decides registers in the callers: the taps as floats, part by part -- a cx copied whole becomes an integer
//  load --, both antennas' selects under one test, and E as the returned value.)
template <int NA>
__device__ __forceinline__ float mlse_window_n(const cx *c9, cx (&h)[NA][5], int &w) {
  float cr[NA][9], ci[NA][9], p[9];
#pragma unroll
  for (int i = 0; i < 9; i++) {
#pragma unroll
    for (int a = 0; a < NA; a++) { cr[a][i] = c9[9 * a + i].r; ci[a][i] = c9[9 * a + i].i; }
    p[i] = cr[0][i] * cr[0][i] + ci[0][i] * ci[0][i];
    if (NA == 2) p[i] = p[i] + (cr[1][i] * cr[1][i] + ci[1][i] * ci[1][i]);
  }
  w = 0;
  float E = (((p[4] + p[5]) + p[6]) + p[7]) + p[8];
#pragma unroll
  for (int q = 1; q <= 4; q++) {                            // w = -q
    const float Ew = (((p[4 - q] + p[5 - q]) + p[6 - q]) + p[7 - q]) + p[8 - q];
    if (Ew > E) { E = Ew; w = -q; }
  }
#pragma unroll
  for (int k = 0; k < 5; k++) {
#pragma unroll
    for (int a = 0; a < NA; a++) { h[a][k].r = cr[a][4 + k]; h[a][k].i = ci[a][4 + k]; }
#pragma unroll
    for (int q = 1; q <= 4; q++) {
      if (w == -q) {
#pragma unroll
        for (int a = 0; a < NA; a++) { h[a][k].r = cr[a][4 - q + k]; h[a][k].i = ci[a][4 - q + k]; }
      }
    }
  }
  return E;
}
__device__ __forceinline__ float mlse_window(const cx *c9, cx (&h)[5], int &w) {
  cx hh[1][5];
  const float E = mlse_window_n<1>(c9, hh, w);
#pragma unroll
  for (int k = 0; k < 5; k++) { h[k].r = hh[0][k].r; h[k].i = hh[0][k].i; }
  return E;
}
__device__ __forceinline__ float mlse_window2(const cx *c18, cx (&h0)[5], cx (&h1)[5], int &w) {
  cx hh[2][5];
  const float E = mlse_window_n<2>(c18, hh, w);
#pragma unroll
  for (int k = 0; k < 5; k++) { h0[k].r = hh[0][k].r; h0[k].i = hh[0][k].i; h1[k].r = hh[1][k].r; h1[k].i = hh[1][k].i; }
  return E;
}

// ---- 3. the trellis of a 16-lane row; lane s of the row is state s ----
// A state's two predecessors (s >> 1, (s >> 1) | 8) and its two successors ((2 s) & 15 and the next) come across the row by
// ds_bpermute: their byte addresses
struct MlsePerm { int pf0, pf1, pb0, pb1; };
__device__ __forceinline__ MlsePerm mlse_perm(int lane) {
  const int rowbase = lane & 48, s = lane & 15;
  MlsePerm a;
  a.pf0 = 4 * (rowbase | (s >> 1)); a.pf1 = a.pf0 + 32;
  a.pb0 = 4 * (rowbase | ((2 * s) & 15)); a.pb1 = a.pb0 + 4;
  return a;
}
// What both trellises do with alpha + beta after step i (alpha and beta both after that step): the minimum over the eight states
// of one parity in three DPP steps, the other parity's by a fourth, M_0 - M_1.
__device__ __forceinline__ float mlse_llr(float t, int s) {
  t = fminf(t, dpp_f<0x4E>(t));                             // lane ^ 2
  t = fminf(t, dpp_f<0x124>(t));                            // the row rotated by 4
  t = fminf(t, dpp_f<0x128>(t));                            // ... by 8: the minimum over the eight states of this lane's parity
  const float o = dpp_f<0xB1>(t);                           // lane ^ 1: the other parity's
  return (s & 1) ? o - t : t - o;                           // M_0 - M_1
}

// STEPS steps of max-log-MAP on one antenna.  Step i works on Y[yi + i dir]; the last three steps are tail symbols (-1: only
// even states are entered).  zf0, zf1: the expected values into state s from s >> 1 and (s >> 1) | 8.  scr: the row's words of
// the dead staging area, where the caller has parked them as scr[12 + s] = zf0, scr[28 + s] = zf1 (with whatever else it wants
// after the trellis): the way back needs Z[2 s], Z[2 s + 1] (out of state s with b = 0, 1) and the STEPS forward metrics want the
// registers.  D[i >> 4] of lane i % 16 comes back as M_0 - M_1 of step i; the caller hands D in as zeros (`float D[n] = {0.0f, ..}`:
// one initialiser for the whole array keeps it the register group the kernels had, cleared element by element here it is not).
// Both loops are fully unrolled: the forward metrics of a lane stay in STEPS VGPRs until the backward pass meets them.  A
// scheduling fence per step, the next step's symbol fetched ahead of it: left alone, the scheduler hoists the LDS reads and their
// metrics to the front of the unrolled loop and k_mlse needs 216 VGPRs instead of fewer than 128.
template <int STEPS>
__device__ __forceinline__ void mlse_trellis(const cx *Y, int yi, int dir, cx zf0, cx zf1, cx *scr, int lane, int start,
                                             float (&D)[(STEPS + 15) / 16]) {
  const int s = lane & 15;
  const MlsePerm pa = mlse_perm(lane);
  float A[STEPS];
  float al = (s == start) ? 0.0f : TRX_MLSE_INF;
  cx y = Y[yi];
#pragma unroll
  for (int i = 0; i < STEPS; i++) {
    if (i < STEPS - 1) yi += dir;
    const cx yn = Y[yi];
    float g0 = mlse_gamma(y, zf0), g1 = mlse_gamma(y, zf1);
    if (i >= STEPS - 3 && (s & 1)) { g0 = TRX_MLSE_INF; g1 = TRX_MLSE_INF; }       // the tail symbols are -1
    const float a0 = bperm(pa.pf0, al) + g0, a1 = bperm(pa.pf1, al) + g1;
    al = fminf(a0, a1);
    A[i] = al;
    y = yn;                                                 // (after the last step the symbol is that step's again: the backward pass starts there)
    __builtin_amdgcn_sched_barrier(0);
  }
  wave_lds_fence();
  const cx zb0 = scr[12 + 2 * s], zb1 = scr[13 + 2 * s];
  asm volatile("" : "+v"(yi));                              // (or the addresses of the way up are kept in registers for the way back)
  float be = 0.0f;
#pragma unroll
  for (int i = STEPS - 1; i >= 0; i--) {
    if (i > 0) yi -= dir;
    const cx yn = Y[yi];
    const float diff = mlse_llr(A[i] + be, s);
    if ((i & 15) == s) D[i >> 4] = diff;
    asm volatile("" : "+v"(D[i >> 4]));                     // (the select happens here: not STEPS differences kept for a chain of selects after the loop)
    if (i > 0) {
      const float g0 = mlse_gamma(y, zb0);
      const float g1 = (i >= STEPS - 3) ? TRX_MLSE_INF : mlse_gamma(y, zb1);
      const float b0 = g0 + bperm(pa.pb0, be), b1 = g1 + bperm(pa.pb1, be);
      be = fminf(b0, b1);
    }
    y = yn;
    __builtin_amdgcn_sched_barrier(0);
  }
}

// a branch metric over two antennas, antenna 0's first; WEIGHTED: det on antenna 0's (k_mlse_irc: antenna 1 is whitened)
template <bool WEIGHTED>
__device__ __forceinline__ float mlse_gamma2(float det, cx y0, cx z0, cx y1, cx z1) {
  if (WEIGHTED) return det * mlse_gamma(y0, z0) + mlse_gamma(y1, z1);
  return mlse_gamma(y0, z0) + mlse_gamma(y1, z1);
}
// The same on two antennas' symbols with the row's taps g0, g1 (already in the row's direction; det is read only where WEIGHTED).
// Two sets of Z[32] would not fit the row's scratch at sps 1: the caller's lane 0 has parked the taps as scr[20 + k] = g0[k],
// scr[25 + k] = g1[k], and the way back forms its own expected values from them again.
template <int STEPS, bool WEIGHTED>
__device__ __forceinline__ void mlse_trellis2(const cx *Y0, const cx *Y1, int yi, int dir, const cx (&g0)[5], const cx (&g1)[5], float det,
                                              cx *scr, int lane, int start, float (&D)[(STEPS + 15) / 16]) {
  const int s = lane & 15;
  const MlsePerm pa = mlse_perm(lane);
  // zf<b><antenna>: into state s from s >> 1 (b = 0), (s >> 1) | 8 (b = 1)
  const cx zf00 = mlse_expected(g0, s), zf10 = mlse_expected(g0, s | 16);
  const cx zf01 = mlse_expected(g1, s), zf11 = mlse_expected(g1, s | 16);
  float A[STEPS];
  float al = (s == start) ? 0.0f : TRX_MLSE_INF;
  cx y0 = Y0[yi], y1 = Y1[yi];
#pragma unroll
  for (int i = 0; i < STEPS; i++) {
    if (i < STEPS - 1) yi += dir;
    const cx yn0 = Y0[yi], yn1 = Y1[yi];
    float m0 = mlse_gamma2<WEIGHTED>(det, y0, zf00, y1, zf01);
    float m1 = mlse_gamma2<WEIGHTED>(det, y0, zf10, y1, zf11);
    if (i >= STEPS - 3 && (s & 1)) { m0 = TRX_MLSE_INF; m1 = TRX_MLSE_INF; }       // the tail symbols are -1
    const float a0 = bperm(pa.pf0, al) + m0, a1 = bperm(pa.pf1, al) + m1;
    al = fminf(a0, a1);
    A[i] = al;
    y0 = yn0; y1 = yn1;
    __builtin_amdgcn_sched_barrier(0);
  }
  wave_lds_fence();
  cx zb00, zb10, zb01, zb11;                                // zb<b><antenna>: out of state s with b = 0, 1 -- Z[2 s], Z[2 s + 1]
  {
    cx b0[5], b1[5];
#pragma unroll
    for (int k = 0; k < 5; k++) { b0[k] = scr[20 + k]; b1[k] = scr[25 + k]; }
    zb00 = mlse_expected(b0, 2 * s); zb10 = mlse_expected(b0, 2 * s + 1);
    zb01 = mlse_expected(b1, 2 * s); zb11 = mlse_expected(b1, 2 * s + 1);
  }
  asm volatile("" : "+v"(yi));
  float be = 0.0f;
#pragma unroll
  for (int i = STEPS - 1; i >= 0; i--) {
    if (i > 0) yi -= dir;
    const cx yn0 = Y0[yi], yn1 = Y1[yi];
    const float diff = mlse_llr(A[i] + be, s);
    if ((i & 15) == s) D[i >> 4] = diff;
    asm volatile("" : "+v"(D[i >> 4]));
    if (i > 0) {
      const float m0 = mlse_gamma2<WEIGHTED>(det, y0, zb00, y1, zb01);
      const float m1 = (i >= STEPS - 3) ? TRX_MLSE_INF : mlse_gamma2<WEIGHTED>(det, y0, zb10, y1, zb11);
      const float b0 = m0 + bperm(pa.pb0, be), b1 = m1 + bperm(pa.pb1, be);
      be = fminf(b0, b1);
    }
    y0 = yn0; y1 = yn1;
    __builtin_amdgcn_sched_barrier(0);
  }
}

// ---- 4 / 5. soft bits out ----
__device__ __forceinline__ void mlse_put(float *sb, uint8_t *hb, int m, float sv) {
  sb[m] = sv;
  if (hb) hb[m] = sv > 0.5F;
}
// a decided symbol: 0.5 + (M_0 - M_1) / (8 E), one correctly rounded division, clamped to [0, 1]
__device__ __forceinline__ void mlse_soft_out(float *sb, uint8_t *hb, int m, float d, float den) {
  float sv = 0.5f + d / den;
  if (sv > 1.0f) sv = 1.0f;
  if (sv < 0.0f) sv = 0.0f;
  mlse_put(sb, hb, m, sv);
}
// a burst that was not equalised, symbols first, first + step, ... below nsoft: the demodulator's formula where it fell back
// (st = 1), zeros where it was not enabled
__device__ __forceinline__ void mlse_fall_back(float *sb, uint8_t *hb, const cx *Y, int st, int first, int step, int nsoft) {
  for (int m = first; m < nsoft; m += step) mlse_put(sb, hb, m, st == 1 ? mlse_slice(Y[m].r) : 0.0f);
}

}  // namespace
