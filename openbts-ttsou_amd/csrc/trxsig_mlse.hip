// trxsig_mlse.hip -- the sequence equaliser for normal bursts (trxsig_mlse_batch; the Transceiver group's TRXSIG_TSCLEG_MLSE):
// a per-burst channel estimate from the midamble and a 16-state max-log-MAP equaliser that hands up soft bits, at any sps.
// The reference has no counterpart (Transceiver/README.Talgorithm only sketches one); the stage is pinned by a float32 model,
// tests/mlse_model.py, which this kernel equals word for word.  The arithmetic is float add, subtract, multiply, minimum,
// compare and one correctly rounded division per soft bit; nothing is fused (-ffp-contract=off), nothing is transcendental.
// The algorithm is stated in include/trxsig.h (trxsig_mlse_batch) and again, operation by operation, in the model.
// The model, and this kernel directly (tests/test_gpu_mlse_ref.py), are graded against a float64 statement of the same soft bits
// as minima over symbol sequences, tests/mlse_ref.py: |soft - clamp(soft64)| <= 1.001 ((2 Q + 124 P) / (8 E) + 5) 2^-24 per burst
// and half (P, Q: sums over the steps of the largest branch metric and of its rounding terms; derived there), exact clamps
// beyond that bound and equal hard bits outside it.
//
// Layout.  One wave takes TWO bursts.
//   * Symbols: the whole wave computes one burst at a time with k_demod's own code (demod_core, RAW form: scaleVector(1/amp),
//     delayVector(-TOA) at the decimated instants), then rotates the 148 outputs by rev[sps m] and keeps them, complex, in LDS.
//   * Trellis: each of the wave's four 16-lane rows is one half-burst trellis (rows 0, 1: the first burst's right and left half;
//     rows 2, 3: the second burst's); lane s of a row is state s.  A state's two predecessors (s >> 1, (s >> 1) | 8) and its two
//     successors come across the row by ds_bpermute; the minimum over the eight states of one parity is three DPP steps
//     (lane ^ 2, the row rotated by 4, by 8).  The received symbol of a step is one LDS broadcast read per row.
//   * The 61 forward metrics of a lane stay in 61 VGPRs until the backward pass meets them (both loops fully unrolled): no LDS
//     for them, so the staging area (5.0 KB at sps 4) and the two symbol vectors (2.4 KB) are all a wave holds -- 20 waves
//     = 40 bursts in flight per CU, where 2 x 2 x 3.9 KB of metrics in LDS would leave 7.  Listing (gfx950, sps 4): 82 VGPRs,
//     90 SGPRs, no scratch, 29,824 B of LDS per workgroup: five waves per SIMD either way (DESIGN.md says what it took).
//   * The difference M_0 - M_1 of step i is kept by lane i % 16 (four registers); the divisions and the stores come after the loop.
#include "trxsig_mlse_dev.h"                               // bperm, sgn, mlse_expected, mlse_gamma, mlse_slice: shared with k_mlse_div

namespace {

// (amdgpu_waves_per_eu(4): a ceiling of 128 VGPRs for the register allocator -- occupancy decides for a dependent chain)
template <int SPS>
__global__ __launch_bounds__(64 * TRX_MLSE_WAVES) __attribute__((amdgpu_waves_per_eu(4)))
void k_mlse(const TrxTables *__restrict__ T, const void *__restrict__ samples, const int32_t *__restrict__ offset,
            const int32_t *__restrict__ length, int B, unsigned tsc_bits /* bit j = training-sequence bit j */,
            const cx *__restrict__ amp_in, const float *__restrict__ toa_in, const uint8_t *__restrict__ flags, int need_mask,
            cx *__restrict__ chan, int32_t *__restrict__ win, float *__restrict__ soft, uint8_t *__restrict__ hard, int nsoft, int stride) {
  typedef DemodGeom<SPS, 148> G;
  __shared__ cx ph[TRX_MLSE_WAVES][G::U];
  __shared__ cx ysh[TRX_MLSE_WAVES][2][TRX_MLSE_NY];

  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int bw = 2 * (blockIdx.x * TRX_MLSE_WAVES + wave);   // the wave's first burst (wave-uniform)
  if (bw >= B) return;

  // ---- 1. symbols, a burst at a time on the whole wave.  state[j]: 0 = equalise, 1 = fall back, 2 = not enabled ----
  int state[2] = {2, 2};
#pragma unroll
  for (int j = 0; j < 2; j++) {
    const int b = bw + j;                                   // wave-uniform
    cx *Y = ysh[wave][j];
    bool enabled = false;
    int off = 0, N = 0;
    cx amp = mk(1.0f, 0.0f);
    float toa = 0.0f;
    if (b < B) {
      off = offset[b]; N = length[b]; amp = amp_in[b]; toa = toa_in[b];
      enabled = (off >= 0) && (N >= 92 * SPS) && (N <= 157 * SPS) && (N % SPS == 0) && (fabsf(toa) <= 4096.0f);   // k_demod's test
      if (flags) enabled = enabled && (need_mask ? ((flags[b] & need_mask) == need_mask) : (flags[b] != 0));
    }
    if (!__builtin_amdgcn_readfirstlane(enabled)) {
      for (int m = lane; m < TRX_MLSE_NY; m += 64) Y[m] = mk(0, 0);      // (the trellis rows of this burst run on zeros; nothing of theirs is stored)
      continue;
    }
    constexpr int NLD = (157 * SPS / 2 + 63) / 64;
    const bool wide = (off & 1) == 0;
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
    wave_lds_fence();                                       // the staging area's readers of the burst before are done
    demod_core<SPS, true, 148>(T, ph[wave], samples, off, N, wide, v, amp, toa, lane, nullptr, nullptr, Y, 148);
    wave_lds_fence();
    // GMSKReverseRotate at the decimated instants, both parts kept: the reference's complex product with rev[sps m]
    bool bad = false;
    const cx *rev = T->rev;
    for (int m = lane; m < TRX_MLSE_NY; m += 64) {
      cx y = mk(0, 0);
      if (m < 148 && m < N / SPS) {                        // (a short burst's symbols past its end are zeros: demodulateBurst has none there)
        y = cmul(Y[m], rev[SPS * m]);
        bad = bad || !(fabsf(y.r) < 0x1p30f) || !(fabsf(y.i) < 0x1p30f);
      }
      Y[m] = y;
    }
    state[j] = (__builtin_amdgcn_ballot_w64(bad) != 0 || N / SPS < 148) ? 1 : 0;
  }
  wave_lds_fence();

  // ---- 2. channel estimate; every row works its burst's out for itself (lanes 0..8: c[-4..4]) ----
  const int s = lane & 15;                                  // the state this lane carries
  const int j = lane >> 5;                                  // which of the wave's two bursts
  const bool left = (lane >> 4) & 1;                        // which half of it
  const int b = bw + j;
  const cx *Y = ysh[wave][j];
  cx *scr = ph[wave] + 44 * (lane >> 4);                    // this row's 44 words of the (dead) staging area: c[9], (E, w), state, Z[32] from word 12
  {
    const int d = (s < 9 ? s : 8) - 4;
    cx acc = mk(0, 0);
#pragma unroll
    for (int i = 0; i < 16; i++) {
      const cx y = Y[66 + i + d];
      const int plus = (tsc_bits >> (5 + i)) & 1;
      acc = cadd(acc, mk(sgn(y.r, plus), sgn(y.i, plus)));
    }
    if (s < 9) scr[s] = cmulr(acc, 0.0625f);
  }
  wave_lds_fence();
  cx c[9];
  float p[9];
#pragma unroll
  for (int i = 0; i < 9; i++) { c[i] = scr[i]; p[i] = c[i].r * c[i].r + c[i].i * c[i].i; }
  int w = 0;
  float E = (((p[4] + p[5]) + p[6]) + p[7]) + p[8];
#pragma unroll
  for (int q = 1; q <= 4; q++) {                            // w = -q; a later window only on a strict >
    const float Ew = (((p[4 - q] + p[5 - q]) + p[6 - q]) + p[7 - q]) + p[8 - q];
    if (Ew > E) { E = Ew; w = -q; }
  }
  cx h[5];
#pragma unroll
  for (int k = 0; k < 5; k++) {
    h[k] = c[4 + k];
#pragma unroll
    for (int q = 1; q <= 4; q++) if (w == -q) h[k] = c[4 - q + k];
  }
  int st = j ? state[1] : state[0];
  if (st == 0 && E == 0.0f) st = 1;

  const int hl = lane & 31;                                 // lane within the burst's two rows
  if (b < B) {
    if (win && hl == 0) win[b] = st == 0 ? w : st;
    if (chan && hl < 5) {
      cx hv = mk(0, 0);
#pragma unroll
      for (int k = 0; k < 5; k++) if (st == 0 && hl == k) hv = h[k];
      chan[(size_t)b * 5 + hl] = hv;
    }
  }

  // ---- 3. the half-burst trellis of this row ----
  cx g[5];
#pragma unroll
  for (int k = 0; k < 5; k++) g[k] = left ? h[4 - k] : h[k];
  const cx zf0 = mlse_expected(g, s), zf1 = mlse_expected(g, s | 16);            // into state s from s >> 1, (s >> 1) | 8
  // (the way back needs Z[2 s], Z[2 s + 1] -- out of state s with b = 0, 1 -- and E, w and the burst's state are wanted after it: all
  //  parked in LDS meanwhile, the 61 forward metrics want the registers)
  scr[12 + s] = zf0; scr[28 + s] = zf1;
  if (s == 0) { scr[9] = mk(E, __int_as_float(w)); scr[10] = mk(__int_as_float(st), 0.0f); }
  const int rowbase = lane & 48;
  const int pf0 = 4 * (rowbase | (s >> 1)), pf1 = pf0 + 32;
  const int pb0 = 4 * (rowbase | ((2 * s) & 15)), pb1 = pb0 + 4;
  // start state: bit 0 first a[86], a[85], a[84], a[83] (right) or a[61], a[62], a[63], a[64] (left); a[61 + t] = training bit t
  const int start = left ? (int)(tsc_bits & 15u)
                         : (int)(((tsc_bits >> 25) & 1u) | (((tsc_bits >> 24) & 1u) << 1) | (((tsc_bits >> 23) & 1u) << 2) | (((tsc_bits >> 22) & 1u) << 3));
  // step i = 0..60 is symbol m = 87 + i with sample y[m + w] (right), m = 60 - i with y[m + 4 + w] (left)
  int yi = left ? 64 + w : 87 + w;
  const int dir = left ? -1 : 1;
  // (a scheduling fence per step, the next step's symbol fetched ahead of it: left alone, the scheduler hoists the 61 LDS reads and
  //  their metrics to the front of the unrolled loop and the kernel needs 216 VGPRs instead of fewer than 128)
  float A[61];
  float al = (s == start) ? 0.0f : TRX_MLSE_INF;
  cx y = Y[yi];
#pragma unroll
  for (int i = 0; i < 61; i++) {
    if (i < 60) yi += dir;
    const cx yn = Y[yi];
    float g0 = mlse_gamma(y, zf0), g1 = mlse_gamma(y, zf1);
    if (i >= 58 && (s & 1)) { g0 = TRX_MLSE_INF; g1 = TRX_MLSE_INF; }            // the tail symbols are -1
    const float a0 = bperm(pf0, al) + g0, a1 = bperm(pf1, al) + g1;
    al = fminf(a0, a1);
    A[i] = al;
    y = yn;                                                 // (after step 60 the symbol is that step's again: the backward pass starts there)
    __builtin_amdgcn_sched_barrier(0);
  }
  wave_lds_fence();
  const cx zb0 = scr[12 + 2 * s], zb1 = scr[13 + 2 * s];
  asm volatile("" : "+v"(yi));                              // (or the 61 addresses of the way up are kept in registers for the way back)
  float be = 0.0f;
  float D[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
  for (int i = 60; i >= 0; i--) {
    if (i > 0) yi -= dir;
    const cx yn = Y[yi];
    float t = A[i] + be;                                    // alpha and beta, both after step i
    t = fminf(t, dpp_f<0x4E>(t));                           // lane ^ 2
    t = fminf(t, dpp_f<0x124>(t));                          // the row rotated by 4
    t = fminf(t, dpp_f<0x128>(t));                          // ... by 8: the minimum over the eight states of this lane's parity
    const float o = dpp_f<0xB1>(t);                         // lane ^ 1: the other parity's
    const float diff = (s & 1) ? o - t : t - o;             // M_0 - M_1
    if ((i & 15) == s) D[i >> 4] = diff;
    asm volatile("" : "+v"(D[i >> 4]));                     // (the select happens here: not 61 differences kept for a chain of selects after the loop)
    if (i > 0) {
      const float g0 = mlse_gamma(y, zb0);
      const float g1 = (i >= 58) ? TRX_MLSE_INF : mlse_gamma(y, zb1);
      const float b0 = g0 + bperm(pb0, be), b1 = g1 + bperm(pb1, be);
      be = fminf(b0, b1);
    }
    y = yn;
    __builtin_amdgcn_sched_barrier(0);
  }

  // ---- 4 / 5. soft bits out ----
  if (b >= B) return;
  const float E_ = scr[9].r;
  const int st_ = __float_as_int(scr[10].r);
  float *sb = soft + (size_t)b * stride;
  uint8_t *hb = hard ? hard + (size_t)b * stride : nullptr;
  if (st_ == 0) {
    const float den = 8.0f * E_;
#pragma unroll
    for (int q = 0; q < 4; q++) {
      const int i = 16 * q + s;
      const int m = left ? 60 - i : 87 + i;
      if (i < 61 && m < nsoft) {
        float sv = 0.5f + D[q] / den;
        if (sv > 1.0f) sv = 1.0f;
        if (sv < 0.0f) sv = 0.0f;
        sb[m] = sv;
        if (hb) hb[m] = sv > 0.5F;
      }
    }
    const int m = 61 + hl;                                  // the midamble: the demodulator's formula
    if (hl < 26 && m < nsoft) {
      const float sv = mlse_slice(Y[m].r);
      sb[m] = sv;
      if (hb) hb[m] = sv > 0.5F;
    }
  } else {
    for (int m = hl; m < nsoft; m += 32) {
      const float sv = st_ == 1 ? mlse_slice(Y[m].r) : 0.0f;
      sb[m] = sv;
      if (hb) hb[m] = sv > 0.5F;
    }
  }
}

}  // namespace

hipError_t trx_launch_mlse(hipStream_t st, int sps, const TrxTables *dT, const trx_c32 *samples, const int32_t *off, const int32_t *len, int B,
                           unsigned tsc_bits, const trx_c32 *amp, const float *toa, const uint8_t *flags, int need_mask, trx_c32 *chan,
                           int32_t *win, float *soft, uint8_t *hard, int nsoft, int stride) {
  if (B <= 0) return hipSuccess;
  if (nsoft < 0 || nsoft > 148) return hipErrorInvalidValue;
  const int per = 2 * TRX_MLSE_WAVES;
  const dim3 grid((B + per - 1) / per), block(64 * TRX_MLSE_WAVES);
  switch (sps) {
    case 1: k_mlse<1><<<grid, block, 0, st>>>(dT, samples, off, len, B, tsc_bits, amp, toa, flags, need_mask, chan, win, soft, hard, nsoft, stride); break;
    case 2: k_mlse<2><<<grid, block, 0, st>>>(dT, samples, off, len, B, tsc_bits, amp, toa, flags, need_mask, chan, win, soft, hard, nsoft, stride); break;
    case 4: k_mlse<4><<<grid, block, 0, st>>>(dT, samples, off, len, B, tsc_bits, amp, toa, flags, need_mask, chan, win, soft, hard, nsoft, stride); break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}
