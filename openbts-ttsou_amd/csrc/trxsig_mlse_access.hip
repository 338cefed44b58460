// trxsig_mlse_access.hip -- the sequence equaliser for access bursts (trxsig_mlse_access_batch, trxsig_mlse_rach_batch; the
// Transceiver group's TRXSIG_RACHLEG_MLSE): a nine-tap least-squares channel estimate from the burst's 49 known leading symbols and
// ONE 16-state max-log-MAP trellis of 39 steps over the 36 coded bits and the 3 tail bits, at any sps.  The reference has no
// counterpart; the stage is pinned by the float32 model tests/mlse_access_model.py, which this kernel equals word for word, and
// graded against the float64 statement tests/mlse_access_ref.py.  The arithmetic rules are k_mlse's (trxsig_mlse.hip): float add,
// subtract, multiply, minimum, compare and one correctly rounded division per soft bit; nothing is fused.  The algorithm is stated
// in include/trxsig.h (trxsig_mlse_access_batch) and again, operation by operation, in the model.
//
// Layout.  One wave takes FOUR bursts.
//   * Symbols: as in k_mlse the whole wave computes one burst at a time with k_demod's own code (demod_core, RAW form) and keeps the
//     148 rotated outputs, complex, in LDS.  The loop over the four bursts is NOT unrolled (the bursts' states travel in one packed
//     register): one copy of demod_core in the listing where k_mlse has two.
//   * Estimate: lanes 0..8 of a row form c[-4..4], 41 multiply-adds each on LDS broadcast-free reads of y[4..44].  The table P32
//     (trxsig_mlse_access_tab.h, 1,476 B) is read from constant memory by plain global loads, lane d its own row: a staged copy would
//     cost every wave 1,476 B of LDS (41,028 B per workgroup with the symbols and the staging area at sps 4: over the 40,960 B that
//     four workgroups per CU leave) or a pass through the dead staging area behind one more LDS fence, and it would be read exactly once per
//     wave either way; the 369 words stay in the L2 and the vector L1 for the whole launch, and the 41 loads of a lane are
//     independent of everything before them, so they are in flight while the symbols are still being computed.
//   * Trellis: each of the wave's four 16-lane rows is one burst's trellis; lane s of a row is state s.  Predecessors and successors
//     come across the row by ds_bpermute, the parity minima by the three DPP steps, the received symbol of a step is one LDS
//     broadcast read per row -- all k_mlse's.  The 39 forward metrics of a lane stay in 39 VGPRs (both loops fully unrolled, the
//     per-step scheduling fence that k_mlse needs); M_0 - M_1 of step i is kept by lane i % 16 (three registers).
//   * LDS: the staging area and four symbol vectors a wave.  Listing (gfx950): DESIGN.md 5.4.w and the README.
#define TRX_MLSE_ACCESS_TAB_QUAL static __device__ __constant__ const
#include "trxsig_mlse_access_tab.h"
#include "trxsig_mlse_dev.h"                                // bperm, sgn, mlse_expected, mlse_gamma, mlse_slice: shared with k_mlse

namespace {

#define TRX_MLSE_ACC_FIRST 49                               /* the first symbol the trellis decides */
#define TRX_MLSE_ACC_STEPS 39                               /* 36 coded bits and 3 tail bits */
#define TRX_MLSE_ACC_START 8                                /* a[48], a[47], a[46], a[45] = 0, 0, 0, 1 (bit 0 first; GSM 05.02 5.2.7) */

template <int SPS>
__global__ __launch_bounds__(64 * TRX_MLSE_WAVES) __attribute__((amdgpu_waves_per_eu(4)))
void k_mlse_access(const TrxTables *__restrict__ T, const void *__restrict__ samples, const int32_t *__restrict__ offset,
                   const int32_t *__restrict__ length, int B, const cx *__restrict__ amp_in, const float *__restrict__ toa_in,
                   const uint8_t *__restrict__ flags, int need_mask, cx *__restrict__ chan, int32_t *__restrict__ win,
                   float *__restrict__ soft, uint8_t *__restrict__ hard, int nsoft, int stride) {
  typedef DemodGeom<SPS, 148> G;
  static_assert(4 * 44 <= G::U, "the rows' scratch lies in the staging area");
  __shared__ cx ph[TRX_MLSE_WAVES][G::U];
  __shared__ cx ysh[TRX_MLSE_WAVES][4][TRX_MLSE_NY];

  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int bw = 4 * (blockIdx.x * TRX_MLSE_WAVES + wave);   // the wave's first burst (wave-uniform)
  if (bw >= B) return;

  // ---- 1. symbols, a burst at a time on the whole wave.  Two bits a burst in `states`: 0 = equalise, 1 = fall back, 2 = not enabled ----
  int states = 0;
#pragma unroll 1
  for (int j = 0; j < 4; j++) {
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
      for (int m = lane; m < TRX_MLSE_NY; m += 64) Y[m] = mk(0, 0);      // (the trellis row of this burst runs on zeros; nothing of its is stored)
      states |= 2 << (2 * j);
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
    if (__builtin_amdgcn_ballot_w64(bad) != 0 || N / SPS < 148) states |= 1 << (2 * j);
  }
  wave_lds_fence();

  // ---- 2. channel estimate: lanes 0..8 of a row form c[-4..4] = P32 y[4..44]; every lane of the row then reads all nine ----
  const int s = lane & 15;                                  // the state this lane carries
  const int j = lane >> 4;                                  // which of the wave's four bursts
  const int b = bw + j;
  const cx *Y = ysh[wave][j];
  cx *scr = ph[wave] + 44 * j;                              // this row's 44 words of the (dead) staging area: c[9], (E, w), state, Z[32] from word 12
  {
    const float *P = trx_mlse_access_p32 + TRX_MLSE_ACCESS_NROW * (s < 9 ? s : 8);
    float ar = 0.0f, ai = 0.0f;
#pragma unroll
    for (int i = 0; i < TRX_MLSE_ACCESS_NROW; i++) {
      const cx y = Y[4 + i];
      const float pk = P[i];
      ar = ar + pk * y.r;
      ai = ai + pk * y.i;
    }
    if (s < 9) scr[s] = mk(ar, ai);
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
  int st = (states >> (2 * j)) & 3;
  if (st == 0 && E == 0.0f) st = 1;

  if (b < B) {
    if (win && s == 0) win[b] = st == 0 ? w : st;
    if (chan && s < 5) {
      cx hv = mk(0, 0);
#pragma unroll
      for (int k = 0; k < 5; k++) if (st == 0 && s == k) hv = h[k];
      chan[(size_t)b * 5 + s] = hv;
    }
  }

  // ---- 3. this row's trellis: step i = 0..38 is symbol m = 49 + i with sample y[m + w] ----
  const cx zf0 = mlse_expected(h, s), zf1 = mlse_expected(h, s | 16);              // into state s from s >> 1, (s >> 1) | 8
  // (the way back needs Z[2 s], Z[2 s + 1] -- out of state s with b = 0, 1 -- and E and the burst's state are wanted after it: parked in LDS)
  scr[12 + s] = zf0; scr[28 + s] = zf1;
  if (s == 0) { scr[9] = mk(E, __int_as_float(w)); scr[10] = mk(__int_as_float(st), 0.0f); }
  const int rowbase = lane & 48;
  const int pf0 = 4 * (rowbase | (s >> 1)), pf1 = pf0 + 32;
  const int pb0 = 4 * (rowbase | ((2 * s) & 15)), pb1 = pb0 + 4;
  int yi = TRX_MLSE_ACC_FIRST + w;
  // (a scheduling fence per step, the next step's symbol fetched ahead of it: see k_mlse)
  float A[TRX_MLSE_ACC_STEPS];
  float al = (s == TRX_MLSE_ACC_START) ? 0.0f : TRX_MLSE_INF;
  cx y = Y[yi];
#pragma unroll
  for (int i = 0; i < TRX_MLSE_ACC_STEPS; i++) {
    if (i < TRX_MLSE_ACC_STEPS - 1) yi += 1;
    const cx yn = Y[yi];
    float g0 = mlse_gamma(y, zf0), g1 = mlse_gamma(y, zf1);
    if (i >= 36 && (s & 1)) { g0 = TRX_MLSE_INF; g1 = TRX_MLSE_INF; }            // the tail symbols are -1
    const float a0 = bperm(pf0, al) + g0, a1 = bperm(pf1, al) + g1;
    al = fminf(a0, a1);
    A[i] = al;
    y = yn;                                                 // (after the last step the symbol is that step's again: the backward pass starts there)
    __builtin_amdgcn_sched_barrier(0);
  }
  wave_lds_fence();
  const cx zb0 = scr[12 + 2 * s], zb1 = scr[13 + 2 * s];
  asm volatile("" : "+v"(yi));                              // (or the addresses of the way up are kept in registers for the way back)
  float be = 0.0f;
  float D[3] = {0.0f, 0.0f, 0.0f};
#pragma unroll
  for (int i = TRX_MLSE_ACC_STEPS - 1; i >= 0; i--) {
    if (i > 0) yi -= 1;
    const cx yn = Y[yi];
    float t = A[i] + be;                                    // alpha and beta, both after step i
    t = fminf(t, dpp_f<0x4E>(t));                           // lane ^ 2
    t = fminf(t, dpp_f<0x124>(t));                          // the row rotated by 4
    t = fminf(t, dpp_f<0x128>(t));                          // ... by 8: the minimum over the eight states of this lane's parity
    const float o = dpp_f<0xB1>(t);                         // lane ^ 1: the other parity's
    const float diff = (s & 1) ? o - t : t - o;             // M_0 - M_1
    if ((i & 15) == s) D[i >> 4] = diff;
    asm volatile("" : "+v"(D[i >> 4]));                     // (the select happens here: not 39 differences kept for a chain of selects after the loop)
    if (i > 0) {
      const float g0 = mlse_gamma(y, zb0);
      const float g1 = (i >= 36) ? TRX_MLSE_INF : mlse_gamma(y, zb1);
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
    for (int q = 0; q < 3; q++) {
      const int i = 16 * q + s;
      const int m = TRX_MLSE_ACC_FIRST + i;
      if (i < TRX_MLSE_ACC_STEPS && m < nsoft) {
        float sv = 0.5f + D[q] / den;
        if (sv > 1.0f) sv = 1.0f;
        if (sv < 0.0f) sv = 0.0f;
        sb[m] = sv;
        if (hb) hb[m] = sv > 0.5F;
      }
    }
    for (int m = s; m < nsoft; m += 16) {                  // the known head and the guard-side rest: the demodulator's formula
      if (m >= TRX_MLSE_ACC_FIRST && m < TRX_MLSE_ACC_FIRST + TRX_MLSE_ACC_STEPS) continue;
      const float sv = mlse_slice(Y[m].r);
      sb[m] = sv;
      if (hb) hb[m] = sv > 0.5F;
    }
  } else {
    for (int m = s; m < nsoft; m += 16) {
      const float sv = st_ == 1 ? mlse_slice(Y[m].r) : 0.0f;
      sb[m] = sv;
      if (hb) hb[m] = sv > 0.5F;
    }
  }
}

}  // namespace

hipError_t trx_launch_mlse_access(hipStream_t st, int sps, const TrxTables *dT, const trx_c32 *samples, const int32_t *off, const int32_t *len,
                                  int B, const trx_c32 *amp, const float *toa, const uint8_t *flags, int need_mask, trx_c32 *chan, int32_t *win,
                                  float *soft, uint8_t *hard, int nsoft, int stride) {
  if (B <= 0) return hipSuccess;
  if (nsoft < 0 || nsoft > 148) return hipErrorInvalidValue;
  const int per = 4 * TRX_MLSE_WAVES;
  const dim3 grid((B + per - 1) / per), block(64 * TRX_MLSE_WAVES);
  switch (sps) {
    case 1: k_mlse_access<1><<<grid, block, 0, st>>>(dT, samples, off, len, B, amp, toa, flags, need_mask, chan, win, soft, hard, nsoft, stride); break;
    case 2: k_mlse_access<2><<<grid, block, 0, st>>>(dT, samples, off, len, B, amp, toa, flags, need_mask, chan, win, soft, hard, nsoft, stride); break;
    case 4: k_mlse_access<4><<<grid, block, 0, st>>>(dT, samples, off, len, B, amp, toa, flags, need_mask, chan, win, soft, hard, nsoft, stride); break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}
