// trxsig_mlse_irc.hip -- interference-rejection combining for the two-antenna sequence equaliser (trxsig_mlse_irc_batch,
// trxsig_mlse_irc_normal_batch; the Transceiver groups' trxsig_trxgroup_combine_irc): k_mlse_div's algorithm with the 2 x 2
// covariance of the disturbance estimated from the midamble residuals (or given by the caller) and the whitened metric
// e^H R^-1 e in the trellis.  The whitening is the square-root-free LDL form: antenna 1's symbols and taps become
// A y_1 - conj(x) y_0 once per burst, antenna 0's metric is scaled by det = A Bv - |x|^2; after that the trellis is k_mlse_div's with
// one more multiply per branch metric.  Pinned by the float32 model tests/mlse_irc_model.py, which this kernel equals word for word,
// and graded against the float64 statement tests/mlse_irc_ref.py.  The algorithm is stated in include/trxsig.h
// (trxsig_mlse_irc_batch).  Nothing is fused, nothing is transcendental; four more divisions per burst than k_mlse_div.
//
// Layout: k_mlse_div's (trxsig_mlse_div.hip); steps 1, 2 and the trellis are the shared code of trxsig_mlse_dev.h.  What is added:
//   * the residual sums: lane s of a row forms the terms of midamble positions 65 + s and (s < 6) 81 + s, and the row adds them up in
//     the stated order through 22 x 4 ds_bpermute -- no LDS words, no fence;
//   * the set (A, Bv, xr, xi), det, the whitened taps and E_w: every lane of a row, redundantly, as the estimate is;
//   * the whitening of y_1 in place in ysh by the 32 lanes of a burst, once; the midamble's soft bits (the demodulator's formula on
//     the unwhitened primary antenna) are written before it, and a burst that falls back is not whitened at all;
//   * det in one more VGPR through the trellis.
// LDS is k_mlse_div's to the byte.  Listing (gfx950): DESIGN.md 5.4.z.
#include "trxsig_mlse_dev.h"

namespace {

#define TRX_MLSE_IRC_SCR 32                                 /* words of the staging area a row uses */

template <int SPS>
__global__ __launch_bounds__(64 * TRX_MLSE_WAVES) __attribute__((amdgpu_waves_per_eu(4)))
void k_mlse_irc(const TrxTables *__restrict__ T, const void *__restrict__ samples0, const int32_t *__restrict__ offset0,
                const void *__restrict__ samples1, const int32_t *__restrict__ offset1, const int32_t *__restrict__ length, int B,
                unsigned tsc_bits /* bit j = training-sequence bit j */, const cx *__restrict__ amp_in, const float *__restrict__ toa_in,
                const uint8_t *__restrict__ primary, const uint8_t *__restrict__ flags, int need_mask, float loading,
                const float *__restrict__ cov_in, float *__restrict__ cov, cx *__restrict__ chan, int32_t *__restrict__ win,
                float *__restrict__ soft, uint8_t *__restrict__ hard, int nsoft, int stride) {
  typedef DemodGeom<SPS, 148> G;
  static_assert(4 * TRX_MLSE_IRC_SCR <= G::U, "the rows' scratch lies in the staging area");
  __shared__ cx ph[TRX_MLSE_WAVES][G::U];
  __shared__ cx ysh[TRX_MLSE_WAVES][2][2][TRX_MLSE_NY];

  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int bw = 2 * (blockIdx.x * TRX_MLSE_WAVES + wave);   // the wave's first burst (wave-uniform)
  if (bw >= B) return;

  // ---- 1. symbols, as in k_mlse_div.  States, four bits per burst: 0 = equalise, 1 = fall back, 2 = not enabled ----
  int states = 0;
#pragma unroll 1
  for (int q = 0; q < 4; q++) {
    const int j = q >> 1, a = q & 1;                        // wave-uniform
    const int b = bw + j;
    cx *Y = ysh[wave][j][a];
    bool enabled = false;
    int off = 0, N = 0;
    cx amp = mk(1.0f, 0.0f);
    float toa = 0.0f;
    const void *samples = a ? samples1 : samples0;
    if (b < B) {
      const int o0 = offset0[b], o1 = offset1[b];
      off = a ? o1 : o0; N = length[b]; amp = amp_in[b]; toa = toa_in[b];
      // k_demod's test, once for the burst: the antennas share the length, and both offsets have to pass
      enabled = (o1 >= 0) && mlse_enabled<SPS>(o0, N, toa, flags, need_mask, b);
    }
    if (!__builtin_amdgcn_readfirstlane(enabled)) {
      mlse_zero(Y, lane);
      states |= 2 << (4 * j);
      continue;
    }
    if (mlse_symbols<SPS>(T, ph[wave], samples, off, N, amp, toa, lane, Y)) states |= 1 << (4 * j);     // (either antenna's)
  }
  wave_lds_fence();

  // ---- 2. channel estimate, as in k_mlse_div: one window for both antennas ----
  const int s = lane & 15;                                  // the state this lane carries
  const int j = lane >> 5;                                  // which of the wave's two bursts
  const bool left = (lane >> 4) & 1;                        // which half of it
  const int b = bw + j;
  const cx *Y0 = ysh[wave][j][0];
  cx *Y1 = ysh[wave][j][1];
  // this row's words of the (dead) staging area: c_0[9], c_1[9], (E_w, w), (state, det), g_0[5] from word 20, g_1'[5] from word 25
  cx *scr = ph[wave] + TRX_MLSE_IRC_SCR * (lane >> 4);
  {
    const int d = (s < 9 ? s : 8) - 4;
    const cx cd0 = mlse_corr_tap(tsc_bits, d, Y0), cd1 = mlse_corr_tap(tsc_bits, d, Y1);
    if (s < 9) { scr[s] = cd0; scr[9 + s] = cd1; }
  }
  wave_lds_fence();
  cx h0[5], h1[5];                                          // one window for both antennas
  int w;
  const float E = mlse_window2(scr, h0, h1, w);
  int st = (states >> (4 * j)) & 15;
  if (st == 0 && E == 0.0f) st = 1;
  const int rowbase = lane & 48;
  const int hl = lane & 31;                                 // lane within the burst's two rows

  // ---- 2b. residuals on the 22 midamble positions whose five symbols are all training symbols: this lane's terms (m = 65 + s and,
  //          for s < 6, 81 + s), then the row's sums from 0 with m ascending ----
  float S00 = 0.0f, S11 = 0.0f, Xr = 0.0f, Xi = 0.0f;
  {
    float t00[2], t11[2], txr[2], txi[2];
#pragma unroll
    for (int u = 0; u < 2; u++) {
      int m = 65 + 16 * u + s;
      if (m > 86) m = 86;                                   // (lanes 6..15 of the second round: a copy of position 86, not summed)
      int x = 0;                                            // bit k of x_m = training bit m - 61 - k
#pragma unroll
      for (int k = 0; k < 5; k++) x |= (int)((tsc_bits >> (m - 61 - k)) & 1u) << k;
      const cx z0 = mlse_expected(h0, x), z1 = mlse_expected(h1, x);
      const cx y0 = Y0[m + w], y1 = Y1[m + w];
      const float r0r = y0.r - z0.r, r0i = y0.i - z0.i, r1r = y1.r - z1.r, r1i = y1.i - z1.i;
      t00[u] = r0r * r0r + r0i * r0i;
      t11[u] = r1r * r1r + r1i * r1i;
      txr[u] = r0r * r1r + r0i * r1i;                       // X = sum r_0 conj(r_1)
      txi[u] = r0i * r1r - r0r * r1i;
    }
#pragma unroll
    for (int q = 0; q < 22; q++) {
      const int from = 4 * (rowbase | (q & 15));
      S00 = S00 + bperm(from, t00[q >> 4]);
      S11 = S11 + bperm(from, t11[q >> 4]);
      Xr = Xr + bperm(from, txr[q >> 4]);
      Xi = Xi + bperm(from, txi[q >> 4]);
    }
  }

  // ---- 2c. the set (A, Bv, xr, xi) and det; the identity set where it cannot be used ----
  float cA, cB, cxr, cxi;
  bool ident = false;
  if (cov_in) {
    cA = 1.0f; cB = 1.0f; cxr = 0.0f; cxi = 0.0f;
    if (b < B) { const float *ci = cov_in + (size_t)b * 4; cA = ci[0]; cB = ci[1]; cxr = ci[2]; cxi = ci[3]; }
  } else {
    const float tt = S00 + S11;
    ident = !(tt > 0.0f);
    cA = S00 / tt + loading; cB = S11 / tt + loading; cxr = Xr / tt; cxi = Xi / tt;
  }
  float det = cA * cB - (cxr * cxr + cxi * cxi);
  ident = ident || !(cA < 0x1p10f) || !(cB < 0x1p10f) || !(fabsf(cxr) < 0x1p10f) || !(fabsf(cxi) < 0x1p10f) || !(cA >= 0.0f) ||
          !(cB >= 0.0f) || !(det > 0.0f);
  if (ident) { cA = 1.0f; cB = 1.0f; cxr = 0.0f; cxi = 0.0f; det = 1.0f; }

  // ---- 2d. the whitened taps of antenna 1 and E_w ----
  cx h1w[5];
  float Ew_;
  {
    float pw[5];
#pragma unroll
    for (int k = 0; k < 5; k++) {
      h1w[k] = mlse_whiten(cA, cxr, cxi, h0[k], h1[k]);
      pw[k] = det * (h0[k].r * h0[k].r + h0[k].i * h0[k].i) + (h1w[k].r * h1w[k].r + h1w[k].i * h1w[k].i);
    }
    Ew_ = (((pw[0] + pw[1]) + pw[2]) + pw[3]) + pw[4];
    if (!(Ew_ > 0.0f) || !(Ew_ < TRX_MLSE_INF)) {           // the identity set after all, and then E_w is E
      cA = 1.0f; cB = 1.0f; cxr = 0.0f; cxi = 0.0f; det = 1.0f; Ew_ = E;
#pragma unroll
      for (int k = 0; k < 5; k++) h1w[k] = mlse_whiten(cA, cxr, cxi, h0[k], h1[k]);
    }
  }

  const cx *Yp = (primary && b < B && primary[b]) ? Y1 : Y0;   // the antenna amp and TOA came from
  float *sb = soft + (size_t)(b < B ? b : 0) * stride;
  uint8_t *hb = hard ? hard + (size_t)(b < B ? b : 0) * stride : nullptr;
  if (b < B) {
    if (win && hl == 0) win[b] = st == 0 ? w : st;
    if (chan && hl < 10) {                                  // chan[b][antenna][k]: the unwhitened taps
      cx hv = mk(0, 0);
#pragma unroll
      for (int k = 0; k < 5; k++) {
        if (st == 0 && hl == k) hv = h0[k];
        if (st == 0 && hl == 5 + k) hv = h1[k];
      }
      chan[(size_t)b * 10 + hl] = hv;
    }
    if (cov && hl < 4) {
      const float cv = hl == 0 ? cA : (hl == 1 ? cB : (hl == 2 ? cxr : cxi));
      cov[(size_t)b * 4 + hl] = st == 0 ? cv : 0.0f;
    }
    // the midamble's soft bits: the demodulator's formula on the primary antenna as it is now, before y_1 is whitened
    const int m = 61 + hl;
    if (st == 0 && hl < 26 && m < nsoft) mlse_put(sb, hb, m, mlse_slice(Yp[m].r));
  }
  wave_lds_fence();                                         // (c_0, c_1, the residuals' and the midamble's symbols have been read)
  if (st == 0) {                                            // y_1 in place; a burst that falls back keeps its symbols for step 5
    for (int m = hl; m < TRX_MLSE_NY; m += 32) Y1[m] = mlse_whiten(cA, cxr, cxi, Y0[m], Y1[m]);
  }
  wave_lds_fence();

  // ---- 3. the half-burst trellis of this row: mlse_trellis2 on (y_0, y_1') with (h_0, h_1') and det on antenna 0's metric ----
  cx g0[5], g1[5];
#pragma unroll
  for (int k = 0; k < 5; k++) { g0[k] = left ? h0[4 - k] : h0[k]; g1[k] = left ? h1w[4 - k] : h1w[k]; }
  if (s == 0) {
    scr[18] = mk(Ew_, __int_as_float(w)); scr[19] = mk(__int_as_float(st), det);
#pragma unroll
    for (int k = 0; k < 5; k++) { scr[20 + k] = g0[k]; scr[25 + k] = g1[k]; }
  }
  // start state and steps: k_mlse_div's
  const int start = left ? (int)(tsc_bits & 15u)
                         : (int)(((tsc_bits >> 25) & 1u) | (((tsc_bits >> 24) & 1u) << 1) | (((tsc_bits >> 23) & 1u) << 2) | (((tsc_bits >> 22) & 1u) << 3));
  float D[4] = {0.0f, 0.0f, 0.0f, 0.0f};
  mlse_trellis2<61, true>(Y0, Y1, left ? 64 + w : 87 + w, left ? -1 : 1, g0, g1, det, scr, lane, start, D);

  // ---- 4 / 5. soft bits out (the midamble of an equalised burst is out already) ----
  if (b >= B) return;
  const float E_ = scr[18].r;
  const int st_ = __float_as_int(scr[19].r);
  if (st_ == 0) {
    const float den = 8.0f * E_;
#pragma unroll
    for (int q = 0; q < 4; q++) {
      const int i = 16 * q + s;
      const int m = left ? 60 - i : 87 + i;
      if (i < 61 && m < nsoft) mlse_soft_out(sb, hb, m, D[q], den);
    }
  } else {
    mlse_fall_back(sb, hb, Yp, st_, hl, 32, nsoft);
  }
}

}  // namespace

hipError_t trx_launch_mlse_irc(hipStream_t st, int sps, const TrxTables *dT, const TrxMlseArgs &a) {
  return mlse_launch<2 * TRX_MLSE_WAVES, true>(sps, a, [&](auto S, dim3 grid, dim3 block) {
    k_mlse_irc<decltype(S)::value><<<grid, block, 0, st>>>(dT, a.samples0, a.off0, a.samples1, a.off1, a.len, a.B, a.tsc_bits, a.amp, a.toa, a.primary,
                                                           a.flags, a.need_mask, a.loading, a.cov_in, a.cov, a.chan, a.win, a.soft, a.hard, a.nsoft,
                                                           a.stride);
  });
}
