// trxsig_mlse_div.hip -- two-antenna receive diversity for the sequence equaliser (trxsig_mlse_div_batch,
// trxsig_mlse_div_normal_batch; the Transceiver groups' trxsig_trxgroup_combine_div): k_mlse's algorithm with the channel
// window chosen on the summed tap powers of both antennas and the branch metric summed over both (maximal-ratio combining inside
// the trellis: both branches are assumed to have the same noise power).  Pinned by the float32 model tests/mlse_div_model.py, which
// this kernel equals word for word, and graded against the float64 statement tests/mlse_div_ref.py.  The algorithm is stated in
// include/trxsig.h (trxsig_mlse_div_batch).  Nothing is fused, nothing is transcendental, one division per soft bit.
//
// Layout: k_mlse's (trxsig_mlse.hip) -- a wave takes two bursts, each of its four 16-lane rows is one half-burst trellis, the 61
// forward metrics of a lane stay in VGPRs, predecessors and successors come by ds_bpermute, the minimum by DPP.  What doubles:
//   * the symbol vectors in LDS, ysh[wave][burst][antenna][152]; demod_core runs four times per wave through the one staging area
//     (a rolled loop: one copy of its code), each antenna with its own sample pointer, offset and 16-byte load decision;
//   * a lane's expected values (zf0, zf1 per antenna) and the LDS symbol reads per step (two);
//   * the per-row scratch in the dead staging area: c[9] per antenna, (E, w), the state, and the row's taps g[5] per antenna, from
//     which the way back forms its own expected values again (k_mlse parks Z[32]; two of those per row would not fit at sps 1).
// Listing (gfx950): DESIGN.md 5.4.y.
#include "trxsig_mlse_dev.h"

namespace {

#define TRX_MLSE_DIV_SCR 32                                 /* words of the staging area a row uses */

template <int SPS>
__global__ __launch_bounds__(64 * TRX_MLSE_WAVES) __attribute__((amdgpu_waves_per_eu(4)))
void k_mlse_div(const TrxTables *__restrict__ T, const void *__restrict__ samples0, const int32_t *__restrict__ offset0,
                const void *__restrict__ samples1, const int32_t *__restrict__ offset1, const int32_t *__restrict__ length, int B,
                unsigned tsc_bits /* bit j = training-sequence bit j */, const cx *__restrict__ amp_in, const float *__restrict__ toa_in,
                const uint8_t *__restrict__ primary, const uint8_t *__restrict__ flags, int need_mask, cx *__restrict__ chan,
                int32_t *__restrict__ win, float *__restrict__ soft, uint8_t *__restrict__ hard, int nsoft, int stride) {
  typedef DemodGeom<SPS, 148> G;
  static_assert(4 * TRX_MLSE_DIV_SCR <= G::U, "the rows' scratch lies in the staging area");
  __shared__ cx ph[TRX_MLSE_WAVES][G::U];
  __shared__ cx ysh[TRX_MLSE_WAVES][2][2][TRX_MLSE_NY];

  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int bw = 2 * (blockIdx.x * TRX_MLSE_WAVES + wave);   // the wave's first burst (wave-uniform)
  if (bw >= B) return;

  // ---- 1. symbols, an antenna of a burst at a time on the whole wave.  States, four bits per burst: 0 = equalise, 1 = fall back,
  //         2 = not enabled ----
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
      enabled = (o0 >= 0) && (o1 >= 0) && (N >= 92 * SPS) && (N <= 157 * SPS) && (N % SPS == 0) && (fabsf(toa) <= 4096.0f);
      if (flags) enabled = enabled && (need_mask ? ((flags[b] & need_mask) == need_mask) : (flags[b] != 0));
    }
    if (!__builtin_amdgcn_readfirstlane(enabled)) {
      for (int m = lane; m < TRX_MLSE_NY; m += 64) Y[m] = mk(0, 0);      // (the trellis rows of this burst run on zeros; nothing of theirs is stored)
      states |= 2 << (4 * j);
      continue;
    }
    constexpr int NLD = (157 * SPS / 2 + 63) / 64;
    const bool wide = (off & 1) == 0;                       // per antenna: the two offsets of a burst may differ in parity
    float4 v[NLD];
#pragma unroll
    for (int i = 0; i < NLD; i++) v[i] = make_float4(0, 0, 0, 0);
    if (wide) {
#pragma unroll
      for (int i = 0; i < NLD; i++) {
        const int p = lane + 64 * i;
        if (p < N / 2) v[i] = SmpC32::ld2(samples, off, p);
      }
    }
    wave_lds_fence();                                       // the staging area's readers of the run before are done
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
    if (__builtin_amdgcn_ballot_w64(bad) != 0 || N / SPS < 148) states |= 1 << (4 * j);     // (either antenna's)
  }
  wave_lds_fence();

  // ---- 2. channel estimate; every row works its burst's out for itself (lanes 0..8: c[-4..4], an antenna after the other) ----
  const int s = lane & 15;                                  // the state this lane carries
  const int j = lane >> 5;                                  // which of the wave's two bursts
  const bool left = (lane >> 4) & 1;                        // which half of it
  const int b = bw + j;
  const cx *Y0 = ysh[wave][j][0], *Y1 = ysh[wave][j][1];
  // this row's words of the (dead) staging area: c_0[9], c_1[9], (E, w), state, g_0[5] from word 20, g_1[5] from word 25
  cx *scr = ph[wave] + TRX_MLSE_DIV_SCR * (lane >> 4);
  {
    const int d = (s < 9 ? s : 8) - 4;
    cx acc0 = mk(0, 0), acc1 = mk(0, 0);
#pragma unroll
    for (int i = 0; i < 16; i++) {
      const cx y0 = Y0[66 + i + d], y1 = Y1[66 + i + d];
      const int plus = (tsc_bits >> (5 + i)) & 1;
      acc0 = cadd(acc0, mk(sgn(y0.r, plus), sgn(y0.i, plus)));
      acc1 = cadd(acc1, mk(sgn(y1.r, plus), sgn(y1.i, plus)));
    }
    if (s < 9) { scr[s] = cmulr(acc0, 0.0625f); scr[9 + s] = cmulr(acc1, 0.0625f); }
  }
  wave_lds_fence();
  cx c0[9], c1[9];
  float p[9];
#pragma unroll
  for (int i = 0; i < 9; i++) {
    c0[i] = scr[i]; c1[i] = scr[9 + i];
    p[i] = (c0[i].r * c0[i].r + c0[i].i * c0[i].i) + (c1[i].r * c1[i].r + c1[i].i * c1[i].i);      // antenna 0's power first
  }
  int w = 0;
  float E = (((p[4] + p[5]) + p[6]) + p[7]) + p[8];
#pragma unroll
  for (int q = 1; q <= 4; q++) {                            // w = -q; a later window only on a strict >
    const float Ew = (((p[4 - q] + p[5 - q]) + p[6 - q]) + p[7 - q]) + p[8 - q];
    if (Ew > E) { E = Ew; w = -q; }
  }
  cx h0[5], h1[5];                                          // one window for both antennas
#pragma unroll
  for (int k = 0; k < 5; k++) {
    h0[k] = c0[4 + k]; h1[k] = c1[4 + k];
#pragma unroll
    for (int q = 1; q <= 4; q++) if (w == -q) { h0[k] = c0[4 - q + k]; h1[k] = c1[4 - q + k]; }
  }
  int st = (states >> (4 * j)) & 15;
  if (st == 0 && E == 0.0f) st = 1;

  const int hl = lane & 31;                                 // lane within the burst's two rows
  if (b < B) {
    if (win && hl == 0) win[b] = st == 0 ? w : st;
    if (chan && hl < 10) {                                  // chan[b][antenna][k]
      cx hv = mk(0, 0);
#pragma unroll
      for (int k = 0; k < 5; k++) {
        if (st == 0 && hl == k) hv = h0[k];
        if (st == 0 && hl == 5 + k) hv = h1[k];
      }
      chan[(size_t)b * 10 + hl] = hv;
    }
  }

  // ---- 3. the half-burst trellis of this row ----
  wave_lds_fence();                                         // (c_0, c_1 have been read by the whole row)
  cx zf00, zf10, zf01, zf11;                                // zf<b><antenna>: into state s from s >> 1 (b = 0), (s >> 1) | 8 (b = 1)
  {
    cx g0[5], g1[5];
#pragma unroll
    for (int k = 0; k < 5; k++) { g0[k] = left ? h0[4 - k] : h0[k]; g1[k] = left ? h1[4 - k] : h1[k]; }
    zf00 = mlse_expected(g0, s); zf10 = mlse_expected(g0, s | 16);
    zf01 = mlse_expected(g1, s); zf11 = mlse_expected(g1, s | 16);
    // (E, w, the burst's state and the row's taps are wanted after the way up: parked in LDS meanwhile, the 61 forward metrics want
    //  the registers)
    if (s == 0) {
      scr[18] = mk(E, __int_as_float(w)); scr[19] = mk(__int_as_float(st), 0.0f);
#pragma unroll
      for (int k = 0; k < 5; k++) { scr[20 + k] = g0[k]; scr[25 + k] = g1[k]; }
    }
  }
  const int rowbase = lane & 48;
  const int pf0 = 4 * (rowbase | (s >> 1)), pf1 = pf0 + 32;
  const int pb0 = 4 * (rowbase | ((2 * s) & 15)), pb1 = pb0 + 4;
  // start state: bit 0 first a[86], a[85], a[84], a[83] (right) or a[61], a[62], a[63], a[64] (left); a[61 + t] = training bit t
  const int start = left ? (int)(tsc_bits & 15u)
                         : (int)(((tsc_bits >> 25) & 1u) | (((tsc_bits >> 24) & 1u) << 1) | (((tsc_bits >> 23) & 1u) << 2) | (((tsc_bits >> 22) & 1u) << 3));
  // step i = 0..60 is symbol m = 87 + i with sample y[m + w] (right), m = 60 - i with y[m + 4 + w] (left)
  int yi = left ? 64 + w : 87 + w;
  const int dir = left ? -1 : 1;
  // (a scheduling fence per step, the next step's symbols fetched ahead of it: as in k_mlse)
  float A[61];
  float al = (s == start) ? 0.0f : TRX_MLSE_INF;
  cx y0 = Y0[yi], y1 = Y1[yi];
#pragma unroll
  for (int i = 0; i < 61; i++) {
    if (i < 60) yi += dir;
    const cx yn0 = Y0[yi], yn1 = Y1[yi];
    float g0 = mlse_gamma(y0, zf00) + mlse_gamma(y1, zf01);  // antenna 0's metric first
    float g1 = mlse_gamma(y0, zf10) + mlse_gamma(y1, zf11);
    if (i >= 58 && (s & 1)) { g0 = TRX_MLSE_INF; g1 = TRX_MLSE_INF; }            // the tail symbols are -1
    const float a0 = bperm(pf0, al) + g0, a1 = bperm(pf1, al) + g1;
    al = fminf(a0, a1);
    A[i] = al;
    y0 = yn0; y1 = yn1;                                     // (after step 60 the symbols are that step's again: the backward pass starts there)
    __builtin_amdgcn_sched_barrier(0);
  }
  wave_lds_fence();
  cx zb00, zb10, zb01, zb11;                                // zb<b><antenna>: out of state s with b = 0, 1 -- Z[2 s], Z[2 s + 1]
  {
    cx g0[5], g1[5];
#pragma unroll
    for (int k = 0; k < 5; k++) { g0[k] = scr[20 + k]; g1[k] = scr[25 + k]; }
    zb00 = mlse_expected(g0, 2 * s); zb10 = mlse_expected(g0, 2 * s + 1);
    zb01 = mlse_expected(g1, 2 * s); zb11 = mlse_expected(g1, 2 * s + 1);
  }
  asm volatile("" : "+v"(yi));                              // (or the 61 addresses of the way up are kept in registers for the way back)
  float be = 0.0f;
  float D[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
  for (int i = 60; i >= 0; i--) {
    if (i > 0) yi -= dir;
    const cx yn0 = Y0[yi], yn1 = Y1[yi];
    float t = A[i] + be;                                    // alpha and beta, both after step i
    t = fminf(t, dpp_f<0x4E>(t));                           // lane ^ 2
    t = fminf(t, dpp_f<0x124>(t));                          // the row rotated by 4
    t = fminf(t, dpp_f<0x128>(t));                          // ... by 8: the minimum over the eight states of this lane's parity
    const float o = dpp_f<0xB1>(t);                         // lane ^ 1: the other parity's
    const float diff = (s & 1) ? o - t : t - o;             // M_0 - M_1
    if ((i & 15) == s) D[i >> 4] = diff;
    asm volatile("" : "+v"(D[i >> 4]));                     // (the select happens here: not 61 differences kept for a chain of selects after the loop)
    if (i > 0) {
      const float g0 = mlse_gamma(y0, zb00) + mlse_gamma(y1, zb01);
      const float g1 = (i >= 58) ? TRX_MLSE_INF : mlse_gamma(y0, zb10) + mlse_gamma(y1, zb11);
      const float b0 = g0 + bperm(pb0, be), b1 = g1 + bperm(pb1, be);
      be = fminf(b0, b1);
    }
    y0 = yn0; y1 = yn1;
    __builtin_amdgcn_sched_barrier(0);
  }

  // ---- 4 / 5. soft bits out ----
  if (b >= B) return;
  const float E_ = scr[18].r;
  const int st_ = __float_as_int(scr[19].r);
  const cx *Yp = (primary && primary[b]) ? Y1 : Y0;         // the antenna amp and TOA came from
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
    const int m = 61 + hl;                                  // the midamble: the demodulator's formula on the primary antenna
    if (hl < 26 && m < nsoft) {
      const float sv = mlse_slice(Yp[m].r);
      sb[m] = sv;
      if (hb) hb[m] = sv > 0.5F;
    }
  } else {
    for (int m = hl; m < nsoft; m += 32) {
      const float sv = st_ == 1 ? mlse_slice(Yp[m].r) : 0.0f;
      sb[m] = sv;
      if (hb) hb[m] = sv > 0.5F;
    }
  }
}

// The selection of a burst's antenna (trxsig.h, trxsig_mlse_div_normal_batch): sel = 1 if v_1 && (!v_0 || n_1 > n_0), else 0 if
// v_0, else 2; n_a = amp_a.re * amp_a.re + amp_a.im * amp_a.im (a NaN compares false).  v_a = (valid_a[b] & need_mask) != 0.
// What is given of the outputs is written: sel; the selected antenna's amp, TOA and -- the Transceiver groups' combine -- its
// flags byte and avgPwr (antenna 0's where sel = 2); valid[b] = need_mask where sel < 2, else 0.
struct DivSelect {
  const uint8_t *valid0, *valid1, *flags0, *flags1;
  const cx *amp0, *amp1;
  const float *toa0, *toa1, *pwr0, *pwr1;
  int B, need_mask;
  uint8_t *sel, *valid, *flags;
  cx *amp;
  float *toa, *pwr;
};
__global__ __launch_bounds__(256) void k_div_select(const DivSelect a) {
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b >= a.B) return;
  const bool v0 = (a.valid0[b] & a.need_mask) != 0, v1 = (a.valid1[b] & a.need_mask) != 0;
  const cx a0 = a.amp0[b], a1 = a.amp1[b];
  const float n0 = a0.r * a0.r + a0.i * a0.i, n1 = a1.r * a1.r + a1.i * a1.i;
  const int sel = (v1 && (!v0 || n1 > n0)) ? 1 : (v0 ? 0 : 2);
  if (a.sel) a.sel[b] = (uint8_t)sel;
  if (a.amp) a.amp[b] = sel == 1 ? a1 : a0;
  if (a.toa) a.toa[b] = sel == 1 ? a.toa1[b] : a.toa0[b];
  if (a.valid) a.valid[b] = sel < 2 ? (uint8_t)a.need_mask : 0;
  if (a.flags) a.flags[b] = sel == 1 ? a.flags1[b] : a.flags0[b];
  if (a.pwr) a.pwr[b] = sel == 1 ? a.pwr1[b] : a.pwr0[b];
}

// trxsig_trxgroup_combine_div's access-burst rows (a workgroup per row): the selected group's soft row where the combined row is
// valid, zeros elsewhere; no taps, window word 2 (not equalised)
__global__ __launch_bounds__(64) void k_div_copy_rows(const uint8_t *__restrict__ valid, const uint8_t *__restrict__ sel,
                                                      const float *__restrict__ soft0, const float *__restrict__ soft1, int stride_in,
                                                      float *__restrict__ soft, int stride, int nsoft, cx *__restrict__ chan,
                                                      int32_t *__restrict__ win) {
  const int r = blockIdx.x;
  const bool ok = valid[r] != 0;
  const float *src = (sel[r] == 1 ? soft1 : soft0) + (size_t)r * stride_in;
  for (int m = threadIdx.x; m < nsoft; m += 64) soft[(size_t)r * stride + m] = ok ? src[m] : 0.0f;
  if (chan && threadIdx.x < 10) chan[(size_t)r * 10 + threadIdx.x] = mk(0, 0);
  if (win && threadIdx.x == 0) win[r] = 2;
}

}  // namespace

hipError_t trx_launch_mlse_div(hipStream_t st, int sps, const TrxTables *dT, const trx_c32 *samples0, const int32_t *off0,
                               const trx_c32 *samples1, const int32_t *off1, const int32_t *len, int B, unsigned tsc_bits, const trx_c32 *amp,
                               const float *toa, const uint8_t *primary, const uint8_t *flags, int need_mask, trx_c32 *chan, int32_t *win,
                               float *soft, uint8_t *hard, int nsoft, int stride) {
  if (B <= 0) return hipSuccess;
  if (nsoft < 0 || nsoft > 148) return hipErrorInvalidValue;
  const int per = 2 * TRX_MLSE_WAVES;
  const dim3 grid((B + per - 1) / per), block(64 * TRX_MLSE_WAVES);
#define TRX_MLSE_DIV_GO(S) k_mlse_div<S><<<grid, block, 0, st>>>(dT, samples0, off0, samples1, off1, len, B, tsc_bits, amp, toa, primary, flags, \
                                                                 need_mask, chan, win, soft, hard, nsoft, stride)
  switch (sps) {
    case 1: TRX_MLSE_DIV_GO(1); break;
    case 2: TRX_MLSE_DIV_GO(2); break;
    case 4: TRX_MLSE_DIV_GO(4); break;
    default: return hipErrorInvalidValue;
  }
#undef TRX_MLSE_DIV_GO
  return hipGetLastError();
}

hipError_t trx_launch_div_select(hipStream_t st, const TrxDivSelect &p) {
  if (p.B <= 0) return hipSuccess;
  DivSelect a;
  a.valid0 = p.valid0; a.valid1 = p.valid1; a.flags0 = p.flags0; a.flags1 = p.flags1; a.amp0 = p.amp0; a.amp1 = p.amp1;
  a.toa0 = p.toa0; a.toa1 = p.toa1; a.pwr0 = p.pwr0; a.pwr1 = p.pwr1; a.B = p.B; a.need_mask = p.need_mask;
  a.sel = p.sel; a.valid = p.valid; a.flags = p.flags; a.amp = p.amp; a.toa = p.toa; a.pwr = p.pwr;
  k_div_select<<<dim3((p.B + 255) / 256), dim3(256), 0, st>>>(a);
  return hipGetLastError();
}

hipError_t trx_launch_div_copy_rows(hipStream_t st, int rows, const uint8_t *valid, const uint8_t *sel, const float *soft0, const float *soft1,
                                    int stride_in, float *soft, int stride, int nsoft, trx_c32 *chan, int32_t *win) {
  if (rows <= 0) return hipSuccess;
  k_div_copy_rows<<<dim3(rows), dim3(64), 0, st>>>(valid, sel, soft0, soft1, stride_in, soft, stride, nsoft, chan, win);
  return hipGetLastError();
}
