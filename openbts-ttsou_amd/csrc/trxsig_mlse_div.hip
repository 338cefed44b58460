// trxsig_mlse_div.hip -- two-antenna receive diversity for the sequence equaliser (trxsig_mlse_div_batch,
// trxsig_mlse_div_normal_batch; the Transceiver groups' trxsig_trxgroup_combine_div): k_mlse's algorithm with the channel
// window chosen on the summed tap powers of both antennas and the branch metric summed over both (maximal-ratio combining inside
// the trellis: both branches are assumed to have the same noise power).  Pinned by the float32 model tests/mlse_div_model.py, which
// this kernel equals word for word, and graded against the float64 statement tests/mlse_div_ref.py.  The algorithm is stated in
// include/trxsig.h (trxsig_mlse_div_batch).  Nothing is fused, nothing is transcendental, one division per soft bit.
//
// Layout: k_mlse's (trxsig_mlse.hip), every shared step from trxsig_mlse_dev.h (mlse_symbols, mlse_corr_tap, mlse_window2,
// mlse_trellis2, mlse_soft_out) -- a wave takes two bursts, each of its four 16-lane rows is one half-burst trellis, the 61
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
    const cx cd0 = mlse_corr_tap(tsc_bits, d, Y0), cd1 = mlse_corr_tap(tsc_bits, d, Y1);
    if (s < 9) { scr[s] = cd0; scr[9 + s] = cd1; }
  }
  wave_lds_fence();
  cx h0[5], h1[5];                                          // one window for both antennas
  int w;
  const float E = mlse_window2(scr, h0, h1, w);
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
  cx g0[5], g1[5];
#pragma unroll
  for (int k = 0; k < 5; k++) { g0[k] = left ? h0[4 - k] : h0[k]; g1[k] = left ? h1[4 - k] : h1[k]; }
  // (E, w, the burst's state and the row's taps are wanted after the way up: parked in LDS meanwhile, the 61 forward metrics want
  //  the registers)
  if (s == 0) {
    scr[18] = mk(E, __int_as_float(w)); scr[19] = mk(__int_as_float(st), 0.0f);
#pragma unroll
    for (int k = 0; k < 5; k++) { scr[20 + k] = g0[k]; scr[25 + k] = g1[k]; }
  }
  // start state: bit 0 first a[86], a[85], a[84], a[83] (right) or a[61], a[62], a[63], a[64] (left); a[61 + t] = training bit t
  const int start = left ? (int)(tsc_bits & 15u)
                         : (int)(((tsc_bits >> 25) & 1u) | (((tsc_bits >> 24) & 1u) << 1) | (((tsc_bits >> 23) & 1u) << 2) | (((tsc_bits >> 22) & 1u) << 3));
  // step i = 0..60 is symbol m = 87 + i with sample y[m + w] (right), m = 60 - i with y[m + 4 + w] (left)
  float D[4] = {0.0f, 0.0f, 0.0f, 0.0f};
  mlse_trellis2<61, false>(Y0, Y1, left ? 64 + w : 87 + w, left ? -1 : 1, g0, g1, 1.0f, scr, lane, start, D);

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
      if (i < 61 && m < nsoft) mlse_soft_out(sb, hb, m, D[q], den);
    }
    const int m = 61 + hl;                                  // the midamble: the demodulator's formula on the primary antenna
    if (hl < 26 && m < nsoft) mlse_put(sb, hb, m, mlse_slice(Yp[m].r));
  } else {
    mlse_fall_back(sb, hb, Yp, st_, hl, 32, nsoft);
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

hipError_t trx_launch_mlse_div(hipStream_t st, int sps, const TrxTables *dT, const TrxMlseArgs &a) {
  return mlse_launch<2 * TRX_MLSE_WAVES, true>(sps, a, [&](auto S, dim3 grid, dim3 block) {
    k_mlse_div<decltype(S)::value><<<grid, block, 0, st>>>(dT, a.samples0, a.off0, a.samples1, a.off1, a.len, a.B, a.tsc_bits, a.amp, a.toa, a.primary,
                                                           a.flags, a.need_mask, a.chan, a.win, a.soft, a.hard, a.nsoft, a.stride);
  });
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
