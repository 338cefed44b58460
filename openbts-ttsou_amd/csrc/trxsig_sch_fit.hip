// trxsig_sch_fit.hip -- the fit detector's statistic for synchronisation bursts (trxsig_sch_fit_batch; trxsig_l1acq's
// TRXSIG_SCHDET_FIT): the burst's symbols, the nine-tap least-squares estimate and the best five-tap window by the code
// k_mlse_sch (trxsig_mlse_sch.hip) forms them with (trxsig_mlse_dev.h), then the residual of that fit on the 56 rows whose symbols are all known and
// q = sqrtf(51 E / R): tap energy over residual power, an SNR estimate that does not care where the echoes of the channel lie.
// The reference has no counterpart; the stage is pinned by the float32 model tests/sch_fit_model.py, which this kernel equals
// word for word, and graded against the float64 statement tests/sch_fit_ref.py.  The arithmetic rules are k_mlse's: float add,
// subtract, multiply, one correctly rounded division and one correctly rounded square root per burst; nothing is fused.  The
// algorithm is stated in include/trxsig.h (trxsig_sch_fit_batch) and again, operation by operation, in the model.
//
// Layout.  One wave takes TWO bursts, one after the other; the loop over them is NOT unrolled (one copy of demod_core in the
// listing, as in k_mlse_sch).
//   * Symbols: the whole wave, k_demod's own code (demod_core, RAW form), the 148 rotated outputs, complex, in LDS.
//   * Estimate: lanes 0..8 form c[-4..4], 56 multiply-adds each on LDS reads of y[46..101]; P32 (trxsig_mlse_sch_tab.h) from
//     constant memory by plain global loads, lane d its own row.  The nine taps go through 9 words of the (dead) staging area
//     to every lane, which picks the window as k_mlse_sch does.
//   * Residual: lane j < 56 forms r[46 + j] = y[46 + j] - Z[x], Z[x] k_mlse's expected value of the five known symbols
//     (mlse_expected: the products with +-1 are sign flips, the sum starts from k = 0 and adds k = 1..4 in order) and
//     e[j] = |r|^2 as k_mlse's branch metric (mlse_gamma); lanes 56..63 carry 0.
//   * R: the pairwise tree over the 64 lanes -- lane ^ 1 and lane ^ 2 by DPP quad permutes, the row's half mirror and the row's
//     mirror (after the steps before them the same as lane ^ 4 and lane ^ 8), then (r0 + r1) + (r2 + r3) on the four rows' results.
//   * LDS: the staging area and ONE symbol vector a wave (k_mlse_sch keeps two).  Listing (gfx950): DESIGN.md 5.4.vi.
#define TRX_MLSE_SCH_TAB_QUAL static __device__ __constant__ const
#include "trxsig_mlse_sch_tab.h"
#include "trxsig_mlse_dev.h"                                // mlse_symbols, mlse_ls_tap, mlse_window, mlse_expected, mlse_gamma

namespace {

// bit t = bit t of the extended training sequence (GSM 05.02 5.2.5; trxsig_tablegen.cpp's kXTS): a[42 + t] = 2 bit - 1
constexpr unsigned long long sch_fit_xts() {
  const char *x = "1011100101100010000001000000111100101101010001010111011000011011";
  unsigned long long m = 0;
  for (int t = 0; t < 64; t++) m |= (unsigned long long)(x[t] == '1') << t;
  return m;
}
constexpr unsigned long long kSchFitXts = sch_fit_xts();

template <int SPS>
__global__ __launch_bounds__(64 * TRX_MLSE_WAVES) __attribute__((amdgpu_waves_per_eu(4)))
void k_sch_fit(const TrxTables *__restrict__ T, const void *__restrict__ samples, const int32_t *__restrict__ offset,
               const int32_t *__restrict__ length, int B, const cx *__restrict__ amp_in, const float *__restrict__ toa_in,
               const uint8_t *__restrict__ flags, int need_mask, cx *__restrict__ chan9, int32_t *__restrict__ win,
               float *__restrict__ E_out, float *__restrict__ R_out, float *__restrict__ q_out) {
  typedef DemodGeom<SPS, 148> G;
  static_assert(TRX_MLSE_SCH_NTAP <= G::U, "the taps' scratch lies in the staging area");
  static_assert(TRX_MLSE_SCH_ROW0 + TRX_MLSE_SCH_NROW <= 148 && TRX_MLSE_SCH_NROW <= 64, "the burst map");
  static_assert(TRX_MLSE_SCH_ROW0 - 42 >= 4 && TRX_MLSE_SCH_ROW0 + TRX_MLSE_SCH_NROW - 1 + 4 - 42 <= 63, "every symbol of a row is known");
  __shared__ cx ph[TRX_MLSE_WAVES][G::U];
  __shared__ cx ysh[TRX_MLSE_WAVES][TRX_MLSE_NY];

  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int bw = 2 * (blockIdx.x * TRX_MLSE_WAVES + wave);   // the wave's first burst (wave-uniform)
  cx *Y = ysh[wave];
  cx *scr = ph[wave];                                       // 9 words of the staging area, dead once the symbols are formed

#pragma unroll 1
  for (int jb = 0; jb < 2; jb++) {
    const int b = bw + jb;                                  // wave-uniform
    if (b >= B) break;
    // ---- 1. symbols (mlse_symbols).  st: 0 = fit, 1 = fell back, 2 = not enabled ----
    const int off = offset[b], N = length[b];
    const cx amp = amp_in[b];
    const float toa = toa_in[b];
    const bool enabled = mlse_enabled<SPS>(off, N, toa, flags, need_mask, b);
    int st = 2;
    if (__builtin_amdgcn_readfirstlane(enabled)) st = mlse_symbols<SPS>(T, ph[wave], samples, off, N, amp, toa, lane, Y) ? 1 : 0;

    cx cm = mk(0, 0);                                       // lane d < 9: c[d - 4]
    int w = 0;
    float E = 0.0f, R = 0.0f, q = 0.0f;
    if (st == 0) {                                          // wave-uniform
      wave_lds_fence();
      // ---- 2. channel estimate: lanes 0..8 form c[-4..4] = P32 y[46..101]; every lane then reads all nine ----
      cm = mlse_ls_tap<TRX_MLSE_SCH_NROW>(trx_mlse_sch_p32 + TRX_MLSE_SCH_NROW * (lane < 9 ? lane : 8), Y, TRX_MLSE_SCH_ROW0);
      if (lane < 9) scr[lane] = cm;
      wave_lds_fence();
      cx h[5];
      E = mlse_window(scr, h, w);
      if (E == 0.0f) {
        st = 1;
      } else {
        // ---- 3. the residual: lane j < 56 takes row n = 46 + j; bit k of x is the bit of a[n - w - k] ----
        const int jr = lane < TRX_MLSE_SCH_NROW ? lane : TRX_MLSE_SCH_NROW - 1;
        const int t0 = jr + (TRX_MLSE_SCH_ROW0 - 42) - w;   // a[n - w] is bit t0 of the sequence; 4 <= t0 - k, t0 <= 63
        int x = 0;
#pragma unroll
        for (int k = 0; k < 5; k++) x |= (int)((kSchFitXts >> (t0 - k)) & 1ull) << k;
        const cx z = mlse_expected(h, x);
        float e = mlse_gamma(Y[TRX_MLSE_SCH_ROW0 + jr], z);
        if (lane >= TRX_MLSE_SCH_NROW) e = 0.0f;
        // ---- 4. R: the pairwise tree over the 64 lanes ----
        e = e + dpp_f<0xB1>(e);                             // lane ^ 1
        e = e + dpp_f<0x4E>(e);                             // lane ^ 2
        e = e + dpp_f<0x141>(e);                            // the row's half mirror: the other quad of the eight
        e = e + dpp_f<0x140>(e);                            // the row's mirror: the other eight of the row
        const float r0 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(e), 0));
        const float r1 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(e), 16));
        const float r2 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(e), 32));
        const float r3 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(e), 48));
        R = (r0 + r1) + (r2 + r3);
        q = sqrtf((51.0f * E) / R);                         // R == 0: +inf, kept
        if (!(q == q)) q = 0.0f;
      }
    }
    if (st != 0) { cm = mk(0, 0); E = 0.0f; R = 0.0f; q = 0.0f; }
    if (chan9 && lane < 9) chan9[(size_t)b * 9 + lane] = cm;
    if (lane == 0) {
      if (win) win[b] = st == 0 ? w : st;
      if (E_out) E_out[b] = E;
      if (R_out) R_out[b] = R;
      if (q_out) q_out[b] = q;
    }
  }
}

}  // namespace

hipError_t trx_launch_sch_fit(hipStream_t st, int sps, const TrxTables *dT, const TrxMlseArgs &a) {
  return mlse_launch<2 * TRX_MLSE_WAVES, false>(sps, a, [&](auto S, dim3 grid, dim3 block) {
    k_sch_fit<decltype(S)::value><<<grid, block, 0, st>>>(dT, a.samples0, a.off0, a.len, a.B, a.amp, a.toa, a.flags, a.need_mask, a.chan, a.win, a.E,
                                                          a.R, a.q);
  });
}
