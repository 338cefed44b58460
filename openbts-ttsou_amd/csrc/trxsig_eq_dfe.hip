// trxsig_eq_dfe.hip -- the equaliser path (sps = 1), second half: scaleVector + delayVector + equalizeBurst.
// Numerical contract: see trxsig_dev.h / DESIGN.md (every float32 operation is the reference's, in the
// reference's order; built with -ffp-contract=off).
#include "trxsig_demod.h"
#include "trxsig_eq.h"
#include "trxsig_eq_probe.h"

namespace {

// delayVector's 21 real taps for the fractional delay `frac` (:584-590): the sinc grid's row where the fraction lies on the
// grid (always after peakDetect), else tap j = sinc(pi*((j - 10) - frac)) (:588) from the table sinc, as the reference computes them.
// off_grid() runs once, only where some lane of the wave is off the grid, and returns the function that yields tap j: how a wave's lanes
// share the 21 sinc evaluations is the caller's arrangement.
template <typename F>
__device__ __forceinline__ void eq_delay_taps(const TrxTables *T, float frac, float (&tp)[21], F &&off_grid) {
  const float f512 = frac * 512.0f;
  const int f = (int)f512;
  const bool grid = f < 512 && (float)f == f512;            // (frac can round to exactly 1.0 for a tiny negative delay: off the grid)
  const float4 *row = reinterpret_cast<const float4 *>(T->sinc_grid[f & 511]);
  float g[24];
#pragma unroll
  for (int q = 0; q < 6; q++) { const float4 r4 = row[q]; g[4 * q] = r4.x; g[4 * q + 1] = r4.y; g[4 * q + 2] = r4.z; g[4 * q + 3] = r4.w; }
#pragma unroll
  for (int j = 0; j < 21; j++) tp[j] = g[j];
  if (__any(!grid)) {
    auto tap = off_grid();
#pragma unroll
    for (int j = 0; j < 21; j++) {
      const float tj = tap(j);
      tp[j] = grid ? g[j] : tj;
    }
  }
}

// ---------------------------------------------------------------------------------------------
// k_eq_delay: equalizeBurst's first step (sigProcLib.cpp:1352-1356 after Transceiver.cpp:346): scaleVector(burst, 1/amp)
//   then delayVector(-(TOA - chanOffset)) (:573-616) at one sample per symbol, every sample kept (the equaliser wants the
//   whole burst).  SIXTEEN lanes per burst, four bursts per wave: a wave per burst (k_demod<1,RAW>) spent more
//   instructions on its bookkeeping than on the 157 x 21 products and kept a third of its lanes idle -- 600 instructions
//   per burst, issue-bound at 44 us per 65,536 bursts.  Here a lane owns TEN CONSECUTIVE outputs, whose 21-tap windows
//   overlap: 30 LDS reads feed 210 multiply-adds (the burst sits in LDS, scaled, between zero pads that stand for
//   "taps outside the vector are skipped", :584-590: +-0 products).  Results go back through LDS so that the stores are
//   coalesced.  Same terms in the same order as delayVector: j ascending over the 21 real taps; the taps come from the
//   sinc grid when the fraction lies on it (always after peakDetect), else from the table sinc as the reference computes them.
// ---------------------------------------------------------------------------------------------
template <typename SMP>
__global__ __launch_bounds__(256) void k_eq_delay(const TrxTables *__restrict__ T, const void *__restrict__ samples,
                                                  const int32_t *__restrict__ offset, const int32_t *__restrict__ length, int B,
                                                  const cx *__restrict__ amp_in, const float *__restrict__ toa_in,
                                                  const uint8_t *__restrict__ flags, int need_mask, cx *__restrict__ xd,
                                                  int xstride) {
  constexpr int PADL = 16, ROW = 208, OPL = 10;            // 16 lanes x OPL outputs >= 157; windows span [PADL - 10, PADL + 169]
  static_assert(PADL >= 10 && PADL + 16 * OPL - 1 + 10 < ROW, "every window stays inside the row");
  __shared__ __attribute__((aligned(16))) cx rows[16][ROW];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int hl = lane & 15, slot = wave * 4 + (lane >> 4);
  const int b = blockIdx.x * 16 + slot;
  const bool live = b < B;
  int off = 0, N = 0;
  cx amp = mk(1.0f, 0.0f);
  float toa = 0.0f;
  uint8_t fl = 0;
  if (live) { off = offset[b]; N = length[b]; amp = amp_in[b]; toa = toa_in[b]; if (flags) fl = flags[b]; }
  bool enabled = live && (off >= 0) && (N >= 92) && (N <= 157) && (fabsf(toa) <= 4096.0f);   // k_demod's gate (also rejects NaN/inf)
  if (flags) enabled = enabled && (need_mask ? ((fl & need_mask) == need_mask) : (fl != 0));
  if (!enabled) N = 0;
  cx *S = rows[slot];
  // ---- the burst's loads first: sample n = hl + 16 i ----
  typename SMP::raw_t v[OPL];
#pragma unroll
  for (int i = 0; i < OPL; i++) {
    const int n = hl + 16 * i;
    v[i] = n < N ? SMP::ldraw(samples, (long long)off + n) : SMP::zero();
  }
  const cx inv = cdiv(mk(1.0f, 0.0f), amp);                // ((complex)1.0)/channel (Transceiver.cpp:346 / :1066)
  const float delay = -toa;                                // delayVector bookkeeping (:577-582)
  const int io = (int)floorf(delay);
  const float frac = delay - (float)io;
  const bool filt = fabs((double)frac) > 1e-2;
  float tp[21];
  eq_delay_taps(T, frac, tp, [&] {                         // off the grid: tap j is computed by lanes j and j - 16 of the burst
    const float tv0 = dev_sinc(T->sinT, TRX_PI_F * ((float)(hl - 10) - frac));
    const float tv1 = dev_sinc(T->sinT, TRX_PI_F * ((float)(hl + 6) - frac));
    const int first = lane & ~15;
    return [=](int j) { return j < 16 ? __shfl(tv0, first + j, 64) : __shfl(tv1, first + j - 16, 64); };
  });
  // ---- the scaled burst between zeros, already moved by the integer delay: sample n at S[PADL + n + io] (what falls
  //      outside the row lies outside every window below) ----
#pragma unroll
  for (int i = 0; i < ROW / 16; i++) S[hl + 16 * i] = mk(0, 0);
  wave_lds_fence();
#pragma unroll
  for (int i = 0; i < OPL; i++) {
    const int n = hl + 16 * i, p = PADL + n + io;
    if (n < N && p >= 0 && p < ROW) S[p] = cmul(SMP::widen(v[i]), inv);   // scaleVector (:713-723)
  }
  wave_lds_fence();
  // ---- outputs m = OPL*hl + i: shifted[m] = filtered[m - io] inside [0, N), else 0 (:597-613); tap j of output m meets
  //      position PADL + m + 10 - j = w[i + 20 - j] ----
  cx y[OPL];
  {
    // packed float32 pairs (one v_pk_mul_f32 + one v_pk_add_f32 per complex-by-real multiply-add, each half rounded on its own:
    // the same values as cmulr + cadd in half the instructions -- this kernel is bound by what its few waves can issue)
    const cx *W = S + (PADL + OPL * hl - 10);
    v2f w[OPL + 20], tp2[21];
#pragma unroll
    for (int k = 0; k < OPL + 20; k++) w[k] = pk(W[k]);
#pragma unroll
    for (int j = 0; j < 21; j++) { tp2[j].x = tp[j]; tp2[j].y = tp[j]; }
#pragma unroll
    for (int i = 0; i < OPL; i++) {
      v2f acc = pk(mk(0, 0));
#pragma unroll
      for (int j = 0; j < 21; j++) acc = pk_cadd(acc, pk_mul(w[i + 20 - j], tp2[j]));   // convolve(..., NO_DELAY), j ascending (:590)
      const int t = OPL * hl + i - io;
      const v2f r = filt ? acc : w[i + 10];
      y[i] = (t >= 0 && t < N) ? mk(r.x, r.y) : mk(0, 0);
    }
  }
  // ---- through LDS again, so that a store instruction writes 16 consecutive samples of each burst ----
  wave_lds_fence();
#pragma unroll
  for (int i = 0; i < OPL; i++) S[OPL * hl + i] = y[i];
  wave_lds_fence();
  // The whole row is written: the delayed burst's N samples, zeros from N to the row's end (and a row of zeros for a burst the
  // gate refused), so the equaliser's tile loads need no mask.  Its feed-forward sums still SKIP the terms beyond the burst, as
  // the reference does: a zero sample stands for a skipped term only while the tap is finite (k_eq_dfe2's producer).
  cx *out = xd + (size_t)(live ? b : 0) * xstride;
#pragma unroll
  for (int i = 0; i < OPL; i++) {
    const int m = hl + 16 * i;
    if (live && m < xstride) out[m] = m < N ? S[m] : mk(0, 0);
  }
}

// Some burst of the wave is equalised with a feed-forward tap that is Inf or NaN (wave-uniform).  Only then does a zero sample stop
// standing for a skipped term -- 0 * w is +-0 for every finite w -- and the feed-forward sums need their range check.
__device__ __forceinline__ bool eq_taps_hostile(bool det, const v2f (&w)[7]) {
  bool fin = true;
#pragma unroll
  for (int j = 0; j < 7; j++) fin = fin && __builtin_isfinite(w[j].x) && __builtin_isfinite(w[j].y);
  return __any(det && !fin);
}

// ---------------------------------------------------------------------------------------------
// k_eq_dfe2: equalizeBurst (:1352-1384) for 64 bursts per workgroup with TWO waves: lane l of the producer wave and
//   lane l of the consumer wave share burst l.
//   * The feed-forward FIR does not depend on the decisions: the PRODUCER computes ff[k] = sum_j x[k+6-j] w[j]
//     (the reference's terms in the reference's order) a tile of 16 symbols ahead and hands it over through LDS.
//   * The CONSUMER runs the serial part only: d = ((((ff + b0 h0) + b1 h1) + ...) -- the same accumulator the
//     reference continues after its feed-forward terms -- reverse rotation, decision, feedback, slicer
//     (66 instead of 125 VALU per symbol on the critical path).
//   * Neither touches global memory per symbol: the delayed burst comes in and the soft bits go out tile-wise, with
//     lanes spread along k (4 rows x 16 symbols per instruction = whole cache lines) instead of 64 rows x one symbol.
//   (The form this replaced, a lane per burst doing everything -- one uncoalesced 8-byte load and 4-byte store per symbol with
//   one step of latency cover -- took 110 us per 64 K bursts.)
// ---------------------------------------------------------------------------------------------
// One symbol of equalizeBurst's decision-feedback loop (:1370-1384) on the feed-forward sum ff: the feedback terms continue the
// same accumulator in the reference's order, reverse rotation, decision, the rotated decision goes into the history, slicer.
// (Round 3 also ran this step on packed float32 pairs -- pk_cmul / pk_cadd of trxsig_dev.h, 31 instead of 66 instructions, the
// same values: k_eq_dfe2 57.2 -> 60.1 us.  The recursion is bound by the latency of its dependent chain, not by the
// consumer wave's instruction count.)
__device__ __forceinline__ float dfe_step(int k, int nout, cx ff, cx rv, cx rt, const v2f (&bq)[5], v2f (&hist)[5]) {
  // Branch-free: a burst shorter than the tile keeps stepping (its history is never looked at again) and only the result is
  // masked.  Packed float32 pairs (pk_cmul / pk_cadd, trxsig_dev.h: the reference's products and sums, each rounded on its
  // own): a complex multiply-add is 4 instructions instead of 8.
  v2f d = pk(ff);                                           // the feed-forward terms, already summed in order
#pragma unroll
  for (int j = 0; j < 5; j++)                               // feedback over past decisions (:1370-1374)
    if (k - 1 - j >= 0) d = pk_cadd(d, pk_cmul(bq[j], hist[j]));
  d = pk_cmul(d, pk(rv));                                   // :1375
  const float re = d.x;
  const cx dec = mk((re > 0.0f) ? 1.0f : -1.0f, 0.0f);      // :1378
  const v2f fbv = pk_cmul(pk(dec), pk(rt));                 // :1380
#pragma unroll
  for (int j = 4; j > 0; j--) hist[j] = hist[j - 1];
  hist[0] = fbv;
  float sv = (re + 1.0F) * 0.5F;                            // vectorSlicer (:513-515): (float)(0.5*(double)(re + 1.0F)); re + 1.0F is 0 or
  //                                                           at least 2^-24 in magnitude, so halving it in float is exact too
  if (sv > 1.0f) sv = 1.0f;
  if (sv < 0.0f) sv = 0.0f;
  return k < nout ? sv : 0.0f;
}

// The taps burst b is equalised with: its own at index b, or, with tap_ix, those at tap_ix[b] (the per-timeslot cache of
// Transceiver.cpp:317-349: many bursts share one estimate; a burst that is not equalised reads entry 0 and uses nothing of it).
__device__ __forceinline__ size_t eq_tap_base(const int32_t *tap_ix, bool det, int bb) {
  return (tap_ix && det) ? (size_t)tap_ix[bb] : (tap_ix ? (size_t)0 : (size_t)bb);
}

// The feed-forward sums of tile u (TK symbols) of one burst: ff[i] = sum_j x[k + 6 - j] w[j], k = TK u + i.  xa: the tile's delayed samples
// (x[k + 6] at xa[i]), win: the six before them (x[TK u + 5 - m] at win[m]).
// convolve general branch: sum += a[t-j]*b[j], t = k+6; k + 6 - j >= 0 always, and a term beyond the burst (k + 6 - j >= N) is
// SKIPPED in the reference (:322-366).  The row holds zero samples there (k_eq_delay), and with FINITE taps the product adds
// +-0 to a sum that starts at +0: the same value, with no branch and no range check.  But the taps may be the caller's
// (trxsig_equalize_taps_batch) or designDFE's answer to a hostile channel, and 0 * Inf and 0 * NaN are NaN: where a tap of
// the wave is not finite, the tiles in which some lane's burst ends select such terms away instead (CHK; Nff: the burst's end).
template <int TK, bool CHK>
__device__ __forceinline__ void eq_ff_tile(int u, int Nff, const v2f (&xa)[TK], const v2f (&win)[6], const v2f (&w)[7], cx *ff) {
#pragma unroll
  for (int i = 0; i < TK; i++) {
    v2f d = pk(mk(0, 0));
#pragma unroll
    for (int j = 0; j < 7; j++) {
      const v2f xv = (i - j >= 0) ? xa[(i - j >= 0) ? i - j : 0] : win[(j - i - 1 < 6) ? j - i - 1 : 5];
      const v2f term = pk_cadd(d, pk_cmul(xv, w[j]));
      d = (!CHK || TK * u + i + 6 - j < Nff) ? term : d;
    }
    ff[i] = unpk(d);
  }
}

// The consumer's tile: the operands up front -- feed-forward sums (LDS), rotation factors (uniform -> scalar loads) -- then TK steps of
// the recursion; the soft bits go to sf (LDS), on their way out.
template <int TK>
__device__ __forceinline__ void eq_dfe_tile(const TrxTables *T, int u, int nout, const cx *ff, float *sf, const v2f (&bq)[5], v2f (&hist)[5]) {
  cx ffv[TK], rv[TK], rt[TK];
#pragma unroll
  for (int i = 0; i < TK; i++) {
    ffv[i] = ff[i];
    rv[i] = T->rev[TK * u + i];                             // (rev/rot hold 157 * 4 entries: in range for k < 160)
    rt[i] = T->rot[TK * u + i];
  }
#pragma unroll
  for (int i = 0; i < TK; i++) sf[i] = dfe_step(TK * u + i, nout, ffv[i], rv[i], rt[i], bq, hist);
}

// Soft tile u of the workgroup's 64 bursts (sf[burst][symbol], LDS) goes out with the wave's lanes along k: 64 / TK rows x TK symbols per
// instruction = whole cache lines, instead of 64 rows x one symbol.
template <int TK>
__device__ __forceinline__ void eq_soft_out(int u, int lane, int b0, int B, int nsoft, int stride, const float (*sf)[TK + 1], float *soft,
                                            uint8_t *hard) {
  const int kc = lane & (TK - 1), r0 = lane / TK;            // this lane moves column kc of rows r0 + (64 / TK) i
#pragma unroll
  for (int i = 0; i < TK; i++) {
    const int r = r0 + (64 / TK) * i, k = TK * u + kc, rb = b0 + r;
    if (rb < B && k < nsoft) {
      const float sv = sf[r][kc];
      soft[(size_t)rb * stride + k] = sv;
      if (hard) hard[(size_t)rb * stride + k] = sv > 0.5F;
    }
  }
}

#define EQ_TK 16             /* symbols per tile */
#define EQ_NT 10             /* tiles: 160 >= 157 symbols */
__global__ __launch_bounds__(128) void k_eq_dfe2(const TrxTables *__restrict__ T, const cx *__restrict__ xd, int xstride,
                                                 const int32_t *__restrict__ length, int B,
                                                 const uint8_t *__restrict__ flags, const float *__restrict__ toa_eq,
                                                 const cx *__restrict__ w_in,
                                                 const cx *__restrict__ b_in, float *__restrict__ soft,
                                                 uint8_t *__restrict__ hard, int nsoft, int stride,
                                                 const int32_t *__restrict__ tap_ix) {
  // tap_ix (optional): burst b is equalised with the taps at w_in + 7 tap_ix[b], b_in + 5 tap_ix[b] (the per-timeslot cache
  // of Transceiver.cpp:317-349: many bursts share one estimate); NULL = its own taps at index b.
  __shared__ cx xt[64][EQ_TK + 1];                          // the producer's own staging of the delayed burst
  __shared__ cx fft[2][64][EQ_TK + 1];                      // producer -> consumer
  __shared__ float sft[2][64][EQ_TK + 1];                   // consumer -> producer (soft bits on their way out)
  const int lane = threadIdx.x & 63;
  const bool producer = threadIdx.x >= 64;                  // wave-uniform
  const int b0 = blockIdx.x * 64;
  const int b = b0 + lane;
  const int bb = b < B ? b : B - 1;
  const int N = length[bb];
  const bool det = b < B && eq_enabled(flags[bb], N, toa_eq[bb]);
  const int nout = det ? (nsoft < N ? nsoft : N) : 0;       // symbols this burst really produces (zeros beyond)
  const size_t tb = eq_tap_base(tap_ix, det, bb);
  // Barrier u (u = 0..9): ff tile u is ready and soft tile u-1 is complete; barrier 10: soft tile 9 is complete.
  // Both waves execute exactly eleven barriers.
  if (producer) {
    const int kc = lane & 15, r0 = lane >> 4;               // tile traffic: this lane moves column kc of rows r0 + 4 i
    const cx *x = xd + (size_t)bb * xstride;
    v2f w[7], win[6];
#pragma unroll
    for (int j = 0; j < 7; j++) w[j] = pk(w_in[tb * 7 + j]);
#pragma unroll
    for (int m = 0; m < 6; m++) win[m] = pk(x[5 - m]);       // win[m] = x[16 u + 5 - m] (the row holds zeros from N on: k_eq_delay)
    const int Nff = det ? N : 160;                          // the burst's end for the feed-forward terms (a burst that is not equalised has none)
    const bool hostile = eq_taps_hostile(det, w);           // (wave-uniform) some burst's taps are not finite
    // sample tile u: a = 16 u + 6 + c, c = 0..15 (output k = 16 u + i needs x[k + 6 - j]: FULL_SPAN keeps [6, 6+N), :1352-1356)
    auto load_tile = [&](int u, cx (&v)[16]) {
#pragma unroll
      for (int i = 0; i < 16; i++) {
        const int rb = b0 + r0 + 4 * i, a = EQ_TK * u + 6 + kc;
        v[i] = (rb < B && a < xstride) ? xd[(size_t)rb * xstride + a] : mk(0, 0);
      }
    };
    cx v[16];
    load_tile(0, v);
    for (int u = 0; u < EQ_NT; u++) {
      wave_lds_fence();                                     // everybody has taken its row of the previous tile
#pragma unroll
      for (int i = 0; i < 16; i++) xt[r0 + 4 * i][kc] = v[i];
      wave_lds_fence();
      if (u + 1 < EQ_NT) load_tile(u + 1, v);               // the next tile's loads fly during this tile's arithmetic
      v2f xa[16];
#pragma unroll
      for (int i = 0; i < 16; i++) xa[i] = pk(xt[lane][i]);
      if (!hostile || __all(EQ_TK * u + 15 + 6 < Nff)) eq_ff_tile<EQ_TK, false>(u, Nff, xa, win, w, fft[u & 1][lane]);
      else eq_ff_tile<EQ_TK, true>(u, Nff, xa, win, w, fft[u & 1][lane]);
#pragma unroll
      for (int m = 0; m < 6; m++) win[m] = xa[15 - m];
      __syncthreads();                                      // barrier u
      if (u >= 1) eq_soft_out<EQ_TK>(u - 1, lane, b0, B, nsoft, stride, sft[(u - 1) & 1], soft, hard);
    }
    __syncthreads();                                        // barrier 10
    eq_soft_out<EQ_TK>(EQ_NT - 1, lane, b0, B, nsoft, stride, sft[(EQ_NT - 1) & 1], soft, hard);
  } else {
    v2f bq[5], hist[5];
#pragma unroll
    for (int j = 0; j < 5; j++) { bq[j] = pk(b_in[tb * 5 + j]); hist[j] = pk(mk(0, 0)); }
    for (int u = 0; u < EQ_NT; u++) {
      __syncthreads();                                      // barrier u
      eq_dfe_tile<EQ_TK>(T, u, nout, fft[u & 1][lane], sft[u & 1][lane], bq, hist);
    }
    __syncthreads();                                        // barrier 10
  }
}

// ---------------------------------------------------------------------------------------------
// k_eq_dfe4 (round 4): scaleVector + delayVector + equalizeBurst in ONE kernel -- what k_eq_delay and k_eq_dfe2 do through the
//   160-sample scratch row of every burst (84 MB written, 107 MB read back per 65,536 bursts), with that row never leaving the chip.
//   Round 3's kernel with the same aim (since removed) lost, 160 us against 37 + 57: its sample ring in LDS and 16-symbol tiles took
//   78 KB, two workgroups per CU, so the 1,024 workgroups ran in two generations, each as long as the recursion's latency chain.
//   Here the delay waves keep their 28-sample windows in REGISTERS, fed by 16-byte loads of the lane's own burst (a lane per burst in
//   every wave: no transposition, no ring), and the tiles are EIGHT symbols: 23 KB of LDS, all 1,024 workgroups of a 65,536-burst
//   call resident at four waves per SIMD (28 KB with the tile buffer in three copies).
//   64 bursts per workgroup, four waves, lane l of every wave = burst l; time runs in steps of eight symbols:
//     waves 2, 3  delayVector (:573-616; k_eq_delay's arithmetic: scaleVector(1/amp) on the way in, 21 real taps from the sinc grid or
//                 the table sinc, j ascending) -- tile u (delayed samples 8 u + 6 .. 8 u + 13) is wave 2 + (u & 1)'s, over steps
//                 u - 2 and u - 1, four outputs in each; tile -1 (samples 0 .. 5: the first window of the feed-forward filter) too;
//     wave 1      the feed-forward FIR of tile u in step u (k_eq_dfe2's producer), soft bits of tile u - 2 out (lanes along k);
//     wave 0      the decision-feedback recursion of tile u - 1 (k_eq_dfe2's consumer).
//   One workgroup barrier per step, 25 steps.  Same terms in the same order as k_eq_delay + k_eq_dfe2: the same values.
// ---------------------------------------------------------------------------------------------
#define EQ4_TK 8
#define EQ4_NT 20             /* 160 >= 157 symbols */
template <typename SMP>
__global__ __launch_bounds__(256, 4) void k_eq_dfe4(const TrxTables *__restrict__ T, const void *__restrict__ samples,
                                                    const int32_t *__restrict__ offset, const int32_t *__restrict__ length, int B,
                                                    const cx *__restrict__ amp_in, const float *__restrict__ toa_eq,
                                                    const uint8_t *__restrict__ flags, const cx *__restrict__ w_in,
                                                    const cx *__restrict__ b_in, const int32_t *__restrict__ tap_ix,
                                                    float *__restrict__ soft, uint8_t *__restrict__ hard, int nsoft, int stride) {
  constexpr int TK = EQ4_TK, NT = EQ4_NT, S0 = -3, S1 = NT + 1;   // steps S0 .. S1
  __shared__ cx xt[3][64][TK + 1];                          // delay waves -> feed-forward wave (tile u in xt[u mod 3]: written over steps u - 2, u - 1, read in step u)
  __shared__ cx fft[2][64][TK + 1];                         // feed-forward wave -> consumer
  __shared__ float sft[2][64][TK + 1];                      // consumer -> feed-forward wave (soft bits on their way out)
  __shared__ __attribute__((aligned(8))) float tapl[2][64][22];   // a delay wave's 21 taps per lane (registers are what the delay waves are short of)
  const int lane = threadIdx.x & 63;
  EqProbe probe;                                            // (probe build: per role, cycles between barriers (work) and at them (wait), tools/dfe4_probe.py)
  // (the roles rotate from workgroup to workgroup: a SIMD then hosts one wave of each role instead of four of a kind, and what it has to
  //  issue per step is the roles' average, not the heaviest role's)
  // (workgroups 256 apart tend to share a CU -- the dispatcher deals them out round-robin over 8 XCDs x 32 CUs --: those get different rotations)
  const int wave = __builtin_amdgcn_readfirstlane((((int)threadIdx.x >> 6) + ((int)blockIdx.x >> 8) + (int)blockIdx.x) & 3);
  const int b0 = blockIdx.x * 64;
  const int b = b0 + lane;
  const int bb = b < B ? b : B - 1;
  const int N = length[bb];
  const float te = toa_eq[bb];
  const bool det = b < B && eq_enabled(flags[bb], N, te);  // k_eq_dfe2's gate
  if (wave >= 2) {
    // ---- delayVector: this wave's tiles u = d - 2, d, d + 2, ... (d = wave - 2; wave 3 starts with tile -1) ----
    const int d = wave - 2;
    const int off = offset[bb];
    const int Nd = (det && off >= 0) ? N : 0;              // k_eq_delay's gate: a refused burst is a row of zeros
    const long long base = Nd > 0 ? (long long)off : 0;
    const v2f inv = pk(cdiv(mk(1.0f, 0.0f), amp_in[bb]));  // ((complex)1.0)/amp (Transceiver.cpp:391)
    const float delay = det ? -te : 0.0f;                  // (a burst that is not equalised may carry any TOA, and the table sinc does not come back from a huge argument)
    const int io = (int)floorf(delay);
    const float frac = delay - (float)io;
    const bool filt = fabs((double)frac) > 1e-2;
    v2f *const tl = reinterpret_cast<v2f *>(tapl[d][lane]);   // taps 2 q, 2 q + 1 at tl[q]
    {
      float g[21];                                         // (off the grid every lane evaluates its own 21 sincs: a lane per burst here)
      eq_delay_taps(T, frac, g, [&] { return [&](int j) { return dev_sinc(T->sinT, TRX_PI_F * ((float)(j - 10) - frac)); }; });
#pragma unroll
      for (int q = 0; q < 10; q++) { v2f t2; t2.x = g[2 * q]; t2.y = g[2 * q + 1]; tl[q] = t2; }
      { v2f t2; t2.x = g[20]; t2.y = 0.0f; tl[10] = t2; }    // (the pair's second half, "tap 21", is never used)
    }
    wave_lds_fence();
    // The window: a RING of 32 scaled samples in registers, sample n at w[(n - n0) & 31] (n0 = the first own tile's first sample).  Own
    // tile number k (u = u_first + 2 k) reads samples n0 + 16 k .. n0 + 16 k + 27 -- tap j of output c meets ring entry
    // (16 k + c + 20 - j) & 31, a compile-time index once k's parity is one (the loop below runs two own tiles per round) -- and the
    // sixteen samples the next own tile adds replace the sixteen this one read first.  No entry is ever moved.
    v2f w[32];
    constexpr int PER = 16 / (16 / SMP::kBytes);           // 16-byte loads that bring sixteen samples (4 at fp16, 8 at complex float)
    constexpr int SPL = 16 / SMP::kBytes;                  // samples per load
    struct __attribute__((packed, aligned(4))) Piece { typename SMP::raw_t q[SPL]; };
    // sixteen samples n .. n + 15 in two moves: the loads (into rv, as stored) are issued a step before they are needed ...
    typename SMP::raw_t rv[16];
    bool rv_inside = false;                                // (wave-uniform) every lane's sixteen lie inside its burst: no masks when they are taken
    auto issue16 = [&](int n) {
      const bool inside = n >= 0 && n + 15 < Nd;
      rv_inside = __all(inside || Nd == 0);
      if (rv_inside) {                                     // (a refused burst reads burst 0's samples: its outputs are zeros whatever they are)
        Piece pc[PER];
        const long long a0 = base + (Nd > 0 ? n : 0);
#pragma unroll
        for (int q = 0; q < PER; q++) pc[q] = *reinterpret_cast<const Piece *>(reinterpret_cast<const typename SMP::raw_t *>(samples) + (a0 + SPL * q));
#pragma unroll
        for (int q = 0; q < PER; q++) {
#pragma unroll
          for (int e = 0; e < SPL; e++) rv[SPL * q + e] = pc[q].q[e];
        }
      } else {                                              // a burst's edge in some lane: sample by sample, index clamped
#pragma unroll
        for (int k = 0; k < 16; k++) {
          const int nn = n + k;
          const int nc = nn < 0 ? 0 : (nn >= Nd ? (Nd > 0 ? Nd - 1 : 0) : nn);
          rv[k] = SMP::ldraw(samples, base + nc);
        }
      }
    };
    // ... and scaled into ring entries R0 .. R0 + 15 (zeros outside [0, Nd)) once the entries' old samples have been read
    auto take16 = [&](int n, auto r0_) {
      constexpr int R0 = decltype(r0_)::value;
      if (rv_inside) {
#pragma unroll
        for (int k = 0; k < 16; k++) w[R0 + k] = pk_cmul(pk(SMP::widen(rv[k])), inv);   // scaleVector (:713-723)
      } else {
#pragma unroll
        for (int k = 0; k < 16; k++) {
          const int nn = n + k;
          const v2f sc = pk_cmul(pk(SMP::widen(rv[k])), inv);
          w[R0 + k] = (nn >= 0 && nn < Nd) ? sc : pk(mk(0, 0));
        }
      }
    };
    const int u_first = d == 1 ? -1 : 0;
    const int n_own = d == 1 ? (NT + 1) / 2 + 1 : NT / 2;  // own tiles: -1, 1, .., NT - 1 / 0, 2, .., NT - 2
    const int n0 = TK * u_first + 6 - io - 10;
    issue16(n0); take16(n0, std::integral_constant<int, 0>());
    issue16(n0 + 16); take16(n0 + 16, std::integral_constant<int, 16>());
    // outputs C0 .. C0 + NC - 1 of own tile u (ring phase PH) into its tile buffer.  (Five in the tile's first step, three in its second, which
    // also takes the next samples in: the two delay waves are in opposite halves of their tiles, and the longer half sets the workgroup's step.)
    constexpr int NC1 = 5;
    auto outputs = [&](int u, auto ph_, auto c0_, auto nc_) {
      constexpr int PH = decltype(ph_)::value, C0 = decltype(c0_)::value, NC = decltype(nc_)::value;
      const int m0 = TK * u + 6;
      cx *row = xt[((u % 3) + 3) % 3][lane];
      v2f acc[NC];
#pragma unroll
      for (int c = 0; c < NC; c++) acc[c] = pk(mk(0, 0));
#pragma unroll
      for (int q = 0; q < 11; q++) {   // convolve(..., NO_DELAY), j ascending (:590): the outputs side by side, tap pair by tap pair
        const v2f tq = tl[q];
#pragma unroll
        for (int c = 0; c < NC; c++) acc[c] = pk_cadd(acc[c], pk_mul_tap<0>(w[(PH + C0 + c + 20 - 2 * q) & 31], tq));
        if (2 * q + 1 <= 20) {
#pragma unroll
          for (int c = 0; c < NC; c++) acc[c] = pk_cadd(acc[c], pk_mul_tap<1>(w[(PH + C0 + c + 19 - 2 * q) & 31], tq));
        }
        if ((q & 3) == 3) __builtin_amdgcn_sched_barrier(0);   // (the tap reads four pairs at a time: all eleven up front cost the registers they were moved to LDS for)
      }
#pragma unroll
      for (int c = 0; c < NC; c++) {
        const int m = m0 + C0 + c, t = m - io;
        const v2f r = filt ? acc[c] : w[(PH + C0 + c + 10) & 31];
        row[C0 + c] = (t >= 0 && t < Nd && m < Nd) ? unpk(r) : mk(0, 0);   // shifted[m] inside [0, N), else 0 (:597-613); the row holds zeros from N on
      }
    };
    // one own tile = two steps.  k: its number; the samples of own tile k + 1 beyond this one's: n0 + 16 k + 32 .. + 47, into the ring's half
    // this tile read first
    auto own_tile = [&](int k, auto ph_) {
      constexpr int PH = decltype(ph_)::value;
      const int u = u_first + 2 * k;
      outputs(u, ph_, std::integral_constant<int, 0>(), std::integral_constant<int, NC1>());
      const bool more = k + 1 < n_own;
      if (more) issue16(n0 + 16 * k + 32);                 // (after the sums: sixteen more live registers they have no room for) a step to land
      probe.barrier();
      outputs(u, ph_, std::integral_constant<int, NC1>(), std::integral_constant<int, TK - NC1>());
      if (more) take16(n0 + 16 * k + 32, std::integral_constant<int, PH>());
      probe.barrier();
    };
    constexpr int STEPS = S1 - S0 + 1;
    const int lead = d == 1 ? 0 : 1;                       // wave 3's tile -1 starts in step S0, wave 2's tile 0 a step later
    for (int i = 0; i < lead; i++) probe.barrier();
    for (int k = 0; k < n_own; k += 2) {
      own_tile(k, std::integral_constant<int, 0>());
      if (k + 1 < n_own) own_tile(k + 1, std::integral_constant<int, 16>());
    }
    for (int i = lead + 2 * n_own; i < STEPS; i++) probe.barrier();
  } else if (wave == 1) {
    // ---- the feed-forward FIR (k_eq_dfe2's producer) and the soft bits' way out ----
    const size_t tb = eq_tap_base(tap_ix, det, bb);
    v2f wf[7], win[6];
#pragma unroll
    for (int j = 0; j < 7; j++) wf[j] = pk(w_in[tb * 7 + j]);
#pragma unroll
    for (int m = 0; m < 6; m++) win[m] = pk(mk(0, 0));
    const int Nff = det ? N : 160;                          // the burst's end for the feed-forward terms (a burst that is not equalised has none)
    const bool hostile = eq_taps_hostile(det, wf);          // (wave-uniform) some burst's taps are not finite: zero samples no longer stand for skipped terms
    for (int s = S0; s <= S1; s++) {
      const int u = s;
      if (u >= -1 && u <= NT - 1) {
        v2f xa[TK];
#pragma unroll
        for (int i = 0; i < TK; i++) xa[i] = pk(xt[((u % 3) + 3) % 3][lane][i]);
        if (u >= 0) {
          // (the terms beyond the burst SKIPPED -- by the range check where a tap of the wave is not finite and some lane's burst ends in
          //  the tile, by the zero samples everywhere else: see eq_ff_tile)
          if (!hostile || __all(TK * u + TK - 1 + 6 < Nff)) eq_ff_tile<TK, false>(u, Nff, xa, win, wf, fft[u & 1][lane]);
          else eq_ff_tile<TK, true>(u, Nff, xa, win, wf, fft[u & 1][lane]);
        }
#pragma unroll
        for (int m = 0; m < 6; m++) win[m] = xa[TK - 1 - m];  // delayed samples 8 u + 13 - m: the next tile's x[k + 6 - j], j > i
      }
      if (s - 2 >= 0 && s - 2 <= NT - 1) eq_soft_out<TK>(s - 2, lane, b0, B, nsoft, stride, sft[s & 1], soft, hard);
      probe.barrier();
    }
  } else {
    // ---- the decision-feedback recursion (k_eq_dfe2's consumer) ----
    const int nout = det ? (nsoft < N ? nsoft : N) : 0;     // symbols this burst really produces (zeros beyond)
    const size_t tb = eq_tap_base(tap_ix, det, bb);
    v2f bq[5], hist[5];
#pragma unroll
    for (int j = 0; j < 5; j++) { bq[j] = pk(b_in[tb * 5 + j]); hist[j] = pk(mk(0, 0)); }
    for (int s = S0; s <= S1; s++) {
      const int u = s - 1;
      if (u >= 0 && u <= NT - 1) {
        eq_dfe_tile<TK>(T, u, nout, fft[u & 1][lane], sft[u & 1][lane], bq, hist);
      }
      probe.barrier();
    }
  }
  if (lane == 0 && b0 + wave < B) probe.report(soft + (size_t)(b0 + wave) * stride, wave);   // (probe build: row b0 + role = {work, wait, total, role})
}

}  // namespace

// trxsig_set_tuning(TRXSIG_TUNE_EQ_TAIL, 2) (A/B and the tests): k_eq_delay + k_eq_dfe2 through the scratch rows instead of the fused k_eq_dfe4
static bool eq_tail_fused() { return trx_knob(TRX_KNOB_EQ_TAIL) != 2; }
static void launch_eq_tail(hipStream_t st, const TrxTables *dT, const void *samples, int fmt, const int32_t *off, const int32_t *len, int B,
                           const trx_c32 *amp, const float *toa_eq, const uint8_t *flags, const trx_c32 *w, const trx_c32 *bq, trx_c32 *xd,
                           int xstride, float *soft, uint8_t *hard, int nsoft, int stride, const int32_t *tap_ix, TrxProfiler *prof) {
  if (eq_tail_fused()) {                                    // one kernel: the delayed burst stays on the chip
    if (prof) prof->begin(TRXSIG_K_EQ_DFE, st);
    eq_with_fmt(fmt, [&](auto smp) {
      k_eq_dfe4<decltype(smp)><<<dim3((B + 63) / 64), dim3(256), 0, st>>>(dT, samples, off, len, B, amp, toa_eq, flags, w, bq, tap_ix, soft, hard, nsoft,
                                                                          stride);
    });
    if (prof) prof->end(TRXSIG_K_EQ_DFE, st);
    return;
  }
  if (prof) prof->begin(TRXSIG_K_EQ_DELAY, st);
  eq_with_fmt(fmt, [&](auto smp) {
    k_eq_delay<decltype(smp)><<<dim3((B + 15) / 16), dim3(256), 0, st>>>(dT, samples, off, len, B, amp, toa_eq, flags, TRXSIG_F_DETECT, xd, xstride);
  });
  if (prof) { prof->end(TRXSIG_K_EQ_DELAY, st); prof->begin(TRXSIG_K_EQ_DFE, st); }
  k_eq_dfe2<<<dim3((B + 63) / 64), dim3(128), 0, st>>>(dT, xd, xstride, len, B, flags, toa_eq, w, bq, soft, hard, nsoft, stride, tap_ix);
  if (prof) prof->end(TRXSIG_K_EQ_DFE, st);
}

// scaleVector(burst, 1/amp) + equalizeBurst(burst, toa_eq, w, b) with caller-supplied taps (7 + 5 per burst): the second half of
// trx_launch_equalize (trxsig_eq_est.hip), and on its own for the Transceiver facade, which caches DFE taps per timeslot
hipError_t trx_launch_equalize_taps(hipStream_t st, const TrxTables *dT, const void *samples, int fmt, const int32_t *off,
                                    const int32_t *len, int B, const trx_c32 *amp, const float *toa_eq,
                                    const uint8_t *flags, const trx_c32 *w, const trx_c32 *bq, trx_c32 *xd, int xstride,
                                    float *soft, uint8_t *hard, int nsoft, int stride, TrxProfiler *prof, const int32_t *tap_ix) {
  if (B <= 0) return hipSuccess;
  launch_eq_tail(st, dT, samples, fmt, off, len, B, amp, toa_eq, flags, w, bq, xd, xstride, soft, hard, nsoft, stride, tap_ix, prof);
  return hipGetLastError();
}
