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
// The steps themselves -- symbols, the tap sum, the window, the trellis, the soft bits out -- are in trxsig_mlse_dev.h, shared with the
// other five equaliser kernels; what is here is this kernel's own: two bursts a wave, the midamble's taps, the half-burst maps.
#include "trxsig_mlse_dev.h"                               // the steps shared with the other five equaliser kernels

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
      enabled = mlse_enabled<SPS>(off, N, toa, flags, need_mask, b);
    }
    if (!__builtin_amdgcn_readfirstlane(enabled)) {
      mlse_zero(Y, lane);
      continue;
    }
    state[j] = mlse_symbols<SPS>(T, ph[wave], samples, off, N, amp, toa, lane, Y) ? 1 : 0;
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
    const cx cd = mlse_corr_tap(tsc_bits, (s < 9 ? s : 8) - 4, Y);
    if (s < 9) scr[s] = cd;
  }
  wave_lds_fence();
  cx h[5];
  int w;
  const float E = mlse_window(scr, h, w);
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
  // start state: bit 0 first a[86], a[85], a[84], a[83] (right) or a[61], a[62], a[63], a[64] (left); a[61 + t] = training bit t
  const int start = left ? (int)(tsc_bits & 15u)
                         : (int)(((tsc_bits >> 25) & 1u) | (((tsc_bits >> 24) & 1u) << 1) | (((tsc_bits >> 23) & 1u) << 2) | (((tsc_bits >> 22) & 1u) << 3));
  // step i = 0..60 is symbol m = 87 + i with sample y[m + w] (right), m = 60 - i with y[m + 4 + w] (left)
  float D[4] = {0.0f, 0.0f, 0.0f, 0.0f};
  mlse_trellis<61>(Y, left ? 64 + w : 87 + w, left ? -1 : 1, zf0, zf1, scr, lane, start, D);

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
      if (i < 61 && m < nsoft) mlse_soft_out(sb, hb, m, D[q], den);
    }
    const int m = 61 + hl;                                  // the midamble: the demodulator's formula
    if (hl < 26 && m < nsoft) mlse_put(sb, hb, m, mlse_slice(Y[m].r));
  } else {
    mlse_fall_back(sb, hb, Y, st_, hl, 32, nsoft);
  }
}

}  // namespace

hipError_t trx_launch_mlse(hipStream_t st, int sps, const TrxTables *dT, const TrxMlseArgs &a) {
  return mlse_launch<2 * TRX_MLSE_WAVES, true>(sps, a, [&](auto S, dim3 grid, dim3 block) {
    k_mlse<decltype(S)::value><<<grid, block, 0, st>>>(dT, a.samples0, a.off0, a.len, a.B, a.tsc_bits, a.amp, a.toa, a.flags, a.need_mask, a.chan,
                                                       a.win, a.soft, a.hard, a.nsoft, a.stride);
  });
}
