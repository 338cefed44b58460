// trxsig_mlse_sch.hip -- the sequence equaliser for synchronisation bursts (trxsig_mlse_sch_batch; trxsig_l1acq's
// TRXSIG_SCHLEG_MLSE): a nine-tap least-squares channel estimate from the burst's 64-symbol extended training sequence and TWO
// half-burst 16-state max-log-MAP trellises of 42 steps each (39 coded bits and 3 tail bits a side), at any sps.  The reference
// has no counterpart; the stage is pinned by the float32 model tests/mlse_sch_model.py, which this kernel equals word for word, and
// graded against the float64 statement tests/mlse_sch_ref.py.  The arithmetic rules are k_mlse's (trxsig_mlse.hip): float add,
// subtract, multiply, minimum, compare and one correctly rounded division per soft bit; nothing is fused.  The algorithm is stated
// in include/trxsig.h (trxsig_mlse_sch_batch) and again, operation by operation, in the model.
//
// Layout.  One wave takes TWO bursts: k_mlse's rows with k_mlse_access's estimator, every step from trxsig_mlse_dev.h.
//   * Symbols: the whole wave computes one burst at a time with k_demod's own code (demod_core, RAW form) and keeps the 148 rotated
//     outputs, complex, in LDS.  The loop over the two bursts is NOT unrolled (the bursts' states travel in one packed register):
//     one copy of demod_core in the listing, as in k_mlse_access.
//   * Estimate: lanes 0..8 of a row form c[-4..4], 56 multiply-adds each on LDS reads of y[46..101]; both rows of a burst do the
//     same sums (a row is the unit everything after it works in, and the other 7 lanes of a row idle either way).  The table P32
//     (trxsig_mlse_sch_tab.h, 2,016 B) is read from constant memory by plain global loads, lane d its own row, as in
//     k_mlse_access: read once per wave, L2- and L1-resident for the whole launch, no LDS for it.
//   * Trellis: each of the wave's four 16-lane rows is one half-burst trellis (rows 0, 1: the first burst's right and left half;
//     rows 2, 3: the second burst's); lane s of a row is state s.  Predecessors and successors come across the row by ds_bpermute,
//     the parity minima by the three DPP steps, the received symbol of a step is one LDS broadcast read per row -- mlse_trellis<42>.
//     The 42 forward metrics of a lane stay in 42 VGPRs (both loops fully unrolled, a scheduling fence per step); M_0 - M_1 of step i is kept by lane i % 16 (three registers).
//   * LDS: the staging area and two symbol vectors a wave: k_mlse's.  Listing (gfx950): DESIGN.md 5.4.v and the README.
#define TRX_MLSE_SCH_TAB_QUAL static __device__ __constant__ const
#include "trxsig_mlse_sch_tab.h"
#include "trxsig_mlse_dev.h"                                // mlse_symbols, mlse_ls_tap, mlse_window, mlse_trellis, mlse_soft_out, ...

namespace {

#define TRX_MLSE_SCH_STEPS 42                               /* per half: 39 coded bits and 3 tail bits */
#define TRX_MLSE_SCH_RIGHT0 106                             /* the right half decides symbols 106..147 */
#define TRX_MLSE_SCH_LEFT0 41                               /* the left half decides symbols 41..0 */

template <int SPS>
__global__ __launch_bounds__(64 * TRX_MLSE_WAVES) __attribute__((amdgpu_waves_per_eu(4)))
void k_mlse_sch(const TrxTables *__restrict__ T, const void *__restrict__ samples, const int32_t *__restrict__ offset,
                const int32_t *__restrict__ length, int B, const cx *__restrict__ amp_in, const float *__restrict__ toa_in,
                const uint8_t *__restrict__ flags, int need_mask, cx *__restrict__ chan, int32_t *__restrict__ win,
                float *__restrict__ soft, uint8_t *__restrict__ hard, int nsoft, int stride) {
  typedef DemodGeom<SPS, 148> G;
  static_assert(4 * 44 <= G::U, "the rows' scratch lies in the staging area");
  static_assert(TRX_MLSE_SCH_ROW0 + TRX_MLSE_SCH_NROW <= 148 && TRX_MLSE_SCH_RIGHT0 + TRX_MLSE_SCH_STEPS == 148, "the burst map");
  __shared__ cx ph[TRX_MLSE_WAVES][G::U];
  __shared__ cx ysh[TRX_MLSE_WAVES][2][TRX_MLSE_NY];

  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int bw = 2 * (blockIdx.x * TRX_MLSE_WAVES + wave);   // the wave's first burst (wave-uniform)
  if (bw >= B) return;

  // ---- 1. symbols, a burst at a time on the whole wave.  Two bits a burst in `states`: 0 = equalise, 1 = fall back, 2 = not enabled ----
  int states = 0;
#pragma unroll 1
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
      states |= 2 << (2 * j);
      continue;
    }
    if (mlse_symbols<SPS>(T, ph[wave], samples, off, N, amp, toa, lane, Y)) states |= 1 << (2 * j);
  }
  wave_lds_fence();

  // ---- 2. channel estimate: lanes 0..8 of a row form c[-4..4] = P32 y[46..101]; every lane of the row then reads all nine ----
  const int s = lane & 15;                                  // the state this lane carries
  const int j = lane >> 5;                                  // which of the wave's two bursts
  const bool left = (lane >> 4) & 1;                        // which half of it
  const int b = bw + j;
  const cx *Y = ysh[wave][j];
  cx *scr = ph[wave] + 44 * (lane >> 4);                    // this row's 44 words of the (dead) staging area: c[9], (E, w), state, Z[32] from word 12
  {
    const cx cd = mlse_ls_tap<TRX_MLSE_SCH_NROW>(trx_mlse_sch_p32 + TRX_MLSE_SCH_NROW * (s < 9 ? s : 8), Y, TRX_MLSE_SCH_ROW0);
    if (s < 9) scr[s] = cd;
  }
  wave_lds_fence();
  cx h[5];
  int w;
  const float E = mlse_window(scr, h, w);
  int st = (states >> (2 * j)) & 3;
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
  // (the way back needs Z[2 s], Z[2 s + 1] -- out of state s with b = 0, 1 -- and E and the burst's state are wanted after it: parked in LDS)
  scr[12 + s] = zf0; scr[28 + s] = zf1;
  if (s == 0) { scr[9] = mk(E, __int_as_float(w)); scr[10] = mk(__int_as_float(st), 0.0f); }
  // start state, bit 0 first: a[105], a[104], a[103], a[102] (right) or a[42], a[43], a[44], a[45] (left), from the extended training sequence
  const int start = left ? TRX_MLSE_SCH_START_LEFT : TRX_MLSE_SCH_START_RIGHT;
  // step i = 0..41 is symbol m = 106 + i with sample y[m + w] (right), m = 41 - i with y[m + 4 + w] (left)
  float D[3] = {0.0f, 0.0f, 0.0f};
  mlse_trellis<TRX_MLSE_SCH_STEPS>(Y, left ? TRX_MLSE_SCH_LEFT0 + 4 + w : TRX_MLSE_SCH_RIGHT0 + w, left ? -1 : 1, zf0, zf1, scr, lane, start, D);

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
      const int m = left ? TRX_MLSE_SCH_LEFT0 - i : TRX_MLSE_SCH_RIGHT0 + i;
      if (i < TRX_MLSE_SCH_STEPS && m < nsoft) mlse_soft_out(sb, hb, m, D[q], den);
    }
#pragma unroll
    for (int q = 0; q < 2; q++) {                           // the extended training sequence, 42..105: the demodulator's formula
      const int m = TRX_MLSE_SCH_LEFT0 + 1 + 32 * q + hl;
      if (m < nsoft) mlse_put(sb, hb, m, mlse_slice(Y[m].r));
    }
  } else {
    mlse_fall_back(sb, hb, Y, st_, hl, 32, nsoft);
  }
}

}  // namespace

hipError_t trx_launch_mlse_sch(hipStream_t st, int sps, const TrxTables *dT, const TrxMlseArgs &a) {
  return mlse_launch<2 * TRX_MLSE_WAVES, true>(sps, a, [&](auto S, dim3 grid, dim3 block) {
    k_mlse_sch<decltype(S)::value><<<grid, block, 0, st>>>(dT, a.samples0, a.off0, a.len, a.B, a.amp, a.toa, a.flags, a.need_mask, a.chan, a.win,
                                                           a.soft, a.hard, a.nsoft, a.stride);
  });
}
