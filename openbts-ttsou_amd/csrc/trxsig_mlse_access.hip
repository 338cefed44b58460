// trxsig_mlse_access.hip -- the sequence equaliser for access bursts (trxsig_mlse_access_batch, trxsig_mlse_rach_batch; the
// Transceiver group's TRXSIG_RACHLEG_MLSE): a nine-tap least-squares channel estimate from the burst's 49 known leading symbols and
// ONE 16-state max-log-MAP trellis of 39 steps over the 36 coded bits and the 3 tail bits, at any sps.  The reference has no
// counterpart; the stage is pinned by the float32 model tests/mlse_access_model.py, which this kernel equals word for word, and
// graded against the float64 statement tests/mlse_access_ref.py.  The arithmetic rules are k_mlse's (trxsig_mlse.hip): float add,
// subtract, multiply, minimum, compare and one correctly rounded division per soft bit; nothing is fused.  The algorithm is stated
// in include/trxsig.h (trxsig_mlse_access_batch) and again, operation by operation, in the model.
//
// Layout.  One wave takes FOUR bursts.
//   * Symbols (mlse_symbols, trxsig_mlse_dev.h): the whole wave computes one burst at a time with k_demod's own code and keeps the
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
//     broadcast read per row -- mlse_trellis<39> of trxsig_mlse_dev.h.  The 39 forward metrics of a lane stay in 39 VGPRs (both loops
//     fully unrolled, a scheduling fence per step); M_0 - M_1 of step i is kept by lane i % 16 (three registers).
//   * LDS: the staging area and four symbol vectors a wave.  Listing (gfx950): DESIGN.md 5.4.w and the README.
#define TRX_MLSE_ACCESS_TAB_QUAL static __device__ __constant__ const
#include "trxsig_mlse_access_tab.h"
#include "trxsig_mlse_dev.h"                                // mlse_symbols, mlse_ls_tap, mlse_window, mlse_trellis, mlse_soft_out, ...

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

  // ---- 2. channel estimate: lanes 0..8 of a row form c[-4..4] = P32 y[4..44]; every lane of the row then reads all nine ----
  const int s = lane & 15;                                  // the state this lane carries
  const int j = lane >> 4;                                  // which of the wave's four bursts
  const int b = bw + j;
  const cx *Y = ysh[wave][j];
  cx *scr = ph[wave] + 44 * j;                              // this row's 44 words of the (dead) staging area: c[9], (E, w), state, Z[32] from word 12
  {
    const cx cd = mlse_ls_tap<TRX_MLSE_ACCESS_NROW>(trx_mlse_access_p32 + TRX_MLSE_ACCESS_NROW * (s < 9 ? s : 8), Y, 4);
    if (s < 9) scr[s] = cd;
  }
  wave_lds_fence();
  cx h[5];
  int w;
  const float E = mlse_window(scr, h, w);
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
  float D[3] = {0.0f, 0.0f, 0.0f};
  mlse_trellis<TRX_MLSE_ACC_STEPS>(Y, TRX_MLSE_ACC_FIRST + w, 1, zf0, zf1, scr, lane, TRX_MLSE_ACC_START, D);

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
      if (i < TRX_MLSE_ACC_STEPS && m < nsoft) mlse_soft_out(sb, hb, m, D[q], den);
    }
    for (int m = s; m < nsoft; m += 16) {                  // the known head and the guard-side rest: the demodulator's formula
      if (m >= TRX_MLSE_ACC_FIRST && m < TRX_MLSE_ACC_FIRST + TRX_MLSE_ACC_STEPS) continue;
      mlse_put(sb, hb, m, mlse_slice(Y[m].r));
    }
  } else {
    mlse_fall_back(sb, hb, Y, st_, s, 16, nsoft);
  }
}

}  // namespace

hipError_t trx_launch_mlse_access(hipStream_t st, int sps, const TrxTables *dT, const TrxMlseArgs &a) {
  return mlse_launch<4 * TRX_MLSE_WAVES, true>(sps, a, [&](auto S, dim3 grid, dim3 block) {
    k_mlse_access<decltype(S)::value><<<grid, block, 0, st>>>(dT, a.samples0, a.off0, a.len, a.B, a.amp, a.toa, a.flags, a.need_mask, a.chan, a.win,
                                                              a.soft, a.hard, a.nsoft, a.stride);
  });
}
