// trxsig_txstage.h -- the fused transmit back end's staging of modulated samples (shared by k_resample<RES_IN_BITS> in
// trxsig_tx.hip and the wideband synthesiser k_tx_wideband in trxsig_txwb.hip).
#pragma once
#include "trxsig_dev.h"

namespace {

// Window samples [lo, hi] that bursts cover, computed from the bursts' bits: burst by burst, a thread per symbol period.
// Sample t = SPS u + r of a burst is modulateBurst's sum over j ascending of a[t + SPS - j] p[j] where only j = r, r + SPS
// (and r + 2 SPS for r = 0) meet a non-zero a[n] = rot[n] * (2 bit - 1), n = SPS (u + 1 - q) (k_modulate's arithmetic): the
// three symbols u + 1, u, u - 1 serve the period's SPS samples.
template <int SPS>
__device__ __forceinline__ void tx_stage_tile(const TrxTables *__restrict__ T, const uint8_t *__restrict__ ring, const float *__restrict__ gring,
                                              const int *tb_start, const int *tb_meta, int M, int lo, int hi, cx *X) {
  float pul[2 * SPS + 1];
#pragma unroll
  for (int j = 0; j < 2 * SPS + 1; j++) pul[j] = T->pulse[j];
  for (int m = 0; m < M; m++) {                            // (uniform: every thread walks the tile's bursts)
    const int start = tb_start[m];
    if (start > hi) break;
    const int meta = tb_meta[m], slot = meta & 0xffff, guard = (meta >> 16) & 0xf;
    const bool scale = (meta >> 20) & 1;
    const int nsym = 148 + guard;
    if (start + SPS * nsym <= lo) continue;
    const float gv = scale ? gring[slot] : 1.0f;
    const uint8_t *bits = ring + (size_t)slot * 148;
    const int u0 = start < lo ? (lo - start) / SPS : 0;
    const int u1 = (hi - start) / SPS < nsym - 1 ? (hi - start) / SPS : nsym - 1;
    for (int u = u0 + (int)threadIdx.x; u <= u1; u += 256) {
      cx av[3];                                            // a[SPS (u + 1 - q)], q = 0, 1, 2; valid: the symbol exists
      bool ok[3];
#pragma unroll
      for (int q = 0; q < 3; q++) {
        const int k = u + 1 - q;
        ok[q] = k >= 0 && k < 148;
        const int kc = ok[q] ? k : 0;
        const float sym = (float)(2.0 * (bits[kc] & 0x01) - 1.0);
        av[q] = cmulr(T->rot[SPS * kc], sym);              // GMSKRotate, realOnly (:235-239)
      }
#pragma unroll
      for (int r = 0; r < SPS; r++) {
        const int i = start + SPS * u + r;
        cx sum = mk(0, 0);
        if (ok[0]) sum = cadd(sum, cmulr(av[0], pul[r]));              // j = r
        if (ok[1]) sum = cadd(sum, cmulr(av[1], pul[r + SPS]));        // j = r + SPS   (convolve, b real: :345-353)
        if (r == 0 && ok[2]) sum = cadd(sum, cmulr(av[2], pul[2 * SPS]));   // j = 2 SPS
        if (scale) sum = cmul(sum, mk(gv, 0.0f));                      // scaleVector(x, complex(g)) (:719-722)
        if (i >= lo && i <= hi) X[i - lo] = sum;
      }
    }
  }
}

}  // namespace
