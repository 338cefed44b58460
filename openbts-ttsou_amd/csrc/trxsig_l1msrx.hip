// trxsig_l1msrx.hip -- the mobile-side downlink L1's kernels (include/trxsig_l1msrx.h, host side in trxsig_l1msrx.cpp).  The
// routing is trxsig_l1rx.hip's, over the downlink mappings trxsig_l1tx walks.
//
// k_l1msrx_demux: a wave per logical channel, slots across the lanes.  A TCH / XCCH / CCCH / BCCH channel walks its own
//   positions (trxsig_tdma.h): slot s of its grid is position 4 * blk_first + s, whose frame is trx_map_frame(); where that
//   frame lies in the call and the input has a burst for (frame, TN, ARFCN), the slot gets the burst's row.  With the mappings
//   disjoint on a slot (tests/test_l1_msrx_model.py) this routes the bursts a [TN][FN % 5304] table would.  The same pass
//   records the row of the last burst the channel accepted (k_l1rx_demux_phy, trxsig_l1rx.hip, turns it into the RSSI / timing
//   the decoder keeps: burst_phy's double log10 stays in that file), writes the TCH phase b0 and every block's closing FN.
//   Positions and frames are 32-bit here and every division is by a constant (the mappings have 4, 5 or 24 frames).  The SCH channel's
//   wave lists its frames of the call and gathers each burst's 78 coded values for the Viterbi launcher; the FCCH channel's
//   wave lists its frames and counts each burst's soft values above 0.5 with a ballot.
// k_l1msrx_finish: after the decoders -- the SACCH orders folded over the call's good SACCH frames (trx_sacch_fold,
//   trxsig_tdma.h: the header SACCHL1Encoder::sendFrame wrote), a thread per XCCH channel;
//   the SCH verdict (tail, parity, LSB8MSB undone, the fields, the frame number, sync), a thread per list entry; the TC of every
//   BCCH block, a thread per block.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "trxsig_l1msrx_dev.h"
#include "trxsig_sch_dec.h"

namespace {

__constant__ TrxTdmaMap c_dl[TRX_N_DL_MAPS] = TRX_TDMA_DL_MAPS_INIT;
__constant__ int8_t c_power[3][32] = TRX_POWER_TABLES_INIT;

// the soft value as the GSM side sees it after the UDP hop (trxsig_fec.hip's wire_value)
__device__ __forceinline__ float wire_value(float v) {
  const int q = (int)round((double)v * 255.0);
  return (float)(unsigned char)q / 256.0F;
}

// trx_map_frame in 32 bits without a division by a variable: the frame (unwrapped) of position q.  M.n is 4, 5 or 24:
// trxsig_l1msrx_create refuses any other table (maps_ordered, trxsig_l1msrx.cpp)
__device__ __forceinline__ int fdivc(int a, int b) { return a >= 0 ? a / b : -((-a + b - 1) / b); }
__device__ __forceinline__ int dl_frame(const TrxTdmaMap &M, int q) {
  int k;
  switch (M.n) {
    case 4: k = q >> 2; break;
    case 5: k = fdivc(q, 5); break;
    default: k = fdivc(q, 24); break;
  }
  int off = M.f[q - k * M.n] - M.f[0];
  if (off < 0) off += M.R;
  return M.f[0] + k * M.R + off;
}

__global__ __launch_bounds__(256) void k_l1msrx_demux(TrxL1msrxCall c, TrxL1msrxDev d, const int32_t *__restrict__ row,
                                                      const uint8_t *__restrict__ valid, const float *__restrict__ soft) {
  const int lane = threadIdx.x & 63;
  const int ch = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int n_blk = c.n_tch + c.n_ctl;
  if (ch >= n_blk + c.n_sch + c.n_fcch) return;              // whole waves only
  const int info = d.chinfo[ch];
  const int a = info & 0xffff, tn = (info >> 16) & 15, m = info >> 20;
  const TrxTdmaMap &M = c_dl[m];
  auto burst_row = [&](int u) -> int {                        // the input's accepted row for frame u on this slot, or -1
    const int k = u - c.fn;
    if (k < 0 || k >= c.n_frames) return -1;
    const int r = row[(size_t)(8 * k + tn) * c.n_arfcn + a];
    return (r >= 0 && r < c.n_rows && valid[r] != 0) ? r : -1;
  };

  if (ch >= n_blk) {                                          // SCH / FCCH: a dense list, one entry per frame of the mapping
    const bool sch = m == TRX_DL_SCH;
    const int cap = sch ? c.sch_cap : c.fcch_cap;
    const int p0 = c.p_first[m];
    int32_t *fno = sch ? d.sch_fn : d.fcch_fn;
    for (int s0 = 0; s0 < cap; s0 += 64) {
      const int s = s0 + lane;
      int r = -1;
      if (s < cap) {
        const int u = dl_frame(M, p0 + s);
        r = burst_row(u);
        fno[s] = u % kTrxHyperframe;
        if (sch) d.sch_present[s] = r >= 0 ? 1 : 0;
      }
      const int n = cap - s0 < 64 ? cap - s0 : 64;
      for (int j = 0; j < n; j++) {                           // the wave takes the chunk's entries one by one
        const int rs = __shfl(r, j);
        const float *src = soft + (size_t)(rs >= 0 ? rs : 0) * c.soft_stride;
        if (sch) {
          float *e = d.sch_e + (size_t)(s0 + j) * 78;
          for (int k = lane; k < 78; k += 64) e[k] = rs >= 0 ? src[k < 39 ? 3 + k : 106 + (k - 39)] : 0.0F;
        } else {
          int ones = 0;
          for (int k0 = 0; k0 < 148; k0 += 64) {
            const int k = k0 + lane;
            bool one = false;
            if (rs >= 0 && k < 148) {
              float v = src[k];
              if (c.wire) v = wire_value(v);
              one = v > 0.5F;
            }
            ones += __popcll(__ballot(one));
          }
          if (lane == 0) d.fcch_ones[s0 + j] = rs >= 0 ? ones : -1;
        }
      }
    }
    return;
  }

  const bool tch = ch < c.n_tch;
  const int ci = tch ? ch : ch - c.n_tch;
  const int nb = tch ? c.nb_tch : c.nb_ctl, T = 4 * nb;
  int32_t *idx = (tch ? d.tch_index : d.ctl_index) + (size_t)ci * T;
  const int q0 = 4 * c.blk_first[m];
  const bool act = d.active[ch] != 0;
  int last = -1;
  for (int s0 = 0; s0 < T; s0 += 64) {
    const int s = s0 + lane;
    int r = -1;
    if (s < T) {
      if (act) r = burst_row(dl_frame(M, q0 + s));
      idx[s] = r;
    }
    const unsigned long long bal = __ballot(r >= 0);
    if (bal) last = __shfl(r, 63 - __clzll((long long)bal));
  }
  if (lane == 0) d.last[ch] = last;
  if (tch && lane == 0) d.tch_b0[ci] = (uint8_t)(q0 & 7);
  int32_t *fno = (tch ? d.tch_fn : d.ctl_fn) + (size_t)ci * nb;
  for (int b = lane; b < nb; b += 64) fno[b] = dl_frame(M, q0 + 4 * b + 3) % kTrxHyperframe;
}

__global__ __launch_bounds__(256) void k_l1msrx_finish(TrxL1msrxCall c, TrxL1msrxDev d) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < c.n_xcch) {                                         // the XCCH channels come first in the control grid
    const int m = d.chinfo[c.n_tch + i] >> 20;
    if (trx_map_is_sacch(m)) trx_sacch_fold(d.ctl_status, d.ctl_frames, c.nb_ctl, i, c_power[c.band], d.ord_power, d.ord_ta);
  }
  if (i < c.sch_cap) {
    unsigned ok = 0, bsic = 0, sync = 0;
    int rfn = 0;
    if (d.sch_present[i]) {
      const uint8_t *u = d.sch_u + (size_t)i * 39;
      trx_sch_verdict([&](int q) -> unsigned { return u[q]; }, &ok, &bsic, &rfn);   // trxsig_sch_dec.h
      sync = (ok && rfn == d.sch_fn[i] && bsic == (unsigned)c.bsic) ? 1u : 0u;
    }
    d.sch_ok[i] = (uint8_t)ok; d.sch_bsic[i] = (uint8_t)bsic; d.sch_sync[i] = (uint8_t)sync; d.sch_rfn[i] = rfn;
  }
  if (i < c.nb_ctl)                                           // TC of the block's first burst (BCCHL1Encoder::generate)
    for (int ci = 0; ci < c.n_bcch; ci++) {
      const int m = d.chinfo[c.n_tch + c.n_xcch + c.n_ccch + ci] >> 20;
      int u = dl_frame(c_dl[m], 4 * c.blk_first[m] + 4 * i) % kTrxHyperframe;
      if (u < 0) u += kTrxHyperframe;
      d.bcch_tc[(size_t)ci * c.nb_ctl + i] = (u / 51) % 8;
    }
}

}  // namespace

hipError_t trx_launch_l1msrx_demux(hipStream_t st, const TrxL1msrxCall &call, const TrxL1msrxDev &dv, const int32_t *row,
                                   const uint8_t *valid, const float *soft) {
  const int n = call.n_tch + call.n_ctl + call.n_sch + call.n_fcch;
  if (n <= 0) return hipSuccess;
  k_l1msrx_demux<<<dim3((n + 3) / 4), dim3(256), 0, st>>>(call, dv, row, valid, soft);
  return hipGetLastError();
}

hipError_t trx_launch_l1msrx_finish(hipStream_t st, const TrxL1msrxCall &call, const TrxL1msrxDev &dv) {
  int n = call.n_xcch > call.sch_cap ? call.n_xcch : call.sch_cap;
  if (call.n_bcch && call.nb_ctl > n) n = call.nb_ctl;
  if (n <= 0) return hipSuccess;
  k_l1msrx_finish<<<dim3((n + 255) / 256), dim3(256), 0, st>>>(call, dv);
  return hipGetLastError();
}
