// trxsig_l1rx.hip -- the uplink L1 demultiplexer's kernels (include/trxsig_l1rx.h, host side in trxsig_l1rx.cpp).
//
// k_l1rx_demux: a wave per logical channel.  Instead of looking every burst up in mDemuxTable[TN][FN % 5304] (TRXManager.cpp:
//   146-168, 474-490), each channel walks its own positions (trxsig_tdma.h): slot s of its grid is position 4 * blk_first + s,
//   whose frame is trx_map_frame(); where that frame lies in the call and the pull returned a burst for (frame, TN, ARFCN), the
//   slot gets the burst's row.  With the mappings disjoint on a slot (tests/test_l1_demux_model.py) both directions route the
//   same bursts.  The same pass keeps the last accepted burst's RSSI / timing (processBurst's mRSSI / mTimingError), writes the
//   TCH phase b0 and every block's closing FN, and, on the RACH channel, lists the detected access bursts in FN order and
//   gathers their soft rows for the RACH decoder.
// k_l1rx_finish: after the decoders -- SACCHL1Decoder::handleGoodFrame's power / TA fold (trx_sacch_fold, trxsig_tdma.h), a thread
//   per XCCH channel, and the RACH verdict ok = tail_ok && BSIC == the cell's (RACHL1Decoder::writeLowSide), a thread per list
//   entry.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "trxsig_l1_phy.h"
#include "trxsig_launch.h"
#include "trxsig_tdma.h"

namespace {

__constant__ TrxTdmaMap c_maps[TRX_N_MAPS] = TRX_TDMA_MAPS_INIT;
__constant__ int8_t c_power[3][32] = TRX_POWER_TABLES_INIT;

__global__ __launch_bounds__(256) void k_l1rx_demux(TrxL1rxCall c, TrxL1rxDev d, const int32_t *__restrict__ row,
                                                    const uint8_t *__restrict__ valid, const float *__restrict__ soft,
                                                    const trx_c32 *__restrict__ amp, const float *__restrict__ toa) {
  const int lane = threadIdx.x & 63;
  const int ch = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (ch >= c.n_tch + c.n_xcch + c.n_rach) return;
  const int info = d.chinfo[ch];
  const int a = info & 0xffff, tn = (info >> 16) & 15, m = info >> 20;
  const TrxTdmaMap &M = c_maps[m];
  const long long F = c.n_frames;
  auto burst_row = [&](long long u) -> int {                  // the pull's accepted row for frame u on this slot, or -1
    const long long k = u - c.fn;
    if (k < 0 || k >= F) return -1;
    const int r = row[(8 * k + tn) * c.n_arfcn + a];
    return (r >= 0 && r < c.n_rows && valid[r] != 0) ? r : -1;
  };

  if (ch >= c.n_tch + c.n_xcch) {                             // the RACH: list the detected bursts of its frames, in FN order
    const long long p0 = c.p_first[m];
    int count = 0;
    for (int s0 = 0; s0 < c.rach_cap; s0 += 64) {
      const int s = s0 + lane;
      long long u = 0;
      int r = -1;
      if (s < c.rach_cap) { u = trx_map_frame(M, p0 + s); r = burst_row(u); }
      const unsigned long long bal = __ballot(r >= 0);
      const int j = count + __popcll(bal & ((1ull << lane) - 1));
      if (r >= 0) {
        d.rach_fn[j] = (int32_t)(u % kTrxHyperframe);
        d.rach_arfcn[j] = a;
        burst_phy(amp, toa, r, c.sps, &d.rach_rssi[j], &d.rach_timing[j]);
      }
      for (unsigned long long b = bal; b; b &= b - 1) {       // the wave copies each listed row
        const int src_lane = __ffsll((long long)b) - 1;
        const int rs = __shfl(r, src_lane);
        const int js = count + __popcll(bal & ((1ull << src_lane) - 1));
        for (int e = lane; e < 148; e += 64) d.rach_soft[(size_t)js * 148 + e] = soft[(size_t)rs * c.soft_stride + e];
      }
      count += __popcll(bal);
    }
    if (lane == 0) *d.rach_count = count;
    return;
  }

  const bool tch = ch < c.n_tch;
  const int ci = tch ? ch : ch - c.n_tch;
  const int nb = tch ? c.nb_tch : c.nb_xcch, T = 4 * nb;
  int32_t *idx = (tch ? d.tch_index : d.xcch_index) + (size_t)ci * T;
  const long long q0 = 4LL * c.blk_first[m];
  const bool act = d.active[ch] != 0;
  int last = -1;
  unsigned n_acc = 0;
  for (int s0 = 0; s0 < T; s0 += 64) {
    const int s = s0 + lane;
    int r = -1;
    if (s < T) {
      if (act) r = burst_row(trx_map_frame(M, q0 + s));
      idx[s] = r;
    }
    const unsigned long long bal = __ballot(r >= 0);
    n_acc += (unsigned)__popcll(bal);
    if (bal) last = __shfl(r, 63 - __clzll((long long)bal));
  }
  if (lane == 0 && last >= 0) burst_phy(amp, toa, last, c.sps, &d.rssi[ch], &d.timing[ch]);
  if (lane == 0 && n_acc) d.accepted[ch] += n_acc;
  if (tch && lane == 0) d.tch_b0[ci] = (uint8_t)(((q0 % 8) + 8) % 8);
  int32_t *fno = (tch ? d.tch_fn : d.xcch_fn) + (size_t)ci * nb;
  for (int b = lane; b < nb; b += 64) fno[b] = (int32_t)(trx_map_frame(M, q0 + 4LL * b + 3) % kTrxHyperframe);
}

__global__ __launch_bounds__(256) void k_l1rx_finish(TrxL1rxCall c, TrxL1rxDev d) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < c.n_xcch) {
    const int m = d.chinfo[c.n_tch + i] >> 20;
    if (trx_map_is_sacch(m)) trx_sacch_fold(d.xcch_status, d.xcch_frames, c.nb_xcch, i, c_power[c.band], d.ms_power, d.ms_ta);
  }
  if (i < c.rach_cap) {
    const bool ok = i < *d.rach_count && d.rach_tail[i] != 0 && d.rach_bsic[i] == d.bsic;
    d.rach_ok[i] = ok ? 1 : 0;
    if (!ok) d.rach_ra[i] = 0;
  }
}

// burst_phy for a list of rows, a lane per channel: last[ch] is the row of the last burst channel ch accepted in the call, or
// -1 (its RSSI / timing stay).  The handsets' demultiplexer (trxsig_l1msrx.hip) records the rows and leaves the arithmetic here,
// beside k_l1rx_demux's: the device library's double log10 stays in this file's kernels (tests/test_no_fma_contraction.py).
__global__ __launch_bounds__(256) void k_l1rx_demux_phy(const int32_t *__restrict__ last, int n, const trx_c32 *__restrict__ amp,
                                                        const float *__restrict__ toa, int sps, int32_t *rssi, int32_t *timing) {
  const int ch = blockIdx.x * blockDim.x + threadIdx.x;
  if (ch >= n) return;
  const int r = last[ch];
  if (r >= 0) burst_phy(amp, toa, r, sps, &rssi[ch], &timing[ch]);
}

__global__ void k_l1rx_set(uint8_t *active, int ch, int open, uint8_t *state_fer, int32_t *ms_power, int32_t *ms_ta, int sacch) {
  if (threadIdx.x != 0) return;
  active[ch] = open ? 1 : 0;
  if (!open) return;
  *reinterpret_cast<float *>(state_fer) = 0.0f;              // mFER = 0; mI kept
  if (sacch) { *ms_power = 40; *ms_ta = 0; }
}

}  // namespace

hipError_t trx_launch_l1rx_demux(hipStream_t st, const TrxL1rxCall &call, const TrxL1rxDev &dv, const int32_t *row,
                                 const uint8_t *valid, const float *soft, const trx_c32 *amp, const float *toa, TrxProfiler *prof) {
  const int n = call.n_tch + call.n_xcch + call.n_rach;
  if (n <= 0) return hipSuccess;
  if (prof) prof->begin(TRXSIG_K_L1RX_DEMUX, st);
  k_l1rx_demux<<<dim3((n + 3) / 4), dim3(256), 0, st>>>(call, dv, row, valid, soft, amp, toa);
  if (prof) prof->end(TRXSIG_K_L1RX_DEMUX, st);
  return hipGetLastError();
}

hipError_t trx_launch_l1rx_finish(hipStream_t st, const TrxL1rxCall &call, const TrxL1rxDev &dv, TrxProfiler *prof) {
  const int n = call.n_xcch > call.rach_cap ? call.n_xcch : call.rach_cap;
  if (n <= 0) return hipSuccess;
  if (prof) prof->begin(TRXSIG_K_L1RX_FINISH, st);
  k_l1rx_finish<<<dim3((n + 255) / 256), dim3(256), 0, st>>>(call, dv);
  if (prof) prof->end(TRXSIG_K_L1RX_FINISH, st);
  return hipGetLastError();
}

hipError_t trx_launch_l1rx_phy(hipStream_t st, const int32_t *last, int n, const trx_c32 *amp, const float *toa, int sps,
                               int32_t *rssi, int32_t *timing) {
  if (n <= 0) return hipSuccess;
  k_l1rx_demux_phy<<<dim3((n + 255) / 256), dim3(256), 0, st>>>(last, n, amp, toa, sps, rssi, timing);
  return hipGetLastError();
}

hipError_t trx_launch_l1rx_set(hipStream_t st, uint8_t *active, int ch, int open, uint8_t *state_fer, int32_t *ms_power,
                               int32_t *ms_ta, int sacch) {
  k_l1rx_set<<<dim3(1), dim3(64), 0, st>>>(active, ch, open, state_fer, ms_power, ms_ta, sacch);
  return hipGetLastError();
}
