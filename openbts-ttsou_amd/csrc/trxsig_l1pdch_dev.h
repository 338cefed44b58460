// trxsig_l1pdch_dev.h -- internal: what the packet data channel object's host side (trxsig_l1pdch.cpp) and its kernels
// (trxsig_l1pdch.hip) share: the 52-multiframe's position arithmetic, the channel record, the per-call argument records and the
// launchers.  Positions: a channel's burst frames counted from frame 0; block = position / 4, burst = position % 4.  Frame
// numbers here are unwrapped (fn + k may pass the hyperframe, which 52 and 104 divide), so all of it is unsigned 32-bit
// arithmetic with division by constants only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "trxsig_launch.h"

constexpr unsigned kPdHyper = 2715648u;
constexpr int kPdRing = 32;                                    // TRXSIG_L1PDCH_RING; divides 12 * 52224

// positions of class cls (0 PDTCH, 1 PTCCH) on frames below u
__host__ __device__ inline unsigned pd_pos_before(int cls, unsigned u) {
  if (cls == 0) { const unsigned r = u % 52u; return 48u * (u / 52u) + r - r / 13u; }
  return 4u * (u / 104u) + (u % 104u + 13u) / 26u;
}
// whether frame u carries a burst of the class
__host__ __device__ inline bool pd_owns(int cls, unsigned u) { return cls == 0 ? (u % 52u) % 13u != 12u : u % 26u == 12u; }
// the frame of position q
__host__ __device__ inline unsigned pd_frame(int cls, unsigned q) {
  if (cls == 0) { const unsigned p = q % 48u; return 52u * (q / 48u) + p + p / 12u; }
  return 104u * (q / 4u) + 12u + 26u * (q % 4u);
}
// absolute number of block blk (below twice the wrap)
__host__ __device__ inline int pd_abs(int cls, unsigned blk) {
  const unsigned wrap = cls == 0 ? 12u * 52224u : 26112u;   // 32 = kPdRing divides the first
  return (int)(blk >= wrap ? blk - wrap : blk);
}

// a channel's record (TRXSIG_L1PDCH_STATE_BYTES).  Transmit: the block whose bursts are not all out yet (all four bursts, the
// sent ones too, so that the record does not depend on where calls were cut) and the USF ring, entry = block << 8 | usf or -1.
// Receive: the soft rows of the block that has not closed yet.  What is not in use is zero (pend_blk / carry_blk: -1).
struct TrxL1pdchChan {
  int32_t pend_blk, carry_blk;
  uint32_t carry_have;
  int32_t pad;
  uint8_t bits[4][148];
  int32_t ring[kPdRing];
  float carry[4][148];
};
static_assert(sizeof(TrxL1pdchChan) == 3104, "TRXSIG_L1PDCH_STATE_BYTES");

struct TrxL1pdchEnc {
  int fn, n_frames, n_pd, n_pt, down, tsc;
  unsigned p_first[2], p_end[2];                 // positions below fn / below fn + n_frames
  unsigned bf[2];                                // the first block that starts in the call
  int nb[2], unit0[2];
  const int32_t *chinfo;                         // [n_pd + n_pt] arfcn | tn << 16
  TrxL1pdchChan *st;
  const uint8_t *kind[2], *cs, *payload[2];
  uint8_t *stage, *cs_eff, *tscs, *ebits;        // [U][54], [U], [U], [U][4][148]
  uint8_t *bits, *what;
};

struct TrxL1pdchDec {
  int fn, n_frames, n_arfcn, n_pd, n_pt, n_rows;
  long long soft_stride;
  unsigned p_first[2], p_end[2];
  unsigned blk0[2];                              // the first block with a burst frame in the call
  int nb[2], nclose[2], unit0[2];                // blocks shown / closing per channel; the class's first closing unit
  const int32_t *chinfo;
  TrxL1pdchChan *st;
  const TrxL1pdchChan *sib;                      // the sibling's PDTCH records or null
  const int32_t *row;
  const uint8_t *valid;
  const float *soft;
  float *rows;                                   // [Uc][4][148]
  int32_t *index;                                // [Uc][4]
  uint8_t *t_payload, *t_cs, *t_dist, *t_ok, *t_usf;   // the decoder's outputs per closing unit
  uint8_t *payload[2], *cs[2], *dist[2], *ok[2], *usf[2], *nbur[2], *granted[2];
  int32_t *bfn[2], *last;                        // closing FN; [n_pd + n_pt] the last accepted row or -1
};

hipError_t trx_launch_l1pdch_stage(hipStream_t st, const TrxL1pdchEnc &e, TrxProfiler *prof);
hipError_t trx_launch_l1pdch_mux(hipStream_t st, const TrxL1pdchEnc &e, TrxProfiler *prof);
hipError_t trx_launch_l1pdch_demux(hipStream_t st, const TrxL1pdchDec &d, TrxProfiler *prof);
hipError_t trx_launch_l1pdch_fold(hipStream_t st, const TrxL1pdchDec &d, TrxProfiler *prof);
