// trxsig_l1pacc_dev.h -- internal: what the packet access object's host side (trxsig_l1pacc_host.cpp) and its kernels
// (trxsig_l1pacc.hip) share: the frame rules, the PDCH record, the per-call argument records and the launchers.  The
// 52-multiframe's position arithmetic is trxsig_l1pdch_dev.h's (class 0: the PDTCH blocks B0..B11, which a PRACH block is one of).
#pragma once
#include "trxsig_l1pdch_dev.h"

// PTCCH/U: the frame with FN mod 416 = 12 + 26 n belongs to TAI n; -1 on any other frame (u may be unwrapped: 416 divides the hyperframe)
__host__ __device__ inline int pacc_tai(unsigned u) { return u % 26u == 12u ? (int)((u % 416u) / 26u) : -1; }
// blocks with a frame in [fn, fn + F): the first, and how many (trxsig_l1pdch_decode's rule)
__host__ __device__ inline unsigned pacc_blk0(unsigned fn) { return pd_pos_before(0, fn) >> 2; }
__host__ __device__ inline int pacc_nb(unsigned fn, unsigned F) {
  const unsigned pf = pd_pos_before(0, fn), pe = pd_pos_before(0, fn + F);
  return pe > pf ? (int)(((pe - 1u) >> 2) - (pf >> 2) + 1u) : 0;
}

struct TrxL1paccChan {                           // TRXSIG_L1PACC_STATE_BYTES
  int32_t ta[16], fn[16];
  uint8_t valid[16];
};
static_assert(sizeof(TrxL1paccChan) == 144, "TRXSIG_L1PACC_STATE_BYTES");

struct TrxL1paccEnc {
  int fn, n_frames, n_pdch, nb, fmt, bsic;
  unsigned blk0;
  const int32_t *chinfo;                         // [n_pdch] arfcn | tn << 16
  const uint8_t *ptcch_kind, *prach_kind;
  const uint16_t *ptcch_ra, *prach_ra;
  uint16_t *ra;                                  // per unit (PDCH g, frame k) = g * n_frames + k: the coder's inputs ...
  uint8_t *fmts, *bsics, *ebits;                 // ... (fmts: 255 where nothing is sent) and its [units][148] output
  uint8_t *bits, *what;
};

struct TrxL1paccDet {
  int fn, n_frames, n_pdch, n_occ, sps, bsic;
  const int32_t *occ0;                           // [n_pdch + 1]: PDCH g's occasions are occ0[g] .. occ0[g + 1] - 1, in frame order
  const int32_t *frame;                          // [n_occ] the occasion's frame k within the call
  const uint8_t *okind;                          // [n_occ] 1 PTCCH/U, 2 PRACH
  const uint8_t *flags, *dfmt, *dtail, *dbsic;   // the detector's and the decoder's outputs per occasion
  const uint16_t *dra;
  const trx_c32 *amp;
  const float *toa, *avgpwr;
  TrxL1paccChan *st;
  uint8_t *kind, *det, *fmt, *ok, *ta;           // dense [n_pdch][n_frames]; kind, tai cleared by the host
  int8_t *tai;
  uint16_t *ra;
  trx_c32 *o_amp;
  float *o_toa, *o_avgpwr;
};

hipError_t trx_launch_l1pacc_stage(hipStream_t st, const TrxL1paccEnc &e, TrxProfiler *prof);
hipError_t trx_launch_l1pacc_mux(hipStream_t st, const TrxL1paccEnc &e, TrxProfiler *prof);
hipError_t trx_launch_l1pacc_fold(hipStream_t st, const TrxL1paccDet &d, TrxProfiler *prof);
hipError_t trx_launch_l1pacc_message(hipStream_t st, const TrxL1paccChan *state, int n_pdch, int nb_pt, uint8_t *kind, uint8_t *payload,
                                     TrxProfiler *prof);
hipError_t trx_launch_l1pacc_read(hipStream_t st, int n_pdch, int nb, const uint8_t *payload, const uint8_t *ok, uint8_t *ta,
                                  TrxProfiler *prof);
