// trxsig_l1trk_dev.h -- internal: what the tracking receiver (include/trxsig_l1trk.h) shares between its host side
// (trxsig_l1trk.cpp) and its kernels (trxsig_l1trk.hip).
#pragma once
#include "trxsig_l1trk.h"
#include "trxsig_launch.h"

// the per-phone state on the device.  The anchor (fn, pos, phase) exists twice: a slice reads one set and writes the other, so
// no workgroup of the launch can read what another has already advanced.
struct TrxTrkState {
  int32_t *fn[2];
  long long *pos[2];
  uint32_t *phase[2];
  uint32_t *step;
  uint8_t *locked;
  int32_t *quiet;
  long long *toa_sum, *adj, *afc_delta;      // what the last update did
  int32_t *toa_n, *afc_n;
};
// the plan (device copies of what create was given) and a slice's records
struct TrxTrkPlan {
  int n_phones, n_cols;
  const int32_t *phone;                      // [n_cols]
  const int32_t *c0;                         // [n_phones], -1: none
  const int32_t *col_start;                  // [n_phones + 1]: phone p's columns are col_list[col_start[p] .. col_start[p + 1])
  const int32_t *col_list;                   // [n_cols]
};
struct TrxTrkMeas {
  uint8_t *status;                           // [n_cols]
  int32_t *fcch_fn;                          // [n_phones][cap]
  double *fcch_c, *fcch_e;                   // [n_phones][cap][2], [n_phones][cap]
  uint8_t *fcch_ok;
  int cap;
};

struct TrxTrkSlice {
  const trx_c32 *streams; long long stream_stride, n0; int n_samples;
  int fn, n_frames;
  trx_c32 *cells; long long slot_stride, col_stride;
  int cur;                                   // the anchor set that is read; cur ^ 1 is written
  float fcch_thresh;
};
// FCCH frames among the x frames that follow a frame with FN % 51 == 0: FN % 51 in {0, 10, 20, 30, 40}
static inline __host__ __device__ unsigned trx_trk_fcch_before(unsigned x) {
  const unsigned r = x % 51u, k = (r + 9u) / 10u;
  return (x / 51u) * 5u + (k < 5u ? k : 5u);
}

hipError_t trx_launch_l1trk_seed(hipStream_t st, int sps, const TrxTrkPlan &plan, const TrxTrkState &s, int cur, int n_streams,
                                 const uint8_t *acq_state, const int32_t *w0, const float *toa, const float *omega, const int32_t *rfn,
                                 const int32_t *src);
hipError_t trx_launch_l1trk_set(hipStream_t st, const TrxTrkState &s, int cur, int phone, int locked, int fn, long long pos,
                                uint32_t step, uint32_t phase);
hipError_t trx_launch_l1trk_slice(hipStream_t st, int sps, const TrxTables *dT, const TrxTrkPlan &plan, const TrxTrkState &s,
                                  const TrxTrkMeas &m, const TrxTrkSlice &p);
// the update behind the pull of the last slice's cells: fn / n_slots / n_fcch are that slice's, cur the anchor set it wrote
hipError_t trx_launch_l1trk_update(hipStream_t st, int sps, const TrxTrkPlan &plan, const TrxTrkState &s, const TrxTrkMeas &m, int cur,
                                   int fn, int n_slots, int n_rows, int n_fcch, const int32_t *row, const uint8_t *valid, const float *toa,
                                   const uint8_t *use, int afc_shift, int toa_gate);
