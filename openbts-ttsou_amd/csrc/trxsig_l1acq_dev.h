// trxsig_l1acq_dev.h -- internal: what the acquisition object (include/trxsig_l1acq.h) shares between its host side
// (trxsig_l1acq.cpp) and its kernels (trxsig_l1acq.hip).
#pragma once
#include "trxsig_l1acq.h"
#include "trxsig_launch.h"

#define TRX_ACQ_WMAX (TRXSIG_L1ACQ_MAX_WINDOW * TRX_MAXSPS)   // workspace row of one stage-2 window, in samples (any sps)
#define TRX_ACQ_FCCH_SYMS 142                                  // the FCCH window and the scan segments, in symbols
#define TRX_ACQ_TILE_SYMS 1136                                 // window starts per stage-1 workgroup: 8 / sps segments

// stage 1, first launch: per (stream, tile) the largest metric and its smallest window start, with C and E there.
// A tile is TRX_ACQ_TILE_SYMS window starts at any sps (8 / sps segments of 142 sps samples); trx_acq_tiles: the tiles that
// hold the window starts 0 .. n_samples - sps - L of a stream, 0 where it has none
int trx_acq_tiles(int sps, int n_samples);
hipError_t trx_launch_l1acq_fcch(hipStream_t st, int sps, const trx_c32 *samples, long long stride, int n_samples, int n_streams,
                                 int n_tiles, float *tile_m, int32_t *tile_k, trx_c32 *tile_c, float *tile_e);

// the per-stream arrays of a search (device)
struct TrxAcqStreams {
  uint8_t *state;
  int32_t *fcch_k;
  float *fcch_m;
  trx_c32 *fcch_c;
  float *fcch_e, *arg, *omega;
  int32_t *w0;
  long long *base;                   // the SCH window's first sample in d_samples
  int32_t *wlen;                     // its length, 0: stage 2 does not run
};
// stage 1, second launch: each stream's winner by the smallest-k rule, the angle, and the set-up of stage 2
hipError_t trx_launch_l1acq_pick(hipStream_t st, int sps, long long stride, int n_samples, int n_streams, int n_tiles,
                                 const float *tile_m, const int32_t *tile_k, const trx_c32 *tile_c, const float *tile_e,
                                 float fcch_thresh, TrxAcqStreams s);

// stage 2.  Window b: samples + base64[b] (a search) or samples + off32[b] (a batch), len[b] samples; omega may be null (no
// shift).  y: [B][TRX_ACQ_WMAX] receives the shifted windows; woff[b] = b * TRX_ACQ_WMAX; wlen[b] = len[b], or 0 for a window
// that is not processed (negative offset, a length outside (0, TRXSIG_L1ACQ_MAX_WINDOW * sps]).
hipError_t trx_launch_l1acq_shift(hipStream_t st, int sps, const TrxTables *dT, const trx_c32 *samples, const long long *base64,
                                  const int32_t *off32, const int32_t *len, const float *omega, int B, trx_c32 *y, int32_t *woff,
                                  int32_t *wlen);
// the tail of the detector on the correlations c [B][TRX_ACQ_WMAX] and peakDetect's (peak, index): the bogus rule, the valley,
// ptm / amp / toa, the verdict, and the demodulator's segment (doff / dlen / dtoa, into y).  search != 0: a window of length 0
// is one stage 2 did not run for (flags 0), and state[b] gains TRXSIG_ACQ_SCH on detection; else it gets TRXSIG_F_BADLEN.
hipError_t trx_launch_l1acq_verdict(hipStream_t st, int sps, const trx_c32 *c, const int32_t *wlen, const trx_c32 *peak,
                                    const float *pidx, int B, trx_c32 gain, float seq_toa, float thresh, int search, uint8_t *flags,
                                    trx_c32 *amp, float *toa, float *ptm, int32_t *doff, int32_t *dlen, float *dtoa, uint8_t *state);
// TRXSIG_SCHDET_FIT, in k_l1acq_verdict's place.  First the candidates, before the fit: no valley; amp = peak / gain where the TOA
// lies inside the window (0 elsewhere), toa as the verdict kernel reports it, the demodulator's segment and flags = TRXSIG_F_DETECT
// for a window that passes the geometry gate (0 <= toa <= n, amp finite and nonzero, floor(toa_b) >= 0, the burst inside).
hipError_t trx_launch_l1acq_candidates(hipStream_t st, int sps, const int32_t *wlen, const trx_c32 *peak, const float *pidx, int B,
                                       trx_c32 gain, float seq_toa, int search, uint8_t *flags, trx_c32 *amp, float *toa, int32_t *doff,
                                       int32_t *dlen, float *dtoa);
// ... then, behind k_sch_fit on the candidates: a candidate keeps TRXSIG_F_DETECT iff q > thresh; ptm (may be null) reports q;
// state[b] (search) gains TRXSIG_ACQ_SCH on detection
hipError_t trx_launch_l1acq_fit_verdict(hipStream_t st, int B, const float *q, float thresh, uint8_t *flags, float *ptm, uint8_t *state);
// state[s] |= TRXSIG_ACQ_DECODED where ok[s]
hipError_t trx_launch_l1acq_finish(hipStream_t st, int n_streams, const uint8_t *ok, uint8_t *state);

// device code shared by trxsig_l1acq.hip (k_l1acq_pick) and trxsig_l1trk.hip (k_l1trk_update)
namespace {

// atan2(y, x) in plain float32 multiplies, adds and divisions: lo / hi in [0, 1]; above tan(pi / 8) the identity
// atan t = pi / 4 + atan((t - 1) / (t + 1)) brings |t| below 0.4143, where the odd series to t^17 is within 3e-9; the octant
// is undone by reflections.  Within a few float32 steps at pi of the true angle (the tests allow 2e-6).
__device__ __forceinline__ float acq_atan2(float y, float x) {
  const float ax = fabsf(x), ay = fabsf(y);
  const float hi = ax > ay ? ax : ay, lo = ax > ay ? ay : ax;
  if (!(hi > 0.0f)) return 0.0f;
  float t = lo / hi, off = 0.0f;
  if (t > 0.41421356f) { t = (t - 1.0f) / (t + 1.0f); off = 0.78539816f; }
  const float z = t * t;
  float p = 1.0f / 17.0f;
  p = p * z - 1.0f / 15.0f;
  p = p * z + 1.0f / 13.0f;
  p = p * z - 1.0f / 11.0f;
  p = p * z + 1.0f / 9.0f;
  p = p * z - 1.0f / 7.0f;
  p = p * z + 1.0f / 5.0f;
  p = p * z - 1.0f / 3.0f;
  p = p * z + 1.0f;
  float r = off + t * p;
  if (ay > ax) r = 1.57079633f - r;
  if (x < 0.0f) r = 3.14159265f - r;
  return y < 0.0f ? -r : r;
}

}  // namespace
