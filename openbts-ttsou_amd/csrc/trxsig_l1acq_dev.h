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
// state[s] |= TRXSIG_ACQ_DECODED where ok[s]
hipError_t trx_launch_l1acq_finish(hipStream_t st, int n_streams, const uint8_t *ok, uint8_t *state);
