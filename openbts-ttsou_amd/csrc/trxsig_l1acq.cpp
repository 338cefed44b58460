// trxsig_l1acq.cpp -- the acquisition object's host side (include/trxsig_l1acq.h): the SCH correlation sequence built once with
// the table generator's restatements, the per-stream arrays and the stage-2 workspace on the device, and per call the launches
// on the context's stream: k_l1acq_fcch, k_l1acq_pick, k_l1acq_shift, the correlation over every lag and peakDetect
// (trxsig_prim.hip), k_l1acq_verdict, the exact demodulator -- or, on TRXSIG_SCHLEG_MLSE, the synchronisation burst's sequence
// equaliser (trxsig_mlse_sch.hip) in its place --, the SCH decode (k_fec_viterbi's SCH mode), k_l1acq_finish.  On
// TRXSIG_SCHDET_FIT k_l1acq_candidates, k_sch_fit (trxsig_sch_fit.hip) and k_l1acq_fit_verdict stand in k_l1acq_verdict's place.
#include <hip/hip_runtime_api.h>

#include <cstring>
#include <memory>
#include <new>
#include <vector>

#include "trxsig_ctx.h"
#include "trxsig_l1acq_dev.h"
#include "trxsig_tablegen.h"

namespace {
constexpr int kSoft = 148;
}  // namespace

struct trxsig_l1acq {
  trxsig_ctx *c = nullptr;
  int sps = 0, max_streams = 0, max_samples = 0, max_tiles = 0;
  std::vector<trx_c32> h_seq;          // 64 * sps
  trx_c32 gain{};
  float seq_toa = 0.0f;
  // persistent: the sequence, the per-stream arrays of a search, the tiles' records
  void *d_persist = nullptr;
  trx_c32 *d_seq = nullptr;
  TrxAcqStreams sv{};
  float *ptm = nullptr, *toa = nullptr, *soft = nullptr;
  trx_c32 *amp = nullptr;
  uint8_t *ok = nullptr, *bsic = nullptr, *flags = nullptr;
  int32_t *rfn = nullptr;
  float *tile_m = nullptr, *tile_e = nullptr;
  int32_t *tile_k = nullptr;
  trx_c32 *tile_c = nullptr;
  // stage-2 workspace for `cap` windows; grows only
  TrxWork work;
  int cap = 0;
  trx_c32 *y = nullptr, *corr = nullptr, *peak = nullptr;
  float *pidx = nullptr, *dtoa = nullptr;
  int32_t *woff = nullptr, *wlen = nullptr, *doff = nullptr, *dlen = nullptr;
  float *wq = nullptr, *wR = nullptr;  // the fit detector's q and R of a batch's windows
  // the SCH leg (trxsig_l1acq_set_sch_leg) and what the equalising leg's last search left: taps [max_streams][5], window words
  int sch_leg = TRXSIG_SCHLEG_DEMOD;
  trx_c32 *chan = nullptr;
  int32_t *win = nullptr;
  bool chan_valid = false;             // false: the arrays are filled (zeros, 2) when trxsig_l1acq_sch_channel next asks for them
  // the SCH detector (trxsig_l1acq_set_sch_detector) and what the fit detector's last search left: q and R [max_streams]
  int sch_det = TRXSIG_SCHDET_VALLEY;
  float *fit_q = nullptr, *fit_R = nullptr;
  bool fit_valid = false;              // false: zeros are filled in when trxsig_l1acq_sch_fit next asks
};

namespace {
int fail(trxsig_l1acq *a, const char *what) { return trx_ctx_fail(a ? a->c : nullptr, TRXSIG_EINVAL, what, hipSuccess); }

// the stage-2 workspace for B windows (a growth waits for the stream first); the caller holds the TrxDeviceGuard
int ensure_work(trxsig_l1acq *a, int B) {
  if (B <= a->cap) return TRXSIG_OK;
  trxsig_ctx *c = a->c;
  const size_t n = (size_t)B;
  const TrxCarve cv = { n * TRX_ACQ_WMAX * sizeof(trx_c32), n * TRX_ACQ_WMAX * sizeof(trx_c32), n * sizeof(trx_c32),   // y, corr, peak
                        n * 4, n * 4, n * 4, n * 4, n * 4, n * 4,                                                          // pidx, dtoa, woff, wlen, doff, dlen
                        n * 4, n * 4 };                                                                                    // the fit detector's q, R
  const int rc = trx_work_ensure(c, a->work, cv.total, true, nullptr);
  if (rc != TRXSIG_OK) { a->cap = 0; return rc; }
  void *b = a->work.p;
  a->y = cv.at<trx_c32>(b, 0); a->corr = cv.at<trx_c32>(b, 1); a->peak = cv.at<trx_c32>(b, 2);
  a->pidx = cv.at<float>(b, 3); a->dtoa = cv.at<float>(b, 4);
  a->woff = cv.at<int32_t>(b, 5); a->wlen = cv.at<int32_t>(b, 6); a->doff = cv.at<int32_t>(b, 7); a->dlen = cv.at<int32_t>(b, 8);
  a->wq = cv.at<float>(b, 9); a->wR = cv.at<float>(b, 10);
  a->cap = B;
  return TRXSIG_OK;
}

// stage 2 on B windows already described by (base64 | off32, len): everything after the window set-up
int stage2(trxsig_l1acq *a, const trxsig_c32 *d_samples, const long long *base64, const int32_t *off32, const int32_t *len,
           const float *omega, int B, float thresh, int search, uint8_t *flags, trxsig_c32 *amp, float *toa, float *ptm, float *soft,
           uint8_t *hard, int soft_stride, uint8_t *state, trx_c32 *chan, int32_t *win, float *fit_q, float *fit_R) {
  trxsig_ctx *c = a->c;
  hipStream_t st = (hipStream_t)trxsig_get_stream(c);
  const TrxTables *dT = (const TrxTables *)trxsig_tables_device(c);
  TrxProfiler *prof = trx_ctx_profiler(c);
  const int sps = a->sps;
  TRX_HIPCHK(c, trx_launch_l1acq_shift(st, sps, dT, (const trx_c32 *)d_samples, base64, off32, len, omega, B, a->y, a->woff, a->wlen));
  TRX_HIPCHK(c, trx_launch_convolve(st, a->y, a->woff, a->wlen, B, TRXSIG_L1ACQ_MAX_WINDOW * sps, a->d_seq, 64 * sps, TRXSIG_NO_DELAY, 0,
                                    1, 0, 0, a->corr, a->woff));
  TRX_HIPCHK(c, trx_launch_peak_detect(st, dT, a->corr, a->woff, a->wlen, B, a->peak, a->pidx, nullptr));
  // the fit detector's and the equalising leg's record: the candidates' segments of the shifted windows, amplitudes, TOAs and mask
  TrxMlseArgs ma;
  ma.samples0 = a->y; ma.off0 = a->doff; ma.len = a->dlen; ma.B = B; ma.amp = (const trx_c32 *)amp; ma.toa = a->dtoa; ma.flags = flags;
  ma.need_mask = TRXSIG_F_DETECT; ma.R = fit_R; ma.q = fit_q;   // (R and q: the fit's alone)
  if (a->sch_det == TRXSIG_SCHDET_FIT) {                    // the geometry gate, the fit on the candidates' segments (the ones step 7 takes), q > thresh
    TRX_HIPCHK(c, trx_launch_l1acq_candidates(st, sps, a->wlen, a->peak, a->pidx, B, a->gain, a->seq_toa, search, flags, (trx_c32 *)amp, toa,
                                              a->doff, a->dlen, a->dtoa));
    TRX_HIPCHK(c, trx_launch_sch_fit(st, sps, dT, ma));
    TRX_HIPCHK(c, trx_launch_l1acq_fit_verdict(st, B, fit_q, thresh, flags, ptm, state));
  } else {
    TRX_HIPCHK(c, trx_launch_l1acq_verdict(st, sps, a->corr, a->wlen, a->peak, a->pidx, B, a->gain, a->seq_toa, thresh, search, flags,
                                           (trx_c32 *)amp, toa, ptm, a->doff, a->dlen, a->dtoa, state));
  }
  if (a->sch_leg == TRXSIG_SCHLEG_MLSE) {                   // the equaliser on the same record, in the demodulator's place
    ma.chan = chan; ma.win = win; ma.soft = soft; ma.hard = hard; ma.nsoft = kSoft; ma.stride = soft_stride;
    TRX_HIPCHK(c, trx_launch_mlse_sch(st, sps, dT, ma));
  } else {                                                  // always with the exact arithmetic, whatever trxsig_set_soft_mode says
    TRX_HIPCHK(c, trx_launch_demod(st, sps, dT, a->y, a->doff, a->dlen, B, (const trx_c32 *)amp, a->dtoa, flags, TRXSIG_F_DETECT, soft,
                                   hard, kSoft, soft_stride, prof, TRXSIG_SOFT_EXACT));
  }
  return TRXSIG_OK;
}
}  // namespace

int trxsig_l1acq_create(trxsig_l1acq **out, trxsig_ctx *c, int max_streams, int max_samples) {
  if (!out || !c) return TRXSIG_EINVAL;
  *out = nullptr;
  if (max_streams < 1 || max_streams > 65535 || max_samples < 1 || (long long)max_streams * max_samples > 0x7fffffffLL)
    return trx_ctx_fail(c, TRXSIG_EINVAL, "trxsig_l1acq_create: bad argument", hipSuccess);
  trxsig_l1acq *a = new (std::nothrow) trxsig_l1acq;
  if (!a) return TRXSIG_ENOMEM;
  a->c = c; a->sps = trxsig_sps(c); a->max_streams = max_streams; a->max_samples = max_samples;
  a->max_tiles = trx_acq_tiles(a->sps, max_samples);
  {
    std::unique_ptr<TrxTables> T(new (std::nothrow) TrxTables);
    a->h_seq.resize(64 * (size_t)a->sps);
    if (!T || trx_build_tables(T.get(), a->sps) != 0 || trx_build_sch_sequence(T.get(), a->h_seq.data(), &a->gain, &a->seq_toa) != 0) {
      delete a;
      return trx_ctx_fail(c, TRXSIG_EINVAL, "trxsig_l1acq_create: the correlation sequence", hipSuccess);
    }
  }
  const size_t S = (size_t)max_streams, NT = S * (size_t)(a->max_tiles > 0 ? a->max_tiles : 1);
  const TrxCarve cv = { a->h_seq.size() * sizeof(trx_c32),
                        S, S * 4, S * 4, S * 8, S * 4, S * 4, S * 4, S * 4, S * 8, S * 4,        // state, k, m, c, e, arg, omega, w0, base, wlen
                        S * 4, S * 4, S * 8, S * kSoft * 4, S, S, S, S * 4,                       // ptm, toa, amp, soft, ok, bsic, flags, rfn
                        NT * 4, NT * 4, NT * 8, NT * 4,                                           // tiles: m, k, c, e
                        S * 5 * 8, S * 4,                                                         // the equalising leg's taps and window words
                        S * 4, S * 4 };                                                           // the fit detector's q and R
  TrxDeviceGuard g(trxsig_device(c));
  int rc = trx_device_block(c, "trxsig_l1acq_create", cv.total, { { cv.off[0], a->h_seq.data(), a->h_seq.size() * sizeof(trx_c32) } }, &a->d_persist);
  if (rc != TRXSIG_OK) { delete a; return rc; }
  void *b = a->d_persist;
  a->d_seq = cv.at<trx_c32>(b, 0);
  TrxAcqStreams &s = a->sv;
  s.state = cv.at<uint8_t>(b, 1); s.fcch_k = cv.at<int32_t>(b, 2); s.fcch_m = cv.at<float>(b, 3);
  s.fcch_c = cv.at<trx_c32>(b, 4); s.fcch_e = cv.at<float>(b, 5); s.arg = cv.at<float>(b, 6); s.omega = cv.at<float>(b, 7);
  s.w0 = cv.at<int32_t>(b, 8); s.base = cv.at<long long>(b, 9); s.wlen = cv.at<int32_t>(b, 10);
  a->ptm = cv.at<float>(b, 11); a->toa = cv.at<float>(b, 12); a->amp = cv.at<trx_c32>(b, 13); a->soft = cv.at<float>(b, 14);
  a->ok = cv.at<uint8_t>(b, 15); a->bsic = cv.at<uint8_t>(b, 16); a->flags = cv.at<uint8_t>(b, 17); a->rfn = cv.at<int32_t>(b, 18);
  a->tile_m = cv.at<float>(b, 19); a->tile_k = cv.at<int32_t>(b, 20); a->tile_c = cv.at<trx_c32>(b, 21); a->tile_e = cv.at<float>(b, 22);
  a->chan = cv.at<trx_c32>(b, 23); a->win = cv.at<int32_t>(b, 24);
  a->fit_q = cv.at<float>(b, 25); a->fit_R = cv.at<float>(b, 26);
  rc = ensure_work(a, max_streams);
  if (rc != TRXSIG_OK) {
    if (a->work.p) (void)hipFree(a->work.p);
    (void)hipFree(a->d_persist);
    delete a;
    return rc;
  }
  trx_ctx_retain(c);
  *out = a;
  return TRXSIG_OK;
}

void trxsig_l1acq_destroy(trxsig_l1acq *a) {
  if (!a) return;
  trx_object_destroy(a->c, { a->work.p, a->d_persist });
  delete a;
}

int trxsig_l1acq_sequence(const trxsig_l1acq *a, trxsig_c32 *h_seq, trxsig_c32 *h_gain, float *h_toa) {
  if (!a) return TRXSIG_EINVAL;
  if (h_seq) std::memcpy(h_seq, a->h_seq.data(), a->h_seq.size() * sizeof(trx_c32));
  if (h_gain) { h_gain->re = a->gain.r; h_gain->im = a->gain.i; }
  if (h_toa) *h_toa = a->seq_toa;
  return TRXSIG_OK;
}

int trxsig_l1acq_search(trxsig_l1acq *a, const trxsig_c32 *d_samples, int64_t stream_stride, int n_samples, int n_streams,
                        float fcch_thresh, float sch_thresh, trxsig_l1acq_out *out) {
  if (!a) return TRXSIG_EINVAL;
  if (!d_samples || !out || n_streams < 1 || n_streams > a->max_streams || n_samples < 1 || n_samples > a->max_samples ||
      stream_stride < n_samples)
    return fail(a, "trxsig_l1acq_search: bad argument");
  trxsig_ctx *c = a->c;
  TrxDeviceGuard g(trxsig_device(c));
  hipStream_t st = (hipStream_t)trxsig_get_stream(c);
  const int n_tiles = trx_acq_tiles(a->sps, n_samples);
  const TrxAcqStreams &s = a->sv;
  TRX_HIPCHK(c, trx_launch_l1acq_fcch(st, a->sps, (const trx_c32 *)d_samples, stream_stride, n_samples, n_streams, n_tiles, a->tile_m,
                                      a->tile_k, a->tile_c, a->tile_e));
  TRX_HIPCHK(c, trx_launch_l1acq_pick(st, a->sps, stream_stride, n_samples, n_streams, n_tiles, a->tile_m, a->tile_k, a->tile_c,
                                      a->tile_e, fcch_thresh, s));
  const int rc = stage2(a, d_samples, s.base, nullptr, s.wlen, s.omega, n_streams, sch_thresh, 1, a->flags, (trxsig_c32 *)a->amp, a->toa,
                        a->ptm, a->soft, nullptr, kSoft, s.state, a->chan, a->win, a->fit_q, a->fit_R);
  if (rc != TRXSIG_OK) return rc;
  a->chan_valid = a->sch_leg == TRXSIG_SCHLEG_MLSE;
  a->fit_valid = a->sch_det == TRXSIG_SCHDET_FIT;
  TRX_HIPCHK(c, trx_launch_fec(st, TRX_FEC_MODE_SCH, a->soft, kSoft, 78, 39, n_streams, 0, a->ok, a->bsic, reinterpret_cast<uint8_t *>(a->rfn), 0,
                               trx_ctx_profiler(c)));
  TRX_HIPCHK(c, trx_launch_l1acq_finish(st, n_streams, a->ok, s.state));
  out->n_streams = n_streams; out->soft_stride = kSoft;
  out->d_state = s.state; out->d_fcch_k = s.fcch_k; out->d_fcch_metric = s.fcch_m; out->d_fcch_c = (const trxsig_c32 *)s.fcch_c;
  out->d_fcch_e = s.fcch_e; out->d_arg = s.arg; out->d_omega = s.omega; out->d_sch_w0 = s.w0; out->d_sch_ptm = a->ptm;
  out->d_sch_amp = (const trxsig_c32 *)a->amp; out->d_sch_toa = a->toa; out->d_soft = a->soft; out->d_ok = a->ok; out->d_bsic = a->bsic;
  out->d_rfn = a->rfn;
  return TRXSIG_OK;
}

int trxsig_l1acq_detect_sch_batch(trxsig_l1acq *a, const trxsig_c32 *d_samples, const int32_t *d_offset, const int32_t *d_length, int B,
                                  const float *d_omega, float detect_thresh, uint8_t *d_flags, trxsig_c32 *d_amp, float *d_toa,
                                  float *d_ptm, float *d_soft, uint8_t *d_hard, int soft_stride) {
  if (!a) return TRXSIG_EINVAL;
  if (B < 0 || B > 65535 || soft_stride < kSoft || (B > 0 && (!d_samples || !d_offset || !d_length || !d_flags || !d_amp || !d_toa || !d_soft)))
    return fail(a, "trxsig_l1acq_detect_sch_batch: bad argument");
  if (B == 0) return TRXSIG_OK;
  TrxDeviceGuard g(trxsig_device(a->c));
  const int rc = ensure_work(a, B);
  if (rc != TRXSIG_OK) return rc;
  return stage2(a, d_samples, nullptr, d_offset, d_length, d_omega, B, detect_thresh, 0, d_flags, d_amp, d_toa, d_ptm, d_soft, d_hard,
                soft_stride, nullptr, nullptr, nullptr, a->wq, a->wR);
}

int trxsig_l1acq_set_sch_leg(trxsig_l1acq *a, int leg) {
  if (!a) return TRXSIG_EINVAL;
  if (leg != TRXSIG_SCHLEG_DEMOD && leg != TRXSIG_SCHLEG_MLSE) return fail(a, "trxsig_l1acq_set_sch_leg: not a leg");
  a->sch_leg = leg;
  return TRXSIG_OK;
}

int trxsig_l1acq_sch_channel(trxsig_l1acq *a, const trxsig_c32 **d_chan, const int32_t **d_win) {
  if (!a) return TRXSIG_EINVAL;
  if (!d_chan || !d_win) return fail(a, "trxsig_l1acq_sch_channel: bad argument");
  if (!a->chan_valid) {                                     // no search on the equalising leg since: zeros and "skipped", filled on demand
    trxsig_ctx *c = a->c;
    TrxDeviceGuard g(trxsig_device(c));
    hipStream_t st = (hipStream_t)trxsig_get_stream(c);
    TRX_HIPCHK(c, hipMemsetAsync(a->chan, 0, (size_t)a->max_streams * 5 * sizeof(trx_c32), st));
    TRX_HIPCHK(c, hipMemsetD32Async((hipDeviceptr_t)a->win, 2, (size_t)a->max_streams, st));
    a->chan_valid = true;
  }
  *d_chan = (const trxsig_c32 *)a->chan;
  *d_win = a->win;
  return TRXSIG_OK;
}

int trxsig_l1acq_set_sch_detector(trxsig_l1acq *a, int detector) {
  if (!a) return TRXSIG_EINVAL;
  if (detector != TRXSIG_SCHDET_VALLEY && detector != TRXSIG_SCHDET_FIT) return fail(a, "trxsig_l1acq_set_sch_detector: not a detector");
  a->sch_det = detector;
  return TRXSIG_OK;
}

int trxsig_l1acq_sch_fit(trxsig_l1acq *a, const float **d_q, const float **d_R) {
  if (!a) return TRXSIG_EINVAL;
  if (!d_q || !d_R) return fail(a, "trxsig_l1acq_sch_fit: bad argument");
  if (!a->fit_valid) {                                      // no search on the fit detector since: zeros, filled on demand
    trxsig_ctx *c = a->c;
    TrxDeviceGuard g(trxsig_device(c));
    hipStream_t st = (hipStream_t)trxsig_get_stream(c);
    TRX_HIPCHK(c, hipMemsetAsync(a->fit_q, 0, (size_t)a->max_streams * sizeof(float), st));
    TRX_HIPCHK(c, hipMemsetAsync(a->fit_R, 0, (size_t)a->max_streams * sizeof(float), st));
    a->fit_valid = true;
  }
  *d_q = a->fit_q;
  *d_R = a->fit_R;
  return TRXSIG_OK;
}
