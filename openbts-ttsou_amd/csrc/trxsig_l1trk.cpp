// trxsig_l1trk.cpp -- the tracking receiver's host side (include/trxsig_l1trk.h): the plan and the per-phone state on the device,
// argument checks, and per call one launch on the context's stream (k_l1trk_seed, k_l1trk_set, k_l1trk_slice, k_l1trk_update).
// The host keeps only which of the two anchor sets is current and what the last slice was called with.
#include <hip/hip_runtime_api.h>

#include <new>
#include <vector>

#include "trxsig_ctx.h"
#include "trxsig_l1trk_dev.h"
#include "trxsig_plan.h"

struct trxsig_l1trk {
  trxsig_ctx *c = nullptr;
  int sps = 0, n_phones = 0, n_cols = 0, max_frames = 0, afc_shift = 0, toa_gate = 0;
  float fcch_thresh = 0.0f;
  void *d_mem = nullptr;
  TrxTrkPlan plan{};
  TrxTrkState st{};
  TrxTrkMeas meas{};
  int cur = 0;                          // the anchor set that holds the state
  bool pending = false;                 // a slice whose update has not been made
  int last_fn = 0, last_frames = 0, last_fcch = 0;
};

namespace {
int fail(trxsig_l1trk *t, const char *what) { return trx_ctx_fail(t ? t->c : nullptr, TRXSIG_EINVAL, what, hipSuccess); }
}  // namespace

int trxsig_l1trk_create(trxsig_l1trk **out, trxsig_ctx *c, int n_phones, int n_cols, const int32_t *h_phone, const int32_t *h_c0,
                        int max_frames, int afc_shift, int toa_gate, float fcch_thresh) {
  if (!out || !c) return TRXSIG_EINVAL;
  *out = nullptr;
  if (!h_phone || !h_c0 || n_phones < 1 || n_phones > 65535 || n_cols < 1 || n_cols > 65535 || max_frames < 1 ||
      max_frames > TRXSIG_L1TRK_MAX_FRAMES || afc_shift < 0 || afc_shift > 8 || toa_gate < 1 || toa_gate > TRXSIG_L1TRK_MAX_GATE ||
      !(fcch_thresh == fcch_thresh))
    return trx_ctx_fail(c, TRXSIG_EINVAL, "trxsig_l1trk_create: bad argument", hipSuccess);
  for (int i = 0; i < n_cols; i++)
    if (h_phone[i] < 0 || h_phone[i] >= n_phones) return trx_ctx_fail(c, TRXSIG_EINVAL, "trxsig_l1trk_create: h_phone names no phone", hipSuccess);
  for (int p = 0; p < n_phones; p++)
    if (h_c0[p] != -1 && (h_c0[p] < 0 || h_c0[p] >= n_cols || h_phone[h_c0[p]] != p))
      return trx_ctx_fail(c, TRXSIG_EINVAL, "trxsig_l1trk_create: h_c0 is -1 or a column of its phone", hipSuccess);
  trxsig_l1trk *t = new (std::nothrow) trxsig_l1trk;
  if (!t) return TRXSIG_ENOMEM;
  t->c = c; t->sps = trxsig_sps(c); t->n_phones = n_phones; t->n_cols = n_cols; t->max_frames = max_frames;
  t->afc_shift = afc_shift; t->toa_gate = toa_gate; t->fcch_thresh = fcch_thresh;
  const int cap = max_frames / 10 + 1;                       // FCCH frames are at least ten apart
  // the phones' column lists
  std::vector<int32_t> start((size_t)n_phones + 1, 0), list((size_t)n_cols);
  for (int i = 0; i < n_cols; i++) start[(size_t)h_phone[i] + 1]++;
  for (int p = 0; p < n_phones; p++) start[(size_t)p + 1] += start[(size_t)p];
  {
    std::vector<int32_t> fill(start.begin(), start.end() - 1);
    for (int i = 0; i < n_cols; i++) list[(size_t)fill[(size_t)h_phone[i]]++] = i;
  }
  const size_t P = (size_t)n_phones, C = (size_t)n_cols, R = P * (size_t)cap;
  const TrxCarve cv = { C * 4, P * 4, (P + 1) * 4, C * 4,                             // phone, c0, col_start, col_list
                        P * 4, P * 4, P * 8, P * 8, P * 4, P * 4, P * 4, P, P * 4,     // fn x2, pos x2, phase x2, step, locked, quiet
                        P * 8, P * 8, P * 8, P * 4, P * 4,                             // toa_sum, adj, afc_delta, toa_n, afc_n
                        C, R * 4, R * 16, R * 8, R };                                  // status, fcch fn / c / e / ok
  TrxDeviceGuard g(trxsig_device(c));
  const int rc = trx_device_block(c, "trxsig_l1trk_create", cv.total, { { cv.off[0], h_phone, C * 4 }, { cv.off[1], h_c0, P * 4 },
                                  { cv.off[2], start.data(), (P + 1) * 4 }, { cv.off[3], list.data(), C * 4 } }, &t->d_mem);
  if (rc != TRXSIG_OK) { delete t; return rc; }
  void *b = t->d_mem;
  t->plan.n_phones = n_phones; t->plan.n_cols = n_cols;
  t->plan.phone = cv.at<const int32_t>(b, 0); t->plan.c0 = cv.at<const int32_t>(b, 1);
  t->plan.col_start = cv.at<const int32_t>(b, 2); t->plan.col_list = cv.at<const int32_t>(b, 3);
  TrxTrkState &s = t->st;
  s.fn[0] = cv.at<int32_t>(b, 4); s.fn[1] = cv.at<int32_t>(b, 5);
  s.pos[0] = cv.at<long long>(b, 6); s.pos[1] = cv.at<long long>(b, 7);
  s.phase[0] = cv.at<uint32_t>(b, 8); s.phase[1] = cv.at<uint32_t>(b, 9);
  s.step = cv.at<uint32_t>(b, 10); s.locked = cv.at<uint8_t>(b, 11); s.quiet = cv.at<int32_t>(b, 12);
  s.toa_sum = cv.at<long long>(b, 13); s.adj = cv.at<long long>(b, 14); s.afc_delta = cv.at<long long>(b, 15);
  s.toa_n = cv.at<int32_t>(b, 16); s.afc_n = cv.at<int32_t>(b, 17);
  TrxTrkMeas &m = t->meas;
  m.status = cv.at<uint8_t>(b, 18); m.fcch_fn = cv.at<int32_t>(b, 19); m.fcch_c = cv.at<double>(b, 20);
  m.fcch_e = cv.at<double>(b, 21); m.fcch_ok = cv.at<uint8_t>(b, 22); m.cap = cap;
  trx_ctx_retain(c);
  *out = t;
  return TRXSIG_OK;
}

void trxsig_l1trk_destroy(trxsig_l1trk *t) {
  if (!t) return;
  trx_object_destroy(t->c, { t->d_mem });
  delete t;
}

int trxsig_l1trk_seed(trxsig_l1trk *t, const trxsig_l1acq_out *acq, const int32_t *d_src) {
  if (!t) return TRXSIG_EINVAL;
  if (!acq || !d_src || acq->n_streams < 1 || !acq->d_state || !acq->d_sch_w0 || !acq->d_sch_toa || !acq->d_omega || !acq->d_rfn)
    return fail(t, "trxsig_l1trk_seed: NULL, or not the result of a search");
  trxsig_ctx *c = t->c;
  TrxDeviceGuard g(trxsig_device(c));
  TRX_HIPCHK(c, trx_launch_l1trk_seed((hipStream_t)trxsig_get_stream(c), t->sps, t->plan, t->st, t->cur, acq->n_streams, acq->d_state,
                                      acq->d_sch_w0, acq->d_sch_toa, acq->d_omega, acq->d_rfn, d_src));
  return TRXSIG_OK;
}

int trxsig_l1trk_set(trxsig_l1trk *t, int phone, int locked, int fn, int64_t pos, uint32_t step, uint32_t phase) {
  if (!t) return TRXSIG_EINVAL;
  if (phone < 0 || phone >= t->n_phones || fn < 0 || fn >= kTrxHyperframe) return fail(t, "trxsig_l1trk_set: no such phone, or fn outside [0, 2715648)");
  trxsig_ctx *c = t->c;
  TrxDeviceGuard g(trxsig_device(c));
  TRX_HIPCHK(c, trx_launch_l1trk_set((hipStream_t)trxsig_get_stream(c), t->st, t->cur, phone, locked, fn, (long long)pos, step, phase));
  return TRXSIG_OK;
}

int trxsig_l1trk_state(trxsig_l1trk *t, trxsig_l1trk_view *out) {
  if (!t) return TRXSIG_EINVAL;
  if (!out) return fail(t, "trxsig_l1trk_state: NULL");
  const TrxTrkState &s = t->st;
  out->n_phones = t->n_phones; out->n_cols = t->n_cols;
  out->d_fn = s.fn[t->cur]; out->d_pos = (const int64_t *)s.pos[t->cur]; out->d_phase = s.phase[t->cur]; out->d_step = s.step;
  out->d_locked = s.locked; out->d_quiet = s.quiet;
  out->d_toa_sum = (const int64_t *)s.toa_sum; out->d_toa_n = s.toa_n; out->d_adj = (const int64_t *)s.adj; out->d_afc_n = s.afc_n;
  out->d_afc_delta = (const int64_t *)s.afc_delta;
  return TRXSIG_OK;
}

int trxsig_l1trk_slice(trxsig_l1trk *t, const trxsig_c32 *d_streams, int64_t stream_stride, int64_t n0, int n_samples, int fn,
                       int n_frames, trxsig_c32 *d_cells, int64_t slot_stride, int64_t col_stride, trxsig_l1trk_meas *out) {
  if (!t) return TRXSIG_EINVAL;
  if (!d_streams || !d_cells || !out) return fail(t, "trxsig_l1trk_slice: NULL");
  if (n_frames < 1 || n_frames > t->max_frames || fn < 0 || fn >= kTrxHyperframe || n_samples <= 0 || stream_stride < n_samples)
    return fail(t, "trxsig_l1trk_slice: bad argument (n_frames in 1..max_frames, fn in [0, 2715648), 0 < n_samples <= stream_stride)");
  trxsig_ctx *c = t->c;
  const int sps = t->sps;
  const long long T = 8LL * n_frames, A = t->n_cols, cell = 157LL * sps;
  long long cells_n = 0, streams_n = 0;
  if (!strides_ok(T, A, cell, slot_stride, col_stride) || !extent(T, A, cell, slot_stride, col_stride, &cells_n))
    return fail(t, "trxsig_l1trk_slice: the strides let cells overlap");
  if (!extent(A, 1, n_samples, stream_stride, 0, &streams_n) || overlap(d_streams, streams_n, d_cells, cells_n))
    return fail(t, "trxsig_l1trk_slice: the cells overlap the streams");
  TrxTrkSlice p{};
  p.streams = (const trx_c32 *)d_streams; p.stream_stride = stream_stride; p.n0 = n0; p.n_samples = n_samples;
  p.fn = fn; p.n_frames = n_frames; p.cells = (trx_c32 *)d_cells; p.slot_stride = slot_stride; p.col_stride = col_stride;
  p.cur = t->cur; p.fcch_thresh = t->fcch_thresh;
  TrxDeviceGuard g(trxsig_device(c));
  TRX_HIPCHK(c, trx_launch_l1trk_slice((hipStream_t)trxsig_get_stream(c), sps, (const TrxTables *)trxsig_tables_device(c), t->plan, t->st,
                                       t->meas, p));
  t->cur ^= 1;
  const unsigned a0 = (unsigned)(fn % 51);
  t->last_fn = fn; t->last_frames = n_frames; t->pending = true;
  t->last_fcch = (int)(trx_trk_fcch_before(a0 + (unsigned)n_frames) - trx_trk_fcch_before(a0));
  out->n_phones = t->n_phones; out->n_cols = t->n_cols; out->n_fcch = t->last_fcch; out->fcch_stride = t->meas.cap;
  out->d_status = t->meas.status; out->d_fcch_fn = t->meas.fcch_fn; out->d_fcch_c = t->meas.fcch_c; out->d_fcch_e = t->meas.fcch_e;
  out->d_fcch_ok = t->meas.fcch_ok;
  return TRXSIG_OK;
}

int trxsig_l1trk_update(trxsig_l1trk *t, const trxsig_trxgroup_result *res, int fn, const uint8_t *d_use) {
  if (!t) return TRXSIG_EINVAL;
  if (!res || !res->d_row || !res->d_valid || !res->d_toa) return fail(t, "trxsig_l1trk_update: NULL");
  if (!t->pending || fn != t->last_fn || res->n_slots != 8 * t->last_frames || res->n_arfcn != t->n_cols || res->n_rows < 0)
    return fail(t, "trxsig_l1trk_update: not the pull of the last slice's cells (fn, n_slots, n_arfcn), or a second update for it");
  trxsig_ctx *c = t->c;
  TrxDeviceGuard g(trxsig_device(c));
  TRX_HIPCHK(c, trx_launch_l1trk_update((hipStream_t)trxsig_get_stream(c), t->sps, t->plan, t->st, t->meas, t->cur, fn, res->n_slots,
                                        res->n_rows, t->last_fcch, res->d_row, res->d_valid, res->d_toa, d_use, t->afc_shift, t->toa_gate));
  t->pending = false;
  return TRXSIG_OK;
}
