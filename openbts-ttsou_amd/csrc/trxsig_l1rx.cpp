// trxsig_l1rx.cpp -- the uplink L1 demultiplexer's host side (include/trxsig_l1rx.h): the channel plan (trxsig_plan.h), the decoders' state
// on the device, and per call the block geometry (which blocks of each mapping the call's frames touch) and five launches on the
// context's stream: k_l1rx_demux, the TCH and XCCH stream decoders, the RACH decoder on the gathered bursts, k_l1rx_finish.
#include <hip/hip_runtime_api.h>

#include <cstring>
#include <vector>

#include "trxsig_ctx.h"
#include "trxsig_l1rx.h"
#include "trxsig_plan.h"

struct trxsig_l1rx {
  trxsig_ctx *c = nullptr;
  int bsic = 0, band = 0;
  TrxPlan plan;                        // uplink: TCH, XCCH, RACH (the public class numbers are the plan's class slots)
  // persistent device state
  void *d_persist = nullptr;
  uint8_t *d_tch_state = nullptr, *d_xcch_state = nullptr, *d_active = nullptr;
  int32_t *d_chinfo = nullptr, *d_rssi = nullptr, *d_timing = nullptr, *d_power = nullptr, *d_ta = nullptr;
  uint32_t *d_accepted = nullptr;
  // per-call workspace
  TrxWork work;
  TrxL1rxDev dv{};
  uint8_t *tch_status = nullptr, *tch_frames = nullptr, *facch = nullptr, *xcch_status = nullptr, *xcch_frames = nullptr;
  float *tch_fer = nullptr, *xcch_fer = nullptr;
};

namespace {
int fail(trxsig_l1rx *l1, const char *what) { return trx_ctx_fail(l1 ? l1->c : nullptr, TRXSIG_EINVAL, what, hipSuccess); }

// carve the per-call workspace for (nb_tch, nb_xcch, rach_cap); grows only (a growth waits for the stream first)
int ensure_work(trxsig_l1rx *l1, int nbt, int nbx, int cap) {
  const size_t T = (size_t)l1->plan.n[TRX_PLAN_TCH], X = (size_t)l1->plan.n[TRX_PLAN_XCCH], R = (size_t)cap;
  const TrxCarve cv = {
    T * 4 * nbt * 4, T, T * nbt * 4, T * nbt, T * nbt * 33, T * nbt * 23, T * nbt * 4,      // tch index, b0, fn, status, frames, facch, fer
    X * 4 * nbx * 4, X * nbx * 4, X * nbx, X * nbx * 23, X * nbx * 4,                      // xcch index, fn, status, frames, fer
    R * 148 * 4, R * 4, R * 4, R * 4, R * 4, 4, R, R, R, R                                  // rach soft, fn, arfcn, rssi, timing, count, tail, bsic, ra, ok
  };
  const int rc = trx_work_ensure(l1->c, l1->work, cv.total, true, nullptr);
  if (rc != TRXSIG_OK) return rc;
  void *b = l1->work.p;
  TrxL1rxDev &d = l1->dv;
  d.tch_index = cv.at<int32_t>(b, 0); d.tch_b0 = cv.at<uint8_t>(b, 1); d.tch_fn = cv.at<int32_t>(b, 2);
  l1->tch_status = cv.at<uint8_t>(b, 3); l1->tch_frames = cv.at<uint8_t>(b, 4); l1->facch = cv.at<uint8_t>(b, 5);
  l1->tch_fer = cv.at<float>(b, 6);
  d.xcch_index = cv.at<int32_t>(b, 7); d.xcch_fn = cv.at<int32_t>(b, 8);
  l1->xcch_status = cv.at<uint8_t>(b, 9); l1->xcch_frames = cv.at<uint8_t>(b, 10); l1->xcch_fer = cv.at<float>(b, 11);
  d.xcch_status = l1->xcch_status; d.xcch_frames = l1->xcch_frames;
  d.rach_soft = cv.at<float>(b, 12); d.rach_fn = cv.at<int32_t>(b, 13); d.rach_arfcn = cv.at<int32_t>(b, 14);
  d.rach_rssi = cv.at<int32_t>(b, 15); d.rach_timing = cv.at<int32_t>(b, 16); d.rach_count = cv.at<int32_t>(b, 17);
  d.rach_tail = cv.at<uint8_t>(b, 18); d.rach_bsic = cv.at<uint8_t>(b, 19); d.rach_ra = cv.at<uint8_t>(b, 20);
  d.rach_ok = cv.at<uint8_t>(b, 21);
  return TRXSIG_OK;
}

int set_active(trxsig_l1rx *l1, int cls, int chan, int open) {
  if (!l1) return TRXSIG_EINVAL;
  const int g = l1->plan.index(cls, chan);
  if (cls == TRXSIG_L1_RACH || g < 0) return fail(l1, "trxsig_l1rx_open / _close: bad channel");
  trxsig_ctx *c = l1->c;
  TrxDeviceGuard gd(trxsig_device(c));
  const bool tch = cls == TRXSIG_L1_TCH;
  uint8_t *st = tch ? l1->d_tch_state + (size_t)chan * TRXSIG_TCH_RX_STATE_BYTES
                    : l1->d_xcch_state + (size_t)chan * TRXSIG_XCCH_RX_STATE_BYTES;
  TRX_HIPCHK(c, trx_launch_l1rx_set((hipStream_t)trxsig_get_stream(c), l1->d_active, g, open, st, tch ? nullptr : l1->d_power + chan,
                                    tch ? nullptr : l1->d_ta + chan, l1->plan.sacch(g)));
  return TRXSIG_OK;
}
}  // namespace

int trxsig_l1rx_create(trxsig_l1rx **out, trxsig_ctx *c, int n_arfcn, const uint8_t *h_comb, int bsic, int band) {
  if (!out || !c) return TRXSIG_EINVAL;
  *out = nullptr;
  int bidx = -1;
  const std::string err = trx_plan_create_error("trxsig_l1rx_create", n_arfcn, h_comb, bsic, band, true, &bidx);
  if (!err.empty()) return trx_ctx_fail(c, TRXSIG_EINVAL, err.c_str(), hipSuccess);
  trxsig_l1rx *l1 = new (std::nothrow) trxsig_l1rx;
  if (!l1) return TRXSIG_ENOMEM;
  l1->c = c; l1->bsic = bsic; l1->band = bidx;
  l1->plan = TrxPlan(n_arfcn, h_comb, TRX_PLAN_UL, 3);
  const TrxPlan &pl = l1->plan;
  const size_t N = (size_t)pl.all(), T = (size_t)pl.n[TRX_PLAN_TCH], X = (size_t)pl.n[TRX_PLAN_XCCH];
  std::vector<int32_t> power, ta;
  trx_plan_sacch_start(pl, power, ta);
  const std::vector<uint8_t> ones(N, 1);
  const TrxCarve cv = { T * TRXSIG_TCH_RX_STATE_BYTES, X * TRXSIG_XCCH_RX_STATE_BYTES, N, N * 4, N * 4, N * 4, X * 4, X * 4, N * 4 };
  TrxDeviceGuard g(trxsig_device(c));
  const int rc = trx_device_block(c, "trxsig_l1rx_create", cv.total, { { cv.off[2], ones.data(), N }, { cv.off[3], pl.chinfo.data(), N * 4 },
                                  { cv.off[6], power.data(), X * 4 }, { cv.off[7], ta.data(), X * 4 } }, &l1->d_persist);
  if (rc != TRXSIG_OK) { delete l1; return rc; }
  void *b = l1->d_persist;
  l1->d_tch_state = cv.at<uint8_t>(b, 0); l1->d_xcch_state = cv.at<uint8_t>(b, 1); l1->d_active = cv.at<uint8_t>(b, 2);
  l1->d_chinfo = cv.at<int32_t>(b, 3); l1->d_rssi = cv.at<int32_t>(b, 4); l1->d_timing = cv.at<int32_t>(b, 5);
  l1->d_power = cv.at<int32_t>(b, 6); l1->d_ta = cv.at<int32_t>(b, 7); l1->d_accepted = cv.at<uint32_t>(b, 8);
  TrxL1rxDev &d = l1->dv;
  d.chinfo = l1->d_chinfo; d.active = l1->d_active; d.rssi = l1->d_rssi; d.timing = l1->d_timing;
  d.ms_power = l1->d_power; d.ms_ta = l1->d_ta; d.accepted = l1->d_accepted; d.bsic = bsic;
  trx_ctx_retain(c);
  *out = l1;
  return TRXSIG_OK;
}

void trxsig_l1rx_destroy(trxsig_l1rx *l1) {
  if (!l1) return;
  trx_object_destroy(l1->c, { l1->work.p, l1->d_persist });
  delete l1;
}

int trxsig_l1rx_channels(const trxsig_l1rx *l1, int cls) {
  return l1 && cls >= 0 && cls < l1->plan.n_cls ? l1->plan.n[cls] : TRXSIG_EINVAL;
}

int trxsig_l1rx_channel(const trxsig_l1rx *l1, int cls, int chan, int *arfcn, int *tn, int *kind, int *sub) {
  return l1 ? l1->plan.describe(l1->plan.index(cls, chan), arfcn, tn, kind, sub) : TRXSIG_EINVAL;
}

int trxsig_l1rx_open(trxsig_l1rx *l1, int cls, int chan) { return set_active(l1, cls, chan, 1); }
int trxsig_l1rx_close(trxsig_l1rx *l1, int cls, int chan) { return set_active(l1, cls, chan, 0); }

int trxsig_l1rx_state(trxsig_l1rx *l1, int cls, void **d_state) {
  if (!l1 || !d_state || (cls != TRXSIG_L1_TCH && cls != TRXSIG_L1_XCCH)) return TRXSIG_EINVAL;
  *d_state = cls == TRXSIG_L1_TCH ? (void *)l1->d_tch_state : (void *)l1->d_xcch_state;
  return TRXSIG_OK;
}

int trxsig_l1rx_decode(trxsig_l1rx *l1, const trxsig_trxgroup_result *res, int fn, int wire, trxsig_l1rx_out *out) {
  if (!l1) return TRXSIG_EINVAL;
  if (!out || fn < 0 || fn >= kTrxHyperframe || !trx_plan_result_ok(res, l1->plan.A))
    return fail(l1, "trxsig_l1rx_decode: bad argument (whole frames from TN 0 of the object's ARFCNs)");
  trxsig_ctx *c = l1->c;
  TrxL1rxCall k{};
  k.fn = fn; k.n_frames = res->n_slots / 8; k.n_arfcn = l1->plan.A; k.n_rows = res->n_rows; k.soft_stride = res->soft_stride;
  k.sps = trxsig_sps(c); k.n_tch = l1->plan.n[TRX_PLAN_TCH]; k.n_xcch = l1->plan.n[TRX_PLAN_XCCH]; k.n_rach = l1->plan.n[TRX_PLAN_RACH]; k.band = l1->band;
  // block geometry per mapping: the positions of frames [fn, fn + F) and the blocks they touch
  for (int m = 0; m < TRX_N_MAPS; m++) {
    const TrxBlockGeom bg = trx_plan_block_geometry(trx_plan_maps(TRX_PLAN_UL)[m], fn, k.n_frames);
    k.p_first[m] = bg.p_first;
    k.blk_first[m] = (int32_t)trx_fdiv(bg.p_first, 4);
    if (l1->plan.map_used[TRX_PLAN_TCH][m] && bg.nb_touched > k.nb_tch) k.nb_tch = bg.nb_touched;
    if (l1->plan.map_used[TRX_PLAN_XCCH][m] && bg.nb_touched > k.nb_xcch) k.nb_xcch = bg.nb_touched;
    if (m == TRX_MAP_RACH_C5 && k.n_rach) k.rach_cap = (int)(bg.p_end - bg.p_first);
  }
  TrxDeviceGuard g(trxsig_device(c));
  int rc = ensure_work(l1, k.nb_tch, k.nb_xcch, k.rach_cap);
  if (rc != TRXSIG_OK) return rc;
  hipStream_t st = (hipStream_t)trxsig_get_stream(c);
  TrxProfiler *prof = trx_ctx_profiler(c);
  const TrxL1rxDev &d = l1->dv;
  TRX_HIPCHK(c, trx_launch_l1rx_demux(st, k, d, res->d_row, res->d_valid, res->d_soft, (const trx_c32 *)res->d_amp, res->d_toa, prof));
  if (k.n_tch && k.nb_tch)
    TRX_HIPCHK(c, trx_launch_fec_rx_stream(st, 1, k.n_tch, 4 * k.nb_tch, res->d_soft, res->soft_stride, res->n_rows, d.tch_index,
                                           d.tch_b0, wire, l1->d_tch_state, l1->tch_status, l1->tch_frames, l1->facch, l1->tch_fer, prof));
  if (k.n_xcch && k.nb_xcch)
    TRX_HIPCHK(c, trx_launch_fec_rx_stream(st, 0, k.n_xcch, 4 * k.nb_xcch, res->d_soft, res->soft_stride, res->n_rows, d.xcch_index,
                                           nullptr, wire, l1->d_xcch_state, l1->xcch_status, nullptr, l1->xcch_frames, l1->xcch_fer,
                                           prof));
  if (k.rach_cap)
    TRX_HIPCHK(c, trx_launch_fec(st, 2, d.rach_soft, 148, 36, 18, k.rach_cap, wire, d.rach_tail, d.rach_bsic, d.rach_ra, 0, prof));
  TRX_HIPCHK(c, trx_launch_l1rx_finish(st, k, d, prof));
  out->n_tch = k.n_tch; out->n_xcch = k.n_xcch; out->nb_tch = k.nb_tch; out->nb_xcch = k.nb_xcch; out->rach_cap = k.rach_cap;
  out->d_tch_status = l1->tch_status; out->d_tch_frames = l1->tch_frames; out->d_facch = l1->facch; out->d_tch_fer = l1->tch_fer;
  out->d_tch_fn = d.tch_fn;
  out->d_xcch_status = l1->xcch_status; out->d_xcch_frames = l1->xcch_frames; out->d_xcch_fer = l1->xcch_fer; out->d_xcch_fn = d.xcch_fn;
  out->d_rach_count = d.rach_count; out->d_rach_fn = d.rach_fn; out->d_rach_arfcn = d.rach_arfcn; out->d_rach_rssi = d.rach_rssi;
  out->d_rach_timing = d.rach_timing; out->d_rach_ok = d.rach_ok; out->d_rach_ra = d.rach_ra;
  out->d_tch_rssi = d.rssi; out->d_tch_timing = d.timing; out->d_xcch_rssi = d.rssi + k.n_tch; out->d_xcch_timing = d.timing + k.n_tch;
  out->d_ms_power = d.ms_power; out->d_ms_ta = d.ms_ta;
  return TRXSIG_OK;
}

void trx_l1rx_sibling(const trxsig_l1rx *l1, TrxL1rxSib *o) {
  const int T = l1->plan.n[TRX_PLAN_TCH];
  o->n_arfcn = l1->plan.A; o->n_tch = T; o->n_xcch = l1->plan.n[TRX_PLAN_XCCH]; o->comb = l1->plan.comb.data();
  o->rssi = l1->d_rssi + T; o->timing = l1->d_timing + T; o->power = l1->d_power; o->ta = l1->d_ta;
  o->accepted = l1->d_accepted + T;
}
