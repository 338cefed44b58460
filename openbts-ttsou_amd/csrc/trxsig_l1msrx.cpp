// trxsig_l1msrx.cpp -- the mobile-side downlink L1's host side (include/trxsig_l1msrx.h): the channel plan over the downlink
// mappings (trxsig_plan.h), the decoders' state on the device, and per call the block geometry (which blocks of each mapping the call's frames
// touch) and the launches on the context's stream: k_l1msrx_demux, k_l1rx_demux_phy on the rows it recorded, the TCH stream
// decoder, the XCCH stream decoder over the control grid (XCCH, CCCH, BCCH), the generic Viterbi on the gathered SCH bursts,
// k_l1msrx_finish.
#include <hip/hip_runtime_api.h>

#include <cstring>
#include <vector>

#include "trxsig_ctx.h"
#include "trxsig_l1msrx.h"
#include "trxsig_l1msrx_dev.h"
#include "trxsig_plan.h"

namespace {
bool block_lengths_ok() {   // 4, 5 or 24 frames a repeat: the lengths dl_frame divides by
  for (int m = 0; m < TRX_N_DL_MAPS; m++) {
    const int n = trx_plan_maps(TRX_PLAN_DL)[m].n;
    if (n != 4 && n != 5 && n != 24) return false;
  }
  return true;
}
// the plan's class slots by name, and the public class numbers (TRXSIG_L1_CCCH = 3 ..: 2 is the uplink's RACH) -> slots
enum { K_TCH = TRX_PLAN_TCH, K_XCCH = TRX_PLAN_XCCH, K_CCCH = TRX_PLAN_CCCH, K_BCCH = TRX_PLAN_BCCH, K_SCH = TRX_PLAN_SCH,
       K_FCCH = TRX_PLAN_FCCH };
int class_slot(int cls) {
  switch (cls) {
    case TRXSIG_L1_TCH: return K_TCH;
    case TRXSIG_L1_XCCH: return K_XCCH;
    case TRXSIG_L1_CCCH: return K_CCCH;
    case TRXSIG_L1_BCCH: return K_BCCH;
    case TRXSIG_L1_SCH: return K_SCH;
    case TRXSIG_L1_FCCH: return K_FCCH;
    default: return -1;
  }
}
}  // namespace

struct trxsig_l1msrx {
  trxsig_ctx *c = nullptr;
  int bsic = 0, band = 0;
  TrxPlan plan;                        // downlink, all six classes
  // persistent device state
  void *d_persist = nullptr;
  uint8_t *d_tch_state = nullptr, *d_ctl_state = nullptr, *d_active = nullptr;
  int32_t *d_chinfo = nullptr, *d_rssi = nullptr, *d_timing = nullptr, *d_power = nullptr, *d_ta = nullptr, *d_last = nullptr;
  // per-call workspace
  TrxWork work;
  TrxL1msrxDev dv{};
  uint8_t *tch_status = nullptr, *tch_frames = nullptr, *facch = nullptr, *ctl_status = nullptr, *ctl_frames = nullptr, *sch_u = nullptr;
  float *tch_fer = nullptr, *ctl_fer = nullptr;
  int n_ctl() const { return plan.n[K_XCCH] + plan.n[K_CCCH] + plan.n[K_BCCH]; }
};

namespace {
int fail(trxsig_l1msrx *rx, const char *what) { return trx_ctx_fail(rx ? rx->c : nullptr, TRXSIG_EINVAL, what, hipSuccess); }

// carve the per-call workspace; grows only (a growth waits for the stream first)
int ensure_work(trxsig_l1msrx *rx, int nbt, int nbx, int scap, int fcap) {
  const size_t T = (size_t)rx->plan.n[K_TCH], X = (size_t)rx->n_ctl(), B = (size_t)rx->plan.n[K_BCCH], S = (size_t)scap, Fc = (size_t)fcap;
  const TrxCarve cv = {
    T * 4 * nbt * 4, T, T * nbt * 4, T * nbt, T * nbt * 33, T * nbt * 23, T * nbt * 4,      // tch index, b0, fn, status, frames, facch, fer
    X * 4 * nbx * 4, X * nbx * 4, X * nbx, X * nbx * 23, X * nbx * 4, B * nbx * 4,         // ctl index, fn, status, frames, fer; bcch tc
    S * 78 * 4, S * 39, S * 4, S * 4, S, S, S, S,                                           // sch e, u, fn, rfn, present, ok, bsic, sync
    Fc * 4, Fc * 4                                                                          // fcch fn, ones
  };
  const int rc = trx_work_ensure(rx->c, rx->work, cv.total, true, nullptr);
  if (rc != TRXSIG_OK) return rc;
  void *b = rx->work.p;
  TrxL1msrxDev &d = rx->dv;
  d.tch_index = cv.at<int32_t>(b, 0); d.tch_b0 = cv.at<uint8_t>(b, 1); d.tch_fn = cv.at<int32_t>(b, 2);
  rx->tch_status = cv.at<uint8_t>(b, 3); rx->tch_frames = cv.at<uint8_t>(b, 4); rx->facch = cv.at<uint8_t>(b, 5);
  rx->tch_fer = cv.at<float>(b, 6);
  d.ctl_index = cv.at<int32_t>(b, 7); d.ctl_fn = cv.at<int32_t>(b, 8);
  rx->ctl_status = cv.at<uint8_t>(b, 9); rx->ctl_frames = cv.at<uint8_t>(b, 10); rx->ctl_fer = cv.at<float>(b, 11);
  d.ctl_status = rx->ctl_status; d.ctl_frames = rx->ctl_frames;
  d.bcch_tc = cv.at<int32_t>(b, 12);
  d.sch_e = cv.at<float>(b, 13); rx->sch_u = cv.at<uint8_t>(b, 14); d.sch_u = rx->sch_u;
  d.sch_fn = cv.at<int32_t>(b, 15); d.sch_rfn = cv.at<int32_t>(b, 16); d.sch_present = cv.at<uint8_t>(b, 17);
  d.sch_ok = cv.at<uint8_t>(b, 18); d.sch_bsic = cv.at<uint8_t>(b, 19); d.sch_sync = cv.at<uint8_t>(b, 20);
  d.fcch_fn = cv.at<int32_t>(b, 21); d.fcch_ones = cv.at<int32_t>(b, 22);
  return TRXSIG_OK;
}

int set_active(trxsig_l1msrx *rx, int cls, int chan, int open) {
  if (!rx) return TRXSIG_EINVAL;
  const int g = rx->plan.index(class_slot(cls), chan);
  if (g < 0 || cls == TRXSIG_L1_SCH || cls == TRXSIG_L1_FCCH) return fail(rx, "trxsig_l1msrx_open / _close: bad channel");
  trxsig_ctx *c = rx->c;
  TrxDeviceGuard gd(trxsig_device(c));
  const bool tch = cls == TRXSIG_L1_TCH;
  uint8_t *st = tch ? rx->d_tch_state + (size_t)g * TRXSIG_TCH_RX_STATE_BYTES
                    : rx->d_ctl_state + (size_t)(g - rx->plan.n[K_TCH]) * TRXSIG_XCCH_RX_STATE_BYTES;
  const int sacch = cls == TRXSIG_L1_XCCH && rx->plan.sacch(g);
  TRX_HIPCHK(c, trx_launch_l1rx_set((hipStream_t)trxsig_get_stream(c), rx->d_active, g, open, st,
                                    sacch ? rx->d_power + chan : nullptr, sacch ? rx->d_ta + chan : nullptr, sacch));
  return TRXSIG_OK;
}
}  // namespace

int trxsig_l1msrx_create(trxsig_l1msrx **out, trxsig_ctx *c, int n_arfcn, const uint8_t *h_comb, int bsic, int band) {
  if (!out || !c) return TRXSIG_EINVAL;
  *out = nullptr;
  int bidx = -1;
  const std::string err = trx_plan_create_error("trxsig_l1msrx_create", n_arfcn, h_comb, bsic, band, block_lengths_ok(), &bidx);
  if (!err.empty()) return trx_ctx_fail(c, TRXSIG_EINVAL, err.c_str(), hipSuccess);
  trxsig_l1msrx *rx = new (std::nothrow) trxsig_l1msrx;
  if (!rx) return TRXSIG_ENOMEM;
  rx->c = c; rx->bsic = bsic; rx->band = bidx;
  rx->plan = TrxPlan(n_arfcn, h_comb, TRX_PLAN_DL, TRX_PLAN_CLASSES);
  const TrxPlan &pl = rx->plan;
  const size_t N = (size_t)pl.all(), T = (size_t)pl.n[K_TCH], X = (size_t)pl.n[K_XCCH], G = (size_t)rx->n_ctl(), NB = T + G;
  std::vector<int32_t> power, ta;
  trx_plan_sacch_start(pl, power, ta);
  const std::vector<uint8_t> ones(NB, 1);
  TrxCarve cv = { T * TRXSIG_TCH_RX_STATE_BYTES, G * TRXSIG_XCCH_RX_STATE_BYTES, NB, N * 4, NB * 4, NB * 4, X * 4, X * 4, NB * 4 };
  if (cv.total == 0) cv.total = 256;
  TrxDeviceGuard g(trxsig_device(c));
  const int rc = trx_device_block(c, "trxsig_l1msrx_create", cv.total, { { cv.off[2], ones.data(), NB }, { cv.off[3], pl.chinfo.data(), N * 4 },
                                  { cv.off[6], power.data(), X * 4 }, { cv.off[7], ta.data(), X * 4 } }, &rx->d_persist);
  if (rc != TRXSIG_OK) { delete rx; return rc; }
  void *b = rx->d_persist;
  rx->d_tch_state = cv.at<uint8_t>(b, 0); rx->d_ctl_state = cv.at<uint8_t>(b, 1); rx->d_active = cv.at<uint8_t>(b, 2);
  rx->d_chinfo = cv.at<int32_t>(b, 3); rx->d_rssi = cv.at<int32_t>(b, 4); rx->d_timing = cv.at<int32_t>(b, 5);
  rx->d_power = cv.at<int32_t>(b, 6); rx->d_ta = cv.at<int32_t>(b, 7); rx->d_last = cv.at<int32_t>(b, 8);
  TrxL1msrxDev &d = rx->dv;
  d.chinfo = rx->d_chinfo; d.active = rx->d_active; d.rssi = rx->d_rssi; d.timing = rx->d_timing;
  d.ord_power = rx->d_power; d.ord_ta = rx->d_ta; d.last = rx->d_last;
  trx_ctx_retain(c);
  *out = rx;
  return TRXSIG_OK;
}

void trxsig_l1msrx_destroy(trxsig_l1msrx *rx) {
  if (!rx) return;
  trx_object_destroy(rx->c, { rx->work.p, rx->d_persist });
  delete rx;
}

int trxsig_l1msrx_channels(const trxsig_l1msrx *rx, int cls) {
  if (!rx || class_slot(cls) < 0) return TRXSIG_EINVAL;
  return rx->plan.n[class_slot(cls)];
}

int trxsig_l1msrx_channel(const trxsig_l1msrx *rx, int cls, int chan, int *arfcn, int *tn, int *kind, int *sub) {
  return rx ? rx->plan.describe(rx->plan.index(class_slot(cls), chan), arfcn, tn, kind, sub) : TRXSIG_EINVAL;
}

int trxsig_l1msrx_open(trxsig_l1msrx *rx, int cls, int chan) { return set_active(rx, cls, chan, 1); }
int trxsig_l1msrx_close(trxsig_l1msrx *rx, int cls, int chan) { return set_active(rx, cls, chan, 0); }

int trxsig_l1msrx_state(trxsig_l1msrx *rx, int cls, void **d_state) {
  if (!rx || !d_state) return TRXSIG_EINVAL;
  const int k = class_slot(cls);
  if (k < 0 || k > K_BCCH) return TRXSIG_EINVAL;
  if (k == K_TCH) { *d_state = (void *)rx->d_tch_state; return TRXSIG_OK; }
  const size_t first = k == K_XCCH ? 0 : k == K_CCCH ? (size_t)rx->plan.n[K_XCCH] : (size_t)rx->plan.n[K_XCCH] + rx->plan.n[K_CCCH];
  *d_state = (void *)(rx->d_ctl_state + first * TRXSIG_XCCH_RX_STATE_BYTES);
  return TRXSIG_OK;
}

int trxsig_l1msrx_decode(trxsig_l1msrx *rx, const trxsig_trxgroup_result *res, int fn, int wire, trxsig_l1msrx_out *out) {
  if (!rx) return TRXSIG_EINVAL;
  if (!out || fn < 0 || fn >= kTrxHyperframe || !trx_plan_result_ok(res, rx->plan.A))
    return fail(rx, "trxsig_l1msrx_decode: bad argument (whole frames from TN 0 of the object's ARFCNs)");
  trxsig_ctx *c = rx->c;
  TrxL1msrxCall k{};
  k.fn = fn; k.n_frames = res->n_slots / 8; k.n_arfcn = rx->plan.A; k.n_rows = res->n_rows; k.soft_stride = res->soft_stride;
  k.sps = trxsig_sps(c); k.wire = wire ? 1 : 0; k.band = rx->band; k.bsic = rx->bsic;
  k.n_tch = rx->plan.n[K_TCH]; k.n_xcch = rx->plan.n[K_XCCH]; k.n_ccch = rx->plan.n[K_CCCH]; k.n_bcch = rx->plan.n[K_BCCH]; k.n_ctl = rx->n_ctl();
  k.n_sch = rx->plan.n[K_SCH]; k.n_fcch = rx->plan.n[K_FCCH];
  // block geometry per mapping: the positions of frames [fn, fn + F) and the blocks they touch
  for (int m = 0; m < TRX_N_DL_MAPS; m++) {
    const TrxBlockGeom bg = trx_plan_block_geometry(trx_plan_maps(TRX_PLAN_DL)[m], fn, k.n_frames);
    const bool (&used)[TRX_PLAN_CLASSES][TRX_N_DL_MAPS] = rx->plan.map_used;
    k.p_first[m] = (int32_t)bg.p_first;
    k.blk_first[m] = (int32_t)trx_fdiv(bg.p_first, 4);
    if (used[K_TCH][m] && bg.nb_touched > k.nb_tch) k.nb_tch = bg.nb_touched;
    if ((used[K_XCCH][m] || used[K_CCCH][m] || used[K_BCCH][m]) && bg.nb_touched > k.nb_ctl) k.nb_ctl = bg.nb_touched;   // one grid width
    if (m == TRX_DL_SCH && k.n_sch) k.sch_cap = (int)(bg.p_end - bg.p_first);
    if (m == TRX_DL_FCCH && k.n_fcch) k.fcch_cap = (int)(bg.p_end - bg.p_first);
  }
  TrxDeviceGuard g(trxsig_device(c));
  int rc = ensure_work(rx, k.nb_tch, k.nb_ctl, k.sch_cap, k.fcch_cap);
  if (rc != TRXSIG_OK) return rc;
  hipStream_t st = (hipStream_t)trxsig_get_stream(c);
  TrxProfiler *prof = trx_ctx_profiler(c);
  const TrxL1msrxDev &d = rx->dv;
  TRX_HIPCHK(c, trx_launch_l1msrx_demux(st, k, d, res->d_row, res->d_valid, res->d_soft));
  TRX_HIPCHK(c, trx_launch_l1rx_phy(st, d.last, k.n_tch + k.n_ctl, (const trx_c32 *)res->d_amp, res->d_toa, k.sps, d.rssi, d.timing));
  if (k.n_tch && k.nb_tch)
    TRX_HIPCHK(c, trx_launch_fec_rx_stream(st, 1, k.n_tch, 4 * k.nb_tch, res->d_soft, res->soft_stride, res->n_rows, d.tch_index,
                                           d.tch_b0, wire, rx->d_tch_state, rx->tch_status, rx->tch_frames, rx->facch, rx->tch_fer, prof));
  if (k.n_ctl && k.nb_ctl)
    TRX_HIPCHK(c, trx_launch_fec_rx_stream(st, 0, k.n_ctl, 4 * k.nb_ctl, res->d_soft, res->soft_stride, res->n_rows, d.ctl_index,
                                           nullptr, wire, rx->d_ctl_state, rx->ctl_status, nullptr, rx->ctl_frames, rx->ctl_fer, prof));
  if (k.sch_cap)
    TRX_HIPCHK(c, trx_launch_fec(st, 0, d.sch_e, 78, 78, 39, k.sch_cap, wire, rx->sch_u, nullptr, nullptr, 39, prof));
  TRX_HIPCHK(c, trx_launch_l1msrx_finish(st, k, d));
  const size_t X = (size_t)k.n_xcch, XC = X + (size_t)k.n_ccch, nb = (size_t)k.nb_ctl;
  out->n_tch = k.n_tch; out->n_xcch = k.n_xcch; out->n_ccch = k.n_ccch; out->n_bcch = k.n_bcch;
  out->nb_tch = k.nb_tch; out->nb_ctl = k.nb_ctl; out->sch_cap = k.sch_cap; out->fcch_cap = k.fcch_cap;
  out->d_tch_status = rx->tch_status; out->d_tch_frames = rx->tch_frames; out->d_facch = rx->facch; out->d_tch_fer = rx->tch_fer;
  out->d_tch_fn = d.tch_fn;
  out->d_xcch_status = rx->ctl_status; out->d_xcch_frames = rx->ctl_frames; out->d_xcch_fer = rx->ctl_fer; out->d_xcch_fn = d.ctl_fn;
  out->d_ccch_status = rx->ctl_status + X * nb; out->d_ccch_frames = rx->ctl_frames + X * nb * 23;
  out->d_ccch_fer = rx->ctl_fer + X * nb; out->d_ccch_fn = d.ctl_fn + X * nb;
  out->d_bcch_status = rx->ctl_status + XC * nb; out->d_bcch_frames = rx->ctl_frames + XC * nb * 23;
  out->d_bcch_fer = rx->ctl_fer + XC * nb; out->d_bcch_fn = d.ctl_fn + XC * nb; out->d_bcch_tc = d.bcch_tc;
  out->d_sch_fn = d.sch_fn; out->d_sch_rfn = d.sch_rfn; out->d_sch_present = d.sch_present; out->d_sch_ok = d.sch_ok;
  out->d_sch_bsic = d.sch_bsic; out->d_sch_sync = d.sch_sync;
  out->d_fcch_fn = d.fcch_fn; out->d_fcch_ones = d.fcch_ones;
  const size_t T = (size_t)k.n_tch;
  out->d_tch_rssi = d.rssi; out->d_tch_timing = d.timing;
  out->d_xcch_rssi = d.rssi + T; out->d_xcch_timing = d.timing + T;
  out->d_ccch_rssi = d.rssi + T + X; out->d_ccch_timing = d.timing + T + X;
  out->d_bcch_rssi = d.rssi + T + XC; out->d_bcch_timing = d.timing + T + XC;
  out->d_ord_power = d.ord_power; out->d_ord_ta = d.ord_ta;
  return TRXSIG_OK;
}

void trx_l1msrx_follow(const trxsig_l1msrx *rx, TrxL1msrxFollow *o) {
  o->ctx = rx->c; o->n_arfcn = rx->plan.A; o->n_xcch = rx->plan.n[K_XCCH]; o->bsic = rx->bsic; o->band = rx->band;
  o->comb = rx->plan.comb.data(); o->ord_power = rx->d_power; o->ord_ta = rx->d_ta;
}
