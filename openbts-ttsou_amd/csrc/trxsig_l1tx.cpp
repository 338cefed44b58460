// trxsig_l1tx.cpp -- the downlink L1 multiplexer's host side (include/trxsig_l1tx.h): the channel plan and the slot-owner table
// the mux reads (trxsig_plan.h), the channels' records on the device (two copies: a call reads one and commits the other), and per call the
// block geometry of every mapping and three launches on the context's stream: k_l1tx_encode, k_l1tx_mux, k_l1tx_commit.
#include <hip/hip_runtime_api.h>

#include <cstring>
#include <vector>

#include "trxsig_ctx.h"
#include "trxsig_l1tx.h"
#include "trxsig_l1mux_host.h"

namespace {
constexpr long long kMaxOutBytes = 1LL << 34;
// the public class numbers -> the plan's class slots: TRXSIG_L1_CCCH = 3 is slot 2; 2 (the uplink's RACH) names no class here
int class_slot(int cls) { return cls == TRXSIG_L1_CCCH ? TRX_PLAN_CCCH : cls == TRXSIG_L1_TCH || cls == TRXSIG_L1_XCCH ? cls : -1; }
}  // namespace

struct trxsig_l1tx {
  trxsig_ctx *c = nullptr;
  int bsic = 0, band = 0;
  float target = 0.0F;
  TrxPlan plan;                         // downlink: TCH, XCCH, CCCH, BCCH
  int cur = 0;
  void *d_persist = nullptr;
  TrxL1txChan *d_st = nullptr;
  uint8_t *d_si = nullptr;
  TrxWork work, dg;                     // the per-call workspace; the datagrams' staging
  TrxL1txDev dv{};
  int last_fn = -1, last_F = 0;         // the last encode (datagrams)
  int32_t *d_wgc = nullptr;             // its workspace's datagram counts [8 F][ceil(A / 256)] + total
};

namespace {
int fail(trxsig_l1tx *l1, const char *what) { return trx_ctx_fail(l1 ? l1->c : nullptr, TRXSIG_EINVAL, what, hipSuccess); }

int set_active(trxsig_l1tx *l1, int cls, int chan, int open) {
  if (!l1) return TRXSIG_EINVAL;
  const int g = l1->plan.index(class_slot(cls), chan);
  if (g < 0) return fail(l1, "trxsig_l1tx_open / _close: bad channel");
  trxsig_ctx *c = l1->c;
  TrxDeviceGuard gd(trxsig_device(c));
  TRX_HIPCHK(c, trx_launch_l1tx_set((hipStream_t)trxsig_get_stream(c), l1->d_st + (size_t)l1->cur * l1->plan.all() + g, open,
                                    l1->plan.sacch(g) && cls == TRXSIG_L1_XCCH, trx_plan_maps(TRX_PLAN_DL)[l1->plan.map(g)].n));
  return TRXSIG_OK;
}

// block geometry of a call
void geometry(const trxsig_l1tx *l1, int fn, int F, TrxL1txCall &k) {
  k = TrxL1txCall{};
  trx_plan_tx_geometry(l1->plan, 4, fn, F, &k);
  k.n_ccch = l1->plan.n[2]; k.n_bcch = l1->plan.n[3];
  k.cur = l1->cur; k.band = l1->band; k.bsic = l1->bsic; k.rssi_target = l1->target;
}
}  // namespace

int trxsig_l1tx_create(trxsig_l1tx **out, trxsig_ctx *c, int n_arfcn, const uint8_t *h_comb, int bsic, int band, float target) {
  if (!out || !c) return TRXSIG_EINVAL;
  *out = nullptr;
  int bidx = -1;
  const std::string err = trx_plan_create_error("trxsig_l1tx_create", n_arfcn, h_comb, bsic, band, target == target, &bidx);
  if (!err.empty()) return trx_ctx_fail(c, TRXSIG_EINVAL, err.c_str(), hipSuccess);
  trxsig_l1tx *l1 = new (std::nothrow) trxsig_l1tx;
  if (!l1) return TRXSIG_ENOMEM;
  l1->c = c; l1->bsic = bsic; l1->band = bidx; l1->target = target;
  l1->plan = TrxPlan(n_arfcn, h_comb, TRX_PLAN_DL, 4);
  const TrxPlan &pl = l1->plan;
  const size_t N = (size_t)pl.all();
  std::vector<TrxL1txChan> rec(2 * N);
  std::memset(rec.data(), 0, rec.size() * sizeof(TrxL1txChan));
  for (size_t i = 0; i < 2 * N; i++) {
    const int g = (int)(i % N);
    const bool sacch = g >= pl.first[TRX_PLAN_XCCH] && g < pl.first[TRX_PLAN_CCCH] && pl.sacch(g);
    rec[i].h.active = 1;
    rec[i].ord_pow = sacch ? 40 : -1;
    rec[i].ord_ta = sacch ? 0.0F : -1.0F;
  }
  TrxDeviceGuard gd(trxsig_device(c));
  void *si = nullptr;                   // [4][23] + [92], zero: no SIs yet
  const int rc = trx_mux_device_block(c, "trxsig_l1tx_create", pl, rec, 96, nullptr, l1->dv, &l1->d_persist, &si);
  if (rc != TRXSIG_OK) { delete l1; return rc; }
  l1->d_st = l1->dv.st; l1->d_si = (uint8_t *)si; l1->dv.si = l1->d_si;
  trx_ctx_retain(c);
  *out = l1;
  return TRXSIG_OK;
}

void trxsig_l1tx_destroy(trxsig_l1tx *l1) {
  if (!l1) return;
  trx_object_destroy(l1->c, { l1->work.p, l1->dg.p, l1->d_persist });
  delete l1;
}

int trxsig_l1tx_channels(const trxsig_l1tx *l1, int cls) {
  return l1 && class_slot(cls) >= 0 ? l1->plan.n[class_slot(cls)] : TRXSIG_EINVAL;
}

int trxsig_l1tx_channel(const trxsig_l1tx *l1, int cls, int chan, int *arfcn, int *tn, int *kind, int *sub) {
  return l1 ? l1->plan.describe(l1->plan.index(class_slot(cls), chan), arfcn, tn, kind, sub) : TRXSIG_EINVAL;
}

int trxsig_l1tx_open(trxsig_l1tx *l1, int cls, int chan) { return set_active(l1, cls, chan, 1); }
int trxsig_l1tx_close(trxsig_l1tx *l1, int cls, int chan) { return set_active(l1, cls, chan, 0); }

int trxsig_l1tx_set_si(trxsig_l1tx *l1, const uint8_t *h_si) {
  if (!l1) return TRXSIG_EINVAL;
  if (!h_si) return fail(l1, "trxsig_l1tx_set_si: NULL");
  trxsig_ctx *c = l1->c;
  TrxDeviceGuard g(trxsig_device(c));
  uint8_t buf[93];
  std::memcpy(buf, h_si, 92);
  buf[92] = 1;
  TRX_HIPCHK(c, hipStreamSynchronize((hipStream_t)trxsig_get_stream(c)));
  TRX_HIPCHK(c, hipMemcpy(l1->d_si, buf, sizeof buf, hipMemcpyHostToDevice));
  return TRXSIG_OK;
}

int trxsig_l1tx_grid(const trxsig_l1tx *l1, int fn, int F, int *nb_tch, int *nb_xcch, int *nb_ccch) {
  if (!l1 || fn < 0 || fn >= kTrxHyperframe || F <= 0) return TRXSIG_EINVAL;
  TrxL1txCall k;
  geometry(l1, fn, F, k);
  if (nb_tch) *nb_tch = k.nb[0];
  if (nb_xcch) *nb_xcch = k.nb[1];
  if (nb_ccch) *nb_ccch = k.nb[2];
  return TRXSIG_OK;
}

int trxsig_l1tx_state(trxsig_l1tx *l1, int cls, void **d_state) {
  if (!l1 || !d_state) return TRXSIG_EINVAL;
  if (class_slot(cls) < 0) return TRXSIG_EINVAL;
  *d_state = (void *)(l1->d_st + (size_t)l1->cur * l1->plan.all() + l1->plan.first[class_slot(cls)]);
  return TRXSIG_OK;
}

int trxsig_l1tx_encode(trxsig_l1tx *l1, int fn, int F, const trxsig_l1tx_in *in, const trxsig_l1rx *sib, trxsig_l1tx_out *out) {
  if (!l1) return TRXSIG_EINVAL;
  if (!in || !out || fn < 0 || fn >= kTrxHyperframe || F <= 0)
    return fail(l1, "trxsig_l1tx_encode: bad argument (fn in [0, 2715648), n_frames > 0)");
  const TrxPlan &pl = l1->plan;
  if ((long long)pl.A * 8 * 148 * F > kMaxOutBytes) return fail(l1, "trxsig_l1tx_encode: output above 2^34 bytes");
  if ((pl.n[0] && (!in->d_tch_kind || !in->d_tch_payload)) || (pl.n[1] && (!in->d_xcch_kind || !in->d_xcch_payload)) ||
      (pl.n[2] && (!in->d_ccch_kind || !in->d_ccch_payload)))
    return fail(l1, "trxsig_l1tx_encode: NULL grid for a class that has channels");
  TrxL1rxSib sb{};
  if (sib) {
    trx_l1rx_sibling(sib, &sb);
    if (!trx_plan_same(pl, sb.n_arfcn, sb.n_xcch, sb.comb))
      return fail(l1, "trxsig_l1tx_encode: the sibling's plan is not this object's");
  }
  TrxL1txCall k;
  geometry(l1, fn, F, k);
  // workspace: scratch c words and flags per unit, bits, what, orders, datagram counts
  const long long units = k.unit0[3] + (long long)pl.n[3] * k.nb[3];
  const size_t slots = (size_t)pl.A * 8 * (size_t)F;
  const size_t gx = ((size_t)pl.A + 255) / 256;
  const TrxCarve cv = { (size_t)units * 64, (size_t)units, slots * 148, slots, (size_t)pl.n[1] * 4, (size_t)pl.n[1] * 4,
                        8 * (size_t)F * gx * 4 + 4 };
  trxsig_ctx *c = l1->c;
  TrxDeviceGuard g(trxsig_device(c));
  bool gone = false;
  const int rc = trx_work_ensure(c, l1->work, cv.total, false, "trxsig_l1tx_encode: workspace", &gone);
  if (gone) {   // the old workspace held the last call's outputs: from here on there is none to hand out (trxsig_l1tx_datagrams)
    l1->last_fn = -1; l1->last_F = 0; l1->d_wgc = nullptr;
    l1->dv.c = nullptr; l1->dv.flag = nullptr; l1->dv.bits = nullptr; l1->dv.what = nullptr;
    l1->dv.ord_pow = nullptr; l1->dv.ord_ta = nullptr;
  }
  if (rc != TRXSIG_OK) return rc;
  void *b = l1->work.p;
  TrxL1txDev &d = l1->dv;
  d.c = cv.at<uint32_t>(b, 0); d.flag = cv.at<uint8_t>(b, 1); d.bits = cv.at<uint8_t>(b, 2); d.what = cv.at<uint8_t>(b, 3);
  d.ord_pow = cv.at<int32_t>(b, 4); d.ord_ta = cv.at<float>(b, 5); l1->d_wgc = cv.at<int32_t>(b, 6);
  d.kind[0] = in->d_tch_kind; d.payload[0] = in->d_tch_payload;
  d.kind[1] = in->d_xcch_kind; d.payload[1] = in->d_xcch_payload;
  d.kind[2] = in->d_ccch_kind; d.payload[2] = in->d_ccch_payload;
  k.has_sib = sib ? 1 : 0;
  d.sib_rssi = sb.rssi; d.sib_timing = sb.timing; d.sib_power = sb.power; d.sib_ta = sb.ta; d.sib_count = sb.accepted;
  hipStream_t st = (hipStream_t)trxsig_get_stream(c);
  TrxProfiler *prof = trx_ctx_profiler(c);
  TRX_HIPCHK(c, trx_launch_l1tx_encode(st, k, d, prof));
  TRX_HIPCHK(c, trx_launch_l1tx_mux(st, k, d, prof));
  l1->cur ^= 1;
  l1->last_fn = fn; l1->last_F = F;
  out->n_arfcn = pl.A; out->n_frames = F; out->n_xcch = pl.n[1];
  out->d_bits = d.bits; out->d_what = d.what; out->d_ms_power = d.ord_pow; out->d_ms_ta = d.ord_ta;
  return TRXSIG_OK;
}

void trx_l1tx_last(const trxsig_l1tx *l1, TrxL1txLast *o) {
  const bool have = l1->last_fn >= 0 && l1->dv.what && l1->dv.bits;
  o->ctx = l1->c; o->n_arfcn = l1->plan.A;
  o->fn = have ? l1->last_fn : 0; o->n_frames = have ? l1->last_F : 0;
  o->what = have ? l1->dv.what : nullptr; o->bits = have ? l1->dv.bits : nullptr;
}

void trx_l1tx_sibling(const trxsig_l1tx *l1, TrxL1txSib *o) {
  o->ctx = l1->c; o->n_arfcn = l1->plan.A; o->n_xcch = l1->plan.n[TRX_PLAN_XCCH]; o->comb = l1->plan.comb.data();
  o->xcch = l1->d_st + (size_t)l1->cur * l1->plan.all() + l1->plan.first[TRX_PLAN_XCCH];
}

int trxsig_l1tx_datagrams(trxsig_l1tx *l1, uint8_t *h_dgram, int32_t *h_arfcn, int cap, int *n) {
  if (!l1) return TRXSIG_EINVAL;
  if (!n || cap < 0 || (cap > 0 && (!h_dgram || !h_arfcn)) || l1->last_fn < 0)
    return fail(l1, "trxsig_l1tx_datagrams: bad argument (or no encode yet)");
  trxsig_ctx *c = l1->c;
  TrxDeviceGuard g(trxsig_device(c));
  const int A = l1->plan.A;
  const size_t slots = (size_t)A * 8 * (size_t)l1->last_F;
  const size_t room = (size_t)cap < slots ? (size_t)cap : slots;
  const size_t need = trx_align256(room * 154) + room * 4 + 4;
  const int rc = trx_work_ensure(c, l1->dg, need, false, "trxsig_l1tx_datagrams: allocation");
  if (rc != TRXSIG_OK) return rc;
  uint8_t *dg = (uint8_t *)l1->dg.p;
  int32_t *da = (int32_t *)(dg + trx_align256(room * 154));
  const size_t gx = ((size_t)A + 255) / 256;
  int32_t *wg = l1->d_wgc;
  int32_t *tot = wg + 8 * (size_t)l1->last_F * gx;
  hipStream_t st = (hipStream_t)trxsig_get_stream(c);
  TRX_HIPCHK(c, trx_launch_l1tx_dgram(st, l1->dv.what, l1->dv.bits, A, l1->last_F, l1->last_fn, wg, tot, dg, da, (int)room,
                                      trx_ctx_profiler(c)));
  int32_t count = 0;
  TRX_HIPCHK(c, hipMemcpyAsync(&count, tot, 4, hipMemcpyDeviceToHost, st));
  TRX_HIPCHK(c, hipStreamSynchronize(st));
  *n = count;
  if (count > cap) return fail(l1, "trxsig_l1tx_datagrams: cap below the count (*n)");
  if (count > 0) {
    TRX_HIPCHK(c, hipMemcpy(h_dgram, dg, (size_t)count * 154, hipMemcpyDeviceToHost));
    TRX_HIPCHK(c, hipMemcpy(h_arfcn, da, (size_t)count * 4, hipMemcpyDeviceToHost));
  }
  return TRXSIG_OK;
}
