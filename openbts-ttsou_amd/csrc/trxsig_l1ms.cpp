// trxsig_l1ms.cpp -- the mobile-side uplink L1's host side (include/trxsig_l1ms.h): the channel plan and the
// slot-owner table of the uplink mappings (trxsig_plan.h), the channels' records on the device (two copies: a call reads one and
// commits the other), per encode the block geometry of every mapping and three launches on the context's stream (k_l1ms_encode,
// k_l1ms_mux, k_l1ms_commit), per radiate one (k_l1ms_radiate).
#include <hip/hip_runtime_api.h>

#include <cstring>
#include <vector>

#include "trxsig_ctx.h"
#include "trxsig_l1ms.h"
#include "trxsig_l1ms_dev.h"
#include "trxsig_l1msrx_dev.h"
#include "trxsig_l1mux_host.h"

namespace {
const int8_t kPower[3][32] = TRX_POWER_TABLES_INIT;

// the power a handset of the band radiates when ordered to `power` dBm: POWER[band][encodePower(band, power)]
int level_power(int band, int power) { return kPower[band][trx_encode_power(kPower[band], power)]; }
constexpr long long kMaxOutBytes = 1LL << 34;
}  // namespace

struct trxsig_l1ms {
  trxsig_ctx *c = nullptr;
  int bsic = 0, band = 0;
  TrxPlan plan;                         // uplink: TCH, XCCH, RACH (the public class numbers are the plan's class slots)
  int n_all = 0, cur = 0;               // n_all: TCH + XCCH, the channels that have records (the RACH has none)
  void *d_persist = nullptr;
  TrxL1msChan *d_st = nullptr;
  TrxWork work;
  TrxL1msDev dv{};
  int last_F = 0, last_rach = 0;        // the last encode (radiate); 0: none
  const trxsig_l1msrx *fol = nullptr;   // the trxsig_l1msrx whose decoded orders the handsets follow, or null
};

namespace {
int fail(trxsig_l1ms *ms, const char *what) { return trx_ctx_fail(ms ? ms->c : nullptr, TRXSIG_EINVAL, what, hipSuccess); }

int set_active(trxsig_l1ms *ms, int cls, int chan, int open) {
  if (!ms) return TRXSIG_EINVAL;
  const int g = ms->plan.index(cls, chan);
  if (cls == TRXSIG_L1_RACH || g < 0) return fail(ms, "trxsig_l1ms_open / _close: bad channel");
  trxsig_ctx *c = ms->c;
  TrxDeviceGuard gd(trxsig_device(c));
  const bool phy = open && cls == TRXSIG_L1_XCCH && ms->plan.sacch(g);
  TRX_HIPCHK(c, trx_launch_l1ms_set((hipStream_t)trxsig_get_stream(c), ms->d_st + (size_t)ms->cur * ms->n_all + g, open, phy,
                                    level_power(ms->band, 40), 0));
  return TRXSIG_OK;
}

// block geometry of a call
void geometry(const trxsig_l1ms *ms, int fn, int F, TrxL1msCall &k) {
  k = TrxL1msCall{};
  trx_plan_tx_geometry(ms->plan, 2, fn, F, &k);
  k.cur = ms->cur; k.band = ms->band; k.bsic = ms->bsic;
  if (ms->plan.n[TRX_PLAN_RACH]) k.n_rach = (int)(k.p_end[TRX_MAP_RACH_C5] - k.p_first[TRX_MAP_RACH_C5]);
}
}  // namespace

int trxsig_l1ms_create(trxsig_l1ms **out, trxsig_ctx *c, int n_arfcn, const uint8_t *h_comb, int bsic, int band) {
  if (!out || !c) return TRXSIG_EINVAL;
  *out = nullptr;
  int bidx = -1;
  const std::string err = trx_plan_create_error("trxsig_l1ms_create", n_arfcn, h_comb, bsic, band, true, &bidx);
  if (!err.empty()) return trx_ctx_fail(c, TRXSIG_EINVAL, err.c_str(), hipSuccess);
  trxsig_l1ms *ms = new (std::nothrow) trxsig_l1ms;
  if (!ms) return TRXSIG_ENOMEM;
  ms->c = c; ms->bsic = bsic; ms->band = bidx;
  ms->plan = TrxPlan(n_arfcn, h_comb, TRX_PLAN_UL, 3);
  const TrxPlan &pl = ms->plan;
  ms->n_all = pl.first[TRX_PLAN_RACH];
  const size_t N = (size_t)ms->n_all;
  std::vector<TrxL1msChan> rec(2 * N);
  if (N) std::memset(rec.data(), 0, rec.size() * sizeof(TrxL1msChan));
  for (size_t i = 0; i < 2 * N; i++) {
    const int g = (int)(i % N);
    const bool sacch = g >= pl.first[TRX_PLAN_XCCH] && pl.sacch(g);
    rec[i].h.active = 1;
    rec[i].power = sacch ? level_power(bidx, 40) : -1;
    rec[i].ta = sacch ? 0 : -1;
  }
  TrxDeviceGuard gd(trxsig_device(c));
  void *handset = nullptr;
  const int rc = trx_mux_device_block(c, "trxsig_l1ms_create", pl, rec, N * 4, pl.handset.data(), ms->dv, &ms->d_persist, &handset);
  if (rc != TRXSIG_OK) { delete ms; return rc; }
  ms->d_st = ms->dv.st; ms->dv.handset = (const int32_t *)handset;
  trx_ctx_retain(c);
  *out = ms;
  return TRXSIG_OK;
}

void trxsig_l1ms_destroy(trxsig_l1ms *ms) {
  if (!ms) return;
  trx_object_destroy(ms->c, { ms->work.p, ms->d_persist });
  delete ms;
}

int trxsig_l1ms_channels(const trxsig_l1ms *ms, int cls) {
  return ms && cls >= 0 && cls < ms->plan.n_cls ? ms->plan.n[cls] : TRXSIG_EINVAL;
}

int trxsig_l1ms_channel(const trxsig_l1ms *ms, int cls, int chan, int *arfcn, int *tn, int *kind, int *sub) {
  return ms ? ms->plan.describe(ms->plan.index(cls, chan), arfcn, tn, kind, sub) : TRXSIG_EINVAL;
}

int trxsig_l1ms_open(trxsig_l1ms *ms, int cls, int chan) { return set_active(ms, cls, chan, 1); }
int trxsig_l1ms_close(trxsig_l1ms *ms, int cls, int chan) { return set_active(ms, cls, chan, 0); }

int trxsig_l1ms_set_phy(trxsig_l1ms *ms, int chan, int power, int ta) {
  if (!ms) return TRXSIG_EINVAL;
  const int g = ms->plan.index(TRXSIG_L1_XCCH, chan);
  if (g < 0 || !ms->plan.sacch(g) || power < 0 || power > 40 || ta < 0 || ta > 63)
    return fail(ms, "trxsig_l1ms_set_phy: a SACCH channel, power 0..40 dBm, TA 0..63");
  trxsig_ctx *c = ms->c;
  TrxDeviceGuard gd(trxsig_device(c));
  TRX_HIPCHK(c, trx_launch_l1ms_set((hipStream_t)trxsig_get_stream(c), ms->d_st + (size_t)ms->cur * ms->n_all + g, -1, 1,
                                    level_power(ms->band, power), ta));
  return TRXSIG_OK;
}

int trxsig_l1ms_grid(const trxsig_l1ms *ms, int fn, int F, int *nb_tch, int *nb_xcch, int *n_rach) {
  if (!ms || fn < 0 || fn >= kTrxHyperframe || F <= 0) return TRXSIG_EINVAL;
  TrxL1msCall k;
  geometry(ms, fn, F, k);
  if (nb_tch) *nb_tch = k.nb[0];
  if (nb_xcch) *nb_xcch = k.nb[1];
  if (n_rach) *n_rach = k.n_rach;
  return TRXSIG_OK;
}

int trxsig_l1ms_state(trxsig_l1ms *ms, int cls, void **d_state) {
  if (!ms || !d_state || (cls != TRXSIG_L1_TCH && cls != TRXSIG_L1_XCCH)) return TRXSIG_EINVAL;
  *d_state = (void *)(ms->d_st + (size_t)ms->cur * ms->n_all + (cls == TRXSIG_L1_XCCH ? ms->plan.n[0] : 0));
  return TRXSIG_OK;
}

int trxsig_l1ms_follow(trxsig_l1ms *ms, const trxsig_l1msrx *rx) {
  if (!ms) return TRXSIG_EINVAL;
  if (rx) {
    TrxL1msrxFollow fo{};
    trx_l1msrx_follow(rx, &fo);
    if (fo.ctx != ms->c || fo.bsic != ms->bsic || fo.band != ms->band || !trx_plan_same(ms->plan, fo.n_arfcn, fo.n_xcch, fo.comb))
      return fail(ms, "trxsig_l1ms_follow: the trxsig_l1msrx's plan (or context) is not this object's");
  }
  ms->fol = rx;
  return TRXSIG_OK;
}

int trxsig_l1ms_encode(trxsig_l1ms *ms, int fn, int F, const trxsig_l1ms_in *in, const trxsig_l1tx *sib, trxsig_l1ms_out *out) {
  if (!ms) return TRXSIG_EINVAL;
  if (!in || !out || fn < 0 || fn >= kTrxHyperframe || F <= 0)
    return fail(ms, "trxsig_l1ms_encode: bad argument (fn in [0, 2715648), n_frames > 0)");
  const TrxPlan &pl = ms->plan;
  if ((long long)pl.A * 8 * 148 * F > kMaxOutBytes) return fail(ms, "trxsig_l1ms_encode: output above 2^34 bytes");
  TrxL1msCall k;
  geometry(ms, fn, F, k);
  if ((pl.n[0] && (!in->d_tch_kind || !in->d_tch_payload)) || (pl.n[1] && (!in->d_xcch_kind || !in->d_xcch_payload)) ||
      (k.n_rach && (!in->d_rach_kind || !in->d_rach_ra)))
    return fail(ms, "trxsig_l1ms_encode: NULL grid for a class that has channels");
  if (sib && ms->fol) return fail(ms, "trxsig_l1ms_encode: a sibling while following a trxsig_l1msrx");
  TrxL1txSib sb{};
  if (sib) {
    trx_l1tx_sibling(sib, &sb);
    if (sb.ctx != ms->c || !trx_plan_same(pl, sb.n_arfcn, sb.n_xcch, sb.comb))
      return fail(ms, "trxsig_l1ms_encode: the sibling's plan (or context) is not this object's");
  }
  // workspace: scratch c words and flags per unit, bits, what, who, the handsets after the call
  const long long units = k.unit0[1] + (long long)pl.n[1] * k.nb[1];
  const size_t slots = (size_t)pl.A * 8 * (size_t)F;
  const TrxCarve cv = { (size_t)units * 64, (size_t)units, slots * 148, slots, slots * 4, (size_t)pl.n[1] * 4, (size_t)pl.n[1] * 4 };
  trxsig_ctx *c = ms->c;
  TrxDeviceGuard g(trxsig_device(c));
  bool gone = false;
  const int rc = trx_work_ensure(c, ms->work, cv.total, false, "trxsig_l1ms_encode: workspace", &gone);
  if (gone) ms->last_F = 0;             // the old workspace held the last call's outputs: there is none to radiate from here on
  if (rc != TRXSIG_OK) return rc;
  void *b = ms->work.p;
  TrxL1msDev &d = ms->dv;
  d.c = cv.at<uint32_t>(b, 0); d.flag = cv.at<uint8_t>(b, 1); d.bits = cv.at<uint8_t>(b, 2); d.what = cv.at<uint8_t>(b, 3);
  d.who = cv.at<int32_t>(b, 4); d.ms_power = cv.at<int32_t>(b, 5); d.ms_ta = cv.at<int32_t>(b, 6);
  d.kind[0] = in->d_tch_kind; d.payload[0] = in->d_tch_payload;
  d.kind[1] = in->d_xcch_kind; d.payload[1] = in->d_xcch_payload;
  d.rach_kind = in->d_rach_kind; d.rach_ra = in->d_rach_ra; d.rach_bsic = in->d_rach_bsic;
  k.has_sib = sib ? 1 : ms->fol ? 2 : 0;
  d.sib = sb.xcch;
  d.fol_power = d.fol_ta = nullptr;
  if (ms->fol) {
    TrxL1msrxFollow fo{};
    trx_l1msrx_follow(ms->fol, &fo);
    d.fol_power = fo.ord_power; d.fol_ta = fo.ord_ta;
  }
  hipStream_t st = (hipStream_t)trxsig_get_stream(c);
  TRX_HIPCHK(c, trx_launch_l1ms_encode(st, k, d));
  TRX_HIPCHK(c, trx_launch_l1ms_mux(st, k, d));
  ms->cur ^= 1;
  ms->last_F = F; ms->last_rach = k.n_rach;
  out->n_arfcn = pl.A; out->n_frames = F; out->n_xcch = pl.n[1];
  out->d_bits = d.bits; out->d_what = d.what; out->d_ms_power = d.ms_power; out->d_ms_ta = d.ms_ta;
  return TRXSIG_OK;
}

int trxsig_l1ms_radiate(trxsig_l1ms *ms, const trxsig_l1ms_air *air, trxsig_c32 *d_samples, int64_t slot_stride,
                        int64_t arfcn_stride) {
  if (!ms) return TRXSIG_EINVAL;
  if (!air || !d_samples) return fail(ms, "trxsig_l1ms_radiate: NULL");
  if (ms->last_F <= 0) return fail(ms, "trxsig_l1ms_radiate: no encode yet (or none since the workspace last grew)");
  trxsig_ctx *c = ms->c;
  const int sps = trxsig_sps(c);
  const TrxPlan &pl = ms->plan;
  const long long T = 8LL * ms->last_F;
  if (!strides_ok(T, pl.A, 157LL * sps, slot_stride, arfcn_stride)) return fail(ms, "trxsig_l1ms_radiate: the strides let cells overlap");
  if ((pl.n[0] && (!air->d_tch_gain || !air->d_tch_delay)) || (pl.n[1] && (!air->d_xcch_gain || !air->d_xcch_delay)) ||
      (ms->last_rach && (!air->d_rach_gain || !air->d_rach_delay)) || (ms->n_all && !air->d_amp_of_power))
    return fail(ms, "trxsig_l1ms_radiate: NULL array for a class that has channels");
  TrxL1msAir p{};
  p.gain[0] = (const trx_c32 *)air->d_tch_gain; p.gain[1] = (const trx_c32 *)air->d_xcch_gain; p.gain[2] = (const trx_c32 *)air->d_rach_gain;
  p.delay[0] = air->d_tch_delay; p.delay[1] = air->d_xcch_delay; p.delay[2] = air->d_rach_delay;
  p.amp_of_power = air->d_amp_of_power;
  const TrxL1msDev &d = ms->dv;
  p.bits = d.bits; p.what = d.what; p.who = d.who; p.handset = d.handset; p.ms_power = d.ms_power; p.ms_ta = d.ms_ta;
  p.out = (trx_c32 *)d_samples; p.slot_stride = slot_stride; p.arfcn_stride = arfcn_stride;
  p.n_arfcn = pl.A; p.n_tch = pl.n[0]; p.rows = T;
  TrxDeviceGuard g(trxsig_device(c));
  TRX_HIPCHK(c, trx_launch_l1ms_radiate((hipStream_t)trxsig_get_stream(c), sps, (const TrxTables *)trxsig_tables_device(c), p));
  return TRXSIG_OK;
}
