// trxsig_l1ciph.cpp -- the ciphering stage's host side (include/trxsig_l1ciph.h): the channel plan and the slot-owner
// table of both directions (trxsig_plan.h: every stage's rules and numbering), the channels' records on the device,
// the 64 key steps of a key change, argument checks, and per call one launch on the context's stream (k_a5_blocks, k_l1ciph_set,
// k_l1ciph_bits, k_l1ciph_soft).  The host keeps nothing between calls but the plan.
#include <hip/hip_runtime_api.h>

#include <new>
#include <vector>

#include "trxsig_ctx.h"
#include "trxsig_l1ciph.h"
#include "trxsig_a5_dev.h"
#include "trxsig_plan.h"

namespace {
constexpr long long kMaxSlots = 1LL << 30;
}  // namespace

struct trxsig_l1ciph {
  trxsig_ctx *c = nullptr;
  TrxPlan plan;                         // the dedicated channels (TCH, then XCCH): the same in both directions
  void *d_mem = nullptr;
  TrxCiphRec *d_rec = nullptr;
  TrxCiphDev dv{};
};

namespace {
int fail(trxsig_l1ciph *o, const char *what) { return trx_ctx_fail(o ? o->c : nullptr, TRXSIG_EINVAL, what, hipSuccess); }
}  // namespace

int trxsig_a5_1_blocks_batch(trxsig_ctx *c, int n, const uint8_t *d_kc, const uint32_t *d_count, uint8_t *d_block1, uint8_t *d_block2) {
  if (!c) return TRXSIG_EINVAL;
  if (n < 0 || n > (1 << 24) || (n > 0 && (!d_kc || !d_count || (!d_block1 && !d_block2))))
    return trx_ctx_fail(c, TRXSIG_EINVAL, "trxsig_a5_1_blocks_batch: bad argument (n in 0..2^24, keys, counts and an output)", hipSuccess);
  if (n == 0) return TRXSIG_OK;
  TrxDeviceGuard g(trxsig_device(c));
  TRX_HIPCHK(c, trx_launch_a5_blocks((hipStream_t)trxsig_get_stream(c), n, d_kc, d_count, d_block1, d_block2));
  return TRXSIG_OK;
}

int trxsig_l1ciph_create(trxsig_l1ciph **out, trxsig_ctx *c, int n_arfcn, const uint8_t *h_comb) {
  if (!out || !c) return TRXSIG_EINVAL;
  *out = nullptr;
  if (n_arfcn <= 0 || n_arfcn > 0xffff || !h_comb) return trx_ctx_fail(c, TRXSIG_EINVAL, "trxsig_l1ciph_create: bad argument", hipSuccess);
  if (!trx_plan_validate(h_comb, n_arfcn))
    return trx_ctx_fail(c, TRXSIG_EINVAL, "trxsig_l1ciph_create: unsupported channel combination or placement", hipSuccess);
  trxsig_l1ciph *o = new (std::nothrow) trxsig_l1ciph;
  if (!o) return TRXSIG_ENOMEM;
  o->c = c;
  o->plan = TrxPlan(n_arfcn, h_comb, TRX_PLAN_DL, 2);
  const TrxPlan &pl = o->plan;
  // the slot owners: [downlink / uplink][combination I / V / VII][TN][fn mod 104 (I) or 102 (V, VII)] -> -1, 0 (the TCH) or
  // 1 + the XCCH channel's place among the slot's
  std::vector<int8_t> route;
  bool disjoint = trx_plan_owner_table(TRX_PLAN_DL, false, true, route);
  disjoint = trx_plan_owner_table(TRX_PLAN_UL, false, true, route) && disjoint;
  const size_t N = (size_t)pl.all(), S = 8 * (size_t)n_arfcn;
  const TrxCarve cv = { (N + 1) * sizeof(TrxCiphRec), S * 4, S * 4, route.size() };
  TrxDeviceGuard g(trxsig_device(c));
  if (!disjoint) { delete o; return trx_ctx_fail(c, TRXSIG_EINVAL, "trxsig_l1ciph_create: device allocation", hipSuccess); }
  const int rc = trx_device_block(c, "trxsig_l1ciph_create", cv.total, { { cv.off[1], pl.slot.data(), S * 4 }, { cv.off[2], pl.slot_x.data(), S * 4 },
                                  { cv.off[3], route.data(), route.size() } }, &o->d_mem);   // the records zero: every channel off
  if (rc != TRXSIG_OK) { delete o; return rc; }
  o->d_rec = cv.at<TrxCiphRec>(o->d_mem, 0);
  TrxCiphDev &d = o->dv;
  d.rec = o->d_rec; d.slot = cv.at<int32_t>(o->d_mem, 1); d.slot_x = cv.at<int32_t>(o->d_mem, 2); d.route = cv.at<int8_t>(o->d_mem, 3);
  trx_ctx_retain(c);
  *out = o;
  return TRXSIG_OK;
}

void trxsig_l1ciph_destroy(trxsig_l1ciph *o) {
  if (!o) return;
  trx_object_destroy(o->c, { o->d_mem });
  delete o;
}

int trxsig_l1ciph_channels(const trxsig_l1ciph *o, int cls) {
  return o && cls >= 0 && cls < o->plan.n_cls ? o->plan.n[cls] : TRXSIG_EINVAL;
}

int trxsig_l1ciph_channel(const trxsig_l1ciph *o, int cls, int chan, int *arfcn, int *tn, int *kind, int *sub) {
  return o ? o->plan.describe(o->plan.index(cls, chan), arfcn, tn, kind, sub) : TRXSIG_EINVAL;
}

int trxsig_l1ciph_set(trxsig_l1ciph *o, int cls, int chan, int algo, const uint8_t *h_kc) {
  if (!o) return TRXSIG_EINVAL;
  const int i = o->plan.index(cls, chan);
  if (i < 0) return fail(o, "trxsig_l1ciph_set: bad channel");
  if ((algo != TRXSIG_A5_OFF && algo != TRXSIG_A5_1) || (algo == TRXSIG_A5_1 && !h_kc))
    return fail(o, "trxsig_l1ciph_set: algo is 0 (off) or TRXSIG_A5_1 with a key");
  const TrxA5 key = algo == TRXSIG_A5_1 ? a5_key(h_kc) : TrxA5{ 0, 0, 0 };
  trxsig_ctx *c = o->c;
  TrxDeviceGuard g(trxsig_device(c));
  TRX_HIPCHK(c, trx_launch_l1ciph_set((hipStream_t)trxsig_get_stream(c), o->d_rec + i, (uint32_t)algo, key));
  return TRXSIG_OK;
}

int trxsig_l1ciph_state(trxsig_l1ciph *o, int cls, const uint32_t **d_state) {
  if (!o || !d_state || (cls != TRXSIG_L1_TCH && cls != TRXSIG_L1_XCCH)) return TRXSIG_EINVAL;
  *d_state = (const uint32_t *)(o->d_rec + o->plan.first[cls]);
  return TRXSIG_OK;
}

int trxsig_l1ciph_bits(trxsig_l1ciph *o, int uplink, int fn, int n_frames, uint8_t *d_bits, const uint8_t *d_what, uint32_t what_mask) {
  if (!o) return TRXSIG_EINVAL;
  if (!d_bits || ((uintptr_t)d_bits & 3) || (uplink != 0 && uplink != 1) || fn < 0 || fn >= kTrxHyperframe || n_frames < 1 ||
      8LL * n_frames * o->plan.A > kMaxSlots)
    return fail(o, "trxsig_l1ciph_bits: bad argument (4-byte aligned bits, uplink 0 / 1, fn in [0, 2715648), 1 <= n_frames, n_arfcn * 8 * n_frames <= 2^30)");
  trxsig_ctx *c = o->c;
  TrxCiphCall k{};
  k.uplink = uplink; k.fn = fn; k.n_frames = n_frames; k.n_arfcn = o->plan.A; k.what_mask = what_mask;
  TrxDeviceGuard g(trxsig_device(c));
  TRX_HIPCHK(c, trx_launch_l1ciph_bits((hipStream_t)trxsig_get_stream(c), k, o->dv, d_bits, d_what));
  return TRXSIG_OK;
}

int trxsig_l1ciph_soft(trxsig_l1ciph *o, int uplink, const trxsig_trxgroup_result *res, int fn) {
  if (!o) return TRXSIG_EINVAL;
  if (!res || (uplink != 0 && uplink != 1) || fn < 0 || fn >= kTrxHyperframe || res->n_arfcn != o->plan.A || res->n_slots <= 0 ||
      (res->n_slots & 7) || (long long)res->n_slots * o->plan.A > kMaxSlots || res->n_rows < 0 || !res->d_row ||
      (res->n_rows > 0 && (!res->d_valid || !res->d_soft || res->soft_stride < 148)))
    return fail(o, "trxsig_l1ciph_soft: bad argument (whole frames from TN 0 of the object's ARFCNs)");
  trxsig_ctx *c = o->c;
  TrxCiphCall k{};
  k.uplink = uplink; k.fn = fn; k.n_frames = res->n_slots / 8; k.n_arfcn = o->plan.A; k.n_rows = res->n_rows; k.soft_stride = res->soft_stride;
  TrxDeviceGuard g(trxsig_device(c));
  TRX_HIPCHK(c, trx_launch_l1ciph_soft((hipStream_t)trxsig_get_stream(c), k, o->dv, res->d_row, res->d_valid, const_cast<float *>(res->d_soft)));
  return TRXSIG_OK;
}
