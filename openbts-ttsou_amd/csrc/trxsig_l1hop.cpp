// trxsig_l1hop.cpp -- the hopping stage's host side (include/trxsig_l1hop.h): the plan and its rules (placement: trxsig_plan.h), the allocations of every
// (TN, group) on the device, the two object-owned index arrays, argument checks, and per call one launch on the context's stream
// (k_hop_mai, k_hop_map, k_hop_bits, k_hop_cells, k_hop_result).  The host keeps nothing between calls but the plan.
#include <hip/hip_runtime_api.h>

#include <new>
#include <vector>

#include "trxsig_ctx.h"
#include "trxsig_l1hop.h"
#include "trxsig_hop_dev.h"
#include "trxsig_plan.h"

static_assert(TRXSIG_L1HOP_MAX_N == kHopMaxN, "one limit");

struct trxsig_l1hop {
  trxsig_ctx *c = nullptr;
  int A = 0, G = 0, max_frames = 0;
  std::vector<uint8_t> count;           // [8][G]
  std::vector<int32_t> member;          // [8][G][64]
  void *d_mem = nullptr;
  int32_t *d_map = nullptr, *d_row = nullptr;   // [8 max_frames][A] each
  TrxHopDev dv{};
};

namespace {
constexpr long long kMaxSlots = 1LL << 30;

int fail(trxsig_l1hop *o, const char *what) { return trx_ctx_fail(o ? o->c : nullptr, TRXSIG_EINVAL, what, hipSuccess); }

bool call_ok(const trxsig_l1hop *o, int fn, int n_frames) {
  return fn >= 0 && fn < kTrxHyperframe && n_frames >= 1 && 8LL * n_frames * o->A <= kMaxSlots;
}
}  // namespace

int trxsig_hop_mai_batch(trxsig_ctx *c, int n, const int32_t *d_fn, const int32_t *d_hsn, const int32_t *d_maio, const int32_t *d_n,
                         int32_t *d_mai) {
  if (!c) return TRXSIG_EINVAL;
  if (n < 0 || n > (1 << 24) || (n > 0 && (!d_fn || !d_hsn || !d_maio || !d_n || !d_mai)))
    return trx_ctx_fail(c, TRXSIG_EINVAL, "trxsig_hop_mai_batch: bad argument (n in 0..2^24, four inputs and an output)", hipSuccess);
  if (n == 0) return TRXSIG_OK;
  TrxDeviceGuard g(trxsig_device(c));
  TRX_HIPCHK(c, trx_launch_hop_mai((hipStream_t)trxsig_get_stream(c), n, d_fn, d_hsn, d_maio, d_n, d_mai));
  return TRXSIG_OK;
}

int trxsig_l1hop_create(trxsig_l1hop **out, trxsig_ctx *c, int n_arfcn, const uint8_t *h_comb, const int8_t *h_group, int n_groups,
                        const uint8_t *h_hsn, int max_frames) {
  if (!out || !c) return TRXSIG_EINVAL;
  *out = nullptr;
  if (n_arfcn <= 0 || n_arfcn > 0xffff || !h_comb || !h_group || n_groups < 0 || n_groups > 128 || (n_groups > 0 && !h_hsn) ||
      max_frames < 1 || 8LL * max_frames * n_arfcn > kMaxSlots)
    return trx_ctx_fail(c, TRXSIG_EINVAL, "trxsig_l1hop_create: bad argument (n_arfcn in 1..65535, n_groups in 0..128, n_arfcn * 8 * max_frames in 8..2^30)", hipSuccess);
  for (int g = 0; g < n_groups; g++)
    if (h_hsn[g] > 63) return trx_ctx_fail(c, TRXSIG_EINVAL, "trxsig_l1hop_create: HSN outside 0..63", hipSuccess);
  const int A = n_arfcn, G = n_groups;
  std::vector<uint8_t> count((size_t)8 * (G ? G : 1), 0), comb_of((size_t)8 * (G ? G : 1), 0), rank((size_t)8 * A, 0);
  std::vector<int32_t> member((size_t)8 * (G ? G : 1) * kHopMaxN, 0);
  std::vector<int8_t> group((size_t)8 * A, -1);
  for (int a = 0; a < A; a++)                                // ascending a: a row's rank is the count before it
    for (int tn = 0; tn < 8; tn++) {
      const int k = h_comb[8 * a + tn], g = h_group[8 * a + tn];
      if (!trx_plan_slot_ok(k, a, tn))
        return trx_ctx_fail(c, TRXSIG_EINVAL, "trxsig_l1hop_create: unsupported channel combination or placement", hipSuccess);
      if (g < -1 || g >= G) return trx_ctx_fail(c, TRXSIG_EINVAL, "trxsig_l1hop_create: group id outside -1..n_groups-1", hipSuccess);
      if (g < 0) continue;
      if (k == 0 || k == 5)
        return trx_ctx_fail(c, TRXSIG_EINVAL, "trxsig_l1hop_create: an OFF slot or a beacon slot cannot hop", hipSuccess);
      const int gi = tn * G + g;
      if (count[gi] == kHopMaxN) return trx_ctx_fail(c, TRXSIG_EINVAL, "trxsig_l1hop_create: more than 64 rows in one allocation", hipSuccess);
      if (count[gi] > 0 && comb_of[gi] != k)
        return trx_ctx_fail(c, TRXSIG_EINVAL, "trxsig_l1hop_create: the members of one allocation differ in their combination", hipSuccess);
      comb_of[gi] = (uint8_t)k;
      group[(size_t)tn * A + a] = (int8_t)g;
      rank[(size_t)tn * A + a] = count[gi];
      member[(size_t)gi * kHopMaxN + count[gi]++] = a;
    }
  trxsig_l1hop *o = new (std::nothrow) trxsig_l1hop;
  if (!o) return TRXSIG_ENOMEM;
  o->c = c; o->A = A; o->G = G; o->max_frames = max_frames;
  o->count = count; o->member = member;
  const size_t rows = (size_t)8 * max_frames * A * sizeof(int32_t);
  const TrxCarve cv = { group.size(), rank.size(), count.size(), member.size() * 4, (size_t)(G ? G : 1), rows, rows };
  TrxDeviceGuard g(trxsig_device(c));
  const int rc = trx_device_block(c, "trxsig_l1hop_create", cv.total,
                                  { { cv.off[0], group.data(), group.size() }, { cv.off[1], rank.data(), rank.size() },
                                    { cv.off[2], count.data(), count.size() }, { cv.off[3], member.data(), member.size() * 4 },
                                    { cv.off[4], h_hsn, (size_t)G } }, &o->d_mem);
  if (rc != TRXSIG_OK) { delete o; return rc; }
  void *b = o->d_mem;
  TrxHopDev &d = o->dv;
  d.n_arfcn = A; d.n_groups = G;
  d.group = cv.at<int8_t>(b, 0); d.rank = cv.at<uint8_t>(b, 1); d.count = cv.at<uint8_t>(b, 2);
  d.member = cv.at<int32_t>(b, 3); d.hsn = cv.at<uint8_t>(b, 4);
  o->d_map = cv.at<int32_t>(b, 5); o->d_row = cv.at<int32_t>(b, 6);
  trx_ctx_retain(c);
  *out = o;
  return TRXSIG_OK;
}

void trxsig_l1hop_destroy(trxsig_l1hop *o) {
  if (!o) return;
  trx_object_destroy(o->c, { o->d_mem });
  delete o;
}

int trxsig_l1hop_groups(const trxsig_l1hop *o) { return o ? o->G : TRXSIG_EINVAL; }

int trxsig_l1hop_members(const trxsig_l1hop *o, int g, int tn, int32_t *h_rows) {
  if (!o || g < 0 || g >= o->G || tn < 0 || tn > 7) return TRXSIG_EINVAL;
  const int gi = tn * o->G + g, n = o->count[gi];
  if (h_rows)
    for (int r = 0; r < n; r++) h_rows[r] = o->member[(size_t)gi * kHopMaxN + r];
  return n;
}

int trxsig_l1hop_map(trxsig_l1hop *o, int fn, int n_frames, const int32_t **d_radio) {
  if (!o) return TRXSIG_EINVAL;
  if (!d_radio || !call_ok(o, fn, n_frames) || n_frames > o->max_frames)
    return fail(o, "trxsig_l1hop_map: bad argument (fn in [0, 2715648), 1 <= n_frames <= max_frames)");
  trxsig_ctx *c = o->c;
  TrxDeviceGuard g(trxsig_device(c));
  TRX_HIPCHK(c, trx_launch_hop_map((hipStream_t)trxsig_get_stream(c), o->dv, fn, n_frames, nullptr, o->d_map));
  *d_radio = o->d_map;
  return TRXSIG_OK;
}

int trxsig_l1hop_bits(trxsig_l1hop *o, int to_radio, int fn, int n_frames, uint8_t *d_bits, uint8_t *d_what) {
  if (!o) return TRXSIG_EINVAL;
  if (!d_bits || ((uintptr_t)d_bits & 3) || !call_ok(o, fn, n_frames))
    return fail(o, "trxsig_l1hop_bits: bad argument (4-byte aligned bits, fn in [0, 2715648), 1 <= n_frames, n_arfcn * 8 * n_frames <= 2^30)");
  trxsig_ctx *c = o->c;
  TrxDeviceGuard g(trxsig_device(c));
  TRX_HIPCHK(c, trx_launch_hop_bits((hipStream_t)trxsig_get_stream(c), o->dv, to_radio != 0, fn, n_frames, d_bits, d_what));
  return TRXSIG_OK;
}

int trxsig_l1hop_cells(trxsig_l1hop *o, int to_radio, int fn, int n_frames, const trxsig_c32 *d_in, int64_t in_slot, int64_t in_arfcn,
                       trxsig_c32 *d_out, int64_t out_slot, int64_t out_arfcn) {
  if (!o) return TRXSIG_EINVAL;
  if (!d_in || !d_out || !call_ok(o, fn, n_frames))
    return fail(o, "trxsig_l1hop_cells: bad argument (buffers, fn in [0, 2715648), 1 <= n_frames, n_arfcn * 8 * n_frames <= 2^30)");
  trxsig_ctx *c = o->c;
  const int sps = trxsig_sps(c);
  const long long T = 8LL * n_frames, A = o->A, cell = 157LL * sps;
  long long in_n = 0, out_n = 0;
  if (!strides_ok(T, A, cell, in_slot, in_arfcn) || !strides_ok(T, A, cell, out_slot, out_arfcn) ||
      !extent(T, A, cell, in_slot, in_arfcn, &in_n) || !extent(T, A, cell, out_slot, out_arfcn, &out_n))
    return fail(o, "trxsig_l1hop_cells: the strides let cells overlap");
  if (overlap(d_in, in_n, d_out, out_n)) return fail(o, "trxsig_l1hop_cells: out overlaps in (the move is out of place)");
  TrxHopCells k{};
  k.in = (const float2 *)d_in; k.out = (float2 *)d_out;
  k.in_slot = in_slot; k.in_arfcn = in_arfcn; k.out_slot = out_slot; k.out_arfcn = out_arfcn;
  k.fn = fn; k.n_frames = n_frames; k.to_radio = to_radio != 0; k.sps = sps;
  // 16 bytes a lane where every cell start of both buffers is 16-byte aligned: the bases, and strides of an even number of samples
  const bool wide = (((uintptr_t)d_in | (uintptr_t)d_out) & 15) == 0 && ((in_slot | in_arfcn | out_slot | out_arfcn) & 1) == 0;
  TrxDeviceGuard g(trxsig_device(c));
  TRX_HIPCHK(c, trx_launch_hop_cells((hipStream_t)trxsig_get_stream(c), o->dv, k, wide));
  return TRXSIG_OK;
}

int trxsig_l1hop_result(trxsig_l1hop *o, int fn, const trxsig_trxgroup_result *res, trxsig_trxgroup_result *out) {
  if (!o) return TRXSIG_EINVAL;
  if (!res || !out || fn < 0 || fn >= kTrxHyperframe || res->n_arfcn != o->A || res->n_slots <= 0 || (res->n_slots & 7) ||
      res->n_slots / 8 > o->max_frames || !res->d_row)
    return fail(o, "trxsig_l1hop_result: bad argument (whole frames from TN 0 of the object's ARFCNs, at most max_frames)");
  trxsig_ctx *c = o->c;
  TrxDeviceGuard g(trxsig_device(c));
  TRX_HIPCHK(c, trx_launch_hop_map((hipStream_t)trxsig_get_stream(c), o->dv, fn, res->n_slots / 8, res->d_row, o->d_row));
  *out = *res;
  out->d_row = o->d_row;
  return TRXSIG_OK;
}
