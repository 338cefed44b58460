// trxsig_l1ciph.cpp -- the ciphering stage's host side (include/trxsig_l1ciph.h): the channel plan (trxsig_l1rx_create's rules
// and numbering), the slot-owner table of both directions from the mappings of trxsig_tdma.h, the channels' records on the device,
// the 64 key steps of a key change, argument checks, and per call one launch on the context's stream (k_a5_blocks, k_l1ciph_set,
// k_l1ciph_bits, k_l1ciph_soft).  The host keeps nothing between calls but the plan.
#include <hip/hip_runtime_api.h>

#include <new>
#include <vector>

#include "trxsig_ctx.h"
#include "trxsig_l1ciph.h"
#include "trxsig_a5_dev.h"
#include "trxsig_tdma.h"

namespace {
const TrxTdmaMap kUl[TRX_N_MAPS] = TRX_TDMA_MAPS_INIT;
const TrxTdmaMap kDl[TRX_N_DL_MAPS] = TRX_TDMA_DL_MAPS_INIT;

void map_kind(int m, int *kind, int *sub) {   // TRXSIG_L1_* kind and sub-channel of a mapping id below TRX_MAP_RACH_C5
  static const int first[] = { TRX_MAP_TCHF, TRX_MAP_SACCH_TF, TRX_MAP_SDCCH8, TRX_MAP_SACCH_C8, TRX_MAP_SDCCH4, TRX_MAP_SACCH_C4 };
  int k = 5;
  while (m < first[k]) k--;
  *kind = k;
  *sub = (k == TRXSIG_L1_SACCH_TF) ? 0 : m - first[k];
}
inline size_t al(size_t x) { return (x + 255) & ~(size_t)255; }
constexpr long long kMaxSlots = 1LL << 30;
}  // namespace

struct trxsig_l1ciph {
  trxsig_ctx *c = nullptr;
  int A = 0, n_tch = 0, n_xcch = 0;
  std::vector<int32_t> chinfo;          // arfcn | tn << 16 | map << 20: TCH, then XCCH
  void *d_mem = nullptr;
  TrxCiphRec *d_rec = nullptr;
  TrxCiphDev dv{};
};

namespace {
int fail(trxsig_l1ciph *o, const char *what) { return trx_ctx_fail(o ? o->c : nullptr, TRXSIG_EINVAL, what, hipSuccess); }

int chan_index(const trxsig_l1ciph *o, int cls, int chan) {   // index into the records, or -1
  if (cls == TRXSIG_L1_TCH && chan >= 0 && chan < o->n_tch) return chan;
  if (cls == TRXSIG_L1_XCCH && chan >= 0 && chan < o->n_xcch) return o->n_tch + chan;
  return -1;
}
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
  for (int a = 0; a < n_arfcn; a++)
    for (int tn = 0; tn < 8; tn++) {
      const int k = h_comb[8 * a + tn];
      if (!(k == 0 || k == 1 || k == 7 || (k == 5 && a == 0 && tn == 0)))
        return trx_ctx_fail(c, TRXSIG_EINVAL, "trxsig_l1ciph_create: unsupported channel combination or placement", hipSuccess);
    }
  trxsig_l1ciph *o = new (std::nothrow) trxsig_l1ciph;
  if (!o) return TRXSIG_ENOMEM;
  o->c = c; o->A = n_arfcn;
  std::vector<int32_t> tch, xcch;
  auto info = [](int a, int tn, int m) { return (int32_t)(a | tn << 16 | m << 20); };
  const size_t S = 8 * (size_t)n_arfcn;
  std::vector<int32_t> slot(S, 0), slot_x(S, 0);
  for (int a = 0; a < n_arfcn; a++)
    for (int tn = 0; tn < 8; tn++) {
      const int k = h_comb[8 * a + tn];
      slot_x[8 * a + tn] = (int32_t)xcch.size();             // XCCH index; made an index into the records below
      slot[8 * a + tn] = k | (int32_t)tch.size() << 4;
      switch (k) {
        case 1:
          tch.push_back(info(a, tn, TRX_MAP_TCHF));
          xcch.push_back(info(a, tn, TRX_MAP_SACCH_TF + tn));
          break;
        case 5:
          for (int s = 0; s < 4; s++) xcch.push_back(info(a, tn, TRX_MAP_SDCCH4 + s));
          for (int s = 0; s < 4; s++) xcch.push_back(info(a, tn, TRX_MAP_SACCH_C4 + s));
          break;
        case 7:
          for (int s = 0; s < 8; s++) xcch.push_back(info(a, tn, TRX_MAP_SDCCH8 + s));
          for (int s = 0; s < 8; s++) xcch.push_back(info(a, tn, TRX_MAP_SACCH_C8 + s));
          break;
        default: break;
      }
    }
  o->n_tch = (int)tch.size(); o->n_xcch = (int)xcch.size();
  o->chinfo = tch;
  o->chinfo.insert(o->chinfo.end(), xcch.begin(), xcch.end());
  for (int32_t &x : slot_x) x += o->n_tch;
  // the slot owners: [downlink / uplink][combination I / V / VII][TN][fn mod 104 (I) or 102 (V, VII)] -> -1, 0 (the TCH) or
  // 1 + the XCCH channel's place among the slot's.  Ids 0..32 name the same logical channels in both directions' tables.
  std::vector<int8_t> route(2 * 3 * 8 * 104, -1);
  bool disjoint = true;
  for (int dir = 0; dir < 2; dir++)
    for (int ci = 0; ci < 3; ci++)
      for (int tn = 0; tn < 8; tn++) {
        std::vector<std::pair<int, int>> ms;                 // (mapping, code)
        if (ci == 0) { ms.push_back({ TRX_MAP_TCHF, 0 }); ms.push_back({ TRX_MAP_SACCH_TF + tn, 1 }); }
        const int ns = ci == 1 ? 4 : 8;
        if (ci == 1) for (int s = 0; s < ns; s++) { ms.push_back({ TRX_MAP_SDCCH4 + s, 1 + s }); ms.push_back({ TRX_MAP_SACCH_C4 + s, 1 + ns + s }); }
        if (ci == 2) for (int s = 0; s < ns; s++) { ms.push_back({ TRX_MAP_SDCCH8 + s, 1 + s }); ms.push_back({ TRX_MAP_SACCH_C8 + s, 1 + ns + s }); }
        const int L = ci == 0 ? 104 : 102;
        for (const auto &mc : ms) {
          const TrxTdmaMap &M = dir ? kUl[mc.first] : kDl[mc.first];
          for (int r = 0; r < L; r++)
            for (int i = 0; i < M.n; i++)
              if (r % M.R == M.f[i]) {
                int8_t &w = route[(size_t)((dir * 3 + ci) * 8 + tn) * 104 + r];
                if (w >= 0) disjoint = false;
                w = (int8_t)mc.second;
              }
        }
      }
  const size_t N = o->chinfo.size();
  const size_t sz[] = { (N + 1) * sizeof(TrxCiphRec), S * 4, S * 4, route.size() };
  constexpr int nsz = sizeof sz / sizeof sz[0];
  size_t off[nsz], total = 0;
  for (int i = 0; i < nsz; i++) { off[i] = total; total += al(sz[i]); }
  TrxDeviceGuard g(trxsig_device(c));
  if (!disjoint || hipMalloc(&o->d_mem, total) != hipSuccess) {
    delete o;
    return trx_ctx_fail(c, disjoint ? TRXSIG_ENOMEM : TRXSIG_EINVAL, "trxsig_l1ciph_create: device allocation", hipSuccess);
  }
  char *b = (char *)o->d_mem;
  o->d_rec = (TrxCiphRec *)(b + off[0]);
  TrxCiphDev &d = o->dv;
  d.rec = o->d_rec; d.slot = (const int32_t *)(b + off[1]); d.slot_x = (const int32_t *)(b + off[2]); d.route = (const int8_t *)(b + off[3]);
  hipError_t e = hipMemset(o->d_mem, 0, total);              // every channel off
  if (e == hipSuccess) e = hipMemcpy(b + off[1], slot.data(), S * 4, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(b + off[2], slot_x.data(), S * 4, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(b + off[3], route.data(), route.size(), hipMemcpyHostToDevice);
  if (e != hipSuccess) {
    (void)hipFree(o->d_mem);
    delete o;
    return trx_ctx_fail(c, TRXSIG_EHIP, "trxsig_l1ciph_create: upload", e);
  }
  trx_ctx_retain(c);
  *out = o;
  return TRXSIG_OK;
}

void trxsig_l1ciph_destroy(trxsig_l1ciph *o) {
  if (!o) return;
  {
    TrxDeviceGuard g(trxsig_device(o->c));
    (void)hipStreamSynchronize((hipStream_t)trxsig_get_stream(o->c));
    if (o->d_mem) (void)hipFree(o->d_mem);
  }
  trx_ctx_release(o->c);
  delete o;
}

int trxsig_l1ciph_channels(const trxsig_l1ciph *o, int cls) {
  if (!o) return TRXSIG_EINVAL;
  return cls == TRXSIG_L1_TCH ? o->n_tch : cls == TRXSIG_L1_XCCH ? o->n_xcch : TRXSIG_EINVAL;
}

int trxsig_l1ciph_channel(const trxsig_l1ciph *o, int cls, int chan, int *arfcn, int *tn, int *kind, int *sub) {
  if (!o) return TRXSIG_EINVAL;
  const int i = chan_index(o, cls, chan);
  if (i < 0) return TRXSIG_EINVAL;
  const int32_t v = o->chinfo[i];
  int k = 0, s = 0;
  map_kind(v >> 20, &k, &s);
  if (arfcn) *arfcn = v & 0xffff;
  if (tn) *tn = (v >> 16) & 15;
  if (kind) *kind = k;
  if (sub) *sub = s;
  return TRXSIG_OK;
}

int trxsig_l1ciph_set(trxsig_l1ciph *o, int cls, int chan, int algo, const uint8_t *h_kc) {
  if (!o) return TRXSIG_EINVAL;
  const int i = chan_index(o, cls, chan);
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
  *d_state = (const uint32_t *)(o->d_rec + (cls == TRXSIG_L1_TCH ? 0 : o->n_tch));
  return TRXSIG_OK;
}

int trxsig_l1ciph_bits(trxsig_l1ciph *o, int uplink, int fn, int n_frames, uint8_t *d_bits, const uint8_t *d_what, uint32_t what_mask) {
  if (!o) return TRXSIG_EINVAL;
  if (!d_bits || ((uintptr_t)d_bits & 3) || (uplink != 0 && uplink != 1) || fn < 0 || fn >= kTrxHyperframe || n_frames < 1 ||
      8LL * n_frames * o->A > kMaxSlots)
    return fail(o, "trxsig_l1ciph_bits: bad argument (4-byte aligned bits, uplink 0 / 1, fn in [0, 2715648), 1 <= n_frames, n_arfcn * 8 * n_frames <= 2^30)");
  trxsig_ctx *c = o->c;
  TrxCiphCall k{};
  k.uplink = uplink; k.fn = fn; k.n_frames = n_frames; k.n_arfcn = o->A; k.what_mask = what_mask;
  TrxDeviceGuard g(trxsig_device(c));
  TRX_HIPCHK(c, trx_launch_l1ciph_bits((hipStream_t)trxsig_get_stream(c), k, o->dv, d_bits, d_what));
  return TRXSIG_OK;
}

int trxsig_l1ciph_soft(trxsig_l1ciph *o, int uplink, const trxsig_trxgroup_result *res, int fn) {
  if (!o) return TRXSIG_EINVAL;
  if (!res || (uplink != 0 && uplink != 1) || fn < 0 || fn >= kTrxHyperframe || res->n_arfcn != o->A || res->n_slots <= 0 ||
      (res->n_slots & 7) || (long long)res->n_slots * o->A > kMaxSlots || res->n_rows < 0 || !res->d_row ||
      (res->n_rows > 0 && (!res->d_valid || !res->d_soft || res->soft_stride < 148)))
    return fail(o, "trxsig_l1ciph_soft: bad argument (whole frames from TN 0 of the object's ARFCNs)");
  trxsig_ctx *c = o->c;
  TrxCiphCall k{};
  k.uplink = uplink; k.fn = fn; k.n_frames = res->n_slots / 8; k.n_arfcn = o->A; k.n_rows = res->n_rows; k.soft_stride = res->soft_stride;
  TrxDeviceGuard g(trxsig_device(c));
  TRX_HIPCHK(c, trx_launch_l1ciph_soft((hipStream_t)trxsig_get_stream(c), k, o->dv, res->d_row, res->d_valid, const_cast<float *>(res->d_soft)));
  return TRXSIG_OK;
}
