// trxsig_l1tx.cpp -- the downlink L1 multiplexer's host side (include/trxsig_l1tx.h): the channel plan, the slot-owner tables
// the mux reads, the channels' records on the device (two copies: a call reads one and commits the other), and per call the
// block geometry of every mapping and three launches on the context's stream: k_l1tx_encode, k_l1tx_mux, k_l1tx_commit.
#include <hip/hip_runtime_api.h>

#include <cstring>
#include <vector>

#include "trxsig_ctx.h"
#include "trxsig_l1tx.h"
#include "trxsig_l1ms_dev.h"

namespace {
const TrxTdmaMap kDl[TRX_N_DL_MAPS] = TRX_TDMA_DL_MAPS_INIT;

void map_kind(int m, int *kind, int *sub) {   // TRXSIG_L1_* kind and sub-channel of a downlink mapping id
  if (m >= TRX_DL_CCCH && m < TRX_DL_BCCH) { *kind = TRXSIG_L1_CCCH_C5; *sub = m - TRX_DL_CCCH; return; }
  static const int first[] = { TRX_MAP_TCHF, TRX_MAP_SACCH_TF, TRX_MAP_SDCCH8, TRX_MAP_SACCH_C8, TRX_MAP_SDCCH4, TRX_MAP_SACCH_C4 };
  int k = 5;
  while (m < first[k]) k--;
  *kind = k;
  *sub = (k == TRXSIG_L1_SACCH_TF) ? 0 : m - first[k];
}
bool map_sacch(int m) {
  int k = 0, s = 0;
  map_kind(m, &k, &s);
  return k == TRXSIG_L1_SACCH_TF || k == TRXSIG_L1_SACCH_C8 || k == TRXSIG_L1_SACCH_C4;
}
bool maps_ordered() {
  for (const TrxTdmaMap &m : kDl)
    for (int r = 1; r < m.n; r++)
      if ((m.f[r] - m.f[0] + m.R) % m.R <= (m.f[r - 1] - m.f[0] + m.R) % m.R) return false;
  return true;
}
inline size_t al(size_t x) { return (x + 255) & ~(size_t)255; }
inline long long ceil4(long long p) { return -trx_fdiv(-p, 4); }
constexpr long long kMaxOutBytes = 1LL << 34;
}  // namespace

struct trxsig_l1tx {
  trxsig_ctx *c = nullptr;
  int A = 0, bsic = 0, band = 0;
  float target = 0.0F;
  int n[4] = {};                        // TCH, XCCH, CCCH, BCCH
  int n_all = 0, cur = 0;
  std::vector<int32_t> chinfo;          // arfcn | tn << 16 | map << 20
  std::vector<uint8_t> comb;
  bool used[4][TRX_N_DL_MAPS] = {};
  void *d_persist = nullptr;
  TrxL1txChan *d_st = nullptr;
  uint8_t *d_si = nullptr;
  void *d_work = nullptr;
  size_t work_bytes = 0;
  TrxL1txDev dv{};
  int last_fn = -1, last_F = 0;         // the last encode (datagrams)
  int32_t *d_wgc = nullptr;             // its workspace's datagram counts [8 F][ceil(A / 256)] + total
  void *d_dg = nullptr;
  size_t dg_bytes = 0;
};

namespace {
int fail(trxsig_l1tx *l1, const char *what) { return trx_ctx_fail(l1 ? l1->c : nullptr, TRXSIG_EINVAL, what, hipSuccess); }

int chan_index(const trxsig_l1tx *l1, int cls, int chan) {
  int off = 0;
  for (int k = 0; k < 3; k++) {
    if (cls == k) return (chan >= 0 && chan < l1->n[k]) ? off + chan : -1;
    off += l1->n[k];
  }
  return -1;
}

int set_active(trxsig_l1tx *l1, int cls, int chan, int open) {
  if (!l1) return TRXSIG_EINVAL;
  const int g = chan_index(l1, cls, chan);
  if (g < 0) return fail(l1, "trxsig_l1tx_open / _close: bad channel");
  trxsig_ctx *c = l1->c;
  TrxDeviceGuard gd(trxsig_device(c));
  const int m = l1->chinfo[g] >> 20;
  TRX_HIPCHK(c, trx_launch_l1tx_set((hipStream_t)trxsig_get_stream(c), l1->d_st + (size_t)l1->cur * l1->n_all + g, open,
                                    map_sacch(m) && cls == TRXSIG_L1_XCCH, kDl[m].n));
  return TRXSIG_OK;
}

// block geometry of a call
void geometry(const trxsig_l1tx *l1, int fn, int F, TrxL1txCall &k) {
  std::memset(&k, 0, sizeof k);
  k.fn = fn; k.n_frames = F; k.n_arfcn = l1->A;
  k.n_tch = l1->n[0]; k.n_xcch = l1->n[1]; k.n_ccch = l1->n[2]; k.n_bcch = l1->n[3]; k.n_all = l1->n_all;
  k.r104 = fn % 104; k.r102 = fn % 102; k.r51 = fn % 51; k.r26 = fn % 26;
  k.cur = l1->cur; k.band = l1->band; k.bsic = l1->bsic; k.rssi_target = l1->target;
  for (int m = 0; m < TRX_N_DL_MAPS; m++) {
    const TrxTdmaMap &M = kDl[m];
    k.p_first[m] = trx_map_count(M, fn);
    k.p_end[m] = trx_map_count(M, (long long)fn + F);
    int below = 0;
    for (int r = 0; r < M.n; r++) below += M.f[r] < fn % M.R;
    k.base[m] = k.p_first[m] - below;
    const long long nb = ceil4(k.p_end[m]) - ceil4(k.p_first[m]);
    for (int cl = 0; cl < 4; cl++)
      if (l1->used[cl][m] && nb > k.nb[cl]) k.nb[cl] = (int)nb;
  }
  long long u = 0;
  for (int cl = 0; cl < 4; cl++) { k.unit0[cl] = u; u += (long long)l1->n[cl] * k.nb[cl]; }
}
}  // namespace

int trxsig_l1tx_create(trxsig_l1tx **out, trxsig_ctx *c, int n_arfcn, const uint8_t *h_comb, int bsic, int band, float target) {
  if (!out || !c) return TRXSIG_EINVAL;
  *out = nullptr;
  const int bidx = (band == 850 || band == 900) ? 0 : band == 1800 ? 1 : band == 1900 ? 2 : -1;
  if (n_arfcn <= 0 || n_arfcn > 0xffff || !h_comb || bsic < 0 || bsic > 63 || bidx < 0 || !maps_ordered() || !(target == target))
    return trx_ctx_fail(c, TRXSIG_EINVAL, "trxsig_l1tx_create: bad argument", hipSuccess);
  for (int a = 0; a < n_arfcn; a++)
    for (int tn = 0; tn < 8; tn++) {
      const int k = h_comb[8 * a + tn];
      if (!(k == 0 || k == 1 || k == 7 || (k == 5 && a == 0 && tn == 0)))
        return trx_ctx_fail(c, TRXSIG_EINVAL, "trxsig_l1tx_create: unsupported channel combination or placement", hipSuccess);
    }
  trxsig_l1tx *l1 = new (std::nothrow) trxsig_l1tx;
  if (!l1) return TRXSIG_ENOMEM;
  l1->c = c; l1->A = n_arfcn; l1->bsic = bsic; l1->band = bidx; l1->target = target;
  l1->comb.assign(h_comb, h_comb + 8 * (size_t)n_arfcn);
  std::vector<int32_t> cl[4];
  auto info = [](int a, int tn, int m) { return (int32_t)(a | tn << 16 | m << 20); };
  std::vector<int32_t> slot(8 * (size_t)n_arfcn, 0), slot_x(8 * (size_t)n_arfcn, 0);
  for (int a = 0; a < n_arfcn; a++)
    for (int tn = 0; tn < 8; tn++) {
      const int k = h_comb[8 * a + tn];
      slot_x[8 * a + tn] = (int32_t)cl[1].size();    // XCCH index; made global below
      slot[8 * a + tn] = k | (int32_t)cl[0].size() << 4;
      switch (k) {
        case 1:
          cl[0].push_back(info(a, tn, TRX_MAP_TCHF));
          cl[1].push_back(info(a, tn, TRX_MAP_SACCH_TF + tn));
          break;
        case 5:
          for (int s = 0; s < 4; s++) cl[1].push_back(info(a, tn, TRX_MAP_SDCCH4 + s));
          for (int s = 0; s < 4; s++) cl[1].push_back(info(a, tn, TRX_MAP_SACCH_C4 + s));
          for (int s = 0; s < 3; s++) cl[2].push_back(info(a, tn, TRX_DL_CCCH + s));
          cl[3].push_back(info(a, tn, TRX_DL_BCCH));
          break;
        case 7:
          for (int s = 0; s < 8; s++) cl[1].push_back(info(a, tn, TRX_MAP_SDCCH8 + s));
          for (int s = 0; s < 8; s++) cl[1].push_back(info(a, tn, TRX_MAP_SACCH_C8 + s));
          break;
        default: break;
      }
    }
  for (int k = 0; k < 4; k++) {
    l1->n[k] = (int)cl[k].size();
    l1->chinfo.insert(l1->chinfo.end(), cl[k].begin(), cl[k].end());
    for (int32_t v : cl[k]) l1->used[k][v >> 20] = true;
  }
  l1->n_all = (int)l1->chinfo.size();
  for (int32_t &x : slot_x) x += l1->n[0];
  // the slot owners: [combination I / V / VII][TN][fn mod 104 (I) or 102 (V, VII)]
  std::vector<int8_t> writer(3 * 8 * 104, -1);
  std::vector<int> maps[3];
  maps[0] = { TRX_MAP_TCHF };
  for (int s = 0; s < 4; s++) { maps[1].push_back(TRX_MAP_SDCCH4 + s); maps[1].push_back(TRX_MAP_SACCH_C4 + s); }
  for (int s = 0; s < 3; s++) maps[1].push_back(TRX_DL_CCCH + s);
  maps[1].insert(maps[1].end(), { TRX_DL_BCCH, TRX_DL_SCH, TRX_DL_FCCH });
  for (int s = 0; s < 8; s++) { maps[2].push_back(TRX_MAP_SDCCH8 + s); maps[2].push_back(TRX_MAP_SACCH_C8 + s); }
  bool disjoint = true;
  for (int ci = 0; ci < 3; ci++)
    for (int tn = 0; tn < 8; tn++) {
      std::vector<int> ms = maps[ci];
      if (ci == 0) ms.push_back(TRX_MAP_SACCH_TF + tn);
      const int L = ci == 0 ? 104 : 102;
      for (int m : ms)
        for (int r = 0; r < L; r++)
          for (int i = 0; i < kDl[m].n; i++)
            if (r % kDl[m].R == kDl[m].f[i]) {
              int8_t &w = writer[(ci * 8 + tn) * 104 + r];
              if (w >= 0) disjoint = false;
              w = (int8_t)m;
            }
    }
  std::vector<int16_t> cnt(TRX_N_DL_MAPS * 105, 0);
  for (int m = 0; m < TRX_N_DL_MAPS; m++)
    for (int x = 0; x <= kDl[m].R; x++) {
      int v = 0;
      for (int i = 0; i < kDl[m].n; i++) v += kDl[m].f[i] < x;
      cnt[m * 105 + x] = (int16_t)v;
    }
  const size_t N = (size_t)l1->n_all, S = 8 * (size_t)n_arfcn;
  std::vector<TrxL1txChan> rec(2 * N);
  std::memset(rec.data(), 0, rec.size() * sizeof(TrxL1txChan));
  for (size_t i = 0; i < 2 * N; i++) {
    const int g = (int)(i % N), m = l1->chinfo[g] >> 20;
    const bool sacch = g >= l1->n[0] && g < l1->n[0] + l1->n[1] && map_sacch(m);
    rec[i].active = 1;
    rec[i].ord_pow = sacch ? 40 : -1;
    rec[i].ord_ta = sacch ? 0.0F : -1.0F;
  }
  const size_t sz[] = { 2 * N * sizeof(TrxL1txChan), N * 4, S * 4, S * 4, writer.size(), cnt.size() * 2, 96 };
  constexpr int nsz = sizeof sz / sizeof sz[0];
  size_t off[nsz], total = 0;
  for (int i = 0; i < nsz; i++) { off[i] = total; total += al(sz[i]); }
  TrxDeviceGuard gd(trxsig_device(c));
  if (!disjoint || hipMalloc(&l1->d_persist, total) != hipSuccess) {
    delete l1;
    return trx_ctx_fail(c, disjoint ? TRXSIG_ENOMEM : TRXSIG_EINVAL, "trxsig_l1tx_create: device allocation", hipSuccess);
  }
  char *b = (char *)l1->d_persist;
  TrxL1txDev &d = l1->dv;
  l1->d_st = (TrxL1txChan *)(b + off[0]);
  d.st = l1->d_st; d.chinfo = (const int32_t *)(b + off[1]); d.slot = (const int32_t *)(b + off[2]);
  d.slot_x = (const int32_t *)(b + off[3]); d.writer = (const int8_t *)(b + off[4]); d.cnt = (const int16_t *)(b + off[5]);
  l1->d_si = (uint8_t *)(b + off[6]); d.si = l1->d_si;
  hipError_t e = hipMemset(l1->d_persist, 0, total);
  if (e == hipSuccess && N) e = hipMemcpy(l1->d_st, rec.data(), 2 * N * sizeof(TrxL1txChan), hipMemcpyHostToDevice);
  if (e == hipSuccess && N) e = hipMemcpy(b + off[1], l1->chinfo.data(), N * 4, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(b + off[2], slot.data(), S * 4, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(b + off[3], slot_x.data(), S * 4, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(b + off[4], writer.data(), writer.size(), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(b + off[5], cnt.data(), cnt.size() * 2, hipMemcpyHostToDevice);
  d.filler = trx_ctx_tch_filler(c);
  if (e != hipSuccess || !d.filler) {
    (void)hipFree(l1->d_persist);
    delete l1;
    return trx_ctx_fail(c, TRXSIG_EHIP, "trxsig_l1tx_create: upload", e);
  }
  trx_ctx_retain(c);
  *out = l1;
  return TRXSIG_OK;
}

void trxsig_l1tx_destroy(trxsig_l1tx *l1) {
  if (!l1) return;
  {
    TrxDeviceGuard g(trxsig_device(l1->c));
    (void)hipStreamSynchronize((hipStream_t)trxsig_get_stream(l1->c));
    if (l1->d_work) (void)hipFree(l1->d_work);
    if (l1->d_dg) (void)hipFree(l1->d_dg);
    if (l1->d_persist) (void)hipFree(l1->d_persist);
  }
  trx_ctx_release(l1->c);
  delete l1;
}

int trxsig_l1tx_channels(const trxsig_l1tx *l1, int cls) {
  if (!l1 || cls < 0 || cls > 3 || cls == TRXSIG_L1_RACH) return TRXSIG_EINVAL;
  return l1->n[cls == TRXSIG_L1_CCCH ? 2 : cls];
}

int trxsig_l1tx_channel(const trxsig_l1tx *l1, int cls, int chan, int *arfcn, int *tn, int *kind, int *sub) {
  if (!l1) return TRXSIG_EINVAL;
  const int g = chan_index(l1, cls == TRXSIG_L1_CCCH ? 2 : cls == 2 ? -1 : cls, chan);
  if (g < 0) return TRXSIG_EINVAL;
  const int32_t v = l1->chinfo[g];
  int k = 0, s = 0;
  map_kind(v >> 20, &k, &s);
  if (arfcn) *arfcn = v & 0xffff;
  if (tn) *tn = (v >> 16) & 15;
  if (kind) *kind = k;
  if (sub) *sub = s;
  return TRXSIG_OK;
}

int trxsig_l1tx_open(trxsig_l1tx *l1, int cls, int chan) {
  return set_active(l1, cls == TRXSIG_L1_CCCH ? 2 : cls == 2 ? -1 : cls, chan, 1);
}
int trxsig_l1tx_close(trxsig_l1tx *l1, int cls, int chan) {
  return set_active(l1, cls == TRXSIG_L1_CCCH ? 2 : cls == 2 ? -1 : cls, chan, 0);
}

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
  const int k = cls == TRXSIG_L1_CCCH ? 2 : (cls == TRXSIG_L1_TCH || cls == TRXSIG_L1_XCCH) ? cls : -1;
  if (k < 0) return TRXSIG_EINVAL;
  int off = 0;
  for (int i = 0; i < k; i++) off += l1->n[i];
  *d_state = (void *)(l1->d_st + (size_t)l1->cur * l1->n_all + off);
  return TRXSIG_OK;
}

int trxsig_l1tx_encode(trxsig_l1tx *l1, int fn, int F, const trxsig_l1tx_in *in, const trxsig_l1rx *sib, trxsig_l1tx_out *out) {
  if (!l1) return TRXSIG_EINVAL;
  if (!in || !out || fn < 0 || fn >= kTrxHyperframe || F <= 0)
    return fail(l1, "trxsig_l1tx_encode: bad argument (fn in [0, 2715648), n_frames > 0)");
  if ((long long)l1->A * 8 * 148 * F > kMaxOutBytes) return fail(l1, "trxsig_l1tx_encode: output above 2^34 bytes");
  if ((l1->n[0] && (!in->d_tch_kind || !in->d_tch_payload)) || (l1->n[1] && (!in->d_xcch_kind || !in->d_xcch_payload)) ||
      (l1->n[2] && (!in->d_ccch_kind || !in->d_ccch_payload)))
    return fail(l1, "trxsig_l1tx_encode: NULL grid for a class that has channels");
  TrxL1rxSib sb{};
  if (sib) {
    trx_l1rx_sibling(sib, &sb);
    if (sb.n_arfcn != l1->A || std::memcmp(sb.comb, l1->comb.data(), l1->comb.size()) != 0 || sb.n_xcch != l1->n[1])
      return fail(l1, "trxsig_l1tx_encode: the sibling's plan is not this object's");
  }
  TrxL1txCall k;
  geometry(l1, fn, F, k);
  // workspace: scratch c words and flags per unit, bits, what, orders, datagram counts
  const long long units = k.unit0[3] + (long long)l1->n[3] * k.nb[3];
  const size_t slots = (size_t)l1->A * 8 * (size_t)F;
  const size_t gx = ((size_t)l1->A + 255) / 256;
  const size_t sz[] = { (size_t)units * 64, (size_t)units, slots * 148, slots, (size_t)l1->n[1] * 4, (size_t)l1->n[1] * 4,
                        8 * (size_t)F * gx * 4 + 4 };
  constexpr int nsz = sizeof sz / sizeof sz[0];
  size_t off[nsz], total = 0;
  for (int i = 0; i < nsz; i++) { off[i] = total; total += al(sz[i]); }
  trxsig_ctx *c = l1->c;
  TrxDeviceGuard g(trxsig_device(c));
  if (total > l1->work_bytes) {
    TRX_HIPCHK(c, hipStreamSynchronize((hipStream_t)trxsig_get_stream(c)));
    // the old workspace held the last call's outputs: from here on there is none to hand out (trxsig_l1tx_datagrams)
    l1->last_fn = -1; l1->last_F = 0; l1->d_wgc = nullptr;
    l1->dv.c = nullptr; l1->dv.flag = nullptr; l1->dv.bits = nullptr; l1->dv.what = nullptr;
    l1->dv.ord_pow = nullptr; l1->dv.ord_ta = nullptr;
    if (l1->d_work) { TRX_HIPCHK(c, hipFree(l1->d_work)); l1->d_work = nullptr; l1->work_bytes = 0; }
    if (hipMalloc(&l1->d_work, total) != hipSuccess) return trx_ctx_fail(c, TRXSIG_ENOMEM, "trxsig_l1tx_encode: workspace", hipSuccess);
    l1->work_bytes = total;
  }
  char *b = (char *)l1->d_work;
  TrxL1txDev &d = l1->dv;
  d.c = (uint32_t *)(b + off[0]); d.flag = (uint8_t *)(b + off[1]); d.bits = (uint8_t *)(b + off[2]); d.what = (uint8_t *)(b + off[3]);
  d.ord_pow = (int32_t *)(b + off[4]); d.ord_ta = (float *)(b + off[5]); l1->d_wgc = (int32_t *)(b + off[6]);
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
  out->n_arfcn = l1->A; out->n_frames = F; out->n_xcch = l1->n[1];
  out->d_bits = d.bits; out->d_what = d.what; out->d_ms_power = d.ord_pow; out->d_ms_ta = d.ord_ta;
  return TRXSIG_OK;
}

void trx_l1tx_last(const trxsig_l1tx *l1, TrxL1txLast *o) {
  const bool have = l1->last_fn >= 0 && l1->dv.what && l1->dv.bits;
  o->ctx = l1->c; o->n_arfcn = l1->A;
  o->fn = have ? l1->last_fn : 0; o->n_frames = have ? l1->last_F : 0;
  o->what = have ? l1->dv.what : nullptr; o->bits = have ? l1->dv.bits : nullptr;
}

void trx_l1tx_sibling(const trxsig_l1tx *l1, TrxL1txSib *o) {
  o->ctx = l1->c; o->n_arfcn = l1->A; o->n_xcch = l1->n[1]; o->comb = l1->comb.data();
  o->xcch = l1->d_st + (size_t)l1->cur * l1->n_all + l1->n[0];
}

int trxsig_l1tx_datagrams(trxsig_l1tx *l1, uint8_t *h_dgram, int32_t *h_arfcn, int cap, int *n) {
  if (!l1) return TRXSIG_EINVAL;
  if (!n || cap < 0 || (cap > 0 && (!h_dgram || !h_arfcn)) || l1->last_fn < 0)
    return fail(l1, "trxsig_l1tx_datagrams: bad argument (or no encode yet)");
  trxsig_ctx *c = l1->c;
  TrxDeviceGuard g(trxsig_device(c));
  const size_t slots = (size_t)l1->A * 8 * (size_t)l1->last_F;
  const size_t room = (size_t)cap < slots ? (size_t)cap : slots;
  const size_t need = al(room * 154) + room * 4 + 4;
  if (need > l1->dg_bytes) {
    TRX_HIPCHK(c, hipStreamSynchronize((hipStream_t)trxsig_get_stream(c)));
    if (l1->d_dg) { TRX_HIPCHK(c, hipFree(l1->d_dg)); l1->d_dg = nullptr; l1->dg_bytes = 0; }
    if (hipMalloc(&l1->d_dg, need) != hipSuccess) return trx_ctx_fail(c, TRXSIG_ENOMEM, "trxsig_l1tx_datagrams: allocation", hipSuccess);
    l1->dg_bytes = need;
  }
  uint8_t *dg = (uint8_t *)l1->d_dg;
  int32_t *da = (int32_t *)(dg + al(room * 154));
  const size_t gx = ((size_t)l1->A + 255) / 256;
  int32_t *wg = l1->d_wgc;
  int32_t *tot = wg + 8 * (size_t)l1->last_F * gx;
  hipStream_t st = (hipStream_t)trxsig_get_stream(c);
  TRX_HIPCHK(c, trx_launch_l1tx_dgram(st, l1->dv.what, l1->dv.bits, l1->A, l1->last_F, l1->last_fn, wg, tot, dg, da, (int)room,
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
