// trxsig_l1ms.cpp -- the mobile-side uplink L1's host side (include/trxsig_l1ms.h): the channel plan (trxsig_l1rx's numbering),
// the slot-owner tables of the uplink mappings, the channels' records on the device (two copies: a call reads one and commits
// the other), per encode the block geometry of every mapping and three launches on the context's stream (k_l1ms_encode,
// k_l1ms_mux, k_l1ms_commit), per radiate one (k_l1ms_radiate).
#include <hip/hip_runtime_api.h>

#include <cstdlib>
#include <cstring>
#include <vector>

#include "trxsig_ctx.h"
#include "trxsig_l1ms.h"
#include "trxsig_l1ms_dev.h"
#include "trxsig_l1msrx_dev.h"

namespace {
const TrxTdmaMap kUl[TRX_N_MAPS] = TRX_TDMA_MAPS_INIT;
const int8_t kPower[3][32] = TRX_POWER_TABLES_INIT;

void map_kind(int m, int *kind, int *sub) {   // TRXSIG_L1_* kind and sub-channel of an uplink mapping id
  static const int first[] = { TRX_MAP_TCHF, TRX_MAP_SACCH_TF, TRX_MAP_SDCCH8, TRX_MAP_SACCH_C8, TRX_MAP_SDCCH4, TRX_MAP_SACCH_C4,
                               TRX_MAP_RACH_C5 };
  int k = 6;
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
  for (const TrxTdmaMap &m : kUl)
    for (int r = 1; r < m.n; r++)
      if ((m.f[r] - m.f[0] + m.R) % m.R <= (m.f[r - 1] - m.f[0] + m.R) % m.R) return false;
  return true;
}
// the power a handset of the band radiates when ordered to `power` dBm: POWER[band][encodePower(band, power)]
int level_power(int band, int power) {
  int min_err = std::abs(power - kPower[band][0]), code = 0;
  for (int i = 1; i < 32; i++) {
    const int e = std::abs(power - kPower[band][i]);
    if (e == 0) { code = i; break; }
    if (e < min_err) { min_err = e; code = i; }
  }
  return kPower[band][code];
}
inline size_t al(size_t x) { return (x + 255) & ~(size_t)255; }
inline long long ceil4(long long p) { return -trx_fdiv(-p, 4); }
constexpr long long kMaxOutBytes = 1LL << 34;
}  // namespace

struct trxsig_l1ms {
  trxsig_ctx *c = nullptr;
  int A = 0, bsic = 0, band = 0;
  int n[3] = {};                        // TCH, XCCH, RACH
  int n_all = 0, cur = 0;               // n_all: TCH + XCCH (the channels that have records)
  std::vector<int32_t> chinfo;          // arfcn | tn << 16 | map << 20; the RACH after the others
  std::vector<uint8_t> comb;
  bool used[2][TRX_N_MAPS] = {};
  void *d_persist = nullptr;
  TrxL1msChan *d_st = nullptr;
  void *d_work = nullptr;
  size_t work_bytes = 0;
  TrxL1msDev dv{};
  int last_F = 0, last_rach = 0;        // the last encode (radiate); 0: none
  const trxsig_l1msrx *fol = nullptr;   // the trxsig_l1msrx whose decoded orders the handsets follow, or null
};

namespace {
int fail(trxsig_l1ms *ms, const char *what) { return trx_ctx_fail(ms ? ms->c : nullptr, TRXSIG_EINVAL, what, hipSuccess); }

int chan_index(const trxsig_l1ms *ms, int cls, int chan) {   // index over all classes, or -1
  if (cls == TRXSIG_L1_TCH && chan >= 0 && chan < ms->n[0]) return chan;
  if (cls == TRXSIG_L1_XCCH && chan >= 0 && chan < ms->n[1]) return ms->n[0] + chan;
  if (cls == TRXSIG_L1_RACH && chan >= 0 && chan < ms->n[2]) return ms->n[0] + ms->n[1] + chan;
  return -1;
}

int set_active(trxsig_l1ms *ms, int cls, int chan, int open) {
  if (!ms) return TRXSIG_EINVAL;
  const int g = chan_index(ms, cls, chan);
  if (cls == TRXSIG_L1_RACH || g < 0) return fail(ms, "trxsig_l1ms_open / _close: bad channel");
  trxsig_ctx *c = ms->c;
  TrxDeviceGuard gd(trxsig_device(c));
  const bool phy = open && cls == TRXSIG_L1_XCCH && map_sacch(ms->chinfo[g] >> 20);
  TRX_HIPCHK(c, trx_launch_l1ms_set((hipStream_t)trxsig_get_stream(c), ms->d_st + (size_t)ms->cur * ms->n_all + g, open, phy,
                                    level_power(ms->band, 40), 0));
  return TRXSIG_OK;
}

// block geometry of a call
void geometry(const trxsig_l1ms *ms, int fn, int F, TrxL1msCall &k) {
  std::memset(&k, 0, sizeof k);
  k.fn = fn; k.n_frames = F; k.n_arfcn = ms->A;
  k.n_tch = ms->n[0]; k.n_xcch = ms->n[1]; k.n_all = ms->n_all;
  k.r104 = fn % 104; k.r102 = fn % 102; k.r51 = fn % 51; k.r26 = fn % 26;
  k.cur = ms->cur; k.band = ms->band; k.bsic = ms->bsic;
  for (int m = 0; m < TRX_N_MAPS; m++) {
    const TrxTdmaMap &M = kUl[m];
    k.p_first[m] = trx_map_count(M, fn);
    k.p_end[m] = trx_map_count(M, (long long)fn + F);
    int below = 0;
    for (int r = 0; r < M.n; r++) below += M.f[r] < fn % M.R;
    k.base[m] = k.p_first[m] - below;
    const long long nb = ceil4(k.p_end[m]) - ceil4(k.p_first[m]);
    for (int cl = 0; cl < 2; cl++)
      if (ms->used[cl][m] && nb > k.nb[cl]) k.nb[cl] = (int)nb;
  }
  if (ms->n[2]) k.n_rach = (int)(k.p_end[TRX_MAP_RACH_C5] - k.p_first[TRX_MAP_RACH_C5]);
  long long u = 0;
  for (int cl = 0; cl < 2; cl++) { k.unit0[cl] = u; u += (long long)ms->n[cl] * k.nb[cl]; }
}
}  // namespace

int trxsig_l1ms_create(trxsig_l1ms **out, trxsig_ctx *c, int n_arfcn, const uint8_t *h_comb, int bsic, int band) {
  if (!out || !c) return TRXSIG_EINVAL;
  *out = nullptr;
  const int bidx = (band == 850 || band == 900) ? 0 : band == 1800 ? 1 : band == 1900 ? 2 : -1;
  if (n_arfcn <= 0 || n_arfcn > 0xffff || !h_comb || bsic < 0 || bsic > 63 || bidx < 0 || !maps_ordered())
    return trx_ctx_fail(c, TRXSIG_EINVAL, "trxsig_l1ms_create: bad argument", hipSuccess);
  for (int a = 0; a < n_arfcn; a++)
    for (int tn = 0; tn < 8; tn++) {
      const int k = h_comb[8 * a + tn];
      if (!(k == 0 || k == 1 || k == 7 || (k == 5 && a == 0 && tn == 0)))
        return trx_ctx_fail(c, TRXSIG_EINVAL, "trxsig_l1ms_create: unsupported channel combination or placement", hipSuccess);
    }
  trxsig_l1ms *ms = new (std::nothrow) trxsig_l1ms;
  if (!ms) return TRXSIG_ENOMEM;
  ms->c = c; ms->A = n_arfcn; ms->bsic = bsic; ms->band = bidx;
  ms->comb.assign(h_comb, h_comb + 8 * (size_t)n_arfcn);
  std::vector<int32_t> cl[3], hs[2];    // hs: the XCCH index of each channel's handset
  auto info = [](int a, int tn, int m) { return (int32_t)(a | tn << 16 | m << 20); };
  std::vector<int32_t> slot(8 * (size_t)n_arfcn, 0), slot_x(8 * (size_t)n_arfcn, 0);
  for (int a = 0; a < n_arfcn; a++)
    for (int tn = 0; tn < 8; tn++) {
      const int k = h_comb[8 * a + tn];
      const int32_t x0 = (int32_t)cl[1].size();
      slot_x[8 * a + tn] = x0;                       // XCCH index; made global below
      slot[8 * a + tn] = k | (int32_t)cl[0].size() << 4;
      switch (k) {
        case 1:
          cl[0].push_back(info(a, tn, TRX_MAP_TCHF)); hs[0].push_back(x0);
          cl[1].push_back(info(a, tn, TRX_MAP_SACCH_TF + tn)); hs[1].push_back(x0);
          break;
        case 5:
          for (int s = 0; s < 4; s++) { cl[1].push_back(info(a, tn, TRX_MAP_SDCCH4 + s)); hs[1].push_back(x0 + 4 + s); }
          for (int s = 0; s < 4; s++) { cl[1].push_back(info(a, tn, TRX_MAP_SACCH_C4 + s)); hs[1].push_back(x0 + 4 + s); }
          cl[2].push_back(info(a, tn, TRX_MAP_RACH_C5));
          break;
        case 7:
          for (int s = 0; s < 8; s++) { cl[1].push_back(info(a, tn, TRX_MAP_SDCCH8 + s)); hs[1].push_back(x0 + 8 + s); }
          for (int s = 0; s < 8; s++) { cl[1].push_back(info(a, tn, TRX_MAP_SACCH_C8 + s)); hs[1].push_back(x0 + 8 + s); }
          break;
        default: break;
      }
    }
  for (int k = 0; k < 3; k++) {
    ms->n[k] = (int)cl[k].size();
    ms->chinfo.insert(ms->chinfo.end(), cl[k].begin(), cl[k].end());
    if (k < 2)
      for (int32_t v : cl[k]) ms->used[k][v >> 20] = true;
  }
  ms->n_all = ms->n[0] + ms->n[1];
  for (int32_t &x : slot_x) x += ms->n[0];
  std::vector<int32_t> handset(hs[0]);
  handset.insert(handset.end(), hs[1].begin(), hs[1].end());
  // the slot owners: [combination I / V / VII][TN][fn mod 104 (I) or 102 (V, VII)]
  std::vector<int8_t> writer(3 * 8 * 104, -1);
  std::vector<int> maps[3];
  maps[0] = { TRX_MAP_TCHF };
  for (int s = 0; s < 4; s++) { maps[1].push_back(TRX_MAP_SDCCH4 + s); maps[1].push_back(TRX_MAP_SACCH_C4 + s); }
  maps[1].push_back(TRX_MAP_RACH_C5);
  for (int s = 0; s < 8; s++) { maps[2].push_back(TRX_MAP_SDCCH8 + s); maps[2].push_back(TRX_MAP_SACCH_C8 + s); }
  bool disjoint = true;
  for (int ci = 0; ci < 3; ci++)
    for (int tn = 0; tn < 8; tn++) {
      std::vector<int> mm = maps[ci];
      if (ci == 0) mm.push_back(TRX_MAP_SACCH_TF + tn);
      const int L = ci == 0 ? 104 : 102;
      for (int m : mm)
        for (int r = 0; r < L; r++)
          for (int i = 0; i < kUl[m].n; i++)
            if (r % kUl[m].R == kUl[m].f[i]) {
              int8_t &w = writer[(ci * 8 + tn) * 104 + r];
              if (w >= 0) disjoint = false;
              w = (int8_t)m;
            }
    }
  std::vector<int16_t> cnt(TRX_N_MAPS * 105, 0);
  for (int m = 0; m < TRX_N_MAPS; m++)
    for (int x = 0; x <= kUl[m].R; x++) {
      int v = 0;
      for (int i = 0; i < kUl[m].n; i++) v += kUl[m].f[i] < x;
      cnt[m * 105 + x] = (int16_t)v;
    }
  const size_t N = (size_t)ms->n_all, S = 8 * (size_t)n_arfcn;
  std::vector<TrxL1msChan> rec(2 * N);
  if (N) std::memset(rec.data(), 0, rec.size() * sizeof(TrxL1msChan));
  for (size_t i = 0; i < 2 * N; i++) {
    const int g = (int)(i % N);
    const bool sacch = g >= ms->n[0] && map_sacch(ms->chinfo[g] >> 20);
    rec[i].active = 1;
    rec[i].power = sacch ? level_power(bidx, 40) : -1;
    rec[i].ta = sacch ? 0 : -1;
  }
  const size_t sz[] = { 2 * N * sizeof(TrxL1msChan), (N + 1) * 4, S * 4, S * 4, (N + 1) * 4, writer.size(), cnt.size() * 2 };
  constexpr int nsz = sizeof sz / sizeof sz[0];
  size_t off[nsz], total = 0;
  for (int i = 0; i < nsz; i++) { off[i] = total; total += al(sz[i]); }
  TrxDeviceGuard gd(trxsig_device(c));
  if (!disjoint || hipMalloc(&ms->d_persist, total) != hipSuccess) {
    delete ms;
    return trx_ctx_fail(c, disjoint ? TRXSIG_ENOMEM : TRXSIG_EINVAL, "trxsig_l1ms_create: device allocation", hipSuccess);
  }
  char *b = (char *)ms->d_persist;
  TrxL1msDev &d = ms->dv;
  ms->d_st = (TrxL1msChan *)(b + off[0]);
  d.st = ms->d_st; d.chinfo = (const int32_t *)(b + off[1]); d.slot = (const int32_t *)(b + off[2]);
  d.slot_x = (const int32_t *)(b + off[3]); d.handset = (const int32_t *)(b + off[4]); d.writer = (const int8_t *)(b + off[5]);
  d.cnt = (const int16_t *)(b + off[6]);
  hipError_t e = hipMemset(ms->d_persist, 0, total);
  if (e == hipSuccess && N) e = hipMemcpy(ms->d_st, rec.data(), 2 * N * sizeof(TrxL1msChan), hipMemcpyHostToDevice);
  if (e == hipSuccess && N) e = hipMemcpy(b + off[1], ms->chinfo.data(), N * 4, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(b + off[2], slot.data(), S * 4, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(b + off[3], slot_x.data(), S * 4, hipMemcpyHostToDevice);
  if (e == hipSuccess && N) e = hipMemcpy(b + off[4], handset.data(), N * 4, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(b + off[5], writer.data(), writer.size(), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(b + off[6], cnt.data(), cnt.size() * 2, hipMemcpyHostToDevice);
  d.filler = trx_ctx_tch_filler(c);
  if (e != hipSuccess || !d.filler) {
    (void)hipFree(ms->d_persist);
    delete ms;
    return trx_ctx_fail(c, TRXSIG_EHIP, "trxsig_l1ms_create: upload", e);
  }
  trx_ctx_retain(c);
  *out = ms;
  return TRXSIG_OK;
}

void trxsig_l1ms_destroy(trxsig_l1ms *ms) {
  if (!ms) return;
  {
    TrxDeviceGuard g(trxsig_device(ms->c));
    (void)hipStreamSynchronize((hipStream_t)trxsig_get_stream(ms->c));
    if (ms->d_work) (void)hipFree(ms->d_work);
    if (ms->d_persist) (void)hipFree(ms->d_persist);
  }
  trx_ctx_release(ms->c);
  delete ms;
}

int trxsig_l1ms_channels(const trxsig_l1ms *ms, int cls) {
  if (!ms || cls < 0 || cls > 2) return TRXSIG_EINVAL;
  return ms->n[cls];
}

int trxsig_l1ms_channel(const trxsig_l1ms *ms, int cls, int chan, int *arfcn, int *tn, int *kind, int *sub) {
  if (!ms) return TRXSIG_EINVAL;
  const int g = chan_index(ms, cls, chan);
  if (g < 0) return TRXSIG_EINVAL;
  const int32_t v = ms->chinfo[g];
  int k = 0, s = 0;
  map_kind(v >> 20, &k, &s);
  if (arfcn) *arfcn = v & 0xffff;
  if (tn) *tn = (v >> 16) & 15;
  if (kind) *kind = k;
  if (sub) *sub = s;
  return TRXSIG_OK;
}

int trxsig_l1ms_open(trxsig_l1ms *ms, int cls, int chan) { return set_active(ms, cls, chan, 1); }
int trxsig_l1ms_close(trxsig_l1ms *ms, int cls, int chan) { return set_active(ms, cls, chan, 0); }

int trxsig_l1ms_set_phy(trxsig_l1ms *ms, int chan, int power, int ta) {
  if (!ms) return TRXSIG_EINVAL;
  const int g = chan_index(ms, TRXSIG_L1_XCCH, chan);
  if (g < 0 || !map_sacch(ms->chinfo[g] >> 20) || power < 0 || power > 40 || ta < 0 || ta > 63)
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
  *d_state = (void *)(ms->d_st + (size_t)ms->cur * ms->n_all + (cls == TRXSIG_L1_XCCH ? ms->n[0] : 0));
  return TRXSIG_OK;
}

int trxsig_l1ms_follow(trxsig_l1ms *ms, const trxsig_l1msrx *rx) {
  if (!ms) return TRXSIG_EINVAL;
  if (rx) {
    TrxL1msrxFollow fo{};
    trx_l1msrx_follow(rx, &fo);
    if (fo.ctx != ms->c || fo.n_arfcn != ms->A || fo.bsic != ms->bsic || fo.band != ms->band || fo.n_xcch != ms->n[1] ||
        std::memcmp(fo.comb, ms->comb.data(), ms->comb.size()) != 0)
      return fail(ms, "trxsig_l1ms_follow: the trxsig_l1msrx's plan (or context) is not this object's");
  }
  ms->fol = rx;
  return TRXSIG_OK;
}

int trxsig_l1ms_encode(trxsig_l1ms *ms, int fn, int F, const trxsig_l1ms_in *in, const trxsig_l1tx *sib, trxsig_l1ms_out *out) {
  if (!ms) return TRXSIG_EINVAL;
  if (!in || !out || fn < 0 || fn >= kTrxHyperframe || F <= 0)
    return fail(ms, "trxsig_l1ms_encode: bad argument (fn in [0, 2715648), n_frames > 0)");
  if ((long long)ms->A * 8 * 148 * F > kMaxOutBytes) return fail(ms, "trxsig_l1ms_encode: output above 2^34 bytes");
  TrxL1msCall k;
  geometry(ms, fn, F, k);
  if ((ms->n[0] && (!in->d_tch_kind || !in->d_tch_payload)) || (ms->n[1] && (!in->d_xcch_kind || !in->d_xcch_payload)) ||
      (k.n_rach && (!in->d_rach_kind || !in->d_rach_ra)))
    return fail(ms, "trxsig_l1ms_encode: NULL grid for a class that has channels");
  if (sib && ms->fol) return fail(ms, "trxsig_l1ms_encode: a sibling while following a trxsig_l1msrx");
  TrxL1txSib sb{};
  if (sib) {
    trx_l1tx_sibling(sib, &sb);
    if (sb.ctx != ms->c || sb.n_arfcn != ms->A || std::memcmp(sb.comb, ms->comb.data(), ms->comb.size()) != 0 ||
        sb.n_xcch != ms->n[1])
      return fail(ms, "trxsig_l1ms_encode: the sibling's plan (or context) is not this object's");
  }
  // workspace: scratch c words and flags per unit, bits, what, who, the handsets after the call
  const long long units = k.unit0[1] + (long long)ms->n[1] * k.nb[1];
  const size_t slots = (size_t)ms->A * 8 * (size_t)F;
  const size_t sz[] = { (size_t)units * 64, (size_t)units, slots * 148, slots, slots * 4, (size_t)ms->n[1] * 4, (size_t)ms->n[1] * 4 };
  constexpr int nsz = sizeof sz / sizeof sz[0];
  size_t off[nsz], total = 0;
  for (int i = 0; i < nsz; i++) { off[i] = total; total += al(sz[i]); }
  trxsig_ctx *c = ms->c;
  TrxDeviceGuard g(trxsig_device(c));
  if (total > ms->work_bytes) {
    TRX_HIPCHK(c, hipStreamSynchronize((hipStream_t)trxsig_get_stream(c)));
    ms->last_F = 0;                     // the old workspace held the last call's outputs: there is none to radiate from here on
    if (ms->d_work) { TRX_HIPCHK(c, hipFree(ms->d_work)); ms->d_work = nullptr; ms->work_bytes = 0; }
    if (hipMalloc(&ms->d_work, total) != hipSuccess) return trx_ctx_fail(c, TRXSIG_ENOMEM, "trxsig_l1ms_encode: workspace", hipSuccess);
    ms->work_bytes = total;
  }
  char *b = (char *)ms->d_work;
  TrxL1msDev &d = ms->dv;
  d.c = (uint32_t *)(b + off[0]); d.flag = (uint8_t *)(b + off[1]); d.bits = (uint8_t *)(b + off[2]); d.what = (uint8_t *)(b + off[3]);
  d.who = (int32_t *)(b + off[4]); d.ms_power = (int32_t *)(b + off[5]); d.ms_ta = (int32_t *)(b + off[6]);
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
  out->n_arfcn = ms->A; out->n_frames = F; out->n_xcch = ms->n[1];
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
  const long long T = 8LL * ms->last_F, A = ms->A, cell = 157LL * sps;
  // cells must not overlap: slots inside an ARFCN's row, or ARFCNs inside a slot's row
  const bool slot_major = arfcn_stride >= cell && (T == 1 || slot_stride >= A * arfcn_stride);
  const bool arfcn_major = slot_stride >= cell && (A == 1 || arfcn_stride >= T * slot_stride);
  if (!slot_major && !arfcn_major) return fail(ms, "trxsig_l1ms_radiate: the strides let cells overlap");
  if ((ms->n[0] && (!air->d_tch_gain || !air->d_tch_delay)) || (ms->n[1] && (!air->d_xcch_gain || !air->d_xcch_delay)) ||
      (ms->last_rach && (!air->d_rach_gain || !air->d_rach_delay)) || (ms->n_all && !air->d_amp_of_power))
    return fail(ms, "trxsig_l1ms_radiate: NULL array for a class that has channels");
  TrxL1msAir p{};
  p.gain[0] = (const trx_c32 *)air->d_tch_gain; p.gain[1] = (const trx_c32 *)air->d_xcch_gain; p.gain[2] = (const trx_c32 *)air->d_rach_gain;
  p.delay[0] = air->d_tch_delay; p.delay[1] = air->d_xcch_delay; p.delay[2] = air->d_rach_delay;
  p.amp_of_power = air->d_amp_of_power;
  const TrxL1msDev &d = ms->dv;
  p.bits = d.bits; p.what = d.what; p.who = d.who; p.handset = d.handset; p.ms_power = d.ms_power; p.ms_ta = d.ms_ta;
  p.out = (trx_c32 *)d_samples; p.slot_stride = slot_stride; p.arfcn_stride = arfcn_stride;
  p.n_arfcn = ms->A; p.n_tch = ms->n[0]; p.rows = T;
  TrxDeviceGuard g(trxsig_device(c));
  TRX_HIPCHK(c, trx_launch_l1ms_radiate((hipStream_t)trxsig_get_stream(c), sps, (const TrxTables *)trxsig_tables_device(c), p));
  return TRXSIG_OK;
}
