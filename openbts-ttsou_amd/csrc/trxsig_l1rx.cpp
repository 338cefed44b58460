// trxsig_l1rx.cpp -- the uplink L1 demultiplexer's host side (include/trxsig_l1rx.h): the channel plan, the decoders' state
// on the device, and per call the block geometry (which blocks of each mapping the call's frames touch) and five launches on the
// context's stream: k_l1rx_demux, the TCH and XCCH stream decoders, the RACH decoder on the gathered bursts, k_l1rx_finish.
#include <hip/hip_runtime_api.h>

#include <cstring>
#include <vector>

#include "trxsig_ctx.h"
#include "trxsig_l1rx.h"
#include "trxsig_tdma.h"

namespace {
const TrxTdmaMap kMaps[TRX_N_MAPS] = TRX_TDMA_MAPS_INIT;

// the mapping kind (TRXSIG_L1_*) and sub-channel of a mapping id
void map_kind(int m, int *kind, int *sub) {
  static const int first[] = { TRX_MAP_TCHF, TRX_MAP_SACCH_TF, TRX_MAP_SDCCH8, TRX_MAP_SACCH_C8, TRX_MAP_SDCCH4, TRX_MAP_SACCH_C4,
                               TRX_MAP_RACH_C5 };
  int k = 6;
  while (m < first[k]) k--;
  *kind = k;
  *sub = (k == TRXSIG_L1_SACCH_TF) ? 0 : m - first[k];
}

bool maps_ordered() {   // positions grow with time: f[r] - f[0] (mod R) increases with r (trxsig_tdma.h)
  for (const TrxTdmaMap &m : kMaps)
    for (int r = 1; r < m.n; r++)
      if ((m.f[r] - m.f[0] + m.R) % m.R <= (m.f[r - 1] - m.f[0] + m.R) % m.R) return false;
  return true;
}
}  // namespace

struct trxsig_l1rx {
  trxsig_ctx *c = nullptr;
  int A = 0, bsic = 0, band = 0;
  int n_tch = 0, n_xcch = 0, n_rach = 0;
  std::vector<int32_t> chinfo;         // host copy: arfcn | tn << 16 | map << 20
  std::vector<uint8_t> comb;           // the plan, [A * 8]
  bool map_used[2][TRX_N_MAPS] = {};   // [TCH, XCCH]
  // persistent device state
  void *d_persist = nullptr;
  uint8_t *d_tch_state = nullptr, *d_xcch_state = nullptr, *d_active = nullptr;
  int32_t *d_chinfo = nullptr, *d_rssi = nullptr, *d_timing = nullptr, *d_power = nullptr, *d_ta = nullptr;
  uint32_t *d_accepted = nullptr;
  // per-call workspace
  void *d_work = nullptr;
  size_t work_bytes = 0;
  TrxL1rxDev dv{};
  uint8_t *tch_status = nullptr, *tch_frames = nullptr, *facch = nullptr, *xcch_status = nullptr, *xcch_frames = nullptr;
  float *tch_fer = nullptr, *xcch_fer = nullptr;
};

namespace {
inline size_t al(size_t x) { return (x + 255) & ~(size_t)255; }

int fail(trxsig_l1rx *l1, const char *what) { return trx_ctx_fail(l1 ? l1->c : nullptr, TRXSIG_EINVAL, what, hipSuccess); }

// carve the per-call workspace for (nb_tch, nb_xcch, rach_cap); grows only (a growth waits for the stream first)
int ensure_work(trxsig_l1rx *l1, int nbt, int nbx, int cap) {
  const size_t T = (size_t)l1->n_tch, X = (size_t)l1->n_xcch, R = (size_t)cap;
  const size_t sizes[] = {
    T * 4 * nbt * 4, T, T * nbt * 4, T * nbt, T * nbt * 33, T * nbt * 23, T * nbt * 4,      // tch index, b0, fn, status, frames, facch, fer
    X * 4 * nbx * 4, X * nbx * 4, X * nbx, X * nbx * 23, X * nbx * 4,                      // xcch index, fn, status, frames, fer
    R * 148 * 4, R * 4, R * 4, R * 4, R * 4, 4, R, R, R, R                                  // rach soft, fn, arfcn, rssi, timing, count, tail, bsic, ra, ok
  };
  constexpr int n = sizeof sizes / sizeof sizes[0];
  size_t off[n], total = 0;
  for (int i = 0; i < n; i++) { off[i] = total; total += al(sizes[i]); }
  trxsig_ctx *c = l1->c;
  if (total > l1->work_bytes) {
    TRX_HIPCHK(c, hipStreamSynchronize((hipStream_t)trxsig_get_stream(c)));
    if (l1->d_work) { TRX_HIPCHK(c, hipFree(l1->d_work)); l1->d_work = nullptr; l1->work_bytes = 0; }
    TRX_HIPCHK(c, hipMalloc(&l1->d_work, total));
    TRX_HIPCHK(c, hipMemset(l1->d_work, 0, total));
    l1->work_bytes = total;
  }
  char *b = (char *)l1->d_work;
  TrxL1rxDev &d = l1->dv;
  d.tch_index = (int32_t *)(b + off[0]); d.tch_b0 = (uint8_t *)(b + off[1]); d.tch_fn = (int32_t *)(b + off[2]);
  l1->tch_status = (uint8_t *)(b + off[3]); l1->tch_frames = (uint8_t *)(b + off[4]); l1->facch = (uint8_t *)(b + off[5]);
  l1->tch_fer = (float *)(b + off[6]);
  d.xcch_index = (int32_t *)(b + off[7]); d.xcch_fn = (int32_t *)(b + off[8]);
  l1->xcch_status = (uint8_t *)(b + off[9]); l1->xcch_frames = (uint8_t *)(b + off[10]); l1->xcch_fer = (float *)(b + off[11]);
  d.xcch_status = l1->xcch_status; d.xcch_frames = l1->xcch_frames;
  d.rach_soft = (float *)(b + off[12]); d.rach_fn = (int32_t *)(b + off[13]); d.rach_arfcn = (int32_t *)(b + off[14]);
  d.rach_rssi = (int32_t *)(b + off[15]); d.rach_timing = (int32_t *)(b + off[16]); d.rach_count = (int32_t *)(b + off[17]);
  d.rach_tail = (uint8_t *)(b + off[18]); d.rach_bsic = (uint8_t *)(b + off[19]); d.rach_ra = (uint8_t *)(b + off[20]);
  d.rach_ok = (uint8_t *)(b + off[21]);
  return TRXSIG_OK;
}

int chan_index(const trxsig_l1rx *l1, int cls, int chan) {   // index over all classes, or -1
  if (cls == TRXSIG_L1_TCH && chan >= 0 && chan < l1->n_tch) return chan;
  if (cls == TRXSIG_L1_XCCH && chan >= 0 && chan < l1->n_xcch) return l1->n_tch + chan;
  if (cls == TRXSIG_L1_RACH && chan >= 0 && chan < l1->n_rach) return l1->n_tch + l1->n_xcch + chan;
  return -1;
}

int set_active(trxsig_l1rx *l1, int cls, int chan, int open) {
  if (!l1) return TRXSIG_EINVAL;
  if (cls == TRXSIG_L1_RACH || chan_index(l1, cls, chan) < 0) return fail(l1, "trxsig_l1rx_open / _close: bad channel");
  trxsig_ctx *c = l1->c;
  TrxDeviceGuard g(trxsig_device(c));
  const bool tch = cls == TRXSIG_L1_TCH;
  uint8_t *st = tch ? l1->d_tch_state + (size_t)chan * TRXSIG_TCH_RX_STATE_BYTES
                    : l1->d_xcch_state + (size_t)chan * TRXSIG_XCCH_RX_STATE_BYTES;
  int kind = 0, sub = 0;
  map_kind(l1->chinfo[chan_index(l1, cls, chan)] >> 20, &kind, &sub);
  const int sacch = kind == TRXSIG_L1_SACCH_TF || kind == TRXSIG_L1_SACCH_C8 || kind == TRXSIG_L1_SACCH_C4;
  TRX_HIPCHK(c, trx_launch_l1rx_set((hipStream_t)trxsig_get_stream(c), l1->d_active, chan_index(l1, cls, chan), open, st,
                                    tch ? nullptr : l1->d_power + chan, tch ? nullptr : l1->d_ta + chan, sacch));
  return TRXSIG_OK;
}
}  // namespace

int trxsig_l1rx_create(trxsig_l1rx **out, trxsig_ctx *c, int n_arfcn, const uint8_t *h_comb, int bsic, int band) {
  if (!out || !c) return TRXSIG_EINVAL;
  *out = nullptr;
  const int bidx = (band == 850 || band == 900) ? 0 : band == 1800 ? 1 : band == 1900 ? 2 : -1;
  if (n_arfcn <= 0 || n_arfcn > 0xffff || !h_comb || bsic < 0 || bsic > 63 || bidx < 0 || !maps_ordered())
    return trx_ctx_fail(c, TRXSIG_EINVAL, "trxsig_l1rx_create: bad argument", hipSuccess);
  for (int a = 0; a < n_arfcn; a++)
    for (int tn = 0; tn < 8; tn++) {
      const int k = h_comb[8 * a + tn];
      if (!(k == 0 || k == 1 || k == 7 || (k == 5 && a == 0 && tn == 0)))   // C-V: C0Only, allowedSlots 0x01
        return trx_ctx_fail(c, TRXSIG_EINVAL, "trxsig_l1rx_create: unsupported channel combination or placement", hipSuccess);
    }
  trxsig_l1rx *l1 = new (std::nothrow) trxsig_l1rx;
  if (!l1) return TRXSIG_ENOMEM;
  l1->c = c; l1->A = n_arfcn; l1->bsic = bsic; l1->band = bidx;
  std::vector<int32_t> tch, xcch, rach;
  auto info = [](int a, int tn, int m) { return (int32_t)(a | tn << 16 | m << 20); };
  for (int a = 0; a < n_arfcn; a++)
    for (int tn = 0; tn < 8; tn++) {
      switch (h_comb[8 * a + tn]) {
        case 1:
          tch.push_back(info(a, tn, TRX_MAP_TCHF));
          xcch.push_back(info(a, tn, TRX_MAP_SACCH_TF + tn));
          break;
        case 5:
          for (int s = 0; s < 4; s++) xcch.push_back(info(a, tn, TRX_MAP_SDCCH4 + s));
          for (int s = 0; s < 4; s++) xcch.push_back(info(a, tn, TRX_MAP_SACCH_C4 + s));
          rach.push_back(info(a, tn, TRX_MAP_RACH_C5));
          break;
        case 7:
          for (int s = 0; s < 8; s++) xcch.push_back(info(a, tn, TRX_MAP_SDCCH8 + s));
          for (int s = 0; s < 8; s++) xcch.push_back(info(a, tn, TRX_MAP_SACCH_C8 + s));
          break;
        default: break;
      }
    }
  l1->n_tch = (int)tch.size(); l1->n_xcch = (int)xcch.size(); l1->n_rach = (int)rach.size();
  l1->chinfo = tch;
  l1->chinfo.insert(l1->chinfo.end(), xcch.begin(), xcch.end());
  l1->chinfo.insert(l1->chinfo.end(), rach.begin(), rach.end());
  for (int32_t v : tch) l1->map_used[0][v >> 20] = true;
  for (int32_t v : xcch) l1->map_used[1][v >> 20] = true;
  const size_t N = l1->chinfo.size(), T = (size_t)l1->n_tch, X = (size_t)l1->n_xcch;
  std::vector<int32_t> power(X, -1), ta(X, -1);
  for (size_t i = 0; i < X; i++) {
    int kind = 0, sub = 0;
    map_kind(xcch[i] >> 20, &kind, &sub);
    if (kind == TRXSIG_L1_SACCH_TF || kind == TRXSIG_L1_SACCH_C8 || kind == TRXSIG_L1_SACCH_C4) { power[i] = 40; ta[i] = 0; }
  }
  const size_t sz[] = { T * TRXSIG_TCH_RX_STATE_BYTES, X * TRXSIG_XCCH_RX_STATE_BYTES, N, N * 4, N * 4, N * 4, X * 4, X * 4, N * 4 };
  size_t off[9], total = 0;
  for (int i = 0; i < 9; i++) { off[i] = total; total += al(sz[i]); }
  TrxDeviceGuard g(trxsig_device(c));
  if (hipMalloc(&l1->d_persist, total) != hipSuccess) { delete l1; return trx_ctx_fail(c, TRXSIG_ENOMEM, "trxsig_l1rx_create: device allocation", hipSuccess); }
  char *b = (char *)l1->d_persist;
  l1->d_tch_state = (uint8_t *)(b + off[0]); l1->d_xcch_state = (uint8_t *)(b + off[1]); l1->d_active = (uint8_t *)(b + off[2]);
  l1->d_chinfo = (int32_t *)(b + off[3]); l1->d_rssi = (int32_t *)(b + off[4]); l1->d_timing = (int32_t *)(b + off[5]);
  l1->d_power = (int32_t *)(b + off[6]); l1->d_ta = (int32_t *)(b + off[7]); l1->d_accepted = (uint32_t *)(b + off[8]);
  std::vector<uint8_t> ones(N, 1);
  hipError_t e = hipMemset(l1->d_persist, 0, total);
  if (e == hipSuccess && N) e = hipMemcpy(l1->d_active, ones.data(), N, hipMemcpyHostToDevice);
  if (e == hipSuccess && N) e = hipMemcpy(l1->d_chinfo, l1->chinfo.data(), N * 4, hipMemcpyHostToDevice);
  if (e == hipSuccess && X) e = hipMemcpy(l1->d_power, power.data(), X * 4, hipMemcpyHostToDevice);
  if (e == hipSuccess && X) e = hipMemcpy(l1->d_ta, ta.data(), X * 4, hipMemcpyHostToDevice);
  if (e != hipSuccess) {
    (void)hipFree(l1->d_persist);
    delete l1;
    return trx_ctx_fail(c, TRXSIG_EHIP, "trxsig_l1rx_create: upload", e);
  }
  TrxL1rxDev &d = l1->dv;
  d.chinfo = l1->d_chinfo; d.active = l1->d_active; d.rssi = l1->d_rssi; d.timing = l1->d_timing;
  d.ms_power = l1->d_power; d.ms_ta = l1->d_ta; d.accepted = l1->d_accepted; d.bsic = bsic;
  l1->comb.assign(h_comb, h_comb + 8 * (size_t)n_arfcn);
  trx_ctx_retain(c);
  *out = l1;
  return TRXSIG_OK;
}

void trxsig_l1rx_destroy(trxsig_l1rx *l1) {
  if (!l1) return;
  {
    TrxDeviceGuard g(trxsig_device(l1->c));
    (void)hipStreamSynchronize((hipStream_t)trxsig_get_stream(l1->c));
    if (l1->d_work) (void)hipFree(l1->d_work);
    if (l1->d_persist) (void)hipFree(l1->d_persist);
  }
  trx_ctx_release(l1->c);
  delete l1;
}

int trxsig_l1rx_channels(const trxsig_l1rx *l1, int cls) {
  if (!l1) return TRXSIG_EINVAL;
  return cls == TRXSIG_L1_TCH ? l1->n_tch : cls == TRXSIG_L1_XCCH ? l1->n_xcch : cls == TRXSIG_L1_RACH ? l1->n_rach : TRXSIG_EINVAL;
}

int trxsig_l1rx_channel(const trxsig_l1rx *l1, int cls, int chan, int *arfcn, int *tn, int *kind, int *sub) {
  if (!l1) return TRXSIG_EINVAL;
  const int i = chan_index(l1, cls, chan);
  if (i < 0) return TRXSIG_EINVAL;
  const int32_t v = l1->chinfo[i];
  int k = 0, s = 0;
  map_kind(v >> 20, &k, &s);
  if (arfcn) *arfcn = v & 0xffff;
  if (tn) *tn = (v >> 16) & 15;
  if (kind) *kind = k;
  if (sub) *sub = s;
  return TRXSIG_OK;
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
  if (!res || !out || fn < 0 || fn >= kTrxHyperframe || res->n_arfcn != l1->A || res->n_slots <= 0 || (res->n_slots & 7) ||
      res->n_rows < 0 || !res->d_row ||
      (res->n_rows > 0 && (!res->d_valid || !res->d_soft || !res->d_amp || !res->d_toa || res->soft_stride < 148)))
    return fail(l1, "trxsig_l1rx_decode: bad argument (whole frames from TN 0 of the object's ARFCNs)");
  trxsig_ctx *c = l1->c;
  TrxL1rxCall k{};
  k.fn = fn; k.n_frames = res->n_slots / 8; k.n_arfcn = l1->A; k.n_rows = res->n_rows; k.soft_stride = res->soft_stride;
  k.sps = trxsig_sps(c); k.n_tch = l1->n_tch; k.n_xcch = l1->n_xcch; k.n_rach = l1->n_rach; k.band = l1->band;
  // block geometry per mapping: the positions of frames [fn, fn + F) and the blocks they touch
  for (int m = 0; m < TRX_N_MAPS; m++) {
    const long long p0 = trx_map_count(kMaps[m], fn), p1 = trx_map_count(kMaps[m], (long long)fn + k.n_frames);
    k.p_first[m] = p0;
    k.blk_first[m] = (int32_t)trx_fdiv(p0, 4);
    const int nb = p1 > p0 ? (int)(trx_fdiv(p1 - 1, 4) - trx_fdiv(p0, 4) + 1) : 0;
    if (l1->map_used[0][m] && nb > k.nb_tch) k.nb_tch = nb;
    if (l1->map_used[1][m] && nb > k.nb_xcch) k.nb_xcch = nb;
    if (m == TRX_MAP_RACH_C5 && l1->n_rach) k.rach_cap = (int)(p1 - p0);
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
  o->n_arfcn = l1->A; o->n_tch = l1->n_tch; o->n_xcch = l1->n_xcch; o->comb = l1->comb.data();
  o->rssi = l1->d_rssi + l1->n_tch; o->timing = l1->d_timing + l1->n_tch; o->power = l1->d_power; o->ta = l1->d_ta;
  o->accepted = l1->d_accepted + l1->n_tch;
}
