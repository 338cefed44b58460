// trxsig_l1msrx.cpp -- the mobile-side downlink L1's host side (include/trxsig_l1msrx.h): the channel plan over the downlink
// mappings, the decoders' state on the device, and per call the block geometry (which blocks of each mapping the call's frames
// touch) and the launches on the context's stream: k_l1msrx_demux, k_l1rx_demux_phy on the rows it recorded, the TCH stream
// decoder, the XCCH stream decoder over the control grid (XCCH, CCCH, BCCH), the generic Viterbi on the gathered SCH bursts,
// k_l1msrx_finish.
#include <hip/hip_runtime_api.h>

#include <cstring>
#include <vector>

#include "trxsig_ctx.h"
#include "trxsig_l1msrx.h"
#include "trxsig_l1msrx_dev.h"

namespace {
const TrxTdmaMap kDl[TRX_N_DL_MAPS] = TRX_TDMA_DL_MAPS_INIT;

// the mapping kind (TRXSIG_L1_*) and sub-channel of a downlink mapping id
void map_kind(int m, int *kind, int *sub) {
  *sub = 0;
  if (m == TRX_DL_FCCH) { *kind = TRXSIG_L1_FCCH_C5; return; }
  if (m == TRX_DL_SCH) { *kind = TRXSIG_L1_SCH_C5; return; }
  if (m == TRX_DL_BCCH) { *kind = TRXSIG_L1_BCCH_C5; return; }
  if (m >= TRX_DL_CCCH) { *kind = TRXSIG_L1_CCCH_C5; *sub = m - TRX_DL_CCCH; return; }
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
bool maps_ordered() {   // positions grow with time (trxsig_tdma.h); 4, 5 or 24 frames a repeat: the lengths dl_frame divides by
  for (const TrxTdmaMap &m : kDl)
    if (m.n != 4 && m.n != 5 && m.n != 24) return false;
  for (const TrxTdmaMap &m : kDl)
    for (int r = 1; r < m.n; r++)
      if ((m.f[r] - m.f[0] + m.R) % m.R <= (m.f[r - 1] - m.f[0] + m.R) % m.R) return false;
  return true;
}
inline size_t al(size_t x) { return (x + 255) & ~(size_t)255; }
enum { K_TCH = 0, K_XCCH = 1, K_CCCH = 2, K_BCCH = 3, K_SCH = 4, K_FCCH = 5, K_N = 6 };   // the classes in channel order
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
  int A = 0, bsic = 0, band = 0;
  int n[K_N] = {};
  std::vector<int32_t> chinfo;         // host copy: arfcn | tn << 16 | map << 20, in channel order
  std::vector<uint8_t> comb;           // the plan, [A * 8]
  bool map_used[2][TRX_N_DL_MAPS] = {};   // [TCH, control grid]
  // persistent device state
  void *d_persist = nullptr;
  uint8_t *d_tch_state = nullptr, *d_ctl_state = nullptr, *d_active = nullptr;
  int32_t *d_chinfo = nullptr, *d_rssi = nullptr, *d_timing = nullptr, *d_power = nullptr, *d_ta = nullptr, *d_last = nullptr;
  // per-call workspace
  void *d_work = nullptr;
  size_t work_bytes = 0;
  TrxL1msrxDev dv{};
  uint8_t *tch_status = nullptr, *tch_frames = nullptr, *facch = nullptr, *ctl_status = nullptr, *ctl_frames = nullptr, *sch_u = nullptr;
  float *tch_fer = nullptr, *ctl_fer = nullptr;
  int n_ctl() const { return n[K_XCCH] + n[K_CCCH] + n[K_BCCH]; }
};

namespace {
int fail(trxsig_l1msrx *rx, const char *what) { return trx_ctx_fail(rx ? rx->c : nullptr, TRXSIG_EINVAL, what, hipSuccess); }

// carve the per-call workspace; grows only (a growth waits for the stream first)
int ensure_work(trxsig_l1msrx *rx, int nbt, int nbx, int scap, int fcap) {
  const size_t T = (size_t)rx->n[K_TCH], X = (size_t)rx->n_ctl(), B = (size_t)rx->n[K_BCCH], S = (size_t)scap, Fc = (size_t)fcap;
  const size_t sizes[] = {
    T * 4 * nbt * 4, T, T * nbt * 4, T * nbt, T * nbt * 33, T * nbt * 23, T * nbt * 4,      // tch index, b0, fn, status, frames, facch, fer
    X * 4 * nbx * 4, X * nbx * 4, X * nbx, X * nbx * 23, X * nbx * 4, B * nbx * 4,         // ctl index, fn, status, frames, fer; bcch tc
    S * 78 * 4, S * 39, S * 4, S * 4, S, S, S, S,                                           // sch e, u, fn, rfn, present, ok, bsic, sync
    Fc * 4, Fc * 4                                                                          // fcch fn, ones
  };
  constexpr int n = sizeof sizes / sizeof sizes[0];
  size_t off[n], total = 0;
  for (int i = 0; i < n; i++) { off[i] = total; total += al(sizes[i]); }
  trxsig_ctx *c = rx->c;
  if (total > rx->work_bytes) {
    TRX_HIPCHK(c, hipStreamSynchronize((hipStream_t)trxsig_get_stream(c)));
    if (rx->d_work) { TRX_HIPCHK(c, hipFree(rx->d_work)); rx->d_work = nullptr; rx->work_bytes = 0; }
    TRX_HIPCHK(c, hipMalloc(&rx->d_work, total));
    TRX_HIPCHK(c, hipMemset(rx->d_work, 0, total));
    rx->work_bytes = total;
  }
  char *b = (char *)rx->d_work;
  TrxL1msrxDev &d = rx->dv;
  d.tch_index = (int32_t *)(b + off[0]); d.tch_b0 = (uint8_t *)(b + off[1]); d.tch_fn = (int32_t *)(b + off[2]);
  rx->tch_status = (uint8_t *)(b + off[3]); rx->tch_frames = (uint8_t *)(b + off[4]); rx->facch = (uint8_t *)(b + off[5]);
  rx->tch_fer = (float *)(b + off[6]);
  d.ctl_index = (int32_t *)(b + off[7]); d.ctl_fn = (int32_t *)(b + off[8]);
  rx->ctl_status = (uint8_t *)(b + off[9]); rx->ctl_frames = (uint8_t *)(b + off[10]); rx->ctl_fer = (float *)(b + off[11]);
  d.ctl_status = rx->ctl_status; d.ctl_frames = rx->ctl_frames;
  d.bcch_tc = (int32_t *)(b + off[12]);
  d.sch_e = (float *)(b + off[13]); rx->sch_u = (uint8_t *)(b + off[14]); d.sch_u = rx->sch_u;
  d.sch_fn = (int32_t *)(b + off[15]); d.sch_rfn = (int32_t *)(b + off[16]); d.sch_present = (uint8_t *)(b + off[17]);
  d.sch_ok = (uint8_t *)(b + off[18]); d.sch_bsic = (uint8_t *)(b + off[19]); d.sch_sync = (uint8_t *)(b + off[20]);
  d.fcch_fn = (int32_t *)(b + off[21]); d.fcch_ones = (int32_t *)(b + off[22]);
  return TRXSIG_OK;
}

int chan_index(const trxsig_l1msrx *rx, int cls, int chan) {   // index over all classes, or -1
  const int k = class_slot(cls);
  if (k < 0 || chan < 0 || chan >= rx->n[k]) return -1;
  int off = 0;
  for (int i = 0; i < k; i++) off += rx->n[i];
  return off + chan;
}

int set_active(trxsig_l1msrx *rx, int cls, int chan, int open) {
  if (!rx) return TRXSIG_EINVAL;
  const int g = chan_index(rx, cls, chan);
  if (g < 0 || cls == TRXSIG_L1_SCH || cls == TRXSIG_L1_FCCH) return fail(rx, "trxsig_l1msrx_open / _close: bad channel");
  trxsig_ctx *c = rx->c;
  TrxDeviceGuard gd(trxsig_device(c));
  const bool tch = cls == TRXSIG_L1_TCH;
  uint8_t *st = tch ? rx->d_tch_state + (size_t)g * TRXSIG_TCH_RX_STATE_BYTES
                    : rx->d_ctl_state + (size_t)(g - rx->n[K_TCH]) * TRXSIG_XCCH_RX_STATE_BYTES;
  const int sacch = cls == TRXSIG_L1_XCCH && map_sacch(rx->chinfo[g] >> 20);
  TRX_HIPCHK(c, trx_launch_l1rx_set((hipStream_t)trxsig_get_stream(c), rx->d_active, g, open, st,
                                    sacch ? rx->d_power + chan : nullptr, sacch ? rx->d_ta + chan : nullptr, sacch));
  return TRXSIG_OK;
}
}  // namespace

int trxsig_l1msrx_create(trxsig_l1msrx **out, trxsig_ctx *c, int n_arfcn, const uint8_t *h_comb, int bsic, int band) {
  if (!out || !c) return TRXSIG_EINVAL;
  *out = nullptr;
  const int bidx = (band == 850 || band == 900) ? 0 : band == 1800 ? 1 : band == 1900 ? 2 : -1;
  if (n_arfcn <= 0 || n_arfcn > 0xffff || !h_comb || bsic < 0 || bsic > 63 || bidx < 0 || !maps_ordered())
    return trx_ctx_fail(c, TRXSIG_EINVAL, "trxsig_l1msrx_create: bad argument", hipSuccess);
  for (int a = 0; a < n_arfcn; a++)
    for (int tn = 0; tn < 8; tn++) {
      const int k = h_comb[8 * a + tn];
      if (!(k == 0 || k == 1 || k == 7 || (k == 5 && a == 0 && tn == 0)))
        return trx_ctx_fail(c, TRXSIG_EINVAL, "trxsig_l1msrx_create: unsupported channel combination or placement", hipSuccess);
    }
  trxsig_l1msrx *rx = new (std::nothrow) trxsig_l1msrx;
  if (!rx) return TRXSIG_ENOMEM;
  rx->c = c; rx->A = n_arfcn; rx->bsic = bsic; rx->band = bidx;
  rx->comb.assign(h_comb, h_comb + 8 * (size_t)n_arfcn);
  std::vector<int32_t> cl[K_N];
  auto info = [](int a, int tn, int m) { return (int32_t)(a | tn << 16 | m << 20); };
  for (int a = 0; a < n_arfcn; a++)
    for (int tn = 0; tn < 8; tn++) {
      switch (h_comb[8 * a + tn]) {
        case 1:
          cl[K_TCH].push_back(info(a, tn, TRX_MAP_TCHF));
          cl[K_XCCH].push_back(info(a, tn, TRX_MAP_SACCH_TF + tn));
          break;
        case 5:
          for (int s = 0; s < 4; s++) cl[K_XCCH].push_back(info(a, tn, TRX_MAP_SDCCH4 + s));
          for (int s = 0; s < 4; s++) cl[K_XCCH].push_back(info(a, tn, TRX_MAP_SACCH_C4 + s));
          for (int s = 0; s < 3; s++) cl[K_CCCH].push_back(info(a, tn, TRX_DL_CCCH + s));
          cl[K_BCCH].push_back(info(a, tn, TRX_DL_BCCH));
          cl[K_SCH].push_back(info(a, tn, TRX_DL_SCH));
          cl[K_FCCH].push_back(info(a, tn, TRX_DL_FCCH));
          break;
        case 7:
          for (int s = 0; s < 8; s++) cl[K_XCCH].push_back(info(a, tn, TRX_MAP_SDCCH8 + s));
          for (int s = 0; s < 8; s++) cl[K_XCCH].push_back(info(a, tn, TRX_MAP_SACCH_C8 + s));
          break;
        default: break;
      }
    }
  for (int k = 0; k < K_N; k++) {
    rx->n[k] = (int)cl[k].size();
    rx->chinfo.insert(rx->chinfo.end(), cl[k].begin(), cl[k].end());
    if (k <= K_BCCH)
      for (int32_t v : cl[k]) rx->map_used[k == K_TCH ? 0 : 1][v >> 20] = true;
  }
  const size_t N = rx->chinfo.size(), T = (size_t)rx->n[K_TCH], X = (size_t)rx->n[K_XCCH], G = (size_t)rx->n_ctl(), NB = T + G;
  std::vector<int32_t> power(X, -1), ta(X, -1);
  for (size_t i = 0; i < X; i++)
    if (map_sacch(cl[K_XCCH][i] >> 20)) { power[i] = 40; ta[i] = 0; }
  const size_t sz[] = { T * TRXSIG_TCH_RX_STATE_BYTES, G * TRXSIG_XCCH_RX_STATE_BYTES, NB, N * 4, NB * 4, NB * 4, X * 4, X * 4, NB * 4 };
  constexpr int nsz = sizeof sz / sizeof sz[0];
  size_t off[nsz], total = 0;
  for (int i = 0; i < nsz; i++) { off[i] = total; total += al(sz[i]); }
  if (total == 0) total = 256;
  TrxDeviceGuard g(trxsig_device(c));
  if (hipMalloc(&rx->d_persist, total) != hipSuccess) {
    delete rx;
    return trx_ctx_fail(c, TRXSIG_ENOMEM, "trxsig_l1msrx_create: device allocation", hipSuccess);
  }
  char *b = (char *)rx->d_persist;
  rx->d_tch_state = (uint8_t *)(b + off[0]); rx->d_ctl_state = (uint8_t *)(b + off[1]); rx->d_active = (uint8_t *)(b + off[2]);
  rx->d_chinfo = (int32_t *)(b + off[3]); rx->d_rssi = (int32_t *)(b + off[4]); rx->d_timing = (int32_t *)(b + off[5]);
  rx->d_power = (int32_t *)(b + off[6]); rx->d_ta = (int32_t *)(b + off[7]); rx->d_last = (int32_t *)(b + off[8]);
  std::vector<uint8_t> ones(NB, 1);
  hipError_t e = hipMemset(rx->d_persist, 0, total);
  if (e == hipSuccess && NB) e = hipMemcpy(rx->d_active, ones.data(), NB, hipMemcpyHostToDevice);
  if (e == hipSuccess && N) e = hipMemcpy(rx->d_chinfo, rx->chinfo.data(), N * 4, hipMemcpyHostToDevice);
  if (e == hipSuccess && X) e = hipMemcpy(rx->d_power, power.data(), X * 4, hipMemcpyHostToDevice);
  if (e == hipSuccess && X) e = hipMemcpy(rx->d_ta, ta.data(), X * 4, hipMemcpyHostToDevice);
  if (e != hipSuccess) {
    (void)hipFree(rx->d_persist);
    delete rx;
    return trx_ctx_fail(c, TRXSIG_EHIP, "trxsig_l1msrx_create: upload", e);
  }
  TrxL1msrxDev &d = rx->dv;
  d.chinfo = rx->d_chinfo; d.active = rx->d_active; d.rssi = rx->d_rssi; d.timing = rx->d_timing;
  d.ord_power = rx->d_power; d.ord_ta = rx->d_ta; d.last = rx->d_last;
  trx_ctx_retain(c);
  *out = rx;
  return TRXSIG_OK;
}

void trxsig_l1msrx_destroy(trxsig_l1msrx *rx) {
  if (!rx) return;
  {
    TrxDeviceGuard g(trxsig_device(rx->c));
    (void)hipStreamSynchronize((hipStream_t)trxsig_get_stream(rx->c));
    if (rx->d_work) (void)hipFree(rx->d_work);
    if (rx->d_persist) (void)hipFree(rx->d_persist);
  }
  trx_ctx_release(rx->c);
  delete rx;
}

int trxsig_l1msrx_channels(const trxsig_l1msrx *rx, int cls) {
  if (!rx || class_slot(cls) < 0) return TRXSIG_EINVAL;
  return rx->n[class_slot(cls)];
}

int trxsig_l1msrx_channel(const trxsig_l1msrx *rx, int cls, int chan, int *arfcn, int *tn, int *kind, int *sub) {
  if (!rx) return TRXSIG_EINVAL;
  const int i = chan_index(rx, cls, chan);
  if (i < 0) return TRXSIG_EINVAL;
  const int32_t v = rx->chinfo[i];
  int k = 0, s = 0;
  map_kind(v >> 20, &k, &s);
  if (arfcn) *arfcn = v & 0xffff;
  if (tn) *tn = (v >> 16) & 15;
  if (kind) *kind = k;
  if (sub) *sub = s;
  return TRXSIG_OK;
}

int trxsig_l1msrx_open(trxsig_l1msrx *rx, int cls, int chan) { return set_active(rx, cls, chan, 1); }
int trxsig_l1msrx_close(trxsig_l1msrx *rx, int cls, int chan) { return set_active(rx, cls, chan, 0); }

int trxsig_l1msrx_state(trxsig_l1msrx *rx, int cls, void **d_state) {
  if (!rx || !d_state) return TRXSIG_EINVAL;
  const int k = class_slot(cls);
  if (k < 0 || k > K_BCCH) return TRXSIG_EINVAL;
  if (k == K_TCH) { *d_state = (void *)rx->d_tch_state; return TRXSIG_OK; }
  const size_t first = k == K_XCCH ? 0 : k == K_CCCH ? (size_t)rx->n[K_XCCH] : (size_t)rx->n[K_XCCH] + rx->n[K_CCCH];
  *d_state = (void *)(rx->d_ctl_state + first * TRXSIG_XCCH_RX_STATE_BYTES);
  return TRXSIG_OK;
}

int trxsig_l1msrx_decode(trxsig_l1msrx *rx, const trxsig_trxgroup_result *res, int fn, int wire, trxsig_l1msrx_out *out) {
  if (!rx) return TRXSIG_EINVAL;
  if (!res || !out || fn < 0 || fn >= kTrxHyperframe || res->n_arfcn != rx->A || res->n_slots <= 0 || (res->n_slots & 7) ||
      res->n_rows < 0 || !res->d_row ||
      (res->n_rows > 0 && (!res->d_valid || !res->d_soft || !res->d_amp || !res->d_toa || res->soft_stride < 148)))
    return fail(rx, "trxsig_l1msrx_decode: bad argument (whole frames from TN 0 of the object's ARFCNs)");
  trxsig_ctx *c = rx->c;
  TrxL1msrxCall k{};
  k.fn = fn; k.n_frames = res->n_slots / 8; k.n_arfcn = rx->A; k.n_rows = res->n_rows; k.soft_stride = res->soft_stride;
  k.sps = trxsig_sps(c); k.wire = wire ? 1 : 0; k.band = rx->band; k.bsic = rx->bsic;
  k.n_tch = rx->n[K_TCH]; k.n_xcch = rx->n[K_XCCH]; k.n_ccch = rx->n[K_CCCH]; k.n_bcch = rx->n[K_BCCH]; k.n_ctl = rx->n_ctl();
  k.n_sch = rx->n[K_SCH]; k.n_fcch = rx->n[K_FCCH];
  // block geometry per mapping: the positions of frames [fn, fn + F) and the blocks they touch
  for (int m = 0; m < TRX_N_DL_MAPS; m++) {
    const long long p0 = trx_map_count(kDl[m], fn), p1 = trx_map_count(kDl[m], (long long)fn + k.n_frames);
    k.p_first[m] = (int32_t)p0;
    k.blk_first[m] = (int32_t)trx_fdiv(p0, 4);
    const int nb = p1 > p0 ? (int)(trx_fdiv(p1 - 1, 4) - trx_fdiv(p0, 4) + 1) : 0;
    if (rx->map_used[0][m] && nb > k.nb_tch) k.nb_tch = nb;
    if (rx->map_used[1][m] && nb > k.nb_ctl) k.nb_ctl = nb;
    if (m == TRX_DL_SCH && k.n_sch) k.sch_cap = (int)(p1 - p0);
    if (m == TRX_DL_FCCH && k.n_fcch) k.fcch_cap = (int)(p1 - p0);
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
  o->ctx = rx->c; o->n_arfcn = rx->A; o->n_xcch = rx->n[K_XCCH]; o->bsic = rx->bsic; o->band = rx->band;
  o->comb = rx->comb.data(); o->ord_power = rx->d_power; o->ord_ta = rx->d_ta;
}
