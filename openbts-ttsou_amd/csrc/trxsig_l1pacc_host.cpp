// trxsig_l1pacc_host.cpp -- the packet access object's host side (include/trxsig_l1pacc.h): the PDCH slots of the plan, the
// PDCHs' timing-advance tables on the device, and per call the launches on the context's stream -- k_l1pacc_stage, the coder's
// k_fec_access_encode, k_l1pacc_mux; the occasion list (built here, uploaded through pinned blocks taken in turn), the
// access-burst detector of the chosen leg as the C ABI offers it, the coder's k_fec_access_decode, k_l1pacc_fold;
// k_l1pacc_message; k_l1pacc_read.  Nothing here waits for the device.
#include <hip/hip_runtime_api.h>

#include <cstring>
#include <vector>

#include "trxsig_ctx.h"
#include "trxsig_l1pacc.h"
#include "trxsig_l1pacc_dev.h"

struct trxsig_l1pacc {
  trxsig_ctx *c = nullptr;
  int A = 0, bsic = 0, n = 0;
  std::vector<int32_t> chinfo;          // arfcn | tn << 16
  void *d_persist = nullptr;
  TrxL1paccChan *d_st = nullptr;
  int32_t *d_chinfo = nullptr;
  TrxWork enc, det;                     // the per-call workspaces
  TrxPinRing pin;                       // the occasion lists on their way up
};

namespace {
constexpr long long kMaxOutBytes = 1LL << 34;

int fail(trxsig_l1pacc *p, const char *what) { return trx_ctx_fail(p ? p->c : nullptr, TRXSIG_EINVAL, what, hipSuccess); }
bool bad_span(int fn, int F) { return fn < 0 || fn >= (int)kPdHyper || F <= 0 || F > (int)kPdHyper; }
}  // namespace

int trxsig_l1pacc_create(trxsig_l1pacc **out, trxsig_ctx *c, int n_arfcn, const uint8_t *h_comb, int bsic) {
  if (!out || !c) return TRXSIG_EINVAL;
  *out = nullptr;
  if (n_arfcn <= 0 || n_arfcn > 0xffff || !h_comb || bsic < 0 || bsic > 63)
    return trx_ctx_fail(c, TRXSIG_EINVAL, "trxsig_l1pacc_create: bad argument (n_arfcn in 1..65535, bsic in 0..63)", hipSuccess);
  for (int i = 0; i < 8 * n_arfcn; i++) {
    const int v = h_comb[i];
    if (v != 0 && v != 1 && v != 5 && v != 7 && v != TRXSIG_L1PDCH_COMB)
      return trx_ctx_fail(c, TRXSIG_EINVAL, "trxsig_l1pacc_create: h_comb holds a combination other than 0 / 1 / 5 / 7 / 13", hipSuccess);
  }
  trxsig_l1pacc *p = new (std::nothrow) trxsig_l1pacc;
  if (!p) return TRXSIG_ENOMEM;
  p->c = c; p->A = n_arfcn; p->bsic = bsic;
  for (int i = 0; i < 8 * n_arfcn; i++)
    if (h_comb[i] == TRXSIG_L1PDCH_COMB) p->chinfo.push_back((i >> 3) | ((i & 7) << 16));
  p->n = (int)p->chinfo.size();
  const size_t N = p->chinfo.size();
  const TrxCarve cv = { N * sizeof(TrxL1paccChan), N * 4 };
  TrxDeviceGuard gd(trxsig_device(c));
  const int rc = trx_device_block(c, "trxsig_l1pacc_create", cv.total + 256, { { cv.off[1], p->chinfo.data(), N * 4 } }, &p->d_persist);
  if (rc != TRXSIG_OK) { delete p; return rc; }
  p->d_st = cv.at<TrxL1paccChan>(p->d_persist, 0); p->d_chinfo = cv.at<int32_t>(p->d_persist, 1);
  trx_ctx_retain(c);
  *out = p;
  return TRXSIG_OK;
}

void trxsig_l1pacc_destroy(trxsig_l1pacc *p) {
  if (!p) return;
  trxsig_ctx *c = p->c;
  trx_ctx_retain(c);                    // the pinned blocks go after the stream has drained, the context after them
  trx_object_destroy(c, { p->enc.p, p->det.p, p->d_persist });
  {
    TrxDeviceGuard g(trxsig_device(c));
    p->pin.release();
  }
  trx_ctx_release(c);
  delete p;
}

int trxsig_l1pacc_channels(const trxsig_l1pacc *p) { return p ? p->n : TRXSIG_EINVAL; }

int trxsig_l1pacc_channel(const trxsig_l1pacc *p, int chan, int *arfcn, int *tn) {
  if (!p || chan < 0 || chan >= p->n) return TRXSIG_EINVAL;
  if (arfcn) *arfcn = p->chinfo[chan] & 0xffff;
  if (tn) *tn = p->chinfo[chan] >> 16;
  return TRXSIG_OK;
}

int trxsig_l1pacc_grid(const trxsig_l1pacc *p, int fn, int F, int *nb) {
  if (!p || bad_span(fn, F)) return TRXSIG_EINVAL;
  if (nb) *nb = pacc_nb((unsigned)fn, (unsigned)F);
  return TRXSIG_OK;
}

int trxsig_l1pacc_state(trxsig_l1pacc *p, void **d_state) {
  if (!p || !d_state) return TRXSIG_EINVAL;
  *d_state = (void *)p->d_st;
  return TRXSIG_OK;
}

int trxsig_l1pacc_encode(trxsig_l1pacc *p, int fn, int F, const trxsig_l1pacc_in *in, uint8_t *d_bits_onto, uint8_t *d_what_onto,
                         trxsig_l1pacc_out *out) {
  if (!p) return TRXSIG_EINVAL;
  if (!in || !out || bad_span(fn, F) || !d_bits_onto != !d_what_onto || (in->fmt != TRXSIG_ACCESS_8 && in->fmt != TRXSIG_ACCESS_11))
    return fail(p, "trxsig_l1pacc_encode: bad argument (fn in [0, 2715648), n_frames > 0, both onto arrays or neither, fmt 0 / 1)");
  if ((long long)p->A * 8 * 148 * F > kMaxOutBytes) return fail(p, "trxsig_l1pacc_encode: output above 2^34 bytes");
  const long long units = (long long)p->n * F;
  if (units > TRXSIG_ACCESS_MAX_BURSTS) return fail(p, "trxsig_l1pacc_encode: more than TRXSIG_ACCESS_MAX_BURSTS (PDCH, frame) pairs");
  TrxL1paccEnc e{};
  e.fn = fn; e.n_frames = F; e.n_pdch = p->n; e.nb = pacc_nb((unsigned)fn, (unsigned)F); e.fmt = in->fmt; e.bsic = p->bsic;
  e.blk0 = pacc_blk0((unsigned)fn);
  if (p->n && (!in->d_ptcch_kind || !in->d_ptcch_ra || ((uintptr_t)in->d_ptcch_ra & 1) ||
               (e.nb && (!in->d_prach_kind || !in->d_prach_ra || ((uintptr_t)in->d_prach_ra & 1)))))
    return fail(p, "trxsig_l1pacc_encode: NULL or misaligned input array");
  const size_t U = (size_t)units, slots = (size_t)p->A * 8 * (size_t)F;
  const bool own = !d_bits_onto;
  const TrxCarve cv = { U * 2, U, U, U * 148, own ? slots * 148 : 0, own ? slots : 0 };
  trxsig_ctx *c = p->c;
  TrxDeviceGuard g(trxsig_device(c));
  const int rc = trx_work_ensure(c, p->enc, cv.total + 256, false, "trxsig_l1pacc_encode: workspace");
  if (rc != TRXSIG_OK) return rc;
  void *b = p->enc.p;
  e.ra = cv.at<uint16_t>(b, 0); e.fmts = cv.at<uint8_t>(b, 1); e.bsics = cv.at<uint8_t>(b, 2); e.ebits = cv.at<uint8_t>(b, 3);
  e.bits = own ? cv.at<uint8_t>(b, 4) : d_bits_onto;
  e.what = own ? cv.at<uint8_t>(b, 5) : d_what_onto;
  e.chinfo = p->d_chinfo;
  e.ptcch_kind = in->d_ptcch_kind; e.ptcch_ra = in->d_ptcch_ra; e.prach_kind = in->d_prach_kind; e.prach_ra = in->d_prach_ra;
  hipStream_t st = (hipStream_t)trxsig_get_stream(c);
  TrxProfiler *prof = trx_ctx_profiler(c);
  if (own) TRX_HIPCHK(c, hipMemsetAsync(e.bits, 0, (size_t)(cv.total - cv.off[4]), st));   // the grid and its what bytes
  TRX_HIPCHK(c, trx_launch_l1pacc_stage(st, e, prof));
  TRX_HIPCHK(c, trx_launch_fec_access_encode(st, e.ra, e.fmts, e.bsics, (int)U, e.ebits, prof));
  TRX_HIPCHK(c, trx_launch_l1pacc_mux(st, e, prof));
  out->n_arfcn = p->A; out->n_frames = F; out->d_bits = e.bits; out->d_what = e.what;
  return TRXSIG_OK;
}

int trxsig_l1pacc_detect(trxsig_l1pacc *p, const trxsig_c32 *d_samples, int64_t slot_stride, int64_t arfcn_stride, int fn, int F,
                         const uint8_t *h_prach, int fmt, int leg, float detect_thresh, float energy_thresh, int wire,
                         trxsig_l1pacc_det *out) {
  if (!p) return TRXSIG_EINVAL;
  if (!out || !d_samples || bad_span(fn, F) || fmt < -1 || fmt > 1 || (leg != TRXSIG_RACHLEG_DEMOD && leg != TRXSIG_RACHLEG_MLSE))
    return fail(p, "trxsig_l1pacc_detect: bad argument (fn in [0, 2715648), n_frames > 0, fmt in -1..1, leg DEMOD / MLSE)");
  if ((long long)p->n * F > (1LL << 31) - 1) return fail(p, "trxsig_l1pacc_detect: more than 2^31 (PDCH, frame) pairs");
  trxsig_ctx *c = p->c;
  const int sps = trxsig_sps(c), nb = pacc_nb((unsigned)fn, (unsigned)F);
  const unsigned blk0 = pacc_blk0((unsigned)fn);
  // the occasions, PDCH by PDCH in frame order
  std::vector<int32_t> off, len, frame, occ0((size_t)p->n + 1, 0);
  std::vector<uint8_t> okind;
  for (int g = 0; g < p->n; g++) {
    const int a = p->chinfo[g] & 0xffff, tn = p->chinfo[g] >> 16;
    occ0[g] = (int32_t)off.size();
    for (int k = 0; k < F; k++) {
      const unsigned u = (unsigned)fn + (unsigned)k;
      int kind = 0;
      if (pacc_tai(u) >= 0) kind = TRXSIG_L1PACC_PTCCH;
      else if (h_prach && pd_owns(0, u) && h_prach[(size_t)g * nb + ((pd_pos_before(0, u) >> 2) - blk0)]) kind = TRXSIG_L1PACC_PRACH;
      if (!kind) continue;
      const long long o = (8LL * k + tn) * slot_stride + (long long)a * arfcn_stride;
      if (o < 0 || o > 0x7fffffffLL) return fail(p, "trxsig_l1pacc_detect: an occasion's offset does not fit int32");
      if (off.size() >= (size_t)TRXSIG_ACCESS_MAX_BURSTS) return fail(p, "trxsig_l1pacc_detect: more than TRXSIG_ACCESS_MAX_BURSTS occasions");
      off.push_back((int32_t)o); len.push_back((156 + (tn % 4 == 0)) * sps); frame.push_back(k); okind.push_back((uint8_t)kind);
    }
  }
  occ0[p->n] = (int32_t)off.size();
  const size_t n_occ = off.size(), N = (size_t)p->n, G = N * (size_t)F;
  // the workspace: what goes up first (one pinned block, laid out as on the device), then the per-occasion results, then the
  // dense outputs (kind first, tai last: both are cleared below, with everything between)
  TrxCarve cv = { n_occ * 4, n_occ * 4, n_occ * 4, n_occ, (N + 1) * 4 };
  const size_t up_bytes = cv.total;
  const int r_flags = cv.add(n_occ), r_amp = cv.add(n_occ * 8), r_toa = cv.add(n_occ * 4), r_pwr = cv.add(n_occ * 4),
            r_soft = cv.add(n_occ * 148 * 4), r_ra = cv.add(n_occ * 2), r_fmt = cv.add(n_occ), r_tail = cv.add(n_occ), r_bsic = cv.add(n_occ);
  const int o_kind = cv.add(G), o_det = cv.add(G), o_fmt = cv.add(G), o_ok = cv.add(G), o_ta = cv.add(G), o_ra = cv.add(G * 2),
            o_amp = cv.add(G * 8), o_toa = cv.add(G * 4), o_pwr = cv.add(G * 4), o_tai = cv.add(G);
  TrxDeviceGuard g(trxsig_device(c));
  int rc = trx_work_ensure(c, p->det, cv.total + 256, false, "trxsig_l1pacc_detect: workspace");
  if (rc != TRXSIG_OK) return rc;
  void *b = p->det.p;
  hipStream_t st = (hipStream_t)trxsig_get_stream(c);
  TrxProfiler *prof = trx_ctx_profiler(c);
  void *h = nullptr;
  int slot = 0;
  TRX_HIPCHK(c, p->pin.take(up_bytes, &h, &slot));
  if (n_occ) {
    std::memcpy((char *)h + cv.off[0], off.data(), n_occ * 4);
    std::memcpy((char *)h + cv.off[1], len.data(), n_occ * 4);
    std::memcpy((char *)h + cv.off[2], frame.data(), n_occ * 4);
    std::memcpy((char *)h + cv.off[3], okind.data(), n_occ);
  }
  std::memcpy((char *)h + cv.off[4], occ0.data(), (N + 1) * 4);
  TRX_HIPCHK(c, p->pin.upload(slot, b, up_bytes, st));
  TrxL1paccDet d{};
  d.fn = fn; d.n_frames = F; d.n_pdch = p->n; d.n_occ = (int)n_occ; d.sps = sps; d.bsic = p->bsic;
  const int32_t *d_off = cv.at<int32_t>(b, 0), *d_len = cv.at<int32_t>(b, 1);
  d.frame = cv.at<int32_t>(b, 2); d.okind = cv.at<uint8_t>(b, 3); d.occ0 = cv.at<int32_t>(b, 4);
  uint8_t *flags = cv.at<uint8_t>(b, r_flags), *dfmt = cv.at<uint8_t>(b, r_fmt), *dtail = cv.at<uint8_t>(b, r_tail),
          *dbsic = cv.at<uint8_t>(b, r_bsic);
  trxsig_c32 *amp = cv.at<trxsig_c32>(b, r_amp);
  float *toa = cv.at<float>(b, r_toa), *pwr = cv.at<float>(b, r_pwr), *soft = cv.at<float>(b, r_soft);
  uint16_t *dra = cv.at<uint16_t>(b, r_ra);
  d.flags = flags; d.dfmt = dfmt; d.dtail = dtail; d.dbsic = dbsic; d.dra = dra; d.amp = (const trx_c32 *)amp; d.toa = toa; d.avgpwr = pwr;
  d.st = p->d_st;
  d.kind = cv.at<uint8_t>(b, o_kind); d.det = cv.at<uint8_t>(b, o_det); d.fmt = cv.at<uint8_t>(b, o_fmt); d.ok = cv.at<uint8_t>(b, o_ok);
  d.ta = cv.at<uint8_t>(b, o_ta); d.ra = cv.at<uint16_t>(b, o_ra); d.o_amp = cv.at<trx_c32>(b, o_amp); d.o_toa = cv.at<float>(b, o_toa);
  d.o_avgpwr = cv.at<float>(b, o_pwr); d.tai = cv.at<int8_t>(b, o_tai);
  if (G) {
    TRX_HIPCHK(c, hipMemsetAsync(d.kind, 0, cv.off[o_tai] - cv.off[o_kind], st));
    TRX_HIPCHK(c, hipMemsetAsync(d.tai, 0xFF, G, st));
  }
  if (n_occ) {
    rc = leg == TRXSIG_RACHLEG_MLSE
             ? trxsig_mlse_rach_batch(c, d_samples, d_off, d_len, (int)n_occ, detect_thresh, energy_thresh, flags, amp, toa, pwr, nullptr,
                                      nullptr, soft, nullptr, 148, 148)
             : trxsig_detect_demod_rach_batch(c, d_samples, d_off, d_len, (int)n_occ, detect_thresh, energy_thresh, flags, amp, toa, pwr,
                                              soft, nullptr, 148, 148);
    if (rc != TRXSIG_OK) return rc;
    TRX_HIPCHK(c, trx_launch_fec_access_decode(st, soft, 148, (long long)n_occ, nullptr, (int)n_occ, wire, fmt, p->bsic, dra, dfmt, dtail,
                                               dbsic, prof));
    TRX_HIPCHK(c, trx_launch_l1pacc_fold(st, d, prof));
  }
  out->n_pdch = p->n; out->n_frames = F;
  out->d_kind = d.kind; out->d_tai = d.tai; out->d_det = d.det; out->d_fmt = d.fmt; out->d_ok = d.ok; out->d_ra = d.ra;
  out->d_amp = (const trxsig_c32 *)d.o_amp; out->d_toa = d.o_toa; out->d_avgpwr = d.o_avgpwr; out->d_ta = d.ta;
  return TRXSIG_OK;
}

int trxsig_l1pacc_ta_message(trxsig_l1pacc *p, uint8_t *d_kind, uint8_t *d_payload, int nb_pt) {
  if (!p) return TRXSIG_EINVAL;
  if (nb_pt < 0 || (long long)p->n * nb_pt > TRXSIG_PDTCH_MAX_BLOCKS || (p->n && nb_pt && (!d_kind || !d_payload)))
    return fail(p, "trxsig_l1pacc_ta_message: bad argument");
  trxsig_ctx *c = p->c;
  TrxDeviceGuard g(trxsig_device(c));
  TRX_HIPCHK(c, trx_launch_l1pacc_message((hipStream_t)trxsig_get_stream(c), p->d_st, p->n, nb_pt, d_kind, d_payload, trx_ctx_profiler(c)));
  return TRXSIG_OK;
}

int trxsig_l1pacc_ta_read(trxsig_l1pacc *p, const trxsig_l1pdch_dec *dec, uint8_t *d_ta) {
  if (!p) return TRXSIG_EINVAL;
  if (!dec || dec->n_ptcch != p->n || dec->nb_ptcch < 0 || (p->n && (!d_ta || (dec->nb_ptcch && (!dec->d_ptcch_payload || !dec->d_ptcch_ok)))))
    return fail(p, "trxsig_l1pacc_ta_read: bad argument (a DOWN object's decode with this plan's PDCHs)");
  trxsig_ctx *c = p->c;
  TrxDeviceGuard g(trxsig_device(c));
  TRX_HIPCHK(c, trx_launch_l1pacc_read((hipStream_t)trxsig_get_stream(c), p->n, dec->nb_ptcch, dec->d_ptcch_payload, dec->d_ptcch_ok, d_ta,
                                       trx_ctx_profiler(c)));
  return TRXSIG_OK;
}
