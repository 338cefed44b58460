// trxsig_l1pdch.cpp -- the packet data channel object's host side (include/trxsig_l1pdch.h): the PDCH slots of the plan, the
// channels' records on the device (one copy: every kernel that writes a record runs after those that read it, and a record's
// writer reads no other record), and per call the block geometry of the two classes and the launches on the context's stream --
// k_l1pdch_stage, the coder's k_fec_pdtch_encode, k_l1pdch_mux, k_l1pdch_commit; k_l1pdch_demux, k_fec_pdtch_decode (PDTCH, then
// PTCCH as CS-1), k_l1pdch_fold, k_l1rx_demux_phy.
#include <hip/hip_runtime_api.h>

#include <cstring>
#include <vector>

#include "trxsig_ctx.h"
#include "trxsig_l1pdch.h"
#include "trxsig_l1pdch_dev.h"
#include "trxsig_plan.h"
#include "trxsig_tablegen.h"

struct trxsig_l1pdch {
  trxsig_ctx *c = nullptr;
  int A = 0, bsic = 0, dir = 0;
  std::vector<uint8_t> comb;
  std::vector<int32_t> chinfo;          // PDTCH channels, then PTCCH: arfcn | tn << 16
  int n[2] = { 0, 0 };
  void *d_persist = nullptr;
  TrxL1pdchChan *d_st = nullptr;
  int32_t *d_chinfo = nullptr, *d_rssi = nullptr, *d_timing = nullptr;
  uint8_t *d_tsc = nullptr;             // 8 x 26 training-sequence bits, as the coder takes them
  TrxWork enc, dec;                     // the per-call workspaces
};

namespace {
constexpr long long kMaxOutBytes = 1LL << 34;

int fail(trxsig_l1pdch *p, const char *what) { return trx_ctx_fail(p ? p->c : nullptr, TRXSIG_EINVAL, what, hipSuccess); }

unsigned ceil4(unsigned x) { return (x + 3u) >> 2; }
}  // namespace

int trxsig_l1pdch_create(trxsig_l1pdch **out, trxsig_ctx *c, int n_arfcn, const uint8_t *h_comb, int bsic, int dir) {
  if (!out || !c) return TRXSIG_EINVAL;
  *out = nullptr;
  if (n_arfcn <= 0 || n_arfcn > 0xffff || !h_comb || bsic < 0 || bsic > 63 || (dir != TRXSIG_L1PDCH_DOWN && dir != TRXSIG_L1PDCH_UP))
    return trx_ctx_fail(c, TRXSIG_EINVAL, "trxsig_l1pdch_create: bad argument (n_arfcn in 1..65535, bsic in 0..63, dir DOWN / UP)",
                        hipSuccess);
  for (int i = 0; i < 8 * n_arfcn; i++) {
    const int v = h_comb[i];
    if (v != 0 && v != 1 && v != 5 && v != 7 && v != TRXSIG_L1PDCH_COMB)
      return trx_ctx_fail(c, TRXSIG_EINVAL, "trxsig_l1pdch_create: h_comb holds a combination other than 0 / 1 / 5 / 7 / 13", hipSuccess);
  }
  trxsig_l1pdch *p = new (std::nothrow) trxsig_l1pdch;
  if (!p) return TRXSIG_ENOMEM;
  p->c = c; p->A = n_arfcn; p->bsic = bsic; p->dir = dir;
  p->comb.assign(h_comb, h_comb + 8 * (size_t)n_arfcn);
  for (int cls = 0; cls < (dir == TRXSIG_L1PDCH_DOWN ? 2 : 1); cls++)
    for (int i = 0; i < 8 * n_arfcn; i++)
      if (h_comb[i] == TRXSIG_L1PDCH_COMB) { p->chinfo.push_back((i >> 3) | ((i & 7) << 16)); p->n[cls]++; }
  const size_t N = p->chinfo.size();
  std::vector<TrxL1pdchChan> rec(N);
  if (N) std::memset(rec.data(), 0, N * sizeof(TrxL1pdchChan));
  for (TrxL1pdchChan &r : rec) {
    r.pend_blk = r.carry_blk = -1;
    for (int i = 0; i < kPdRing; i++) r.ring[i] = -1;
  }
  uint8_t tsc[8 * 26];
  for (int t = 0; t < 8; t++)
    for (int k = 0; k < 26; k++) tsc[26 * t + k] = trx_training_sequence(t)[k] == '1';
  const TrxCarve cv = { N * sizeof(TrxL1pdchChan), N * 4, N * 4, N * 4, sizeof tsc };
  TrxDeviceGuard gd(trxsig_device(c));
  const int rc = trx_device_block(c, "trxsig_l1pdch_create", cv.total,
                                  { { cv.off[0], rec.data(), N * sizeof(TrxL1pdchChan) }, { cv.off[1], p->chinfo.data(), N * 4 },
                                    { cv.off[4], tsc, sizeof tsc } }, &p->d_persist);
  if (rc != TRXSIG_OK) { delete p; return rc; }
  void *b = p->d_persist;
  p->d_st = cv.at<TrxL1pdchChan>(b, 0); p->d_chinfo = cv.at<int32_t>(b, 1); p->d_rssi = cv.at<int32_t>(b, 2);
  p->d_timing = cv.at<int32_t>(b, 3); p->d_tsc = cv.at<uint8_t>(b, 4);
  trx_ctx_retain(c);
  *out = p;
  return TRXSIG_OK;
}

void trxsig_l1pdch_destroy(trxsig_l1pdch *p) {
  if (!p) return;
  trx_object_destroy(p->c, { p->enc.p, p->dec.p, p->d_persist });
  delete p;
}

int trxsig_l1pdch_channels(const trxsig_l1pdch *p, int cls) { return p && (cls == 0 || cls == 1) ? p->n[cls] : TRXSIG_EINVAL; }

int trxsig_l1pdch_channel(const trxsig_l1pdch *p, int cls, int chan, int *arfcn, int *tn) {
  if (!p || (cls != 0 && cls != 1) || chan < 0 || chan >= p->n[cls]) return TRXSIG_EINVAL;
  const int info = p->chinfo[(size_t)(cls ? p->n[0] : 0) + chan];
  if (arfcn) *arfcn = info & 0xffff;
  if (tn) *tn = info >> 16;
  return TRXSIG_OK;
}

int trxsig_l1pdch_grid(const trxsig_l1pdch *p, int fn, int F, int *nb_pdtch, int *nb_ptcch) {
  if (!p || fn < 0 || fn >= (int)kPdHyper || F <= 0 || F > (int)kPdHyper) return TRXSIG_EINVAL;
  int nb[2];
  for (int cls = 0; cls < 2; cls++)
    nb[cls] = p->n[cls] ? (int)(ceil4(pd_pos_before(cls, (unsigned)fn + (unsigned)F)) - ceil4(pd_pos_before(cls, (unsigned)fn))) : 0;
  if (nb_pdtch) *nb_pdtch = nb[0];
  if (nb_ptcch) *nb_ptcch = nb[1];
  return TRXSIG_OK;
}

int trxsig_l1pdch_state(trxsig_l1pdch *p, int cls, void **d_state) {
  if (!p || !d_state || (cls != 0 && cls != 1)) return TRXSIG_EINVAL;
  *d_state = (void *)(p->d_st + (cls ? p->n[0] : 0));
  return TRXSIG_OK;
}

int trxsig_l1pdch_encode(trxsig_l1pdch *p, int fn, int F, const trxsig_l1pdch_in *in, uint8_t *d_bits_onto, uint8_t *d_what_onto,
                         trxsig_l1pdch_out *out) {
  if (!p) return TRXSIG_EINVAL;
  if (!in || !out || fn < 0 || fn >= (int)kPdHyper || F <= 0 || F > (int)kPdHyper || !d_bits_onto != !d_what_onto)
    return fail(p, "trxsig_l1pdch_encode: bad argument (fn in [0, 2715648), n_frames > 0, both onto arrays or neither)");
  if ((long long)p->A * 8 * 148 * F > kMaxOutBytes) return fail(p, "trxsig_l1pdch_encode: output above 2^34 bytes");
  TrxL1pdchEnc e{};
  e.fn = fn; e.n_frames = F; e.n_pd = p->n[0]; e.n_pt = p->n[1]; e.down = p->dir == TRXSIG_L1PDCH_DOWN;
  e.tsc = p->bsic & 7;
  long long units = 0;
  for (int cls = 0; cls < 2; cls++) {
    e.p_first[cls] = pd_pos_before(cls, (unsigned)fn);
    e.p_end[cls] = pd_pos_before(cls, (unsigned)fn + (unsigned)F);
    e.bf[cls] = ceil4(e.p_first[cls]);
    e.nb[cls] = p->n[cls] ? (int)(ceil4(e.p_end[cls]) - e.bf[cls]) : 0;
    e.unit0[cls] = (int)units;
    units += (long long)p->n[cls] * e.nb[cls];
    if (units > TRXSIG_PDTCH_MAX_BLOCKS) return fail(p, "trxsig_l1pdch_encode: more than TRXSIG_PDTCH_MAX_BLOCKS blocks");
  }
  if ((e.nb[0] && (!in->d_pdtch_kind || !in->d_pdtch_cs || !in->d_pdtch_payload)) || (e.nb[1] && (!in->d_ptcch_kind || !in->d_ptcch_payload)))
    return fail(p, "trxsig_l1pdch_encode: NULL grid for a class that has channels");
  const size_t U = (size_t)units, slots = (size_t)p->A * 8 * (size_t)F;
  const bool own = !d_bits_onto;
  const TrxCarve cv = { U * 54, U, U, U * 592, own ? slots * 148 : 0, own ? slots : 0 };
  trxsig_ctx *c = p->c;
  TrxDeviceGuard g(trxsig_device(c));
  const int rc = trx_work_ensure(c, p->enc, cv.total + 256, false, "trxsig_l1pdch_encode: workspace");
  if (rc != TRXSIG_OK) return rc;
  void *b = p->enc.p;
  e.stage = cv.at<uint8_t>(b, 0); e.cs_eff = cv.at<uint8_t>(b, 1); e.tscs = cv.at<uint8_t>(b, 2); e.ebits = cv.at<uint8_t>(b, 3);
  e.bits = own ? cv.at<uint8_t>(b, 4) : d_bits_onto;
  e.what = own ? cv.at<uint8_t>(b, 5) : d_what_onto;
  e.chinfo = p->d_chinfo; e.st = p->d_st;
  e.kind[0] = in->d_pdtch_kind; e.cs = in->d_pdtch_cs; e.payload[0] = in->d_pdtch_payload;
  e.kind[1] = in->d_ptcch_kind; e.payload[1] = in->d_ptcch_payload;
  hipStream_t st = (hipStream_t)trxsig_get_stream(c);
  TrxProfiler *prof = trx_ctx_profiler(c);
  if (own) TRX_HIPCHK(c, hipMemsetAsync(e.bits, 0, (size_t)(cv.total - cv.off[4]), st));   // the grid and its what bytes
  TRX_HIPCHK(c, trx_launch_l1pdch_stage(st, e, prof));
  TRX_HIPCHK(c, trx_launch_fec_pdtch_encode(st, e.stage, e.cs_eff, e.tscs, (int)U, p->d_tsc, e.ebits, prof));
  TRX_HIPCHK(c, trx_launch_l1pdch_mux(st, e, prof));
  out->n_arfcn = p->A; out->n_frames = F; out->d_bits = e.bits; out->d_what = e.what;
  return TRXSIG_OK;
}

int trxsig_l1pdch_decode(trxsig_l1pdch *p, const trxsig_trxgroup_result *res, int fn, int wire, int cs_force,
                         const trxsig_l1pdch *sib, trxsig_l1pdch_dec *out) {
  if (!p) return TRXSIG_EINVAL;
  if (!out || fn < 0 || fn >= (int)kPdHyper || cs_force < -1 || cs_force > 3 || !trx_plan_result_ok(res, p->A) ||
      res->n_slots / 8 > (int)kPdHyper)
    return fail(p, "trxsig_l1pdch_decode: bad argument (whole frames from TN 0 of the object's ARFCNs, cs_force in -1..3)");
  if (sib && (sib->A != p->A || sib->c != p->c || sib->comb != p->comb))
    return fail(p, "trxsig_l1pdch_decode: the sibling's plan is not this object's");
  TrxL1pdchDec d{};
  const int F = res->n_slots / 8;
  d.fn = fn; d.n_frames = F; d.n_arfcn = p->A; d.n_pd = p->n[0]; d.n_pt = p->n[1]; d.n_rows = res->n_rows;
  d.soft_stride = res->soft_stride;
  long long units = 0;
  for (int cls = 0; cls < 2; cls++) {
    const unsigned pf = pd_pos_before(cls, (unsigned)fn), pe = pd_pos_before(cls, (unsigned)fn + (unsigned)F);
    d.p_first[cls] = pf; d.p_end[cls] = pe; d.blk0[cls] = pf >> 2;
    const bool any = p->n[cls] && pe > pf;
    d.nb[cls] = any ? (int)(((pe - 1) >> 2) - (pf >> 2) + 1) : 0;
    d.nclose[cls] = any ? (int)((pe >> 2) - (pf >> 2)) : 0;
    d.unit0[cls] = (int)units;
    units += (long long)p->n[cls] * d.nclose[cls];
    if (units > TRXSIG_PDTCH_MAX_BLOCKS) return fail(p, "trxsig_l1pdch_decode: more than TRXSIG_PDTCH_MAX_BLOCKS blocks");
  }
  const size_t Uc = (size_t)units, N = (size_t)(p->n[0] + p->n[1]);
  const size_t G0 = (size_t)p->n[0] * d.nb[0], G1 = (size_t)p->n[1] * d.nb[1];
  TrxCarve cv = { Uc * 4 * 148 * 4, Uc * 16, Uc * 54, Uc, Uc, Uc, Uc, N * 4 };
  int r0[2];
  for (int cls = 0; cls < 2; cls++) {
    const size_t G = cls ? G1 : G0;
    r0[cls] = cv.add(G * (cls ? 23 : 54));
    for (int i = 0; i < 6; i++) cv.add(G);
    cv.add(G * 4);
  }
  trxsig_ctx *c = p->c;
  TrxDeviceGuard g(trxsig_device(c));
  const int rc = trx_work_ensure(c, p->dec, cv.total + 256, false, "trxsig_l1pdch_decode: workspace");
  if (rc != TRXSIG_OK) return rc;
  void *b = p->dec.p;
  d.rows = cv.at<float>(b, 0); d.index = cv.at<int32_t>(b, 1); d.t_payload = cv.at<uint8_t>(b, 2); d.t_cs = cv.at<uint8_t>(b, 3);
  d.t_dist = cv.at<uint8_t>(b, 4); d.t_ok = cv.at<uint8_t>(b, 5); d.t_usf = cv.at<uint8_t>(b, 6); d.last = cv.at<int32_t>(b, 7);
  for (int cls = 0; cls < 2; cls++) {
    const int r = r0[cls];
    d.payload[cls] = cv.at<uint8_t>(b, r); d.cs[cls] = cv.at<uint8_t>(b, r + 1); d.dist[cls] = cv.at<uint8_t>(b, r + 2);
    d.ok[cls] = cv.at<uint8_t>(b, r + 3); d.usf[cls] = cv.at<uint8_t>(b, r + 4); d.nbur[cls] = cv.at<uint8_t>(b, r + 5);
    d.granted[cls] = cv.at<uint8_t>(b, r + 6); d.bfn[cls] = cv.at<int32_t>(b, r + 7);
  }
  d.chinfo = p->d_chinfo; d.st = p->d_st; d.sib = sib ? sib->d_st : nullptr;
  d.row = res->d_row; d.valid = res->d_valid; d.soft = res->d_soft;
  hipStream_t st = (hipStream_t)trxsig_get_stream(c);
  TrxProfiler *prof = trx_ctx_profiler(c);
  if (N && (d.nb[0] || d.nb[1])) {
    TRX_HIPCHK(c, hipMemsetAsync(d.last, 0xFF, N * 4, st));   // -1: a channel the fold does not visit keeps its RSSI / timing
    TRX_HIPCHK(c, trx_launch_l1pdch_demux(st, d, prof));
    for (int cls = 0; cls < 2; cls++) {
      const size_t u0 = (size_t)d.unit0[cls];
      const int nu = p->n[cls] * d.nclose[cls];
      // the class's units are rows 4 u0 .. of the gathered array; its index entries count from the array's start
      TRX_HIPCHK(c, trx_launch_fec_pdtch_decode(st, d.rows, 148, (long long)Uc * 4, d.index + u0 * 4, nu, wire, cls ? 0 : cs_force,
                                                d.t_payload + u0 * 54, d.t_cs + u0, d.t_dist + u0, d.t_ok + u0, d.t_usf + u0, prof));
    }
    TRX_HIPCHK(c, trx_launch_l1pdch_fold(st, d, prof));
    TRX_HIPCHK(c, trx_launch_l1rx_phy(st, d.last, (int)N, (const trx_c32 *)res->d_amp, res->d_toa, trxsig_sps(c), p->d_rssi, p->d_timing));
  }
  out->n_pdtch = p->n[0]; out->n_ptcch = p->n[1]; out->nb_pdtch = d.nb[0]; out->nb_ptcch = d.nb[1];
  out->d_pdtch_payload = d.payload[0]; out->d_pdtch_cs = d.cs[0]; out->d_pdtch_cs_dist = d.dist[0]; out->d_pdtch_ok = d.ok[0];
  out->d_pdtch_usf = d.usf[0]; out->d_pdtch_nb = d.nbur[0]; out->d_pdtch_granted = d.granted[0]; out->d_pdtch_fn = d.bfn[0];
  out->d_ptcch_payload = d.payload[1]; out->d_ptcch_cs = d.cs[1]; out->d_ptcch_cs_dist = d.dist[1]; out->d_ptcch_ok = d.ok[1];
  out->d_ptcch_usf = d.usf[1]; out->d_ptcch_nb = d.nbur[1]; out->d_ptcch_granted = d.granted[1]; out->d_ptcch_fn = d.bfn[1];
  out->d_pdtch_rssi = p->d_rssi; out->d_pdtch_timing = p->d_timing;
  out->d_ptcch_rssi = p->d_rssi + p->n[0]; out->d_ptcch_timing = p->d_timing + p->n[0];
  return TRXSIG_OK;
}
