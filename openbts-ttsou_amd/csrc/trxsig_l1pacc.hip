// trxsig_l1pacc.hip -- the packet access object's kernels (include/trxsig_l1pacc.h, host side in trxsig_l1pacc_host.cpp).  The
// access burst's coder and decoder exist once, in trxsig_fec.hip, and the detector in trxsig_rach.hip / trxsig_mlse_access.hip:
// the host runs k_fec_access_encode between k_l1pacc_stage and k_l1pacc_mux, and the detector and k_fec_access_decode before
// k_l1pacc_fold.  The kernels here only place, move and fold; the frame arithmetic is trxsig_l1pacc_dev.h's.
//
//   k_l1pacc_stage: a lane per (PDCH, frame of the call): what the handset sends there, if anything -- its TAI's entry on a
//     PTCCH/U frame, the block's entry on a frame of a block B0..B11 -- as the coder's inputs; format 255, which the coder turns
//     into a zero row and the mux skips, where nothing is sent or the word does not fit the format.
//   k_l1pacc_mux: a wave per (PDCH, frame): 37 lanes move four bytes each of a sent burst into its slot, lane 0 writes the what
//     byte.  Nothing else of the grid is touched.
//   k_l1pacc_fold: a wave per PDCH, after the detector and the decoder: its occasions' results into the dense per-frame
//     arrays, a lane an occasion; then lane n < 16 walks the PDCH's occasions in frame order and takes every PTCCH/U burst of
//     TAI n with ok into the table (the results it reads are the earlier kernels', so the two halves need no order).
//   k_l1pacc_message, k_l1pacc_read: the table into PTCCH/D payloads; PTCCH/D payloads into a handset's table.
#include "trxsig_l1pacc_dev.h"

namespace {

constexpr int kWhatPacc = 9;                                 // TRXSIG_L1TX_PACC

__global__ __launch_bounds__(256) void k_l1pacc_stage(TrxL1paccEnc e) {
  const unsigned unit = blockIdx.x * 256u + threadIdx.x;     // at most TRXSIG_ACCESS_MAX_BURSTS units: 32-bit arithmetic throughout
  if (unit >= (unsigned)e.n_pdch * (unsigned)e.n_frames) return;
  const int g = (int)(unit / (unsigned)e.n_frames), k = (int)(unit - (unsigned)g * (unsigned)e.n_frames);
  const unsigned u = (unsigned)e.fn + (unsigned)k;
  unsigned kind = 0, ra = 0;
  const int tai = pacc_tai(u);
  if (tai >= 0) {
    kind = e.ptcch_kind[g * 16 + tai]; ra = e.ptcch_ra[g * 16 + tai];
  } else if (pd_owns(0, u)) {
    const unsigned q = pd_pos_before(0, u);
    const size_t i = ((size_t)g * e.nb + ((q >> 2) - e.blk0)) * 4 + (q & 3u);
    kind = e.prach_kind[i]; ra = e.prach_ra[i];
  }
  const bool sent = kind == 1 && ra < (e.fmt ? 2048u : 256u);
  e.ra[unit] = (uint16_t)ra;
  e.fmts[unit] = sent ? (uint8_t)e.fmt : (uint8_t)255;
  e.bsics[unit] = (uint8_t)e.bsic;
}

__global__ __launch_bounds__(256) void k_l1pacc_mux(TrxL1paccEnc e) {
  const int lane = threadIdx.x & 63;
  const unsigned unit = blockIdx.x * 4u + (threadIdx.x >> 6);
  if (unit >= (unsigned)e.n_pdch * (unsigned)e.n_frames) return;
  if (e.fmts[unit] > 1) return;
  const int g = (int)(unit / (unsigned)e.n_frames), k = (int)(unit - (unsigned)g * (unsigned)e.n_frames);
  const int info = e.chinfo[g], a = info & 0xffff, tn = info >> 16;
  const size_t slot = (size_t)a * 8 * (size_t)e.n_frames + 8 * (size_t)k + tn;
  const uint8_t *src = e.ebits + (size_t)unit * 148;         // 4-byte aligned: the workspace's region, 148 a multiple of 4
  uint8_t *dst = e.bits + slot * 148;
  if (lane < 37) {
    const unsigned v = *reinterpret_cast<const unsigned *>(src + 4 * lane);
    if (((uintptr_t)dst & 3) == 0) *reinterpret_cast<unsigned *>(dst + 4 * lane) = v;
    else for (int i = 0; i < 4; i++) dst[4 * lane + i] = (uint8_t)(v >> (8 * i));
  }
  if (lane == 0) e.what[slot] = kWhatPacc;
}

struct PaccResult { bool det, ok; int ta; };
__device__ __forceinline__ PaccResult pacc_result(const TrxL1paccDet &d, int i) {
  PaccResult r;
  r.det = (d.flags[i] & TRXSIG_F_DETECT) != 0;
  r.ok = r.det && d.dtail[i] != 0 && d.dbsic[i] == (uint8_t)d.bsic;
  const float t = d.toa[i] / (float)d.sps;
  r.ta = !(t >= 0.0F) ? 0 : t >= 63.0F ? 63 : (int)(t + 0.5F);   // t < 0 ? 0 : min(63, (int)(t + 0.5F)); a NaN gives 0
  if (r.ta > 63) r.ta = 63;
  return r;
}

__global__ __launch_bounds__(256) void k_l1pacc_fold(TrxL1paccDet d) {
  const int lane = threadIdx.x & 63, g = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (g >= d.n_pdch) return;
  const int i0 = d.occ0[g], i1 = d.occ0[g + 1];
  for (int i = i0 + lane; i < i1; i += 64) {
    const PaccResult r = pacc_result(d, i);
    const int k = d.frame[i];
    const size_t c = (size_t)g * d.n_frames + k;
    const int kind = d.okind[i];
    d.kind[c] = (uint8_t)kind;
    d.tai[c] = (int8_t)(kind == 1 ? pacc_tai((unsigned)d.fn + (unsigned)k) : -1);
    d.det[c] = r.det;
    d.fmt[c] = r.det ? d.dfmt[i] : (uint8_t)0;
    d.ok[c] = r.ok;
    d.ra[c] = r.det ? d.dra[i] : (uint16_t)0;
    d.ta[c] = (uint8_t)(r.det ? r.ta : 0);
    d.o_amp[c] = d.amp[i];
    d.o_toa[c] = d.toa[i];
    d.o_avgpwr[c] = d.avgpwr[i];
  }
  if (lane >= 16) return;
  TrxL1paccChan &S = d.st[g];
  for (int i = i0; i < i1; i++) {
    if (d.okind[i] != 1) continue;
    const unsigned u = (unsigned)d.fn + (unsigned)d.frame[i];
    if (pacc_tai(u) != lane) continue;
    const PaccResult r = pacc_result(d, i);
    if (!r.ok) continue;
    S.ta[lane] = r.ta;
    S.fn[lane] = (int32_t)(u >= kPdHyper ? u - kPdHyper : u);
    S.valid[lane] = 1;
  }
}

__global__ __launch_bounds__(256) void k_l1pacc_message(const TrxL1paccChan *__restrict__ state, int n_pdch, int nb_pt,
                                                        uint8_t *__restrict__ kind, uint8_t *__restrict__ payload) {
  const unsigned j = blockIdx.x * 256u + threadIdx.x;        // (PDCH, block, octet 0..23: octet 23 is the kind byte's turn)
  if (j >= (unsigned)n_pdch * (unsigned)nb_pt * 24u) return;  // at most TRXSIG_PDTCH_MAX_BLOCKS * 24 < 2^32
  const unsigned gb = j / 24u;
  const int i = (int)(j - gb * 24u), g = (int)(gb / (unsigned)nb_pt);
  if (i == 23) { kind[gb] = 1; return; }
  uint8_t v = 0x2B;
  if (i < 16) v = state[g].valid[i] ? (uint8_t)(state[g].ta[i] & 0x7F) : (uint8_t)0x7F;
  payload[(size_t)gb * 23 + i] = v;
}

__global__ __launch_bounds__(256) void k_l1pacc_read(int n_pdch, int nb, const uint8_t *__restrict__ payload,
                                                     const uint8_t *__restrict__ ok, uint8_t *__restrict__ ta) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= n_pdch * 16) return;
  const int g = j >> 4, i = j & 15;
  for (int b = nb - 1; b >= 0; b--) {
    if (!ok[(size_t)g * nb + b]) continue;
    const uint8_t v = payload[((size_t)g * nb + b) * 23 + i];
    if (v <= 63) ta[j] = v;                                  // 0x7F: the message holds no value for this TAI
    return;
  }
}

}  // namespace

hipError_t trx_launch_l1pacc_stage(hipStream_t st, const TrxL1paccEnc &e, TrxProfiler *prof) {
  const long long units = (long long)e.n_pdch * e.n_frames;
  if (units <= 0) return hipSuccess;
  if (prof) prof->begin(TRXSIG_K_FEC, st);
  k_l1pacc_stage<<<dim3((unsigned)((units + 255) / 256)), dim3(256), 0, st>>>(e);
  if (prof) prof->end(TRXSIG_K_FEC, st);
  return hipGetLastError();
}

hipError_t trx_launch_l1pacc_mux(hipStream_t st, const TrxL1paccEnc &e, TrxProfiler *prof) {
  const long long units = (long long)e.n_pdch * e.n_frames;
  if (units <= 0) return hipSuccess;
  if (prof) prof->begin(TRXSIG_K_FEC, st);
  k_l1pacc_mux<<<dim3((unsigned)((units + 3) / 4)), dim3(256), 0, st>>>(e);
  if (prof) prof->end(TRXSIG_K_FEC, st);
  return hipGetLastError();
}

hipError_t trx_launch_l1pacc_fold(hipStream_t st, const TrxL1paccDet &d, TrxProfiler *prof) {
  if (d.n_pdch <= 0) return hipSuccess;
  if (prof) prof->begin(TRXSIG_K_FEC, st);
  k_l1pacc_fold<<<dim3((unsigned)((d.n_pdch + 3) / 4)), dim3(256), 0, st>>>(d);
  if (prof) prof->end(TRXSIG_K_FEC, st);
  return hipGetLastError();
}

hipError_t trx_launch_l1pacc_message(hipStream_t st, const TrxL1paccChan *state, int n_pdch, int nb_pt, uint8_t *kind, uint8_t *payload,
                                     TrxProfiler *prof) {
  const long long n = (long long)n_pdch * nb_pt * 24;
  if (n <= 0) return hipSuccess;
  if (prof) prof->begin(TRXSIG_K_FEC, st);
  k_l1pacc_message<<<dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st>>>(state, n_pdch, nb_pt, kind, payload);
  if (prof) prof->end(TRXSIG_K_FEC, st);
  return hipGetLastError();
}

hipError_t trx_launch_l1pacc_read(hipStream_t st, int n_pdch, int nb, const uint8_t *payload, const uint8_t *ok, uint8_t *ta,
                                  TrxProfiler *prof) {
  if (n_pdch <= 0 || nb <= 0) return hipSuccess;
  if (prof) prof->begin(TRXSIG_K_FEC, st);
  k_l1pacc_read<<<dim3((unsigned)((n_pdch * 16 + 255) / 256)), dim3(256), 0, st>>>(n_pdch, nb, payload, ok, ta);
  if (prof) prof->end(TRXSIG_K_FEC, st);
  return hipGetLastError();
}
