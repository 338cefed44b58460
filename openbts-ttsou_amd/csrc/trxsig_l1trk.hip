// trxsig_l1trk.hip -- the tracking receiver's kernels (include/trxsig_l1trk.h, host side in trxsig_l1trk.cpp).
// k_l1trk_slice: workgroup (x, y) forms column y's cells x, x + gridDim.x, ... (k_air_cells' grid): the stream samples of the cell
//   come in coalesced, are turned by the NCO (expjLookup of the top 24 phase bits, Complex<float>::operator* in trxsig_dev.h's
//   cmul_sum form, which hands a NaN sample on with the model's words) and go out.  A cell
//   that holds a frequency burst stays in LDS as well: the workgroup forms d[] and e[] from it in float32, sums them in float64
//   (lane, wave, workgroup) and writes the phone's record -- no second pass over HBM.  Workgroup (0, y) also writes column y's
//   status and advances the anchors of phones y, y + gridDim.y, ... from the set the launch reads into the other set.
// k_l1trk_update: a wave per phone over the rows of the phone's columns; integer sums through __shfl_xor, then lane 0 applies
//   the timing rule (a shift-and-subtract floor division: no 64-bit divide), the AFC and the quiet counter.
// k_l1trk_seed / k_l1trk_set: a thread per phone / one thread.
// Built with -ffp-contract=off like every kernel file.
#include "trxsig_dev.h"
#include "trxsig_l1acq_dev.h"
#include "trxsig_l1trk_dev.h"

namespace {

constexpr int kHyper = 2715648;
constexpr double kTurn = 4294967296.0 / 6.283185307179586;   // 2^-32 turn per radian
constexpr long long kTrkWg = 16384;                          // as k_air_cells: the cells beyond go round the loop

// the anchor moved to the call's frame: D = the signed shortest distance modulo the hyperframe
__device__ __forceinline__ void trk_moved(int afn, long long pos, unsigned phase, unsigned step, int fn, int frame_len, long long *P,
                                          unsigned *PH) {
  int d = fn - afn;
  if (d < 0) d += kHyper;
  if (d >= kHyper / 2) d -= kHyper;
  const long long shift = (long long)d * frame_len;
  *P = pos + shift;
  *PH = phase + (unsigned)(unsigned long long)shift * step;
}

__device__ __forceinline__ bool trk_finite(double v) { return fabs(v) <= 1.7976931348623157e308; }

// (long long) of a double that holds an integer below 2^46 in magnitude, in two 32-bit conversions: the compiler's own 64-bit
// conversion splits the value with a fused multiply-add by -2^32 -- exact, but a fused multiply-add, which this library's
// kernels do not contain.  hi = trunc(x / 2^16); x - hi 2^16 is exact and lies inside (-2^16, 2^16).
__device__ __forceinline__ long long trk_d2ll(double x) {
  if (!(fabs(x) < 70368744177664.0)) return 0;
  const int hi = __double2int_rz(x * 1.52587890625e-05);
  const int lo = __double2int_rz(x - (double)hi * 65536.0);
  return (long long)hi * 65536 + lo;
}

template <int SPS>
__global__ __launch_bounds__(256) void k_l1trk_slice(const TrxTables *__restrict__ T, TrxTrkPlan plan, TrxTrkState s, TrxTrkMeas m,
                                                     TrxTrkSlice p) {
  constexpr int kFrame = 1250 * SPS;
  constexpr int L = 142 * SPS;
  __shared__ cx y[157 * SPS];
  __shared__ double red[4][3];
  const int c = blockIdx.y, tid = threadIdx.x;
  const int ph_i = plan.phone[c];
  const bool locked = s.locked[ph_i] != 0;
  const unsigned step = s.step[ph_i];
  long long P;
  unsigned PH;
  trk_moved(s.fn[p.cur][ph_i], s.pos[p.cur][ph_i], s.phase[p.cur][ph_i], step, p.fn, kFrame, &P, &PH);
  const int rows = 8 * p.n_frames;
  const bool is_c0 = plan.c0[ph_i] == c;
  const cx *x = p.streams + (long long)c * p.stream_stride;
  const long long q0 = P - p.n0;                             // the buffer position of stream offset 0

  if (blockIdx.x == 0 && tid == 0) {
    const long long span = (long long)p.n_frames * kFrame;
    uint8_t st = 0;
    if (!locked) st = TRXSIG_TRK_UNLOCKED;
    else if (q0 < 0 || q0 + span > (long long)p.n_samples) st = TRXSIG_TRK_CLIPPED;
    m.status[c] = st;
    for (int q = c; q < plan.n_phones; q += gridDim.y) {     // the anchors: read from set cur, written to the other
      const int afn = s.fn[p.cur][q];
      const long long apos = s.pos[p.cur][q];
      const unsigned aph = s.phase[p.cur][q];
      if (s.locked[q]) {
        long long Pq;
        unsigned PHq;
        trk_moved(afn, apos, aph, s.step[q], p.fn, kFrame, &Pq, &PHq);
        s.fn[p.cur ^ 1][q] = (p.fn + p.n_frames) % kHyper;
        s.pos[p.cur ^ 1][q] = Pq + span;
        s.phase[p.cur ^ 1][q] = PHq + (unsigned)(unsigned long long)span * s.step[q];
      } else {
        s.fn[p.cur ^ 1][q] = afn; s.pos[p.cur ^ 1][q] = apos; s.phase[p.cur ^ 1][q] = aph;
      }
    }
  }

  for (int t = blockIdx.x; t < rows; t += gridDim.x) {
    const int N = SPS * (156 + ((t & 3) == 0));
    const int blk = t >> 2, sl = t & 3;
    const int st = blk * (625 * SPS) + (sl ? (157 + 156 * (sl - 1)) * SPS : 0);   // s_t
    cx *o = p.cells + (long long)t * p.slot_stride + (long long)c * p.col_stride;
    const int f = t >> 3;
    const unsigned f51 = ((unsigned)(p.fn % 51) + (unsigned)f) % 51u;   // 2715648 is a multiple of 51: the wrap does not show
    const bool fcch = is_c0 && (t & 7) == 0 && f51 < 50u && f51 % 10u == 0;
    if (fcch) __syncthreads();                               // the previous frequency burst's readers of y / red are done
    for (int i = tid; i < N; i += 256) {
      const long long q = q0 + st + i;
      cx v = mk(0, 0);
      if (locked && q >= 0 && q < (long long)p.n_samples) {
        const unsigned ph = PH + (unsigned)(st + i) * step;
        v = cmul_sum(x[q], dev_expj_lookup(T, (float)(ph >> 8) * 5.9604644775390625e-8f * TRX_2PI_F));
      }
      o[i] = v;
      if (fcch) y[i] = v;
    }
    if (!fcch) continue;
    __syncthreads();
    double cr = 0.0, ci = 0.0, e = 0.0;
    for (int k = tid; k < L; k += 256) {
      const int n = 3 * SPS + k;
      const cx b = y[n], a = y[n + SPS];
      const float dr = a.i * b.r - a.r * b.i;                // y[n + sps] conj(y[n]) (-j): k_l1acq_fcch's terms
      const float di = -(a.r * b.r + a.i * b.i);
      const float ee = 0.5f * ((b.r * b.r + b.i * b.i) + (a.r * a.r + a.i * a.i));
      cr += (double)dr; ci += (double)di; e += (double)ee;
    }
#pragma unroll
    for (int w = 32; w >= 1; w >>= 1) { cr += __shfl_xor(cr, w, 64); ci += __shfl_xor(ci, w, 64); e += __shfl_xor(e, w, 64); }
    if ((tid & 63) == 0) { red[tid >> 6][0] = cr; red[tid >> 6][1] = ci; red[tid >> 6][2] = e; }
    __syncthreads();
    if (tid == 0) {
      double Cr = 0.0, Ci = 0.0, E = 0.0;
      for (int w = 0; w < 4; w++) { Cr += red[w][0]; Ci += red[w][1]; E += red[w][2]; }
      const unsigned a0 = (unsigned)(p.fn % 51);
      const int j = (int)(trx_trk_fcch_before(a0 + (unsigned)f) - trx_trk_fcch_before(a0));
      bool ok = false;
      if (!locked) { Cr = 0.0; Ci = 0.0; E = 0.0; }
      else if (Cr > 0.0 && E > 0.0 && trk_finite(Cr) && trk_finite(Ci) && trk_finite(E)) {
        const double q = (Cr * Cr + Ci * Ci) / (E * E);
        ok = trk_finite(q) && q > (double)p.fcch_thresh;
      }
      if (j < m.cap) {
        const size_t r = (size_t)ph_i * m.cap + j;
        m.fcch_fn[r] = (p.fn + f) % kHyper;
        m.fcch_c[2 * r] = Cr; m.fcch_c[2 * r + 1] = Ci; m.fcch_e[r] = E; m.fcch_ok[r] = ok ? 1 : 0;
      }
    }
  }
}

// floor(a / b), b > 0, without a 64-bit divide (the compiler's expansion estimates the reciprocal in float32 with a fused
// multiply-add, which this library's kernels do not contain): restoring division of |a|, the floor fixed up by the sign
__device__ __forceinline__ long long trk_floor_div(long long a, long long b) {
  const bool neg = a < 0;
  unsigned long long n = neg ? 0ull - (unsigned long long)a : (unsigned long long)a, q = 0, r = 0;
  const unsigned long long d = (unsigned long long)b;
  for (int i = 63; i >= 0; i--) {
    r = (r << 1) | ((n >> i) & 1ull);
    if (r >= d) { r -= d; q |= 1ull << i; }
  }
  if (!neg) return (long long)q;
  return r ? -(long long)q - 1 : -(long long)q;
}

__global__ __launch_bounds__(64) void k_l1trk_update(int sps, TrxTrkPlan plan, TrxTrkState s, TrxTrkMeas m, int cur, int fn,
                                                     int n_slots, int n_rows, int n_fcch, const int32_t *__restrict__ row,
                                                     const uint8_t *__restrict__ valid, const float *__restrict__ toa,
                                                     const uint8_t *__restrict__ use, int afc_shift, int toa_gate) {
  const int p = blockIdx.x, lane = threadIdx.x;
  if (!s.locked[p]) {
    if (lane == 0) { s.toa_sum[p] = 0; s.toa_n[p] = 0; s.adj[p] = 0; s.afc_n[p] = 0; s.afc_delta[p] = 0; }
    return;
  }
  const int c_lo = plan.col_start[p], nc = plan.col_start[p + 1] - c_lo, c0 = plan.c0[p];
  const double scale = (double)(256 / sps);
  const unsigned a0 = (unsigned)(fn % 51);
  long long S = 0;
  int N = 0;
  for (int t = lane; t < n_slots; t += 64)                    // a lane per slot, the phone's columns in turn (no division)
   for (int j = 0; j < nc; j++) {
    const int c = plan.col_list[c_lo + j];
    const size_t cell = (size_t)t * plan.n_cols + c;
    const int r = row[cell];
    if (r < 0 || r >= n_rows || !valid[r] || (use && !use[cell])) continue;
    if (c == c0 && (t & 7) == 0) {
      const unsigned f51 = (a0 + (unsigned)(t >> 3)) % 51u;  // 2715648 is a multiple of 51: the wrap does not show
      if (f51 < 50u && f51 % 10u <= 1u) continue;            // an FCCH or SCH frame
    }
    const double v = (double)toa[r] * scale;
    if (!(fabs(v) <= (double)toa_gate + 1.0)) continue;     // (not finite, or far beyond the gate)
    const long long q = __double2int_rn(v);              // |v| <= 2^24 + 1
    if (q > toa_gate || q < -(long long)toa_gate) continue;
    S += q; N += 1;
  }
#pragma unroll
  for (int w = 32; w >= 1; w >>= 1) { S += __shfl_xor(S, w, 64); N += __shfl_xor(N, w, 64); }
  if (lane != 0) return;
  const unsigned step = s.step[p];
  long long adj = 0;
  if (N >= 1) {
    adj = trk_floor_div(2 * S * sps + 256LL * N, 512LL * N);
    s.pos[cur][p] += adj;
    s.phase[cur][p] += (unsigned)(unsigned long long)adj * step;
  }
  double scr = 0.0, sci = 0.0;
  int K = 0;
  const int nrec = n_fcch < m.cap ? n_fcch : m.cap;
  if (c0 >= 0)
    for (int j = 0; j < nrec; j++) {
      const size_t r = (size_t)p * m.cap + j;
      if (m.fcch_ok[r]) { scr += m.fcch_c[2 * r]; sci += m.fcch_c[2 * r + 1]; K++; }
    }
  long long delta = 0;
  if (K >= 1) {
    const float a = acq_atan2((float)sci, (float)scr);
    delta = trk_d2ll(rint((double)(-a) / (double)sps * kTurn));
    s.step[p] = step + (unsigned)(unsigned long long)(delta >> afc_shift);
  }
  s.quiet[p] = (N + K > 0) ? 0 : s.quiet[p] + 1;
  s.toa_sum[p] = S; s.toa_n[p] = N; s.adj[p] = adj; s.afc_n[p] = K; s.afc_delta[p] = delta;
}

__global__ __launch_bounds__(64) void k_l1trk_seed(int sps, TrxTrkPlan plan, TrxTrkState s, int cur, int n_streams,
                                                   const uint8_t *__restrict__ acq_state, const int32_t *__restrict__ w0,
                                                   const float *__restrict__ toa, const float *__restrict__ omega,
                                                   const int32_t *__restrict__ rfn, const int32_t *__restrict__ src) {
  const int p = blockIdx.x * 64 + threadIdx.x;
  if (p >= plan.n_phones) return;
  const int k = src[p];
  if (k < 0 || k >= n_streams) return;
  if (acq_state[k] != 15) { s.locked[p] = 0; return; }
  const long long pos0 = trk_d2ll(floor((double)w0[k] + (double)toa[k] + 0.5));
  s.pos[cur][p] = pos0 + 1250LL * sps;
  int f = rfn[k] + 1;
  if (f >= kHyper || f < 0) f = 0;                           // (a decoded RFN is inside the hyperframe)
  s.fn[cur][p] = f;
  s.step[p] = (unsigned)(unsigned long long)trk_d2ll(rint((double)omega[k] * kTurn));
  s.phase[cur][p] = 0u;
  s.quiet[p] = 0;
  s.locked[p] = 1;
}

__global__ void k_l1trk_set(TrxTrkState s, int cur, int phone, int locked, int fn, long long pos, unsigned step, unsigned phase) {
  s.locked[phone] = locked ? 1 : 0; s.fn[cur][phone] = fn; s.pos[cur][phone] = pos; s.step[phone] = step; s.phase[cur][phone] = phase;
  s.quiet[phone] = 0;
}

}  // namespace

hipError_t trx_launch_l1trk_seed(hipStream_t st, int sps, const TrxTrkPlan &plan, const TrxTrkState &s, int cur, int n_streams,
                                 const uint8_t *acq_state, const int32_t *w0, const float *toa, const float *omega, const int32_t *rfn,
                                 const int32_t *src) {
  k_l1trk_seed<<<dim3((plan.n_phones + 63) / 64), dim3(64), 0, st>>>(sps, plan, s, cur, n_streams, acq_state, w0, toa, omega, rfn, src);
  return hipGetLastError();
}

hipError_t trx_launch_l1trk_set(hipStream_t st, const TrxTrkState &s, int cur, int phone, int locked, int fn, long long pos,
                                uint32_t step, uint32_t phase) {
  k_l1trk_set<<<dim3(1), dim3(1), 0, st>>>(s, cur, phone, locked, fn, pos, step, phase);
  return hipGetLastError();
}

hipError_t trx_launch_l1trk_slice(hipStream_t st, int sps, const TrxTables *dT, const TrxTrkPlan &plan, const TrxTrkState &s,
                                  const TrxTrkMeas &m, const TrxTrkSlice &p) {
  if (p.n_frames <= 0 || plan.n_cols <= 0 || plan.n_cols > 65535) return hipErrorInvalidValue;
  const long long rows = 8LL * p.n_frames;
  long long gx = kTrkWg / plan.n_cols > 0 ? kTrkWg / plan.n_cols : 1;
  if (gx > rows) gx = rows;
  const dim3 grid((unsigned)gx, (unsigned)plan.n_cols), block(256);
  switch (sps) {
    case 1: k_l1trk_slice<1><<<grid, block, 0, st>>>(dT, plan, s, m, p); break;
    case 2: k_l1trk_slice<2><<<grid, block, 0, st>>>(dT, plan, s, m, p); break;
    case 4: k_l1trk_slice<4><<<grid, block, 0, st>>>(dT, plan, s, m, p); break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

hipError_t trx_launch_l1trk_update(hipStream_t st, int sps, const TrxTrkPlan &plan, const TrxTrkState &s, const TrxTrkMeas &m, int cur,
                                   int fn, int n_slots, int n_rows, int n_fcch, const int32_t *row, const uint8_t *valid, const float *toa,
                                   const uint8_t *use, int afc_shift, int toa_gate) {
  k_l1trk_update<<<dim3(plan.n_phones), dim3(64), 0, st>>>(sps, plan, s, m, cur, fn, n_slots, n_rows, n_fcch, row, valid, toa, use, afc_shift,
                                                          toa_gate);
  return hipGetLastError();
}
