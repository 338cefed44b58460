// trxsig_l1acq.hip -- the acquisition object's kernels (include/trxsig_l1acq.h, host side in trxsig_l1acq.cpp).
//
// Stage 1, the FCCH search -- this project's own arithmetic, pinned by a float64 model within 8 (L + 8) 2^-24:
// k_l1acq_fcch: a workgroup takes one stream and a tile of 8 / sps whole segments of L = 142 sps samples plus one halo segment.
//   The tile's samples are loaded once, coalesced, into LDS; a wave takes a segment at a time: each lane forms d[] and e[] of
//   its consecutive samples, the inclusive prefix and suffix scans run inside the lane, across the lanes with __shfl_up /
//   __shfl_down (an exclusive scan of the lanes' totals, added once: no subtraction anywhere) and go to LDS -- the suffixes of
//   the tile's segments, the prefixes of the segments one further.  A window is one suffix plus one prefix: no float32 sum
//   spans more than L terms.  Each thread evaluates its window starts; a block argmax (largest m, then smallest k) writes
//   (m, k, C, E) of the tile.
// k_l1acq_pick: a wave per stream picks the winner over the tiles by the same rule, forms the angle -- an octant reduction and
//   an odd polynomial in plain multiplies and adds: the device library's atan2f is built on fused multiply-adds -- and sets up
//   stage 2.  Two plain launches; no workgroup waits for another.
//
// Stage 2, the SCH detector -- the reference's primitives, bit for bit:
// k_l1acq_shift: frequencyShift (sigProcLib.cpp:432-471; k_frequency_shift's loop, trxsig_prim.hip) of each window into the
//   object's workspace row.  The correlation over every lag and peakDetect are trxsig_prim.hip's kernels on those rows.
// k_l1acq_verdict: the tail of analyzeTrafficBurst (:961-1000) for the extended training sequence, a thread per window, and the
//   demodulator's segment.  demodulateBurst is k_demod (trxsig_demod.h), exact arithmetic.
// k_l1acq_candidates, k_l1acq_fit_verdict: TRXSIG_SCHDET_FIT's two halves of the verdict, round k_sch_fit (trxsig_sch_fit.hip):
//   the geometry gate with amp, TOA and the segment before it, q > thresh behind it.  k_l1acq_verdict is untouched by them.
// Built with -ffp-contract=off like every kernel file.
#include "trxsig_dev.h"
#include "trxsig_l1acq_dev.h"

namespace {

constexpr int kAcqThreads = 256;

__device__ __forceinline__ bool acq_finite(float v) { return fabsf(v) <= 3.402823466e+38F; }   // false for NaN and infinities

// larger m wins; equal m: the smaller k
__device__ __forceinline__ void acq_take(float &m, int &k, float om, int ok) {
  const bool take = (om > m) || (om == m && ok < k);
  m = take ? om : m;
  k = take ? ok : k;
}

template <int SPS>
__global__ __launch_bounds__(kAcqThreads) void k_l1acq_fcch(const cx *__restrict__ x, long long stride, int N, int n_tiles,
                                                            float *__restrict__ tile_m, int32_t *__restrict__ tile_k,
                                                            cx *__restrict__ tile_c, float *__restrict__ tile_e) {
  constexpr int L = TRX_ACQ_FCCH_SYMS * SPS;               // samples per segment and per window
  constexpr int TS = 8 / SPS;                              // segments per tile
  constexpr int W = TS * L;                                // window starts per tile (TRX_ACQ_TILE_SYMS)
  constexpr int NS = W + L;                                // d / e entries the tile needs: its segments and the halo segment
  constexpr int NX = NS + SPS;                             // samples behind them
  constexpr int CH = (L + 63) / 64;                        // consecutive entries per lane in a scan
  static_assert(W == TRX_ACQ_TILE_SYMS, "tile geometry");
  __shared__ cx xs[NX];
  __shared__ float suf[3][W], pre[3][W];                   // [Re d, Im d, e]; suf: segments 0 .. TS-1, pre: segments 1 .. TS
  __shared__ float red_m[kAcqThreads / 64];
  __shared__ int red_k[kAcqThreads / 64];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int tile = blockIdx.x, s = blockIdx.y;
  const int n0 = tile * W;                                 // the tile's first sample / window start
  const int Nd = N - SPS;                                  // d[] and e[] exist on [0, Nd)
  const int Kmax = Nd - L;                                 // the last window start (>= 0: the host launches nothing otherwise)
  const cx *xv = x + (long long)s * stride;

  for (int i = tid; i < NX; i += kAcqThreads) xs[i] = (n0 + i < N) ? xv[n0 + i] : mk(0, 0);
  __syncthreads();

  for (int seg = wave; seg <= TS; seg += kAcqThreads / 64) {
    float vr[CH], vi[CH], ve[CH];
#pragma unroll
    for (int q = 0; q < CH; q++) {
      const int r = lane * CH + q, i = seg * L + r;
      float dr = 0.0f, di = 0.0f, e = 0.0f;
      if (r < L && n0 + i < Nd) {
        const cx b = xs[i], a = xs[i + SPS];
        dr = a.i * b.r - a.r * b.i;                        // x[n + sps] conj(x[n]) (-j)
        di = -(a.r * b.r + a.i * b.i);
        e = 0.5f * ((b.r * b.r + b.i * b.i) + (a.r * a.r + a.i * a.i));
      }
      vr[q] = dr; vi[q] = di; ve[q] = e;
    }
    if (seg >= 1) {                                        // inclusive prefix scan -> pre[.][(seg - 1) L + r]
      float pr[CH], pi[CH], pe[CH];
      float tr = 0.0f, ti = 0.0f, te = 0.0f;
#pragma unroll
      for (int q = 0; q < CH; q++) { tr += vr[q]; ti += vi[q]; te += ve[q]; pr[q] = tr; pi[q] = ti; pe[q] = te; }
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {                   // inclusive scan of the lanes' totals
        const float ur = __shfl_up(tr, o, 64), ui = __shfl_up(ti, o, 64), ue = __shfl_up(te, o, 64);
        if (lane >= o) { tr += ur; ti += ui; te += ue; }
      }
      float xr = __shfl_up(tr, 1, 64), xi = __shfl_up(ti, 1, 64), xe = __shfl_up(te, 1, 64);   // exclusive: the lanes before
      if (lane == 0) { xr = 0.0f; xi = 0.0f; xe = 0.0f; }
#pragma unroll
      for (int q = 0; q < CH; q++) {
        const int r = lane * CH + q;
        if (r < L) {
          const int o = (seg - 1) * L + r;
          pre[0][o] = xr + pr[q]; pre[1][o] = xi + pi[q]; pre[2][o] = xe + pe[q];
        }
      }
    }
    if (seg < TS) {                                        // inclusive suffix scan -> suf[.][seg L + r]
      float sr[CH], si[CH], se[CH];
      float tr = 0.0f, ti = 0.0f, te = 0.0f;
#pragma unroll
      for (int q = CH - 1; q >= 0; q--) { tr += vr[q]; ti += vi[q]; te += ve[q]; sr[q] = tr; si[q] = ti; se[q] = te; }
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const float ur = __shfl_down(tr, o, 64), ui = __shfl_down(ti, o, 64), ue = __shfl_down(te, o, 64);
        if (lane + o < 64) { tr += ur; ti += ui; te += ue; }
      }
      float xr = __shfl_down(tr, 1, 64), xi = __shfl_down(ti, 1, 64), xe = __shfl_down(te, 1, 64);   // the lanes after
      if (lane == 63) { xr = 0.0f; xi = 0.0f; xe = 0.0f; }
#pragma unroll
      for (int q = 0; q < CH; q++) {
        const int r = lane * CH + q;
        if (r < L) {
          const int o = seg * L + r;
          suf[0][o] = xr + sr[q]; suf[1][o] = xi + si[q]; suf[2][o] = xe + se[q];
        }
      }
    }
  }
  __syncthreads();

  // window start n0 + idx, idx = jj L + r: the suffix of segment jj from r, the prefix of segment jj + 1 of length r
  auto window = [&](int idx, float *cr, float *ci, float *e) {
    const int jj = idx / L, r = idx - jj * L;
    float a = suf[0][idx], b = suf[1][idx], c = suf[2][idx];
    if (r > 0) { a += pre[0][idx - 1]; b += pre[1][idx - 1]; c += pre[2][idx - 1]; }
    *cr = a; *ci = b; *e = c;
  };
  float bm = -1.0f;
  int bk = 0x7fffffff;
  for (int idx = tid; idx < W; idx += kAcqThreads) {
    const int k = n0 + idx;
    if (k > Kmax) break;
    float cr, ci, e;
    window(idx, &cr, &ci, &e);
    const float q = (cr * cr + ci * ci) / (e * e);
    const float m = (cr > 0.0f && e > 0.0f && acq_finite(cr) && acq_finite(ci) && acq_finite(e) && acq_finite(q)) ? q : 0.0f;
    if (m > bm) { bm = m; bk = k; }                        // a thread's k ascend: strict > keeps the first
  }
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) acq_take(bm, bk, __shfl_xor(bm, o, 64), __shfl_xor(bk, o, 64));
  if (lane == 0) { red_m[wave] = bm; red_k[wave] = bk; }
  __syncthreads();
  if (tid == 0) {
    for (int w = 1; w < kAcqThreads / 64; w++) acq_take(bm, bk, red_m[w], red_k[w]);
    const size_t o = (size_t)s * n_tiles + tile;
    float cr = 0.0f, ci = 0.0f, e = 0.0f;
    if (bk != 0x7fffffff) window(bk - n0, &cr, &ci, &e);
    else { bm = -1.0f; bk = -1; }                          // (a tile past the last window: the host launches none)
    tile_m[o] = bm; tile_k[o] = bk; tile_c[o] = mk(cr, ci); tile_e[o] = e;
  }
}

// acq_atan2 (the angle of C): trxsig_l1acq_dev.h -- the tracking receiver's AFC uses it too

__global__ __launch_bounds__(64) void k_l1acq_pick(int sps, long long stride, int N, int n_streams, int n_tiles,
                                                   const float *__restrict__ tile_m, const int32_t *__restrict__ tile_k,
                                                   const cx *__restrict__ tile_c, const float *__restrict__ tile_e,
                                                   float fcch_thresh, TrxAcqStreams o) {
  const int s = blockIdx.x, lane = threadIdx.x;
  if (s >= n_streams) return;
  float bm = -1.0f;
  int bk = 0x7fffffff, bt = -1;
  for (int t = lane; t < n_tiles; t += 64) {
    const float m = tile_m[(size_t)s * n_tiles + t];
    const int k = tile_k[(size_t)s * n_tiles + t];
    if (k >= 0 && ((m > bm) || (m == bm && k < bk))) { bm = m; bk = k; bt = t; }
  }
#pragma unroll
  for (int w = 1; w < 64; w <<= 1) {
    const float om = __shfl_xor(bm, w, 64);
    const int ok = __shfl_xor(bk, w, 64), ot = __shfl_xor(bt, w, 64);
    const bool take = (om > bm) || (om == bm && ok < bk);
    if (take) { bm = om; bk = ok; bt = ot; }
  }
  if (lane != 0) return;
  cx C = mk(0, 0);
  float E = 0.0f, m = 0.0f, arg = 0.0f;
  int k = -1;
  if (bt >= 0) {
    k = bk; m = bm;
    C = tile_c[(size_t)s * n_tiles + bt];
    E = tile_e[(size_t)s * n_tiles + bt];
    if (acq_finite(C.r) && acq_finite(C.i)) arg = acq_atan2(C.i, C.r);   // the angle of a poisoned window is 0
  }
  const float omega = -arg / (float)sps;
  const int n = 172 * sps;
  const int w0 = k >= 0 ? k - 3 * sps + 1250 * sps - 12 * sps : 0;
  uint8_t st = (k >= 0 && m > fcch_thresh) ? TRXSIG_ACQ_FCCH : 0;
  if (st && w0 >= 0 && w0 <= N - n) st |= TRXSIG_ACQ_WINDOW;
  o.state[s] = st;
  o.fcch_k[s] = k; o.fcch_m[s] = m; o.fcch_c[s] = C; o.fcch_e[s] = E;
  o.arg[s] = arg; o.omega[s] = omega; o.w0[s] = w0;
  o.base[s] = (long long)s * stride + w0;
  o.wlen[s] = (st & TRXSIG_ACQ_WINDOW) ? n : 0;
}

__global__ __launch_bounds__(64) void k_l1acq_shift(int sps, const TrxTables *__restrict__ T, const cx *__restrict__ in,
                                                    const long long *__restrict__ base64, const int32_t *__restrict__ off32,
                                                    const int32_t *__restrict__ len, const float *__restrict__ omega,
                                                    cx *__restrict__ out, int32_t *__restrict__ woff, int32_t *__restrict__ wlen) {
  const int b = blockIdx.x, lane = threadIdx.x;
  const long long off = base64 ? base64[b] : (long long)off32[b];
  const int n = len[b];
  const bool valid = off >= 0 && n > 0 && n <= TRXSIG_L1ACQ_MAX_WINDOW * sps;
  if (lane == 0) { woff[b] = b * TRX_ACQ_WMAX; wlen[b] = valid ? n : 0; }
  if (!valid) return;
  const cx *x = in + off;
  cx *y = out + (size_t)b * TRX_ACQ_WMAX;
  if (!omega) {
    for (int i = lane; i < n; i += 64) y[i] = x[i];
    return;
  }
  const float f = omega[b];
  float phase = 0.0f;                                      // startPhase 0
  for (int base = 0; base < n; base += 64) {               // k_frequency_shift's loop: every lane runs the chain of additions
    float mine = phase;
    const int cnt = n - base < 64 ? n - base : 64;
    for (int q = 0; q < cnt; q++) {
      mine = q == lane ? phase : mine;
      phase += f;                                          // :460
    }
    const int i = base + lane;
    if (i < n) y[i] = cmul(x[i], dev_expj_lookup(T, mine));   // :459 (*xP)*expjLookup(phase)
  }
}

__global__ __launch_bounds__(64) void k_l1acq_verdict(int sps, const cx *__restrict__ corr, const int32_t *__restrict__ wlen,
                                                      const cx *__restrict__ peak, const float *__restrict__ pidx, int B, cx gain,
                                                      float seq_toa, float thresh, int search, uint8_t *__restrict__ flags,
                                                      cx *__restrict__ amp_out, float *__restrict__ toa_out,
                                                      float *__restrict__ ptm_out, int32_t *__restrict__ doff,
                                                      int32_t *__restrict__ dlen, float *__restrict__ dtoa,
                                                      uint8_t *__restrict__ state) {
  const int b = blockIdx.x * 64 + threadIdx.x;
  if (b >= B) return;
  const int n = wlen[b];
  uint8_t fl = 0;
  cx amp = mk(0, 0);
  float toa_b = 0.0f, ptm = 0.0f, rest = 0.0f;
  int i0 = 0, nd = 0;
  if (n <= 0) {
    fl = search ? 0 : TRXSIG_F_BADLEN;
  } else {
    const cx *c = corr + (size_t)b * TRX_ACQ_WMAX;
    const cx pk = peak[b];
    const float toa = pidx[b];
    bool bogus = !(toa >= 0.0f && toa <= (float)n);        // :964 (a NaN index is bogus too)
    if (!bogus) {
      const int p = (int)rintf(toa);
      float valley = 0.0f;
      int numRms = 0;
      for (int i = 2 * sps; i <= 5 * sps; i++) {           // :971-980, this order
        if (p - i >= 0) { valley += norm2(c[p - i]); numRms++; }
        if (p + i < n) { valley += norm2(c[p + i]); numRms++; }
      }
      if (numRms < 2) {
        bogus = true;                                      // :982
      } else {
        const float RMS = (float)((double)sqrtf(valley / (float)numRms) + 0.00001);   // :989
        ptm = sqrtf(norm2(pk)) / RMS;                      // Complex::abs() via double sqrt == sqrtf
        amp = cdiv(pk, gain);                              // :997
      }
    }
    toa_b = toa - seq_toa;                                 // :998
    toa_b = toa_b - (float)(42 * sps);                     // the sequence starts at bit 42
    if (!bogus && ptm > thresh) {
      const float fl0 = floorf(toa_b);
      if (fl0 >= 0.0f && fl0 <= (float)(n - 148 * sps)) {
        i0 = (int)fl0;
        const int sh = sps >> 1;                           // log2(sps) for 1, 2, 4
        nd = ((n - i0) >> sh) << sh;                       // whole symbols
        if (nd > 156 * sps) nd = 156 * sps;
        rest = toa_b - fl0;
        fl = TRXSIG_F_DETECT;
      }
    }
  }
  flags[b] = fl;
  amp_out[b] = amp;
  toa_out[b] = toa_b;
  if (ptm_out) ptm_out[b] = ptm;
  doff[b] = b * TRX_ACQ_WMAX + i0;
  dlen[b] = nd;
  dtoa[b] = rest;
  if (state && (fl & TRXSIG_F_DETECT)) state[b] |= TRXSIG_ACQ_SCH;
}

// TRXSIG_SCHDET_FIT: the geometry gate in the valley rule's place (a thread per window); the verdict waits for k_sch_fit
__global__ __launch_bounds__(64) void k_l1acq_candidates(int sps, const int32_t *__restrict__ wlen, const cx *__restrict__ peak,
                                                         const float *__restrict__ pidx, int B, cx gain, float seq_toa, int search,
                                                         uint8_t *__restrict__ flags, cx *__restrict__ amp_out,
                                                         float *__restrict__ toa_out, int32_t *__restrict__ doff,
                                                         int32_t *__restrict__ dlen, float *__restrict__ dtoa) {
  const int b = blockIdx.x * 64 + threadIdx.x;
  if (b >= B) return;
  const int n = wlen[b];
  uint8_t fl = 0;
  cx amp = mk(0, 0);
  float toa_b = 0.0f, rest = 0.0f;
  int i0 = 0, nd = 0;
  if (n <= 0) {
    fl = search ? 0 : TRXSIG_F_BADLEN;
  } else {
    const float toa = pidx[b];
    const bool inside = toa >= 0.0f && toa <= (float)n;    // :964 (a NaN index is outside too)
    if (inside) amp = cdiv(peak[b], gain);                 // :997
    toa_b = toa - seq_toa;                                 // :998
    toa_b = toa_b - (float)(42 * sps);                     // the sequence starts at bit 42
    if (inside && acq_finite(amp.r) && acq_finite(amp.i) && (amp.r != 0.0f || amp.i != 0.0f)) {
      const float fl0 = floorf(toa_b);
      if (fl0 >= 0.0f && fl0 <= (float)(n - 148 * sps)) {
        i0 = (int)fl0;
        const int sh = sps >> 1;                           // log2(sps) for 1, 2, 4
        nd = ((n - i0) >> sh) << sh;                       // whole symbols
        if (nd > 156 * sps) nd = 156 * sps;
        rest = toa_b - fl0;
        fl = TRXSIG_F_DETECT;                              // a candidate; k_l1acq_fit_verdict decides
      }
    }
  }
  flags[b] = fl;
  amp_out[b] = amp;
  toa_out[b] = toa_b;
  doff[b] = b * TRX_ACQ_WMAX + i0;
  dlen[b] = nd;
  dtoa[b] = rest;
}

__global__ __launch_bounds__(64) void k_l1acq_fit_verdict(int B, const float *__restrict__ q, float thresh, uint8_t *__restrict__ flags,
                                                          float *__restrict__ ptm_out, uint8_t *__restrict__ state) {
  const int b = blockIdx.x * 64 + threadIdx.x;
  if (b >= B) return;
  uint8_t fl = flags[b];
  const float qb = (fl & TRXSIG_F_DETECT) ? q[b] : 0.0f;   // (k_sch_fit wrote 0 for the others already)
  if ((fl & TRXSIG_F_DETECT) && !(qb > thresh)) fl = 0;
  flags[b] = fl;
  if (ptm_out) ptm_out[b] = qb;
  if (state && (fl & TRXSIG_F_DETECT)) state[b] |= TRXSIG_ACQ_SCH;
}

__global__ __launch_bounds__(256) void k_l1acq_finish(int n, const uint8_t *__restrict__ ok, uint8_t *__restrict__ state) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n && ok[i] && (state[i] & TRXSIG_ACQ_SCH)) state[i] |= TRXSIG_ACQ_DECODED;
}

}  // namespace

int trx_acq_tiles(int sps, int n_samples) {
  const int L = TRX_ACQ_FCCH_SYMS * sps, W = TRX_ACQ_TILE_SYMS;
  const long long starts = (long long)n_samples - sps - L + 1;      // window starts 0 .. n_samples - sps - L
  return starts <= 0 ? 0 : (int)((starts + W - 1) / W);
}

hipError_t trx_launch_l1acq_fcch(hipStream_t st, int sps, const trx_c32 *samples, long long stride, int n_samples, int n_streams,
                                 int n_tiles, float *tile_m, int32_t *tile_k, trx_c32 *tile_c, float *tile_e) {
  if (n_streams <= 0 || n_tiles <= 0) return hipSuccess;
  if (n_streams > 65535) return hipErrorInvalidValue;
  const dim3 grid(n_tiles, n_streams), block(kAcqThreads);
  switch (sps) {
    case 1: k_l1acq_fcch<1><<<grid, block, 0, st>>>(samples, stride, n_samples, n_tiles, tile_m, tile_k, tile_c, tile_e); break;
    case 2: k_l1acq_fcch<2><<<grid, block, 0, st>>>(samples, stride, n_samples, n_tiles, tile_m, tile_k, tile_c, tile_e); break;
    case 4: k_l1acq_fcch<4><<<grid, block, 0, st>>>(samples, stride, n_samples, n_tiles, tile_m, tile_k, tile_c, tile_e); break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

hipError_t trx_launch_l1acq_pick(hipStream_t st, int sps, long long stride, int n_samples, int n_streams, int n_tiles,
                                 const float *tile_m, const int32_t *tile_k, const trx_c32 *tile_c, const float *tile_e,
                                 float fcch_thresh, TrxAcqStreams s) {
  if (n_streams <= 0) return hipSuccess;
  k_l1acq_pick<<<dim3(n_streams), dim3(64), 0, st>>>(sps, stride, n_samples, n_streams, n_tiles, tile_m, tile_k, tile_c, tile_e,
                                                    fcch_thresh, s);
  return hipGetLastError();
}

hipError_t trx_launch_l1acq_shift(hipStream_t st, int sps, const TrxTables *dT, const trx_c32 *samples, const long long *base64,
                                  const int32_t *off32, const int32_t *len, const float *omega, int B, trx_c32 *y, int32_t *woff,
                                  int32_t *wlen) {
  if (B <= 0) return hipSuccess;
  k_l1acq_shift<<<dim3(B), dim3(64), 0, st>>>(sps, dT, samples, base64, off32, len, omega, y, woff, wlen);
  return hipGetLastError();
}

hipError_t trx_launch_l1acq_verdict(hipStream_t st, int sps, const trx_c32 *c, const int32_t *wlen, const trx_c32 *peak,
                                    const float *pidx, int B, trx_c32 gain, float seq_toa, float thresh, int search, uint8_t *flags,
                                    trx_c32 *amp, float *toa, float *ptm, int32_t *doff, int32_t *dlen, float *dtoa, uint8_t *state) {
  if (B <= 0) return hipSuccess;
  k_l1acq_verdict<<<dim3((B + 63) / 64), dim3(64), 0, st>>>(sps, c, wlen, peak, pidx, B, gain, seq_toa, thresh, search, flags, amp,
                                                           toa, ptm, doff, dlen, dtoa, state);
  return hipGetLastError();
}

hipError_t trx_launch_l1acq_candidates(hipStream_t st, int sps, const int32_t *wlen, const trx_c32 *peak, const float *pidx, int B,
                                       trx_c32 gain, float seq_toa, int search, uint8_t *flags, trx_c32 *amp, float *toa, int32_t *doff,
                                       int32_t *dlen, float *dtoa) {
  if (B <= 0) return hipSuccess;
  k_l1acq_candidates<<<dim3((B + 63) / 64), dim3(64), 0, st>>>(sps, wlen, peak, pidx, B, gain, seq_toa, search, flags, amp, toa, doff,
                                                              dlen, dtoa);
  return hipGetLastError();
}

hipError_t trx_launch_l1acq_fit_verdict(hipStream_t st, int B, const float *q, float thresh, uint8_t *flags, float *ptm, uint8_t *state) {
  if (B <= 0) return hipSuccess;
  k_l1acq_fit_verdict<<<dim3((B + 63) / 64), dim3(64), 0, st>>>(B, q, thresh, flags, ptm, state);
  return hipGetLastError();
}

hipError_t trx_launch_l1acq_finish(hipStream_t st, int n_streams, const uint8_t *ok, uint8_t *state) {
  if (n_streams <= 0) return hipSuccess;
  k_l1acq_finish<<<dim3((n_streams + 255) / 256), dim3(256), 0, st>>>(n_streams, ok, state);
  return hipGetLastError();
}
