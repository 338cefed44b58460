// trxsig_air.hip -- the air (include/trxsig_air.h): multipath, oscillator offset and white Gaussian noise on the device.
// k_air_cells: slot cells -> slot cells (the uplink: what trxsig_l1ms_radiate wrote -> what trxsig_trxgroup_pull reads).
// k_air_stream: a carrier's cells -> one delayed, rotated, scaled, noisy stream per handset (what trxsig_l1acq_search reads).
// k_air_fade: the taps k_air_cells reads, from a sum-of-sinusoids fading process per (link, path) (k_air_fade_params: its integers).
// The signal path is the reference's arithmetic (convolve START_ONLY, expjLookup, delayVector, scaleVector) under the library's
// numerical contract; the noise is counter-based (Philox4x32-10 -> Box-Muller) with ln / cos / sin in the kernel's own float32
// arithmetic: the device library's logf / sincosf hold fused multiply-adds, which no kernel of this library may contain.
#include "trxsig_dev.h"

namespace {

constexpr unsigned kAirRows = 8u * 2715648u;                 // slots per hyperframe: the cell form's noise row wraps there
constexpr int kAirPad = 31;                                  // zeros before the cell in LDS: the longest channel less one

// Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11), Random123's constants
__device__ __forceinline__ void philox4x32_10(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1,
                                              unsigned (&w)[4]) {
#pragma unroll
  for (int r = 0; r < 10; r++) {
    const unsigned hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
    const unsigned hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
    c0 = hi1 ^ c1 ^ k0; c1 = lo1; c2 = hi0 ^ c3 ^ k1; c3 = lo0;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  w[0] = c0; w[1] = c1; w[2] = c2; w[3] = c3;
}

// (cos, sin) of a 24-bit phase k, in 2^-24 turn: the phase is reduced to an octant in integers (exact), the angle theta in
// [0, pi/4] is one rounded product, Taylor polynomials to theta^9 / theta^10 leave 2e-9.  Every step is a separately rounded
// float32 operation; each component is well inside the 1e-5 trxsig_air.h promises.  A phase on an axis has theta = 0: exactly (+-1, +-0) or
// (+-0, +-1).  Shared by the noise (odd phases) and the fading generator (every phase).
__device__ __forceinline__ void air_cossin(unsigned k, float &c, float &sgn) {
  const unsigned quad = k >> 22;
  unsigned f = k & 0x3fffffu;                                                // inside the quarter turn, in 2^-22 of it
  const bool mirror = f > 0x200000u;
  if (mirror) f = 0x400000u - f;
  const float th = (float)f * 3.74507028e-7f;                                // (pi / 2) 2^-22
  const float t2 = th * th;
  float ps = t2 * 2.75573192e-6f + -1.98412698e-4f;
  ps = ps * t2 + 8.33333333e-3f;
  ps = ps * t2 + -0.166666667f;
  ps = ps * t2;
  float sn = th + th * ps;
  float pc = t2 * -2.75573192e-7f + 2.48015873e-5f;
  pc = pc * t2 + -1.38888889e-3f;
  pc = pc * t2 + 4.16666667e-2f;
  pc = pc * t2 + -0.5f;
  float cs = 1.0f + pc * t2;
  if (mirror) { const float t = sn; sn = cs; cs = t; }
  switch (quad) {
    case 0: c = cs; sgn = sn; break;
    case 1: c = -sn; sgn = cs; break;
    case 2: c = -cs; sgn = -sn; break;
    default: c = sn; sgn = -cs; break;
  }
}

// Box-Muller on a pair of words: u = (2 (wa >> 9) + 1) 2^-24, v likewise; g = sqrt(-2 ln u) (cos 2 pi v, sin 2 pi v).
// ln u: u = m 2^e with m in [sqrt(1/2), sqrt 2) by integer operations (u near 1 has e = 0: nothing cancels), ln m = 2 atanh(s),
// s = (m - 1) / (m + 1), |s| < 0.1716: the series to s^9 leaves 2e-9 relative; e ln 2 with ln 2 split so that e * hi is exact.
// cos, sin: air_cossin of the odd 24-bit phase.  Every step is a separately rounded float32 operation; the sum of the
// rounding errors keeps each component of g within 3e-6 of the formulas' exact value (trxsig_air.h promises 1e-5).
__device__ __forceinline__ cx air_gauss(unsigned wa, unsigned wb) {
  const float u = (float)(2u * (wa >> 9) + 1u) * 5.9604644775390625e-8f;      // exact: 24 bits times 2^-24
  const int bits = __float_as_int(u);
  int e = (bits >> 23) - 127;
  float m = __int_as_float((bits & 0x007fffff) | 0x3f800000);                 // [1, 2)
  if (m > 1.41421354f) { m = m * 0.5f; e += 1; }
  const float s = (m - 1.0f) / (m + 1.0f);
  const float s2 = s * s;
  float q = s2 * 0.111111111f + 0.142857143f;
  q = q * s2 + 0.2f;
  q = q * s2 + 0.333333333f;
  q = q * s2;
  const float lnm = (s + s * q) * 2.0f;
  const float fe = (float)e;
  const float lnu = fe * 0.693145751953125f + (lnm + fe * 1.42860682030941723212e-6f);
  const float r = sqrtf(-2.0f * lnu);
  float c, sgn;
  air_cossin(2u * (wb >> 9) + 1u, c, sgn);                                    // the phase in 2^-24 turn, odd
  return mk(r * c, r * sgn);
}

// expjLookup of an NCO phase (2^-32 turn): the top 24 bits as a float, exact; one rounded product with (float)(2 pi)
__device__ __forceinline__ cx air_rot(const TrxTables *__restrict__ T, unsigned ph) {
  return dev_expj_lookup(T, (float)(ph >> 8) * 5.9604644775390625e-8f * TRX_2PI_F);
}
// (the complex products are trxsig_dev.h's cmul_sum: a NaN sample leaves with the reference's words)
__device__ __forceinline__ cx air_add_noise(cx v, float sigma, cx g) { return mk(v.r + sigma * g.r, v.i + sigma * g.i); }

// ---------------------------------------------------------------------------------------------
// k_air_cells: workgroup (x, y) takes ARFCN y's slots x, x + gridDim.x, ... (k_l1ms_radiate's grid).  The cell goes to LDS once,
// behind kAirPad zeros: the tap loop then runs over all its taps without the reference's break (i - j < 0).  The terms that
// adds are x * 0 = +-0 and come last; a sum that started at +0 is never -0, so adding +-0 to it changes nothing (the argument
// k_l1ms_radiate makes for its own zero padding).  A lane forms samples 2 p and 2 p + 1: they share one Philox block and all
// but one of their LDS reads.
// ---------------------------------------------------------------------------------------------
template <int SPS>
__global__ __launch_bounds__(256) void k_air_cells(const TrxTables *__restrict__ T, TrxAirCells p) {
  __shared__ cx row[kAirPad + 157 * SPS + 1];
  __shared__ cx hs[32];
  __shared__ float hni[32];                                  // -h.i (cmul_sum)
  const int a = blockIdx.y;
  if (threadIdx.x < kAirPad) row[threadIdx.x] = mk(0, 0);
  if (threadIdx.x == 0) row[kAirPad + 157 * SPS] = mk(0, 0);
  for (long long t = blockIdx.x; t < p.rows; t += gridDim.x) {
    const int N = SPS * (156 + ((t & 3) == 0));
    const size_t cell = (size_t)a * p.rows + t;
    const cx *x = p.in + t * p.in_slot + a * p.in_arfcn;
    cx *o = p.out + t * p.out_slot + a * p.out_arfcn;
    __syncthreads();                                         // the previous cell's readers of row / hs are done
    for (int i = threadIdx.x; i < N; i += 256) row[kAirPad + i] = x[i];
    if (p.taps && (int)threadIdx.x < p.n_taps) {
      const cx h = p.taps[cell * p.n_taps + threadIdx.x];
      hs[threadIdx.x] = h;
      hni[threadIdx.x] = -h.i;
    }
    __syncthreads();
    const unsigned step = p.step ? p.step[cell] : 0u;
    const unsigned phase = (p.step && p.phase) ? p.phase[cell] : 0u;
    const float sigma = p.sigma ? p.sigma[cell] : 0.0f;
    const unsigned nrow = (p.row0 + (unsigned)t) % kAirRows;
    for (int i = 2 * threadIdx.x; i < N; i += 512) {
      cx u0, u1;
      if (p.taps) {                                          // convolve(x, h, START_ONLY): j ascending, (*aP) * (*bP)
        u0 = mk(0, 0); u1 = mk(0, 0);
        cx xa = row[kAirPad + i + 1];
        for (int j = 0; j < p.n_taps; j++) {
          const cx xb = row[kAirPad + i - j];
          const cx h = hs[j];
          const float nh = hni[j];
          u1 = cadd(u1, cmul_sum(xa, h, nh));
          u0 = cadd(u0, cmul_sum(xb, h, nh));
          xa = xb;
        }
      } else {
        u0 = row[kAirPad + i]; u1 = row[kAirPad + i + 1];
      }
      if (p.step) {                                          // frequencyShift: (*xP) * expjLookup(phase)
        const unsigned ph = phase + (unsigned)i * step;
        u0 = cmul_sum(u0, air_rot(T, ph));
        u1 = cmul_sum(u1, air_rot(T, ph + step));
      }
      if (p.sigma) {
        unsigned w[4];
        philox4x32_10((unsigned)i >> 1, nrow, (unsigned)a, 0u, p.key0, p.key1, w);
        u0 = air_add_noise(u0, sigma, air_gauss(w[0], w[1]));
        u1 = air_add_noise(u1, sigma, air_gauss(w[2], w[3]));
      }
      if (p.accumulate) {
        u0 = cadd(o[i], u0);
        if (i + 1 < N) u1 = cadd(o[i + 1], u1);
      }
      o[i] = u0;
      if (i + 1 < N) o[i + 1] = u1;
    }
  }
}

// ---------------------------------------------------------------------------------------------
// k_air_stream: workgroup (x, y) forms outputs [x TILE, (x + 1) TILE) of handset y.  The carrier's samples the tile needs --
// its own and the ten on either side delayVector's 21 taps reach, shifted by the delay's integer part -- are gathered from
// the cells into LDS, zeros outside the stream: the tap sum then runs without the reference's break / skip (the zero terms
// come first or last in it and are +-0, as above).  Stream position -> (cell, offset) by constant divisions only.
// ---------------------------------------------------------------------------------------------
template <int SPS>
__global__ __launch_bounds__(256) void k_air_stream(const TrxTables *__restrict__ T, TrxAirStream p) {
  __shared__ cx xs[TRX_AIR_TILE + 20];
  __shared__ float tap[21];
  const int h = blockIdx.y;
  const int n_base = blockIdx.x * TRX_AIR_TILE;
  const int a = p.arfcn[h];
  const long long cut = p.cut[h];
  const float d = p.delay ? p.delay[h] : 0.0f;
  const bool refused = !(fabsf(d) <= TRXSIG_MAX_INDEX);      // k_delay_vector: zeros
  const int io = refused ? 0 : (int)floorf(d);               // sigProcLib.cpp:577
  const float frac = d - (float)io;                          // :578
  const bool filt = fabs((double)frac) > 1e-2;               // :582
  const int rem = p.n_cells & 3;
  const long long Ls = (long long)(p.n_cells >> 2) * (625 * SPS) + (rem ? (157 + 156 * (rem - 1)) * SPS : 0);
  const bool carrier = a >= 0 && a < p.n_arfcn && !refused;
  // xs[m] = c[q0 + m]
  const long long q0 = (long long)((unsigned long long)cut + (unsigned long long)(long long)(n_base - 10 - io));
  for (int m = threadIdx.x; m < TRX_AIR_TILE + 20; m += 256) {
    const long long q = q0 + m;
    cx v = mk(0, 0);
    if (carrier && q >= 0 && q < Ls) {
      const unsigned uq = (unsigned)q;                       // Ls < 2^31 (the host checks)
      const unsigned blk = uq / (625u * SPS);
      unsigned r = uq - blk * (625u * SPS), s = 0;
      if (r >= 157u * SPS) {
        r -= 157u * SPS;
        s = r / (156u * SPS);
        r -= s * (156u * SPS);
        s += 1;
      }
      v = p.in[(long long)(4u * blk + s) * p.in_slot + (long long)a * p.in_arfcn + r];
    }
    xs[m] = v;
  }
  if (threadIdx.x < 21) tap[threadIdx.x] = dev_sinc(T->sinT, TRX_PI_F * ((float)((int)threadIdx.x - 10) - frac));   // :588
  __syncthreads();
  float tp[21];
#pragma unroll
  for (int j = 0; j < 21; j++) tp[j] = tap[j];
  const unsigned step = p.step ? p.step[h] : 0u;
  const unsigned phase = (p.step && p.phase) ? p.phase[h] : 0u;
  const cx gain = p.gain ? p.gain[h] : mk(1, 0);
  const float ngi = neg_opaque(gain.i);
  const float sigma = p.sigma ? p.sigma[h] : 0.0f;
  const unsigned n0 = p.n0 ? p.n0[h] : 0u;
  for (int l = threadIdx.x; l < TRX_AIR_TILE; l += 256) {
    const int n = n_base + l;
    if (n >= p.len) break;
    const long long k = (long long)((unsigned long long)cut + (unsigned long long)n);   // position in z
    const long long tt = k - io;                             // ... in c
    cx r = mk(0, 0);
    if (carrier && k >= 0 && k < Ls && tt >= 0 && tt < Ls) {
      if (filt) {
#pragma unroll
        for (int j = 0; j < 21; j++) r = cadd(r, cmulr(xs[l + 20 - j], tp[j]));   // convolve(.., NO_DELAY): start 10, j ascending
      } else {
        r = xs[l + 10];
      }
    }
    if (p.step) r = cmul_sum(r, air_rot(T, phase + (unsigned)n * step));
    if (p.gain) r = cmul_sum(r, gain, ngi);                           // scaleVector (:719)
    if (p.sigma) {
      const unsigned i = n0 + (unsigned)n;
      unsigned w[4];
      philox4x32_10(i >> 1, (unsigned)h, 0u, 1u, p.key0, p.key1, w);
      r = air_add_noise(r, sigma, (i & 1u) ? air_gauss(w[2], w[3]) : air_gauss(w[0], w[1]));
    }
    p.out[(long long)h * p.out_stride + n] = r;
  }
}

// ---------------------------------------------------------------------------------------------
// The fading-tap generator (trxsig_air.h, "Time-varying multipath").  One (link, path, sinusoid) is one Philox block:
// phase w0, Doppler cosine from w1 (the line-of-sight sinusoid s = S takes the profile's).  Integers only from there to the
// phase theta of a slot, so the values are functions of (seed, link, path, row, column) alone.
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ void fade_pair(unsigned key0, unsigned key1, unsigned link, int path, int s, int S, unsigned D, int los_c,
                                          unsigned &phi, int &step) {
  unsigned w[4];
  philox4x32_10((unsigned)s, (unsigned)path, link, 2u, key0, key1, w);
  phi = w[0];
  int C = los_c;
  if (s != S) {
    float c, sn;
    air_cossin(2u * (w[1] >> 9) + 1u, c, sn);
    C = (int)rintf(c * 8388608.0f);                          // Q23; the product is exact
  }
  step = (int)(((long long)C * (long long)D) >> 23);
}

__device__ __forceinline__ cx fade_e(unsigned theta) {
  float c, s;
  air_cossin(theta >> 8, c, s);
  return mk(c, s);
}

// k_air_fade_params: thread i = (link, path, s) in that nesting writes phi and step (what the tests grade word for word)
__global__ __launch_bounds__(256) void k_air_fade_params(TrxAirFade p) {
  const int n_pairs = p.P * (p.S + 1);
  const int i = blockIdx.x * 256 + threadIdx.x;              // the pair inside the link (blockIdx.y)
  if (i >= n_pairs) return;
  const unsigned link = blockIdx.y + 65535u * blockIdx.z;
  if (link >= (unsigned)p.n_links) return;
  const int path = (int)(((unsigned)i * p.inv) >> 16), s = i - path * (p.S + 1);
  unsigned phi; int step;
  fade_pair(p.key0, p.key1, link, path, s, p.S, p.doppler[link] & 0x7fffffffu, p.tab->los_c[path], phi, step);
  const size_t o = (size_t)link * n_pairs + i;
  p.phase[o] = phi; p.step[o] = step;
}

// k_air_fade: workgroup (x, y) takes column y's slots 4 x + wave, 4 (x + gridDim.x) + wave, ...: a wave per cell.  The weights,
// amplitudes and the column's rotations go to LDS once.  Per cell: lane i, i + 64, ... of the wave forms e(theta) of pair i
// into LDS; lane p < P sums its path's S diffuse terms in the order s = 0, 1, ..., S - 1 (a chain of S - 1 rounded sums from
// e(theta_0): the same in every geometry), forms g_p = a_p sum + b_p e(theta_S) and rotates it by the column's e; lane l forms
// taps 2 l and 2 l + 1, p ascending.  The barriers are the workgroup's: every wave takes every trip, with or without a cell.
__global__ __launch_bounds__(256) void k_air_fade(TrxAirFade p) {
  __shared__ float ws[TRX_FADE_MAX_PATHS * 32];
  __shared__ float as[TRX_FADE_MAX_PATHS], bs[TRX_FADE_MAX_PATHS];
  __shared__ int lc[TRX_FADE_MAX_PATHS];
  __shared__ cx rs[TRX_FADE_MAX_PATHS];
  __shared__ cx es[4][TRX_FADE_MAX_PATHS * (TRX_FADE_MAX_SIN + 1)];
  __shared__ cx gs[4][TRX_FADE_MAX_PATHS];
  const int a = blockIdx.y, wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int P = p.P, S = p.S, n_pairs = P * (S + 1);
  for (int i = threadIdx.x; i < TRX_FADE_MAX_PATHS * 32; i += 256) ws[i] = p.tab->w[i >> 5][i & 31];
  if ((int)threadIdx.x < P) {
    as[threadIdx.x] = p.tab->a[threadIdx.x]; bs[threadIdx.x] = p.tab->b[threadIdx.x]; lc[threadIdx.x] = p.tab->los_c[threadIdx.x];
    rs[threadIdx.x] = fade_e(p.tab->rot[a][threadIdx.x]);
  }
  __syncthreads();
  for (long long t0 = 4LL * blockIdx.x; t0 < p.rows; t0 += 4LL * gridDim.x) {
    const long long t = t0 + wv;
    const bool cell = t < p.rows;
    int link = -1;
    if (cell) link = p.link ? p.link[(size_t)a * p.rows + t] : 8 * a + (int)(t & 7);
    const bool live = link >= 0 && link < p.n_links;
    if (live) {
      const unsigned D = p.doppler[link] & 0x7fffffffu;
      const unsigned nrow = (p.row0 + (unsigned)t) % kAirRows;
      for (int i = lane; i < n_pairs; i += 64) {
        const int path = (int)(((unsigned)i * p.inv) >> 16), s = i - path * (S + 1);
        unsigned phi; int step;
        fade_pair(p.key0, p.key1, (unsigned)link, path, s, S, D, lc[path], phi, step);
        es[wv][i] = fade_e(phi + nrow * (unsigned)step);
      }
    }
    __syncthreads();
    if (live && lane < P) {
      const cx *e = &es[wv][lane * (S + 1)];
      cx sum = e[0];
      for (int s = 1; s < S; s++) sum = cadd(sum, e[s]);
      const float av = as[lane], bv = bs[lane];
      const cx g = mk(av * sum.r + bv * e[S].r, av * sum.i + bv * e[S].i);
      const cx r = rs[lane];
      gs[wv][lane] = mk(g.r * r.r - g.i * r.i, g.r * r.i + g.i * r.r);
    }
    __syncthreads();
    if (cell && 2 * lane < p.n_taps) {
      const int j = 2 * lane;
      cx h0 = mk(0, 0), h1 = mk(0, 0);
      if (live) {
        cx g = gs[wv][0];
        h0 = mk(g.r * ws[j], g.i * ws[j]); h1 = mk(g.r * ws[j + 1], g.i * ws[j + 1]);   // (j + 1 <= 31; a weight beyond n_taps is zero and its tap is not stored)
        for (int q = 1; q < P; q++) {
          g = gs[wv][q];
          const float w0 = ws[32 * q + j], w1 = ws[32 * q + j + 1];
          h0 = mk(h0.r + g.r * w0, h0.i + g.i * w0);
          h1 = mk(h1.r + g.r * w1, h1.i + g.i * w1);
        }
      }
      cx *o = p.taps + ((size_t)a * p.rows + t) * p.n_taps + j;
      if (p.vec) {
        *reinterpret_cast<float4 *>(o) = make_float4(h0.r, h0.i, h1.r, h1.i);
      } else {
        o[0] = h0;
        if (j + 1 < p.n_taps) o[1] = h1;
      }
    }
  }
}

constexpr long long kAirCellsWg = 16384;                     // as k_l1ms_radiate: the slots beyond go round the loop

}  // namespace

hipError_t trx_launch_air_cells(hipStream_t st, int sps, const TrxTables *dT, const TrxAirCells &p) {
  if (p.rows <= 0 || p.n_arfcn <= 0 || p.n_arfcn > 65535) return hipErrorInvalidValue;
  long long gx = kAirCellsWg / p.n_arfcn > 0 ? kAirCellsWg / p.n_arfcn : 1;
  if (gx > p.rows) gx = p.rows;
  const dim3 grid((unsigned)gx, (unsigned)p.n_arfcn), block(256);
  switch (sps) {
    case 1: k_air_cells<1><<<grid, block, 0, st>>>(dT, p); break;
    case 2: k_air_cells<2><<<grid, block, 0, st>>>(dT, p); break;
    case 4: k_air_cells<4><<<grid, block, 0, st>>>(dT, p); break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

hipError_t trx_launch_air_stream(hipStream_t st, int sps, const TrxTables *dT, const TrxAirStream &p) {
  if (p.len <= 0 || p.n_handsets <= 0 || p.n_handsets > 65535) return hipErrorInvalidValue;
  const dim3 grid((unsigned)((p.len + TRX_AIR_TILE - 1) / TRX_AIR_TILE), (unsigned)p.n_handsets), block(256);
  switch (sps) {
    case 1: k_air_stream<1><<<grid, block, 0, st>>>(dT, p); break;
    case 2: k_air_stream<2><<<grid, block, 0, st>>>(dT, p); break;
    case 4: k_air_stream<4><<<grid, block, 0, st>>>(dT, p); break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

hipError_t trx_launch_air_fade(hipStream_t st, const TrxAirFade &p) {
  if (p.rows <= 0 || p.n_arfcn <= 0 || p.n_arfcn > TRX_FADE_MAX_COLS || p.P < 1 || p.P > TRX_FADE_MAX_PATHS || p.S < 1 ||
      p.S > TRX_FADE_MAX_SIN || p.n_taps < 1 || p.n_taps > 32)
    return hipErrorInvalidValue;
  const long long quads = (p.rows + 3) / 4;
  long long gx = kAirCellsWg / p.n_arfcn > 0 ? kAirCellsWg / p.n_arfcn : 1;
  if (gx > quads) gx = quads;
  k_air_fade<<<dim3((unsigned)gx, (unsigned)p.n_arfcn), dim3(256), 0, st>>>(p);
  return hipGetLastError();
}

hipError_t trx_launch_air_fade_params(hipStream_t st, const TrxAirFade &p) {
  if (p.n_links <= 0 || p.P < 1 || p.P > TRX_FADE_MAX_PATHS || p.S < 1 || p.S > TRX_FADE_MAX_SIN) return hipErrorInvalidValue;
  const unsigned gy = p.n_links < 65535 ? (unsigned)p.n_links : 65535u, gz = (unsigned)((p.n_links + 65534) / 65535);
  k_air_fade_params<<<dim3((unsigned)((p.P * (p.S + 1) + 255) / 256), gy, gz), dim3(256), 0, st>>>(p);
  return hipGetLastError();
}
