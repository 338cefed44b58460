// trxsig_txwb.hip -- the wideband transmit synthesiser (include/trxsig_frontend.h, trxsig_txbe_create_wideband): C ARFCN streams
// modulated from their queued bits, each resampled P = 96 R : Q = 65 sps, moved to its carrier by the channeliser's mixer and summed
// in carrier order into one int16 stream at R x 400 kS/s.  One launch per pop, from bits to int16.
// Numerical contract: see the header; every float32 operation is separately rounded (built with -ffp-contract=off).
#include "trxsig_dev.h"
#include "trxsig_txstage.h"

namespace {

constexpr int kNJ = TRX_TXWB_OB / 256;                      // outputs per lane

// ---------------------------------------------------------------------------------------------
// k_tx_wideband<SPS>: a workgroup per (tile of TRX_TXWB_OB outputs, wideband stream w).  Lane t owns outputs o0 + t + 256 j.
//   The taps are staged once, branch-major (TP[row][k] = lpf[row g + P k], zero past L): an output reads its own row.  Then for
//   every carrier c in order, the tile's span of ARFCN stream w*C + c's window is staged from its bit ring (tx_stage_tile, the
//   narrowband fused back end's arithmetic) and every lane forms its outputs' y_c -- polyphaseResampleVector's terms in its
//   order -- multiplies by expjLookup(phase of output k) and adds into its accumulators.  int16 out once.
//   The window sits in LDS between zero samples: the reference's two edge rules (skip taps whose sample lies at or past the
//   window's end, stop before its start) become products with zero samples; the samples are finite, and a term of +-0 never
//   changes a non-zero running sum (a zero sum may change sign, which the complex multiply-adds and the int16 cast below lose).
//   The burst schedule is the same on every ARFCN stream, so which staged samples no burst covers (zeros) is the same for every
//   carrier: X is cleared once per tile.
//   No integer division: the (row, input offset) of every output comes from the host's tile and lane tables plus additions.
// ---------------------------------------------------------------------------------------------
template <int SPS>
__global__ __launch_bounds__(256) void k_tx_wideband(TrxTxwbArgs a) {
  extern __shared__ __attribute__((aligned(16))) char wb_lds[];
  float *TP = reinterpret_cast<float *>(wb_lds);
  cx *X = reinterpret_cast<cx *>(wb_lds + sizeof(float) * (size_t)((a.Pr * a.pitch + 1) & ~1));
  __shared__ int tb_start[64], tb_meta[64], tb_first;
  const int tile = a.tile0 + (int)blockIdx.x, w = blockIdx.y;
  const int o0 = a.o_skip + tile * TRX_TXWB_OB;
  if (o0 >= a.n_out) return;                                // (uniform)
  const int o1 = o0 + TRX_TXWB_OB < a.n_out ? o0 + TRX_TXWB_OB : a.n_out;
  const int4 td = a.tiles[tile];
  const int lo = td.y - (a.KT - 1), hi = td.z;              // staged inputs [lo, hi]: X[i - lo]
  const int slo = lo > 0 ? lo : 0, shi = hi < a.n - 1 ? hi : a.n - 1;   // of which the window holds [slo, shi]
  int row[kNJ], ix[kNJ];                                    // a lane's outputs: tap row, input offset - lo
  {
    const int2 l = a.lane[threadIdx.x];
    int r = td.x + l.x, i = td.y + l.y;
    if (r >= a.Pr) { r -= a.Pr; i++; }
#pragma unroll
    for (int j = 0; j < kNJ; j++) {
      row[j] = r; ix[j] = i - lo;
      r += a.step_r; i += a.step_i;
      if (r >= a.Pr) { r -= a.Pr; i++; }
    }
  }
  if (threadIdx.x == 0) {                                   // last burst that starts at or before slo (0 if none does)
    int a0 = 0, b0 = a.tx_n - 1;
    while (a0 < b0) { const int mid = (a0 + b0 + 1) >> 1; if (a.tx_start[mid] <= slo) a0 = mid; else b0 = mid - 1; }
    tb_first = a0 < 0 ? 0 : a0;
  }
  for (int e = threadIdx.x; e < a.Pr * a.pitch; e += 256) TP[e] = a.tpb[e];
  for (int i = threadIdx.x; i <= hi - lo; i += 256) X[i] = mk(0, 0);
  __syncthreads();
  const int m_first = tb_first;
  const int M = a.tx_n - m_first < 64 ? a.tx_n - m_first : 64;   // (a span of TRX_TXWB_XCAP samples meets at most 26 bursts)
  if ((int)threadIdx.x < M) { tb_start[threadIdx.x] = a.tx_start[m_first + threadIdx.x]; tb_meta[threadIdx.x] = a.tx_meta[m_first + threadIdx.x]; }
  double kd[kNJ];                                           // the outputs' wideband sample counts
#pragma unroll
  for (int j = 0; j < kNJ; j++) kd[j] = (double)(a.k0 + (long long)(o0 + (int)threadIdx.x + 256 * j - a.o_skip));
  cx acc[kNJ];
#pragma unroll
  for (int j = 0; j < kNJ; j++) acc[j] = mk(0, 0);
  __syncthreads();
  for (int c = 0; c < a.C; c++) {
    const size_t s = (size_t)w * a.C + c;                   // ARFCN stream w*C + c
    if (slo <= shi) tx_stage_tile<SPS>(a.T, a.ring + s * a.cap * 148, a.gring + s * a.cap, tb_start, tb_meta, M, slo, shi, X + (slo - lo));
    __syncthreads();
    const double f = (double)a.freq[c];
#pragma unroll
    for (int j = 0; j < kNJ; j++) {
      if (o0 + (int)threadIdx.x + 256 * j < o1) {
        const float *tr = TP + row[j] * a.pitch;
        const cx *xr = X + ix[j];
        cx y = mk(0, 0);
        for (int k = 0; k < a.KT; k++) y = cadd(y, cmulr(xr[-k], tr[k]));   // fi = branch + P k ascending (:1196-1200)
        // the channeliser's mixer (Oracle.mix_phase): phase of sample k formed directly, every step an IEEE operation
        const double t = kd[j] * f;
        const double kk = floor(t * 0.15915494309189535);
        const float phase = (float)(t - kk * 6.283185307179586);
        acc[j] = cadd(acc[j], cmul(y, dev_expj_lookup(a.T, phase)));
      }
    }
    __syncthreads();                                        // every lane is done with X before the next carrier lands
  }
#pragma unroll
  for (int j = 0; j < kNJ; j++) {
    const int o = o0 + (int)threadIdx.x + 256 * j;
    if (o < o1) {
      // scaleVector(z, gain) up to the sign of a zero (lost in the cast), truncation toward zero, then the DAC's clip: clamping
      // before the truncation gives the same int16 as clamping after it
      float vr = acc[j].r * a.gain, vi = acc[j].i * a.gain;
      vr = fminf(fmaxf(vr, -32768.0f), 32767.0f);
      vi = fminf(fmaxf(vi, -32768.0f), 32767.0f);
      short2 q;
      q.x = (short)(int)vr;
      q.y = (short)(int)vi;
      a.out[(size_t)w * a.out_stride + (size_t)(o - a.o_skip)] = q;
    }
  }
}

}  // namespace

hipError_t trx_launch_tx_wideband(hipStream_t st, TrxTxwbArgs a, int sps, int Sw, int n_tiles, TrxProfiler *prof) {
  if (Sw <= 0 || n_tiles <= 0 || a.n_out <= a.o_skip) return hipSuccess;
  if (Sw > 65535 || a.KT < 1 || a.KT > TRX_TXWB_KT || a.xcap < 1 || a.xcap > TRX_TXWB_XCAP ||
      sizeof(float) * (size_t)a.Pr * a.pitch > TRX_TXWB_TAPB || a.C < 1)
    return hipErrorInvalidValue;
  const size_t lds = sizeof(float) * (size_t)((a.Pr * a.pitch + 1) & ~1) + sizeof(trx_c32) * (size_t)a.xcap;
  // slices of at most 2^24 workgroups: a dispatch's work-item count stays inside 32 bits (one launch at any bench shape)
  const int per = (1 << 24) / Sw;
  if (prof) prof->begin(TRXSIG_K_TXWB, st);
  for (int t0 = 0; t0 < n_tiles; t0 += per) {
    a.tile0 = t0;
    const dim3 grid((unsigned)(n_tiles - t0 < per ? n_tiles - t0 : per), (unsigned)Sw), block(256);
    switch (sps) {
      case 1: k_tx_wideband<1><<<grid, block, lds, st>>>(a); break;
      case 2: k_tx_wideband<2><<<grid, block, lds, st>>>(a); break;
      case 4: k_tx_wideband<4><<<grid, block, lds, st>>>(a); break;
      default: return hipErrorInvalidValue;
    }
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  if (prof) prof->end(TRXSIG_K_TXWB, st);
  return hipGetLastError();
}
