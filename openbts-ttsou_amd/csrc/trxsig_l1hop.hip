// trxsig_l1hop.hip -- the hopping stage's kernels (include/trxsig_l1hop.h, host side in trxsig_l1hop.cpp, the sequence itself in
// trxsig_hop_dev.h).
//
// Every kernel computes the sequence itself: RNTABLE lies in constant memory (k_hop_mai, whose index differs lane by lane,
// copies it into LDS first), and none reads the array trxsig_l1hop_map returns.  In a slot, the channels of one group are a
// rotation of its allocation by S(FN, HSN, N): rank r goes to rank (r + S) mod N, and comes from rank (r - S) mod N.
//   k_hop_mai     the primitive, a lane per entry.
//   k_hop_map     a thread per (slot, row): the radio row of a channel row.
//   k_hop_result  a thread per (slot, row): the entry of a pull's d_row at that radio row (indices move, soft rows stay).
//   k_hop_bits    a workgroup per (slot, group), in place: the N member rows (37 dwords each) and their `what` bytes go into LDS,
//                 consecutive lanes on consecutive dwords; a barrier; then every row is stored from its rotated source.  Without
//                 the staging a row could be overwritten before the workgroup that needs it has read it.
//   k_hop_cells   a bandwidth-bound gather, out of place: a wave per cell and round of a grid-stride loop.  The wave finds the
//                 source row of its output cell (scalar work: the cell index is wave-uniform) and copies the cell with consecutive
//                 lanes on consecutive 16-byte (or, where a cell start is not 16-byte aligned, 8-byte) words, kCellBatch loads
//                 a lane issued before the first store: at sps 4 a cell is 314 16-byte words, one batch of five a lane.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "trxsig_dev.h"
#include "trxsig_hop_dev.h"
#include "trxsig_tdma.h"

namespace {

__constant__ uint8_t kHopRn[kHopTable] = TRX_HOP_RNTABLE_INIT;

constexpr int kHopGridMax = 2048;                           // workgroups of 256: eight a CU on 256 CUs
constexpr int kCellBatch = 5;                               // loads a lane has in flight before its first store

// the place in its allocation that rank `r` of (tn, group gi) goes to (dir = 1) or comes from (dir = 0) in frame fnw
__device__ __forceinline__ int hop_rotate(const TrxHopDev &d, int g, int n, int r, int fnw, int dir) {
  const int s = hop_s(fnw, d.hsn[g], n, kHopRn);
  return dir ? hop_wrap(r + s, n) : hop_wrap(r - s + n, n);
}

// the row that row a's slot goes to (dir = 1: the radio row of channel row a) or comes from (dir = 0: the channel row of radio
// row a) in slot (tn, fnw); a itself where the slot does not hop
__device__ __forceinline__ int hop_row(const TrxHopDev &d, int a, int tn, int fnw, int dir) {
  const int g = d.group[tn * d.n_arfcn + a];
  if (g < 0) return a;
  const int gi = tn * d.n_groups + g, n = d.count[gi];
  return d.member[gi * kHopMaxN + hop_rotate(d, g, n, d.rank[tn * d.n_arfcn + a], fnw, dir)];
}

__global__ __launch_bounds__(256) void k_hop_mai(int n, const int32_t *__restrict__ fn, const int32_t *__restrict__ hsn,
                                                 const int32_t *__restrict__ maio, const int32_t *__restrict__ nn,
                                                 int32_t *__restrict__ mai) {
  __shared__ uint8_t rn[kHopTable];
  if (threadIdx.x < kHopTable) rn[threadIdx.x] = kHopRn[threadIdx.x];
  __syncthreads();
  const int i = (int)blockIdx.x * 256 + (int)threadIdx.x;    // n <= 2^24 (the host checks)
  if (i < n) mai[i] = hop_mai(fn[i], hsn[i], maio[i], nn[i], rn);
}

__global__ __launch_bounds__(256) void k_hop_map(TrxHopDev d, int fn, int n_slots, int32_t *__restrict__ out) {
  const int N = n_slots * d.n_arfcn;                         // at most 2^30 (the host checks)
  for (int i = (int)blockIdx.x * 256 + (int)threadIdx.x; i < N; i += (int)gridDim.x * 256) {
    const int t = i / d.n_arfcn, a = i - t * d.n_arfcn;
    out[i] = hop_row(d, a, t & 7, (fn + t / 8) % kTrxHyperframe, 1);
  }
}

__global__ __launch_bounds__(256) void k_hop_result(TrxHopDev d, int fn, int n_slots, const int32_t *__restrict__ src,
                                                    int32_t *__restrict__ out) {
  const int N = n_slots * d.n_arfcn;
  for (int i = (int)blockIdx.x * 256 + (int)threadIdx.x; i < N; i += (int)gridDim.x * 256) {
    const int t = i / d.n_arfcn, a = i - t * d.n_arfcn;
    out[i] = src[t * d.n_arfcn + hop_row(d, a, t & 7, (fn + t / 8) % kTrxHyperframe, 1)];
  }
}

__global__ __launch_bounds__(256) void k_hop_bits(TrxHopDev d, int to_radio, int fn, int n_frames, uint32_t *__restrict__ bits,
                                                  uint8_t *__restrict__ what) {
  __shared__ uint32_t rows[kHopMaxN * 37];
  __shared__ uint8_t wh[kHopMaxN];
  const int t = blockIdx.x, g = blockIdx.y, tn = t & 7;
  const int gi = tn * d.n_groups + g, n = d.count[gi];
  if (n <= 1) return;                                        // (uniform over the workgroup)
  const int s = hop_s((fn + t / 8) % kTrxHyperframe, d.hsn[g], n, kHopRn);
  if (s == 0) return;                                        // every row stays
  const size_t T = 8 * (size_t)n_frames;
  const int32_t *mem = d.member + gi * kHopMaxN;
  const int tid = threadIdx.x;
  for (int e = tid; e < n * 37; e += 256) {
    const int r = e / 37, dw = e - 37 * r;
    rows[e] = bits[((size_t)mem[r] * T + t) * 37 + dw];
  }
  if (what && tid < n) wh[tid] = what[(size_t)mem[tid] * T + t];
  __syncthreads();
  for (int e = tid; e < n * 37; e += 256) {                  // rank r receives rank q's row
    const int r = e / 37, dw = e - 37 * r;
    const int q = to_radio ? hop_wrap(r - s + n, n) : hop_wrap(r + s, n);
    bits[((size_t)mem[r] * T + t) * 37 + dw] = rows[q * 37 + dw];
  }
  if (what && tid < n) what[(size_t)mem[tid] * T + t] = wh[to_radio ? hop_wrap(tid - s + n, n) : hop_wrap(tid + s, n)];
}

template <typename V>
__device__ __forceinline__ void hop_copy(const V *__restrict__ ip, V *__restrict__ op, int n, int lane) {
  for (int base = 0; base < n; base += 64 * kCellBatch) {
    V v[kCellBatch];
#pragma unroll
    for (int u = 0; u < kCellBatch; u++) {
      const int i = base + 64 * u + lane;
      if (i < n) v[u] = ip[i];
    }
#pragma unroll
    for (int u = 0; u < kCellBatch; u++) {
      const int i = base + 64 * u + lane;
      if (i < n) op[i] = v[u];
    }
  }
}

template <bool WIDE>
__global__ __launch_bounds__(256) void k_hop_cells(TrxHopDev d, TrxHopCells c) {
  const int lane = threadIdx.x & 63;
  const int T = 8 * c.n_frames, N = T * d.n_arfcn;           // at most 2^30 (the host checks)
  const int wave0 = __builtin_amdgcn_readfirstlane((int)blockIdx.x * 4 + (int)(threadIdx.x >> 6));
  for (int cell = wave0; cell < N; cell += (int)gridDim.x * 4) {
    const int t = cell / d.n_arfcn, a = cell - t * d.n_arfcn;  // the output cell: slot t of row a
    const int src = hop_row(d, a, t & 7, (c.fn + t / 8) % kTrxHyperframe, c.to_radio ? 0 : 1);
    const int n = (156 + ((t & 3) == 0)) * c.sps;            // samples
    const float2 *ip = c.in + t * c.in_slot + src * c.in_arfcn;
    float2 *op = c.out + t * c.out_slot + a * c.out_arfcn;
    if (WIDE) {                                              // both cell starts are 16-byte aligned (the host checked)
      hop_copy(reinterpret_cast<const float4 *>(ip), reinterpret_cast<float4 *>(op), n >> 1, lane);
      if ((n & 1) && lane == 0) op[n - 1] = ip[n - 1];
    } else {
      hop_copy(ip, op, n, lane);
    }
  }
}

inline int hop_grid(long long n, int per) {
  const long long g = (n + per - 1) / per;
  return (int)(g < kHopGridMax ? g : kHopGridMax);
}

}  // namespace

hipError_t trx_launch_hop_mai(hipStream_t st, int n, const int32_t *fn, const int32_t *hsn, const int32_t *maio, const int32_t *nn,
                              int32_t *mai) {
  if (n <= 0) return hipSuccess;
  k_hop_mai<<<dim3((n + 255) / 256), dim3(256), 0, st>>>(n, fn, hsn, maio, nn, mai);
  return hipGetLastError();
}

hipError_t trx_launch_hop_map(hipStream_t st, const TrxHopDev &dv, int fn, int n_frames, const int32_t *src, int32_t *out) {
  const long long n = 8LL * n_frames * dv.n_arfcn;
  if (n <= 0) return hipSuccess;
  if (src)
    k_hop_result<<<dim3(hop_grid(n, 256)), dim3(256), 0, st>>>(dv, fn, 8 * n_frames, src, out);
  else
    k_hop_map<<<dim3(hop_grid(n, 256)), dim3(256), 0, st>>>(dv, fn, 8 * n_frames, out);
  return hipGetLastError();
}

hipError_t trx_launch_hop_bits(hipStream_t st, const TrxHopDev &dv, int to_radio, int fn, int n_frames, uint8_t *bits, uint8_t *what) {
  if (n_frames <= 0 || dv.n_groups <= 0) return hipSuccess;
  k_hop_bits<<<dim3(8 * n_frames, dv.n_groups), dim3(256), 0, st>>>(dv, to_radio, fn, n_frames, reinterpret_cast<uint32_t *>(bits), what);
  return hipGetLastError();
}

hipError_t trx_launch_hop_cells(hipStream_t st, const TrxHopDev &dv, const TrxHopCells &call, bool wide) {
  const long long n = 8LL * call.n_frames * dv.n_arfcn;
  if (n <= 0) return hipSuccess;
  if (wide)
    k_hop_cells<true><<<dim3(hop_grid(n, 4)), dim3(256), 0, st>>>(dv, call);
  else
    k_hop_cells<false><<<dim3(hop_grid(n, 4)), dim3(256), 0, st>>>(dv, call);
  return hipGetLastError();
}
