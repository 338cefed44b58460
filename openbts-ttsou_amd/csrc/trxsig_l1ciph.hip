// trxsig_l1ciph.hip -- the ciphering stage's kernels (include/trxsig_l1ciph.h, host side in trxsig_l1ciph.cpp, A5/1 itself in
// trxsig_a5_dev.h).
//
// Two phases per wave and round of 64 slots, both kernels alike:
//   generation   a lane per slot.  The lane finds the slot's owner (the host's route table by combination, TN and FN mod 104 /
//                102; then the channel's record), and where the slot is ciphered runs its generator from the record's registers:
//                22 + 100 clocks, then 114 (downlink: BLOCK1) or 228 (uplink: BLOCK1 cannot be skipped) -- the keystream in four
//                words in registers.  A lane whose slot is not ciphered clocks nothing; the generator is branch-free, so the
//                ciphered lanes of a wave run in step.
//   application  lane-per-burst would touch 148-byte (or soft_stride-float) rows a word per lane and row: uncoalesced.  Instead
//                the wave stages its keystream words in LDS (16 bytes a slot), lists its ciphered slots, and walks their rows
//                with consecutive lanes on consecutive words: k_l1ciph_bits two rows a step, 30 lanes a row on the 30 dwords
//                that hold payload bytes (dwords 0..14 and 22..36 of the 37); k_l1ciph_soft a row a step, lanes on the 114
//                payload floats.  Rows of slots that are not ciphered are neither read nor written.  A wave's steps depend on
//                nothing but memory latency, and there are fewer than two waves a SIMD on the production plan, so the steps go
//                in batches of kCiphBatch: all of a batch's loads are issued before its first store.
// The LDS arrays are private to a wave (no workgroup barrier: the waves of a workgroup run different numbers of rounds), and the
// grid strides over the slots, so a call larger than the grid is the same call.
// k_a5_blocks is the primitive: the whole key setup on the device, both blocks, staged and written the same way.
// k_l1ciph_set is a channel's key change in stream order: one thread, the record's four words from its arguments.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "trxsig_dev.h"
#include "trxsig_a5_dev.h"
#include "trxsig_tdma.h"

namespace {

constexpr int kCiphGridMax = 2048;                          // workgroups of 256: eight a CU on 256 CUs
constexpr int kCiphBatch = 8;                               // steps of the application whose loads are in flight together

// the record of the channel slot (a, t) belongs to in this direction, or null.  slot_i = a * 8 + TN
__device__ __forceinline__ const TrxCiphRec *ciph_owner(const TrxCiphCall &c, const TrxCiphDev &d, int a, int tn, int fnw) {
  const int sl = d.slot[a * 8 + tn], comb = sl & 15;
  if (comb == 0) return nullptr;
  const int cix = comb == 1 ? 0 : comb == 5 ? 1 : 2;
  const int r = comb == 1 ? fnw % 104 : fnw % 102;
  const int code = d.route[((c.uplink * 3 + cix) * 8 + tn) * 104 + r];
  if (code < 0) return nullptr;
  return d.rec + (code == 0 ? sl >> 4 : d.slot_x[a * 8 + tn] + code - 1);
}

// the slot's keystream from its channel's registers: BLOCK1 (downlink) or BLOCK2 (uplink) of COUNT(fnw)
__device__ __forceinline__ void ciph_generate(const TrxCiphRec &rec, int uplink, int fnw, uint32_t w[4]) {
  TrxA5 s{ rec.r1, rec.r2, rec.r3 };
  a5_frame(s, a5_count(fnw));
  a5_block(s, w);
  if (uplink) a5_block(s, w);
}

// the four keystream bits of burst bytes 4 dw .. 4 dw + 3 as a byte mask (0 or 1 in each byte): burst bit p carries keystream
// bit p - 3 (3 <= p < 60) or p - 31 (88 <= p < 145)
__device__ __forceinline__ uint32_t ciph_byte_mask(const uint32_t *ks, int dw) {
  uint32_t m = 0;
#pragma unroll
  for (int i = 0; i < 4; i++) {
    const int p = 4 * dw + i;
    const int k = p < 60 ? p - 3 : p - 31;
    const bool on = (p >= 3 && p < 60) || (p >= 88 && p < 145);
    const uint32_t bit = on ? (ks[k >> 5] >> (k & 31)) & 1u : 0u;
    m |= bit << (8 * i);
  }
  return m;
}

__global__ __launch_bounds__(256) void k_l1ciph_bits(TrxCiphCall c, TrxCiphDev d, uint32_t *__restrict__ bits,
                                                     const uint8_t *__restrict__ what) {
  __shared__ uint32_t ks[4][64][4];
  __shared__ uint8_t list[4][64];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int T = 8 * c.n_frames, N = T * c.n_arfcn;           // at most 2^30 (the host checks): 32-bit indices, no 64-bit division
  for (int base = ((int)blockIdx.x * 4 + wv) * 64; base < N; base += (int)gridDim.x * 256) {
    const int i = base + lane;                               // slot i = a * T + t: d_bits' and d_what's order
    const TrxCiphRec *rec = nullptr;
    int fnw = 0;
    if (i < N) {
      const int a = i / T, t = i - a * T;
      fnw = (c.fn + t / 8) % kTrxHyperframe;
      rec = ciph_owner(c, d, a, t & 7, fnw);
      if (rec && rec->algo == 0) rec = nullptr;
      if (rec && what) {
        const unsigned w = what[i];
        if (w > 31 || !((c.what_mask >> w) & 1u)) rec = nullptr;
      }
    }
    const bool on = rec != nullptr;
    const unsigned long long bal = __ballot(on);
    if (bal == 0) continue;                                  // (wave-uniform)
    wave_lds_fence();                                        // the round before has read its list
    if (on) {
      uint32_t w[4];
      ciph_generate(*rec, c.uplink, fnw, w);
      list[wv][__popcll(bal & ((1ull << lane) - 1))] = (uint8_t)lane;
#pragma unroll
      for (int j = 0; j < 4; j++) ks[wv][lane][j] = w[j];
    }
    wave_lds_fence();
    const int n = __popcll(bal);
    const int half = lane / 30, q = lane - 30 * half;        // lanes 0..29 the step's first row, 30..59 its second
    const int dw = q < 15 ? q : q + 7;
    for (int p = 0; p < n; p += 2 * kCiphBatch) {             // a batch of steps: every load issued before the first store
      uint32_t *at[kCiphBatch], v[kCiphBatch], m[kCiphBatch];
#pragma unroll
      for (int u = 0; u < kCiphBatch; u++) {
        const int idx = p + 2 * u + half;
        at[u] = nullptr;
        if (half < 2 && idx < n) {
          const int src = list[wv][idx];
          at[u] = bits + (size_t)(base + src) * 37 + dw;
          m[u] = ciph_byte_mask(ks[wv][src], dw);
          v[u] = *at[u];
        }
      }
#pragma unroll
      for (int u = 0; u < kCiphBatch; u++)
        if (at[u]) *at[u] = v[u] ^ m[u];
    }
  }
}

__global__ __launch_bounds__(256) void k_l1ciph_soft(TrxCiphCall c, TrxCiphDev d, const int32_t *__restrict__ rowix,
                                                     const uint8_t *__restrict__ valid, float *__restrict__ soft) {
  __shared__ uint32_t ks[4][64][4];
  __shared__ int32_t list[4][64];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int T = 8 * c.n_frames, N = T * c.n_arfcn;           // at most 2^30 (the host checks): 32-bit indices, no 64-bit division
  for (int base = ((int)blockIdx.x * 4 + wv) * 64; base < N; base += (int)gridDim.x * 256) {
    const int i = base + lane;                               // slot i = t * n_arfcn + a: d_row's order
    const TrxCiphRec *rec = nullptr;
    int fnw = 0, r = -1;
    if (i < N) {
      const int t = i / c.n_arfcn, a = i - t * c.n_arfcn;
      r = rowix[i];
      if (r >= 0 && r < c.n_rows && valid[r] != 0) {
        fnw = (c.fn + t / 8) % kTrxHyperframe;
        rec = ciph_owner(c, d, a, t & 7, fnw);
        if (rec && rec->algo == 0) rec = nullptr;
      }
    }
    const bool on = rec != nullptr;
    const unsigned long long bal = __ballot(on);
    if (bal == 0) continue;
    wave_lds_fence();
    if (on) {
      uint32_t w[4];
      ciph_generate(*rec, c.uplink, fnw, w);
      const int at = __popcll(bal & ((1ull << lane) - 1));
      list[wv][at] = r;
#pragma unroll
      for (int j = 0; j < 4; j++) ks[wv][at][j] = w[j];
    }
    wave_lds_fence();
    const int n = __popcll(bal);
    for (int p = 0; p < n; p += kCiphBatch) {                 // a batch of rows: every load issued before the first store
      float *at[kCiphBatch][2], v[kCiphBatch][2];
#pragma unroll
      for (int u = 0; u < kCiphBatch; u++)
#pragma unroll
        for (int h = 0; h < 2; h++) {
          const int k = lane + 64 * h;
          at[u][h] = nullptr;
          if (p + u < n && k < 114 && ((ks[wv][p + u][k >> 5] >> (k & 31)) & 1u)) {
            at[u][h] = soft + (size_t)list[wv][p + u] * c.soft_stride + (k < 57 ? 3 + k : 31 + k);
            v[u][h] = *at[u][h];
          }
        }
#pragma unroll
      for (int u = 0; u < kCiphBatch; u++)
#pragma unroll
        for (int h = 0; h < 2; h++)
          if (at[u][h]) *at[u][h] = 1.0f - v[u][h];
    }
  }
}

__global__ __launch_bounds__(256) void k_a5_blocks(int n, const uint8_t *__restrict__ kc, const uint32_t *__restrict__ count,
                                                   uint8_t *__restrict__ block1, uint8_t *__restrict__ block2) {
  __shared__ uint32_t ks[4][64][8];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  for (int base = ((int)blockIdx.x * 4 + wv) * 64; base < n; base += (int)gridDim.x * 256) {   // n <= 2^24 (the host checks)
    const int i = base + lane;
    wave_lds_fence();
    if (i < n) {
      uint8_t key[8];
#pragma unroll
      for (int j = 0; j < 8; j++) key[j] = kc[(size_t)i * 8 + j];
      TrxA5 s = a5_key(key);
      a5_frame(s, count[i]);
      uint32_t w[8];
      a5_block(s, w);
      a5_block(s, w + 4);
#pragma unroll
      for (int j = 0; j < 8; j++) ks[wv][lane][j] = w[j];
    }
    wave_lds_fence();
    const int m = n - base < 64 ? n - base : 64;
    for (int e = lane; e < m * 114; e += 64) {               // consecutive lanes on consecutive output bytes
      const int s = e / 114, k = e - 114 * s;
      if (block1) block1[(size_t)base * 114 + e] = (uint8_t)((ks[wv][s][k >> 5] >> (k & 31)) & 1u);
      if (block2) block2[(size_t)base * 114 + e] = (uint8_t)((ks[wv][s][4 + (k >> 5)] >> (k & 31)) & 1u);
    }
  }
}

__global__ void k_l1ciph_set(TrxCiphRec *rec, uint32_t algo, TrxA5 key) {
  if (threadIdx.x != 0) return;
  rec->algo = algo;
  rec->r1 = key.r1;
  rec->r2 = key.r2;
  rec->r3 = key.r3;
}

inline int ciph_grid(long long n) {
  const long long g = (n + 255) / 256;
  return (int)(g < kCiphGridMax ? g : kCiphGridMax);
}

}  // namespace

hipError_t trx_launch_a5_blocks(hipStream_t st, int n, const uint8_t *kc, const uint32_t *count, uint8_t *block1, uint8_t *block2) {
  if (n <= 0) return hipSuccess;
  k_a5_blocks<<<dim3(ciph_grid(n)), dim3(256), 0, st>>>(n, kc, count, block1, block2);
  return hipGetLastError();
}

hipError_t trx_launch_l1ciph_set(hipStream_t st, TrxCiphRec *rec, uint32_t algo, TrxA5 key) {
  k_l1ciph_set<<<dim3(1), dim3(64), 0, st>>>(rec, algo, key);
  return hipGetLastError();
}

hipError_t trx_launch_l1ciph_bits(hipStream_t st, const TrxCiphCall &call, const TrxCiphDev &dv, uint8_t *bits, const uint8_t *what) {
  const long long n = 8LL * call.n_frames * call.n_arfcn;
  if (n <= 0) return hipSuccess;
  k_l1ciph_bits<<<dim3(ciph_grid(n)), dim3(256), 0, st>>>(call, dv, reinterpret_cast<uint32_t *>(bits), what);
  return hipGetLastError();
}

hipError_t trx_launch_l1ciph_soft(hipStream_t st, const TrxCiphCall &call, const TrxCiphDev &dv, const int32_t *row,
                                  const uint8_t *valid, float *soft) {
  const long long n = 8LL * call.n_frames * call.n_arfcn;
  if (n <= 0 || call.n_rows <= 0) return hipSuccess;
  k_l1ciph_soft<<<dim3(ciph_grid(n)), dim3(256), 0, st>>>(call, dv, row, valid, soft);
  return hipGetLastError();
}
