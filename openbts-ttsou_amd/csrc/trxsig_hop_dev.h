// trxsig_hop_dev.h -- internal: the GSM 05.02 section 6.2.3 hopping sequence as include/trxsig_l1hop.h states it, for the host and the
// device, and what the hopping object's host side (trxsig_l1hop.cpp) and kernels (trxsig_l1hop.hip) share.
// Pure 32-bit integer work.  S, the part of the sequence that does not depend on the MAIO, is a function of (FN, HSN, N) alone:
// the kernels compute it once per (slot, group) and rotate the allocation by it.
#pragma once
#include <hip/hip_runtime_api.h>
#include <stdint.h>

// RNTABLE, GSM 05.02 table 6: 114 entries.  The kernels keep it in constant memory (an index that is uniform over a wave) or
// copy it into LDS (k_hop_mai: an index per lane).
#define TRX_HOP_RNTABLE_INIT                                                                                                        \
  { 48,  98,  63,  1,   36,  95,  78,  102, 94,  73,  0,   64,  25,  81,  76,  59,  124, 23,  104, 100, 101, 47,  118,              \
    85,  18,  56,  96,  86,  54,  2,   80,  34,  127, 13,  6,   89,  57,  103, 12,  74,  55,  111, 75,  38,  109, 71,               \
    112, 29,  11,  88,  87,  19,  3,   68,  110, 26,  33,  31,  8,   45,  82,  58,  40,  107, 32,  5,   106, 92,  62,               \
    67,  77,  108, 122, 37,  60,  66,  121, 42,  51,  126, 117, 114, 4,   90,  43,  52,  53,  113, 120, 72,  16,  49,               \
    7,   79,  119, 61,  22,  84,  9,   97,  91,  15,  21,  24,  46,  39,  93,  105, 65,  70,  125, 99,  17,  123 }
constexpr int kHopTable = 114;
constexpr int kHopMaxN = 64;          // frequencies in a mobile allocation

// x mod n for x in [0, 2 n): a compare and a subtraction.  (The small remainders of the sequence are formed this way, not with
// %: for operands it knows to be small the compiler divides in float32 with an fma, which the kernels' listings must not hold.)
__host__ __device__ inline int hop_wrap(int x, int n) { return x >= n ? x - n : x; }

// S of (FN, HSN, N): MAI = (S + MAIO) mod N.  fn in [0, 2715648), hsn in 0..63, n in 1..64; rn: RNTABLE
__host__ __device__ inline int hop_s(int fn, int hsn, int n, const uint8_t *rn) {
  if (hsn == 0) {                                             // cyclic: fn mod n by the reciprocal, exact for fn < 2^22 and n <= 64
    if (n == 1) return 0;                                     // (ceil(2^32 / n) n - 2^32 < n and fn n < 2^32)
    const unsigned rcp = 0xFFFFFFFFu / (unsigned)n + 1u;
    return fn - (int)(((unsigned long long)(unsigned)fn * rcp) >> 32) * n;
  }
  const int t1r = (fn / 1326) & 63, t2 = fn % 26, t3 = fn % 51;
  const int mask = (2 << (31 - __builtin_clz((unsigned)n))) - 1;   // 2^NBIN - 1, NBIN = floor(log2 n) + 1
  const int m = (t2 + rn[(hsn ^ t1r) + t3]) & mask, tp = t3 & mask;
  return m < n ? m : hop_wrap(hop_wrap(m + tp, 2 * n), n);   // M' and T' are below 2^NBIN <= 2 n: the sum is below 4 n
}
__host__ __device__ inline int hop_mai(int fn, int hsn, int maio, int n, const uint8_t *rn) { return hop_wrap(hop_s(fn, hsn, n, rn) + maio, n); }

// ---- the hopping object (include/trxsig_l1hop.h; trxsig_l1hop.cpp / .hip) ------------------------------------------------------
struct TrxHopDev {
  int n_arfcn, n_groups;
  const int8_t *group;               // [8 TN][n_arfcn]: the row's group on that TN, -1 where the slot does not hop
  const uint8_t *rank;               // [8 TN][n_arfcn]: the row's place in its allocation (its MAIO)
  const uint8_t *count;              // [8 TN][n_groups]: N of (TN, group), 0 where the group has no member there
  const int32_t *member;             // [8 TN][n_groups][64]: the allocation's rows in ascending order
  const uint8_t *hsn;                // [n_groups]
};

struct TrxHopCells {
  const float2 *in;
  float2 *out;
  long long in_slot, in_arfcn, out_slot, out_arfcn;   // strides in samples
  int fn, n_frames, to_radio, sps;
};

hipError_t trx_launch_hop_mai(hipStream_t st, int n, const int32_t *fn, const int32_t *hsn, const int32_t *maio, const int32_t *nn, int32_t *mai);
hipError_t trx_launch_hop_map(hipStream_t st, const TrxHopDev &dv, int fn, int n_frames, const int32_t *src, int32_t *out);
hipError_t trx_launch_hop_bits(hipStream_t st, const TrxHopDev &dv, int to_radio, int fn, int n_frames, uint8_t *bits, uint8_t *what);
hipError_t trx_launch_hop_cells(hipStream_t st, const TrxHopDev &dv, const TrxHopCells &call, bool wide);
