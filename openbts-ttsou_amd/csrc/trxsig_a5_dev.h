// trxsig_a5_dev.h -- internal: A5/1 (GSM 03.20 Annex C) as include/trxsig_l1ciph.h states it, for the host (the 64 key steps of
// trxsig_l1ciph_set) and the device (trxsig_l1ciph.hip), and what the ciphering object's host side and kernels share.
// Pure 32-bit integer work: three registers in three words, every step branch-free (a register that does not move keeps its
// word through a select), so the 64 lanes of a wave -- 64 slots with 64 keys -- never diverge.
#pragma once
#include <hip/hip_runtime_api.h>
#include <stdint.h>

struct TrxA5 {
  uint32_t r1, r2, r3;
};

constexpr uint32_t kA5Mask1 = (1u << 19) - 1, kA5Mask2 = (1u << 22) - 1, kA5Mask3 = (1u << 23) - 1;

// the feedback taps: R1 bits 18, 17, 16, 13; R2 bits 21, 20; R3 bits 22, 21, 20, 7.  The XOR of a register's tap bits is the parity of
// the register under the tap mask: an AND, a bit count and an AND, whatever the number of taps.
constexpr uint32_t kA5Taps1 = 1u << 18 | 1u << 17 | 1u << 16 | 1u << 13, kA5Taps2 = 1u << 21 | 1u << 20,
                   kA5Taps3 = 1u << 22 | 1u << 21 | 1u << 20 | 1u << 7;

__host__ __device__ inline uint32_t a5_parity(uint32_t x) { return (uint32_t)__builtin_popcount(x) & 1u; }
__host__ __device__ inline uint32_t a5_next1(uint32_t r) { return ((r << 1) & kA5Mask1) | a5_parity(r & kA5Taps1); }
__host__ __device__ inline uint32_t a5_next2(uint32_t r) { return ((r << 1) & kA5Mask2) | a5_parity(r & kA5Taps2); }
__host__ __device__ inline uint32_t a5_next3(uint32_t r) { return ((r << 1) & kA5Mask3) | a5_parity(r & kA5Taps3); }

// clock all three, then XOR `bit` (0 or 1) into bit 0 of each
__host__ __device__ inline void a5_clock_all(TrxA5 &s, uint32_t bit) {
  s.r1 = a5_next1(s.r1) ^ bit;
  s.r2 = a5_next2(s.r2) ^ bit;
  s.r3 = a5_next3(s.r3) ^ bit;
}

// one majority-clocked step; returns the output bit after it
__host__ __device__ inline uint32_t a5_clock_maj(TrxA5 &s) {
  const uint32_t c1 = (s.r1 >> 8) & 1u, c2 = (s.r2 >> 10) & 1u, c3 = (s.r3 >> 10) & 1u;
  const uint32_t m = (c1 + c2 + c3) >> 1;                    // the majority of three bits
  const uint32_t n1 = a5_next1(s.r1), n2 = a5_next2(s.r2), n3 = a5_next3(s.r3);
  s.r1 = c1 == m ? n1 : s.r1;
  s.r2 = c2 == m ? n2 : s.r2;
  s.r3 = c3 == m ? n3 : s.r3;
  return ((s.r1 >> 18) ^ (s.r2 >> 21) ^ (s.r3 >> 22)) & 1u;
}

// the 64 key steps from all-zero registers
__host__ __device__ inline TrxA5 a5_key(const uint8_t *kc) {
  TrxA5 s{ 0, 0, 0 };
  for (int i = 0; i < 64; i++) a5_clock_all(s, (uint32_t)(kc[i >> 3] >> (i & 7)) & 1u);
  return s;
}

// from the state after the key: the 22 count steps and the 100 steps thrown away
__host__ __device__ inline void a5_frame(TrxA5 &s, uint32_t count) {
  for (int i = 0; i < 22; i++) a5_clock_all(s, (count >> i) & 1u);
  for (int i = 0; i < 100; i++) (void)a5_clock_maj(s);
}

// the next 114 output bits, bit k in w[k / 32] bit k % 32 (w[3]'s bits 18..31 zero)
__host__ __device__ inline void a5_block(TrxA5 &s, uint32_t w[4]) {
  for (int j = 0; j < 4; j++) {
    uint32_t v = 0;
    const int n = j < 3 ? 32 : 18;
    for (int b = 0; b < n; b++) v |= a5_clock_maj(s) << b;
    w[j] = v;
  }
}

__host__ __device__ inline uint32_t a5_count(int fn) { return (uint32_t)(fn / 1326) << 11 | (uint32_t)(fn % 51) << 5 | (uint32_t)(fn % 26); }

// ---- the ciphering object (include/trxsig_l1ciph.h; trxsig_l1ciph.cpp / .hip) ---------------------------------------------
struct TrxCiphRec {                  // a channel's record (TRXSIG_L1CIPH_STATE_BYTES)
  uint32_t algo, r1, r2, r3;
};
static_assert(sizeof(TrxCiphRec) == 16, "TrxCiphRec layout");

struct TrxCiphDev {
  const int32_t *slot;               // [n_arfcn * 8]: combination (0, 1, 5, 7) | the slot's TCH channel << 4
  const int32_t *slot_x;             // [n_arfcn * 8]: the slot's first XCCH channel, as an index into rec
  const int8_t *route;               // [2 downlink / uplink][3 combination I / V / VII][8 TN][104 FN mod 104 (I) or 102 (V, VII)]:
                                     // -1 nobody's, 0 the slot's TCH, 1 + j the slot's j-th XCCH channel
  const TrxCiphRec *rec;             // [n_tch + n_xcch]
};

struct TrxCiphCall {
  int uplink, fn, n_frames, n_arfcn;
  uint32_t what_mask;                // bits
  int n_rows, soft_stride;           // soft
};

hipError_t trx_launch_a5_blocks(hipStream_t st, int n, const uint8_t *kc, const uint32_t *count, uint8_t *block1, uint8_t *block2);
hipError_t trx_launch_l1ciph_set(hipStream_t st, TrxCiphRec *rec, uint32_t algo, TrxA5 key);
hipError_t trx_launch_l1ciph_bits(hipStream_t st, const TrxCiphCall &call, const TrxCiphDev &dv, uint8_t *bits, const uint8_t *what);
hipError_t trx_launch_l1ciph_soft(hipStream_t st, const TrxCiphCall &call, const TrxCiphDev &dv, const int32_t *row,
                                  const uint8_t *valid, float *soft);
