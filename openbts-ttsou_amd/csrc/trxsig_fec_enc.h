// trxsig_fec_enc.h -- internal: the block coders' device routines, shared by trxsig_fec.hip (k_fec_xcch_encode,
// k_fec_tch_encode) and, through trxsig_l1mux_dev.h (mux_encode_block, mux_normal_bit), by the two transmit multiplexers'
// kernels in trxsig_l1tx.hip and trxsig_l1ms.hip (the SCH coder's kGen and the access burst's coder rach_e36 are used by those
// two files directly).  Each including file gets its own copy of the constant tables.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace {

// coder output for the 5-bit input history idx: generator 0x19 in bit 1, 0x1b in bit 0 (bv:306-330),
// two bits per entry, 32 entries
constexpr unsigned apply_poly(unsigned val, unsigned poly) {
  unsigned prod = val & poly, sum = prod;
  for (unsigned i = 1; i < 5; i++) sum ^= prod >> i;
  return sum & 1u;
}
constexpr unsigned long long gen_table() {
  unsigned long long t = 0;
  for (unsigned idx = 0; idx < 32; idx++)
    t |= (unsigned long long)((apply_poly(idx, 0x19) << 1) | apply_poly(idx, 0x1b)) << (2 * idx);
  return t;
}
constexpr unsigned long long kGen = gen_table();

struct TchPar {                                            // encoderShift response, 50 bits, generator 0x0b (3 bits)
  unsigned v[50];
  constexpr TchPar() : v() {
    for (int i = 0; i < 50; i++) {
      unsigned st = 0;
      for (int k = 0; k < 50; k++) {
        const unsigned fb = ((st >> 2) ^ (k == i ? 1u : 0u)) & 1u;
        st <<= 1;
        if (fb) st ^= 0x0bu;
      }
      v[i] = st & 7u;
    }
  }
};
__device__ __constant__ const TchPar kTchPar;

__device__ __forceinline__ void wave_fence() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

struct XcchPar {                                           // encoderShift response (bh:80-85) to a 1 at position i of 184
  unsigned long long v[184];
  constexpr XcchPar() : v() {
    unsigned long long st = 0x10004820009ULL & ((1ULL << 40) - 1);   // the bit just went in: fb = 1, state = coeff
    for (int i = 183; i >= 0; i--) {
      v[i] = st & ((1ULL << 40) - 1);
      const unsigned long long fb = (st >> 39) & 1ULL;     // one more zero behind it
      st <<= 1;
      if (fb) st ^= 0x10004820009ULL;
    }
  }
};
__device__ __constant__ const XcchPar kXcchPar;

struct TchInv {                                            // (burst b, e-bit j) -> k; j even: c_m[k], j odd: c_{m-1}[k]
  uint16_t k[4][114];
  constexpr TchInv() : k() {
    for (int c = 0; c < 456; c++) k[(c % 8) & 3][2 * ((49 * c) % 57) + ((c % 8) / 4)] = (uint16_t)c;
  }
};
__device__ __constant__ const TchInv kTchInv;

// The access burst's 36 coded bits (GSM 05.03 4.6; the inverse of RACHL1Decoder::writeLowSide, GSML1FEC.cpp:470-510), bit i of
// the result = e[i]: u[0..7] = the RA, LSB first (the decoder's LSB8MSB reads it back MSB first); u[8..13] = ~(bsic ^ parity),
// MSB first, parity = the 6-bit encoderShift register (generator 0x6f) over u[0..7]; u[14..17] = 0; the rate-1/2 coder.
// ND = 8 is that coder.  ND = 11 is the packet access burst's (GSM 05.03 5.3.2) before its puncturing: the same register over
// d(0..10), the same colouring, u(0..20), C(0..41).
template <int ND>
__device__ __forceinline__ unsigned long long access_coder(unsigned d, unsigned bsic) {
  unsigned st = 0;
  for (int k = 0; k < ND; k++) {
    const unsigned fb = ((st >> 5) ^ (d >> k)) & 1u;
    st <<= 1;
    if (fb) st ^= 0x6fu;
  }
  const unsigned p = ~(bsic ^ st) & 0x3fu;
  unsigned u = d & ((1u << ND) - 1u);
  for (int i = 0; i < 6; i++) u |= ((p >> (5 - i)) & 1u) << (ND + i);
  unsigned long long e = 0;
  unsigned acc = 0;
  for (int q = 0; q < ND + 10; q++) {
    acc = (acc << 1) | ((u >> q) & 1u);
    const unsigned long long gg = (kGen >> (2 * (acc & 31u))) & 3ULL;
    e |= (gg >> 1) << (2 * q);
    e |= (gg & 1ULL) << (2 * q + 1);
  }
  return e;
}
__device__ __forceinline__ unsigned long long rach_e36(unsigned ra, unsigned bsic) { return access_coder<8>(ra, bsic); }

// The 36 coded bits of either access-burst format (TRXSIG_ACCESS_8 / TRXSIG_ACCESS_11 of include/trxsig.h).  The 11-bit format
// does not send C(0), C(2), C(5), C(37), C(39), C(41); access_cindex is that rule the other way round, for the decoder:
// coder output C(P) -> its index in e[36], or -1 where it is deleted.
__device__ __forceinline__ unsigned long long access_e36(unsigned word, unsigned fmt, unsigned bsic) {
  if (fmt == 0) return rach_e36(word, bsic);
  const unsigned long long C = access_coder<11>(word, bsic);
  return ((C >> 1) & 1ULL) | (((C >> 3) & 3ULL) << 1) | (((C >> 6) & 0x7fffffffULL) << 3) | (((C >> 38) & 1ULL) << 34) |
         (((C >> 40) & 1ULL) << 35);
}
__device__ __forceinline__ int access_cindex(int P) {
  if (P == 0 || P == 2 || P == 5 || P == 37 || P == 39 || P == 41) return -1;
  return P < 2 ? 0 : P < 5 ? P - 2 : P < 37 ? P - 3 : P == 38 ? 34 : 35;
}

// bits 0..48 of an access burst (GSM 05.02 5.2.7): the extended tail, then the 41-bit synch sequence; bit i = the i-th sent
constexpr unsigned long long access_head() {
  const char *ab = "00111010" "01001011011111111001100110101010001111000";
  unsigned long long w = 0;
  for (int i = 0; i < 49; i++) w |= (unsigned long long)(ab[i] == '1') << i;
  return w;
}
constexpr unsigned long long kAccessHead = access_head();

enum { TCH_FILLER = 0, TCH_SPEECH = 1, TCH_FACCH = 2 };
constexpr int kTchState = 32;                              // TRXSIG_TCH_TX_STATE_BYTES
constexpr int kTchOddBytes = 29;                           // 228 bits of c[k], k mod 8 >= 4, bit i = (byte i/8 >> i%8) & 1

// c[456] of one block into LDS (one byte per bit); the whole wave calls it with the same kind.  pl: the block's 33
// payload octets (global), u: 232 bytes of LDS scratch.
__device__ void tch_form_c(int kind, const uint8_t *__restrict__ pl, const uint8_t *__restrict__ filler, uint8_t *u,
                           uint8_t *c, uint8_t *pls, int lane) {
  if (kind == TCH_SPEECH || kind == TCH_FACCH) {
    if (lane < 33) pls[lane] = pl[lane];
    wave_fence();
  }
  if (kind == TCH_SPEECH) {
    auto dq = [&](int q) { return (unsigned)(pls[q >> 3] >> (7 - (q & 7))) & 1u; };   // d[q], octets MSB first
    unsigned par = (lane < 50 && dq(lane)) ? kTchPar.v[lane] : 0u;                     // encoderShift over d[0..50)
    for (int m = 1; m < 64; m <<= 1) par ^= (unsigned)__shfl_xor((int)par, m, 64);
    par = ~par & 7u;                                                                   // writeParityWord inverts (bv:413)
    for (int i = lane; i < 189; i += 64) {
      unsigned v = 0;
      if (i <= 90) v = dq(2 * i);                                                      // u[k] = d[2k]
      else if (i <= 93) v = (par >> (93 - i)) & 1u;                                    // u[91..93] = parity, MSB first
      else if (i <= 184) v = dq(2 * (184 - i) + 1);                                    // u[184-k] = d[2k+1]
      u[i] = (uint8_t)v;                                                               // u[185..188] = 0
    }
    for (int i = lane; i < 78; i += 64) c[378 + i] = (uint8_t)dq(182 + i);             // class 2 copied
    wave_fence();
    for (int k = lane; k < 189; k += 64) {
      unsigned idx = 0;
      for (int h = 0; h < 5; h++) idx |= (k - h >= 0 ? (unsigned)u[k - h] : 0u) << h;
      const unsigned g = (unsigned)(kGen >> (2 * idx)) & 3u;
      c[2 * k] = (uint8_t)(g >> 1); c[2 * k + 1] = (uint8_t)(g & 1u);
    }
  } else if (kind == TCH_FACCH) {
    // d[] = the L2 frame after LSB8MSB: u[8o + b] = bit b of octet o; 40 inverted Fire parity bits; 4 zero tail bits
    unsigned long long par = 0;
    for (int i = lane; i < 184; i += 64)
      if ((pls[i >> 3] >> (i & 7)) & 1u) par ^= kXcchPar.v[i];
    unsigned lo = (unsigned)par, hi = (unsigned)(par >> 32);
    for (int m = 1; m < 64; m <<= 1) { lo ^= (unsigned)__shfl_xor((int)lo, m, 64); hi ^= (unsigned)__shfl_xor((int)hi, m, 64); }
    const unsigned long long pw = ~(((unsigned long long)hi << 32) | lo) & ((1ULL << 40) - 1);
    for (int i = lane; i < 228; i += 64) {
      unsigned v = 0;
      if (i < 184) v = (pls[i >> 3] >> (i & 7)) & 1u;
      else if (i < 224) v = (unsigned)(pw >> (39 - (i - 184))) & 1u;
      u[i] = (uint8_t)v;
    }
    wave_fence();
    for (int k = lane; k < 228; k += 64) {
      unsigned idx = 0;
      for (int h = 0; h < 5; h++) idx |= (k - h >= 0 ? (unsigned)u[k - h] : 0u) << h;
      const unsigned g = (unsigned)(kGen >> (2 * idx)) & 3u;
      c[2 * k] = (uint8_t)(g >> 1); c[2 * k + 1] = (uint8_t)(g & 1u);
    }
  } else {
    for (int i = lane; i < 456; i += 64) c[i] = kind == TCH_FILLER ? (uint8_t)(filler[i] & 1u) : (uint8_t)0;
  }
  wave_fence();
}

}  // namespace
