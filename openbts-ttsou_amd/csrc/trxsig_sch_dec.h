// trxsig_sch_dec.h -- internal: the verdict on a decoded SCH burst, shared by the mobile-side downlink L1 (k_l1msrx_finish,
// trxsig_l1msrx.hip) and trxsig_fec_sch_decode_batch (k_fec_viterbi's SCH mode, trxsig_fec.hip).  Integer work only.
// ubit(q) = u[q], the q-th of the 39 bits SoftVector::decode gave (include/trxsig_l1msrx.h states the arithmetic): ok = the
// four tail bits are zero and u[25..35) is the inverted parity (generator 0x575) of u[0..25); LSB8MSB undone on the first three
// octets; BSIC (6) T1 (11) T2 (5) T3' (3) MSB first; rfn = 1326 T1 + 51 ((T3 - T2) mod 26) + T3 with T3 = 10 T3' + 1.
#pragma once
#include <hip/hip_runtime.h>

template <class UBit>
__device__ __forceinline__ void trx_sch_verdict(UBit ubit, unsigned *ok, unsigned *bsic, int *rfn) {
  unsigned dw = 0, par = 0, sent = 0;                     // dw: bit 24 - q = u[q]
  for (int q = 0; q < 25; q++) {
    const unsigned b = ubit(q) & 1u;
    dw = (dw << 1) | b;
    const unsigned fb = ((par >> 9) ^ b) & 1u;            // the encoder's parity register, generator 0x575
    par <<= 1;
    if (fb) par ^= 0x575u;
  }
  for (int k = 0; k < 10; k++) sent = (sent << 1) | (ubit(25 + k) & 1u);
  const unsigned tail = (ubit(35) | ubit(36) | ubit(37) | ubit(38)) & 1u;
  *ok = (tail == 0 && sent == (~par & 0x3ffu)) ? 1u : 0u;
  unsigned D = 0;                                         // LSB8MSB undone on the first three octets: bit 24 stays
  for (int q = 0; q < 25; q++) {
    const int src = q < 24 ? 8 * (q >> 3) + 7 - (q & 7) : 24;
    D |= ((dw >> (24 - src)) & 1u) << (24 - q);
  }
  *bsic = (D >> 19) & 63u;
  const int t1 = (int)((D >> 8) & 2047u), t2 = (int)((D >> 3) & 31u), t3 = 10 * (int)(D & 7u) + 1;
  *rfn = 1326 * t1 + 51 * ((((t3 - t2) % 26) + 26) % 26) + t3;
}
