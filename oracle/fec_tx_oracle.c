/*
 * oracle/fec_tx_oracle.c -- TEST INFRASTRUCTURE ONLY (see oracle/README.md).
 *
 * CPU restatement (plain C99) of the GSM downlink L1 encoders of traffic and sync channels:
 * TCHFACCHL1Encoder::dispatch / encodeTCH / interleave (GSM/GSML1FEC.cpp:1213-1224, 1252-1393, "fec:<line>")
 * restated LITERALLY -- eight interleaver rows mI[], the alternating mOffset, mPreviousFACCH, block by block -- so
 * that the device's closed form is checked against it rather than restated by it; and SCHL1Encoder::generate
 * (fec:879-920) with the frame-number fields of GSM/GSMCommon.h:465-474.  The coder, the parity registers and
 * LSB8MSB are those of oracle/fec_oracle.c (linked into the same library by oracle/fec_tx.mk).
 *
 * Parity status: PINNED -- checked bit for bit against the real reference compiled in place
 * (oracle/_ref/libref_fec_tx.so, tests/test_fec_tx_oracle.py, replayed from tests/golden/ref_calls/ elsewhere) and
 * against the golden streams captured from it (tests/golden/fec_tx.npz).
 */
#include "fec_tx_oracle.h"

#include <omp.h>
#include <string.h>

#include "fec_oracle.h"

/* XCCHL1Encoder::encode of an L2 frame (fec:789, 796-808): 23 octets -> c[456] */
static void xcch_c(const uint8_t *frame23, uint8_t *c) {
  uint8_t u[228];
  memset(u, 0, sizeof u);
  for (int i = 0; i < 184; i++) u[i] = (frame23[i / 8] >> (7 - i % 8)) & 1u;   /* the L2 frame, MSB first */
  fo_lsb8msb(u, 184);                                                           /* fec:1320 */
  const uint64_t pw = ~fo_parity(0x10004820009ULL, 40, u, 184);                 /* writeParityWord, inverted (bv:409-416) */
  for (int k = 0; k < 40; k++) u[184 + k] = (uint8_t)((pw >> (39 - k)) & 1u);
  fo_encode(u, 228, c);
}

/* TCHFACCHL1Encoder::encodeTCH (fec:1252-1284): d[260] in GSM 05.03 order -> c[456] */
static void tch_c(const uint8_t *d, uint8_t *c) {
  uint8_t u[189];
  const unsigned pw = ~(unsigned)fo_parity(0x0b, 3, d, 50);                    /* writeParityWord into u[91..93] */
  for (int t = 0; t < 3; t++) u[91 + t] = (uint8_t)((pw >> (2 - t)) & 1u);
  for (int k = 0; k <= 90; k++) { u[k] = d[2 * k]; u[184 - k] = d[2 * k + 1]; }
  for (int k = 185; k <= 188; k++) u[k] = 0;
  fo_encode(u, 189, c);                                                        /* class 1: c[0..378) */
  for (int i = 0; i < 78; i++) c[378 + i] = d[182 + i];                        /* class 2 copied */
}

/* TCHFACCHL1Encoder::dispatch (fec:1297-1382) and interleave (fec:1384-1393), literally: eight interleaver rows mI[],
   the alternating mOffset and mPreviousFACCH, block by block.  Channel s: n_blocks blocks of kind[s][m] (0 filler,
   1 speech: payload = d[260] packed MSB first, 2 FACCH: payload[0..23) = the L2 frame, else an all-zero c[] that is not
   stolen) -> bits[s][m][4][148].  state[s][32] in / out: bytes 0..28 = the odd half of the last block's c[] (c[k],
   k mod 8 >= 4, bit i at byte i/8, weight 1 << i%8), byte 29 = mPreviousFACCH; zero = a freshly constructed encoder.
   A channel whose tsc is above 7 gets zero bursts and keeps its state. */
void fo_tch_encode_stream(int n_chan, int n_blocks, const uint8_t *kind, const uint8_t *payload, const uint8_t *tsc,
                          const uint8_t *tsc_bits8x26, const uint8_t *filler456, uint8_t *state, uint8_t *bits, int nthreads) {
#pragma omp parallel for num_threads(nthreads) schedule(dynamic)
  for (int s = 0; s < n_chan; s++) {
    uint8_t *out = bits + (size_t)s * n_blocks * 592;
    uint8_t *st = state + (size_t)s * 32;
    if (tsc[s] > 7) { memset(out, 0, (size_t)n_blocks * 592); continue; }
    uint8_t mI[8][114];
    memset(mI, 0, sizeof mI);
    int mOffset = 0;
    /* the state as the rows the next block (offset 0) reads its odd positions from: the last block ran at offset 4 */
    for (int k = 0; k < 456; k++) {
      if (k % 8 < 4) continue;
      const int i = 4 * (k / 8) + (k % 8) - 4, j = 2 * ((49 * k) % 57) + ((k % 8) / 4);
      mI[(k + 4) % 8][j] = (st[i / 8] >> (i % 8)) & 1u;
    }
    int mPreviousFACCH = st[29] & 1u;
    for (int m = 0; m < n_blocks; m++) {
      const size_t blk = (size_t)s * n_blocks + m;
      const uint8_t *pl = payload + blk * 33;
      uint8_t c[456];
      int currentFACCH = 0;
      if (kind[blk] == 2) {
        currentFACCH = 1;
        xcch_c(pl, c);
      } else if (kind[blk] == 1) {
        uint8_t d[260];
        for (int q = 0; q < 260; q++) d[q] = (pl[q / 8] >> (7 - q % 8)) & 1u;
        tch_c(d, c);
      } else if (kind[blk] == 0) {
        for (int k = 0; k < 456; k++) c[k] = filler456[k] & 1u;
      } else {
        memset(c, 0, sizeof c);
      }
      for (int k = 0; k < 456; k++) {                                          /* interleave(mOffset) */
        const int B = (k + mOffset) % 8, j = 2 * ((49 * k) % 57) + ((k % 8) / 4);
        mI[B][j] = c[k];
      }
      for (int B = 0; B < 4; B++) {
        uint8_t *b = out + ((size_t)m * 4 + B) * 148;
        memset(b, 0, 148);
        memcpy(b + 3, mI[B + mOffset], 57);
        memcpy(b + 88, mI[B + mOffset] + 57, 57);
        for (int k = 0; k < 26; k++) b[61 + k] = tsc_bits8x26[26 * tsc[s] + k] & 1u;
        b[87] = (uint8_t)currentFACCH;                                           /* Hu */
        b[60] = (uint8_t)mPreviousFACCH;                                         /* Hl */
      }
      mOffset = mOffset == 0 ? 4 : 0;
      mPreviousFACCH = currentFACCH;
    }
    if (n_blocks > 0) {
      const int last = mOffset == 0 ? 4 : 0;                                    /* the offset the last block ran at */
      memset(st, 0, 32);
      for (int k = 0; k < 456; k++) {
        if (k % 8 < 4) continue;
        const int i = 4 * (k / 8) + (k % 8) - 4, j = 2 * ((49 * k) % 57) + ((k % 8) / 4);
        st[i / 8] |= (uint8_t)(mI[(k + last) % 8][j] << (i % 8));
      }
      st[29] = (uint8_t)mPreviousFACCH;
    }
  }
}

/* SCHL1Encoder::generate (fec:879-920): (FN, BSIC) -> one 148-bit burst.  T1 / T2 / T3' as GSMCommon.h:465-474, unsigned.
   An FN outside the hyperframe or a BSIC above 63: zero burst. */
void fo_sch_encode(const uint32_t *fn, const uint8_t *bsic, int n, const uint8_t *xts64, uint8_t *bits) {
  for (int i = 0; i < n; i++) {
    uint8_t *b = bits + (size_t)i * 148;
    memset(b, 0, 148);
    if (fn[i] >= 2715648u || bsic[i] > 63) continue;
    const unsigned f = fn[i];
    const unsigned T1 = (f / (26u * 51u)) % 2048u, T2 = f % 26u, T3 = f % 51u, T3p = (T3 - 1u) / 10u;
    uint8_t u[39], e[78];
    int wp = 0;
    const unsigned vals[4] = { bsic[i], T1, T2, T3p }, lens[4] = { 6, 11, 5, 3 };
    for (int fld = 0; fld < 4; fld++)                                          /* writeField: low bits, MSB first */
      for (unsigned q = 0; q < lens[fld]; q++) u[wp++] = (uint8_t)((vals[fld] >> (lens[fld] - 1 - q)) & 1u);
    fo_lsb8msb(u, 25);
    const unsigned pw = ~(unsigned)fo_parity(0x0575, 10, u, 25);
    for (int k = 0; k < 10; k++) u[25 + k] = (uint8_t)((pw >> (9 - k)) & 1u);
    for (int k = 35; k < 39; k++) u[k] = 0;
    fo_encode(u, 39, e);
    memcpy(b + 3, e, 39);
    for (int k = 0; k < 64; k++) b[42 + k] = xts64[k] & 1u;
    memcpy(b + 106, e + 39, 39);
  }
}
