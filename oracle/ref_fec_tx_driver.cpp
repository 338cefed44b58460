// oracle/ref_fec_tx_driver.cpp -- TEST INFRASTRUCTURE ONLY.
//
// extern "C" entry points around the UNMODIFIED reference CommonLibs/BitVector.{h,cpp} and GSM::Time
// (GSM/GSMCommon.h, whose T1 / T2 / T3p are inline), compiled in place from /root/reference by
// `make -C oracle -f fec_tx.mk ref`, never copied.  The downlink L1 encoders TCHFACCHL1Encoder::dispatch and
// SCHL1Encoder::generate (GSM/GSML1FEC.cpp) sit inside the GSM stack's threaded channel objects and cannot be built
// alone, so they are re-enacted here call by call on the reference's own primitives, in the reference's order, with
// their member state (mI[8], mOffset, mPreviousFACCH, mBurst) as locals.  The filler c[] and the SCH extended training
// sequence come in as data.  Used to pin oracle/fec_tx_oracle.c and to generate tests/golden/fec_tx.npz.
#include <stdint.h>
#include <string.h>

#include "BitVector.h"
#include "GSMCommon.h"

extern "C" {

// TCHFACCHL1Encoder (GSML1FEC.cpp:1213-1224) constructed fresh, then dispatch (:1297-1382) n_blocks times: block m
// carries kind[m] (2 = an L2 frame in payload[m][0..23), octets MSB first, 1 = a speech d[260] in GSM 05.03 order,
// payload[m][0..33) MSB first, 0 = filler; the caller has made the queue decision).  tsc26: the channel's training
// sequence, filler456: the filler c[] (data, :1348).  -> bits[m][4][148] as the encoder hands them to mDownstream.
void reffec_tch_dispatch(int n_blocks, const unsigned char *kind, const unsigned char *payload, const unsigned char *tsc26,
                         const unsigned char *filler456, unsigned char *bits) {
  // XCCHL1Encoder part of the object (:700-727)
  Parity mBlockCoder(0x10004820009ULL, 40, 224);
  ViterbiR2O4 mVCoder;
  BitVector mC(456), mU(228);
  BitVector mD(mU.head(184)), mP(mU.segment(184, 40));
  mU.zero();
  BitVector mBurst(148);                                   // TxBurst: zero tails, training sequence at 61
  mBurst.zero();
  for (int k = 0; k < 26; k++) mBurst[61 + k] = tsc26[k] & 0x01;
  // TCHFACCHL1Encoder part (:1213-1224)
  bool mPreviousFACCH = false;
  int mOffset = 0;
  BitVector mTCHU(189), mTCHD(260);
  BitVector mClass1_c(mC.head(378)), mClass1A_d(mTCHD.head(50)), mClass2_d(mTCHD.segment(182, 78));
  Parity mTCHParity(0x0b, 3, 50);
  BitVector mI[8];
  for (int k = 0; k < 8; k++) { mI[k] = BitVector(114); mI[k].fill(0); }
  BitVector fillerC(456);
  for (int i = 0; i < 456; i++) fillerC[i] = filler456[i] & 0x01;

  for (int m = 0; m < n_blocks; m++) {
    const unsigned char *pl = payload + (size_t)m * 33;
    bool currentFACCH = false;
    if (kind[m] == 2) {
      currentFACCH = true;
      BitVector fFrame(184);                               // the L2Frame
      for (int i = 0; i < 184; i++) fFrame[i] = (pl[i / 8] >> (7 - i % 8)) & 0x01;
      fFrame.LSB8MSB();
      fFrame.copyTo(mU);
      mBlockCoder.writeParityWord(mD, mP);                 // encode() (:796-808)
      mU.encode(mVCoder, mC);
    } else if (kind[m] == 1) {
      for (int i = 0; i < 260; i++) mTCHD[i] = (pl[i / 8] >> (7 - i % 8)) & 0x01;   // encodeTCH (:1252-1284)
      BitVector p = mTCHU.segment(91, 3);
      mTCHParity.writeParityWord(mClass1A_d, p);
      for (unsigned k = 0; k <= 90; k++) {
        mTCHU[k] = mTCHD[2 * k];
        mTCHU[184 - k] = mTCHD[2 * k + 1];
      }
      for (unsigned k = 185; k <= 188; k++) mTCHU[k] = 0;
      mTCHU.encode(mVCoder, mClass1_c);
      mClass2_d.copyToSegment(mC, 378);
    } else {
      fillerC.copyTo(mC);
    }
    for (int k = 0; k < 456; k++) {                        // interleave(mOffset) (:1384-1393)
      int B = (k + mOffset) % 8;
      int j = 2 * ((49 * k) % 57) + ((k % 8) / 4);
      mI[B][j] = mC[k];
    }
    for (int B = 0; B < 4; B++) {
      mI[B + mOffset].segment(0, 57).copyToSegment(mBurst, 3);
      mI[B + mOffset].segment(57, 57).copyToSegment(mBurst, 88);
      mBurst[87] = currentFACCH;                           // Hu / Hl (GSMTransfer.h:47-48)
      mBurst[60] = mPreviousFACCH;
      for (int i = 0; i < 148; i++) bits[((size_t)m * 4 + B) * 148 + i] = mBurst[i] & 0x01;
    }
    if (mOffset == 0) mOffset = 4;
    else mOffset = 0;
    mPreviousFACCH = currentFACCH;
  }
}

// SCHL1Encoder (GSML1FEC.cpp:879-893) and generate (:897-920) for each (fn[i], bsic[i]): xts64 = the extended
// training sequence of the constructor (data) -> bits[i][148]
void reffec_sch_encode(const uint32_t *fn, const unsigned char *bsic, int n, const unsigned char *xts64, unsigned char *bits) {
  Parity mBlockCoder(0x0575, 10, 25);
  ViterbiR2O4 mVCoder;
  BitVector mU(25 + 10 + 4), mE(78);
  BitVector mD(mU.head(25)), mP(mU.segment(25, 10));
  BitVector mE1(mE.segment(0, 39)), mE2(mE.segment(39, 39));
  BitVector mBurst(148);
  mBurst.zero();
  for (int k = 0; k < 64; k++) mBurst[42 + k] = xts64[k] & 0x01;
  mU.fillField(35, 0, 4);
  for (int i = 0; i < n; i++) {
    GSM::Time t((int)fn[i]);
    size_t wp = 0;
    mD.writeField(wp, bsic[i], 6);
    mD.writeField(wp, t.T1(), 11);
    mD.writeField(wp, t.T2(), 5);
    mD.writeField(wp, t.T3p(), 3);
    mD.LSB8MSB();
    mBlockCoder.writeParityWord(mD, mP);
    mU.encode(mVCoder, mE);
    mE1.copyToSegment(mBurst, 3);
    mE2.copyToSegment(mBurst, 106);
    for (int k = 0; k < 148; k++) bits[(size_t)i * 148 + k] = mBurst[k] & 0x01;
  }
}

}  // extern "C"
