// trxsig_bursts.h -- internal: burst constants shared by the host (trxsig_transceiver.cpp) and the kernels (trxsig_l1tx.hip).
#pragma once

// the dummy burst of GSM 05.02 5.2.6 (gDummyBurst, GSM/GSMCommon.cpp), one character per bit
#define TRX_DUMMY_BURST_BITS                                                                                 \
  "0001111101101110110000010100100111000001001000100000001111100011100010111000101110001010111010010100" \
  "011001100111001111010011111000100101111101010000"
