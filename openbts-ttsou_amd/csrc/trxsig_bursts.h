// trxsig_bursts.h -- internal: burst constants shared by the host (trxsig_transceiver.cpp, trxsig_tablegen.cpp) and the kernels
// (trxsig_l1mux_dev.h, trxsig_l1tx.hip).
#pragma once

// the dummy burst of GSM 05.02 5.2.6 (gDummyBurst, GSM/GSMCommon.cpp), one character per bit
#define TRX_DUMMY_BURST_BITS                                                                                 \
  "0001111101101110110000010100100111000001001000100000001111100011100010111000101110001010111010010100" \
  "011001100111001111010011111000100101111101010000"

// the eight training sequences of GSM 05.02 5.2.3 (gTrainingSequence, GSM/GSMCommon.cpp:44-53), one character per bit
#define TRX_TSC_BITS                                                                                  \
  { "00100101110000100010010111", "00101101110111100010110111", "01000011101110100100001110",       \
    "01000111101101000100011110", "00011010111001000001101011", "01001110101100000100111010",       \
    "10100111110110001010011111", "11101111000100101110111100" }
