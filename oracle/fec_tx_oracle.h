/*
 * oracle/fec_tx_oracle.h -- TEST INFRASTRUCTURE ONLY: CPU restatement of the downlink L1 encoders of traffic and sync
 * channels (TCH/FS + FACCH/F stream, SCH).  See fec_tx_oracle.c for the references.  Only tests/ and
 * tools/fec_tx_bench.py's cpu_baseline leg may load it.
 */
#ifndef FEC_TX_ORACLE_H
#define FEC_TX_ORACLE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

void fo_tch_encode_stream(int n_chan, int n_blocks, const uint8_t *kind, const uint8_t *payload, const uint8_t *tsc,
                          const uint8_t *tsc_bits8x26, const uint8_t *filler456, uint8_t *state, uint8_t *bits, int nthreads);
void fo_sch_encode(const uint32_t *fn, const uint8_t *bsic, int n, const uint8_t *xts64, uint8_t *bits);

#ifdef __cplusplus
}
#endif
#endif
