// trxsig_l1ms_dev.h -- internal: what the mobile-side uplink L1 (include/trxsig_l1ms.h) shares between its host side
// (trxsig_l1ms.cpp) and its kernels (trxsig_l1ms.hip).  The mappings are the uplink tables of trxsig_tdma.h; positions, blocks
// and the per-call geometry are trxsig_l1tx's (TrxL1txCall), over those tables.
#pragma once
#include "trxsig_launch.h"
#include "trxsig_tdma.h"

// what one encode needs of its call (by value); per mapping as TrxL1txCall
struct TrxL1msCall {
  int fn, n_frames, n_arfcn, n_tch, n_xcch, n_all;
  int nb[2];                         // per class (TCH, XCCH): the most blocks any channel opens
  int n_rach;                        // RACH frames of the call (0 without a combination-V slot)
  long long unit0[2];                // per class: the first scratch unit ([n_chan][nb] after it)
  int r104, r102, r51, r26;          // fn mod 104 / 102 / 51 / 26
  int cur, has_sib, band, bsic;      // has_sib: 0 none, 1 a sibling trxsig_l1tx's orders, 2 a followed trxsig_l1msrx's
  long long p_first[TRX_N_MAPS], p_end[TRX_N_MAPS], base[TRX_N_MAPS];
};

// a channel's record in the object (two copies: the call reads copy `cur`, the commit writes copy `cur ^ 1`)
struct TrxL1msChan {
  uint32_t last_c[16];               // c[456] of the last block the channel encoded, bit i = word i/32 bit i%32
  uint32_t prev_c[16];               // ... and of the one before it (TCH: the odd half interleaves into the next block)
  uint8_t last_f, prev_f;            // their FACCH flags
  uint8_t pend;                      // the last block's last burst lies after the last call: its tail goes out next
  uint8_t active;
  int32_t power, ta;                 // the handset (SACCH channels): actual power (dBm) and TA; -1 on the others
  uint32_t pad[5];
};
static_assert(sizeof(TrxL1msChan) == 160, "TrxL1msChan layout");

struct TrxL1msDev {
  const int32_t *chinfo;             // [n_all]: arfcn | tn << 16 | map << 20
  const int32_t *slot;               // [n_arfcn * 8]: combination | the slot's TCH channel << 4
  const int32_t *slot_x;             // [n_arfcn * 8]: the slot's first XCCH channel (index over all classes)
  const int32_t *handset;            // [n_all]: the XCCH index of the SACCH channel whose handset sends this channel
  const int8_t *writer;              // [3][8][104]: the mapping that owns (combination I / V / VII, TN, fn mod 104 or 102)
  const int16_t *cnt;                // [TRX_N_MAPS][105]
  TrxL1msChan *st;                   // [2][n_all]
  uint32_t *c;                       // scratch [units][16]
  uint8_t *flag;                     // scratch [units]: 1 encoded, 2 FACCH
  const uint8_t *kind[2], *payload[2];   // TCH / XCCH grids
  const uint8_t *rach_kind, *rach_ra, *rach_bsic;
  const uint8_t *filler;             // the context's TCH filler c[456]
  int32_t *ms_power, *ms_ta;         // [n_xcch] out: the handsets after the call
  uint8_t *bits, *what;              // [n_arfcn][8 F][148], [n_arfcn][8 F]
  int32_t *who;                      // [n_arfcn][8 F]: the slot's channel within its class, or its RACH entry
  const TrxL1txChan *sib;            // the sibling's XCCH records (current copy), or null
  const int32_t *fol_power, *fol_ta; // the followed trxsig_l1msrx's decoded SACCH orders (XCCH-indexed), or null
};

// what trxsig_l1ms reads of a sibling trxsig_l1tx (trxsig_l1tx.cpp): its plan and its XCCH channels' current records
struct trxsig_l1tx;
struct TrxL1txSib {
  trxsig_ctx *ctx;
  int n_arfcn, n_xcch;
  const uint8_t *comb;               // [n_arfcn * 8] (host)
  const TrxL1txChan *xcch;           // [n_xcch] device: the records the next call of the sibling reads
};
void trx_l1tx_sibling(const trxsig_l1tx *l1, TrxL1txSib *out);

// one radiate (by value)
struct TrxL1msAir {
  const trx_c32 *gain[3];            // TCH, XCCH, RACH
  const float *delay[3];
  const float *amp_of_power;         // [41]
  const uint8_t *bits, *what;
  const int32_t *who, *handset, *ms_power, *ms_ta;
  trx_c32 *out;
  long long slot_stride, arfcn_stride;
  int n_arfcn, n_tch;
  long long rows;                    // 8 * n_frames
};

hipError_t trx_launch_l1ms_encode(hipStream_t st, const TrxL1msCall &call, const TrxL1msDev &dv);
hipError_t trx_launch_l1ms_mux(hipStream_t st, const TrxL1msCall &call, const TrxL1msDev &dv);
// open (1) / close (0) of a channel's record; phy != 0: power / ta are set too (open of a SACCH channel, set_phy)
hipError_t trx_launch_l1ms_set(hipStream_t st, TrxL1msChan *rec, int active /* -1: keep */, int phy, int power, int ta);
hipError_t trx_launch_l1ms_radiate(hipStream_t st, int sps, const TrxTables *dT, const TrxL1msAir &air);
