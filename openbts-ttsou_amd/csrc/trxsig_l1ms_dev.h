// trxsig_l1ms_dev.h -- internal: what the mobile-side uplink L1 (include/trxsig_l1ms.h) shares between its host side
// (trxsig_l1ms.cpp) and its kernels (trxsig_l1ms.hip).  The mappings are the uplink tables of trxsig_tdma.h; the call, record and
// device structs are that file's TrxMuxCall / TrxMuxChan / TrxMuxDev with the uplink's own fields after them.
#pragma once
#include "trxsig_launch.h"
#include "trxsig_tdma.h"

struct TrxL1msCall : TrxMuxCall {    // has_sib: 0 none, 1 a sibling trxsig_l1tx's orders, 2 a followed trxsig_l1msrx's
  int n_rach;                        // RACH frames of the call (0 without a combination-V slot)
};

struct TrxL1msChan {
  TrxMuxChan h;
  int32_t power, ta;                 // the handset (SACCH channels): actual power (dBm) and TA; -1 on the others
  uint32_t pad[5];
};
// trxsig_l1ms_state hands these bytes to callers
static_assert(sizeof(TrxL1msChan) == 160, "TrxL1msChan layout");
static_assert(offsetof(TrxL1msChan, h.last_c) == 0 && offsetof(TrxL1msChan, h.prev_c) == 64 && offsetof(TrxL1msChan, h.last_f) == 128 &&
              offsetof(TrxL1msChan, h.prev_f) == 129 && offsetof(TrxL1msChan, h.pend) == 130 && offsetof(TrxL1msChan, h.active) == 131 &&
              offsetof(TrxL1msChan, power) == 132 && offsetof(TrxL1msChan, ta) == 136 && offsetof(TrxL1msChan, pad) == 140,
              "TrxL1msChan layout");

struct TrxL1msDev : TrxMuxDev<TrxL1msChan> {
  const int32_t *handset;            // [n_all]: the XCCH index of the SACCH channel whose handset sends this channel
  const uint8_t *rach_kind, *rach_ra, *rach_bsic;
  int32_t *ms_power, *ms_ta;         // [n_xcch] out: the handsets after the call
  int32_t *who;                      // [n_arfcn][8 F]: the slot's channel within its class, or its RACH entry
  const TrxL1txChan *sib;            // the sibling's XCCH records (current copy), or null
  const int32_t *fol_power, *fol_ta; // the followed trxsig_l1msrx's decoded SACCH orders (XCCH-indexed), or null
};

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
