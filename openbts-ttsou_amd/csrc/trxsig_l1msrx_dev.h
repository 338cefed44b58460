// trxsig_l1msrx_dev.h -- internal: what the mobile-side downlink L1 (include/trxsig_l1msrx.h) shares between its host side
// (trxsig_l1msrx.cpp) and its kernels (trxsig_l1msrx.hip), and what trxsig_l1ms reads of it (trxsig_l1ms_follow).  The mappings
// are the downlink tables of trxsig_tdma.h; positions and blocks are trxsig_l1rx's (TrxL1rxCall), over those tables.
//
// Channel order over all classes: TCH, then the control grid (XCCH, CCCH, BCCH: one decoder launch, one grid width), then the
// SCH and the FCCH channel of the combination-V slot.
#pragma once
#include "trxsig_launch.h"
#include "trxsig_tdma.h"

// what the demux kernel and the finish need of one call (by value)
struct TrxL1msrxCall {
  int fn, n_frames, n_arfcn, n_rows, soft_stride, sps, wire;
  int n_tch, n_xcch, n_ccch, n_bcch, n_ctl, n_sch, n_fcch;   // n_ctl = n_xcch + n_ccch + n_bcch; n_sch, n_fcch: 0 or 1
  int nb_tch, nb_ctl, sch_cap, fcch_cap, band, bsic;
  int32_t blk_first[TRX_N_DL_MAPS];  // per mapping: floor(first position at or after fn / 4)
  int32_t p_first[TRX_N_DL_MAPS];    // per mapping: the first position at or after fn (positions fit 32 bits: at most 24 per 26 frames)
};

// the device side of one object (pointers into its allocations)
struct TrxL1msrxDev {
  const int32_t *chinfo;             // [n_all]: arfcn | tn << 16 | map << 20
  const uint8_t *active;             // [n_tch + n_ctl]
  int32_t *rssi, *timing;            // [n_tch + n_ctl]: the last accepted burst's, as the decoder records them
  int32_t *last;                     // [n_tch + n_ctl]: the row of the last burst each channel accepted in the call, or -1
  int32_t *ord_power, *ord_ta;       // [n_xcch]: the SACCH orders, -1 on channels that are not SACCH
  int32_t *tch_index, *ctl_index;    // [n_tch][4 nb_tch], [n_ctl][4 nb_ctl]
  uint8_t *tch_b0;                   // [n_tch]
  int32_t *tch_fn, *ctl_fn;          // closing frame numbers [..][nb]
  const uint8_t *ctl_status, *ctl_frames;
  int32_t *bcch_tc;                  // [n_bcch][nb_ctl]
  float *sch_e;                      // [sch_cap][78]: the gathered coded values
  const uint8_t *sch_u;              // [sch_cap][39]: the Viterbi's bits
  int32_t *sch_fn, *sch_rfn;
  uint8_t *sch_present, *sch_ok, *sch_bsic, *sch_sync;
  int32_t *fcch_fn, *fcch_ones;
};

hipError_t trx_launch_l1msrx_demux(hipStream_t st, const TrxL1msrxCall &call, const TrxL1msrxDev &dv, const int32_t *row,
                                   const uint8_t *valid, const float *soft);
hipError_t trx_launch_l1msrx_finish(hipStream_t st, const TrxL1msrxCall &call, const TrxL1msrxDev &dv);

// what trxsig_l1ms reads of the trxsig_l1msrx it follows (trxsig_l1msrx.cpp): its plan and its SACCH orders on the device
struct trxsig_l1msrx;
struct TrxL1msrxFollow {
  trxsig_ctx *ctx;
  int n_arfcn, n_xcch, bsic, band;
  const uint8_t *comb;               // [n_arfcn * 8] (host)
  const int32_t *ord_power, *ord_ta; // XCCH-indexed device arrays
};
void trx_l1msrx_follow(const trxsig_l1msrx *rx, TrxL1msrxFollow *out);
