/* trxsig_l1msrx.h -- the mobile side of the downlink L1: received downlink bursts to the logical channels' payloads, the cell's
 * frame number and BSIC, and the handsets' SACCH orders, on the device.  The fourth sibling of trxsig_l1rx.h / trxsig_l1tx.h /
 * trxsig_l1ms.h: what the handsets of a cell do with what trxsig_l1tx emits -- the XCCH and TCH/FACCH decoders of
 * GSM/GSML1FEC.cpp (the same stream decoders trxsig_l1rx feeds) walking the DOWNLINK TDMAMappings of GSM/GSMTDMA.cpp, the
 * SACCH L1 header read back as SACCHL1Decoder::handleGoodFrame reads the uplink's, and a decoder for the SCH burst.
 *
 * THE SCH DECODER HAS NO REFERENCE COUNTERPART.  The reference is a base station: it only encodes SCH (SCHL1Encoder::generate).
 * The decoder here is the inverse of trxsig_fec_sch_encode_batch as trxsig.h states that encoder, built from the reference's
 * generic SoftVector::decode; it is pinned by this project's own model (tests/l1_msrx_model.py), not by the reference.
 *
 * Acquisition -- finding the FCCH and SCH bursts in raw samples, the frequency offset, the frame grid, the frame number and the
 * BSIC -- is trxsig_l1acq.h; the normal-burst detector of a group pull does not find those bursts, so a caller that wants their
 * slots decoded here supplies the rows (trxsig_l1acq_detect_sch_batch produces SCH rows).  Combination IV is not supported.
 * The group's detectors and tables are used as they are.
 *
 * Plan and channels.  h_comb, bsic and band mean what they mean for trxsig_l1rx_create: h_comb[a][tn] in 0 / 1 (I) / 5 (V, on
 * ARFCN 0 TN 0 only) / 7 (VII); anything else is TRXSIG_EINVAL.  Classes: TRXSIG_L1_TCH and TRXSIG_L1_XCCH numbered exactly as
 * trxsig_l1rx numbers them, TRXSIG_L1_CCCH as trxsig_l1tx numbers it (CCCH_0..2 of the combination-V slot), and TRXSIG_L1_BCCH,
 * TRXSIG_L1_SCH, TRXSIG_L1_FCCH: one channel each on the combination-V slot.  Class 2 (the uplink's RACH) is TRXSIG_EINVAL.
 * The mappings are the downlink tables trxsig_l1tx walks (FACCH_TCHF, SACCH_TF_Tn, SDCCH_x_yD, SACCH_Cx_yD, CCCH_0..2, BCCH,
 * SCH, FCCH); positions are numbered as in trxsig_l1rx.
 *
 * Input: a trxsig_trxgroup_result of whole frames [fn, fn + n_slots / 8) from TN 0, read exactly as trxsig_l1rx_decode reads
 * one (d_row, d_valid, d_soft, soft_stride, n_rows, d_amp, d_toa, n_slots, n_arfcn; a slot counts where its row is in range
 * and d_valid is set).  It may come from a pull of downlink samples, from rows the caller produced, or from bits turned into
 * soft values.  wire_quantise applies to every class, as in the stream decoders.
 *
 * TCH, XCCH, CCCH, BCCH: trxsig_l1rx's rules.  Block b of a channel is its b-th block overlapping the call; a straddling block
 * shows in both calls and is decoded only in the call of its closing burst; one call of F frames equals calls that split F at
 * any frame boundaries, in every output and in the state bytes; a closed channel ignores its bursts.  CCCH and BCCH use the
 * XCCH decoder and its state layout.  XCCH, CCCH and BCCH share one decoder launch and one grid width nb_ctl: the most blocks
 * any channel of the three classes has in the call.  A dummy burst (the downlink's idle fill) is a burst like any other: its
 * block decodes and fails parity.
 * SACCH orders, per XCCH channel (-1 on channels that are not SACCH): after every good SACCH frame of the call ord_power =
 * POWER[band][frame[0] & 31] and, if frame[1] & 127 is below 64, ord_ta = that -- the header trxsig_l1tx writes, read as
 * SACCHL1Decoder::handleGoodFrame reads the uplink's.  A new object, and open of a SACCH channel, set power 40 and TA 0.
 * SCH: one entry per SCH frame of the call, in FN order.  e[0..39) = soft values 3..41, e[39..78) = 106..144;
 * SoftVector::decode gives u[39]; ok = the four tail bits are zero and u[25..35) is the inverted parity (generator 0x575) of
 * u[0..25); LSB8MSB is undone on the first three octets; BSIC (6) T1 (11) T2 (5) T3' (3) are read MSB first; rfn = 1326 T1 +
 * 51 ((T3 - T2) mod 26) + T3 with T3 = 10 T3' + 1; sync = ok && rfn == the slot's FN && BSIC == the cell's.  Entries where no
 * burst arrived are zero except d_sch_fn.
 * FCCH: one entry per FCCH frame of the call, in FN order: the count of the slot's 148 soft values strictly above 0.5 (after
 * the wire hop if asked; a clean frequency-correction burst gives 0), -1 where no burst arrived.
 * Thread safety: one caller at a time per object.
 */
#ifndef TRXSIG_L1MSRX_H
#define TRXSIG_L1MSRX_H

#include "trxsig_l1tx.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct trxsig_l1msrx trxsig_l1msrx;

/* the new classes; TRXSIG_L1_TCH / _XCCH as in trxsig_l1rx.h, TRXSIG_L1_CCCH as in trxsig_l1tx.h */
enum { TRXSIG_L1_BCCH = 4, TRXSIG_L1_SCH = 5, TRXSIG_L1_FCCH = 6 };
/* their mapping kinds (trxsig_l1msrx_channel); kinds 0..7 as in trxsig_l1rx.h / trxsig_l1tx.h */
enum { TRXSIG_L1_BCCH_C5 = 8, TRXSIG_L1_SCH_C5 = 9, TRXSIG_L1_FCCH_C5 = 10 };

/* The object keeps ctx alive: trxsig_destroy on ctx takes effect when the object is gone too. */
int trxsig_l1msrx_create(trxsig_l1msrx **out, trxsig_ctx *ctx, int n_arfcn, const uint8_t *h_comb, int bsic, int band);
void trxsig_l1msrx_destroy(trxsig_l1msrx *rx);
/* number of channels of a class (negative: bad argument) */
int trxsig_l1msrx_channels(const trxsig_l1msrx *rx, int cls);
int trxsig_l1msrx_channel(const trxsig_l1msrx *rx, int cls, int chan, int *arfcn, int *tn, int *kind, int *sub);
/* open / close of one TCH, XCCH, CCCH or BCCH channel, in stream order on the context's stream, as trxsig_l1rx_open / _close
 * (open: FER 0, mI kept; a SACCH channel: orders 40 / 0).  SCH and FCCH have no active flag: TRXSIG_EINVAL. */
int trxsig_l1msrx_open(trxsig_l1msrx *rx, int cls, int chan);
int trxsig_l1msrx_close(trxsig_l1msrx *rx, int cls, int chan);

/* What one decode leaves, device resident, owned by the object, valid until its next decode. */
typedef struct {
  int n_tch, n_xcch, n_ccch, n_bcch, nb_tch, nb_ctl, sch_cap, fcch_cap;
  /* TCH [n_tch][nb_tch], as trxsig_l1rx_out */
  const uint8_t *d_tch_status, *d_tch_frames, *d_facch;
  const float *d_tch_fer;
  const int32_t *d_tch_fn;
  /* XCCH [n_xcch][nb_ctl], CCCH [n_ccch][nb_ctl], BCCH [n_bcch][nb_ctl]: status / frames (23) / FER / closing FN as
   * trxsig_l1rx_out's XCCH; d_bcch_tc = (FN / 51) % 8 of the block's first burst */
  const uint8_t *d_xcch_status, *d_xcch_frames;
  const float *d_xcch_fer;
  const int32_t *d_xcch_fn;
  const uint8_t *d_ccch_status, *d_ccch_frames;
  const float *d_ccch_fer;
  const int32_t *d_ccch_fn;
  const uint8_t *d_bcch_status, *d_bcch_frames;
  const float *d_bcch_fer;
  const int32_t *d_bcch_fn, *d_bcch_tc;
  /* SCH [sch_cap]: the slot's FN (modulo the hyperframe), burst present, ok, BSIC, the decoded frame number, sync */
  const int32_t *d_sch_fn, *d_sch_rfn;
  const uint8_t *d_sch_present, *d_sch_ok, *d_sch_bsic, *d_sch_sync;
  /* FCCH [fcch_cap]: the slot's FN, the soft values above 0.5 (-1: no burst) */
  const int32_t *d_fcch_fn, *d_fcch_ones;
  /* per channel, after the call: RSSI / timing of the last burst the channel accepted, as trxsig_l1rx_out's */
  const int32_t *d_tch_rssi, *d_tch_timing, *d_xcch_rssi, *d_xcch_timing, *d_ccch_rssi, *d_ccch_timing, *d_bcch_rssi,
      *d_bcch_timing;
  /* [n_xcch]: the SACCH orders after the call (dBm, symbols), -1 on channels that are not SACCH */
  const int32_t *d_ord_power, *d_ord_ta;
} trxsig_l1msrx_out;

/* Decode whole frames that start at (fn, TN 0): res->n_slots a multiple of 8, res->n_arfcn the object's, fn in [0, 2715648).
 * Everything is enqueued on the context's stream (k_l1msrx_demux, k_l1rx_demux_phy, the TCH and XCCH stream decoders, the SCH
 * Viterbi, k_l1msrx_finish); nothing synchronises and nothing is copied to the host.  NULL pointers, n_slots not a multiple of 8,
 * another n_arfcn or a bad fn return TRXSIG_EINVAL before any launch. */
int trxsig_l1msrx_decode(trxsig_l1msrx *rx, const trxsig_trxgroup_result *res, int fn, int wire_quantise, trxsig_l1msrx_out *out);

/* the channels' decoder records of TCH / XCCH / CCCH / BCCH, [n_chan][TRXSIG_TCH_RX_STATE_BYTES] (TCH) or
 * [n_chan][TRXSIG_XCCH_RX_STATE_BYTES] (the others), device arrays in the stream decoders' layouts */
int trxsig_l1msrx_state(trxsig_l1msrx *rx, int cls, void **d_state);

#ifdef __cplusplus
}
#endif
#endif /* TRXSIG_L1MSRX_H */
