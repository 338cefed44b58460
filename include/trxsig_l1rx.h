/* trxsig_l1rx.h -- the uplink L1 demultiplexer: a Transceiver group pull (trxsig_trxgroup.h) to the logical channels' decoders,
 * on the device.  What TRXManager's ARFCNManager does behind the reference's UDP data socket -- installDecoder's
 * mDemuxTable[TN][FN % 5304] built from the GSM 05.02 uplink mappings (GSM/GSMTDMA.cpp), receiveBurst's routing, the wire
 * parse of RSSI / timing (TRXManager/TRXManager.cpp:146-168, 215-233, 474-490) -- and the decoders it feeds:
 * TCHFACCHL1Decoder, XCCHL1Decoder / SACCHL1Decoder and RACHL1Decoder (GSM/GSML1FEC.cpp).
 *
 * Channel plan, fixed at create: h_comb[a][tn] in the CMD SETSLOT numbering -- 0 none, 1 = combination I (TCH/F + FACCH/F +
 * SACCH/TF), 5 = combination V (SDCCH/4 + SACCH/C4 + RACH; legal on TN 0 of ARFCN 0 only), 7 = combination VII (SDCCH/8 +
 * SACCH/C8).  Anything else (combination IV included: the reference leaves its RACH map as a TODO) is TRXSIG_EINVAL.
 *
 * Channel numbering, per class, in (ARFCN, TN, sub-channel) order:
 *   TRXSIG_L1_TCH   one TCH/F (FACCH_TCHF) per combination-I slot.
 *   TRXSIG_L1_XCCH  per slot: VII -> SDCCH/8 0..7 then SACCH/C8 0..7 (16 channels); V -> SDCCH/4 0..3 then SACCH/C4 0..3 (8);
 *                   I -> SACCH/TF of the slot's TN (1).
 *   TRXSIG_L1_RACH  the combination-V slot's RACH (RACHC5), if there is one.
 * trxsig_l1rx_channel tells a channel's (ARFCN, TN, mapping kind, sub-channel).
 *
 * State on the device, per channel: the stream decoders' records (TRXSIG_TCH_RX_STATE_BYTES / TRXSIG_XCCH_RX_STATE_BYTES,
 * trxsig.h), an active flag, the RSSI / timing error of the last burst the decoder accepted, and on SACCH channels the
 * handset's actual power / timing advance.  A new object is every decoder freshly constructed and opened: FER 0, mI all 0.0,
 * RSSI / timing 0, SACCH power 40 dBm / TA 0.
 * Thread safety: one caller at a time per object.
 */
#ifndef TRXSIG_L1RX_H
#define TRXSIG_L1RX_H

#include "trxsig_trxgroup.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct trxsig_l1rx trxsig_l1rx;

enum { TRXSIG_L1_TCH = 0, TRXSIG_L1_XCCH = 1, TRXSIG_L1_RACH = 2 };
/* mapping kinds of trxsig_l1rx_channel */
enum { TRXSIG_L1_TCHF = 0, TRXSIG_L1_SACCH_TF = 1, TRXSIG_L1_SDCCH8 = 2, TRXSIG_L1_SACCH_C8 = 3, TRXSIG_L1_SDCCH4 = 4,
       TRXSIG_L1_SACCH_C4 = 5, TRXSIG_L1_RACH_C5 = 6 };

/* bsic: the cell's BSIC (0..63), which an access burst's parity must encode; band: 850, 900 (GSM 05.05 low band), 1800 or 1900,
 * the power table SACCH headers are read with.  The object keeps ctx alive: trxsig_destroy on ctx takes effect when the object
 * is gone too. */
int trxsig_l1rx_create(trxsig_l1rx **out, trxsig_ctx *ctx, int n_arfcn, const uint8_t *h_comb, int bsic, int band);
void trxsig_l1rx_destroy(trxsig_l1rx *l1);
/* number of channels of a class (negative: bad argument) */
int trxsig_l1rx_channels(const trxsig_l1rx *l1, int cls);
int trxsig_l1rx_channel(const trxsig_l1rx *l1, int cls, int chan, int *arfcn, int *tn, int *kind, int *sub);

/* L1Decoder::open / close (GSM/GSML1FEC.cpp:333-354) of one TCH or XCCH channel, in stream order on the context's stream:
 * open sets the FER to 0 (mI kept, as trxsig.h's state bytes 0..3) and, on a SACCH channel, power 40 / TA 0
 * (SACCHL1Decoder::open); a closed channel ignores its bursts -- nothing is recorded, its blocks come back undecoded.  The RACH
 * decoder has no active test (RACHL1Decoder::writeLowSide): open / close of TRXSIG_L1_RACH is TRXSIG_EINVAL. */
int trxsig_l1rx_open(trxsig_l1rx *l1, int cls, int chan);
int trxsig_l1rx_close(trxsig_l1rx *l1, int cls, int chan);

/* What one decode leaves, device resident, owned by the object, valid until its next decode.  Blocks: per class the grid is
 * [n_chan][n_blocks]; block b of a channel is the b-th block (4 bursts, B = 0..3, or 4..7 on TCH) of its mapping that overlaps
 * the call's frames, counted from the first one.  n_blocks is the most any channel of the class has; a channel with fewer gets
 * trailing blocks no burst falls in.  A block that straddles two calls shows in both: its bursts enter mI in the call they
 * arrive in (the rest of the block is "no burst" there), and it is decoded -- only -- in the call of its closing burst.  So
 * one call of F frames gives, block for block by closing FN, what calls that split F at frame boundaries give. */
typedef struct {
  int n_tch, n_xcch, nb_tch, nb_xcch, rach_cap;
  /* TCH [n_tch][nb_tch]: trxsig_fec_tch_decode_stream's d_status / d_tch (33) / d_facch (23) / d_fer, and the block's closing
   * frame number (the FN of its B = 3 or B = 7 burst, modulo the hyperframe) */
  const uint8_t *d_tch_status, *d_tch_frames, *d_facch;
  const float *d_tch_fer;
  const int32_t *d_tch_fn;
  /* XCCH [n_xcch][nb_xcch]: trxsig_fec_xcch_decode_stream's d_status / d_frames (23) / d_fer, closing FN */
  const uint8_t *d_xcch_status, *d_xcch_frames;
  const float *d_xcch_fer;
  const int32_t *d_xcch_fn;
  /* RACH: the detected bursts on RACH frames, in (FN, ARFCN) order, *d_rach_count of them (a device word; at most rach_cap,
   * the number of RACH frames in the call).  ok = tail bits zero && the parity's BSIC is the cell's (RACHL1Decoder::
   * writeLowSide); ra = the 8-bit RA where ok, else 0; fn / arfcn / rssi / timing of the burst (rules below).  Entries from
   * *d_rach_count on are unspecified. */
  const int32_t *d_rach_count, *d_rach_fn, *d_rach_arfcn, *d_rach_rssi, *d_rach_timing;
  const uint8_t *d_rach_ok, *d_rach_ra;
  /* per channel, after the call: [n_tch] / [n_xcch] the RSSI and timing error of the last burst the channel accepted
   * (processBurst's mRSSI / mTimingError; unchanged where none): RSSI = -(signed char)(the pull's RSSI), timing = (the pull's
   * timing as int16) / 256 truncated toward zero -- the UDP datagram (Transceiver.cpp:660-667) read back by TRXManager.cpp:
   * 220-233.  [n_xcch] SACCH power (dBm) / TA after the call's good SACCH frames (SACCHL1Decoder::handleGoodFrame: power from
   * the header's 5-bit level, TA if < 64), -1 on channels that are not SACCH. */
  const int32_t *d_tch_rssi, *d_tch_timing, *d_xcch_rssi, *d_xcch_timing, *d_ms_power, *d_ms_ta;
} trxsig_l1rx_out;

/* Decode a pull of whole frames that starts at (fn, TN 0): res->n_slots a multiple of 8, res->n_arfcn the object's, fn in
 * [0, 2715648).  THE CALLER MUST HAVE PULLED FROM TN 0 (trxsig_trxgroup_pull's tn = 0): a result carries no timeslot, so a pull
 * that starts at another TN cannot be told apart here and would be routed as if slot 0 were TN 0.  Reads res's d_row, d_valid,
 * d_soft, soft_stride, n_rows, d_amp, d_toa, n_slots and n_arfcn only.  A burst is routed by its (TN, FN mod 5304) as receiveBurst does, where d_valid is set; the channel's decoder takes it as writeLowSide
 * does.  wire_quantise as the stream decoders (trxsig.h).  Everything is enqueued on the context's stream (the demux kernel,
 * the TCH and XCCH stream decoders, the RACH decoder, a fold); nothing synchronises.  Bad arguments return TRXSIG_EINVAL before
 * any launch. */
int trxsig_l1rx_decode(trxsig_l1rx *l1, const trxsig_trxgroup_result *res, int fn, int wire_quantise, trxsig_l1rx_out *out);

/* the channels' decoder records, for tests and checkpoints: [n_chan][TRXSIG_*_RX_STATE_BYTES] device arrays (TCH / XCCH) */
int trxsig_l1rx_state(trxsig_l1rx *l1, int cls, void **d_state);

#ifdef __cplusplus
}
#endif
#endif /* TRXSIG_L1RX_H */
