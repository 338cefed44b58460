/* trxsig_l1tx.h -- the downlink L1 multiplexer: the logical channels' encoders to timed bursts, on the device.  The mirror of
 * trxsig_l1rx.h: what the reference's L1Encoder objects do behind TRXManager's data socket -- each encoder's walk of its
 * downlink TDMAMapping (L1Encoder::rollForward, GSM/GSMTDMA.cpp), XCCHL1Encoder / SACCHL1Encoder / TCHFACCHL1Encoder and the
 * beacon generators FCCHL1Encoder / SCHL1Encoder / BCCHL1Encoder (GSM/GSML1FEC.cpp), sendIdleFill on close -- and the
 * datagrams ARFCNManager::writeHighSide sends (TRXManager/TRXManager.cpp:173-200).
 *
 * Plan and channels.  h_comb, bsic and band mean what they mean for trxsig_l1rx_create: h_comb[a][tn] in 0 / 1 (I) / 5 (V, on
 * ARFCN 0 TN 0 only) / 7 (VII); anything else is TRXSIG_EINVAL.  TCH and XCCH channels are numbered exactly as trxsig_l1rx
 * numbers them, so channel c of a class names the same logical channel in both objects and XCCH channel c's SACCH sibling is
 * trxsig_l1rx's XCCH channel c.  TRXSIG_L1_CCCH holds CCCH_0..2 of the combination-V slot.  FCCH, SCH and BCCH of that slot are
 * generators: always on, never opened or closed.  The downlink mappings are GSMTDMA.cpp's *D tables (SDCCH_8_xD, SACCH_C8_xD,
 * SDCCH_4_xD, SACCH_C4_xD), SACCH_TF_Tn and FACCH_TCHF.  Every normal burst carries the training sequence of the BCC, bsic & 7.
 *
 * Blocks and calls.  A call covers whole frames [fn, fn + n_frames) from TN 0.  Block b of a channel is its b-th block whose
 * first burst (mapping position = 0 mod 4, positions as in trxsig_l1rx: absolute, on GSM 05.02's block grid) is at or after
 * fn; the caller gives its payload in that call.  Bursts of a block that fall after the call's last frame stay on the device
 * and go out in the following call(s).  trxsig_l1tx_grid reports, per class, the most blocks any channel opens: the grids are
 * [n_chan][nb]; a channel with fewer has trailing entries that are ignored.  One call of F frames equals calls that split F
 * at any frame boundaries, in every output byte (concatenated) and in the state.
 *
 * Inputs (trxsig_l1tx_in, device arrays).
 *   TCH: kind [n_tch][nb_tch], payload [n_tch][nb_tch][33], exactly as trxsig_fec_tch_encode_batch takes them (FILLER /
 *     SPEECH / FACCH, the context's filler, a kind above 2 an all-zero c[] that is not stolen); the interleaver state is
 *     carried per channel in the object.
 *   XCCH, CCCH: kind [n][nb] -- 1: a 23-octet L2 frame in payload [n][nb][23]; any other value: no frame, nothing is sent.
 *     On SACCH channels octets 0..1 are replaced by the L1 header (below).
 *   BCCH: from trxsig_l1tx_set_si; the block of TC = (FN / 51) % 8 of its first burst sends SI1, 2, 3, 4, 3, 2, 3, 4 for TC
 *     0..7 (BCCHL1Encoder::generate).  Until SIs are set, BCCH slots stay empty.
 *   SCH: SCHL1Encoder::generate for the burst's own FN and the cell's BSIC (as trxsig_fec_sch_encode_batch).  FCCH: 148 zeros.
 *
 * SACCH L1 header (SACCHL1Encoder::sendFrame, GSML1FEC.cpp:1455-1494), decided per call from the sibling trxsig_l1rx's device
 * state for the channel: its RSSI, timing error, actual MS power and TA.  phyNew: the sibling's channel has accepted at least one
 * burst since the orders were last decided, counting in stream order; every SACCH block of one call sees the same snapshot and
 * the first block sent consumes phyNew.  Then, in float32 as written: deltaP = RSSI - rssi_target; ordered = actual -
 * (int)round(deltaP * 0.5F) clamped to 0..40; orderedTA = actualTA - 0.5F * timingError clamped to 0..63.  Header octet 0 =
 * encodePower(ordered) (the band's table, nearest code, first on ties); octet 1 = (int)(orderedTA + 0.5F).  open of a SACCH
 * channel resets the orders to 40 dBm / 0.0; without a sibling they never change.  rssi_target is GSM.RSSITarget.
 *
 * Open / close.  A new object has every channel open.  A closed channel's grid entries are ignored and nothing of it is sent; its
 * encoder state is left as it is (the reference's open does not reset mI / mOffset / mPreviousFACCH either).  close queues
 * sendIdleFill: the channel's next numFrames mapping positions (24 for TCH, 4 otherwise), after any bursts it still has
 * pending, carry the dummy burst of GSM 05.02 5.2.6.
 * Deliberate deviations, both from keeping every channel on GSM 05.02's block grid:
 *   1. The reference's open() resets mTotalBursts without re-aligning mNextWriteTime, so a reopened encoder can leave the block
 *      grid; this object always stays on it (absolute positions, as trxsig_l1rx reads them).
 *   2. open cancels idle fill not yet sent.  The reference's close writes all numFrames dummy bursts at once, so they always go
 *      out and a reopened encoder starts after them (off the grid, see 1).  Here a reopened channel's blocks sit at their grid
 *      positions, which can be the very positions the rest of the idle fill would take; giving those slots to the channel's
 *      new blocks is the only way a slot keeps a single writer.
 * Thread safety: one caller at a time per object.
 */
#ifndef TRXSIG_L1TX_H
#define TRXSIG_L1TX_H

#include "trxsig_l1rx.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct trxsig_l1tx trxsig_l1tx;

/* the new class; TRXSIG_L1_TCH / TRXSIG_L1_XCCH as in trxsig_l1rx.h */
enum { TRXSIG_L1_CCCH = 3 };
/* mapping kind of a CCCH channel (trxsig_l1tx_channel); TCH / XCCH kinds as in trxsig_l1rx.h */
enum { TRXSIG_L1_CCCH_C5 = 7 };
/* d_what codes: which encoder wrote a slot */
enum { TRXSIG_L1TX_NONE = 0, TRXSIG_L1TX_FCCH = 1, TRXSIG_L1TX_SCH = 2, TRXSIG_L1TX_BCCH = 3, TRXSIG_L1TX_CCCH = 4,
       TRXSIG_L1TX_XCCH = 5, TRXSIG_L1TX_TCH = 6, TRXSIG_L1TX_IDLE = 7 };
/* size of a channel record (trxsig_l1tx_state) */
#define TRXSIG_L1TX_STATE_BYTES 160

int trxsig_l1tx_create(trxsig_l1tx **out, trxsig_ctx *ctx, int n_arfcn, const uint8_t *h_comb, int bsic, int band,
                       float rssi_target);
void trxsig_l1tx_destroy(trxsig_l1tx *l1);
int trxsig_l1tx_channels(const trxsig_l1tx *l1, int cls);
int trxsig_l1tx_channel(const trxsig_l1tx *l1, int cls, int chan, int *arfcn, int *tn, int *kind, int *sub);
/* L1Encoder::open / close of one TCH, XCCH or CCCH channel, in stream order on the context's stream */
int trxsig_l1tx_open(trxsig_l1tx *l1, int cls, int chan);
int trxsig_l1tx_close(trxsig_l1tx *l1, int cls, int chan);
/* SI1..SI4, [4][23] octets (host); synchronises the context's stream: calls already enqueued keep the SIs they had */
int trxsig_l1tx_set_si(trxsig_l1tx *l1, const uint8_t *h_si);
/* the grid sizes of a call of n_frames frames from fn (no launch) */
int trxsig_l1tx_grid(const trxsig_l1tx *l1, int fn, int n_frames, int *nb_tch, int *nb_xcch, int *nb_ccch);

typedef struct {
  const uint8_t *d_tch_kind, *d_tch_payload;     /* [n_tch][nb_tch], [n_tch][nb_tch][33] */
  const uint8_t *d_xcch_kind, *d_xcch_payload;   /* [n_xcch][nb_xcch], [n_xcch][nb_xcch][23] */
  const uint8_t *d_ccch_kind, *d_ccch_payload;   /* [n_ccch][nb_ccch], [n_ccch][nb_ccch][23] */
} trxsig_l1tx_in;

/* device resident, owned by the object, valid until its next encode */
typedef struct {
  int n_arfcn, n_frames, n_xcch;
  const uint8_t *d_bits;      /* [n_arfcn][8 n_frames][148], one bit per byte: what trxsig_modulate_batch takes */
  const uint8_t *d_what;      /* [n_arfcn][8 n_frames]: TRXSIG_L1TX_*; empty slots are zero bits */
  const int32_t *d_ms_power;  /* [n_xcch] the SACCH orders after the call (dBm), -1 on channels that are not SACCH */
  const float *d_ms_ta;       /* [n_xcch] ... (symbols), -1 on channels that are not SACCH */
} trxsig_l1tx_out;

/* Encode frames [fn, fn + n_frames) (fn in [0, 2715648), n_frames > 0, n_arfcn * 8 * n_frames * 148 <= 2^34 bytes).  sibling:
 * the trxsig_l1rx whose SACCH state drives the orders, with the same plan, or NULL.  Enqueued on the context's stream (k_l1tx_
 * encode, k_l1tx_mux, k_l1tx_commit); nothing synchronises.  NULL grids for a class that has channels, a bad fn / n_frames, a
 * sibling with another plan or sizes that overflow return TRXSIG_EINVAL before any launch. */
int trxsig_l1tx_encode(trxsig_l1tx *l1, int fn, int n_frames, const trxsig_l1tx_in *in, const trxsig_l1rx *sibling,
                       trxsig_l1tx_out *out);
/* The last encode's non-empty slots as the 154-byte datagrams of ARFCNManager::writeHighSide (TN, FN big-endian, power byte 0,
 * 148 bits), in (FN, TN, ARFCN) order, with each one's ARFCN: what trxsig_trxgroup_add_bursts takes.  Compacted on the device
 * and copied down once; synchronises.  *n = the count; if cap is smaller, TRXSIG_EINVAL with *n the count needed. */
int trxsig_l1tx_datagrams(trxsig_l1tx *l1, uint8_t *h_dgram, int32_t *h_arfcn, int cap, int *n);
/* addRadioVector for every non-empty slot of l1's LAST encode, device to device.  Same effect on g as
 * trxsig_l1tx_datagrams + trxsig_trxgroup_add_bursts of what it returns (power byte 0, gain 1.0), without the copy down, the
 * host parse or the upload: per ARFCN the bursts enter in (FN, TN) order, a full queue or payload pool accepts the same prefix
 * and marks the same ARFCNs dropped.  Enqueues only (k_group_tx_arrive_grid on the context's stream, behind the encode; the
 * payloads move into the group's own memory there, so l1 may encode again at once); never synchronises; copies nothing to the
 * host.  The ingest stays pending exactly as after trxsig_trxgroup_add_bursts: the push that follows takes it into its launch.
 * Only a call larger than any before allocates (and waits for the group's earlier transmit work while it does).
 * TRXSIG_EINVAL, with nothing queued: g or l1 NULL, different contexts, l1's n_arfcn is not g's, no encode yet (or none since
 * l1's workspace last grew), a staging block lent out by trxsig_trxgroup_tx_staging and not yet added.  An encode whose slots
 * are all empty is TRXSIG_OK and queues nothing. */
int trxsig_trxgroup_add_l1tx(trxsig_trxgroup *g, trxsig_l1tx *l1);
/* the channel records of a class, [n_chan][TRXSIG_L1TX_STATE_BYTES] (device; opaque; for tests and checkpoints) */
int trxsig_l1tx_state(trxsig_l1tx *l1, int cls, void **d_state);

#ifdef __cplusplus
}
#endif
#endif /* TRXSIG_L1TX_H */
