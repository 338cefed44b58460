/* trxsig_l1pacc.h -- packet access through L1: the access bursts a packet handset sends on a packet data channel before its first
 * normal burst, on the device.  Two jobs: asking for resources with an access burst on a PRACH block, and keeping the timing
 * advance current without a dedicated channel, with an access burst on the handset's PTCCH/U frame every 416 frames, answered by
 * the timing-advance message on PTCCH/D.  The object stands beside trxsig_l1pdch (whose header text, record size and kernel list
 * are that object's own): the handset side writes trxsig_l1tx's burst grid, the base-station side reads the slot cells a
 * Transceiver-group pull reads, runs the access-burst detector on the frames that can carry an access burst, decodes what it
 * finds with the access burst's coders of trxsig.h (trxsig_fec_access_encode_batch / _decode_batch), turns arrival times into
 * timing advances per TAI and forms the PTCCH/D message.  The reference has no packet channel.
 *
 * Plan.  h_comb[n_arfcn][8] as trxsig_l1pdch takes it: 13 marks a packet data channel; 0, 1, 5 and 7 are accepted and ignored;
 * anything else is TRXSIG_EINVAL.  PDCHs are numbered in (ARFCN, TN) order, as trxsig_l1pdch numbers its channels.  bsic: the
 * cell's, 0..63; it colours the parity of every burst sent and is what a received burst's parity must give.
 *
 * Frames.  WRITTEN FROM MEMORY of GSM 05.02 / 03.64, NOT CHECKED AGAINST THE STANDARD; tests/l1_pacc_model.py is this statement
 * in numpy.
 *   PTCCH/U: the frame with FN mod 416 = 12 + 26 n belongs to the handset with timing-advance index TAI n = 0..15.  These are
 *     the frames with FN mod 52 = 12 or 38, the frames trxsig_l1pdch.h gives to PTCCH/D on the downlink.
 *   PRACH: a block B0..B11 (trxsig_pdch_map_host) that the caller marks gives four access occasions, one per frame: what a block
 *     announced with USF = FREE is.
 *   Block indexing in a call follows trxsig_l1pdch_decode's rule: block b is the b-th block with a frame in [fn, fn + n_frames);
 *     trxsig_l1pacc_grid reports that count nb.  Entry t = 0..3 of a block is its t-th frame whether or not it lies in the call.
 *
 * Handset side, trxsig_l1pacc_encode.  Device inputs per PDCH: ptcch_kind / ptcch_ra [n_pdch][16] by TAI -- kind 1 sends on every
 *   frame of that TAI inside the call; prach_kind / prach_ra [n_pdch][nb][4] -- kind 1 sends on that frame of that block; ra is
 *   uint16; one fmt (TRXSIG_ACCESS_8 / _11) per call.  An ra that does not fit the format is not sent.  Output: trxsig_l1tx's
 *   grid layout, d_bits [n_arfcn][8 n_frames][148] and d_what [n_arfcn][8 n_frames], with TRXSIG_L1TX_PACC on a written slot; the
 *   bits are the coder's (k_fec_access_encode).  With d_bits_onto == d_what_onto == NULL the object writes its own grid, zeros
 *   elsewhere (valid until its next encode); otherwise it writes only the slots it puts a burst on, exactly as
 *   trxsig_l1pdch_encode does.  Access bursts are sent with timing advance 0: turning bits into samples, the delay and the level
 *   stay with trxsig_modulate_batch, trxsig_delay_vector_batch and trxsig_scale_vector_batch.  The call keeps no state.
 *
 * Base-station side, trxsig_l1pacc_detect.  d_samples: slot cells in the layout trxsig_trxgroup_pull reads (slot t = 8 k + TN of
 *   frame fn + k and ARFCN a at d_samples + t * slot_stride + a * arfcn_stride, (156 + (TN % 4 == 0)) * sps samples).  h_prach
 *   [n_pdch][nb] is a HOST array (nonzero: the block is a PRACH block): the scheduler knows its PRACH blocks before the uplink
 *   arrives, and a host list sizes the detector without a synchronise; NULL means none.  The host lists the occasions -- every
 *   PTCCH/U frame of every PDCH, plus the four frames of each marked block, where they lie in the call -- and every offset must
 *   fit int32 (else TRXSIG_EINVAL).  On the list it runs trxsig_detect_demod_rach_batch (leg TRXSIG_RACHLEG_DEMOD) or
 *   trxsig_mlse_rach_batch (TRXSIG_RACHLEG_MLSE) as they are, then k_fec_access_decode (fmt 0, 1 or -1 with the cell's BSIC,
 *   wire_quantise as there), then one fold kernel.
 *   Outputs, dense per frame [n_pdch][n_frames], the object's own arrays (valid until its next detect): kind (0 none, 1 PTCCH/U,
 *   2 PRACH), tai (int8; -1 where kind is not 1); det (the detector's TRXSIG_F_DETECT as 0 / 1); fmt, ok (det, tail bits zero and
 *   the parity's BSIC is the cell's) and ra (uint16) -- all 0 where det is 0; amp, toa, avgpwr as the detector gave them (0 where
 *   kind is 0); ta = t < 0 ? 0 : min(63, (int)(t + 0.5F)) with t = toa / (float)sps (0 where det is 0).
 *   State per PDCH (TRXSIG_L1PACC_STATE_BYTES): a table of 16 entries by TAI -- TA, FN of the measurement, valid.  The fold
 *   updates it in frame order from every PTCCH/U burst with ok.  One call of F frames equals any split of it, in every output
 *   and in the state.
 * trxsig_l1pacc_ta_message fills d_kind [n_pdch][nb_pt] and d_payload [n_pdch][nb_pt][23] in the form trxsig_l1pdch_encode takes
 *   for its PTCCH class: kind 1 throughout; octet i < 16 is the TA of TAI i with bit 7 zero, or 0x7F where the table holds none;
 *   octets 16..22 are 0x2B.  THE OCTET LAYOUT IS FROM MEMORY of GSM 04.04 / 04.60, not checked.  It is a pure function of the
 *   table at the point of the call in stream order.
 * trxsig_l1pacc_ta_read is the handset's side: from the trxsig_l1pdch_dec of a handset's decode (a DOWN object with this plan:
 *   n_ptcch must be n_pdch) it writes d_ta [n_pdch][16]: octets 0..15 of the latest PTCCH/D block of the call with ok set,
 *   where they hold a value (0..63); unchanged where the octet holds none and where no block came with ok.
 *
 * Every call only enqueues on the context's stream (k_l1pacc_stage, k_fec_access_encode, k_l1pacc_mux; the detector's own
 * kernels, k_fec_access_decode, k_l1pacc_fold; k_l1pacc_message; k_l1pacc_read), its own kernels booked under TRXSIG_K_FEC;
 * nothing synchronises or reads back; the occasion list goes up through pinned blocks taken in turn; the workspaces only grow.
 * Bad arguments return TRXSIG_EINVAL before any launch.
 *
 * Out of scope: any change to the group's classifier (it has no type for a PDCH), the multiplexers or trxsig_l1pdch;
 * device-resident PRACH marks; USF scheduling and RLC/MAC; EGPRS training sequences for access bursts; two antennas; the
 * PACKET CHANNEL REQUEST contents.
 * Thread safety: one caller at a time per object.
 */
#ifndef TRXSIG_L1PACC_H
#define TRXSIG_L1PACC_H

#include "trxsig_l1pdch.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct trxsig_l1pacc trxsig_l1pacc;

/* d_what code of a slot this object wrote (after trxsig_l1tx.h's TRXSIG_L1TX_* and TRXSIG_L1TX_PDCH) */
enum { TRXSIG_L1TX_PACC = 9 };
/* d_kind of a frame in trxsig_l1pacc_det */
enum { TRXSIG_L1PACC_NONE = 0, TRXSIG_L1PACC_PTCCH = 1, TRXSIG_L1PACC_PRACH = 2 };
/* size of a PDCH's record (trxsig_l1pacc_state): int32 ta[16], int32 fn[16], uint8 valid[16] */
#define TRXSIG_L1PACC_STATE_BYTES 144

int trxsig_l1pacc_create(trxsig_l1pacc **out, trxsig_ctx *ctx, int n_arfcn, const uint8_t *h_comb, int bsic);
void trxsig_l1pacc_destroy(trxsig_l1pacc *p);
int trxsig_l1pacc_channels(const trxsig_l1pacc *p);
int trxsig_l1pacc_channel(const trxsig_l1pacc *p, int chan, int *arfcn, int *tn);
/* the number of blocks with a frame in a call of n_frames frames from fn (no launch) */
int trxsig_l1pacc_grid(const trxsig_l1pacc *p, int fn, int n_frames, int *nb);
/* the PDCHs' records, [n_pdch][TRXSIG_L1PACC_STATE_BYTES] (device; for tests and checkpoints) */
int trxsig_l1pacc_state(trxsig_l1pacc *p, void **d_state);

typedef struct {
  int fmt;                                        /* TRXSIG_ACCESS_8 or TRXSIG_ACCESS_11 */
  const uint8_t *d_ptcch_kind;                    /* [n_pdch][16] */
  const uint16_t *d_ptcch_ra;                     /* [n_pdch][16] */
  const uint8_t *d_prach_kind;                    /* [n_pdch][nb][4] */
  const uint16_t *d_prach_ra;                     /* [n_pdch][nb][4] */
} trxsig_l1pacc_in;

typedef struct {
  int n_arfcn, n_frames;
  uint8_t *d_bits;            /* [n_arfcn][8 n_frames][148]: the object's own grid, or d_bits_onto */
  uint8_t *d_what;            /* [n_arfcn][8 n_frames]: TRXSIG_L1TX_PACC on a written slot */
} trxsig_l1pacc_out;

/* fn in [0, 2715648), 0 < n_frames <= 2715648, n_arfcn * 8 * n_frames * 148 <= 2^34 bytes, n_pdch * n_frames <=
 * TRXSIG_ACCESS_MAX_BURSTS; d_bits_onto and d_what_onto both NULL or both given; the input arrays where there is a PDCH (the PRACH pair where the call has a block). */
int trxsig_l1pacc_encode(trxsig_l1pacc *p, int fn, int n_frames, const trxsig_l1pacc_in *in, uint8_t *d_bits_onto,
                         uint8_t *d_what_onto, trxsig_l1pacc_out *out);

/* device resident, owned by the object, valid until its next detect; all [n_pdch][n_frames] */
typedef struct {
  int n_pdch, n_frames;
  const uint8_t *d_kind;
  const int8_t *d_tai;
  const uint8_t *d_det, *d_fmt, *d_ok;
  const uint16_t *d_ra;
  const trxsig_c32 *d_amp;
  const float *d_toa, *d_avgpwr;
  const uint8_t *d_ta;
} trxsig_l1pacc_det;

/* fmt in -1..1, leg TRXSIG_RACHLEG_DEMOD or TRXSIG_RACHLEG_MLSE, fn and n_frames as above, at most TRXSIG_ACCESS_MAX_BURSTS
 * occasions, every occasion's offset in [0, 2^31). */
int trxsig_l1pacc_detect(trxsig_l1pacc *p, const trxsig_c32 *d_samples, int64_t slot_stride, int64_t arfcn_stride, int fn,
                         int n_frames, const uint8_t *h_prach, int fmt, int leg, float detect_thresh, float energy_thresh,
                         int wire_quantise, trxsig_l1pacc_det *out);

int trxsig_l1pacc_ta_message(trxsig_l1pacc *p, uint8_t *d_kind, uint8_t *d_payload, int nb_pt);
int trxsig_l1pacc_ta_read(trxsig_l1pacc *p, const trxsig_l1pdch_dec *dec, uint8_t *d_ta);

#ifdef __cplusplus
}
#endif
#endif /* TRXSIG_L1PACC_H */
