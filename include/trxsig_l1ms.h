/* trxsig_l1ms.h -- the mobile side of the uplink L1: per-channel uplink payloads to timed uplink bursts, and those bursts to the
 * complex samples trxsig_trxgroup_pull takes, on the device.  The third sibling of trxsig_l1rx.h / trxsig_l1tx.h: what the
 * handsets of a cell do -- XCCHL1Encoder / SACCHL1Encoder / TCHFACCHL1Encoder (GSM/GSML1FEC.cpp) walking the UPLINK
 * TDMAMappings (GSM/GSMTDMA.cpp), the access burst RACHL1Decoder::writeLowSide reads, the handset's transmit power and timing
 * advance as the SACCH orders of trxsig_l1tx set them -- so that l1tx -> l1ms -> radiate -> pull -> l1rx closes the loop.
 *
 * Plan and channels.  h_comb, bsic and band mean what they mean for trxsig_l1rx_create: h_comb[a][tn] in 0 / 1 (I) / 5 (V, on
 * ARFCN 0 TN 0 only) / 7 (VII); anything else is TRXSIG_EINVAL.  TCH and XCCH channels are numbered exactly as trxsig_l1rx
 * numbers them; TRXSIG_L1_RACH is the combination-V slot's RACH.  The mappings are the uplink ones the demultiplexer reads
 * (FACCH_TCHF, SACCH_TF_Tn, SDCCH_4_xU, SACCH_C4_xU, SDCCH_8_xU, SACCH_C8_xU, RACHC5).  Every normal burst carries the
 * training sequence of the BCC, bsic & 7.
 *
 * Blocks and calls, as trxsig_l1tx.h.  A call covers whole frames [fn, fn + n_frames) from TN 0.  Block b of a channel is its
 * b-th block whose first burst (mapping position = 0 mod 4) is at or after fn; the caller gives its payload in that call.
 * Bursts of a block that fall after the call's last frame stay on the device and go out in the following call(s).
 * trxsig_l1ms_grid reports, per class, the most blocks any channel opens, and the number of RACH frames of the call (equal to
 * trxsig_l1rx's rach_cap for the same call).  One call of F frames equals calls that split F at any frame boundaries, in every
 * output byte (concatenated) and in the state.
 *
 * Inputs (trxsig_l1ms_in, device arrays).
 *   TCH: kind [n_tch][nb_tch], payload [n_tch][nb_tch][33], exactly as trxsig_fec_tch_encode_batch takes them (the context's
 *     filler; a kind above 2 an all-zero c[] that is not stolen); the interleaver state is carried per channel in the object.
 *   XCCH: kind [n_xcch][nb_xcch] -- 1: a 23-octet L2 frame in payload [n_xcch][nb_xcch][23]; any other value: nothing is sent
 *     (there is no uplink idle fill; LAPDm fill frames are the caller's).  On SACCH channels octets 0..1 are replaced by the
 *     handset's L1 header: octet 0 = encodePower(power) of the band's table (5 bits), octet 1 = the TA -- the fields
 *     SACCHL1Decoder::handleGoodFrame reads back.
 *   RACH: rach_kind [n_rach], rach_ra [n_rach], optional rach_bsic [n_rach] (NULL: the cell's BSIC; else the low 6 bits), one
 *     entry per RACH frame of the call in FN order.  Kind 1 sends an access burst: bits 0..7 the extended tail of GSM 05.02
 *     5.2.7 (0,0,1,1,1,0,1,0), 8..48 the 41-bit synch sequence, 49..84 the 36 coded bits (GSM 05.03 4.6: the RA LSB first, six
 *     parity bits coloured with the BSIC, four tail bits, the rate-1/2 coder), 85..147 zero.
 *
 * Handset state, per SACCH channel: the actual power (dBm, always an entry of the band's table) and the actual TA.  The
 * dedicated channel that shares the handset uses its SACCH's state: the TCH of a combination-I slot that slot's SACCH/TF, SDCCH
 * s SACCH s.  A new object, and open of a SACCH channel, set power POWER[band][encodePower(band, 40)] and TA 0.
 * trxsig_l1ms_set_phy sets power POWER[band][encodePower(band, power_dbm)] and the TA.  With a sibling trxsig_l1tx, every open
 * SACCH channel takes the sibling's current orders for the same channel number at the start of the call: power =
 * POWER[band][encodePower(band, ordered)], TA = (int)(orderedTA + 0.5F) -- what the header trxsig_l1tx writes decodes to.  Every
 * block of the call sees that one snapshot.  Without a sibling only set_phy and open move the state -- unless the object follows
 * a trxsig_l1msrx (trxsig_l1ms_follow): then the orders are the ones that object DECODED from the downlink's SACCH headers.
 *
 * Open / close.  A new object has every channel open.  A closed channel's grid entries are ignored and nothing new of it is
 * sent (a block already begun goes out to its end); its encoder state is left as it is.  The RACH has no active flag.
 * Thread safety: one caller at a time per object.
 */
#ifndef TRXSIG_L1MS_H
#define TRXSIG_L1MS_H

#include "trxsig_l1tx.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct trxsig_l1ms trxsig_l1ms;

/* d_what codes: which encoder wrote a slot */
enum { TRXSIG_L1MS_NONE = 0, TRXSIG_L1MS_TCH = 1, TRXSIG_L1MS_XCCH = 2, TRXSIG_L1MS_ACCESS = 3 };
/* size of a channel record (trxsig_l1ms_state) */
#define TRXSIG_L1MS_STATE_BYTES 160

/* The object keeps ctx alive: trxsig_destroy on ctx takes effect when the object is gone too. */
int trxsig_l1ms_create(trxsig_l1ms **out, trxsig_ctx *ctx, int n_arfcn, const uint8_t *h_comb, int bsic, int band);
void trxsig_l1ms_destroy(trxsig_l1ms *ms);
/* number of channels of a class (negative: bad argument) */
int trxsig_l1ms_channels(const trxsig_l1ms *ms, int cls);
int trxsig_l1ms_channel(const trxsig_l1ms *ms, int cls, int chan, int *arfcn, int *tn, int *kind, int *sub);
/* open / close of one TCH or XCCH channel, in stream order on the context's stream; TRXSIG_L1_RACH is TRXSIG_EINVAL, as in
 * trxsig_l1rx */
int trxsig_l1ms_open(trxsig_l1ms *ms, int cls, int chan);
int trxsig_l1ms_close(trxsig_l1ms *ms, int cls, int chan);
/* the handset of SACCH channel xcch_chan: power_dbm in 0..40 (taken to the band's nearest level), ta in 0..63; stream-ordered.
 * A channel that is not SACCH or a value out of range is TRXSIG_EINVAL. */
int trxsig_l1ms_set_phy(trxsig_l1ms *ms, int xcch_chan, int power_dbm, int ta);
/* the grid sizes of a call of n_frames frames from fn (no launch) */
int trxsig_l1ms_grid(const trxsig_l1ms *ms, int fn, int n_frames, int *nb_tch, int *nb_xcch, int *n_rach);

typedef struct {
  const uint8_t *d_tch_kind, *d_tch_payload;     /* [n_tch][nb_tch], [n_tch][nb_tch][33] */
  const uint8_t *d_xcch_kind, *d_xcch_payload;   /* [n_xcch][nb_xcch], [n_xcch][nb_xcch][23] */
  const uint8_t *d_rach_kind, *d_rach_ra;        /* [n_rach], [n_rach] */
  const uint8_t *d_rach_bsic;                    /* [n_rach] or NULL */
} trxsig_l1ms_in;

/* device resident, owned by the object, valid until its next encode */
typedef struct {
  int n_arfcn, n_frames, n_xcch;
  const uint8_t *d_bits;      /* [n_arfcn][8 n_frames][148], one bit per byte */
  const uint8_t *d_what;      /* [n_arfcn][8 n_frames]: TRXSIG_L1MS_*; empty slots are zero bits */
  const int32_t *d_ms_power;  /* [n_xcch] the handsets' power after the call (dBm), -1 on channels that are not SACCH */
  const int32_t *d_ms_ta;     /* [n_xcch] ... their TA (symbols), -1 on channels that are not SACCH */
} trxsig_l1ms_out;

/* Encode frames [fn, fn + n_frames) (fn in [0, 2715648), n_frames > 0, n_arfcn * 8 * n_frames * 148 <= 2^34 bytes).  sibling:
 * the trxsig_l1tx whose orders the handsets follow, with the same plan and context, or NULL.  Enqueued on the context's stream
 * (k_l1ms_encode, k_l1ms_mux, k_l1ms_commit); nothing synchronises.  NULL grids for a class that has channels in the call, a
 * bad fn / n_frames, a sibling with another plan or sizes that overflow return TRXSIG_EINVAL before any launch. */
int trxsig_l1ms_encode(trxsig_l1ms *ms, int fn, int n_frames, const trxsig_l1ms_in *in, const trxsig_l1tx *sibling,
                       trxsig_l1ms_out *out);

/* the air between the handsets and the base station's antenna (device arrays) */
typedef struct {
  const trxsig_c32 *d_tch_gain;  const float *d_tch_delay;    /* [n_tch]: path gain, delay in symbols */
  const trxsig_c32 *d_xcch_gain; const float *d_xcch_delay;   /* [n_xcch] */
  const trxsig_c32 *d_rach_gain; const float *d_rach_delay;   /* [n_rach] of the last encode */
  const float *d_amp_of_power;                                /* [41]: amplitude of a handset at 0..40 dBm */
} trxsig_l1ms_air;

/* The last encode as samples, in the layout trxsig_trxgroup_pull reads: slot t (of 8 n_frames) of ARFCN a at d_samples +
 * t * slot_stride + a * arfcn_stride, N = (156 + (TN % 4 == 0)) * sps samples.  A non-empty slot is
 *   scaleVector(delayVector(modulateBurst(bits, guard = 8 + (TN % 4 == 0), sps), d), A)
 * with d = (delay - (float)TA) * (float)sps and A = (gain.r * s, gain.i * s), s = amp_of_power[power], for a dedicated channel
 * (its handset's TA and power after the encode), d = delay * (float)sps and A = gain for an access burst, all in float32 as
 * written: IEEE-equal to trxsig_modulate_batch (no gain) -> trxsig_delay_vector_batch -> trxsig_scale_vector_batch on the same
 * bursts (a delay those refuse gives zeros, as they do).  Empty slots are N zeros; nothing outside the N samples is written.
 * One launch (k_l1ms_radiate) on the context's stream; nothing synchronises.  TRXSIG_EINVAL before any launch: NULL arrays for
 * a class that has channels, no encode yet (or none since the workspace last grew), strides under which cells overlap
 * (slot_stride and arfcn_stride at least 157 sps apart, in either nesting). */
int trxsig_l1ms_radiate(trxsig_l1ms *ms, const trxsig_l1ms_air *air, trxsig_c32 *d_samples, int64_t slot_stride,
                        int64_t arfcn_stride);
/* the channel records of a class (TCH / XCCH), [n_chan][TRXSIG_L1MS_STATE_BYTES] (device; opaque; for tests and checkpoints) */
int trxsig_l1ms_state(trxsig_l1ms *ms, int cls, void **d_state);

/* Follow the SACCH orders a trxsig_l1msrx (trxsig_l1msrx.h) decodes.  rx must have ms's context and plan (n_arfcn, h_comb,
 * bsic, band), else TRXSIG_EINVAL; rx = NULL stops following.  While following, an encode with sibling == NULL gives every open
 * SACCH channel, at the start of the call, power POWER[band][encodePower(band, ord_power)] and TA ord_ta, read from rx's device
 * state in stream order: one snapshot per call, what trxsig_l1ms_set_phy(chan, ord_power, ord_ta) before the encode would
 * give.  An encode with a non-NULL sibling while following is TRXSIG_EINVAL.  The caller stops following before it destroys
 * rx.  No launch. */
struct trxsig_l1msrx;
int trxsig_l1ms_follow(trxsig_l1ms *ms, const struct trxsig_l1msrx *rx);

#ifdef __cplusplus
}
#endif
#endif /* TRXSIG_L1MS_H */
