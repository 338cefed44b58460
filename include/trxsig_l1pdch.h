/* trxsig_l1pdch.h -- packet data channels through L1: the GPRS block coders of trxsig.h (trxsig_fec_pdtch_encode_batch /
 * _decode_batch) on the 52-multiframe, on the device.  What trxsig_l1tx / trxsig_l1rx and trxsig_l1ms / trxsig_l1msrx do for the
 * circuit-switched channels, this object does for the slots of GSM 05.02 combination XIII (PDTCH/F + PACCH/F + PTCCH/F): it
 * writes trxsig_l1tx's burst grid and reads a Transceiver-group pull, keeps state across calls, takes missing bursts and lets a
 * call be cut at any frame.  The reference has no packet channel.  The four multiplexers, the plan module and the group are not
 * changed: the packet channels live in this object beside them.
 *
 * The object is symmetric: it encodes payloads to timed bursts and decodes a pull to payloads.  A base station encodes on a
 * TRXSIG_L1PDCH_DOWN object and decodes on a TRXSIG_L1PDCH_UP object; a test handset does the reverse.
 *
 * Plan.  h_comb[n_arfcn][8] in the SETSLOT numbering: 13 marks a packet data channel; 0, 1, 5 and 7 are accepted and ignored;
 * anything else is TRXSIG_EINVAL.  The same array with 13 replaced by 0 is what the four multiplexers and the group take.  On a
 * PDCH's uplink slot the group wants SETSLOT type 1 (normal bursts on every frame).
 *
 * Channels, two classes, each numbered in (ARFCN, TN) order:
 *   TRXSIG_L1PDCH_PDTCH  one per PDCH, both directions.  Blocks B0..B11 of every 52-multiframe exactly as trxsig_pdch_map_host
 *     places them (frames 0-3, 4-7, 8-11, 13-16, ..., 47-50).  Absolute block number = 12 * (FN / 52) + B, modulo 12 * 52224.
 *   TRXSIG_L1PDCH_PTCCH  one per PDCH on a DOWN object; an UP object has none.  One CS-1 block per 104 frames, on the frames
 *     with FN mod 104 = 12, 38, 64, 90.  Absolute block number = FN / 104, modulo 26112.
 *   Frames 25 and 51 of the 52-multiframe belong to nobody; on an UP object frames 12 and 38 belong to nobody either.
 * NOT CHECKED AGAINST THE STANDARD: the PTCCH/D block positions are written from memory of GSM 05.02, as the coders' tables in
 * trxsig.h are from memory of GSM 05.03; no copy was at hand.  tests/l1_pdch_model.py is this statement in numpy.
 * Every normal burst carries training sequence bsic & 7.  There is no open / close: a PDCH is a shared channel, and "nothing to
 * send" is a kind, not a channel state.
 *
 * Encode.  A call covers whole frames [fn, fn + n_frames).  Block b of a channel is its b-th block whose first burst is at or
 *   after fn (trxsig_l1tx's rule); trxsig_l1pdch_grid gives the block counts nb, the same for every channel of a class.
 *   Inputs, device arrays: PDTCH kind [n][nb] (1: send, anything else: nothing), cs [n][nb] (TRXSIG_CS1..4; above 3: not sent),
 *   payload [n][nb][54] in the coders' payload convention; PTCCH kind [n][nb_pt], payload [n][nb_pt][23] (CS-1).
 *   Bursts of a block that fall after the call's last frame stay in the channel's record and go out in the following calls (for
 *   a PTCCH block up to 78 frames later), provided those calls continue where this one ended.
 *   Output: trxsig_l1tx's layout, d_bits [n_arfcn][8 n_frames][148] and d_what [n_arfcn][8 n_frames], with TRXSIG_L1TX_PDCH on
 *   a written slot.  With d_bits_onto == d_what_onto == NULL the object writes its own grid, zeros elsewhere (valid until its
 *   next encode).  Otherwise both are the caller's arrays of that layout and the object writes only the slots it puts a burst on
 *   (148 bytes and the what byte); it neither reads nor clears any other slot.  A caller may overlay onto trxsig_l1tx's last
 *   grid until that object's next encode (the const of its trxsig_l1tx_out is cast away): trxsig_l1tx leaves the slots of a
 *   combination-0 position as zero bits with what 0, and trxsig_trxgroup_add_l1tx, which tests what != 0, then queues the packet
 *   bursts with the rest.
 *   USF record: a DOWN object records, per PDTCH channel, the USF (d(0) | d(1) << 1 | d(2) << 2 of the payload) of each block it
 *   sends, in a ring of TRXSIG_L1PDCH_RING entries keyed by absolute block number.
 *   One call of F frames equals calls that split F at any frame boundaries, in every output byte and in the state.
 *
 * Decode.  res: a trxsig_trxgroup_result of whole frames pulled from TN 0 (read as trxsig_l1rx_decode reads it).  A burst is
 *   taken where d_row >= 0 and d_valid is set, on a frame its channel owns.  Block b of a channel is the b-th block that has a
 *   burst frame in the call, counted from the first (trxsig_l1rx's rule): a block shows in every call its frames overlap and is
 *   decoded only in the call that holds its fourth burst's frame, whether or not that burst arrived.  Soft rows that arrived in
 *   earlier calls are carried in the object as raw floats.  So one call equals any split of it, block for block by closing FN,
 *   provided wire_quantise is the same throughout.
 *   Per block [n][nb]: d_payload (54 / 23 octets), d_cs, d_cs_dist, d_ok, d_usf as trxsig_fec_pdtch_decode_batch gives them;
 *   d_nb = accepted bursts so far (0..4); d_fn = the closing FN modulo the hyperframe, -1 on a block that does not close in this
 *   call (its other outputs: ok 0, cs = cs_dist = usf = 255, zero payload); d_granted.  A block that closes with d_nb == 0
 *   reports ok = 0, cs = cs_dist = usf = 255 and a zero payload; one with 1..3 bursts is decoded with the missing bursts at 0.5.
 *   cs_force as the coder's (-1: detect); PTCCH blocks are decoded as CS-1.
 *   d_granted: 255 when sibling is NULL (and on PTCCH); else the USF the sibling recorded for absolute block n - 1 on the same
 *   (ARFCN, TN), or 255 if that slot of its ring holds another block.  A sibling with another h_comb is TRXSIG_EINVAL.
 *   Per channel: RSSI and timing of the last accepted burst, by trxsig_l1rx's formulas (unchanged where none).
 *
 * Both calls only enqueue on the context's stream (k_l1pdch_stage, the coder's own k_fec_pdtch_encode, k_l1pdch_mux,
 * k_l1pdch_commit; k_l1pdch_demux, k_fec_pdtch_decode, k_l1pdch_fold), booked under TRXSIG_K_FEC; nothing synchronises, reads
 * back or allocates except a workspace that only grows.  Bad arguments return TRXSIG_EINVAL before any launch.
 *
 * Out of scope: PTCCH/U and PRACH (access bursts on a PDCH slot need the group's classifier); forming the timing-advance
 * message; USF gating on the handset side (kind is a device array: the caller can mask it from d_usf); dummy control blocks;
 * RLC/MAC; EGPRS; hopping or ciphering of packet slots (GPRS ciphers above L1); any change to the four multiplexers, the plan
 * module or the group.
 * Thread safety: one caller at a time per object.
 */
#ifndef TRXSIG_L1PDCH_H
#define TRXSIG_L1PDCH_H

#include "trxsig_l1tx.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct trxsig_l1pdch trxsig_l1pdch;

enum { TRXSIG_L1PDCH_DOWN = 0, TRXSIG_L1PDCH_UP = 1 };
enum { TRXSIG_L1PDCH_PDTCH = 0, TRXSIG_L1PDCH_PTCCH = 1 };
/* the SETSLOT number of a packet data channel in h_comb */
enum { TRXSIG_L1PDCH_COMB = 13 };
/* d_what code of a slot this object wrote (after trxsig_l1tx.h's TRXSIG_L1TX_*) */
enum { TRXSIG_L1TX_PDCH = 8 };
/* size of a channel record (trxsig_l1pdch_state); entries of its USF ring */
#define TRXSIG_L1PDCH_STATE_BYTES 3104
#define TRXSIG_L1PDCH_RING 32

int trxsig_l1pdch_create(trxsig_l1pdch **out, trxsig_ctx *ctx, int n_arfcn, const uint8_t *h_comb, int bsic, int dir);
void trxsig_l1pdch_destroy(trxsig_l1pdch *p);
int trxsig_l1pdch_channels(const trxsig_l1pdch *p, int cls);
int trxsig_l1pdch_channel(const trxsig_l1pdch *p, int cls, int chan, int *arfcn, int *tn);
/* the encode grid sizes of a call of n_frames frames from fn (no launch) */
int trxsig_l1pdch_grid(const trxsig_l1pdch *p, int fn, int n_frames, int *nb_pdtch, int *nb_ptcch);
/* the channel records of a class, [n_chan][TRXSIG_L1PDCH_STATE_BYTES] (device; opaque; for tests and checkpoints) */
int trxsig_l1pdch_state(trxsig_l1pdch *p, int cls, void **d_state);

typedef struct {
  const uint8_t *d_pdtch_kind, *d_pdtch_cs, *d_pdtch_payload;   /* [n][nb], [n][nb], [n][nb][54] */
  const uint8_t *d_ptcch_kind, *d_ptcch_payload;                /* [n][nb_pt], [n][nb_pt][23] */
} trxsig_l1pdch_in;

typedef struct {
  int n_arfcn, n_frames;
  uint8_t *d_bits;            /* [n_arfcn][8 n_frames][148]: the object's own grid, or d_bits_onto */
  uint8_t *d_what;            /* [n_arfcn][8 n_frames]: TRXSIG_L1TX_PDCH on a written slot */
} trxsig_l1pdch_out;

/* fn in [0, 2715648), 0 < n_frames <= 2715648, n_arfcn * 8 * n_frames * 148 <= 2^34 bytes, at most TRXSIG_PDTCH_MAX_BLOCKS blocks;
 * d_bits_onto and d_what_onto both NULL or both given; a NULL input array for a class that has channels and blocks in the call
 * is TRXSIG_EINVAL. */
int trxsig_l1pdch_encode(trxsig_l1pdch *p, int fn, int n_frames, const trxsig_l1pdch_in *in, uint8_t *d_bits_onto,
                         uint8_t *d_what_onto, trxsig_l1pdch_out *out);

/* device resident, owned by the object, valid until its next decode */
typedef struct {
  int n_pdtch, n_ptcch, nb_pdtch, nb_ptcch;
  const uint8_t *d_pdtch_payload, *d_pdtch_cs, *d_pdtch_cs_dist, *d_pdtch_ok, *d_pdtch_usf, *d_pdtch_nb, *d_pdtch_granted;
  const int32_t *d_pdtch_fn;                     /* [n_pdtch][nb_pdtch]([54]) */
  const uint8_t *d_ptcch_payload, *d_ptcch_cs, *d_ptcch_cs_dist, *d_ptcch_ok, *d_ptcch_usf, *d_ptcch_nb, *d_ptcch_granted;
  const int32_t *d_ptcch_fn;                     /* [n_ptcch][nb_ptcch]([23]) */
  const int32_t *d_pdtch_rssi, *d_pdtch_timing, *d_ptcch_rssi, *d_ptcch_timing;   /* [n_pdtch] / [n_ptcch] */
} trxsig_l1pdch_dec;

/* res->n_slots a multiple of 8, res->n_arfcn the object's, fn in [0, 2715648), cs_force in -1..3.  sibling: the DOWN object whose
 * USF record answers d_granted, with the same h_comb, or NULL. */
int trxsig_l1pdch_decode(trxsig_l1pdch *p, const trxsig_trxgroup_result *res, int fn, int wire_quantise, int cs_force,
                         const trxsig_l1pdch *sibling, trxsig_l1pdch_dec *out);

#ifdef __cplusplus
}
#endif
#endif /* TRXSIG_L1PDCH_H */
