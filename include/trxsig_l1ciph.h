/* trxsig_l1ciph.h -- ciphering for dedicated channels on the device: the stage GSM 05.03 puts between the interleaver and the
 * burst builder (GSM 03.20 Annex C, algorithm A5/1), in both directions and on both sides of the air:
 *   l1tx_encode -> BITS(downlink) -> add_l1tx / modulate -> ... -> pull -> SOFT(downlink) -> l1msrx_decode
 *   l1ms_encode -> BITS(uplink)   -> radiate            -> ... -> pull -> SOFT(uplink)   -> l1rx_decode
 * THIS STAGE HAS NO REFERENCE COUNTERPART (the reference is a base station that never enables ciphering).  Every output is exact
 * and equal to tests/l1_ciph_model.py, which the published A5/1 test vector below pins.
 *
 * The algorithm.  Three shift registers; one clock of a register is R = ((R << 1) & mask) | feedback:
 *   R1  19 bits  feedback = XOR of bits 18, 17, 16, 13   clocking bit  8   output bit 18
 *   R2  22 bits  feedback = XOR of bits 21, 20           clocking bit 10   output bit 21
 *   R3  23 bits  feedback = XOR of bits 22, 21, 20, 7    clocking bit 10   output bit 22
 * Key setup: all three start at 0.  For i = 0..63: clock all three, then XOR key bit (kc[i / 8] >> (i & 7)) & 1 into bit 0 of
 * each.  For i = 0..21: the same with (count >> i) & 1.  Then 100 majority-clocked steps whose output is thrown away: in a
 * majority-clocked step a register moves when its clocking bit equals the majority of the three clocking bits.
 * Output: 228 majority-clocked steps; after each, the output bit is the XOR of the three output bits.  BLOCK1 is the first 114
 * bits, BLOCK2 the next 114.
 * COUNT of a slot: (T1 << 11) | (T3 << 5) | T2 with T1 = FN / 1326, T3 = FN % 51, T2 = FN % 26, FN the slot's frame number in
 * [0, 2715648).  The downlink uses BLOCK1, the uplink BLOCK2, of the same COUNT for the same FN.
 * In a burst: keystream bit k goes to burst bit 3 + k for k < 57 and to burst bit 31 + k for k >= 57 -- the 2 x 57 payload bits
 * at 3..59 and 88..144.  The tail bits, the two stealing flags (60, 87) and the training sequence are never touched.
 * Known answer: kc = 12 23 45 67 89 AB CD EF, count = 0x134 gives, packed MSB first,
 *   BLOCK1 = 53 4E AA 58 2F E8 15 1A B6 E1 85 5A 72 8C 00      BLOCK2 = 24 FD 35 A3 5D 5F B6 52 6D 32 F9 06 DF 1A C0
 * kc = 0 with count = 0 gives an all-zero keystream (the registers never leave 0): a legal input, and a fixed point.
 *
 * Channel plan and numbering: exactly trxsig_l1rx_create's (trxsig_l1rx.h) -- h_comb[a][tn] of 0, 1 (I), 5 (V, TN 0 of ARFCN 0
 * only), 7 (VII); classes TRXSIG_L1_TCH and TRXSIG_L1_XCCH only, in (ARFCN, TN, sub-channel) order.  Every SDCCH and SACCH
 * sub-channel is a channel of its own with a key of its own: each belongs to another handset.
 *
 * Routing.  Slot t of ARFCN a of a call that starts at (fn, TN 0) has FN = (fn + t / 8) % 2715648 and TN = t % 8.  It belongs
 * to the TCH or XCCH channel whose GSM 05.02 mapping holds FN on that (ARFCN, TN): downlink, the tables trxsig_l1tx walks; uplink,
 * the ones trxsig_l1rx reads (both csrc/trxsig_tdma.h) -- the SACCH/TF position of a combination-I slot belongs to its SACCH, the
 * idle frame to nothing, and combination V's beacon and RACH frames to nothing.  A slot is ciphered when it belongs to a channel
 * whose algorithm is on.
 *
 * Everything is enqueued on the context's stream; nothing synchronises.  Bad arguments return TRXSIG_EINVAL before any launch.
 * The stage keeps no state between calls: one call of F frames equals any split of it at frame boundaries, bit for bit.
 * Thread safety: one caller at a time per object.
 */
#ifndef TRXSIG_L1CIPH_H
#define TRXSIG_L1CIPH_H

#include "trxsig_l1ms.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct trxsig_l1ciph trxsig_l1ciph;

enum { TRXSIG_A5_OFF = 0, TRXSIG_A5_1 = 1 };
#define TRXSIG_L1CIPH_STATE_BYTES 16 /* a channel's record: uint32 algo, R1, R2, R3 (the registers after the 64 key steps) */

/* The primitive: BLOCK1 and BLOCK2 of n (key, count) pairs, one bit per byte.  d_kc [n][8], d_count [n] (all 32 bits are
 * clocked in as stated; a COUNT has 22), d_block1 / d_block2 [n][114], either may be NULL (not both).  n == 0 is TRXSIG_OK with
 * no launch. */
int trxsig_a5_1_blocks_batch(trxsig_ctx *ctx, int n, const uint8_t *d_kc, const uint32_t *d_count, uint8_t *d_block1,
                             uint8_t *d_block2);

/* The object keeps ctx alive: trxsig_destroy on ctx takes effect when the object is gone too.  A new object has every channel
 * off. */
int trxsig_l1ciph_create(trxsig_l1ciph **out, trxsig_ctx *ctx, int n_arfcn, const uint8_t *h_comb);
void trxsig_l1ciph_destroy(trxsig_l1ciph *c);
/* as trxsig_l1rx_channels / trxsig_l1rx_channel, for TRXSIG_L1_TCH and TRXSIG_L1_XCCH (any other class: TRXSIG_EINVAL) */
int trxsig_l1ciph_channels(const trxsig_l1ciph *c, int cls);
int trxsig_l1ciph_channel(const trxsig_l1ciph *c, int cls, int chan, int *arfcn, int *tn, int *kind, int *sub);

/* One channel's algorithm and key, in stream order on the context's stream: the calls enqueued before it use the old key, the
 * ones after it the new.  algo: TRXSIG_A5_OFF (h_kc may be NULL) or TRXSIG_A5_1 (h_kc: 8 host bytes, read before the call
 * returns); anything else is TRXSIG_EINVAL.  The 64 key steps depend on the key alone: they run here, on the host, once, and the
 * three register words travel as the arguments of a one-thread kernel -- no staging copy, and the per-burst kernels start from
 * that state. */
int trxsig_l1ciph_set(trxsig_l1ciph *c, int cls, int chan, int algo, const uint8_t *h_kc);

/* the channels' records, for tests: device [n_chan][4] uint32 = algo, R1, R2, R3 after the key (zeros where off) */
int trxsig_l1ciph_state(trxsig_l1ciph *c, int cls, const uint32_t **d_state);

/* Cipher (or decipher: the same call) n_frames whole frames of burst bits in place.  d_bits is [n_arfcn][8 n_frames][148], one
 * bit per byte, 4-byte aligned: the layout of trxsig_l1tx_out.d_bits and trxsig_l1ms_out.d_bits, WHOSE const THE CALLER CASTS
 * AWAY ON PURPOSE -- the encoder's output is ciphered where it lies, before add_l1tx / radiate read it.  uplink: 0 = the
 * downlink's mapping and BLOCK1, 1 = the uplink's and BLOCK2.  fn in [0, 2715648), n_frames >= 1,
 * n_arfcn * 8 * n_frames <= 2^30.  Every ciphered slot gets bit ^= keystream on its 114 payload bits; every other byte keeps its
 * value.  d_what (or NULL) is the encoder's [n_arfcn][8 n_frames] map: only slots with (what_mask >> d_what[a][t]) & 1 are
 * eligible (codes above 31 never are) -- the downlink passes 1 << TRXSIG_L1TX_XCCH | 1 << TRXSIG_L1TX_TCH, the uplink
 * 1 << TRXSIG_L1MS_TCH | 1 << TRXSIG_L1MS_XCCH, so empty slots, idle fill, beacon channels and access bursts stay byte for byte. */
int trxsig_l1ciph_bits(trxsig_l1ciph *c, int uplink, int fn, int n_frames, uint8_t *d_bits, const uint8_t *d_what,
                       uint32_t what_mask);

/* Decipher a pull's soft bits IN PLACE, IN THE ROWS OF res (whose const is cast away on purpose): A RESULT IS DECIPHERED EXACTLY
 * ONCE -- a second call ciphers it again.  res is read as trxsig_l1rx_decode reads it: whole frames from TN 0 (n_slots a
 * multiple of 8, n_arfcn the object's), d_row, d_valid, d_soft, soft_stride, n_rows.  For every slot that has a row in
 * [0, n_rows) with d_valid set and that is ciphered, each of the 114 payload soft values whose keystream bit is 1 becomes
 * 1.0f - s (one float32 subtraction; NaN stays NaN).  All other rows and values keep their words.  Rows are taken to be distinct
 * (a pull gives every slot its own). */
int trxsig_l1ciph_soft(trxsig_l1ciph *c, int uplink, const trxsig_trxgroup_result *res, int fn);

#ifdef __cplusplus
}
#endif
#endif /* TRXSIG_L1CIPH_H */
