/* trxsig_l1hop.h -- slow frequency hopping for dedicated channels on the device (GSM 05.02 section 6.2.3): the second of the two
 * things GSM puts around a dedicated channel's bursts, after ciphering (trxsig_l1ciph.h).  In both directions:
 *   l1tx_encode -> l1ciph_bits -> BITS(to radio) -> add_l1tx -> ... -> pull -> RESULT -> l1ciph_soft -> l1msrx_decode
 *   l1ms_encode -> l1ciph_bits -> radiate -> CELLS(to radio) -> air_cells -> pull -> RESULT -> l1ciph_soft -> l1rx_decode
 * THIS STAGE HAS NO REFERENCE COUNTERPART (the reference never hops).  Every output is exact and equal to tests/l1_hop_model.py.
 *
 * The algorithm, as this project states it.  Inputs: FN in [0, 2715648), HSN in 0..63, MAIO in 0..N-1, N in 1..64 (the number of
 * frequencies in the mobile allocation).  T1 = FN / 1326, T2 = FN % 26, T3 = FN % 51, T1R = T1 % 64, NBIN = the number of bits of
 * N = floor(log2 N) + 1 (N = 4 gives 3, N = 64 gives 7).
 *   HSN == 0:  MAI = (FN + MAIO) mod N                                   (cyclic hopping)
 *   else:      M  = T2 + RNTABLE[(HSN xor T1R) + T3]
 *              M' = M mod 2^NBIN,  T' = T3 mod 2^NBIN
 *              S  = M' if M' < N else (M' + T') mod N
 *              MAI = (S + MAIO) mod N
 * RNTABLE, 114 entries, index 0..113:
 *    48  98  63   1  36  95  78 102  94  73     0  64  25  81  76  59 124  23 104 100
 *   101  47 118  85  18  56  96  86  54   2    80  34 127  13   6  89  57 103  12  74
 *    55 111  75  38 109  71 112  29  11  88    87  19   3  68 110  26  33  31   8  45
 *    82  58  40 107  32   5 106  92  62  67    77 108 122  37  60  66 121  42  51 126
 *   117 114   4  90  43  52  53 113 120  72    16  49   7  79 119  61  22  84   9  97
 *    91  15  21  24  46  39  93 105  65  70   125  99  17 123
 * (114 distinct values, all <= 127, sum 7446, CRC-32 of the 114 bytes 0xED53E222; 10, 14, 20, 27, 28, 30, 35, 41, 44, 50, 69, 83,
 * 115 and 116 do not occur.)
 * Known answers.  THEY WERE COMPUTED FROM THE STATEMENT ABOVE AND PIN THIS READING OF IT, NOT THE STANDARD, which publishes no
 * test vector:
 *   HSN 1,  MAIO 0, N 4,  FN 0..19                     ->  2 0 3 2 3 3 2 0 1 1 2 3 1 1 1 3 3 1 0 0
 *   HSN 63, MAIO 2, N 64, FN 83578..83589 (T1 = 63)    ->  47 41 7 57 45 9 6 52 35 34 35 11
 * S depends on (FN, HSN, N) only: channels that share an allocation and an HSN and have distinct MAIOs never collide -- in every
 * frame the map is a rotation of the allocation.  The design relies on that.
 *
 * The plan.  h_comb[a][tn] in trxsig_l1rx_create's numbering (0, 1 (I), 5 (V, TN 0 of ARFCN 0 only), 7 (VII)); h_group[a][tn]
 * (int8): -1 where the slot does not hop, else a group id in [0, n_groups); h_hsn[g].  The allocation of group g on timeslot tn
 * is the set of rows a with h_group[a][tn] == g, in ascending a; N is its size; a row's MAIO is its rank in that list; the
 * frequency with index MAI is the row of rank MAI.  A channel-domain row is what the encoders and decoders call an ARFCN; a
 * radio-domain row is what the group, the air and the pull call one: in slot (tn, FN), channel row a of rank r is on the radio
 * row of rank (S + r) mod N.
 * TRXSIG_EINVAL at create: N > 64 on any (g, tn); an HSN outside 0..63; a group id outside -1..n_groups-1; members of one
 * (g, tn) whose combinations differ; a member whose combination is 0 or 5.  (The pull's expected burst type is per radio row, so
 * a burst that hops onto an OFF row would never be demodulated; a beacon slot does not hop.)
 *
 * The order of the stages is part of the contract: ciphering is in the channel domain.  On transmit, hop after
 * trxsig_l1ciph_bits; on receive, call trxsig_l1hop_result before trxsig_l1ciph_soft.
 *
 * Everything is enqueued on the context's stream; nothing synchronises, and no call allocates.  Bad arguments return
 * TRXSIG_EINVAL before any launch.  The stage keeps no state between calls: one call of F frames equals any split of it at frame
 * boundaries, word for word.  Every kernel computes the sequence itself; none reads the array trxsig_l1hop_map returns.
 * Out of scope: hopping of the beacon slot, MAIOs other than by rank, synthesiser settling, handover.
 * Thread safety: one caller at a time per object.
 */
#ifndef TRXSIG_L1HOP_H
#define TRXSIG_L1HOP_H

#include "trxsig_l1ms.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct trxsig_l1hop trxsig_l1hop;

#define TRXSIG_L1HOP_MAX_N 64 /* frequencies in a mobile allocation */

/* The primitive: d_mai[i] = MAI(d_fn[i], d_hsn[i], d_maio[i], d_n[i]), device int32 arrays of n entries, one lane per entry.
 * n in 0..2^24; n == 0 is TRXSIG_OK with no launch.  AN ENTRY WHOSE INPUTS ARE OUT OF THE RANGES ABOVE IS UNDEFINED (the host
 * cannot see device values): it may read outside RNTABLE or divide by zero. */
int trxsig_hop_mai_batch(trxsig_ctx *ctx, int n, const int32_t *d_fn, const int32_t *d_hsn, const int32_t *d_maio, const int32_t *d_n,
                         int32_t *d_mai);

/* h_comb and h_group are [n_arfcn][8] host arrays, h_hsn [n_groups] (may be NULL with n_groups == 0: nothing hops); n_groups in
 * 0..128, n_arfcn in 1..65535.  max_frames >= 1, n_arfcn * 8 * max_frames <= 2^30: the longest call of trxsig_l1hop_map and
 * trxsig_l1hop_result, whose arrays are allocated here.  The object keeps ctx alive: trxsig_destroy on ctx takes effect when the
 * object is gone too. */
int trxsig_l1hop_create(trxsig_l1hop **out, trxsig_ctx *ctx, int n_arfcn, const uint8_t *h_comb, const int8_t *h_group, int n_groups,
                        const uint8_t *h_hsn, int max_frames);
void trxsig_l1hop_destroy(trxsig_l1hop *h);
/* the number of groups */
int trxsig_l1hop_groups(const trxsig_l1hop *h);
/* N of group g on timeslot tn (0 where it has no member there), and, with h_rows != NULL, its rows in ascending order (room for
 * TRXSIG_L1HOP_MAX_N) */
int trxsig_l1hop_members(const trxsig_l1hop *h, int g, int tn, int32_t *h_rows);

/* The radio row of every channel row: *d_radio is an object-owned device array [8 n_frames][n_arfcn], entry [t][a] the radio row
 * of channel row a in slot t of a call that starts at (fn, TN 0) -- a itself where the slot does not hop.  Valid until the next
 * trxsig_l1hop_map.  fn in [0, 2715648), 1 <= n_frames <= max_frames.  For tests and for callers that hop arrays of their own. */
int trxsig_l1hop_map(trxsig_l1hop *h, int fn, int n_frames, const int32_t **d_radio);

/* Hop n_frames whole frames of burst bits IN PLACE.  d_bits is [n_arfcn][8 n_frames][148], 4-byte aligned, and d_what (or NULL)
 * the [n_arfcn][8 n_frames] map that goes with it: trxsig_l1tx_out's and trxsig_l1ms_out's, WHOSE const THE CALLER CASTS AWAY
 * ON PURPOSE, as for trxsig_l1ciph_bits.  to_radio != 0: slot (radio(a, t), t) receives what slot (a, t) held; to_radio == 0:
 * the inverse.  Slots that do not hop keep every byte.  fn in [0, 2715648), n_frames >= 1, n_arfcn * 8 * n_frames <= 2^30.
 * The downlink's form: l1tx_encode -> l1ciph_bits -> l1hop_bits -> add_l1tx. */
int trxsig_l1hop_bits(trxsig_l1hop *h, int to_radio, int fn, int n_frames, uint8_t *d_bits, uint8_t *d_what);

/* The same move on sample cells, OUT OF PLACE, addressed exactly as trxsig_air_cells addresses them: slot t (of 8 n_frames, t = 0
 * at TN 0 of frame fn) of row a is at base + t * slot_stride + a * arfcn_stride and holds N = (156 + (t % 4 == 0)) * sps samples
 * (sps is the context's); nothing outside the N samples is read or written.  Every cell of d_out is written: cells that do not
 * hop are copied.  The words move untouched (NaN payloads included).  TRXSIG_EINVAL: NULL, fn or n_frames out of range (as
 * trxsig_l1hop_bits), strides under which cells overlap (trxsig_air_cells' rule, in either nesting), d_out's region overlapping
 * d_in's.  Cells are moved 16 bytes a lane where both bases are 16-byte aligned and all four strides even, 8 bytes a lane
 * otherwise.  The uplink's form after trxsig_l1ms_radiate (whose gains and delays are per channel, so its bits cannot be hopped
 * first); trxsig_air_cells' per-frequency fading then applies in the radio domain.  With to_radio == 0 it is what a hopping
 * handset's synthesiser does to the downlink carriers before trxsig_air_stream cuts its stream. */
int trxsig_l1hop_cells(trxsig_l1hop *h, int to_radio, int fn, int n_frames, const trxsig_c32 *d_in, int64_t in_slot_stride,
                       int64_t in_arfcn_stride, trxsig_c32 *d_out, int64_t out_slot_stride, int64_t out_arfcn_stride);

/* Dehop a pull without moving a soft bit: *out = *res with d_row replaced by an object-owned [n_slots][n_arfcn] array,
 * out->d_row[t][a] = res->d_row[t][radio(a, t)].  Valid until the object's next trxsig_l1hop_result.  res: whole frames from TN 0
 * of frame fn (n_slots a positive multiple of 8, at most 8 max_frames), n_arfcn the object's, d_row not NULL.
 * trxsig_l1ciph_soft, trxsig_l1rx_decode and trxsig_l1msrx_decode take out as they take any result.  The per-ARFCN energy
 * threshold stays with the radio frequency, where it physically belongs; RSSI and timing follow the channel. */
int trxsig_l1hop_result(trxsig_l1hop *h, int fn, const trxsig_trxgroup_result *res, trxsig_trxgroup_result *out);

#ifdef __cplusplus
}
#endif
#endif /* TRXSIG_L1HOP_H */
