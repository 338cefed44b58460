/* trxsig_l1trk.h -- the handset's tracking receiver on the device: from the continuous streams trxsig_air_stream hands every
 * handset, and the grid trxsig_l1acq_search found in them, to the slot cells trxsig_trxgroup_pull reads -- and, call after call,
 * the frequency and timing corrections that keep the grid on a drifting oscillator and a drifting sample clock.  The link of
 *   l1tx -> modulate -> air_stream -> l1acq_search -> L1TRK -> pull -> l1msrx_decode
 * between "synchronised" and "reads the BCCH".  Per call it does three things:
 *   slice    cuts the streams on the tracked grid into slot cells, derotated by an exact NCO, and measures the residual frequency
 *            offset on every frequency-correction burst (FCCH) it passes -- one launch, k_l1trk_slice, one read of the stream;
 *   update   reads the timing error from the TOAs the pull of those cells reports and moves the grid, and steers the NCO by the
 *            FCCH measurements (the AFC) -- one small launch, k_l1trk_update.
 * THIS STAGE HAS NO REFERENCE COUNTERPART (the reference is a base station).  Its cells are the reference's arithmetic
 * (expjLookup, Complex<float>::operator*), word for word equal to tests/l1_trk_model.py; its integer rules are exact; its FCCH
 * sums are held to a bound against float64 that follows from the roundings stated below.
 *
 * Columns and phones.  Columns are receivers: column c is one carrier as one phone hears it, and becomes "ARFCN" c of the group
 * pull.  Phones are oscillators: every column belongs to one phone (h_phone[c]).  At most one column of a phone is its C0 column
 * (h_c0[p], -1: none), the one that hears a combination-V TN 0: FCCH bursts in frames with FN % 51 in {0, 10, 20, 30, 40}.
 *
 * State, per phone, on the device: an anchor and three counters / flags.
 *   fn (int32)      the frame the anchor refers to
 *   pos (int64)     the ABSOLUTE stream sample of sample 0 of TN 0 of frame fn (absolute: counted from sample 0 of the stream the
 *                   search was given; a later buffer says where it starts with n0)
 *   phase (uint32)  the NCO's phase at sample pos, in 2^-32 turn
 *   step (uint32)   the NCO's step, in 2^-32 turn per sample
 *   locked (uint8), quiet (int32: updates in a row that had nothing to go by)
 *
 * Seeding (trxsig_l1trk_seed, device to device).  For phone p with s = d_src[p] >= 0 (negative, or not a stream of acq: the phone
 * is left as it is), in double, where acq's d_state[s] == 15:
 *   K = 4294967296.0 / 6.283185307179586
 *   pos0 = (int64) floor((double) d_sch_w0[s] + (double) d_sch_toa[s] + 0.5),   pos = pos0 + 1250 sps
 *   fn = (d_rfn[s] + 1) mod 2715648,   step = (uint32)(int64) llrint((double) d_omega[s] * K)
 *   phase = 0, quiet = 0, locked = 1
 * and any other state leaves locked = 0 (the rest untouched).  d_omega is the shift the search applied: it has the sign wanted.
 *
 * Slice.  Column c's buffer starts at d_streams + c * stream_stride and holds the absolute samples [n0, n0 + n_samples).  For
 * phone p, with H = 2715648:
 *   D = the signed shortest distance from the anchor's fn to the call's fn modulo H:  ((fn - anchor.fn) mod H), less H where
 *       that is H / 2 or more
 *   P = pos + D * 1250 sps,   PH = phase + (uint32)(D * 1250 sps) * step   (uint32 wrap-around arithmetic)
 * Cell t, t = 0 .. 8 n_frames - 1, lies at d_cells + t * slot_stride + c * col_stride, has (156 + (t % 4 == 0)) sps samples and
 * starts at stream offset s_t, the sum of the lengths of the cells before it.  Its sample i is
 *   x[P + s_t + i - n0] * expjLookup((float)(ph >> 8) * 2^-24f * (float)(2 pi)),   ph = PH + (uint32)(s_t + i) * step
 * -- trxsig_air.h's NCO, frequencyShift's operand order, every product and sum separately rounded.  A position outside
 * [0, n_samples) is not read: the cell gets (+0, +0) there and the column's TRXSIG_TRK_CLIPPED bit is set in d_status.  The
 * columns of a phone that is not locked get (+0, +0) everywhere and TRXSIG_TRK_UNLOCKED.  Nothing outside a cell's samples is
 * written.  After the call a locked phone's anchor is (fn + n_frames, P + n_frames * 1250 sps, PH + (uint32)(n_frames * 1250 sps)
 * * step): one call of F frames equals any split of it, bit for bit.
 *
 * The AFC measurement (the same launch; the workgroup that forms the cell keeps it in LDS: the stream is read once).  For every
 * frame f of the call with (fn + f) % 51 in {0, 10, 20, 30, 40} and every phone with a C0 column, on the derotated TN 0 cell y of
 * that column, L = 142 sps, n = 3 sps .. 3 sps + L - 1:
 *   d[n] = y[n + sps] conj(y[n]) (-j)        e[n] = 0.5 (|y[n]|^2 + |y[n + sps]|^2)
 * in float32, unfused, as trxsig_l1acq.h's stage 1 forms them (three roundings per component); C = sum d and E = sum e in
 * float64, in any order.  Record j of the phone (j counts the call's FCCH frames) carries the frame, C, E and
 *   ok = Re C > 0 and E > 0 and C, E finite and |C|^2 / E^2 > fcch_thresh   (in double)
 * C and E are the sums of the float32 terms, not of exact ones: a term that is not finite in float32 (a sample above about
 * 1.8e19 in modulus overflows e[n]; a NaN or Inf sample) makes its sum Inf or NaN and gives ok = 0 even where the exact sum
 * would be finite, and terms that underflow to 0 give E = 0 and ok = 0.
 * A phone that is not locked gets C = E = 0, ok = 0; a phone without a C0 column has no records (its entries stay zero).
 *
 * Update.  res is the pull of the cells just sliced (res->n_arfcn == n_cols; fn and res->n_slots those of the last slice, and
 * one update per slice: TRXSIG_EINVAL otherwise).  Per locked phone:
 *   timing     over slots t and the phone's columns c with a row (d_row[t][c] >= 0) whose d_valid is set, d_use[t][c] != 0 where
 *              d_use is given, EXCEPT the C0 column's TN 0 in frames with FN % 51 in {0, 1, 10, 11, 20, 21, 30, 31, 40, 41} (the
 *              pull's midamble detector has no business on an FCCH or SCH burst) and rows with |q| > toa_gate:
 *                q = llrint((double) toa * (256 / sps))      (exact: 256 / sps is a power of two; a TOA that is not finite is
 *                                                             excluded as beyond the gate)
 *                S = sum q,  N = the count                   (integers: any order, exact)
 *              N >= 1:  adj = floor((2 S sps + 256 N) / (512 N))  -- S sps / (256 N) samples, rounded half up --
 *                       pos += adj,  phase += (uint32) adj * step  (the step BEFORE this update's AFC: the NCO is continuous in
 *                       absolute time)
 *   frequency  over the ok records of the last slice, K of them, in record order, in double: SC = sum C.  K >= 1:
 *                a = acq_atan2((float) Im SC, (float) Re SC)   (trxsig_l1acq's own arctangent, within 2e-6)
 *                delta = llrint((double)(-a) / sps * K_turn)   (K_turn = the seed's K)
 *                step += (uint32)(delta >> afc_shift)          (an arithmetic shift: floor)
 *   quiet      0 where N + K > 0, else quiet + 1.  Losing lock is the caller's decision: locked does not change.
 * A phone that is not locked is left alone (its sums read 0).
 *
 * Deliberately outside: timing from the SCH bursts (the cells are there for trxsig_l1acq_detect_sch_batch), re-acquisition,
 * multipath, the int16 route.
 *
 * Everything is enqueued on the context's stream; nothing synchronises.  Thread safety: one caller at a time per object.
 */
#ifndef TRXSIG_L1TRK_H
#define TRXSIG_L1TRK_H

#include "trxsig_l1acq.h"
#include "trxsig_trxgroup.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct trxsig_l1trk trxsig_l1trk;

#define TRXSIG_L1TRK_MAX_FRAMES 65536            /* the most frames one slice may take */
#define TRXSIG_L1TRK_MAX_GATE (1 << 24)          /* the widest toa_gate, in 1/256 symbol */

/* d_status bits */
enum { TRXSIG_TRK_CLIPPED = 1,       /* part of the column's span lay outside the buffer: zeros there */
       TRXSIG_TRK_UNLOCKED = 2 };    /* the column's phone is not locked: zeros everywhere */

/* n_phones, n_cols in 1..65535; h_phone[c] in [0, n_phones); h_c0[p] -1 or a column of phone p (host arrays, copied);
 * max_frames in 1..TRXSIG_L1TRK_MAX_FRAMES; afc_shift in 0..8; toa_gate in 1..TRXSIG_L1TRK_MAX_GATE, in 1/256 symbol;
 * fcch_thresh as trxsig_l1acq_search's.  Every phone starts unlocked.  The object keeps ctx alive: trxsig_destroy on ctx takes
 * effect when the object is gone too. */
int  trxsig_l1trk_create(trxsig_l1trk **out, trxsig_ctx *ctx, int n_phones, int n_cols, const int32_t *h_phone /* [n_cols] */,
                         const int32_t *h_c0 /* [n_phones], -1: none */, int max_frames, int afc_shift /* 0..8 */,
                         int toa_gate /* 1/256 symbol, > 0 */, float fcch_thresh);
void trxsig_l1trk_destroy(trxsig_l1trk *trk);

/* d_src: device array [n_phones], the stream of acq's last search that phone p was acquired on, -1: leave the phone as it is */
int  trxsig_l1trk_seed(trxsig_l1trk *trk, const trxsig_l1acq_out *acq, const int32_t *d_src);
/* host scalars, enqueued: a caller that already knows the grid (fn in [0, 2715648)); quiet = 0 */
int  trxsig_l1trk_set(trxsig_l1trk *trk, int phone, int locked, int fn, int64_t pos, uint32_t step, uint32_t phase);

/* The device arrays, one entry per phone, owned by the object.  The anchor's three arrays alternate between two sets: the
 * pointers are those of the anchor as it stands after the calls made so far, and are valid until the next slice. */
typedef struct {
  int n_phones, n_cols;
  const int32_t *d_fn;
  const int64_t *d_pos;
  const uint32_t *d_phase, *d_step;
  const uint8_t *d_locked;
  const int32_t *d_quiet;
  /* what the last update did */
  const int64_t *d_toa_sum;            /* S */
  const int32_t *d_toa_n;              /* N */
  const int64_t *d_adj;                /* adj, 0 where N = 0 */
  const int32_t *d_afc_n;              /* K */
  const int64_t *d_afc_delta;          /* delta before the shift, 0 where K = 0 */
} trxsig_l1trk_view;
int  trxsig_l1trk_state(trxsig_l1trk *trk, trxsig_l1trk_view *out);

/* What one slice leaves, owned by the object, valid until its next slice */
typedef struct {
  int n_phones, n_cols;
  int n_fcch;                          /* FCCH frames in the call: records 0 .. n_fcch - 1 of every phone with a C0 column */
  int fcch_stride;                     /* records per phone in the arrays below */
  const uint8_t *d_status;             /* [n_cols] TRXSIG_TRK_* */
  const int32_t *d_fcch_fn;            /* [n_phones][fcch_stride] */
  const double *d_fcch_c;              /* [n_phones][fcch_stride][2]: Re C, Im C */
  const double *d_fcch_e;              /* [n_phones][fcch_stride] */
  const uint8_t *d_fcch_ok;            /* [n_phones][fcch_stride] */
} trxsig_l1trk_meas;

/* TRXSIG_EINVAL before any launch: NULL object, buffers or out; n_frames outside 1..max_frames; fn outside [0, 2715648);
 * n_samples <= 0 or >= 2^31; stream_stride < n_samples; cell strides under which cells overlap (trxsig_l1ms_radiate's rule:
 * slot_stride and col_stride at least 157 sps apart, in either nesting); cells overlapping the streams. */
int  trxsig_l1trk_slice(trxsig_l1trk *trk, const trxsig_c32 *d_streams, int64_t stream_stride, int64_t n0, int n_samples,
                        int fn, int n_frames, trxsig_c32 *d_cells, int64_t slot_stride, int64_t col_stride,
                        trxsig_l1trk_meas *out);

/* d_use: device array [n_slots][n_cols] (0: the row is not used for timing), or NULL: every row may be */
int  trxsig_l1trk_update(trxsig_l1trk *trk, const trxsig_trxgroup_result *res, int fn, const uint8_t *d_use);

#ifdef __cplusplus
}
#endif
#endif /* TRXSIG_L1TRK_H */
