/* trxsig_air.h -- the air between the transmitters and the receivers of a cell, on the device: clean bursts in, received
 * samples out.  The link that l1tx -> (air) -> l1acq -> l1msrx -> l1ms -> radiate -> (air) -> pull -> l1rx lacked: per burst a
 * multipath channel, an oscillator offset and white Gaussian noise, in two forms.
 *   The cell form (uplink): slot cells -> slot cells in the layout trxsig_trxgroup_pull reads (what trxsig_l1ms_radiate writes).
 *   The stream form (downlink): a carrier's cells -> one continuous stream per handset with its own cut, delay, offset, gain
 *     and noise, in the layout trxsig_l1acq_search reads.
 * Every float32 operation of the signal path is stated below and is separately rounded (the library's numerical contract), so
 * a model that does the same operations in the same order reproduces every word.
 *
 * The noise generator (both forms).  Philox4x32-10 (Salmon et al., SC'11; the Random123 constants), key = the call's 64-bit
 * seed (low word, high word), counter = (i >> 1, row, plane, form):
 *   cell form:    i = the sample's index in its cell, row = (8 fn + t) mod (8 * 2715648), plane = the ARFCN, form = 0
 *   stream form:  i = n0 + n (uint32, wrapping),     row = the handset,                  plane = 0,         form = 1
 * An even i takes the words (w0, w1) of the block, an odd i (w2, w3).  From a pair (wa, wb):
 *   u = (2 (wa >> 9) + 1) 2^-24,  v = (2 (wb >> 9) + 1) 2^-24   (both exact in float32, inside (0, 1))
 *   r = sqrt(-2 ln u)  (at most 5.77),  g = (r cos 2 pi v, r sin 2 pi v)
 * Each component of g is N(0, 1); with d_sigma the complex noise power is 2 sigma^2.  The counter holds the absolute slot (or
 * n0), never a launch index: the values do not depend on the launch geometry, and a run cut into calls gives the samples of one
 * call.  ln, cos and sin are the kernel's own float32 arithmetic (an atanh series, polynomials on an octant of an exactly reduced
 * argument): every component of g is within 1e-5 of the exact value of the formulas above -- the bar the tests hold it to
 * against a float64 model.  (The context's 1,024-step trig table is good to 4.7e-6, 2.7e-5 at the largest r: it does not meet
 * that bar and is not used here.)
 *
 * Thread safety: one caller at a time per object.  Everything is enqueued on the context's stream; nothing synchronises.
 */
#ifndef TRXSIG_AIR_H
#define TRXSIG_AIR_H

#include "trxsig.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct trxsig_air trxsig_air;

#define TRXSIG_AIR_MAX_TAPS 32

/* max_taps in 1..TRXSIG_AIR_MAX_TAPS: the longest channel a cell call may name.  The object keeps ctx alive: trxsig_destroy on
 * ctx takes effect when the object is gone too. */
int trxsig_air_create(trxsig_air **out, trxsig_ctx *ctx, int max_taps);
void trxsig_air_destroy(trxsig_air *air);

/* Per-cell parameters of the cell form: device arrays indexed [a][t], t = 0 .. 8 n_frames - 1.  A NULL array skips its stage
 * (skipping is not multiplying by one: the words pass through untouched). */
typedef struct {
  const trxsig_c32 *d_taps;   /* [a][t][n_taps]: the burst's channel (block fading: other taps per cell); NULL: no multipath */
  int n_taps;                 /* 1 .. the object's max_taps (read only with d_taps) */
  const uint32_t *d_step;     /* [a][t]: oscillator step per sample, in 2^-32 turn; NULL: no offset */
  const uint32_t *d_phase;    /* [a][t]: phase of sample 0, in 2^-32 turn; NULL (with d_step set): 0 */
  const float *d_sigma;       /* [a][t]: noise standard deviation per real component; NULL: no noise */
} trxsig_air_cell_params;

/* The cell form.  Slot t (of 8 n_frames, t = 0 at TN 0 of frame fn) of ARFCN a is at base + t * slot_stride + a * arfcn_stride
 * and holds N = (156 + (t % 4 == 0)) * sps samples; nothing outside the N samples is read or written.  Per cell, in float32:
 *   1. u = convolve(x, h, START_ONLY): u[i] = sum over j < n_taps, j ascending, of x[i-j] * h[j] (Complex<float>::operator*: four
 *      rounded products, a rounded difference and a rounded sum), the terms with i - j < 0 left out.  Non-finite taps give
 *      unspecified values.
 *   2. v[i] = u[i] * expjLookup((float)(p_i >> 8) * 2^-24f * (float)(2 pi)), p_i = d_phase + i * d_step in uint32 wrap-around
 *      arithmetic (an NCO: exact, no float phase chain), frequencyShift's operand order.
 *   3. w[i] = v[i] + sigma * g[i]: one rounded product and one rounded sum per component.
 *   4. out[i] = w[i], or out[i] + w[i] with accumulate != 0 (co-channel interferers, colliding access bursts).
 * Empty cells (zeros in) still receive noise.  d_out may be exactly d_in with d_in's strides; otherwise the two regions (first
 * cell to the end of the last) must not overlap.  One launch (k_air_cells).  TRXSIG_EINVAL before any launch: NULL object, params
 * or buffers, n_arfcn outside 1..65535, n_frames outside 1..2^24, fn outside [0, 2715648), n_taps out of range, strides under which
 * cells overlap (the rule trxsig_l1ms_radiate, trxsig_l1trk_slice and trxsig_l1hop_cells share: slot_stride and arfcn_stride at least 157 sps apart, in either nesting), out
 * overlapping in without being identical. */
int trxsig_air_cells(trxsig_air *air, int fn, int n_arfcn, int n_frames, uint64_t seed, const trxsig_c32 *d_in, int64_t in_slot_stride,
                     int64_t in_arfcn_stride, const trxsig_air_cell_params *params, trxsig_c32 *d_out, int64_t out_slot_stride,
                     int64_t out_arfcn_stride, int accumulate);

/* Per-handset parameters of the stream form: device arrays [n_handsets].  d_arfcn and d_cut are required; a NULL array among
 * the others skips its stage. */
typedef struct {
  int n_arfcn;                /* carriers in d_in; a handset whose d_arfcn is outside [0, n_arfcn) hears none (zeros) */
  const int32_t *d_arfcn;     /* the carrier the handset listens to */
  const int64_t *d_cut;       /* where its stream starts in the (delayed) carrier, in samples; may be negative */
  const float *d_delay;       /* path delay in samples; NULL: none */
  const uint32_t *d_step;     /* oscillator step per sample / phase of its sample 0, in 2^-32 turn; d_step NULL: no offset */
  const uint32_t *d_phase;
  const trxsig_c32 *d_gain;   /* path gain; NULL: none */
  const float *d_sigma;       /* noise standard deviation per real component; NULL: no noise */
  const uint32_t *d_n0;       /* index of its sample 0 in its noise sequence; NULL: 0 */
} trxsig_air_stream_params;

/* The stream form.  Carrier a's clean stream c_a is the concatenation of its cells t = 0 .. n_cells - 1 (cell 0 is TN 0:
 * 157 / 156 / 156 / 156 sps samples per four slots), cells addressed as in the cell form.  For handset h, n < len:
 *   z = delayVector(c_a, delay) over the whole stream: integer part by floor, the 21-tap un-windowed sinc of the context's table
 *       where |frac| > 1e-2, zero fill (a delay beyond +-TRXSIG_MAX_INDEX or not finite: zeros, as trxsig_delay_vector_batch)
 *   out[h * out_stride + n] = (z[cut + n] * e(d_phase + n * d_step)) * gain + sigma * g[n0 + n]
 * with the cell form's rotation, scaleVector's complex product and the noise sum; positions outside the stream read as zero.
 * One launch (k_air_stream).  TRXSIG_EINVAL before any launch: NULL object, params, d_arfcn, d_cut or buffers, n_cells <= 0 or a
 * stream of 2^31 samples or more, n_handsets outside 1..65535, len <= 0, out_stride < len, strides under which cells overlap,
 * out overlapping in. */
int trxsig_air_stream(trxsig_air *air, int n_cells, uint64_t seed, const trxsig_c32 *d_in, int64_t slot_stride, int64_t arfcn_stride,
                      int n_handsets, const trxsig_air_stream_params *params, int len, trxsig_c32 *d_out, int64_t out_stride);

#ifdef __cplusplus
}
#endif
#endif /* TRXSIG_AIR_H */
