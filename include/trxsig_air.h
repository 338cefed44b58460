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
 * The channel itself can come from the library too: trxsig_air_fade (below) writes the cell form's d_taps from a time-varying,
 * frequency-selective multipath model.
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

/* ---- Time-varying multipath: the fading-tap generator -------------------------------------------------------------------------
 * Writes the [a][t][n_taps] array that trxsig_air_cell_params.d_taps reads: per cell the taps of a tapped-delay-line channel
 * whose paths fade as sums of sinusoids (Clarke's model by Monte Carlo arrival angles, plus an optional line-of-sight term), with
 * the noise generator's property: counter-based, a function of (seed, link, path, absolute slot, column) and of nothing else.  A
 * run cut into calls gives the taps of one call; the launch geometry does not matter.  Every integer rule below is exact.
 *
 * Link.  One transmitter-receiver pair with its own fading process.  d_link[a][t] (int32, device) names the link of each cell;
 *   NULL: link = 8 a + (t % 8).  A link outside [0, n_links) gives a cell whose taps are all +0.  With hopping the caller gives a
 *   handset one link id on whichever radio row it lands on (trxsig_l1hop_map tells where).
 * Time.  row = (8 fn + t) mod (8 * 2715648), the noise generator's row; slots are taken as equally long (the 157-symbol slots are
 *   not told apart).  The process jumps at the hyperframe's wrap, as the noise row does: row 0 follows row 8 * 2715648 - 1.
 * Profile (caller data; no GSM 05.05 table is in the library).  P paths, 1 <= P <= 12, each with a delay in integer nanoseconds
 *   (0 .. 10^6), a power (finite, >= 0), optionally a line-of-sight share of that power in [0, 1] and the line-of-sight arrival
 *   cosine in Q23 (|.| <= 2^23); S diffuse sinusoids per path, 1 <= S <= 32.
 * Per (link l, path p, sinusoid s), s = 0 .. S: one Philox4x32-10 block, key = the call's seed, counter = (s, p, l, 2)  (form 2;
 *   the cell form of the noise uses 0, the stream form 1).
 *     phi  = w0, a phase in 2^-32 turn
 *     k    = 2 (w1 >> 9) + 1;  c = cos(2 pi k 2^-24) by the separately rounded float32 steps of the noise's cosine
 *     C    = (int) rintf(c * 2^23)  (ties to even; |C| <= 2^23).  The line-of-sight sinusoid is s = S: its phi is its own block's
 *            w0, its C the profile's Q23 cosine.
 *     step = (int32) (((int64) C * D_l) >> 23)  (an arithmetic shift: towards minus infinity), D_l = d_doppler[l] & 0x7fffffff:
 *            the link's maximum Doppler shift in 2^-32 turn per slot, a uint32 below 2^31 (the top bit is not read).
 * Path gain.  theta = phi + row * step in uint32 wrap-around arithmetic; e(theta) = (cos, sin) of the top 24 bits of theta by
 *   the same float32 steps (a phase of 0 gives exactly (1, 0)); each component of e is within 1e-5 of the exact value.
 *     g_p = a_p (e(theta_0) + e(theta_1) + ... + e(theta_{S-1})) + b_p e(theta_S)
 *   the sum a chain of S - 1 rounded float32 additions per component in the order s = 0, 1, .., S - 1, then per component two
 *   rounded products and a rounded sum.  a_p = sqrt(power_p (1 - los_p) / S), b_p = sqrt(power_p los_p), computed on the host in
 *   double from the float32 arguments and rounded once to float32.
 * Frequency selectivity.  trxsig_air_fade_columns gives column a its carrier offset f_a in kHz (|f_a| <= 10^7; before the first
 *   call: 1,024 columns at 200 a).  With hopping these are the radio rows.  Per (column, path) the host forms the phase
 *   -f_a tau_p 10^-6 turn exactly in integers: r = (-f_a tau_p) mod 10^6 in [0, 10^6), rot = (r 2^32 + 500000) div 10^6 mod 2^32
 *   (rounded once, halves up).  The kernel multiplies g_p by e(rot): four rounded products, a rounded difference and a rounded sum.
 * Projection onto taps.  The host computes w[p][j], j < n_taps, in double, rounded to float32: with
 *   x = j - centre - tau_p sps 13 / 48000  (samples; 48000 x is an integer and is formed as one),
 *     w = 1 where x = 0, 0 where x is another whole number or |x| >= 4, else sin(pi x) / (pi x) * (0.5 + 0.5 cos(pi x / 4))
 *   (a Hann-windowed sinc of half-width 4 samples).  A path whose delay is a whole number of samples has exactly one non-zero
 *   weight, 1.0f.  centre in 0..8 is the caller's bulk delay; centre = 0 truncates the precursors (the receiver's TOA absorbs the
 *   rest).  tap[j] = sum over p, ascending, of (g_p rotated) * w[p][j]: per component a rounded product and a rounded sum, the
 *   first term starting the sum.
 * Error bound (what the tests hold the taps to against a float64 evaluation of the formulas above from the same integers).  With
 *   d = 1e-5 (the promise for e), u = 2^-24, G_p = S a_p + b_p (no component of g_p exceeds it):
 *     E_p = a_p (S d + S^2 u) + b_p d + 3 u G_p                 per component of g_p: the trig errors, the chain's and g_p's roundings
 *     R_p = 2 E_p + 2 G_p d + 6 u G_p                           ... after the rotation (each component sums two products)
 *     |tap[j] - exact| <= sum_p |w[p][j]| (R_p + 2 G_p (2 u + (P + 1) u))   per component
 *   (2 u: w within one float32 spacing of its formula, whichever libm made it; (P + 1) u: the product and the P - 1 sums).
 * Out of scope: the stream form (a fading downlink needs a per-handset copy of the carrier through trxsig_air_cells); variation
 *   inside a burst (block fading: one set of taps per cell); correlated shadowing; antenna diversity. */

#define TRXSIG_AIR_FADE_MAX_PATHS 12
#define TRXSIG_AIR_FADE_MAX_SINUSOIDS 32
#define TRXSIG_AIR_FADE_MAX_COLUMNS 1024

/* Sets the profile, in stream order (as trxsig_l1ciph_set: launches enqueued before see the old one, launches after the new).
 * h_* are host arrays [n_paths]; h_los_share and h_los_cos_q23 may be NULL (no line of sight / cosine 0).  n_taps in
 * 1..the object's max_taps is the length of the taps trxsig_air_fade then writes.  The first call allocates the object's only
 * device block.  TRXSIG_EINVAL: NULL object, delays or powers, a count or a path value outside the ranges above. */
int trxsig_air_fade_profile(trxsig_air *air, int n_paths, const int32_t *h_delay_ns, const float *h_power, const float *h_los_share,
                            const int32_t *h_los_cos_q23, int n_sinusoids, int n_taps, int centre);

/* Sets the columns' carrier offsets (host int32 [n_arfcn], kHz), in stream order; n_arfcn in 1..1024 is from then on the most
 * columns a trxsig_air_fade call may name.  TRXSIG_EINVAL: NULL object or array, n_arfcn or an offset out of range. */
int trxsig_air_fade_columns(trxsig_air *air, int n_arfcn, const int32_t *h_col_khz);

/* d_taps[a][t][n_taps] for a < n_arfcn, t < 8 n_frames, t = 0 at TN 0 of frame fn.  d_link: int32 [a][t] or NULL; d_doppler:
 * uint32 [n_links].  One launch (k_air_fade); nothing synchronises.  Two taps leave in one 16-byte store where n_taps is even and
 * d_taps is 16-byte aligned.  TRXSIG_EINVAL before any launch: NULL object, d_doppler or d_taps, no profile set, n_arfcn outside
 * 1..the columns set, n_frames outside 1..2^24, fn outside [0, 2715648), n_links outside 1..2^30. */
int trxsig_air_fade(trxsig_air *air, int fn, int n_arfcn, int n_frames, uint64_t seed, const int32_t *d_link, int n_links,
                    const uint32_t *d_doppler, trxsig_c32 *d_taps);

/* The integers behind the taps: d_phase (uint32) and d_step (int32), both [n_links][P][S + 1] -- phi and step of every
 * (link, path, sinusoid), the line-of-sight one last.  One launch (k_air_fade_params).  TRXSIG_EINVAL: NULL object or arrays, no
 * profile set, n_links outside 1..2^24. */
int trxsig_air_fade_params(trxsig_air *air, uint64_t seed, int n_links, const uint32_t *d_doppler, uint32_t *d_phase, int32_t *d_step);

#ifdef __cplusplus
}
#endif
#endif /* TRXSIG_AIR_H */
