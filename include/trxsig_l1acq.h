/* trxsig_l1acq.h -- mobile-side acquisition on the device: from raw downlink samples of a C0 carrier, with unknown timing and
 * a carrier frequency offset, to the frame grid, the frame number and the BSIC.  The stage in front of trxsig_l1msrx.h: it
 * finds the frequency-correction burst (FCCH), estimates the frequency offset from it, finds and demodulates the
 * synchronisation burst (SCH) one frame later, decodes it (trxsig_fec_sch_decode_batch, trxsig.h) and reports where the frame
 * grid lies in the stream -- for many streams per call.
 *
 * THE FCCH STAGE HAS NO REFERENCE COUNTERPART.  The reference is a base station: it never looks for a frequency burst.  Stage 1
 * is pinned by this project's own float64 model (tests/l1_acq_model.py) within a stated tolerance.  Stage 2 is a composition of
 * the reference's own primitives (frequencyShift, correlate, peakDetect, the valley rule of analyzeTrafficBurst,
 * demodulateBurst) and is bit-identical to that composition on the CPU oracle.
 *
 * Input.  Complex float32 samples at the context's sps (1, 2 or 4); stream s starts at d_samples + s * stream_stride.  int16
 * radio streams go through trxsig_unpack_int16 or the front end first.  Acquisition always uses the exact arithmetic, whatever
 * trxsig_set_soft_mode says.
 *
 * Stage 1, the FCCH search.  L = 142 sps.  Per stream, for n in [0, N - sps):
 *     d[n] = x[n + sps] conj(x[n]) (-j)        e[n] = 0.5 (|x[n]|^2 + |x[n + sps]|^2)
 *   and for every window start k in [0, N - sps - L]:
 *     C[k] = sum_{i < L} d[k + i]    E[k] = sum_{i < L} e[k + i]
 *     m[k] = |C|^2 / E^2  if Re C > 0, E > 0 and C, E and the quotient are finite;  0 otherwise.
 *   The quotient is formed as written, in float32: |C|^2 and E^2 first.  A window whose E exceeds about 1.8e19 (E^2 beyond
 *   float32) therefore scores 0 although its exact metric is an ordinary number -- twelve orders of magnitude above any radio
 *   amplitude; the model (float64) is not bound by it.
 *   A frequency burst is a pure tone that advances pi / 2 per symbol, so it gives m ~ 1; random, dummy and alternating-bit
 *   bursts stay small (measured on the CPU model with offsets up to +-0.1 cycle / symbol: at most 0.26; the rest of an
 *   FCCH-bearing stream: at most 0.33).  Without the Re C > 0 rule an alternating-bit burst scores 0.99.
 *   The stream's answer is the smallest k of the largest m (k = 0 where every window scores 0; k = -1, everything else 0, where
 *   N < L + sps and there is no window), with C, E and m there, arg = atan2(Im C, Re C) in radians per symbol (0 where C is
 *   zero or not finite), omega = -arg / sps in radians per sample, and state bit 1 iff m > fcch_thresh.
 *   Every product and sum is float32, nothing is fused, and NO SUM SPANS MORE THAN L TERMS: the stream is cut into segments of
 *   L samples, each gets an inclusive prefix scan and an inclusive suffix scan, and a window is one suffix plus one prefix --
 *   no subtraction.  (A running sum that is differenced loses a quiet frequency burst beside a loud slot: 0.13 of metric error,
 *   up to infinite, with neighbours 40 dB up; the segment form stays within 8e-7 of float64 on the same streams.)  The order of
 *   the additions inside a scan is the implementation's; the tests' tolerance, 8 (L + 8) 2^-24 on m, follows from the L-term
 *   bound.
 *
 * Stage 2, the SCH detector and demodulator (trxsig_l1acq_detect_sch_batch; the search runs it on its own windows).
 *   The correlation sequence is built once at create on the host with the table generator's restatements:
 *   seq = modulateBurst(XTS, gsmPulse, 0, sps) with XTS the 64-bit extended training sequence (GSM 05.02 5.2.5),
 *   scaleVector(seq, (-1, 0)) -- the sequence starts at bit 42 and j^42 = -1, as generateMidamble's -1 for bit 66 -- and
 *   gain = peakDetect(correlate(seq, seq, NO_DELAY), &seq_toa).  It lives in the object's device memory; the constant-table blob
 *   is untouched.
 *   Per window (samples x at d_offset[b], length n = d_length[b], omega = d_omega[b]):
 *     1. y = frequencyShift(x, omega, startPhase 0)                      (skipped when d_omega is NULL)
 *     2. c = correlate(y, seq, NO_DELAY) over every lag, the reference's terms in the reference's order
 *     3. peak = peakDetect(c, &toa)
 *     4. the bogus-result rule and the valley of analyzeTrafficBurst (sigProcLib.cpp:961-990): toa < 0 or toa > n is bogus;
 *        lags +-2 sps .. +-5 sps round (int) rint(toa) that lie inside c; numRms < 2 is bogus;
 *        RMS = sqrtf(v / numRms) + 0.00001.  A bogus window reports amp = 0, ptm = 0 and is not detected.
 *     5. ptm = |peak| / RMS, amp = peak / gain, toa_b = toa - seq_toa - 42 sps
 *     6. detected iff ptm > detect_thresh, i0 = floor(toa_b) >= 0 and i0 + 148 sps <= n
 *     7. on detection soft = demodulateBurst(y[i0 : i0 + len), amp, toa_b - i0), first 148 values, with
 *        len = min(156 sps, n - i0) cut down to whole symbols (demodulateBurst's decimation is defined for whole symbols only:
 *        the reference writes past its allocation otherwise); zeros otherwise.  d_hard = soft > 0.5F.
 *     8. d_toa reports toa_b, d_ptm reports ptm, d_flags = TRXSIG_F_DETECT or 0.
 *   The interface carries no buffer length: THE CALLER GUARANTEES that every window [d_offset[b], d_offset[b] + d_length[b])
 *   lies inside d_samples; the kernels cannot check it.  (A search checks its own windows against n_samples.)
 *   A window with a negative offset or a length outside (0, TRXSIG_L1ACQ_MAX_WINDOW sps] gets TRXSIG_F_BADLEN and zeros.
 *   On SCH bursts ptm was at least 14 at 10 dB SNR on the CPU model; on windows without one at most 4.7.
 *   Steps 4 to 6 as written are TRXSIG_SCHDET_VALLEY, the default; under delay spread the valley fills with echoes and ptm
 *   falls to 1.5 .. 9.  trxsig_l1acq_set_sch_detector (below) puts the fit detector in their place.
 *
 * In a search: w0 = k - 3 sps + 1250 sps - 12 sps (the FCCH window starts three tail symbols into its burst, the SCH burst
 *   starts one frame later; a margin of 12 symbols, more than three times the largest FCCH position error seen on the model,
 *   3.3 symbols at 10 dB), n = 172 sps.  Stage 2 runs when bit 1 is set and [w0, w0 + n) lies inside the stream: that condition
 *   is state bit 2.  The suggested thresholds are TRXSIG_L1ACQ_FCCH_THRESH (0.5) and TRXSIG_L1ACQ_SCH_THRESH (8.0).
 *
 * THE RESULT A CALLER NEEDS: where state is 15, stream sample d_sch_w0 + d_sch_toa is bit 0 of TN 0 of frame d_rfn.
 *
 * Everything is enqueued on the context's stream; nothing synchronises.  Bad arguments -- NULL pointers, n_streams or
 * n_samples beyond what was created (or not positive), a stride below n_samples, B above 65535 -- return TRXSIG_EINVAL before
 * any launch.  Thread safety: one caller at a time per object.
 */
#ifndef TRXSIG_L1ACQ_H
#define TRXSIG_L1ACQ_H

#include "trxsig.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct trxsig_l1acq trxsig_l1acq;

#define TRXSIG_L1ACQ_FCCH_THRESH 0.5f
#define TRXSIG_L1ACQ_SCH_THRESH 8.0f
/* The suggested threshold of TRXSIG_SCHDET_FIT (below), measured on the float32 model (tests/sch_fit_model.py;
 * tests/test_sch_fit_model.py repeats the measurement), sps 1 and 4:
 *   (a) the largest q on candidate windows that hold no SCH -- white noise; random, dummy, frequency and alternating-bit bursts
 *       through the flat, five-tap and precursor channels at 15 dB, cut as a search cuts them; the SCH windows of the negative
 *       streams -- 28,601 windows a rate, of which 2,803 (sps 1) and 2,720 (sps 4) pass the geometry gate: 0.923 (sps 4: 0.874);
 *   (b) the smallest q on 60 SCH windows a profile at 10 dB: 2.06 (sps 1, precursor; flat 2.69, five 2.18; sps 4: 2.82, 2.09, 2.49).
 *   (b) / (a) = 2.23; the constant is their geometric mean, 1.379, to two digits.  At 6 dB the smallest q is 1.37 (sps 1, five):
 *   there the detector begins to miss.  At 15 dB the smallest is 2.88. */
#define TRXSIG_L1ACQ_SCH_FIT_THRESH 1.4f
#define TRXSIG_L1ACQ_MAX_WINDOW 256           /* symbols: the longest window trxsig_l1acq_detect_sch_batch takes */

/* d_state bits */
enum { TRXSIG_ACQ_FCCH = 1,      /* FCCH found: m > fcch_thresh */
       TRXSIG_ACQ_WINDOW = 2,    /* and the SCH window lies inside the stream */
       TRXSIG_ACQ_SCH = 4,       /* SCH detected and demodulated */
       TRXSIG_ACQ_DECODED = 8 }; /* SCH decoded with good parity */

/* What one search leaves: device arrays, one entry per stream, owned by the object, valid until its next search. */
typedef struct {
  int n_streams, soft_stride;
  const uint8_t *d_state;
  const int32_t *d_fcch_k;                     /* the window start, -1: the stream has no window */
  const float *d_fcch_metric;
  const trxsig_c32 *d_fcch_c;
  const float *d_fcch_e;
  const float *d_arg;                          /* radians per symbol */
  const float *d_omega;                        /* radians per sample: the shift applied to the SCH window */
  const int32_t *d_sch_w0;
  const float *d_sch_ptm;
  const trxsig_c32 *d_sch_amp;
  const float *d_sch_toa;
  const float *d_soft;                         /* [n_streams][soft_stride], soft_stride >= 148 */
  const uint8_t *d_ok, *d_bsic;
  const int32_t *d_rfn;
} trxsig_l1acq_out;

/* The object keeps ctx alive (trxsig_live_children counts it): trxsig_destroy on ctx takes effect when the object is gone too.
 * max_streams >= 1; max_samples >= 1, max_streams * max_samples below 2^31. */
int  trxsig_l1acq_create(trxsig_l1acq **out, trxsig_ctx *ctx, int max_streams, int max_samples);
void trxsig_l1acq_destroy(trxsig_l1acq *acq);
int  trxsig_l1acq_search(trxsig_l1acq *acq, const trxsig_c32 *d_samples, int64_t stream_stride,
                         int n_samples, int n_streams, float fcch_thresh, float sch_thresh,
                         trxsig_l1acq_out *out);
/* Stage 2 on caller-chosen windows (B <= 65535; d_ptm and d_hard may be NULL; soft_stride >= 148).  The object's workspace
 * grows on demand (a growth waits for the stream first). */
int  trxsig_l1acq_detect_sch_batch(trxsig_l1acq *acq, const trxsig_c32 *d_samples, const int32_t *d_offset,
                                   const int32_t *d_length, int B, const float *d_omega /* may be NULL */,
                                   float detect_thresh, uint8_t *d_flags, trxsig_c32 *d_amp, float *d_toa,
                                   float *d_ptm, float *d_soft, uint8_t *d_hard, int soft_stride);
/* the correlation sequence as built at create (host copies): seq[64 sps], its gain and TOA; any pointer may be NULL */
int  trxsig_l1acq_sequence(const trxsig_l1acq *acq, trxsig_c32 *h_seq, trxsig_c32 *h_gain, float *h_toa);

/* The SCH leg: what step 7 of stage 2 makes of a detected window.  TRXSIG_SCHLEG_DEMOD (the default): demodulateBurst, as stated
 * above; with it every output of trxsig_l1acq_search and trxsig_l1acq_detect_sch_batch is what it was before the switch existed,
 * byte for byte.  TRXSIG_SCHLEG_MLSE: trxsig_mlse_sch_batch (trxsig.h) in the demodulator's place, for a channel with delay
 * spread -- on the same shifted window y[i0 : i0 + len), with the same amp and toa_b - i0 and on the same windows (the detected
 * ones; zeros elsewhere).  Flags, amp, TOA, ptm and state bits 1, 2 and 4 do not depend on the leg; d_soft, d_hard and what the
 * SCH decoder makes of them (d_ok, d_bsic, d_rfn, state bit 8) do.  Host-side switch, takes effect from the next call on; anything
 * but the two values returns TRXSIG_EINVAL. */
enum { TRXSIG_SCHLEG_DEMOD = 0, TRXSIG_SCHLEG_MLSE = 1 };
int  trxsig_l1acq_set_sch_leg(trxsig_l1acq *acq, int leg);
/* The channel the equalising leg estimated in the last trxsig_l1acq_search: device arrays owned by the object, d_chan
 * [n_streams][5] taps h[0..4] and d_win [n_streams] window words (w = -4..0 equalised, 1 fell back, 2 skipped), as
 * trxsig_mlse_sch_batch reports them.  Zeros and 2 where the last search ran on TRXSIG_SCHLEG_DEMOD, where there was none yet, or
 * where nothing was detected (those are filled, on the context's stream, by this call).  trxsig_l1acq_detect_sch_batch leaves them
 * alone: a caller who wants the taps of caller-chosen windows calls trxsig_mlse_sch_batch. */
int  trxsig_l1acq_sch_channel(trxsig_l1acq *acq, const trxsig_c32 **d_chan, const int32_t **d_win);

/* The SCH detector: how steps 4 to 6 of stage 2 decide that a window holds a synchronisation burst.  TRXSIG_SCHDET_VALLEY (the
 * default): the valley rule, as stated above; with it every output of trxsig_l1acq_search and trxsig_l1acq_detect_sch_batch is
 * what it was before the switch existed, byte for byte -- also after the switch has been used and set back -- and nothing more
 * is enqueued.  TRXSIG_SCHDET_FIT: the fit detector, for a channel with delay spread (the valley rule takes its noise 2 to 5
 * symbols beside the peak, which is where the echoes lie: peak-to-valley falls from 18..37 to 1.5..9 there).
 *   Steps 1 to 3 are unchanged.  A window is a CANDIDATE iff 0 <= toa <= n, amp = peak / gain is finite and nonzero,
 *   i0 = floor(toa_b) >= 0 and i0 + 148 sps <= n; the valley is not evaluated (no numRms rule).  trxsig_sch_fit_batch's kernel
 *   (trxsig.h) then runs on the candidates, on the segment, amp and toa_b - i0 that step 7 takes, and a candidate is detected iff
 *   its q > detect_thresh.  Step 7, on either leg, runs on the detected windows as before.
 *   d_amp = peak / gain wherever 0 <= toa <= n (0 elsewhere) and d_toa = toa_b: the bytes VALLEY reports for every window the
 *   valley rule does not call bogus.  d_ptm and d_sch_ptm CARRY q, THE METRIC OF THE ACTIVE DETECTOR (0 for a window that is no
 *   candidate).  Flags, state bit 4 and everything behind them follow the fit verdict.
 *   The threshold is the caller's, as ever (sch_thresh, detect_thresh); the suggested one is TRXSIG_L1ACQ_SCH_FIT_THRESH below.
 * Host-side switch, independent of trxsig_l1acq_set_sch_leg (all four combinations work), takes effect from the next call on;
 * anything but the two values returns TRXSIG_EINVAL. */
enum { TRXSIG_SCHDET_VALLEY = 0, TRXSIG_SCHDET_FIT = 1 };
int  trxsig_l1acq_set_sch_detector(trxsig_l1acq *acq, int detector);
/* What the fit detector left in the last trxsig_l1acq_search: device arrays owned by the object, d_q and d_R [n_streams], as
 * trxsig_sch_fit_batch reports them (zeros for a stream that was no candidate).  Zeros where the last search ran on
 * TRXSIG_SCHDET_VALLEY or where there was none yet (filled, on the context's stream, by this call).
 * trxsig_l1acq_detect_sch_batch leaves them alone. */
int  trxsig_l1acq_sch_fit(trxsig_l1acq *acq, const float **d_q, const float **d_R);

#ifdef __cplusplus
}
#endif
#endif /* TRXSIG_L1ACQ_H */
