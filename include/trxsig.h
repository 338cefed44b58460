/*
 * trxsig.h -- C-ABI of libtrxsig: the MI355X (gfx950) burst-processing path of the
 * OpenBTS software transceiver.
 *
 * This is the drop-in boundary for the reference's `sigProcLib.h` seam
 * (Transceiver/sigProcLib.h:101-384) as it is driven by
 * Transceiver::pullRadioVector / addRadioVector (Transceiver/Transceiver.cpp:271-410,
 * 100-113) and RadioInterface::pullBuffer / pushBuffer (Transceiver/radioInterface.cpp:
 * 197-273, 123-194).  Plain pointers and sizes only; no C++ or torch types.  Every entry
 * point names the reference interface it replaces.
 *
 * Conventions
 *  - complex samples are interleaved float32 {re, im} (the layout of the reference's
 *    Complex<float>, Transceiver/Complex.h:39-44, inside Vector<complex>).
 *  - "d_" pointers are DEVICE pointers on the context's GPU; "h_" pointers are host.
 *  - a batch is B bursts packed in one sample array: burst b occupies
 *    samples[offset[b] .. offset[b]+length[b]).  offset[b] >= 0 (even offsets, i.e. 16-byte
 *    aligned bursts, take the wide-load path); length[b] a multiple of sps with
 *    92*sps <= length[b] <= 157*sps (the reference's own limits: sigProcLib.cpp:215-216,
 *    951, 1045-1050).
 *  - all work is enqueued on the context's HIP stream (trxsig_set_stream) and is
 *    asynchronous; the library never synchronises unless the entry point's comment says so.
 *  - return value: 0 on success, negative TRXSIG_E* on error; no exceptions cross the ABI.
 *  - results are bit-identical to the reference's float32 arithmetic (see DESIGN.md,
 *    "Numerical contract"), except where an entry point's comment states a tolerance.
 *  - There is NO CPU fallback: without a gfx950 device trxsig_create fails.
 */
#ifndef TRXSIG_H
#define TRXSIG_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 2: TRXSIG_K_COUNT grew (trxsig_profile_collect writes TRXSIG_K_COUNT entries: a host built against an older header must
 * not be run against this library -- compare trxsig_abi_version() with TRXSIG_ABI_VERSION at start-up, or use
 * trxsig_profile_collect_n, which takes the caller's capacity). */
#define TRXSIG_ABI_VERSION 2

typedef struct trxsig_ctx trxsig_ctx;
typedef struct { float re, im; } trxsig_c32;

enum {
  TRXSIG_OK = 0,
  TRXSIG_EINVAL = -1,   /* bad argument */
  TRXSIG_ENODEV = -2,   /* no usable gfx950 device / HIP runtime error at create */
  TRXSIG_EHIP = -3,     /* HIP runtime error (see trxsig_last_error) */
  TRXSIG_ENOMEM = -4
};

/* per-burst status byte written by the detect entry points */
enum {
  TRXSIG_F_ENERGY = 1,   /* energyDetect() passed           (sigProcLib.cpp:916-932)      */
  TRXSIG_F_DETECT = 2,   /* correlator peak/valley test passed (sigProcLib.cpp:913,1035)   */
  TRXSIG_F_BADLEN = 128  /* length[b]/offset[b] violates the conventions above; burst skipped */
};

/* ---- library set-up: sigProcLibSetup / sigProcLibDestroy (sigProcLib.h:110-113) -------------
 * trxsig_create = generateGSMPulse(2,sps) + sigProcLibSetup(sps) + generateRACHSequence +
 * generateMidamble(0..7) (the calls of Transceiver.cpp:62-64, 424, 553), built on the host and
 * uploaded once.  device = HIP device ordinal.  sps in {1,2,4}.
 * trxsig_destroy on a context that front ends, back ends or Transceiver groups (trxsig_frontend.h, trxsig_trxgroup.h) still live
 * on takes effect when the last of them has been destroyed: such an object never outlives the context it was created on. */
int  trxsig_abi_version(void);
int  trxsig_create(trxsig_ctx **out, int device, int sps);
void trxsig_destroy(trxsig_ctx *ctx);
int  trxsig_sps(const trxsig_ctx *ctx);
int  trxsig_device(const trxsig_ctx *ctx);
/* front ends, back ends and Transceiver groups currently alive on the context (each keeps it alive past trxsig_destroy);
 * a create call that fails leaves this count where it was */
int  trxsig_live_children(const trxsig_ctx *ctx);
/* stream = hipStream_t (NULL = the device's null stream).  One context per calling thread. */
int  trxsig_set_stream(trxsig_ctx *ctx, void *hip_stream);
/* hipStreamSynchronize on the context's stream */
int  trxsig_synchronize(trxsig_ctx *ctx);
void *trxsig_get_stream(trxsig_ctx *ctx);      /* the hipStream_t the context enqueues on */
int  trxsig_get_device(trxsig_ctx *ctx);
const char *trxsig_last_error(const trxsig_ctx *ctx);
/* pre-size the internal device workspace for batches up to max_bursts (allocates; call outside
 * any timed or graph-captured region).  The batch entry points grow it on demand otherwise. */
int  trxsig_reserve(trxsig_ctx *ctx, int max_bursts);

/* ---- constant tables ------------------------------------------------------------------------
 * The constant tables (trig lookup, GMSK rotation, pulse, 8 midambles, RACH sequence, sinc grid)
 * live in ONE device blob so that a multi-GPU job can build them on rank 0 and broadcast them
 * (RCCL ncclBroadcast over xGMI) instead of rebuilding per rank: SURVEY 8e.
 *   trxsig_tables_bytes   size of the blob
 *   trxsig_tables_device  device pointer of this context's blob
 *   trxsig_create_from_tables  build a context on `device` from a blob that is already in that
 *                         device's memory (d_blob); copies it, validates header + checksum.
 *   trxsig_tables_export  copy the blob to host memory (synchronises)
 *   trxsig_tables_build_host  build the blob into host memory without touching any device
 *                         (what rank 0 uploads; also lets the table construction be tested on CPU) */
size_t trxsig_tables_bytes(int sps);
int    trxsig_tables_build_host(int sps, void *h_buf, size_t cap);
void  *trxsig_tables_device(trxsig_ctx *ctx);
int    trxsig_create_from_tables(trxsig_ctx **out, int device, const void *d_blob, size_t bytes);
int    trxsig_tables_export(trxsig_ctx *ctx, void *h_buf, size_t cap);

/* host-side view of the tables (for the C++ facade and tests); pointers valid for ctx lifetime */
typedef struct {
  int sps;
  const float *cos_table;            /* 1025: cosTable  (sigProcLib.cpp:39,207-212) */
  const float *sin_table;            /* 1025: sinTable                              */
  const trxsig_c32 *gmsk_rotation;   /* 157*sps: GMSKRotation (sigProcLib.cpp:214-225) */
  const trxsig_c32 *gmsk_reverse;    /* 157*sps: GMSKReverseRotation                   */
  const float *gsm_pulse;            /* 2*sps+1: generateGSMPulse(2,sps) (sigProcLib.cpp:411-430) */
  const trxsig_c32 *midamble[8];     /* 16*sps each: gMidambles[t]->sequence (sigProcLib.cpp:779-828) */
  float midamble_toa[8];
  trxsig_c32 midamble_gain[8];
  const trxsig_c32 *rach;            /* 41*sps: gRACHSequence->sequence (sigProcLib.cpp:830-857) */
  float rach_toa;
  trxsig_c32 rach_gain;
} trxsig_tables_view;
int trxsig_tables_view_get(const trxsig_ctx *ctx, trxsig_tables_view *out);

/* ---- RX hot path ----------------------------------------------------------------------------
 * trxsig_detect_demod_normal_batch
 *   For every burst: energyDetect(burst, 20*sps, energy_thresh) -> analyzeTrafficBurst(burst, tsc,
 *   detect_thresh, sps, &amp, &TOA) -> on detection demodulateBurst(burst, pulse, sps, amp, TOA):
 *   the TSC leg of Transceiver::pullRadioVector (Transceiver.cpp:298, 327-335, 385-388 /
 *   Transceiver52M/Transceiver.cpp:382-389) with the sequential threshold state machine left to
 *   the caller (SURVEY 8a' item 14).  Replaces sigProcLib.h:246-249, 277-285, 316-320.
 *
 *   d_flags[b]   status byte (TRXSIG_F_*)
 *   d_amp[b]     amplitude estimate (0 when the reference returns "bogus result")
 *   d_toa[b]     time of arrival in samples
 *   d_avgpwr[b]  energyDetect's avgPwr                                   (may be NULL)
 *   d_soft       B x soft_stride floats; the first nsoft (<= min(157, length/sps)) soft bits of
 *                demodulateBurst for detected bursts, zeros otherwise
 *   d_hard       B x soft_stride bytes, SoftVector::bit() = soft > 0.5F (BitVector.h:415-420)
 *                                                                        (may be NULL)
 *   Bursts whose energy test fails are reported undetected (amp = 0, TOA = 0), as the reference
 *   does not run the correlator for them (Transceiver.cpp:298-306).  energy_thresh < 0 disables
 *   the energy gate (every burst is analysed; TRXSIG_F_ENERGY is set). */
int trxsig_detect_demod_normal_batch(trxsig_ctx *ctx,
                                     const trxsig_c32 *d_samples, const int32_t *d_offset,
                                     const int32_t *d_length, int B,
                                     int tsc, float detect_thresh, float energy_thresh,
                                     uint8_t *d_flags, trxsig_c32 *d_amp, float *d_toa,
                                     float *d_avgpwr,
                                     float *d_soft, uint8_t *d_hard, int nsoft, int soft_stride);

/* trxsig_detect_demod_rach_batch: same for access bursts: detectRACHBurst(burst, detect_thresh,
 *   sps, &amp, &TOA) + demodulateBurst (Transceiver.cpp:362-366, 385-388; sigProcLib.h:263-267).
 *   The 41*sps-tap correlation is evaluated over every lag exactly as the reference does
 *   (same terms, same order), so flags/amp/TOA/soft/hard are all bit-identical. */
int trxsig_detect_demod_rach_batch(trxsig_ctx *ctx,
                                   const trxsig_c32 *d_samples, const int32_t *d_offset,
                                   const int32_t *d_length, int B,
                                   float detect_thresh, float energy_thresh,
                                   uint8_t *d_flags, trxsig_c32 *d_amp, float *d_toa,
                                   float *d_avgpwr,
                                   float *d_soft, uint8_t *d_hard, int nsoft, int soft_stride);


/* trxsig_demodulate_batch: demodulateBurst alone with caller-supplied amp/TOA
 *   (sigProcLib.h:316-320; used for RACH after detect and by TRANSMIT_LOGGING,
 *   Transceiver.cpp:115-136).  d_enable[b]==0 skips burst b (zeros out); NULL = all. */
int trxsig_demodulate_batch(trxsig_ctx *ctx,
                            const trxsig_c32 *d_samples, const int32_t *d_offset,
                            const int32_t *d_length, int B,
                            const trxsig_c32 *d_amp, const float *d_toa, const uint8_t *d_enable,
                            float *d_soft, uint8_t *d_hard, int nsoft, int soft_stride);

/* trxsig_set_soft_mode: how demodulateBurst's soft bits (sigProcLib.cpp:1056-1097) are computed behind the three calls above
 *   (and behind the Transceiver group's demodulating leg on a complex float32 stream).  Flags, amplitude, TOA and avgPwr are the
 *   reference's values bit for bit in either mode, and so is every HARD bit (SoftVector::bit, soft > 0.5F).
 *   TRXSIG_SOFT_EXACT (the default): every soft bit equals the reference's float32 value (IEEE ==): scaleVector, delayVector's
 *     21 taps, the reverse rotation and the slicer operation by operation, in the reference's order.
 *   TRXSIG_SOFT_TOLERANCE: the accuracy the reference's users are promised elsewhere ("within 1e-4 on soft symbols") spent on
 *     speed -- 1/amp is applied to the 148 outputs instead of the 625 samples and the delay filter accumulates with fused
 *     multiply-adds (csrc/trxsig_demod.h, fused_demod_tol: ~200 instead of ~530 VALU instructions per burst).  Guaranteed
 *     |soft - reference soft| <= 3.7e-5 on the [0, 1] scale of a soft bit (derivation there); the parity contract (<= 1e-6, or
 *     1e-4 relative) is held on tested input families, a hostile one included; a burst for
 *     which the guarantee cannot be given (a soft symbol too close to the slicer's 0.5 for the hard bit to be certain, a NaN or
 *     infinity anywhere, max|sample| * |1/amp| > 4, a TOA off peakDetect's 1/512 grid, an odd burst geometry) is computed by
 *     the exact code inside the same launch and comes out IEEE-equal.  nsoft > 148 always takes the exact code.
 *   Takes effect from the next call on (host-side switch, no synchronisation). */
enum { TRXSIG_SOFT_EXACT = 0, TRXSIG_SOFT_TOLERANCE = 1 };
int trxsig_set_soft_mode(trxsig_ctx *ctx, int mode);
int trxsig_get_soft_mode(const trxsig_ctx *ctx);

/* ---- the sequence equaliser for normal bursts (csrc/trxsig_mlse.hip) -------------------------------------------------------
 * trxsig_mlse_batch: the mirror of trxsig_demodulate_batch for a channel with delay spread -- a per-burst channel estimate from
 *   the midamble and a 16-state max-log-MAP equaliser that hands up soft bits, at sps 1, 2 and 4, in one launch.  The reference
 *   has no counterpart (Transceiver/README.Talgorithm is a design note); the stage is pinned by the float32 model
 *   tests/mlse_model.py, which the kernel equals word for word: float add, subtract, multiply, minimum, compare and one correctly
 *   rounded division per soft bit, nothing fused, no tolerance.  trxsig_set_soft_mode has no bearing on it.
 *   The model, and the kernel directly, are in turn graded against tests/mlse_ref.py: step 3 below as a statement about symbol
 *   sequences in float64 (exact min-marginals of a chain, proved against enumeration), with the a-priori bound
 *   |soft - clamp(soft64)| <= 1.001 ((2 Q + 124 P) / (8 E) + 5) 2^-24 per burst and half -- P the sum over the 61 steps of the
 *   step's largest finite branch metric, Q the same sum of the metrics' own rounding terms, 8 to 11 P; 2.4e-4 to 7.0e-4 on the
 *   tests' bursts -- exact clamps beyond it and equal hard bits outside it (tests/test_mlse_ref.py, tests/test_gpu_mlse_ref.py).
 *   With a[n] = 2 bit[n] - 1 and t[j] = a[61 + j] the training sequence `tsc`:
 *   1. Symbols.  y[0..147] = demodulateBurst's vector just before vectorSlicer, both parts kept: scaleVector(1/amp),
 *      delayVector(-TOA), GMSKReverseRotate (the complex product with rev[sps m]), decimateVector(sps); exact-mode arithmetic.
 *   2. Channel.  c[d] = 0.0625f * sum_{i=0..15} t[5+i] * y[66+i+d] for d = -4..4 (complex float32, the sum starts from 0, i
 *      ascending); p[d] = c.re*c.re + c.im*c.im; E_w = (((p[w] + p[w+1]) + p[w+2]) + p[w+3]) + p[w+4]; w = 0, -1, .., -4 is
 *      scanned in that order and a later w is taken only on a strict >; h[k] = c[w+k], k = 0..4, E = E_w.
 *      The model of the burst: y[n] = sum_k h[k] a[n-w-k].
 *   3. Two independent half-burst trellises of 16 states and 61 steps.  Bit j of a state s is the j-th most recent symbol
 *      (1 = +1); a step with symbol b leads to ((s << 1) & 15) | b and has the 5-bit index x = (s << 1) | b, the expected value
 *      Z[x] = ((((+-g[0]) + +-g[1]) + +-g[2]) + +-g[3]) + +-g[4] (sign of term k: bit k of x) and the branch metric
 *      dr*dr + di*di, (dr, di) = y - Z[x].  Right half: g = h, steps m = 87..147 on y[m+w], start state a[86], a[85], a[84],
 *      a[83] (bit 0 first), a[145..147] = -1 known.  Left half: g[k] = h[4-k], steps m = 60..0 on y[m+4+w], start state a[61],
 *      a[62], a[63], a[64], a[0..2] = -1 known.  alpha is 0 in the start state and +inf elsewhere; a branch against a known
 *      symbol costs +inf.  alpha'[s'] = min(alpha[s'>>1] + gamma, alpha[(s'>>1)|8] + gamma); beta = 0 after the last step,
 *      beta[s] = min_b(gamma[(s<<1)|b] + beta'[((s<<1)|b) & 15]).  Per step T[s] = alpha[s] + beta[s], both after the step,
 *      and M_b = the minimum of T over the eight states whose bit 0 is b.
 *   4. soft[m] = clamp(0.5f + (M_0 - M_1) / (8.0f * E), 0, 1); hard = soft > 0.5F.  A known symbol comes out as exactly 0.
 *      Positions 61..86 carry the demodulator's formula clamp((y.re + 1) * 0.5).  (On a one-tap channel (M_0 - M_1) / (8 E) is
 *      Re(y / h) / 2: the demodulator's soft bit.)
 *   5. A burst gets the demodulator's formula on all of y instead -- demodulateBurst's exact-mode soft bits -- when
 *      length/sps < 148 (y[m] = 0, soft bit 0.5, for m >= length/sps, where demodulateBurst has no symbol), or some component of y[0..147] fails fabsf(v) < 0x1p30f (a NaN or an infinity among them; what passes
 *      keeps every metric finite), or E == 0.  No NaN can then arise in steps 2-4, and there is no survivor path to break ties on.
 *   d_enable[b] == 0 skips burst b; NULL = all.  A burst k_demod would refuse (offset < 0, a length outside 92..157 symbols or
 *   no multiple of sps, |TOA| > 4096 or NaN) counts as skipped.
 *   d_chan   B x 5 taps h[0..4]; zeros for a burst that fell back or was skipped          (may be NULL)
 *   d_win    w (-4..0) where the burst was equalised, 1 where it fell back, 2 where it was skipped (soft bits zeros)  (may be NULL)
 *   d_soft / d_hard / nsoft (<= 148) / soft_stride: as trxsig_demodulate_batch
 * trxsig_mlse_normal_batch: trxsig_detect_demod_normal_batch's detector (flags, amp, TOA and avgPwr are that call's, in either
 *   soft mode) and then the equaliser on the bursts it flagged TRXSIG_F_DETECT. */
int trxsig_mlse_batch(trxsig_ctx *ctx,
                      const trxsig_c32 *d_samples, const int32_t *d_offset,
                      const int32_t *d_length, int B, int tsc,
                      const trxsig_c32 *d_amp, const float *d_toa, const uint8_t *d_enable,
                      trxsig_c32 *d_chan, int32_t *d_win,
                      float *d_soft, uint8_t *d_hard, int nsoft, int soft_stride);
int trxsig_mlse_normal_batch(trxsig_ctx *ctx,
                             const trxsig_c32 *d_samples, const int32_t *d_offset,
                             const int32_t *d_length, int B,
                             int tsc, float detect_thresh, float energy_thresh,
                             uint8_t *d_flags, trxsig_c32 *d_amp, float *d_toa,
                             float *d_avgpwr, trxsig_c32 *d_chan, int32_t *d_win,
                             float *d_soft, uint8_t *d_hard, int nsoft, int soft_stride);

/* ---- the sequence equaliser for access bursts (csrc/trxsig_mlse_access.hip) ------------------------------------------------
 * trxsig_mlse_access_batch: trxsig_mlse_batch's counterpart for the access burst (GSM 05.02 5.2.7): a least-squares channel
 *   estimate of nine taps from the burst's 49 known leading symbols and ONE trellis of 39 steps over the 36 coded bits and the
 *   three tail bits, at sps 1, 2 and 4, in one launch.  Pinned by the float32 model tests/mlse_access_model.py, which the kernel
 *   equals word for word; the arithmetic rules are trxsig_mlse_batch's: every step is one float32 operation in the order written,
 *   nothing fused, one correctly rounded division per soft bit.  Graded against the float64 statement tests/mlse_access_ref.py
 *   with the a-priori bound |soft - clamp(soft64)| <= 1.001 ((2 Q + 80 P) / (8 E) + 5) 2^-24 per burst (P, Q as in
 *   trxsig_mlse_batch, over the 39 steps; derived there).
 *   With a[n] = 2 bit[n] - 1: bits 0..48 are the extended tail and the synchronisation sequence, 49..84 the coded bits, 85..87 are 0.
 *   1. Symbols.  y[0..147] is step 1 of trxsig_mlse_batch with the amplitude and TOA detectRACHBurst reports; that TOA is relative
 *      to the start of the burst, so a[n] sits at y[n].
 *   2. Channel.  The model of the burst is y[n] = sum_{d=-4..4} c[d] a[n-d]; for the 41 positions n = 4..44 all nine symbols are
 *      known.  With A[n-4][d+4] = a[n-d] (41 x 9), G = A^T A (integer: diagonal 41, off-diagonals of magnitude <= 5, condition
 *      number 1.8), N = adj(G) A^T and det = det(G) exact integers below 2^53:
 *          P32[d+4][j] = (float)((double)N[d+4][j] / (double)det)       (csrc/trxsig_mlse_access_tab.h; |P32| < 0.04)
 *          c[d].re = sum_{j=0..40} P32[d+4][j] * y[4+j].re, the sum starts from 0, j ascending, one multiply and one add per
 *      term; c[d].im likewise.  p[d], E_w, the scan w = 0, -1, .., -4 with a strict >, h[k] = c[w+k] and E = E_w are
 *      trxsig_mlse_batch's step 2.  The estimator's noise gain is 0.0248 to 0.0258 per tap (1/16 = 0.0625 for the normal burst's).
 *   3. One trellis of 16 states and 39 steps: state, branch index, Z[x] and the metric as in trxsig_mlse_batch, g = h.  Step
 *      i = 0..38 is symbol m = 49 + i on y[m+w]; the start state is a[48], a[47], a[46], a[45] (bit 0 first); for i >= 36 a
 *      branch with b = 1 costs +inf.  alpha, beta, T and M_b word for word as there.
 *   4. soft[m] = clamp(0.5f + (M_0 - M_1) / (8.0f * E), 0, 1) for m = 49..87; the three tail bits come out as exactly 0.
 *      Positions 0..48 and 88..147 carry the demodulator's formula clamp((y.re + 1) * 0.5).  hard = soft > 0.5F.
 *   5. Fall back and skip exactly as trxsig_mlse_batch: the demodulator's formula on all of y when length/sps < 148, when a
 *      component of y fails fabsf(v) < 0x1p30f, or when E == 0; a burst k_demod's geometry test refuses, or d_enable[b] == 0,
 *      is skipped.  Every metric stays finite under that guard: |c| components <= 41 * 0.04 * 2^30 < 2^31, so |Z| components
 *      < 5 * 2^31 < 2^34, a branch metric < 2 * (2^34 + 2^30)^2 < 2^70, 39 of them and one more sum < 2^77, and E < 10 * 2^62 < 2^66.
 *   d_chan / d_win / d_soft / d_hard / nsoft (<= 148) / soft_stride: as trxsig_mlse_batch.  Refusals are trxsig_mlse_batch's.
 * trxsig_mlse_rach_batch: trxsig_detect_demod_rach_batch's detector (flags, amp, TOA and avgPwr are that call's, bit for bit, in
 *   either soft mode), then the equaliser on the bursts flagged TRXSIG_F_DETECT; the others get zeros and d_win = 2.
 * trxsig_mlse_access_pinv_host: P32, row d + 4 first, to the caller's 9 * 41 floats. */
int trxsig_mlse_access_batch(trxsig_ctx *ctx,
                             const trxsig_c32 *d_samples, const int32_t *d_offset,
                             const int32_t *d_length, int B,
                             const trxsig_c32 *d_amp, const float *d_toa, const uint8_t *d_enable,
                             trxsig_c32 *d_chan, int32_t *d_win,
                             float *d_soft, uint8_t *d_hard, int nsoft, int soft_stride);
int trxsig_mlse_rach_batch(trxsig_ctx *ctx,
                           const trxsig_c32 *d_samples, const int32_t *d_offset,
                           const int32_t *d_length, int B,
                           float detect_thresh, float energy_thresh,
                           uint8_t *d_flags, trxsig_c32 *d_amp, float *d_toa,
                           float *d_avgpwr, trxsig_c32 *d_chan, int32_t *d_win,
                           float *d_soft, uint8_t *d_hard, int nsoft, int soft_stride);
int trxsig_mlse_access_pinv_host(float out[9 * 41]);

/* ---- the sequence equaliser for synchronisation bursts (csrc/trxsig_mlse_sch.hip) ------------------------------------------
 * trxsig_mlse_sch_batch: trxsig_mlse_batch's counterpart for the synchronisation burst (SCH, GSM 05.02 5.2.5): a least-squares
 *   channel estimate of nine taps from the burst's 64-symbol extended training sequence and TWO half-burst trellises of 42 steps
 *   each over the 39 coded bits and the three tail bits of a side, at sps 1, 2 and 4, in one launch.  Pinned by the float32 model
 *   tests/mlse_sch_model.py, which the kernel equals word for word; the arithmetic rules are trxsig_mlse_batch's: every step is
 *   one float32 operation in the order written, nothing fused, one correctly rounded division per soft bit.  trxsig_set_soft_mode
 *   has no bearing on it.  Graded against the float64 statement tests/mlse_sch_ref.py with the a-priori bound
 *   |soft - clamp(soft64)| <= 1.001 ((2 Q + 86 P) / (8 E) + 5) 2^-24 per burst and half (P, Q as in trxsig_mlse_batch, over the
 *   42 steps; derived there).
 *   With a[n] = 2 bit[n] - 1: bits 0..2 are tail (0), 3..41 coded, 42..105 the extended training sequence XTS
 *   (a[42 + i] = 2 XTS[i] - 1), 106..144 coded, 145..147 tail.
 *   1. Symbols.  y[0..147] is step 1 of trxsig_mlse_batch; the TOA is relative to the start of the burst, so a[n] sits at y[n].
 *   2. Channel.  The model of the burst is y[n] = sum_{d=-4..4} c[d] a[n-d]; for the 56 positions n = 46..101 all nine symbols are
 *      known.  With A[n-46][d+4] = a[n-d] (56 x 9), G = A^T A (integer: diagonal 56, off-diagonals of magnitude <= 6, condition
 *      number 1.64), N = adj(G) A^T and det = det(G) exact integers below 2^53:
 *          P32[d+4][j] = (float)((double)N[d+4][j] / (double)det)       (csrc/trxsig_mlse_sch_tab.h; |P32| < 0.0253)
 *          c[d].re = sum_{j=0..55} P32[d+4][j] * y[46+j].re, the sum starts from 0, j ascending, one multiply and one add per
 *      term; c[d].im likewise.  p[d], E_w, the scan w = 0, -1, .., -4 with a strict >, h[k] = c[w+k] and E = E_w are
 *      trxsig_mlse_batch's step 2.  The estimator's noise gain is 0.01824 to 0.01850 per tap (0.0248 for the access burst's,
 *      1/16 = 0.0625 for the normal burst's).
 *   3. Two independent half-burst trellises of 16 states and 42 steps: state, branch index, Z[x], the metric, alpha, beta, T and
 *      M_b as in trxsig_mlse_batch.  Right half: g = h, steps m = 106..147 on y[m+w], start state a[105], a[104], a[103], a[102]
 *      (bit 0 first: 11), a[145..147] = -1 known.  Left half: g[k] = h[4-k], steps m = 41..0 on y[m+4+w], start state a[42],
 *      a[43], a[44], a[45] (13), a[0..2] = -1 known.
 *   4. soft[m] = clamp(0.5f + (M_0 - M_1) / (8.0f * E), 0, 1) for m = 0..41 and 106..147; the six tail bits come out as exactly 0.
 *      Positions 42..105 carry the demodulator's formula clamp((y.re + 1) * 0.5).  hard = soft > 0.5F.
 *   5. Fall back and skip exactly as trxsig_mlse_batch: the demodulator's formula on all of y when length/sps < 148, when a
 *      component of y fails fabsf(v) < 0x1p30f, or when E == 0; a burst k_demod's geometry test refuses, or d_enable[b] == 0,
 *      is skipped.  Every metric stays finite under that guard: the rows of P32 sum to S1 <= 1.0001 in magnitude, so |c|
 *      components stay below 1.0001 * 2^30 < 2^31, and from there on the access burst's chain holds with 42 steps for 39:
 *      |Z| components < 2^34, a branch metric < 2^70, 42 of them and one more sum < 2^77, E < 2^66.
 *   d_chan / d_win / d_soft / d_hard / nsoft (<= 148) / soft_stride: as trxsig_mlse_batch.  Refusals are trxsig_mlse_batch's.
 *   trxsig_l1acq_set_sch_leg (trxsig_l1acq.h) puts it behind acquisition's SCH detector.
 * trxsig_mlse_sch_pinv_host: P32, row d + 4 first, to the caller's 9 * 56 floats. */
int trxsig_mlse_sch_batch(trxsig_ctx *ctx,
                          const trxsig_c32 *d_samples, const int32_t *d_offset,
                          const int32_t *d_length, int B,
                          const trxsig_c32 *d_amp, const float *d_toa, const uint8_t *d_enable,
                          trxsig_c32 *d_chan, int32_t *d_win,
                          float *d_soft, uint8_t *d_hard, int nsoft, int soft_stride);
int trxsig_mlse_sch_pinv_host(float out[9 * 56]);

/* ---- the fit detector's statistic for synchronisation bursts (csrc/trxsig_sch_fit.hip) --------------------------------------
 * trxsig_sch_fit_batch: how well the burst's 56 fully known rows fit the five-tap channel trxsig_mlse_sch_batch estimates from
 *   them: q = sqrt(51 E / R), tap energy over residual power.  51 is 56 rows less 5 taps, so q^2 estimates the linear SNR, and it
 *   does not care where the echoes of the channel lie (the valley rule of trxsig_l1acq.h takes its noise 2 to 5 symbols beside the
 *   correlation peak, where they are).  Pinned by the float32 model tests/sch_fit_model.py, which the kernel equals word for word;
 *   every step is one float32 operation in the order written, nothing fused, one correctly rounded division and one correctly
 *   rounded square root per burst.  Graded against the float64 statement tests/sch_fit_ref.py with the a-priori bounds
 *   (u = 2^-24, g_k = k u / (1 - k u), H.re = sum_k |h[k].re|, r, e and R below the float64 values; derived there)
 *       d.re[n] = u |r[n].re| + (1 + u) g_4 H.re, d.im[n] likewise            (four additions in Z, one subtraction)
 *       b[n] = (1 + g_2) (2 (|r.re| d.re + |r.im| d.im) + d.re^2 + d.im^2) + g_2 e[n]          (two squares, one addition)
 *       |R32 - R| <= bR = sum b[n] + g_6 (R + sum b[n])                                        (six levels of the tree)
 *       |q32 - q| <= q (sqrt((1 + g_8) / (1 - bR / R)) (1 + u) - 1)   where bR < R     (E: six roundings, 51 E, the quotient; the root)
 *   1. Symbols y[0..147]: step 1 of trxsig_mlse_sch_batch, word for word.
 *   2. c[-4..4] = P32 y[46..101], the window w, h[k] = c[w + k] and E: step 2 of trxsig_mlse_sch_batch, word for word.
 *   3. The residual on the rows n = 46..101 (every a[n - w - k] lies in the extended training sequence, 42..105):
 *          Z[n] = h[0] a[n - w], then + h[1] a[n - w - 1], .., + h[4] a[n - w - 4], in this order (the products with +-1 are sign
 *          flips; real and imaginary parts apart): trxsig_mlse_batch's Z[x] with bit k of x the bit of a[n - w - k];
 *          r[n] = y[n] - Z[n];  e[n - 46] = r.re * r.re + r.im * r.im.
 *   4. R = the pairwise tree over e[0..63] with e[56..63] = 0: s1[i] = e[2 i] + e[2 i + 1], s2[i] = s1[2 i] + s1[2 i + 1], .. six
 *      levels down to one number (the kernel's reduction over the 64 lanes of a wave).
 *   5. q = sqrtf((51.0f * E) / R): the product first, then the division, then the root.  R == 0 with E > 0 gives +inf and stays
 *      +inf.  q = 0 where the result is a NaN.
 *   6. Where trxsig_mlse_sch_batch falls back (length/sps < 148, a component of y that fails fabsf(v) < 0x1p30f, E == 0) or skips
 *      (k_demod's geometry test refuses the burst, d_enable[b] == 0): q = 0, E = 0, R = 0, the nine taps zero, d_win = 1 or 2.
 *      Under the guard everything is finite: |Z| components < 2^34, |r| components < 2^35, R < 2^78, 51 E < 2^72.
 *   d_chan9 [B][9] receives c[-4..4], d_win [B] the window word as trxsig_mlse_sch_batch reports it, d_E, d_R, d_q [B]; any of
 *   the five may be NULL.  Inputs and refusals are trxsig_mlse_sch_batch's.  trxsig_l1acq_set_sch_detector (trxsig_l1acq.h) makes
 *   q acquisition's SCH verdict. */
int trxsig_sch_fit_batch(trxsig_ctx *ctx,
                         const trxsig_c32 *d_samples, const int32_t *d_offset,
                         const int32_t *d_length, int B,
                         const trxsig_c32 *d_amp, const float *d_toa, const uint8_t *d_enable,
                         trxsig_c32 *d_chan9, int32_t *d_win,
                         float *d_E, float *d_R, float *d_q);

/* ---- two-antenna receive diversity for the sequence equaliser (csrc/trxsig_mlse_div.hip) ------------------------------------
 * trxsig_mlse_div_batch: trxsig_mlse_batch on two receive antennas -- one channel window for both, the branch metric summed over
 *   both: maximal-ratio combining inside the trellis.  Both branches are assumed to have the same noise power (a common scale
 *   1/amp keeps their noise on one footing; that is what makes the plain sum maximal-ratio).  Pinned by the float32 model
 *   tests/mlse_div_model.py, which the kernel equals word for word, and graded against the float64 statement
 *   tests/mlse_div_ref.py with the a-priori bound |soft - clamp(soft64)| <= 1.001 ((2 Q + 124 P) / (8 E) + 6) 2^-24 (P, Q: the sums
 *   of trxsig_mlse_batch's bound over the summed metric, E = sum_a sum_k |h_a[k]|^2; derived there).
 *   It is trxsig_mlse_batch's algorithm with these changes and no others; a = 0, 1 is the antenna:
 *   1. Symbols.  y_a[0..147] = step 1 there on antenna a's samples (d_samples<a>, d_offset<a>; the length is shared), both with the
 *      SAME amplitude and TOA: one d_amp[b], one d_toa[b] per burst.
 *   2. Channel.  c_a[d] per antenna as there; p[d] = (c_0.re*c_0.re + c_0.im*c_0.im) + (c_1.re*c_1.re + c_1.im*c_1.im) (antenna
 *      0's power first, one float32 addition); E_w, the scan order and the strict > as there, on this p: ONE window w for both
 *      antennas; h_a[k] = c_a[w+k], E = E_w.
 *   3. Trellis.  Z_a[x] per antenna from g_a (h_a for the right half, h_a reversed for the left); the branch metric is
 *      gamma = (dr_0*dr_0 + di_0*di_0) + (dr_1*dr_1 + di_1*di_1), (dr_a, di_a) = y_a - Z_a[x]: each parenthesis the metric there,
 *      joined by one float32 addition.  Start states, known tail symbols as +inf, alpha, beta, T, M_b: word for word as there.
 *   4. soft[m] = clamp(0.5f + (M_0 - M_1) / (8.0f * E), 0, 1).  Positions 61..86 carry the demodulator's formula on y_p.re,
 *      p = d_primary[b] the antenna that amp and TOA came from (0 or 1; NULL = 0 for every burst).
 *   5. Fallback: the demodulator's formula on all of y_p when length/sps < 148, or a component of y_0 or y_1 fails
 *      fabsf(v) < 0x1p30f, or E == 0.  The skip rule (d_enable, k_demod's geometry test) is as there and is applied once: the
 *      antennas share the length and the TOA, and a negative offset on either antenna skips the burst.
 *   Three identities hold exactly in IEEE arithmetic.  Antenna 1 all zeros: soft bits, hard bits and the window equal
 *   trxsig_mlse_batch's on antenna 0, chan[b][0] its taps, chan[b][1] zeros.  The same samples on both antennas: p, gamma, E and
 *   M_0 - M_1 all double exactly; soft bits, hard bits and the window equal trxsig_mlse_batch's.  Antennas swapped (d_primary
 *   too): soft bits and the window are identical, chan[b][0] and chan[b][1] exchanged.
 *   d_chan   B x 2 x 5 taps h_a[0..4]; zeros for a burst that fell back or was skipped     (may be NULL)
 *   d_win    as trxsig_mlse_batch                                                            (may be NULL)
 * trxsig_mlse_div_normal_batch: trxsig_detect_demod_normal_batch's detector on each antenna (d_flags, d_amp, d_toa, d_avgpwr:
 *   2 x B, antenna a at [a * B + b]; that call's values bit for bit, in either soft mode), the selection, and the equaliser on the
 *   bursts with d_sel[b] < 2 with the selected antenna's amp and TOA and d_primary = d_sel.
 *   The selection rule: v_a = antenna a detected (TRXSIG_F_DETECT); n_a = amp_a.re*amp_a.re + amp_a.im*amp_a.im in float32, not
 *   fused; sel = 1 if v_1 && (!v_0 || n_1 > n_0) (a NaN compares false); otherwise sel = 0 if v_0; otherwise sel = 2: neither
 *   antenna detected, the soft bits are zeros and d_win is 2.
 *   Refusals are trxsig_mlse_batch's: TRXSIG_EINVAL for a NULL context, nsoft > 148, tsc outside 0..7, NULL required arrays. */
int trxsig_mlse_div_batch(trxsig_ctx *ctx,
                          const trxsig_c32 *d_samples0, const int32_t *d_offset0,
                          const trxsig_c32 *d_samples1, const int32_t *d_offset1,
                          const int32_t *d_length, int B, int tsc,
                          const trxsig_c32 *d_amp, const float *d_toa, const uint8_t *d_primary, const uint8_t *d_enable,
                          trxsig_c32 *d_chan, int32_t *d_win,
                          float *d_soft, uint8_t *d_hard, int nsoft, int soft_stride);
int trxsig_mlse_div_normal_batch(trxsig_ctx *ctx,
                                 const trxsig_c32 *d_samples0, const int32_t *d_offset0,
                                 const trxsig_c32 *d_samples1, const int32_t *d_offset1,
                                 const int32_t *d_length, int B, int tsc,
                                 float detect_thresh, float energy_thresh,
                                 uint8_t *d_flags, trxsig_c32 *d_amp, float *d_toa, float *d_avgpwr,
                                 uint8_t *d_sel, trxsig_c32 *d_chan, int32_t *d_win,
                                 float *d_soft, uint8_t *d_hard, int nsoft, int soft_stride);

/* ---- interference-rejection combining for the two-antenna sequence equaliser (csrc/trxsig_mlse_irc.hip) ---------------------
 * trxsig_mlse_irc_batch: trxsig_mlse_div_batch for a disturbance that is NOT white, equally strong and uncorrelated between the
 *   antennas -- a co-channel interferer reaches both antennas and its contributions there are correlated; unequal noise power per
 *   branch is the diagonal special case.  The 2 x 2 covariance R of the disturbance is estimated from the midamble residuals (or
 *   given by the caller) and the trellis runs on the whitened metric e^H R^-1 e, in a square-root-free LDL form: with
 *   R ~ [[A, x], [conj(x), Bv]], det = A Bv - |x|^2,  A det e^H R^-1 e = det |e_0|^2 + |A e_1 - conj(x) e_0|^2.
 *   Pinned by the float32 model tests/mlse_irc_model.py, which the kernel equals word for word, and graded against the float64
 *   statement tests/mlse_irc_ref.py with the a-priori bounds derived there:
 *     |soft - clamp(soft64)| <= 1.001 ((2 Q + 124 P) / (8 E_w) + e / 2 + 2) 2^-24   (P, Q: trxsig_mlse_div_batch's sums over the
 *         whitened metric, Q with the whitening's and the det multiply's roundings; e: the relative rounding of E_w in units
 *         of 2^-24, 7 there and at most 11 for the identity set),
 *     |S - S64| <= 1.001 (sum_m tau_m + 21 sum_m |term_m|) 2^-24   for S = S00, S11, Xr, Xi (tau_m: the rounding a term inherits
 *         from its residuals and its own operations).
 *   It is trxsig_mlse_div_batch's algorithm with the changes below and no others; every step is one float32 operation in the order
 *   written, nothing is fused.  Steps 1 and 2 are unchanged: the symbols, the correlations, the ONE window w chosen on the summed
 *   tap powers, h_a, E, the skip rule and the fall-back rule.
 *   2b. Residuals, on the 22 midamble positions whose five contributing symbols are all training symbols: for m = 65..86, x_m is
 *      the 5-bit index whose bit k is training bit m - 61 - k (a[m - k]); r_a[m] = y_a[m + w] - Z_a[x_m], Z_a formed from h_a
 *      exactly as step 3 forms the right half's expected values.  The sums start from 0, m ascending:
 *      S00 += r0.re*r0.re + r0.im*r0.im, S11 likewise from r1; Xr += r0.re*r1.re + r0.im*r1.im, Xi += r0.im*r1.re - r0.re*r1.im
 *      (X = sum r0 conj(r1)).
 *   2c. The set (A, Bv, xr, xi).  Estimated (d_cov_in NULL): tt = S00 + S11, A = S00/tt + loading, Bv = S11/tt + loading,
 *      xr = Xr/tt, xi = Xi/tt: four correctly rounded divisions per burst.  Given: the caller's four floats d_cov_in[b][0..3],
 *      taken as they are (no loading).  Either way det = A*Bv - (xr*xr + xi*xi).  The set is replaced by the identity set
 *      (1, 1, 0, 0) with det = 1 when !(tt > 0) (an estimated set only); when any of A, Bv, |xr|, |xi| fails v < 0x1p10f, or A or
 *      Bv fails v >= 0 (negative or NaN); or when !(det > 0).  The magnitude bound, with |y| < 2^30, keeps every metric finite.
 *   2d. Whitening, once per burst (the LDL form; no square root):
 *      y1'[n].re = A*y1[n].re - (xr*y0[n].re + xi*y0[n].im),  y1'[n].im = A*y1[n].im - (xr*y0[n].im - xi*y0[n].re);
 *      the same map takes (h0, h1) to h1'.  Antenna 0 is untouched.  pw[k] = det*(h0[k].re*h0[k].re + h0[k].im*h0[k].im) +
 *      (h1'[k].re*h1'[k].re + h1'[k].im*h1'[k].im); E_w = (((pw[0] + pw[1]) + pw[2]) + pw[3]) + pw[4].  If !(E_w > 0) or E_w is
 *      not finite the burst takes the identity set, and then E_w is E.
 *   3. Trellis: trxsig_mlse_div_batch's on (y0, y1') with (h0, h1'), with one change:
 *      gamma = det*(dr0*dr0 + di0*di0) + (dr1*dr1 + di1*di1).
 *   4. soft = clamp(0.5f + (M_0 - M_1) / (8.0f * E_w)).  Positions 61..86, and every fall-back, use the UNWHITENED y_p of the
 *      primary antenna, as there.
 *   Identities.  (1) d_cov_in = (1, 1, 0, 0) on every burst: soft, hard, win and chan equal trxsig_mlse_div_batch's bit for bit
 *   (1*v and v - 0 are exact).  (2) Antenna 1 all zeros and loading == 0: det is 0, the identity set is taken, and the outputs equal
 *   trxsig_mlse_batch's on antenna 0 bit for bit.  (3) Antenna 1 all zeros and loading > 0: the soft bits equal trxsig_mlse_batch's
 *   only up to the two roundings of det; the float64 reference grades that case.  The antenna-swap identity of
 *   trxsig_mlse_div_batch does NOT carry over exactly: the LDL form is not symmetric in the antennas (antenna 1 is the one that is
 *   whitened); it holds within the graded bound.
 *   loading  0 <= loading <= 16, else TRXSIG_EINVAL (a NaN too); the tools and the Transceiver groups use 1/64: the estimate is
 *            from 22 residuals, and a little loading keeps a near-singular estimate from nulling the wanted signal
 *   d_cov_in B x 4 floats (A, Bv, xr, xi) per burst, or NULL = estimate; the hook for covariance smoothing across bursts
 *   d_cov    B x 4: the set used -- (1, 1, 0, 0) where the identity set was taken, zeros for a burst that fell back or was
 *            skipped                                                                        (may be NULL)
 *   d_chan   B x 2 x 5: the UNWHITENED taps h_a[0..4]; d_win: as trxsig_mlse_div_batch        (may be NULL)
 * trxsig_mlse_irc_normal_batch: the detector on each antenna and the selection exactly as trxsig_mlse_div_normal_batch, then this
 *   equaliser with an estimated set.  Refusals are trxsig_mlse_div_batch's, and the loading's. */
int trxsig_mlse_irc_batch(trxsig_ctx *ctx,
                          const trxsig_c32 *d_samples0, const int32_t *d_offset0,
                          const trxsig_c32 *d_samples1, const int32_t *d_offset1,
                          const int32_t *d_length, int B, int tsc,
                          const trxsig_c32 *d_amp, const float *d_toa, const uint8_t *d_primary, const uint8_t *d_enable,
                          float loading, const float *d_cov_in, float *d_cov,
                          trxsig_c32 *d_chan, int32_t *d_win,
                          float *d_soft, uint8_t *d_hard, int nsoft, int soft_stride);
int trxsig_mlse_irc_normal_batch(trxsig_ctx *ctx,
                                 const trxsig_c32 *d_samples0, const int32_t *d_offset0,
                                 const trxsig_c32 *d_samples1, const int32_t *d_offset1,
                                 const int32_t *d_length, int B, int tsc,
                                 float detect_thresh, float energy_thresh, float loading,
                                 uint8_t *d_flags, trxsig_c32 *d_amp, float *d_toa, float *d_avgpwr,
                                 uint8_t *d_sel, float *d_cov, trxsig_c32 *d_chan, int32_t *d_win,
                                 float *d_soft, uint8_t *d_hard, int nsoft, int soft_stride);

/* ---- TX path: modulateBurst (sigProcLib.h:171-174) as called by Transceiver::addRadioVector
 *   (Transceiver.cpp:100-113): bits -> GMSK-rotated impulses -> pulse shaping, then scaleVector by
 *   a real gain.  d_bits: B x 148 bytes (only bit 0 is used, BitVector.cpp:54-63); d_guard[b] =
 *   guard period in symbols (8 or 9); output burst b at d_out[d_out_offset[b]..] with
 *   sps*(148+guard) samples; d_gain may be NULL (no scaling pass, as generateMidamble's use). */
int trxsig_modulate_batch(trxsig_ctx *ctx, const uint8_t *d_bits, const int32_t *d_guard,
                          const float *d_gain, int B,
                          trxsig_c32 *d_out, const int32_t *d_out_offset);

/* The two halves of trxsig_equalize_normal_batch (declared further down) on their own, for callers that keep the reference's per-timeslot cache
 * (Transceiver.cpp:317-349: channel estimate + DFE design only on the first burst of a slot or after 50
 * frames; every burst is then equalised with the cached taps):
 *   trxsig_estimate_dfe_batch: analyzeTrafficBurst(requestChannel) + scaleVector(chan, 1/amp) + designDFE, no
 *     energy gate; snr_thresh = the threshold in SNR = |amp|^2/(thr^2+1) (the reference uses mEnergyThreshold
 *     after its "-= 1" update, :338-340), or snr_value > 0 = the SNR estimate itself for every burst (a caller
 *     that forms it in the reference's double arithmetic).  d_chan_off = chanRespOffset, d_w: B x 7, d_b: B x 5.
 *   trxsig_equalize_taps_batch: scaleVector(burst, 1/amp) + equalizeBurst(burst, toa_eq, w, b) with the taps of
 *     burst b at d_w + 7b, d_b + 5b; d_enable[b] & TRXSIG_F_DETECT selects the bursts to process (zeros otherwise).
 *     The taps and the amplitude are the caller's and may be anything, Inf and NaN included: a feed-forward term that
 *     reaches beyond the burst (sample k + 6 - j >= length) is SKIPPED, as the reference's convolve skips it
 *     (sigProcLib.cpp:322-366), never formed as 0 * w[j] -- so with w[j] not finite the last 6 - j soft bits are the
 *     finite values the reference gives, and a NaN soft bit (hard bit 0) stands exactly where the reference's does. */
int trxsig_estimate_dfe_batch(trxsig_ctx *ctx, const trxsig_c32 *d_samples, const int32_t *d_offset,
                              const int32_t *d_length, int B, int tsc, float detect_thresh, float snr_thresh,
                              float snr_value, int variant52m, int max_toa, uint8_t *d_flags, trxsig_c32 *d_amp, float *d_toa,
                              float *d_chan_off, trxsig_c32 *d_w, trxsig_c32 *d_b);
int trxsig_equalize_taps_batch(trxsig_ctx *ctx, const trxsig_c32 *d_samples, const int32_t *d_offset,
                               const int32_t *d_length, int B, const trxsig_c32 *d_amp, const float *d_toa_eq,
                               const uint8_t *d_enable, const trxsig_c32 *d_w, const trxsig_c32 *d_b,
                               float *d_soft, uint8_t *d_hard, int nsoft, int soft_stride);
/* The same steps as the reference's free functions hand them to each other (sigProcLib.h:277-285, 372-384), for the
 * source-compatible facade:
 *   trxsig_channel_estimate_batch: analyzeTrafficBurst(..., requestChannel = true): flags/amp/TOA as the detect calls
 *     (no energy gate), d_chan_off = channelResponseOffset, d_chan = channelResponse (B x 6 taps, already divided by
 *     the midamble gain, sigProcLib.cpp:1024-1025; zeros for bursts that were not detected).
 *   trxsig_design_dfe_batch: designDFE(channelResponse, SNRestimate, Nf = 7, &w, &b) (sigProcLib.cpp:1246-1340) for B
 *     channel estimates; d_amp != NULL applies scaleVector(channelResponse, 1/amp) first (Transceiver.cpp:346),
 *     NULL = the caller has done that.  d_w: B x 7, d_b: B x 5. */
int trxsig_channel_estimate_batch(trxsig_ctx *ctx, const trxsig_c32 *d_samples, const int32_t *d_offset,
                                  const int32_t *d_length, int B, int tsc, float detect_thresh, int variant52m, int max_toa,
                                  uint8_t *d_flags, trxsig_c32 *d_amp, float *d_toa, float *d_chan_off, trxsig_c32 *d_chan);
int trxsig_design_dfe_batch(trxsig_ctx *ctx, const trxsig_c32 *d_chan, const trxsig_c32 *d_amp, const float *d_snr, int B,
                            trxsig_c32 *d_w, trxsig_c32 *d_b);
/* single-burst host-buffer forms (one PCIe round trip each; what include/sigProcLib_trx.h calls):
 * trxsig_equalize_taps_host = scaleVector(burst, 1/amp) + equalizeBurst(burst, toa_eq, 1, w, b) (sigProcLib.h:372-384);
 * pass amp = {1, 0} for a burst that is scaled already. */
int trxsig_channel_estimate_host(trxsig_ctx *ctx, const trxsig_c32 *h_samples, int n, int tsc, float detect_thresh,
                                 int variant52m, int max_toa, uint8_t *h_flags, trxsig_c32 *h_amp, float *h_toa,
                                 float *h_chan_off, trxsig_c32 h_chan[6]);
int trxsig_design_dfe_host(trxsig_ctx *ctx, const trxsig_c32 h_chan[6], float snr, trxsig_c32 h_w[7], trxsig_c32 h_b[5]);
int trxsig_equalize_taps_host(trxsig_ctx *ctx, const trxsig_c32 *h_samples, int n, trxsig_c32 amp, float toa_eq,
                              const trxsig_c32 h_w[7], const trxsig_c32 h_b[5], float *h_soft, int nsoft);

/* ---- rate conversion: polyphaseResampleVector (sigProcLib.h:352-354) -------------------------
 * S independent streams (one per ARFCN).  Stream s: input d_in + s*in_stride (n_in samples),
 * output d_out + s*out_stride, ceil(n_in*P/Q) samples each, exactly the reference's indexing
 * (sigProcLib.cpp:1171-1205).  d_lpf: L real taps on the device (createLPF output). */
int trxsig_resample_batch(trxsig_ctx *ctx, const trxsig_c32 *d_in, int n_in, int64_t in_stride,
                          int S, int P, int Q, const float *d_lpf, int L,
                          trxsig_c32 *d_out, int64_t out_stride);
int trxsig_resample_out_len(int n_in, int P, int Q);
/* one stream, host buffers (one PCIe round trip): returns the number of output samples, < 0 on error */
int trxsig_resample_host(trxsig_ctx *ctx, const trxsig_c32 *h_in, int n_in, int P, int Q, const float *h_lpf, int L,
                         trxsig_c32 *h_out, int out_capacity);

/* int16 I/Q <-> float: RadioInterface::unUSRPifyVector / USRPifyVector
 *   (radioInterface.cpp:74-116).  swap_iq = 1 reproduces the non-SWLOOPBACK I/Q flip on RX. */
int trxsig_unpack_int16(trxsig_ctx *ctx, const int16_t *d_iq, int64_t n_samples, int swap_iq,
                        trxsig_c32 *d_out);
int trxsig_pack_int16(trxsig_ctx *ctx, const trxsig_c32 *d_in, int64_t n_samples, int16_t *d_iq);
/* scaleVector(x, gain) + USRPifyVector in one pass: the tail of RadioInterface::pushBuffer
 *   (radioInterface.cpp:149-152; the reference uses gain = 13500.0). */
int trxsig_pack_int16_scaled(trxsig_ctx *ctx, const trxsig_c32 *d_in, int64_t n_samples, float gain, int16_t *d_iq);
/* IEEE binary16 I/Q pairs (the sample storage format of BASELINE config 5) -> float.  The reference has
 * no such format (its radio side is int16, radioInterface.cpp:74-116); widening is exact, so results
 * downstream equal the float pipeline's on the same values.  d_iq: 2*n_samples binary16 values. */
int trxsig_unpack_half(trxsig_ctx *ctx, const uint16_t *d_iq, int64_t n_samples, trxsig_c32 *d_out);

/* ---- equaliser: analyzeTrafficBurst(requestChannel) + designDFE + equalizeBurst ---------------
 *   (sigProcLib.h:277-285, 366-370, 382-386; Transceiver.cpp:327-349, 391-396; the windowed
 *   Transceiver52M form with maxTOA when variant52m != 0: Transceiver52M/sigProcLib.cpp:966-1076).
 *   sps must be 1 for equalizeBurst ("Assumes symbol-rate sampling", sigProcLib.cpp:1342).
 *   Per burst: detect + channel estimate; scale channel by 1/amp; SNR = |amp|^2/(thr^2+1);
 *   designDFE(chan, SNR, 7); equalizeBurst(burst/amp, TOA-chanOffset, w, b).  thr is the
 *   energy_thresh argument (the reference uses its adaptive mEnergyThreshold, whose sequential
 *   update stays with the caller: SURVEY 8a' item 14); energy_thresh < 0 disables the gate and
 *   uses thr = 0.  d_w: B x 7, d_b: B x 5 complex, written for detected bursts (may be NULL).
 *   max_toa (52M variant only): 0..17.  The 52M correlation window covers samples 66 - span .. 81 + span, span =
 *   max(max_toa, 5); the reference reads it unchecked.  A burst that passes the energy gate but is too short for the
 *   window (length < 82 + span: lengths 92..98 at the widest windows, max_toa 11..17) gets TRXSIG_F_BADLEN alone, amp = 0,
 *   TOA = 0 and zero soft bits -- in this call, trxsig_estimate_dfe_batch and trxsig_channel_estimate_batch alike. */
int trxsig_equalize_normal_batch(trxsig_ctx *ctx,
                                 const trxsig_c32 *d_samples, const int32_t *d_offset,
                                 const int32_t *d_length, int B,
                                 int tsc, float detect_thresh, float energy_thresh,
                                 int variant52m, int max_toa,
                                 uint8_t *d_flags, trxsig_c32 *d_amp, float *d_toa,
                                 trxsig_c32 *d_w, trxsig_c32 *d_b,
                                 float *d_soft, uint8_t *d_hard, int nsoft, int soft_stride);
/* The same with the bursts stored as fp16 I/Q pairs (BASELINE config 5): sample_format TRXSIG_SAMPLES_F16 = d_samples is
 * an array of half-precision {re, im} pairs (4 bytes per sample; d_offset / d_length still count samples),
 * TRXSIG_SAMPLES_C32 = complex float32 as above.  The kernels read the fp16 words themselves and widen in registers (exact),
 * so the results equal the float32 call on the same values bit for bit -- there is no float32 copy of the batch in HBM. */
enum { TRXSIG_SAMPLES_C32 = 0, TRXSIG_SAMPLES_F16 = 1 };
int trxsig_equalize_normal_batch_fmt(trxsig_ctx *ctx, const void *d_samples, int sample_format, const int32_t *d_offset,
                                     const int32_t *d_length, int B, int tsc, float detect_thresh, float energy_thresh,
                                     int variant52m, int max_toa, uint8_t *d_flags, trxsig_c32 *d_amp, float *d_toa,
                                     trxsig_c32 *d_w, trxsig_c32 *d_b, float *d_soft, uint8_t *d_hard, int nsoft,
                                     int soft_stride);
/* trxsig_equalize_taps_batch (cached DFE taps, Transceiver.cpp:391-396) on either sample storage */
int trxsig_equalize_taps_batch_fmt(trxsig_ctx *ctx, const void *d_samples, int sample_format, const int32_t *d_offset,
                                   const int32_t *d_length, int B, const trxsig_c32 *d_amp, const float *d_toa_eq,
                                   const uint8_t *d_enable, const trxsig_c32 *d_w, const trxsig_c32 *d_b, float *d_soft,
                                   uint8_t *d_hard, int nsoft, int soft_stride);

/* ---- convenience: host-buffer single-call wrappers (copy in, run, copy out, synchronise).
 *   These exist so Transceiver::pullRadioVector can keep calling one burst at a time; they are
 *   PCIe-inclusive and are never what bench.py times. */
int trxsig_detect_demod_normal_host(trxsig_ctx *ctx, const trxsig_c32 *h_samples,
                                    const int32_t *h_offset, const int32_t *h_length, int B,
                                    int tsc, float detect_thresh, float energy_thresh,
                                    uint8_t *h_flags, trxsig_c32 *h_amp, float *h_toa,
                                    float *h_avgpwr, float *h_soft, int nsoft, int soft_stride);
int trxsig_detect_demod_rach_host(trxsig_ctx *ctx, const trxsig_c32 *h_samples,
                                  const int32_t *h_offset, const int32_t *h_length, int B,
                                  float detect_thresh, float energy_thresh,
                                  uint8_t *h_flags, trxsig_c32 *h_amp, float *h_toa,
                                  float *h_avgpwr, float *h_soft, int nsoft, int soft_stride);
/* one burst, caller-supplied amp/TOA: demodulateBurst (sigProcLib.h:316-320).  TRXSIG_EINVAL for a burst outside the
 * accepted geometry (92..157 symbols, a multiple of sps samples) or |TOA| > 4096 / NaN -- the batch form writes zeros for
 * such a burst, the one-burst form refuses it (the reference itself handles any length). */
int trxsig_demodulate_host(trxsig_ctx *ctx, const trxsig_c32 *h_samples, int n_samples,
                           trxsig_c32 amp, float toa, float *h_soft, int nsoft);
int trxsig_modulate_host(trxsig_ctx *ctx, const uint8_t *h_bits, const int32_t *h_guard,
                         const float *h_gain, int B, trxsig_c32 *h_out, const int32_t *h_out_offset,
                         int64_t out_samples);

/* ---- L1 FEC soft decode: the consumer of the soft bits (next row after the burst path) ---------
 * SoftVector::decode with ViterbiR2O4 (rate 1/2, order 4, deferral 24; CommonLibs/BitVector.cpp:290-524),
 * the Parity shift registers (CommonLibs/BitVector.h:39-112) and the decoder flows of GSM/GSML1FEC.cpp.
 * d_soft is the soft-bit array the detect/demod calls produce: burst b at d_soft + b*soft_stride, 148
 * values in [0,1].  wire_quantise != 0 applies what the UDP hop does to them in the reference chain --
 * byte = (char)round(v*255.0) (Transceiver.cpp:669), v' = byte/256.0F (TRXManager.cpp:231) -- so the
 * result is what GSM::XCCHL1Decoder / RACHL1Decoder would have produced behind TRXManager.
 *
 * Values the demodulator never produces.  With wire_quantise == 0 (and in trxsig_fec_viterbi_batch and
 * trxsig_fec_sch_decode_batch, which have no such switch) any float32 word is accepted and decoded as
 * SoftVector::decode is written: a value outside [0,1], +-Inf included, goes through the metric clamps of
 * BitVector.cpp:481-485 and gives finite costs; a NaN makes every cost NaN from its trellis step on, and every
 * later step takes the last survivor (16th of 16), as the scan of BitVector.cpp:382-393 does when no comparison
 * holds.  Sliced values (TCH class 2, the stealing flag) are v > 0.5F, false for a NaN.  One block's output never
 * depends on another block's input.  With wire_quantise != 0 the result is unspecified for a value outside [0,1]
 * or a NaN: the reference's conversion (char)round(v*255.0) is undefined there.
 *
 * XCCH (SACCH/SDCCH/BCCH..., GSML1FEC.cpp:584-653): block k = bursts 4k..4k+3 in arrival order (the "B"
 *   index of GSM 05.03 4.1.4); e-bits = burst[3..59] and [88..144]; deinterleave, decode 456 -> 228,
 *   invert the 40 parity bits, Fire-code syndrome.  d_frames: 23 octets per block = d[] after LSB8MSB,
 *   packed MSB first (the L2 frame); d_ok[k] = 1 iff the syndrome is zero ("good frame").
 * RACH (GSML1FEC.cpp:475-514): one access burst per entry, e = burst[49..84]; decode 36 -> 18;
 *   d_tail_ok = the four tail bits are zero; d_bsic = the BSIC the parity word encodes (the caller
 *   compares it with its own, :493); d_ra = the 8-bit RA.
 * TCH/FACCH full rate (GSML1FEC.cpp:1030-1163): n_bursts consecutive bursts of one traffic channel; block m
 *   (m < n_bursts/4 - 1) spans bursts 4m..4m+7 through the diagonal deinterleaver.  d_tch: 33 octets per
 *   block = d[260] in GSM 05.03 order packed MSB first (the fixed g610BitOrder permutation into the
 *   vocoder frame is left to the caller); d_tch_good = class-1a parity and tail bits check (decodeTCH's
 *   `good` for a frame that is not stolen); d_stolen = the Hl stealing flag of the block's last burst;
 *   d_facch / d_facch_ok (optional, both or neither) = the XCCH decode of the same block, which the
 *   reference runs when the frame is stolen.  Bad-frame substitution (GSM 06.11, uses random()) stays
 *   with the caller.
 * Generic: n_blocks independent SoftVector::decode runs, n_soft (even, <= 1024) values in, n_soft/2 bits out
 *   (one per byte). */
int trxsig_fec_xcch_decode_batch(trxsig_ctx *ctx, const float *d_soft, int soft_stride, int n_blocks,
                                 int wire_quantise, uint8_t *d_frames, uint8_t *d_ok);
int trxsig_fec_rach_decode_batch(trxsig_ctx *ctx, const float *d_soft, int soft_stride, int n_bursts,
                                 int wire_quantise, uint8_t *d_tail_ok, uint8_t *d_bsic, uint8_t *d_ra);
/* XCCH L1 encode, the transmit-side mirror (XCCHL1Encoder::sendFrame/encode/interleave/transmit,
 * GSML1FEC.cpp:772-845): n_blocks L2 frames of 23 octets -> 4*n_blocks normal bursts of 148 bits, one bit per
 * byte, ready for trxsig_modulate_batch: e-bits at 3..59 / 88..144, zero tails, both stealing flags set, the
 * training sequence `tsc` at 61..86. */
int trxsig_fec_xcch_encode_batch(trxsig_ctx *ctx, const uint8_t *d_frames, int n_blocks, int tsc, uint8_t *d_bits);
int trxsig_fec_tch_decode_batch(trxsig_ctx *ctx, const float *d_soft, int soft_stride, int n_bursts,
                                int wire_quantise, uint8_t *d_tch, uint8_t *d_tch_good, uint8_t *d_facch,
                                uint8_t *d_facch_ok, uint8_t *d_stolen);
int trxsig_fec_viterbi_batch(trxsig_ctx *ctx, const float *d_soft, int n_soft, int64_t in_stride, int n_blocks,
                             uint8_t *d_bits, int64_t out_stride);

/* ---- GPRS packet data channel: the block coders CS-1..CS-4 (GSM 05.03 5.1) ------------------------------------------
 * One radio block = four normal bursts, as XCCH: the same rate-1/2 K = 5 coder (BitVector::encode), the same 456-bit
 * rectangular interleaver (GSM 05.03 4.1.4: c[k] in burst k mod 4 at e-bit j = 2 ((49 k) mod 57) + (k mod 8) / 4, e-bits at
 * 3..59 and 88..144), the same SoftVector::decode and the same wire_quantise.  The reference has no packet channel.
 * NOT CHECKED AGAINST THE STANDARD: the tables, the puncturing and the flag words below are written from memory of GSM 05.03;
 * no copy of it was at hand.  What follows from them is pinned by tests/test_pdtch_model.py: the bit counts close (456 each
 * way), the 6-bit and 12-bit tables are linear codes of minimum distance 3 and 5, the four flag words are at least 5 apart,
 * and CS-1 is the XCCH coder bit for bit.  tests/pdtch_model.py is this statement in numpy.
 *
 * Payload.  Scheme cs = TRXSIG_CS1..TRXSIG_CS4 carries K = 184 / 271 / 315 / 431 information bits d(0..K-1) in 23 / 34 / 40 /
 *   54 octets; a block is a row of TRXSIG_PDTCH_BLOCK_BYTES = 54 octets whatever its scheme.  d(k) is bit k mod 8 of octet
 *   k / 8, counted from the least significant bit (what LSB8MSB makes of XCCH's 23 octets: a CS-1 block is an XCCH frame).  The
 *   spare high bits of the last octet are ignored on encode and written 0 on decode; octets past the scheme's size are ignored
 *   on encode and written 0 on decode.  usf = d(0) | d(1) << 1 | d(2) << 2.
 * Block check, CS-2..4.  p(0..15) with g(D) = D^16 + D^12 + D^5 + 1: d(0) D^(K+15) + ... + d(K-1) D^16 + p(0) D^15 + ... +
 *   p(15) leaves the all-ones remainder -- Parity(0x11021, 16, K) with the inverted parity word written most significant
 *   bit first, as XCCH and SCH use theirs.  It is computed on d, before the pre-coding.
 * USF pre-coding.  Row d(0) d(1) d(2) (a string: d(0) first) of
 *     000  001  010  011  100  101  110  111
 *   CS-2 / CS-3: 000000 001011 010110 011101 100101 101110 110011 111000
 *   CS-4: 000000000000 000011011101 001101110110 001110101011 110100001011 110111010110 111001111101 111010100000
 *   the first character being the first bit sent.
 * Code word c[456].
 *   CS-1: XCCH's, word for word: u = d(0..183), 40 inverted Fire parity bits, 0000; c = the coder's 456 bits.
 *   CS-2: u' = precoded(6), d(3..270), p(0..15), 0000 (294 bits); the coder gives C(0..587); C(3 + 4j) is deleted for j = 3..146
 *     except j = 9, 21, 33, ..., 141 (j = 9 mod 12): 132 deleted, 456 left, in order.
 *   CS-3: u' = precoded(6), d(3..314), p(0..15), 0000 (338 bits); C(0..675); C(3 + 6j) and C(5 + 6j) are deleted for j = 2..111:
 *     220 deleted, 456 left.
 *   CS-4: c = precoded(12), d(3..430), p(0..15), uncoded.
 * Bursts.  c[] through XCCH's interleaver; zero tails; training sequence d_tsc[k] at 61..86; the eight stealing flags carry
 *   q(0..7) in the order XCCH's interleaver places its flags: q(2B) is bit 87 and q(2B + 1) bit 60 of burst B.
 *     CS-1 11111111   CS-2 11001000   CS-3 00100001   CS-4 00010110
 *   CS-1's four bursts equal trxsig_fec_xcch_encode_batch's byte for byte.
 * Encode: d_blocks [n][54], d_cs [n], d_tsc [n] -> d_bits [n][4][148], one bit per byte.  A block whose d_cs is above 3 or
 *   whose d_tsc is above 7 encodes as four all-zero bursts.
 * Decode.  Burst t of block k is row d_index[k][t] of d_soft (148 values at d_soft + row * soft_stride); d_index == NULL means
 *   rows 4k..4k+3.  A row outside [0, n_rows) means the burst is missing: all its values, flags included, are exactly 0.5.
 *   Present values pass the UDP hop first when wire_quantise != 0.  Values the demodulator never produces behave as the
 *   paragraph above says for XCCH; a sliced value (a flag, a CS-4 bit) is v > 0.5F, false for a NaN.
 *   Scheme: cs_force in 0..3, or -1 to detect: hard flags q(i) = v > 0.5F, the Hamming distance to the four words, the
 *     smallest, ties to the lower scheme.  d_cs = the scheme decoded with, d_cs_dist = the hard flags' distance to its word
 *     (with cs_force that of the forced scheme).
 *   CS-1: the XCCH decoder; ok = the Fire syndrome is zero; octets 0..22 equal trxsig_fec_xcch_decode_batch's frame.
 *   CS-2 / CS-3: the 588 / 676 coder outputs with the deleted positions reading exactly 0.5F; SoftVector::decode gives u'
 *     (294 / 338 bits).  Its first 6 bits go to the nearest row of the table (Hamming distance, ties to the first row), which
 *     gives d(0..2); the rest of d is copied; ok = the block check on that d against the received p.  The tail bits are not
 *     checked (XCCH does not check its own).
 *   CS-4: v > 0.5F on all 456; the first 12 go to the nearest row; ok = the block check.
 *   Outputs: d_blocks [n][54], d_cs [n], d_cs_dist [n], d_ok [n], d_usf [n]; any but d_blocks may be NULL.  One block's output
 *   never depends on another block's input.
 * Host side: a NULL context or required pointer, a negative size, n_blocks > TRXSIG_PDTCH_MAX_BLOCKS, soft_stride < 148,
 *   cs_force outside -1..3 or a d_index not 4-byte aligned return TRXSIG_EINVAL before any launch; n_blocks == 0 is a no-op.
 *   One launch each (k_fec_pdtch_encode, k_fec_pdtch_decode; DESIGN.md 5.4.x, GPRS packet data blocks), booked under TRXSIG_K_FEC.
 * trxsig_pdch_map_host: frame fn of the 52-multiframe (fn mod 52) -> *block = 0..11 (B0..B11: frames 0-3, 4-7, 8-11, 13-16,
 *   17-20, 21-24, 26-29, 30-33, 34-37, 39-42, 43-46, 47-50) and *burst = 0..3; frames 12 and 38 (PTCCH) and 25 and 51 (idle)
 *   give -1 in both.  A negative fn or a NULL pointer returns TRXSIG_EINVAL. */
enum { TRXSIG_CS1 = 0, TRXSIG_CS2 = 1, TRXSIG_CS3 = 2, TRXSIG_CS4 = 3 };
#define TRXSIG_PDTCH_BLOCK_BYTES 54
#define TRXSIG_PDTCH_MAX_BLOCKS 16777216    /* 2^24 blocks a call */
int trxsig_fec_pdtch_encode_batch(trxsig_ctx *ctx, const uint8_t *d_blocks, const uint8_t *d_cs, const uint8_t *d_tsc,
                                  int n_blocks, uint8_t *d_bits);
int trxsig_fec_pdtch_decode_batch(trxsig_ctx *ctx, const float *d_soft, int soft_stride, int64_t n_rows, const int32_t *d_index,
                                  int n_blocks, int wire_quantise, int cs_force, uint8_t *d_blocks, uint8_t *d_cs,
                                  uint8_t *d_cs_dist, uint8_t *d_ok, uint8_t *d_usf);
int trxsig_pdch_map_host(int32_t fn, int *block, int *burst);

/* ---- the access burst's coders, both formats (GSM 05.03 4.6 and 5.3.2) ------------------------------------------------
 * What a handset sends before it has a channel: the 8-bit access burst of the RACH and, on a packet data channel (PRACH,
 * PTCCH/U), either that or the 11-bit packet access burst.  One burst of 148 bits, laid out as trxsig_l1ms.h states it: bits
 * 0..7 the extended tail, 8..48 the 41-bit synch sequence (GSM 05.02 5.2.7), 49..84 the 36 coded bits e(0..35), the rest zero.
 * TRXSIG_ACCESS_8 (GSM 05.03 4.6, the reference's RACHL1Decoder read backwards): d(0..7) = the RA, least significant bit
 *   first; p = ~(bsic ^ parity) in six bits, most significant first, parity = Parity(0x6f, 6, 8) over d; four zero tail bits;
 *   u(0..17) through the rate-1/2 coder gives e(0..35).  The encoder writes the bytes trxsig_l1ms_encode writes for an access
 *   burst, the decoder returns what trxsig_fec_rach_decode_batch returns.
 * TRXSIG_ACCESS_11 (GSM 05.03 5.3.2): d(0..10) = the 11-bit word, least significant bit first; six parity bits by the same
 *   generator over d(0..10), coloured with the BSIC and written the same way; four zero tail bits give u(0..20); the same coder
 *   gives C(0..41); C(0), C(2), C(5), C(37), C(39) and C(41) are not sent, which leaves e(0..35), in order.
 *   NOT CHECKED AGAINST THE STANDARD: these six positions and the bit order of d and p are written from memory of GSM 05.03;
 *   no copy of it was at hand.  What follows from them is pinned by tests/test_access_model.py: 21 -> 42 -> 36 bits, the
 *   punctured code's minimum weight over its 2^11 - 1 nonzero words is 7, every word comes back from clean bits, and after
 *   any single flipped bit the word and the BSIC still do.  The tail bits do not always: SoftVector::decode does not end its
 *   trellis in the zero state, so a flip in e(31..35) -- in e(34..35) of the 8-bit format, the reference's own -- comes out as
 *   a nonzero tail bit.  tests/access_model.py is this statement in numpy on the oracle's coder and decoder.
 * Encode: d_ra [n] (uint16), d_fmt [n], d_bsic [n] -> d_bits [n][148], one bit per byte.  A d_fmt above 1, a d_bsic above 63 or
 *   a d_ra that does not fit its format (above 255 / 2047) encodes as an all-zero row.
 * Decode.  Burst k is row d_index[k] of d_soft (values 49..84 of d_soft + row * soft_stride are read); d_index == NULL means
 *   row k.  A row outside [0, n_rows) means the burst is missing: its 36 values are exactly 0.5.  Present values pass the UDP
 *   hop first when wire_quantise != 0.  Values the demodulator never produces behave as the paragraph above says for XCCH.
 *   fmt 0: SoftVector::decode of e(0..35) into u(0..17).  fmt 1: the 42 coder outputs with the six deleted positions reading
 *   exactly 0.5F, decoded into u(0..20).  Either way d_ra = d as a number, d_tail_ok = the four tail bits are zero, d_bsic = the
 *   BSIC the parity word encodes, ~p ^ parity(d) (the caller compares it with its own), d_fmt = fmt.
 *   fmt -1 (either): both hypotheses are decoded.  A hypothesis holds if its tail bits are zero and its parity gives `bsic`
 *   (0..63; not looked at for fmt 0 or 1).  The result is the 11-bit one only if it holds and the 8-bit one does not; otherwise
 *   the 8-bit one -- ties to the lower scheme, as the PDTCH decoder's vote.  All four outputs are the chosen hypothesis's.
 *   Ten bits decide whether a hypothesis holds, so about one clean 11-bit word in 2^10 also holds as an 8-bit burst of the
 *   same cell and is returned as that (3 of the 8192 that tests/test_access_model.py tries); a cell that uses one format
 *   passes it as fmt.
 *   Outputs: d_ra [n] (uint16), d_fmt [n], d_tail_ok [n], d_bsic [n]; any but d_ra may be NULL.  One burst's output never
 *   depends on another burst's input.
 * Host side: a NULL context or required pointer, a negative size, n > TRXSIG_ACCESS_MAX_BURSTS, soft_stride < 85, fmt outside
 *   -1..1, bsic outside 0..63 with fmt -1, a d_index not 4-byte aligned or a d_ra not 2-byte aligned return TRXSIG_EINVAL
 *   before any launch; n == 0 is a no-op.  One launch each (k_fec_access_encode, k_fec_access_decode; a row of 16 lanes per
 *   code word, four rows a wave, through the trellis every decoder here shares), booked under TRXSIG_K_FEC. */
enum { TRXSIG_ACCESS_8 = 0, TRXSIG_ACCESS_11 = 1 };
#define TRXSIG_ACCESS_MAX_BURSTS 16777216    /* 2^24 bursts a call */
int trxsig_fec_access_encode_batch(trxsig_ctx *ctx, const uint16_t *d_ra, const uint8_t *d_fmt, const uint8_t *d_bsic, int n,
                                   uint8_t *d_bits);
int trxsig_fec_access_decode_batch(trxsig_ctx *ctx, const float *d_soft, int soft_stride, int64_t n_rows, const int32_t *d_index,
                                   int n, int wire_quantise, int fmt, int bsic, uint16_t *d_ra, uint8_t *d_fmt, uint8_t *d_tail_ok,
                                   uint8_t *d_bsic);

/* ---- uplink TCH/FACCH and XCCH decoders as multi-channel streams ---------------------------------------------------
 * The reference's per-channel decoders -- TCHFACCHL1Decoder::processBurst / deinterleave / decodeTCH up to the parity and
 * tail check (GSML1FEC.cpp:1030-1163) and XCCHL1Decoder::writeLowSide / processBurst / deinterleave / decode (:556-653) --
 * for n_chan channels x n_slots burst slots per call, their deinterleaving buffer mI[][] and FER carried on the device.
 *   Slots: slot t of channel s is the burst at d_soft + d_index[s][t] * soft_stride (148 soft values).  An index of -1 --
 *     or any index outside [0, n_rows) -- means no burst arrived in that slot (detection failed, the pull returned
 *     nothing, the channel was idle).  d_soft / n_rows may be a trxsig_trxgroup_result's d_soft / n_rows: d_index[s][t] =
 *     the row of the channel's timeslot where d_valid is set, -1 elsewhere.
 *   B index: TCH: B = (d_b0[s] + t) mod 8, d_b0[s] in {0, 4} (NULL: all 0); XCCH: B = t mod 4.  Mapping a frame number to B
 *     (reverseMapping) is the caller's.  n_slots is a multiple of 4: n_blocks = n_slots / 4 blocks, block m closing at slot
 *     4m+3 (B = 3 or 7).  A channel whose d_b0 is neither 0 nor 4 is treated as one where no burst arrived in any slot:
 *     nothing is decoded, its FER and its state stay as they are.
 *   Per block, exactly as the reference: a present burst's 114 e-bits (after the UDP hop when wire_quantise != 0, as in
 *     the batch forms) enter row B of mI; a block is decoded only if its closing burst is present, reading c[] through
 *     the deinterleaver and marking what it read as 0.5 (a block whose closing burst is missing is never deinterleaved,
 *     and its rows stay for a later block to read).  TCH: stolen = Hl (bit 60 after the UDP hop) of the closing burst
 *     > 0.5; a stolen block runs the FACCH (XCCH) decode, any other decoded block the class-1 decode -- one Viterbi pass.
 *   Outputs, [n_chan][n_blocks] (any alignment): d_status = TRXSIG_FEC_* bits: DECODED; STOLEN; FACCH_OK (the FACCH
 *     frame's parity); TCH_GOOD (decodeTCH's `good`; for XCCH the parity of the L2 frame).  d_tch [..][33] = d[260] as
 *     trxsig_fec_tch_decode_batch writes it, for every decoded block that is not stolen, good or bad.  d_facch / d_frames
 *     [..][23] = the L2 frame, for every decoded stolen (TCH) or decoded (XCCH) block.  Every other output block is zero.
 *     d_fer [..] (float, may be NULL) = mFER after the block (L1Decoder::countGoodFrame / countBadFrame, :390-405, float
 *     arithmetic as written).  Count order as the reference: a stolen block counts its FACCH frame, then one bad traffic
 *     frame (decodeTCH(true) returns false); a block that is not decoded does not count.
 *   d_state[s] (in / out, TRXSIG_TCH_RX_STATE_BYTES / TRXSIG_XCCH_RX_STATE_BYTES per channel, 4-byte aligned): mI as the
 *     reference holds it after the call's last slot, and mFER.  Bytes 0..3 are mFER as a float: zeroing them is
 *     L1Decoder::open() (FER reset, mI kept).  The rest is opaque.  All-zero bytes are a freshly constructed decoder (mI
 *     filled with 0.0, mFER 0).  The call reads the old state and writes the new one in place, race-free: one call of n
 *     blocks equals k calls of n/k, in every output and in the state byte for byte.
 *   Host side: a NULL d_soft / d_index / d_state / d_status / d_tch / d_facch / d_frames, a negative size, n_slots not a
 *     multiple of 4, soft_stride < 148, n_chan * n_slots >= 2^31 or a d_state not 4-byte aligned return TRXSIG_EINVAL
 *     before any launch; n_chan == 0 or n_slots == 0 is a no-op.  The blocks of a call decode in parallel (a closed form of
 *     mI): two launches on the context's stream. */
enum { TRXSIG_FEC_DECODED = 1, TRXSIG_FEC_STOLEN = 2, TRXSIG_FEC_FACCH_OK = 4, TRXSIG_FEC_TCH_GOOD = 8 };
#define TRXSIG_TCH_RX_STATE_BYTES 3664      /* 16 + 8 x 114 floats */
#define TRXSIG_XCCH_RX_STATE_BYTES 1840     /* 16 + 4 x 114 floats */
int trxsig_fec_tch_decode_stream(trxsig_ctx *ctx, int n_chan, int n_slots, const float *d_soft, int soft_stride, int64_t n_rows,
                                 const int32_t *d_index, const uint8_t *d_b0, int wire_quantise, void *d_state,
                                 uint8_t *d_status, uint8_t *d_tch, uint8_t *d_facch, float *d_fer);
int trxsig_fec_xcch_decode_stream(trxsig_ctx *ctx, int n_chan, int n_slots, const float *d_soft, int soft_stride, int64_t n_rows,
                                  const int32_t *d_index, int wire_quantise, void *d_state, uint8_t *d_status,
                                  uint8_t *d_frames, float *d_fer);

/* ---- downlink L1 encode of traffic and sync channels ------------------------------------------------------
 * TCH/FS + FACCH/F stream encoder (TCHFACCHL1Encoder::dispatch / encodeTCH / interleave, GSML1FEC.cpp:1252-1393):
 *   n_chan channels x n_blocks 20-ms blocks per call, the interleaver state carried from call to call.
 *   d_kind[s][m]: what block m of channel s carries -- TRXSIG_TCH_SPEECH: d_payload[s][m][0..33) = d[260] in GSM 05.03
 *     order, packed MSB first (exactly what trxsig_fec_tch_decode_batch writes to d_tch; the g610BitOrder permutation
 *     of the vocoder frame stays with the caller, as on the decode side).  TRXSIG_TCH_FACCH: d_payload[s][m][0..23) =
 *     the 23-octet L2 frame trxsig_fec_xcch_encode_batch takes (octets 23..32 are ignored); the block is stolen (Hu
 *     set, and Hl of the next block).  TRXSIG_TCH_FILLER: the context's filler c[] (trxsig_fec_tch_set_filler).
 *     The kind of every block is the caller's choice: the reference's priority rule (FACCH, then speech, then
 *     filler) and its speech-queue latency control (mMaxQSize) are queue policy and stay with the host.
 *   d_tsc[s] (0..7): the channel's training sequence.  d_bits[s][m][4][148]: the block's four normal bursts, one bit
 *     per byte, ready for trxsig_modulate_batch / trxsig_trx_add_radio_vector: zero tails, e-bits at 3..59 and
 *     88..144, Hl (bit 60) = the previous block's FACCH flag, the training sequence at 61..86, Hu (bit 87) = this
 *     block's FACCH flag.  Burst b of block m carries this block's c[k], k = b mod 8, at the even e-bit positions and
 *     the previous block's c[k], k = b+4 mod 8, at the odd ones (GSM 05.03 3.1.3).
 *   d_state[s][TRXSIG_TCH_TX_STATE_BYTES] (in / out): what the encoder carries from one block to the next.  Bytes
 *     0..28 hold the odd half of the previous block's c[] -- the 228 bits c[k] with k mod 8 >= 4 in increasing k,
 *     bit i in byte i/8 at weight 1 << (i mod 8); byte 29 = the previous block's FACCH flag (mPreviousFACCH);
 *     bytes 30..31 are written as zero.  All-zero bytes are a freshly constructed encoder (mI[] zero-filled,
 *     mPreviousFACCH false).  The call reads the old state and writes the new one (after block n_blocks-1) in
 *     place, race-free: one call of n blocks equals k calls of n/k.  Treat the layout as opaque.
 *   Bad inputs (device side, deterministic): a channel whose d_tsc is above 7 gets all-zero bursts and its state is
 *     left untouched; a block whose kind is above 2 encodes as an all-zero c[] that is not stolen, and its bursts (and
 *     its successor's) are formed normally.  Host side: a NULL pointer, a negative size or n_chan * n_blocks >= 2^31
 *     returns TRXSIG_EINVAL before any launch; n_chan == 0 or n_blocks == 0 is a no-op.
 * trxsig_fec_tch_set_filler: the 456 bits (one per byte, low bit used) the encoder sends in a block of kind
 *   TRXSIG_TCH_FILLER.  The reference's pattern (a capture, GSML1FEC.cpp:1348) is not a GSM constant and is not built
 *   in: the default is all zero, and an integrator who wants the reference's behaviour passes its pattern at set-up.
 *   Synchronises the context's stream (blocks already enqueued keep the filler they were enqueued with).
 * SCH encoder (SCHL1Encoder::generate, GSML1FEC.cpp:879-920): n (d_fn[i], d_bsic[i]) -> d_bits[i][148]: d[25] =
 *   BSIC (6 bits), T1 (11), T2 (5), T3' (3), MSB first; LSB8MSB (the first three octets: bit 24 stays); 10 inverted
 *   parity bits (generator 0x575); 4 zero tail bits; rate-1/2 coder; e[0..39) at 3..41, the extended training
 *   sequence (GSM 05.02 5.2.5) at 42..105, e[39..78) at 106..144, zero tails.  T1 / T2 / T3' follow GSMCommon.h:465-474
 *   for any FN, including T3' = (T3 - 1) / 10 in unsigned arithmetic (its low 3 bits are 1 at T3 = 0; the reference
 *   itself only sends SCH at T3 = 1, 11, 21, 31, 41).  An FN outside [0, 2715648) or a BSIC above 63 gives a zero
 *   burst.  FCCH bursts are 148 zero bits and need no kernel. */
enum { TRXSIG_TCH_FILLER = 0, TRXSIG_TCH_SPEECH = 1, TRXSIG_TCH_FACCH = 2 };
#define TRXSIG_TCH_TX_STATE_BYTES 32
int trxsig_fec_tch_set_filler(trxsig_ctx *ctx, const uint8_t *h_c456);
int trxsig_fec_tch_encode_batch(trxsig_ctx *ctx, int n_chan, int n_blocks, const uint8_t *d_kind, const uint8_t *d_payload,
                                const uint8_t *d_tsc, void *d_state, uint8_t *d_bits);
int trxsig_fec_sch_encode_batch(trxsig_ctx *ctx, const uint32_t *d_fn, const uint8_t *d_bsic, int n, uint8_t *d_bits);
/* SCH decoder, the inverse of trxsig_fec_sch_encode_batch (the reference, a base station, has none: the arithmetic is the one
 * trxsig_l1msrx.h states for its SCH entries, and the device code is shared with it).  Row i = the burst's 148 soft values at
 * d_soft + i * soft_stride, as they are (no UDP hop): e[0..39) = values 3..41, e[39..78) = 106..144; SoftVector::decode gives
 * u[39]; d_ok[i] = the four tail bits are zero and u[25..35) is the inverted parity (generator 0x575) of u[0..25); LSB8MSB is
 * undone on the first three octets; d_bsic[i] = BSIC (6 bits), and d_rfn[i] = 1326 T1 + 51 ((T3 - T2) mod 26) + T3 with T3 =
 * 10 T3' + 1 from T1 (11) T2 (5) T3' (3), all MSB first -- written whether or not the parity holds.  soft_stride >= 148;
 * d_rfn 4-byte aligned; n == 0 is a no-op. */
int trxsig_fec_sch_decode_batch(trxsig_ctx *ctx, const float *d_soft, int soft_stride, int n, uint8_t *d_ok, uint8_t *d_bsic,
                                int32_t *d_rfn);

/* ---- the free-standing vector primitives of sigProcLib.h (csrc/trxsig_prim.hip) -------------------------------
 * On the burst path these only run fused into the burst kernels above; the stand-alone forms complete the
 * sigProcLib.h surface (convolve :126, correlate :162, vectorSlicer :168, delayVector :180, interpolatePoint :198,
 * peakDetect :208, scaleVector :215, decimateVector :304 of Transceiver/sigProcLib.h; GMSKRotate / GMSKReverseRotate
 * are sigProcLib.cpp:232-264) and are what config 1's call sequence (Transceiver/sigProcLibTest.cpp) runs through.
 * Batch forms: B independent vectors packed in one device array (d_off / d_len in samples); max_len = the largest
 * d_len (sizes the launch).  Values are the reference's, bit for bit: every sum in the reference's order with its
 * skip / break rules.  Host forms: one vector, pageable host buffers, one PCIe round trip.
 * span: ConvType of sigProcLib.h:41-48 (+ CUSTOM of Transceiver52M/sigProcLib.h:47 with cust_start / cust_len).
 * flags: bit 0 = a is real-only, bit 1 = b is real-only (signalVector::isRealOnly: the four arithmetic forms of
 * sigProcLib.cpp:326-365), bit 2 = b has ABSSYM symmetry (:369-398; convolve only); correlate != 0: b is used reversed and conjugated (sigProcLib.cpp:474-503). */
enum { TRXSIG_FULL_SPAN = 0, TRXSIG_OVERLAP_ONLY = 1, TRXSIG_START_ONLY = 2, TRXSIG_WITH_TAIL = 3, TRXSIG_NO_DELAY = 4,
       TRXSIG_CUSTOM = 5 };
int trxsig_convolve_out_len(int La, int Lb, int span, int cust_len);   /* < 0: unknown span */
/* one filter d_b (Lb taps) for all B vectors; out vector i (trxsig_convolve_out_len(d_a_len[i], ...) samples) at d_out_off[i] */
int trxsig_convolve_batch(trxsig_ctx *ctx, const trxsig_c32 *d_a, const int32_t *d_a_off, const int32_t *d_a_len, int B,
                          int max_len, const trxsig_c32 *d_b, int Lb, int span, int flags, int correlate, int cust_start,
                          int cust_len, trxsig_c32 *d_out, const int32_t *d_out_off);
int trxsig_convolve_host(trxsig_ctx *ctx, const trxsig_c32 *h_a, int La, const trxsig_c32 *h_b, int Lb, int span, int flags,
                         int correlate, int cust_start, int cust_len, trxsig_c32 *h_out, int out_cap);   /* returns the length */
/* A delay or an index beyond +-TRXSIG_MAX_INDEX (2^24: a float there has no fractional bits left), an infinity or a NaN is
 * one the reference's table-sinc range reduction (sigProcLib.cpp:163-188, reached from :573-616 and :639-659) cannot reduce
 * -- its `arg -= 1` loop no longer changes arg, the call never returns.  The host forms answer TRXSIG_EINVAL before any
 * launch; the batch forms (the values are on the device) write zeros for such a vector / point.  The device-side reduction
 * itself is loop-free (csrc/trxsig_dev.h, dev_range_reduce), so no argument can keep a wave running. */
#define TRXSIG_MAX_INDEX 16777216.0f
/* delayVector(x, delay): d_out has d_in's layout and must not overlap it */
int trxsig_delay_vector_batch(trxsig_ctx *ctx, const trxsig_c32 *d_in, const int32_t *d_off, const int32_t *d_len, int B,
                              const float *d_delay, int real_only, trxsig_c32 *d_out);
int trxsig_delay_vector_host(trxsig_ctx *ctx, trxsig_c32 *h_x /* in place */, int n, float delay, int real_only);
/* interpolatePoint(x_i, d_ix[i]) -> d_out[i] */
int trxsig_interpolate_point_batch(trxsig_ctx *ctx, const trxsig_c32 *d_in, const int32_t *d_off, const int32_t *d_len, int B,
                                   const float *d_ix, int real_only, trxsig_c32 *d_out);
int trxsig_interpolate_point_host(trxsig_ctx *ctx, const trxsig_c32 *h_x, int n, float ix, int real_only, trxsig_c32 *h_out);
/* peakDetect(x_i, &d_index[i], &d_avgpwr[i]) -> d_peak[i]; d_index / d_avgpwr may be NULL */
int trxsig_peak_detect_batch(trxsig_ctx *ctx, const trxsig_c32 *d_in, const int32_t *d_off, const int32_t *d_len, int B,
                             trxsig_c32 *d_peak, float *d_index, float *d_avgpwr);
int trxsig_peak_detect_host(trxsig_ctx *ctx, const trxsig_c32 *h_x, int n, trxsig_c32 *h_peak, float *h_index, float *h_avgpwr);
/* energyDetect(x_i, window, thresh, &d_avgpwr[i]) -> d_ok[i] (sigProcLib.h:255-258) for any window length; sample_step 1
 * (Transceiver/) or 4 (the Transceiver52M variant, Transceiver52M/sigProcLib.cpp:946-963).  d_avgpwr / d_ok may be NULL. */
int trxsig_energy_detect_batch(trxsig_ctx *ctx, const trxsig_c32 *d_in, const int32_t *d_off, const int32_t *d_len, int B,
                               unsigned window, int sample_step, float thresh, float *d_avgpwr, uint8_t *d_ok);
int trxsig_energy_detect_host(trxsig_ctx *ctx, const trxsig_c32 *h_x, int n, unsigned window, int sample_step, float thresh,
                              float *h_avgpwr);   /* returns 1 / 0 (the reference's bool), < 0 on error */
/* in place: scaleVector(x_i, d_scale[i]); GMSKRotate / GMSKReverseRotate (elements past the 157*sps table entries are
 * left as they are -- the reference reads past its table there); vectorSlicer */
int trxsig_scale_vector_batch(trxsig_ctx *ctx, trxsig_c32 *d_x, const int32_t *d_off, const int32_t *d_len, int B, int max_len,
                              const trxsig_c32 *d_scale, int real_only);
int trxsig_gmsk_rotate_batch(trxsig_ctx *ctx, trxsig_c32 *d_x, const int32_t *d_off, const int32_t *d_len, int B, int max_len,
                             int reverse, int real_only);
int trxsig_vector_slicer_batch(trxsig_ctx *ctx, trxsig_c32 *d_x, const int32_t *d_off, const int32_t *d_len, int B, int max_len);
/* decimateVector(x_i, factor): d_len[i] / factor samples at d_out_off[i] (d_len[i] must be a multiple of factor: the
 * reference writes past its allocation otherwise, sigProcLib.cpp:1045-1050) */
int trxsig_decimate_batch(trxsig_ctx *ctx, const trxsig_c32 *d_in, const int32_t *d_off, const int32_t *d_len, int B, int max_len,
                          int factor, trxsig_c32 *d_out, const int32_t *d_out_off);
/* ---- the rest of sigProcLib.h: the functions no caller on the burst path uses, for a complete surface -------------------
 * dB (sigProcLib.h:102; sigProcLib.cpp:88-114) and dBinv (:105; :117-144): the reference's piecewise-linear float
 *   approximations, on the host (scalar functions of one float).  sinc (:177; :567-571) against the context's trig table.
 * gaussianNoise (:188-190; :618-637): Box-Muller on the C library's rand(), two draws per sample in the reference's
 *   order (more after a zero draw) -- the caller's srand() seed decides the values, as with the reference.  Host.
 * vectorNorm2 / vectorPower (:108, 111; :146-160): the powers summed in index order; d_norm2 / d_power may be NULL.
 * frequencyShift (:149-153; :432-471): y[k] = x[k] * expjLookup(phase_k) (real-only x: expjLookup(phase_k) * x[k].real()),
 *   phase_0 = start_phase, phase_{k+1} = phase_k + freq in float; d_final_phase[i] (optional) = the phase after the last
 *   sample.  d_out may be d_in.  The reference's range reduction is a subtract-one loop that never ends for a float too large
 *   to change by 1: phases beyond +-25000 rad (|start| + n |freq|) are refused by the host forms (TRXSIG_EINVAL); the batch
 *   form bounds the loop instead and its values beyond that range are unspecified.
 * addVector (:184-185; :746-758): x[k] += y[k] over the shorter of the two, in place.
 * offsetVector (:225-226; :760-777): x[k] += offset (real-only x: x[k] = offset + x[k].real()), in place.
 * resampleVector (:352-354; :1213-1243) AS THE REFERENCE BEHAVES: its loop never advances the output iterator, so every
 *   interpolated value lands in element 0 and the other ceil(n * exp_factor) - 1 elements stay zero.  exp_factor >= 1 (NULL in
 *   the reference otherwise: TRXSIG_EINVAL); out vector i at d_out_off[i], trxsig_resample_linear_out_len(n, f) samples.
 * convolve's ABSSYM form (:369-398): trxsig_convolve_batch / _host with flags bit 2 set (b is an ABSSYM filter: half its
 *   taps are used, each on a[t-j] and on a[t-Lb+j]); the reference's reads beyond a's end (its fourth arm has no upper
 *   bound) count as zero. */
float trxsig_db(float x);
float trxsig_dbinv(float x);
int trxsig_sinc_host(const trxsig_ctx *ctx, float x, float *out);
int trxsig_gaussian_noise_host(int length, float variance, trxsig_c32 mean, trxsig_c32 *h_out);
int trxsig_vector_norm2_batch(trxsig_ctx *ctx, const trxsig_c32 *d_in, const int32_t *d_off, const int32_t *d_len, int B, float *d_norm2,
                              float *d_power);
int trxsig_vector_norm2_host(trxsig_ctx *ctx, const trxsig_c32 *h_x, int n, float *norm2, float *power);
int trxsig_frequency_shift_batch(trxsig_ctx *ctx, const trxsig_c32 *d_in, const int32_t *d_off, const int32_t *d_len, int B,
                                 const float *d_freq, const float *d_start_phase, int real_only, trxsig_c32 *d_out, float *d_final_phase);
int trxsig_frequency_shift_host(trxsig_ctx *ctx, const trxsig_c32 *h_x, int n, float freq, float start_phase, int real_only,
                                trxsig_c32 *h_out, float *final_phase);
int trxsig_add_vector_batch(trxsig_ctx *ctx, trxsig_c32 *d_x, const int32_t *d_xoff, const int32_t *d_xlen, const trxsig_c32 *d_y,
                            const int32_t *d_yoff, const int32_t *d_ylen, int B, int max_len);
int trxsig_add_vector_host(trxsig_ctx *ctx, trxsig_c32 *h_x, int nx, const trxsig_c32 *h_y, int ny);
int trxsig_offset_vector_batch(trxsig_ctx *ctx, trxsig_c32 *d_x, const int32_t *d_off, const int32_t *d_len, int B, int max_len,
                               const trxsig_c32 *d_offset, int real_only);
int trxsig_resample_linear_out_len(int n, float exp_factor);   /* < 0: exp_factor < 1 */
int trxsig_resample_linear_batch(trxsig_ctx *ctx, const trxsig_c32 *d_in, const int32_t *d_off, const int32_t *d_len, int B,
                                 float exp_factor, const trxsig_c32 *d_end_point, trxsig_c32 *d_out, const int32_t *d_out_off);
int trxsig_resample_linear_host(trxsig_ctx *ctx, const trxsig_c32 *h_x, int n, float exp_factor, trxsig_c32 end_point, trxsig_c32 *h_out,
                                int out_cap);   /* returns the length */
/* one vector, in place on the host buffer; op: 0 scaleVector(scale), 1 GMSKRotate, 2 GMSKReverseRotate, 3 vectorSlicer,
 * 4 offsetVector(scale = the offset) */
int trxsig_elementwise_host(trxsig_ctx *ctx, int op, trxsig_c32 *h_x, int n, trxsig_c32 scale, int real_only);
int trxsig_decimate_host(trxsig_ctx *ctx, const trxsig_c32 *h_x, int n, int factor, trxsig_c32 *h_out);   /* returns n / factor */

/* ---- measurement helpers (HIP events on the context's stream; used by bench.py) ---------------
 * trxsig_timer_*: one start/stop event pair around whatever the caller enqueues in between.
 * trxsig_profile_*: when enabled, every kernel launch made by the library is bracketed by its own
 *   event pair on the context's stream; trxsig_profile_collect synchronises, adds up the elapsed
 *   time and launch count per kernel and resets.  kernel ids: TRXSIG_K_*. */
int trxsig_timer_start(trxsig_ctx *ctx);
int trxsig_timer_stop(trxsig_ctx *ctx, float *elapsed_ms);   /* synchronises on the stop event */
enum { TRXSIG_K_TSC_CORR = 0, TRXSIG_K_TSC_PEAK = 1, TRXSIG_K_DEMOD = 2, TRXSIG_K_RACH_CORR = 3,
       TRXSIG_K_RACH_PEAK = 4, TRXSIG_K_MODULATE = 5, TRXSIG_K_RESAMPLE = 6, TRXSIG_K_EQUALIZE = 7,
       TRXSIG_K_CONVERT = 8, TRXSIG_K_NORMAL_FUSED = 9, TRXSIG_K_FEC = 10, TRXSIG_K_NORMAL_CHAIN = 11,
       TRXSIG_K_EQ_DELAY = 12, TRXSIG_K_EQ_DFE = 13, TRXSIG_K_GROUP = 14, TRXSIG_K_COUNT = 15 };
/* TRXSIG_K_EQUALIZE = k_eq_detect / k_design_dfe; TRXSIG_K_GROUP = the Transceiver group's replay (trxsig_trxgroup.h) */
/* Kernels added after TRXSIG_K_COUNT was fixed for ABI 2 (k_fec_tch_encode, k_fec_sch_encode, the stream decoders'
 * k_fec_rx_stream for TCH and for XCCH and their k_fec_rx_fold): trxsig_profile_collect (arrays of TRXSIG_K_COUNT entries)
 * leaves them out; trxsig_profile_collect_n reports them, and trxsig_kernel_count() counts them. */
enum { TRXSIG_K_FEC_TCH_ENC = 15, TRXSIG_K_FEC_SCH_ENC = 16, TRXSIG_K_FEC_TCH_RX = 17, TRXSIG_K_FEC_XCCH_RX = 18,
       TRXSIG_K_FEC_RX_FOLD = 19 };
/* the uplink L1 demultiplexer's own kernels (trxsig_l1rx.h): k_l1rx_demux and k_l1rx_finish */
enum { TRXSIG_K_L1RX_DEMUX = 20, TRXSIG_K_L1RX_FINISH = 21 };
/* the downlink L1 multiplexer's (trxsig_l1tx.h): k_l1tx_encode, k_l1tx_mux, the datagram compaction, k_l1tx_commit */
enum { TRXSIG_K_L1TX_ENCODE = 22, TRXSIG_K_L1TX_MUX = 23, TRXSIG_K_L1TX_DGRAM = 24, TRXSIG_K_L1TX_COMMIT = 25 };
/* the wideband transmit synthesiser's (trxsig_frontend.h, trxsig_txbe_create_wideband): k_tx_wideband */
enum { TRXSIG_K_TXWB = 26 };
/* the device-to-device hand-off of the multiplexer's bursts to a group's transmit queues (trxsig_trxgroup_add_l1tx):
 * k_group_tx_arrive_grid */
enum { TRXSIG_K_GROUP_TX_GRID = 27 };
const char *trxsig_kernel_name(int kernel_id);
int trxsig_profile_enable(trxsig_ctx *ctx, int on);
int trxsig_profile_collect(trxsig_ctx *ctx, float total_ms[TRXSIG_K_COUNT], int launches[TRXSIG_K_COUNT]);
/* the same for a caller that states how many entries its arrays hold (at most `cap` are written); returns the library's
 * kernel count, so a caller built against another header version can tell */
int trxsig_profile_collect_n(trxsig_ctx *ctx, int cap, float *total_ms, int *launches);
int trxsig_kernel_count(void);
/* Implementation choice for A/B measurements (tuning build: libtrxsig_tune.so, `make -C csrc tune`); results are bit-identical
 * whatever is selected.
 *   TRXSIG_TUNE_NORMAL_PATH (trxsig_detect_demod_normal_batch; initial value: env TRXSIG_TSC_VARIANT, else 0):
 *     0 = three kernels: correlate, peak, demodulate (the default and the fastest measured);
 *     1 = one fused kernel, a wave per burst;   2 = fused, two bursts per wave;
 *     3 = fused, four bursts per wave (k_normal_quad);   4 = k_normal_quad's detection half, then k_demod.
 *     5 = ONE launch whose detect workgroups hand over to its demodulate workgroups (k_normal_chain,
 *     trxsig_chain.hip).
 *     The fused kernels and the chain need nsoft <= 148 (the chain also nsoft > 0); otherwise the call takes path 0.
 *   TRXSIG_TUNE_CHAIN_LAG: path 5, tiles of 16 bursts (per stream of every 8th tile) between a tile's detect
 *     workgroup and its demodulate workgroups in launch order.  TRXSIG_TUNE_CHAIN_SPIN: polls before a demodulate
 *     wave gives up waiting for its burst's detection (then the call is reported as failed at the library's next
 *     entry and path 0 is used from there on; 0 makes every wait that is not satisfied at once fail -- tests).
 *     Path 5 is for A/B measurements only: its outputs are valid only after trxsig_synchronize (or the next library
 *     call on the context) has returned TRXSIG_OK -- a caller that waits on the stream by other means would read the
 *     soft bits of a batch whose hand-over timed out without seeing the error; its forward progress also rests on
 *     workgroups starting in launch order, which HIP does not promise.
 *   TRXSIG_TUNE_RACH_PATH (initial value: env TRXSIG_RACH_VARIANT, else 2): 0 = exact correlation at every
 *     lag (k_rach_corr + k_rach_peak), 1 = approximate-then-exact in one kernel, a wave per burst (k_rach_fast),
 *     2 = the same with peakDetect's bisection and the tail in their own kernel, two lanes per burst
 *     (k_rach_front + k_rach_peak2; bursts too close to the threshold to call from approximate valley powers
 *     are handed back to k_rach_fast).  All three give the reference's results.
 *   TRXSIG_TUNE_DEMOD_BESIDE (both libraries; default 0): 1 = trxsig_detect_demod_normal_batch (path 0) detects on the context's
 *     stream and DEMODULATES ON A SIDE STREAM of the context, from its own copy of (flags, amp, TOA): the call returns with
 *     d_flags / d_amp / d_toa / d_avgpwr ordered on the context's stream as always, while d_soft / d_hard -- and the READS of
 *     d_samples / d_offset / d_length -- complete only behind trxsig_synchronize (or the next call that is not of this kind).
 *     The next call's correlator (VALU-bound) then runs beside this call's demodulator (HBM-bound): a throughput lever for a
 *     caller that pipelines batches (bench.py reports it as a side field, never as `value`); same results.
 *   TRXSIG_TUNE_BESIDE_DET_CUS (both libraries; default 0; only meaningful with TRXSIG_TUNE_DEMOD_BESIDE = 1): x > 0 = the two
 *     streams of that arrangement PARTITION the compute units (hipExtStreamCreateWithCUMask): the detectors (k_tsc_corr,
 *     k_tsc_peak2) run on a stream of the library masked to x CUs, the demodulator on one masked to the other CUs, so that the
 *     VALU-bound and the HBM-bound kernel of neighbouring calls co-run without contending for the same CUs' wave slots and LDS.
 *     Then d_flags / d_amp / d_toa / d_avgpwr too are complete only behind trxsig_synchronize.  TRXSIG_TUNE_CU_LAYOUT: 0 = the
 *     detect set is mask bits 0..x-1, 1 = every eighth-of-the-mask takes x/8 of them (tools/cu_split.py measures both).
 *     TRXSIG_TUNE_BESIDE_PRIORITY (without masks): the side stream's priority, 0 = normal, 1 = the device's highest, 2 = its lowest.
 *   TRXSIG_TUNE_GENERIC_TAPS: 1 = midamble correlators without the "exactly +-1 tap component" form (which
 *     is only taken when the actual taps have that shape).  Default 0.
 *   TRXSIG_TUNE_SPECULATIVE_PEAK: path 0's peakDetect kernel.  0 = two lanes per burst (early and late point of
 *     each bisection step side by side, sinc table in LDS, window in registers; k_tsc_peak2, the default),
 *     1 = eight lanes per burst with the bisection speculated two levels at a time (k_tsc_peak8; 25 us per
 *     64 K bursts, LDS bandwidth), 2 = a lane per burst, the reference's serial loop (k_tsc_peak; 18 us,
 *     k_tsc_peak2 15 us).  All three are bit-identical.
 *   LIBRARY-WIDE knobs (both libraries; they act on every context of the process and are read by the launchers -- the library
 *   reads no environment variable on a launch path; all give the same results):
 *   TRXSIG_TUNE_EQ_TAIL: 1 = scaleVector + delayVector + equalizeBurst in one kernel (k_eq_dfe4, the default), 2 = k_eq_delay +
 *     k_eq_dfe2 through the scratch rows.  TRXSIG_TUNE_EQ_DENSE: marked bursts per call above which the Transceiver group's channel
 *     estimate runs a lane per burst instead of a wave per burst (default 4096).  TRXSIG_TUNE_RXRES_WPB: windows per workgroup of the
 *     receive resampler (0 = chosen from the launch size); TRXSIG_TUNE_RXRES_ROWS: 1 = its tap rows in visiting order (default),
 *     0 = in branch order.  TRXSIG_TUNE_CHAN_TPW: tiles per workgroup of the shared-filter channeliser (0 = chosen from the launch size).
 *   TRXSIG_TUNE_GROUP_REPLAY: the Transceiver group's receive state machine (trxsig_trxgroup.h).  0 = a wave per ARFCN and segment
 *     (32 timeslots in calls of up to 512, 64 in longer ones: at most 16 segments) that visits only the timeslots at which the state
 *     can move (calls of up to 1,024 timeslots; the default), 1 = a lane per
 *     ARFCN (and segment) stepping through every timeslot (round 4's kernels, also what longer calls take). */
enum { TRXSIG_TUNE_NORMAL_PATH = 0, TRXSIG_TUNE_RACH_PATH = 1, TRXSIG_TUNE_GENERIC_TAPS = 2, TRXSIG_TUNE_SPECULATIVE_PEAK = 3,
       TRXSIG_TUNE_CHAIN_LAG = 4, TRXSIG_TUNE_CHAIN_SPIN = 5, TRXSIG_TUNE_DEMOD_BESIDE = 7, TRXSIG_TUNE_BESIDE_DET_CUS = 8,
       TRXSIG_TUNE_CU_LAYOUT = 9, TRXSIG_TUNE_BESIDE_PRIORITY = 11, TRXSIG_TUNE_EQ_TAIL = 12, TRXSIG_TUNE_EQ_DENSE = 13,
       TRXSIG_TUNE_RXRES_WPB = 14, TRXSIG_TUNE_RXRES_ROWS = 15, TRXSIG_TUNE_CHAN_TPW = 16, TRXSIG_TUNE_GROUP_REPLAY = 17 };
int trxsig_set_tuning(trxsig_ctx *ctx, int key, int value);
/* 1 in libtrxsig_tune.so (every implementation above selectable), 0 in the product library libtrxsig.so, which carries the
 * defaults only (normal path 0 with the two-lane peak kernel, RACH paths 1 and 2) and answers TRXSIG_EINVAL to the rest. */
int trxsig_tuning_build(void);
/* validate a host copy of the table blob (magic, version, size, checksum): 0 if valid */
int trxsig_tables_validate_host(const void *h_blob, size_t bytes);
/* Multi-GPU set-up for a host that is not Python (one process or thread per GPU): the ONE collective of the
 * path, an RCCL broadcast of the table blob over xGMI.  Every rank calls it with its ncclComm_t and a device buffer of
 * trxsig_tables_bytes() bytes -- on `root` that buffer holds the blob (trxsig_tables_device(ctx) of a context made with
 * trxsig_create, or an upload of trxsig_tables_build_host), on the others it receives it; then the others call
 * trxsig_create_from_tables, which validates magic / version / checksum.  Equivalent to
 *   ncclBroadcast(d_blob, d_blob, bytes, ncclUint8, root, comm, stream);
 * librccl.so is loaded at the first call (libtrxsig does not link it).  Stream-ordered: synchronise `hip_stream` before
 * trxsig_create_from_tables. */
int trxsig_tables_broadcast(void *nccl_comm, void *d_blob, size_t bytes, int root, void *hip_stream);
/* The error bar of the access-burst detector's approximate correlation pass for this table blob (host computation,
 * no GPU): *bound x sqrt(sum |x[n]|^2 over the burst) bounds |approximate - reference| correlation amplitude at any
 * lag (derivation: csrc/trxsig_rach.hip); *seq_norm (optional) = the 2-norm of the RACH sequence, for scale.  The
 * detector only uses the approximate values to decide what to recompute with the reference's arithmetic
 * (detectRACHBurst, Transceiver/sigProcLib.cpp:860-914), so the bound affects speed, never results. */
int trxsig_tables_rach_error_bound(const void *h_blob, size_t bytes, float *bound, float *seq_norm);

#ifdef __cplusplus
}
#endif
#endif /* TRXSIG_H */
