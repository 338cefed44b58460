// trxsig_launch.h -- internal launcher prototypes.  The kernels live in trxsig_normal.hip (default normal-burst
// path), trxsig_fused.hip (single-launch alternates), trxsig_rach.hip, trxsig_eq_est.hip, trxsig_eq_dfe.hip, trxsig_tx.hip, trxsig_fec.hip;
// shared device code in trxsig_dev.h, trxsig_corr.h, trxsig_bisect.h, trxsig_demod.h.
#pragma once
#include <hip/hip_runtime_api.h>
#include <hip/hip_vector_types.h>
#include <stdint.h>

#include "trxsig.h"
#include "trxsig_tables.h"

// optional per-kernel event bracketing (trxsig_profile_*): called by the launchers around each kernel
struct TrxProfiler {
  virtual void begin(int kernel_id, hipStream_t st) = 0;
  virtual void end(int kernel_id, hipStream_t st) = 0;
  virtual ~TrxProfiler() {}
};

// number of complex slots per burst in the detect->peak record (SoA, [slot][Bpad])
int trx_rec_slots(int sps);

// dT: device tables, hT: the host copy (the midamble taps travel as a kernel argument)
hipError_t trx_launch_copy_verdict(hipStream_t st, const uint8_t *flags, const trx_c32 *amp, const float *toa, int B, uint8_t *flags_out,
                                   trx_c32 *amp_out, float *toa_out);
hipError_t trx_launch_tsc_detect(hipStream_t st, int sps, const TrxTables *dT, const TrxTables *hT, const trx_c32 *samples,
                                 const int32_t *off, const int32_t *len, int B, int tsc,
                                 float detect_thresh, float energy_thresh, trx_c32 *rec, int Bpad,
                                 uint8_t *flags, trx_c32 *amp, float *toa, float *avgpwr,
                                 int variant /* bit 0: generic taps (no tap-class specialisation); bit 1: 8-lanes-per-burst speculative peak kernel; bit 2: lane-per-burst peak kernel (default: 2 lanes per burst) */,
                                 TrxProfiler *prof);

// the whole normal-burst leg in one kernel (k_normal_fused); lanes_per_burst = 64 or 32, nsoft <= 148
hipError_t trx_launch_normal_fused(hipStream_t st, int sps, int lanes_per_burst, const TrxTables *dT, const TrxTables *hT,
                                   const trx_c32 *samples, const int32_t *off, const int32_t *len, int B, int tsc,
                                   float detect_thresh, float energy_thresh, uint8_t *flags, trx_c32 *amp, float *toa,
                                   float *avgpwr, float *soft, uint8_t *hard, int nsoft, int stride,
                                   int generic_taps /* 1: no tap-class specialisation */, TrxProfiler *prof, int soft_tolerance = 0);

// the whole normal-burst leg in ONE launch with an in-launch hand-over (trxsig_chain.hip); nsoft 1..148; det: 16 bytes
// per burst, tag words clear on entry (left clear on exit); status: host-visible word raised when a wait runs out
size_t trx_chain_ws_bytes(int bursts);
hipError_t trx_launch_normal_chain(hipStream_t st, int sps, const TrxTables *dT, const TrxTables *hT, const trx_c32 *samples,
                                   const int32_t *off, const int32_t *len, int B, int tsc, float detect_thresh,
                                   float energy_thresh, uint8_t *flags, trx_c32 *amp, float *toa, float *avgpwr, float *soft,
                                   uint8_t *hard, int nsoft, int stride, void *det, unsigned *status, int lag,
                                   unsigned spin_limit, int generic_taps, TrxProfiler *prof, int dbg = 0, int soft_tolerance = 0);

// free-standing vector primitives of sigProcLib.h (trxsig_prim.hip); op: 0 scaleVector, 1 GMSKRotate, 2 GMSKReverseRotate,
// 3 vectorSlicer, 4 offsetVector (scale[v] = the offset)
int trx_convolve_out_len(int La, int Lb, int span, int cust_len);
hipError_t trx_launch_convolve(hipStream_t st, const trx_c32 *a, const int32_t *a_off, const int32_t *a_len, int B, int max_out,
                               const trx_c32 *b, int Lb, int span, int flags, int correlate, int cust_start, int cust_len,
                               trx_c32 *out, const int32_t *out_off);
hipError_t trx_launch_delay_vector(hipStream_t st, const TrxTables *dT, const trx_c32 *in, const int32_t *off, const int32_t *len,
                                   int B, const float *delay, int real_only, trx_c32 *out);
hipError_t trx_launch_interpolate_point(hipStream_t st, const TrxTables *dT, const trx_c32 *in, const int32_t *off,
                                        const int32_t *len, int B, const float *ix, int real_only, trx_c32 *out);
hipError_t trx_launch_peak_detect(hipStream_t st, const TrxTables *dT, const trx_c32 *in, const int32_t *off, const int32_t *len,
                                  int B, trx_c32 *peak, float *index, float *avgpwr);
hipError_t trx_launch_energy_detect(hipStream_t st, const trx_c32 *in, const int32_t *off, const int32_t *len, int B, unsigned window,
                                    int step, float thresh, float *avgpwr, uint8_t *ok);
hipError_t trx_launch_elementwise(hipStream_t st, int op, const TrxTables *dT, trx_c32 *x, const int32_t *off, const int32_t *len,
                                  int B, int max_len, const trx_c32 *scale, int real_only);
hipError_t trx_launch_decimate(hipStream_t st, const trx_c32 *in, const int32_t *off, const int32_t *len, int B, int max_len,
                               int factor, trx_c32 *out, const int32_t *out_off);

// the rest of sigProcLib.h's surface (trxsig_prim.hip): vectorNorm2 / vectorPower, frequencyShift, addVector, resampleVector
hipError_t trx_launch_vector_norm2(hipStream_t st, const trx_c32 *in, const int32_t *off, const int32_t *len, int B, float *norm2_out,
                                   float *power_out);
float trx_frequency_shift_max_phase(void);
hipError_t trx_launch_frequency_shift(hipStream_t st, const TrxTables *dT, const trx_c32 *in, const int32_t *off, const int32_t *len,
                                      int B, const float *freq, const float *start, int real_only, trx_c32 *out, float *final_phase);
hipError_t trx_launch_add_vector(hipStream_t st, trx_c32 *x, const int32_t *xoff, const int32_t *xlen, const trx_c32 *y,
                                 const int32_t *yoff, const int32_t *ylen, int B, int max_len);
hipError_t trx_launch_resample_linear(hipStream_t st, const trx_c32 *in, const int32_t *off, const int32_t *len, int B, float exp_factor,
                                      const trx_c32 *end_point, trx_c32 *out, const int32_t *out_off);

// RACH detect: ws = workspace of trx_rach_rec_floats(sps) * Bpad floats
int trx_rach_rec_floats(int sps);
hipError_t trx_launch_rach_detect(hipStream_t st, int sps, const TrxTables *dT, const trx_c32 *samples,
                                  const int32_t *off, const int32_t *len, int B, float detect_thresh,
                                  float energy_thresh, float *ws, int Bpad, uint8_t *flags, trx_c32 *amp,
                                  float *toa, float *avgpwr, TrxProfiler *prof);

// bound on |approximate - reference| correlation amplitude per unit of sqrt(burst energy) (error model in trxsig_rach.hip)
float trx_rach_amp_err(const TrxTables *hT);
// same results, approximate-then-exact single kernel (k_rach_fast)
hipError_t trx_launch_rach_fast(hipStream_t st, int sps, const TrxTables *dT, const trx_c32 *samples,
                                const int32_t *off, const int32_t *len, int B, float detect_thresh,
                                float energy_thresh, float amp_err /* trx_rach_amp_err(host tables) */,
                                float *ws /* trx_rach_rec_floats() floats per burst */, int Bpad,
                                int split /* 1: k_rach_front + k_rach_peak2 + hand-over, 0: k_rach_fast alone */,
                                uint8_t *flags, trx_c32 *amp, float *toa, float *avgpwr, TrxProfiler *prof);

// need_mask != 0: burst enabled iff (flags[b] & need_mask) == need_mask; need_mask == 0: iff flags[b] != 0;
// flags == NULL: every burst enabled.
// Library-wide implementation knobs (A/B measurements and the tests that force a route): set through trxsig_set_tuning, read by the
// launchers -- the library reads NO environment variable on a launch path.  Defaults in trxsig_api.cpp.
enum { TRX_KNOB_EQ_TAIL = 0,      // 1 = k_eq_dfe4 (scale + delay + DFE in one kernel, default), 2 = k_eq_delay + k_eq_dfe2 through the scratch rows
       TRX_KNOB_EQ_DENSE = 1,     // marked bursts above which the lane-per-burst k_eq_detect takes over from the wave-per-burst estimate (4096)
       TRX_KNOB_RXRES_WPB = 2,    // k_rx_resample: windows per workgroup; 0 = chosen from the launch size
       TRX_KNOB_RXRES_ROWS = 3,   // k_rx_resample: 1 = tap rows in visiting order (default), 0 = in branch order
       TRX_KNOB_CHAN_TPW = 4,     // k_channelise16: tiles per workgroup; 0 = chosen from the launch size
       TRX_KNOB_GROUP_REPLAY = 5, // the Transceiver group's state machine: 0 = a wave per 64-slot segment visiting the slots that move the state
                                  // (k_group_replay_wave, default), 1 = a lane per ARFCN (and segment) stepping through every slot (round 4)
       TRX_KNOB_COUNT = 6 };
int trx_knob(int id);
void trx_knob_set(int id, int value);

hipError_t trx_launch_demod(hipStream_t st, int sps, const TrxTables *dT, const trx_c32 *samples,
                            const int32_t *off, const int32_t *len, int B, const trx_c32 *amp,
                            const float *toa, const uint8_t *flags, int need_mask, float *soft,
                            uint8_t *hard, int nsoft, int stride, TrxProfiler *prof, int soft_tolerance = 0);
// (soft_tolerance: TRXSIG_SOFT_TOLERANCE -- the rearranged demodulator of trxsig_demod.h; hard bits exact, soft bits within 3.7e-5)
// The six sequence-equaliser kernels' arguments, one record for all (a member a kind does not read stays as it is here).  Every
// kind reads samples0 / off0 / len / B, amp / toa, flags / need_mask (as trx_launch_demod; flags may be NULL), chan and win (may
// each be NULL).  All but sch_fit: soft, hard, nsoft (<= 148), stride.  No profiler id.
//   mlse        (trxsig_mlse.hip; trxsig_mlse_batch): + tsc_bits (bit j = bit j of the training sequence); chan is B x 5
//   mlse_access (trxsig_mlse_access.hip; trxsig_mlse_access_batch): the burst's 49 leading symbols are fixed
//   mlse_sch    (trxsig_mlse_sch.hip; trxsig_mlse_sch_batch; trxsig_l1acq's TRXSIG_SCHLEG_MLSE): the 64-symbol sequence is fixed
//   sch_fit     (trxsig_sch_fit.hip; trxsig_sch_fit_batch; trxsig_l1acq's TRXSIG_SCHDET_FIT): chan is B x 9; + E, R, q (B each, may be NULL)
//   mlse_div    (trxsig_mlse_div.hip; trxsig_mlse_div_batch): mlse's + samples1 / off1 (an antenna each, one amp / TOA per burst) and
//               primary (may be NULL = 0), the antenna they came from; chan is B x 2 x 5
//   mlse_irc    (trxsig_mlse_irc.hip; trxsig_mlse_irc_batch): mlse_div's + loading (0..16, added to the diagonal of the estimated
//               set), cov_in (B x 4, may be NULL = estimate: the caller's set A, Bv, xr, xi) and cov (B x 4, may be NULL: the set used)
struct TrxMlseArgs {
  const trx_c32 *samples0 = nullptr, *samples1 = nullptr;
  const int32_t *off0 = nullptr, *off1 = nullptr, *len = nullptr;
  int B = 0;
  unsigned tsc_bits = 0;
  const trx_c32 *amp = nullptr;
  const float *toa = nullptr;
  const uint8_t *primary = nullptr, *flags = nullptr;
  int need_mask = 0;
  float loading = 0.0f;
  const float *cov_in = nullptr;
  float *cov = nullptr;
  trx_c32 *chan = nullptr;
  int32_t *win = nullptr;
  float *soft = nullptr;
  uint8_t *hard = nullptr;
  int nsoft = 0, stride = 0;
  float *E = nullptr, *R = nullptr, *q = nullptr;
};
typedef hipError_t TrxMlseLaunch(hipStream_t st, int sps, const TrxTables *dT, const TrxMlseArgs &a);
TrxMlseLaunch trx_launch_mlse, trx_launch_mlse_access, trx_launch_mlse_sch, trx_launch_sch_fit, trx_launch_mlse_div, trx_launch_mlse_irc;
// the selection rule of trxsig_mlse_div_normal_batch, v_a = (valid_a[b] & need_mask) != 0: sel (0, 1, 2 = neither); the selected
// antenna's amp, TOA, flags byte and avgPwr (antenna 0's where neither); valid[b] = need_mask where sel < 2 else 0.  Every output,
// and with flags / pwr their inputs, may be NULL.
struct TrxDivSelect {
  const uint8_t *valid0 = nullptr, *valid1 = nullptr, *flags0 = nullptr, *flags1 = nullptr;
  const trx_c32 *amp0 = nullptr, *amp1 = nullptr;
  const float *toa0 = nullptr, *toa1 = nullptr, *pwr0 = nullptr, *pwr1 = nullptr;
  int B = 0, need_mask = 0;
  uint8_t *sel = nullptr, *valid = nullptr, *flags = nullptr;
  trx_c32 *amp = nullptr;
  float *toa = nullptr, *pwr = nullptr;
};
hipError_t trx_launch_div_select(hipStream_t st, const TrxDivSelect &p);
// trxsig_trxgroup_combine_div's access-burst rows: soft row r = the selected group's (sel[r] == 1: soft1) where valid[r], else zeros;
// chan (rows x 2 x 5, may be NULL) zeros, win (may be NULL) 2
hipError_t trx_launch_div_copy_rows(hipStream_t st, int rows, const uint8_t *valid, const uint8_t *sel, const float *soft0, const float *soft1,
                                    int stride_in, float *soft, int stride, int nsoft, trx_c32 *chan, int32_t *win);

hipError_t trx_launch_modulate(hipStream_t st, int sps, const TrxTables *dT, const uint8_t *bits, const int32_t *guard,
                               const float *gain, int B, trx_c32 *out, const int32_t *out_off, TrxProfiler *prof);
hipError_t trx_launch_resample(hipStream_t st, const trx_c32 *in, int n, long long in_stride, int S, int P, int Q,
                               const float *lpf, int L, trx_c32 *out, long long out_stride, int nout,
                               TrxProfiler *prof);
// the tiled resampler in full (trxsig_tx.hip): int16 I/Q in with history windows (RadioInterface::pullBuffer) or int16 out
// with gain (pushBuffer); see k_resample.  OB is filled in by the launcher.
struct TrxResampleArgs {
  const void *in; long long in_stride;                     // stream s at in + s*in_stride (elements: trx_c32 or int16 pairs)
  const short2 *hist; int hist_len;                        // int16 input: the hist_len samples before each stream's start
  int n, win_step, swap;                                   // samples per window, start-to-start distance of windows, I/Q swap
  const float *lpf; int L, P, Q;
  int o_skip, n_out;                                       // outputs [o_skip, n_out) of every window are produced
  void *out; long long out_stride, out_win_step;           // window w of stream s writes at out + s*out_stride + w*out_win_step
  float gain;                                              // int16 output
  int OB, xcap, taps_lds, tap_pitch, tap_g, row_inv;       // filled in by the launcher
  // int16 input, wideband (the channeliser): output stream s is carrier s % mix_carriers of raw stream s / mix_carriers, mixed down
  // on the way into LDS: z[n] = x[n] * expjLookup(phase[n]) (frequencyShift's arithmetic, sigProcLib.cpp:459) with the phase of
  // raw sample n formed directly, phase[n] = (float)(t - 2 pi floor(t / 2 pi)), t = (double) n * (double) freq, instead of by
  // the reference's running float sum (trxsig_frontend.h says why).
  // mix_freq: [mix_carriers] floats (device); mix_n0: global index of raw sample 0 of this launch's `in`; mix_tables: the
  // context's tables (trig lookup)
  const float *mix_freq; int mix_carriers; long long mix_n0; const TrxTables *mix_tables;
  // input computed from burst bits (the fused transmit back end): in = the bit ring [S][in_stride slots][148], tx_gain the gains
  // [S][in_stride]; tx_start[m] / tx_meta[m] (m < tx_n, device, ascending): where burst m starts in the window and
  // slot | guard << 16 | has_gain << 20
  const TrxTables *tx_tables; const float *tx_gain; const int32_t *tx_start, *tx_meta; int tx_n, tx_sps;
};
hipError_t trx_launch_resample_ex(hipStream_t st, TrxResampleArgs a, int S, int n_windows, bool in_i16, bool out_i16,
                                  TrxProfiler *prof, bool in_bits = false);
// the channeliser's per-carrier form (mix_carriers > 0): does a tile's span of the window fit the launcher's staging?  (The front
// end refuses what does not at create time, instead of failing a push.)
bool trx_resample_mix_fits(int P, int Q, int L, int n_out, int o_skip);
// the channeliser's shared-filter form (trxsig_chan.hip): C carriers on a grid of sixteenths of the wideband rate in one pass
// binmap: four bits per carrier c, its bin k_c (theta_c = 2 pi k_c / 16): with four carriers or more the kernel takes the bins from one FFT
hipError_t trx_launch_channelise16(hipStream_t st, TrxResampleArgs a, int S_wide, int C, int n_windows, const float2 *tw, TrxProfiler *prof,
                                   unsigned long long binmap);
// what trx_launch_channelise16 can launch, apart from the carriers' grid: C in {1, 2, 4, 8, 16}, at most 32 taps per output, the tile's span of
// the window (xcap) inside the kernel's staging and its LDS inside 64 KiB.  trxsig_rxfe_set_shared_filter refuses the rest with it.
bool trx_channelise16_fits(int P, int Q, int L, int C);
// The wideband transmit synthesiser (trxsig_txbe_create_wideband; k_tx_wideband, trxsig_txwb.hip): for every wideband stream w and
// tile of TRX_TXWB_OB outputs, carrier by carrier, the modulated window of ARFCN stream w*C + c is staged from its bit ring,
// resampled P : Q with the branch-major taps, mixed by expjLookup(phase of output k) and summed in carrier order; int16 out once.
// Tables built by the host at create time: tpb [Pr][pitch] (Pr = P / gcd(P, Q); row r holds lpf[r gcd + P k], zero past L),
// lane[256] = ((t Q') mod Pr, (t Q') / Pr) for t = 0..255 (Q' = Q / gcd), tiles[t] = (row, inOff) of the tile's first output and the
// last input its outputs reach;
// freq[C] = -h_carrier_freq.
#define TRX_TXWB_OB 1024                                   // outputs per workgroup (four per lane)
#define TRX_TXWB_KT 32                                     // taps per output at most
#define TRX_TXWB_TAPB 32768                                // bytes of the branch-major tap table at most
#define TRX_TXWB_XCAP 3584                                 // staged samples per carrier and tile at most
struct TrxTxwbArgs {
  const TrxTables *T;
  const uint8_t *ring; const float *gring; int cap;        // bit ring [S][cap][148], gains [S][cap]
  const int32_t *tx_start, *tx_meta; int tx_n;             // the window's bursts (as TrxResampleArgs)
  const float *tpb; int Pr, pitch, KT;                     // branch-major taps
  const int2 *lane; int step_r, step_i;                    // a lane's first output; 256 outputs on: rows / input offsets further
  const int4 *tiles; int tile0;                            // (row, inOff, hi) of every tile: its first output's, the last input it
                                                           // can reach; this slice's first tile
  int n, o_skip, n_out, C, xcap;                           // window length, first kept output, outputs, carriers, staged samples
  const float *freq; long long k0;                         // mixer frequencies; wideband sample count of output o_skip
  float gain; short2 *out; long long out_stride;           // int16 out: stream w at out + w*out_stride
};
hipError_t trx_launch_tx_wideband(hipStream_t st, TrxTxwbArgs a, int sps, int Sw, int n_tiles, TrxProfiler *prof);
hipError_t trx_launch_tx_ring_store(hipStream_t st, const uint8_t *bits, const float *gain, int S, int nb, int head, int cap, uint8_t *ring,
                                    float *gring);
hipError_t trx_launch_burst_index(hipStream_t st, int S, int nb, long long stride, int rd, int tn0, int sps, int32_t *off,
                                  int32_t *len);
// The receive front end fused into the normal-burst detectors (trxsig_rxgen.h, sps = 4, 65*4 : 96 with at most four taps per
// output): the bursts are described by where they start in the stream of resampled samples, and the kernels compute those
// samples from the raw int16 stream as they need them.
struct TrxRxGen {
  const short2 *raw; long long raw_stride;                 // this push: stream s at raw + s*raw_stride, K*864 samples each
  const short2 *keep;                                      // [S][1056]: history + last chunk of the previous push (its window)
  const float4 *tpb;                                       // [65] taps of branch 4*(24 n mod 65) in slot n: lpf[br + 260 k], k = 0..3
  int K, swap, skipD;                                      // chunks in this push; I/Q swap; INHISTORY outputs skipped + (L-1)/2/Q
  int w0, w1;                                              // the last w0 (w1) outputs of a chunk have tap 0 (tap 1) beyond the window's end
  int tail, tn0, nb;                                       // uncut resampled samples before this push; TN of burst 0; bursts per stream
  const int32_t *sel;                                      // optional: launch index b stands for burst sel[b] (= s*nb + j); NULL: b itself
};
hipError_t trx_launch_rx_normal(hipStream_t st, const TrxTables *dT, const TrxTables *hT, const TrxRxGen &gen, int B, int tsc,
                                float detect_thresh, float energy_thresh, trx_c32 *rec, int Bpad, uint8_t *flags, trx_c32 *amp,
                                float *toa, float *avgpwr, float *soft, uint8_t *hard, int nsoft, int stride, int generic_taps,
                                TrxProfiler *prof, int soft_tolerance = 0);
// the other legs on bursts computed from the raw stream (the Transceiver group's fused front end): detectRACHBurst
// (k_rach_front_rx + k_rach_peak2 + the hand-over in k_rach_fast_rx; ws as trx_launch_rach_fast) and demodulateBurst alone
// with caller-supplied amplitude / TOA / enable flags (k_demod_rx)
hipError_t trx_launch_rx_rach(hipStream_t st, const TrxTables *dT, const TrxRxGen &gen, const int32_t *len /* samples per burst */, int B,
                              float detect_thresh, float energy_thresh, float amp_err, float *ws, int Bpad, uint8_t *flags, trx_c32 *amp,
                              float *toa, float *avgpwr, TrxProfiler *prof);
hipError_t trx_launch_rx_demod(hipStream_t st, const TrxTables *dT, const TrxRxGen &gen, int B, const trx_c32 *amp, const float *toa,
                               const uint8_t *flags, int need_mask, float *soft, uint8_t *hard, int nsoft, int stride, TrxProfiler *prof,
                               int soft_tolerance = 0);
// pack: 0 = int16 I/Q -> complex float (swap: I/Q flipped), 1 = complex float -> int16 I/Q, 2 = fp16 I/Q -> complex float
hipError_t trx_launch_convert(hipStream_t st, int pack, const void *in, long long n, int swap, void *out,
                              TrxProfiler *prof, float gain = 1.0f /* pack == 1: scaleVector before the cast */);

// sps = 1 equaliser path; xd: B x xstride complex scratch (xstride >= 157), toa_eq: B floats scratch,
// w: B x 7, bq: B x 5 complex
hipError_t trx_launch_equalize(hipStream_t st, const TrxTables *dT, const void *samples, int fmt /* TRXSIG_SAMPLES_* */, const int32_t *off,
                               const int32_t *len, int B, int tsc, float detect_thresh, float energy_thresh,
                               int variant52m, int max_toa, uint8_t *flags, trx_c32 *amp, float *toa, float *toa_eq,
                               trx_c32 *w, trx_c32 *bq, trx_c32 *xd, int xstride, float *soft, uint8_t *hard,
                               int nsoft, int stride, TrxProfiler *prof, bool geom52 = false /* trx_eq52_geometry(host tables, tsc) */);
// analyzeTrafficBurst's 52M window (ref52:983-1000) has the geometry k_eq_detect52 is written for when maxTOA = 4 AND the
// training sequence's expectedTOAPeak is 20 (true of all eight sequences of the tables this library builds; checked, not assumed)
inline bool trx_eq52_geometry(const TrxTables *hT, int tsc) {
  return hT && tsc >= 0 && tsc < 8 && (unsigned)round((double)((hT->mid_toa[tsc] + 5.0f) + (float)(size_t)((16 - 1) / 2))) == 20u;
}


// L1 FEC soft decode (trxsig_fec.hip).  mode 0: generic SoftVector::decode of nblk blocks of n soft values ->
// nout bits (one byte each) at out0 + b*out_stride; mode 1: XCCH (four bursts per block, in_stride = floats per
// burst): out0 = 23 octets per block, out1 = parity ok; mode 2: RACH (one burst per block): out0 = tail ok,
// out1 = BSIC, out2 = RA; mode 4: SCH (one burst per block, n = 78, nout = 39): out0 = ok, out1 = BSIC, out2 = the decoded
// frame number, an int32 array.  wire != 0: the UDP hop's 8-bit quantisation of the soft values first.
#define TRX_FEC_MODE_SCH 4   // what the SCH callers pass (trxsig_fec_sch_decode_batch, trxsig_l1acq_search); FEC_SCH in trxsig_fec.hip
hipError_t trx_launch_fec(hipStream_t st, int mode, const float *soft, long long in_stride, int n, int nout, int nblk,
                          int wire, uint8_t *out0, uint8_t *out1, uint8_t *out2, long long out_stride, TrxProfiler *prof,
                          int ilv8 = 0 /* mode 1 through the 8-burst TCH deinterleaver (FACCH); mode 3 = TCH: out0 = 33
                                          octets of d[260], out1 = good, out2 = stolen */);

// the halves of trx_launch_equalize (see trxsig_eq_est.hip, trxsig_eq_dfe.hip): channel estimate + designDFE with an explicit SNR
// threshold and no energy gate; equalizeBurst with caller-supplied taps (flags: DETECT bit = burst enabled)
hipError_t trx_launch_estimate_dfe(hipStream_t st, const TrxTables *dT, const void *samples, int fmt, const int32_t *off,
                                   const int32_t *len, int B, int tsc, float detect_thresh, float snr_thresh,
                                   float snr_value, int variant52m, int max_toa, uint8_t *flags, trx_c32 *amp, float *toa,
                                   float *toa_eq, float *chan_off, trx_c32 *w, trx_c32 *bq, trx_c32 *chan /* B x 6 or NULL */,
                                   TrxProfiler *prof, const uint8_t *enable = nullptr /* only bursts with enable[b] != 0; nothing
                                   is written for the others */, const float *snr_in = nullptr /* SNR estimate per burst */,
                                   bool geom52 = false, int32_t *work = nullptr /* B + 1 ints of scratch: lets a marked subset (enable) of
                                   the Transceiver/ variant be listed and estimated a wave per burst (k_eq_estimate_wave) */,
                                   bool listed = false /* work holds the list already: the count, then the marked bursts in any order */);
// designDFE(chan, snr, 7) alone; amp != NULL: scaleVector(chan, 1/amp) first
hipError_t trx_launch_design_dfe(hipStream_t st, const trx_c32 *chan, const trx_c32 *amp, const float *snr, int B, trx_c32 *w,
                                 trx_c32 *bq, TrxProfiler *prof);
hipError_t trx_launch_equalize_taps(hipStream_t st, const TrxTables *dT, const void *samples, int fmt, const int32_t *off,
                                    const int32_t *len, int B, const trx_c32 *amp, const float *toa_eq,
                                    const uint8_t *flags, const trx_c32 *w, const trx_c32 *bq, trx_c32 *xd, int xstride,
                                    float *soft, uint8_t *hard, int nsoft, int stride, TrxProfiler *prof,
                                    const int32_t *tap_ix = nullptr /* burst b uses the taps at index tap_ix[b] */);

// XCCH L1 encode: nblk L2 frames (23 octets each) -> 4*nblk bursts of 148 bits (one per byte); tsc_bits: the 26
// training-sequence bits (device)
hipError_t trx_launch_fec_xcch_encode(hipStream_t st, const uint8_t *frames, int nblk, const uint8_t *tsc_bits, uint8_t *bits,
                                      TrxProfiler *prof);
// TCH/FS + FACCH/F stream encode (trxsig_fec_tch_encode_batch): n_chan x n_blocks blocks -> 4 bursts of 148 bits each;
// tsc_bits: the 8 x 26 training-sequence bits, filler: 456 bits, state: 32 bytes per channel, in / out (all device)
hipError_t trx_launch_fec_tch_encode(hipStream_t st, int n_chan, int n_blocks, const uint8_t *kinds, const uint8_t *payload,
                                     const uint8_t *tscs, const uint8_t *tsc_bits, const uint8_t *filler, uint8_t *state,
                                     uint8_t *bits, TrxProfiler *prof);
// SCH encode (trxsig_fec_sch_encode_batch): n (FN, BSIC) -> n bursts of 148 bits; xts: bit t = extended training sequence bit t
hipError_t trx_launch_fec_sch_encode(hipStream_t st, const uint32_t *fns, const uint8_t *bsics, int n, unsigned long long xts,
                                     uint8_t *bits, TrxProfiler *prof);
// GPRS packet data blocks (trxsig_fec_pdtch_encode_batch / _decode_batch): k_fec_pdtch_encode, k_fec_pdtch_decode.  blocks: 54
// octets per block; cs, tsc: per block; tsc_bits: the 8 x 26 training-sequence bits (device); index: [nblk][4] or NULL; every
// decoder output but blocks may be NULL
hipError_t trx_launch_fec_pdtch_encode(hipStream_t st, const uint8_t *blocks, const uint8_t *cs, const uint8_t *tsc, int nblk,
                                       const uint8_t *tsc_bits, uint8_t *bits, TrxProfiler *prof);
hipError_t trx_launch_fec_pdtch_decode(hipStream_t st, const float *soft, long long stride, long long n_rows, const int32_t *index,
                                       int nblk, int wire, int cs_force, uint8_t *blocks, uint8_t *cs, uint8_t *dist, uint8_t *ok,
                                       uint8_t *usf, TrxProfiler *prof);
// access bursts in both formats (trxsig_fec_access_encode_batch / _decode_batch): k_fec_access_encode, k_fec_access_decode.
// index: [n] or NULL; fmt: 0, 1 or -1 (either, with the cell's bsic); every decoder output but ra may be NULL
hipError_t trx_launch_fec_access_encode(hipStream_t st, const uint16_t *ra, const uint8_t *fmt, const uint8_t *bsic, int n,
                                        uint8_t *bits, TrxProfiler *prof);
hipError_t trx_launch_fec_access_decode(hipStream_t st, const float *soft, long long stride, long long n_rows, const int32_t *index,
                                        int n, int wire, int fmt, int bsic, uint16_t *ra, uint8_t *ofmt, uint8_t *tail_ok,
                                        uint8_t *obsic, TrxProfiler *prof);
// uplink stream decode (trxsig_fec_tch_decode_stream / _xcch_decode_stream): k_fec_rx_stream, then k_fec_rx_fold.  tch != 0:
// TCH/FACCH (out_tch = 33 octets, out_l2 = the FACCH frame), 0: XCCH (out_l2 = the frame; out_tch and b0 unused)
hipError_t trx_launch_fec_rx_stream(hipStream_t st, int tch, int n_chan, int n_slots, const float *soft, long long stride,
                                    long long n_rows, const int32_t *index, const uint8_t *b0, int wire, uint8_t *state,
                                    uint8_t *status, uint8_t *out_tch, uint8_t *out_l2, float *fer, TrxProfiler *prof);

// the air (include/trxsig_air.h; trxsig_air.hip): k_air_cells, k_air_stream.  NULL arrays skip their stage, as the header says.
struct TrxAirCells {
  const trx_c32 *in; long long in_slot, in_arfcn;          // cell (t, a) at in + t * in_slot + a * in_arfcn
  trx_c32 *out; long long out_slot, out_arfcn;
  const trx_c32 *taps; int n_taps;                         // [a][t][n_taps]
  const uint32_t *step, *phase; const float *sigma;        // [a][t]
  long long rows; int n_arfcn;                             // rows: 8 n_frames
  unsigned row0;                                           // 8 fn: the noise counter's row of slot 0
  unsigned key0, key1;                                     // the seed
  int accumulate;
};
hipError_t trx_launch_air_cells(hipStream_t st, int sps, const TrxTables *dT, const TrxAirCells &p);
struct TrxAirStream {
  const trx_c32 *in; long long in_slot, in_arfcn; int n_arfcn, n_cells;
  const int32_t *arfcn; const long long *cut; const float *delay; const uint32_t *step, *phase; const trx_c32 *gain;
  const float *sigma; const uint32_t *n0;
  int n_handsets, len; trx_c32 *out; long long out_stride;
  unsigned key0, key1;
};
#define TRX_AIR_TILE 512                                   // outputs per workgroup of k_air_stream
hipError_t trx_launch_air_stream(hipStream_t st, int sps, const TrxTables *dT, const TrxAirStream &p);
// the fading-tap generator (trxsig_air_fade; k_air_fade, k_air_fade_params).  The profile's image on the device, written by
// trxsig_air_fade_profile / _columns in stream order: amplitudes, line-of-sight cosines, tap weights, column rotations.
#define TRX_FADE_MAX_PATHS 12
#define TRX_FADE_MAX_SIN 32
#define TRX_FADE_MAX_COLS 1024
struct TrxAirFadeTab {
  float a[TRX_FADE_MAX_PATHS], b[TRX_FADE_MAX_PATHS];      // sqrt(power (1 - los) / S), sqrt(power los)
  int32_t los_c[TRX_FADE_MAX_PATHS];                       // the line-of-sight arrival cosine, Q23
  float w[TRX_FADE_MAX_PATHS][32];                         // w[p][j]: path p's weight on tap j (zero beyond n_taps)
  uint32_t rot[TRX_FADE_MAX_COLS][TRX_FADE_MAX_PATHS];     // -f_kHz tau_ns 1e-6 turn, in 2^-32 turn
};
struct TrxAirFade {
  const TrxAirFadeTab *tab;
  int P, S, n_taps;
  unsigned inv;                                            // ceil(2^16 / (S + 1)): pair i is path (i * inv) >> 16
  const int32_t *link; const uint32_t *doppler; int n_links;
  trx_c32 *taps; int vec;                                  // vec: two taps leave in one 16-byte store
  uint32_t *phase; int32_t *step;                          // k_air_fade_params' outputs
  long long rows; int n_arfcn;
  unsigned row0, key0, key1;
};
hipError_t trx_launch_air_fade(hipStream_t st, const TrxAirFade &p);
hipError_t trx_launch_air_fade_params(hipStream_t st, const TrxAirFade &p);
