// trxsig_eq_est.hip -- the equaliser path (sps = 1), first half: channel estimate and designDFE.
// Numerical contract: see trxsig_dev.h / DESIGN.md (every float32 operation is the reference's, in the
// reference's order; built with -ffp-contract=off).
#include <cstdlib>

#include "trxsig_bisect.h"
#include "trxsig_demod.h"
#include "trxsig_eq.h"
#include "trxsig_eq_probe.h"

namespace {

static constexpr int kEqWaveMax = 2048;   // k_eq_estimate_wave: waves launched; a call of at most this many bursts takes it without a list
// more marked bursts than this: a lane per burst (k_eq_detect) is the faster arrangement again (TRXSIG_EQ_DENSE: the tests force either route)
static int eq_dense() { return trx_knob(TRX_KNOB_EQ_DENSE); }   // (trxsig_set_tuning(TRXSIG_TUNE_EQ_DENSE): a test switches it between cases)
// A/B (tuning build only): TRXSIG_EQ_DETECT_GENERIC=1 never takes k_eq_detect52 (nor the wave-per-burst kernel): k_eq_detect serves every call
static int eq_detect_generic() {
#ifdef TRX_TUNING_BUILD
  static const int v = std::getenv("TRXSIG_EQ_DETECT_GENERIC") ? std::atoi(std::getenv("TRXSIG_EQ_DETECT_GENERIC")) : 0;
  return v;
#else
  return 0;
#endif
}

// designDFE(channelResponse, SNRestimate, Nf = 7, ...) (sigProcLib.cpp:1246-1340), nu = 5: fully unrolled in registers.
// chan: the six channel taps (already scaled by 1/amp, Transceiver.cpp:346); w: feed-forward, bq: feedback taps.
__device__ __forceinline__ void design_dfe7(const cx (&chan)[6], float snr, cx (&w)[7], cx (&bq)[5]) {
  // Complex arithmetic on packed float32 pairs (pk_cmul / pk_cadd / pk_csub of trxsig_dev.h: Complex.h's products and sums, each
  // rounded on its own); norms, divisions and square roots stay scalar.  A lane per channel estimate: what bounds it is the
  // number of instructions one wave can issue.
  constexpr int Nf = 7, nu = 5;
  auto conj2 = [](v2f z) { v2f r; r.x = z.x; r.y = -z.y; return r; };
  auto nrm = [](v2f z) { return z.y * z.y + z.x * z.x; };    // Complex::norm2 (Complex.h:119)
  v2f G0[Nf], G1[Nf];
#pragma unroll
  for (int k = 0; k < Nf; k++) { G0[k] = pk(mk(0, 0)); G1[k] = pk(mk(0, 0)); }
  G0[0] = pk(mk((float)(1.0 / (double)sqrtf(snr)), 0.0f));  // :1261
#pragma unroll
  for (int j = 0; j <= nu; j++) G1[j] = pk(mk(chan[j].r, -chan[j].i));
  v2f Lu[Nf - 1][Nf - 1];                                   // L[i][j], i < j <= Nf-1, stored at [i][j-i-1]
  v2f Lfb[nu];                                              // L[Nf-1][Nf .. Nf+nu-1]
  float d = 0.0f;
#pragma unroll
  for (int i = 0; i < Nf; i++) {
    d = nrm(G0[0]) + nrm(G1[0]);                            // :1272
    const v2f g0c = conj2(G0[0]), g1c = conj2(G1[0]);
#pragma unroll
    for (int k = 1; k < Nf; k++) {                          // *Lptr = (G0[k]*conj(G0[0]) + G1[k]*conj(G1[0]))/d (:1277)
      const int col = i + k;
      const bool need = (i < Nf - 1) ? (col <= Nf - 1) : (col >= Nf && col < Nf + nu);
      if (need) {
        const v2f tt = pk_cadd(pk_cmul(G0[k], g0c), pk_cmul(G1[k], g1c));
        v2f v; v.x = tt.x / d; v.y = tt.y / d;
        if (i < Nf - 1) Lu[i][k - 1] = v; else Lfb[col - Nf] = v;
      }
    }
    v2f kk;                                                 // G1[0] / G0[0] = G1[0] * G0[0].inv() (:1282; Complex.h:85, 154-160)
    {
      const float n = nrm(G0[0]);
      v2f inv; inv.x = G0[0].x / n; inv.y = -G0[0].y / n;
      kk = pk_cmul(G1[0], inv);
    }
    if (i != Nf - 1) {
      v2f G0n[Nf], G1n[Nf];
      const v2f kc = conj2(kk);
      v2f km; km.x = kk.x * -1.0f; km.y = kk.y * -1.0f;      // k * -1
#pragma unroll
      for (int q = 0; q < Nf; q++) G0n[q] = pk_cadd(pk_cmul(G1[q], kc), G0[q]);      // :1285-1287
#pragma unroll
      for (int q = 0; q < Nf; q++) G1n[q] = pk_cadd(pk_cmul(G0[q], km), G1[q]);      // :1289-1291
#pragma unroll
      for (int q = 0; q < Nf - 1; q++) G1n[q] = G1n[q + 1];                           // delayVector(G1new,-1) (:1292)
      G1n[Nf - 1] = pk(mk(0, 0));
      const v2f sc = pk(mk((float)(1.0 / (double)sqrtf((float)(1.0 + (double)nrm(kk)))), 0.0f));   // :1294-1295
#pragma unroll
      for (int q = 0; q < Nf; q++) { G0[q] = pk_cmul(G0n[q], sc); G1[q] = pk_cmul(G1n[q], sc); }
    }
  }
#pragma unroll
  for (int j = 0; j < nu; j++) {                            // :1301-1304: * -1, conj
    const v2f t1 = pk_cmul(Lfb[j], pk(mk(-1.0f, 0.0f)));
    bq[j] = mk(t1.x, -t1.y);
  }
  v2f v[Nf];
  v[Nf - 1] = pk(mk(1.0f, 0.0f));
#pragma unroll
  for (int k = Nf - 2; k >= 0; k--) {                       // :1310-1319
    v2f vk = pk(mk(0, 0));
#pragma unroll
    for (int j = k + 1; j < Nf; j++) vk = pk_csub(vk, pk_cmul(v[j], Lu[k][j - k - 1]));
    v[k] = vk;
  }
#pragma unroll
  for (int i = 0; i < Nf; i++) {                            // :1323-1335
    v2f wi = pk(mk(0, 0));
    const int endPt = (nu < (Nf - 1 - i)) ? nu : (Nf - 1 - i);
#pragma unroll
    for (int k = 0; k < Nf; k++)
      if (k < endPt + 1) wi = pk_cadd(wi, pk_cmul(v[i + k < Nf ? i + k : Nf - 1], pk(mk(chan[k < 6 ? k : 5].r, -chan[k < 6 ? k : 5].i))));
    w[i] = mk(wi.x / d, wi.y / d);
  }
}

// ---- what the two lane-per-burst detectors (k_eq_detect, k_eq_detect52) say alike ----

// energyDetect on the burst's 20 energy samples (:916-932; the 52M variant's are every fourth sample, ref52:946-963); thresh < 0: no gate
__device__ __forceinline__ bool eq_energy_ok(const cx (&ev)[20], float thresh) {
  float energy = 0.0f;
#pragma unroll
  for (int i = 0; i < 20; i++) energy += norm2(ev[i]);
  return thresh < 0.0f || energy / (float)20u > thresh * thresh;
}

// A burst that goes no further: its flag (0: no energy; TRXSIG_F_BADLEN: its length or its window does not fit), no amplitude, no TOA
__device__ __forceinline__ void eq_refuse(int b, uint8_t flag, uint8_t *flags, cx *amp_out, float *toa_out, float *toa_eq) {
  flags[b] = flag; amp_out[b] = mk(0, 0); toa_out[b] = 0.0f; toa_eq[b] = 0.0f;
}

// Transceiver.cpp:341-347 for a detected burst: the SNR estimate -- the caller's per burst (snr_burst, where `given`), else snr_value > 0:
// the estimate itself (the Transceiver facade forms it on the host in the reference's double arithmetic, :340), else |amp|^2/(thr^2+1)
// with thr = snr_thresh >= 0, else the energy threshold --, scaleVector(chan, 1/amp), designDFE(chan, SNR, 7) (:1246-1340), 7 + 5 taps out.
__device__ __forceinline__ void eq_design_store(cx (&chan)[6], cx amp, bool given, float snr_burst, float snr_value, float snr_thresh,
                                                float energy_thresh, int b, cx *w_out, cx *b_out) {
  const float thr = snr_thresh >= 0.0f ? snr_thresh : (energy_thresh < 0.0f ? 0.0f : energy_thresh);
  const float snr = given ? snr_burst : (snr_value > 0.0f ? snr_value : (float)((double)norm2(amp) / ((double)(thr * thr) + 1.0)));
  const cx ainv = cdiv(mk(1.0f, 0.0f), amp);
#pragma unroll
  for (int k = 0; k < 6; k++) chan[k] = cmul(chan[k], ainv);
  cx w7[7], bq[5];
  design_dfe7(chan, snr, w7, bq);
#pragma unroll
  for (int i = 0; i < 7; i++) w_out[(size_t)b * 7 + i] = w7[i];
#pragma unroll
  for (int j = 0; j < 5; j++) b_out[(size_t)b * 5 + j] = bq[j];
}

// The burst loads of a wave's 64 bursts, coalesced through LDS (complex-float staging): a lane per burst would touch 64 different lines
// with every load instruction (46 instructions x 64 lines per wave: 28 % of k_eq_detect went there).  Instead the wave fetches burst k's 20
// energy samples and its correlation window with ONE instruction (a lane per sample slot: ~8 lines), all 64 bursts' loads in flight
// together (eq_load64), parks them burst-major in LDS (eq_park64; st_re / st_im, odd pitch: conflict-free both ways), and every lane
// then reads its own burst's samples back (eq_unpark): slots 0..19 the energy samples, 20.. the window.
// No load is predicated per burst (a mask per load cost ~12 instructions with VALU -> SALU -> exec round trips: the 64 loads took 12 k
// cycles to ISSUE): offv / nm1v hold each lane's burst offset and last index -- of the wave's first good burst where the lane's own is
// not good -- and an index beyond a burst's end (only possible when its window does not fit, which the callers refuse) is clamped to
// its last sample: what such loads return is never used.  The callers put ONE mask round all 64 loads: it does not depend on the burst.
// (readlane takes offv / nm1v from EVERY lane, also from lanes that mask switches off: the callers pin them with an empty asm, or the
// compiler sinks their computation under the mask and the masked lanes' registers hold whatever was there)
template <typename SMP>
__device__ __forceinline__ void eq_load64(const void *samples, int offv, int nm1v, int idx, typename SMP::raw_t (&v)[64]) {
#pragma unroll
  for (int k = 0; k < 64; k++) {
    const int off_k = __builtin_amdgcn_readlane(offv, k), nm1_k = __builtin_amdgcn_readlane(nm1v, k);
    v[k] = SMP::ldraw(samples, (long long)off_k + (idx < nm1_k ? idx : nm1_k));
  }
}
template <typename SMP, int PITCH>
__device__ __forceinline__ void eq_park64(const typename SMP::raw_t (&v)[64], int slot, float *st_re, float *st_im) {
#pragma unroll
  for (int k = 0; k < 64; k++) { const cx f = SMP::widen(v[k]); st_re[k * PITCH + slot] = f.r; st_im[k * PITCH + slot] = f.i; }
}
template <int PITCH, int NX>
__device__ __forceinline__ void eq_unpark(const float *st_re, const float *st_im, int lane, cx (&ev)[20], cx (&wv)[NX]) {
#pragma unroll
  for (int i = 0; i < 20; i++) ev[i] = mk(st_re[lane * PITCH + i], st_im[lane * PITCH + i]);
#pragma unroll
  for (int a = 0; a < NX; a++) wv[a] = mk(st_re[lane * PITCH + 20 + a], st_im[lane * PITCH + 20 + a]);
}

// k_eq_detect: a lane per burst, every geometry (the launcher picks <12, 26> for the 52M window with maxTOA <= 5 -- 11 lags, 26 window
// samples -- and <EQ_NC, 52> for everything else: the classic 36-lag window, wide 52M windows).  Config 5's own geometry has k_eq_detect52.
template <int NCMAX, int NXMAX, typename SMP>                // correlation lags / window samples kept per burst; sample storage
__global__ __launch_bounds__(64) void k_eq_detect(const TrxTables *__restrict__ T, const void *__restrict__ samples,
                                                  const int32_t *__restrict__ offset,
                                                  const int32_t *__restrict__ length, int B, int tsc,
                                                  float detect_thresh, float energy_thresh, int variant52m,
                                                  int max_toa, uint8_t *__restrict__ flags,
                                                  cx *__restrict__ amp_out, float *__restrict__ toa_out,
                                                  float *__restrict__ toa_eq, cx *__restrict__ w_out,
                                                  cx *__restrict__ b_out, float snr_thresh, float snr_value,
                                                  float *__restrict__ chan_off_out, cx *__restrict__ chan_out,
                                                  const uint8_t *__restrict__ enable, const float *__restrict__ snr_in,
                                                  const int32_t *__restrict__ dense_gate, int dense_min) {
  // dense_gate (optional): the number of marked bursts (k_eq_list); this kernel serves the call only when they are MANY
  // (> dense_min: the wave-per-burst kernel launched before it has then left them alone), else it ends at once.
  if (dense_gate && *dense_gate <= dense_min) return;
  // enable (optional): only bursts with enable[b] != 0 are processed, nothing is written for the others (the Transceiver
  // group estimates the channel of the few bursts its replay marks, trxsig_group.hip); snr_in (optional): the SNR
  // estimate per burst.  snr_value > 0: the SNR estimate itself (the Transceiver facade forms it on the host in the reference's
  // double arithmetic, Transceiver.cpp:340); else snr_thresh >= 0: the threshold that enters
  // SNR = |amp|^2/(thr^2+1); else energy_thresh.  chan_off_out (optional): chanRespOffset (:343).
  // LDS (one wave per workgroup, a column per lane), rows of 64 complex:
  //   xp  rows [0, XROWS): the correlation window between zero pads (row PADF + a = window sample a; zeros from La on);
  //   cp  the correlation between zero pads: logical row CPAD + i = lag i.  Its front pad IS xp's last CPAD rows (window
  //       samples until the correlation is done, zeroed after it; only delayVector reads the pads);
  //   loc (peakDetect's 26 rows) and, after it, shf (the delayed correlation) reuse xp's first rows.
  // The pads turn the reference's "skip the taps that fall outside" (:480-498, :584-590) into products with zero samples
  // (+-0: adding them never changes a value), so the inner loops carry no bounds checks.  The same storage first serves as
  // the staging area of the burst loads.  29 KB for the 52M window: five workgroups per CU (four would be every one of the
  // 1024 workgroups of a 65,536-burst launch resident only if the dispatcher balanced them perfectly).
  constexpr int PADF = 10, XROWS = PADF + NXMAX, CPAD = 10, CROWS = NCMAX + CPAD;    // cp body + back pad
  constexpr int NSLOT = 20 + NXMAX, PITCH = NSLOT | 1;
  static_assert(XROWS - CPAD >= 26 && XROWS - CPAD >= NCMAX, "loc / shf must stay clear of cp's front pad");
  constexpr size_t kWork = sizeof(cx) * 64 * (XROWS + CROWS), kStage = sizeof(float) * 2 * 64 * PITCH;
  __shared__ __attribute__((aligned(16))) char lds_raw[kWork > kStage ? kWork : kStage];
  cx (*xp)[64] = reinterpret_cast<cx (*)[64]>(lds_raw);
  cx (*cp)[64] = xp + (XROWS - CPAD);
  cx (*shf)[64] = xp;
  float *st_re = reinterpret_cast<float *>(lds_raw), *st_im = st_re + 64 * PITCH;
  const int lane = threadIdx.x;
  const int b = blockIdx.x * 64 + lane;
  const bool live = b < B && (!enable || enable[b < B ? b : 0] != 0);
  if (enable && !__any(live)) return;                      // (wave-uniform: the workgroup is one wave)
  EqProbe probe;                                           // (probe builds: clock64() stamps come back through toa_out, tools/eq_probe.py)
  const int off = live ? offset[b] : 0, N = live ? length[b] : 0;
  uint8_t fl = 0;
  cx amp = mk(0, 0);
  float toa = 0.0f;
  const bool good = live && (off >= 0) && (N >= 92) && (N <= 157);
  // ---- window geometry (pure arithmetic, the same for every burst but for the length check) ----
  int ncorr, winStart, La, startIndex;
  unsigned maxTOA = (unsigned)max_toa;
  bool winOk;
  if (!variant52m) {
    ncorr = 36; winStart = 56; La = 36; startIndex = 7;    // NO_DELAY, Lb = 16 (:951-955, 295-300)
    winOk = ncorr <= NCMAX && La <= NXMAX;                 // (the launcher picks an instantiation that fits)
  } else {                                                 // ref52:983-1000
    if (maxTOA < 3) maxTOA = 3;
    unsigned spanTOA = maxTOA;
    if (spanTOA < 5) spanTOA = 5;
    winStart = (int)(66 - spanTOA);
    La = (int)(16 + 2 * spanTOA);
    ncorr = (int)(2 * maxTOA + 1);
    const unsigned expectedTOAPeak = (unsigned)round((double)((T->mid_toa[tsc] + 5.0f) + (float)(size_t)((16 - 1) / 2)));
    startIndex = (int)(expectedTOAPeak - maxTOA);
    winOk = !(ncorr > NCMAX || La > NXMAX || winStart < 0 || winStart + La > N);
  }

  // ---- the burst loads, coalesced through LDS (see eq_load64); the window's samples past La are zeros ----
  cx ev[20], wv[NXMAX];
  {
    const int step = variant52m ? 4 : 1;
    const unsigned long long goodm = __ballot(good);
    probe.stamp2();                                      // (2: 1) offsets and lengths are here
    const int safe_off = __builtin_amdgcn_readlane(off, goodm ? (int)__builtin_ctzll(goodm) : 0);
    int offv = good ? off : safe_off, nm1v = good ? N - 1 : 0;
    asm volatile("" : "+v"(offv), "+v"(nm1v));
#pragma unroll
    for (int p = 0; p < (NSLOT + 63) / 64; p++) {
      const int slot = lane + 64 * p;
      const bool slot_ok = slot < 20 + La && slot < NSLOT;
      int idx = slot >= 20 ? winStart + (slot - 20) : slot * step;
      idx = idx < 0 ? 0 : idx;
      typename SMP::raw_t v[64];                          // as stored; widened only once every load has been issued
#pragma unroll
      for (int k = 0; k < 64; k++) v[k] = SMP::zero();
      if (slot_ok && goodm) eq_load64<SMP>(samples, offv, nm1v, idx, v);
      probe.stamp2();                                    // (2: 2) loads issued
      if (slot < NSLOT) eq_park64<SMP, PITCH>(v, slot, st_re, st_im);
    }
    wave_lds_fence();
    probe.stamp2();                                      // (2: 3) loads complete, parked in LDS
    eq_unpark<PITCH>(st_re, st_im, lane, ev, wv);
    wave_lds_fence();                                      // the staging area is dead: xp / cp take its place
    probe.stamp2();                                      // (2: 4) read back
  }
  if (!live) return;                                       // no barriers below: each lane owns its columns
  if (!good) { eq_refuse(b, TRXSIG_F_BADLEN, flags, amp_out, toa_out, toa_eq); return; }
  // ---- energyDetect (:916-932; the 52M variant strides by 4, ref52:946-963) ----
  if (!eq_energy_ok(ev, energy_thresh)) { eq_refuse(b, 0, flags, amp_out, toa_out, toa_eq); return; }
  fl = TRXSIG_F_ENERGY;
  probe.stamp();                                           // 1: energy
  // ---- correlation ----
  if (!winOk) { eq_refuse(b, TRXSIG_F_BADLEN, flags, amp_out, toa_out, toa_eq); return; }
#pragma unroll
  for (int a = 0; a < PADF; a++) xp[a][lane] = mk(0, 0);
#pragma unroll
  for (int a = 0; a < NXMAX; a++) xp[PADF + a][lane] = wv[a];   // the lane's LDS column (zeros from La on)
#pragma unroll
  for (int a = 0; a < CPAD; a++) cp[CPAD + ncorr + a][lane] = mk(0, 0);
  v2f ctap[16];                                              // (packed float32 pairs from here on: see trxsig_dev.h)
#pragma unroll
  for (int j = 0; j < 16; j++) ctap[j] = pk(T->mid_ctap[tsc][15 - j]);
  // every tap index t - j of every lag lies in [-PADF, NXMAX): no checks (always so for the geometries above)
  const bool padded = startIndex - 15 >= -PADF && startIndex + ncorr - 1 < NXMAX;
  if (padded) {
    for (int i = 0; i < ncorr; i++) {
      const cx (*row)[64] = xp + (PADF + startIndex + i);
      v2f sum = pk(mk(0, 0));
#pragma unroll
      for (int j = 0; j < 16; j++) sum = pk_cadd(sum, pk_cmul(pk(row[-j][lane]), ctap[j]));   // tmp[j] = conj(mid[15-j]) (:480-498), j ascending
      cp[CPAD + i][lane] = unpk(sum);
    }
  } else {
    for (int i = 0; i < ncorr; i++) {
      const int t = startIndex + i;
      v2f sum = pk(mk(0, 0));
#pragma unroll
      for (int j = 0; j < 16; j++) {
        const int ai = t - j;
        if (ai >= 0 && ai < La) sum = pk_cadd(sum, pk_cmul(pk(xp[PADF + ai][lane]), ctap[j]));
      }
      cp[CPAD + i][lane] = unpk(sum);
    }
  }
#pragma unroll
  for (int a = 0; a < CPAD; a++) cp[a][lane] = mk(0, 0);    // the window is dead: its last rows become cp's front pad

  probe.stamp();                                           // 2: correlation
  // ---- peakDetect (:663-711) ----
  float maxP = 0.0f, maxIndex = -1.0f;
  for (int i = 0; i < ncorr; i++) {
    const float p = norm2(cp[CPAD + i][lane]);
    if (p > maxP) { maxP = p; maxIndex = (float)i; }
  }
  {
    // the bisection itself as k_tsc_peak runs it (peak_bisect: both candidate sinc rows of the next step prefetched
    // with 16-byte loads while this step computes; the eq_interp form made two dependent gather round trips per step).
    // loc = corr[M-12 .. M+11] with zeros where interpolatePoint skips (lag < 0, lag > n-2); the window's LDS is free now.
    cx (*loc)[64] = xp;
    const int M = (int)maxIndex;
#pragma unroll
    for (int j = 0; j < 24; j++) {
      const int lag = M - 12 + j;
      loc[j][lane] = (lag >= 0 && lag <= ncorr - 2) ? cp[CPAD + (lag < 0 ? 0 : (lag > NCMAX - 1 ? NCMAX - 1 : lag))][lane] : mk(0, 0);
    }
    loc[24][lane] = mk(0, 0);
    loc[25][lane] = mk(0, 0);
    float peakIx;
    amp = peak_bisect<64>(T->sinc_grid, loc, lane, M, &peakIx);
    toa = peakIx;
  }

  probe.stamp();                                           // 3: peakDetect
  // ---- analyzeTrafficBurst tail (:961-1035) ----
  bool detected = false;
  float chanOff = 0.0f;
  cx chan[6];
  if ((toa < 0.0f) || (toa > (float)ncorr)) {
    amp = mk(0, 0);
  } else {
    const int p = (int)rintf(toa);
    float valley = 0.0f;
    int numRms = 0;
    for (int i = 2; i <= 5; i++) {
      if (p - i >= 0) { valley += norm2(cp[CPAD + p - i][lane]); numRms++; }
      if (p + i < ncorr) { valley += norm2(cp[CPAD + p + i][lane]); numRms++; }
    }
    if (numRms < 2) {
      amp = mk(0, 0);
    } else {
      const float RMS = (float)((double)sqrtf(valley / (float)numRms) + 0.00001);
      const float peakToMean = sqrtf(norm2(amp)) / RMS;
      amp = cdiv(amp, T->mid_gain[tsc]);
      float TOAoffset;
      if (!variant52m) {
        toa = toa - T->mid_toa[tsc];
        toa = toa - 10.0f;
        TOAoffset = T->mid_toa[tsc] + 10.0f;
      } else {
        toa = toa - (float)maxTOA;
        TOAoffset = (float)maxTOA;
      }
      detected = peakToMean > detect_thresh;
      if (detected) {
        // delayVector(corr, -TOA) (:573-616) on the lane's column
        const float delay = -toa;
        const int io = (int)floorf(delay);
        const float frac = delay - (float)io;
        const cx (*src)[64] = cp + CPAD;
        if (fabs((double)frac) > 1e-2) {
          v2f row[12];                                     // two consecutive taps per register pair
          {
            const float4 *r4 = reinterpret_cast<const float4 *>(T->sinc_grid[(int)(frac * 512.0f) & 511]);
#pragma unroll
            for (int q = 0; q < 6; q++) { const float4 v4 = r4[q]; row[2 * q].x = v4.x; row[2 * q].y = v4.y; row[2 * q + 1].x = v4.z; row[2 * q + 1].y = v4.w; }
          }
          for (int t = 0; t < ncorr; t++) {              // taps t + 10 - j outside [0, ncorr) meet cp's zero pads
            const cx (*crow)[64] = cp + (CPAD + t + 10);
            v2f sum = pk(mk(0, 0));
#pragma unroll
            for (int j = 0; j < 21; j++)
              sum = (j & 1) ? pk_cadd(sum, pk_mul_tap<1>(pk(crow[-j][lane]), row[j >> 1])) : pk_cadd(sum, pk_mul_tap<0>(pk(crow[-j][lane]), row[j >> 1]));
            shf[t][lane] = unpk(sum);
          }
          src = shf;
        }
        // integer shift folded into the reads: w[k] = src[k - io] inside [0,n), else 0
        auto wv = [&](int k) {
          const int q = k - io;
          return (q >= 0 && q < ncorr) ? src[q][lane] : mk(0, 0);
        };
        float maxEnergy = -1.0f;
        int maxI = -1;
        for (int i = 0; i < 7; i++) {                      // :1012-1021
          const float st = TOAoffset + (float)(i - 5);
          if (st + (float)6u > (float)(unsigned)ncorr) continue;
          if (st < 0.0f) continue;
          const int s0 = (int)floorf(st);
          float energy = 0.0f;
          for (int k = 0; k < 6; k++) energy += norm2(wv(s0 + k));
          if ((double)energy > 0.95 * (double)maxEnergy) { maxI = i; maxEnergy = energy; }
        }
        const int s0 = (int)floorf(TOAoffset + (float)(maxI - 5));
        const cx ginv = cdiv(mk(1.0f, 0.0f), T->mid_gain[tsc]);
#pragma unroll
        for (int k = 0; k < 6; k++) chan[k] = cmul(wv(s0 + k), ginv);   // :1024-1025
        chanOff = (float)(5 - maxI);                       // :1029
      }
    }
  }
  fl |= detected ? TRXSIG_F_DETECT : 0;
  flags[b] = fl;
  amp_out[b] = amp;
  toa_out[b] = toa;
  toa_eq[b] = toa - chanOff;                               // equalizeBurst(..., TOA - chanRespOffset, ...)
  if (chan_off_out) chan_off_out[b] = chanOff;
  if (chan_out) {                                          // analyzeTrafficBurst's channelResponse (:1024-1025), zeros if not detected
#pragma unroll
    for (int k = 0; k < 6; k++) chan_out[(size_t)b * 6 + k] = detected ? chan[k] : mk(0, 0);
  }
  if (!detected) return;
  probe.stamp();                                           // 4: tail, delayVector, channel pick

  eq_design_store(chan, amp, snr_in != nullptr, snr_in ? snr_in[b] : 0.0f, snr_value, snr_thresh, energy_thresh, b, w_out, b_out);
  probe.report(b, toa_out);                                // 5: designDFE + taps
}

// ---------------------------------------------------------------------------------------------
// k_eq_detect52 (round 4): k_eq_detect's job for the ONE geometry config 5 runs -- the 52M window with maxTOA = 4 (nine lags from
// lag 16 on, a 26-sample window from sample 61, expectedTOAPeak = 20: ref52:983-1000; the launcher checks the last on the host's
// copy of the tables) -- with 256 threads = four waves, still a lane per burst, around ONE copy of the sinc table in LDS.
// What the general kernel spends and this one does not (tools/eq_probe.py: 67 k cycles per wave, 23 k of them in peakDetect):
//   * the bisection's sinc rows came from L2 with twelve 16-byte gathers per step, every lane another row (64 lines per
//     instruction: the texture path, shared by the CU's four waves, was the bound).  Here they are ten 4-byte LDS reads;
//   * with nine lags interpolatePoint's loop (:646-657) runs over the SAME eight lags i = 0..7 at every point the bisection
//     visits (start = max(0, floor(ix) - 10) = 0 and end = min(floor(ix) + 11, 8) = 8 for floor(ix) in [-3, 9], which
//     M - 2 <= floor(ix) <= M + 1, -1 <= M <= 8 guarantees), tap i - floor(ix) + 10 in [1, 20]: eight multiply-adds from
//     registers per point in place of twenty-one (thirteen of them products with the zeros that stood for skipped terms);
//     early, late and final point of a step share floor(early) after step 0, hence one run of ten taps serves all three;
//   * the correlation never leaves registers for the argmax, the bisection and delayVector; valley, channel pick and the
//     integer shift read their dynamic lags from the lane's LDS column with all reads in flight at once.
// Same terms in the same order as k_eq_detect (and the reference): the results are the same values.
// LDS: 48 KB table + per wave max(staging area, 18 rows of 64 complex): 96 KB (fp16 storage) / 144 KB (complex float) -- one
// workgroup per CU, as many waves per SIMD as the 64-thread form has at 65,536 bursts.
// ---------------------------------------------------------------------------------------------
template <typename SMP>
struct EqDetect52 {
  static constexpr int MT = 4, NC = 2 * MT + 1, NX = 26, START = 20 - MT, WIN0 = 61;
  static constexpr bool RAWST = sizeof(typename SMP::raw_t) == 4;
  // fp16 storage: a burst's first NCHUNK 16-byte pieces (samples 0 .. 4 NCHUNK - 1: the energy samples 0, 4, .., 76 and the window
  // 61 .. 86) are parked as stored; complex float storage: the 46 samples themselves, widened
  static constexpr int NCHUNK = (WIN0 + NX + 3) / 4;
  static constexpr int NSLOT = RAWST ? 4 * NCHUNK : 20 + NX, PITCH = NSLOT | 1;
  static constexpr size_t kStage = (RAWST ? sizeof(unsigned) : sizeof(float) * 2) * 64 * PITCH;
  static constexpr size_t kCols = sizeof(cx) * 64 * (2 * NC);
  static constexpr size_t kSlice = ((kStage > kCols ? kStage : kCols) + 15) & ~(size_t)15;
  static constexpr size_t kLds = sizeof(SincLds) + 4 * kSlice;
};

template <typename SMP>
__global__ __launch_bounds__(256) void k_eq_detect52(const TrxTables *__restrict__ T, const void *__restrict__ samples,
                                                     const int32_t *__restrict__ offset, const int32_t *__restrict__ length, int B, int tsc,
                                                     float detect_thresh, float energy_thresh, uint8_t *__restrict__ flags,
                                                     cx *__restrict__ amp_out, float *__restrict__ toa_out, float *__restrict__ toa_eq,
                                                     cx *__restrict__ w_out, cx *__restrict__ b_out, float snr_thresh, float snr_value,
                                                     float *__restrict__ chan_off_out, cx *__restrict__ chan_out,
                                                     const uint8_t *__restrict__ enable, const float *__restrict__ snr_in) {
  typedef EqDetect52<SMP> G;
  constexpr int NC = G::NC, NX = G::NX, PITCH = G::PITCH, NSLOT = G::NSLOT;
  extern __shared__ __attribute__((aligned(16))) char lds52[];
  SincLds &stab = *reinterpret_cast<SincLds *>(lds52);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  char *mine = lds52 + sizeof(SincLds) + (size_t)wave * G::kSlice;
  cx (*cp)[64] = reinterpret_cast<cx (*)[64]>(mine);        // the correlation, a column per lane; shf: its delayed copy
  cx (*shf)[64] = cp + NC;
  float *st_re = reinterpret_cast<float *>(mine), *st_im = st_re + 64 * PITCH;
  typename SMP::raw_t *st_raw = reinterpret_cast<typename SMP::raw_t *>(mine);
  const int b = blockIdx.x * 256 + tid;
  const bool live = b < B && (!enable || enable[b < B ? b : 0] != 0);
  if (enable && !__syncthreads_or(live)) return;            // (workgroup-uniform)
  EqProbe probe;
  const int off = live ? offset[b] : 0, N = live ? length[b] : 0;
  // (loaded here, with the offsets: a load issued behind the result stores further down would make the wave wait for those stores to land --
  //  the counter of outstanding memory operations does not tell loads from stores -- before designDFE could start)
  const float snr_pre = (snr_in && live) ? snr_in[b] : 0.0f;
  uint8_t fl = 0;
  cx amp = mk(0, 0);
  float toa = 0.0f;
  const bool good = live && (off >= 0) && (N >= 92) && (N <= 157);
  const bool winOk = G::WIN0 + NX <= N;                     // ref52:993-1000: the window must lie inside the burst
  // ---- the burst loads, coalesced through LDS exactly as k_eq_detect does them (see there) ----
  cx ev[20], wv[NX];
  {
    const unsigned long long goodm = __ballot(good);
    probe.stamp2();                                        // (2: 1) offsets and lengths are here
    const int safe_off = __builtin_amdgcn_readlane(off, goodm ? (int)__builtin_ctzll(goodm) : 0);
    int offv = good ? off : safe_off, nm1v = good ? N - 1 : 0;
    asm volatile("" : "+v"(offv), "+v"(nm1v));
    if constexpr (G::RAWST) {
      // fp16 storage: TWO bursts per load instruction, a lane per 16-byte piece (lanes 0..21 burst 2 j, lanes 32..53 burst 2 j + 1):
      // the same lines as a lane per sample would touch, in half the load instructions, four samples per lane.  (A good burst has
      // at least 92 samples: pieces 0 .. NCHUNK - 1 = samples 0..87 lie inside it.)
      static_assert(G::NCHUNK <= 32 && 4 * G::NCHUNK <= 92, "two bursts per wave instruction, inside the shortest burst");
      struct __attribute__((packed, aligned(4))) Piece { unsigned q[4]; };
      const int c = lane & 31, half = lane >> 5;
      const bool piece_ok = c < G::NCHUNK;
      Piece v[32];
#pragma unroll
      for (int j = 0; j < 32; j++) v[j] = Piece{{0u, 0u, 0u, 0u}};
      int off_k[32];                                       // (every lane takes part in the exchange: before the branch)
#pragma unroll
      for (int j = 0; j < 32; j++) off_k[j] = __shfl(offv, 2 * j + half, 64);
      if (piece_ok && goodm) {
#pragma unroll
        for (int j = 0; j < 32; j++)
          v[j] = *reinterpret_cast<const Piece *>(reinterpret_cast<const unsigned *>(samples) + ((long long)off_k[j] + 4 * c));
      }
      probe.stamp2();                                      // (2: 2) loads issued
      {                                                    // the table's loads queue behind the bursts': nothing waits for them alone
        float4 tv[3072 / 256];
        sinc_lds_issue<256>(T, tid, tv);
        sinc_lds_store<256>(stab, tid, tv);
      }
      if (piece_ok) {
#pragma unroll
        for (int j = 0; j < 32; j++) {
#pragma unroll
          for (int q = 0; q < 4; q++) st_raw[(2 * j + half) * PITCH + 4 * c + q] = v[j].q[q];
        }
      }
      wave_lds_fence();
      probe.stamp2();                                      // (2: 3) loads complete, table and bursts parked
#pragma unroll
      for (int i = 0; i < 20; i++) ev[i] = SMP::widen(st_raw[lane * PITCH + 4 * i]);   // energyDetect strides by 4 (ref52:946-963)
#pragma unroll
      for (int a = 0; a < NX; a++) wv[a] = SMP::widen(st_raw[lane * PITCH + G::WIN0 + a]);
    } else {
      const int slot = lane;
      const bool slot_ok = slot < NSLOT;
      const int idx = slot >= 20 ? G::WIN0 + (slot - 20) : slot * 4;   // energyDetect strides by 4 (ref52:946-963)
      typename SMP::raw_t v[64];
#pragma unroll
      for (int k = 0; k < 64; k++) v[k] = SMP::zero();
      if (slot_ok && goodm) eq_load64<SMP>(samples, offv, nm1v, idx, v);
      probe.stamp2();                                    // (2: 2) loads issued
      {
        float4 tv[3072 / 256];
        sinc_lds_issue<256>(T, tid, tv);
        sinc_lds_store<256>(stab, tid, tv);
      }
      if (slot_ok) eq_park64<SMP, PITCH>(v, slot, st_re, st_im);
      wave_lds_fence();
      probe.stamp2();                                    // (2: 3) loads complete, table and bursts parked
      eq_unpark<PITCH>(st_re, st_im, lane, ev, wv);
    }
    wave_lds_fence();                                      // the staging area is dead: cp / shf take its place
  }
  probe.stamp2();                                          // (2: 4) read back
  __syncthreads();                                         // the table is whole; no barrier below (each lane owns its columns)
  probe.stamp2();                                          // (2: 5) barrier
  if (!live) return;
  if (!good || !winOk) {
    // (energyDetect comes first in the reference: a short burst that fails it reports 0, not BADLEN -- as k_eq_detect)
    eq_refuse(b, (!good || eq_energy_ok(ev, energy_thresh)) ? TRXSIG_F_BADLEN : 0, flags, amp_out, toa_out, toa_eq);
    return;
  }
  // ---- energyDetect ----
  if (!eq_energy_ok(ev, energy_thresh)) { eq_refuse(b, 0, flags, amp_out, toa_out, toa_eq); return; }
  fl = TRXSIG_F_ENERGY;
  probe.stamp();                                           // 1: energy
  // ---- correlation (:480-498): lag i ends on window sample START + i; tmp[j] = conj(mid[15 - j]), j ascending ----
  v2f cr[NC];
  {
    v2f ctap[16];
#pragma unroll
    for (int j = 0; j < 16; j++) ctap[j] = pk(T->mid_ctap[tsc][15 - j]);
#pragma unroll
    for (int i = 0; i < NC; i++) {
      v2f sum = pk(mk(0, 0));
#pragma unroll
      for (int j = 0; j < 16; j++) sum = pk_cadd(sum, pk_cmul(pk(wv[G::START + i - j]), ctap[j]));
      cr[i] = sum;
      cp[i][lane] = unpk(sum);
    }
  }
  static_assert(G::START - 15 >= 0 && G::START + NC - 1 < NX, "every tap of every lag lies inside the window");
  probe.stamp();                                           // 2: correlation
  // ---- peakDetect (:663-711) ----
  float maxP = 0.0f, maxIndex = -1.0f;
#pragma unroll
  for (int i = 0; i < NC; i++) {
    const float p = norm2(unpk(cr[i]));
    if (p > maxP) { maxP = p; maxIndex = (float)i; }
  }
  int e = 0;
  {
    const int M = (int)maxIndex;
    // the ten taps row[f][col0 .. col0 + 9], col0 = 8 - floor(early): late point = taps 0..7, final point 1..8, early point 2..9
    v2f t[5];
    auto load_taps = [&](int f, int col0) {
      const float *rw = &stab.row[f][col0];
#pragma unroll
      for (int k = 0; k < 5; k++) { t[k].x = rw[2 * k]; t[k].y = rw[2 * k + 1]; }
    };
    auto point = [&](auto sh) {                            // interpolatePoint: sum over lags 0..7 of corr[i] * tap[sh + i], i ascending
      constexpr int SH = decltype(sh)::value;
      v2f pt = pk(mk(0, 0));
#pragma unroll
      for (int i = 0; i < NC - 1; i++)
        pt = ((SH + i) & 1) ? pk_cadd(pt, pk_mul_tap<1>(cr[i], t[(SH + i) >> 1])) : pk_cadd(pt, pk_mul_tap<0>(cr[i], t[(SH + i) >> 1]));
      return unpk(pt);
    };
    bool active = true;
    auto decide = [&](int inc) {                           // :690-697
      const float ne = norm2(point(std::integral_constant<int, 2>())), nl = norm2(point(std::integral_constant<int, 0>()));
      if (active) {
        if (ne < nl) e += inc;
        else if (ne > nl) e -= inc;
        else active = false;                               // "else break" (:695)
      }
    };
    load_taps(0, 9 - M);                                   // early = M - 1: floor = M - 1
    decide(256);
    const int col0 = e < 0 ? 10 - M : 9 - M;               // floor(early) = M - 2 once the first step went down, else M - 1: it stays
#pragma unroll 1
    for (int inc = 128; inc >= 1; inc >>= 1) {             // increments 2^-2 .. 2^-9
      load_taps(e & 511, col0);
      decide(inc);
    }
    load_taps(e & 511, col0);                              // early + 1 has the same fractional part
    amp = point(std::integral_constant<int, 1>());
    toa = ((float)(M - 1) + (float)e * 0.001953125f) + 1.0f;   // exact: the reference's +-2^-k steps are exact too
  }
  probe.stamp();                                           // 3: peakDetect
  // ---- analyzeTrafficBurst's tail (:961-1035, ref52) ----
  bool detected = false;
  float chanOff = 0.0f;
  cx chan[6];
  if ((toa < 0.0f) || (toa > (float)NC)) {
    amp = mk(0, 0);
  } else {
    const int p = (int)rintf(toa);
    cx vlo[4], vhi[4];
#pragma unroll
    for (int i = 2; i <= 5; i++) {                          // all eight reads in flight
      const int a = p - i, c = p + i;
      vlo[i - 2] = cp[a < 0 ? 0 : (a > NC - 1 ? NC - 1 : a)][lane];
      vhi[i - 2] = cp[c < 0 ? 0 : (c > NC - 1 ? NC - 1 : c)][lane];
    }
    float valley = 0.0f;
    int numRms = 0;
#pragma unroll
    for (int i = 2; i <= 5; i++) {
      if (p - i >= 0) { valley += norm2(vlo[i - 2]); numRms++; }
      if (p + i < NC) { valley += norm2(vhi[i - 2]); numRms++; }
    }
    if (numRms < 2) {
      amp = mk(0, 0);
    } else {
      const float RMS = (float)((double)sqrtf(valley / (float)numRms) + 0.00001);
      const float peakToMean = sqrtf(norm2(amp)) / RMS;
      amp = cdiv(amp, T->mid_gain[tsc]);
      toa = toa - (float)(unsigned)G::MT;
      const float TOAoffset = (float)(unsigned)G::MT;
      detected = peakToMean > detect_thresh;
      if (detected) {
        // delayVector(corr, -TOA) (:573-616): a tap that would meet a lag outside [0, NC) is not formed (it would add +-0)
        const float delay = -toa;
        const int io = (int)floorf(delay);
        const float frac = delay - (float)io;
        const cx (*src)[64] = cp;
        if (fabs((double)frac) > 1e-2) {
          v2f row[12];
          {
            const float4 *r4 = reinterpret_cast<const float4 *>(stab.row[(int)(frac * 512.0f) & 511]);
#pragma unroll
            for (int q = 0; q < 6; q++) { const float4 v4 = r4[q]; row[2 * q].x = v4.x; row[2 * q].y = v4.y; row[2 * q + 1].x = v4.z; row[2 * q + 1].y = v4.w; }
          }
#pragma unroll
          for (int tq = 0; tq < NC; tq++) {
            v2f sum = pk(mk(0, 0));
#pragma unroll
            for (int j = 0; j < 21; j++) {
              const int q = tq + 10 - j;
              if (q >= 0 && q < NC)
                sum = (j & 1) ? pk_cadd(sum, pk_mul_tap<1>(cr[q < 0 ? 0 : (q >= NC ? NC - 1 : q)], row[j >> 1]))
                              : pk_cadd(sum, pk_mul_tap<0>(cr[q < 0 ? 0 : (q >= NC ? NC - 1 : q)], row[j >> 1]));
            }
            shf[tq][lane] = unpk(sum);
          }
          src = shf;
        }
        // integer shift folded into the reads: w[k] = src[k - io] inside [0, NC), else 0
        auto wdyn = [&](int k) {
          const int q = k - io;
          return (q >= 0 && q < NC) ? src[q][lane] : mk(0, 0);
        };
        cx wk[NC];
#pragma unroll
        for (int k = 0; k < NC; k++) {
          const int q = k - io;
          const cx r = src[q < 0 ? 0 : (q > NC - 1 ? NC - 1 : q)][lane];
          wk[k] = (q >= 0 && q < NC) ? r : mk(0, 0);
        }
        float nk[NC];
#pragma unroll
        for (int k = 0; k < NC; k++) nk[k] = norm2(wk[k]);
        // :1012-1021 with TOAoffset = 4 and nine lags: windows i = 1..4 start on lag i - 1 (i = 0: st < 0; i = 5, 6: st + 6 > 9)
        float maxEnergy = -1.0f;
        int maxI = -1;
#pragma unroll
        for (int i = 1; i <= 4; i++) {
          float energy = 0.0f;
#pragma unroll
          for (int k = 0; k < 6; k++) energy += nk[i - 1 + k];
          if ((double)energy > 0.95 * (double)maxEnergy) { maxI = i; maxEnergy = energy; }
        }
        static_assert(G::MT == 4 && NC == 9, "the window list above");
        const cx ginv = cdiv(mk(1.0f, 0.0f), T->mid_gain[tsc]);
        // (dynamic reads of the lane's column again: a select chain over wk[] makes the compiler put wk[] in scratch.  maxI = -1 --
        //  no window taken, energies that do not compare: NaN -- reads from TOAoffset - 6 on like the reference)
        const int s0 = (int)floorf(TOAoffset + (float)(maxI - 5));
#pragma unroll
        for (int k = 0; k < 6; k++) chan[k] = cmul(wdyn(s0 + k), ginv);   // :1024-1025
        chanOff = (float)(5 - maxI);                       // :1029
      }
    }
  }
  fl |= detected ? TRXSIG_F_DETECT : 0;
  flags[b] = fl;
  amp_out[b] = amp;
  toa_out[b] = toa;
  toa_eq[b] = toa - chanOff;
  if (chan_off_out) chan_off_out[b] = chanOff;
  if (chan_out) {
#pragma unroll
    for (int k = 0; k < 6; k++) chan_out[(size_t)b * 6 + k] = detected ? chan[k] : mk(0, 0);
  }
  if (!detected) return;
  probe.stamp();                                           // 4: tail, delayVector, channel pick
  eq_design_store(chan, amp, snr_in != nullptr, snr_pre, snr_value, snr_thresh, energy_thresh, b, w_out, b_out);
  probe.report(b, toa_out);
}

// designDFE(Nf = 7, nu = 5) with the lanes of a wave (design_dfe7 above is the same computation in one lane): lane q holds G0[q] and
// G1[q]; every iteration of the recursion (:1270-1297) updates the seven columns side by side, element 0 is broadcast, G1's delay by
// one (:1292) is a shift between neighbouring lanes.  Lane k's column quotients L[i][i + k] go to LDS for the back-substitution
// (:1310-1319), which is serial and done by every lane alike; lane i then forms w[i] (:1323-1335).  Every element sees the operations
// design_dfe7 applies to it, in the same order: the same values.  Results: lane i < 7 returns w[i], lane j + 1 (j < 5) returns b[j].
// Lu_s: 36 complex, v_s: 8 complex of the wave's LDS.
__device__ __forceinline__ void design_dfe7_lanes(const cx (&chan)[6], float snr, int lane, cx *Lu_s, cx *v_s, cx &w_mine, cx &b_mine) {
  constexpr int Nf = 7, nu = 5;
  auto conj2 = [](v2f z) { v2f r; r.x = z.x; r.y = -z.y; return r; };
  auto nrm = [](v2f z) { return z.y * z.y + z.x * z.x; };    // Complex::norm2 (Complex.h:119)
  auto bcast0 = [](v2f z) {
    v2f r;
    r.x = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(z.x), 0));
    r.y = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(z.y), 0));
    return r;
  };
  const int q = lane < Nf ? lane : Nf - 1;                   // (lanes beyond the seventh shadow lane 6: their values are never used)
  v2f G0 = pk(mk(0, 0)), G1 = pk(mk(0, 0));
  if (q == 0) G0 = pk(mk((float)(1.0 / (double)sqrtf(snr)), 0.0f));   // :1261
#pragma unroll
  for (int j = 0; j <= nu; j++)
    if (q == j) G1 = pk(mk(chan[j].r, -chan[j].i));
  v2f lfb = pk(mk(0, 0));
  float d = 0.0f;
#pragma unroll
  for (int i = 0; i < Nf; i++) {
    const v2f G00 = bcast0(G0), G10 = bcast0(G1);
    d = nrm(G00) + nrm(G10);                                 // :1272
    const v2f g0c = conj2(G00), g1c = conj2(G10);
    {                                                        // *Lptr = (G0[k]*conj(G0[0]) + G1[k]*conj(G1[0]))/d (:1277), k = this lane
      const v2f tt = pk_cadd(pk_cmul(G0, g0c), pk_cmul(G1, g1c));
      v2f v; v.x = tt.x / d; v.y = tt.y / d;
      const int col = i + q;
      if (i < Nf - 1) { if (q >= 1 && col <= Nf - 1 && lane < Nf) Lu_s[i * 6 + (q - 1)] = unpk(v); }
      else if (q >= 1 && col >= Nf && col < Nf + nu) lfb = v;
    }
    v2f kk;                                                  // G1[0] / G0[0] (:1282)
    {
      const float n = nrm(G00);
      v2f inv; inv.x = G00.x / n; inv.y = -G00.y / n;
      kk = pk_cmul(G10, inv);
    }
    if (i != Nf - 1) {
      const v2f kc = conj2(kk);
      v2f km; km.x = kk.x * -1.0f; km.y = kk.y * -1.0f;
      const v2f G0n = pk_cadd(pk_cmul(G1, kc), G0);          // :1285-1287
      v2f G1n = pk_cadd(pk_cmul(G0, km), G1);                // :1289-1291
      v2f sh;                                                // delayVector(G1new, -1) (:1292): lane q takes lane q + 1's, the last a zero
      sh.x = __shfl_down(G1n.x, 1, 64); sh.y = __shfl_down(G1n.y, 1, 64);
      G1n = (lane < Nf - 1) ? sh : pk(mk(0, 0));
      const v2f sc = pk(mk((float)(1.0 / (double)sqrtf((float)(1.0 + (double)nrm(kk)))), 0.0f));   // :1294-1295
      G0 = pk_cmul(G0n, sc);
      G1 = pk_cmul(G1n, sc);
    }
  }
  {                                                          // :1301-1304: * -1, conj
    const v2f t1 = pk_cmul(lfb, pk(mk(-1.0f, 0.0f)));
    b_mine = mk(t1.x, -t1.y);
  }
  wave_lds_fence();
  v2f v[Nf];
  v[Nf - 1] = pk(mk(1.0f, 0.0f));
#pragma unroll
  for (int k = Nf - 2; k >= 0; k--) {                        // :1310-1319
    v2f vk = pk(mk(0, 0));
#pragma unroll
    for (int j = k + 1; j < Nf; j++) vk = pk_csub(vk, pk_cmul(v[j], pk(Lu_s[k * 6 + (j - k - 1)])));
    v[k] = vk;
  }
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < Nf; k++) v_s[k] = unpk(v[k]);
  }
  wave_lds_fence();
  {                                                          // :1323-1335, i = this lane
    v2f wi = pk(mk(0, 0));
    const int endPt = (nu < (Nf - 1 - q)) ? nu : (Nf - 1 - q);
#pragma unroll
    for (int k = 0; k < Nf - 1; k++)
      if (k < endPt + 1) wi = pk_cadd(wi, pk_cmul(pk(v_s[q + k < Nf ? q + k : Nf - 1]), pk(mk(chan[k].r, -chan[k].i))));
    w_mine = mk(wi.x / d, wi.y / d);
  }
}

// ---------------------------------------------------------------------------------------------
// k_eq_list + k_eq_estimate_wave (round 4): analyzeTrafficBurst(requestChannel) + designDFE for FEW bursts, a WAVE per burst.
// The Transceiver asks for a channel estimate once per timeslot and 51 frames (Transceiver.cpp:313-325): of the group's rows some 2 %
// are marked, one or two per wave of a lane-per-burst kernel -- k_eq_detect<36, 52> then runs 936 waves at one or two active lanes
// each and takes one wave's full latency (46 us with VALU 0 % busy, profiles/r04_pmc_config4_reference_chain.txt), and the one-ARFCN
// object's one-burst call (trxsig_estimate_dfe_batch, B = 1) pays the same.  Here the marked bursts are listed first (k_eq_list: one
// workgroup, a prefix sum over the flags -- the list comes out in the same order every run) and each listed burst gets a wave:
//   lanes 0..35 the 36 lags of the correlation (sigProcLib.cpp:480-498; the Transceiver/ variant: whole 36-lag window from sample 56);
//   the argmax by a wave reduction with the reference's first-maximum rule; peakDetect's bisection SPECULATED in two super-steps
//   (trxsig_bisect.h: every node of the next five / four levels evaluated at once, the decisions replayed along the reference's path);
//   fused_tail (valley, peak-to-mean, TOA bookkeeping); lanes 0..35 the outputs of delayVector on the correlation; lanes 0..6 the
//   channel-pick windows; designDFE with a lane per column of its generator recursion (design_dfe7_lanes).
// Each value is formed by the same operations in the same order as in k_eq_detect (and the reference): same results.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(1024) void k_eq_list(const uint8_t *__restrict__ enable, int B, int32_t *__restrict__ list, int32_t *__restrict__ count) {
  // thread t owns bursts t, t + 1024, t + 2048, ...: a wave's loads are 64 consecutive bytes, 32 of a thread's in flight at a time
  // (unconditional, index clamped: a load under a branch is waited for at the join).  The first 64 flags of a thread are kept as a
  // bit mask, so a call of up to 65,536 bursts reads its flags once.  The list holds thread 0's bursts first, then thread 1's, ...:
  // not sorted, but the same on every run.
  __shared__ int wsum[16];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int K = (B + 1023) / 1024;
  int n = 0;
  unsigned long long m = 0;
  for (int k0 = 0; k0 < K; k0 += 32) {
    uint8_t v[32];
#pragma unroll
    for (int u = 0; u < 32; u++) { const int i = (k0 + u) * 1024 + t; v[u] = enable[i < B ? i : B - 1]; }
#pragma unroll
    for (int u = 0; u < 32; u++) {
      const bool on = ((k0 + u) * 1024 + t < B) && v[u] != 0;
      n += on;
      if (k0 + u < 64) m |= (unsigned long long)on << ((k0 + u) & 63);
    }
  }
  int incl = n;                                             // inclusive prefix sum: inside the wave, then over the sixteen waves
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) { const int o = __shfl_up(incl, d, 64); if (lane >= d) incl += o; }
  if (lane == 63) wsum[wave] = incl;
  __syncthreads();
  int before = 0;
#pragma unroll
  for (int w = 0; w < 16; w++) before += w < wave ? wsum[w] : 0;
  int pos = before + incl - n;
  while (m) {
    const int k = (int)__builtin_ctzll(m);
    m &= m - 1;
    list[pos++] = k * 1024 + t;
  }
  for (int k = 64; k < K; k++) {                            // (calls beyond 65,536 bursts)
    const int i = k * 1024 + t;
    if (i < B && enable[i] != 0) list[pos++] = i;
  }
  if (t == 1023) *count = before + incl;
}

template <typename SMP>
__global__ __launch_bounds__(256) void k_eq_estimate_wave(const TrxTables *__restrict__ T, const void *__restrict__ samples,
                                                          const int32_t *__restrict__ offset, const int32_t *__restrict__ length, int B, int tsc,
                                                          float detect_thresh, uint8_t *__restrict__ flags, cx *__restrict__ amp_out,
                                                          float *__restrict__ toa_out, float *__restrict__ toa_eq, cx *__restrict__ w_out,
                                                          cx *__restrict__ b_out, float snr_thresh, float snr_value,
                                                          float *__restrict__ chan_off_out, cx *__restrict__ chan_out,
                                                          const float *__restrict__ snr_in, const int32_t *__restrict__ list,
                                                          const int32_t *__restrict__ count, int dense_min) {
  constexpr int NL = 36, FRONT = 8, BACK = 8, PADC = 13, W0 = 56, START = 7;   // :951-955, 295-300: NO_DELAY correlation, Lb = 16
  static_assert(START - 15 >= -FRONT && START + NL - 1 < NL + BACK, "every tap of every lag meets a sample or a zero pad");
  __shared__ cx Ws[4][FRONT + NL + BACK];
  __shared__ cx Cs[4][PADC + NL + PADC];
  __shared__ cx locs[4][26];
  __shared__ cx shfs[4][NL];
  __shared__ __attribute__((aligned(16))) float Vs[4][8];
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  cx *W = Ws[wave], *Cc = Cs[wave], *loc = locs[wave], *shf = shfs[wave];
  float *V = Vs[wave];
  const int n_waves = gridDim.x * 4, w0 = blockIdx.x * 4 + wave;
  const int n = list ? *count : B;
  if (list && n > dense_min) return;                         // many marked bursts: k_eq_detect, launched next, takes the call
  const cx gain = T->mid_gain[tsc];
  const float mid_toa = T->mid_toa[tsc];
  cx ctap[16];
#pragma unroll
  for (int j = 0; j < 16; j++) ctap[j] = T->mid_ctap[tsc][15 - j];   // tmp[j] = conj(mid[15 - j]) (:480-498)
  for (int it = w0; it < n; it += n_waves) {
    const int b = __builtin_amdgcn_readfirstlane(list ? list[it] : it);
    const int off = offset[b], N = length[b];
    if (!((off >= 0) && (N >= 92) && (N <= 157))) {
      if (lane == 0) eq_refuse(b, TRXSIG_F_BADLEN, flags, amp_out, toa_out, toa_eq);
      continue;
    }
    // ---- the window between zero pads; the correlation's pads ----
    if (lane < FRONT) W[lane] = mk(0, 0);
    if (lane < BACK) W[FRONT + NL + lane] = mk(0, 0);
    if (lane < PADC) { Cc[lane] = mk(0, 0); Cc[PADC + NL + lane] = mk(0, 0); }
    if (lane < NL) W[FRONT + lane] = SMP::ld(samples, (long long)off + W0 + lane);
    wave_lds_fence();
    // ---- correlation: lag i = lane ends on window sample START + i; j ascending ----
    float P = 0.0f;
    int Tm = -1;
    if (lane < NL) {
      cx acc = mk(0, 0);
      const cx *wp = W + (FRONT + START + lane);
#pragma unroll
      for (int j = 0; j < 16; j++) acc = cadd(acc, cmul(wp[-j], ctap[j]));
      Cc[PADC + lane] = acc;
      const float pw = norm2(acc);
      if (pw > 0.0f) { P = pw; Tm = lane; }                 // "if (p > maxP)" from maxP = 0 (:675): a lag without power is never the maximum
    }
    // the first super-step's points do not depend on the data (early starts at M - 1): fetch its sinc rows under the reduction
    const int relA = kFusedRel5.v[lane];
    const int eA = (relA >> 2) * 16;
    float rowA[24];
    fused_row(T, eA, rowA);
    wave_argmax(P, Tm);                                     // larger power wins, equal power: the smaller lag (the first maximum)
    const int M = Tm;
    wave_lds_fence();
    if (lane < 26) {                                        // lags M-12 .. M+11 as interpolatePoint sees them (never the last sample, :646)
      const int lag = M - 12 + lane;
      loc[lane] = (lane >= 24 || lag < 0 || lag > NL - 2) ? mk(0, 0) : Cc[PADC + lag];
    }
    wave_lds_fence();
    // ---- peakDetect's bisection, speculated (k_normal_fused's arrangement for 64 lanes per burst) ----
    int e = 0;                                              // early = M-1 + e/512
    bool active = true;
    cx peak = mk(0, 0);
    {
      const cx ptA = fused_point(loc, eA, relA & 3, rowA);                  // levels 1-5: +-256 .. +-16
      fused_decide<64, 5, false>(ptA, lane, 256, e, active, peak);
      const int relB = kFusedRel4F.v[lane], eB = e + (relB >> 2);           // levels 6-9: +-8 .. +-1, and the finals
      float rowB[24];
      fused_row(T, eB, rowB);
      const cx ptB = fused_point(loc, eB, relB & 3, rowB);
      fused_decide<64, 4, true>(ptB, lane, 8, e, active, peak);
    }
    if (!active) {                                          // the reference left its loop on equal powers (:695): interpolatePoint(early + 1) where it stopped
      float srow[24];
      fused_row(T, e, srow);
      peak = fused_point(loc, e, 1, srow);
    }
    cx amp;
    float toa;
    bool detected, energy_ok;
    fused_tail<1, 64>([&](int lag) { return norm2(Cc[PADC + lag]); }, V, lane, M, e, peak, true, 0.0f, cinv(gain), mid_toa, detect_thresh,
                      -1.0f, amp, toa, detected, energy_ok);
    float chanOff = 0.0f;
    cx chan[6];
#pragma unroll
    for (int k = 0; k < 6; k++) chan[k] = mk(0, 0);
    if (detected) {                                         // (wave-uniform)
      const float TOAoffset = mid_toa + 10.0f;
      // delayVector(corr, -TOA) (:573-616): output t = lane; taps t + 10 - j outside [0, 36) meet the zero pads
      const float delay = -toa;
      const int io = (int)floorf(delay);
      const float frac = delay - (float)io;
      const cx *src = Cc + PADC;
      if (fabs((double)frac) > 1e-2) {
        const float *row = T->sinc_grid[(int)(frac * 512.0f) & 511];
        if (lane < NL) {
          cx sum = mk(0, 0);
          const cx *cp = Cc + (PADC + lane + 10);
#pragma unroll
          for (int j = 0; j < 21; j++) sum = cadd(sum, cmulr(cp[-j], row[j]));
          shf[lane] = sum;
        }
        src = shf;
        wave_lds_fence();
      }
      auto wv = [&](int k) {                                // the integer shift folded into the reads
        const int q = k - io;
        return (q >= 0 && q < NL) ? src[q] : mk(0, 0);
      };
      // :1012-1021: window i = lane
      float energy = 0.0f;
      bool valid = false;
      if (lane < 7) {
        const float st = TOAoffset + (float)(lane - 5);
        valid = !(st + (float)6u > (float)(unsigned)NL) && !(st < 0.0f);
        const int s0 = (int)floorf(st);
        for (int k = 0; k < 6; k++) energy += norm2(wv(s0 + k));
      }
      float maxEnergy = -1.0f;
      int maxI = -1;
#pragma unroll
      for (int i = 0; i < 7; i++) {
        const float en = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(energy), i));
        const bool ok = __builtin_amdgcn_readlane((int)valid, i) != 0;
        if (ok && (double)en > 0.95 * (double)maxEnergy) { maxI = i; maxEnergy = en; }
      }
      const int s0 = (int)floorf(TOAoffset + (float)(maxI - 5));
      const cx ginv = cdiv(mk(1.0f, 0.0f), gain);
#pragma unroll
      for (int k = 0; k < 6; k++) chan[k] = cmul(wv(s0 + k), ginv);   // :1024-1025
      chanOff = (float)(5 - maxI);                           // :1029
    }
    if (lane == 0) {
      flags[b] = (uint8_t)(TRXSIG_F_ENERGY | (detected ? TRXSIG_F_DETECT : 0));
      amp_out[b] = amp;
      toa_out[b] = toa;
      toa_eq[b] = toa - chanOff;
      if (chan_off_out) chan_off_out[b] = chanOff;
    }
    if (chan_out && lane == 0) {                           // zeros if not detected
#pragma unroll
      for (int k = 0; k < 6; k++) chan_out[(size_t)b * 6 + k] = chan[k];
    }
    if (detected) {
      // Transceiver.cpp:341-347: SNR, scaleVector(chan, 1/amp), designDFE(chan, SNR, 7)
      const float thr = snr_thresh >= 0.0f ? snr_thresh : 0.0f;
      const float snr = snr_in ? snr_in[b] : (snr_value > 0.0f ? snr_value : (float)((double)norm2(amp) / ((double)(thr * thr) + 1.0)));
      const cx ainv = cdiv(mk(1.0f, 0.0f), amp);
#pragma unroll
      for (int k = 0; k < 6; k++) chan[k] = cmul(chan[k], ainv);
      cx w_mine, b_mine;
      design_dfe7_lanes(chan, snr, lane, shf, loc, w_mine, b_mine);   // (shf, loc: dead by now)
      if (lane < 7) w_out[(size_t)b * 7 + lane] = w_mine;
      if (lane >= 1 && lane < 6) b_out[(size_t)b * 5 + (lane - 1)] = b_mine;
    }
    wave_lds_fence();                                       // the next burst reuses the wave's LDS
  }
}

// designDFE on its own (a lane per channel estimate): chan B x 6 (as analyzeTrafficBurst returns it, i.e. before the
// 1/amp scaling -- pass amp = NULL if the caller has scaled it already), snr B floats
__global__ __launch_bounds__(64) void k_design_dfe(const cx *__restrict__ chan_in, const cx *__restrict__ amp, const float *__restrict__ snr,
                                                   int B, cx *__restrict__ w_out, cx *__restrict__ b_out) {
  const int b = blockIdx.x * 64 + threadIdx.x;
  if (b >= B) return;
  cx chan[6], w[7], bq[5];
#pragma unroll
  for (int k = 0; k < 6; k++) chan[k] = chan_in[(size_t)b * 6 + k];
  if (amp) {
    const cx ainv = cdiv(mk(1.0f, 0.0f), amp[b]);          // scaleVector(chan, 1/amp) (Transceiver.cpp:346)
#pragma unroll
    for (int k = 0; k < 6; k++) chan[k] = cmul(chan[k], ainv);
  }
  design_dfe7(chan, snr[b], w, bq);
#pragma unroll
  for (int i = 0; i < 7; i++) w_out[(size_t)b * 7 + i] = w[i];
#pragma unroll
  for (int j = 0; j < 5; j++) b_out[(size_t)b * 5 + j] = bq[j];
}

}  // namespace

// k_eq_detect52 needs more LDS than a kernel gets by default: raise the limit once per instantiation
template <typename SMP, typename... A>
static hipError_t launch_eq_detect52(hipStream_t st, int B, A... a) {
  static bool raised[64] = {};                              // per device (a process may drive several)
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return hipErrorInvalidDevice;
  if (!raised[dev]) {                                       // (idempotent: two threads racing here both set the same value)
    const hipError_t attr = hipFuncSetAttribute(reinterpret_cast<const void *>(&k_eq_detect52<SMP>),
                                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)EqDetect52<SMP>::kLds);
    if (attr != hipSuccess) return attr;
    raised[dev] = true;
  }
  k_eq_detect52<SMP><<<dim3((B + 255) / 256), dim3(256), EqDetect52<SMP>::kLds, st>>>(a...);
  return hipSuccess;
}
// A lane per burst: k_eq_detect52 for config 5's geometry (52M window, maxTOA 4, expectedTOAPeak 20: `geom52`, which the caller derives from
// the host's copy of the tables -- trx_eq52_geometry, trxsig_launch.h); else k_eq_detect: <12, 26> for the 52M window with maxTOA <= 5 (11
// lags, 26 window samples), <EQ_NC, 52> for everything else (the classic 36-lag window, wide 52M windows).
static hipError_t launch_eq_detect(hipStream_t st, const TrxTables *dT, const void *samples, int fmt, const int32_t *off, const int32_t *len, int B,
                                   int tsc, float detect_thresh, float energy_thresh, int variant52m, int max_toa, bool geom52, uint8_t *flags,
                                   trx_c32 *amp, float *toa, float *toa_eq, trx_c32 *w, trx_c32 *bq, float snr_thresh, float snr_value,
                                   float *chan_off, trx_c32 *chan, const uint8_t *enable, const float *snr_in, const int32_t *dense_gate,
                                   int dense_min) {
  return eq_with_fmt(fmt, [&](auto smp) -> hipError_t {
    using SMP = decltype(smp);
    if (geom52 && variant52m && max_toa == 4 && eq_detect_generic() == 0)
      return launch_eq_detect52<SMP>(st, B, dT, samples, off, len, B, tsc, detect_thresh, energy_thresh, flags, amp, toa, toa_eq, w, bq, snr_thresh,
                                     snr_value, chan_off, chan, enable, snr_in);
    auto go = [&](auto kernel) {
      kernel<<<dim3((B + 63) / 64), dim3(64), 0, st>>>(dT, samples, off, len, B, tsc, detect_thresh, energy_thresh, variant52m, max_toa, flags, amp,
                                                       toa, toa_eq, w, bq, snr_thresh, snr_value, chan_off, chan, enable, snr_in, dense_gate,
                                                       dense_min);
    };
    if (variant52m && max_toa <= 5) go(k_eq_detect<12, 26, SMP>); else go(k_eq_detect<EQ_NC, 52, SMP>);
    return hipSuccess;
  });
}

hipError_t trx_launch_design_dfe(hipStream_t st, const trx_c32 *chan, const trx_c32 *amp, const float *snr, int B, trx_c32 *w,
                                 trx_c32 *bq, TrxProfiler *prof) {
  if (B <= 0) return hipSuccess;
  if (prof) prof->begin(TRXSIG_K_EQUALIZE, st);
  k_design_dfe<<<dim3((B + 63) / 64), dim3(64), 0, st>>>(chan, amp, snr, B, w, bq);
  if (prof) prof->end(TRXSIG_K_EQUALIZE, st);
  return hipGetLastError();
}

hipError_t trx_launch_equalize(hipStream_t st, const TrxTables *dT, const void *samples, int fmt, const int32_t *off,
                               const int32_t *len, int B, int tsc, float detect_thresh, float energy_thresh,
                               int variant52m, int max_toa, uint8_t *flags, trx_c32 *amp, float *toa, float *toa_eq,
                               trx_c32 *w, trx_c32 *bq, trx_c32 *xd, int xstride, float *soft, uint8_t *hard,
                               int nsoft, int stride, TrxProfiler *prof, bool geom52) {
  if (B <= 0) return hipSuccess;
  if (prof) prof->begin(TRXSIG_K_EQUALIZE, st);
  const hipError_t e = launch_eq_detect(st, dT, samples, fmt, off, len, B, tsc, detect_thresh, energy_thresh, variant52m, max_toa, geom52, flags, amp,
                                        toa, toa_eq, w, bq, -1.0f, 0.0f, nullptr, nullptr, nullptr, nullptr, nullptr, 0);
  if (prof) prof->end(TRXSIG_K_EQUALIZE, st);
  if (e != hipSuccess) return e;
  return trx_launch_equalize_taps(st, dT, samples, fmt, off, len, B, amp, toa_eq, flags, w, bq, xd, xstride, soft, hard, nsoft, stride, prof, nullptr);
}

// the two halves of trx_launch_equalize on their own (the Transceiver facade caches DFE taps per timeslot):
// channel estimate + designDFE only (energy gate off, explicit SNR threshold); the other half is trx_launch_equalize_taps (trxsig_eq_dfe.hip)
hipError_t trx_launch_estimate_dfe(hipStream_t st, const TrxTables *dT, const void *samples, int fmt, const int32_t *off,
                                   const int32_t *len, int B, int tsc, float detect_thresh, float snr_thresh,
                                   float snr_value, int variant52m, int max_toa, uint8_t *flags, trx_c32 *amp, float *toa,
                                   float *toa_eq, float *chan_off, trx_c32 *w, trx_c32 *bq, trx_c32 *chan, TrxProfiler *prof,
                                   const uint8_t *enable, const float *snr_in, bool geom52, int32_t *work, bool listed) {
  if (B <= 0) return hipSuccess;
  if (prof) prof->begin(TRXSIG_K_EQUALIZE, st);
  hipError_t e = hipSuccess;
  // few bursts (the Transceiver/ variant): a wave per burst -- a marked subset (listed first; `work`: B + 1 ints) or a small call
  if (!variant52m && eq_detect_generic() == 0 && ((enable && work) || (!enable && B <= kEqWaveMax))) {
    const int32_t *list = nullptr, *count = nullptr;
    if (enable) {
      if (!listed) k_eq_list<<<dim3(1), dim3(1024), 0, st>>>(enable, B, work + 1, work);
      list = work + 1; count = work;
    }
    const int waves = B < kEqWaveMax ? B : kEqWaveMax;
    const dim3 grid((waves + 3) / 4), block(256);
    eq_with_fmt(fmt, [&](auto smp) {
      k_eq_estimate_wave<decltype(smp)><<<grid, block, 0, st>>>(dT, samples, off, len, B, tsc, detect_thresh, flags, amp, toa, toa_eq, w, bq, snr_thresh,
                                                                snr_value, chan_off, chan, snr_in, list, count, eq_dense());
    });
    if (enable && B > eq_dense())                             // the marked bursts may be many (a cell in bad shape: every miss costs the slot its cache)
      e = launch_eq_detect(st, dT, samples, fmt, off, len, B, tsc, detect_thresh, -1.0f, variant52m, max_toa, false, flags, amp, toa, toa_eq, w, bq,
                           snr_thresh, snr_value, chan_off, chan, enable, snr_in, count, eq_dense());
  } else
    e = launch_eq_detect(st, dT, samples, fmt, off, len, B, tsc, detect_thresh, -1.0f, variant52m, max_toa, geom52, flags, amp, toa, toa_eq, w, bq,
                         snr_thresh, snr_value, chan_off, chan, enable, snr_in, nullptr, 0);
  if (prof) prof->end(TRXSIG_K_EQUALIZE, st);
  return e != hipSuccess ? e : hipGetLastError();
}
