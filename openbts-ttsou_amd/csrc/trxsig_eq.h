// trxsig_eq.h -- what the two halves of the equaliser path share (trxsig_eq_est.hip, trxsig_eq_dfe.hip).
// ---------------------------------------------------------------------------------------------
// Equaliser path (sps = 1; "Assumes symbol-rate sampling", sigProcLib.cpp:1342): the TSC leg of
// pullRadioVector with a channel estimate and a decision-feedback equaliser
// (Transceiver.cpp:298-349, 391-396; Transceiver52M/Transceiver.cpp for the windowed variant).
//
//   trxsig_eq_est.hip  energyDetect, analyzeTrafficBurst(requestChannel) -- correlation (full 36-lag window, or the 52M
//                      CUSTOM span of 2*maxTOA+1 lags), peakDetect, valley test, delayVector on the correlation, 6-tap
//                      channel pick -- then scaleVector(chan, 1/amp), SNR and designDFE(chan, SNR, 7).  All of it tiny
//                      and strictly sequential per burst: a lane per burst (k_eq_detect, k_eq_detect52), or a wave per
//                      burst where the bursts are few (k_eq_estimate_wave).
//   trxsig_eq_dfe.hip  delayVector(burst/amp, -(TOA - chanOffset)), the 7-tap feed-forward FIR, the 156-step
//                      decision-feedback recursion of equalizeBurst (:1352-1384) and the slicer: one kernel
//                      (k_eq_dfe4) or two through a scratch row per burst (k_eq_delay + k_eq_dfe2).
// ---------------------------------------------------------------------------------------------
#pragma once
#include "trxsig_dev.h"

#define EQ_NC 36            /* max correlation lags kept per burst */

namespace {

// f(SmpF16{}) or f(SmpC32{}): the kernels are instantiated per sample storage (TRXSIG_SAMPLES_*), the launchers pick at run time
template <typename F>
auto eq_with_fmt(int fmt, F &&f) {
  return fmt == TRXSIG_SAMPLES_F16 ? f(SmpF16{}) : f(SmpC32{});
}

// The burst's row of xd was written by k_eq_delay only if that kernel accepted the burst (k_demod's gate: DETECT flag,
// 92..157 samples, |TOA| <= 4096 and not NaN).  The equaliser must apply the same gate, or it would equalise whatever an
// earlier call left in the row and hand back plausible-looking soft bits.
__device__ __forceinline__ bool eq_enabled(uint8_t fl, int N, float toa_eq) {
  return (fl & TRXSIG_F_DETECT) && N >= 92 && N <= 157 && (fabsf(toa_eq) <= 4096.0f);
}

}  // namespace
