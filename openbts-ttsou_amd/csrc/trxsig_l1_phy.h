// trxsig_l1_phy.h -- internal: the RSSI and timing error a logical channel's decoder records for a burst it accepted, shared by
// the demultiplexers of both sides: k_l1rx_demux applies it itself, the handsets' k_l1msrx_demux records the row and
// k_l1rx_demux_phy applies it (both kernels in trxsig_l1rx.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "trxsig_launch.h"

// the burst's RSSI and timing as the decoder records them: trxsig_trxgroup_collect's integers (Transceiver.cpp:400-402) through
// the datagram (one signed byte of RSSI, negated by TRXManager; timing as int16, / 256.0F, into an int parameter)
__device__ inline void burst_phy(const trx_c32 *amp, const float *toa, int r, int sps, int32_t *rssi, int32_t *timing) {
  const trx_c32 a = amp[r];
  const float n2 = __fadd_rn(__fmul_rn(a.i, a.i), __fmul_rn(a.r, a.r));
  const float absA = (float)sqrt((double)n2);
  const double x = 9450.0 / (double)absA;
  double l = log10(x);
  // where x is an exact power of ten the host's log10 returns the integer exactly and floor() sits on it: pin the device's
  // value there too, so the floor boundary is decided the same way (tests/test_gpu_l1rx.py, test_rssi_at_the_floor_boundaries)
  const double ri = rint(l);
  if (ri >= 0.0 && ri <= 22.0 && fabs(l - ri) < 1e-9) {
    double p = 1.0;
    for (int i = 0; i < (int)ri; i++) p *= 10.0;              // exact up to 1e22
    if (p == x) l = ri;
  }
  const int db = (int)floor(20.0 * l);
  const int t = (int)round((double)toa[r] * 256.0 / (double)sps);
  *rssi = -(int)(signed char)db;
  *timing = (int)(int16_t)t / 256;
}
