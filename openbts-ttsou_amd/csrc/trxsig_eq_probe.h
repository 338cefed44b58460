// trxsig_eq_probe.h -- clock64() stamps inside the equaliser's kernels, for the probe builds only (make probe_eq, make probe_dfe4).
// Without TRX_EQ_PROBE / TRX_D4_PROBE every method is empty (barrier() is the bare __syncthreads()): the product's kernels carry nothing.
#pragma once
#include "trxsig_dev.h"

namespace {

struct EqProbe {
#ifdef TRX_EQ_PROBE
  // k_eq_detect / k_eq_detect52 (tools/eq_probe.py).  TRX_EQ_PROBE=1: stamp() marks the phases; =2: stamp2() marks the staging block in
  // detail instead.  pt[0] is the kernel's start; report() hands burst b's slot (b & 7) back through toa_out: slots 1..5 the stamps
  // relative to the start, 6 and 7 the absolute start and end (24 bits): the launch's spread over time.
  long long pt[8] = {0};
  int n = 1;
  __device__ __forceinline__ EqProbe() { pt[0] = clock64(); }
  __device__ __forceinline__ void stamp() { if (TRX_EQ_PROBE != 2) pt[n++] = clock64(); }
  __device__ __forceinline__ void stamp2() { if (TRX_EQ_PROBE == 2) pt[n++] = clock64(); }
  __device__ __forceinline__ void report(int b, float *toa_out) {
    pt[5] = clock64();
    long long v = 0;
    for (int k = 1; k < 8; k++) if ((b & 7) == k) v = pt[k] - pt[0];
    if ((b & 7) == 6) v = pt[0] & 0xFFFFFF;
    if ((b & 7) == 7) v = pt[5] & 0xFFFFFF;
    toa_out[b] = (float)v;
  }
#else
  __device__ __forceinline__ void stamp() {}
  __device__ __forceinline__ void stamp2() {}
  __device__ __forceinline__ void report(int, float *) {}
#endif
#ifdef TRX_D4_PROBE
  // k_eq_dfe4 (tools/dfe4_probe.py): barrier() splits a wave's cycles into those between the workgroup's barriers (work) and those at
  // them (wait); report() writes {work, wait, total, role} over the first soft bits of a row -- this build's outputs are NOT results.
  long long t0 = clock64(), t = t0, work = 0, wait = 0;
  __device__ __forceinline__ void barrier() {
    const long long a = clock64();
    work += a - t;
    __syncthreads();
    t = clock64();
    wait += t - a;
  }
  __device__ __forceinline__ void report(float *o, int role) {
    o[0] = (float)work; o[1] = (float)wait; o[2] = (float)(clock64() - t0); o[3] = (float)role;
  }
#else
  __device__ __forceinline__ void barrier() { __syncthreads(); }
  __device__ __forceinline__ void report(float *, int) {}
#endif
};

}  // namespace
