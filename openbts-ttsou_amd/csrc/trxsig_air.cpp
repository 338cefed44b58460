// trxsig_air.cpp -- the air's host side (include/trxsig_air.h): argument checks and one launch per call on the context's stream
// (k_air_cells, k_air_stream).  The object holds no device memory: the noise is counter-based and the channel is the caller's.
#include <hip/hip_runtime_api.h>

#include <new>

#include "trxsig_air.h"
#include "trxsig_ctx.h"
#include "trxsig_plan.h"

struct trxsig_air {
  trxsig_ctx *c = nullptr;
  int max_taps = 0;
};

namespace {
int fail(trxsig_air *a, const char *what) { return trx_ctx_fail(a ? a->c : nullptr, TRXSIG_EINVAL, what, hipSuccess); }
}  // namespace

int trxsig_air_create(trxsig_air **out, trxsig_ctx *c, int max_taps) {
  if (!out || !c) return TRXSIG_EINVAL;
  *out = nullptr;
  if (max_taps < 1 || max_taps > TRXSIG_AIR_MAX_TAPS)
    return trx_ctx_fail(c, TRXSIG_EINVAL, "trxsig_air_create: max_taps in 1..32", hipSuccess);
  trxsig_air *a = new (std::nothrow) trxsig_air;
  if (!a) return TRXSIG_ENOMEM;
  a->c = c; a->max_taps = max_taps;
  trx_ctx_retain(c);
  *out = a;
  return TRXSIG_OK;
}

void trxsig_air_destroy(trxsig_air *a) {
  if (!a) return;
  trx_object_destroy(a->c, {});
  delete a;
}

int trxsig_air_cells(trxsig_air *a, int fn, int n_arfcn, int n_frames, uint64_t seed, const trxsig_c32 *d_in, int64_t in_slot,
                     int64_t in_arfcn, const trxsig_air_cell_params *pr, trxsig_c32 *d_out, int64_t out_slot, int64_t out_arfcn,
                     int accumulate) {
  if (!a) return TRXSIG_EINVAL;
  if (!d_in || !d_out || !pr) return fail(a, "trxsig_air_cells: NULL");
  if (n_arfcn < 1 || n_arfcn > 65535 || n_frames < 1 || n_frames > (1 << 24) || fn < 0 || fn >= kTrxHyperframe)
    return fail(a, "trxsig_air_cells: bad argument (n_arfcn in 1..65535, n_frames in 1..2^24, fn in [0, 2715648))");
  if (pr->d_taps && (pr->n_taps < 1 || pr->n_taps > a->max_taps)) return fail(a, "trxsig_air_cells: n_taps outside 1..max_taps");
  trxsig_ctx *c = a->c;
  const int sps = trxsig_sps(c);
  const long long T = 8LL * n_frames, A = n_arfcn, cell = 157LL * sps;
  long long in_n = 0, out_n = 0;
  if (!strides_ok(T, A, cell, in_slot, in_arfcn) || !strides_ok(T, A, cell, out_slot, out_arfcn) ||
      !extent(T, A, cell, in_slot, in_arfcn, &in_n) || !extent(T, A, cell, out_slot, out_arfcn, &out_n))
    return fail(a, "trxsig_air_cells: the strides let cells overlap");
  const bool same = d_out == d_in && out_slot == in_slot && out_arfcn == in_arfcn;
  if (!same && overlap(d_in, in_n, d_out, out_n)) return fail(a, "trxsig_air_cells: out overlaps in without being identical");
  TrxAirCells p{};
  p.in = (const trx_c32 *)d_in; p.in_slot = in_slot; p.in_arfcn = in_arfcn;
  p.out = (trx_c32 *)d_out; p.out_slot = out_slot; p.out_arfcn = out_arfcn;
  p.taps = (const trx_c32 *)pr->d_taps; p.n_taps = pr->d_taps ? pr->n_taps : 0;
  p.step = pr->d_step; p.phase = pr->d_phase; p.sigma = pr->d_sigma;
  p.rows = T; p.n_arfcn = n_arfcn; p.row0 = 8u * (unsigned)fn;
  p.key0 = (unsigned)(seed & 0xffffffffu); p.key1 = (unsigned)(seed >> 32);
  p.accumulate = accumulate != 0;
  TrxDeviceGuard g(trxsig_device(c));
  TRX_HIPCHK(c, trx_launch_air_cells((hipStream_t)trxsig_get_stream(c), sps, (const TrxTables *)trxsig_tables_device(c), p));
  return TRXSIG_OK;
}

int trxsig_air_stream(trxsig_air *a, int n_cells, uint64_t seed, const trxsig_c32 *d_in, int64_t slot_stride, int64_t arfcn_stride,
                      int n_handsets, const trxsig_air_stream_params *pr, int len, trxsig_c32 *d_out, int64_t out_stride) {
  if (!a) return TRXSIG_EINVAL;
  if (!d_in || !d_out || !pr || !pr->d_arfcn || !pr->d_cut) return fail(a, "trxsig_air_stream: NULL");
  trxsig_ctx *c = a->c;
  const int sps = trxsig_sps(c);
  if (n_cells < 1 || (long long)n_cells * 157 * sps > 0x7fffffffLL || pr->n_arfcn < 1 || pr->n_arfcn > 65535 || n_handsets < 1 ||
      n_handsets > 65535 || len < 1 || out_stride < len)
    return fail(a, "trxsig_air_stream: bad argument (n_cells, n_arfcn, n_handsets in 1..65535, len > 0, out_stride >= len)");
  const long long T = n_cells, A = pr->n_arfcn, cell = 157LL * sps;
  long long in_n = 0, out_n = 0;
  if (!strides_ok(T, A, cell, slot_stride, arfcn_stride) || !extent(T, A, cell, slot_stride, arfcn_stride, &in_n))
    return fail(a, "trxsig_air_stream: the strides let cells overlap");
  if (!extent(n_handsets, 1, len, out_stride, 0, &out_n) || overlap(d_in, in_n, d_out, out_n))
    return fail(a, "trxsig_air_stream: out overlaps in");
  TrxAirStream p{};
  p.in = (const trx_c32 *)d_in; p.in_slot = slot_stride; p.in_arfcn = arfcn_stride; p.n_arfcn = pr->n_arfcn; p.n_cells = n_cells;
  p.arfcn = pr->d_arfcn; p.cut = (const long long *)pr->d_cut; p.delay = pr->d_delay; p.step = pr->d_step; p.phase = pr->d_phase;
  p.gain = (const trx_c32 *)pr->d_gain; p.sigma = pr->d_sigma; p.n0 = pr->d_n0;
  p.n_handsets = n_handsets; p.len = len; p.out = (trx_c32 *)d_out; p.out_stride = out_stride;
  p.key0 = (unsigned)(seed & 0xffffffffu); p.key1 = (unsigned)(seed >> 32);
  TrxDeviceGuard g(trxsig_device(c));
  TRX_HIPCHK(c, trx_launch_air_stream((hipStream_t)trxsig_get_stream(c), sps, (const TrxTables *)trxsig_tables_device(c), p));
  return TRXSIG_OK;
}
