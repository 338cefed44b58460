// trxsig_air.cpp -- the air's host side (include/trxsig_air.h): argument checks and one launch per call on the context's stream
// (k_air_cells, k_air_stream, k_air_fade).  The noise is counter-based and needs no memory; the fading generator's profile (path
// amplitudes, tap weights, column rotations: all made here, in double or in integers) is one small device block, allocated with
// the first profile and written in stream order through a pinned ring.
#include <hip/hip_runtime_api.h>

#include <cmath>
#include <cstddef>
#include <cstring>
#include <new>

#include "trxsig_air.h"
#include "trxsig_ctx.h"
#include "trxsig_plan.h"

struct trxsig_air {
  trxsig_ctx *c = nullptr;
  int max_taps = 0;
  // the fading generator: the profile as given, the columns' carrier offsets, and the image of both on the device
  bool profiled = false;
  int P = 0, S = 0, n_taps = 0;
  int32_t delay_ns[TRX_FADE_MAX_PATHS] = {};
  int n_cols = TRX_FADE_MAX_COLS;
  int32_t col_khz[TRX_FADE_MAX_COLS];
  TrxAirFadeTab img{};
  TrxAirFadeTab *d_tab = nullptr;
  TrxPinRing up;
};

namespace {
int fail(trxsig_air *a, const char *what) { return trx_ctx_fail(a ? a->c : nullptr, TRXSIG_EINVAL, what, hipSuccess); }

constexpr int kFadeMaxDelayNs = 1000000, kFadeMaxKhz = 10000000, kFadeMaxLinks = 1 << 30;

// -f_kHz tau_ns 1e-6 turn in 2^-32 turn: whole turns dropped first (exact), then one rounding, halves up
uint32_t fade_rot(int32_t khz, int32_t ns) {
  long long r = (-(long long)khz * ns) % 1000000;
  if (r < 0) r += 1000000;
  return (uint32_t)(((r << 32) + 500000) / 1000000);
}

// the profile's image with the rotations of the columns as they stand, up in stream order.  The caller holds the TrxDeviceGuard.
int fade_upload(trxsig_air *a) {
  trxsig_ctx *c = a->c;
  for (int k = 0; k < a->n_cols; k++)
    for (int p = 0; p < TRX_FADE_MAX_PATHS; p++) a->img.rot[k][p] = p < a->P ? fade_rot(a->col_khz[k], a->delay_ns[p]) : 0u;
  if (!a->d_tab) {
    void *d = nullptr;
    if (hipMalloc(&d, sizeof(TrxAirFadeTab)) != hipSuccess) return trx_ctx_fail(c, TRXSIG_ENOMEM, "trxsig_air_fade_profile: device allocation", hipSuccess);
    a->d_tab = (TrxAirFadeTab *)d;
  }
  const size_t bytes = offsetof(TrxAirFadeTab, rot) + sizeof(a->img.rot[0]) * (size_t)a->n_cols;
  void *blk = nullptr;
  int slot = 0;
  TRX_HIPCHK(c, a->up.take(bytes, &blk, &slot));
  std::memcpy(blk, &a->img, bytes);
  TRX_HIPCHK(c, a->up.upload(slot, a->d_tab, bytes, (hipStream_t)trxsig_get_stream(c)));
  return TRXSIG_OK;
}

TrxAirFade fade_args(const trxsig_air *a, uint64_t seed, int n_links, const uint32_t *d_doppler) {
  TrxAirFade p{};
  p.tab = a->d_tab; p.P = a->P; p.S = a->S; p.n_taps = a->n_taps;
  p.inv = (65536u + (unsigned)a->S) / (unsigned)(a->S + 1);
  p.doppler = d_doppler; p.n_links = n_links;
  p.key0 = (unsigned)(seed & 0xffffffffu); p.key1 = (unsigned)(seed >> 32);
  return p;
}
}  // namespace

int trxsig_air_create(trxsig_air **out, trxsig_ctx *c, int max_taps) {
  if (!out || !c) return TRXSIG_EINVAL;
  *out = nullptr;
  if (max_taps < 1 || max_taps > TRXSIG_AIR_MAX_TAPS)
    return trx_ctx_fail(c, TRXSIG_EINVAL, "trxsig_air_create: max_taps in 1..32", hipSuccess);
  trxsig_air *a = new (std::nothrow) trxsig_air;
  if (!a) return TRXSIG_ENOMEM;
  a->c = c; a->max_taps = max_taps;
  for (int k = 0; k < TRX_FADE_MAX_COLS; k++) a->col_khz[k] = 200 * k;
  trx_ctx_retain(c);
  *out = a;
  return TRXSIG_OK;
}

void trxsig_air_destroy(trxsig_air *a) {
  if (!a) return;
  {
    TrxDeviceGuard g(trxsig_device(a->c));
    a->up.release();                                         // (waits for the uploads still on their way)
  }
  trx_object_destroy(a->c, { a->d_tab });
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

int trxsig_air_fade_profile(trxsig_air *a, int n_paths, const int32_t *h_delay_ns, const float *h_power, const float *h_los_share,
                            const int32_t *h_los_cos_q23, int n_sinusoids, int n_taps, int centre) {
  if (!a) return TRXSIG_EINVAL;
  if (!h_delay_ns || !h_power) return fail(a, "trxsig_air_fade_profile: NULL");
  if (n_paths < 1 || n_paths > TRX_FADE_MAX_PATHS || n_sinusoids < 1 || n_sinusoids > TRX_FADE_MAX_SIN || n_taps < 1 ||
      n_taps > a->max_taps || centre < 0 || centre > 8)
    return fail(a, "trxsig_air_fade_profile: bad argument (n_paths in 1..12, n_sinusoids in 1..32, n_taps in 1..max_taps, centre in 0..8)");
  for (int p = 0; p < n_paths; p++) {
    const float los = h_los_share ? h_los_share[p] : 0.0f;
    const int32_t lc = h_los_cos_q23 ? h_los_cos_q23[p] : 0;
    if (h_delay_ns[p] < 0 || h_delay_ns[p] > kFadeMaxDelayNs || !(h_power[p] >= 0.0f) || !std::isfinite(h_power[p]) || !(los >= 0.0f) ||
        !(los <= 1.0f) || lc < -(1 << 23) || lc > (1 << 23))
      return fail(a, "trxsig_air_fade_profile: bad path (delay in 0..10^6 ns, finite power >= 0, share in [0, 1], |cosine| <= 2^23)");
  }
  const int sps = trxsig_sps(a->c);
  const double pi = 3.14159265358979323846;
  TrxAirFadeTab &m = a->img;
  std::memset(&m, 0, offsetof(TrxAirFadeTab, rot));
  for (int p = 0; p < n_paths; p++) {
    const double pw = h_power[p], los = h_los_share ? h_los_share[p] : 0.0;
    m.a[p] = (float)std::sqrt(pw * (1.0 - los) / n_sinusoids);
    m.b[p] = (float)std::sqrt(pw * los);
    m.los_c[p] = h_los_cos_q23 ? h_los_cos_q23[p] : 0;
    a->delay_ns[p] = h_delay_ns[p];
    const long long at = 48000LL * centre + 13LL * sps * h_delay_ns[p];   // where the path arrives, in 1 / 48000 sample
    for (int j = 0; j < n_taps; j++) {
      const long long num = 48000LL * j - at;
      double w = 0.0;
      if (num % 48000 == 0) w = num == 0 ? 1.0 : 0.0;         // a whole sample away: sinc's zeros, exactly
      else if (num > -4 * 48000LL && num < 4 * 48000LL) {
        const double x = (double)num / 48000.0;
        w = std::sin(pi * x) / (pi * x) * (0.5 + 0.5 * std::cos(pi * x / 4.0));
      }
      m.w[p][j] = (float)w;
    }
  }
  a->P = n_paths; a->S = n_sinusoids; a->n_taps = n_taps; a->profiled = true;
  TrxDeviceGuard g(trxsig_device(a->c));
  return fade_upload(a);
}

int trxsig_air_fade_columns(trxsig_air *a, int n_arfcn, const int32_t *h_col_khz) {
  if (!a) return TRXSIG_EINVAL;
  if (!h_col_khz) return fail(a, "trxsig_air_fade_columns: NULL");
  if (n_arfcn < 1 || n_arfcn > TRX_FADE_MAX_COLS) return fail(a, "trxsig_air_fade_columns: n_arfcn in 1..1024");
  for (int k = 0; k < n_arfcn; k++)
    if (h_col_khz[k] < -kFadeMaxKhz || h_col_khz[k] > kFadeMaxKhz) return fail(a, "trxsig_air_fade_columns: an offset beyond +-10^7 kHz");
  std::memcpy(a->col_khz, h_col_khz, sizeof(int32_t) * (size_t)n_arfcn);
  a->n_cols = n_arfcn;
  if (!a->profiled) return TRXSIG_OK;                        // the rotations go up with the profile
  TrxDeviceGuard g(trxsig_device(a->c));
  return fade_upload(a);
}

int trxsig_air_fade(trxsig_air *a, int fn, int n_arfcn, int n_frames, uint64_t seed, const int32_t *d_link, int n_links,
                    const uint32_t *d_doppler, trxsig_c32 *d_taps) {
  if (!a) return TRXSIG_EINVAL;
  if (!d_doppler || !d_taps) return fail(a, "trxsig_air_fade: NULL");
  if (!a->profiled) return fail(a, "trxsig_air_fade: no profile set");
  if (n_arfcn < 1 || n_arfcn > a->n_cols || n_frames < 1 || n_frames > (1 << 24) || fn < 0 || fn >= kTrxHyperframe || n_links < 1 ||
      n_links > kFadeMaxLinks)
    return fail(a, "trxsig_air_fade: bad argument (n_arfcn in 1..the columns set, n_frames in 1..2^24, fn in [0, 2715648), n_links in 1..2^30)");
  trxsig_ctx *c = a->c;
  TrxAirFade p = fade_args(a, seed, n_links, d_doppler);
  p.link = d_link; p.taps = (trx_c32 *)d_taps;
  p.vec = (a->n_taps & 1) == 0 && ((uintptr_t)d_taps & 15) == 0;
  p.rows = 8LL * n_frames; p.n_arfcn = n_arfcn; p.row0 = 8u * (unsigned)fn;
  TrxDeviceGuard g(trxsig_device(c));
  TRX_HIPCHK(c, trx_launch_air_fade((hipStream_t)trxsig_get_stream(c), p));
  return TRXSIG_OK;
}

int trxsig_air_fade_params(trxsig_air *a, uint64_t seed, int n_links, const uint32_t *d_doppler, uint32_t *d_phase, int32_t *d_step) {
  if (!a) return TRXSIG_EINVAL;
  if (!d_doppler || !d_phase || !d_step) return fail(a, "trxsig_air_fade_params: NULL");
  if (!a->profiled) return fail(a, "trxsig_air_fade_params: no profile set");
  if (n_links < 1 || n_links > (1 << 24)) return fail(a, "trxsig_air_fade_params: n_links in 1..2^24");
  trxsig_ctx *c = a->c;
  TrxAirFade p = fade_args(a, seed, n_links, d_doppler);
  p.phase = d_phase; p.step = d_step;
  TrxDeviceGuard g(trxsig_device(c));
  TRX_HIPCHK(c, trx_launch_air_fade_params((hipStream_t)trxsig_get_stream(c), p));
  return TRXSIG_OK;
}
