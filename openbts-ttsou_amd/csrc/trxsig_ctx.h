// trxsig_ctx.h -- internal: what the other host translation units of the library (trxsig_frontend.cpp, trxsig_trxgroup.cpp,
// trxsig_transceiver.cpp) may ask of a context (trxsig_api.cpp owns struct trxsig_ctx).
#pragma once
#include <cassert>
#include <cstring>
#include <initializer_list>
#include <string>
#include <vector>

#include "trxsig.h"
#include "trxsig_launch.h"

int trx_ctx_fail(trxsig_ctx *c, int code, const char *what, hipError_t e);

// (TRX_INTERNAL: a class of the library's own that adds no exported symbol)
#define TRX_INTERNAL __attribute__((visibility("hidden")))

// the context's device is current for the call; the caller's comes back after it
struct TRX_INTERNAL TrxDeviceGuard {
  int prev = -1;
  explicit TrxDeviceGuard(int dev) { if (hipGetDevice(&prev) != hipSuccess) prev = -1; if (prev != dev) (void)hipSetDevice(dev); }
  ~TrxDeviceGuard() { if (prev >= 0) (void)hipSetDevice(prev); }
};

// a failing HIP call returns TRXSIG_EHIP from the enclosing function, with the call's text as the context's last error
#define TRX_HIPCHK(c, call)                                                   \
  do {                                                                        \
    hipError_t e_ = (call);                                                   \
    if (e_ != hipSuccess) return trx_ctx_fail((c), TRXSIG_EHIP, #call, e_);   \
  } while (0)

// One *_host call's round trip through the context's device staging area:
//   TrxHostCall hc(c);
//   const auto x = hc.in(h_x, n);      n elements uploaded from h_x (h_x == nullptr: the region is only reserved)
//   const auto k = hc.val(delay);      one scalar, copied here at once: nothing on the caller's stack is read later
//   const auto z = hc.inout(h_src, h_dst, n);   uploaded from h_src, downloaded to h_dst (the in-place forms: the same pointer)
//   const auto y = hc.out(h_y, n);     downloaded to h_y (h_y == nullptr: a device region only); out(h_y, n, m) reserves m >= n
//   const auto o = hc.zeroed_out(h_o, n);       an out() that is cleared on the device first
//   int rc = hc.stage();               sizes the scratch, uploads
//   if (rc == TRXSIG_OK) rc = trxsig_..._batch(c, hc.dev(x), ...);
//   return hc.finish(rc);              downloads if rc is TRXSIG_OK, waits for the stream, returns rc (or the copy's error)
// The regions are laid out inputs, in/outs, outputs (256-byte aligned), so the upload and the download are one range each.  A
// call that fits in kPinnedMax goes through the context's pinned mirror of the staging area, one DMA each way (115 -> 38 us for
// the one-burst detect + demodulate, tools/host_path_bench.py); a larger one copies each region straight from and to the caller's
// buffers.  Once a copy is queued, every way out waits for the stream -- the destructor does it for the early returns -- so no
// copy outlives the call.
class TRX_INTERNAL TrxHostCall {
 public:
  static constexpr size_t kPinnedMax = 256 * 1024;
  template <class T> struct Reg { int i; };
  explicit TrxHostCall(trxsig_ctx *c);
  ~TrxHostCall();
  TrxHostCall(const TrxHostCall &) = delete;
  TrxHostCall &operator=(const TrxHostCall &) = delete;

  template <class T> Reg<T> in(const T *h, size_t n) { return add<T>(kIn, h, nullptr, n, n); }
  template <class T> Reg<T> val(const T &v) {
    static_assert(sizeof(T) <= sizeof(Region::v), "val() takes a scalar");
    const Reg<T> r = add<T>(kIn, nullptr, nullptr, 1, 1);
    std::memcpy(regs_[r.i].v, &v, sizeof(T));
    regs_[r.i].inline_val = true;
    return r;
  }
  template <class T> Reg<T> inout(const T *src, T *dst, size_t n) { return add<T>(kInOut, src, dst, n, n); }
  template <class T> Reg<T> out(T *h, size_t n, size_t reserve = 0) { return add<T>(kOut, nullptr, h, n, reserve > n ? reserve : n); }
  template <class T> Reg<T> zeroed_out(T *h, size_t n) {
    const Reg<T> r = out(h, n);
    regs_[r.i].zero = true;
    return r;
  }
  int stage();
  template <class T> T *dev(Reg<T> r) const { return (T *)(d_ + regs_[r.i].off); }
  int finish(int rc);

 private:
  enum Kind { kIn, kInOut, kOut };
  struct Region {
    Kind kind;
    const void *src;
    void *dst;
    size_t bytes, dev_bytes, off;
    bool inline_val, zero;
    alignas(8) unsigned char v[8];
  };
  template <class T> Reg<T> add(Kind kind, const void *src, void *dst, size_t n, size_t dev_n) {
    regs_.push_back(Region{kind, src, dst, sizeof(T) * n, sizeof(T) * dev_n, 0, false, false, {}});
    return Reg<T>{(int)regs_.size() - 1};
  }
  trxsig_ctx *c_;
  TrxDeviceGuard guard_;
  std::vector<Region> regs_;
  char *d_ = nullptr;                  // the staging area
  char *m_ = nullptr;                  // its pinned mirror (a call that fits in kPinnedMax), else nullptr
  size_t dl_lo_ = 0, dl_hi_ = 0;       // the download range
  bool queued_ = false;                // a copy is queued that nobody has waited for yet
};

// Small tables a call makes on the host and a kernel of the same call reads: pinned staging blocks taken in turn, each free again
// when the upload that read it has run.  (A PAGEABLE source makes hipMemcpyAsync wait until the stream has drained -- the host then
// cannot run ahead of the device at all: ~0.5 ms a call with the device busy, profiles/r05_group_tx_bench.txt.)
struct TrxPinRing {
  static constexpr int kSlots = 4;
  void *p[kSlots] = {nullptr, nullptr, nullptr, nullptr};
  size_t cap[kSlots] = {0, 0, 0, 0};
  hipEvent_t ev[kSlots] = {nullptr, nullptr, nullptr, nullptr};
  bool armed[kSlots] = {false, false, false, false};
  unsigned turn = 0;
  // the next block, at least `bytes` long (waits for the upload that used it four calls ago, if that has not run yet)
  hipError_t take(size_t bytes, void **out, int *slot) {
    const int k = (int)(turn++ % kSlots);
    hipError_t e = hipSuccess;
    if (!ev[k] && (e = hipEventCreateWithFlags(&ev[k], hipEventDisableTiming)) != hipSuccess) return e;
    if (armed[k]) { if ((e = hipEventSynchronize(ev[k])) != hipSuccess) return e; armed[k] = false; }
    if (bytes > cap[k]) {
      void *q = nullptr;
      const size_t want = bytes + bytes / 4 + 256;
      if ((e = hipHostMalloc(&q, want, hipHostMallocDefault)) != hipSuccess) return e;
      if (p[k]) (void)hipHostFree(p[k]);
      p[k] = q; cap[k] = want;
    }
    *out = p[k]; *slot = k;
    return hipSuccess;
  }
  // hipMemcpyAsync(dst, block, bytes) on st, and the block's event behind it
  hipError_t upload(int slot, void *dst, size_t bytes, hipStream_t st) {
    hipError_t e = hipMemcpyAsync(dst, p[slot], bytes, hipMemcpyHostToDevice, st);
    if (e != hipSuccess) return e;
    if ((e = hipEventRecord(ev[slot], st)) != hipSuccess) return e;
    armed[slot] = true;
    return hipSuccess;
  }
  void release() {
    for (int k = 0; k < kSlots; k++) {
      if (ev[k]) { if (armed[k]) (void)hipEventSynchronize(ev[k]); (void)hipEventDestroy(ev[k]); ev[k] = nullptr; }
      if (p[k]) { (void)hipHostFree(p[k]); p[k] = nullptr; }
      cap[k] = 0; armed[k] = false;
    }
  }
};
TrxProfiler *trx_ctx_profiler(trxsig_ctx *c);
// the context's TCH filler c[456] on the device (allocated, all zero, on first use; trxsig_fec_tch_set_filler), or null
extern "C" const uint8_t *trx_ctx_tch_filler(trxsig_ctx *c);   // defined in trxsig_api.cpp's C block
// the normal-burst leg on bursts computed from the raw int16 stream (trxsig_rxfe_push_detect_demod_normal)
// (on != nullptr: launched on that stream instead of the context's; the caller orders it against the context's stream)
int trx_ctx_rx_normal(trxsig_ctx *c, const TrxRxGen &gen, int B, int tsc, float detect_thresh, float energy_thresh, uint8_t *d_flags,
                      trxsig_c32 *d_amp, float *d_toa, float *d_avgpwr, float *d_soft, uint8_t *d_hard, int nsoft, int soft_stride,
                      hipStream_t on = nullptr);
// ... detectRACHBurst (d_len[b] = the burst's length as the front end cuts it) and demodulateBurst with caller-supplied
// amplitude / TOA for the bursts whose d_enable[b] != 0, on such bursts
// (own_records != 0: the detect -> peak records go to a scratch of the call's own, so that it may run beside trx_ctx_rx_normal)
int trx_ctx_rx_rach(trxsig_ctx *c, const TrxRxGen &gen, const int32_t *d_len, int B, float detect_thresh, float energy_thresh,
                    uint8_t *d_flags, trxsig_c32 *d_amp, float *d_toa, float *d_avgpwr, int own_records = 0);
int trx_ctx_rx_demod(trxsig_ctx *c, const TrxRxGen &gen, int B, const trxsig_c32 *d_amp, const float *d_toa, const uint8_t *d_enable,
                     int need_mask, float *d_soft, int nsoft, int soft_stride);
int trx_ctx_demod_masked(trxsig_ctx *c, const trxsig_c32 *d_samples, const int32_t *d_offset, const int32_t *d_length, int B,
                         const trxsig_c32 *d_amp, const float *d_toa, const uint8_t *d_enable, int need_mask, float *d_soft, int nsoft,
                         int soft_stride);
// The six equaliser kinds' one checked path from the C ABI to the launch: kind's row of the table in trxsig_api.cpp says whether
// the second antenna, tsc (packed into a.tsc_bits here) and a.loading are checked, which entry point's name the refusal carries
// and which launcher runs.  a.need_mask spells the enable test out as trx_ctx_demod_masked's does (the group's TRXSIG_TSCLEG_MLSE
// and TRXSIG_RACHLEG_MLSE, trxsig_trxgroup_combine_div / _irc: a launch per TSC class)
enum TrxMlseKind { TRX_MLSE_NORMAL, TRX_MLSE_ACCESS, TRX_MLSE_SCH, TRX_MLSE_DIV, TRX_MLSE_IRC };
int trx_ctx_mlse(trxsig_ctx *c, TrxMlseKind kind, int tsc, const TrxMlseArgs &a);
unsigned trx_tsc_bits(int tsc);                            // bit k = bit k of training sequence tsc (0..7)
// the receive front end's side of a fused push (trxsig_frontend.cpp): which bursts this push completes and how the kernels
// find their samples (begin), and the window / clock bookkeeping once the kernels are enqueued (end)
struct trxsig_rxfe;
struct TrxRxfePush { TrxRxGen gen; int nb, tn0, n_streams; };
int trx_rxfe_fused_begin(trxsig_rxfe *fe, const int16_t *d_iq, int n_chunks, TrxRxfePush *out);
int trx_rxfe_fused_end(trxsig_rxfe *fe, const int16_t *d_iq, int n_chunks, const TrxRxfePush &p);
// an object that lives on a context keeps it alive: trxsig_destroy on a context with such objects takes effect when the last is gone
void trx_ctx_retain(trxsig_ctx *c);
void trx_ctx_release(trxsig_ctx *c);
struct trxsig_txbe;
trxsig_ctx *trx_txbe_context(const trxsig_txbe *be);         // the context a transmit back end was created on (trxsig_frontend.cpp)
trxsig_ctx *trx_rxfe_ctx(trxsig_rxfe *fe);
int trx_rxfe_rate_factor(const trxsig_rxfe *fe);            // 0: a narrowband front end; else the channeliser's rate factor
int trx_rxfe_streams(const trxsig_rxfe *fe);
int trx_rxfe_next_tn(const trxsig_rxfe *fe);
// Transceiver group (trxsig_trxgroup.cpp), equalising TSC leg (sps = 1):
//   estimate: analyzeTrafficBurst(requestChannel) + scaleVector(chan, 1/amp) + designDFE(chan, d_snr[b], 7) for the bursts with
//     d_enable[b] != 0 only (Transceiver.cpp:341-349); nothing is written for the others.  Detection threshold 3.0 (:331).
//   equalize: scaleVector(burst, 1/amp) + equalizeBurst(burst, d_toa_eq[b], w, b) (:391-396) for the bursts whose d_gate has
//     TRXSIG_F_DETECT, burst b with the taps at entry d_tap_ix[b] of the tap table.
int trx_ctx_group_estimate(trxsig_ctx *c, const trxsig_c32 *d_samples, const int32_t *d_offset, const int32_t *d_length, int B, int tsc,
                           const uint8_t *d_enable, const float *d_snr, uint8_t *d_flags, trxsig_c32 *d_amp, float *d_toa,
                           float *d_toa_eq, float *d_chan_off, trxsig_c32 *d_w, trxsig_c32 *d_b,
                           int32_t *d_listed = nullptr /* the marked bursts already listed: their count, then their indices (any order) */);
int trx_ctx_group_equalize(trxsig_ctx *c, const trxsig_c32 *d_samples, const int32_t *d_offset, const int32_t *d_length, int B,
                           const trxsig_c32 *d_amp, const float *d_toa_eq, const uint8_t *d_gate, const trxsig_c32 *d_w_tab,
                           const trxsig_c32 *d_b_tab, const int32_t *d_tap_ix, float *d_soft, int nsoft, int soft_stride);

// ---- what every object that lives on a context does the same way (trxsig_l1*.cpp, trxsig_air.cpp) ---------------------------
#pragma GCC visibility push(hidden)
inline size_t trx_align256(size_t x) { return (x + 255) & ~(size_t)255; }

// One device block carved into regions that each start on a 256-byte boundary: sizes in (the list, or add() one by one, which
// returns the region's handle: its place in the order), `total` and, once the block is there, typed pointers out.
struct TrxCarve {
  static constexpr int kMax = 32;
  size_t off[kMax] = {}, total = 0;
  int n = 0;
  TrxCarve() = default;
  TrxCarve(std::initializer_list<size_t> sizes) { for (size_t s : sizes) add(s); }
  int add(size_t bytes) { assert(n < kMax); off[n] = total; total += trx_align256(bytes); return n++; }
  template <class T> T *at(void *base, int region) const { return (T *)((char *)base + off[region]); }
};

// An object's persistent block: `total` bytes, zero-filled, then the pieces copied from the host in the order given (empty
// ones skipped).  On failure nothing stays allocated, *out is null and the context's last error is "<who>: device allocation"
// (TRXSIG_ENOMEM) or "<who>: upload" (TRXSIG_EHIP).  The caller holds the TrxDeviceGuard.
struct TrxUpload { size_t off; const void *src; size_t bytes; };
inline int trx_device_block(trxsig_ctx *c, const char *who, size_t total, std::initializer_list<TrxUpload> pieces, void **out) {
  *out = nullptr;
  if (hipMalloc(out, total) != hipSuccess) {
    *out = nullptr;
    return trx_ctx_fail(c, TRXSIG_ENOMEM, (std::string(who) + ": device allocation").c_str(), hipSuccess);
  }
  hipError_t e = hipMemset(*out, 0, total);
  for (const TrxUpload &u : pieces)
    if (e == hipSuccess && u.bytes) e = hipMemcpy((char *)*out + u.off, u.src, u.bytes, hipMemcpyHostToDevice);
  if (e == hipSuccess) return TRXSIG_OK;
  (void)hipFree(*out);
  *out = nullptr;
  return trx_ctx_fail(c, TRXSIG_EHIP, (std::string(who) + ": upload").c_str(), e);
}

// A per-call workspace that only grows.  A growth waits for the context's stream first (the old block may still be read), and
// from then on the old contents are gone (*gone = true, also where the growth then fails).  oom: the last-error text of a
// failed allocation, reported as TRXSIG_ENOMEM; null: it is reported as any failed HIP call (TRXSIG_EHIP).
struct TrxWork { void *p = nullptr; size_t bytes = 0; };
inline int trx_work_ensure(trxsig_ctx *c, TrxWork &w, size_t need, bool zero, const char *oom, bool *gone = nullptr) {
  if (need <= w.bytes) return TRXSIG_OK;
  TRX_HIPCHK(c, hipStreamSynchronize((hipStream_t)trxsig_get_stream(c)));
  if (gone) *gone = true;
  if (w.p) { TRX_HIPCHK(c, hipFree(w.p)); w.p = nullptr; w.bytes = 0; }
  if (!oom) TRX_HIPCHK(c, hipMalloc(&w.p, need));
  else if (hipMalloc(&w.p, need) != hipSuccess) return trx_ctx_fail(c, TRXSIG_ENOMEM, oom, hipSuccess);
  if (zero) TRX_HIPCHK(c, hipMemset(w.p, 0, need));
  w.bytes = need;
  return TRXSIG_OK;
}

// An object's end: wait for the context's stream, free its device blocks (null ones skipped), give the context back (which
// destroys a context whose trxsig_destroy waited for this object).  The caller deletes the object afterwards.
inline void trx_object_destroy(trxsig_ctx *c, std::initializer_list<void *> blocks) {
  {
    TrxDeviceGuard g(trxsig_device(c));
    (void)hipStreamSynchronize((hipStream_t)trxsig_get_stream(c));
    for (void *p : blocks)
      if (p) (void)hipFree(p);
  }
  trx_ctx_release(c);
}
#pragma GCC visibility pop
