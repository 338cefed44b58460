// trxsig_l1tx.hip -- the downlink L1 multiplexer's kernels (include/trxsig_l1tx.h, host side in trxsig_l1tx.cpp).  What the
// downlink has in common with the mobile side's uplink multiplexer (trxsig_l1ms.hip) -- the block encoder's tail, the slot
// writer's block lookup and normal-burst gather, the commit's head -- is trxsig_l1mux_dev.h; here are the kernels and the
// downlink's own part: four channel classes, the orders, the BCCH's SI, the beacon's FCCH / SCH bursts and the idle fill.
//
// k_l1tx_encode: a wave per (channel, block b) of the call.  It decides whether the block is sent (open channel; TCH any kind,
//   XCCH / CCCH kind 1, BCCH once SIs are set), stages the 23 octets (SACCH: octets 0..1 = the L1 header of the call's
//   orders; BCCH: the SI of TC = (FN / 51) % 8) and forms c[456] with trxsig_fec_enc.h's tch_form_c -- the FACCH branch is
//   exactly XCCHL1Encoder::encode on the LSB8MSB'd frame, the others TCHFACCHL1Encoder::encodeTCH / filler / zero.  c[] goes
//   to the scratch packed (16 words), with a flag byte (1 sent, 2 FACCH).  The b = 0 wave of an XCCH channel also writes the
//   channel's orders after the call (SACCHL1Encoder::sendFrame's phyNew branch, decided from the sibling's snapshot).
// k_l1tx_mux: a wave per (ARFCN, frame, half frame): four slots, 592 contiguous output bytes.  Lanes 0..3 find each slot's
//   writer -- the mapping that owns (combination, TN, FN mod 104 / 102) from the host's table, the channel, the position q
//   (trxsig_tdma.h) -- and stage its c[] words (block q / 4 of the call from the scratch, or the channel's pending block from
//   its record); then 37 lanes gather 16 bytes each through the inverse interleaver (GSM 05.03 4.1.4 for XCCH-like blocks,
//   3.1.3 for TCH) and store them at once.
// k_l1tx_commit (same stream, after the mux; a wave per channel): each channel's record into the other copy -- the last two
//   blocks sent, the pending flag, idle fill left, the orders.  The call reads copy `cur` only, so no wave races another.
// k_l1tx_count / k_l1tx_scan / k_l1tx_pack: the datagrams of the non-empty slots, in (FN, TN, ARFCN) order.
#include "trxsig_l1mux_dev.h"

namespace {

__constant__ TrxTdmaMap c_dl[TRX_N_DL_MAPS] = TRX_TDMA_DL_MAPS_INIT;
__constant__ int8_t c_pw[3][32] = TRX_POWER_TABLES_INIT;

// the dummy burst of trxsig_bursts.h as bytes and the GSM 05.02 5.2.5 SCH extended training sequence (public constants of
// the standard)
struct Consts {
  uint8_t dummy[148];
  unsigned long long xts;
  constexpr Consts() : dummy(), xts(0) {
    const char *d = TRX_DUMMY_BURST_BITS;
    for (int i = 0; i < 148; i++) dummy[i] = (uint8_t)(d[i] == '1');
    const char *x = "1011100101100010000001000000111100101101010001010111011000011011";
    for (int i = 0; i < 64; i++) xts |= (unsigned long long)(x[i] == '1') << i;
  }
};
__device__ __constant__ const Consts kC;

enum { W_NONE = 0, W_FCCH = 1, W_SCH = 2, W_BCCH = 3, W_CCCH = 4, W_XCCH = 5, W_TCH = 6, W_IDLE = 7 };

// the class (0 TCH, 1 XCCH, 2 CCCH, 3 BCCH) and index in it of channel g
__device__ __forceinline__ int chan_class(const TrxL1txCall &c, int g, int *ci) {
  if (g < c.n_tch) { *ci = g; return 0; }
  g -= c.n_tch;
  if (g < c.n_xcch) { *ci = g; return 1; }
  g -= c.n_xcch;
  if (g < c.n_ccch) { *ci = g; return 2; }
  *ci = g - c.n_ccch;
  return 3;
}

// SACCHL1Encoder::sendFrame's orders for the call: phyNew = the sibling's SACCH channel accepted a burst since the orders were
// last decided; consumed only where the call sends a SACCH block
struct Orders { int pow; float ta; bool consumed; };
__device__ Orders call_orders(const TrxL1txCall &c, const TrxL1txDev &d, const TrxL1txChan &S, int ci, int m) {
  Orders o{ S.ord_pow, S.ord_ta, false };
  if (!c.has_sib || d.sib_count[ci] == S.seen || !S.h.active) return o;
  long long bf = 0;
  const int nbc = mux_chan_blocks(c, m, &bf);
  bool any = false;
  for (int b = 0; b < nbc; b++) any |= d.kind[1][(size_t)ci * c.nb[1] + b] == 1;
  if (!any) return o;
  const float rssi = (float)d.sib_rssi[ci];
  const float dP = __fsub_rn(rssi, c.rssi_target);
  const float actual = (float)d.sib_power[ci];
  int p = (int)__fsub_rn(actual, (float)(int)roundf(__fmul_rn(dP, 0.5F)));
  if (p > 40) p = 40; else if (p < 0) p = 0;
  float t = __fsub_rn((float)d.sib_ta[ci], __fmul_rn(0.5F, (float)d.sib_timing[ci]));
  if (t > 63.0F) t = 63.0F;
  if (t < 0.0F) t = 0.0F;
  o.pow = p; o.ta = t; o.consumed = true;
  return o;
}

__global__ __launch_bounds__(256) void k_l1tx_encode(TrxL1txCall c, TrxL1txDev d, int b_off) {
  __shared__ uint8_t s_c[4][456], s_u[4][232], s_pls[4][36], s_fr[4][36];
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int g = blockIdx.x * 4 + w, b = (int)blockIdx.y + b_off;
  if (g >= c.n_all) return;                                  // whole waves only: nothing below syncs across waves
  int ci = 0;
  const int cls = chan_class(c, g, &ci);
  const int m = d.chinfo[g] >> 20;
  const TrxL1txChan &S = d.st[(size_t)c.cur * c.n_all + g];
  const bool sacch = cls == 1 && trx_map_is_sacch(m);
  Orders o{ -1, -1.0F, false };
  if (sacch) o = call_orders(c, d, S, ci, m);
  if (cls == 1 && b == 0 && lane == 0) { d.ord_pow[ci] = o.pow; d.ord_ta[ci] = sacch ? o.ta : -1.0F; }
  const int nbk = c.nb[cls];
  if (b >= nbk) return;
  long long bf = 0;
  const int nbc = mux_chan_blocks(c, m, &bf);
  const size_t unit = (size_t)c.unit0[cls] + (size_t)ci * nbk + b;
  const size_t gi = (size_t)ci * nbk + b;
  int kind = 0;
  bool send = false;
  const uint8_t *pl = nullptr;
  if (b < nbc && S.h.active) {
    if (cls != 3) send = mux_grid_block(d, cls, gi, &kind, &pl);
    else if (d.si[92]) {
      const long long u = c_dl[TRX_DL_BCCH].f[0] + ((bf + b) * 51);   // the block's first frame (n = 4: q = 4 (bf + b))
      const int tc = (int)((u % kTrxHyperframe) / 51) % 8;
      const int sel = tc == 0 ? 0 : (tc == 1 || tc == 5) ? 1 : (tc == 3 || tc == 7) ? 3 : 2;   // SI1, 2, 3, 4, 3, 2, 3, 4
      send = true; pl = d.si + 23 * sel;
    }
  }
  auto hdr = [&](int i) { return (uint8_t)(i == 0 ? trx_encode_power(c_pw[c.band], o.pow) : (int)__fadd_rn(o.ta, 0.5F)); };
  mux_encode_block(send, pl, cls == 0, kind, sacch, hdr, d.filler, d.c + unit * 16, d.flag + unit, s_c[w], s_u[w], s_pls[w],
                   s_fr[w], lane);
}

struct SlotW {
  int code, B;
  unsigned curF, prevF;
  unsigned long long e0, e1;                                 // SCH e-bits
};

// SCHL1Encoder::generate for frame fn, as k_fec_sch_encode
__device__ void sch_bits(unsigned fn, unsigned bsic, unsigned long long *pe0, unsigned long long *pe1) {
  unsigned long long e0 = 0, e1 = 0;
  const unsigned t1 = (fn / (26u * 51u)) % 2048u, t2 = fn % 26u, t3 = fn % 51u;
  const unsigned t3p = (t3 - 1u) / 10u;
  const unsigned D = (bsic << 19) | (t1 << 8) | ((t2 & 31u) << 3) | (t3p & 7u);
  unsigned dd = 0;
  for (int q = 0; q < 25; q++) {
    const int src = q < 24 ? 8 * (q >> 3) + 7 - (q & 7) : 24;
    dd |= ((D >> (24 - src)) & 1u) << (24 - q);
  }
  unsigned par = 0;
  for (int q = 0; q < 25; q++) {
    const unsigned fb = ((par >> 9) ^ (dd >> (24 - q))) & 1u;
    par <<= 1;
    if (fb) par ^= 0x575u;
  }
  const unsigned pw = ~par & 0x3ffu;
  const unsigned long long uu = ((unsigned long long)dd << 14) | ((unsigned long long)pw << 4);
  unsigned acc = 0;
  for (int q = 0; q < 39; q++) {
    acc = (acc << 1) | (unsigned)((uu >> (38 - q)) & 1ULL);
    const unsigned long long gg = (kGen >> (2 * (acc & 31u))) & 3ULL;
    const int p = 2 * q;
    if (p < 64) e0 |= (gg >> 1) << p; else e1 |= (gg >> 1) << (p - 64);
    if (p + 1 < 64) e0 |= (gg & 1ULL) << (p + 1); else e1 |= (gg & 1ULL) << (p + 1 - 64);
  }
  *pe0 = e0; *pe1 = e1;
}

// record commit: a wave per channel
__global__ __launch_bounds__(256) void k_l1tx_commit(TrxL1txCall c, TrxL1txDev d) {
  const int g = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (g >= c.n_all) return;
  int ci = 0;
  const int cls = chan_class(c, g, &ci);
  const int m = d.chinfo[g] >> 20;
  const TrxL1txChan &S = d.st[(size_t)c.cur * c.n_all + g];
  TrxL1txChan &N = d.st[(size_t)(c.cur ^ 1) * c.n_all + g];
  const MuxCommit k = mux_commit_read(c, d, S.h, cls, ci, m, lane);
  const long long pe = c.p_end[m];
  const long long idle0 = S.h.pend ? 4 * k.bf : c.p_first[m];
  const long long sent = pe > idle0 ? pe - idle0 : 0;
  const long long il = (long long)S.idle_left - sent;
  const bool sacch = cls == 1 && trx_map_is_sacch(m);
  Orders o{ S.ord_pow, S.ord_ta, false };
  if (sacch) o = call_orders(c, d, S, ci, m);
  const uint32_t seen = o.consumed ? d.sib_count[ci] : S.seen;
  mux_commit_write(N.h, k, S.h.active, lane);
  if (lane == 0) {
    N.idle_left = il > 0 ? (int32_t)il : 0;
    N.ord_pow = o.pow; N.ord_ta = o.ta; N.seen = seen;
    N.pad[0] = N.pad[1] = N.pad[2] = 0;
  }
}

__global__ __launch_bounds__(256) void k_l1tx_mux(TrxL1txCall c, TrxL1txDev d, int a_off) {
  __shared__ SlotW s_w[4][4];
  __shared__ uint32_t s_cw[4][4][32];                        // per slot: this block's c words, then the previous block's
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int a = (int)blockIdx.y + a_off;
  const int unit = blockIdx.x * 4 + w;                       // half frame of this ARFCN
  const int F = c.n_frames;
  if (unit >= 2 * F) return;
  const int k = unit >> 1, h = unit & 1;
  if (lane < 4) {
    const int tn = 4 * h + lane;
    SlotW sw{ W_NONE, 0, 0u, 0u, 0ULL, 0ULL };
    const uint32_t *cur = nullptr, *prev = nullptr;
    const int sl = d.slot[a * 8 + tn];
    const int m = mux_slot_owner(c, d, sl, tn, k);
    if (m == TRX_DL_FCCH) sw.code = W_FCCH;
    else if (m == TRX_DL_SCH) {
      sw.code = W_SCH;
      sch_bits((unsigned)(((long long)c.fn + k) % kTrxHyperframe), (unsigned)c.bsic, &sw.e0, &sw.e1);
    } else if (m >= 0) {
      int g;
      if (m < TRX_DL_CCCH) g = mux_slot_chan(m, sl, d.slot_x[a * 8 + tn]);
      else if (m < TRX_DL_BCCH) g = c.n_tch + c.n_xcch + (m - TRX_DL_CCCH);
      else g = c.n_tch + c.n_xcch + c.n_ccch;
      int ci = 0;
      const int cls = chan_class(c, g, &ci);
      const TrxL1txChan &S = d.st[(size_t)c.cur * c.n_all + g];
      const MuxBlock blk = mux_block(c, d, c_dl[m], S.h, cls, ci, m, k);
      sw.B = blk.B;
      if (blk.cur) {
        sw.code = cls == 0 ? W_TCH : cls == 1 ? W_XCCH : cls == 2 ? W_CCCH : W_BCCH;
        cur = blk.cur; prev = blk.prev; sw.curF = blk.curF; sw.prevF = blk.prevF;
      } else if (S.idle_left > 0 && blk.q >= blk.idle0 && blk.q - blk.idle0 < S.idle_left) {
        sw.code = W_IDLE;
      }
    }
    s_w[w][lane] = sw;
    mux_stage(s_cw[w][lane], cur, prev);
  }
  wave_fence();
  const uint8_t *tsc = kMux.tsc[c.bsic & 7];
  auto obyte = [&](int i) -> unsigned {
    const int s = i / 148, pos = i - 148 * s;
    const SlotW &sw = s_w[w][s];
    switch (sw.code) {
      case W_IDLE: return kC.dummy[pos];
      case W_SCH:
        if (pos < 3 || pos >= 145) return 0u;
        if (pos < 42) { const int e = pos - 3; return (unsigned)((e < 64 ? sw.e0 >> e : sw.e1 >> (e - 64)) & 1ULL); }
        if (pos < 106) return (unsigned)(kC.xts >> (pos - 42)) & 1u;
        { const int e = 39 + pos - 106; return (unsigned)((e < 64 ? sw.e0 >> e : sw.e1 >> (e - 64)) & 1ULL); }
      case W_BCCH: case W_CCCH: case W_XCCH: case W_TCH:
        return mux_normal_bit(s_cw[w][s], sw.B, sw.curF, sw.prevF, sw.code == W_TCH, tsc, pos);
      default: return 0u;
    }
  };
  mux_store(d.bits, d.what, (size_t)a * (8LL * F) + 8 * (size_t)k + 4 * h, lane, obyte, [&](int s) { return s_w[w][s].code; });
}

__global__ void k_l1tx_set(TrxL1txChan *rec, int open, int sacch, int idle_fill) {
  if (threadIdx.x != 0) return;
  if (open) {
    rec->h.active = 1; rec->idle_left = 0;
    if (sacch) { rec->ord_pow = 40; rec->ord_ta = 0.0F; }
  } else {
    rec->h.active = 0; rec->idle_left = idle_fill;
  }
}

// datagrams: workgroup (x, y) takes slot row y (frame y / 8, TN y % 8) of ARFCNs 256 x .. 256 x + 255
__global__ __launch_bounds__(256) void k_l1tx_count(const uint8_t *__restrict__ what, int A, long long F8, int r0, int32_t *wg_count) {
  __shared__ int s_n[4];
  const int a = blockIdx.x * 256 + threadIdx.x;
  const int row = (int)blockIdx.y + r0;
  const bool on = a < A && what[(size_t)a * F8 + row] != 0;
  const unsigned long long bal = __ballot(on);
  if ((threadIdx.x & 63) == 0) s_n[threadIdx.x >> 6] = __popcll(bal);
  __syncthreads();
  if (threadIdx.x == 0) wg_count[(size_t)row * gridDim.x + blockIdx.x] = s_n[0] + s_n[1] + s_n[2] + s_n[3];
}

// exclusive scan of n counts in place, one workgroup; total to *total
__global__ __launch_bounds__(256) void k_l1tx_scan(int32_t *cnt, long long n, int32_t *total) {
  __shared__ int s_x[256];
  __shared__ int s_carry;
  if (threadIdx.x == 0) s_carry = 0;
  __syncthreads();
  for (long long b0 = 0; b0 < n; b0 += 256) {
    const long long i = b0 + threadIdx.x;
    const int v = i < n ? cnt[i] : 0;
    s_x[threadIdx.x] = v;
    __syncthreads();
    for (int off = 1; off < 256; off <<= 1) {
      const int t = threadIdx.x >= (unsigned)off ? s_x[threadIdx.x - off] : 0;
      __syncthreads();
      s_x[threadIdx.x] += t;
      __syncthreads();
    }
    const int carry = s_carry;
    if (i < n) cnt[i] = carry + s_x[threadIdx.x] - v;
    __syncthreads();
    if (threadIdx.x == 255) s_carry = carry + s_x[255];
    __syncthreads();
  }
  if (threadIdx.x == 0) *total = s_carry;
}

__global__ __launch_bounds__(256) void k_l1tx_pack(const uint8_t *__restrict__ what, const uint8_t *__restrict__ bits, int A,
                                                   long long F8, int r0, int fn, const int32_t *__restrict__ wg_off,
                                                   uint8_t *dgram, int32_t *arfcn, int cap) {
  __shared__ int s_n[4];
  const int a = blockIdx.x * 256 + threadIdx.x, lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int row = (int)blockIdx.y + r0;                      // 8 k + tn
  const bool on = a < A && what[(size_t)a * F8 + row] != 0;
  const unsigned long long bal = __ballot(on);
  if (lane == 0) s_n[wv] = __popcll(bal);
  __syncthreads();
  int j = wg_off[(size_t)row * gridDim.x + blockIdx.x] + __popcll(bal & ((1ULL << lane) - 1));
  for (int x = 0; x < wv; x++) j += s_n[x];
  if (!on || j >= cap) return;
  const unsigned f = (unsigned)(((long long)fn + (row >> 3)) % kTrxHyperframe);
  uint8_t *o = dgram + (size_t)j * 154;
  o[0] = (uint8_t)(row & 7);
  o[1] = (uint8_t)(f >> 24); o[2] = (uint8_t)(f >> 16); o[3] = (uint8_t)(f >> 8); o[4] = (uint8_t)f;
  o[5] = 0;
  const uint8_t *src = bits + ((size_t)a * F8 + row) * 148;
  for (int i = 0; i < 148; i++) o[6 + i] = src[i];
  arfcn[j] = a;
}

}  // namespace

hipError_t trx_launch_l1tx_encode(hipStream_t st, const TrxL1txCall &call, const TrxL1txDev &dv, TrxProfiler *prof) {
  if (call.n_all <= 0) return hipSuccess;
  int nbm = 1;
  for (int i = 0; i < 4; i++) nbm = call.nb[i] > nbm ? call.nb[i] : nbm;
  if (prof) prof->begin(TRXSIG_K_L1TX_ENCODE, st);
  mux_launch_slices((call.n_all + 3) / 4, nbm, [&](dim3 grid, int b0) { k_l1tx_encode<<<grid, dim3(256), 0, st>>>(call, dv, b0); });
  if (prof) prof->end(TRXSIG_K_L1TX_ENCODE, st);
  return hipGetLastError();
}

hipError_t trx_launch_l1tx_mux(hipStream_t st, const TrxL1txCall &call, const TrxL1txDev &dv, TrxProfiler *prof) {
  if (prof) prof->begin(TRXSIG_K_L1TX_MUX, st);
  mux_launch_slices((2LL * call.n_frames + 3) / 4, call.n_arfcn,
                    [&](dim3 grid, int a0) { k_l1tx_mux<<<grid, dim3(256), 0, st>>>(call, dv, a0); });
  if (prof) prof->end(TRXSIG_K_L1TX_MUX, st);
  if (call.n_all > 0) {
    if (prof) prof->begin(TRXSIG_K_L1TX_COMMIT, st);
    k_l1tx_commit<<<dim3((unsigned)((call.n_all + 3) / 4)), dim3(256), 0, st>>>(call, dv);
    if (prof) prof->end(TRXSIG_K_L1TX_COMMIT, st);
  }
  return hipGetLastError();
}

hipError_t trx_launch_l1tx_set(hipStream_t st, TrxL1txChan *rec, int open, int sacch, int idle_fill) {
  k_l1tx_set<<<dim3(1), dim3(64), 0, st>>>(rec, open, sacch, idle_fill);
  return hipGetLastError();
}

hipError_t trx_launch_l1tx_dgram(hipStream_t st, const uint8_t *what, const uint8_t *bits, int n_arfcn, int n_frames, int fn,
                                 int32_t *wg_count, int32_t *total, uint8_t *dgram, int32_t *arfcn, int cap, TrxProfiler *prof) {
  const long long F8 = 8LL * n_frames, gx = (n_arfcn + 255) / 256;
  if (prof) prof->begin(TRXSIG_K_L1TX_DGRAM, st);
  // rows (8 F) are at most 2^31 / 8 / 148 apart from the output bound, and gx * rows workgroups fit a dispatch's y-dimension
  for (long long r0 = 0; r0 < F8; r0 += kMaxY) {
    const long long nr = F8 - r0 < kMaxY ? F8 - r0 : kMaxY;
    k_l1tx_count<<<dim3((unsigned)gx, (unsigned)nr), dim3(256), 0, st>>>(what, n_arfcn, F8, (int)r0, wg_count);
  }
  k_l1tx_scan<<<dim3(1), dim3(256), 0, st>>>(wg_count, F8 * gx, total);
  for (long long r0 = 0; r0 < F8; r0 += kMaxY) {
    const long long nr = F8 - r0 < kMaxY ? F8 - r0 : kMaxY;
    k_l1tx_pack<<<dim3((unsigned)gx, (unsigned)nr), dim3(256), 0, st>>>(what, bits, n_arfcn, F8, (int)r0, fn, wg_count, dgram,
                                                                        arfcn, cap);
  }
  if (prof) prof->end(TRXSIG_K_L1TX_DGRAM, st);
  return hipGetLastError();
}
