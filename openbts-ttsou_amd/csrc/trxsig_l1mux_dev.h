// trxsig_l1mux_dev.h -- internal, device code: what the two transmit multiplexers have in common, the downlink's of the
// base-station side (trxsig_l1tx.hip) and the uplink's of the mobile side (trxsig_l1ms.hip): the block encoder's tail, the
// slot writer's lookup, staging and normal-burst gather, the record commit's shared head, and the launchers' slicing.  The
// routines are templates over the direction's Dev struct (TrxMuxDev<Chan>, trxsig_tdma.h) and take the direction's mapping as
// an argument, so nothing here names a direction.  The __global__ kernels, with their LDS arrays, stay in the two .hip files.
//
// Every routine is called by whole waves and syncs within the wave only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "trxsig_bursts.h"
#include "trxsig_fec_enc.h"
#include "trxsig_launch.h"
#include "trxsig_tdma.h"

// GSM 05.02 5.2.3 training sequences as bytes and the XCCH inverse interleaver (TCH's is trxsig_fec_enc.h's kTchInv)
struct MuxConsts {
  uint8_t tsc[8][26];
  uint16_t xinv[4][114];                     // XCCH: (burst B, e-bit j) -> c index
  constexpr MuxConsts() : tsc(), xinv() {
    const char *ts[8] = TRX_TSC_BITS;
    for (int t = 0; t < 8; t++)
      for (int i = 0; i < 26; i++) tsc[t][i] = (uint8_t)(ts[t][i] == '1');
    for (int c = 0; c < 456; c++) xinv[c & 3][2 * ((49 * c) % 57) + ((c % 8) / 4)] = (uint16_t)c;
  }
};
__device__ __constant__ const MuxConsts kMux;

__device__ __forceinline__ long long mux_ceil4(long long p) { return -((-p) >> 2); }

// the blocks of mapping m whose first burst lies in the call, and the first of them
__device__ __forceinline__ int mux_chan_blocks(const TrxMuxCall &c, int m, long long *blk_first) {
  *blk_first = mux_ceil4(c.p_first[m]);
  const long long nb = mux_ceil4(c.p_end[m]) - *blk_first;
  return nb > 0 ? (int)nb : 0;
}

// position of frame fn + k in mapping m = M (trxsig_tdma.h: base + n * Q + cnt[rem], Q / rem by the constant repeat length)
template <class Dev>
__device__ __forceinline__ long long mux_map_pos(const TrxMuxCall &c, const Dev &d, const TrxTdmaMap &M, int m, int k) {
  const int R = M.R;
  int Q, rem;
  switch (R) {
    case 26: { const int t = c.r26 + k; Q = t / 26; rem = t - 26 * Q; break; }
    case 51: { const int t = c.r51 + k; Q = t / 51; rem = t - 51 * Q; break; }
    case 102: { const int t = c.r102 + k; Q = t / 102; rem = t - 102 * Q; break; }
    default: { const int t = c.r104 + k; Q = t / 104; rem = t - 104 * Q; break; }
  }
  return c.base[m] + (long long)M.n * Q + d.cnt[m * 105 + rem];
}

// ---- k_*_encode ------------------------------------------------------------------------------------------------------------
// block gi of the call's grid of class cls (0 TCH: any kind, 33 octets; else kind 1, 23 octets): whether it is sent, its payload
template <class Dev>
__device__ __forceinline__ bool mux_grid_block(const Dev &d, int cls, size_t gi, int *kind, const uint8_t **pl) {
  if (cls == 0) { *kind = d.kind[0][gi]; *pl = d.payload[0] + gi * 33; return true; }
  if (d.kind[cls][gi] != 1) return false;
  *pl = d.payload[cls] + gi * 23;
  return true;
}

// One wave forms a block's c[456] and writes it packed (16 words) with its flag byte (1 sent, 2 FACCH).  tch: tch_form_c on the
// payload by its kind; else the 23 octets are staged -- a SACCH's octets 0 and 1 are hdr(0), hdr(1), the L1 header -- and coded as
// a FACCH block (XCCHL1Encoder::encode).  cc, u, pls, fr: the wave's LDS rows of 456, 232, 36 and 36 bytes.
template <class Hdr>
__device__ __forceinline__ void mux_encode_block(bool send, const uint8_t *pl, bool tch, int kind, bool sacch, Hdr hdr,
                                                 const uint8_t *filler, uint32_t *cw, uint8_t *flag, uint8_t *cc, uint8_t *u,
                                                 uint8_t *pls, uint8_t *fr, int lane) {
  if (!send) { if (lane == 0) *flag = 0; return; }
  if (tch) {
    tch_form_c(kind, pl, filler, u, cc, pls, lane);
  } else {
    if (lane < 36) {
      uint8_t v = lane < 23 ? pl[lane] : (uint8_t)0;
      if (sacch && lane < 2) v = hdr(lane);
      fr[lane] = v;
    }
    wave_fence();
    tch_form_c(TCH_FACCH, fr, filler, u, cc, pls, lane);
  }
  if (lane < 16) {
    uint32_t v = 0;
    for (int k = 0; k < 32; k++)
      if (32 * lane + k < 456) v |= (uint32_t)(cc[32 * lane + k] & 1u) << k;
    cw[lane] = v;
  }
  if (lane == 0) *flag = (uint8_t)(1u | (tch && kind == TCH_FACCH ? 2u : 0u));
}

// ---- k_*_commit ------------------------------------------------------------------------------------------------------------
// what the call leaves in the head of a channel's record, read by the whole wave before any of it is written
struct MuxCommit {
  uint32_t lv, pv;                           // lanes 0..15: a word of last_c, prev_c
  uint8_t lf, pf, pend;
  long long bf;                              // the mapping's first block of the call
};

template <class Dev>
__device__ __forceinline__ MuxCommit mux_commit_read(const TrxMuxCall &c, const Dev &d, const TrxMuxChan &S, int cls, int ci, int m,
                                                     int lane) {
  MuxCommit r{};
  const int nbc = mux_chan_blocks(c, m, &r.bf);
  const size_t u0 = (size_t)c.unit0[cls] + (size_t)ci * c.nb[cls];
  int L = -1, L2 = -1;                                       // the last two blocks sent in the call
  for (int b0 = 0; b0 < nbc; b0 += 64) {
    const int b = b0 + lane;
    const unsigned long long bal = __ballot(b < nbc && (d.flag[u0 + b] & 1u));
    for (unsigned long long x = bal; x; x &= x - 1) { L2 = L; L = b0 + __ffsll((long long)x) - 1; }
  }
  const uint32_t *lastc = L >= 0 ? d.c + (u0 + L) * 16 : S.last_c;
  const uint32_t *prevc = L >= 0 ? (L2 >= 0 ? d.c + (u0 + L2) * 16 : S.last_c) : S.prev_c;
  if (lane < 16) { r.lv = lastc[lane]; r.pv = prevc[lane]; }
  r.lf = L >= 0 ? (uint8_t)((d.flag[u0 + L] >> 1) & 1u) : S.last_f;
  r.pf = L >= 0 ? (L2 >= 0 ? (uint8_t)((d.flag[u0 + L2] >> 1) & 1u) : S.last_f) : S.prev_f;
  const long long pe = c.p_end[m];
  if (nbc > 0) r.pend = (L == nbc - 1 && 4 * (r.bf + L) + 3 >= pe) ? 1 : 0;
  else r.pend = (S.pend && pe < 4 * r.bf) ? 1 : 0;
  return r;
}

// ... and its write into the other copy's head; the direction's fields follow from lane 0
__device__ __forceinline__ void mux_commit_write(TrxMuxChan &N, const MuxCommit &k, uint8_t active, int lane) {
  __builtin_amdgcn_wave_barrier();
  if (lane < 16) { N.last_c[lane] = k.lv; N.prev_c[lane] = k.pv; }
  if (lane == 0) { N.last_f = k.lf; N.prev_f = k.pf; N.pend = k.pend; N.active = active; }
}

// ---- k_*_mux ---------------------------------------------------------------------------------------------------------------
// the mapping that owns the slot (sl = its word of d.slot, TN tn) in frame fn + k, or -1
template <class Dev>
__device__ __forceinline__ int mux_slot_owner(const TrxMuxCall &c, const Dev &d, int sl, int tn, int k) {
  const int comb = sl & 15;
  if (!comb) return -1;
  const int cix = comb == 1 ? 0 : comb == 5 ? 1 : 2;
  int r;
  if (comb == 1) { const int t = c.r104 + k; r = t - 104 * (t / 104); }
  else { const int t = c.r102 + k; r = t - 102 * (t / 102); }
  return d.writer[(cix * 8 + tn) * 104 + r];
}

// the channel (over all classes) that dedicated mapping m (an id below 33) names on a slot whose first XCCH channel is x0
__device__ __forceinline__ int mux_slot_chan(int m, int sl, int x0) {
  if (m == TRX_MAP_TCHF) return sl >> 4;
  if (m < TRX_MAP_SDCCH8) return x0;
  if (m < TRX_MAP_SACCH_C8) return x0 + (m - TRX_MAP_SDCCH8);
  if (m < TRX_MAP_SDCCH4) return x0 + 8 + (m - TRX_MAP_SACCH_C8);
  if (m < TRX_MAP_SACCH_C4) return x0 + (m - TRX_MAP_SDCCH4);
  return x0 + 4 + (m - TRX_MAP_SACCH_C4);
}

// The block that channel (cls, ci), record S, sends in frame fn + k of its mapping m = M: its c words and the block's before it
// with their FACCH flags, from the call's scratch or (a block begun in an earlier call: pend) from the record, and the burst
// B of the block.  cur == nullptr: no block here -- where the channel has idle fill left it applies to positions from idle0.
struct MuxBlock {
  const uint32_t *cur, *prev;
  unsigned curF, prevF;
  int B;
  long long q, idle0;
};

template <class Dev>
__device__ __forceinline__ MuxBlock mux_block(const TrxMuxCall &c, const Dev &d, const TrxTdmaMap &M, const TrxMuxChan &S, int cls,
                                              int ci, int m, int k) {
  MuxBlock r{ nullptr, nullptr, 0u, 0u, 0, 0, 0 };
  r.q = mux_map_pos(c, d, M, m, k);
  const long long bf = mux_ceil4(c.p_first[m]);
  const long long rel = (r.q >> 2) - bf;
  r.B = (int)(r.q & 3);
  r.idle0 = c.p_first[m];
  if (rel < 0) {
    if (S.pend) { r.cur = S.last_c; r.prev = S.prev_c; r.curF = S.last_f; r.prevF = S.prev_f; }
  } else {
    const size_t u = (size_t)c.unit0[cls] + (size_t)ci * c.nb[cls] + (size_t)rel;
    const unsigned f = d.flag[u];
    if (f & 1u) {
      r.cur = d.c + u * 16; r.curF = (f >> 1) & 1u;
      if (rel > 0) { r.prev = d.c + (u - 1) * 16; r.prevF = (d.flag[u - 1] >> 1) & 1u; }
      else { r.prev = S.last_c; r.prevF = S.last_f; }
    } else if (S.pend) {
      r.idle0 = 4 * bf;
    }
  }
  return r;
}

// a slot's 32 staged words: this block's c words, then the previous block's
__device__ __forceinline__ void mux_stage(uint32_t *cw, const uint32_t *cur, const uint32_t *prev) {
  for (int i = 0; i < 16; i++) {
    cw[i] = cur ? cur[i] : 0u;
    cw[16 + i] = prev ? prev[i] : 0u;
  }
}

// bit pos of a normal burst from a slot's staged words: tail, e-bits through the inverse interleaver (GSM 05.03 4.1.4 for
// XCCH-like blocks, 3.1.3 for TCH, whose odd bits are the previous block's), stealing flags, training sequence
__device__ __forceinline__ unsigned mux_normal_bit(const uint32_t *cw, int B, unsigned curF, unsigned prevF, bool tch,
                                                   const uint8_t *tsc, int pos) {
  auto cbit = [&](int idx, int half) { return (cw[16 * half + (idx >> 5)] >> (idx & 31)) & 1u; };
  if (pos < 3 || pos >= 145) return 0u;
  if (pos == 60) return tch ? prevF : 1u;
  if (pos == 87) return tch ? curF : 1u;
  if (pos > 60 && pos < 87) return tsc[pos - 61];
  const int j = pos < 60 ? pos - 3 : pos - 31;
  if (!tch) return cbit(kMux.xinv[B][j], 0);
  return cbit(kTchInv.k[B][j], j & 1);
}

// a half frame's four slots: 37 lanes store 16 bytes of bits each, byte i of the 592 being obyte(i); lane 0 the `what` word,
// code(s) of slot s in byte s.  base: the first slot's index in [n_arfcn][8 F]
template <class Byte, class Code>
__device__ __forceinline__ void mux_store(uint8_t *bits, uint8_t *what, size_t base, int lane, Byte obyte, Code code) {
  uint8_t *out = bits + base * 148;
  if (lane < 37) {
    unsigned v4[4];
    for (int q = 0; q < 4; q++) {
      unsigned v = 0;
      for (int r = 0; r < 4; r++) v |= obyte(16 * lane + 4 * q + r) << (8 * r);
      v4[q] = v;
    }
    reinterpret_cast<uint4 *>(out)[lane] = make_uint4(v4[0], v4[1], v4[2], v4[3]);
  }
  if (lane == 0) {
    unsigned v = 0;
    for (int s = 0; s < 4; s++) v |= (unsigned)code(s) << (8 * s);
    *reinterpret_cast<uint32_t *>(what + base) = v;
  }
}

// ---- launchers -------------------------------------------------------------------------------------------------------------
// a slice's workgroups: 256 * (2^24 - 1) work-items < 2^32 (a dispatch's work-item count), and a grid's y at most 65535
constexpr long long kMaxWg = (1LL << 24) - 1;
constexpr long long kMaxY = 65535;

// n rows of gx workgroups in slices a dispatch can hold: launch(grid, y0) per slice
template <class Launch>
inline void mux_launch_slices(long long gx, long long n, Launch launch) {
  long long ys = kMaxWg / gx > 0 ? kMaxWg / gx : 1;         // rows per slice
  if (ys > kMaxY) ys = kMaxY;
  for (long long y0 = 0; y0 < n; y0 += ys) launch(dim3((unsigned)gx, (unsigned)(n - y0 < ys ? n - y0 : ys)), (int)y0);
}
