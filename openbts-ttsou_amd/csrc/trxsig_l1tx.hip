// trxsig_l1tx.hip -- the downlink L1 multiplexer's kernels (include/trxsig_l1tx.h, host side in trxsig_l1tx.cpp).
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
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "trxsig_bursts.h"
#include "trxsig_fec_enc.h"
#include "trxsig_launch.h"
#include "trxsig_tdma.h"

namespace {

__constant__ TrxTdmaMap c_dl[TRX_N_DL_MAPS] = TRX_TDMA_DL_MAPS_INIT;
__constant__ int8_t c_pw[3][32] = TRX_POWER_TABLES_INIT;

// GSM 05.02 5.2.3 training sequences and 5.2.5 SCH extended training sequence (public constants of the standard), the dummy
// burst of trxsig_bursts.h as bytes, and the XCCH inverse interleaver (TCH's is trxsig_fec_enc.h's kTchInv)
struct Consts {
  uint8_t tsc[8][26];
  uint8_t dummy[148];
  unsigned long long xts;
  uint16_t xinv[4][114];                     // XCCH: (burst B, e-bit j) -> c index
  constexpr Consts() : tsc(), dummy(), xts(0), xinv() {
    const char *ts[8] = { "00100101110000100010010111", "00101101110111100010110111", "01000011101110100100001110",
                          "01000111101101000100011110", "00011010111001000001101011", "01001110101100000100111010",
                          "10100111110110001010011111", "11101111000100101110111100" };
    for (int t = 0; t < 8; t++)
      for (int i = 0; i < 26; i++) tsc[t][i] = (uint8_t)(ts[t][i] == '1');
    const char *d = TRX_DUMMY_BURST_BITS;
    for (int i = 0; i < 148; i++) dummy[i] = (uint8_t)(d[i] == '1');
    const char *x = "1011100101100010000001000000111100101101010001010111011000011011";
    for (int i = 0; i < 64; i++) xts |= (unsigned long long)(x[i] == '1') << i;
    for (int c = 0; c < 456; c++) xinv[c & 3][2 * ((49 * c) % 57) + ((c % 8) / 4)] = (uint16_t)c;
  }
};
__device__ __constant__ const Consts kC;

enum { W_NONE = 0, W_FCCH = 1, W_SCH = 2, W_BCCH = 3, W_CCCH = 4, W_XCCH = 5, W_TCH = 6, W_IDLE = 7 };

__device__ __forceinline__ bool is_sacch(int m) {
  return (m >= TRX_MAP_SACCH_TF && m < TRX_MAP_SDCCH8) || (m >= TRX_MAP_SACCH_C8 && m < TRX_MAP_SDCCH4) ||
         (m >= TRX_MAP_SACCH_C4 && m < TRX_DL_CCCH);
}
__device__ __forceinline__ long long ceil4(long long p) { return -((-p) >> 2); }

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

// the blocks of mapping m whose first burst lies in the call, and the first of them
__device__ __forceinline__ int chan_blocks(const TrxL1txCall &c, int m, long long *blk_first) {
  *blk_first = ceil4(c.p_first[m]);
  const long long nb = ceil4(c.p_end[m]) - *blk_first;
  return nb > 0 ? (int)nb : 0;
}

// SACCHL1Encoder::sendFrame's orders for the call: phyNew = the sibling's SACCH channel accepted a burst since the orders were
// last decided; consumed only where the call sends a SACCH block
struct Orders { int pow; float ta; bool consumed; };
__device__ Orders call_orders(const TrxL1txCall &c, const TrxL1txDev &d, const TrxL1txChan &S, int ci, int m) {
  Orders o{ S.ord_pow, S.ord_ta, false };
  if (!c.has_sib || d.sib_count[ci] == S.seen || !S.active) return o;
  long long bf = 0;
  const int nbc = chan_blocks(c, m, &bf);
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

// encodePower: the band's table, nearest code, first on ties, an exact match at once
__device__ int encode_power(int band, int power) {
  unsigned minErr = (unsigned)abs(power - c_pw[band][0]), code = 0;
  for (int i = 1; i < 32; i++) {
    const unsigned e = (unsigned)abs(power - c_pw[band][i]);
    if (e == 0) return i;
    if (e < minErr) { minErr = e; code = (unsigned)i; }
  }
  return (int)code;
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
  const bool sacch = cls == 1 && is_sacch(m);
  Orders o{ -1, -1.0F, false };
  if (sacch) o = call_orders(c, d, S, ci, m);
  if (cls == 1 && b == 0 && lane == 0) { d.ord_pow[ci] = o.pow; d.ord_ta[ci] = sacch ? o.ta : -1.0F; }
  const int nbk = c.nb[cls];
  if (b >= nbk) return;
  long long bf = 0;
  const int nbc = chan_blocks(c, m, &bf);
  const size_t unit = (size_t)c.unit0[cls] + (size_t)ci * nbk + b;
  const size_t gi = (size_t)ci * nbk + b;
  int kind = 0;
  bool send = false;
  const uint8_t *pl = nullptr;
  if (b < nbc && S.active) {
    if (cls == 0) { kind = d.kind[0][gi]; send = true; pl = d.payload[0] + gi * 33; }
    else if (cls == 3) {
      if (d.si[92]) {
        const long long u = c_dl[TRX_DL_BCCH].f[0] + ((bf + b) * 51);   // the block's first frame (n = 4: q = 4 (bf + b))
        const int tc = (int)((u % kTrxHyperframe) / 51) % 8;
        const int sel = tc == 0 ? 0 : (tc == 1 || tc == 5) ? 1 : (tc == 3 || tc == 7) ? 3 : 2;   // SI1, 2, 3, 4, 3, 2, 3, 4
        send = true; pl = d.si + 23 * sel;
      }
    } else if (d.kind[cls][gi] == 1) { send = true; pl = d.payload[cls] + gi * 23; }
  }
  if (!send) { if (lane == 0) d.flag[unit] = 0; return; }
  uint8_t *cc = s_c[w];
  if (cls == 0) {
    tch_form_c(kind, pl, d.filler, s_u[w], cc, s_pls[w], lane);
  } else {
    uint8_t *fr = s_fr[w];
    if (lane < 36) {
      uint8_t v = lane < 23 ? pl[lane] : (uint8_t)0;
      if (sacch && lane == 0) v = (uint8_t)encode_power(c.band, o.pow);
      if (sacch && lane == 1) v = (uint8_t)(int)__fadd_rn(o.ta, 0.5F);
      fr[lane] = v;
    }
    wave_fence();
    tch_form_c(TCH_FACCH, fr, d.filler, s_u[w], cc, s_pls[w], lane);
  }
  if (lane < 16) {
    uint32_t v = 0;
    for (int k = 0; k < 32; k++)
      if (32 * lane + k < 456) v |= (uint32_t)(cc[32 * lane + k] & 1u) << k;
    d.c[unit * 16 + lane] = v;
  }
  if (lane == 0) d.flag[unit] = (uint8_t)(1u | (cls == 0 && kind == TCH_FACCH ? 2u : 0u));
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

// position of frame fn + k in mapping m (trxsig_tdma.h: base + n * Q + cnt[rem], Q / rem by the constant repeat length)
__device__ __forceinline__ long long map_pos(const TrxL1txCall &c, const TrxL1txDev &d, int m, int k) {
  const int R = c_dl[m].R;
  int Q, rem;
  switch (R) {
    case 26: { const int t = c.r26 + k; Q = t / 26; rem = t - 26 * Q; break; }
    case 51: { const int t = c.r51 + k; Q = t / 51; rem = t - 51 * Q; break; }
    case 102: { const int t = c.r102 + k; Q = t / 102; rem = t - 102 * Q; break; }
    default: { const int t = c.r104 + k; Q = t / 104; rem = t - 104 * Q; break; }
  }
  return c.base[m] + (long long)c_dl[m].n * Q + d.cnt[m * 105 + rem];
}

// record commit of channel g (one wave)
__device__ void commit(const TrxL1txCall &c, const TrxL1txDev &d, int g, int lane) {
  int ci = 0;
  const int cls = chan_class(c, g, &ci);
  const int m = d.chinfo[g] >> 20;
  const TrxL1txChan &S = d.st[(size_t)c.cur * c.n_all + g];
  TrxL1txChan &N = d.st[(size_t)(c.cur ^ 1) * c.n_all + g];
  long long bf = 0;
  const int nbc = chan_blocks(c, m, &bf);
  const size_t u0 = (size_t)c.unit0[cls] + (size_t)ci * c.nb[cls];
  int L = -1, L2 = -1;                                       // the last two blocks sent in the call
  for (int b0 = 0; b0 < nbc; b0 += 64) {
    const int b = b0 + lane;
    const unsigned long long bal = __ballot(b < nbc && (d.flag[u0 + b] & 1u));
    for (unsigned long long x = bal; x; x &= x - 1) { L2 = L; L = b0 + __ffsll((long long)x) - 1; }
  }
  const uint32_t *lastc = L >= 0 ? d.c + (u0 + L) * 16 : S.last_c;
  const uint32_t *prevc = L >= 0 ? (L2 >= 0 ? d.c + (u0 + L2) * 16 : S.last_c) : S.prev_c;
  uint32_t lv = 0, pv = 0;
  if (lane < 16) { lv = lastc[lane]; pv = prevc[lane]; }
  const uint8_t lf = L >= 0 ? (uint8_t)((d.flag[u0 + L] >> 1) & 1u) : S.last_f;
  const uint8_t pf = L >= 0 ? (L2 >= 0 ? (uint8_t)((d.flag[u0 + L2] >> 1) & 1u) : S.last_f) : S.prev_f;
  const long long pe = c.p_end[m];
  uint8_t pend;
  if (nbc > 0) pend = (L == nbc - 1 && 4 * (bf + L) + 3 >= pe) ? 1 : 0;
  else pend = (S.pend && pe < 4 * bf) ? 1 : 0;
  const long long idle0 = S.pend ? 4 * bf : c.p_first[m];
  const long long sent = pe > idle0 ? pe - idle0 : 0;
  const long long il = (long long)S.idle_left - sent;
  const bool sacch = cls == 1 && is_sacch(m);
  Orders o{ S.ord_pow, S.ord_ta, false };
  if (sacch) o = call_orders(c, d, S, ci, m);
  const uint32_t seen = o.consumed ? d.sib_count[ci] : S.seen;
  __builtin_amdgcn_wave_barrier();
  if (lane < 16) { N.last_c[lane] = lv; N.prev_c[lane] = pv; }
  if (lane == 0) {
    N.last_f = lf; N.prev_f = pf; N.pend = pend; N.active = S.active;
    N.idle_left = il > 0 ? (int32_t)il : 0;
    N.ord_pow = o.pow; N.ord_ta = o.ta; N.seen = seen;
    N.pad[0] = N.pad[1] = N.pad[2] = 0;
  }
}

__global__ __launch_bounds__(256) void k_l1tx_commit(TrxL1txCall c, TrxL1txDev d) {
  const int g = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (g < c.n_all) commit(c, d, g, threadIdx.x & 63);
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
  const long long F8 = 8LL * F;
  if (lane < 4) {
    const int tn = 4 * h + lane;
    SlotW sw{ W_NONE, 0, 0u, 0u, 0ULL, 0ULL };
    const uint32_t *cur = nullptr, *prev = nullptr;
    const int sl = d.slot[a * 8 + tn], comb = sl & 15;
    if (comb) {
      const int cix = comb == 1 ? 0 : comb == 5 ? 1 : 2;
      int r;
      if (comb == 1) { const int t = c.r104 + k; r = t - 104 * (t / 104); }
      else { const int t = c.r102 + k; r = t - 102 * (t / 102); }
      const int m = d.writer[(cix * 8 + tn) * 104 + r];
      if (m == TRX_DL_FCCH) sw.code = W_FCCH;
      else if (m == TRX_DL_SCH) {
        sw.code = W_SCH;
        sch_bits((unsigned)(((long long)c.fn + k) % kTrxHyperframe), (unsigned)c.bsic, &sw.e0, &sw.e1);
      } else if (m >= 0) {
        const int x0 = d.slot_x[a * 8 + tn];
        int g;
        if (m == TRX_MAP_TCHF) g = sl >> 4;
        else if (m < TRX_MAP_SDCCH8) g = x0;
        else if (m < TRX_MAP_SACCH_C8) g = x0 + (m - TRX_MAP_SDCCH8);
        else if (m < TRX_MAP_SDCCH4) g = x0 + 8 + (m - TRX_MAP_SACCH_C8);
        else if (m < TRX_MAP_SACCH_C4) g = x0 + (m - TRX_MAP_SDCCH4);
        else if (m < TRX_DL_CCCH) g = x0 + 4 + (m - TRX_MAP_SACCH_C4);
        else if (m < TRX_DL_BCCH) g = c.n_tch + c.n_xcch + (m - TRX_DL_CCCH);
        else g = c.n_tch + c.n_xcch + c.n_ccch;
        int ci = 0;
        const int cls = chan_class(c, g, &ci);
        const int code = cls == 0 ? W_TCH : cls == 1 ? W_XCCH : cls == 2 ? W_CCCH : W_BCCH;
        const long long q = map_pos(c, d, m, k);
        const long long bf = ceil4(c.p_first[m]);
        const long long rel = (q >> 2) - bf;
        const TrxL1txChan &S = d.st[(size_t)c.cur * c.n_all + g];
        sw.B = (int)(q & 3);
        bool idle_ok = false;
        long long idle0 = c.p_first[m];
        if (rel < 0) {
          if (S.pend) {
            sw.code = code; cur = S.last_c; prev = S.prev_c; sw.curF = S.last_f; sw.prevF = S.prev_f;
          } else idle_ok = true;
        } else {
          const size_t u = (size_t)c.unit0[cls] + (size_t)ci * c.nb[cls] + (size_t)rel;
          const unsigned f = d.flag[u];
          if (f & 1u) {
            sw.code = code; cur = d.c + u * 16; sw.curF = (f >> 1) & 1u;
            if (rel > 0) { prev = d.c + (u - 1) * 16; sw.prevF = (d.flag[u - 1] >> 1) & 1u; }
            else { prev = S.last_c; sw.prevF = S.last_f; }
          } else {
            idle_ok = true;
            if (S.pend) idle0 = 4 * bf;
          }
        }
        if (idle_ok && S.idle_left > 0 && q >= idle0 && q - idle0 < S.idle_left) sw.code = W_IDLE;
      }
    }
    s_w[w][lane] = sw;
    for (int i = 0; i < 16; i++) {
      s_cw[w][lane][i] = cur ? cur[i] : 0u;
      s_cw[w][lane][16 + i] = prev ? prev[i] : 0u;
    }
  }
  wave_fence();
  const uint8_t *tsc = kC.tsc[c.bsic & 7];
  auto cbit = [&](int s, int idx, int half) { return (s_cw[w][s][16 * half + (idx >> 5)] >> (idx & 31)) & 1u; };
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
      case W_BCCH: case W_CCCH: case W_XCCH: case W_TCH: {
        if (pos < 3 || pos >= 145) return 0u;
        const bool tch = sw.code == W_TCH;
        if (pos == 60) return tch ? sw.prevF : 1u;
        if (pos == 87) return tch ? sw.curF : 1u;
        if (pos > 60 && pos < 87) return tsc[pos - 61];
        const int j = pos < 60 ? pos - 3 : pos - 31;
        if (!tch) return cbit(s, kC.xinv[sw.B][j], 0);
        return cbit(s, kTchInv.k[sw.B][j], j & 1);
      }
      default: return 0u;
    }
  };
  const size_t base = ((size_t)a * F8 + 8 * (size_t)k + 4 * h);
  uint8_t *out = d.bits + base * 148;
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
    for (int s = 0; s < 4; s++) v |= (unsigned)s_w[w][s].code << (8 * s);
    *reinterpret_cast<uint32_t *>(d.what + base) = v;
  }
}

__global__ void k_l1tx_set(TrxL1txChan *rec, int open, int sacch, int idle_fill) {
  if (threadIdx.x != 0) return;
  if (open) {
    rec->active = 1; rec->idle_left = 0;
    if (sacch) { rec->ord_pow = 40; rec->ord_ta = 0.0F; }
  } else {
    rec->active = 0; rec->idle_left = idle_fill;
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

namespace {
// a slice's workgroups: 256 * (2^24 - 1) work-items < 2^32 (a dispatch's work-item count), and a grid's y at most 65535
constexpr long long kMaxWg = (1LL << 24) - 1;
constexpr long long kMaxY = 65535;
}

hipError_t trx_launch_l1tx_encode(hipStream_t st, const TrxL1txCall &call, const TrxL1txDev &dv, TrxProfiler *prof) {
  if (call.n_all <= 0) return hipSuccess;
  int nbm = 1;
  for (int i = 0; i < 4; i++) nbm = call.nb[i] > nbm ? call.nb[i] : nbm;
  const long long gx = (call.n_all + 3) / 4;
  long long ys = kMaxWg / gx > 0 ? kMaxWg / gx : 1;          // block rows per slice
  if (ys > kMaxY) ys = kMaxY;
  if (prof) prof->begin(TRXSIG_K_L1TX_ENCODE, st);
  for (long long b0 = 0; b0 < nbm; b0 += ys) {
    const long long ny = nbm - b0 < ys ? nbm - b0 : ys;
    k_l1tx_encode<<<dim3((unsigned)gx, (unsigned)ny), dim3(256), 0, st>>>(call, dv, (int)b0);
  }
  if (prof) prof->end(TRXSIG_K_L1TX_ENCODE, st);
  return hipGetLastError();
}

hipError_t trx_launch_l1tx_mux(hipStream_t st, const TrxL1txCall &call, const TrxL1txDev &dv, TrxProfiler *prof) {
  const long long gx = (2LL * call.n_frames + 3) / 4;
  long long rows = kMaxWg / gx > 0 ? kMaxWg / gx : 1;      // ARFCN rows per slice
  if (rows > kMaxY) rows = kMaxY;
  if (prof) prof->begin(TRXSIG_K_L1TX_MUX, st);
  for (long long a0 = 0; a0 < call.n_arfcn; a0 += rows) {
    const long long na = call.n_arfcn - a0 < rows ? call.n_arfcn - a0 : rows;
    k_l1tx_mux<<<dim3((unsigned)gx, (unsigned)na), dim3(256), 0, st>>>(call, dv, (int)a0);
  }
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
