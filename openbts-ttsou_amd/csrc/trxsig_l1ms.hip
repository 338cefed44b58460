// trxsig_l1ms.hip -- the mobile-side uplink L1's kernels (include/trxsig_l1ms.h, host side in trxsig_l1ms.cpp).  The encode
// half is trxsig_l1tx.hip's, over the uplink mappings and without the beacon and the idle fill.
//
// k_l1ms_encode: a wave per (channel, block b) of the call.  It decides whether the block is sent (open channel; TCH any kind,
//   XCCH kind 1), stages the 23 octets (SACCH: octets 0..1 = the handset's L1 header) and forms c[456] with trxsig_fec_enc.h's
//   tch_form_c.  c[] goes to the scratch packed (16 words), with a flag byte (1 sent, 2 FACCH).  The b = 0 wave of an XCCH
//   channel also writes the handset's power / TA after the call (the call's snapshot: the sibling's orders where there is one).
// k_l1ms_mux: a wave per (ARFCN, frame, half frame): four slots, 592 contiguous output bytes.  Lanes 0..3 find each slot's
//   writer -- the mapping that owns (combination, TN, FN mod 104 / 102) from the host's table, the channel, the position q --
//   and stage its c[] words, or code the access burst of the slot's RACH entry (rach_e36); then 37 lanes gather 16 bytes each
//   through the inverse interleaver and store them at once.  d_who gets the slot's channel (or RACH entry) for the radiate.
// k_l1ms_commit (same stream, after the mux; a wave per channel): each channel's record into the other copy.
// k_l1ms_radiate: a workgroup per slot cell: modulateBurst into LDS, delayVector's 21 taps formed once per burst by the
//   routines trxsig_prim.hip uses, the shifted / filtered sample scaled and written once.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "trxsig_dev.h"
#include "trxsig_fec_enc.h"
#include "trxsig_l1ms_dev.h"

namespace {

__constant__ TrxTdmaMap c_ul[TRX_N_MAPS] = TRX_TDMA_MAPS_INIT;
__constant__ int8_t c_pw[3][32] = TRX_POWER_TABLES_INIT;

// GSM 05.02 5.2.3 training sequences, 5.2.7 access burst (extended tail, synch sequence), and the XCCH inverse interleaver
struct Consts {
  uint8_t tsc[8][26];
  uint8_t acc[49];
  uint16_t xinv[4][114];                     // XCCH: (burst B, e-bit j) -> c index
  constexpr Consts() : tsc(), acc(), xinv() {
    const char *ts[8] = { "00100101110000100010010111", "00101101110111100010110111", "01000011101110100100001110",
                          "01000111101101000100011110", "00011010111001000001101011", "01001110101100000100111010",
                          "10100111110110001010011111", "11101111000100101110111100" };
    for (int t = 0; t < 8; t++)
      for (int i = 0; i < 26; i++) tsc[t][i] = (uint8_t)(ts[t][i] == '1');
    const char *ab = "00111010" "01001011011111111001100110101010001111000";
    for (int i = 0; i < 49; i++) acc[i] = (uint8_t)(ab[i] == '1');
    for (int c = 0; c < 456; c++) xinv[c & 3][2 * ((49 * c) % 57) + ((c % 8) / 4)] = (uint16_t)c;
  }
};
__device__ __constant__ const Consts kC;

enum { W_NONE = 0, W_TCH = 1, W_XCCH = 2, W_ACCESS = 3 };

__device__ __forceinline__ bool is_sacch(int m) {
  return (m >= TRX_MAP_SACCH_TF && m < TRX_MAP_SDCCH8) || (m >= TRX_MAP_SACCH_C8 && m < TRX_MAP_SDCCH4) ||
         (m >= TRX_MAP_SACCH_C4 && m < TRX_MAP_RACH_C5);
}
__device__ __forceinline__ long long ceil4(long long p) { return -((-p) >> 2); }

// the blocks of mapping m whose first burst lies in the call, and the first of them
__device__ __forceinline__ int chan_blocks(const TrxL1msCall &c, int m, long long *blk_first) {
  *blk_first = ceil4(c.p_first[m]);
  const long long nb = ceil4(c.p_end[m]) - *blk_first;
  return nb > 0 ? (int)nb : 0;
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

// the handset of XCCH channel ci during the call: the sibling's current orders as its header decodes them (or the orders the
// followed trxsig_l1msrx decoded from that header), else the record's
struct Phy { int power, ta; };
__device__ Phy call_phy(const TrxL1msCall &c, const TrxL1msDev &d, const TrxL1msChan &S, int ci, bool sacch) {
  if (!sacch) return Phy{ -1, -1 };
  if (!c.has_sib || !S.active) return Phy{ S.power, S.ta };
  if (c.has_sib == 2) return Phy{ c_pw[c.band][encode_power(c.band, d.fol_power[ci])], d.fol_ta[ci] };
  const TrxL1txChan &o = d.sib[ci];
  return Phy{ c_pw[c.band][encode_power(c.band, o.ord_pow)], (int)__fadd_rn(o.ord_ta, 0.5F) };
}

__global__ __launch_bounds__(256) void k_l1ms_encode(TrxL1msCall c, TrxL1msDev d, int b_off) {
  __shared__ uint8_t s_c[4][456], s_u[4][232], s_pls[4][36], s_fr[4][36];
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int g = blockIdx.x * 4 + w, b = (int)blockIdx.y + b_off;
  if (g >= c.n_all) return;                                  // whole waves only: nothing below syncs across waves
  const int cls = g < c.n_tch ? 0 : 1, ci = g - (cls ? c.n_tch : 0);
  const int m = d.chinfo[g] >> 20;
  const TrxL1msChan &S = d.st[(size_t)c.cur * c.n_all + g];
  const bool sacch = cls == 1 && is_sacch(m);
  const Phy ph = call_phy(c, d, S, ci, sacch);
  if (cls == 1 && b == 0 && lane == 0) { d.ms_power[ci] = ph.power; d.ms_ta[ci] = ph.ta; }
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
    else if (d.kind[1][gi] == 1) { send = true; pl = d.payload[1] + gi * 23; }
  }
  if (!send) { if (lane == 0) d.flag[unit] = 0; return; }
  uint8_t *cc = s_c[w];
  if (cls == 0) {
    tch_form_c(kind, pl, d.filler, s_u[w], cc, s_pls[w], lane);
  } else {
    uint8_t *fr = s_fr[w];
    if (lane < 36) {
      uint8_t v = lane < 23 ? pl[lane] : (uint8_t)0;
      if (sacch && lane == 0) v = (uint8_t)(encode_power(c.band, ph.power) & 31);
      if (sacch && lane == 1) v = (uint8_t)ph.ta;
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
  int code, B, who;
  unsigned curF, prevF;
  unsigned long long e;                                      // the access burst's coded bits
};

// position of frame fn + k in mapping m (trxsig_tdma.h: base + n * Q + cnt[rem], Q / rem by the constant repeat length)
__device__ __forceinline__ long long map_pos(const TrxL1msCall &c, const TrxL1msDev &d, int m, int k) {
  const int R = c_ul[m].R;
  int Q, rem;
  switch (R) {
    case 26: { const int t = c.r26 + k; Q = t / 26; rem = t - 26 * Q; break; }
    case 51: { const int t = c.r51 + k; Q = t / 51; rem = t - 51 * Q; break; }
    case 102: { const int t = c.r102 + k; Q = t / 102; rem = t - 102 * Q; break; }
    default: { const int t = c.r104 + k; Q = t / 104; rem = t - 104 * Q; break; }
  }
  return c.base[m] + (long long)c_ul[m].n * Q + d.cnt[m * 105 + rem];
}

// record commit of channel g (one wave)
__global__ __launch_bounds__(256) void k_l1ms_commit(TrxL1msCall c, TrxL1msDev d) {
  const int g = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (g >= c.n_all) return;
  const int cls = g < c.n_tch ? 0 : 1, ci = g - (cls ? c.n_tch : 0);
  const int m = d.chinfo[g] >> 20;
  const TrxL1msChan &S = d.st[(size_t)c.cur * c.n_all + g];
  TrxL1msChan &N = d.st[(size_t)(c.cur ^ 1) * c.n_all + g];
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
  const Phy ph = call_phy(c, d, S, ci, cls == 1 && is_sacch(m));
  __builtin_amdgcn_wave_barrier();
  if (lane < 16) { N.last_c[lane] = lv; N.prev_c[lane] = pv; }
  if (lane == 0) {
    N.last_f = lf; N.prev_f = pf; N.pend = pend; N.active = S.active;
    N.power = ph.power; N.ta = ph.ta;
    for (int i = 0; i < 5; i++) N.pad[i] = 0;
  }
}

__global__ __launch_bounds__(256) void k_l1ms_mux(TrxL1msCall c, TrxL1msDev d, int a_off) {
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
    SlotW sw{ W_NONE, 0, -1, 0u, 0u, 0ULL };
    const uint32_t *cur = nullptr, *prev = nullptr;
    const int sl = d.slot[a * 8 + tn], comb = sl & 15;
    if (comb) {
      const int cix = comb == 1 ? 0 : comb == 5 ? 1 : 2;
      int r;
      if (comb == 1) { const int t = c.r104 + k; r = t - 104 * (t / 104); }
      else { const int t = c.r102 + k; r = t - 102 * (t / 102); }
      const int m = d.writer[(cix * 8 + tn) * 104 + r];
      if (m == TRX_MAP_RACH_C5) {
        const long long j = map_pos(c, d, m, k) - c.p_first[m];
        if (j >= 0 && j < c.n_rach && d.rach_kind[j] == 1) {
          sw.code = W_ACCESS; sw.who = (int)j;
          sw.e = rach_e36(d.rach_ra[j], d.rach_bsic ? (unsigned)(d.rach_bsic[j] & 63u) : (unsigned)c.bsic);
        }
      } else if (m >= 0) {
        const int x0 = d.slot_x[a * 8 + tn];
        int g;
        if (m == TRX_MAP_TCHF) g = sl >> 4;
        else if (m < TRX_MAP_SDCCH8) g = x0;
        else if (m < TRX_MAP_SACCH_C8) g = x0 + (m - TRX_MAP_SDCCH8);
        else if (m < TRX_MAP_SDCCH4) g = x0 + 8 + (m - TRX_MAP_SACCH_C8);
        else if (m < TRX_MAP_SACCH_C4) g = x0 + (m - TRX_MAP_SDCCH4);
        else g = x0 + 4 + (m - TRX_MAP_SACCH_C4);
        const int cls = g < c.n_tch ? 0 : 1, ci = g - (cls ? c.n_tch : 0);
        const int code = cls == 0 ? W_TCH : W_XCCH;
        const long long q = map_pos(c, d, m, k);
        const long long bf = ceil4(c.p_first[m]);
        const long long rel = (q >> 2) - bf;
        const TrxL1msChan &S = d.st[(size_t)c.cur * c.n_all + g];
        sw.B = (int)(q & 3);
        if (rel < 0) {
          if (S.pend) { sw.code = code; cur = S.last_c; prev = S.prev_c; sw.curF = S.last_f; sw.prevF = S.prev_f; }
        } else {
          const size_t u = (size_t)c.unit0[cls] + (size_t)ci * c.nb[cls] + (size_t)rel;
          const unsigned f = d.flag[u];
          if (f & 1u) {
            sw.code = code; cur = d.c + u * 16; sw.curF = (f >> 1) & 1u;
            if (rel > 0) { prev = d.c + (u - 1) * 16; sw.prevF = (d.flag[u - 1] >> 1) & 1u; }
            else { prev = S.last_c; sw.prevF = S.last_f; }
          }
        }
        if (sw.code) sw.who = ci;
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
      case W_ACCESS:
        if (pos < 49) return kC.acc[pos];
        if (pos < 85) return (unsigned)(sw.e >> (pos - 49)) & 1u;
        return 0u;
      case W_XCCH: case W_TCH: {
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
  if (lane < 4) d.who[base + lane] = s_w[w][lane].who;
}

__global__ void k_l1ms_set(TrxL1msChan *rec, int active, int phy, int power, int ta) {
  if (threadIdx.x != 0) return;
  if (active >= 0) rec->active = (uint8_t)active;
  if (phy) { rec->power = power; rec->ta = ta; }
}

// ---------------------------------------------------------------------------------------------
// k_l1ms_radiate: for slot cell (t, a): scaleVector(delayVector(modulateBurst(bits, guard, sps), d), A), the three primitives'
// arithmetic (k_modulate without its gain pass, k_delay_vector, k_elementwise<EW_SCALE>) with the burst held in LDS between
// them.  Workgroup (x, y) takes ARFCN y's slots x, x + gridDim.x, ... (so no launch dimension grows with the call).
// ---------------------------------------------------------------------------------------------
template <int SPS>
__global__ __launch_bounds__(256) void k_l1ms_radiate(const TrxTables *__restrict__ T, TrxL1msAir p) {
  __shared__ float sym[148];
  // the burst with ten zeros before it and zeros from its end to ten past the longest: the 21-tap sum below runs over all its
  // taps without the reference's break (t - j < 0) and skip (t - j >= N).  The terms that adds are +-0 * tap = +-0, and a sum
  // that starts at +0 is never -0 (x + -x and +0 + -0 round to +0), so adding +-0 to it anywhere in the order changes nothing.
  __shared__ cx xs[157 * SPS + 20];
  cx *const x = xs + 10;
  __shared__ float tap[21];
  const int a = blockIdx.y;
  for (long long t = blockIdx.x; t < p.rows; t += gridDim.x) {
    const int guard = 8 + ((t & 3) == 0);                    // TN % 4 == 0: t = 8 k + TN
    const int N = SPS * (148 + guard);
    const size_t s = (size_t)a * p.rows + t;
    cx *o = p.out + t * p.slot_stride + a * p.arfcn_stride;
    const int w = p.what[s];
    if (w == W_NONE) {
      for (int k = threadIdx.x; k < N; k += 256) o[k] = mk(0, 0);
      continue;
    }
    const int who = p.who[s];
    const int cls = w - 1;                                   // W_TCH, W_XCCH, W_ACCESS -> the air's arrays
    const cx gain = p.gain[cls][who];
    float d, sc;
    if (w == W_ACCESS) {
      d = p.delay[cls][who] * (float)SPS;
      sc = 1.0F;
    } else {
      const int hs = p.handset[(w == W_TCH ? 0 : p.n_tch) + who];
      d = (p.delay[cls][who] - (float)p.ms_ta[hs]) * (float)SPS;
      sc = p.amp_of_power[p.ms_power[hs]];
    }
    const cx A = mk(gain.r * sc, gain.i * sc);
    __syncthreads();                                         // the previous cell's readers of sym / x / tap are done
    for (int i = threadIdx.x; i < 148; i += 256) sym[i] = (float)(2.0 * (p.bits[s * 148 + i] & 0x01) - 1.0);
    for (int i = threadIdx.x; i < 157 * SPS + 20; i += 256)
      if (i < 10 || i >= 10 + N) xs[i] = mk(0, 0);
    const bool refused = !(fabsf(d) <= TRXSIG_MAX_INDEX);    // k_delay_vector: zeros
    const int io = (int)floorf(d);                           // sigProcLib.cpp:577
    const float frac = d - (float)io;                        // :578
    const bool filt = fabs((double)frac) > 1e-2;             // :582
    if (threadIdx.x < 21) tap[threadIdx.x] = dev_sinc(T->sinT, TRX_PI_F * ((float)((int)threadIdx.x - 10) - frac));   // :588
    __syncthreads();
    for (int n0 = threadIdx.x; n0 < N; n0 += 256) {          // k_modulate's sample(), no gain
      cx sum = mk(0, 0);
#pragma unroll
      for (int q = 0; q < 3; q++) {
        const int j = (n0 % SPS) + q * SPS;
        const int n = n0 + SPS - j;
        if (j <= 2 * SPS && n >= 0 && n < N && n / SPS < 148) {
          const cx av = cmulr(T->rot[n], sym[n / SPS]);
          sum = cadd(sum, cmulr(av, T->pulse[j]));
        }
      }
      x[n0] = sum;
    }
    __syncthreads();
    float tp[21];
#pragma unroll
    for (int j = 0; j < 21; j++) tp[j] = tap[j];
    for (int k = threadIdx.x; k < N; k += 256) {
      const int tt = k - io;
      cx r = mk(0, 0);
      if (!refused && tt >= 0 && tt < N) {
        if (filt) {
#pragma unroll
          for (int j = 0; j < 21; j++) r = cadd(r, cmulr(x[tt + 10 - j], tp[j]));   // convolve(.., NO_DELAY): start 10, j ascending
        } else {
          r = x[tt];
        }
      }
      o[k] = cmul(r, A);                                     // scaleVector (:719)
    }
  }
}

// a slice's workgroups: 256 * (2^24 - 1) work-items < 2^32 (a dispatch's work-item count), and a grid's y at most 65535
constexpr long long kMaxWg = (1LL << 24) - 1;
constexpr long long kMaxY = 65535;
constexpr long long kRadiateWg = 16384;                      // 64 workgroups per CU: the slots beyond go round the loop

}  // namespace

hipError_t trx_launch_l1ms_encode(hipStream_t st, const TrxL1msCall &call, const TrxL1msDev &dv) {
  if (call.n_all <= 0) return hipSuccess;
  int nbm = 1;
  for (int i = 0; i < 2; i++) nbm = call.nb[i] > nbm ? call.nb[i] : nbm;
  const long long gx = (call.n_all + 3) / 4;
  long long ys = kMaxWg / gx > 0 ? kMaxWg / gx : 1;          // block rows per slice
  if (ys > kMaxY) ys = kMaxY;
  for (long long b0 = 0; b0 < nbm; b0 += ys) {
    const long long ny = nbm - b0 < ys ? nbm - b0 : ys;
    k_l1ms_encode<<<dim3((unsigned)gx, (unsigned)ny), dim3(256), 0, st>>>(call, dv, (int)b0);
  }
  return hipGetLastError();
}

hipError_t trx_launch_l1ms_mux(hipStream_t st, const TrxL1msCall &call, const TrxL1msDev &dv) {
  const long long gx = (2LL * call.n_frames + 3) / 4;
  long long rows = kMaxWg / gx > 0 ? kMaxWg / gx : 1;      // ARFCN rows per slice
  if (rows > kMaxY) rows = kMaxY;
  for (long long a0 = 0; a0 < call.n_arfcn; a0 += rows) {
    const long long na = call.n_arfcn - a0 < rows ? call.n_arfcn - a0 : rows;
    k_l1ms_mux<<<dim3((unsigned)gx, (unsigned)na), dim3(256), 0, st>>>(call, dv, (int)a0);
  }
  if (call.n_all > 0) k_l1ms_commit<<<dim3((unsigned)((call.n_all + 3) / 4)), dim3(256), 0, st>>>(call, dv);
  return hipGetLastError();
}

hipError_t trx_launch_l1ms_set(hipStream_t st, TrxL1msChan *rec, int active, int phy, int power, int ta) {
  k_l1ms_set<<<dim3(1), dim3(64), 0, st>>>(rec, active, phy, power, ta);
  return hipGetLastError();
}

hipError_t trx_launch_l1ms_radiate(hipStream_t st, int sps, const TrxTables *dT, const TrxL1msAir &air) {
  if (air.rows <= 0 || air.n_arfcn <= 0 || air.n_arfcn > kMaxY) return hipSuccess;
  long long gx = kRadiateWg / air.n_arfcn > 0 ? kRadiateWg / air.n_arfcn : 1;
  if (gx > air.rows) gx = air.rows;
  const dim3 grid((unsigned)gx, (unsigned)air.n_arfcn), block(256);
  switch (sps) {
    case 1: k_l1ms_radiate<1><<<grid, block, 0, st>>>(dT, air); break;
    case 2: k_l1ms_radiate<2><<<grid, block, 0, st>>>(dT, air); break;
    case 4: k_l1ms_radiate<4><<<grid, block, 0, st>>>(dT, air); break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}
