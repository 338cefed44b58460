// trxsig_l1ms.hip -- the mobile-side uplink L1's kernels (include/trxsig_l1ms.h, host side in trxsig_l1ms.cpp).  What the
// uplink multiplexer has in common with the base-station side's downlink one (trxsig_l1tx.hip) -- the block encoder's tail, the
// slot writer's block lookup and normal-burst gather, the commit's head -- is trxsig_l1mux_dev.h; here are the kernels and the
// uplink's own part: the handsets' power / TA, the access burst and the slot's sender (who), and the radiate.
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
#include "trxsig_dev.h"
#include "trxsig_l1ms_dev.h"
#include "trxsig_l1mux_dev.h"

namespace {

__constant__ TrxTdmaMap c_ul[TRX_N_MAPS] = TRX_TDMA_MAPS_INIT;
__constant__ int8_t c_pw[3][32] = TRX_POWER_TABLES_INIT;

// GSM 05.02 5.2.7 access burst: extended tail, synch sequence
struct Consts {
  uint8_t acc[49];
  constexpr Consts() : acc() {
    const char *ab = "00111010" "01001011011111111001100110101010001111000";
    for (int i = 0; i < 49; i++) acc[i] = (uint8_t)(ab[i] == '1');
  }
};
__device__ __constant__ const Consts kC;

enum { W_NONE = 0, W_TCH = 1, W_XCCH = 2, W_ACCESS = 3 };

// the handset of XCCH channel ci during the call: the sibling's current orders as its header decodes them (or the orders the
// followed trxsig_l1msrx decoded from that header), else the record's
struct Phy { int power, ta; };
__device__ Phy call_phy(const TrxL1msCall &c, const TrxL1msDev &d, const TrxL1msChan &S, int ci, bool sacch) {
  if (!sacch) return Phy{ -1, -1 };
  if (!c.has_sib || !S.h.active) return Phy{ S.power, S.ta };
  const int8_t *pw = c_pw[c.band];
  if (c.has_sib == 2) return Phy{ pw[trx_encode_power(pw, d.fol_power[ci])], d.fol_ta[ci] };
  const TrxL1txChan &o = d.sib[ci];
  return Phy{ pw[trx_encode_power(pw, o.ord_pow)], (int)__fadd_rn(o.ord_ta, 0.5F) };
}

__global__ __launch_bounds__(256) void k_l1ms_encode(TrxL1msCall c, TrxL1msDev d, int b_off) {
  __shared__ uint8_t s_c[4][456], s_u[4][232], s_pls[4][36], s_fr[4][36];
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int g = blockIdx.x * 4 + w, b = (int)blockIdx.y + b_off;
  if (g >= c.n_all) return;                                  // whole waves only: nothing below syncs across waves
  const int cls = g < c.n_tch ? 0 : 1, ci = g - (cls ? c.n_tch : 0);
  const int m = d.chinfo[g] >> 20;
  const TrxL1msChan &S = d.st[(size_t)c.cur * c.n_all + g];
  const bool sacch = cls == 1 && trx_map_is_sacch(m);
  const Phy ph = call_phy(c, d, S, ci, sacch);
  if (cls == 1 && b == 0 && lane == 0) { d.ms_power[ci] = ph.power; d.ms_ta[ci] = ph.ta; }
  const int nbk = c.nb[cls];
  if (b >= nbk) return;
  long long bf = 0;
  const int nbc = mux_chan_blocks(c, m, &bf);
  const size_t unit = (size_t)c.unit0[cls] + (size_t)ci * nbk + b;
  int kind = 0;
  const uint8_t *pl = nullptr;
  const bool send = b < nbc && S.h.active && mux_grid_block(d, cls, (size_t)ci * nbk + b, &kind, &pl);
  auto hdr = [&](int i) { return (uint8_t)(i == 0 ? trx_encode_power(c_pw[c.band], ph.power) & 31 : ph.ta); };
  mux_encode_block(send, pl, cls == 0, kind, sacch, hdr, d.filler, d.c + unit * 16, d.flag + unit, s_c[w], s_u[w], s_pls[w],
                   s_fr[w], lane);
}

struct SlotW {
  int code, B, who;
  unsigned curF, prevF;
  unsigned long long e;                                      // the access burst's coded bits
};

// record commit: a wave per channel
__global__ __launch_bounds__(256) void k_l1ms_commit(TrxL1msCall c, TrxL1msDev d) {
  const int g = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (g >= c.n_all) return;
  const int cls = g < c.n_tch ? 0 : 1, ci = g - (cls ? c.n_tch : 0);
  const int m = d.chinfo[g] >> 20;
  const TrxL1msChan &S = d.st[(size_t)c.cur * c.n_all + g];
  TrxL1msChan &N = d.st[(size_t)(c.cur ^ 1) * c.n_all + g];
  const MuxCommit k = mux_commit_read(c, d, S.h, cls, ci, m, lane);
  const Phy ph = call_phy(c, d, S, ci, cls == 1 && trx_map_is_sacch(m));
  mux_commit_write(N.h, k, S.h.active, lane);
  if (lane == 0) {
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
  if (lane < 4) {
    const int tn = 4 * h + lane;
    SlotW sw{ W_NONE, 0, -1, 0u, 0u, 0ULL };
    const uint32_t *cur = nullptr, *prev = nullptr;
    const int sl = d.slot[a * 8 + tn];
    const int m = mux_slot_owner(c, d, sl, tn, k);
    if (m == TRX_MAP_RACH_C5) {
      const long long j = mux_map_pos(c, d, c_ul[m], m, k) - c.p_first[m];
      if (j >= 0 && j < c.n_rach && d.rach_kind[j] == 1) {
        sw.code = W_ACCESS; sw.who = (int)j;
        sw.e = rach_e36(d.rach_ra[j], d.rach_bsic ? (unsigned)(d.rach_bsic[j] & 63u) : (unsigned)c.bsic);
      }
    } else if (m >= 0) {
      const int g = mux_slot_chan(m, sl, d.slot_x[a * 8 + tn]);
      const int cls = g < c.n_tch ? 0 : 1, ci = g - (cls ? c.n_tch : 0);
      const MuxBlock blk = mux_block(c, d, c_ul[m], d.st[(size_t)c.cur * c.n_all + g].h, cls, ci, m, k);
      sw.B = blk.B;
      if (blk.cur) {
        sw.code = cls == 0 ? W_TCH : W_XCCH; sw.who = ci;
        cur = blk.cur; prev = blk.prev; sw.curF = blk.curF; sw.prevF = blk.prevF;
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
      case W_ACCESS:
        if (pos < 49) return kC.acc[pos];
        if (pos < 85) return (unsigned)(sw.e >> (pos - 49)) & 1u;
        return 0u;
      case W_XCCH: case W_TCH:
        return mux_normal_bit(s_cw[w][s], sw.B, sw.curF, sw.prevF, sw.code == W_TCH, tsc, pos);
      default: return 0u;
    }
  };
  const size_t base = (size_t)a * (8LL * F) + 8 * (size_t)k + 4 * h;
  mux_store(d.bits, d.what, base, lane, obyte, [&](int s) { return s_w[w][s].code; });
  if (lane < 4) d.who[base + lane] = s_w[w][lane].who;
}

__global__ void k_l1ms_set(TrxL1msChan *rec, int active, int phy, int power, int ta) {
  if (threadIdx.x != 0) return;
  if (active >= 0) rec->h.active = (uint8_t)active;
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

constexpr long long kRadiateWg = 16384;                      // 64 workgroups per CU: the slots beyond go round the loop

}  // namespace

hipError_t trx_launch_l1ms_encode(hipStream_t st, const TrxL1msCall &call, const TrxL1msDev &dv) {
  if (call.n_all <= 0) return hipSuccess;
  int nbm = 1;
  for (int i = 0; i < 2; i++) nbm = call.nb[i] > nbm ? call.nb[i] : nbm;
  mux_launch_slices((call.n_all + 3) / 4, nbm, [&](dim3 grid, int b0) { k_l1ms_encode<<<grid, dim3(256), 0, st>>>(call, dv, b0); });
  return hipGetLastError();
}

hipError_t trx_launch_l1ms_mux(hipStream_t st, const TrxL1msCall &call, const TrxL1msDev &dv) {
  mux_launch_slices((2LL * call.n_frames + 3) / 4, call.n_arfcn,
                    [&](dim3 grid, int a0) { k_l1ms_mux<<<grid, dim3(256), 0, st>>>(call, dv, a0); });
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
