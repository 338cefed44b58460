// trxsig_fec.hip -- gfx950 kernel of the GSM L1 FEC soft decode that consumes the burst path's soft
// bits: SoftVector::decode with the rate-1/2, order-4 Viterbi coder
// (CommonLibs/BitVector.cpp:290-524, "bv:"), the Parity/Generator shift registers
// (CommonLibs/BitVector.h:39-112, "bh:"), LSB8MSB + pack (bv:166-195, 541-552) and the XCCH / RACH
// decoder flows (GSM/GSML1FEC.cpp:475-514, 584-653, "fec:"), optionally with the UDP hop's 8-bit
// quantisation in between (Transceiver/Transceiver.cpp:669, TRXManager/TRXManager.cpp:231).
//
// Decomposition: the decoder has 16 survivors, so one block (code word) takes 16 lanes -- lane s IS
// survivor s -- and a wave decodes four blocks.  Measured (MI355X, 16 K XCCH blocks = 64 K bursts):
// 102 us; it is bound by the ~50-instruction dependent chain of a trellis step (4 waves per SIMD), not
// by memory -- the first version, whose whole-block metric table left 2.5 waves per SIMD, took 217 us.  Per trellis step a lane fetches its two predecessors
// (survivors s>>1 and 8 + s>>1: ds_bpermute), adds the branch costs and keeps the cheaper one; the
// first-minimum survivor (bv:382-393) is found with four DPP min exchanges + a ballot and its deferred
// input bit (24 steps back) is the output.  Numerical contract as in trxsig_dev.h: float costs are added
// exactly as the reference adds them (cost + (second-bit cost + first-bit cost), -ffp-contract=off),
// so survivor selection, ties included, is bit-identical.
// The downlink encoders live here too: k_fec_xcch_encode, k_fec_tch_encode (TCH/FS + FACCH/F streams), k_fec_sch_encode; and
// the multi-channel uplink stream decoders k_fec_rx_stream + k_fec_rx_fold (TCH/FACCH and XCCH, mI[][] carried on the device).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "trxsig_fec_enc.h"
#include "trxsig_launch.h"
#include "trxsig_sch_dec.h"

namespace {

constexpr int kDeferral = 24;                              // 6*mOrder (bh:138)
constexpr int kChunk = 64;                                 // trellis steps per table refill (8 positions per lane)


// The syndrome / parity registers are linear over GF(2) (they start from zero), so the word for a
// bit string is the XOR of the words of its set bits.  XcchSyn::v[i] = syndromeShift response
// (bh:69-74) to a single 1 at position i of a 224-bit code word, generator 0x10004820009 (40 bits);
// RachPar::v[i] = encoderShift response (bh:80-85) to a single 1 at position i of 8 bits, generator 0x6f.
struct XcchSyn {
  unsigned long long v[224];
  constexpr XcchSyn() : v() {
    unsigned long long st = 1;                             // the bit has just been shifted in
    for (int i = 223; i >= 0; i--) {
      v[i] = st & ((1ULL << 40) - 1);
      const unsigned long long fb = (st >> 39) & 1ULL;     // one more zero shifted in behind it
      st <<= 1;
      if (fb) st ^= 0x10004820009ULL;
    }
  }
};
struct RachPar {
  unsigned v[8];
  constexpr RachPar() : v() {
    for (int i = 0; i < 8; i++) {
      unsigned st = 0;
      for (int k = 0; k < 8; k++) {
        const unsigned fb = ((st >> 5) ^ (k == i ? 1u : 0u)) & 1u;
        st <<= 1;
        if (fb) st ^= 0x6fu;
      }
      v[i] = st & 0x3fu;
    }
  }
};
__device__ __constant__ const XcchSyn kXcchSyn;
__device__ __constant__ const RachPar kRachPar;

template <int CTRL>
__device__ __forceinline__ int dpp_i(int v) { return __builtin_amdgcn_update_dpp(0, v, CTRL, 0xf, 0xf, true); }
template <int CTRL>
__device__ __forceinline__ float dpp_f(float v) { return __int_as_float(dpp_i<CTRL>(__float_as_int(v))); }


// the soft value as the GSM side sees it after the UDP hop
__device__ __forceinline__ float wire_value(float v) {
  const int q = (int)round((double)v * 255.0);             // (char) round(x*255.0), Transceiver.cpp:669
  return (float)(unsigned char)q / 256.0F;                 // TRXManager.cpp:231
}

enum { FEC_GENERIC = 0, FEC_XCCH = 1, FEC_RACH = 2, FEC_TCH = 3, FEC_SCH = TRX_FEC_MODE_SCH };

// The trellis of SoftVector::decode (bv:334-399, metric tables bv:462-485) for the code word of this lane's 16-lane row:
// lane s IS survivor s.  fetch(p) loads soft value p of the row's code word (called for p < n of a live row, eight loads
// issued together per table refill) and finish(v, p) turns the loaded value into the one the decoder sees.  `steps`
// (wave-uniform) is at least nout + kDeferral of every row; a row that runs past its own end sees unknowns (0.5) there,
// which changes none of its first nout output bits.  tab: the row's kChunk-entry LDS table.  Returns lane s's output
// bits 32s .. 32s+31.
template <class Fetch, class Finish>
__device__ __forceinline__ unsigned fec_trellis(float4 *tab, int n, int steps, bool live, int lane, Fetch fetch, Finish finish) {
  const int s = lane & 15;
  float2 *K2 = reinterpret_cast<float2 *>(tab);
  const float4 *K = tab;
  float cost = 0.0f;                                       // lane s is survivor s (bv:334-399)
  unsigned ist = 0, outw = 0;
  const int srcA = (lane & 48) + (s >> 1), srcB = srcA + 8;
  for (int c0 = 0; c0 < steps; c0 += kChunk) {
    // ---- metric tables (bv:462-485) for steps c0 .. c0+kChunk-1: positions 2*c0 .. 2*c0 + 2*kChunk - 1,
    //      eight per lane, their loads issued together ----
    float vv[8];
#pragma unroll
    for (int q = 0; q < 8; q++) {
      const int p = 2 * c0 + s + 16 * q;
      float v = 0.0f;
      if (p < n && live) v = fetch(p);
      vv[q] = v;
    }
#pragma unroll
    for (int q = 0; q < 8; q++) {
      const int p = 2 * c0 + s + 16 * q;
      float k0 = 0.5F, k1 = 0.5F;                          // past the data: unknowns (bv:481-484)
      if (p < n && live) {
        const float v = finish(vv[q], p);
        const bool hard = v > 0.5F;                        // sliced() (bv:424-433)
        float pVal = v;
        if (pVal > 0.5F) pVal = 1.0F - pVal;
        float ipVal = 1.0F - pVal;
        if (pVal < 0.01F) pVal = (float)0.01;
        if (ipVal < 0.01F) ipVal = (float)0.01;
        const float match = 0.25F / ipVal, mismatch = 0.25F / pVal;
        k0 = hard ? mismatch : match;                      // coder bit 0 mismatches a received 1
        k1 = hard ? match : mismatch;
      }
      K2[s + 16 * q] = make_float2(k0, k1);
    }
    wave_fence();

    // ---- kChunk trellis steps ----
    const int tend = (c0 + kChunk < steps) ? c0 + kChunk : steps;
    for (int t = c0; t < tend; t++) {
      const float4 k = K[t - c0];                          // {first bit: cost of coder 0, 1; second bit: cost of coder 0, 1}
      const float cA0 = __shfl(cost, srcA, 64), cB0 = __shfl(cost, srcB, 64);
      const unsigned iA = (__shfl(ist, srcA, 64) << 1) | (s & 1), iB = (__shfl(ist, srcB, 64) << 1) | (s & 1);
      const unsigned gA = (unsigned)(kGen >> (2 * (iA & 31))) & 3u, gB = (unsigned)(kGen >> (2 * (iB & 31))) & 3u;
      // cost += cTab[m&1][1] + cTab[(m>>1)&1][0] (bv:365)
      const float cA = cA0 + (((gA & 1u) ? k.w : k.z) + ((gA >> 1) ? k.y : k.x));
      const float cB = cB0 + (((gB & 1u) ? k.w : k.z) + ((gB >> 1) ? k.y : k.x));
      const bool takeA = cA < cB;                          // pruneCandidates (bv:371-379)
      cost = takeA ? cA : cB;
      ist = takeA ? iA : iB;
      if (t >= kDeferral) {
        // minCost (bv:382-393): the FIRST survivor with the minimum cost.  The minimum itself by four DPP
        // exchanges; the lanes that hold it by ballot; the first of them = lowest set bit of the row's mask.
        // NaN costs: a step's branch costs are shared by all 16 survivors, a NaN soft value makes both costs of
        // its bit NaN (match and mismatch both derive from it) and every candidate adds one of the two; no other
        // input gives a NaN (costs lie in [0, 25], at most 2 * 536 of them are summed).  So either all 16 costs
        // of a row are NaN -- from the NaN's step on, NaN being absorbing -- or none is.  With all NaN the
        // reference's scan skips no survivor (`thisCost >= minCost` is false, bv:388) and ends on survivor 15;
        // here fminf gives NaN, no lane equals it and the row's mask is 0.  Bit 15 ORed in makes ctz answer 15
        // then, changes nothing when a lower bit is set, and keeps mi inside the row.
        float mc = cost;
        mc = fminf(mc, dpp_f<0xB1>(mc));                   // quad_perm [1,0,3,2]
        mc = fminf(mc, dpp_f<0x4E>(mc));                   // quad_perm [2,3,0,1]
        mc = fminf(mc, dpp_f<0x141>(mc));                  // row_half_mirror
        mc = fminf(mc, dpp_f<0x140>(mc));                  // row_mirror
        const unsigned long long eq = __builtin_amdgcn_ballot_w64(cost == mc);
        const unsigned long long ob = __builtin_amdgcn_ballot_w64((ist >> kDeferral) & 1u);
        const unsigned rowmask = (unsigned)(eq >> (lane & 48)) & 0xFFFFu;
        const int mi = __builtin_ctz(rowmask | 0x8000u);
        const int op = t - kDeferral;
        const unsigned bit = (unsigned)(ob >> ((lane & 48) + mi)) & 1u;
        if ((op >> 5) == s) outw |= bit << (op & 31);      // lane s collects output bits 32s .. 32s+31
      }
    }
    wave_fence();                                          // table reads done before the next chunk overwrites it
  }
  return outw;
}

// XCCHL1Decoder::decode after the trellis (fec:598, 644-651) for the row of lane s, whose output word is outw: the 23 L2
// octets to out23 and the parity verdict (every lane of the row returns it).  The whole row must be active.
__device__ __forceinline__ bool xcch_finish(unsigned outw, int s, uint8_t *__restrict__ out23) {
  // d[] = u[0..184) with every octet bit-reversed (LSB8MSB, fec:598) and packed MSB first: octet o is
  // u[8o .. 8o+7] with u[8o] as its LSB, i.e. the bytes of the output words as they stand
  for (int q = 0; q < 4; q++)
    if (4 * s + q < 23) out23[4 * s + q] = (uint8_t)(outw >> (8 * q));
  // syndrome of d[]:~p[] (fec:644-651): XOR of the unit responses of the set bits
  unsigned w = outw;
  if (s == 5) w ^= 0xFF000000u;                            // parity bits 184..223 are inverted
  if (s == 6) w ^= 0xFFFFFFFFu;
  unsigned long long syn = 0;
  if (s < 7) {
    for (int k = 0; k < 32; k++) {
      const unsigned long long r = kXcchSyn.v[32 * s + k];
      if ((w >> k) & 1u) syn ^= r;
    }
  }
  unsigned lo = (unsigned)syn, hi = (unsigned)(syn >> 32);
  lo ^= (unsigned)dpp_i<0xB1>((int)lo); hi ^= (unsigned)dpp_i<0xB1>((int)hi);
  lo ^= (unsigned)dpp_i<0x4E>((int)lo); hi ^= (unsigned)dpp_i<0x4E>((int)hi);
  lo ^= (unsigned)dpp_i<0x141>((int)lo); hi ^= (unsigned)dpp_i<0x141>((int)hi);
  lo ^= (unsigned)dpp_i<0x140>((int)lo); hi ^= (unsigned)dpp_i<0x140>((int)hi);
  return (lo | hi) == 0;
}

// decodeTCH(false) after the trellis (fec:1133-1163): uw = u[189] in LDS (word w = bits 32w..32w+31, visible to the row),
// cbit(k) = c[k] sliced for class 2 (k >= 378).  Writes d[260] packed MSB first (33 octets) to out33; lane s == 0 returns
// `good` (parity of class 1a and the tail bits), the other lanes false.
template <class CBit>
__device__ __forceinline__ bool tch_finish(const unsigned *uw, int s, CBit cbit, uint8_t *__restrict__ out33) {
  auto ubit = [&](int i) { return (uw[i >> 5] >> (i & 31)) & 1u; };
  auto dbit = [&](int q) -> unsigned {
    if (q >= 260) return 0u;
    if (q >= 182) return cbit(378 + q - 182);
    const int k = q >> 1;
    return (q & 1) ? ubit(184 - k) : ubit(k);
  };
  for (int o = s; o < 33; o += 16) {
    unsigned byte = 0;
    for (int q = 0; q < 8; q++) byte = (byte << 1) | dbit(8 * o + q);
    out33[o] = (uint8_t)byte;
  }
  bool good = false;
  if (s == 0) {
    unsigned calc = 0;
    for (int i = 0; i < 50; i++) if (dbit(i)) calc ^= kTchPar.v[i];
    const unsigned sent = (~((ubit(91) << 2) | (ubit(92) << 1) | ubit(93))) & 7u;      // peekField(91,3)
    const unsigned tail = ubit(185) | ubit(186) | ubit(187) | ubit(188);
    good = (sent == calc) && (tail == 0);
  }
  return good;
}

// MODE FEC_GENERIC: block b reads soft[b*in_stride + p], p < n, and writes nout bits as bytes to out0 + b*out_stride.
// MODE FEC_XCCH   : block b = bursts 4b..4b+3 of soft[burst*in_stride + 0..147]; c[k] = i[k%4][j(k)] with the
//                   e-bits at 3..59 and 88..144 (fec:607-608, 618-629); out0 = 23 octets per block, out1 = ok.
// MODE FEC_RACH   : block b = burst b, e = burst[49..85) (fec:479); out0 = tail ok, out1 = BSIC, out2 = RA.
// MODE FEC_TCH    : block b = bursts 4b..4b+7 (diagonal deinterleaver, fec:1108-1116), class 1 = c[0..378) decoded,
//                   class 2 = c[378..456) sliced (fec:1133-1163); out0 = d[260] packed MSB first (33 octets),
//                   out1 = good (parity of class 1a and tail), out2 = stolen (Hl of the block's last burst, fec:1077).
// MODE FEC_SCH    : block b = burst b, e = burst[3..42) + burst[106..145) (the inverse of trxsig_fec_sch_encode_batch); out0 = ok,
//                   out1 = BSIC, out2 = the decoded frame number as int32 (trx_sch_verdict, trxsig_sch_dec.h).
// ilv8 (FEC_XCCH only): read c[] through the TCH deinterleaver instead -- the FACCH decode of a stolen block.
template <int MODE>
__global__ __launch_bounds__(64) void k_fec_viterbi(const float *__restrict__ soft, long long in_stride, int n, int nout,
                                                    int nblk, int wire, int ilv8, uint8_t *__restrict__ out0,
                                                    uint8_t *__restrict__ out1, uint8_t *__restrict__ out2,
                                                    long long out_stride) {
  // costs of coder bit 0/1 for both bits of a step, kChunk steps at a time: a small table keeps 8 waves
  // per SIMD resident (the whole 252-step table of an XCCH block would be 4 KB per block: 2.5 waves)
  __shared__ float4 ktab[4][kChunk];
  const int lane = threadIdx.x & 63, row = lane >> 4, s = lane & 15;
  const int blk = blockIdx.x * 4 + row;
  const bool live = blk < nblk;
  auto fetch = [&](int p) -> float {
    if (MODE == FEC_XCCH || MODE == FEC_TCH) {
      const int B = (MODE == FEC_TCH || ilv8) ? (p & 7) : (p & 3);      // burst within the block
      const int j = 2 * ((49 * p) % 57) + ((p % 8) / 4);                // GSM 05.03 4.1.4 / 3.1.3 (fec:622-625, 1111)
      return soft[(size_t)(4 * blk + B) * in_stride + (j < 57 ? 3 + j : 88 + (j - 57))];
    } else if (MODE == FEC_RACH) {
      return soft[(size_t)blk * in_stride + 49 + p];
    } else if (MODE == FEC_SCH) {
      return soft[(size_t)blk * in_stride + (p < 39 ? 3 + p : 106 + (p - 39))];
    } else {
      return soft[(size_t)blk * in_stride + p];
    }
  };
  auto finish = [&](float v, int) -> float { return wire ? wire_value(v) : v; };
  const unsigned outw = fec_trellis(ktab[row], n, nout + kDeferral, live, lane, fetch, finish);
  if (MODE == FEC_SCH) {                                   // u[39]: bits 0..31 in the row's lane 0, 32..38 in its lane 1
    const unsigned lo = __shfl(outw, 16 * row, 64), hi = __shfl(outw, 16 * row + 1, 64);
    if (live && s == 0) {
      unsigned ok, bsic;
      int rfn;
      trx_sch_verdict([&](int q) -> unsigned { return q < 32 ? (lo >> q) & 1u : (hi >> (q - 32)) & 1u; }, &ok, &bsic, &rfn);
      out0[blk] = (uint8_t)ok;
      out1[blk] = (uint8_t)bsic;
      reinterpret_cast<int32_t *>(out2)[blk] = rfn;
    }
    return;
  }
  if (!live) return;

  if (MODE == FEC_GENERIC) {
    for (int k = 0; k < 32; k++) {
      const int i = 32 * s + k;
      if (i < nout) out0[(size_t)blk * out_stride + i] = (uint8_t)((outw >> k) & 1u);
    }
  } else if (MODE == FEC_XCCH) {
    const bool ok = xcch_finish(outw, s, out0 + (size_t)blk * 23);
    if (s == 0) out1[blk] = ok;
  } else if (MODE == FEC_TCH) {
    // u[189] -> LDS (word w = bits 32w..32w+31), then d[] (fec:1141-1146) octet by octet
    unsigned *uw = reinterpret_cast<unsigned *>(ktab[row]);
    if (s < 6) uw[s] = outw;
    wave_fence();
    auto cbit = [&](int k) {                               // class 2: c[k] sliced, k >= 378
      const int j = 2 * ((49 * k) % 57) + ((k % 8) / 4);
      float v = soft[(size_t)(4 * blk + (k & 7)) * in_stride + (j < 57 ? 3 + j : 88 + (j - 57))];
      if (wire) v = wire_value(v);
      return v > 0.5F ? 1u : 0u;
    };
    const bool good = tch_finish(uw, s, cbit, out0 + (size_t)blk * 33);
    if (s == 0) {
      out1[blk] = good;
      float hl = soft[(size_t)(4 * blk + 7) * in_stride + 60];
      if (wire) hl = wire_value(hl);
      out2[blk] = hl > 0.5F;
    }
  } else {
    if (s == 0) {
      const unsigned u = outw;                             // bit k = u[k]
      const bool tail_ok = ((u >> 14) & 0xFu) == 0;        // fec:485
      unsigned sent = 0, chk = 0;
      for (int k = 0; k < 6; k++) sent |= ((u >> (8 + k)) & 1u) << (5 - k);     // peekField(8,6), MSB first
      for (int i = 0; i < 8; i++) if ((u >> i) & 1u) chk ^= kRachPar.v[i];
      out0[blk] = tail_ok;
      out1[blk] = (uint8_t)((~sent ^ chk) & 0x3fu);        // fec:490-493
      out2[blk] = (uint8_t)(u & 0xFFu);                    // RA = d[] after LSB8MSB, MSB first (fec:506-507)
    }
  }
}

// ---------------------------------------------------------------------------------------------
// k_fec_xcch_encode: XCCHL1Encoder::sendFrame / encode / interleave / transmit (fec:772-845), one wave per L2
// frame: d[] = the 23 octets LSB first (LSB8MSB, fec:789), 40 parity bits = ~(Fire-code remainder of d[])
// (writeParityWord, bv:409-416), four zero tail bits, rate-1/2 coder (BitVector::encode, bv:217-239),
// GSM 05.03 4.1.4 interleaver into the e-bits of four bursts, plus what the encoder's constructor puts in
// every burst: zero tails, both stealing flags set (fec:713-717) and the training sequence at 61..86.
// All integer work; the parity word uses the register's GF(2) linearity (XOR of unit responses).
// ---------------------------------------------------------------------------------------------

__global__ __launch_bounds__(64) void k_fec_xcch_encode(const uint8_t *__restrict__ frames, int nblk,
                                                        const uint8_t *__restrict__ tsc_bits /* 26 */, uint8_t *__restrict__ bits) {
  __shared__ unsigned uw[8];                                // u[228], bit k of word w = u[32w + k]
  const int lane = threadIdx.x, blk = blockIdx.x;
  if (blk >= nblk) return;
  // d[]: octet o contributes u[8o + m] = bit m of the octet (LSB first)
  unsigned w = 0;
  if (lane < 6)
    for (int q = 0; q < 4; q++)
      if (4 * lane + q < 23) w |= (unsigned)frames[(size_t)blk * 23 + 4 * lane + q] << (8 * q);
  // parity word of d[0..184): every lane XORs the unit responses of its word's set bits
  unsigned long long par = 0;
  if (lane < 6)
    for (int k = 0; k < 32; k++)
      if (32 * lane + k < 184 && ((w >> k) & 1u)) par ^= kXcchPar.v[32 * lane + k];
  unsigned lo = (unsigned)par, hi = (unsigned)(par >> 32);
  for (int m = 1; m < 8; m <<= 1) { lo ^= __shfl_xor(lo, m, 64); hi ^= __shfl_xor(hi, m, 64); }
  const unsigned long long pw = ~(((unsigned long long)hi << 32) | lo) & ((1ULL << 40) - 1);   // inverted (bv:413)
  // u[184 + k] = bit (39 - k) of the word (fillField, MSB first); u[224..227] = 0
  if (lane == 5) for (int k = 0; k < 8; k++) w |= (unsigned)((pw >> (39 - k)) & 1ULL) << (24 + k);
  if (lane == 6) { w = 0; for (int k = 0; k < 32; k++) w |= (unsigned)((pw >> (39 - 8 - k)) & 1ULL) << k; }
  if (lane == 7) w = 0;
  if (lane < 8) uw[lane] = w;
  wave_fence();
  auto ubit = [&](int i) { return i < 0 ? 0u : ((uw[i >> 5] >> (i & 31)) & 1u); };
  uint8_t *out = bits + (size_t)blk * 4 * 148;
  // burst skeleton: zeros, stealing flags, training sequence
  for (int i = lane; i < 4 * 148; i += 64) {
    const int p = i % 148;
    uint8_t v = 0;
    if (p == 60 || p == 87) v = 1;
    else if (p >= 61 && p < 87) v = tsc_bits[p - 61] & 1u;
    if (p < 3 || p >= 145 || (p >= 60 && p < 88)) out[i] = v;
  }
  // c[2k], c[2k+1] from the 5-bit history ending at u[k]; interleave and place (fec:812-817, 833-836)
  for (int k = lane; k < 228; k += 64) {
    const unsigned idx = ubit(k) | (ubit(k - 1) << 1) | (ubit(k - 2) << 2) | (ubit(k - 3) << 3) | (ubit(k - 4) << 4);
    const unsigned g = (unsigned)(kGen >> (2 * idx)) & 3u;
    for (int h = 0; h < 2; h++) {
      const int c = 2 * k + h;
      const int B = c & 3, j = 2 * ((49 * c) % 57) + ((c % 8) / 4);
      out[B * 148 + (j < 57 ? 3 + j : 88 + (j - 57))] = (uint8_t)(h == 0 ? (g >> 1) : (g & 1u));
    }
  }
}

// ---------------------------------------------------------------------------------------------
// k_fec_tch_encode: TCHFACCHL1Encoder::dispatch / encodeTCH / interleave (fec:1252-1284, 1297-1393) for S channels x
// n blocks, a wave per (channel, block).  The encoder's eight interleaver rows mI[] and its alternating mOffset carry
// no information of their own: burst b (0..3) of block m carries, at e-bit position j = 2*((49k) mod 57) + (k mod 8)/4,
// c_m[k] (k = b mod 8) where j is even and c_{m-1}[k] (k = b+4 mod 8) where j is odd -- whatever the offset.  So a
// block's bursts depend on its own input and its predecessor's only: the wave re-forms c_{m-1} (or, for m = 0, takes
// its odd half from the channel's state) and every (channel, block) runs in the same launch.  The wave of block 0
// is the only one that touches a channel's state: it reads the old state and writes the new one (from block n-1).
// c[] is formed as the reference forms it: FACCH = the XCCH coder on the LSB8MSB'd L2 frame (fec:1320-1327),
// speech = encodeTCH (3 inverted parity bits over class 1a, u[] reordering, coder on u[189], class 2 copied),
// filler = the caller's c[] (fec:1346-1350), any other kind = zeros.  The output is gathered: each lane forms 16
// consecutive bytes of the block's 592 through an inverse interleaver table and stores them at once.
// ---------------------------------------------------------------------------------------------


template <bool VEC>
__global__ __launch_bounds__(64) void k_fec_tch_encode(int n_blocks, const uint8_t *__restrict__ kinds,
                                                       const uint8_t *__restrict__ payload, const uint8_t *__restrict__ tscs,
                                                       const uint8_t *__restrict__ tsc_bits /* 8 x 26 */,
                                                       const uint8_t *__restrict__ filler /* 456 */, uint8_t *state,
                                                       uint8_t *__restrict__ bits) {
  __shared__ uint8_t ca[456], cb[456], u[232], pls[36];
  const int lane = threadIdx.x;
  const int ch = blockIdx.x / n_blocks, m = blockIdx.x - ch * n_blocks;
  const size_t blk = (size_t)ch * n_blocks + m;
  uint8_t *out = bits + blk * 592;
  const unsigned tsc = tscs[ch];
  if (tsc > 7) {                                           // bad training sequence: zero bursts, state untouched
    if (VEC) { if (lane < 37) reinterpret_cast<uint4 *>(out)[lane] = make_uint4(0, 0, 0, 0); }
    else for (int i = lane; i < 592; i += 64) out[i] = 0;
    return;
  }
  const int kind = kinds[blk];
  tch_form_c(kind, payload + blk * 33, filler, u, ca, pls, lane);
  const unsigned curF = kind == TCH_FACCH;
  unsigned prevF;
  uint8_t *st = state + (size_t)ch * kTchState;
  if (m > 0) {
    const int pk = kinds[blk - 1];
    tch_form_c(pk, payload + (blk - 1) * 33, filler, u, cb, pls, lane);
    prevF = pk == TCH_FACCH;
  } else {
    for (int k = lane; k < 456; k += 64) {
      const int i = 4 * (k >> 3) + (k & 3);
      cb[k] = (k & 4) ? (uint8_t)((st[i >> 3] >> (i & 7)) & 1u) : (uint8_t)0;
    }
    prevF = st[kTchOddBytes] & 1u;
    wave_fence();
  }
  const uint8_t *tb = tsc_bits + 26 * tsc;
  auto obyte = [&](int p) -> unsigned {
    const int b = p / 148, pos = p - 148 * b;
    if (pos < 3 || pos >= 145) return 0u;
    if (pos == 60) return prevF;                           // Hl: the previous block was stolen (fec:1367)
    if (pos == 87) return curF;                            // Hu: this block is stolen (fec:1366)
    if (pos > 60 && pos < 87) return tb[pos - 61] & 1u;
    const int j = pos < 60 ? pos - 3 : pos - 31;
    const int k = kTchInv.k[b][j];
    return (j & 1) ? cb[k] : ca[k];
  };
  if (VEC) {
    if (lane < 37) {
      unsigned w[4];
      for (int q = 0; q < 4; q++) {
        unsigned v = 0;
        for (int r = 0; r < 4; r++) v |= obyte(16 * lane + 4 * q + r) << (8 * r);
        w[q] = v;
      }
      reinterpret_cast<uint4 *>(out)[lane] = make_uint4(w[0], w[1], w[2], w[3]);
    }
  } else {
    for (int i = lane; i < 592; i += 64) out[i] = (uint8_t)obyte(i);
  }
  if (m != 0) return;
  // the channel's new state: the odd half of block n-1's c[] and its FACCH flag (the old state is in cb already)
  const int lk = kinds[blk + n_blocks - 1];
  if (n_blocks > 1) {
    wave_fence();
    tch_form_c(lk, payload + (blk + n_blocks - 1) * 33, filler, u, ca, pls, lane);
  }
  if (lane < kTchState) {
    unsigned v = 0;
    if (lane < kTchOddBytes) {
      for (int t = 0; t < 8; t++) {
        const int i = 8 * lane + t;
        if (i < 228) v |= (unsigned)ca[8 * (i >> 2) + 4 + (i & 3)] << t;
      }
    } else if (lane == kTchOddBytes) {
      v = lk == TCH_FACCH;
    }
    st[lane] = (uint8_t)v;
  }
}

// ---------------------------------------------------------------------------------------------
// k_fec_sch_encode: SCHL1Encoder::generate (fec:897-920): d[25] = BSIC, T1, T2, T3' (writeField, MSB first), LSB8MSB
// (the first three octets only: bit 24 stays), 10 inverted parity bits (Parity(0x0575, 10, 25)), 4 zero tail bits,
// rate-1/2 coder, e[0..39) at 3..41, the extended training sequence at 42..105, e[39..78) at 106..144.  16 lanes per
// burst, each storing a dword of its 148 bytes; an FN outside the hyperframe or a BSIC above 63 gives a zero burst.
// ---------------------------------------------------------------------------------------------
template <bool VEC>
__global__ __launch_bounds__(64) void k_fec_sch_encode(const uint32_t *__restrict__ fns, const uint8_t *__restrict__ bsics,
                                                       int n, unsigned long long xts /* bit t = XTS[t] */,
                                                       uint8_t *__restrict__ bits) {
  const int lane = threadIdx.x & 15, i = blockIdx.x * 4 + (threadIdx.x >> 4);
  if (i >= n) return;
  const unsigned fn = fns[i], bsic = bsics[i];
  const bool valid = fn < 2715648u && bsic < 64u;
  unsigned long long e0 = 0, e1 = 0;                       // e[0..64), e[64..78)
  if (valid) {
    const unsigned t1 = (fn / (26u * 51u)) % 2048u, t2 = fn % 26u, t3 = fn % 51u;
    const unsigned t3p = (t3 - 1u) / 10u;                  // unsigned, as GSMCommon.h:474: wraps at T3 = 0
    const unsigned D = (bsic << 19) | (t1 << 8) | ((t2 & 31u) << 3) | (t3p & 7u);   // d[i] = bit 24-i
    unsigned d = 0;                                        // after LSB8MSB: bit 24-i = d'[i]
    for (int q = 0; q < 25; q++) {
      const int src = q < 24 ? 8 * (q >> 3) + 7 - (q & 7) : 24;
      d |= ((D >> (24 - src)) & 1u) << (24 - q);
    }
    unsigned par = 0;                                      // encoderShift (bh:80-85), generator 0x575
    for (int q = 0; q < 25; q++) {
      const unsigned fb = ((par >> 9) ^ (d >> (24 - q))) & 1u;
      par <<= 1;
      if (fb) par ^= 0x575u;
    }
    const unsigned pw = ~par & 0x3ffu;
    unsigned long long uu = ((unsigned long long)d << 14) | ((unsigned long long)pw << 4);   // u[i] = bit 38-i
    unsigned acc = 0;
    for (int q = 0; q < 39; q++) {
      acc = (acc << 1) | (unsigned)((uu >> (38 - q)) & 1ULL);
      const unsigned long long g = (kGen >> (2 * (acc & 31u))) & 3ULL;
      const int p = 2 * q;
      if (p < 64) e0 |= (g >> 1) << p; else e1 |= (g >> 1) << (p - 64);
      if (p + 1 < 64) e0 |= (g & 1ULL) << (p + 1); else e1 |= (g & 1ULL) << (p + 1 - 64);
    }
  }
  auto ebit = [&](int k) { return (unsigned)((k < 64 ? e0 >> k : e1 >> (k - 64)) & 1ULL); };
  auto obyte = [&](int pos) -> unsigned {
    if (!valid || pos < 3 || pos >= 145) return 0u;
    if (pos < 42) return ebit(pos - 3);
    if (pos < 106) return (unsigned)(xts >> (pos - 42)) & 1u;
    return ebit(39 + pos - 106);
  };
  uint8_t *out = bits + (size_t)i * 148;
  for (int w = lane; w < 37; w += 16) {
    if (VEC) {
      unsigned v = 0;
      for (int r = 0; r < 4; r++) v |= obyte(4 * w + r) << (8 * r);
      reinterpret_cast<unsigned *>(out)[w] = v;
    } else {
      for (int r = 0; r < 4; r++) out[4 * w + r] = (uint8_t)obyte(4 * w + r);
    }
  }
}

// ---------------------------------------------------------------------------------------------
// k_fec_rx_stream / k_fec_rx_fold: the uplink decoders of many channels as streams -- TCHFACCHL1Decoder::processBurst /
// deinterleave / decodeTCH (fec:1030-1163) and XCCHL1Decoder::writeLowSide / processBurst / deinterleave / decode
// (fec:556-653) with the deinterleaving buffer mI[][] carried from call to call in a per-channel state record.
//
// Closed form of mI.  Slot t of a channel writes row B(t) of mI in full when its burst is present; the block that closes
// at slot 4m+3 (B % 4 == 3) is decoded when that burst is present, and then reads half of every row (TCH: the odd half of
// rows 0..3 and the even half of rows 4..7 at B = 3, the other way round at B = 7; XCCH: all of every row) and leaves 0.5
// behind.  Each (row, half) therefore sees one possible write and one possible read per period (P = 8 slots for TCH, 4 for
// XCCH), and its value at any point of the stream is decided by its most recent event: a present burst (its value), a
// decoded read (0.5), or -- when the scan back through the periods of the call finds neither -- the incoming state.  A write
// and a read in the same slot happen in that order.  So every (channel, block) gathers its c[] independently: a 16-lane row
// of k_fec_rx_stream per code word, one Viterbi pass (the FACCH/XCCH decode of 456 -> 228 or the class-1 decode of
// 378 -> 189, whichever the block needs), and k_fec_rx_fold, launched after it, writes the new state and folds the FER.
// ---------------------------------------------------------------------------------------------
constexpr int kRxHdr = 16;                                 // state: bytes 0..3 mFER (float), 4..15 zero, then the rows of mI
constexpr int kSrcHalf = -1, kSrcState = -2;               // source of a (row, half): a burst's row (>= 0), 0.5, or the state

struct RxStream {
  const float *soft;
  long long stride, n_rows;
  const int32_t *index;                                    // [n_chan][n_slots]
  const uint8_t *b0;                                       // [n_chan] or null
  int n_chan, n_slots, wire;
};

// the row of slot t's burst, or -1 (no burst: -1, or any index outside [0, n_rows))
__device__ __forceinline__ int rx_row(const RxStream &a, const int32_t *idx, int t) {
  const int i = idx[t];
  return (i >= 0 && (long long)i < a.n_rows) ? i : -1;
}

// the source of a (row, half) at a point of the stream: tw = the last slot up to the point that writes the row, tr = the
// last decodable read of the half before the point (both step back by P; negative = before the call)
__device__ __forceinline__ int rx_source(const RxStream &a, const int32_t *idx, bool chan_ok, int tw, int tr, int P) {
  if (!chan_ok) return kSrcState;
  while (tw >= 0 || tr >= 0) {
    if (tr >= tw) {                                        // the read is the later event (same slot: write, then read)
      if (rx_row(a, idx, tr) >= 0) return kSrcHalf;
      tr -= P;
    } else {
      const int r = rx_row(a, idx, tw);
      if (r >= 0) return r;
      tw -= P;
    }
  }
  return kSrcState;
}

// e-bit j (0..113) of a burst: data1 = burst[3..60), data2 = burst[88..145) (fec:607-608, 1051-1052)
__device__ __forceinline__ int rx_pos(int j) { return j < 57 ? 3 + j : 88 + (j - 57); }

// a channel's d_b0 (TCH): 0 or 4; any other value makes the channel one where no burst arrives
__device__ __forceinline__ int rx_b0(const RxStream &a, int ch) { return a.b0 ? (int)a.b0[ch] : 0; }

template <bool TCH>
__global__ __launch_bounds__(64) void k_fec_rx_stream(RxStream a, int blk0, const uint8_t *__restrict__ state,
                                                      uint8_t *__restrict__ status, uint8_t *__restrict__ out_tch,
                                                      uint8_t *__restrict__ out_l2) {
  constexpr int R = TCH ? 8 : 4, P = TCH ? 8 : 4;
  constexpr int kStateBytes = kRxHdr + R * 114 * 4;
  __shared__ float4 ktab[4][kChunk];
  __shared__ int srcd[4][8];
  const int lane = threadIdx.x & 63, row = lane >> 4, s = lane & 15;
  const int n_blocks = a.n_slots >> 2;
  const int blk = blk0 + blockIdx.x * 4 + row;             // (channel, block) = blk; n_chan * n_blocks < 2^29
  const bool live = blk < a.n_chan * n_blocks;
  const int ch = live ? blk / n_blocks : 0, m = live ? blk - ch * n_blocks : 0;
  const int32_t *idx = a.index + (size_t)ch * a.n_slots;
  const int b0 = TCH ? rx_b0(a, ch) : 0;
  const bool chan_ok = !TCH || b0 == 0 || b0 == 4;
  const int tc = 4 * m + 3;                                // the closing slot
  const int cl = (live && chan_ok) ? rx_row(a, idx, tc) : -1;
  const bool decoded = cl >= 0;
  const int Bc = TCH ? ((b0 + tc) & 7) : 3;                // B of the closing burst: 3 or 7 (TCH), 3 (XCCH)
  const int off = Bc == 3 ? 4 : 0;                         // deinterleave(4) at B = 3, deinterleave(0) at B = 7 (fec:1072-1073)
  bool stolen = false;
  if (TCH && decoded) {                                    // Hl of the closing burst (fec:1076-1077)
    float hl = a.soft[(size_t)cl * a.stride + 60];
    if (a.wire) hl = wire_value(hl);
    stolen = hl > 0.5F;
  }
  // the sources of the row's c[]: (row r, the half this block reads) for r = s < R
  if (s < R) {
    const int tw = tc - ((Bc - s) & (P - 1));              // the last slot up to tc with B = r
    srcd[row][s] = decoded ? rx_source(a, idx, chan_ok, tw, tc - P, P) : kSrcState;
  }
  wave_fence();
  const float *st_rows = reinterpret_cast<const float *>(state + (size_t)ch * kStateBytes + kRxHdr);
  const int *sd = srcd[row];
  auto rowB = [&](int k) { return TCH ? ((k + off) & 7) : (k & 3); };
  auto fetch = [&](int k) -> float {
    const int B = rowB(k);
    const int j = 2 * ((49 * k) % 57) + ((k % 8) / 4);     // GSM 05.03 3.1.3 / 4.1.4 (fec:622-625, 1111)
    const int src = sd[B];
    if (src >= 0) return a.soft[(size_t)src * a.stride + rx_pos(j)];
    return src == kSrcHalf ? 0.5F : st_rows[B * 114 + j];
  };
  auto finish = [&](float v, int k) -> float {             // the UDP hop applies to a burst's values as they enter mI
    return (a.wire && sd[rowB(k)] >= 0) ? wire_value(v) : v;
  };
  const bool l2 = !TCH || stolen;                          // the FACCH / XCCH decode (456 -> 228), else class 1 (378 -> 189)
  const unsigned long long any = __builtin_amdgcn_ballot_w64(decoded);
  const unsigned long long anyl2 = __builtin_amdgcn_ballot_w64(decoded && l2);
  const int steps = any == 0 ? 0 : (anyl2 ? 228 : 189) + kDeferral;
  const unsigned outw = fec_trellis(ktab[row], l2 ? 456 : 378, steps, decoded, lane, fetch, finish);
  if (!live) return;

  const size_t ob = (size_t)blk;
  bool okl2 = false, good = false;
  if (TCH) {
    unsigned *uw = reinterpret_cast<unsigned *>(ktab[row]);
    if (s < 6) uw[s] = outw;
    wave_fence();
    if (decoded && !stolen) {
      auto cbit = [&](int k) { return finish(fetch(k), k) > 0.5F ? 1u : 0u; };    // class 2 sliced (fec:1141)
      good = tch_finish(uw, s, cbit, out_tch + ob * 33);
    } else {
      for (int o = s; o < 33; o += 16) out_tch[ob * 33 + o] = 0;
    }
  }
  if (decoded && l2) {
    okl2 = xcch_finish(outw, s, out_l2 + ob * 23);
  } else {
    for (int o = s; o < 23; o += 16) out_l2[ob * 23 + o] = 0;
  }
  if (s == 0) {
    unsigned f = 0;
    if (decoded) {
      f = TRXSIG_FEC_DECODED;
      if (TCH && stolen) f |= TRXSIG_FEC_STOLEN | (okl2 ? TRXSIG_FEC_FACCH_OK : 0u);
      if (TCH ? good : okl2) f |= TRXSIG_FEC_TCH_GOOD;
    }
    status[ob] = (uint8_t)f;
  }
}

// A workgroup per channel, after k_fec_rx_stream: the FER after every block (L1Decoder::countGoodFrame / countBadFrame,
// fec:390-405, in the reference's count order) and the new state -- mFER and the rows of mI after the call's last slot.
// Every position of the state is read and rewritten by the same lane, so the update in place is race-free.
template <bool TCH>
__global__ __launch_bounds__(64) void k_fec_rx_fold(RxStream a, int ch0, uint8_t *state, const uint8_t *__restrict__ status,
                                                    uint8_t *__restrict__ fer_out) {
  constexpr int R = TCH ? 8 : 4, P = TCH ? 8 : 4;
  constexpr int kStateBytes = kRxHdr + R * 114 * 4;
  __shared__ int srcd[16];
  const int lane = threadIdx.x, ch = ch0 + blockIdx.x;
  const int n_blocks = a.n_slots >> 2, T = a.n_slots;
  const int32_t *idx = a.index + (size_t)ch * a.n_slots;
  const int b0 = TCH ? rx_b0(a, ch) : 0;
  const bool chan_ok = !TCH || b0 == 0 || b0 == 4;
  uint8_t *st = state + (size_t)ch * kStateBytes;
  float *rows = reinterpret_cast<float *>(st + kRxHdr);
  // sources after the last slot: TCH (row r, half h) = srcd[2r + h], XCCH row r = srcd[r]
  if (lane < (TCH ? 16 : 4)) {
    const int r = TCH ? lane >> 1 : lane, h = lane & 1;
    const int Bl = TCH ? ((b0 + T - 1) & 7) : 3;           // B of the last slot
    const int Br = TCH ? ((((r < 4) == (h == 1)) ? 3 : 7)) : 3;   // the closing B that reads (r, h)
    srcd[lane] = rx_source(a, idx, chan_ok, T - 1 - ((Bl - r) & (P - 1)), T - 1 - ((Bl - Br) & (P - 1)), P);
  }
  wave_fence();
  for (int i = lane; i < R * 114; i += 64) {
    const int r = i / 114, j = i - 114 * r;
    const int src = srcd[TCH ? 2 * r + (j & 1) : r];       // half = the parity of j (fec:1111)
    if (src >= 0) {
      float v = a.soft[(size_t)src * a.stride + rx_pos(j)];
      if (a.wire) v = wire_value(v);
      rows[i] = v;
    } else if (src == kSrcHalf) {
      rows[i] = 0.5F;
    }                                                      // kSrcState: the old value stays
  }
  // the FER, 64 blocks at a time: every lane runs the recurrence on the broadcast status bytes
  const float fa = 1.0F / 20.0F, fb = 1.0F - fa;          // mFERMemory = 20 (GSML1FEC.h:226)
  float fer = *reinterpret_cast<const float *>(st);
  for (int m0 = 0; m0 < n_blocks; m0 += 64) {
    const int mine = m0 + lane < n_blocks ? (int)status[(size_t)ch * n_blocks + m0 + lane] : 0;
    const int cnt = n_blocks - m0 < 64 ? n_blocks - m0 : 64;
    float keep = 0.0F;
    for (int q = 0; q < cnt; q++) {
      const int f = __shfl(mine, q, 64);
      if (f & TRXSIG_FEC_DECODED) {
        if (TCH && (f & TRXSIG_FEC_STOLEN)) {
          if (f & TRXSIG_FEC_FACCH_OK) fer *= fb; else fer = fb * fer + fa;   // the FACCH frame (fec:1079-1089)
          fer = fb * fer + fa;                             // decodeTCH(true) returns false (fec:1094-1098)
        } else if (f & TRXSIG_FEC_TCH_GOOD) {
          fer *= fb;
        } else {
          fer = fb * fer + fa;
        }
      }
      if (q == lane) keep = fer;
    }
    if (fer_out && lane < cnt) {                           // bytewise: d_fer may be unaligned
      const unsigned u = __float_as_uint(keep);
      uint8_t *o = fer_out + 4 * ((size_t)ch * n_blocks + m0 + lane);
      o[0] = (uint8_t)u; o[1] = (uint8_t)(u >> 8); o[2] = (uint8_t)(u >> 16); o[3] = (uint8_t)(u >> 24);
    }
  }
  if (lane == 0) *reinterpret_cast<float *>(st) = fer;
  if (lane >= 1 && lane < 4) reinterpret_cast<unsigned *>(st)[lane] = 0u;
}

// ---------------------------------------------------------------------------------------------
// k_fec_pdtch_encode / k_fec_pdtch_decode: the GPRS packet data block coders CS-1..CS-4 (GSM 05.03 5.1) as include/trxsig.h
// states them.  They share the coder (kGen), the interleaver and the trellis with XCCH; theirs are the payload convention, the
// 16-bit block check, the USF pre-coding, the puncturing and the scheme in the eight stealing flags.  The reference has no
// packet channel: the constants are the header's, the arithmetic is tests/pdtch_model.py's.
//
// One bit stream per scheme, so that both kernels treat the four alike: the bits in front of d(3) (`pre` of them: d(0..2)
// themselves for CS-1, the 6- or 12-bit USF word otherwise), d(3..K-1), the parity bits, the tail.  CS-1..3 send it through
// the coder, CS-4 as it is.
// ---------------------------------------------------------------------------------------------
struct PdPar {                                             // r[m]: encoderShift response (generator 0x11021, 16 bits) to a 1 with m zeros behind it
  uint16_t r[431];
  constexpr PdPar() : r() {
    unsigned st = 0x1021u;                                 // the bit just went in: fb = 1, state = coeff
    for (int m = 0; m < 431; m++) {
      r[m] = (uint16_t)st;
      const unsigned fb = (st >> 15) & 1u;
      st = (st << 1) & 0xFFFFu;
      if (fb) st ^= 0x1021u;
    }
  }
};
__device__ __constant__ const PdPar kPdPar;

constexpr unsigned long long pd_pack(const char *const *rows, int n, int width) {   // row r at bits r*width .., first character lowest
  unsigned long long w = 0;
  for (int r = 0; r < n; r++)
    for (int i = 0; i < width; i++) w |= (unsigned long long)(rows[r][i] == '1') << (r * width + i);
  return w;
}
constexpr const char *kPdUsf6Rows[8] = { "000000", "001011", "010110", "011101", "100101", "101110", "110011", "111000" };
constexpr const char *kPdUsf12Rows[8] = { "000000000000", "000011011101", "001101110110", "001110101011",
                                          "110100001011", "110111010110", "111001111101", "111010100000" };
constexpr const char *kPdFlagRows[4] = { "11111111", "11001000", "00100001", "00010110" };
constexpr unsigned long long kPdUsf6 = pd_pack(kPdUsf6Rows, 8, 6);
constexpr unsigned long long kPdUsf12Lo = pd_pack(kPdUsf12Rows, 4, 12), kPdUsf12Hi = pd_pack(kPdUsf12Rows + 4, 4, 12);
constexpr unsigned kPdFlags = (unsigned)pd_pack(kPdFlagRows, 4, 8);

__device__ __forceinline__ int pd_k(unsigned cs) { return cs == 0 ? 184 : cs == 1 ? 271 : cs == 2 ? 315 : 431; }
__device__ __forceinline__ int pd_nu(unsigned cs) { return cs == 0 ? 228 : cs == 1 ? 294 : cs == 2 ? 338 : 456; }   // the stream's length
__device__ __forceinline__ int pd_pre(unsigned cs) { return cs == 0 ? 3 : cs == 3 ? 12 : 6; }
// the USF word of row r = d(0) d(1) d(2) read as a number, bit i = the i-th bit sent
__device__ __forceinline__ unsigned pd_usf_word(unsigned cs, unsigned r) {
  if (cs == 3) return (unsigned)((r < 4 ? kPdUsf12Lo >> (12 * r) : kPdUsf12Hi >> (12 * (r - 4))) & 0xFFFu);
  return (unsigned)(kPdUsf6 >> (6 * r)) & 0x3Fu;
}
__device__ __forceinline__ unsigned pd_flag_word(unsigned cs) { return (kPdFlags >> (8 * cs)) & 0xFFu; }   // bit i = q(i)

// The puncturing in closed form: coder output C(P) -> its index in c[456], or -1 where C(P) is deleted.
// CS-2 deletes C(3 + 4j), j = 3..146 but not j = 9 mod 12; CS-3 deletes C(3 + 6j) and C(5 + 6j), j = 2..111.
__device__ __forceinline__ int pd_cindex(unsigned cs, int P) {
  if (cs == 1) {
    const int j = (P - 3) >> 2;
    if ((P & 3) == 3 && j >= 3 && j <= 146 && j % 12 != 9) return -1;
    int m = (P - 4) >> 2;                                  // the last j with 3 + 4j < P
    if (m > 146) m = 146;
    return m < 3 ? P : P - (m - 2 - (m + 3) / 12);
  }
  if (cs == 2) {
    const int j = P / 6, r = P - 6 * j;
    const bool in = j >= 2 && j <= 111;
    if (in && (r == 3 || r == 5)) return -1;
    const int full = (j < 112 ? j : 112) - 2;              // whole groups below P's own
    return P - (full > 0 ? 2 * full : 0) - ((in && r > 3) ? 1 : 0);
  }
  return P;
}

// A wave per block, laid out as k_fec_xcch_encode: the payload and the stream in LDS (a byte per bit), the parity word by the
// register's GF(2) linearity, the coder with the puncturing as a scatter into c[456], and the four bursts gathered through
// the inverse interleaver table, 16 bytes a lane.  A cs above 3 or a tsc above 7: four all-zero bursts.
template <bool VEC>
__global__ __launch_bounds__(64) void k_fec_pdtch_encode(const uint8_t *__restrict__ blocks, const uint8_t *__restrict__ css,
                                                         const uint8_t *__restrict__ tscs, int nblk,
                                                         const uint8_t *__restrict__ tsc_bits /* 8 x 26 */, uint8_t *__restrict__ bits) {
  __shared__ uint8_t pls[56], u[456], c[456];
  const int lane = threadIdx.x, blk = blockIdx.x;
  if (blk >= nblk) return;
  uint8_t *out = bits + (size_t)blk * 592;
  const unsigned cs = css[blk], tsc = tscs[blk];
  if (cs > 3 || tsc > 7) {
    if (VEC) { if (lane < 37) reinterpret_cast<uint4 *>(out)[lane] = make_uint4(0, 0, 0, 0); }
    else for (int i = lane; i < 592; i += 64) out[i] = 0;
    return;
  }
  if (lane < 54) pls[lane] = blocks[(size_t)blk * 54 + lane];
  wave_fence();
  auto dq = [&](int k) { return (unsigned)(pls[k >> 3] >> (k & 7)) & 1u; };   // d(k): bit k mod 8 of octet k / 8, LSB first
  const int K = pd_k(cs), nu = pd_nu(cs), pre = pd_pre(cs), np = cs == 0 ? 40 : 16;
  // the parity word of d(0..K-1): XOR of the unit responses of its set bits (CS-1: XCCH's Fire code)
  unsigned long long par = 0;
  for (int i = lane; i < K; i += 64)
    if (dq(i)) par ^= cs == 0 ? kXcchPar.v[i] : (unsigned long long)kPdPar.r[K - 1 - i];
  unsigned lo = (unsigned)par, hi = (unsigned)(par >> 32);
  for (int m = 1; m < 64; m <<= 1) { lo ^= (unsigned)__shfl_xor((int)lo, m, 64); hi ^= (unsigned)__shfl_xor((int)hi, m, 64); }
  const unsigned long long pw = ~(((unsigned long long)hi << 32) | lo) & ((1ULL << np) - 1);   // inverted (bv:413)
  const unsigned head = cs == 0 ? (dq(0) | (dq(1) << 1) | (dq(2) << 2)) : pd_usf_word(cs, (dq(0) << 2) | (dq(1) << 1) | dq(2));
  for (int i = lane; i < nu; i += 64) {
    const int k = i - pre + 3;                             // d's index from the stream's, past the head
    unsigned v = 0;
    if (i < pre) v = (head >> i) & 1u;
    else if (k < K) v = dq(k);
    else if (k < K + np) v = (unsigned)(pw >> (np - 1 - (k - K))) & 1u;   // MSB first; the tail bits stay 0
    u[i] = (uint8_t)v;
  }
  wave_fence();
  if (cs == 3) {
    for (int i = lane; i < 456; i += 64) c[i] = u[i];
  } else {
    for (int k = lane; k < nu; k += 64) {
      unsigned idx = 0;
      for (int h = 0; h < 5; h++) idx |= (k - h >= 0 ? (unsigned)u[k - h] : 0u) << h;
      const unsigned g = (unsigned)(kGen >> (2 * idx)) & 3u;
      const int c0 = pd_cindex(cs, 2 * k), c1 = pd_cindex(cs, 2 * k + 1);
      if (c0 >= 0) c[c0] = (uint8_t)(g >> 1);
      if (c1 >= 0) c[c1] = (uint8_t)(g & 1u);
    }
  }
  wave_fence();
  const uint8_t *tb = tsc_bits + 26 * tsc;
  const unsigned fw = pd_flag_word(cs);
  auto obyte = [&](int p) -> unsigned {
    const int b = p / 148, pos = p - 148 * b;
    if (pos < 3 || pos >= 145) return 0u;
    if (pos == 87) return (fw >> (2 * b)) & 1u;            // q(2b)
    if (pos == 60) return (fw >> (2 * b + 1)) & 1u;        // q(2b + 1)
    if (pos > 60 && pos < 87) return tb[pos - 61] & 1u;
    const int j = pos < 60 ? pos - 3 : pos - 31;
    return c[kTchInv.k[b][j]];                             // XCCH's interleaver: burst k mod 4, the same j as TCH's
  };
  if (VEC) {
    if (lane < 37) {
      unsigned w[4];
      for (int q = 0; q < 4; q++) {
        unsigned v = 0;
        for (int r = 0; r < 4; r++) v |= obyte(16 * lane + 4 * q + r) << (8 * r);
        w[q] = v;
      }
      reinterpret_cast<uint4 *>(out)[lane] = make_uint4(w[0], w[1], w[2], w[3]);
    }
  } else {
    for (int i = lane; i < 592; i += 64) out[i] = (uint8_t)obyte(i);
  }
}

struct PdDecode {
  const float *soft;
  long long stride, n_rows;
  const int32_t *index;                                    // [nblk][4] or null
  int nblk, cs_force;
  uint8_t *blocks, *cs, *dist, *ok, *usf;                  // all but blocks may be null
};

// 16 lanes a block, four blocks a wave, as k_fec_viterbi; the four rows may hold four schemes (fec_trellis takes the row's n
// and the wave's step count).  Per row: the four bursts' rows (a missing burst costs no load: its values are 0.5), the flag
// vote on the row's lanes 0..7, then CS-4 slices its 456 values while CS-1..3 wait for nothing (a CS-4 row is not live in
// the trellis), the trellis with the depuncturing in the fetch functor, and the finish: XCCH's for CS-1; for CS-2..4 the
// stream's words in LDS, d() as a funnel shift of two of them, the nearest USF row, the block check by unit responses.
// WIRE: the UDP hop's quantisation of every value read (wire_quantise != 0).
template <bool WIRE>
__global__ __launch_bounds__(64) void k_fec_pdtch_decode(PdDecode a) {
  __shared__ float4 ktab[4][kChunk];
  __shared__ int srcd[4][4];
  const int lane = threadIdx.x & 63, row = lane >> 4, s = lane & 15;
  const int blk = blockIdx.x * 4 + row;
  const bool live = blk < a.nblk;
  if (s < 4) {
    long long i = -1;
    if (live) i = a.index ? (long long)a.index[(size_t)blk * 4 + s] : 4LL * blk + s;
    srcd[row][s] = (i >= 0 && i < a.n_rows) ? (int)i : -1;
  }
  wave_fence();
  const int *sd = srcd[row];
  auto value = [&](int k) -> float {                       // c[k] as the decoder sees it
    const int src = sd[k & 3];
    if (src < 0) return 0.5F;
    const int j = 2 * ((49 * k) % 57) + ((k % 8) / 4);     // GSM 05.03 4.1.4 (fec:622-625)
    const float v = a.soft[(size_t)src * a.stride + rx_pos(j)];
    return WIRE ? wire_value(v) : v;
  };
  // the scheme: hard flags q(i) on lane i (bit 87, then bit 60, of burst i / 2), nearest word, ties to the lower scheme
  bool flag = false;
  if (s < 8 && sd[s >> 1] >= 0) {
    float v = a.soft[(size_t)sd[s >> 1] * a.stride + ((s & 1) ? 60 : 87)];
    if (WIRE) v = wire_value(v);
    flag = v > 0.5F;
  }
  const unsigned hard = (unsigned)(__builtin_amdgcn_ballot_w64(flag) >> (lane & 48)) & 0xFFu;
  unsigned cs = 0;
  int dist = __builtin_popcount(hard ^ pd_flag_word(0));
  for (unsigned r = 1; r < 4; r++) {
    const int d = __builtin_popcount(hard ^ pd_flag_word(r));
    if (d < dist) { dist = d; cs = r; }
  }
  if (a.cs_force >= 0) { cs = (unsigned)a.cs_force; dist = __builtin_popcount(hard ^ pd_flag_word(cs)); }
  // CS-4: the 456 values sliced, sixteen a row at a time; lane s keeps the stream's word s
  const bool c4 = live && cs == 3;
  unsigned word = 0;
  if (__builtin_amdgcn_ballot_w64(c4)) {
    for (int q = 0; q < 29; q++) {
      const int k = s + 16 * q;
      const bool b = c4 && k < 456 && value(k) > 0.5F;
      const unsigned w16 = (unsigned)(__builtin_amdgcn_ballot_w64(b) >> (lane & 48)) & 0xFFFFu;
      if ((q >> 1) == s) word |= w16 << (16 * (q & 1));
    }
  }
  // CS-1..3: the trellis over the coder's 2 nu outputs, a deleted one reading exactly 0.5 (wire_value(0.5F) is 0.5F, so
  // `finish` need not know which they are)
  const bool dec = live && cs != 3;
  const int nu = pd_nu(cs);
  const int steps = __builtin_amdgcn_ballot_w64(dec && cs == 2) ? 338 + kDeferral
                  : __builtin_amdgcn_ballot_w64(dec && cs == 1) ? 294 + kDeferral
                  : __builtin_amdgcn_ballot_w64(dec) ? 228 + kDeferral : 0;
  auto fetch = [&](int p) -> float {
    const int k = pd_cindex(cs, p);
    if (k < 0) return 0.5F;
    const int src = sd[k & 3];
    if (src < 0) return 0.5F;
    const int j = 2 * ((49 * k) % 57) + ((k % 8) / 4);
    return a.soft[(size_t)src * a.stride + rx_pos(j)];
  };
  auto finish = [&](float v, int) -> float { return WIRE ? wire_value(v) : v; };
  const unsigned outw = fec_trellis(ktab[row], 2 * nu, steps, dec, lane, fetch, finish);
  if (!live) return;

  uint8_t *ob = a.blocks + (size_t)blk * 54;
  bool ok;
  unsigned usf;
  if (cs == 0) {
    ok = xcch_finish(outw, s, ob);                         // octets 0..22 and the Fire syndrome
    for (int o = 23 + s; o < 54; o += 16) ob[o] = 0;
    usf = (unsigned)__shfl((int)outw, lane & 48, 64) & 7u;
  } else {
    if (cs != 3) word = outw;
    unsigned *uw = reinterpret_cast<unsigned *>(ktab[row]); // the stream, bit i = (uw[i / 32] >> i % 32) & 1
    uw[s] = word;
    if (s == 0) uw[16] = 0;
    wave_fence();
    const int K = pd_k(cs), pre = pd_pre(cs), sh = pre - 3; // d(k) = stream bit k + sh for k >= 3
    // d(0..2): the nearest row of the USF table (Hamming, ties to the first row)
    const unsigned head = uw[0] & ((1u << pre) - 1u);
    unsigned best = 0;
    int bd = __builtin_popcount(head ^ pd_usf_word(cs, 0));
    for (unsigned r = 1; r < 8; r++) {
      const int d = __builtin_popcount(head ^ pd_usf_word(cs, r));
      if (d < bd) { bd = d; best = r; }
    }
    usf = ((best >> 2) & 1u) | (((best >> 1) & 1u) << 1) | ((best & 1u) << 2);
    // this lane's word of d: bits 32s .. 32s+31, nothing at or past K
    unsigned dw = (unsigned)(((((unsigned long long)uw[s + 1]) << 32) | uw[s]) >> sh);
    if (s == 0) dw = (dw & ~7u) | usf;
    const int nb = K - 32 * s;
    if (nb <= 0) dw = 0;
    else if (nb < 32) dw &= (1u << nb) - 1u;
    for (int q = 0; q < 4; q++)
      if (4 * s + q < 54) ob[4 * s + q] = (uint8_t)(dw >> (8 * q));
    // the block check on d: the parity register's word against the sent one, which is its inverse
    unsigned par = 0;
    for (int k = 0; k < 32; k++)
      if ((dw >> k) & 1u) par ^= kPdPar.r[K - 1 - (32 * s + k)];
    par ^= (unsigned)dpp_i<0xB1>((int)par);
    par ^= (unsigned)dpp_i<0x4E>((int)par);
    par ^= (unsigned)dpp_i<0x141>((int)par);
    par ^= (unsigned)dpp_i<0x140>((int)par);
    unsigned sent = 0;
    for (int k = 0; k < 16; k++) {
      const int i = K + sh + k;
      sent |= ((uw[i >> 5] >> (i & 31)) & 1u) << (15 - k);
    }
    ok = (par ^ sent) == 0xFFFFu;
  }
  if (s == 0) {
    if (a.cs) a.cs[blk] = (uint8_t)cs;
    if (a.dist) a.dist[blk] = (uint8_t)dist;
    if (a.ok) a.ok[blk] = ok;
    if (a.usf) a.usf[blk] = (uint8_t)usf;
  }
}

// ---------------------------------------------------------------------------------------------
// k_fec_access_encode / k_fec_access_decode: the access burst in both formats, the 8-bit one of GSM 05.03 4.6 (rach_e36, what
// FEC_RACH decodes) and the 11-bit packet access burst of 5.3.2 as include/trxsig.h states it.  The coder is access_e36 of
// trxsig_fec_enc.h; the reference has no 11-bit format: its arithmetic is tests/access_model.py's.
// ---------------------------------------------------------------------------------------------

// 16 lanes a burst, each storing dwords of its 148 bytes, as k_fec_sch_encode.  A format above 1, a BSIC above 63 or a word
// that does not fit its format: an all-zero row.
template <bool VEC>
__global__ __launch_bounds__(64) void k_fec_access_encode(const uint16_t *__restrict__ ras, const uint8_t *__restrict__ fmts,
                                                          const uint8_t *__restrict__ bsics, int n, uint8_t *__restrict__ bits) {
  const int lane = threadIdx.x & 15, i = blockIdx.x * 4 + (threadIdx.x >> 4);
  if (i >= n) return;
  const unsigned ra = ras[i], fmt = fmts[i], bsic = bsics[i];
  const bool valid = fmt <= 1u && bsic < 64u && ra < (fmt ? 2048u : 256u);
  const unsigned long long e = valid ? access_e36(ra, fmt, bsic) : 0ULL;
  auto obyte = [&](int pos) -> unsigned {
    if (!valid || pos >= 85) return 0u;
    return (unsigned)((pos < 49 ? kAccessHead >> pos : e >> (pos - 49)) & 1ULL);
  };
  uint8_t *out = bits + (size_t)i * 148;
  for (int w = lane; w < 37; w += 16) {
    if (VEC) {
      unsigned v = 0;
      for (int r = 0; r < 4; r++) v |= obyte(4 * w + r) << (8 * r);
      reinterpret_cast<unsigned *>(out)[w] = v;
    } else {
      for (int r = 0; r < 4; r++) out[4 * w + r] = (uint8_t)obyte(4 * w + r);
    }
  }
}

struct AccDecode {
  const float *soft;
  long long stride, n_rows;
  const int32_t *index;                                    // [n] or null
  int n, fmt, bsic;
  uint16_t *ra;
  uint8_t *ofmt, *tail_ok, *obsic;                         // may be null
};

// what a hypothesis reads out of its u[]: ND data bits, six parity bits MSB first, four tail bits (fec:485-507 for ND = 8)
template <int ND>
__device__ __forceinline__ void access_verdict(unsigned u, unsigned *ra, unsigned *tail_ok, unsigned *bsic) {
  unsigned sent = 0, st = 0;
  for (int k = 0; k < 6; k++) sent |= ((u >> (ND + k)) & 1u) << (5 - k);
  for (int k = 0; k < ND; k++) {                           // encoderShift (bh:80-85), generator 0x6f
    const unsigned fb = ((st >> 5) ^ (u >> k)) & 1u;
    st <<= 1;
    if (fb) st ^= 0x6fu;
  }
  *tail_ok = ((u >> (ND + 6)) & 0xFu) == 0;
  *bsic = (~sent ^ st) & 0x3fu;
  *ra = u & ((1u << ND) - 1u);
}

// 16 lanes a burst, four bursts a wave, as k_fec_viterbi<FEC_RACH>, whose fetch the 8-bit pass repeats; the 11-bit pass reads
// the six deleted coder outputs as exactly 0.5 (wire_value(0.5F) is 0.5F).  fmt -1 runs both passes on every row.
template <bool WIRE>
__global__ __launch_bounds__(64) void k_fec_access_decode(AccDecode a) {
  __shared__ float4 ktab[4][kChunk];
  const int lane = threadIdx.x & 63, row = lane >> 4, s = lane & 15;
  const int blk = blockIdx.x * 4 + row;
  const bool live = blk < a.n;
  long long src = -1;
  if (live) src = a.index ? (long long)a.index[blk] : (long long)blk;
  if (src >= a.n_rows) src = -1;
  const float *e = a.soft + (src < 0 ? 0 : src) * a.stride + 49;   // the 36 coded values; read only where src >= 0
  auto finish = [&](float v, int) -> float { return WIRE ? wire_value(v) : v; };
  unsigned u8 = 0, u11 = 0;
  if (a.fmt != 1) {
    auto fetch = [&](int p) -> float { return src < 0 ? 0.5F : e[p]; };
    u8 = fec_trellis(ktab[row], 36, 18 + kDeferral, live, lane, fetch, finish);
  }
  if (a.fmt != 0) {
    auto fetch = [&](int p) -> float {
      const int k = access_cindex(p);
      return (k < 0 || src < 0) ? 0.5F : e[k];
    };
    u11 = fec_trellis(ktab[row], 42, 21 + kDeferral, live, lane, fetch, finish);
  }
  if (!live || s != 0) return;                             // u[0..20] is in the row's lane 0
  unsigned ra8 = 0, t8 = 0, b8 = 0, ra11 = 0, t11 = 0, b11 = 0;
  if (a.fmt != 1) access_verdict<8>(u8, &ra8, &t8, &b8);
  if (a.fmt != 0) access_verdict<11>(u11, &ra11, &t11, &b11);
  bool long_fmt = a.fmt == 1;
  if (a.fmt < 0) long_fmt = (t11 && b11 == (unsigned)a.bsic) && !(t8 && b8 == (unsigned)a.bsic);
  a.ra[blk] = (uint16_t)(long_fmt ? ra11 : ra8);
  if (a.ofmt) a.ofmt[blk] = (uint8_t)long_fmt;
  if (a.tail_ok) a.tail_ok[blk] = (uint8_t)(long_fmt ? t11 : t8);
  if (a.obsic) a.obsic[blk] = (uint8_t)(long_fmt ? b11 : b8);
}

}  // namespace

hipError_t trx_launch_fec_xcch_encode(hipStream_t st, const uint8_t *frames, int nblk, const uint8_t *tsc_bits, uint8_t *bits,
                                      TrxProfiler *prof) {
  if (nblk <= 0) return hipSuccess;
  if (prof) prof->begin(TRXSIG_K_FEC, st);
  k_fec_xcch_encode<<<dim3(nblk), dim3(64), 0, st>>>(frames, nblk, tsc_bits, bits);
  if (prof) prof->end(TRXSIG_K_FEC, st);
  return hipGetLastError();
}

hipError_t trx_launch_fec(hipStream_t st, int mode, const float *soft, long long in_stride, int n, int nout, int nblk,
                          int wire, uint8_t *out0, uint8_t *out1, uint8_t *out2, long long out_stride, TrxProfiler *prof,
                          int ilv8) {
  if (nblk <= 0) return hipSuccess;
  if (nout <= 0 || nout > 512 || n < 0 || n > 2 * nout) return hipErrorInvalidValue;
  const dim3 grid((nblk + 3) / 4), block(64);
  if (prof) prof->begin(TRXSIG_K_FEC, st);
  switch (mode) {
    case FEC_GENERIC: k_fec_viterbi<FEC_GENERIC><<<grid, block, 0, st>>>(soft, in_stride, n, nout, nblk, wire, ilv8, out0, out1, out2, out_stride); break;
    case FEC_XCCH: k_fec_viterbi<FEC_XCCH><<<grid, block, 0, st>>>(soft, in_stride, n, nout, nblk, wire, ilv8, out0, out1, out2, out_stride); break;
    case FEC_RACH: k_fec_viterbi<FEC_RACH><<<grid, block, 0, st>>>(soft, in_stride, n, nout, nblk, wire, ilv8, out0, out1, out2, out_stride); break;
    case FEC_TCH: k_fec_viterbi<FEC_TCH><<<grid, block, 0, st>>>(soft, in_stride, n, nout, nblk, wire, ilv8, out0, out1, out2, out_stride); break;
    case FEC_SCH: k_fec_viterbi<FEC_SCH><<<grid, block, 0, st>>>(soft, in_stride, n, nout, nblk, wire, ilv8, out0, out1, out2, out_stride); break;
    default: return hipErrorInvalidValue;
  }
  if (prof) prof->end(TRXSIG_K_FEC, st);
  return hipGetLastError();
}

hipError_t trx_launch_fec_tch_encode(hipStream_t st, int n_chan, int n_blocks, const uint8_t *kinds, const uint8_t *payload,
                                     const uint8_t *tscs, const uint8_t *tsc_bits, const uint8_t *filler, uint8_t *state,
                                     uint8_t *bits, TrxProfiler *prof) {
  if (n_chan <= 0 || n_blocks <= 0) return hipSuccess;
  const dim3 grid((unsigned)((long long)n_chan * n_blocks)), block(64);
  if (prof) prof->begin(TRXSIG_K_FEC_TCH_ENC, st);
  if (((uintptr_t)bits & 15) == 0)
    k_fec_tch_encode<true><<<grid, block, 0, st>>>(n_blocks, kinds, payload, tscs, tsc_bits, filler, state, bits);
  else
    k_fec_tch_encode<false><<<grid, block, 0, st>>>(n_blocks, kinds, payload, tscs, tsc_bits, filler, state, bits);
  if (prof) prof->end(TRXSIG_K_FEC_TCH_ENC, st);
  return hipGetLastError();
}

hipError_t trx_launch_fec_sch_encode(hipStream_t st, const uint32_t *fns, const uint8_t *bsics, int n, unsigned long long xts,
                                     uint8_t *bits, TrxProfiler *prof) {
  if (n <= 0) return hipSuccess;
  const dim3 grid((unsigned)((n + 3) / 4)), block(64);
  if (prof) prof->begin(TRXSIG_K_FEC_SCH_ENC, st);
  if (((uintptr_t)bits & 3) == 0)
    k_fec_sch_encode<true><<<grid, block, 0, st>>>(fns, bsics, n, xts, bits);
  else
    k_fec_sch_encode<false><<<grid, block, 0, st>>>(fns, bsics, n, xts, bits);
  if (prof) prof->end(TRXSIG_K_FEC_SCH_ENC, st);
  return hipGetLastError();
}

hipError_t trx_launch_fec_rx_stream(hipStream_t st, int tch, int n_chan, int n_slots, const float *soft, long long stride,
                                    long long n_rows, const int32_t *index, const uint8_t *b0, int wire, uint8_t *state,
                                    uint8_t *status, uint8_t *out_tch, uint8_t *out_l2, float *fer, TrxProfiler *prof) {
  if (n_chan <= 0 || n_slots <= 0) return hipSuccess;
  if (n_slots & 3) return hipErrorInvalidValue;
  const RxStream a = { soft, stride, n_rows, index, tch ? b0 : nullptr, n_chan, n_slots, wire };
  // the host allows n_chan * n_blocks < 2^29 code words, 2^27 workgroups of 64: 2^33 work-items, but a dispatch counts its
  // work-items in 32 bits.  So both kernels go out in slices of at most kRxSlice workgroups (one launch at any bench shape).
  constexpr long long kRxSlice = 1LL << 24;
  const long long nblk = (long long)n_chan * (n_slots / 4), ngrp = (nblk + 3) / 4;
  const dim3 block(64);
  const int id = tch ? TRXSIG_K_FEC_TCH_RX : TRXSIG_K_FEC_XCCH_RX;
  if (prof) prof->begin(id, st);
  for (long long g0 = 0; g0 < ngrp; g0 += kRxSlice) {
    const dim3 grid((unsigned)(ngrp - g0 < kRxSlice ? ngrp - g0 : kRxSlice));
    if (tch) k_fec_rx_stream<true><<<grid, block, 0, st>>>(a, (int)(4 * g0), state, status, out_tch, out_l2);
    else k_fec_rx_stream<false><<<grid, block, 0, st>>>(a, (int)(4 * g0), state, status, out_tch, out_l2);
  }
  if (prof) prof->end(id, st);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  if (prof) prof->begin(TRXSIG_K_FEC_RX_FOLD, st);
  for (long long c0 = 0; c0 < n_chan; c0 += kRxSlice) {
    const dim3 grid((unsigned)(n_chan - c0 < kRxSlice ? n_chan - c0 : kRxSlice));
    if (tch) k_fec_rx_fold<true><<<grid, block, 0, st>>>(a, (int)c0, state, status, reinterpret_cast<uint8_t *>(fer));
    else k_fec_rx_fold<false><<<grid, block, 0, st>>>(a, (int)c0, state, status, reinterpret_cast<uint8_t *>(fer));
  }
  if (prof) prof->end(TRXSIG_K_FEC_RX_FOLD, st);
  return hipGetLastError();
}

hipError_t trx_launch_fec_pdtch_encode(hipStream_t st, const uint8_t *blocks, const uint8_t *cs, const uint8_t *tsc, int nblk,
                                       const uint8_t *tsc_bits, uint8_t *bits, TrxProfiler *prof) {
  if (nblk <= 0) return hipSuccess;
  const dim3 grid((unsigned)nblk), block(64);
  if (prof) prof->begin(TRXSIG_K_FEC, st);
  if (((uintptr_t)bits & 15) == 0)
    k_fec_pdtch_encode<true><<<grid, block, 0, st>>>(blocks, cs, tsc, nblk, tsc_bits, bits);
  else
    k_fec_pdtch_encode<false><<<grid, block, 0, st>>>(blocks, cs, tsc, nblk, tsc_bits, bits);
  if (prof) prof->end(TRXSIG_K_FEC, st);
  return hipGetLastError();
}

hipError_t trx_launch_fec_pdtch_decode(hipStream_t st, const float *soft, long long stride, long long n_rows, const int32_t *index,
                                       int nblk, int wire, int cs_force, uint8_t *blocks, uint8_t *cs, uint8_t *dist, uint8_t *ok,
                                       uint8_t *usf, TrxProfiler *prof) {
  if (nblk <= 0) return hipSuccess;
  if (cs_force < -1 || cs_force > 3) return hipErrorInvalidValue;
  const PdDecode a = { soft, stride, n_rows, index, nblk, cs_force, blocks, cs, dist, ok, usf };
  const dim3 grid((unsigned)((nblk + 3) / 4)), block(64);
  if (prof) prof->begin(TRXSIG_K_FEC, st);
  if (wire) k_fec_pdtch_decode<true><<<grid, block, 0, st>>>(a);
  else k_fec_pdtch_decode<false><<<grid, block, 0, st>>>(a);
  if (prof) prof->end(TRXSIG_K_FEC, st);
  return hipGetLastError();
}

hipError_t trx_launch_fec_access_encode(hipStream_t st, const uint16_t *ra, const uint8_t *fmt, const uint8_t *bsic, int n,
                                        uint8_t *bits, TrxProfiler *prof) {
  if (n <= 0) return hipSuccess;
  const dim3 grid((unsigned)((n + 3) / 4)), block(64);
  if (prof) prof->begin(TRXSIG_K_FEC, st);
  if (((uintptr_t)bits & 3) == 0)
    k_fec_access_encode<true><<<grid, block, 0, st>>>(ra, fmt, bsic, n, bits);
  else
    k_fec_access_encode<false><<<grid, block, 0, st>>>(ra, fmt, bsic, n, bits);
  if (prof) prof->end(TRXSIG_K_FEC, st);
  return hipGetLastError();
}

hipError_t trx_launch_fec_access_decode(hipStream_t st, const float *soft, long long stride, long long n_rows, const int32_t *index,
                                        int n, int wire, int fmt, int bsic, uint16_t *ra, uint8_t *ofmt, uint8_t *tail_ok,
                                        uint8_t *obsic, TrxProfiler *prof) {
  if (n <= 0) return hipSuccess;
  if (fmt < -1 || fmt > 1 || (fmt < 0 && (bsic < 0 || bsic > 63))) return hipErrorInvalidValue;
  const AccDecode a = { soft, stride, n_rows, index, n, fmt, bsic, ra, ofmt, tail_ok, obsic };
  const dim3 grid((unsigned)((n + 3) / 4)), block(64);
  if (prof) prof->begin(TRXSIG_K_FEC, st);
  if (wire) k_fec_access_decode<true><<<grid, block, 0, st>>>(a);
  else k_fec_access_decode<false><<<grid, block, 0, st>>>(a);
  if (prof) prof->end(TRXSIG_K_FEC, st);
  return hipGetLastError();
}
