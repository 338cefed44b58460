// trxsig_l1pdch.hip -- the packet data channel object's kernels (include/trxsig_l1pdch.h, host side in trxsig_l1pdch.cpp).  The
// block coder and decoder exist once, in trxsig_fec.hip: the host runs k_fec_pdtch_encode between k_l1pdch_stage and
// k_l1pdch_mux, and k_fec_pdtch_decode between k_l1pdch_demux and k_l1pdch_fold.  Every channel of a class has the same block
// geometry (one mapping per class), so the host computes it once per call (TrxL1pdchEnc / TrxL1pdchDec) and the kernels do the
// per-frame arithmetic of trxsig_l1pdch_dev.h: unsigned, 32-bit, division by constants only.
//
// Encode.
//   k_l1pdch_stage: a wave per (channel, block that starts in the call): the payload into the coder's row of 54 octets (PTCCH:
//     23 and zeros), the coder's scheme -- 255, which it encodes as four zero bursts, where nothing is sent -- and the TSC.
//   k_l1pdch_mux: a wave per (channel, frame of the call).  On a frame the channel owns, the burst comes from the coder's output
//     (a block that started in the call and is sent) or from the record (the block pending from earlier calls); 37 lanes move
//     four bytes each, lane 0 writes the what byte.  Nothing else of the grid is touched.
//   k_l1pdch_commit: a wave per channel, after the mux, in place (it reads the coder's output and its own record only): the
//     block that straddles the call's end becomes the pending one; the USF ring takes the blocks sent, a lane per ring entry.
// Decode.
//   k_l1pdch_demux: a wave per (channel, block with a burst frame in the call): each of the four bursts from the pull (d_row >=
//     0, d_valid set) or from the carried rows, the count so far, the closing FN; the rows of a block that closes in the call
//     gathered for the decoder with their index.
//   k_l1pdch_fold: after the decoder, a wave per (channel, block): the outputs into the [n][nb] grids (empty and open blocks),
//     d_granted from the sibling's ring; the block 0 wave also finds the channel's last accepted row (RSSI / timing:
//     k_l1rx_demux_phy) and writes the carry for the next call, in place.
#include "trxsig_l1pdch_dev.h"

namespace {

constexpr int kWhatPdch = 8;                                 // TRXSIG_L1TX_PDCH

__device__ __forceinline__ int pd_class(int g, int n_pd, int *ci) {
  if (g < n_pd) { *ci = g; return 0; }
  *ci = g - n_pd;
  return 1;
}

__global__ __launch_bounds__(256) void k_l1pdch_stage(TrxL1pdchEnc e, int g0) {
  const int lane = threadIdx.x & 63, b = blockIdx.x * 4 + (threadIdx.x >> 6), g = (int)blockIdx.y + g0;
  int ci = 0;
  const int cls = pd_class(g, e.n_pd, &ci);
  if (b >= e.nb[cls]) return;
  const size_t gi = (size_t)ci * e.nb[cls] + b, unit = (size_t)e.unit0[cls] + gi;
  const unsigned cs = cls == 0 ? e.cs[gi] : 0u;
  const bool sent = e.kind[cls][gi] == 1 && cs <= 3u;
  if (lane < 54) {
    uint8_t v = 0;
    if (cls == 0) v = e.payload[0][gi * 54 + lane];
    else if (lane < 23) v = e.payload[1][gi * 23 + lane];
    e.stage[unit * 54 + lane] = v;
  }
  if (lane == 0) { e.cs_eff[unit] = sent ? (uint8_t)cs : (uint8_t)255; e.tscs[unit] = (uint8_t)e.tsc; }
}

__global__ __launch_bounds__(256) void k_l1pdch_mux(TrxL1pdchEnc e, int g0) {
  const int lane = threadIdx.x & 63, k = blockIdx.x * 4 + (threadIdx.x >> 6), g = (int)blockIdx.y + g0;
  if (k >= e.n_frames) return;
  int ci = 0;
  const int cls = pd_class(g, e.n_pd, &ci);
  const unsigned u = (unsigned)e.fn + (unsigned)k;
  if (!pd_owns(cls, u)) return;
  const unsigned q = pd_pos_before(cls, u), blk = q >> 2, t = q & 3u;
  const uint8_t *src = nullptr;
  if (blk >= e.bf[cls]) {
    const size_t unit = (size_t)e.unit0[cls] + (size_t)ci * e.nb[cls] + (blk - e.bf[cls]);
    if (e.cs_eff[unit] <= 3) src = e.ebits + unit * 592 + t * 148;
  } else {
    const TrxL1pdchChan &S = e.st[g];
    if (S.pend_blk == pd_abs(cls, blk)) src = S.bits[t];
  }
  if (!src) return;
  const int info = e.chinfo[g], a = info & 0xffff, tn = info >> 16;
  const size_t slot = (size_t)a * 8 * (size_t)e.n_frames + 8 * (size_t)k + tn;
  uint8_t *dst = e.bits + slot * 148;
  if (lane < 37) {
    const unsigned v = *reinterpret_cast<const unsigned *>(src + 4 * lane);   // both sources are 4-byte aligned
    if (((uintptr_t)dst & 3) == 0) *reinterpret_cast<unsigned *>(dst + 4 * lane) = v;
    else for (int i = 0; i < 4; i++) dst[4 * lane + i] = (uint8_t)(v >> (8 * i));
  }
  if (lane == 0) e.what[slot] = kWhatPdch;
}

__global__ __launch_bounds__(256) void k_l1pdch_commit(TrxL1pdchEnc e) {
  const int lane = threadIdx.x & 63, g = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (g >= e.n_pd + e.n_pt) return;
  int ci = 0;
  const int cls = pd_class(g, e.n_pd, &ci);
  TrxL1pdchChan &S = e.st[g];
  const int nb = e.nb[cls];
  const size_t unit0 = (size_t)e.unit0[cls] + (size_t)ci * nb;
  // the USF ring: entry s takes the last block sent whose number is s modulo the ring (32 divides the wrap of the numbers)
  if (e.down && cls == 0 && lane < kPdRing) {
    const int r = (int)(((unsigned)lane - e.bf[0]) & (kPdRing - 1));
    for (int b = r + kPdRing * ((nb - 1 - r) / kPdRing); b >= 0 && r < nb; b -= kPdRing) {
      if (e.cs_eff[unit0 + b] > 3) continue;
      S.ring[lane] = (pd_abs(0, e.bf[0] + b) << 8) | (e.stage[(unit0 + b) * 54] & 7);
      break;
    }
  }
  // the block that straddles the call's end
  const unsigned pe = e.p_end[cls], blk = pe >> 2;
  int pend = -1;
  const uint8_t *src = nullptr;
  bool keep = false;
  if (pe & 3u) {
    if (blk >= e.bf[cls]) {
      const size_t unit = unit0 + (blk - e.bf[cls]);
      if (e.cs_eff[unit] <= 3) { pend = pd_abs(cls, blk); src = e.ebits + unit * 592; }
    } else if (S.pend_blk == pd_abs(cls, blk)) {
      keep = true;
    }
  }
  if (keep) return;
  unsigned *w = reinterpret_cast<unsigned *>(&S.bits[0][0]);
  for (int i = lane; i < 148; i += 64) w[i] = src ? reinterpret_cast<const unsigned *>(src)[i] : 0u;
  if (lane == 0) { S.pend_blk = pend; S.pad = 0; }
}

// burst t of block blk of channel (cls, a, tn): the pull's accepted row, or -1
struct PdBurst { int row; bool carried; };
__device__ __forceinline__ PdBurst pd_burst(const TrxL1pdchDec &d, const TrxL1pdchChan &S, int cls, int a, int tn, unsigned blk,
                                            int t) {
  PdBurst o{ -1, false };
  const unsigned q = 4u * blk + (unsigned)t;
  if (q >= d.p_end[cls]) return o;
  if (q >= d.p_first[cls]) {
    const unsigned k = pd_frame(cls, q) - (unsigned)d.fn;
    const int r = d.row[((size_t)8 * k + tn) * (size_t)d.n_arfcn + a];
    if (r >= 0 && r < d.n_rows && d.valid[r] != 0) o.row = r;
  } else {
    o.carried = S.carry_blk == pd_abs(cls, blk) && ((S.carry_have >> t) & 1u);
  }
  return o;
}

__global__ __launch_bounds__(256) void k_l1pdch_demux(TrxL1pdchDec d, int g0) {
  const int lane = threadIdx.x & 63, j = blockIdx.x * 4 + (threadIdx.x >> 6), g = (int)blockIdx.y + g0;
  int ci = 0;
  const int cls = pd_class(g, d.n_pd, &ci);
  if (j >= d.nb[cls]) return;
  const int info = d.chinfo[g], a = info & 0xffff, tn = info >> 16;
  const TrxL1pdchChan &S = d.st[g];
  const unsigned blk = d.blk0[cls] + (unsigned)j;
  const bool closing = j < d.nclose[cls];
  const size_t gi = (size_t)ci * d.nb[cls] + j;
  const size_t unit = (size_t)d.unit0[cls] + (size_t)ci * d.nclose[cls] + j;   // used where closing
  int count = 0;
  for (int t = 0; t < 4; t++) {
    const PdBurst b = pd_burst(d, S, cls, a, tn, blk, t);
    const bool have = b.row >= 0 || b.carried;
    count += have;
    if (!closing) continue;
    float *o = d.rows + (unit * 4 + t) * 148;
    const float *s = b.row >= 0 ? d.soft + (size_t)b.row * d.soft_stride : S.carry[t];
    for (int i = lane; i < 148; i += 64) o[i] = have ? s[i] : 0.0F;
    if (lane == 0) d.index[unit * 4 + t] = have ? (int32_t)(unit * 4 + t) : -1;
  }
  if (lane == 0) {
    d.nbur[cls][gi] = (uint8_t)count;
    const unsigned f = pd_frame(cls, 4u * blk + 3u);
    d.bfn[cls][gi] = closing ? (int32_t)(f >= kPdHyper ? f - kPdHyper : f) : -1;
  }
}

__global__ __launch_bounds__(256) void k_l1pdch_fold(TrxL1pdchDec d, int g0) {
  const int lane = threadIdx.x & 63, j = blockIdx.x * 4 + (threadIdx.x >> 6), g = (int)blockIdx.y + g0;
  int ci = 0;
  const int cls = pd_class(g, d.n_pd, &ci);
  const int nb = d.nb[cls];
  if (j >= nb) return;
  const unsigned blk = d.blk0[cls] + (unsigned)j;
  const size_t gi = (size_t)ci * nb + j;
  const int np = cls == 0 ? 54 : 23;
  const bool dec = j < d.nclose[cls] && d.nbur[cls][gi] != 0;
  const size_t unit = (size_t)d.unit0[cls] + (size_t)ci * d.nclose[cls] + j;
  if (lane < np) d.payload[cls][gi * np + lane] = dec ? d.t_payload[unit * 54 + lane] : (uint8_t)0;
  if (lane == 0) {
    d.cs[cls][gi] = dec ? d.t_cs[unit] : (uint8_t)255;
    d.dist[cls][gi] = dec ? d.t_dist[unit] : (uint8_t)255;
    d.ok[cls][gi] = dec ? d.t_ok[unit] : (uint8_t)0;
    d.usf[cls][gi] = dec ? d.t_usf[unit] : (uint8_t)255;
    int gr = 255;
    if (cls == 0 && d.sib) {
      const int n = pd_abs(0, blk), m = n == 0 ? 12 * 52224 - 1 : n - 1;
      const int ent = d.sib[ci].ring[m & (kPdRing - 1)];
      if (ent >= 0 && (ent >> 8) == m) gr = ent & 255;
    }
    d.granted[cls][gi] = (uint8_t)gr;
  }
  if (j != 0) return;
  // the channel's own: its last accepted row of the call, and the carry (the last block shown, if it stays open)
  const int info = d.chinfo[g], a = info & 0xffff, tn = info >> 16;
  TrxL1pdchChan &S = d.st[g];
  int last = -1;
  const unsigned p0 = d.p_first[cls], n_pos = d.p_end[cls] - p0;
  for (unsigned s0 = 0; s0 < n_pos; s0 += 64) {
    const unsigned s = s0 + (unsigned)lane;
    int r = -1;
    if (s < n_pos) r = pd_burst(d, S, cls, a, tn, (p0 + s) >> 2, (int)((p0 + s) & 3u)).row;
    const unsigned long long bal = __ballot(r >= 0);
    if (bal) last = __shfl(r, 63 - __clzll((long long)bal));
  }
  if (lane == 0) d.last[g] = last;
  const unsigned bl = d.blk0[cls] + (unsigned)(nb - 1);
  const bool open = nb > d.nclose[cls];
  unsigned have = 0;
  for (int t = 0; t < 4; t++) {
    PdBurst b{ -1, false };
    if (open) b = pd_burst(d, S, cls, a, tn, bl, t);
    if (b.row >= 0 || b.carried) have |= 1u << t;
    if (b.carried) continue;                                  // the row stays where it is
    const float *s = d.soft + (size_t)(b.row >= 0 ? b.row : 0) * d.soft_stride;
    for (int i = lane; i < 148; i += 64) S.carry[t][i] = b.row >= 0 ? s[i] : 0.0F;
  }
  if (lane == 0) { S.carry_blk = open ? pd_abs(cls, bl) : -1; S.carry_have = have; }
}

// grid (x, channels): the y dimension in slices a dispatch can take
template <class L>
void pd_slices(int nx, int n_chan, L launch) {
  constexpr int kMaxY = 32768;
  for (int g0 = 0; g0 < n_chan; g0 += kMaxY)
    launch(dim3((unsigned)nx, (unsigned)(n_chan - g0 < kMaxY ? n_chan - g0 : kMaxY)), g0);
}

}  // namespace

hipError_t trx_launch_l1pdch_stage(hipStream_t st, const TrxL1pdchEnc &e, TrxProfiler *prof) {
  const int nbm = e.nb[0] > e.nb[1] ? e.nb[0] : e.nb[1], n = e.n_pd + e.n_pt;
  if (nbm <= 0 || n <= 0) return hipSuccess;
  if (prof) prof->begin(TRXSIG_K_FEC, st);
  pd_slices((nbm + 3) / 4, n, [&](dim3 grid, int g0) { k_l1pdch_stage<<<grid, dim3(256), 0, st>>>(e, g0); });
  if (prof) prof->end(TRXSIG_K_FEC, st);
  return hipGetLastError();
}

hipError_t trx_launch_l1pdch_mux(hipStream_t st, const TrxL1pdchEnc &e, TrxProfiler *prof) {
  const int n = e.n_pd + e.n_pt;
  if (n <= 0) return hipSuccess;
  if (prof) prof->begin(TRXSIG_K_FEC, st);
  pd_slices((e.n_frames + 3) / 4, n, [&](dim3 grid, int g0) { k_l1pdch_mux<<<grid, dim3(256), 0, st>>>(e, g0); });
  k_l1pdch_commit<<<dim3((unsigned)((n + 3) / 4)), dim3(256), 0, st>>>(e);
  if (prof) prof->end(TRXSIG_K_FEC, st);
  return hipGetLastError();
}

hipError_t trx_launch_l1pdch_demux(hipStream_t st, const TrxL1pdchDec &d, TrxProfiler *prof) {
  const int nbm = d.nb[0] > d.nb[1] ? d.nb[0] : d.nb[1], n = d.n_pd + d.n_pt;
  if (nbm <= 0 || n <= 0) return hipSuccess;
  if (prof) prof->begin(TRXSIG_K_FEC, st);
  pd_slices((nbm + 3) / 4, n, [&](dim3 grid, int g0) { k_l1pdch_demux<<<grid, dim3(256), 0, st>>>(d, g0); });
  if (prof) prof->end(TRXSIG_K_FEC, st);
  return hipGetLastError();
}

hipError_t trx_launch_l1pdch_fold(hipStream_t st, const TrxL1pdchDec &d, TrxProfiler *prof) {
  const int nbm = d.nb[0] > d.nb[1] ? d.nb[0] : d.nb[1], n = d.n_pd + d.n_pt;
  if (nbm <= 0 || n <= 0) return hipSuccess;
  if (prof) prof->begin(TRXSIG_K_FEC, st);
  pd_slices((nbm + 3) / 4, n, [&](dim3 grid, int g0) { k_l1pdch_fold<<<grid, dim3(256), 0, st>>>(d, g0); });
  if (prof) prof->end(TRXSIG_K_FEC, st);
  return hipGetLastError();
}
