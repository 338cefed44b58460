// trxsig_tdma.h -- internal: the TDMA mappings of GSM 05.02 in both directions -- the numbers of GSM/GSMTDMA.cpp's TDMAMapping
// tables (repeat length, frame list in reverse-mapping order) -- with the position arithmetic over them, the SACCH rule and the
// power-level tables, and the by-value structs of the stages that walk them: the uplink demultiplexer (trxsig_l1rx) and the two
// transmit multiplexers (trxsig_l1tx here, trxsig_l1ms in trxsig_l1ms_dev.h), whose common part is TrxMuxCall / TrxMuxChan /
// TrxMuxDev below and the device code of trxsig_l1mux_dev.h.  tests/golden/tdma_uplink.npz and tdma_downlink.npz record the
// same tables for the CPU models (tests/l1_demux_model.py, tests/l1_mux_model.py).
//
// Positions.  A mapping with n frames per repeat R numbers its bursts in time order: the burst of frame u (an unwrapped frame
// count) sits at position p(u) = n * floor((u - f[0]) / R) + r, where f[r] == u mod R.  Because f[r] - f[0] (mod R) grows with r
// (checked at create), positions grow with time and p mod n is reverseMapping(u) -- so p mod 4 is the XCCH decoders' B and, with
// n = 24, p mod 8 the TCH decoder's.  R divides 5304 and 5304 divides the hyperframe, so the numbering is the same modulo the
// hyperframe wrap up to a multiple of n * 5304 / R positions (a whole number of blocks).
#pragma once
#include <stddef.h>
#include <stdint.h>

// TRX_TDMA_TABLES_ONLY (trxsig_plan.cpp, which a plain host compiler builds too): the tables, the position arithmetic and the
// structs, without the launch declarations -- those need trxsig_launch.h before this file
#if defined(TRX_TDMA_TABLES_ONLY) && !defined(__HIPCC__)
#define __host__
#define __device__
#endif

enum {
  TRX_MAP_TCHF = 0,            // FACCH_TCHF
  TRX_MAP_SACCH_TF = 1,        // + TN: SACCH_TF_T0..T7
  TRX_MAP_SDCCH8 = 9,          // + sub-channel: SDCCH_8_0U..7U
  TRX_MAP_SACCH_C8 = 17,       // + sub-channel: SACCH_C8_0U..7U
  TRX_MAP_SDCCH4 = 25,         // + sub-channel: SDCCH_4_0U..3U
  TRX_MAP_SACCH_C4 = 29,       // + sub-channel: SACCH_C4_0U..3U
  TRX_MAP_RACH_C5 = 33,        // RACHC5
  TRX_N_MAPS = 34
};

struct TrxTdmaMap {
  int16_t R, n;
  int16_t f[27];
};

#define TRX_M4(R, a, b, c, d) { R, 4, { a, b, c, d } }
#define TRX_TDMA_MAPS_INIT                                                                                                   \
  {                                                                                                                          \
    { 26, 24, { 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 14, 15, 16, 17, 18, 19, 20, 21, 22, 23, 24 } },                    \
    TRX_M4(104, 12, 38, 64, 90), TRX_M4(104, 25, 51, 77, 103), TRX_M4(104, 38, 64, 90, 12), TRX_M4(104, 51, 77, 103, 25),  \
    TRX_M4(104, 64, 90, 12, 38), TRX_M4(104, 77, 103, 25, 51), TRX_M4(104, 90, 12, 38, 64), TRX_M4(104, 103, 25, 51, 77),  \
    TRX_M4(51, 15, 16, 17, 18), TRX_M4(51, 19, 20, 21, 22), TRX_M4(51, 23, 24, 25, 26), TRX_M4(51, 27, 28, 29, 30),        \
    TRX_M4(51, 31, 32, 33, 34), TRX_M4(51, 35, 36, 37, 38), TRX_M4(51, 39, 40, 41, 42), TRX_M4(51, 43, 44, 45, 46),        \
    TRX_M4(102, 47, 48, 49, 50), TRX_M4(102, 51, 52, 53, 54), TRX_M4(102, 55, 56, 57, 58), TRX_M4(102, 59, 60, 61, 62),    \
    TRX_M4(102, 98, 99, 100, 101), TRX_M4(102, 0, 1, 2, 3), TRX_M4(102, 4, 5, 6, 7), TRX_M4(102, 8, 9, 10, 11),            \
    TRX_M4(51, 37, 38, 39, 40), TRX_M4(51, 41, 42, 43, 44), TRX_M4(51, 47, 48, 49, 50), TRX_M4(51, 0, 1, 2, 3),            \
    TRX_M4(102, 57, 58, 59, 60), TRX_M4(102, 61, 62, 63, 64), TRX_M4(102, 6, 7, 8, 9), TRX_M4(102, 10, 11, 12, 13),        \
    { 51, 27, { 4, 5, 14, 15, 16, 17, 18, 19, 20, 21, 22, 23, 24, 25, 26, 27, 28, 29, 30, 31, 32, 33, 34, 35, 36, 45, 46 } } \
  }

constexpr int kTrxHyperframe = 2715648;   // 2048 * 26 * 51

// floor division for a positive divisor
__host__ __device__ inline long long trx_fdiv(long long a, long long b) { return a >= 0 ? a / b : -((-a + b - 1) / b); }

// the frame (unwrapped) of position q of mapping m
__host__ __device__ inline long long trx_map_frame(const TrxTdmaMap &m, long long q) {
  const long long k = trx_fdiv(q, m.n), r = q - k * m.n;
  return m.f[0] + k * m.R + ((m.f[r] - m.f[0] + m.R) % m.R);
}

// the number of positions of mapping m in frames before u (the position of the first burst at or after frame u)
__host__ __device__ inline long long trx_map_count(const TrxTdmaMap &m, long long u) {
  const long long d = u - m.f[0], k = trx_fdiv(d, m.R), rem = d - k * m.R;
  long long c = k * m.n;
  for (int r = 0; r < m.n; r++) c += ((m.f[r] - m.f[0] + m.R) % m.R) < rem;
  return c;
}

// GSM 05.05 4.1.1 power control levels -> dBm, SACCHL1Decoder's decodePower (GSM/GSML1FEC.cpp): 0 = GSM850 / EGSM900,
// 1 = DCS1800, 2 = PCS1900
#define TRX_POWER_TABLES_INIT                                                                                     \
  {                                                                                                               \
    { 39, 39, 39, 37, 35, 33, 31, 29, 27, 25, 23, 21, 19, 17, 15, 13, 11, 9, 7, 5, 5, 5, 5, 5, 5, 5, 5, 5, 5, 5, 5, 5 }, \
    { 30, 28, 26, 24, 22, 20, 18, 16, 14, 12, 10, 8, 6, 4, 2, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 36, 24, 23 },     \
    { 30, 28, 26, 24, 22, 20, 18, 16, 14, 12, 10, 8, 6, 4, 2, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0 }         \
  }

// whether mapping m is a SACCH: ids below 33 name the same logical channel in both directions' tables
__host__ __device__ inline bool trx_map_is_sacch(int m) {
  return (m >= TRX_MAP_SACCH_TF && m < TRX_MAP_SDCCH8) || (m >= TRX_MAP_SACCH_C8 && m < TRX_MAP_SDCCH4) ||
         (m >= TRX_MAP_SACCH_C4 && m < TRX_MAP_RACH_C5);
}

// encodePower over a band's row of the tables above: nearest code, first on ties, an exact match at once
__host__ __device__ inline int trx_encode_power(const int8_t *row, int power) {
  unsigned minErr = (unsigned)(power < row[0] ? row[0] - power : power - row[0]), code = 0;
  for (int i = 1; i < 32; i++) {
    const unsigned e = (unsigned)(power < row[i] ? row[i] - power : power - row[i]);
    if (e == 0) return i;
    if (e < minErr) { minErr = e; code = (unsigned)i; }
  }
  return (int)code;
}

// what the demux kernel and the fold need of one call (by value)
struct TrxL1rxCall {
  int fn, n_frames, n_arfcn, n_rows, soft_stride, sps;
  int n_tch, n_xcch, n_rach, nb_tch, nb_xcch, rach_cap, band;
  int32_t blk_first[TRX_N_MAPS];   // per mapping: floor(first position at or after fn / 4)
  long long p_first[TRX_N_MAPS];   // per mapping: the first position at or after fn
};

// the device side of one object (pointers into its allocations)
struct TrxL1rxDev {
  const int32_t *chinfo;           // [n_all]: arfcn | tn << 16 | map << 20
  const uint8_t *active;           // [n_all]
  int32_t *rssi, *timing;          // [n_all]: the last accepted burst's, as the decoder records them
  int32_t *ms_power, *ms_ta;       // [n_xcch]: SACCH actuals, -1 on channels that are not SACCH
  int32_t *tch_index, *xcch_index; // [n_tch][4 nb_tch], [n_xcch][4 nb_xcch]
  uint8_t *tch_b0;                 // [n_tch]
  int32_t *tch_fn, *xcch_fn;       // closing frame numbers [..][nb]
  const uint8_t *xcch_status, *xcch_frames;
  float *rach_soft;                // [rach_cap][148] gathered rows
  int32_t *rach_fn, *rach_arfcn, *rach_rssi, *rach_timing, *rach_count;
  uint8_t *rach_tail, *rach_bsic, *rach_ra, *rach_ok;
  uint32_t *accepted;              // [n_all]: bursts each channel has accepted since create (the downlink's phyNew, trxsig_l1tx)
  int bsic;
};

#ifndef TRX_TDMA_TABLES_ONLY
// The receive sides' finish (k_l1rx_finish, k_l1msrx_finish), a thread per SACCH channel: channel i's power / TA folded over the
// call's good SACCH frames (SACCHL1Decoder::handleGoodFrame): octet 0's bits 3..7 are the level (mU.peekField(3,5)), octet 1's
// low seven the TA, kept where below 64 (mU.peekField(9,7)).  levels: the band's row of the tables above
__device__ inline void trx_sacch_fold(const uint8_t *status, const uint8_t *frames, int nb, int i, const int8_t *levels,
                                      int32_t *power, int32_t *ta) {
  int pw = power[i], t = ta[i];
  for (int b = 0; b < nb; b++) {
    const size_t k = (size_t)i * nb + b;
    if ((status[k] & (TRXSIG_FEC_DECODED | TRXSIG_FEC_TCH_GOOD)) != (TRXSIG_FEC_DECODED | TRXSIG_FEC_TCH_GOOD)) continue;
    const uint8_t *fr = frames + k * 23;
    pw = levels[fr[0] & 31];
    const int taf = fr[1] & 127;
    if (taf < 64) t = taf;
  }
  power[i] = pw;
  ta[i] = t;
}

hipError_t trx_launch_l1rx_demux(hipStream_t st, const TrxL1rxCall &call, const TrxL1rxDev &dv, const int32_t *row,
                                 const uint8_t *valid, const float *soft, const trx_c32 *amp, const float *toa, TrxProfiler *prof);
hipError_t trx_launch_l1rx_finish(hipStream_t st, const TrxL1rxCall &call, const TrxL1rxDev &dv, TrxProfiler *prof);
// burst_phy (trxsig_l1_phy.h) for n channels: channel ch's RSSI / timing from row last[ch] of amp / toa; last[ch] < 0 keeps them
hipError_t trx_launch_l1rx_phy(hipStream_t st, const int32_t *last, int n, const trx_c32 *amp, const float *toa, int sps,
                               int32_t *rssi, int32_t *timing);
// open (1) / close (0) channel `ch` of the object (index over all classes): the active flag; on open also FER = 0 (state_fer)
// and, where `sacch`, power 40 / TA 0 (ms_power / ms_ta, unused otherwise)
hipError_t trx_launch_l1rx_set(hipStream_t st, uint8_t *active, int ch, int open, uint8_t *state_fer, int32_t *ms_power,
                               int32_t *ms_ta, int sacch);
#endif

// ---- the downlink (trxsig_l1tx.h) ----------------------------------------------------------------------------------------
// GSM/GSMTDMA.cpp's downlink TDMAMapping tables: the *D tables of SDCCH/8, SACCH/C8, SDCCH/4 and SACCH/C4, FACCH_TCHF and
// SACCH_TF_Tn (which serve both directions), and combination V's beacon: CCCH_0..2, BCCH, SCH, FCCH.  Ids 0..32 name the same
// logical channels as the uplink ids above (TRX_MAP_TCHF .. TRX_MAP_SACCH_C4 + 3); positions are numbered as above.
// tests/golden/tdma_downlink.npz records the same tables for the CPU model (tests/l1_mux_model.py).
enum {
  TRX_DL_CCCH = 33,            // + sub-channel: CCCH_0..2
  TRX_DL_BCCH = 36,
  TRX_DL_SCH = 37,
  TRX_DL_FCCH = 38,
  TRX_N_DL_MAPS = 39
};

#define TRX_M5(R, a, b, c, d, e) { R, 5, { a, b, c, d, e } }
#define TRX_TDMA_DL_MAPS_INIT                                                                                                \
  {                                                                                                                          \
    { 26, 24, { 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 14, 15, 16, 17, 18, 19, 20, 21, 22, 23, 24 } },                    \
    TRX_M4(104, 12, 38, 64, 90), TRX_M4(104, 25, 51, 77, 103), TRX_M4(104, 38, 64, 90, 12), TRX_M4(104, 51, 77, 103, 25),  \
    TRX_M4(104, 64, 90, 12, 38), TRX_M4(104, 77, 103, 25, 51), TRX_M4(104, 90, 12, 38, 64), TRX_M4(104, 103, 25, 51, 77),  \
    TRX_M4(51, 0, 1, 2, 3), TRX_M4(51, 4, 5, 6, 7), TRX_M4(51, 8, 9, 10, 11), TRX_M4(51, 12, 13, 14, 15),                  \
    TRX_M4(51, 16, 17, 18, 19), TRX_M4(51, 20, 21, 22, 23), TRX_M4(51, 24, 25, 26, 27), TRX_M4(51, 28, 29, 30, 31),        \
    TRX_M4(102, 32, 33, 34, 35), TRX_M4(102, 36, 37, 38, 39), TRX_M4(102, 40, 41, 42, 43), TRX_M4(102, 44, 45, 46, 47),    \
    TRX_M4(102, 83, 84, 85, 86), TRX_M4(102, 87, 88, 89, 90), TRX_M4(102, 91, 92, 93, 94), TRX_M4(102, 95, 96, 97, 98),    \
    TRX_M4(51, 22, 23, 24, 25), TRX_M4(51, 26, 27, 28, 29), TRX_M4(51, 32, 33, 34, 35), TRX_M4(51, 36, 37, 38, 39),        \
    TRX_M4(102, 42, 43, 44, 45), TRX_M4(102, 46, 47, 48, 49), TRX_M4(102, 93, 94, 95, 96), TRX_M4(102, 97, 98, 99, 100),   \
    TRX_M4(51, 6, 7, 8, 9), TRX_M4(51, 12, 13, 14, 15), TRX_M4(51, 16, 17, 18, 19), TRX_M4(51, 2, 3, 4, 5),                \
    TRX_M5(51, 1, 11, 21, 31, 41), TRX_M5(51, 0, 10, 20, 30, 40)                                                           \
  }

// ---- the transmit multiplexers: what trxsig_l1tx and trxsig_l1ms (trxsig_l1ms_dev.h) have in common ----------------------
// What one encode needs of its call (by value).  Per mapping m: p_first = the first position at or after fn, p_end = the
// first position at or after fn + n_frames, base = p_first minus the mapping's positions in frames [fn - fn % R, fn) -- so
// the frame fn + k, k = q * R + rem - fn % R, is position base + n * q + cnt[m][rem] (cnt: the host's table of frames below
// rem), no division by a variable.  trx_plan_tx_geometry (trxsig_plan.h) fills everything but cur, has_sib, band and bsic.
// The per-class and per-mapping arrays have the downlink's lengths in both directions (the uplink uses 2 classes, 34 mappings).
struct TrxMuxCall {
  int fn, n_frames, n_arfcn, n_tch, n_xcch, n_all;   // n_all: the channels that have records
  int nb[4];                         // per class (TCH, XCCH, CCCH, BCCH): the most blocks any channel opens
  long long unit0[4];                // per class: the first scratch unit ([n_chan][nb] after it)
  int r104, r102, r51, r26;          // fn mod 104 / 102 / 51 / 26
  int cur, has_sib, band, bsic;
  long long p_first[TRX_N_DL_MAPS], p_end[TRX_N_DL_MAPS], base[TRX_N_DL_MAPS];
};

// the head of a channel's record in the object (two copies: the call reads copy `cur`, the commit writes copy `cur ^ 1`)
struct TrxMuxChan {
  uint32_t last_c[16];               // c[456] of the last block the channel encoded, bit i = word i/32 bit i%32
  uint32_t prev_c[16];               // ... and of the one before it (TCH: the odd half interleaves into the next block)
  uint8_t last_f, prev_f;            // their FACCH flags
  uint8_t pend;                      // the last block's last burst lies after the last call: its tail goes out next
  uint8_t active;
};
static_assert(sizeof(TrxMuxChan) == 132, "TrxMuxChan layout");

// the device side of one object (pointers into its allocations); Chan is the direction's record, TrxMuxChan h first
template <class Chan>
struct TrxMuxDev {
  const int32_t *chinfo;             // [n_all]: arfcn | tn << 16 | map << 20
  const int32_t *slot;               // [n_arfcn * 8]: combination | the slot's TCH channel << 4
  const int32_t *slot_x;             // [n_arfcn * 8]: the slot's first XCCH channel (index over all classes)
  const int8_t *writer;              // [3][8][104]: the mapping that owns (combination I / V / VII, TN, fn mod 104 or 102)
  const int16_t *cnt;                // [the direction's mappings][105]
  Chan *st;                          // [2][n_all]
  uint32_t *c;                       // scratch [units][16]
  uint8_t *flag;                     // scratch [units]: 1 encoded, 2 FACCH
  const uint8_t *kind[3], *payload[3];   // TCH / XCCH / CCCH grids
  const uint8_t *filler;             // the context's TCH filler c[456]
  uint8_t *bits, *what;              // [n_arfcn][8 F][148], [n_arfcn][8 F]
};

// ---- the downlink multiplexer (trxsig_l1tx) ---------------------------------------------------------------------------------
struct TrxL1txCall : TrxMuxCall {
  int n_ccch, n_bcch;
  float rssi_target;
};

struct TrxL1txChan {
  TrxMuxChan h;
  int32_t idle_left;                 // dummy bursts still to send (close)
  int32_t ord_pow;                   // SACCH orders (dBm), -1 on channels that are not SACCH
  float ord_ta;
  uint32_t seen;                     // the sibling's accepted-burst count when the orders were last decided
  uint32_t pad[3];
};
// trxsig_l1tx_state hands these bytes to callers
static_assert(sizeof(TrxL1txChan) == 160, "TrxL1txChan layout");
static_assert(offsetof(TrxL1txChan, h.last_c) == 0 && offsetof(TrxL1txChan, h.prev_c) == 64 && offsetof(TrxL1txChan, h.last_f) == 128 &&
              offsetof(TrxL1txChan, h.prev_f) == 129 && offsetof(TrxL1txChan, h.pend) == 130 && offsetof(TrxL1txChan, h.active) == 131 &&
              offsetof(TrxL1txChan, idle_left) == 132 && offsetof(TrxL1txChan, ord_pow) == 136 && offsetof(TrxL1txChan, ord_ta) == 140 &&
              offsetof(TrxL1txChan, seen) == 144 && offsetof(TrxL1txChan, pad) == 148, "TrxL1txChan layout");

struct TrxL1txDev : TrxMuxDev<TrxL1txChan> {
  const uint8_t *si;                 // [4][23] + [92] = 1 once set
  int32_t *ord_pow;                  // [n_xcch] out
  float *ord_ta;                     // [n_xcch] out
  // sibling (trxsig_l1rx) device state, or null
  const int32_t *sib_rssi, *sib_timing, *sib_power, *sib_ta;   // XCCH-indexed
  const uint32_t *sib_count;         // XCCH-indexed accepted-burst counters
};

// what trxsig_l1tx reads of a sibling trxsig_l1rx (trxsig_l1rx.cpp): its plan and its XCCH channels' device state
struct trxsig_l1rx;
struct TrxL1rxSib {
  int n_arfcn, n_tch, n_xcch;
  const uint8_t *comb;               // [n_arfcn * 8] (host)
  const int32_t *rssi, *timing, *power, *ta;   // XCCH-indexed device arrays
  const uint32_t *accepted;          // XCCH-indexed
};
void trx_l1rx_sibling(const trxsig_l1rx *l1, TrxL1rxSib *out);

// what trxsig_trxgroup_add_l1tx reads of a trxsig_l1tx (trxsig_l1tx.cpp): its last encode, as left on the context's stream
struct trxsig_l1tx;
struct TrxL1txLast {
  trxsig_ctx *ctx;
  int n_arfcn, fn, n_frames;         // n_frames = 0: no encode yet (or the workspace that held it is gone)
  const uint8_t *what, *bits;        // [n_arfcn][8 n_frames], [n_arfcn][8 n_frames][148] (device)
};
void trx_l1tx_last(const trxsig_l1tx *l1, TrxL1txLast *out);

// what trxsig_l1ms reads of a sibling trxsig_l1tx (trxsig_l1tx.cpp): its plan and its XCCH channels' current records
struct TrxL1txSib {
  trxsig_ctx *ctx;
  int n_arfcn, n_xcch;
  const uint8_t *comb;               // [n_arfcn * 8] (host)
  const TrxL1txChan *xcch;           // [n_xcch] device: the records the next call of the sibling reads
};
void trx_l1tx_sibling(const trxsig_l1tx *l1, TrxL1txSib *out);

#ifndef TRX_TDMA_TABLES_ONLY
hipError_t trx_launch_l1tx_encode(hipStream_t st, const TrxL1txCall &call, const TrxL1txDev &dv, TrxProfiler *prof);
hipError_t trx_launch_l1tx_mux(hipStream_t st, const TrxL1txCall &call, const TrxL1txDev &dv, TrxProfiler *prof);
// open (1) / close (0) of global channel ch on copy `cur`: open sets active, cancels idle fill and, where sacch, orders 40 / 0;
// close clears active and queues idle_fill dummy bursts
hipError_t trx_launch_l1tx_set(hipStream_t st, TrxL1txChan *rec, int open, int sacch, int idle_fill);
// compaction of the slots d_what != 0 into datagrams, in (FN, TN, ARFCN) order: counts [n_wg], then the datagrams
hipError_t trx_launch_l1tx_dgram(hipStream_t st, const uint8_t *what, const uint8_t *bits, int n_arfcn, int n_frames, int fn,
                                 int32_t *wg_count, int32_t *total, uint8_t *dgram, int32_t *arfcn, int cap, TrxProfiler *prof);
#endif
