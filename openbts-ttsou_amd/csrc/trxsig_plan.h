// trxsig_plan.h -- internal, host only (plain C++17, no HIP): the channel plan every L1 stage shares.  A CMD SETSLOT plan
// h_comb[8 * n_arfcn] becomes numbered channels here and nowhere else, so a channel index means the same channel to
// trxsig_l1rx, trxsig_l1tx, trxsig_l1ms, trxsig_l1msrx and trxsig_l1ciph (and trxsig_l1hop accepts the same plans).
//
// Order.  Slots are walked ARFCN by ARFCN, TN 0..7.  Combination I gives a TCH channel (FACCH_TCHF) and an XCCH channel
// (SACCH_TF_T<tn>); V gives XCCH SDCCH/4 0..3 then SACCH/C4 0..3 and the common channels (uplink: the RACH; downlink: CCCH 0..2,
// BCCH, SCH, FCCH); VII gives XCCH SDCCH/8 0..7 then SACCH/C8 0..7.  Channels are numbered per class in that order, and over all
// classes with the classes one after the other: TCH, XCCH, then RACH (uplink) or CCCH, BCCH, SCH, FCCH (downlink).  Mapping
// ids below 33 name the same logical channel in both directions' tables (trxsig_tdma.h), so the dedicated classes of an uplink
// and a downlink plan are equal word for word.
#pragma once
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "trxsig_l1msrx.h"
#include "trxsig_tdma.h"

#pragma GCC visibility push(hidden)   // nothing here is part of the C-ABI

enum { TRX_PLAN_DL = 0, TRX_PLAN_UL = 1 };                     // direction: the mapping table (trxsig_l1ciph's `uplink`)
enum { TRX_PLAN_TCH = 0, TRX_PLAN_XCCH = 1, TRX_PLAN_RACH = 2, /* uplink */ TRX_PLAN_CCCH = 2, TRX_PLAN_BCCH = 3, TRX_PLAN_SCH = 4,
       TRX_PLAN_FCCH = 5, TRX_PLAN_CLASSES = 6 };              // class slots, in channel order

const TrxTdmaMap *trx_plan_maps(int dir);                      // the host's one copy of the direction's table
inline int trx_plan_n_maps(int dir) { return dir == TRX_PLAN_UL ? (int)TRX_N_MAPS : (int)TRX_N_DL_MAPS; }
// properties of the constants: in every mapping of both tables f[r] - f[0] (mod R) grows with r (positions grow with time,
// trxsig_tdma.h), and no two mappings that share a slot claim one frame (every owner table below is disjoint)
bool trx_plan_selfcheck();
// the placement rule of one slot / of a plan (n_arfcn in 1..65535, h_comb not null)
bool trx_plan_slot_ok(int comb, int a, int tn);
bool trx_plan_validate(const uint8_t *h_comb, int n_arfcn);
int trx_plan_band_index(int band);                             // 850 / 900 -> 0, 1800 -> 1, 1900 -> 2, else -1
// the create arguments of a plan-based object (trxsig_l1rx, _l1tx, _l1ms, _l1msrx): empty and the band's index, or the refusal
// as `who` reports it.  more_ok: the caller's own conditions, refused as a bad argument
std::string trx_plan_create_error(const char *who, int n_arfcn, const uint8_t *h_comb, int bsic, int band, bool more_ok, int *band_index);
// whether res holds whole frames from TN 0 of n_arfcn ARFCNs, with every array its rows need (the two receivers' decode)
bool trx_plan_result_ok(const trxsig_trxgroup_result *res, int n_arfcn);
// TRXSIG_L1_* kind and sub-channel of mapping id m of a direction's table
void trx_plan_map_kind(int m, int dir, int *kind, int *sub);
inline bool trx_plan_map_sacch(int m) { return trx_map_is_sacch(m); }

struct TrxPlan {
  int A = 0, dir = 0, n_cls = 0;
  int n[TRX_PLAN_CLASSES] = {};                 // channels per class slot
  int first[TRX_PLAN_CLASSES + 1] = {};         // a class's first channel over all classes; first[n_cls] = all of them
  std::vector<uint8_t> comb;                    // [8 A]
  std::vector<int32_t> chinfo;                  // per channel over all classes: arfcn | tn << 16 | map << 20
  std::vector<int32_t> slot, slot_x;            // [8 A]: combination | the slot's TCH channel << 4; its first XCCH channel over all classes
  std::vector<int32_t> handset;                 // [n TCH + n XCCH]: the XCCH channel (in its class) whose SACCH is the sender's
  bool map_used[TRX_PLAN_CLASSES][TRX_N_DL_MAPS] = {};
  TrxPlan() = default;
  // a validated plan; n_cls class slots are wanted (2: the dedicated channels only)
  TrxPlan(int n_arfcn, const uint8_t *h_comb, int dir, int n_cls);
  int all() const { return first[n_cls]; }
  int index(int cls_slot, int chan) const {     // over all classes, or -1
    return cls_slot >= 0 && cls_slot < n_cls && chan >= 0 && chan < n[cls_slot] ? first[cls_slot] + chan : -1;
  }
  int map(int index) const { return chinfo[(size_t)index] >> 20; }
  bool sacch(int index) const { return trx_plan_map_sacch(map(index)); }
  // TRXSIG_OK and the channel's (arfcn, tn, kind, sub) where wanted; TRXSIG_EINVAL for index < 0
  int describe(int index, int *arfcn, int *tn, int *kind, int *sub) const;
};

// whether a sibling's plan -- its ARFCNs, XCCH channels and combinations comb[8 n_arfcn] -- is pl's
bool trx_plan_same(const TrxPlan &pl, int n_arfcn, int n_xcch, const uint8_t *comb);
// the SACCH power / TA the receivers start from, per XCCH channel: 40 dBm / 0 on SACCH channels, -1 on the others
void trx_plan_sacch_start(const TrxPlan &pl, std::vector<int32_t> &power, std::vector<int32_t> &ta);

// the slot owners of a direction, appended to out: [combination I / V / VII][TN][fn mod 104 (I) or 102 (V, VII)] -> -1 or the
// owning mapping's value.  common: combination V's common channels take part.  code: the value is 0 for the TCH and 1 + the XCCH
// channel's place among the slot's, else the mapping id.  Returns whether no frame had two owners.
bool trx_plan_owner_table(int dir, bool common, bool code, std::vector<int8_t> &out);
// cnt[m * 105 + x] = mapping m's frames below x, x in 0..R
std::vector<int16_t> trx_plan_count_table(int dir);

// the positions of frames [fn, fn + F) of a mapping: p_first / p_end the first position at or after fn / fn + F, base = p_first
// minus the positions in [fn - fn % R, fn).  Blocks are four positions.  The receivers count the blocks the call touches
// (nb_touched: a block it ends in is decoded in it); the transmitters the blocks that start in it (nb_started: a block is
// encoded when its first burst goes out).  Two numbers on purpose.
struct TrxBlockGeom { long long p_first, p_end, base; int nb_touched, nb_started; };
TrxBlockGeom trx_plan_block_geometry(const TrxTdmaMap &M, int fn, int F);
// a transmit multiplexer's call over frames [fn, fn + F): k zeroed, then the plan's counts (the first n_cls classes have records:
// n_all), fn's remainders, p_first / p_end / base of every mapping of the plan's direction, nb[] = the most blocks a class's
// channels start in the call and unit0[] = the classes' scratch units one after the other
void trx_plan_tx_geometry(const TrxPlan &pl, int n_cls, int fn, int F, TrxMuxCall *k);

// Cell layouts.  trxsig_air_cells, trxsig_l1ms_radiate, trxsig_l1trk_slice and trxsig_l1hop_cells address T slots of A columns,
// cells of `cell` samples, by two strides.  Cells must not overlap in either nesting: the smaller stride holds a cell and the
// larger holds the other dimension's whole row (by division: no product can overflow).
inline bool strides_ok(long long T, long long A, long long cell, long long slot_stride, long long col_stride) {
  const bool slot_major = col_stride >= cell && (T == 1 || (slot_stride >= cell && slot_stride / A >= col_stride));
  const bool col_major = slot_stride >= cell && (A == 1 || (col_stride >= cell && col_stride / T >= slot_stride));
  return slot_major || col_major;
}
// one past the last sample of the last cell, from the base; false where that overflows or passes 2^58
inline bool extent(long long T, long long A, long long cell, long long slot_stride, long long col_stride, long long *out) {
  long long x = 0, y = 0;
  if (__builtin_mul_overflow(T - 1, slot_stride, &x) || __builtin_mul_overflow(A - 1, col_stride, &y) ||
      __builtin_add_overflow(x, y, &x) || __builtin_add_overflow(x, cell, &x) || x > (1LL << 58))
    return false;
  *out = x;
  return true;
}
// whether np samples at p and nq samples at q share a sample
inline bool overlap(const trxsig_c32 *p, long long np, const trxsig_c32 *q, long long nq) {
  const uintptr_t a = (uintptr_t)p, b = (uintptr_t)q;
  return a < b + (uintptr_t)nq * sizeof(trxsig_c32) && b < a + (uintptr_t)np * sizeof(trxsig_c32);
}

#pragma GCC visibility pop
