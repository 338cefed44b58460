// trxsig_plan.cpp -- the channel plan (trxsig_plan.h): the host's copy of the two mapping tables, the placement rule, the
// enumeration of a plan's channels, and the tables the stages derive from the mappings.  Plain host C++.
#define TRX_TDMA_TABLES_ONLY
#include "trxsig_plan.h"

#include <cstring>
#include <utility>

namespace {
const TrxTdmaMap kUl[TRX_N_MAPS] = TRX_TDMA_MAPS_INIT;
const TrxTdmaMap kDl[TRX_N_DL_MAPS] = TRX_TDMA_DL_MAPS_INIT;

inline long long ceil4(long long p) { return -trx_fdiv(-p, 4); }

// the (mapping, code) pairs that share a slot of combination I / V / VII (ci 0 / 1 / 2) on timeslot tn
std::vector<std::pair<int, int>> slot_maps(int dir, int ci, int tn, bool common) {
  std::vector<std::pair<int, int>> ms;
  if (ci == 0) return { { TRX_MAP_TCHF, 0 }, { TRX_MAP_SACCH_TF + tn, 1 } };
  const int ns = ci == 1 ? 4 : 8, sd = ci == 1 ? TRX_MAP_SDCCH4 : TRX_MAP_SDCCH8, sa = ci == 1 ? TRX_MAP_SACCH_C4 : TRX_MAP_SACCH_C8;
  for (int s = 0; s < ns; s++) { ms.push_back({ sd + s, 1 + s }); ms.push_back({ sa + s, 1 + ns + s }); }
  if (ci == 1 && common)
    for (int m = TRX_MAP_RACH_C5; m < trx_plan_n_maps(dir); m++) ms.push_back({ m, -1 });   // ids 33..: the RACH, or the beacon's
  return ms;
}
}  // namespace

const TrxTdmaMap *trx_plan_maps(int dir) { return dir == TRX_PLAN_UL ? kUl : kDl; }

bool trx_plan_selfcheck() {
  static const bool ok = [] {
    std::vector<int8_t> t;
    for (int dir = 0; dir < 2; dir++) {
      for (int i = 0; i < trx_plan_n_maps(dir); i++) {
        const TrxTdmaMap &m = trx_plan_maps(dir)[i];
        for (int r = 1; r < m.n; r++)
          if ((m.f[r] - m.f[0] + m.R) % m.R <= (m.f[r - 1] - m.f[0] + m.R) % m.R) return false;
      }
      if (!trx_plan_owner_table(dir, true, false, t)) return false;
    }
    return true;
  }();
  return ok;
}

bool trx_plan_slot_ok(int k, int a, int tn) {
  return k == 0 || k == 1 || k == 7 || (k == 5 && a == 0 && tn == 0);   // C-V: C0Only, allowedSlots 0x01
}

bool trx_plan_validate(const uint8_t *h_comb, int n_arfcn) {
  if (!h_comb || n_arfcn <= 0 || n_arfcn > 0xffff) return false;
  for (int a = 0; a < n_arfcn; a++)
    for (int tn = 0; tn < 8; tn++)
      if (!trx_plan_slot_ok(h_comb[8 * a + tn], a, tn)) return false;
  return true;
}

int trx_plan_band_index(int band) { return (band == 850 || band == 900) ? 0 : band == 1800 ? 1 : band == 1900 ? 2 : -1; }

void trx_plan_map_kind(int m, int dir, int *kind, int *sub) {
  static const int first[] = { TRX_MAP_TCHF, TRX_MAP_SACCH_TF, TRX_MAP_SDCCH8, TRX_MAP_SACCH_C8, TRX_MAP_SDCCH4, TRX_MAP_SACCH_C4,
                               TRX_MAP_RACH_C5 };
  *sub = 0;
  if (dir == TRX_PLAN_DL && m >= TRX_DL_CCCH) {
    if (m < TRX_DL_BCCH) { *kind = TRXSIG_L1_CCCH_C5; *sub = m - TRX_DL_CCCH; }
    else *kind = m == TRX_DL_BCCH ? TRXSIG_L1_BCCH_C5 : m == TRX_DL_SCH ? TRXSIG_L1_SCH_C5 : TRXSIG_L1_FCCH_C5;
    return;
  }
  int k = 6;
  while (m < first[k]) k--;
  *kind = k;
  if (k != TRXSIG_L1_SACCH_TF) *sub = m - first[k];
}

std::string trx_plan_create_error(const char *who, int n_arfcn, const uint8_t *h_comb, int bsic, int band, bool more_ok, int *band_index) {
  *band_index = trx_plan_band_index(band);
  if (n_arfcn <= 0 || n_arfcn > 0xffff || !h_comb || bsic < 0 || bsic > 63 || *band_index < 0 || !more_ok || !trx_plan_selfcheck())
    return std::string(who) + ": bad argument";
  if (!trx_plan_validate(h_comb, n_arfcn)) return std::string(who) + ": unsupported channel combination or placement";
  return std::string();
}

bool trx_plan_result_ok(const trxsig_trxgroup_result *res, int n_arfcn) {
  return res && res->n_arfcn == n_arfcn && res->n_slots > 0 && !(res->n_slots & 7) && res->n_rows >= 0 && res->d_row &&
         (res->n_rows == 0 || (res->d_valid && res->d_soft && res->d_amp && res->d_toa && res->soft_stride >= 148));
}

bool trx_plan_same(const TrxPlan &pl, int n_arfcn, int n_xcch, const uint8_t *comb) {
  return n_arfcn == pl.A && n_xcch == pl.n[TRX_PLAN_XCCH] && std::memcmp(comb, pl.comb.data(), pl.comb.size()) == 0;
}

void trx_plan_sacch_start(const TrxPlan &pl, std::vector<int32_t> &power, std::vector<int32_t> &ta) {
  const size_t X = (size_t)pl.n[TRX_PLAN_XCCH];
  power.assign(X, -1);
  ta.assign(X, -1);
  for (size_t i = 0; i < X; i++)
    if (pl.sacch(pl.first[TRX_PLAN_XCCH] + (int)i)) { power[i] = 40; ta[i] = 0; }
}

TrxPlan::TrxPlan(int n_arfcn, const uint8_t *h_comb, int dir_, int n_cls_) : A(n_arfcn), dir(dir_), n_cls(n_cls_) {
  comb.assign(h_comb, h_comb + 8 * (size_t)A);
  slot.assign(comb.size(), 0);
  slot_x.assign(comb.size(), 0);
  std::vector<int32_t> cl[TRX_PLAN_CLASSES], hs[2];
  auto add = [&](int cls, int a, int tn, int m) { if (cls < n_cls) cl[cls].push_back((int32_t)(a | tn << 16 | m << 20)); };
  for (int a = 0; a < A; a++)
    for (int tn = 0; tn < 8; tn++) {
      const int k = comb[8 * (size_t)a + tn];
      const int32_t x0 = (int32_t)cl[TRX_PLAN_XCCH].size();
      slot_x[8 * (size_t)a + tn] = x0;
      slot[8 * (size_t)a + tn] = k | (int32_t)cl[TRX_PLAN_TCH].size() << 4;
      const int ns = k == 5 ? 4 : 8;
      switch (k) {
        case 1:
          add(TRX_PLAN_TCH, a, tn, TRX_MAP_TCHF); hs[0].push_back(x0);
          add(TRX_PLAN_XCCH, a, tn, TRX_MAP_SACCH_TF + tn); hs[1].push_back(x0);
          break;
        case 5:
        case 7:
          for (int s = 0; s < ns; s++) { add(TRX_PLAN_XCCH, a, tn, (k == 5 ? TRX_MAP_SDCCH4 : TRX_MAP_SDCCH8) + s); hs[1].push_back(x0 + ns + s); }
          for (int s = 0; s < ns; s++) { add(TRX_PLAN_XCCH, a, tn, (k == 5 ? TRX_MAP_SACCH_C4 : TRX_MAP_SACCH_C8) + s); hs[1].push_back(x0 + ns + s); }
          if (k == 7) break;
          if (dir == TRX_PLAN_UL) { add(TRX_PLAN_RACH, a, tn, TRX_MAP_RACH_C5); break; }
          for (int s = 0; s < 3; s++) add(TRX_PLAN_CCCH, a, tn, TRX_DL_CCCH + s);
          add(TRX_PLAN_BCCH, a, tn, TRX_DL_BCCH);
          add(TRX_PLAN_SCH, a, tn, TRX_DL_SCH);
          add(TRX_PLAN_FCCH, a, tn, TRX_DL_FCCH);
          break;
        default: break;
      }
    }
  for (int k = 0; k < n_cls; k++) {
    n[k] = (int)cl[k].size();
    first[k + 1] = first[k] + n[k];
    chinfo.insert(chinfo.end(), cl[k].begin(), cl[k].end());
    for (int32_t v : cl[k]) map_used[k][v >> 20] = true;
  }
  for (int32_t &x : slot_x) x += n[TRX_PLAN_TCH];
  handset = hs[0];
  handset.insert(handset.end(), hs[1].begin(), hs[1].end());
}

int TrxPlan::describe(int i, int *arfcn, int *tn, int *kind, int *sub) const {
  if (i < 0) return TRXSIG_EINVAL;
  const int32_t v = chinfo[(size_t)i];
  int k = 0, s = 0;
  trx_plan_map_kind(v >> 20, dir, &k, &s);
  if (arfcn) *arfcn = v & 0xffff;
  if (tn) *tn = (v >> 16) & 15;
  if (kind) *kind = k;
  if (sub) *sub = s;
  return TRXSIG_OK;
}

bool trx_plan_owner_table(int dir, bool common, bool code, std::vector<int8_t> &out) {
  const size_t at = out.size();
  out.resize(at + 3 * 8 * 104, -1);
  bool disjoint = true;
  for (int ci = 0; ci < 3; ci++)
    for (int tn = 0; tn < 8; tn++)
      for (const auto &mc : slot_maps(dir, ci, tn, common)) {
        const TrxTdmaMap &M = trx_plan_maps(dir)[mc.first];
        for (int r = 0; r < (ci == 0 ? 104 : 102); r++)
          for (int i = 0; i < M.n; i++)
            if (r % M.R == M.f[i]) {
              int8_t &w = out[at + (size_t)(ci * 8 + tn) * 104 + r];
              if (w >= 0) disjoint = false;
              w = (int8_t)(code ? mc.second : mc.first);
            }
      }
  return disjoint;
}

std::vector<int16_t> trx_plan_count_table(int dir) {
  const int N = trx_plan_n_maps(dir);
  std::vector<int16_t> cnt((size_t)N * 105, 0);
  for (int m = 0; m < N; m++) {
    const TrxTdmaMap &M = trx_plan_maps(dir)[m];
    for (int x = 0; x <= M.R; x++) {
      int v = 0;
      for (int i = 0; i < M.n; i++) v += M.f[i] < x;
      cnt[(size_t)m * 105 + x] = (int16_t)v;
    }
  }
  return cnt;
}

TrxBlockGeom trx_plan_block_geometry(const TrxTdmaMap &M, int fn, int F) {
  TrxBlockGeom g{};
  g.p_first = trx_map_count(M, fn);
  g.p_end = trx_map_count(M, (long long)fn + F);
  int below = 0;
  for (int r = 0; r < M.n; r++) below += M.f[r] < fn % M.R;
  g.base = g.p_first - below;
  g.nb_touched = g.p_end > g.p_first ? (int)(trx_fdiv(g.p_end - 1, 4) - trx_fdiv(g.p_first, 4) + 1) : 0;
  g.nb_started = (int)(ceil4(g.p_end) - ceil4(g.p_first));
  return g;
}

void trx_plan_tx_geometry(const TrxPlan &pl, int n_cls, int fn, int F, TrxMuxCall *k) {
  *k = TrxMuxCall{};
  k->fn = fn; k->n_frames = F; k->n_arfcn = pl.A;
  k->n_tch = pl.n[TRX_PLAN_TCH]; k->n_xcch = pl.n[TRX_PLAN_XCCH]; k->n_all = pl.first[n_cls];
  k->r104 = fn % 104; k->r102 = fn % 102; k->r51 = fn % 51; k->r26 = fn % 26;
  for (int m = 0; m < trx_plan_n_maps(pl.dir); m++) {
    const TrxBlockGeom bg = trx_plan_block_geometry(trx_plan_maps(pl.dir)[m], fn, F);
    k->p_first[m] = bg.p_first; k->p_end[m] = bg.p_end; k->base[m] = bg.base;
    for (int cl = 0; cl < n_cls; cl++)
      if (pl.map_used[cl][m] && bg.nb_started > k->nb[cl]) k->nb[cl] = bg.nb_started;
  }
  long long u = 0;
  for (int cl = 0; cl < n_cls; cl++) { k->unit0[cl] = u; u += (long long)pl.n[cl] * k->nb[cl]; }
}
