// plan_check.cpp -- tests/test_plan.py builds this with trxsig_plan.cpp by the host compiler under AddressSanitizer + UBSan and
// feeds it commands, one a line; every answer is one line (or, for `plan` and `maps`, a block that ends with `end`).
//   maps                               the self-check, then both tables: dir m R f...
//   plan A c0 c1 ...                   the plan comb[8 A]: `refused`, or per direction every class's channels in order
//   strides T A cell slot col          strides_ok, then extent (`-` where refused)
//   overlap p np q nq                  two sample ranges by address
//   geom dir m fn F                    block geometry of one mapping
//   txgeom dir fn F A c0 c1 ...        trx_plan_tx_geometry of the plan as the direction's multiplexer calls it, against a
//                                      brute-force count by trx_map_count / trx_map_frame: `ok`, or `bad` and what differs
//   power                              trx_encode_power against the rule written out, every band, power -5..45: `ok` or `bad ...`
#define TRX_TDMA_TABLES_ONLY
#include "trxsig_plan.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <sstream>
#include <string>

namespace {
const int8_t kPower[3][32] = TRX_POWER_TABLES_INIT;

// the transmit geometry of plan pl over frames [fn, fn + F), counted frame by frame; empty, or what differs
std::string tx_geometry_diff(const TrxPlan &pl, int n_cls, int fn, int F) {
  TrxMuxCall k;
  trx_plan_tx_geometry(pl, n_cls, fn, F, &k);
  auto bad = [](const char *what, int m) { return std::string(what) + " " + std::to_string(m); };
  if (k.fn != fn || k.n_frames != F || k.n_arfcn != pl.A || k.n_tch != pl.n[0] || k.n_xcch != pl.n[1] || k.n_all != pl.first[n_cls] ||
      k.r104 != fn % 104 || k.r102 != fn % 102 || k.r51 != fn % 51 || k.r26 != fn % 26)
    return "counts";
  const std::vector<int16_t> cnt = trx_plan_count_table(pl.dir);
  int started[TRX_N_DL_MAPS] = {};                              // per mapping: positions q = 0 mod 4 of the call's frames
  for (int m = 0; m < trx_plan_n_maps(pl.dir); m++) {
    const TrxTdmaMap &M = trx_plan_maps(pl.dir)[m];
    if (k.p_first[m] != trx_map_count(M, fn)) return bad("p_first", m);
    if (k.p_end[m] != trx_map_count(M, (long long)fn + F)) return bad("p_end", m);
    if (k.base[m] != trx_map_count(M, fn - fn % M.R)) return bad("base", m);
    for (int j = 0; j < F; j++) {
      const long long u = (long long)fn + j, q = trx_map_count(M, u);
      const int t = fn % M.R + j, Q = t / M.R, rem = t % M.R;
      if (k.base[m] + (long long)M.n * Q + cnt[(size_t)m * 105 + rem] != q) return bad("position", m);
      if (trx_map_frame(M, q) != u) continue;                   // the mapping has no burst in this frame
      if (q < k.p_first[m] || q >= k.p_end[m]) return bad("range", m);
      started[m] += ((q % 4) + 4) % 4 == 0;
    }
  }
  long long unit = 0;
  for (int cl = 0; cl < 4; cl++) {
    int nb = 0;
    for (int i = 0; cl < n_cls && i < pl.n[cl]; i++) nb = std::max(nb, started[pl.map(pl.index(cl, i))]);
    if (k.nb[cl] != nb) return bad("nb", cl);
    if (k.unit0[cl] != (cl < n_cls ? unit : 0)) return bad("unit0", cl);
    unit += (long long)pl.n[cl] * nb;
  }
  return std::string();
}

// encodePower as GSML1FEC.cpp states it: the code whose table value is nearest, the first of equals, an exact match at once
int encode_power_rule(const int8_t *row, int power) {
  int best = 0;
  for (int i = 1; i < 32; i++) {
    if (row[i] == power) return i;
    if (std::abs(power - row[i]) < std::abs(power - row[best])) best = i;
  }
  return best;
}
}  // namespace

int main() {
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    std::string cmd;
    in >> cmd;
    if (cmd == "maps") {
      std::printf("selfcheck %d\n", trx_plan_selfcheck() ? 1 : 0);
      for (int dir = 0; dir < 2; dir++)
        for (int m = 0; m < trx_plan_n_maps(dir); m++) {
          const TrxTdmaMap &M = trx_plan_maps(dir)[m];
          std::printf("%s %d %d", dir == TRX_PLAN_UL ? "UL" : "DL", m, M.R);
          for (int r = 0; r < M.n; r++) std::printf(" %d", M.f[r]);
          std::printf("\n");
        }
      std::printf("end\n");
    } else if (cmd == "plan") {
      int A = 0;
      in >> A;
      std::vector<uint8_t> comb;
      for (int v; in >> v;) comb.push_back((uint8_t)v);
      if (A >= 1 && A <= 0xffff && comb.size() != 8 * (size_t)A) return 4;   // not a plan at all: the test's own mistake
      if (!trx_plan_validate(comb.data(), A)) {
        std::printf("refused\nend\n");
        continue;
      }
      for (int dir = 1; dir >= 0; dir--) {
        const TrxPlan pl(A, comb.data(), dir, dir == TRX_PLAN_UL ? 3 : TRX_PLAN_CLASSES);
        for (int cls = 0; cls < pl.n_cls; cls++)
          for (int i = 0; i < pl.n[cls]; i++) {
            int a = -1, tn = -1, kind = -1, sub = -1;
            const int g = pl.index(cls, i);
            if (pl.describe(g, &a, &tn, &kind, &sub) != TRXSIG_OK) return 2;
            std::printf("%s %d %d %d %d %d %d %d\n", dir == TRX_PLAN_UL ? "UL" : "DL", cls, i, a, tn, pl.map(g), kind, sub);
          }
        if (pl.index(pl.n_cls, 0) != -1 || pl.index(0, pl.n[0]) != -1 || pl.index(-1, 0) != -1 || pl.describe(-1, 0, 0, 0, 0) != TRXSIG_EINVAL)
          return 3;
      }
      std::printf("end\n");
    } else if (cmd == "strides") {
      long long T, A, cell, s, c, n = 0;
      in >> T >> A >> cell >> s >> c;
      const bool ok = strides_ok(T, A, cell, s, c), ex = extent(T, A, cell, s, c, &n);
      if (ex) std::printf("%d %lld\n", ok ? 1 : 0, n);
      else std::printf("%d -\n", ok ? 1 : 0);
    } else if (cmd == "overlap") {
      unsigned long long p, q;
      long long np, nq;
      in >> p >> np >> q >> nq;
      std::printf("%d\n", overlap((const trxsig_c32 *)(uintptr_t)p, np, (const trxsig_c32 *)(uintptr_t)q, nq) ? 1 : 0);
    } else if (cmd == "geom") {
      int dir, m, fn, F;
      in >> dir >> m >> fn >> F;
      const TrxBlockGeom g = trx_plan_block_geometry(trx_plan_maps(dir)[m], fn, F);
      std::printf("%lld %lld %lld %d %d\n", g.p_first, g.p_end, g.base, g.nb_touched, g.nb_started);
    } else if (cmd == "txgeom") {
      int dir, fn, F, A = 0;
      in >> dir >> fn >> F >> A;
      std::vector<uint8_t> comb;
      for (int v; in >> v;) comb.push_back((uint8_t)v);
      if (comb.size() != 8 * (size_t)A || !trx_plan_validate(comb.data(), A)) return 5;
      // trxsig_l1ms: an uplink plan of three classes, records for two; trxsig_l1tx: a downlink plan of four, all with records
      const TrxPlan pl(A, comb.data(), dir, dir == TRX_PLAN_UL ? 3 : 4);
      const std::string diff = tx_geometry_diff(pl, dir == TRX_PLAN_UL ? 2 : 4, fn, F);
      std::printf("%s\n", diff.empty() ? "ok" : ("bad " + diff).c_str());
    } else if (cmd == "power") {
      std::string diff;
      for (int band = 0; band < 3 && diff.empty(); band++)
        for (int p = -5; p <= 45 && diff.empty(); p++)
          if (trx_encode_power(kPower[band], p) != encode_power_rule(kPower[band], p))
            diff = "bad band " + std::to_string(band) + " power " + std::to_string(p);
      std::printf("%s\n", diff.empty() ? "ok" : diff.c_str());
    } else if (!cmd.empty()) {
      return 1;
    }
  }
  return 0;
}
