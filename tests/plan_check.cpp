// plan_check.cpp -- tests/test_plan.py builds this with trxsig_plan.cpp by the host compiler under AddressSanitizer + UBSan and
// feeds it commands, one a line; every answer is one line (or, for `plan` and `maps`, a block that ends with `end`).
//   maps                               the self-check, then both tables: dir m R f...
//   plan A c0 c1 ...                   the plan comb[8 A]: `refused`, or per direction every class's channels in order
//   strides T A cell slot col          strides_ok, then extent (`-` where refused)
//   overlap p np q nq                  two sample ranges by address
//   geom dir m fn F                    block geometry of one mapping
#define TRX_TDMA_TABLES_ONLY
#include "trxsig_plan.h"

#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>

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
    } else if (!cmd.empty()) {
      return 1;
    }
  }
  return 0;
}
