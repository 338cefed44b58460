// trxsig_l1mux_host.h -- internal, host side: what the two transmit multiplexers (trxsig_l1tx.cpp, trxsig_l1ms.cpp) put on the
// device at create.  The plain-host parts of their common code are trxsig_plan.h's (trx_plan_tx_geometry, trx_plan_same, ...);
// this one allocates, so it lives beside trxsig_ctx.h's helpers.
#pragma once
#include <string>
#include <vector>

#include "trxsig_ctx.h"
#include "trxsig_plan.h"

// One persistent block for an object of plan pl: the record pairs rec[2][N], chinfo, slot, slot_x, the slot-owner table by
// mapping id, the count table, and one more region of more_bytes bytes of the caller's (copied from more_src where that is not
// null; *more_at gets its place).  d gets the pointers and the context's TCH filler.  On failure nothing stays allocated and
// the context's last error is `who`'s.  The caller holds the TrxDeviceGuard.
template <class Chan>
int trx_mux_device_block(trxsig_ctx *c, const char *who, const TrxPlan &pl, const std::vector<Chan> &rec, size_t more_bytes,
                         const void *more_src, TrxMuxDev<Chan> &d, void **block, void **more_at) {
  *block = nullptr;
  std::vector<int8_t> writer;
  if (!trx_plan_owner_table(pl.dir, true, false, writer))
    return trx_ctx_fail(c, TRXSIG_EINVAL, (std::string(who) + ": device allocation").c_str(), hipSuccess);
  const std::vector<int16_t> cnt = trx_plan_count_table(pl.dir);
  const size_t N = rec.size() / 2, S = pl.comb.size();
  const TrxCarve cv = { rec.size() * sizeof(Chan), (N + 1) * 4, S * 4, S * 4, writer.size(), cnt.size() * 2, more_bytes };
  const int rc = trx_device_block(c, who, cv.total,
                                  { { cv.off[0], rec.data(), rec.size() * sizeof(Chan) }, { cv.off[1], pl.chinfo.data(), N * 4 },
                                    { cv.off[2], pl.slot.data(), S * 4 }, { cv.off[3], pl.slot_x.data(), S * 4 },
                                    { cv.off[4], writer.data(), writer.size() }, { cv.off[5], cnt.data(), cnt.size() * 2 },
                                    { cv.off[6], more_src, more_src ? more_bytes : 0 } }, block);
  if (rc != TRXSIG_OK) return rc;
  d.st = cv.at<Chan>(*block, 0); d.chinfo = cv.at<int32_t>(*block, 1); d.slot = cv.at<int32_t>(*block, 2);
  d.slot_x = cv.at<int32_t>(*block, 3); d.writer = cv.at<int8_t>(*block, 4); d.cnt = cv.at<int16_t>(*block, 5);
  *more_at = cv.at<void>(*block, 6);
  d.filler = trx_ctx_tch_filler(c);
  if (d.filler) return TRXSIG_OK;
  (void)hipFree(*block);
  *block = nullptr;
  return trx_ctx_fail(c, TRXSIG_EHIP, (std::string(who) + ": upload").c_str(), hipSuccess);
}
