"""Time one trxsig_l1tx_encode of the production plan (128 ARFCNs; C0: combination V on TN 0, VII on TN 1, I elsewhere; I on
every other carrier) over 104 frames: the median of repeated HIP-event windows around the whole call, Mbursts/s of output slots,
the per-kernel averages from the library's own event profiler, and the same inputs through the composition a caller writes
today -- trxsig_fec_tch_encode_batch, trxsig_fec_xcch_encode_batch (per TSC: one call, every block uses the BCC),
trxsig_fec_sch_encode_batch, then torch index_copy_ of every burst into the [n_arfcn][8 F][148] frame layout with slot indices
built beforehand on the host.  The kernel trace is a separate run: rocprofv3 --kernel-trace --stats.

    python tools/l1tx_bench.py [--arfcns 128] [--frames 104] [--reps 50]"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")]


def main():
    import torch
    import _pkg
    import l1_mux_model as lmm
    ap = argparse.ArgumentParser()
    ap.add_argument("--arfcns", type=int, default=128)
    ap.add_argument("--frames", type=int, default=104)
    ap.add_argument("--reps", type=int, default=50)
    a = ap.parse_args()
    m = _pkg.load()
    ctx = m.TrxSig(4, 0)
    ctx.use_torch_stream()
    rng = np.random.default_rng(1)
    A, F, bsic = a.arfcns, a.frames, 33
    comb = np.ones((A, 8), np.uint8)
    comb[0, 0], comb[0, 1] = 5, 7
    l1 = m.L1Tx(ctx, comb, bsic)
    l1.set_si(rng.integers(0, 256, (4, 23)).astype(np.uint8))
    fn = 1326 * 3                                            # a 51- and 26-multiframe boundary: every block of the call is whole
    nbt, nbx, nbc = l1.grid(fn, F)
    nt, nx, nc = l1.channels(m.L1_TCH), l1.channels(m.L1_XCCH), l1.channels(m.L1_CCCH)
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    tk = dev(rng.choice(np.array([0, 1, 1, 2], np.uint8), (nt, nbt)))
    tp = dev(rng.integers(0, 256, (nt, nbt, 33)).astype(np.uint8))
    xk = dev(np.ones((nx, nbx), np.uint8)); xp = dev(rng.integers(0, 256, (nx, nbx, 23)).astype(np.uint8))
    ck = dev(np.ones((nc, nbc), np.uint8)); cp = dev(rng.integers(0, 256, (nc, nbc, 23)).astype(np.uint8))

    def fused():
        l1.encode(fn, F, tk, tp, xk, xp, ck, cp)

    def window(fnc):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        ts = []
        for _ in range(a.reps):
            ev[0].record(); fnc(); ev[1].record(); torch.cuda.synchronize()
            ts.append(ev[0].elapsed_time(ev[1]) * 1000.0)
        return float(np.median(ts))

    for _ in range(5):
        fused()
    torch.cuda.synchronize()
    whole = window(fused)
    r = l1.collect(state=False)
    n_sent = int((r["what"] != 0).sum())
    ctx.L.trxsig_profile_enable(ctx.h, 1)
    for _ in range(a.reps):
        fused()
    n = ctx.L.trxsig_kernel_count()
    ms = (C.c_float * n)(); cnt = (C.c_int * n)()
    ctx.L.trxsig_profile_collect_n(ctx.h, n, ms, cnt)
    ctx.L.trxsig_profile_enable(ctx.h, 0)
    split = {ctx.L.trxsig_kernel_name(i).decode(): round(ms[i] * 1000.0 / cnt[i], 2) for i in range(n) if cnt[i]}
    t0 = torch.cuda.Event(enable_timing=True); t1 = torch.cuda.Event(enable_timing=True)
    t0.record(); dg, _ = l1.datagrams(); t1.record(); torch.cuda.synchronize()
    dgram_us = t0.elapsed_time(t1) * 1000.0

    # ---- the composition: the three batch encoders, then a scatter into the frame layout (indices built on the host) ----
    model = lmm.MuxModel(comb, bsic, oracle=object())
    slots_t, slots_x, slots_s, fns = [], [], [], []
    for cls, dst, nb in ((lmm.TCH, slots_t, nbt), (lmm.XCCH, slots_x, nbx), (lmm.CCCH, slots_x, nbc), (lmm.BCCH, slots_x, 1)):
        for c in model.ch[cls]:
            w = [(k, B) for k, B in model.walk(c.m, fn, F)]
            blocks = [w[i:i + 4] for i in range(0, len(w), 4)][:nb]
            for blk in blocks:
                blk = (blk + [blk[-1]] * 4)[:4]                  # (a call on a block boundary: every block is whole)
                dst += [c.a * 8 * F + 8 * k + c.tn for k, _ in blk]
    for aa, tn, mp, code in model.gen:
        for k, _ in model.walk(mp, fn, F):
            if code == lmm.W_SCH:
                slots_s.append(aa * 8 * F + 8 * k + tn); fns.append(fn + k)
    n_xblk = len(slots_x) // 4
    idx_t, idx_x, idx_s = (torch.tensor(s, dtype=torch.long, device="cuda") for s in (slots_t, slots_x, slots_s))
    frames_x = dev(rng.integers(0, 256, (n_xblk, 23)).astype(np.uint8))
    tsc_t = dev(np.full(nt, bsic & 7, np.uint8)); st_t = torch.zeros(nt, 32, dtype=torch.uint8, device="cuda")
    bits_t = torch.empty(nt, nbt, 4, 148, dtype=torch.uint8, device="cuda")
    bits_x = torch.empty(n_xblk * 4, 148, dtype=torch.uint8, device="cuda")
    fn_s = dev(np.array(fns, np.uint32)); bs_s = dev(np.full(len(fns), bsic, np.uint8))
    bits_s = torch.empty(len(fns), 148, dtype=torch.uint8, device="cuda")
    out = torch.zeros(A * 8 * F, 148, dtype=torch.uint8, device="cuda")

    def composed():
        ctx.fec_tch_encode(tk, tp, tsc_t, st_t, bits_t)
        ctx.fec_xcch_encode(frames_x, n_xblk, bsic & 7, bits_x)
        ctx.fec_sch_encode(fn_s, bs_s, bits_s)
        out.zero_()
        out.index_copy_(0, idx_t, bits_t.view(-1, 148)[:len(slots_t)])
        out.index_copy_(0, idx_x, bits_x)
        out.index_copy_(0, idx_s, bits_s)
    for _ in range(3):
        composed()
    comp = window(composed)
    print(json.dumps(dict(arfcns=A, frames=F, n_tch=nt, n_xcch=nx, n_ccch=nc, nb_tch=nbt, nb_xcch=nbx, nb_ccch=nbc,
                          slots=A * 8 * F, slots_sent=n_sent, encode_us=round(whole, 1),
                          mbursts_per_s=round(A * 8 * F / whole, 1), per_kernel_us=split, datagrams=len(dg),
                          datagrams_call_us=round(dgram_us, 1), composed_us=round(comp, 1),
                          composed_note="batch encoders + index_copy_ scatter, same blocks, no pending-burst or idle handling")))


if __name__ == "__main__":
    main()
