"""Time one trxsig_l1rx_decode of 128 ARFCNs x 104 frames (C0T0 = combination V, the other slots a mix of I and VII) from a
pull built from tensors: the median of repeated HIP-event windows around the whole call, the per-kernel averages from the library's
own event profiler (trxsig_profile_collect_n: k_l1rx_demux against the decoders' launches), and the two stream decoders alone on
synthetic host-built indices of the same shapes.  The kernel trace is a separate run: rocprofv3 --kernel-trace --stats.

    python tools/l1rx_bench.py [--arfcns 128] [--frames 104] [--reps 50]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle")]


def main():
    import torch
    import _pkg
    ap = argparse.ArgumentParser()
    ap.add_argument("--arfcns", type=int, default=128)
    ap.add_argument("--frames", type=int, default=104)
    ap.add_argument("--reps", type=int, default=50)
    a = ap.parse_args()
    m = _pkg.load()
    ctx = m.TrxSig(4, 0)
    ctx.use_torch_stream()
    rng = np.random.default_rng(1)
    A, F = a.arfcns, a.frames
    comb = rng.choice(np.array([1, 7], np.uint8), (A, 8))
    comb[0, 0] = 5
    T = 8 * F
    n_rows = T * A
    row = torch.from_numpy(rng.permutation(n_rows).astype(np.int32).reshape(T, A)).cuda()
    valid = torch.full((n_rows,), m.F_DETECT, dtype=torch.uint8, device="cuda")
    amp = torch.full((n_rows, 2), 1000.0, device="cuda")
    toa = torch.zeros(n_rows, device="cuda")
    soft = torch.rand(n_rows, 148, device="cuda")
    res = m.TrxGroupResult(n_slots=T, n_arfcn=A, n_rows=n_rows, d_row=row.data_ptr(), d_valid=valid.data_ptr(), d_flags=None,
                           d_amp=amp.data_ptr(), d_toa=toa.data_ptr(), d_avgpwr=None, d_threshold=None, d_soft=soft.data_ptr(),
                           soft_stride=148)
    l1 = m.L1Rx(ctx, comb, 0)
    fn = 1000

    def window(fnc):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        ts = []
        for i in range(a.reps):
            ev[0].record(); fnc(); ev[1].record(); torch.cuda.synchronize()
            ts.append(ev[0].elapsed_time(ev[1]) * 1000.0)
        return float(np.median(ts))

    for _ in range(5):
        l1.decode(res, fn)
    torch.cuda.synchronize()
    whole = window(lambda: l1.decode(res, fn))
    ctx.L.trxsig_profile_enable(ctx.h, 1)
    for _ in range(a.reps):
        l1.decode(res, fn)
    n = ctx.L.trxsig_kernel_count()
    import ctypes as C
    ms = (C.c_float * n)(); cnt = (C.c_int * n)()
    ctx.L.trxsig_profile_collect_n(ctx.h, n, ms, cnt)
    ctx.L.trxsig_profile_enable(ctx.h, 0)
    split = {ctx.L.trxsig_kernel_name(i).decode(): round(ms[i] * 1000.0 / cnt[i], 2) for i in range(n) if cnt[i]}
    # the same two stream decoders on the same grid shapes, fed SYNTHETIC indices built beforehand (strided rows, every slot
    # present): a lower bound for "decoders without the demux", not the demux's permuted-row access pattern
    out = l1.out
    nt, nx = out.n_tch, out.n_xcch
    o = l1.collect(state=False)
    st_t = torch.zeros(nt, m.TCH_RX_STATE_BYTES, dtype=torch.uint8, device="cuda")
    st_x = torch.zeros(nx, m.XCCH_RX_STATE_BYTES, dtype=torch.uint8, device="cuda")
    idx_t = torch.full((nt, 4 * out.nb_tch), -1, dtype=torch.int32, device="cuda")
    idx_x = torch.full((nx, 4 * out.nb_xcch), -1, dtype=torch.int32, device="cuda")
    stat_t = torch.zeros(nt, out.nb_tch, dtype=torch.uint8, device="cuda"); fr_t = torch.zeros(nt, out.nb_tch, 33, dtype=torch.uint8, device="cuda")
    fa_t = torch.zeros(nt, out.nb_tch, 23, dtype=torch.uint8, device="cuda")
    stat_x = torch.zeros(nx, out.nb_xcch, dtype=torch.uint8, device="cuda"); fr_x = torch.zeros(nx, out.nb_xcch, 23, dtype=torch.uint8, device="cuda")
    idx_t.copy_(torch.arange(4 * out.nb_tch, device="cuda", dtype=torch.int32).repeat(nt, 1) * 7 % n_rows)
    idx_x.copy_(torch.arange(4 * out.nb_xcch, device="cuda", dtype=torch.int32).repeat(nx, 1) * 11 % n_rows)

    def decoders_only():
        ctx.fec_tch_decode_stream(soft, idx_t, st_t, stat_t, fr_t, fa_t)
        ctx.fec_xcch_decode_stream(soft, idx_x, st_x, stat_x, fr_x)
    for _ in range(3):
        decoders_only()
    host_fed = window(decoders_only)
    print(json.dumps(dict(arfcns=A, frames=F, n_tch=nt, n_xcch=nx, nb_tch=out.nb_tch, nb_xcch=out.nb_xcch, rach_cap=out.rach_cap,
                          rach_listed=int(len(o["rach"]["fn"])), decode_us=round(whole, 1), per_kernel_us=split,
                          tch_xcch_decoders_host_indices_us=round(host_fed, 1))))


if __name__ == "__main__":
    main()
