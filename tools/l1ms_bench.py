"""Time the mobile-side uplink L1 on the production plan of the l1rx / l1tx tests (128 ARFCNs; C0: combination V on TN 0, VII on
TN 1, I elsewhere; I on every other carrier) over 104 frames at sps 4: one trxsig_l1ms_encode, one trxsig_l1ms_radiate of it,
and the composition a caller would write for the radiate today on the same bursts -- trxsig_modulate_batch (no gain) ->
trxsig_delay_vector_batch -> trxsig_scale_vector_batch over the non-empty slots, into packed rows (the empty cells' zeros and
the scatter into the pull layout are not even counted).  Medians of repeated HIP-event windows.  A side measurement: no
threshold anywhere.  Results go to profiles/l1ms_bench.json (or --out) and to stdout.

    python tools/l1ms_bench.py [--arfcns 128] [--frames 104] [--reps 30] [--out profiles/l1ms_bench.json]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")]


def main():
    import torch
    import _pkg
    ap = argparse.ArgumentParser()
    ap.add_argument("--arfcns", type=int, default=128)
    ap.add_argument("--frames", type=int, default=104)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "l1ms_bench.json"))
    a = ap.parse_args()
    m = _pkg.load()
    sps = 4
    ctx = m.TrxSig(sps, 0)
    ctx.use_torch_stream()
    rng = np.random.default_rng(1)
    A, F, bsic = a.arfcns, a.frames, 33
    comb = np.ones((A, 8), np.uint8)
    comb[0, 0], comb[0, 1] = 5, 7
    ms = m.L1Ms(ctx, comb, bsic)
    fn = 1326 * 3                                            # a 51- and 26-multiframe boundary
    nbt, nbx, nr = ms.grid(fn, F)
    nt, nx = ms.channels(m.L1_TCH), ms.channels(m.L1_XCCH)
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    tk = dev(rng.choice(np.array([0, 1, 1, 2], np.uint8), (nt, nbt)))
    tp = dev(rng.integers(0, 256, (nt, nbt, 33)).astype(np.uint8))
    xk = dev(np.ones((nx, nbx), np.uint8)); xp = dev(rng.integers(0, 256, (nx, nbx, 23)).astype(np.uint8))
    rk = dev(np.ones(nr, np.uint8)); ra = dev(rng.integers(0, 256, nr).astype(np.uint8))

    def gains(n):
        g = rng.uniform(300, 3000, n) * np.exp(2j * np.pi * rng.uniform(size=n))
        return dev(g.astype(np.complex64).view(np.float32).reshape(-1, 2))
    air = dict(tch_gain=gains(nt), xcch_gain=gains(nx), rach_gain=gains(nr),
               tch_delay=dev(rng.uniform(-0.5, 1.5, nt).astype(np.float32)), xcch_delay=dev(rng.uniform(-0.5, 1.5, nx).astype(np.float32)),
               rach_delay=dev(rng.uniform(0, 63, nr).astype(np.float32)),
               amp_of_power=dev((10.0 ** ((np.arange(41) - 33) / 20.0)).astype(np.float32)))
    T, cell = 8 * F, 160 * sps
    buf = torch.zeros(T, A, cell, 2, dtype=torch.float32, device="cuda")

    def encode():
        ms.encode(fn, F, tk, tp, xk, xp, rk, ra)

    def radiate():
        ms.radiate(buf, A * cell, cell, **air)

    def window(fnc):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        ts = []
        for _ in range(a.reps):
            ev[0].record(); fnc(); ev[1].record(); torch.cuda.synchronize()
            ts.append(ev[0].elapsed_time(ev[1]) * 1000.0)
        return float(np.median(ts))

    for _ in range(3):
        encode(); radiate()
    torch.cuda.synchronize()
    enc_us, rad_us = window(encode), window(radiate)
    r = ms.collect(state=False)
    on = r["what"] != 0
    n_sent = int(on.sum())

    # ---- the three primitives on the same bursts, packed ----
    sel = np.argwhere(on)                                    # (arfcn, slot)
    bits = dev(r["bits"][on])
    guard = dev((8 + (sel[:, 1] % 4 == 0)).astype(np.int32))
    B, pitch = n_sent, 157 * sps
    off = dev((np.arange(B, dtype=np.int64) * pitch).astype(np.int32))
    length = dev(((148 + 8 + (sel[:, 1] % 4 == 0)) * sps).astype(np.int32))
    delays = dev(rng.uniform(-2, 6, B).astype(np.float32))
    scales = gains(B)
    x = torch.zeros(B * pitch, 2, dtype=torch.float32, device="cuda")
    y = torch.zeros_like(x)
    L = ctx.L

    def chain():
        ctx.modulate(bits, guard, x, off)
        L.trxsig_delay_vector_batch(ctx.h, x.data_ptr(), off.data_ptr(), length.data_ptr(), B, delays.data_ptr(), 0, y.data_ptr())
        L.trxsig_scale_vector_batch(ctx.h, y.data_ptr(), off.data_ptr(), length.data_ptr(), B, pitch, scales.data_ptr(), 0)
    for _ in range(3):
        chain()
    chain_us = window(chain)
    out = dict(arfcns=A, frames=F, sps=sps, n_tch=nt, n_xcch=nx, nb_tch=nbt, nb_xcch=nbx, n_rach=nr, slots=A * T, slots_sent=n_sent,
               encode_us=round(enc_us, 1), radiate_us=round(rad_us, 1), radiate_mbursts_per_s=round(A * T / rad_us, 2),
               radiate_gbytes_per_s=round(A * T * 156.125 * sps * 8 / rad_us / 1e3, 1),
               chain_us=round(chain_us, 1),
               chain_note="modulate + delayVector + scaleVector on the non-empty slots only, packed rows; no zero fill, no scatter")
    print(json.dumps(out))
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
