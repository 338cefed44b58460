"""The wideband transmit synthesiser (trxsig_txbe_create_wideband) at a site's shape: 16 wideband streams x 8 carriers 400 kHz apart
(128 ARFCNs), rate factor 8 (3.2 MS/s), sps 4, 480 bursts per push then one pop; beside it the narrowband back end's own shape
(tools/txbe_bench.py: 128 streams x 480 bursts, fused) on the same box.  Prints one JSON line.
    python tools/txwb_bench.py [--sw 16] [--carriers 8] [--rate 8] [--bursts 480] [--reps 50]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import numpy as np
import torch

import _pkg

pkg = _pkg.load()
from openbts_ttsou_amd.frontend import TxBackEnd
from openbts_ttsou_amd import synth


def measure(be, bits, guard, gain, reps):
    def step():
        be.push_bursts(bits, guard, gain)
        return be.pop_samples()
    for _ in range(5):
        step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        iq = step()
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / reps
    L, h = be.ctx.L, be.ctx.h
    L.trxsig_profile_enable(h, 1)
    for _ in range(10):
        step()
    n = L.trxsig_kernel_count()
    ms = (C.c_float * n)(); cnt = (C.c_int * n)()
    L.trxsig_profile_collect_n(h, n, ms, cnt)
    L.trxsig_profile_enable(h, 0)
    L.trxsig_kernel_name.restype = C.c_char_p
    kern = {L.trxsig_kernel_name(i).decode(): round(ms[i] * 1000.0 / cnt[i], 1) for i in range(n) if cnt[i]}
    return dt, kern, iq


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sw", type=int, default=16)
    ap.add_argument("--carriers", type=int, default=8)
    ap.add_argument("--rate", type=int, default=8)
    ap.add_argument("--bursts", type=int, default=480)
    ap.add_argument("--reps", type=int, default=50)
    a = ap.parse_args()
    sps, Sw, Cn, R, nb = 4, a.sw, a.carriers, a.rate, a.bursts
    S = Sw * Cn
    dev = torch.device("cuda:0")
    fs = 400e3 * R
    freq = np.float32([-2.0 * np.pi * (c - (Cn - 1) / 2.0) * 400e3 / fs for c in range(Cn)])
    lpf = synth.design_lpf(7 * 96 * R + 1, 96 * R, beta=6.0, cutoff=0.5)
    g = torch.Generator(device=dev); g.manual_seed(1)
    bits = torch.randint(0, 2, (S, nb, 148), dtype=torch.uint8, device=dev, generator=g)
    gain = torch.rand(S, nb, device=dev, generator=g) * 0.9 + 0.1
    guard = np.array([8 + (k % 4 == 0) for k in range(nb)], np.int32)
    ctx = pkg.TrxSig(sps, 0); ctx.use_torch_stream()
    be = TxBackEnd(ctx, Sw, lpf, gain=13500.0 / Cn, max_bursts=nb, carrier_freq=freq, rate_factor=R)
    dt, kern, iq = measure(be, bits, guard, gain, a.reps)
    k_us = kern.get("k_tx_wideband", 0.0)
    out = {"shape": {"wide_streams": Sw, "carriers": Cn, "arfcns": S, "rate_factor": R, "sps": sps, "bursts_per_push": nb,
                     "taps": int(lpf.size), "taps_per_output": -(-lpf.size // (96 * R))},
           "wideband": {"us_per_step": round(dt * 1e6, 1), "Mbursts_per_s": round(S * nb / dt / 1e6, 1),
                        "kernel_Mbursts_per_s": round(S * nb / (k_us * 1e-6) / 1e6, 1) if k_us else None,
                        "int16_samples_per_pop": int(iq.shape[1]) * Sw, "kernels_us": kern,
                        "ns_per_output_carrier": round(k_us * 1e3 / (iq.shape[1] * Sw * Cn), 4) if k_us else None}}
    be.close()
    nbe = TxBackEnd(ctx, 128, synth.design_lpf(651, 96), max_bursts=480)
    bits_n = torch.randint(0, 2, (128, 480, 148), dtype=torch.uint8, device=dev, generator=g)
    gain_n = torch.rand(128, 480, device=dev, generator=g) * 0.9 + 0.1
    guard_n = np.array([8 + (k % 4 == 0) for k in range(480)], np.int32)
    dt_n, kern_n, _ = measure(nbe, bits_n, guard_n, gain_n, a.reps)
    out["narrowband_reference"] = {"shape": "128 streams x 480 bursts, sps 4, fused (tools/txbe_bench.py)", "us_per_step": round(dt_n * 1e6, 1),
                                   "Mbursts_per_s": round(128 * 480 / dt_n / 1e6, 1), "kernels_us": kern_n}
    nbe.close(); ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
