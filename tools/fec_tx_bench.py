#!/usr/bin/env python3
"""Side measurement for the downlink L1 encode: k_fec_tch_encode on 1,024 traffic channels x 16 blocks (65,536 bursts,
mixed speech / FACCH / filler) and k_fec_sch_encode on 65,536 SCH bursts, inputs resident in HBM, with the CPU oracle
(oracle/fec_tx_oracle.c, OpenMP over channels) timed beside it.  Prints one JSON line per workload in the shape of
tools/fec_bench.py's.  Run on the GPU box: python tools/fec_tx_bench.py"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "oracle"))
import numpy as np
import torch
import _pkg
import fectxbind

pkg = _pkg.load()
t = pkg.TrxSig(4, 0); t.use_torch_stream()
o = fectxbind.FecTxOracle()
cores = min(os.cpu_count() or 1, 16)
rng = np.random.default_rng(1)
S, n = 1024, 16
B = 4 * S * n
kind = rng.integers(0, 3, (S, n)).astype(np.uint8)
payload = rng.integers(0, 256, (S, n, 33)).astype(np.uint8)
tsc = rng.integers(0, 8, S).astype(np.uint8)
filler = rng.integers(0, 2, 456).astype(np.uint8)
t.fec_tch_set_filler(filler)
dk, dp, dt_ = (torch.from_numpy(a).cuda() for a in (kind, payload, tsc))
state = torch.zeros(S, 32, dtype=torch.uint8, device="cuda")
tch_bits = torch.zeros(S, n, 4, 148, dtype=torch.uint8, device="cuda")
fn = rng.integers(0, 2715648, B).astype(np.uint32); bsic = rng.integers(0, 64, B).astype(np.uint8)
dfn, dbs = torch.from_numpy(fn.view(np.int32)).cuda(), torch.from_numpy(bsic).cuda()
sch_bits = torch.zeros(B, 148, dtype=torch.uint8, device="cuda")
ns = 64                                                   # channels in the CPU sample of the TCH workload
work = {
    # bytes moved by the kernel: 592 B out per block, 33 + 1 B in per block, 32 B state in + out per channel (TCH);
    # 148 B out + 5 B in per burst (SCH)
    "tch": ("k_fec_tch_encode", lambda: t.fec_tch_encode(dk, dp, dt_, state, tch_bits), 592 * S * n, (33 + 1) * S * n + 64 * S,
            lambda: o.tch_encode_stream(kind[:ns], payload[:ns], tsc[:ns], filler, nthreads=cores), 4 * ns * n,
            "TCH/FS + FACCH/F: %d channels x %d blocks (%d bursts), kinds uniform over speech / FACCH / filler" % (S, n, B)),
    "sch": ("k_fec_sch_encode", lambda: t.fec_sch_encode(dfn, dbs, sch_bits), 148 * B, 5 * B,
            lambda: o.sch_encode(fn[:16384], bsic[:16384]), 16384, "SCH: %d bursts, random FN and BSIC" % B),
}
for name, (kname, fnc, out_bytes, in_bytes, cpu, cpu_bursts, desc) in work.items():
    for _ in range(400): fnc()
    torch.cuda.synchronize(); t0 = time.perf_counter()
    K = 500
    for _ in range(K): fnc()
    torch.cuda.synchronize(); dt = (time.perf_counter() - t0) / K
    t.profile_enable(True)
    for _ in range(50): fnc()
    prof = t.profile_collect(); t.profile_enable(False)
    kms = prof[kname][0] / prof[kname][1]
    c0 = time.perf_counter(); reps = 0
    while time.perf_counter() - c0 < 4.0:
        cpu(); reps += 1
    cdt = (time.perf_counter() - c0) / reps
    gbs = (out_bytes + in_bytes) / (kms * 1e-3) / 1e9
    print(json.dumps({
        "metric": "Mbursts/s through the downlink L1 encode (%s)" % name, "value": round(B / (kms * 1e-3) / 1e6, 2),
        "unit": "Mbursts/s", "n_gpus": 1, "steps": K, "ms_per_step": round(dt * 1e3, 4),
        "host_loop_mbursts_s": round(B / dt / 1e6, 2), "dtype": "u8 bits", "data": "synthetic",
        "config": {"workload": desc},
        "roofline": {"bound": "hbm", "kernel": kname, "achieved": round(gbs, 1), "peak": 8000.0, "unit": "GB/s",
                     "frac": round(gbs / 8000.0, 4), "avg_kernel_ms": round(kms, 4), "write_bytes": out_bytes,
                     "read_bytes": in_bytes, "write_floor_us": round(out_bytes / 8000e9 * 1e6, 3)},
        "cpu_baseline": {"value": round(cpu_bursts / cdt / 1e6, 3), "unit": "Mbursts/s", "cores": cores, "kind": "port",
                         "sample": "%d passes over %d bursts (oracle/fec_tx_oracle.c%s)" % (reps, cpu_bursts, ", OpenMP over channels"
                                                                                        if name == "tch" else ", one thread")}}),
          flush=True)
