"""Time the air (include/trxsig_air.h) at sps 4.  Cell form: 128 ARFCNs x 104 frames of the production plan's radiated cells,
every stage on, channels of 1, 5 and 32 taps -- beside trxsig_l1ms_radiate of the same plan and beside the time the cells'
traffic (one read and one write of 5 KB per cell) would take at the sustained HBM rate tools/hbm_bench.hip reports on the same
box (--hbm-bench: the compiled binary, run first in a process of its own; or --hbm-tbps: a figure measured elsewhere).  Stream
form: 128 handsets x 13 frames of one carrier each, every stage on.  Medians of repeated HIP-event windows.  Last, not timed:
the uplink loop l1ms -> radiate -> cells (noise alone) -> trxsig_trxgroup_pull -> trxsig_l1rx_decode at 6, 10 and 20 dB, and
how many TCH and XCCH blocks the stream decoders erase at each.  A side measurement: no threshold anywhere.  Results go to
profiles/air_bench.json (or --out) and to stdout.

    hipcc --offload-arch=gfx950 -O3 tools/hbm_bench.hip -o hbm_bench
    python tools/air_bench.py --hbm-bench ./hbm_bench [--arfcns 128] [--frames 104] [--reps 30] [--out profiles/air_bench.json]"""
import argparse
import json
import os
import re
import subprocess
import sys

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")]


def hbm_rate(path):
    """the read-only line of tools/hbm_bench.hip: TB/s"""
    out = subprocess.run([path], check=True, capture_output=True, text=True, timeout=300).stdout
    m = re.search(r"write 0 B .*= ([0-9.]+) TB/s", out)
    if not m:
        raise SystemExit("no read-only line in the output of %s:\n%s" % (path, out))
    return float(m.group(1)), m.group(0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--arfcns", type=int, default=128)
    ap.add_argument("--frames", type=int, default=104)
    ap.add_argument("--handsets", type=int, default=128)
    ap.add_argument("--stream-frames", type=int, default=13)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--hbm-bench", default=None, help="compiled tools/hbm_bench.hip, run before anything else")
    ap.add_argument("--hbm-tbps", type=float, default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "air_bench.json"))
    a = ap.parse_args()
    if (a.hbm_bench is None) == (a.hbm_tbps is None):
        raise SystemExit("give --hbm-bench or --hbm-tbps")
    tbps, line = hbm_rate(a.hbm_bench) if a.hbm_bench else (a.hbm_tbps, "given on the command line")

    import torch
    import _pkg
    m = _pkg.load()
    sps = 4
    ctx = m.TrxSig(sps, 0)
    ctx.use_torch_stream()
    rng = np.random.default_rng(1)
    A, F, bsic = a.arfcns, a.frames, 33
    T, cell = 8 * F, 160 * sps
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    u32 = lambda x: dev(np.asarray(x, np.uint32).view(np.int32))

    # ---- the plan's cells, radiated ----
    comb = np.ones((A, 8), np.uint8)
    comb[0, 0], comb[0, 1] = 5, 7
    ms = m.L1Ms(ctx, comb, bsic)
    fn = 1326 * 3
    nbt, nbx, nr = ms.grid(fn, F)
    nt, nx = ms.channels(m.L1_TCH), ms.channels(m.L1_XCCH)
    tk = rng.choice(np.array([0, 1, 1, 2], np.uint8), (nt, nbt))
    tp = rng.integers(0, 256, (nt, nbt, 33)).astype(np.uint8)
    ms.encode(fn, F, dev(tk), dev(tp), dev(np.ones((nx, nbx), np.uint8)), dev(rng.integers(0, 256, (nx, nbx, 23)).astype(np.uint8)),
              dev(np.ones(nr, np.uint8)), dev(rng.integers(0, 256, nr).astype(np.uint8)))
    amp = 1000.0

    def gains(n):
        return dev((amp * np.exp(2j * np.pi * rng.uniform(size=n))).astype(np.complex64).view(np.float32).reshape(-1, 2))
    air_kw = dict(tch_gain=gains(nt), xcch_gain=gains(nx), rach_gain=gains(nr), tch_delay=dev(np.zeros(nt, np.float32)),
                  xcch_delay=dev(np.zeros(nx, np.float32)), rach_delay=dev(np.zeros(nr, np.float32)),
                  amp_of_power=dev(np.ones(41, np.float32)))
    clean = torch.zeros(T, A, cell, 2, dtype=torch.float32, device="cuda")
    rxbuf = torch.zeros_like(clean)
    radiate = lambda: ms.radiate(clean, A * cell, cell, **air_kw)
    radiate()
    air = m.Air(ctx)
    step, phase = u32(rng.integers(0, 1 << 20, (A, T))), u32(rng.integers(0, 1 << 32, (A, T)))
    sigma = dev(np.full((A, T), amp * 10.0 ** (-20.0 / 20.0) / np.sqrt(2.0), np.float32))

    def window(fnc):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        ts = []
        for _ in range(a.reps):
            ev[0].record(); fnc(); ev[1].record(); torch.cuda.synchronize()
            ts.append(ev[0].elapsed_time(ev[1]) * 1000.0)
        return float(np.median(ts))

    out = dict(arfcns=A, frames=F, sps=sps, cells=A * T, hbm_read_tbps=tbps, hbm_bench_line=line)
    traffic = A * T * 156.125 * sps * 8 * 2
    out["cells_traffic_at_hbm_rate_us"] = round(traffic / (tbps * 1e12) * 1e6, 1)
    for _ in range(3):
        radiate()
    out["radiate_us"] = round(window(radiate), 1)
    for Lh in (1, 5, 32):
        taps = dev((rng.standard_normal((A, T, Lh, 2)) / np.sqrt(2.0 * Lh)).astype(np.float32))
        call = lambda: air.cells(fn, A, F, 7, clean, A * cell, cell, rxbuf, A * cell, cell, taps=taps, step=step, phase=phase, sigma=sigma)
        for _ in range(3):
            call()
        us = window(call)
        out["cells_%d_taps_us" % Lh] = round(us, 1)
        out["cells_%d_taps_gbytes_per_s" % Lh] = round(traffic / us / 1e3, 1)
    noise_only = lambda: air.cells(fn, A, F, 7, clean, A * cell, cell, rxbuf, A * cell, cell, sigma=sigma)
    noise_only()
    out["cells_noise_only_us"] = round(window(noise_only), 1)

    # ---- the stream form: every handset on a carrier of its own plan, one carrier each ----
    H, SF = a.handsets, a.stream_frames
    n_cells = 8 * SF
    N = SF * 1250 * sps - 200 * sps
    carriers = min(A, 8)
    sout = torch.zeros(H, N, 2, dtype=torch.float32, device="cuda")
    skw = dict(delay=dev(rng.uniform(0, 1, H).astype(np.float32)), step=u32(rng.integers(0, 1 << 26, H)), phase=u32(rng.integers(0, 1 << 32, H)),
               gain=dev(np.exp(2j * np.pi * rng.uniform(size=H)).astype(np.complex64).view(np.float32).reshape(-1, 2)),
               sigma=dev(np.full(H, amp * 0.1 / np.sqrt(2.0), np.float32)), n0=u32(np.zeros(H)))
    arf, cut = dev(rng.integers(0, carriers, H).astype(np.int32)), dev(rng.integers(0, 100 * sps, H).astype(np.int64))
    scall = lambda: air.stream(carriers, n_cells, 9, clean, A * cell, cell, sout, N, N, arf, cut, **skw)
    for _ in range(3):
        scall()
    us = window(scall)
    out.update(stream_handsets=H, stream_frames=SF, stream_samples=N, stream_us=round(us, 1),
               stream_gbytes_written_per_s=round(H * N * 8 / us / 1e3, 1))

    # ---- not timed: what the stream decoders erase through the uplink loop ----
    fer = {}
    for snr in (6, 10, 20):
        sg = dev(np.full((A, T), amp * 10.0 ** (-snr / 20.0) / np.sqrt(2.0), np.float32))
        air.cells(fn, A, F, 100 + snr, clean, A * cell, cell, rxbuf, A * cell, cell, sigma=sg)
        grp = m.TrxGroup(ctx, A, tsc_leg=m.TSCLEG_DEMOD, start=(fn, 0))
        for ar in range(A):
            for cmd in ["CMD RXTUNE 890000", "CMD TXTUNE 935000", "CMD SETTSC %d" % (bsic & 7)] + \
                       ["CMD SETSLOT %d %d" % (tn, comb[ar, tn]) for tn in range(8)] + ["CMD POWERON"]:
                grp.control(ar, cmd)
        rx = m.L1Rx(ctx, comb, bsic)
        res = grp.pull(rxbuf.data_ptr(), A * cell, cell, fn, 0, T)
        grp.sync()
        rx.decode(res, fn)
        got = rx.collect(state=False)
        sent = tk[:, :-1] == m.TCH_SPEECH                       # stream block b carries encoded block b - 1
        st = got["tch_status"][:, 1:1 + sent.shape[1]]
        sent = sent[:, :st.shape[1]]
        xs = got["xcch_status"]
        fer["%d_db" % snr] = dict(tch_speech_blocks=int(sent.sum()), tch_erased=int((sent & ((st & m.FEC_TCH_GOOD) == 0)).sum()),
                                  xcch_blocks=int(((xs & m.FEC_DECODED) != 0).sum()),
                                  xcch_erased=int((((xs & m.FEC_DECODED) != 0) & ((xs & m.FEC_TCH_GOOD) == 0)).sum()))
        rx.destroy(); grp.close()
    out["uplink_loop_erasures"] = fer
    out["note"] = ("cells_*: every stage on (taps, offset, noise), out of place; cells_traffic_at_hbm_rate_us: one read and one write of "
                   "every cell over hbm_read_tbps; SNR = amplitude^2 / (2 sigma^2); each SNR runs the same frames through a fresh group and a fresh decoder")
    print(json.dumps(out))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
