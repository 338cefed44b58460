"""Time the fading-tap generator (trxsig_air_fade, include/trxsig_air.h) at sps 4 on the production plan: 128 ARFCNs x 104 frames,
a six-path profile with 16 sinusoids per path, 32 taps -- beside trxsig_air_cells run with those taps (every stage on), and
beside the time its own bytes (the taps written, the Doppler words and the profile read) would take at the sustained HBM rate
tools/hbm_bench.hip reports on the same box (--hbm-bench: the compiled binary, run first in a process of its own; or --hbm-tbps: a
figure measured elsewhere).  Medians of repeated HIP-event windows, the taps going to a rotation of arrays larger than the
Infinity Cache together.  Last, not timed: the uplink loop l1ms -> radiate -> [l1hop] -> fade + cells -> [l1hop back] ->
trxsig_trxgroup_pull -> trxsig_l1rx_decode of tools/air_bench.py under a slow, frequency-selective profile at one noise level,
once without and once with trxsig_l1hop, and how many XCCH blocks the stream decoder erases in each (--leg mlse: with the
sequence equaliser on the group's TSC leg instead of demodulateBurst).  Side measurements: no
threshold anywhere.  The profiles are tests/air_fade_model.py's (written from memory: inputs, not contract).  Results go to
profiles/air_fade_bench.json (or --out) and to stdout.

    hipcc --offload-arch=gfx950 -O3 tools/hbm_bench.hip -o hbm_bench
    python tools/air_fade_bench.py --hbm-bench ./hbm_bench [--arfcns 128] [--frames 104] [--reps 30] [--leg demod|mlse] [--out profiles/air_fade_bench.json]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]
SLOT_S = 15.0 / 26.0 * 1e-3                                   # a slot: 0.577 ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--arfcns", type=int, default=128)
    ap.add_argument("--frames", type=int, default=104)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--profile", default="TU6")
    ap.add_argument("--sinusoids", type=int, default=16)
    ap.add_argument("--taps", type=int, default=32)
    ap.add_argument("--loop-taps", type=int, default=12)
    ap.add_argument("--doppler-hz", type=float, default=2.0, help="the loop's maximum Doppler shift")
    ap.add_argument("--snr-db", type=float, default=15.0, help="the loop's mean SNR")
    ap.add_argument("--leg", choices=("demod", "mlse"), default="demod",
                    help="the loop's TSC leg: demodulateBurst, or the sequence equaliser (TRXSIG_TSCLEG_MLSE)")
    ap.add_argument("--hbm-bench", default=None, help="compiled tools/hbm_bench.hip, run before anything else")
    ap.add_argument("--hbm-tbps", type=float, default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "air_fade_bench.json"))
    a = ap.parse_args()
    if (a.hbm_bench is None) == (a.hbm_tbps is None):
        raise SystemExit("give --hbm-bench or --hbm-tbps")
    from air_bench import hbm_rate
    from l1hop_bench import production_plan
    tbps, line = hbm_rate(a.hbm_bench) if a.hbm_bench else (a.hbm_tbps, "given on the command line")

    import torch
    import _pkg
    import air_fade_model as fm
    m = _pkg.load()
    sps = 4
    ctx = m.TrxSig(sps, 0)
    ctx.use_torch_stream()
    rng = np.random.default_rng(1)
    A, F, bsic = a.arfcns, a.frames, 33
    T, cell = 8 * F, 160 * sps
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    u32 = lambda x: dev(np.asarray(x, np.uint32).view(np.int32))
    prof = fm.profile(a.profile)
    P, S = len(prof["delay_ns"]), a.sinusoids
    n_links = 8 * A
    fn = 1326 * 3

    def window(fnc):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        ts = []
        for _ in range(a.reps):
            ev[0].record(); fnc(); ev[1].record(); torch.cuda.synchronize()
            ts.append(ev[0].elapsed_time(ev[1]) * 1000.0)
        return float(np.median(ts))

    # ---- the generator alone, then the cell form run with its taps ----
    air = m.Air(ctx)
    air.fade_profile(n_sinusoids=S, n_taps=a.taps, centre=4, **prof)
    dop = u32(rng.integers(0, int(200.0 * SLOT_S * 2 ** 32), n_links))      # up to 200 Hz
    tap_bytes = A * T * a.taps * 8
    n_copies = max(2, (512 << 20) // tap_bytes + 1)
    taps = [torch.zeros(A, T, a.taps, 2, dtype=torch.float32, device="cuda") for _ in range(n_copies)]
    turn = [0]

    def fade_call():
        turn[0] += 1
        air.fade(fn, A, F, 7, n_links, dop, taps[turn[0] % n_copies])
    for _ in range(3):
        fade_call()
    fade_us = window(fade_call)
    touched = tap_bytes + 4 * n_links + 2048                   # the taps written; the Doppler words and the profile read
    floor = touched / (tbps * 1e12) * 1e6
    out = dict(arfcns=A, frames=F, sps=sps, cells=A * T, profile=a.profile, paths=P, sinusoids=S, n_taps=a.taps,
               philox_blocks=A * T * P * (S + 1), tap_bytes=tap_bytes, tap_arrays_in_rotation=n_copies, hbm_read_tbps=tbps,
               hbm_bench_line=line, fade_us=round(fade_us, 1), fade_bytes_at_hbm_rate_us=round(floor, 2),
               fade_over_floor=round(fade_us / floor, 2), fade_gblocks_per_s=round(A * T * P * (S + 1) / fade_us / 1e3, 2))
    clean = torch.zeros(T, A, cell, 2, dtype=torch.float32, device="cuda")
    clean[:, :, :156 * sps] = dev(rng.standard_normal((A, 156 * sps, 2)).astype(np.float32))[None]
    rxbuf = torch.zeros_like(clean)
    step, phase = u32(rng.integers(0, 1 << 20, (A, T))), u32(rng.integers(0, 1 << 32, (A, T)))
    sigma = dev(np.full((A, T), 0.1, np.float32))
    cells_call = lambda: air.cells(fn, A, F, 7, clean, A * cell, cell, rxbuf, A * cell, cell, taps=taps[0], step=step, phase=phase, sigma=sigma)
    for _ in range(3):
        cells_call()
    out["cells_with_those_taps_us"] = round(window(cells_call), 1)
    out["fade_share_of_cells"] = round(fade_us / out["cells_with_those_taps_us"], 4)
    del taps, rxbuf

    # ---- not timed: XCCH erasures through the uplink loop, without and with hopping ----
    comb, group, hsn = production_plan(A)
    ms = m.L1Ms(ctx, comb, bsic)
    nbt, nbx, nr = ms.grid(fn, F)
    nt, nx = ms.channels(m.L1_TCH), ms.channels(m.L1_XCCH)
    tk = rng.choice(np.array([0, 1, 1, 2], np.uint8), (nt, nbt))
    ms.encode(fn, F, dev(tk), dev(rng.integers(0, 256, (nt, nbt, 33)).astype(np.uint8)), dev(np.ones((nx, nbx), np.uint8)),
              dev(rng.integers(0, 256, (nx, nbx, 23)).astype(np.uint8)), dev(np.ones(nr, np.uint8)), dev(rng.integers(0, 256, nr).astype(np.uint8)))
    amp = 1000.0
    gains = lambda n: dev((amp * np.exp(2j * np.pi * rng.uniform(size=n))).astype(np.complex64).view(np.float32).reshape(-1, 2))
    clean.zero_()
    ms.radiate(clean, A * cell, cell, tch_gain=gains(nt), xcch_gain=gains(nx), rach_gain=gains(nr), tch_delay=dev(np.zeros(nt, np.float32)),
               xcch_delay=dev(np.zeros(nx, np.float32)), rach_delay=dev(np.zeros(nr, np.float32)), amp_of_power=dev(np.ones(41, np.float32)))
    Lh = a.loop_taps
    air.fade_profile(n_sinusoids=S, n_taps=Lh, centre=0, **prof)
    D = int(round(a.doppler_hz * SLOT_S * 2 ** 32))
    dop = u32(np.full(n_links, D))
    sg = dev(np.full((A, T), amp * 10.0 ** (-a.snr_db / 20.0) / np.sqrt(2.0), np.float32))
    ltaps = torch.zeros(A, T, Lh, 2, dtype=torch.float32, device="cuda")
    radio, back = torch.zeros_like(clean), torch.zeros_like(clean)
    hp = m.L1Hop(ctx, comb, group, hsn, max_frames=F)
    # a handset keeps its link on whichever radio row it lands on: link[radio row][t] = 8 a + t % 8 of the channel row a there
    rmap = hp.map(fn, F).to(torch.int64)                        # [T][A]: the radio row of channel row a in slot t
    t_ix = torch.arange(T, device="cuda")[:, None].expand(T, A)
    link_ch = (8 * torch.arange(A, device="cuda")[None, :] + (t_ix % 8)).to(torch.int32)
    link = torch.full((A, T), -1, dtype=torch.int32, device="cuda")
    link[rmap.reshape(-1), t_ix.reshape(-1)] = link_ch.reshape(-1)
    fer = {}
    for hop in (0, 1):
        if hop:
            hp.cells(1, fn, F, clean, A * cell, cell, radio, A * cell, cell)
            air.fade(fn, A, F, 11, n_links, dop, ltaps, link)
            air.cells(fn, A, F, 100, radio, A * cell, cell, taps=ltaps, sigma=sg)
            hp.cells(0, fn, F, radio, A * cell, cell, back, A * cell, cell)
        else:
            air.fade(fn, A, F, 11, n_links, dop, ltaps)
            air.cells(fn, A, F, 100, clean, A * cell, cell, back, A * cell, cell, taps=ltaps, sigma=sg)
        grp = m.TrxGroup(ctx, A, tsc_leg=m.TSCLEG_MLSE if a.leg == "mlse" else m.TSCLEG_DEMOD, start=(fn, 0))
        for ar in range(A):
            for cmd in ["CMD RXTUNE 890000", "CMD TXTUNE 935000", "CMD SETTSC %d" % (bsic & 7)] + \
                       ["CMD SETSLOT %d %d" % (tn, comb[ar, tn]) for tn in range(8)] + ["CMD POWERON"]:
                grp.control(ar, cmd)
        rx = m.L1Rx(ctx, comb, bsic)
        res = grp.pull(back.data_ptr(), A * cell, cell, fn, 0, T)
        grp.sync()
        rx.decode(res, fn)
        xs = rx.collect(state=False)["xcch_status"]
        done = (xs & m.FEC_DECODED) != 0
        fer["with_l1hop" if hop else "without_l1hop"] = dict(xcch_blocks=int(done.sum()), xcch_erased=int((done & ((xs & m.FEC_TCH_GOOD) == 0)).sum()))
        rx.destroy(); grp.close()
    out["uplink_loop"] = dict(profile=a.profile, doppler_hz=a.doppler_hz, snr_db=a.snr_db, n_taps=Lh, leg=a.leg, erasures=fer)
    out["note"] = ("fade_bytes_at_hbm_rate_us: the taps written plus the Doppler words and the profile read, over hbm_read_tbps; "
                   "cells_with_those_taps_us: trxsig_air_cells, every stage on, out of place, reading the generated taps; the loop: "
                   "one link per (ARFCN, TN), SNR = mean |h|^2 amplitude^2 / (2 sigma^2), the TSC leg of --leg (demod: demodulateBurst, "
                   "no equaliser; mlse: trxsig_mlse_batch's sequence equaliser), the same encoded frames and the same links without and with hopping (groups of 64 rows per TN)")
    print(json.dumps(out))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    hp.destroy(); ms.destroy(); air.destroy()
    ctx.close()


if __name__ == "__main__":
    main()
