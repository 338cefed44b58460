"""Time the interference-rejection equaliser (trxsig_mlse_irc_batch, include/trxsig.h) at sps 4 on 65,536 normal bursts, beside
trxsig_mlse_div_batch on the same batch in the same run, and both beside the time ONE read of both antennas' samples would take at
the sustained HBM rate tools/hbm_bench.hip reports on the same box (--hbm-bench: the compiled binary, run first in a process of its
own; or --hbm-tbps: a figure measured elsewhere).  Medians of repeated HIP-event windows; the sample buffers rotate, together larger
than the memory-side cache, as in tools/mlse_div_bench.py, so that every timed call reads its samples from HBM.  The ratio to
k_mlse_div is reported, not asserted.  Last, not timed: tools/mlse_div_bench.py's uplink loop (l1ms -> radiate -> fade + cells ->
trxsig_trxgroup_pull per antenna) with an INTERFERING handset on every ARFCN -- a second l1ms with another training sequence, its
own fade per antenna, accumulated onto both antennas' cells through trxsig_air_cells at --ci-db below the wanted handsets -- and
the payload bit errors of the dedicated channels' normal bursts through trxsig_trxgroup_combine_div and through
trxsig_trxgroup_combine_irc (loading 1/64).  Side measurements: nothing is asserted.  Results go to profiles/mlse_irc_bench.json
(or --out) and to stdout.

    hipcc --offload-arch=gfx950 -O3 tools/hbm_bench.hip -o hbm_bench
    python tools/mlse_irc_bench.py --hbm-bench ./hbm_bench [--bursts 65536] [--reps 30] [--arfcns 128] [--frames 104] [--ci-db 3]"""
import numpy as np

import mlse_bench_lib as lib
from mlse_bench_lib import PAYLOAD

SLOT_S = 15.0 / 26.0 * 1e-3                                   # a slot: 0.577 ms


def kernel_times(m, a, tbps, line):
    import torch
    from openbts_ttsou_amd import synth
    sps, B, tsc = 4, a.bursts, a.tsc
    ctx = m.TrxSig(sps, 0)
    ctx.use_torch_stream()
    # tools/mlse_div_bench.py's batch (the wanted bursts plus an echo per antenna) with an interferer: the library's synthetic bursts
    # of another training sequence and another seed, through another gain per antenna, 3 dB down
    x, off, length, meta = synth.normal_batch_torch(sps, B, tsc, seed=3)
    xi = synth.normal_batch_torch(sps, B, (tsc + 3) % 8, seed=4)[0]
    x0 = (lib.echoed(x, sps) + xi * complex(0.5, 0.5)).contiguous()
    x1 = (lib.echoed(x, 2 * sps, complex(-0.2, 0.5)) * complex(0.3, 0.8) + xi * complex(-0.6, 0.37)).contiguous()
    del x, xi
    rot = lib.Rotation(a.reps, x0, x1)
    xs0, xs1 = rot.xs
    w = lib.TwoAntennas(B)
    soft_d, soft_i = w.soft
    cov = torch.zeros(B, 4, device="cuda")
    ctx.mlse_irc_normal(x0, off, x1, off, length, tsc, w.flags, w.amp, w.toa, w.sel, soft_i, cov=cov, chan=w.chan, win=w.win, energy_thresh=-1.0)
    w.select()
    div = lambda k: ctx.mlse_div(xs0[k], off, xs1[k], off, length, tsc, w.amp_s, w.toa_s, soft_d, primary=w.sel, enable=w.en, chan=w.chan, win=w.win)
    irc = lambda k: ctx.mlse_irc(xs0[k], off, xs1[k], off, length, tsc, w.amp_s, w.toa_s, soft_i, primary=w.sel, enable=w.en, cov=cov, chan=w.chan,
                                 win=w.win)
    d_us, i_us = rot.timed(div, irc)
    out, floor = w.head(B, sps, tsc, rot, tbps, line)
    out.update(**lib.us("mlse_div", d_us), **lib.us("mlse_irc", i_us),
               mlse_irc_over_one_read=round(i_us[0] / floor, 2), mlse_irc_over_mlse_div=round(i_us[0] / d_us[0], 3),
               mlse_irc_ns_per_burst=round(i_us[0] * 1e3 / B, 2),
               payload_bit_errors=w.errors(meta["bits"], mlse_div=soft_d, mlse_irc=soft_i))
    ctx.close()
    return out


def uplink_loop(m, a):
    import torch
    import air_fade_model as fm
    from l1hop_bench import production_plan
    sps = 4
    ctx = m.TrxSig(sps, 0)
    ctx.use_torch_stream()
    rng = np.random.default_rng(1)
    A, F, bsic, ibsic = a.arfcns, a.frames, 33, 37            # training sequences 1 (wanted) and 5 (interferer)
    T, cell = 8 * F, 160 * sps
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    u32 = lambda x: dev(np.asarray(x, np.uint32).view(np.int32))
    prof = fm.profile(a.profile)
    S, n_links, fn = a.sinusoids, 8 * A, 1326 * 3
    comb, group, hsn = production_plan(A)
    air = m.Air(ctx)
    amp = 1000.0

    def handsets(code, level):
        """An l1ms of random payloads on every channel of the plan, radiated at `level`: (the object, its cells)."""
        ms = m.L1Ms(ctx, comb, code)
        nbt, nbx, nr = ms.grid(fn, F)
        nt, nx = ms.channels(m.L1_TCH), ms.channels(m.L1_XCCH)
        tk = rng.choice(np.array([0, 1, 1, 2], np.uint8), (nt, nbt))
        ms.encode(fn, F, dev(tk), dev(rng.integers(0, 256, (nt, nbt, 33)).astype(np.uint8)), dev(np.ones((nx, nbx), np.uint8)),
                  dev(rng.integers(0, 256, (nx, nbx, 23)).astype(np.uint8)), dev(np.ones(nr, np.uint8)), dev(rng.integers(0, 256, nr).astype(np.uint8)))
        gains = lambda n: dev((level * np.exp(2j * np.pi * rng.uniform(size=n))).astype(np.complex64).view(np.float32).reshape(-1, 2))
        cells = torch.zeros(T, A, cell, 2, dtype=torch.float32, device="cuda")
        ms.radiate(cells, A * cell, cell, tch_gain=gains(nt), xcch_gain=gains(nx), rach_gain=gains(nr), tch_delay=dev(np.zeros(nt, np.float32)),
                   xcch_delay=dev(np.zeros(nx, np.float32)), rach_delay=dev(np.zeros(nr, np.float32)), amp_of_power=dev(np.ones(41, np.float32)))
        return ms, cells
    ms, clean = handsets(bsic, amp)
    ims, iclean = handsets(ibsic, amp * 10.0 ** (-a.ci_db / 20.0))
    Lh = a.loop_taps
    air.fade_profile(n_sinusoids=S, n_taps=Lh, centre=0, **prof)
    dop = u32(np.full(n_links, int(round(a.doppler_hz * SLOT_S * 2 ** 32))))
    sg = dev(np.full((A, T), amp * 10.0 ** (-a.snr_db / 20.0) / np.sqrt(2.0), np.float32))
    ltaps = torch.zeros(A, T, Lh, 2, dtype=torch.float32, device="cuda")
    rx = [torch.zeros_like(clean), torch.zeros_like(clean)]
    for k in (0, 1):                                          # antenna k: its own fade and noise seeds, for the wanted handsets ...
        air.fade(fn, A, F, 11 + k, n_links, dop, ltaps)
        air.cells(fn, A, F, 100 + k, clean, A * cell, cell, rx[k], A * cell, cell, taps=ltaps, sigma=sg)
        air.fade(fn, A, F, 21 + k, n_links, dop, ltaps)       # ... and for the interferers, accumulated onto the cells that are there
        air.cells(fn, A, F, 200 + k, iclean, A * cell, cell, rx[k], A * cell, cell, taps=ltaps, accumulate=True)
    groups, pulls = [], []
    for k in (0, 1):
        grp = m.TrxGroup(ctx, A, tsc_leg=m.TSCLEG_DEMOD, start=(fn, 0))
        for ar in range(A):
            for cmd in ["CMD RXTUNE 890000", "CMD TXTUNE 935000", "CMD SETTSC %d" % (bsic & 7)] + \
                       ["CMD SETSLOT %d %d" % (tn, comb[ar, tn]) for tn in range(8)] + ["CMD POWERON"]:
                grp.control(ar, cmd)
        pulls.append(grp.pull(rx[k], A * cell, cell, fn, 0, T))
        grp.sync()
        groups.append(grp)
    R = pulls[0].n_rows
    view = lambda p, shape, ty: m._dev_tensor(ctx, p, shape, ty)
    sent = ms.collect(state=False)
    normal = (sent["what"].T == 1) | (sent["what"].T == 2)     # [T][A]: TRXSIG_L1MS_TCH, _XCCH
    ber, n_sel = {}, None
    for name in ("combine_div", "combine_irc"):
        sel = torch.zeros(R, dtype=torch.uint8, device="cuda")
        cov = torch.zeros(R, 4, device="cuda")
        res = groups[0].combine_div(rx[0], groups[1], rx[1], sel=sel) if name == "combine_div" else \
            groups[0].combine_irc(rx[0], groups[1], rx[1], sel=sel, cov=cov)
        torch.cuda.synchronize()
        row = view(res.d_row, (T, A), "<i4").cpu().numpy()
        rr = row[normal & (row >= 0)]
        want = np.transpose(sent["bits"], (1, 0, 2))[normal & (row >= 0)]
        found = view(res.d_valid, (R,), "|u1").cpu().numpy()[rr] != 0
        soft = view(res.d_soft, (R, res.soft_stride), "<f4").cpu().numpy()[rr][:, :148]
        e = ((soft > 0.5) != want)[:, PAYLOAD].sum(axis=1)
        ber[name] = int(np.where(found, e, len(PAYLOAD) // 2).sum())   # a burst not handed up counts as half its payload bits
        ber[name + "_on_the_bursts_handed_up"] = int(e[found].sum())
        ber.update(bursts=int(len(rr)), payload_bits=int(len(rr)) * len(PAYLOAD), handed_up_by_either=int(found.sum()))
        n_sel = [int((sel == k).sum().item()) for k in (0, 1, 2)]
        if name == "combine_irc":
            c = cov.cpu().numpy()[rr][found]
            ber["irc_sets_identity"] = int(np.all(c == np.array([1, 1, 0, 0], np.float32), axis=1).sum())
            ber["irc_median_abs_x_over_sqrt_A_Bv"] = round(float(np.median(np.hypot(c[:, 2], c[:, 3]) / np.sqrt(np.maximum(c[:, 0] * c[:, 1], 1e-30)))), 3)
    ber["combine_irc_over_combine_div"] = round(ber["combine_irc"] / max(ber["combine_div"], 1), 3)
    for grp in groups:
        grp.close()
    ms.destroy(); ims.destroy(); air.destroy(); ctx.close()
    return dict(arfcns=A, frames=F, profile=a.profile, doppler_hz=a.doppler_hz, snr_db=a.snr_db, ci_db=a.ci_db, n_taps=Lh, rows=R,
                loading=m.IRC_LOADING, rows_selected_antenna_0_1_neither=n_sel, payload_bit_errors=ber)


def main():
    ap = lib.parser("mlse_irc_bench.json", tsc=True)
    ap.add_argument("--arfcns", type=int, default=128)
    ap.add_argument("--frames", type=int, default=104)
    ap.add_argument("--profile", default="TU6")
    ap.add_argument("--sinusoids", type=int, default=16)
    ap.add_argument("--loop-taps", type=int, default=12)
    ap.add_argument("--doppler-hz", type=float, default=2.0, help="the loop's maximum Doppler shift")
    ap.add_argument("--snr-db", type=float, default=25.0, help="the loop's mean SNR, per antenna")
    ap.add_argument("--ci-db", type=float, default=3.0, help="the loop's mean carrier-to-interferer ratio, per antenna")
    a, tbps, line = lib.parse(ap)
    import _pkg
    m = _pkg.load()
    out = kernel_times(m, a, tbps, line)
    out["uplink_loop"] = uplink_loop(m, a)
    out["note"] = ("the batch: tools/mlse_div_bench.py's (synthetic normal bursts, an echo per antenna) plus an interferer of another training "
                   "sequence through a gain per antenna, 3 dB down; detection, selection, amplitude and TOA from trxsig_mlse_irc_normal_batch; "
                   "both kernels run on the same buffers with the same amplitudes and TOAs; medians of --reps HIP-event windows, one call each, "
                   "the samples read from buffers not touched since the rotation came round.  The loop: tools/mlse_div_bench.py's with a second "
                   "l1ms (BSIC 37) radiated --ci-db down, faded per antenna with seeds of its own and accumulated by trxsig_air_cells; both "
                   "groups on the demodulating leg; a burst neither antenna detected counts as half its payload bits")
    lib.write(out, a.out)


if __name__ == "__main__":
    main()
