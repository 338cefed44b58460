"""Time the two-antenna sequence equaliser (trxsig_mlse_div_batch, include/trxsig.h) at sps 4 on 65,536 normal bursts, beside
trxsig_mlse_batch on antenna 0 of the same batch in the same run, and both beside the time ONE read of both antennas' samples would
take at the sustained HBM rate tools/hbm_bench.hip reports on the same box (--hbm-bench: the compiled binary, run first in a process
of its own; or --hbm-tbps: a figure measured elsewhere).  Medians of repeated HIP-event windows; the sample buffers rotate, together
larger than the memory-side cache, so that every timed call reads its samples from HBM.  Last, not timed: the uplink loop of
tools/air_fade_bench.py (l1ms -> radiate -> fade + cells -> trxsig_trxgroup_pull -> trxsig_l1rx_decode, same profile, Doppler and
SNR arguments, no hopping) run three ways, with the XCCH blocks the stream decoder erases in each: one antenna on the MLSE leg;
two antennas with selection only (the selected pull's soft rows); two antennas through trxsig_trxgroup_combine_div.  The second
antenna is a second trxsig_air_fade seed and a second noise seed.  Side measurements: nothing is asserted.  Results go to
profiles/mlse_div_bench.json (or --out) and to stdout.

    hipcc --offload-arch=gfx950 -O3 tools/hbm_bench.hip -o hbm_bench
    python tools/mlse_div_bench.py --hbm-bench ./hbm_bench [--bursts 65536] [--reps 30] [--arfcns 128] [--frames 104] [--out profiles/mlse_div_bench.json]"""
import ctypes

import numpy as np

import mlse_bench_lib as lib

SLOT_S = 15.0 / 26.0 * 1e-3                                   # a slot: 0.577 ms


def kernel_times(m, a, tbps, line):
    import torch
    from openbts_ttsou_amd import synth
    sps, B, tsc = 4, a.bursts, a.tsc
    ctx = m.TrxSig(sps, 0)
    ctx.use_torch_stream()
    # antenna 0: the library's synthetic normal bursts plus an echo one symbol late (tools/mlse_bench.py's batch); antenna 1: the same
    # bursts through another gain and an echo two symbols late
    x, off, length, meta = synth.normal_batch_torch(sps, B, tsc, seed=3)
    x0 = lib.echoed(x, sps).contiguous()
    x1 = (lib.echoed(x, 2 * sps, complex(-0.2, 0.5)) * complex(0.3, 0.8)).contiguous()
    del x
    rot = lib.Rotation(a.reps, x0, x1)
    xs0, xs1 = rot.xs
    w = lib.TwoAntennas(B)
    soft1, soft2 = w.soft
    ctx.mlse_div_normal(x0, off, x1, off, length, tsc, w.flags, w.amp, w.toa, w.sel, soft2, chan=w.chan, win=w.win, energy_thresh=-1.0)
    w.select()
    one = lambda k: ctx.mlse(xs0[k], off, length, tsc, w.amp_s, w.toa_s, soft1, enable=w.en)
    two = lambda k: ctx.mlse_div(xs0[k], off, xs1[k], off, length, tsc, w.amp_s, w.toa_s, soft2, primary=w.sel, enable=w.en, chan=w.chan, win=w.win)
    o_us, t_us = rot.timed(one, two)
    out, floor = w.head(B, sps, tsc, rot, tbps, line)
    out.update(**lib.us("mlse_one_antenna", o_us), **lib.us("mlse_div", t_us),
               mlse_div_over_one_read=round(t_us[0] / floor, 2), mlse_div_over_mlse=round(t_us[0] / o_us[0], 2),
               mlse_div_ns_per_burst=round(t_us[0] * 1e3 / B, 2),
               payload_bit_errors=w.errors(meta["bits"], mlse_antenna_0=soft1, mlse_div=soft2))
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
    A, F, bsic = a.arfcns, a.frames, 33
    T, cell = 8 * F, 160 * sps
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    u32 = lambda x: dev(np.asarray(x, np.uint32).view(np.int32))
    prof = fm.profile(a.profile)
    S, n_links, fn = a.sinusoids, 8 * A, 1326 * 3
    comb, group, hsn = production_plan(A)
    air = m.Air(ctx)
    ms = m.L1Ms(ctx, comb, bsic)
    nbt, nbx, nr = ms.grid(fn, F)
    nt, nx = ms.channels(m.L1_TCH), ms.channels(m.L1_XCCH)
    tk = rng.choice(np.array([0, 1, 1, 2], np.uint8), (nt, nbt))
    ms.encode(fn, F, dev(tk), dev(rng.integers(0, 256, (nt, nbt, 33)).astype(np.uint8)), dev(np.ones((nx, nbx), np.uint8)),
              dev(rng.integers(0, 256, (nx, nbx, 23)).astype(np.uint8)), dev(np.ones(nr, np.uint8)), dev(rng.integers(0, 256, nr).astype(np.uint8)))
    amp = 1000.0
    gains = lambda n: dev((amp * np.exp(2j * np.pi * rng.uniform(size=n))).astype(np.complex64).view(np.float32).reshape(-1, 2))
    clean = torch.zeros(T, A, cell, 2, dtype=torch.float32, device="cuda")
    ms.radiate(clean, A * cell, cell, tch_gain=gains(nt), xcch_gain=gains(nx), rach_gain=gains(nr), tch_delay=dev(np.zeros(nt, np.float32)),
               xcch_delay=dev(np.zeros(nx, np.float32)), rach_delay=dev(np.zeros(nr, np.float32)), amp_of_power=dev(np.ones(41, np.float32)))
    Lh = a.loop_taps
    air.fade_profile(n_sinusoids=S, n_taps=Lh, centre=0, **prof)
    dop = u32(np.full(n_links, int(round(a.doppler_hz * SLOT_S * 2 ** 32))))
    sg = dev(np.full((A, T), amp * 10.0 ** (-a.snr_db / 20.0) / np.sqrt(2.0), np.float32))
    ltaps = torch.zeros(A, T, Lh, 2, dtype=torch.float32, device="cuda")
    rx = [torch.zeros_like(clean), torch.zeros_like(clean)]
    for k in (0, 1):                                          # antenna k: its own fade seed and its own noise seed
        air.fade(fn, A, F, 11 + k, n_links, dop, ltaps)
        air.cells(fn, A, F, 100 + k, clean, A * cell, cell, rx[k], A * cell, cell, taps=ltaps, sigma=sg)
    groups, pulls = [], []
    for k in (0, 1):
        grp = m.TrxGroup(ctx, A, tsc_leg=m.TSCLEG_MLSE, start=(fn, 0))
        for ar in range(A):
            for cmd in ["CMD RXTUNE 890000", "CMD TXTUNE 935000", "CMD SETTSC %d" % (bsic & 7)] + \
                       ["CMD SETSLOT %d %d" % (tn, comb[ar, tn]) for tn in range(8)] + ["CMD POWERON"]:
                grp.control(ar, cmd)
        pulls.append(grp.pull(rx[k], A * cell, cell, fn, 0, T))
        grp.sync()
        groups.append(grp)
    R = pulls[0].n_rows
    sel = torch.zeros(R, dtype=torch.uint8, device="cuda")
    joint = groups[0].combine_div(rx[0], groups[1], rx[1], sel=sel)
    # selection only: the combined result's fields with the selected pull's soft rows in d_soft's place
    view = lambda p, shape, ty: m._dev_tensor(ctx, p, shape, ty)
    s0, s1 = view(pulls[0].d_soft, (R, pulls[0].soft_stride), "<f4"), view(pulls[1].d_soft, (R, pulls[1].soft_stride), "<f4")
    valid = view(joint.d_valid, (R,), "|u1")
    picked = torch.where((sel == 1)[:, None], s1, s0)
    picked = torch.where((valid != 0)[:, None], picked, torch.zeros_like(picked)).contiguous()
    chosen = type(joint)()
    ctypes.memmove(ctypes.byref(chosen), ctypes.byref(joint), ctypes.sizeof(joint))
    chosen.d_soft = picked.data_ptr()
    # A slot in which nothing was sent still reaches the correlator, and a false alarm there hands the decoder a block of noise.  Each
    # way is therefore decoded twice: as it is, and with d_valid cleared on the slots in which nothing was sent (what a receiver that
    # knew the schedule of its handsets would do), so that the erasures of blocks that WERE sent can be read apart from the false alarms.
    sent = ms.collect(state=False)
    row = view(joint.d_row, (T, A), "<i4").cpu().numpy()
    on_air = np.zeros(R, bool)
    on_air[row[(row >= 0) & (sent["what"].T != 0)]] = True
    d_on_air = dev(on_air.astype(np.uint8))

    def only_sent(res):
        r = type(res)()
        ctypes.memmove(ctypes.byref(r), ctypes.byref(res), ctypes.sizeof(res))
        keep = (view(res.d_valid, (R,), "|u1") * d_on_air).contiguous()
        r.d_valid = keep.data_ptr()
        return r, keep
    fer, alarms = {}, {}
    for name, res in (("one_antenna_mlse_leg", pulls[0]), ("two_antennas_selection_only", chosen), ("two_antennas_combine_div", joint)):
        masked, keep = only_sent(res)
        for key, rr_ in ((name, res), (name + "_sent_slots_only", masked)):
            l1 = m.L1Rx(ctx, comb, bsic)
            l1.decode(rr_, fn)
            xs = l1.collect(state=False)["xcch_status"]
            done = (xs & m.FEC_DECODED) != 0
            fer[key] = dict(xcch_blocks=int(done.sum()), xcch_erased=int((done & ((xs & m.FEC_TCH_GOOD) == 0)).sum()))
            l1.destroy()
        alarms[name] = int(((view(res.d_valid, (R,), "|u1").cpu().numpy() != 0) & ~on_air).sum())
        del keep
    torch.cuda.synchronize()
    n_sel = [int((sel == k).sum().item()) for k in (0, 1, 2)]
    # burst level: payload bit errors against the bits sent, on the dedicated channels' normal bursts; a burst a way did not
    # hand up counts as half its payload bits
    normal = (sent["what"].T == 1) | (sent["what"].T == 2)     # [T][A]: TRXSIG_L1MS_TCH, _XCCH
    rr = row[normal & (row >= 0)]
    want = np.transpose(sent["bits"], (1, 0, 2))[normal & (row >= 0)]
    pay = np.r_[3:61, 87:145]
    v0 = view(pulls[0].d_valid, (R,), "|u1").cpu().numpy()[rr] != 0
    vj = valid.cpu().numpy()[rr] != 0

    def errors(soft, found):
        e = ((soft.cpu().numpy()[rr][:, :148] > 0.5) != want)[:, pay].sum(axis=1)
        return int(np.where(found, e, len(pay) // 2).sum())
    ber = dict(bursts=int(len(rr)), payload_bits=int(len(rr)) * len(pay), handed_up_by_antenna_0=int(v0.sum()), handed_up_by_either=int(vj.sum()),
               one_antenna_mlse_leg=errors(s0, v0), two_antennas_selection_only=errors(picked, vj),
               two_antennas_combine_div=errors(view(joint.d_soft, (R, joint.soft_stride), "<f4"), vj))
    for grp in groups:
        grp.close()
    ms.destroy(); air.destroy(); ctx.close()
    return dict(arfcns=A, frames=F, profile=a.profile, doppler_hz=a.doppler_hz, snr_db=a.snr_db, n_taps=Lh, rows=R,
                rows_selected_antenna_0_1_neither=n_sel, erasures=fer, rows_handed_up_where_nothing_was_sent=alarms,
                rows_where_nothing_was_sent=int((~on_air).sum()), payload_bit_errors=ber)


def main():
    ap = lib.parser("mlse_div_bench.json", tsc=True)
    ap.add_argument("--arfcns", type=int, default=128)
    ap.add_argument("--frames", type=int, default=104)
    ap.add_argument("--profile", default="TU6")
    ap.add_argument("--sinusoids", type=int, default=16)
    ap.add_argument("--loop-taps", type=int, default=12)
    ap.add_argument("--doppler-hz", type=float, default=2.0, help="the loop's maximum Doppler shift")
    ap.add_argument("--snr-db", type=float, default=15.0, help="the loop's mean SNR, per antenna")
    a, tbps, line = lib.parse(ap)
    import _pkg
    m = _pkg.load()
    out = kernel_times(m, a, tbps, line)
    out["uplink_loop"] = uplink_loop(m, a)
    out["note"] = ("the batch: the library's synthetic normal bursts (sigma 0 / 0.1 / 0.3 in turn), antenna 0 plus an echo one symbol late, "
                   "antenna 1 the same bursts through another gain and an echo two symbols late; detection, selection, amplitude and TOA from "
                   "trxsig_mlse_div_normal_batch; trxsig_mlse_batch runs on antenna 0 with the same amplitudes and TOAs; medians of --reps "
                   "HIP-event windows, one call each, the samples read from buffers not touched since the rotation came round.  The loop: "
                   "tools/air_fade_bench.py's without hopping, one link per (ARFCN, TN) and antenna, both groups on the MLSE leg")
    lib.write(out, a.out)


if __name__ == "__main__":
    main()
