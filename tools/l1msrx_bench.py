"""Time the mobile-side downlink L1 on the production plan of tools/l1ms_bench.py (128 ARFCNs; C0: combination V on TN 0, VII on
TN 1, I elsewhere; I on every other carrier) over 104 frames: a live trxsig_l1tx (SIs set, random payloads, a sibling trxsig_l1rx
whose state moves every round, so the SACCH orders move) -> its d_bits as soft values (0.1 / 0.9 and uniform noise of 0.25, every
non-empty slot a row) -> trxsig_l1msrx_decode, with a trxsig_l1ms following the decoded orders.

Reported: the per-call median over repeated HIP-event windows of --calls trxsig_l1msrx_decode calls each, and, in windows that
alternate with those, of trxsig_l1rx_decode of the very same rows as the yardstick (the uplink demultiplexer routes them by the
uplink tables: the same stream decoders on a comparable number of blocks); and, per SACCH channel and round, how many rounds back the orders lie that the following handset
holds (the nearest earlier round whose orders they equal; the follower encodes a round before that round's downlink is decoded,
so 1 is the least) -- 0 is what the sibling shortcut (trxsig_l1ms_encode with the trxsig_l1tx itself) gives, by construction.  A side
measurement: no threshold anywhere.  Results go to profiles/l1msrx_bench.json (or --out) and to stdout.

    python tools/l1msrx_bench.py [--arfcns 128] [--frames 104] [--rounds 6] [--reps 30] [--calls 20] [--out profiles/l1msrx_bench.json]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")]

POWER = {900: [39, 39, 39, 37, 35, 33, 31, 29, 27, 25, 23, 21, 19, 17, 15, 13, 11, 9, 7, 5] + [5] * 12}


def level_power(band, power):
    """POWER[band][encodePower(band, power)]: nearest level, first on ties"""
    t = POWER[band]
    err = [abs(power - v) for v in t]
    return t[err.index(min(err))]


def main():
    import torch
    import _pkg
    ap = argparse.ArgumentParser()
    ap.add_argument("--arfcns", type=int, default=128)
    ap.add_argument("--frames", type=int, default=104)
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--reps", type=int, default=30, help="timed windows per call under test")
    ap.add_argument("--calls", type=int, default=20, help="decodes per window (one event pair)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "l1msrx_bench.json"))
    a = ap.parse_args()
    m = _pkg.load()
    ctx = m.TrxSig(4, 0)
    ctx.use_torch_stream()
    rng = np.random.default_rng(1)
    gen = torch.Generator(device="cuda").manual_seed(1)
    A, F, bsic, band = a.arfcns, a.frames, 33, 900
    T = 8 * F
    comb = np.ones((A, 8), np.uint8)
    comb[0, 0], comb[0, 1] = 5, 7
    tx, ul = m.L1Tx(ctx, comb, bsic, band), m.L1Rx(ctx, comb, bsic, band)
    rx, rx_timed, ul_timed = m.L1MsRx(ctx, comb, bsic, band), m.L1MsRx(ctx, comb, bsic, band), m.L1Rx(ctx, comb, bsic, band)
    follower, shortcut = m.L1Ms(ctx, comb, bsic, band), m.L1Ms(ctx, comb, bsic, band)
    follower.follow(rx)
    tx.set_si(rng.integers(0, 256, (4, 23)).astype(np.uint8))
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    nx = tx.channels(m.L1_XCCH)
    sacch = [i for i in range(nx) if tx.channel(m.L1_XCCH, i)[2] in (m.L1_SACCH_TF, m.L1_SACCH_C8, m.L1_SACCH_C4)]

    def result(row, soft, amp, toa, valid):
        keep = (row, soft, amp, toa, valid)
        return m.TrxGroupResult(n_slots=T, n_arfcn=A, n_rows=soft.shape[0], d_row=row.data_ptr(), d_valid=valid.data_ptr(),
                                d_flags=None, d_amp=amp.data_ptr(), d_toa=toa.data_ptr(), d_avgpwr=None, d_threshold=None,
                                d_soft=soft.data_ptr(), soft_stride=soft.shape[1]), keep

    def uplink_noise():
        """a random uplink pull into the sibling: its RSSI / timing (and so the downlink's orders) move"""
        row = torch.arange(T * A, dtype=torch.int32, device="cuda").reshape(T, A)
        soft = torch.rand(T * A, 148, device="cuda", generator=gen)
        amp = torch.randn(T * A, 2, device="cuda", generator=gen) * 3000
        toa = torch.randn(T * A, device="cuda", generator=gen) * 40
        valid = torch.full((T * A,), m.F_DETECT, dtype=torch.uint8, device="cuda")
        return result(row, soft, amp, toa, valid)

    def grids(obj, fn, rach=False):
        g = obj.grid(fn, F)
        nt, nxc = obj.channels(m.L1_TCH), obj.channels(m.L1_XCCH)
        out = [dev(rng.choice(np.array([1, 1, 2], np.uint8), (nt, g[0]))), dev(rng.integers(0, 256, (nt, g[0], 33)).astype(np.uint8)),
               dev(np.ones((nxc, g[1]), np.uint8)), dev(rng.integers(0, 256, (nxc, g[1], 23)).astype(np.uint8))]
        if rach:
            out += [dev(np.ones(g[2], np.uint8)), dev(rng.integers(0, 256, g[2]).astype(np.uint8))]
        else:
            nc = obj.channels(m.L1_CCCH)
            out += [dev(np.ones((nc, g[2]), np.uint8)), dev(rng.integers(0, 256, (nc, g[2], 23)).astype(np.uint8))]
        return out

    def downlink_rows(o):
        """the encode's d_bits [A][T][148] as rows: slot (t, a) is row a * T + t where the slot is not empty"""
        from openbts_ttsou_amd.frontend import _DevView
        bits = torch.as_tensor(_DevView(o.d_bits, (A * T, 148), "|u1"), device="cuda:0")
        what = torch.as_tensor(_DevView(o.d_what, (A, T), "|u1"), device="cuda:0")
        soft = (0.1 + 0.8 * bits.float() + (torch.rand(A * T, 148, device="cuda", generator=gen) - 0.5) * 0.5).clamp_(0, 1)
        idx = (torch.arange(A, device="cuda", dtype=torch.int32)[None, :] * T + torch.arange(T, device="cuda", dtype=torch.int32)[:, None])
        row = torch.where(what.T != 0, idx, torch.full_like(idx, -1)).contiguous()
        amp = torch.full((A * T, 2), 2000.0, device="cuda")
        toa = torch.zeros(A * T, device="cuda")
        valid = torch.full((A * T,), m.F_DETECT, dtype=torch.uint8, device="cuda")
        return result(row, soft, amp, toa, valid)

    def windows(fa, fb):
        """the two calls timed in alternating windows of a.calls calls each: per-call microseconds (median, p10, p90) of both"""
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        ts = ([], [])
        for _ in range(a.reps):
            for k, fnc in enumerate((fa, fb)):
                ev[0].record()
                for _ in range(a.calls):
                    fnc()
                ev[1].record(); torch.cuda.synchronize()
                ts[k].append(ev[0].elapsed_time(ev[1]) * 1000.0 / a.calls)
        return [(float(np.median(t)), float(np.percentile(t, 10)), float(np.percentile(t, 90))) for t in ts]

    fn0 = 1326 * 3                                           # a 51- and 26-multiframe boundary
    sent, held, short_ok, timing = [], [], True, None
    for rnd in range(a.rounds):
        fn = fn0 + rnd * F
        res_ul, keep_ul = uplink_noise()
        ul.decode(res_ul, fn)
        o = tx.encode(fn, F, *grids(tx, fn), sibling=ul)
        t = tx.collect(state=False)
        sent.append([(level_power(band, int(t["ms_power"][i])), int(np.float32(t["ms_ta"][i] + np.float32(0.5)))) for i in sacch])
        g = grids(follower, fn, rach=True)
        shortcut.encode(fn, F, *g, sibling=tx)
        s = shortcut.collect(state=False)
        short_ok &= [(int(s["ms_power"][i]), int(s["ms_ta"][i])) for i in sacch] == sent[-1]
        follower.encode(fn, F, *g)                           # holds what was decoded before this round
        h = follower.collect(state=False)
        held.append([(int(h["ms_power"][i]), int(h["ms_ta"][i])) for i in sacch])
        res, keep = downlink_rows(o)
        rx.decode(res, fn)
        ctx.synchronize()
        if rnd == 1:                                         # time this round's rows on objects of their own
            for _ in range(3):
                rx_timed.decode(res, fn); ul_timed.decode(res, fn)
            torch.cuda.synchronize()
            timing = (*windows(lambda: rx_timed.decode(res, fn), lambda: ul_timed.decode(res, fn)),
                      dict(n_tch=rx_timed.out.n_tch, n_xcch=rx_timed.out.n_xcch, n_ccch=rx_timed.out.n_ccch, n_bcch=rx_timed.out.n_bcch,
                           nb_tch=rx_timed.out.nb_tch, nb_ctl=rx_timed.out.nb_ctl, sch_cap=rx_timed.out.sch_cap,
                           fcch_cap=rx_timed.out.fcch_cap, rows=int((keep[0] >= 0).sum()),
                           l1rx_nb_tch=ul_timed.out.nb_tch, l1rx_nb_xcch=ul_timed.out.nb_xcch))
    # how many rounds back the orders lie that the follower held in each round (from the third round on: the pipeline is full)
    lag = {}
    for rnd in range(2, a.rounds):
        for j in range(len(sacch)):
            back = next((d for d in range(1, rnd + 1) if sent[rnd - d][j] == held[rnd][j]), None)
            lag[str(back)] = lag.get(str(back), 0) + 1
    changed = sum(sent[r][j] != sent[r - 1][j] for r in range(1, a.rounds) for j in range(len(sacch)))
    (dec, dec10, dec90), (yard, yard10, yard90), shape = timing
    out = dict(arfcns=A, frames=F, rounds=a.rounds, reps=a.reps, calls_per_window=a.calls, sacch_channels=len(sacch), **shape,
               l1msrx_decode_us=round(dec, 1), l1msrx_decode_us_p10_p90=[round(dec10, 1), round(dec90, 1)],
               l1rx_decode_same_rows_us=round(yard, 1), l1rx_decode_us_p10_p90=[round(yard10, 1), round(yard90, 1)],
               orders_changed_between_rounds=int(changed), orders_total=(a.rounds - 1) * len(sacch),
               shortcut_rounds_behind=0 if short_ok else None,
               follower_rounds_behind_histogram=lag,
               note="rounds behind: the follower's handset in round r holds the orders the downlink sent in round r - d; 'None': the "
                    "orders of no earlier round (a channel not yet heard); the shortcut reads the multiplexer's records and is 0 behind")
    print(json.dumps(out))
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
