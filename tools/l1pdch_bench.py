"""Time the packet data channel object (include/trxsig_l1pdch.h) on 128 ARFCNs x 104 frames with every TN 1..7 a PDCH and every
block sent: ONE trxsig_l1pdch_encode (a DOWN object: PDTCH and PTCCH blocks, the USF ring) and ONE trxsig_l1pdch_decode (an UP
object, with the DOWN object as sibling), beside the composition a caller writes without the object -- trxsig_fec_pdtch_encode_batch
plus index_copy_ scatters into the grid; a torch-built d_index plus trxsig_fec_pdtch_decode_batch -- and beside the time one
read and one write of the bytes each call touches would take at the sustained HBM rate tools/hbm_bench.hip reports on the same
box (--hbm-bench: the compiled binary, run first in a process of its own; or --hbm-tbps).  The soft rows are the UP encoder's
bursts with noise (sigma 0.2, clipped to [0, 1]); medians of repeated HIP-event windows; the soft buffers rotate, together larger
than the memory-side cache.  Side measurements: nothing is asserted.  Results go to profiles/l1pdch_bench.json (or --out).

    hipcc --offload-arch=gfx950 -O3 tools/hbm_bench.hip -o hbm_bench
    python tools/l1pdch_bench.py --hbm-bench ./hbm_bench [--arfcns 128] [--frames 104] [--reps 30]"""
import numpy as np

import mlse_bench_lib as lib


def main():
    ap = lib.parser("l1pdch_bench.json")
    ap.add_argument("--arfcns", type=int, default=128)
    ap.add_argument("--frames", type=int, default=104)
    a, tbps, line = lib.parse(ap)

    import torch
    import _pkg
    import l1_pdch_model as lp
    m = _pkg.load()
    A, F, fn, bsic = a.arfcns, a.frames, 0, 0x15
    T = 8 * F
    comb = np.full((A, 8), m.L1PDCH_COMB, np.uint8)
    comb[:, 0] = 0
    ctx = m.TrxSig(4, 0)
    ctx.use_torch_stream()
    gen = torch.Generator(device="cuda"); gen.manual_seed(5)
    down, up = m.L1Pdch(ctx, comb, bsic, m.L1PDCH_DOWN), m.L1Pdch(ctx, comb, bsic, m.L1PDCH_UP)
    n = down.channels(m.L1PDCH_PDTCH)
    nb, nbt = down.grid(fn, F)
    rnd = lambda *shape, hi=256: torch.randint(0, hi, shape, device="cuda", generator=gen, dtype=torch.uint8)
    kind, cs, payload = torch.ones(n, nb, dtype=torch.uint8, device="cuda"), rnd(n, nb, hi=4), rnd(n, nb, 54)
    pt_kind, pt_payload = torch.ones(n, nbt, dtype=torch.uint8, device="cuda"), rnd(n, nbt, 23)
    enc = lambda k: down.encode(fn, F, kind, cs, payload, pt_kind, pt_payload)
    out = enc(0)
    torch.cuda.synchronize()
    # the uplink's bursts -> a pull: every written slot a row, all valid
    uo = up.encode(fn, F, kind, cs, payload)
    what = m._dev_tensor(ctx, uo.d_what, (A, T), "|u1").t().contiguous()            # [T][A]
    ubits = m._dev_tensor(ctx, uo.d_bits, (A, T, 148), "|u1").transpose(0, 1)[what != 0]
    n_rows = int(ubits.shape[0])
    row = torch.full((T, A), -1, dtype=torch.int32, device="cuda")
    row[what != 0] = torch.arange(n_rows, dtype=torch.int32, device="cuda")
    soft = (ubits.to(torch.float32) + 0.2 * torch.randn(n_rows, 148, device="cuda", generator=gen)).clamp_(0, 1).contiguous()
    valid = torch.full((n_rows,), m.F_DETECT, dtype=torch.uint8, device="cuda")
    amp = torch.full((n_rows, 2), 700.0, device="cuda"); toa = torch.zeros(n_rows, device="cuda")
    rot = lib.Rotation(a.reps, torch.view_as_complex(soft.view(-1, 2)))
    xs = rot.xs[0]
    results = [m.TrxGroupResult(n_slots=T, n_arfcn=A, n_rows=n_rows, d_row=row.data_ptr(), d_valid=valid.data_ptr(), d_flags=None,
                                d_amp=amp.data_ptr(), d_toa=toa.data_ptr(), d_avgpwr=None, d_threshold=None, d_soft=x.data_ptr(),
                                soft_stride=148) for x in xs]
    dec = lambda k: up.decode(results[k], fn, wire=True, sibling=down)

    # the composition a caller writes today.  Static: which grid slot each burst of each block goes to / comes from.
    chans = [up.channel(m.L1PDCH_PDTCH, i) for i in range(n)]
    bf, _ = lp.encode_blocks(lp.PDTCH, fn, F)
    slot = np.array([[[8 * (lp.frame_of(lp.PDTCH, 4 * (bf + b) + t) - fn) + tn + T * arf for t in range(4)] for b in range(nb)]
                     for arf, tn in chans], np.int64).reshape(-1)                   # into the [A][T] grid
    inside = slot < np.array([T * (arf + 1) for arf, tn in chans for b in range(nb) for t in range(4)])
    assert inside.all()                                       # 104 frames from 0: no block straddles the call's end
    d_slot = torch.from_numpy(slot).cuda()
    d_slot_ta = torch.from_numpy((slot % T) * A + slot // T).cuda()                   # into the pull's [T][A] row map
    tsc = torch.full((n * nb,), bsic & 7, dtype=torch.uint8, device="cuda")
    tmp = torch.zeros(n * nb, 4, 148, dtype=torch.uint8, device="cuda")
    grid, gwhat = torch.zeros(A * T, 148, dtype=torch.uint8, device="cuda"), torch.zeros(A * T, dtype=torch.uint8, device="cuda")
    eight = torch.full((n * nb * 4,), m.L1TX_PDCH, dtype=torch.uint8, device="cuda")

    def by_hand_enc(k):
        ctx.pdtch_encode(payload.view(-1, 54), cs.view(-1), tsc, tmp)
        grid.index_copy_(0, d_slot, tmp.view(-1, 148))
        gwhat.index_copy_(0, d_slot, eight)

    ob, ocs, odist, ook, ousf = (torch.zeros(n * nb, w, dtype=torch.uint8, device="cuda") for w in (54, 1, 1, 1, 1))

    def by_hand_dec(k):
        r = row.view(-1)[d_slot_ta]
        idx = torch.where((r >= 0) & (valid[r.clamp(min=0).long()] != 0), r, torch.full_like(r, -1))
        ctx.pdtch_decode(xs[k].data_ptr(), n * nb, ob, cs=ocs, cs_dist=odist, ok=ook, usf=ousf, index=idx, wire=True, n_rows=n_rows,
                         soft_stride=148)

    e_us, d_us, he_us, hd_us = rot.timed(enc, dec, by_hand_enc, by_hand_dec)
    dec(0)
    g = up.collect_decode()["pdtch"]
    by_hand_dec(0); by_hand_enc(0); enc(0)
    torch.cuda.synchronize()
    same = bool(np.array_equal(g["payload"].reshape(-1, 54), ob.cpu().numpy()) and np.array_equal(g["ok"].reshape(-1), ook.cpu().numpy()[:, 0]))
    pd = (m._dev_tensor(ctx, out.d_what, (A * T,), "|u1") != 0)
    grid_same = bool(torch.equal(m._dev_tensor(ctx, out.d_bits, (A * T, 148), "|u1")[d_slot], grid[d_slot])) and int(pd.sum()) > len(slot)
    n_bursts_down = int(pd.sum())
    enc_bytes = n * nb * 56 + n * nbt * 24 + n_bursts_down * 149 + A * T * 149          # inputs, the bursts, the zeroed grid
    dec_bytes = T * A * 4 + n_rows * (148 * 4 + 1) + n * nb * (54 + 7 + 4)
    floor = lambda b: b / (tbps * 1e12) * 1e6
    o = dict(arfcns=A, frames=F, pdch_slots=n, pdtch_blocks=n * nb, ptcch_blocks=n * nbt, bursts_down=n_bursts_down, bursts_up=n_rows,
             hbm_read_tbps=tbps, hbm_bench_line=line, sample_buffers_in_rotation=rot.n,
             **lib.us("l1pdch_encode", e_us), **lib.us("l1pdch_decode", d_us), **lib.us("by_hand_encode", he_us), **lib.us("by_hand_decode", hd_us),
             encode_over_by_hand=round(e_us[0] / he_us[0], 2), decode_over_by_hand=round(d_us[0] / hd_us[0], 2),
             encode_touched_bytes=enc_bytes, decode_touched_bytes=dec_bytes,
             one_pass_over_the_encode_bytes_us=round(floor(enc_bytes), 1), one_pass_over_the_decode_bytes_us=round(floor(dec_bytes), 1),
             encode_over_one_pass=round(e_us[0] / floor(enc_bytes), 1), decode_over_one_pass=round(d_us[0] / floor(dec_bytes), 1),
             blocks_ok=int(g["ok"].sum()), object_equals_by_hand=dict(decode=same, encode=grid_same),
             note="the object's encode also zeroes its own grid, sends the PTCCH blocks and keeps the USF ring and the pending bursts; "
                  "its decode also gathers the rows, counts bursts, writes closing FNs, grants, RSSI / timing and the carry.  The by-hand "
                  "encode scatters into a grid that is never cleared; the by-hand decode builds d_index with four torch kernels.  The "
                  "touched bytes are counted once each, read or written, at the read rate hbm_bench reports; medians of --reps "
                  "HIP-event windows, the soft rows read from a buffer not touched since the rotation came round")
    lib.write(o, a.out)
    down.destroy(); up.destroy()
    ctx.close()


if __name__ == "__main__":
    main()
