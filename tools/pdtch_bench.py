"""Time the GPRS packet data block coders on 16,384 blocks per coding scheme, and on a mix of the four:
trxsig_fec_pdtch_decode_batch and trxsig_fec_pdtch_encode_batch (include/trxsig.h) beside trxsig_fec_xcch_decode_batch and
trxsig_fec_xcch_encode_batch on the same number of blocks in the same run, the decoders beside the time ONE read of the blocks'
soft rows would take at the sustained HBM rate tools/hbm_bench.hip reports on the same box (--hbm-bench: the compiled binary,
run first in a process of its own; or --hbm-tbps: a figure measured elsewhere).  The soft rows are the encoder's own bursts with
noise (sigma 0.2, clipped to [0, 1]); medians of repeated HIP-event windows; the soft buffers rotate, together larger than the
memory-side cache, so that every timed decode reads its rows from HBM.  By step count CS-2 / CS-3 would take 294/228 and 338/228
of CS-1's time.  Side measurements: nothing is asserted.  Results go to profiles/pdtch_bench.json (or --out) and to stdout.

    hipcc --offload-arch=gfx950 -O3 tools/hbm_bench.hip -o hbm_bench
    python tools/pdtch_bench.py --hbm-bench ./hbm_bench [--blocks 16384] [--reps 30] [--out profiles/pdtch_bench.json]"""
import numpy as np

import mlse_bench_lib as lib


def main():
    ap = lib.parser("pdtch_bench.json")
    ap.add_argument("--blocks", type=int, default=16384)
    a, tbps, line = lib.parse(ap)

    import torch
    import _pkg
    m = _pkg.load()
    n = a.blocks
    ctx = m.TrxSig(4, 0)
    ctx.use_torch_stream()
    gen = torch.Generator(device="cuda"); gen.manual_seed(5)
    u8 = lambda *shape: torch.zeros(*shape, dtype=torch.uint8, device="cuda")
    payload = torch.randint(0, 256, (n, m.PDTCH_BLOCK_BYTES), device="cuda", generator=gen, dtype=torch.uint8)
    tsc = torch.randint(0, 8, (n,), device="cuda", generator=gen, dtype=torch.uint8)
    bits, out = u8(n, 4, 148), u8(n, m.PDTCH_BLOCK_BYTES)
    ocs, dist, ok, usf = u8(n), u8(n), u8(n), u8(n)
    frames, xok = u8(n, 23), u8(n)
    soft_bytes = n * 4 * 148 * 4
    floor = soft_bytes / (tbps * 1e12) * 1e6
    res = {}
    schemes = [("cs%d" % (s + 1), torch.full((n,), s, dtype=torch.uint8, device="cuda")) for s in range(4)]
    schemes.append(("mixed", torch.randint(0, 4, (n,), device="cuda", generator=gen, dtype=torch.uint8)))
    for name, cs in schemes:
        ctx.pdtch_encode(payload, cs, tsc, bits)
        soft = (bits.view(4 * n, 148).to(torch.float32) + 0.2 * torch.randn(4 * n, 148, device="cuda", generator=gen)).clamp_(0, 1)
        rot = lib.Rotation(a.reps, torch.view_as_complex(soft.view(-1, 2)))      # (a float pair counted as one element: the bytes agree)
        assert rot.sample_bytes == soft_bytes
        xs = rot.xs[0]
        dec = lambda k: ctx.pdtch_decode(xs[k].data_ptr(), n, out, cs=ocs, cs_dist=dist, ok=ok, usf=usf, wire=True, n_rows=4 * n,
                                         soft_stride=148)
        xdec = lambda k: ctx.fec_xcch_decode(xs[k].data_ptr(), n, frames, xok, wire=True, soft_stride=148)
        enc = lambda k: ctx.pdtch_encode(payload, cs, tsc, bits)
        xenc = lambda k: ctx.fec_xcch_encode(payload, n, 2, bits)               # (reads the first 23 octets of a 54-octet row: a timing, not a frame)
        d_us, xd_us, e_us, xe_us = rot.timed(dec, xdec, enc, xenc)
        dec(0)
        torch.cuda.synchronize()
        res[name] = dict(**lib.us("pdtch_decode", d_us), **lib.us("xcch_decode", xd_us), **lib.us("pdtch_encode", e_us),
                         **lib.us("xcch_encode", xe_us), decode_over_xcch=round(d_us[0] / xd_us[0], 2),
                         encode_over_xcch=round(e_us[0] / xe_us[0], 2), decode_over_one_read=round(d_us[0] / floor, 2),
                         decode_ns_per_block=round(d_us[0] * 1e3 / n, 2), blocks_ok=int(ok.sum()),
                         schemes_detected_right=int((ocs == cs).sum()), sample_buffers_in_rotation=rot.n)
        del rot, xs, soft
    ratio = lambda k: round(res[k]["pdtch_decode_us"] / res["cs1"]["pdtch_decode_us"], 2)
    o = dict(blocks=n, soft_bytes=soft_bytes, hbm_read_tbps=tbps, hbm_bench_line=line, one_read_of_the_soft_rows_us=round(floor, 1),
             **res, decode_over_cs1=dict(cs2=ratio("cs2"), cs3=ratio("cs3"), cs4=ratio("cs4"), mixed=ratio("mixed")),
             decode_over_cs1_by_step_count=dict(cs2=round(294 / 228, 2), cs3=round(338 / 228, 2)),
             note="16,384 blocks = 65,536 bursts a call; soft rows = the encoder's bursts plus noise of sigma 0.2, clipped to [0, 1], "
                  "wire_quantise on, the scheme read from the stealing flags; the XCCH calls run on the same rows (for CS-2..4 they decode "
                  "to bad frames: a timing, the work does not depend on the values); medians of --reps HIP-event windows, the rows read "
                  "from a buffer not touched since the rotation came round; the encoders' inputs (0.9 MB) stay cached")
    lib.write(o, a.out)
    ctx.close()


if __name__ == "__main__":
    main()
