"""Side measurement, the hop between the downlink multiplexer and the Transceiver group's transmit queues: the production plan
(128 ARFCNs; C0: combination V on TN 0, VII on TN 1, I elsewhere; I on every other carrier), 32 frames a step, the loop

    trxsig_l1tx_encode -> hand-off -> trxsig_trxgroup_push_txbe -> trxsig_txbe_pop_samples

with the hand-off done (host) by trxsig_l1tx_datagrams + trxsig_trxgroup_add_bursts into preallocated host arrays, or (device) by
trxsig_trxgroup_add_l1tx.  A step's time is the wall clock over a window of --steps steps with ONE device synchronise at the
window's end, divided by the steps; windows of the two routes alternate in one process on one multiplexer, group and back end
(--reps windows each, after warm-up windows of both), and the medians are reported with each route's spread.

    python tools/l1tx_handoff_bench.py [--arfcns 128] [--frames 32] [--steps 50] [--reps 7] [--out profiles/l1tx_handoff_bench.json]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/l1tx_handoff_bench.py --reps 1 --out ""     (the kernel trace: a run of its own)"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def main():
    import torch
    import _pkg
    ap = argparse.ArgumentParser()
    ap.add_argument("--arfcns", type=int, default=128)
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "l1tx_handoff_bench.json"))
    a = ap.parse_args()
    m = _pkg.load()
    from openbts_ttsou_amd import synth
    from openbts_ttsou_amd.frontend import TxBackEnd
    assert torch.cuda.is_available(), "this measurement needs the MI355X"
    ctx = m.TrxSig(4, 0)
    ctx.use_torch_stream()
    L = ctx.L
    rng = np.random.default_rng(1)
    A, F = a.arfcns, a.frames
    comb = np.ones((A, 8), np.uint8)
    comb[0, 0], comb[0, 1] = 5, 7
    l1 = m.L1Tx(ctx, comb, 33)
    l1.set_si(rng.integers(0, 256, (4, 23)).astype(np.uint8))
    grp = m.TrxGroup(ctx, A, tsc_leg=m.TSCLEG_DEMOD)
    be = TxBackEnd(ctx, A, synth.design_lpf(651, 96), max_bursts=8 * F)
    nt, nx, nc = l1.channels(m.L1_TCH), l1.channels(m.L1_XCCH), l1.channels(m.L1_CCCH)
    # the payload grids of any step are views of one random pool per array (a step's grid sizes depend on its first frame)
    nb_max = F // 4 + 3
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    pool_tk = dev(rng.choice(np.array([0, 1, 1, 2], np.uint8), nt * nb_max))
    pool_tp = dev(rng.integers(0, 256, nt * nb_max * 33).astype(np.uint8))
    pool_1 = dev(np.ones(max(nx, nc) * nb_max, np.uint8))
    pool_p = dev(rng.integers(0, 256, max(nx, nc) * nb_max * 23).astype(np.uint8))
    cap = A * 8 * F
    h_dg = np.zeros((cap, 154), np.uint8)
    h_ar = np.zeros(cap, np.int32)
    n_dg = C.c_int()
    state = dict(fn=1326 * 3, bursts=0)

    def step(device_route):
        fn = state["fn"]
        nbt, nbx, nbc = l1.grid(fn, F)
        assert max(nbt, nbx, nbc) <= nb_max
        l1.encode(fn, F, pool_tk[:nt * nbt].view(nt, nbt), pool_tp[:nt * nbt * 33].view(nt, nbt, 33),
                  pool_1[:nx * nbx].view(nx, nbx), pool_p[:nx * nbx * 23].view(nx, nbx, 23),
                  pool_1[:nc * nbc].view(nc, nbc), pool_p[:nc * nbc * 23].view(nc, nbc, 23))
        if device_route:
            grp.add_l1tx(l1)
        else:
            rc = L.trxsig_l1tx_datagrams(l1.h, h_dg.ctypes.data, h_ar.ctypes.data, cap, C.byref(n_dg))
            assert rc == 0, rc
            rc = L.trxsig_trxgroup_add_bursts(grp.h, h_dg.ctypes.data, h_ar.ctypes.data, n_dg.value)
            assert rc == 0, rc
            state["bursts"] = n_dg.value
        grp.push_txbe(be, fn, 0, 8 * F)
        iq = be.pop_samples()
        state["fn"] = (fn + F) % 2715648
        return iq

    def window(device_route, steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            step(device_route)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / steps * 1e6

    for route in (False, True, False, True):                 # warm-up: every shape, every staging set, both routes
        window(route, 10)
    t = {False: [], True: []}
    for _ in range(a.reps):
        for route in (False, True):
            t[route].append(window(route, a.steps))
    dropped = [grp.tx_queue_size(x) for x in (0, 1, A - 1)]
    host, devc = float(np.median(t[False])), float(np.median(t[True]))
    res = dict(arfcns=A, frames_per_step=F, bursts_per_step=state["bursts"], steps_per_window=a.steps, windows_per_route=a.reps,
               host_route="trxsig_l1tx_datagrams + trxsig_trxgroup_add_bursts (preallocated pageable arrays)",
               device_route="trxsig_trxgroup_add_l1tx",
               host_us_per_step=round(host, 1), device_us_per_step=round(devc, 1), host_over_device=round(host / devc, 2),
               host_us_min_max=[round(min(t[False]), 1), round(max(t[False]), 1)],
               device_us_min_max=[round(min(t[True]), 1), round(max(t[True]), 1)],
               device_mbursts_per_s=round(state["bursts"] / devc, 1),
               loop="encode -> hand-off -> push_txbe -> pop_samples; wall clock per window, one synchronise at its end",
               queues_left_and_dropped=dropped)
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
