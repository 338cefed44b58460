"""What the GPU tests of the two combine calls share (tests/test_gpu_mlse_div_group.py: trxsig_trxgroup_combine_div,
test_gpu_mlse_irc_group.py: trxsig_trxgroup_combine_irc): two Transceiver groups, one per receive antenna, of 2 ARFCNs x 16 slots at
sps 4 with a training sequence per ARFCN and one access-burst slot -- the slot combinations, the received cells, the groups, a
result's arrays on the host and the canaried optional outputs."""
import numpy as np

import mlse_family
import mlse_run
import oraclebind
import synth
import transceiver_model as tm

SPS, S, T, FN0 = 4, 2, 16, 101
TSCS = (2, 5)
CELL = 160 * SPS
PROFILES = [mlse_family.PROFILES[k] for k in ("five", "precursor", "flat")]      # what the cells' channels cycle through


def combination(a, tn):
    return tm.IV if (a == 0 and tn == 0) else tm.I           # ARFCN 0's slot 0 hears access bursts


def make_cells(seed, received, silent0, silent1, loud1=()):
    """(x [2 antennas][T][S][CELL] complex64, ctype [T][S]).  received(rng, o, s, t, a, n): the two antennas' samples of a normal
    burst's modulated s in cell (t, a); silent0 / silent1: the cells where that antenna hears nothing; loud1: where antenna 1 is
    the louder."""
    rng = np.random.default_rng(seed)
    o = oraclebind.Oracle(SPS)
    x = np.zeros((2, T, S, CELL), np.complex64)
    ctype = np.zeros((T, S), np.int8)
    rx, roff, rlen, _ = synth.rach_batch(SPS, 8, seed=5, sigmas=(0.0, 0.1), max_delay_sym=10)
    m = tm.TransceiverModel.__new__(tm.TransceiverModel)
    for t in range(T):
        tn, fn = t % 8, FN0 + t // 8
        n = (156 + (tn % 4 == 0)) * SPS
        for a in range(S):
            m.chan_type = np.array([combination(a, k) for k in range(8)])
            ctype[t, a] = m.expected_corr_type(tn, fn)
            if ctype[t, a] == tm.RACH:
                i = 4 * (t // 8)                               # (bursts 0 and 4 of the pack are the 157-symbol ones)
                r = rx[roff[i]:roff[i] + rlen[i]][:n]
                x[0, t, a, :n] = r
                x[1, t, a, :n] = r * np.complex64((1.5 if t == 0 else 0.5) * np.exp(0.7j))     # the louder antenna: 1 at t = 0, 0 at t = 8
                continue
            bits = synth.normal_bits(rng, 1, TSCS[a])[0]
            s = o.modulate(bits.astype(np.int8), 9 if tn % 4 == 0 else 8)
            x[0, t, a, :n], x[1, t, a, :n] = received(rng, o, s, t, a, n)
            if (t, a) in loud1:
                x[1, t, a] *= np.float32(2.5)
            if (t, a) in silent0:
                x[0, t, a] = 0
            if (t, a) in silent1:
                x[1, t, a] = 0
    assert (ctype == tm.RACH).sum() == 2 and (ctype == tm.TSC).sum() == T * S - 2
    return x, ctype


def make_group(pkg, ctx, leg, tscs=TSCS, n_arfcn=S, comb=combination):
    g = pkg.TrxGroup(ctx, n_arfcn, tsc_leg=leg, start=(FN0, 0))
    for a in range(n_arfcn):
        for cmd in ["CMD RXTUNE 890000", "CMD TXTUNE 935000", "CMD SETTSC %d" % tscs[a]] + \
                   ["CMD SETSLOT %d %d" % (tn, comb(a, tn)) for tn in range(8)] + ["CMD POWERON"]:
            g.control(a, cmd)
    return g


def fetch(pkg, ctx, res):
    R = res.n_rows
    return dict(row=pkg._to_host(ctx, res.d_row, (T, S), "<i4"), valid=pkg._to_host(ctx, res.d_valid, (R,), "|u1"),
                flags=pkg._to_host(ctx, res.d_flags, (R,), "|u1"), amp=pkg._to_host(ctx, res.d_amp, (R, 2), "<f4").view(np.complex64).ravel(),
                toa=pkg._to_host(ctx, res.d_toa, (R,), "<f4"), avgpwr=pkg._to_host(ctx, res.d_avgpwr, (R,), "<f4"),
                threshold=pkg._to_host(ctx, res.d_threshold, (R,), "<f8"), soft=pkg._to_host(ctx, res.d_soft, (R, res.soft_stride), "<f4"))


def to_dev(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x).view(np.float32).reshape(-1)).to("cuda:0")


def aux(R):
    """The canaried optional outputs of a combine call: sel of 9, taps of -7, window of -99."""
    import torch
    return dict(mlse_run.canaries(R, (2, 5)), sel=torch.full((R,), 9, dtype=torch.uint8, device="cuda:0"))


def aux_host(a, R):
    return dict(mlse_run.fetched(a, R), sel=a["sel"].cpu().numpy())
