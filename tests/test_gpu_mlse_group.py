"""The Transceiver group on the sequence-equalising leg (TRXSIG_TSCLEG_MLSE): 3 ARFCNs x 16 slots at sps 4, a different training
sequence per ARFCN, one access-burst slot, the same samples into an MLSE group and a DEMOD group.  Everything but the
training-sequence rows' soft bits is identical between the two (rows, valid, flags, amplitude, TOA, avgPwr, thresholds, the
access-burst rows' soft bits); the training-sequence rows equal the model (tests/mlse_model.py) with the group's own amplitude
and TOA; trxsig_trxgroup_set_beside_rows(1) and set_pipelined give the same values.  Last, one closed loop: l1ms -> radiate ->
trxsig_air_cells with a fixed tap set of three symbols' spread -> pull -> l1rx on one SDCCH/8 slot (tests/mlse_loop.py)."""
import numpy as np
import pytest

import mlse_family
import mlse_model
import oraclebind
import synth
import transceiver_model as tm
from mlse_run import dev, dev_c, pkg  # noqa: F401  (the fixtures)
from util import assert_veq

pytestmark = pytest.mark.gpu

SPS, S, T, FN0 = 4, 3, 16, 101
TSCS = (2, 5, 7)
CELL = 160 * SPS


def combination(a, tn):
    return tm.IV if (a == 0 and tn == 0) else tm.I           # ARFCN 0's slot 0 hears access bursts


@pytest.fixture(scope="module")
def cells():
    """(x [T][S][CELL] complex64, ctype [T][S]): multipath and flat normal bursts with the ARFCN's training sequence, access bursts in
    ARFCN 0's slot 0, one silent cell and one cell of loud noise."""
    rng = np.random.default_rng(31)
    o = oraclebind.Oracle(SPS)
    x = np.zeros((T, S, CELL), np.complex64)
    ctype = np.zeros((T, S), np.int8)
    rx, roff, rlen, _ = synth.rach_batch(SPS, 8, seed=5, sigmas=(0.0, 0.1), max_delay_sym=10)
    m = tm.TransceiverModel.__new__(tm.TransceiverModel)
    profiles = ["five", "precursor", "flat"]
    for t in range(T):
        tn, fn = t % 8, FN0 + t // 8
        n = (156 + (tn % 4 == 0)) * SPS
        for a in range(S):
            m.chan_type = np.array([combination(a, k) for k in range(8)])
            ctype[t, a] = m.expected_corr_type(tn, fn)
            if ctype[t, a] == tm.RACH:
                i = 4 * (t // 8)                               # (bursts 0 and 4 of the pack are the 157-symbol ones)
                x[t, a, :n] = rx[roff[i]:roff[i] + rlen[i]][:n]
            elif (t, a) == (5, 1):
                pass                                           # silence
            elif (t, a) == (9, 2):
                x[t, a, :n] = (rng.standard_normal(n) + 1j * rng.standard_normal(n)) * 900.0
            else:
                bits = synth.normal_bits(rng, 1, TSCS[a])[0]
                s = o.modulate(bits.astype(np.int8), 9 if tn % 4 == 0 else 8)
                x[t, a, :n] = mlse_family.channel(rng, s, SPS, mlse_family.PROFILES[profiles[(t + a) % 3]], 18.0)[:n]
    assert (ctype == tm.RACH).sum() == 2 and (ctype == tm.TSC).sum() == T * S - 2
    return x, ctype


def run_group(pkg, x, leg, beside_rows=0, pipelined=False):
    import torch
    ctx = pkg.TrxSig(SPS, 0)
    ctx.use_torch_stream()
    g = pkg.TrxGroup(ctx, S, tsc_leg=leg, start=(FN0, 0))
    if beside_rows:
        g.set_beside_rows(beside_rows)
    if pipelined:
        g.set_pipelined(True)
    for a in range(S):
        for cmd in ["CMD RXTUNE 890000", "CMD TXTUNE 935000", "CMD SETTSC %d" % TSCS[a]] + \
                   ["CMD SETSLOT %d %d" % (tn, combination(a, tn)) for tn in range(8)] + ["CMD POWERON"]:
            g.control(a, cmd)
    dx = torch.from_numpy(x.view(np.float32).reshape(-1)).to("cuda:0")
    res = g.pull(dx, S * CELL, CELL, FN0, 0, T)
    g.sync()
    torch.cuda.synchronize()
    R = res.n_rows
    out = dict(row=pkg._to_host(ctx, res.d_row, (T, S), "<i4"), valid=pkg._to_host(ctx, res.d_valid, (R,), "|u1"),
               flags=pkg._to_host(ctx, res.d_flags, (R,), "|u1"), amp=pkg._to_host(ctx, res.d_amp, (R, 2), "<f4").view(np.complex64).ravel(),
               toa=pkg._to_host(ctx, res.d_toa, (R,), "<f4"), avgpwr=pkg._to_host(ctx, res.d_avgpwr, (R,), "<f4"),
               threshold=pkg._to_host(ctx, res.d_threshold, (R,), "<f8"), soft=pkg._to_host(ctx, res.d_soft, (R, res.soft_stride), "<f4"))
    out["collect"] = g.collect()
    g.close(); ctx.close()
    return out


@pytest.fixture(scope="module")
def pulls(pkg, cells):
    x, _ = cells
    return run_group(pkg, x, pkg.TSCLEG_MLSE), run_group(pkg, x, pkg.TSCLEG_DEMOD)


def test_group_differs_from_the_demodulating_leg_only_in_the_tsc_soft_bits(pkg, cells, pulls):
    x, ctype = cells
    eq, dm = pulls
    for k in ("row", "valid", "flags", "amp", "toa", "avgpwr", "threshold"):
        assert eq[k].tobytes() == dm[k].tobytes(), k
    for k in ("valid", "rssi", "timing", "threshold"):
        assert eq["collect"][k].tobytes() == dm["collect"][k].tobytes(), "collect " + k
    valid = eq["valid"] != 0
    rach_rows = eq["row"][ctype == tm.RACH]
    assert len(rach_rows) == 2 and valid[rach_rows].all()
    assert_veq(eq["soft"][rach_rows], dm["soft"][rach_rows], "access-burst rows' soft bits")
    tsc_rows = eq["row"][ctype == tm.TSC]
    assert valid[tsc_rows].sum() >= 36
    differ = sum(eq["soft"][r].tobytes() != dm["soft"][r].tobytes() for r in tsc_rows if valid[r])
    assert differ >= 30                                        # the equaliser did run on them


def test_group_tsc_rows_equal_the_model(pkg, cells, pulls):
    x, ctype = cells
    eq, _ = pulls
    o = oraclebind.Oracle(SPS)
    n_checked = 0
    for t in range(T):
        n = (156 + (t % 8 % 4 == 0)) * SPS
        for a in range(S):
            r = eq["row"][t, a]
            if ctype[t, a] != tm.TSC:
                continue
            assert r >= 0
            if not eq["valid"][r]:
                assert not eq["soft"][r].any()                 # (no side stream here: a row the machine did not accept is zeros)
                continue
            want = mlse_model.mlse_batch(SPS, x[t, a], np.array([0], np.int32), np.array([n], np.int32), TSCS[a], eq["amp"][r:r + 1],
                                         eq["toa"][r:r + 1], oracle=o)
            assert want["win"][0] <= 0
            assert_veq(eq["soft"][r, :148], want["soft"][0], "slot %d ARFCN %d" % (t, a))
            assert_veq(eq["collect"]["soft"][t, a], want["soft"][0], "collect: slot %d ARFCN %d" % (t, a))
            n_checked += 1
    assert n_checked >= 36


@pytest.mark.parametrize("pipelined", [False, True])
def test_group_beside_rows(pkg, cells, pulls, pipelined):
    """The state machine on the side stream (every pull, and with the join left to sync): the same values where d_valid is set."""
    x, _ = cells
    eq, _ = pulls
    b = run_group(pkg, x, pkg.TSCLEG_MLSE, beside_rows=1, pipelined=pipelined)
    for k in ("row", "valid", "flags", "amp", "toa", "avgpwr", "threshold"):
        assert b[k].tobytes() == eq[k].tobytes(), k
    v = eq["valid"] != 0
    assert b["soft"][v].tobytes() == eq["soft"][v].tobytes()
    assert b["collect"]["soft"].tobytes() == eq["collect"]["soft"].tobytes()


def test_group_leg_rules(pkg):
    """The leg is accepted at any sps; the one-burst Transceiver object keeps refusing it."""
    for sps in (1, 2, 4):
        ctx = pkg.TrxSig(sps, 0)
        g = pkg.TrxGroup(ctx, 2, tsc_leg=pkg.TSCLEG_MLSE)
        g.set_pipelined(True)
        g.close()
        with pytest.raises(pkg.TrxSigError):
            pkg.TrxGroup(ctx, 2, tsc_leg=3)
        ctx.close()
    t = pkg.TrxHost(4, 0)
    assert t.L.trxsig_trx_set_tsc_leg(t.h, pkg.TSCLEG_MLSE) < 0
    t.close()


# ---- the closed loop: l1ms -> radiate -> trxsig_air_cells with a fixed tap set -> pull -> l1rx, one SDCCH/8 slot ----
def test_closed_loop_through_three_symbols_of_spread(pkg):
    """L1Ms.encode -> radiate -> Air.cells with tests/mlse_loop.py's fixed taps (three symbols of spread at sps 4, no noise) ->
    TrxGroup.pull -> L1Rx.decode on one SDCCH/8 slot: 16 channels, 24 blocks, 96 bursts.  The tap set was chosen on the CPU through
    air_model, the oracle, the equaliser's model and the FEC oracle: there every burst is detected, the modelled equalising chain
    decodes 24 of 24 blocks and the modelled demodulating chain 4 of 24 (asserted again here, on the CPU model of the cells).  On
    the GPU the equalising leg's blocks all decode with the payloads sent, its soft rows equal the model's on the cells the
    device made, and the demodulating leg loses at least one block."""
    import torch
    import fectxbind
    import fec_stream_model as fsm
    import mlse_loop as ml
    o = oraclebind.Oracle(ml.SPS)
    c = ml.case(fectxbind.FecTxOracle())
    cpu = ml.cpu_chains(o, c, ml.cpu_cells(o, c))
    blk = cpu["blocks"]
    assert len(blk) == 24 and cpu["detected"].all() and cpu["ok_mlse"].all() and (~cpu["ok_demod"]).sum() >= 1
    assert cpu["ok_demod"].sum() == 4
    sps, A, F, fn0, comb, m = ml.SPS, ml.A, ml.F, ml.FN0, c["comb"], c["m"]
    T, cell = 8 * F, 160 * sps
    ctx = pkg.TrxSig(sps, 0)
    ctx.use_torch_stream()
    ms = pkg.L1Ms(ctx, comb, ml.BSIC, ml.BAND)
    ms.encode(fn0, F, **{k: dev(v) for k, v in c["grids"].items()})
    r = ms.collect(state=False)
    assert np.array_equal(r["what"], m["what"]) and np.array_equal(r["bits"], m["bits"])
    nx = len(c["model"].ch[ml.lms.XCCH])
    clean = torch.zeros(T, A, cell, 2, dtype=torch.float32, device="cuda")
    none_c, none_f = dev_c(np.zeros(0, np.complex64)), dev(np.zeros(0, np.float32))
    ms.radiate(clean, A * cell, cell, tch_gain=none_c, tch_delay=none_f, xcch_gain=dev_c(np.full(nx, ml.GAIN, np.complex64)),
               xcch_delay=dev(np.zeros(nx, np.float32)), rach_gain=none_c, rach_delay=none_f, amp_of_power=dev(np.ones(41, np.float32)))
    h = ml.taps()
    air = pkg.Air(ctx, len(h))
    rxbuf = torch.zeros_like(clean)
    air.cells(fn0, A, F, 1, clean, A * cell, cell, rxbuf, A * cell, cell, taps=dev_c(np.broadcast_to(h, (A, T, len(h)))))
    cells = rxbuf.cpu().numpy().view(np.complex64).reshape(T, A, cell)
    out = {}
    for leg in (pkg.TSCLEG_MLSE, pkg.TSCLEG_DEMOD):
        grp = pkg.TrxGroup(ctx, A, tsc_leg=leg, start=(fn0, 0))
        for cmd in ["CMD RXTUNE 890000", "CMD TXTUNE 935000", "CMD SETTSC %d" % (ml.BSIC & 7)] + \
                   ["CMD SETSLOT %d %d" % (tn, comb[0, tn]) for tn in range(8)] + ["CMD POWERON"]:
            grp.control(0, cmd)
        res = grp.pull(rxbuf, A * cell, cell, fn0, 0, T)
        grp.sync()
        rx = pkg.L1Rx(ctx, comb, ml.BSIC, ml.BAND)
        rx.decode(res, fn0)
        got = rx.collect()
        torch.cuda.synchronize()
        R = res.n_rows
        out[leg] = dict(got=got, col=grp.collect(), row=pkg._to_host(ctx, res.d_row, (T, A), "<i4"),
                        amp=pkg._to_host(ctx, res.d_amp, (R, 2), "<f4").view(np.complex64).ravel(), toa=pkg._to_host(ctx, res.d_toa, (R,), "<f4"))
        rx.destroy(); grp.close()

    def decoded(got):
        ok = []
        for i, b, want, slots in blk:
            jb = list(got["xcch_fn"][i]).index((fn0 + slots[3] // 8) % tm.HYPERFRAME)
            ok.append(got["xcch_status"][i, jb] == fsm.DECODED | fsm.TCH_GOOD and np.array_equal(got["xcch"][i, jb], want))
        return np.array(ok)
    eq = out[pkg.TSCLEG_MLSE]
    assert all(eq["col"]["valid"][s, 0] for _, _, _, slots in blk for s in slots), "a burst was not detected"
    assert decoded(eq["got"]).all(), "the equalising leg lost a block"
    assert (~decoded(out[pkg.TSCLEG_DEMOD]["got"])).sum() >= 1, "the demodulating leg lost nothing: the tap set proves nothing"
    # the soft rows: the model on the cells the device made, with the group's amplitude and TOA
    n = 0
    for _, _, _, slots in blk:
        for s in slots:
            x = cells[s, 0, :(156 + (s % 4 == 0)) * sps]
            row = eq["row"][s, 0]
            want = mlse_model.mlse_batch(sps, x, np.array([0], np.int32), np.array([len(x)], np.int32), ml.BSIC & 7, eq["amp"][row:row + 1],
                                         eq["toa"][row:row + 1], oracle=o)
            assert want["win"][0] <= 0
            assert_veq(eq["col"]["soft"][s, 0], want["soft"][0], "slot %d" % s)
            n += 1
    assert n == 96
    ms.destroy(); air.destroy(); ctx.close()
