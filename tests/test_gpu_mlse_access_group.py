"""The Transceiver group with the access-burst sequence equaliser (trxsig_trxgroup_set_rach_leg): 3 ARFCNs x 16 slots, three slots
that hear access bursts (six access-burst rows: flat and multipath, delays of 0 to 12 symbols), the same samples into groups with
and without the setter.  The default leg is byte-identical to a group the setter was never called on; with TRXSIG_RACHLEG_MLSE
everything but the access-burst rows' soft bits is identical to the default, and those rows equal the model
(tests/mlse_access_model.py) with the group's own amplitude and TOA -- on the demodulating and the sequence-equalising tsc leg at
sps 4 and on the reference's equalising leg at sps 1; set_beside_rows(1) and set_pipelined give the same values; pull_rxfe equals
push + pop + pull_bursts.  Last, one closed loop: l1ms -> radiate -> trxsig_air_cells with a fixed tap set of three symbols'
spread -> pull -> l1rx on one combination-V slot (tests/mlse_access_loop.py)."""
import numpy as np
import pytest

import mlse_access_family as family
import mlse_access_model as model
import mlse_family
import oraclebind
import synth
import transceiver_model as tm
from mlse_run import dev, dev_c, pkg  # noqa: F401  (the fixtures)
from util import assert_veq

pytestmark = pytest.mark.gpu

S, T, FN0 = 3, 16, 101
TSCS = (2, 5, 7)
ACCESS_SLOTS = {(0, 0), (0, 3), (1, 4)}                       # (ARFCN, TN) on combination IV: every frame's burst is an access burst
KEYS = ("row", "valid", "flags", "amp", "toa", "avgpwr", "threshold")


def combination(a, tn):
    return tm.IV if (a, tn) in ACCESS_SLOTS else tm.I


def make_cells(sps):
    """(x [T][S][160 sps] complex64, ctype [T][S]): normal bursts with the ARFCN's training sequence (flat and multipath, 18 dB), six
    access bursts on the access slots (flat, clean and at 18 dB; `precursor` and `five` at 18 dB; delays 0, 3, 9, 5, 12, 7 symbols:
    pullRadioVector's energy gate looks at the first 20 symbols of the slot, a later burst is never handed up), one silent cell."""
    rng = np.random.default_rng(76 + sps)                     # (a seed with five of the six access bursts detected at either rate)
    o = oraclebind.Oracle(sps)
    x = np.zeros((T, S, 160 * sps), np.complex64)
    ctype = np.zeros((T, S), np.int8)
    abits, _, _ = family.access_bits(rng, 6)
    akind = [("flat", None, 0), ("precursor", 18.0, 3), ("precursor", 18.0, 9), ("five", 18.0, 5), ("flat", 18.0, 12), ("precursor", 18.0, 7)]
    m = tm.TransceiverModel.__new__(tm.TransceiverModel)
    profiles = ["five", "precursor", "flat"]
    k = 0
    for t in range(T):
        tn, fn = t % 8, FN0 + t // 8
        n = (156 + (tn % 4 == 0)) * sps
        for a in range(S):
            m.chan_type = np.array([combination(a, q) for q in range(8)])
            ctype[t, a] = m.expected_corr_type(tn, fn)
            if ctype[t, a] == tm.RACH:
                prof, snr, delay = akind[k]
                x[t, a, :n] = family.received(rng, o, abits[k], sps, prof, snr, delay, 157)[:n]
                k += 1
            elif (t, a) == (5, 2):
                pass                                           # silence
            else:
                bits = synth.normal_bits(rng, 1, TSCS[a])[0]
                s = o.modulate(bits.astype(np.int8), 9 if tn % 4 == 0 else 8)
                x[t, a, :n] = mlse_family.channel(rng, s, sps, mlse_family.PROFILES[profiles[(t + a) % 3] if sps > 1 else "flat"], 18.0)[:n]
    assert k == 6 and (ctype == tm.RACH).sum() == 6 and (ctype == tm.TSC).sum() == T * S - 6
    return x, ctype


@pytest.fixture(scope="module")
def cells():
    return {sps: make_cells(sps) for sps in (1, 4)}


def configure(g, pkg):
    for a in range(S):
        for cmd in ["CMD RXTUNE 890000", "CMD TXTUNE 935000", "CMD SETTSC %d" % TSCS[a]] + \
                   ["CMD SETSLOT %d %d" % (tn, combination(a, tn)) for tn in range(8)] + ["CMD POWERON"]:
            g.control(a, cmd)


def result(pkg, ctx, g, res, n_slots):
    import torch
    g.sync()
    torch.cuda.synchronize()
    R = res.n_rows
    out = dict(row=pkg._to_host(ctx, res.d_row, (n_slots, S), "<i4"), valid=pkg._to_host(ctx, res.d_valid, (R,), "|u1"),
               flags=pkg._to_host(ctx, res.d_flags, (R,), "|u1"), amp=pkg._to_host(ctx, res.d_amp, (R, 2), "<f4").view(np.complex64).ravel(),
               toa=pkg._to_host(ctx, res.d_toa, (R,), "<f4"), avgpwr=pkg._to_host(ctx, res.d_avgpwr, (R,), "<f4"),
               threshold=pkg._to_host(ctx, res.d_threshold, (R,), "<f8"), soft=pkg._to_host(ctx, res.d_soft, (R, res.soft_stride), "<f4"))
    out["collect"] = g.collect()
    return out


def run_group(pkg, sps, x, leg, rach_leg=None, beside_rows=0, pipelined=False):
    import torch
    ctx = pkg.TrxSig(sps, 0)
    ctx.use_torch_stream()
    g = pkg.TrxGroup(ctx, S, tsc_leg=leg, start=(FN0, 0))
    if rach_leg is not None:
        g.set_rach_leg(rach_leg)
    if beside_rows:
        g.set_beside_rows(beside_rows)
    if pipelined:
        g.set_pipelined(True)
    configure(g, pkg)
    cell = 160 * sps
    dx = torch.from_numpy(x.view(np.float32).reshape(-1)).to("cuda:0")
    out = result(pkg, ctx, g, g.pull(dx, S * cell, cell, FN0, 0, T), T)
    g.close(); ctx.close()
    return out


CONFIGS = {"demod-4": (4, "TSCLEG_DEMOD"), "mlse-4": (4, "TSCLEG_MLSE"), "equalize-1": (1, "TSCLEG_EQUALIZE")}


@pytest.fixture(scope="module")
def pulls(pkg, cells):
    """{config: (never set, set to the default, set to TRXSIG_RACHLEG_MLSE)}"""
    out = {}
    for name, (sps, leg) in CONFIGS.items():
        x = cells[sps][0]
        out[name] = tuple(run_group(pkg, sps, x, getattr(pkg, leg), rach_leg=r) for r in (None, pkg.RACHLEG_DEMOD, pkg.RACHLEG_MLSE))
    return out


@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_default_leg_changes_nothing(pulls, name):
    never, default, _ = pulls[name]
    for k in KEYS + ("soft",):
        assert never[k].tobytes() == default[k].tobytes(), k
    for k in ("valid", "soft", "rssi", "timing", "threshold"):
        assert never["collect"][k].tobytes() == default["collect"][k].tobytes(), "collect " + k


@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_mlse_leg_changes_only_the_access_rows_and_they_equal_the_model(pkg, cells, pulls, name):
    sps = CONFIGS[name][0]
    x, ctype = cells[sps]
    _, dm, eq = pulls[name]
    for k in KEYS:
        assert eq[k].tobytes() == dm[k].tobytes(), k
    for k in ("valid", "rssi", "timing", "threshold"):
        assert eq["collect"][k].tobytes() == dm["collect"][k].tobytes(), "collect " + k
    tsc_rows = eq["row"][ctype == tm.TSC]
    assert (tsc_rows >= 0).all() and (eq["valid"][tsc_rows] != 0).sum() >= 30
    assert eq["soft"][tsc_rows].tobytes() == dm["soft"][tsc_rows].tobytes(), "a training-sequence row changed"
    o = oraclebind.Oracle(sps)
    n_checked = n_differ = 0
    for t, a in np.argwhere(ctype == tm.RACH):
        r = eq["row"][t, a]
        assert r >= 0
        if not eq["valid"][r]:
            assert not eq["soft"][r].any()                     # (no side stream here: a row the machine did not accept is zeros)
            continue
        n = (156 + (t % 8 % 4 == 0)) * sps
        want = model.access_batch(sps, x[t, a], np.array([0], np.int32), np.array([n], np.int32), eq["amp"][r:r + 1], eq["toa"][r:r + 1], oracle=o)
        assert want["win"][0] <= 0
        assert_veq(eq["soft"][r, :148], want["soft"][0], "slot %d ARFCN %d" % (t, a))
        assert_veq(eq["collect"]["soft"][t, a], want["soft"][0], "collect: slot %d ARFCN %d" % (t, a))
        n_checked += 1
        n_differ += eq["soft"][r].tobytes() != dm["soft"][r].tobytes()
    assert n_checked >= 4 and n_differ >= 4, (n_checked, n_differ)


@pytest.mark.parametrize("pipelined", [False, True])
@pytest.mark.parametrize("name", ["demod-4", "mlse-4"])
def test_beside_rows_and_pipelined(pkg, cells, pulls, name, pipelined):
    """The state machine on the side stream (every pull, and with the join left to sync): the same values where d_valid is set."""
    sps, leg = CONFIGS[name]
    eq = pulls[name][2]
    b = run_group(pkg, sps, cells[sps][0], getattr(pkg, leg), rach_leg=pkg.RACHLEG_MLSE, beside_rows=1, pipelined=pipelined)
    for k in KEYS:
        assert b[k].tobytes() == eq[k].tobytes(), k
    v = eq["valid"] != 0
    assert b["soft"][v].tobytes() == eq["soft"][v].tobytes()
    assert b["collect"]["soft"].tobytes() == eq["collect"]["soft"].tobytes()


def test_pull_rxfe_takes_the_push_pop_route(pkg, cells):
    """The 16 slots as int16 streams at the radio's rate into trxsig_trxgroup_pull_rxfe on a group with TRXSIG_RACHLEG_MLSE (sps 4,
    the demodulating tsc leg: the configuration that would otherwise take the fused source): every collected output equals
    push + pop + trxsig_trxgroup_pull_bursts on a second group; access bursts do come back, and their soft bits are not the fused
    default group's."""
    import torch
    from scipy.signal import resample_poly
    from openbts_ttsou_amd.frontend import RxFrontEnd
    sps = 4
    x, ctype = cells[sps]
    rng = np.random.default_rng(5)
    iq = []
    for a in range(S):
        sig = np.concatenate([x[t, a, :(156 + (t % 4 == 0)) * sps] for t in range(T)]).astype(np.complex128)
        lo = resample_poly(sig, 96, 65 * sps)
        lo = lo + (rng.standard_normal(lo.size) + 1j * rng.standard_normal(lo.size)) * 5.0
        v = np.empty((lo.size, 2), np.int16)
        v[:, 0] = np.clip(np.round(lo.imag), -32768, 32767)   # the radio delivers Q first
        v[:, 1] = np.clip(np.round(lo.real), -32768, 32767)
        iq.append(v)
    K = min(len(v) for v in iq) // 864
    d_iq = torch.from_numpy(np.ascontiguousarray(np.stack([v[:K * 864] for v in iq]))).cuda()
    lpf = synth.design_lpf(961, 65 * sps)
    ctx = pkg.TrxSig(sps, 0); ctx.use_torch_stream()
    keys = ("valid", "soft", "rssi", "timing", "threshold")
    got = []
    for route, rach_leg in (("rxfe", pkg.RACHLEG_MLSE), ("bursts", pkg.RACHLEG_MLSE), ("rxfe", pkg.RACHLEG_DEMOD)):
        g = pkg.TrxGroup(ctx, S, tsc_leg=pkg.TSCLEG_DEMOD, start=(FN0, 0))
        g.set_rach_leg(rach_leg)
        configure(g, pkg)
        fe = RxFrontEnd(ctx, S, lpf, max_chunks=K)
        if route == "rxfe":
            ns, res = g.pull_rxfe(fe, d_iq, FN0)
        else:
            fe.push_chunk(d_iq)
            xs, off, length, _ = fe.pop_bursts()
            ns = off.numel() // S
            res = g.pull_bursts(xs, off, length, ns, FN0, 0)
        assert ns >= 12 and res.n_slots == ns
        got.append((ns, g.collect()))
        torch.cuda.synchronize()
        fe.close(); g.close()
    ctx.close()
    (na, a), (nb, b), (nc, c) = got
    assert na == nb == nc
    for k in keys:
        assert np.array_equal(a[k], b[k], equal_nan=True), k
    acc = (ctype[:na] == tm.RACH) & a["valid"]
    assert acc.sum() >= 3 and np.array_equal(a["valid"], c["valid"])
    assert all(a["soft"][t, s].tobytes() != c["soft"][t, s].tobytes() for t, s in np.argwhere(acc))
    tsc = (ctype[:na] == tm.TSC) & a["valid"]
    assert tsc.sum() >= 25 and np.array_equal(a["soft"][tsc], c["soft"][tsc])             # (the fused source gives the push / pop route's values)


def test_setter_refusals(pkg):
    """Any value but the two legs is refused (TRXSIG_EINVAL) and leaves the leg as it was; both legs are accepted on every tsc leg."""
    for sps, legs in ((1, ("TSCLEG_EQUALIZE", "TSCLEG_DEMOD", "TSCLEG_MLSE")), (4, ("TSCLEG_DEMOD", "TSCLEG_MLSE"))):
        ctx = pkg.TrxSig(sps, 0)
        for leg in legs:
            g = pkg.TrxGroup(ctx, 2, tsc_leg=getattr(pkg, leg))
            for bad in (2, -1, 255):
                with pytest.raises(pkg.TrxSigError):
                    g.set_rach_leg(bad)
            g.set_rach_leg(pkg.RACHLEG_MLSE); g.set_rach_leg(pkg.RACHLEG_DEMOD)
            g.close()
        ctx.close()
    t = pkg.TrxHost(4, 0)
    assert not hasattr(t.L, "trxsig_trx_set_rach_leg")         # the one-burst object does not get the setter
    t.close()


# ---- the closed loop: l1ms -> radiate -> trxsig_air_cells with a fixed tap set -> pull -> l1rx, one combination-V slot ----
def test_closed_loop_through_three_symbols_of_spread(pkg):
    """L1Ms.encode -> radiate -> Air.cells with tests/mlse_access_loop.py's fixed taps (three symbols of spread at sps 4, no noise) ->
    TrxGroup.pull -> L1Rx.decode on the RACH of one combination-V slot: 27 access bursts in 51 frames, each with a random RA and the
    cell's BSIC.  The tap set, (-0.72 + 0.13j, -0.15 + 0.99j, 0.73 + 0.03j, -0.33 - 0.43j) a symbol apart, was chosen on the CPU
    through air_model, the oracle, the equaliser's model and the FEC oracle: there every burst is detected (the smallest
    peak-to-mean ratio is 8.3 against the threshold of 5; with tests/mlse_loop.py's own taps it is 4.8 and nothing is detected),
    the modelled equalising chain decodes 27 of 27 RAs and the modelled demodulating chain 22 of 27 (asserted again here, on the CPU
    model of the cells).  On the GPU every RA comes back on TRXSIG_RACHLEG_MLSE, its soft rows equal the model's on the cells the
    device made, and the default leg loses at least one."""
    import torch
    import fectxbind
    import mlse_access_loop as ml
    o = oraclebind.Oracle(ml.SPS)
    c = ml.case(fectxbind.FecTxOracle())
    cpu = ml.cpu_chains(o, c, ml.cpu_cells(o, c))
    sent = c["sent"]
    assert len(sent) == 27 and cpu["detected"].all() and cpu["ok_mlse"].all() and cpu["ok_demod"].sum() == 22
    sps, A, F, fn0, comb, m = ml.SPS, ml.A, ml.F, ml.FN0, c["comb"], c["m"]
    T_, cell = 8 * F, 160 * sps
    ctx = pkg.TrxSig(sps, 0)
    ctx.use_torch_stream()
    ms = pkg.L1Ms(ctx, comb, ml.BSIC, ml.BAND)
    ms.encode(fn0, F, **{k: dev(v) for k, v in c["grids"].items()})
    r = ms.collect(state=False)
    assert np.array_equal(r["what"], m["what"]) and np.array_equal(r["bits"], m["bits"])
    clean = torch.zeros(T_, A, cell, 2, dtype=torch.float32, device="cuda")
    none_c, none_f = dev_c(np.zeros(0, np.complex64)), dev(np.zeros(0, np.float32))
    nx = len(c["model"].ch[ml.lms.XCCH])
    nr = len(c["grids"]["rach_kind"])                          # (a gain and a delay per access burst of the call)
    ms.radiate(clean, A * cell, cell, tch_gain=none_c, tch_delay=none_f, xcch_gain=dev_c(np.full(nx, ml.GAIN, np.complex64)),
               xcch_delay=dev(np.zeros(nx, np.float32)), rach_gain=dev_c(np.full(nr, ml.GAIN, np.complex64)),
               rach_delay=dev(np.zeros(nr, np.float32)), amp_of_power=dev(np.ones(41, np.float32)))
    h = ml.taps()
    air = pkg.Air(ctx, len(h))
    rxbuf = torch.zeros_like(clean)
    air.cells(fn0, A, F, 1, clean, A * cell, cell, rxbuf, A * cell, cell, taps=dev_c(np.broadcast_to(h, (A, T_, len(h)))))
    cells = rxbuf.cpu().numpy().view(np.complex64).reshape(T_, A, cell)
    out = {}
    for leg in (pkg.RACHLEG_MLSE, pkg.RACHLEG_DEMOD):
        grp = pkg.TrxGroup(ctx, A, tsc_leg=pkg.TSCLEG_DEMOD, start=(fn0, 0))
        grp.set_rach_leg(leg)
        for cmd in ["CMD RXTUNE 890000", "CMD TXTUNE 935000", "CMD SETTSC %d" % (ml.BSIC & 7)] + \
                   ["CMD SETSLOT %d %d" % (tn, comb[0, tn]) for tn in range(8)] + ["CMD POWERON"]:
            grp.control(0, cmd)
        res = grp.pull(rxbuf, A * cell, cell, fn0, 0, T_)
        grp.sync()
        rx = pkg.L1Rx(ctx, comb, ml.BSIC, ml.BAND)
        rx.decode(res, fn0)
        got = rx.collect()
        torch.cuda.synchronize()
        R = res.n_rows
        out[leg] = dict(got=got, col=grp.collect(), row=pkg._to_host(ctx, res.d_row, (T_, A), "<i4"),
                        amp=pkg._to_host(ctx, res.d_amp, (R, 2), "<f4").view(np.complex64).ravel(), toa=pkg._to_host(ctx, res.d_toa, (R,), "<f4"))
        rx.destroy(); grp.close()

    def decoded(got):
        rr = got["rach"]
        heard = {int(f): (bool(ok), int(v)) for f, ok, v in zip(rr["fn"], rr["ok"], rr["ra"])}
        return np.array([heard.get((fn0 + s // 8) % tm.HYPERFRAME) == (True, ra) for s, ra in sent])
    eq = out[pkg.RACHLEG_MLSE]
    assert all(eq["col"]["valid"][s, 0] for s, _ in sent), "a burst was not detected"
    assert decoded(eq["got"]).all(), "the equalising leg lost an access burst"
    assert (~decoded(out[pkg.RACHLEG_DEMOD]["got"])).sum() >= 1, "the demodulating leg lost nothing: the tap set proves nothing"
    for s, _ in sent:                                          # the soft rows: the model on the cells the device made
        x = cells[s, 0, :(156 + (s % 4 == 0)) * sps]
        row = eq["row"][s, 0]
        want = model.access_batch(sps, x, np.array([0], np.int32), np.array([len(x)], np.int32), eq["amp"][row:row + 1], eq["toa"][row:row + 1], oracle=o)
        assert want["win"][0] <= 0
        assert_veq(eq["col"]["soft"][s, 0], want["soft"][0], "slot %d" % s)
    ms.destroy(); air.destroy(); ctx.close()
