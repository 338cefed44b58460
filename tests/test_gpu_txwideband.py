"""The wideband transmit synthesiser (include/trxsig_frontend.h, trxsig_txbe_create_wideband; csrc/trxsig_txwb.hip): C ARFCN
streams modulated from their bits, resampled 96 R : 65 sps, mixed to their carriers and summed into one int16 stream at
R x 400 kS/s.  Checked value for value against the oracle chain of tests/txwb_model.py (modulate -> scale_vector ->
polyphase_resample with history -> mix_down -> carrier-order complex64 sum -> scale_vector(gain) -> trunc -> clip), for split
invariance, against the narrowband back end in the degenerate case, through saturation, over the air into the wideband receive
front end (both forms), through two Transceiver groups, and for its refusals."""
import ctypes as C

import numpy as np
import pytest

import _pkg
import oraclebind
from txwb_model import TxwbModel

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pkg():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return _pkg.load()


def tx_lpf(R):
    """The synthesiser's filter: 7 * 96 R + 1 taps for interpolation by 96 R (8 taps per output), Kaiser beta 6, cutoff at half the
    narrowband Nyquist (design_lpf(5377, 768, beta=6.0, cutoff=0.5) at R = 8)."""
    from openbts_ttsou_amd import synth
    return synth.design_lpf(7 * 96 * R + 1, 96 * R, beta=6.0, cutoff=0.5)


def spaced(C, R, spacing=400e3):
    """C carriers `spacing` apart round the centre, as the receive channeliser takes them: -2 pi f / fs radians per sample."""
    fs = 400e3 * R
    return np.float32([-2.0 * np.pi * (c - (C - 1) / 2.0) * spacing / fs for c in range(C)])


def guards(tn, nb):
    return np.array([8 + ((tn + k) % 4 == 0) for k in range(nb)], np.int32)


def run_schedule(pkg, be, model, rng, pushes, tsc=0, with_gain=False, bits_out=None):
    """Push the given burst counts (popping after each), compare every pop with the model; returns the concatenated int16."""
    from openbts_ttsou_amd import synth
    got, tn = [], 0
    for nb in pushes:
        bits = np.stack([synth.normal_bits(rng, nb, tsc) for _ in range(be.S)])
        gain = rng.uniform(0.2, 1.0, (be.S, nb)).astype(np.float32) if with_gain else None
        g = guards(tn, nb); tn = (tn + nb) % 8
        be.push_bursts(bits, g, gain)
        if model is not None:
            model.push(bits, g, gain)
        if bits_out is not None:
            bits_out.append(bits)
        d = be.pop_samples()
        want = model.pop() if model is not None else None
        if d is None:
            assert want is None
            continue
        iq = d.cpu().numpy()
        if model is not None:
            assert iq.shape == want.shape, (iq.shape, want.shape)
            bad = np.argwhere(np.any(iq != want, axis=2))
            assert bad.size == 0, "first mismatch at (stream, sample) %s: %s vs %s" % (bad[0], iq[tuple(bad[0])], want[tuple(bad[0])])
        got.append(iq.copy())
    return np.concatenate(got, axis=1)


CASES = [(1, 1, 2), (1, 4, 8), (1, 8, 2), (4, 1, 8), (4, 4, 2), (4, 8, 8)]


@pytest.mark.parametrize("with_gain", [False, True])
@pytest.mark.parametrize("sps,C,R", CASES)
def test_value_exact_against_the_oracle_chain(pkg, sps, C, R, with_gain):
    rng = np.random.default_rng(1000 * sps + 10 * C + R + with_gain)
    Sw = 2
    freq = rng.uniform(-3.1, 3.1, C).astype(np.float32)
    lpf = tx_lpf(R)
    ctx = pkg.TrxSig(sps, 0); ctx.use_torch_stream()
    from openbts_ttsou_amd.frontend import TxBackEnd
    be = TxBackEnd(ctx, Sw, lpf, gain=13500.0 / C, max_bursts=48, carrier_freq=freq, rate_factor=R)
    assert be.S == Sw * C and be.Sw == Sw
    model = TxwbModel(oraclebind.Oracle(sps), Sw, freq, R, lpf, 13500.0 / C)
    pushes = [int(rng.integers(1, 6)) for _ in range(6)] + [40] + [int(rng.integers(1, 9)) for _ in range(3)]   # (40: a multi-chunk pop)
    out = run_schedule(pkg, be, model, rng, pushes, with_gain=with_gain)
    assert out.shape[1] >= 864 * R * 8
    assert np.abs(out.astype(np.int32)).max() > 100                  # (not a stream of zeros)
    be.close(); ctx.close()


def test_split_invariance(pkg):
    """Two different push schedules of the same bursts, a pop after every push, give the same concatenated int16 streams.  (Every
    push here is shorter than a chunk, so every pop takes at most one chunk in both schedules: what a pop emits also depends on how
    many chunks it takes -- its last outputs' taps that reach past the window's end are skipped, as in pushBuffer.)"""
    from openbts_ttsou_amd import synth
    from openbts_ttsou_amd.frontend import TxBackEnd
    sps, Sw, C, R = 4, 2, 4, 8
    freq = spaced(C, R)
    lpf = tx_lpf(R)
    rng = np.random.default_rng(5)
    nb = 60
    bits = np.stack([synth.normal_bits(rng, nb, 1) for _ in range(Sw * C)])
    g = guards(0, nb)
    outs = []
    ctx = pkg.TrxSig(sps, 0); ctx.use_torch_stream()
    for seed in (1, 2):
        r = np.random.default_rng(seed)
        cuts = [0]
        while cuts[-1] < nb:
            cuts.append(min(nb, cuts[-1] + int(r.integers(1, 4))))    # 1-3 bursts: less than a chunk (585 x 4 samples)
        be = TxBackEnd(ctx, Sw, lpf, gain=13500.0 / C, max_bursts=8, carrier_freq=freq, rate_factor=R)
        got = []
        for a, b in zip(cuts[:-1], cuts[1:]):
            be.push_bursts(np.ascontiguousarray(bits[:, a:b]), g[a:b])
            d = be.pop_samples()
            if d is not None:
                assert d.shape[1] == 864 * R
                got.append(d.cpu().numpy().copy())
        outs.append(np.concatenate(got, axis=1))
        be.close()
    assert outs[0].shape == outs[1].shape and outs[0].shape[1] >= 864 * R * 12
    assert np.array_equal(outs[0], outs[1])
    ctx.close()


@pytest.mark.parametrize("sps", [1, 4])
def test_degenerate_case_equals_the_narrowband_back_end(pkg, sps):
    """C = 1, R = 1, f = 0: the synthesiser is the narrowband back end sample for sample."""
    from openbts_ttsou_amd import synth
    from openbts_ttsou_amd.frontend import TxBackEnd
    lpf = synth.design_lpf(651, 96)
    ctx = pkg.TrxSig(sps, 0); ctx.use_torch_stream()
    nbe = TxBackEnd(ctx, 3, lpf, gain=13500.0, max_bursts=48)
    wbe = TxBackEnd(ctx, 3, lpf, gain=13500.0, max_bursts=48, carrier_freq=[0.0], rate_factor=1)
    rng = np.random.default_rng(11 + sps)
    tn, n = 0, 0
    for it, nb in enumerate((2, 5, 1, 40, 3, 7)):
        bits = np.stack([synth.normal_bits(rng, nb, 4) for _ in range(3)])
        gain = rng.uniform(0.1, 1.0, (3, nb)).astype(np.float32) if it % 2 else None
        g = guards(tn, nb); tn = (tn + nb) % 8
        nbe.push_bursts(bits, g, gain); wbe.push_bursts(bits, g, gain)
        a, b = nbe.pop_samples(), wbe.pop_samples()
        assert (a is None) == (b is None)
        if a is not None:
            assert np.array_equal(a.cpu().numpy(), b.cpu().numpy()), it
            n += a.shape[1]
    assert n > 5000
    nbe.close(); wbe.close(); ctx.close()


def test_saturation_clips_to_the_oracle_values(pkg):
    """Eight carriers at gain 13500 (each carrier at the narrowband level): the sum passes full scale and is clipped, exactly."""
    from openbts_ttsou_amd.frontend import TxBackEnd
    sps, Sw, C, R = 4, 1, 8, 8
    freq = spaced(C, R)
    lpf = tx_lpf(R)
    ctx = pkg.TrxSig(sps, 0); ctx.use_torch_stream()
    be = TxBackEnd(ctx, Sw, lpf, gain=13500.0, max_bursts=32, carrier_freq=freq, rate_factor=R)
    model = TxwbModel(oraclebind.Oracle(sps), Sw, freq, R, lpf, 13500.0)
    rng = np.random.default_rng(17)
    out = run_schedule(pkg, be, model, rng, [24], tsc=3)
    assert model.peak > 32767.0, model.peak                          # (about 1e5 for this shape)
    clipped = int(np.count_nonzero((out == 32767) | (out == -32768)))
    assert clipped > 100, clipped
    be.close(); ctx.close()


RX_LPF = (8001, 260, 6.0, 0.09)      # the receive channeliser's filter (bench.py's): ~145 kHz at the 3.2 MS/s input rate


@pytest.mark.parametrize("shared", [False, True])
def test_over_the_air_into_the_wideband_receive_front_end(pkg, shared):
    """C = 8 carriers 400 kHz apart at R = 8, sps 4: the synthesiser's int16 stream, fed to RxFrontEnd with the same carrier array
    (per-carrier or shared-filter form), then detect + demodulate.  Image rejection of the filters: the transmit filter
    (design_lpf(5377, 768, beta=6, cutoff=0.5)) leaves the images of the 400 kS/s stream at 400 kHz multiples below -60 dB;
    the receive filter's stop band at the 400 kHz neighbour is below -60 dB as well."""
    import torch
    from openbts_ttsou_amd import synth
    from openbts_ttsou_amd.frontend import TxBackEnd, RxFrontEnd
    sps, Sw, C, R, tsc = 4, 1, 8, 8, 5
    freq = spaced(C, R)
    ctx = pkg.TrxSig(sps, 0); ctx.use_torch_stream()
    be = TxBackEnd(ctx, Sw, tx_lpf(R), gain=13500.0 / C, max_bursts=32, carrier_freq=freq, rate_factor=R)
    rx_lpf = synth.design_lpf(RX_LPF[0], RX_LPF[1], beta=RX_LPF[2], cutoff=RX_LPF[3])
    fe = RxFrontEnd(ctx, Sw, rx_lpf, swap_iq=False, max_chunks=16, carrier_freq=freq, rate_factor=R)
    if shared:
        fe.set_shared_filter(True)
    rng = np.random.default_rng(23)
    sent = []
    iq = run_schedule(pkg, be, None, rng, [24], tsc=tsc, bits_out=sent)
    sent = sent[0]                                                   # [S, 24, 148]
    assert np.abs(iq.astype(np.int32)).max() < 32767                  # nothing clipped at 13500 / 8
    fe.push_wideband(torch.from_numpy(iq).cuda())
    x, off, length, tnv = fe.pop_bursts()
    S = Sw * C
    nb = off.numel() // S
    B = S * nb
    flags = torch.zeros(B, dtype=torch.uint8, device="cuda"); amp = torch.zeros(B, 2, device="cuda")
    toa = torch.zeros(B, device="cuda"); soft = torch.zeros(B, 148, device="cuda")
    ctx.detect_demod_normal(x, off, length, tsc, flags, amp, toa, soft, energy_thresh=50.0)
    torch.cuda.synchronize()
    fl = flags.cpu().numpy(); sf = soft.cpu().numpy()
    complete = min(nb, sent.shape[1]) - 1                              # (the last one cut may be incomplete)
    for s in range(S):
        det = 0
        for j in range(1, complete):                                   # (burst 0 loses its head to the filters' delay)
            i = s * nb + j
            if fl[i] & pkg.F_DETECT:
                assert np.array_equal((sf[i] > 0.5).astype(np.uint8), sent[s, j]), (s, j)
                det += 1
        assert det >= 0.9 * (complete - 1), (s, det, complete - 1)
    assert complete >= 15
    fe.close(); be.close(); ctx.close()


def test_through_two_transceiver_groups(pkg):
    """A group of Sw * C ARFCNs takes 154-byte datagrams, pushes them into the synthesiser; its int16 stream goes through the wideband
    receive front end into a second group's pull_rxfe, which hands back the queued bursts' bits per ARFCN."""
    from openbts_ttsou_amd import synth
    from openbts_ttsou_amd.frontend import TxBackEnd, RxFrontEnd
    import torch
    sps, Sw, C, R, tsc, F, fn0 = 4, 1, 8, 8, 2, 12, 1000
    S = Sw * C
    freq = spaced(C, R)
    ctx = pkg.TrxSig(sps, 0); ctx.use_torch_stream()
    ga = pkg.TrxGroup(ctx, S, tsc_leg=pkg.TSCLEG_DEMOD, start=(fn0, 0))
    gb = pkg.TrxGroup(ctx, S, tsc_leg=pkg.TSCLEG_DEMOD, start=(fn0, 0))
    for g in (ga, gb):
        for a in range(S):
            for m in ["CMD RXTUNE 890000", "CMD TXTUNE 935000", "CMD SETTSC %d" % tsc] + ["CMD SETSLOT %d 1" % t for t in range(8)] + ["CMD POWERON"]:
                g.control(a, m)
    rng = np.random.default_rng(41)
    n = S * F * 8
    arf = np.repeat(np.arange(S, dtype=np.int32), F * 8)
    f = np.tile(np.repeat(np.arange(F), 8), S)
    tn = np.tile(np.arange(8), S * F)
    fn = fn0 + f
    dg = np.zeros((n, 154), np.uint8)
    dg[:, 0] = tn
    dg[:, 1] = fn >> 24; dg[:, 2] = (fn >> 16) & 255; dg[:, 3] = (fn >> 8) & 255; dg[:, 4] = fn & 255
    dg[:, 5] = 0                                                      # RSSI 0: gain 1
    dg[:, 6:] = synth.normal_bits(rng, n, tsc)
    ga.add_bursts(dg, arf)
    be = TxBackEnd(ctx, Sw, tx_lpf(R), gain=13500.0 / C, max_bursts=F * 8, carrier_freq=freq, rate_factor=R)
    ga.push_txbe(be, fn0, 0, F * 8)
    iq = be.pop_samples()
    assert iq is not None
    rx_lpf = synth.design_lpf(RX_LPF[0], RX_LPF[1], beta=RX_LPF[2], cutoff=RX_LPF[3])
    fe = RxFrontEnd(ctx, Sw, rx_lpf, swap_iq=False, max_chunks=64, carrier_freq=freq, rate_factor=R)
    n_slots, res = gb.pull_rxfe(fe, iq.contiguous(), fn0)
    assert n_slots >= 8 * (F - 2)
    out = gb.collect()
    valid, soft = out["valid"], out["soft"]
    sent = dg[:, 6:].reshape(S, F * 8, 148)
    ok = 0
    for t in range(1, n_slots):
        for a in range(S):
            if valid[t][a]:
                assert np.array_equal((np.asarray(soft[t][a]) > 0.5).astype(np.uint8), sent[a, t]), (t, a)
                ok += 1
    assert ok >= 0.9 * (n_slots - 1) * S, (ok, n_slots, S)
    ga.close(); gb.close(); fe.close(); be.close(); ctx.close()


def test_refusals(pkg):
    ctx = pkg.TrxSig(4, 0)
    L = ctx.L
    from openbts_ttsou_amd.frontend import TxBackEnd
    base = L.trxsig_live_children(ctx.h)
    lpf = tx_lpf(8)
    fr = spaced(8, 8)
    h = C.c_void_p()

    def create(Sw=2, nc=8, freq=fr, R=8, lpf=lpf, L_=None):
        f = None if freq is None else np.ascontiguousarray(freq, np.float32)
        lp = np.ascontiguousarray(lpf, np.float32)
        return L.trxsig_txbe_create_wideband(C.byref(h), ctx.h, Sw, nc, None if f is None else f.ctypes.data, R, 16,
                                             lp.ctypes.data, lp.size if L_ is None else L_, 1000.0)
    EINVAL = create(nc=0)
    assert EINVAL < 0
    for kw in (dict(nc=65, freq=np.zeros(65)), dict(nc=0), dict(R=0), dict(R=65), dict(freq=None), dict(Sw=0),
               dict(freq=np.float32([4.0] * 8)),
               dict(lpf=np.ones(32 * 96 * 8 + 1)),                   # 33 taps per output
               dict(R=64, nc=1, freq=[0.0], lpf=np.ones(96 * 64 * 6))):   # (6 taps per output, but 1,536 rows x 7 floats: 42 KiB)
        assert create(**kw) == EINVAL, kw
        assert not h.value
        assert L.trxsig_live_children(ctx.h) == base, kw
    # the limits as stated: 32 taps per output are accepted
    assert create(lpf=np.ones(32 * 96 * 8)) == 0
    L.trxsig_txbe_destroy(h)
    assert L.trxsig_live_children(ctx.h) == base
    be = TxBackEnd(ctx, 2, lpf, gain=1000.0, max_bursts=16, carrier_freq=fr, rate_factor=8)
    assert L.trxsig_live_children(ctx.h) == base + 1
    assert L.trxsig_txbe_streams(be.h) == 16
    assert L.trxsig_txbe_set_fused(be.h, 0) == EINVAL
    assert L.trxsig_txbe_set_fused(be.h, 1) == 0
    # a group whose ARFCN count is not the back end's stream count is refused
    g = pkg.TrxGroup(ctx, 8, tsc_leg=pkg.TSCLEG_DEMOD)
    with pytest.raises(Exception):
        g.push_txbe(be, 100, 0, 8)
    g.close()
    g = pkg.TrxGroup(ctx, 16, tsc_leg=pkg.TSCLEG_DEMOD)
    g.push_txbe(be, 100, 0, 8)                                       # (16 = 2 x 8: taken)
    g.close()
    be.close()
    assert L.trxsig_live_children(ctx.h) == base
    ctx.close()
