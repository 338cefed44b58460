"""The channeliser graded per output on the card (trxsig_rxfe_push_wideband, both forms), across the shapes where the
kernels differ: C = 1, 2, 4, 8, 16 carriers on odd AND even bins (DC and +-pi included, scrambled so that the carrier ->
output-row mapping is checked), (sps, rate factor) pairs with different gcd(P, Q), tap-row orders and tail tiles, filters
of exactly 32 / an odd number of / a few taps per output, 1 and 3 wideband streams, pushes of 1 and max_chunks chunks.

- The per-carrier form (k_resample with the mixer) equals the oracle chain (Oracle.mix_down + polyphase_resample,
  pullBuffer's slicing) bit for bit.
- The shared-filter form (k_channelise16) is graded against tests/chan_ref.py with the exact grid frequencies:
  |y - y_ref| <= c u A(o) per output, u = 2^-24, A(o) = sum_k |h_k| (|Re x| + |Im x|) (see test_shared_form_matrix).
- set_shared_filter refuses exactly what the kernel cannot launch, and the front end keeps working in the per-carrier form."""
import numpy as np
import pytest

import _pkg
import chan_ref
import oraclebind
import synth

pytestmark = pytest.mark.gpu

U = chan_ref.U
C_FFT = 26                                           # derived in test_shared_form_matrix's docstring
C_DIRECT = 53

PAIRS = [(4, 8), (4, 1), (4, 5), (4, 10), (2, 5), (2, 3), (1, 2), (1, 1)]
BINSETS = [
    [5, -2, 8, 0, -7, 3, -4, 6, 1, -1, 4, -6, 7, 2, -3, -5],     # all sixteen, scrambled; bin 8 as +pi
    [6, -4, 0, -8, -2, 4, 2, -6],                                # the even bins, scrambled; bin 8 as -pi
    [0, 8, 3, -5],
    [0, -8], [-1, 6],
    [0], [8], [-8], [5],
]
_ctxs = {}


def ctx_for(pkg, sps):
    if sps not in _ctxs:
        t = pkg.TrxSig(sps, 0)
        t.use_torch_stream()
        _ctxs[sps] = t
    return _ctxs[sps]


def lpf_for(kind, P, cw):
    L = {"32": 32 * P, "odd": 20 * P + 37, "short": 3 * P + 5}[kind]
    return synth.design_lpf(L, P, beta=6.0, cutoff=min(0.9, 0.09 * 8 / cw))


def freqs_of(bins):
    return np.float32([2.0 * np.pi * b / 16.0 for b in bins])


def full_scale(rng, Sw, n):
    iq = rng.integers(-32768, 32768, size=(Sw, n, 2)).astype(np.int16)
    m = max(1, n // 50)
    for w in range(Sw):
        iq[w, rng.integers(0, n, size=m), rng.integers(0, 2, size=m)] = -32768
    return iq


def run_form(pkg, ctx, iq, sps, cw, lpf, freqs, swap, pushes, max_chunks, shared):
    """Push iq [Sw, n, 2] in `pushes` chunk counts; return every stream's resampled samples taken out so far (complex64)."""
    import torch
    from openbts_ttsou_amd.frontend import RxFrontEnd
    Sw = iq.shape[0]
    C = len(freqs)
    S = Sw * C
    chunk = chan_ref.OUTCHUNK * cw
    fe = RxFrontEnd(ctx, Sw, lpf, max_chunks=max_chunks, carrier_freq=freqs, rate_factor=cw, swap_iq=swap)
    try:
        if shared:
            fe.set_shared_filter(True)
        d_iq = torch.from_numpy(np.ascontiguousarray(iq)).cuda()
        got = [np.zeros(0, np.complex64) for _ in range(S)]
        c = 0
        for k in pushes:
            fe.push_wideband(d_iq[:, c * chunk:(c + k) * chunk]); c += k
            popped = fe.pop_bursts()
            if popped is None:
                continue
            x, off, length, _ = popped
            nb = off.numel() // S
            xh = x.cpu().numpy().view(np.complex64).ravel(); offh = off.cpu().numpy(); lenh = length.cpu().numpy()
            for s in range(S):
                n = int(lenh[s * nb:(s + 1) * nb].sum())
                got[s] = np.concatenate([got[s], xh[offh[s * nb]:offh[s * nb] + n]])
        torch.cuda.synchronize()
        assert c * chunk == iq.shape[1]
        return got
    finally:
        fe.close()


def oracle_streams(iq, sps, cw, lpf, freqs, swap):
    """The per-carrier chain on the reference's primitives (as tests/test_gpu_channeliser.py builds it), stream w * C + c."""
    from test_chan_ref import oracle_chain
    o = oraclebind.Oracle(sps)
    return [oracle_chain(o, iq[w], sps, cw, lpf, f, swap) for w in range(iq.shape[0]) for f in freqs]


def reference_streams(iq, sps, cw, lpf, bins, swap):
    ys, As = [], []
    for w in range(iq.shape[0]):
        y, A = chan_ref.channelise(iq[w], sps, cw, lpf, chan_ref.grid_mixer(bins), swap_iq=swap)
        ys += list(y); As += [A] * len(bins)
    return ys, As


def grade(got, ys, As, c, what):
    """Largest err / (u A) over every output taken out; fails past c (where A = 0 the output must be exactly 0)."""
    worst = 0.0
    for s, (g, y, A) in enumerate(zip(got, ys, As)):
        n = g.size
        assert n > 0 and n <= y.size, (what, s, n, y.size)
        err = np.abs(g.astype(np.complex128) - y[:n])
        zero = A[:n] == 0
        assert not err[zero].any(), "%s: stream %d: non-zero output where every input the taps meet is zero" % (what, s)
        r = err[~zero] / (U * A[:n][~zero])
        if r.size:
            i = int(np.argmax(r))
            assert r[i] <= c, "%s: stream %d output %d: |err| = %.3g = %.1f u A(o) > %d u A(o)" % (what, s, i, err[~zero][i], r[i], c)
            worst = max(worst, float(r[i]))
    return worst


@pytest.mark.timeout(900)
@pytest.mark.parametrize("sps,cw", PAIRS)
def test_shared_form_matrix(sps, cw):
    """Both forms on every bin set of BINSETS at this (sps, CW); filters rotate through 32 / odd / short taps per output,
    1 and 3 wideband streams, swap_iq on and off, pushes of 1 and max_chunks = 3 chunks (the history crosses calls).

    The shared form's bound, to first order in u, with x exact (int16) and the taps the float32 values the reference uses:
    - partial sums T_j = fma(h, x, T_j), at most two taps per j (kt <= 32): each component's error is <= 2 u sum |h| |x_part|,
      so sum_j |dT_j| <= 2 u A.
    - FFT path (C >= 4): four radix-2 stages.  An add or subtract rounds each component (<= u |z|); a twiddle multiply by
      the float32-rounded twiddle (|w^ - w| <= u) costs two products and a sum per component (<= 2 sqrt 2 u |z|), so a
      stage adds <= (1 + 1 + 2 sqrt 2) u = 4.83 u of the modulus of each node.  Every later stage has modulus gain 1 per
      path, and the nodes a bin depends on at any stage partition the inputs, so each stage contributes <= 4.83 u sum |T_j|
      <= 4.83 u A to a bin: 19.3 u A for four.  The final rotation by the float32-rounded m_c[rho] (|m^ - m| <= u; a product
      and an fma per component, <= 2 sqrt 2 u): 3.83 u A.  c_fft = 2 + 19.3 + 3.83 = 25.2 -> C_FFT = 26.
    - Direct path (C < 4): 32 chained fmas per component with float32-rounded exp(-j theta j) (<= u sum |T_j| = u A); the
      i-th fma's rounding is <= u times the partial sum, so the chain is <= 32 u sum of its terms, and the two components'
      terms sum to <= sqrt 2 A: 45.3 u A.  c_direct = 2 + 1 + 45.3 + 3.83 = 52.1 -> C_DIRECT = 53.
    The test prints the largest measured err / (u A) of each path."""
    pkg = _pkg.load()
    ctx = ctx_for(pkg, sps)
    P = 65 * sps
    chunk = chan_ref.OUTCHUNK * cw
    rng = np.random.default_rng(1000 * sps + cw)
    worst = {"fft": 0.0, "direct": 0.0}
    for i, bins in enumerate(BINSETS):
        kind = ("32", "odd", "short")[(i + PAIRS.index((sps, cw))) % 3]
        lpf = lpf_for(kind, P, cw)
        Sw = 3 if i % 2 == 0 else 1
        swap = i % 3 != 1
        pushes = (1, 3) if i % 2 == 0 else (3, 1)
        iq = full_scale(rng, Sw, sum(pushes) * chunk)
        freqs = freqs_of(bins)
        what = "sps %d CW %d bins %s L %d Sw %d swap %d" % (sps, cw, bins, lpf.size, Sw, swap)
        per = run_form(pkg, ctx, iq, sps, cw, lpf, freqs, swap, pushes, 3, shared=False)
        want = oracle_streams(iq, sps, cw, lpf, freqs, swap)
        for s, (g, w) in enumerate(zip(per, want)):
            assert g.size > 0 and np.array_equal(g, w[:g.size]), "per-carrier form vs oracle chain: %s stream %d" % (what, s)
        sh = run_form(pkg, ctx, iq, sps, cw, lpf, freqs, swap, pushes, 3, shared=True)
        ys, As = reference_streams(iq, sps, cw, lpf, bins, swap)
        path = "fft" if len(bins) >= 4 else "direct"
        worst[path] = max(worst[path], grade(sh, ys, As, C_FFT if path == "fft" else C_DIRECT, what))
    print("shared form vs float64 reference, sps %d CW %d: worst err/(u A) FFT path %.2f (c = %d), direct path %.2f (c = %d)"
          % (sps, cw, worst["fft"], C_FFT, worst["direct"], C_DIRECT))


def band_noise(rng, n, bw):
    """Complex noise band-limited to |f| < bw (cycles per sample), unit RMS."""
    X = rng.standard_normal(n) + 1j * rng.standard_normal(n)
    f = np.fft.fftfreq(n)
    X[np.abs(f) >= bw] = 0
    x = np.fft.ifft(X)
    return x / np.sqrt(np.mean(np.abs(x) ** 2))


@pytest.mark.timeout(300)
@pytest.mark.parametrize("bins", [[2, 4, -5, 8], [2, 4]])
def test_weak_carrier_per_output_bound(bins):
    """A carrier 60 dB below its neighbour 400 kHz away (bin 4 beside bin 2 at 3.2 MS/s) stays inside the per-output bound:
    the old global bound, 1e-4 of the largest sample anywhere, allows an error of a fifth of the weak carrier's RMS in every
    one of its samples."""
    pkg = _pkg.load()
    sps, cw = 4, 8
    ctx = ctx_for(pkg, sps)
    P = 65 * sps
    chunk = chan_ref.OUTCHUNK * cw
    rng = np.random.default_rng(60)
    n = 4 * chunk
    t = np.arange(n)
    amp = {2: 8000.0, 4: 8.0, -5: 3000.0, 8: 3000.0}
    sig = sum(amp[b] * band_noise(rng, n, 0.02) * np.exp(-2j * np.pi * b * t / 16.0) for b in bins)
    iq = np.empty((1, n, 2), np.int16)
    iq[0, :, 0] = np.clip(np.round(sig.imag), -32768, 32767)
    iq[0, :, 1] = np.clip(np.round(sig.real), -32768, 32767)
    lpf = lpf_for("32", P, cw)
    freqs = freqs_of(bins)
    per = run_form(pkg, ctx, iq, sps, cw, lpf, freqs, True, (1, 3), 3, shared=False)
    want = oracle_streams(iq, sps, cw, lpf, freqs, True)
    for g, w in zip(per, want):
        assert np.array_equal(g, w[:g.size])
    sh = run_form(pkg, ctx, iq, sps, cw, lpf, freqs, True, (1, 3), 3, shared=True)
    ys, As = reference_streams(iq, sps, cw, lpf, bins, True)
    c = C_FFT if len(bins) >= 4 else C_DIRECT
    worst = grade(sh, ys, As, c, "weak carrier %s" % bins)
    weak, strong = bins.index(4), bins.index(2)
    pw = np.mean(np.abs(ys[weak][P:sh[weak].size]) ** 2); ps = np.mean(np.abs(ys[strong][P:sh[strong].size]) ** 2)
    rel = float(np.abs(sh[weak] - ys[weak][:sh[weak].size]).max() / np.sqrt(pw))
    glob = 1e-4 * max(float(np.abs(y).max()) for y in ys)
    print("weak carrier %.1f dB below its neighbour: worst err/(u A) %.2f (c = %d); worst error %.2e of the weak carrier's RMS "
          "(a global 1e-4 bound would allow %.1f x its RMS)" % (10 * np.log10(ps / pw), worst, c, rel, glob / np.sqrt(pw)))
    assert 10 * np.log10(ps / pw) > 50
    assert glob > 0.1 * np.sqrt(pw)
    assert rel < 1e-3


@pytest.mark.timeout(120)
@pytest.mark.parametrize("bins", [[0, 8, 3, -5], [5]])
def test_zero_stream_gives_exact_zeros(bins):
    pkg = _pkg.load()
    sps, cw = 4, 8
    ctx = ctx_for(pkg, sps)
    iq = np.zeros((2, 4 * chan_ref.OUTCHUNK * cw, 2), np.int16)
    lpf = lpf_for("odd", 65 * sps, cw)
    for shared in (False, True):
        got = run_form(pkg, ctx, iq, sps, cw, lpf, freqs_of(bins), True, (1, 3), 3, shared=shared)
        for g in got:
            assert g.size > 0 and not g.view(np.float32).any()


@pytest.mark.timeout(300)
def test_tiles_per_workgroup_knob_is_bit_identical():
    """TRXSIG_TUNE_CHAN_TPW = 1, 2, 3, 4, 7 (3 and 7 leave a short last workgroup: ten tiles per window) give the default's bits."""
    pkg = _pkg.load()
    sps, cw = 4, 8
    ctx = ctx_for(pkg, sps)
    rng = np.random.default_rng(7)
    iq = full_scale(rng, 3, 4 * chan_ref.OUTCHUNK * cw)
    lpf = lpf_for("32", 65 * sps, cw)
    freqs = freqs_of(BINSETS[1])
    base = run_form(pkg, ctx, iq, sps, cw, lpf, freqs, True, (1, 3), 3, shared=True)
    try:
        for v in (1, 2, 3, 4, 7):
            ctx.set_tuning(chan_tpw=v)
            got = run_form(pkg, ctx, iq, sps, cw, lpf, freqs, True, (1, 3), 3, shared=True)
            for s, (g, b) in enumerate(zip(got, base)):
                assert np.array_equal(g, b), "TRXSIG_TUNE_CHAN_TPW=%d, stream %d" % (v, s)
    finally:
        ctx.set_tuning(chan_tpw=0)


@pytest.mark.timeout(300)
def test_closed_loop_even_bins():
    """C = 8 carriers 400 kHz apart on the even bins (DC and +-1.6 MHz = bin 8 included), built as make_wideband builds its
    signal: the bursts detected and demodulated from the shared form carry the bits that were sent."""
    import torch
    from openbts_ttsou_amd.frontend import RxFrontEnd
    from test_gpu_channeliser import CW, SPS, make_wideband
    pkg = _pkg.load()
    ctx = ctx_for(pkg, SPS)
    tsc = 5
    fs = 400e3 * CW
    offsets = (-1.6e6, -1.2e6, -0.8e6, -0.4e6, 0.0, 0.4e6, 0.8e6, 1.2e6)
    freqs = np.float32([-2.0 * np.pi * f / fs for f in offsets])
    lpf = synth.design_lpf(8001, 65 * SPS, beta=6.0, cutoff=0.09)
    iq, nchunks, bits_all = make_wideband(1, offsets, 24, tsc, seed=21)
    nchunks = min(nchunks, 5)
    C = len(offsets)
    chunk = 864 * CW
    fe = RxFrontEnd(ctx, 1, lpf, max_chunks=3, carrier_freq=freqs, rate_factor=CW)
    try:
        fe.set_shared_filter(True)
        d_iq = torch.from_numpy(np.ascontiguousarray(iq[:, :nchunks * chunk])).cuda()
        c = tn = checked = 0
        for k in (2, 3):
            fe.push_wideband(d_iq[:, c * chunk:(c + k) * chunk]); c += k
            x, off, length, _ = fe.pop_bursts()
            nb = off.numel() // C
            B = C * nb
            flags = torch.zeros(B, dtype=torch.uint8, device="cuda"); amp = torch.zeros(B, 2, device="cuda")
            toa = torch.zeros(B, device="cuda"); soft = torch.zeros(B, 148, device="cuda")
            ctx.detect_demod_normal(x, off, length, tsc, flags, amp, toa, soft, energy_thresh=50.0)
            torch.cuda.synchronize()
            fl = flags.cpu().numpy(); sf = soft.cpu().numpy()
            for s in range(C):
                for j in range(nb):
                    if tn + j >= 1 and (fl[s * nb + j] & pkg.F_DETECT):
                        assert np.array_equal((sf[s * nb + j] > 0.5).astype(np.uint8), bits_all[0][s][tn + j]), (offsets[s], tn + j)
                        checked += 1
            tn += nb
        assert checked >= C * (tn - 2) * 0.9, (checked, C, tn)
    finally:
        fe.close()


def kernel_fits(sps, cw):
    """What k_channelise16 stages per tile: 255 Q / P + 36 raw samples, at most 4 x 256."""
    P, Q = 65 * sps, 96 * cw
    return (255 * Q) // P + 36 <= 1024


@pytest.mark.timeout(600)
def test_shared_filter_refuses_what_it_cannot_launch():
    """Every (sps, rate factor) create_wideband accepts, with sixteen carriers and 32 taps per output: where set_shared_filter
    accepts, one push works and is graded; where the kernel cannot stage a tile's window -- e.g. (1, 8), (2, 8), (4, 12) --
    set_shared_filter refuses with TRXSIG_EINVAL and the same front end pushes in the per-carrier form, bit-exact."""
    import torch
    from openbts_ttsou_amd.frontend import RxFrontEnd
    pkg = _pkg.load()
    bins = BINSETS[0]
    freqs = freqs_of(bins)
    refused, accepted, not_created = [], [], []
    for sps in (1, 2, 4):
        ctx = ctx_for(pkg, sps)
        P = 65 * sps
        lpf = lpf_for("32", P, 8)
        for cw in range(1, 65):
            chunk = chan_ref.OUTCHUNK * cw
            try:
                fe = RxFrontEnd(ctx, 1, lpf, max_chunks=1, carrier_freq=freqs, rate_factor=cw)
            except pkg.TrxSigError as e:
                assert "(-1)" in str(e), str(e)
                not_created.append((sps, cw))
                continue
            try:
                iq = full_scale(np.random.default_rng(cw), 1, chunk)
                try:
                    fe.set_shared_filter(True)
                    ok = True
                except pkg.TrxSigError as e:
                    assert "(-1)" in str(e), str(e)
                    ok = False
                assert ok == kernel_fits(sps, cw), (sps, cw, ok)
                fe.push_wideband(torch.from_numpy(iq).cuda())
                popped = fe.pop_bursts()
                assert popped is not None
                x, off, length, _ = popped
                nb = off.numel() // len(bins)
                xh = x.cpu().numpy().view(np.complex64).ravel(); offh = off.cpu().numpy(); lenh = length.cpu().numpy()
                got = [xh[offh[s * nb]:offh[s * nb] + int(lenh[s * nb:(s + 1) * nb].sum())] for s in range(len(bins))]
                if ok:
                    accepted.append((sps, cw))
                    ys, As = reference_streams(iq, sps, cw, lpf, bins, True)
                    grade(got, ys, As, C_FFT, "sps %d CW %d" % (sps, cw))
                else:
                    refused.append((sps, cw))
                    want = oracle_streams(iq, sps, cw, lpf, freqs, True)
                    for s, (g, w) in enumerate(zip(got, want)):
                        assert g.size > 0 and np.array_equal(g, w[:g.size]), (sps, cw, s)
            finally:
                fe.close()
    print("set_shared_filter accepts %d (sps, CW) pairs, refuses %d: %s" % (len(accepted), len(refused), refused))
    print("create_wideband refuses (per-carrier staging): %s" % not_created)
    for need in ((1, 8), (2, 8), (4, 12)):
        assert need in refused
    assert {(1, 3), (2, 6), (4, 11)} <= set(refused) and {(1, 2), (2, 5), (4, 10)} <= set(accepted)
