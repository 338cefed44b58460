"""Synchronisation-burst families for the SCH sequence equaliser's tests (tests/test_mlse_sch_model.py, tests/test_gpu_mlse_sch*.py,
tests/test_gpu_l1acq_mlse.py): the oracle's SCH encoder and modulator, tests/mlse_family.py's static multipath and noise, a delay
in front of the burst, acquisition's own SCH detector (tests/l1_acq_model.py) for amplitude and TOA; and, for the search, whole
C0 streams of tests/l1_acq_model.py through a fixed tap set.  Test INPUT generation only; the expected values come from
tests/mlse_sch_model.py."""
import functools

import numpy as np

import fectxbind
import l1_acq_model as am
import l1_msrx_model as lrm
import mlse_family
import mlse_sch_model as model
import oraclebind

CODED = np.r_[3:42, 106:145]                                   # the 78 coded bits
F32 = np.float32


@functools.lru_cache(maxsize=None)
def _tx():
    return fectxbind.FecTxOracle()


@functools.lru_cache(maxsize=None)
def detector(sps):
    return am.SchDetector(oraclebind.Oracle(sps))


def sch_bits(rng, n):
    """(bits [n, 148], fn [n], bsic [n]): SCH bursts with random reduced frame numbers and BSICs, through the oracle's encoder."""
    fn = np.array([51 * int(rng.integers(0, am.HYPER // 51)) + int(am.SCH_T3[int(rng.integers(0, 5))]) for _ in range(n)], np.uint32)
    bsic = rng.integers(0, 64, n).astype(np.uint8)
    return np.asarray(_tx().sch_encode(fn, bsic), np.uint8), fn, bsic


def received(rng, o, bits, sps, profile, snr_db, delay_sym, nsym=156):
    """One burst's `nsym` symbols of received samples: the burst `delay_sym` symbols (any real number) into the window, through the
    profile's channel with noise."""
    s = o.modulate(bits.astype(np.int8), 68)                  # 148 + 68 symbols: enough behind the burst for any delay
    d = int(round(delay_sym * sps))
    s = np.r_[np.zeros(d, np.complex64), s]
    x = mlse_family.channel(rng, s, sps, mlse_family.PROFILES[profile], snr_db)
    return np.ascontiguousarray(x[:nsym * sps])


def static_family(sps, profile, snr_db, n, seed, spread=4, thresh=8.0):
    """n windows of one profile as a search cuts them: 172 symbols, the burst 12 +- spread whole symbols in (the detector needs room
    in front of the burst for a precursor and 148 symbols behind the TOA it finds): (oracle, bits [n, 148], fn, bsic, list of windows,
    amp [n], toa [n], detected [n]) with acquisition's SCH detector at `thresh` (8.0 is its default; no frequency shift)."""
    rng = np.random.default_rng(seed)
    det = detector(sps)
    o = det.o
    bits, fn, bsic = sch_bits(rng, n)
    xs, amp, toa, ok = [], [], [], []
    for b in range(n):
        x = received(rng, o, bits[b], sps, profile, snr_db, 12 + int(rng.integers(-spread, spread + 1)), 172)
        r = det.detect(x, None, thresh)
        xs.append(x); amp.append(r["amp"]); toa.append(r["toa"]); ok.append(bool(r["flags"] & 2))
    return o, bits, fn, bsic, xs, np.array(amp, np.complex64), np.array(toa, np.float32), np.array(ok, bool)


def _amp_toa(det, x, fallback_toa):
    r = det.detect(x, None)
    if (r["flags"] & 2) and r["amp"] != 0:
        return r["amp"], r["toa"]
    return np.complex64(800 - 300j), np.float32(fallback_toa)


@functools.lru_cache(maxsize=None)
def mixed_batch(sps, B, seed):
    """B SCH bursts for the parity tests: clean, noisy and multipath bursts in turn, 157- and 156-symbol lengths, every third burst
    at an odd sample offset, delays of 0..8 symbols (whole and fractional: the burst must lie inside the 156 symbols k_demod takes),
    amplitude and TOA from acquisition's SCH detector (a fixed pair where it finds nothing) with every fifth TOA moved off the 1/512
    grid.  Returns a dict with the packed batch and the model's results (computed once, shared)."""
    rng = np.random.default_rng(seed)
    det = detector(sps)
    o = det.o
    bits, fn, bsic = sch_bits(rng, B)
    kinds = [("flat", None), ("flat", 12.0), ("five", 15.0), ("precursor", 15.0), ("five", None), ("precursor", 8.0)]
    xs, amp, toa = [], [], []
    for b in range(B):
        prof, snr = kinds[b % len(kinds)]
        delay = [0.0, 7.0, 2.0, 8.0, 3.25, 0.5][(b // 2) % 6]
        x = received(rng, o, bits[b], sps, prof, snr, delay, 157 if b % 4 == 0 else 156)
        a, t = _amp_toa(det, x, delay * sps)
        if b % 5 == 4:
            t = np.float32(t + rng.uniform(-1.0 * sps, 1.0 * sps))
        xs.append(x); amp.append(a); toa.append(t)
    x, off, length = mlse_family.pack(xs, gaps=[1 if b % 3 == 0 else 2 for b in range(B)])
    amp = np.array(amp, np.complex64); toa = np.array(toa, np.float32)
    want = model.sch_batch(sps, x, off, length, amp, toa, oracle=o)
    return dict(sps=sps, bits=bits, fn=fn, bsic=bsic, x=x, off=off, length=length, amp=amp, toa=toa, want=want)


HOSTILE = ["plain", "zeros", "nan", "plain", "big", "short", "tiny_amp", "disabled", "inf", "plain", "p30", "toa_4096", "toa_-4096",
           "toa_past", "toa_nan", "plain", "len_91", "len_92", "len_odd", "plain"]


@functools.lru_cache(maxsize=None)
def hostile_batch(sps, seed=131):
    """tests/mlse_access_family.py's hostile set remade for SCH bursts and lengthened: all-zero samples, a NaN sample, a component of
    2^31 and one of 2^30 (after scaling by 1/amp), an infinity, 147, 92 and 91 symbols, a length that is no multiple of sps, a tiny
    caller-supplied amplitude, TOA = +-4096 exactly, one float beyond and NaN, d_enable == 0, between ordinary bursts, at odd and
    even sample offsets.  `kind` names each burst."""
    rng = np.random.default_rng(seed)
    det = detector(sps)
    o = det.o
    kind = list(HOSTILE)
    B = len(kind)
    bits, fn, bsic = sch_bits(rng, B)
    xs, amp, toa = [], [], []
    for b, k in enumerate(kind):
        x = received(rng, o, bits[b], sps, "five", 20.0, 2)
        a, t = _amp_toa(det, x, 2 * sps)
        if k == "zeros":
            x[:] = 0
        elif k == "nan":
            x[70 * sps + 1:71 * sps + 1] = np.complex64(complex(np.nan, 1.0))      # (sps samples in a row: one of them is a decimated instant)
        elif k == "big":
            x[60 * sps:61 * sps] = np.complex64(complex(1.0, 2.0 ** 31) * a)
        elif k == "p30":
            x[120 * sps:121 * sps] = np.complex64(complex(2.0 ** 30, 0.0) * a)
        elif k == "inf":
            x[30 * sps:31 * sps] = np.complex64(complex(-np.inf, 0.0))
        elif k == "short":
            x = x[:147 * sps]
        elif k == "len_91":
            x = x[:91 * sps]
        elif k == "len_92":
            x = x[:92 * sps]
        elif k == "len_odd":
            x = x[:155 * sps + (1 if sps > 1 else 0)]             # (at sps 1 every length is a multiple: an ordinary 155-symbol burst)
        elif k == "tiny_amp":
            a = np.complex64(1e-12 + 1e-12j)
        elif k == "toa_4096":
            t = F32(4096.0)
        elif k == "toa_-4096":
            t = F32(-4096.0)
        elif k == "toa_past":
            t = F32(np.nextafter(F32(4096.0), F32(np.inf)))
        elif k == "toa_nan":
            t = F32(np.nan)
        xs.append(x); amp.append(a); toa.append(t)
    x, off, length = mlse_family.pack(xs, gaps=[b % 2 for b in range(B)])
    amp = np.array(amp, np.complex64); toa = np.array(toa, np.float32)
    enable = np.array([k != "disabled" for k in kind], np.uint8)
    want = model.sch_batch(sps, x, off, length, amp, toa, enable=enable, oracle=o)
    return dict(sps=sps, kind=kind, bits=bits, x=x, off=off, length=length, amp=amp, toa=toa, enable=enable, want=want)


# ---- acquisition on the equalising leg -------------------------------------------------------------------------------------------
class MlseSchDetector(am.SchDetector):
    """tests/l1_acq_model.py's SCH detector with the equaliser in the demodulator's place (TRXSIG_SCHLEG_MLSE): flags, amp, toa and
    ptm are the parent's; on detection soft = the model on the same shifted window y[i0 : i0 + nd), amp and toa_b - i0, and the
    result carries the taps and the window word as well (zeros and 2 otherwise)."""

    def detect(self, x, omega, thresh=8.0):
        out = super().detect(x, omega, thresh)
        out["chan"] = np.zeros(5, np.complex64); out["win"] = model.WIN_SKIPPED
        if out["flags"] & 2:
            o, sps = self.o, self.sps
            x = np.asarray(x, np.complex64)
            n = len(x)
            y = x if omega is None else o.frequency_shift(x, F32(omega), 0.0)[0]
            fl0 = np.floor(out["toa"])
            i0 = int(fl0)
            nd = min(156 * sps, ((n - i0) // sps) * sps)
            r = model.sch_batch(sps, np.ascontiguousarray(y[i0:i0 + nd]), np.array([0]), np.array([nd]), np.array([out["amp"]], np.complex64),
                                np.array([F32(out["toa"] - F32(fl0))], F32), oracle=o)
            out.update(soft=r["soft"][0], chan=r["chan"][0], win=int(r["win"][0]))
        return out


# The search's channel: taps a symbol apart, three symbols of spread, no dominant tap; 12 dB.  Chosen on the CPU models
# (l1_acq_model.search_model with SchDetector and with MlseSchDetector) so that the equalising leg reaches state 15 on all four
# streams at sps 1 and 4 and the demodulating leg on fewer (1 and 2 of 4).  SEARCH_SCH_THRESH: at the default SCH threshold (8.0)
# NO tap set with this property was found (some 200 random draws and a dozen hand-made ones): the detector's valley rule counts the
# echoes 2 to 5 symbols beside the peak as noise, so peak-to-valley falls to 1.5 .. 9 under such spread (18 .. 37 on a flat channel)
# and stage 2 stops at state 3 on BOTH legs before either demodulates; wherever it passes 8 the demodulator's soft bits decode too.
# The search therefore runs with sch_thresh = 2.5 (peak-to-valley is 3.3 to 6.6 on these streams), an argument of trxsig_l1acq_search.
SEARCH_TAPS = (0.77j, -0.389 - 0.389j, -0.453 - 0.453j, 0.32j, 0.0)
SEARCH_SNR_DB = 12.0
SEARCH_SCH_THRESH = 2.5


def through_taps(x, sps, taps=SEARCH_TAPS):
    """A whole stream through a fixed tap set (taps a symbol apart), on the host: complex64, the stream's own length."""
    h = np.zeros((len(taps) - 1) * sps + 1, np.complex128)
    h[::sps] = np.asarray(taps, np.complex128)
    return np.convolve(np.asarray(x, np.complex128), h)[:len(x)].astype(np.complex64)


@functools.lru_cache(maxsize=None)
def search_streams(sps, n=4, snr_db=SEARCH_SNR_DB, taps=SEARCH_TAPS, seed=900):
    """n seeded C0 streams of tests/l1_acq_model.py (N_FRAMES frames; impair: a cut-in, a fractional delay, a carrier offset, a gain,
    noise), each then through the fixed tap set as a whole: [(x complex64, case)], all of one length."""
    o = detector(sps).o
    tx = _tx()
    cases = am.truth_cases(sps)[:n]
    out = []
    for i, case in enumerate(cases):
        rng = np.random.default_rng(seed + 10 * sps + i)
        clean, slots = am.build_stream(o, tx, rng, case["fn0"], am.N_FRAMES, case["bsic"])
        x = through_taps(am.impair(clean, rng, sps, case["cut"], case["frac8"], case["f"], case["gain"], snr_db), sps, taps)
        x = np.concatenate([x, np.zeros(len(clean) - len(x), np.complex64)])
        sch = [(fn, at - case["cut"] + case["frac8"] / 8.0) for fn, tn, kind, at in slots if kind == "sch"]
        out.append((x, dict(case, sch=sch)))
    return out


def decode(soft):
    """(ok, bsic, rfn) of the SCH decoder on one burst's soft bits."""
    return lrm.sch_decode(_tx(), np.asarray(soft, F32))
