"""GPU parity of the downlink L1 encode (k_fec_tch_encode, k_fec_sch_encode) through the C-ABI: golden streams and SCH
bursts captured from the real reference's encoder steps, the literal-dispatch CPU oracle on random multi-channel streams,
state chaining across calls, the bad-input rules, and the closed loops encode -> modulate -> noise -> detect/demod ->
decode on the card.  Bit-exact."""
import numpy as np
import pytest

import _pkg
import fectxbind

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pkg():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return _pkg.load()


@pytest.fixture(scope="module")
def t(pkg):
    c = pkg.TrxSig(4, 0)
    c.use_torch_stream()
    return c


@pytest.fixture(scope="module")
def o():
    return fectxbind.FecTxOracle()


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def gpu_tch(t, kind, payload, tsc, state=None, poison=7):
    """One trxsig_fec_tch_encode_batch call -> (bits[S, n, 4, 148], state[S, 32]) on the host."""
    import torch
    S, n = kind.shape
    st = dev(np.zeros((S, 32), np.uint8) if state is None else state)
    bits = torch.full((S, n, 4, 148), poison, dtype=torch.uint8, device="cuda")
    t.fec_tch_encode(dev(kind.astype(np.uint8)), dev(payload.astype(np.uint8)), dev(np.asarray(tsc, np.uint8)), st, bits)
    torch.cuda.synchronize()
    return bits.cpu().numpy(), st.cpu().numpy()


def gpu_sch(t, fn, bsic):
    import torch
    bits = torch.full((len(fn), 148), 7, dtype=torch.uint8, device="cuda")
    t.fec_sch_encode(dev(np.asarray(fn, np.uint32).view(np.int32)), dev(np.asarray(bsic, np.uint8)), bits)
    torch.cuda.synchronize()
    return bits.cpu().numpy()


def random_stream(rng, S, n):
    kind = rng.integers(0, 3, (S, n)).astype(np.uint8)
    runs = rng.random((S, n)) < 0.3                          # runs of one kind next to each other
    kind[:, 1:][runs[:, 1:]] = kind[:, :-1][runs[:, 1:]]
    return kind, rng.integers(0, 256, (S, n, 33)).astype(np.uint8), rng.integers(0, 8, S).astype(np.uint8)


def test_golden_tch_and_sch(t, golden):
    """Bit-exact against the reference's dispatch() streams (its filler set) and its generate() SCH bursts; the stream is
    also sent as two calls with the state carried in between."""
    g = golden("fec_tx.npz")
    t.fec_tch_set_filler(g["filler"])
    try:
        kind, pl, tsc = g["tch_kind"], g["tch_payload"], g["tch_tsc"]
        bits, _ = gpu_tch(t, kind, pl, tsc)
        assert np.array_equal(bits, g["tch_bits"])
        k = int(g["tch_split"])
        b1, s1 = gpu_tch(t, kind[:, :k], pl[:, :k], tsc)
        b2, _ = gpu_tch(t, kind[:, k:], pl[:, k:], tsc, state=s1)
        assert np.array_equal(np.concatenate([b1, b2], axis=1), g["tch_bits"])
    finally:
        t.fec_tch_set_filler(np.zeros(456, np.uint8))
    assert np.array_equal(gpu_sch(t, g["sch_fn"], g["sch_bsic"]), g["sch_bits"])


@pytest.mark.parametrize("n", [1, 2, 3, 63, 64, 65, 257])
def test_random_streams_vs_oracle(t, o, n):
    """Random multi-channel streams (random kinds incl. bad ones, per-channel TSC, random filler, random starting state):
    bursts and final state equal the literal dispatch() of the oracle."""
    rng = np.random.default_rng(1000 + n)
    filler = rng.integers(0, 2, 456).astype(np.uint8)
    t.fec_tch_set_filler(filler)
    try:
        for S in (1, 5, 33):
            kind, pl, tsc = random_stream(rng, S, n)
            kind[rng.random((S, n)) < 0.03] = 3 + rng.integers(0, 250)            # a few kinds above 2
            _, st0 = o.tch_encode_stream(*random_stream(rng, S, 3)[:2], tsc, filler)  # a state some stream left behind
            st0[: S // 2] = 0
            want_b, want_s = o.tch_encode_stream(kind, pl, tsc, filler, state=st0)
            got_b, got_s = gpu_tch(t, kind, pl, tsc, state=st0)
            assert np.array_equal(got_b, want_b), (S, n)
            assert np.array_equal(got_s, want_s), (S, n)
    finally:
        t.fec_tch_set_filler(np.zeros(456, np.uint8))


def test_chaining_invariance(t, o):
    """One call of n blocks equals k calls of n/k with the state carried in place on the device."""
    import torch
    rng = np.random.default_rng(5)
    S, n = 9, 48
    kind, pl, tsc = random_stream(rng, S, n)
    whole, s_whole = gpu_tch(t, kind, pl, tsc)
    for k in (2, 3, 4, 6, 16, 48):
        st = torch.zeros(S, 32, dtype=torch.uint8, device="cuda")
        parts = []
        for c in range(k):
            sl = slice(c * n // k, (c + 1) * n // k)
            b = torch.full((S, n // k, 4, 148), 7, dtype=torch.uint8, device="cuda")
            t.fec_tch_encode(dev(kind[:, sl]), dev(pl[:, sl]), dev(tsc), st, b)
            parts.append(b)
        torch.cuda.synchronize()
        assert np.array_equal(torch.cat(parts, dim=1).cpu().numpy(), whole), k
        assert np.array_equal(st.cpu().numpy(), s_whole), k
    assert np.array_equal(whole, o.tch_encode_stream(kind, pl, tsc, np.zeros(456, np.uint8))[0])


def test_bad_inputs(pkg, t, o):
    """A TSC above 7 gives zero bursts and leaves the channel's state untouched; a kind above 2 is an all-zero c[] that
    is not stolen; host argument checks return TRXSIG_EINVAL before any launch; empty batches are no-ops."""
    import torch
    rng = np.random.default_rng(9)
    S, n = 4, 6
    kind, pl, _ = random_stream(rng, S, n)
    kind[0, 2] = 200; kind[1, 2] = 200; kind[2, :] = 3
    tsc = np.array([2, 8, 4, 255], np.uint8)
    st0 = rng.integers(0, 256, (S, 32)).astype(np.uint8)
    st0[:, 29] &= 1
    st0[:, 28] &= 0x0f; st0[:, 30:] = 0
    bits, st = gpu_tch(t, kind, pl, tsc, state=st0)
    assert not bits[1].any() and not bits[3].any()
    assert np.array_equal(st[1], st0[1]) and np.array_equal(st[3], st0[3])
    want_b, want_s = o.tch_encode_stream(kind, pl, tsc, np.zeros(456, np.uint8), state=st0)
    assert np.array_equal(bits, want_b) and np.array_equal(st, want_s)
    assert not bits[0, 2, :, 87].any() and not bits[0, 3, :, 60].any()                 # bad kind: not stolen
    # channel 2 is all bad kinds: the e-bits are zero from block 1 on (block 0 carries the old state's odd half)
    assert not bits[2, 1:, :, 3:60].any() and not bits[2, 1:, :, 88:145].any() and not st[2].any()
    L = pkg.lib()
    p = lambda x: x.data_ptr()
    k1 = torch.zeros(4, dtype=torch.uint8, device="cuda"); big = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    assert L.trxsig_fec_tch_encode_batch(t.h, 0, 5, None, None, None, None, None) == 0
    assert L.trxsig_fec_tch_encode_batch(t.h, 5, 0, None, None, None, None, None) == 0
    assert L.trxsig_fec_tch_encode_batch(t.h, -1, 1, p(k1), p(big), p(k1), p(big), p(big)) == pkg.lib().trxsig_fec_tch_encode_batch(t.h, 1, -1, p(k1), p(big), p(k1), p(big), p(big)) == -1
    assert L.trxsig_fec_tch_encode_batch(t.h, 1 << 20, 1 << 12, p(k1), p(big), p(k1), p(big), p(big)) == -1   # 2^32 blocks
    for i in range(5):
        a = [p(k1), p(big), p(k1), p(big), p(big)]
        a[i] = None
        assert L.trxsig_fec_tch_encode_batch(t.h, 1, 1, *a) == -1, i
    assert L.trxsig_fec_tch_set_filler(t.h, None) == -1
    assert L.trxsig_fec_sch_encode_batch(t.h, None, None, 0, None) == 0
    assert L.trxsig_fec_sch_encode_batch(t.h, p(big), p(k1), -1, p(big)) == -1
    assert L.trxsig_fec_sch_encode_batch(t.h, None, p(k1), 1, p(big)) == -1
    assert L.trxsig_fec_sch_encode_batch(t.h, p(big), p(k1), 1, None) == -1
    assert b"bad argument" in L.trxsig_last_error(t.h)
    torch.cuda.synchronize()


def test_unaligned_output(t, o):
    """Output buffers that are not 16- (TCH) or 4-byte (SCH) aligned take the byte-store form: same bits."""
    import torch
    rng = np.random.default_rng(3)
    S, n = 3, 5
    kind, pl, tsc = random_stream(rng, S, n)
    raw = torch.full((S * n * 592 + 1,), 7, dtype=torch.uint8, device="cuda")
    st = torch.zeros(S, 32, dtype=torch.uint8, device="cuda")
    t.fec_tch_encode(dev(kind), dev(pl), dev(tsc), st, raw[1:])
    fn = rng.integers(0, 2715648, 9).astype(np.uint32); bs = rng.integers(0, 64, 9).astype(np.uint8)
    raw2 = torch.full((9 * 148 + 1,), 7, dtype=torch.uint8, device="cuda")
    t.fec_sch_encode(dev(fn.view(np.int32)), dev(bs), raw2[1:])
    torch.cuda.synchronize()
    assert np.array_equal(raw[1:].cpu().numpy().reshape(S, n, 4, 148), o.tch_encode_stream(kind, pl, tsc, np.zeros(456, np.uint8))[0])
    assert np.array_equal(raw2[1:].cpu().numpy().reshape(9, 148), o.sch_encode(fn, bs))


def test_closed_loop_speech_and_facch(pkg, t):
    """Speech and FACCH blocks -> TCH encode -> GMSK modulate -> noise -> TSC detect + demodulate -> TCH decode, all on
    the card: every speech frame comes back good and equal, `stolen` marks exactly the FACCH blocks, and the FACCH
    frames decode ok and equal."""
    import torch
    sps, tsc, n = 4, 3, 256
    rng = np.random.default_rng(21)
    kind = np.where(rng.random(n) < 0.25, pkg.TCH_FACCH, pkg.TCH_SPEECH).astype(np.uint8)
    pl = rng.integers(0, 256, (n, 33)).astype(np.uint8)
    pl[:, 32] &= 0xF0                                       # d[260..263] do not exist: the decoder writes them as zero
    bits = torch.zeros(1, n, 4, 148, dtype=torch.uint8, device="cuda")
    st = torch.zeros(1, 32, dtype=torch.uint8, device="cuda")
    t.fec_tch_encode(dev(kind[None]), dev(pl[None]), dev(np.array([tsc], np.uint8)), st, bits)
    B = 4 * n
    bits = bits.view(B, 148)
    g = torch.Generator(device="cuda"); g.manual_seed(12)
    guard = torch.full((B,), 8, dtype=torch.int32, device="cuda")
    ns = sps * 156
    off = (torch.arange(B, dtype=torch.int32, device="cuda") * ns).contiguous()
    length = torch.full((B,), ns, dtype=torch.int32, device="cuda")
    x = torch.zeros(B * ns, 2, dtype=torch.float32, device="cuda")
    t.modulate(bits, guard, x, off)
    x += 0.15 * torch.randn(x.shape, device="cuda", generator=g)
    flags = torch.zeros(B, dtype=torch.uint8, device="cuda"); amp = torch.zeros(B, 2, device="cuda"); toa = torch.zeros(B, device="cuda")
    soft = torch.zeros(B, 148, device="cuda")
    t.detect_demod_normal(x, off, length, tsc, flags, amp, toa, soft, nsoft=148, soft_stride=148)
    # the decoder's block m spans bursts 4m .. 4m+7: encoded block m (its odd half rides in block m+1's bursts)
    nb = n - 1
    tch = torch.zeros(nb, 33, dtype=torch.uint8, device="cuda"); good = torch.zeros(nb, dtype=torch.uint8, device="cuda")
    stolen = torch.zeros(nb, dtype=torch.uint8, device="cuda")
    facch = torch.zeros(nb, 23, dtype=torch.uint8, device="cuda"); fok = torch.zeros(nb, dtype=torch.uint8, device="cuda")
    t.fec_tch_decode(soft, B, tch, good, stolen, facch=facch, facch_ok=fok, wire=True)
    torch.cuda.synchronize()
    assert bool(((flags & pkg.F_DETECT) != 0).all())
    k = kind[:nb]
    sp, fa = k == pkg.TCH_SPEECH, k == pkg.TCH_FACCH
    assert np.array_equal(stolen.cpu().numpy().astype(bool), fa)
    assert good.cpu().numpy()[sp].all() and np.array_equal(tch.cpu().numpy()[sp], pl[:nb][sp])
    assert fok.cpu().numpy()[fa].all() and np.array_equal(facch.cpu().numpy()[fa], pl[:nb, :23][fa])


def test_sch_vs_oracle_and_round_trip(t, o):
    """Random FN and BSIC against the oracle; invalid FN / BSIC give zero bursts; the 78 e-bits through the generic
    Viterbi decoder give back u[39]: the fields, a zero parity remainder and zero tail bits."""
    import torch
    rng = np.random.default_rng(31)
    H = 2715648
    fn = rng.integers(0, H, 4099).astype(np.uint32); bsic = rng.integers(0, 64, 4099).astype(np.uint8)
    fn[:5] = [H, H + 1, 0xFFFFFFFF, 5, 6]; bsic[3:5] = [64, 255]
    got = gpu_sch(t, fn, bsic)
    assert np.array_equal(got, o.sch_encode(fn, bsic))
    assert not got[:5].any() and got[5:, 42:106].any()
    v = slice(5, None)
    e = np.concatenate([got[v, 3:42], got[v, 106:145]], axis=1).astype(np.float32)
    u = torch.zeros(e.shape[0], 39, dtype=torch.uint8, device="cuda")
    t.fec_viterbi(dev(e), 78, e.shape[0], u)
    torch.cuda.synchronize()
    u = u.cpu().numpy()
    assert not u[:, 35:].any()
    for i in range(0, u.shape[0], 7):
        par = o.parity(0x0575, 10, u[i, :25])
        sent = int("".join(map(str, u[i, 25:35])), 2)
        assert (par ^ sent) == 0x3ff                        # inverted parity word: remainder of d[] + ~p[] is zero
        d = o.lsb8msb(u[i, :25])
        f = int(fn[5 + i]); val = int("".join(map(str, d)), 2)
        assert val >> 19 == bsic[5 + i]
        assert (val >> 8) & 2047 == (f // 1326) % 2048 and (val >> 3) & 31 == f % 26
        assert val & 7 == ((f % 51 - 1) % (1 << 32)) // 10 & 7
