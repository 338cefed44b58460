"""trxsig_trxgroup_add_l1tx (include/trxsig_l1tx.h): the downlink multiplexer's bursts into a Transceiver group's transmit queues
device to device, against the route through the host -- trxsig_l1tx_datagrams + trxsig_trxgroup_add_bursts.  Every test drives two
groups on one context by the same L1Tx encodes and the same calls: H is fed by datagrams() + add_bursts, D by add_l1tx.  After
every step trxsig_trxgroup_push's bits, gain and from-queue arrays are compared with np.array_equal and trxsig_trxgroup_tx_queue_size
(size and dropped flag) for every ARFCN: everything a caller can observe."""
import ctypes as C

import numpy as np
import pytest

import _pkg
import l1_mux_model as lmm
from test_gpu_l1tx import Content, gpu_call, grids, si_frames

pytestmark = pytest.mark.gpu
HYPER = lmm.HYPERFRAME
EINVAL = -1


@pytest.fixture(scope="module")
def pkg():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return _pkg.load()


@pytest.fixture(scope="module")
def ctx(pkg):
    c = pkg.TrxSig(4, 0)
    c.use_torch_stream()
    return c


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def datagram(tn, fn, rssi, bits):
    d = np.zeros(154, np.uint8)
    d[0] = tn
    d[1:5] = [(fn >> 24) & 255, (fn >> 16) & 255, (fn >> 8) & 255, fn & 255]
    d[5] = np.uint8(rssi & 255)
    d[6:] = bits
    return d


class Pair:
    """One L1Tx, its grids' source, and the two groups: H (through the host) and D (device to device)."""

    def __init__(self, pkg, ctx, comb, bsic=21, seed=1, si=True):
        self.pkg, self.ctx = pkg, ctx
        self.comb = np.ascontiguousarray(comb, np.uint8)
        self.A = self.comb.shape[0]
        rng = np.random.default_rng(seed)
        self.l1 = pkg.L1Tx(ctx, self.comb, bsic)
        self.model = lmm.MuxModel(self.comb, bsic, oracle=object())   # (only its walk of the mappings: the grids' shapes)
        if si:
            self.l1.set_si(si_frames(rng))
        self.content = Content(rng)
        self.H = pkg.TrxGroup(ctx, self.A, tsc_leg=pkg.TSCLEG_DEMOD)
        self.D = pkg.TrxGroup(ctx, self.A, tsc_leg=pkg.TSCLEG_DEMOD)
        self._keep = []

    def encode(self, fn, F, collect=False):
        """trxsig_l1tx_encode of frames [fn, fn + F); nothing synchronises unless the outputs are asked for"""
        g, _ = grids(self.model, self.content, fn, F)
        if collect:
            return gpu_call(self.pkg, self.l1, fn % HYPER, F, g)
        t = {k: (dev(v[0]), dev(v[1])) for k, v in g.items()}
        self._keep = (self._keep + [t])[-4:]
        self.l1.encode(fn % HYPER, F, t[lmm.TCH][0], t[lmm.TCH][1], t[lmm.XCCH][0], t[lmm.XCCH][1], t[lmm.CCCH][0], t[lmm.CCCH][1])
        return None

    def hand(self):
        """the last encode into both groups, each by its route; returns the number of bursts"""
        dg, ar = self.l1.datagrams()
        self.D.add_l1tx(self.l1)
        self.H.add_bursts(dg, ar)
        return len(dg)

    def both(self, fnc):
        return fnc(self.H), fnc(self.D)

    def same_push(self, fn, tn, n, what=""):
        import torch
        h = self.H.push(fn % HYPER, tn, n)
        d = self.D.push(fn % HYPER, tn, n)
        torch.cuda.synchronize()
        h = [x.cpu().numpy() for x in h]
        d = [x.cpu().numpy() for x in d]
        for name, x, y in zip(("bits", "gain", "from_queue"), h, d):
            assert np.array_equal(x, y), (what, name, fn, tn, n, np.argwhere(x != y)[:6])
        return d

    def same_queues(self, what=""):
        qs = []
        for a in range(self.A):
            h, d = self.both(lambda g: g.tx_queue_size(a))
            assert h == d, (what, a, h, d)
            qs.append(d)
        return qs

    def close(self):
        self.H.close(); self.D.close(); self.l1.destroy()


MIXED = np.array([[5, 1, 7, 1, 1, 0, 7, 1], [1, 1, 1, 1, 1, 1, 1, 1], [7, 0, 0, 1, 0, 0, 0, 0]], np.uint8)


def production_plan():
    comb = np.ones((128, 8), np.uint8)
    comb[0, 0], comb[0, 1] = 5, 7
    return comb


def test_small_mixed_plan(pkg, ctx):
    """The 3-ARFCN plan of test_datagrams_through_the_transmit_queue, 3 calls of 32 frames: D equals H, and D equals the encode
    itself -- from_queue exactly where d_what != 0, the encode's bits there, gain 1.0 on every queued slot."""
    p = Pair(pkg, ctx, MIXED, seed=5)
    fn, n_all = 2000, 0
    for call in range(3):
        F = 32
        r = p.encode(fn, F, collect=True)
        n_all += p.hand()
        p.same_queues(call)
        b, gain, fq = p.same_push(fn, 0, 8 * F, call)
        on = r["what"] != 0
        assert np.array_equal(fq != 0, on), call
        assert np.array_equal(b[on], r["bits"][on]), call
        assert (gain[on] == 1.0).all(), call
        assert all(q == (0, False) for q in p.same_queues(call)), call
        fn += F
    assert n_all > 1000
    p.close()


def test_production_plan(pkg, ctx):
    """128 ARFCNs x 32 frames x 4 steps; every second step is pushed in two halves: its ingest merges with the first push and the
    second push walks alone."""
    p = Pair(pkg, ctx, production_plan(), bsic=33, seed=3)
    fn = 123456
    for step in range(4):
        p.encode(fn, 32)
        n = p.hand()
        assert n > 30000, n
        if step % 2:
            _, _, fq0 = p.same_push(fn, 0, 128, step)
            p.same_queues(step)
            _, _, fq1 = p.same_push(fn + 16, 0, 128, step)
            assert int((fq0 != 0).sum() + (fq1 != 0).sum()) == n
        else:
            _, _, fq = p.same_push(fn, 0, 256, step)
            assert int((fq != 0).sum()) == n
        assert all(q == (0, False) for q in p.same_queues(step))
        fn += 32
    p.close()


def test_overflow_drops_the_same_bursts(pkg, ctx):
    """One 51-frame encode: a carrier with combination I on every timeslot (about 390 bursts for a queue of 256) beside a sparse
    one.  The same sizes, the same dropped flags -- set on the full carrier, clear on the sparse one -- and the same pushed bits over
    those 51 frames on both routes."""
    comb = np.array([[1] * 8, [1, 0, 0, 0, 0, 0, 0, 0]], np.uint8)
    p = Pair(pkg, ctx, comb, seed=9, si=False)
    fn = 5304 * 3
    r = p.encode(fn, 51, collect=True)
    on = r["what"] != 0
    assert on[0].sum() > 256 > on[1].sum() > 0
    p.hand()
    qs = p.same_queues()
    assert qs[0] == (256, True), qs                          # the full carrier: a prefix was accepted, the rest dropped
    assert qs[1] == (int(on[1].sum()), False), qs
    b, _, fq = p.same_push(fn, 0, 8 * 51)
    first = np.flatnonzero(on[0])[:256]                      # the accepted bursts are the FIRST 256 in (FN, TN) order
    want = np.zeros(8 * 51, bool)
    want[first] = True
    assert np.array_equal(fq[0] != 0, want)
    assert np.array_equal(b[0][want], r["bits"][0][want])
    assert np.array_equal(fq[1] != 0, on[1])
    qs = p.same_queues()
    assert qs[0] == (0, True) and qs[1] == (0, False), qs    # (the flag stays)
    p.close()


def test_encode_again_at_once(pkg, ctx):
    """encode(k), add_l1tx, encode(k + 1) with no synchronise in between, then the frames of k are pushed: D saw encode k's
    grid (H got its datagrams before the second encode)."""
    p = Pair(pkg, ctx, production_plan(), bsic=33, seed=4)
    fn = 40000
    for _ in range(2):                                       # (the first round sizes every workspace; the second runs without one allocation)
        p.encode(fn, 32)
        dg, ar = p.l1.datagrams()                            # H's copy of encode k
        p.D.add_l1tx(p.l1)
        p.encode(fn + 32, 32)                                # ... overwrites the grid at once
        p.H.add_bursts(dg, ar)
        _, _, fq = p.same_push(fn, 0, 256)
        assert int((fq != 0).sum()) == len(dg)
        p.hand()                                             # and encode k + 1 itself
        _, _, fq = p.same_push(fn + 32, 0, 256)
        assert int((fq != 0).sum()) > 30000
        p.same_queues()
        fn += 64
    p.close()


def test_ordering_paths(pkg, ctx):
    """An add behind an add (the earlier ingest is flushed), an add behind a queue-size query, and adds interleaved with host
    add_bursts of hand-made datagrams for other frames of the same ARFCNs."""
    p = Pair(pkg, ctx, MIXED, seed=6)
    rng = np.random.default_rng(60)
    fn = 7000
    # add, add (adjacent spans), one push
    p.encode(fn, 16); n0 = p.hand()
    p.encode(fn + 16, 16); n1 = p.hand()
    _, _, fq = p.same_push(fn, 0, 256, "add add")
    assert int((fq != 0).sum()) == n0 + n1
    fn += 32
    # add, queue size (flushes), push
    p.encode(fn, 16); n0 = p.hand()
    qs = p.same_queues("add size")
    assert sum(q[0] for q in qs) == n0
    _, _, fq = p.same_push(fn, 0, 128, "add size")
    assert int((fq != 0).sum()) == n0
    fn += 16
    # hand-made datagrams for the frames BEHIND and BEFORE the encode's span, the same ARFCNs, RSSI 10 (gain 0.1): before, between
    # and after two adds
    def hand_made(f0, nf):
        d, a = [], []
        for f in range(f0, f0 + nf):
            for arfcn in range(p.A):
                d.append(datagram(int(rng.integers(0, 8)), f, 10, rng.integers(0, 2, 148).astype(np.uint8)))
                a.append(arfcn)
        return np.stack(d), np.array(a, np.int32)
    hm = [hand_made(fn + 32, 4), hand_made(fn + 36, 4), hand_made(fn + 40, 4)]
    p.both(lambda g: g.add_bursts(*hm[0]))
    p.encode(fn, 16); n0 = p.hand()
    p.both(lambda g: g.add_bursts(*hm[1]))
    p.encode(fn + 16, 16); n1 = p.hand()
    p.both(lambda g: g.add_bursts(*hm[2]))
    _, gain, fq = p.same_push(fn, 0, 8 * 44, "interleaved")
    assert int((fq[:, :256] != 0).sum()) == n0 + n1
    assert (fq[:, 256:] != 0).sum() > 0 and np.isclose(gain[:, 256:][fq[:, 256:] != 0], 0.1).all()
    p.same_queues("interleaved")
    p.close()


def test_hyperframe_wrap_and_the_slow_path(pkg, ctx):
    """A span across the hyperframe wrap; then pushes that start 2^16 frames and more from the added frames (the pending ingest is
    launched alone, not taken into the push) and 2^17 and more (the packed queue entries' window is left: the workgroups walk the
    arrays in memory)."""
    p = Pair(pkg, ctx, MIXED, seed=7)
    fn = HYPER - 16
    r = p.encode(fn, 32, collect=True)
    n = p.hand()
    _, _, fq = p.same_push(fn, 0, 256, "wrap")
    assert np.array_equal(fq != 0, r["what"] != 0) and int((fq != 0).sum()) == n
    # far BEFORE the added frames: nothing is due, the walk takes the slow path with the bursts still queued
    fn = 400000
    p.encode(fn, 16); n = p.hand()
    _, _, fq = p.same_push(fn - (1 << 17) - 7, 3, 8, "far before")
    assert not fq.any()
    assert sum(q[0] for q in p.same_queues("far before")) == n
    _, _, fq = p.same_push(fn, 0, 128, "then on time")
    assert int((fq != 0).sum()) == n
    # 2^16 frames AFTER: every burst is stale on the push and goes to the filler table; then 2^17 after
    fn += 16
    for dist in ((1 << 16) + 3, (1 << 17) + 11):
        p.encode(fn, 16); n = p.hand()
        _, _, fq = p.same_push(fn + dist, 0, 8, ("far after", dist))
        assert not fq.any()
        assert all(q[0] == 0 for q in p.same_queues(("far after", dist)))
        p.same_push(fn + dist + 1, 0, 8 * 104, ("the filler table", dist))   # what the stale bursts left there
        fn += 16
    p.close()


def test_refusals(pkg, ctx):
    """Every TRXSIG_EINVAL of the contract leaves D's queues as they were; an all-empty encode is OK and changes nothing."""
    p = Pair(pkg, ctx, MIXED, seed=8)
    L = pkg.lib()
    fn = 9000
    p.encode(fn, 8); n = p.hand()                            # something in the queues to stay unchanged
    before = p.same_queues()
    assert sum(q[0] for q in before) == n

    def unchanged(what):
        assert p.same_queues(what) == before, what

    assert L.trxsig_trxgroup_add_l1tx(None, p.l1.h) == EINVAL
    assert L.trxsig_trxgroup_add_l1tx(p.D.h, None) == EINVAL
    unchanged("NULL")
    fresh = pkg.L1Tx(ctx, MIXED, 21)                         # no encode yet
    with pytest.raises(pkg.TrxSigError):
        p.D.add_l1tx(fresh)
    unchanged("no encode")
    fresh.destroy()
    other = pkg.L1Tx(ctx, MIXED[:2], 21)                     # another ARFCN count
    z = dev(np.zeros((64, 64, 33), np.uint8))
    other.encode(fn, 8, z, z, z, z, z, z)
    with pytest.raises(pkg.TrxSigError):
        p.D.add_l1tx(other)
    unchanged("n_arfcn")
    other.destroy()
    ctx2 = pkg.TrxSig(4, 0)                                  # another context
    ctx2.use_torch_stream()
    foreign = pkg.L1Tx(ctx2, MIXED, 21)
    foreign.encode(fn, 8, z, z, z, z, z, z)
    with pytest.raises(pkg.TrxSigError):
        p.D.add_l1tx(foreign)
    unchanged("context")
    foreign.destroy(); ctx2.close()
    # a staging block lent out and not yet added
    bits = np.ones(148, np.uint8)
    for g in (p.H, p.D):
        d, a = g.tx_staging(4)
        d[0] = datagram(2, fn + 20, 0, bits); a[0] = 1
    with pytest.raises(pkg.TrxSigError):
        p.D.add_l1tx(p.l1)
    p.both(lambda g: g.add_staged(1))                        # the block goes back; both groups got the one burst
    before[1] = (before[1][0] + 1, False)
    unchanged("staging")
    # an encode whose slots are all empty
    empty = pkg.L1Tx(ctx, np.zeros((3, 8), np.uint8), 21)
    empty.encode(fn, 8)
    assert not empty.collect(state=False)["what"].any()
    p.D.add_l1tx(empty)
    unchanged("all empty")
    empty.destroy()
    # and the good call still goes through
    _, _, fq = p.same_push(fn, 0, 8 * 24)
    assert int((fq != 0).sum()) == n + 1
    p.close()


def test_no_host_round_trip(pkg, ctx):
    """Structural check (the library's profiler hooks bracket kernels, they do not count host waits): the production step is run
    four times first, so that each of the group's three staging sets has its arrays; then the context's stream is given work that
    outlasts a host call by far -- 80 in-place passes over 1 GiB, 2 GiB of traffic each: tens of milliseconds, against the few
    microseconds a launch costs (tools/launch_bench.hip) -- and encode + add_l1tx must return while that stream is still busy.  A
    synchronise of the context's stream, or a copy to the host enqueued on it and waited for, would have drained it first."""
    import torch
    p = Pair(pkg, ctx, production_plan(), bsic=33, seed=2)
    fn = 60000
    for _ in range(4):
        p.encode(fn, 32)
        p.D.add_l1tx(p.l1)
        p.D.push(fn, 0, 256)
        fn += 32
    g, _ = grids(p.model, p.content, fn, 32)
    t = {k: (dev(v[0]), dev(v[1])) for k, v in g.items()}
    big = torch.ones(1 << 28, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    st = torch.cuda.current_stream()
    for _ in range(80):
        big.mul_(1.0001)
    assert st.query() is False, "the gap work ran out before the call: the check shows nothing"
    p.l1.encode(fn, 32, t[lmm.TCH][0], t[lmm.TCH][1], t[lmm.XCCH][0], t[lmm.XCCH][1], t[lmm.CCCH][0], t[lmm.CCCH][1])
    p.D.add_l1tx(p.l1)
    busy = st.query() is False
    b, _, fq = p.D.push(fn, 0, 256)                          # (enqueues only as well)
    still = st.query() is False
    torch.cuda.synchronize()
    assert busy, "trxsig_trxgroup_add_l1tx returned only after the context's stream had drained"
    assert still, "trxsig_trxgroup_push after the device add waited for the context's stream"
    assert int((fq != 0).sum().item()) > 30000               # and the step did its work
    del big
    p.close()
