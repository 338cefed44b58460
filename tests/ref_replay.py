"""Record / replay of the compiled reference's answers, for the tests that hold the CPU oracle against the REAL reference
library on seeded random inputs (tests/test_oracle_vs_ref.py, tests/test_fec_oracle.py).

Where oracle/_ref is built (`make -C oracle ref`, which needs the reference's sources) a test talks to the real library
through a Recorder: every call is forwarded and logged -- the method, a digest of its arguments and its result.  When the
test ends, the log must equal the test's fixture, tests/golden/ref_calls/<module>.<test>.npz, bit for bit; with
TRXSIG_RECORD_REF=1 in the environment the log is written there instead.  Everywhere else the test talks to a Replayer:
it answers the same calls, in the same order, with the recorded results, and checks each call's arguments against the
recorded digest.  The oracle's side of every comparison is computed either way, so the test compares the oracle with the
reference bit for bit whether or not the reference is present.

A test may name reference methods whose results the oracle reproduces with the same arguments (`derive`, e.g. modulate:
the input signals a test builds through the reference).  Of those calls only a 128-bit digest of the reference's result is
kept; a replay computes the result with the oracle and requires the recorded digest of it, so the fixtures stay small."""
import hashlib
import json
import os

import numpy as np
import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_calls")


def _feed(h, v):
    """Canonical bytes of a call's arguments: container shape, then each leaf's dtype, shape and bytes."""
    if isinstance(v, (list, tuple)):
        h.update(b"(%d" % len(v))
        for x in v:
            _feed(h, x)
    elif isinstance(v, dict):
        h.update(b"{%d" % len(v))
        for k in sorted(v):
            h.update(k.encode())
            _feed(h, v[k])
    elif isinstance(v, str):
        h.update(b"s" + v.encode())
    elif v is None:
        h.update(b"N")
    else:
        a = np.ascontiguousarray(v)
        h.update(a.dtype.str.encode() + repr(a.shape).encode() + a.tobytes())


def _digest(args, kw):
    h = hashlib.blake2b(digest_size=8)
    _feed(h, (list(args), kw))
    return h.hexdigest()


class _Digest:
    """Stands for a result that is kept as its digest only (a derived method's)."""

    def __init__(self, value):
        h = hashlib.blake2b(digest_size=16)
        _feed(h, value)
        self.hex = h.hexdigest()


_PY = {"bool": bool, "int": int, "float": float, "complex": complex}


def _pack(v, leaves):
    """A result as a JSON-able structure whose leaves are numpy arrays appended to `leaves` (types kept exactly)."""
    if isinstance(v, (tuple, list)):
        return {"t": type(v).__name__, "v": [_pack(x, leaves) for x in v]}
    if isinstance(v, dict):
        return {"t": "dict", "k": list(v), "v": [_pack(x, leaves) for x in v.values()]}
    if v is None:
        return {"t": "none"}
    if isinstance(v, _Digest):
        return {"t": "digest", "h": v.hex}
    if isinstance(v, np.ndarray):
        t = {"t": "arr"}
    elif isinstance(v, np.generic):
        t = {"t": "np"}
    elif type(v).__name__ in _PY:
        t = {"t": "py", "py": type(v).__name__}
    else:
        raise TypeError("cannot record a result of type %r" % type(v))
    leaves.append(np.asarray(v))
    t["i"] = len(leaves) - 1
    return t


def _unpack(s, leaves):
    t = s["t"]
    if t in ("tuple", "list"):
        r = [_unpack(x, leaves) for x in s["v"]]
        return tuple(r) if t == "tuple" else r
    if t == "dict":
        return {k: _unpack(x, leaves) for k, x in zip(s["k"], s["v"])}
    if t == "none":
        return None
    a = leaves[s["i"]]
    if t == "arr":
        return a.copy()
    return a[()] if t == "np" else _PY[s["py"]](a[()])


class _Recorder:
    def __init__(self, book, obj, tag, derive):
        self._book, self._obj, self._tag, self._derive = book, obj, tag, derive

    def __getattr__(self, name):
        attr = getattr(self._obj, name)
        if not callable(attr):
            return attr

        def call(*args, **kw):
            d = _digest(args, kw)
            r = attr(*args, **kw)
            self._book.log.append(("%s.%s" % (self._tag, name), d, _Digest(r) if name in self._derive else r))
            return r
        return call


class _Replayer:
    def __init__(self, book, tag, derive):
        self._book, self._tag, self._derive = book, tag, derive

    def __getattr__(self, name):
        def call(*args, **kw):
            s = self._book.replay("%s.%s" % (self._tag, name), _digest(args, kw))
            if name not in self._derive:
                return _unpack(s, self._book.leaves)
            r = self._derive[name](*args, **kw)
            assert s == {"t": "digest", "h": _Digest(r).hex}, "%s: %s differs from the reference's result" % (self._book.name, name)
            return r
        return call


class CallBook:
    """The reference objects of one test, live or replayed, and the log of their calls."""

    def __init__(self, name):
        self.name = name
        self.path = os.path.join(GOLDEN, name + ".npz")
        self.live = None
        self.log = []
        self.nobj = 0

    def _open(self, available, make, what, derive):
        live = bool(available())
        if self.live is None:
            self.live = live
            if not live:
                assert os.path.exists(self.path), "no fixture %s and no reference library to record one from" % self.path
                self.rec, self.leaves = _load(self.path)
                self.cursor = 0
        assert live == self.live, "%s: one test's reference objects must all be live or all be replayed" % self.name
        tag = "%s%d" % (what, self.nobj)
        self.nobj += 1
        derive = derive or {}
        return _Recorder(self, make(), tag, derive) if live else _Replayer(self, tag, derive)

    def sigproc(self, sps, variant="", derive=None):
        """refbind.Ref(sps, variant): the reference's sigProcLib (Transceiver/ or Transceiver52M/)."""
        import refbind
        return self._open(lambda: refbind.available(variant), lambda: refbind.Ref(sps, variant), "sigproc%s_%d_" % (variant, sps), derive)

    def fec(self, derive=None):
        """reffec.RefFec(): the reference's BitVector / ViterbiR2O4 / Parity code."""
        import reffec
        return self._open(reffec.available, reffec.RefFec, "fec", derive)

    def replay(self, method, digest):
        i = self.cursor
        assert i < len(self.rec), "%s: call %d (%s) was not recorded" % (self.name, i, method)
        m, d, s = self.rec[i]
        assert (m, d) == (method, digest), "%s: call %d is %s(%s), the fixture recorded %s(%s)" % (self.name, i, method, digest, m, d)
        self.cursor += 1
        return s

    def _packed(self):
        leaves = []
        calls = [(m, d, _pack(r, leaves)) for m, d, r in self.log]
        return calls, leaves

    def finish(self):
        if self.live is None:
            return
        if not self.live:
            assert self.cursor == len(self.rec), "%s: %d of the %d recorded calls were made" % (self.name, self.cursor, len(self.rec))
            return
        calls, leaves = self._packed()
        if os.environ.get("TRXSIG_RECORD_REF"):
            _save(self.path, calls, leaves)
            return
        assert os.path.exists(self.path), "%s: no fixture; record one with TRXSIG_RECORD_REF=1" % self.path
        rec, rec_leaves = _load(self.path)
        assert rec == json.loads(json.dumps(calls)), "%s: the calls differ from the fixture's" % self.name
        for i, (a, b) in enumerate(zip(leaves, rec_leaves)):
            assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), \
                "%s: result leaf %d differs from the fixture's" % (self.name, i)


def _save(path, calls, leaves):
    """One npz of two byte arrays: the JSON index (calls, and each leaf's dtype / shape) and the leaves' bytes end to end."""
    os.makedirs(os.path.dirname(path), exist_ok=True)
    index = json.dumps({"calls": calls, "leaves": [(a.dtype.str, a.shape) for a in leaves]}, separators=(",", ":"))
    blob = b"".join(np.ascontiguousarray(a).tobytes() for a in leaves)
    np.savez_compressed(path, index=np.frombuffer(index.encode(), np.uint8), blob=np.frombuffer(blob, np.uint8))


def _load(path):
    z = np.load(path)
    index = json.loads(z["index"].tobytes().decode())
    blob, leaves, pos = z["blob"].tobytes(), [], 0
    for dt, shape in index["leaves"]:
        dt = np.dtype(dt)
        n = dt.itemsize * int(np.prod(shape, dtype=np.int64))
        leaves.append(np.frombuffer(blob[pos:pos + n], dt).reshape(shape).copy())
        pos += n
    assert pos == len(blob), path
    return index["calls"], leaves


@pytest.fixture
def refs(request):
    """The test's CallBook; the log is checked (or written) when the test has passed."""
    book = CallBook("%s.%s" % (request.module.__name__.rsplit(".", 1)[-1], request.node.name))
    failed = request.session.testsfailed
    yield book
    if request.session.testsfailed == failed:
        book.finish()
