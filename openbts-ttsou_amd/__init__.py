"""openbts-ttsou_amd: MI355X-native burst processing for the OpenBTS software transceiver.

The product is the C-ABI shared library `libtrxsig.so` (include/trxsig.h; sources in csrc/).  This
Python module is plumbing only: a ctypes binding used by tests/ and bench.py to hand torch device
buffers and streams to the library.  There is no CPU fallback anywhere in this package: loading
fails loudly if the library is missing, and creating a context fails without a gfx950 GPU.
"""
import ctypes as C
import os
import subprocess

from ._abi import (TrxSigError, bind, C32, TrxGroupResult, L1RxOut, L1TxIn, L1TxOut, L1MsIn, L1MsOut, L1MsAir,  # noqa: F401
                   L1MsRxOut, L1AcqOut, AirCellParams, AirStreamParams, L1TrkView, L1TrkMeas)
from ._abi_l1pdch import L1PdchIn, L1PdchOut, L1PdchDec  # noqa: F401
from ._abi_l1pacc import L1PaccIn, L1PaccOut, L1PaccDet  # noqa: F401

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("TRXSIG_LIB", os.path.join(_HERE, "libtrxsig.so"))   # TRXSIG_LIB: tuning builds

F_ENERGY, F_DETECT, F_BADLEN = 1, 2, 128
SOFT_EXACT, SOFT_TOLERANCE = 0, 1                # trxsig_set_soft_mode
ABI_VERSION = 2                                  # TRXSIG_ABI_VERSION of include/trxsig.h
IRC_LOADING = 1.0 / 64.0                         # the diagonal loading the tools and the groups use (trxsig_mlse_irc_batch)
TCH_FILLER, TCH_SPEECH, TCH_FACCH = 0, 1, 2      # block kinds of trxsig_fec_tch_encode_batch
TCH_TX_STATE_BYTES = 32                          # TRXSIG_TCH_TX_STATE_BYTES
FEC_DECODED, FEC_STOLEN, FEC_FACCH_OK, FEC_TCH_GOOD = 1, 2, 4, 8   # status bits of the stream decoders (TRXSIG_FEC_*)
TCH_RX_STATE_BYTES, XCCH_RX_STATE_BYTES = 3664, 1840              # TRXSIG_TCH_RX_STATE_BYTES, TRXSIG_XCCH_RX_STATE_BYTES
CS1, CS2, CS3, CS4 = 0, 1, 2, 3                  # TRXSIG_CS1..TRXSIG_CS4: the GPRS coding schemes of pdtch_encode / pdtch_decode
PDTCH_BLOCK_BYTES = 54                           # TRXSIG_PDTCH_BLOCK_BYTES
ACCESS_8, ACCESS_11 = 0, 1                       # TRXSIG_ACCESS_8 / _11: the access burst's formats of access_encode / access_decode


def build(verbose=False):
    """Compile csrc/ into libtrxsig.so for gfx950 (hipcc cross-compiles without a GPU)."""
    cmd = ["make", "-j8", "-C", os.path.join(_HERE, "csrc")]
    if not verbose:
        cmd.insert(1, "-s")
    subprocess.check_call(cmd)
    return LIB_PATH


TUNE_LIB_PATH = os.path.join(_HERE, "libtrxsig_tune.so")
_lib = None
_libs = {}


def tune_lib():
    """libtrxsig_tune.so: the product's code plus the alternates that measured slower (trxsig_set_tuning) -- for A/B
    measurements and the tests that keep those alternates bit-identical.  Same C-ABI; both libraries can be loaded at once
    (linked -Bsymbolic)."""
    return lib(TUNE_LIB_PATH)


def lib(path=None):
    """The loaded libtrxsig.so.  torch (if used) must be imported first so that the library binds to
    the HIP runtime torch already loaded (same libamdhip64.so.7 soname) and device pointers are
    shared between the two."""
    global _lib
    if path is not None:
        if path not in _libs:
            _libs[path] = _load(path)
        return _libs[path]
    if _lib is None:
        _lib = _load(LIB_PATH)
    return _lib


def _load(path):
    if not os.path.exists(path):
        raise TrxSigError("%s not built: run `python -c 'import __graft_entry__ as g; g.build()'` "
                          "or `make -C openbts-ttsou_amd/csrc` (there is no CPU fallback)" % os.path.basename(path))
    L = C.CDLL(path, mode=C.RTLD_GLOBAL)
    if hasattr(L, "trxsig_abi_version") and L.trxsig_abi_version() != ABI_VERSION:   # (said before a symbol of the other ABI is missed)
        raise TrxSigError("%s speaks ABI %d, this binding was written for %d" % (path, L.trxsig_abi_version(), ABI_VERSION))
    return bind(L, path)


def tables_dtype():
    """numpy view of the TrxTables blob (csrc/trxsig_tables.h)."""
    import numpy as np
    return np.dtype([("magic", "<u4"), ("version", "<u4"), ("sps", "<u4"), ("bytes", "<u4"), ("checksum", "<u4"),
                     ("pad0", "<u4", 3), ("cosT", "<f4", 1028), ("sinT", "<f4", 1028), ("rot", "<c8", 628),
                     ("rev", "<c8", 628), ("pulse", "<f4", 12), ("mid", "<c8", (8, 64)), ("mid_toa", "<f4", 8),
                     ("mid_gain", "<c8", 8), ("rach", "<c8", 164), ("rach_toa", "<f4"), ("pad1", "<f4"),
                     ("rach_gain", "<c8"), ("mid_ctap", "<c8", (8, 16)), ("pad2", "<f4", 16),
                     ("sinc_grid", "<f4", (512, 32))])


def build_tables_host(sps):
    """The constant-table blob built on the host (no device needed): uint8 array."""
    import numpy as np
    n = lib().trxsig_tables_bytes(sps)
    buf = np.zeros(n, np.uint8)
    rc = lib().trxsig_tables_build_host(sps, buf.ctypes.data, n)
    if rc != 0:
        raise TrxSigError("trxsig_tables_build_host(%d) failed (%d)" % (sps, rc))
    return buf


def tables_valid(blob):
    """True if a host uint8 array holds a valid table blob (header + checksum)."""
    return lib().trxsig_tables_validate_host(blob.ctypes.data, blob.size) == 0


def _ptr(t):
    """torch tensor / int / None -> device address."""
    if t is None:
        return None
    if isinstance(t, int):
        return t
    return t.data_ptr()


class _DevView:
    """A device buffer owned by the library, presented to torch (zero copy) through __cuda_array_interface__."""

    def __init__(self, ptr, shape, typestr):
        self.__cuda_array_interface__ = dict(data=(int(ptr), False), shape=tuple(shape), typestr=typestr, version=2)


def _dev_tensor(ctx, ptr, shape, typestr):
    """A device buffer owned by the library as a torch tensor on the context's device (a view: no copy)."""
    import torch
    return torch.as_tensor(_DevView(ptr, shape, typestr), device="cuda:%d" % ctx.device)


def _to_host(ctx, ptr, shape, typestr):
    """The same buffer as a host numpy array; zeros of that shape where there is nothing to read (no pointer, or no elements)."""
    import numpy as np
    if ptr is None or int(np.prod(shape)) == 0:
        return np.zeros(shape, np.dtype(typestr))
    return _dev_tensor(ctx, ptr, shape, typestr).cpu().numpy()


def _fill(struct, names, tensors, itemsize=None, empty_as_one=False):
    """Optional device tensors into a struct of device pointers (names: its fields, None: every pointer field in order); a None
    tensor leaves its field NULL.  itemsize: what an element of each must measure.  empty_as_one: an empty tensor is "given, no rows"
    (the address 1) and not NULL.  Returns the tensors, which the caller keeps alive while the launch may read them."""
    if names is None:
        names = [n for n, t in struct._fields_ if t is C.c_void_p]
    for name, t in zip(names, tensors):
        if t is not None:
            assert t.is_contiguous() and (itemsize is None or t.element_size() == itemsize)
            setattr(struct, name, 1 if empty_as_one and not t.numel() else t.data_ptr())
    return tuple(tensors)


class _Object:
    """A library object made on a context by <_prefix>_create and released by <_prefix>_destroy.  Calls raise on rc < 0 with the
    context's last error and return rc; destroy() is idempotent and runs at collection."""
    _prefix = None

    def __init__(self, ctx):
        import numpy as np
        self.np = np
        self.ctx = ctx
        self.L = ctx.L
        self.h = C.c_void_p()

    def _create(self, *args, name="create"):
        name = "%s_%s" % (self._prefix, name)
        rc = getattr(self.L, name)(C.byref(self.h), self.ctx.h, *args)
        if rc != 0:
            raise TrxSigError("%s failed (%d): %s" % (name, rc, self._last_error()))

    def destroy(self):
        if self.h:
            getattr(self.L, self._prefix + "_destroy")(self.h); self.h = None

    def __del__(self):
        try:
            self.destroy()
        except Exception:
            pass

    def _last_error(self):
        return self.L.trxsig_last_error(self.ctx.h).decode()

    def _chk(self, rc, what):
        if rc < 0:
            raise TrxSigError("%s: %d (%s)" % (what, rc, self._last_error()))
        return rc

    def _call(self, name, *args):
        name = "%s_%s" % (self._prefix, name)
        return self._chk(getattr(self.L, name)(self.h, *args), name)


class _PlanView(_Object):
    """An object built on a channel plan (comb: uint8 [n_arfcn, 8] in the CMD SETSLOT numbering -- 0 none, 1 = I, 5 = V on ARFCN 0
    TN 0, 7 = VII): its channels per class, where each lies, and the device array of their state records."""

    def __init__(self, ctx, comb, *args):
        super().__init__(ctx)
        self.comb = self.np.ascontiguousarray(comb, self.np.uint8)
        self._create(self.comb.shape[0], self.comb.ctypes.data, *args)

    def channels(self, cls):
        return self._call("channels", cls)

    def channel(self, cls, chan):
        """(arfcn, tn, kind, sub) of a channel"""
        v = [C.c_int() for _ in range(4)]
        self._call("channel", cls, chan, *[C.byref(x) for x in v])
        return tuple(x.value for x in v)

    def state(self, cls):
        p = C.c_void_p()
        self._call("state", cls, C.byref(p))
        return p.value


class _PlanObject(_PlanView):
    """A plan object whose channels are opened and closed one by one (what that means: each class's docstring)."""

    def open(self, cls, chan):
        self._call("open", cls, chan)

    def close(self, cls, chan):
        self._call("close", cls, chan)


class TrxSig:
    """One library context = one GPU + one stream (trxsig.h)."""

    def __init__(self, sps=4, device=0, tables_blob=None, tuning=False):
        self.L = tune_lib() if tuning else lib()
        self.h = C.c_void_p()
        if tables_blob is None:
            rc = self.L.trxsig_create(C.byref(self.h), device, sps)
        else:
            rc = self.L.trxsig_create_from_tables(C.byref(self.h), device, _ptr(tables_blob),
                                                  tables_blob.numel() * tables_blob.element_size())
        if rc != 0:
            raise TrxSigError("trxsig_create failed (%d): no gfx950 device or bad arguments; "
                              "this library has no CPU fallback" % rc)
        self.sps = self.L.trxsig_sps(self.h)
        self.device = device

    def close(self):
        if self.h:
            self.L.trxsig_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc, what):
        if rc != 0:
            raise TrxSigError("%s failed (%d): %s" % (what, rc, self.L.trxsig_last_error(self.h).decode()))

    def set_stream(self, stream_handle):
        self._chk(self.L.trxsig_set_stream(self.h, stream_handle), "trxsig_set_stream")

    def use_torch_stream(self):
        import torch
        self.set_stream(torch.cuda.current_stream(self.device).cuda_stream)

    def synchronize(self):
        self._chk(self.L.trxsig_synchronize(self.h), "trxsig_synchronize")

    def reserve(self, max_bursts):
        self._chk(self.L.trxsig_reserve(self.h, max_bursts), "trxsig_reserve")

    def tables_bytes(self):
        return self.L.trxsig_tables_bytes(self.sps)

    def tables_device_ptr(self):
        return self.L.trxsig_tables_device(self.h)

    def tables_export(self):
        import numpy as np
        buf = np.zeros(self.tables_bytes(), np.uint8)
        self._chk(self.L.trxsig_tables_export(self.h, buf.ctypes.data, buf.size), "trxsig_tables_export")
        return buf

    def detect_demod_normal(self, samples, offset, length, tsc, flags, amp, toa, soft, avgpwr=None, hard=None,
                            detect_thresh=3.0, energy_thresh=0.0, nsoft=148, soft_stride=None):
        B = offset.numel() if hasattr(offset, "numel") else len(offset)
        if soft_stride is None:
            soft_stride = soft.shape[-1] if soft is not None and hasattr(soft, "shape") else nsoft
        self._chk(self.L.trxsig_detect_demod_normal_batch(
            self.h, _ptr(samples), _ptr(offset), _ptr(length), B, tsc, detect_thresh, energy_thresh,
            _ptr(flags), _ptr(amp), _ptr(toa), _ptr(avgpwr), _ptr(soft), _ptr(hard), nsoft, soft_stride),
            "trxsig_detect_demod_normal_batch")

    def detect_demod_rach(self, samples, offset, length, flags, amp, toa, soft, avgpwr=None, hard=None,
                          detect_thresh=5.0, energy_thresh=0.0, nsoft=148, soft_stride=None):
        B = offset.numel() if hasattr(offset, "numel") else len(offset)
        if soft_stride is None:
            soft_stride = soft.shape[-1] if soft is not None and hasattr(soft, "shape") else nsoft
        self._chk(self.L.trxsig_detect_demod_rach_batch(
            self.h, _ptr(samples), _ptr(offset), _ptr(length), B, detect_thresh, energy_thresh,
            _ptr(flags), _ptr(amp), _ptr(toa), _ptr(avgpwr), _ptr(soft), _ptr(hard), nsoft, soft_stride),
            "trxsig_detect_demod_rach_batch")

    def detect_demod_host(self, x, off, length, tsc=None, detect_thresh=None, energy_thresh=0.0, nsoft=148):
        """Host-buffer convenience call (numpy in/out, PCIe-inclusive): tsc=None -> RACH path."""
        import numpy as np
        x = np.ascontiguousarray(x, np.complex64); off = np.ascontiguousarray(off, np.int32)
        length = np.ascontiguousarray(length, np.int32)
        B = len(off)
        flags = np.zeros(B, np.uint8); amp = np.zeros(B, np.complex64); toa = np.zeros(B, np.float32)
        pwr = np.zeros(B, np.float32); soft = np.zeros((B, nsoft), np.float32)
        a = lambda v: v.ctypes.data
        if tsc is None:
            rc = self.L.trxsig_detect_demod_rach_host(self.h, a(x), a(off), a(length), B,
                                                      5.0 if detect_thresh is None else detect_thresh, energy_thresh,
                                                      a(flags), a(amp), a(toa), a(pwr), a(soft), nsoft, nsoft)
        else:
            rc = self.L.trxsig_detect_demod_normal_host(self.h, a(x), a(off), a(length), B, tsc,
                                                        3.0 if detect_thresh is None else detect_thresh,
                                                        energy_thresh, a(flags), a(amp), a(toa), a(pwr), a(soft),
                                                        nsoft, nsoft)
        self._chk(rc, "trxsig_detect_demod_*_host")
        return dict(flags=flags, amp=amp, toa=toa, pwr=pwr, soft=soft)

    def demodulate(self, samples, offset, length, amp, toa, soft, enable=None, hard=None, nsoft=148,
                   soft_stride=None):
        B = offset.numel()
        if soft_stride is None:
            soft_stride = soft.shape[-1]
        self._chk(self.L.trxsig_demodulate_batch(self.h, _ptr(samples), _ptr(offset), _ptr(length), B, _ptr(amp),
                                                 _ptr(toa), _ptr(enable), _ptr(soft), _ptr(hard), nsoft,
                                                 soft_stride), "trxsig_demodulate_batch")

    def _mlse(self, name, offset, head, tail, soft=None, nsoft=None, soft_stride=None):
        """One sequence-equaliser call: self.L.<name>(handle, *head, B, *tail[, nsoft, soft_stride]) with B = offset's element
        count and soft_stride = soft's row length unless given (nsoft None: the call has no soft bits); arrays go as device
        addresses, numbers as they are."""
        B = offset.numel() if hasattr(offset, "numel") else len(offset)
        if nsoft is not None:
            tail += (nsoft, soft.shape[-1] if soft_stride is None else soft_stride)
        self._chk(getattr(self.L, name)(self.h, *[_ptr(a) if hasattr(a, "data_ptr") else a for a in head + (B,) + tail]), name)

    def mlse(self, samples, offset, length, tsc, amp, toa, soft, enable=None, chan=None, win=None, hard=None, nsoft=148,
             soft_stride=None):
        """The sequence equaliser with the caller's amp / TOA (trxsig_mlse_batch): chan [B, 5] complex, win [B] int32."""
        self._mlse("trxsig_mlse_batch", offset, (samples, offset, length), (tsc, amp, toa, enable, chan, win, soft, hard), soft, nsoft,
                   soft_stride)

    def mlse_normal(self, samples, offset, length, tsc, flags, amp, toa, soft, avgpwr=None, chan=None, win=None, hard=None,
                    detect_thresh=3.0, energy_thresh=0.0, nsoft=148, soft_stride=None):
        """detect_demod_normal's detector, then the sequence equaliser on the detected bursts (trxsig_mlse_normal_batch)."""
        self._mlse("trxsig_mlse_normal_batch", offset, (samples, offset, length),
                   (tsc, detect_thresh, energy_thresh, flags, amp, toa, avgpwr, chan, win, soft, hard), soft, nsoft, soft_stride)

    def mlse_access(self, samples, offset, length, amp, toa, soft, enable=None, chan=None, win=None, hard=None, nsoft=148,
                    soft_stride=None):
        """The sequence equaliser for access bursts with the caller's amp / TOA (trxsig_mlse_access_batch): chan [B, 5] complex,
        win [B] int32."""
        self._mlse("trxsig_mlse_access_batch", offset, (samples, offset, length), (amp, toa, enable, chan, win, soft, hard), soft, nsoft,
                   soft_stride)

    def mlse_rach(self, samples, offset, length, flags, amp, toa, soft, avgpwr=None, chan=None, win=None, hard=None,
                  detect_thresh=5.0, energy_thresh=0.0, nsoft=148, soft_stride=None):
        """detect_demod_rach's detector, then the access-burst sequence equaliser on the detected bursts (trxsig_mlse_rach_batch)."""
        self._mlse("trxsig_mlse_rach_batch", offset, (samples, offset, length),
                   (detect_thresh, energy_thresh, flags, amp, toa, avgpwr, chan, win, soft, hard), soft, nsoft, soft_stride)

    def mlse_access_pinv(self):
        """The access-burst equaliser's least-squares table P32 [9, 41] float32, from the library (trxsig_mlse_access_pinv_host)."""
        import numpy as np
        out = np.zeros((9, 41), np.float32)
        self._chk(self.L.trxsig_mlse_access_pinv_host(out.ctypes.data), "trxsig_mlse_access_pinv_host")
        return out

    def mlse_sch(self, samples, offset, length, amp, toa, soft, enable=None, chan=None, win=None, hard=None, nsoft=148,
                 soft_stride=None):
        """The sequence equaliser for synchronisation bursts with the caller's amp / TOA (trxsig_mlse_sch_batch): chan [B, 5]
        complex, win [B] int32."""
        self._mlse("trxsig_mlse_sch_batch", offset, (samples, offset, length), (amp, toa, enable, chan, win, soft, hard), soft, nsoft,
                   soft_stride)

    def mlse_sch_pinv(self):
        """The synchronisation-burst equaliser's least-squares table P32 [9, 56] float32, from the library (trxsig_mlse_sch_pinv_host)."""
        import numpy as np
        out = np.zeros((9, 56), np.float32)
        self._chk(self.L.trxsig_mlse_sch_pinv_host(out.ctypes.data), "trxsig_mlse_sch_pinv_host")
        return out

    def sch_fit(self, samples, offset, length, amp, toa, enable=None, chan9=None, win=None, E=None, R=None, q=None):
        """The fit detector's statistic for synchronisation bursts with the caller's amp / TOA (trxsig_sch_fit_batch): chan9 [B, 9]
        complex, win [B] int32, E, R, q [B] float32; each may be None."""
        self._mlse("trxsig_sch_fit_batch", offset, (samples, offset, length), (amp, toa, enable, chan9, win, E, R, q))

    def mlse_div(self, samples0, offset0, samples1, offset1, length, tsc, amp, toa, soft, primary=None, enable=None, chan=None,
                 win=None, hard=None, nsoft=148, soft_stride=None):
        """The sequence equaliser over two receive antennas with the caller's amp / TOA (trxsig_mlse_div_batch): one amp / TOA per
        burst, primary [B] uint8 the antenna they came from, chan [B, 2, 5] complex, win [B] int32."""
        self._mlse("trxsig_mlse_div_batch", offset0, (samples0, offset0, samples1, offset1, length),
                   (tsc, amp, toa, primary, enable, chan, win, soft, hard), soft, nsoft, soft_stride)

    def mlse_div_normal(self, samples0, offset0, samples1, offset1, length, tsc, flags, amp, toa, sel, soft, avgpwr=None, chan=None,
                        win=None, hard=None, detect_thresh=3.0, energy_thresh=0.0, nsoft=148, soft_stride=None):
        """detect_demod_normal's detector on each antenna (flags, amp, toa, avgpwr: [2, B]), the selection (sel [B] uint8) and the
        two-antenna sequence equaliser on the bursts either antenna detected (trxsig_mlse_div_normal_batch)."""
        self._mlse("trxsig_mlse_div_normal_batch", offset0, (samples0, offset0, samples1, offset1, length),
                   (tsc, detect_thresh, energy_thresh, flags, amp, toa, avgpwr, sel, chan, win, soft, hard), soft, nsoft, soft_stride)

    def mlse_irc(self, samples0, offset0, samples1, offset1, length, tsc, amp, toa, soft, primary=None, enable=None, loading=IRC_LOADING,
                 cov_in=None, cov=None, chan=None, win=None, hard=None, nsoft=148, soft_stride=None):
        """mlse_div with interference-rejection combining (trxsig_mlse_irc_batch): the 2 x 2 covariance of the disturbance is
        estimated per burst from the midamble residuals with `loading` on its diagonal, or given as cov_in [B, 4] float32
        (A, Bv, xr, xi); cov [B, 4] returns the set used."""
        self._mlse("trxsig_mlse_irc_batch", offset0, (samples0, offset0, samples1, offset1, length),
                   (tsc, amp, toa, primary, enable, loading, cov_in, cov, chan, win, soft, hard), soft, nsoft, soft_stride)

    def mlse_irc_normal(self, samples0, offset0, samples1, offset1, length, tsc, flags, amp, toa, sel, soft, loading=IRC_LOADING,
                        avgpwr=None, cov=None, chan=None, win=None, hard=None, detect_thresh=3.0, energy_thresh=0.0, nsoft=148,
                        soft_stride=None):
        """mlse_div_normal's detector and selection, then mlse_irc with an estimated set (trxsig_mlse_irc_normal_batch)."""
        self._mlse("trxsig_mlse_irc_normal_batch", offset0, (samples0, offset0, samples1, offset1, length),
                   (tsc, detect_thresh, energy_thresh, loading, flags, amp, toa, avgpwr, sel, cov, chan, win, soft, hard), soft, nsoft,
                   soft_stride)

    def equalize_normal(self, samples, offset, length, tsc, flags, amp, toa, soft, w=None, b=None, hard=None,
                        detect_thresh=3.0, energy_thresh=0.0, variant52m=True, max_toa=4, nsoft=148,
                        soft_stride=None, fp16=False):
        """fp16=True: `samples` holds half-precision I/Q pairs (read directly by the kernels)."""
        if soft_stride is None:
            soft_stride = soft.shape[-1]
        self._chk(self.L.trxsig_equalize_normal_batch_fmt(
            self.h, _ptr(samples), int(bool(fp16)), _ptr(offset), _ptr(length), offset.numel(), tsc, detect_thresh, energy_thresh,
            int(variant52m), max_toa, _ptr(flags), _ptr(amp), _ptr(toa), _ptr(w), _ptr(b), _ptr(soft), _ptr(hard),
            nsoft, soft_stride), "trxsig_equalize_normal_batch")

    def modulate(self, bits, guard, out, out_offset, gain=None):
        """bits [B,148] uint8, guard [B] int32, out packed complex (as float32 pairs), out_offset [B] int32."""
        self._chk(self.L.trxsig_modulate_batch(self.h, _ptr(bits), _ptr(guard), _ptr(gain), guard.numel(), _ptr(out),
                                               _ptr(out_offset)), "trxsig_modulate_batch")

    def modulate_host(self, bits, guard, gain=None):
        import numpy as np
        bits = np.ascontiguousarray(bits, np.uint8); guard = np.ascontiguousarray(guard, np.int32)
        B = len(guard)
        length = (self.sps * (148 + guard)).astype(np.int32)
        off = np.concatenate([[0], np.cumsum(length)[:-1]]).astype(np.int32)
        out = np.zeros(int(length.sum()), np.complex64)
        g = None if gain is None else np.ascontiguousarray(gain, np.float32)
        self._chk(self.L.trxsig_modulate_host(self.h, bits.ctypes.data, guard.ctypes.data,
                                              None if g is None else g.ctypes.data, B, out.ctypes.data,
                                              off.ctypes.data, out.size), "trxsig_modulate_host")
        return out, off, length

    # ---- sigProcLib.h's free-standing primitives, single-vector host forms (numpy in / out) ----
    # ---- the rest of sigProcLib.h (host forms) ----
    def db(self, x): return self.L.trxsig_db(float(x))
    def dbinv(self, x): return self.L.trxsig_dbinv(float(x))

    def sinc_host(self, x):
        v = C.c_float()
        self._chk(self.L.trxsig_sinc_host(self.h, float(x), C.byref(v)), "trxsig_sinc_host")
        return v.value

    def gaussian_noise_host(self, seed, length, variance=1.0, mean=0j):
        import numpy as np
        C.CDLL(None).srand(int(seed))
        out = np.zeros(length, np.complex64)
        self._chk(self.L.trxsig_gaussian_noise_host(length, float(variance), C32(float(np.real(mean)), float(np.imag(mean))), out.ctypes.data),
                  "trxsig_gaussian_noise_host")
        return out

    def vector_norm2_host(self, x):
        import numpy as np
        x = np.ascontiguousarray(x, np.complex64); e = C.c_float(); p = C.c_float()
        self._chk(self.L.trxsig_vector_norm2_host(self.h, x.ctypes.data, x.size, C.byref(e), C.byref(p)), "trxsig_vector_norm2_host")
        return np.float32(e.value), np.float32(p.value)

    def frequency_shift_host(self, x, freq, start_phase=0.0, real_only=False):
        import numpy as np
        x = np.ascontiguousarray(x, np.complex64); y = np.zeros_like(x); fin = C.c_float()
        self._chk(self.L.trxsig_frequency_shift_host(self.h, x.ctypes.data, x.size, float(freq), float(start_phase), int(real_only),
                                                     y.ctypes.data, C.byref(fin)), "trxsig_frequency_shift_host")
        return y, np.float32(fin.value)

    def add_vector_host(self, x, y):
        import numpy as np
        x = np.array(x, np.complex64, copy=True); y = np.ascontiguousarray(y, np.complex64)
        self._chk(self.L.trxsig_add_vector_host(self.h, x.ctypes.data, x.size, y.ctypes.data, y.size), "trxsig_add_vector_host")
        return x

    def resample_linear_host(self, x, exp_factor, end_point=0j):
        import numpy as np
        x = np.ascontiguousarray(x, np.complex64)
        n = self.L.trxsig_resample_linear_out_len(x.size, float(exp_factor))
        if n < 0:
            return None
        out = np.zeros(max(n, 1), np.complex64)
        rc = self.L.trxsig_resample_linear_host(self.h, x.ctypes.data, x.size, float(exp_factor),
                                                C32(float(np.real(end_point)), float(np.imag(end_point))), out.ctypes.data, out.size)
        if rc < 0:
            self._chk(rc, "trxsig_resample_linear_host")
        return out[:rc]

    def convolve_host(self, a, b, span, a_real=False, b_real=False, correlate=False, cust_start=0, cust_len=0, abssym=False):
        import numpy as np
        a = np.ascontiguousarray(a, np.complex64); b = np.ascontiguousarray(b, np.complex64)
        n = self.L.trxsig_convolve_out_len(a.size, b.size, span, cust_len)
        out = np.zeros(max(n, 1), np.complex64)
        rc = self.L.trxsig_convolve_host(self.h, a.ctypes.data, a.size, b.ctypes.data, b.size, span,
                                         int(a_real) | (int(b_real) << 1) | (int(abssym) << 2), int(correlate), cust_start, cust_len, out.ctypes.data, out.size)
        if rc < 0:
            self._chk(rc, "trxsig_convolve_host")
        return out[:rc]

    def delay_vector_host(self, x, delay, real_only=False):
        import numpy as np
        y = np.array(x, np.complex64, copy=True)
        self._chk(self.L.trxsig_delay_vector_host(self.h, y.ctypes.data, y.size, float(delay), int(real_only)), "trxsig_delay_vector_host")
        return y

    def interpolate_point_host(self, x, ix, real_only=False):
        import numpy as np
        x = np.ascontiguousarray(x, np.complex64); out = np.zeros(1, np.complex64)
        self._chk(self.L.trxsig_interpolate_point_host(self.h, x.ctypes.data, x.size, float(ix), int(real_only), out.ctypes.data),
                  "trxsig_interpolate_point_host")
        return out[0]

    def peak_detect_host(self, x):
        import numpy as np
        x = np.ascontiguousarray(x, np.complex64); pk = np.zeros(1, np.complex64); ix = np.zeros(1, np.float32); av = np.zeros(1, np.float32)
        self._chk(self.L.trxsig_peak_detect_host(self.h, x.ctypes.data, x.size, pk.ctypes.data, ix.ctypes.data, av.ctypes.data),
                  "trxsig_peak_detect_host")
        return pk[0], ix[0], av[0]

    def elementwise_host(self, op, x, scale=1.0, real_only=False):
        """op: 0 scaleVector, 1 GMSKRotate, 2 GMSKReverseRotate, 3 vectorSlicer."""
        import numpy as np
        y = np.array(x, np.complex64, copy=True)
        sc = C32(float(np.real(scale)), float(np.imag(scale)))
        self._chk(self.L.trxsig_elementwise_host(self.h, op, y.ctypes.data, y.size, sc, int(real_only)), "trxsig_elementwise_host")
        return y

    def energy_detect_host(self, x, window, thresh, step=1):
        import numpy as np
        x = np.ascontiguousarray(x, np.complex64); av = np.zeros(1, np.float32)
        rc = self.L.trxsig_energy_detect_host(self.h, x.ctypes.data, x.size, int(window), step, float(thresh), av.ctypes.data)
        if rc < 0:
            self._chk(rc, "trxsig_energy_detect_host")
        return bool(rc), av[0]

    def decimate_host(self, x, factor):
        import numpy as np
        x = np.ascontiguousarray(x, np.complex64); out = np.zeros(max(x.size // factor, 1), np.complex64)
        rc = self.L.trxsig_decimate_host(self.h, x.ctypes.data, x.size, factor, out.ctypes.data)
        if rc < 0:
            self._chk(rc, "trxsig_decimate_host")
        return out[:rc]

    def resample_out_len(self, n_in, P, Q):
        return self.L.trxsig_resample_out_len(n_in, P, Q)

    def resample(self, x, n_in, in_stride, S, P, Q, lpf, out, out_stride):
        self._chk(self.L.trxsig_resample_batch(self.h, _ptr(x), n_in, in_stride, S, P, Q, _ptr(lpf), lpf.numel(),
                                               _ptr(out), out_stride), "trxsig_resample_batch")

    def unpack_int16(self, iq, n, out, swap_iq=True):
        self._chk(self.L.trxsig_unpack_int16(self.h, _ptr(iq), n, int(swap_iq), _ptr(out)), "trxsig_unpack_int16")

    def fec_xcch_decode(self, soft, n_blocks, frames, ok, wire=True, soft_stride=None):
        self._chk(self.L.trxsig_fec_xcch_decode_batch(self.h, _ptr(soft), soft_stride or soft.shape[-1], n_blocks,
                                                      int(wire), _ptr(frames), _ptr(ok)), "trxsig_fec_xcch_decode_batch")

    def fec_rach_decode(self, soft, n_bursts, tail_ok, bsic, ra, wire=True, soft_stride=None):
        self._chk(self.L.trxsig_fec_rach_decode_batch(self.h, _ptr(soft), soft_stride or soft.shape[-1], n_bursts,
                                                      int(wire), _ptr(tail_ok), _ptr(bsic), _ptr(ra)),
                  "trxsig_fec_rach_decode_batch")

    def channel_estimate(self, samples, offset, length, tsc, flags, amp, toa, chan_off, chan, detect_thresh=3.0, variant52m=False,
                         max_toa=4):
        self._chk(self.L.trxsig_channel_estimate_batch(self.h, _ptr(samples), _ptr(offset), _ptr(length), offset.numel(), tsc,
                                                       detect_thresh, int(variant52m), max_toa, _ptr(flags), _ptr(amp), _ptr(toa),
                                                       _ptr(chan_off), _ptr(chan)), "trxsig_channel_estimate_batch")

    def estimate_dfe(self, samples, offset, length, tsc, flags, amp, toa, chan_off, w, b, detect_thresh=3.0, snr_thresh=-1.0,
                     snr_value=0.0, variant52m=False, max_toa=4):
        """analyzeTrafficBurst(requestChannel) + scaleVector(chan, 1/amp) + designDFE(., SNR, 7) (Transceiver.cpp:326-347), no energy gate."""
        self._chk(self.L.trxsig_estimate_dfe_batch(self.h, _ptr(samples), _ptr(offset), _ptr(length), offset.numel(), tsc,
                                                   detect_thresh, snr_thresh, snr_value, int(variant52m), max_toa, _ptr(flags), _ptr(amp),
                                                   _ptr(toa), _ptr(chan_off), _ptr(w), _ptr(b)), "trxsig_estimate_dfe_batch")

    def design_dfe(self, chan, snr, w, b, amp=None):
        self._chk(self.L.trxsig_design_dfe_batch(self.h, _ptr(chan), _ptr(amp), _ptr(snr), snr.numel(), _ptr(w), _ptr(b)),
                  "trxsig_design_dfe_batch")

    def fec_xcch_encode(self, frames, n_blocks, tsc, bits):
        self._chk(self.L.trxsig_fec_xcch_encode_batch(self.h, _ptr(frames), n_blocks, tsc, _ptr(bits)), "trxsig_fec_xcch_encode_batch")

    def fec_tch_set_filler(self, c456):
        """The 456 bits (host array, one per byte) sent in a TCH block of kind TCH_FILLER; all zero until set."""
        import numpy as np
        h = np.ascontiguousarray(np.asarray(c456, dtype=np.uint8).ravel())
        if h.size != 456:
            raise ValueError("the filler is 456 bits")
        self._chk(self.L.trxsig_fec_tch_set_filler(self.h, h.ctypes.data), "trxsig_fec_tch_set_filler")

    def fec_tch_encode(self, kind, payload, tsc, state, bits):
        """TCH/FS + FACCH/F stream encode of kind[S, n] blocks (TCH_FILLER / TCH_SPEECH / TCH_FACCH); payload[S, n, 33],
        tsc[S] (uint8), state[S, TCH_TX_STATE_BYTES] (in / out, zero = a fresh encoder), bits[S, n, 4, 148] (all device)."""
        S, n = kind.shape
        self._chk(self.L.trxsig_fec_tch_encode_batch(self.h, S, n, _ptr(kind), _ptr(payload), _ptr(tsc), _ptr(state), _ptr(bits)),
                  "trxsig_fec_tch_encode_batch")

    def fec_sch_encode(self, fn, bsic, bits):
        """SCH bursts for fn[n] (uint32 / int32) and bsic[n] (uint8) -> bits[n, 148] (all device)."""
        self._chk(self.L.trxsig_fec_sch_encode_batch(self.h, _ptr(fn), _ptr(bsic), fn.numel(), _ptr(bits)),
                  "trxsig_fec_sch_encode_batch")

    def fec_sch_decode(self, soft, n, ok, bsic, rfn, soft_stride=None):
        """The inverse of fec_sch_encode: soft[n, >= 148] float32 -> ok[n], bsic[n] (uint8), rfn[n] (int32) (all device)."""
        self._chk(self.L.trxsig_fec_sch_decode_batch(self.h, _ptr(soft), soft_stride or soft.shape[-1], n, _ptr(ok), _ptr(bsic),
                                                     _ptr(rfn)), "trxsig_fec_sch_decode_batch")

    def fec_tch_decode(self, soft, n_bursts, tch, tch_good, stolen, facch=None, facch_ok=None, wire=True, soft_stride=None):
        self._chk(self.L.trxsig_fec_tch_decode_batch(self.h, _ptr(soft), soft_stride or soft.shape[-1], n_bursts, int(wire),
                                                     _ptr(tch), _ptr(tch_good), _ptr(facch), _ptr(facch_ok), _ptr(stolen)),
                  "trxsig_fec_tch_decode_batch")

    def fec_tch_decode_stream(self, soft, index, state, status, tch, facch, b0=None, fer=None, wire=True, n_rows=None,
                              soft_stride=None):
        """TCH/FACCH uplink stream decode: index[S, T] (int32, -1 = no burst) into soft[n_rows, soft_stride] (a tensor, or a
        device address with n_rows / soft_stride given); b0[S] (uint8, 0 or 4; None = all 0); state[S, TCH_RX_STATE_BYTES]
        (in / out); status[S, T/4], tch[S, T/4, 33], facch[S, T/4, 23], fer[S, T/4] float32 or None."""
        S, T = index.shape
        if n_rows is None:
            n_rows = soft.shape[0]
        self._chk(self.L.trxsig_fec_tch_decode_stream(self.h, S, T, _ptr(soft), soft_stride or soft.shape[-1], n_rows, _ptr(index),
                                                      _ptr(b0), int(wire), _ptr(state), _ptr(status), _ptr(tch), _ptr(facch),
                                                      _ptr(fer)), "trxsig_fec_tch_decode_stream")

    def fec_xcch_decode_stream(self, soft, index, state, status, frames, fer=None, wire=True, n_rows=None, soft_stride=None):
        """XCCH uplink stream decode: as fec_tch_decode_stream with B = t mod 4; state[S, XCCH_RX_STATE_BYTES],
        frames[S, T/4, 23]."""
        S, T = index.shape
        if n_rows is None:
            n_rows = soft.shape[0]
        self._chk(self.L.trxsig_fec_xcch_decode_stream(self.h, S, T, _ptr(soft), soft_stride or soft.shape[-1], n_rows, _ptr(index),
                                                       int(wire), _ptr(state), _ptr(status), _ptr(frames), _ptr(fer)),
                  "trxsig_fec_xcch_decode_stream")

    def fec_viterbi(self, soft, n_soft, n_blocks, bits, in_stride=None, out_stride=None):
        self._chk(self.L.trxsig_fec_viterbi_batch(self.h, _ptr(soft), n_soft, in_stride or soft.shape[-1], n_blocks,
                                                  _ptr(bits), out_stride or bits.shape[-1]), "trxsig_fec_viterbi_batch")

    def pdtch_encode(self, blocks, cs, tsc, bits):
        """GPRS packet data blocks: blocks[n, PDTCH_BLOCK_BYTES], cs[n] (CS1..CS4), tsc[n] (uint8) -> bits[n, 4, 148] (all device)."""
        self._chk(self.L.trxsig_fec_pdtch_encode_batch(self.h, _ptr(blocks), _ptr(cs), _ptr(tsc), cs.numel(), _ptr(bits)),
                  "trxsig_fec_pdtch_encode_batch")

    def pdtch_decode(self, soft, n_blocks, blocks, cs=None, cs_dist=None, ok=None, usf=None, index=None, wire=True, cs_force=-1,
                     n_rows=None, soft_stride=None):
        """The inverse: soft[n_rows, >= 148] float32 (a tensor, or a device address with n_rows / soft_stride given), index[n, 4]
        int32 (None: rows 4k..4k+3; a row outside [0, n_rows) = a missing burst) -> blocks[n, PDTCH_BLOCK_BYTES] and, where
        given, cs[n], cs_dist[n], ok[n], usf[n] (uint8).  cs_force: CS1..CS4, or -1 to read the scheme from the stealing flags."""
        if n_rows is None:
            n_rows = soft.shape[0]
        self._chk(self.L.trxsig_fec_pdtch_decode_batch(self.h, _ptr(soft), soft_stride or soft.shape[-1], n_rows, _ptr(index),
                                                       n_blocks, int(wire), cs_force, _ptr(blocks), _ptr(cs), _ptr(cs_dist),
                                                       _ptr(ok), _ptr(usf)), "trxsig_fec_pdtch_decode_batch")

    def access_encode(self, ra, fmt, bsic, bits):
        """Access bursts of either format: ra[n] (int16 / uint16), fmt[n] (ACCESS_8 / ACCESS_11), bsic[n] (uint8) -> bits[n, 148]
        (all device)."""
        self._chk(self.L.trxsig_fec_access_encode_batch(self.h, _ptr(ra), _ptr(fmt), _ptr(bsic), fmt.numel(), _ptr(bits)),
                  "trxsig_fec_access_encode_batch")

    def access_decode(self, soft, n, ra, fmt_out=None, tail_ok=None, bsic_out=None, index=None, wire=True, fmt=-1, bsic=0,
                      n_rows=None, soft_stride=None):
        """The inverse: soft[n_rows, >= 85] float32 (a tensor, or a device address with n_rows / soft_stride given), index[n] int32
        (None: row k; a row outside [0, n_rows) = a missing burst) -> ra[n] (16 bits a row) and, where given, fmt_out[n],
        tail_ok[n], bsic_out[n] (uint8).  fmt: ACCESS_8, ACCESS_11, or -1 to try both against the cell's bsic."""
        if n_rows is None:
            n_rows = soft.shape[0]
        self._chk(self.L.trxsig_fec_access_decode_batch(self.h, _ptr(soft), soft_stride or soft.shape[-1], n_rows, _ptr(index), n,
                                                        int(wire), fmt, bsic, _ptr(ra), _ptr(fmt_out), _ptr(tail_ok),
                                                        _ptr(bsic_out)), "trxsig_fec_access_decode_batch")

    def unpack_half(self, iq, n, out):
        self._chk(self.L.trxsig_unpack_half(self.h, _ptr(iq), n, _ptr(out)), "trxsig_unpack_half")

    def pack_int16_scaled(self, x, n, gain, iq):
        self._chk(self.L.trxsig_pack_int16_scaled(self.h, _ptr(x), n, float(gain), _ptr(iq)), "trxsig_pack_int16_scaled")

    def pack_int16(self, x, n, iq):
        self._chk(self.L.trxsig_pack_int16(self.h, _ptr(x), n, _ptr(iq)), "trxsig_pack_int16")

    def set_tuning(self, normal_path=None, rach_path=None, generic_taps=None, spec_peak=None, chain_lag=None,
                   chain_spin=None, demod_beside=None, beside_det_cus=None, cu_layout=None, beside_priority=None,
                   eq_tail=None, eq_dense=None, rxres_wpb=None, rxres_rows=None, chan_tpw=None, group_replay=None):
        """A/B implementation choice (results are bit-identical): see trxsig_set_tuning.  eq_tail / eq_dense / rxres_* / chan_tpw /
        group_replay are LIBRARY-WIDE (every context of the process): restore the default (1 / 4096 / 0 / 1 / 0 / 0) when done."""
        for key, v in ((12, eq_tail), (13, eq_dense), (14, rxres_wpb), (15, rxres_rows), (16, chan_tpw), (17, group_replay)):
            if v is not None:
                self._chk(self.L.trxsig_set_tuning(self.h, key, int(v)), "trxsig_set_tuning")
        if demod_beside is not None:
            self._chk(self.L.trxsig_set_tuning(self.h, 7, int(demod_beside)), "trxsig_set_tuning")
        if beside_det_cus is not None:
            self._chk(self.L.trxsig_set_tuning(self.h, 8, int(beside_det_cus)), "trxsig_set_tuning")
        if beside_priority is not None:
            self._chk(self.L.trxsig_set_tuning(self.h, 11, int(beside_priority)), "trxsig_set_tuning")
        if cu_layout is not None:
            self._chk(self.L.trxsig_set_tuning(self.h, 9, int(cu_layout)), "trxsig_set_tuning")
        if chain_lag is not None:
            self._chk(self.L.trxsig_set_tuning(self.h, 4, int(chain_lag)), "trxsig_set_tuning")
        if chain_spin is not None:
            self._chk(self.L.trxsig_set_tuning(self.h, 5, int(chain_spin)), "trxsig_set_tuning")
        if spec_peak is not None:
            self._chk(self.L.trxsig_set_tuning(self.h, 3, int(spec_peak)), "trxsig_set_tuning")
        if generic_taps is not None:
            self._chk(self.L.trxsig_set_tuning(self.h, 2, int(generic_taps)), "trxsig_set_tuning")
        if normal_path is not None:
            self._chk(self.L.trxsig_set_tuning(self.h, 0, int(normal_path)), "trxsig_set_tuning")
        if rach_path is not None:
            self._chk(self.L.trxsig_set_tuning(self.h, 1, int(rach_path)), "trxsig_set_tuning")

    def set_soft_mode(self, mode):
        """SOFT_EXACT (default: soft bits IEEE-equal to the reference's) or SOFT_TOLERANCE (hard bits, flags, amp, TOA exact;
        soft bits within 3.7e-5 of the reference's, and within 1e-6 or 1e-4 relative on the tested input families --
        trxsig_set_soft_mode)."""
        self._chk(self.L.trxsig_set_soft_mode(self.h, int(mode)), "trxsig_set_soft_mode")

    def soft_mode(self):
        return int(self.L.trxsig_get_soft_mode(self.h))

    def profile_enable(self, on=True):
        self._chk(self.L.trxsig_profile_enable(self.h, int(on)), "trxsig_profile_enable")

    def profile_collect(self):
        """{kernel name: (total_ms, launches)} since the last collect (synchronises)."""
        n = self.L.trxsig_kernel_count()
        ms = (C.c_float * n)(); cnt = (C.c_int * n)()
        if self.L.trxsig_profile_collect_n(self.h, n, ms, cnt) < 0:
            self._chk(-1, "trxsig_profile_collect_n")
        return {self.L.trxsig_kernel_name(i).decode(): (ms[i], cnt[i]) for i in range(n) if cnt[i]}

    def timer_start(self):
        self._chk(self.L.trxsig_timer_start(self.h), "trxsig_timer_start")

    def timer_stop(self):
        ms = C.c_float()
        self._chk(self.L.trxsig_timer_stop(self.h, C.byref(ms)), "trxsig_timer_stop")
        return ms.value


class TrxHost(_Object):
    """ctypes view of include/trxsig_transceiver.h: the per-ARFCN Transceiver orchestration (pullRadioVector,
    addRadioVector / pushRadioVector, control commands, UDP datagram codecs) on top of the GPU library.  It makes its own
    context: errors are read from its own handle, and close() releases it."""
    _prefix = "trxsig_trx"

    def __init__(self, sps, device=0, start=(0, 0), tsc_leg=0):
        import numpy as np
        self.np = np
        self.L = lib()
        self.sps = sps
        self.h = C.c_void_p()
        rc = self.L.trxsig_trx_create(C.byref(self.h), device, sps, start[0], start[1])
        if rc != 0:
            raise RuntimeError("trxsig_trx_create failed: %d" % rc)
        if tsc_leg:
            self._call("set_tsc_leg", tsc_leg)

    close = _Object.destroy

    def _last_error(self):
        return self.L.trxsig_trx_last_error(self.h).decode()

    def control(self, msg):
        buf = C.create_string_buffer(128)
        self._call("control", msg.encode(), buf, 128)
        return buf.value.decode()

    def expected_corr_type(self, tn, fn):
        return self.L.trxsig_trx_expected_corr_type(self.h, tn, fn)

    def pull_radio_vector(self, x, tn, fn):
        np = self.np
        x = np.ascontiguousarray(x, np.complex64)
        soft = np.zeros(160, np.float32)
        ns, rssi, toa = C.c_int(), C.c_int(), C.c_int()
        rc = self._call("pull_radio_vector", x.ctypes.data, len(x), tn, fn, soft.ctypes.data, C.byref(ns), C.byref(rssi), C.byref(toa))
        if rc == 0:
            return None
        return soft[:ns.value].copy(), rssi.value, toa.value

    def encode_rx_datagram(self, tn, fn, rssi, toa, soft):
        np = self.np
        soft = np.ascontiguousarray(soft, np.float32)
        out = np.zeros(158, np.uint8)
        self._chk(self.L.trxsig_trx_encode_rx_datagram(tn, fn, rssi, toa, soft.ctypes.data, len(soft), out.ctypes.data), "encode")
        return out.tobytes()

    def decode_tx_datagram(self, b):
        np = self.np
        a = np.frombuffer(b, np.uint8).copy()
        tn, fn, rssi = C.c_int(), C.c_int(), C.c_int()
        bits = np.zeros(148, np.uint8)
        rc = self.L.trxsig_trx_decode_tx_datagram(a.ctypes.data, len(a), C.byref(tn), C.byref(fn), C.byref(rssi), bits.ctypes.data)
        if rc != 0:
            return None
        return tn.value, fn.value, rssi.value, bits

    def add_radio_vector(self, bits, rssi, tn, fn):
        np = self.np
        bits = np.ascontiguousarray(bits, np.uint8)
        self._call("add_radio_vector", bits.ctypes.data, rssi, tn, fn)

    def push_radio_vector(self, tn, fn):
        np = self.np
        out = np.zeros(157 * self.sps, np.complex64)
        n, fq = C.c_int(), C.c_int()
        self._chk(self.L.trxsig_trx_push_radio_vector(self.h, tn, fn, out.ctypes.data, C.byref(n), C.byref(fq)), "push")
        return out[:n.value].copy(), bool(fq.value)

    @property
    def energy_threshold(self):
        return self.L.trxsig_trx_energy_threshold(self.h)

    def filler_modulus(self, tn):
        return self.L.trxsig_trx_filler_modulus(self.h, tn)

    def queue_size(self):
        return self.L.trxsig_trx_queue_size(self.h)

    def create_lpf(self, raw, gain):
        np = self.np
        raw = np.ascontiguousarray(raw, np.float32)
        out = np.zeros(len(raw), np.float32)
        self._chk(self.L.trxsig_create_lpf_host(raw.ctypes.data, len(raw), float(gain), out.ctypes.data), "create_lpf")
        return out


TSCLEG_EQUALIZE, TSCLEG_DEMOD, TSCLEG_MLSE = 0, 1, 2
RACHLEG_DEMOD, RACHLEG_MLSE = 0, 1


class TrxGroup(_Object):
    """ctypes view of include/trxsig_trxgroup.h: S Transceivers' pullRadioVector per call, state machine on the device.
    close() releases it."""
    _prefix = "trxsig_trxgroup"

    def __init__(self, ctx, n_arfcn, tsc_leg=TSCLEG_EQUALIZE, start=(0, 0)):
        super().__init__(ctx)
        self.S = n_arfcn
        self._create(n_arfcn, tsc_leg, start[0], start[1])
        self.n_slots = 0

    close = _Object.destroy

    def control(self, arfcn, msg):
        buf = C.create_string_buffer(128)
        self._call("control", arfcn, msg.encode(), buf, 128)
        return buf.value.decode()

    def expected_corr_type(self, arfcn, tn, fn):
        return self.L.trxsig_trxgroup_expected_corr_type(self.h, arfcn, tn, fn)

    def pull(self, samples, slot_stride, arfcn_stride, fn, tn, n_slots, burst_len=0):
        """samples: torch complex64-as-float32 device tensor (or a device address)."""
        res = TrxGroupResult()
        self._call("pull", _ptr(samples), slot_stride, arfcn_stride, burst_len, fn, tn, n_slots, C.byref(res))
        self.n_slots = n_slots
        return res

    def pull_bursts(self, samples, offset, length, n_per_arfcn, fn, tn):
        """pull on LISTED bursts: burst t of ARFCN a is entry a*n_per_arfcn + t of offset / length (int32 device tensors or addresses,
        samples into `samples`); (fn, tn) = the time of burst 0.  The samples are only read: entries may share a burst."""
        res = TrxGroupResult()
        self._call("pull_bursts", _ptr(samples), _ptr(offset), _ptr(length), n_per_arfcn, fn, tn, C.byref(res))
        self.n_slots = n_per_arfcn
        return res

    def combine_div(self, samples0, other, samples1, sel=None, chan=None, win=None):
        """Two-antenna receive diversity (trxsig_trxgroup_combine_div): this group has pulled antenna 0's samples0, `other` (a group of
        the same configuration on the same context) antenna 1's samples1, for the same time and slots.  Returns one combined result
        like pull's, owned by this group: the selected group's flags / amp / TOA / avgPwr, the training-sequence rows' soft bits from
        the two-antenna sequence equaliser.  sel [n_rows] uint8, chan [n_rows, 2, 5] complex, win [n_rows] int32: optional outputs."""
        res = TrxGroupResult()
        self._call("combine_div", _ptr(samples0), other.h if other is not None else None, _ptr(samples1), _ptr(sel), _ptr(chan), _ptr(win),
                   C.byref(res))
        return res

    def combine_irc(self, samples0, other, samples1, loading=IRC_LOADING, sel=None, cov=None, chan=None, win=None):
        """combine_div with interference-rejection combining on the training-sequence rows (trxsig_trxgroup_combine_irc): the
        covariance of the disturbance is estimated per burst, `loading` on its diagonal.  cov [n_rows, 4] float32: the set used."""
        res = TrxGroupResult()
        self._call("combine_irc", _ptr(samples0), other.h if other is not None else None, _ptr(samples1), loading, _ptr(sel), _ptr(cov),
                   _ptr(chan), _ptr(win), C.byref(res))
        return res

    def pull_rxfe(self, fe, iq, fn):
        """fe: frontend.RxFrontEnd on the same context; iq: int16 device tensor [S, K*864, 2] ([Sw, K*864*R, 2] for a wideband front
        end, whose Sw * C streams are the group's ARFCNs).  Returns (slots completed, result)."""
        iq = iq.contiguous()
        res = TrxGroupResult()
        n = C.c_int()
        chunk = 864 * max(1, getattr(fe, "rate_factor", 0) or 1)   # (a wideband front end: iq [Sw, K*864*R, 2])
        self._call("pull_rxfe", fe.h, iq.data_ptr(), iq.shape[1] // chunk, fn, C.byref(n), C.byref(res))
        fe._keep = iq
        self.n_slots = n.value
        return n.value, res

    # ---- transmit half ----
    def add_bursts(self, datagrams, arfcn):
        """datagrams: uint8 [n, 154] (the 154-byte transmit datagrams, host); arfcn: int32 [n] the ARFCN each arrived for."""
        np = self.np
        d = np.ascontiguousarray(datagrams, np.uint8); a = np.ascontiguousarray(arfcn, np.int32)
        assert d.ndim == 2 and d.shape[1] == 154 and a.shape == (d.shape[0],)
        self._call("add_bursts", d.ctypes.data, a.ctypes.data, d.shape[0])

    def tx_staging(self, n_max):
        """The pinned block to RECEIVE the next batch into: (datagrams uint8 [n_max, 154], arfcn int32 [n_max]) as numpy views of the
        library's memory; valid until add_staged."""
        np = self.np
        pd, pa = C.c_void_p(), C.c_void_p()
        self._call("tx_staging", int(n_max), C.byref(pd), C.byref(pa))
        d = np.ctypeslib.as_array(C.cast(pd, C.POINTER(C.c_uint8)), shape=(n_max, 154))
        a = np.ctypeslib.as_array(C.cast(pa, C.POINTER(C.c_int32)), shape=(n_max,))
        return d, a

    def add_staged(self, n):
        """The first n datagrams of the staging block: header check on the host, one upload, one kernel."""
        self._call("add_staged", int(n))

    def add_l1tx(self, l1):
        """Every non-empty slot of l1's (an L1Tx on the same context) last encode into the queues, device to device: the effect of
        add_bursts(*l1.datagrams()) without the copy down, the host's header loop and the upload.  Enqueues only."""
        self._call("add_l1tx", l1.h if l1 is not None else None)

    def push(self, fn, tn, n_slots, device="cuda:0"):
        """pushRadioVector for n_slots timeslots from (fn, tn): (bits uint8 [S, n, 148], gain float32 [S, n], from_queue uint8 [S, n])
        as torch views of the group's device buffers (valid until the next push)."""
        import torch
        pb, pg, pq = C.c_void_p(), C.c_void_p(), C.c_void_p()
        self._call("push", fn, tn, n_slots, C.byref(pb), C.byref(pg), C.byref(pq))
        dev = torch.device(device)
        return (torch.as_tensor(_DevView(pb.value, (self.S, n_slots, 148), "|u1"), device=dev),
                torch.as_tensor(_DevView(pg.value, (self.S, n_slots), "<f4"), device=dev),
                torch.as_tensor(_DevView(pq.value, (self.S, n_slots), "|u1"), device=dev))

    def push_txbe(self, be, fn, tn, n_slots):
        self._call("push_txbe", be.h, fn, tn, n_slots)

    def tx_queue_size(self, arfcn):
        dropped = C.c_int()
        n = self._call("tx_queue_size", arfcn, C.byref(dropped))
        return n, bool(dropped.value)

    def pull_host(self, x, slot_stride, arfcn_stride, fn, tn, n_slots, burst_len=0):
        np = self.np
        x = np.ascontiguousarray(x, np.complex64)
        self._call("pull_host", x.ctypes.data, slot_stride, arfcn_stride, burst_len, fn, tn, n_slots)
        self.n_slots = n_slots

    def collect(self, soft=True):
        """dict of host arrays indexed [slot][arfcn]: valid, soft (x148), rssi, timing, threshold."""
        np = self.np
        n = self.n_slots * self.S
        valid = np.zeros(n, np.uint8); rssi = np.zeros(n, np.int32); timing = np.zeros(n, np.int32); thr = np.zeros(n, np.float64)
        sb = np.zeros((n, 148), np.float32) if soft else None
        self._call("collect", valid.ctypes.data, sb.ctypes.data if soft else None, rssi.ctypes.data, timing.ctypes.data, thr.ctypes.data)
        sh = (self.n_slots, self.S)
        return dict(valid=valid.reshape(sh).astype(bool), soft=None if sb is None else sb.reshape(sh + (148,)), rssi=rssi.reshape(sh),
                    timing=timing.reshape(sh), threshold=thr.reshape(sh))

    def set_pipelined(self, on=True):
        """Large pulls return without joining the side stream the state machine replays on (see trxsig_trxgroup.h)."""
        self._call("set_pipelined", 1 if on else 0)

    def set_beside_rows(self, rows):
        """Pulls with at least `rows` rows replay the state machine on the group's side stream (0 = never, the default)."""
        self._call("set_beside_rows", int(rows))

    def set_rach_leg(self, rach_leg):
        """RACHLEG_DEMOD (the default: demodulateBurst) or RACHLEG_MLSE (trxsig_mlse_access_batch) for the access-burst rows."""
        self._call("set_rach_leg", int(rach_leg))

    def set_split_rows(self, rows):
        """Fused pulls with at least `rows` rows and both kinds of burst detect the access bursts beside the normal ones (0 = never)."""
        self._call("set_split_rows", int(rows))

    def sync(self):
        self._call("sync")

    def energy_threshold(self, arfcn):
        v = C.c_double()
        self._call("energy_threshold", arfcn, C.byref(v))
        return v.value


L1_TCH, L1_XCCH, L1_RACH = 0, 1, 2               # channel classes of trxsig_l1rx.h
L1_TCHF, L1_SACCH_TF, L1_SDCCH8, L1_SACCH_C8, L1_SDCCH4, L1_SACCH_C4, L1_RACH_C5 = range(7)   # mapping kinds (TRXSIG_L1_*)


class L1Rx(_PlanObject):
    """ctypes view of include/trxsig_l1rx.h: a Transceiver group pull -> the logical channels' decoders, on the device.
    open(cls, chan): L1Decoder::open of one TCH / XCCH channel (FER reset; SACCH: power 40, TA 0).
    close(cls, chan): L1Decoder::close of one TCH / XCCH channel: its bursts are ignored until it is opened again.
    destroy(): trxsig_l1rx_destroy (channels are closed with close(cls, chan))."""
    _prefix = "trxsig_l1rx"

    def __init__(self, ctx, comb, bsic, band=900):
        super().__init__(ctx, comb, int(bsic), int(band))
        self.out = None

    def decode(self, res, fn, wire=True):
        """res: a TrxGroupResult (of trxsig_trxgroup_pull, or built from tensors); whole frames from (fn, TN 0)."""
        out = L1RxOut()
        self._call("decode", C.byref(res), int(fn), int(bool(wire)), C.byref(out))
        self.out = out
        return out

    def collect(self, state=True):
        """The last decode's outputs as host numpy arrays (synchronises the context's stream)."""
        o = self.out
        self.ctx.synchronize()
        host = lambda p, shape, ts: _to_host(self.ctx, p, shape, ts)
        T, X, bt, bx, R = o.n_tch, o.n_xcch, o.nb_tch, o.nb_xcch, o.rach_cap
        r = dict(tch_status=host(o.d_tch_status, (T, bt), "|u1"), tch=host(o.d_tch_frames, (T, bt, 33), "|u1"),
                 facch=host(o.d_facch, (T, bt, 23), "|u1"), tch_fer=host(o.d_tch_fer, (T, bt), "<f4"),
                 tch_fn=host(o.d_tch_fn, (T, bt), "<i4"),
                 xcch_status=host(o.d_xcch_status, (X, bx), "|u1"), xcch=host(o.d_xcch_frames, (X, bx, 23), "|u1"),
                 xcch_fer=host(o.d_xcch_fer, (X, bx), "<f4"), xcch_fn=host(o.d_xcch_fn, (X, bx), "<i4"),
                 tch_rssi=host(o.d_tch_rssi, (T,), "<i4"), tch_timing=host(o.d_tch_timing, (T,), "<i4"),
                 xcch_rssi=host(o.d_xcch_rssi, (X,), "<i4"), xcch_timing=host(o.d_xcch_timing, (X,), "<i4"),
                 ms_power=host(o.d_ms_power, (X,), "<i4"), ms_ta=host(o.d_ms_ta, (X,), "<i4"))
        n = int(host(o.d_rach_count, (1,), "<i4")[0]) if R else 0
        r["rach"] = dict(fn=host(o.d_rach_fn, (R,), "<i4")[:n], arfcn=host(o.d_rach_arfcn, (R,), "<i4")[:n],
                         rssi=host(o.d_rach_rssi, (R,), "<i4")[:n], timing=host(o.d_rach_timing, (R,), "<i4")[:n],
                         ok=host(o.d_rach_ok, (R,), "|u1")[:n], ra=host(o.d_rach_ra, (R,), "|u1")[:n])
        if state:
            r["tch_state"] = host(self.state(L1_TCH), (T, TCH_RX_STATE_BYTES), "|u1")
            r["xcch_state"] = host(self.state(L1_XCCH), (X, XCCH_RX_STATE_BYTES), "|u1")
        return r


L1_CCCH = 3                                      # the downlink's CCCH class (trxsig_l1tx.h)
L1TX_STATE_BYTES = 160                           # TRXSIG_L1TX_STATE_BYTES
L1TX_NONE, L1TX_FCCH, L1TX_SCH, L1TX_BCCH, L1TX_CCCH, L1TX_XCCH, L1TX_TCH, L1TX_IDLE = range(8)   # d_what codes


class L1Tx(_PlanObject):
    """ctypes view of include/trxsig_l1tx.h: per-channel payloads for whole frames -> timed bursts, on the device.
    comb as for L1Rx; rssi_target is GSM.RSSITarget.
    open(cls, chan): L1Encoder::open of one TCH / XCCH / CCCH channel (SACCH: orders 40 dBm / TA 0; pending idle fill cancelled).
    close(cls, chan): L1Encoder::close: nothing more is sent; the next numFrames positions carry the dummy burst."""
    _prefix = "trxsig_l1tx"

    def __init__(self, ctx, comb, bsic, band=900, rssi_target=-15.0):
        super().__init__(ctx, comb, int(bsic), int(band), float(rssi_target))
        self.out = None
        self._keep = None

    def set_si(self, si):
        """si: uint8 [4, 23], SI1..SI4."""
        si = self.np.ascontiguousarray(si, self.np.uint8).reshape(4, 23)
        self._call("set_si", si.ctypes.data)

    def grid(self, fn, n_frames):
        """(nb_tch, nb_xcch, nb_ccch) of a call"""
        v = [C.c_int() for _ in range(3)]
        self._call("grid", int(fn), int(n_frames), *[C.byref(x) for x in v])
        return tuple(x.value for x in v)

    def encode(self, fn, n_frames, tch_kind=None, tch_payload=None, xcch_kind=None, xcch_payload=None, ccch_kind=None,
               ccch_payload=None, sibling=None):
        """Grids as torch uint8 tensors on the context's device (or None for a class without channels)."""
        ins, out = L1TxIn(), L1TxOut()
        keep = _fill(ins, None, (tch_kind, tch_payload, xcch_kind, xcch_payload, ccch_kind, ccch_payload), itemsize=1, empty_as_one=True)
        self._call("encode", int(fn), int(n_frames), C.byref(ins), sibling.h if sibling is not None else None, C.byref(out))
        self._keep = keep
        self.out = out
        return out

    def collect(self, state=True):
        """The last encode's outputs as host numpy arrays (synchronises the context's stream)."""
        o = self.out
        self.ctx.synchronize()
        host = lambda p, shape, ts: _to_host(self.ctx, p, shape, ts)
        A, F, X = o.n_arfcn, o.n_frames, o.n_xcch
        r = dict(bits=host(o.d_bits, (A, 8 * F, 148), "|u1"), what=host(o.d_what, (A, 8 * F), "|u1"),
                 ms_power=host(o.d_ms_power, (X,), "<i4"), ms_ta=host(o.d_ms_ta, (X,), "<f4"))
        if state:
            for cls, key in ((L1_TCH, "tch_state"), (L1_XCCH, "xcch_state"), (L1_CCCH, "ccch_state")):
                r[key] = host(self.state(cls), (self.channels(cls), L1TX_STATE_BYTES), "|u1")
        return r

    def datagrams(self, cap=None):
        """(datagrams uint8 [n, 154], arfcn int32 [n]) of the last encode's non-empty slots, in (FN, TN, ARFCN) order."""
        np = self.np
        n = C.c_int()
        if cap is None:
            o = self.out
            cap = o.n_arfcn * 8 * o.n_frames
        d = np.zeros((max(cap, 1), 154), np.uint8); a = np.zeros(max(cap, 1), np.int32)
        self._call("datagrams", d.ctypes.data, a.ctypes.data, int(cap), C.byref(n))
        return d[:n.value], a[:n.value]


L1MS_STATE_BYTES = 160                           # TRXSIG_L1MS_STATE_BYTES
L1MS_NONE, L1MS_TCH, L1MS_XCCH, L1MS_ACCESS = range(4)   # d_what codes of trxsig_l1ms.h


class L1Ms(_PlanObject):
    """ctypes view of include/trxsig_l1ms.h: the handsets of a cell -- per-channel uplink payloads for whole frames -> timed
    uplink bursts -> the samples TrxGroup.pull takes, on the device.  comb as for L1Rx.
    open(cls, chan): open of one TCH / XCCH channel (SACCH: the handset back at the band's level nearest 40 dBm, TA 0).
    close(cls, chan): no new block of the channel is sent until it is opened again."""
    _prefix = "trxsig_l1ms"

    def __init__(self, ctx, comb, bsic, band=900):
        super().__init__(ctx, comb, int(bsic), int(band))
        self.out = None
        self._keep = None

    def set_phy(self, xcch_chan, power_dbm, ta):
        """The handset of a SACCH channel: power (0..40 dBm, taken to the band's nearest level) and TA (0..63)."""
        self._call("set_phy", int(xcch_chan), int(power_dbm), int(ta))

    def grid(self, fn, n_frames):
        """(nb_tch, nb_xcch, n_rach) of a call"""
        v = [C.c_int() for _ in range(3)]
        self._call("grid", int(fn), int(n_frames), *[C.byref(x) for x in v])
        return tuple(x.value for x in v)

    def encode(self, fn, n_frames, tch_kind=None, tch_payload=None, xcch_kind=None, xcch_payload=None, rach_kind=None,
               rach_ra=None, rach_bsic=None, sibling=None):
        """Grids as torch uint8 tensors on the context's device (or None for a class without channels); sibling: an L1Tx."""
        ins, out = L1MsIn(), L1MsOut()
        keep = _fill(ins, None, (tch_kind, tch_payload, xcch_kind, xcch_payload, rach_kind, rach_ra, rach_bsic), itemsize=1,
                     empty_as_one=True)
        self._call("encode", int(fn), int(n_frames), C.byref(ins), sibling.h if sibling is not None else None, C.byref(out))
        self._keep = keep
        self.out = out
        return out

    def radiate(self, samples, slot_stride, arfcn_stride, tch_gain=None, tch_delay=None, xcch_gain=None, xcch_delay=None,
                rach_gain=None, rach_delay=None, amp_of_power=None):
        """The last encode as samples into `samples` (a complex64 / float32 tensor or a device address), strides in complex
        samples.  Gains: complex64 (or float32 [n, 2]) tensors, delays float32 (symbols), amp_of_power float32 [41]."""
        air = L1MsAir()
        keep = _fill(air, None, (tch_gain, tch_delay, xcch_gain, xcch_delay, rach_gain, rach_delay, amp_of_power), empty_as_one=True)
        self._call("radiate", C.byref(air), _ptr(samples), int(slot_stride), int(arfcn_stride))
        self._keep_air = keep

    def follow(self, rx):
        """Follow the SACCH orders an L1MsRx decodes (same context and plan); None stops following."""
        self._call("follow", rx.h if rx is not None else None)
        self._follow = rx

    def collect(self, state=True):
        """The last encode's outputs as host numpy arrays (synchronises the context's stream)."""
        o = self.out
        self.ctx.synchronize()
        host = lambda p, shape, ts: _to_host(self.ctx, p, shape, ts)
        A, F, X = o.n_arfcn, o.n_frames, o.n_xcch
        r = dict(bits=host(o.d_bits, (A, 8 * F, 148), "|u1"), what=host(o.d_what, (A, 8 * F), "|u1"),
                 ms_power=host(o.d_ms_power, (X,), "<i4"), ms_ta=host(o.d_ms_ta, (X,), "<i4"))
        if state:
            for cls, key in ((L1_TCH, "tch_state"), (L1_XCCH, "xcch_state")):
                r[key] = host(self.state(cls), (self.channels(cls), L1MS_STATE_BYTES), "|u1")
        return r


L1_BCCH, L1_SCH, L1_FCCH = 4, 5, 6               # the downlink-only classes of trxsig_l1msrx.h
L1_CCCH_C5, L1_BCCH_C5, L1_SCH_C5, L1_FCCH_C5 = 7, 8, 9, 10   # mapping kinds (TRXSIG_L1_*)


class L1MsRx(_PlanObject):
    """ctypes view of include/trxsig_l1msrx.h: the handsets' receive side -- downlink bursts (a TrxGroupResult of whole frames)
    -> the logical channels' payloads, the SCH's frame number and BSIC, the FCCH, and the SACCH orders, on the device.  comb as
    for L1Rx.
    open(cls, chan): open of one TCH / XCCH / CCCH / BCCH channel (FER reset; SACCH: orders 40 dBm / TA 0).
    close(cls, chan): the channel's bursts are ignored until it is opened again.
    destroy(): trxsig_l1msrx_destroy (an L1Ms that follows this object stops following first)."""
    _prefix = "trxsig_l1msrx"

    def __init__(self, ctx, comb, bsic, band=900):
        super().__init__(ctx, comb, int(bsic), int(band))
        self.out = None

    def decode(self, res, fn, wire=True):
        """res: a TrxGroupResult (of a pull of downlink samples, or built from tensors); whole frames from (fn, TN 0)."""
        out = L1MsRxOut()
        self._call("decode", C.byref(res), int(fn), int(bool(wire)), C.byref(out))
        self.out = out
        return out

    def collect(self, state=True):
        """The last decode's outputs as host numpy arrays (synchronises the context's stream)."""
        o = self.out
        self.ctx.synchronize()
        host = lambda p, shape, ts: _to_host(self.ctx, p, shape, ts)
        T, bt, bx, S, Fc = o.n_tch, o.nb_tch, o.nb_ctl, o.sch_cap, o.fcch_cap
        r = dict(tch_status=host(o.d_tch_status, (T, bt), "|u1"), tch=host(o.d_tch_frames, (T, bt, 33), "|u1"),
                 facch=host(o.d_facch, (T, bt, 23), "|u1"), tch_fer=host(o.d_tch_fer, (T, bt), "<f4"),
                 tch_fn=host(o.d_tch_fn, (T, bt), "<i4"), tch_rssi=host(o.d_tch_rssi, (T,), "<i4"),
                 tch_timing=host(o.d_tch_timing, (T,), "<i4"))
        for key, n in (("xcch", o.n_xcch), ("ccch", o.n_ccch), ("bcch", o.n_bcch)):
            f = lambda name: getattr(o, "d_%s_%s" % (key, name))
            r.update({key + "_status": host(f("status"), (n, bx), "|u1"), key: host(f("frames"), (n, bx, 23), "|u1"),
                      key + "_fer": host(f("fer"), (n, bx), "<f4"), key + "_fn": host(f("fn"), (n, bx), "<i4"),
                      key + "_rssi": host(f("rssi"), (n,), "<i4"), key + "_timing": host(f("timing"), (n,), "<i4")})
        r["bcch_tc"] = host(o.d_bcch_tc, (o.n_bcch, bx), "<i4")
        r["ord_power"] = host(o.d_ord_power, (o.n_xcch,), "<i4")
        r["ord_ta"] = host(o.d_ord_ta, (o.n_xcch,), "<i4")
        r["sch"] = dict(fn=host(o.d_sch_fn, (S,), "<i4"), present=host(o.d_sch_present, (S,), "|u1"), ok=host(o.d_sch_ok, (S,), "|u1"),
                        bsic=host(o.d_sch_bsic, (S,), "|u1"), rfn=host(o.d_sch_rfn, (S,), "<i4"), sync=host(o.d_sch_sync, (S,), "|u1"))
        r["fcch"] = dict(fn=host(o.d_fcch_fn, (Fc,), "<i4"), ones=host(o.d_fcch_ones, (Fc,), "<i4"))
        if state:
            r["tch_state"] = host(self.state(L1_TCH), (T, TCH_RX_STATE_BYTES), "|u1")
            for cls, key, n in ((L1_XCCH, "xcch", o.n_xcch), (L1_CCCH, "ccch", o.n_ccch), (L1_BCCH, "bcch", o.n_bcch)):
                r[key + "_state"] = host(self.state(cls), (n, XCCH_RX_STATE_BYTES), "|u1")
        return r


ACQ_FCCH, ACQ_WINDOW, ACQ_SCH, ACQ_DECODED = 1, 2, 4, 8   # trxsig_l1acq_out.d_state bits (TRXSIG_ACQ_*)
ACQ_FCCH_THRESH, ACQ_SCH_THRESH = 0.5, 8.0                # TRXSIG_L1ACQ_FCCH_THRESH / _SCH_THRESH
ACQ_MAX_WINDOW = 256                                      # TRXSIG_L1ACQ_MAX_WINDOW (symbols)
SCHLEG_DEMOD, SCHLEG_MLSE = 0, 1                          # TRXSIG_SCHLEG_*
SCHDET_VALLEY, SCHDET_FIT = 0, 1                          # TRXSIG_SCHDET_*
ACQ_SCH_FIT_THRESH = 1.4                                  # TRXSIG_L1ACQ_SCH_FIT_THRESH: the threshold to pass with SCHDET_FIT


class L1Acq(_Object):
    """ctypes view of include/trxsig_l1acq.h: mobile-side acquisition -- raw downlink samples of a C0 carrier -> the FCCH's
    position and frequency offset, the SCH burst's soft values, FN and BSIC, and where the frame grid lies, on the device."""
    _prefix = "trxsig_l1acq"

    def __init__(self, ctx, max_streams, max_samples):
        super().__init__(ctx)
        self._create(int(max_streams), int(max_samples))
        self.out = None

    def sequence(self):
        """(seq[64 sps] complex64, gain complex64, toa float32): the SCH correlation sequence as built at create."""
        np = self.np
        seq = np.zeros(64 * self.ctx.sps, np.complex64); gain = np.zeros(1, np.complex64); toa = np.zeros(1, np.float32)
        self._call("sequence", seq.ctypes.data, gain.ctypes.data, toa.ctypes.data)
        return seq, gain[0], toa[0]

    def search(self, samples, stream_stride, n_samples, n_streams, fcch_thresh=ACQ_FCCH_THRESH, sch_thresh=ACQ_SCH_THRESH):
        """samples: device tensor (complex64, or float32 pairs) holding n_streams streams stream_stride samples apart."""
        out = L1AcqOut()
        self._call("search", _ptr(samples), int(stream_stride), int(n_samples), int(n_streams), float(fcch_thresh), float(sch_thresh),
                   C.byref(out))
        self.out = out
        return out

    def detect_sch(self, samples, offset, length, flags, amp, toa, soft, omega=None, ptm=None, hard=None,
                   detect_thresh=ACQ_SCH_THRESH, soft_stride=None):
        """Stage 2 on caller-chosen windows (all device tensors): offset / length int32 [B]; flags uint8 [B], amp [B, 2], toa [B],
        soft [B, >= 148] are written; omega float32 [B] (None: no frequency shift), ptm float32 [B], hard uint8 [B, stride]."""
        self._call("detect_sch_batch", _ptr(samples), _ptr(offset), _ptr(length), offset.numel(), _ptr(omega), float(detect_thresh),
                   _ptr(flags), _ptr(amp), _ptr(toa), _ptr(ptm), _ptr(soft), _ptr(hard), soft_stride or soft.shape[-1])

    def set_sch_leg(self, sch_leg):
        """SCHLEG_DEMOD (the default: demodulateBurst) or SCHLEG_MLSE (trxsig_mlse_sch_batch) behind the SCH detector."""
        self._call("set_sch_leg", int(sch_leg))

    def sch_channel(self):
        """(chan [n_streams, 5] complex64, win [n_streams] int32) of the last search as host numpy arrays: the equalising leg's
        taps and window words; zeros and 2 on SCHLEG_DEMOD or where nothing was detected (synchronises the context's stream)."""
        np = self.np
        d_chan, d_win = C.c_void_p(), C.c_void_p()
        self._call("sch_channel", C.byref(d_chan), C.byref(d_win))
        self.ctx.synchronize()
        S = self.out.n_streams if self.out is not None else 0
        chan = _to_host(self.ctx, d_chan.value, (S, 10), "<f4").view(np.complex64).reshape(S, 5)
        return chan, _to_host(self.ctx, d_win.value, (S,), "<i4")

    def set_sch_detector(self, detector):
        """SCHDET_VALLEY (the default: analyzeTrafficBurst's valley rule) or SCHDET_FIT (trxsig_sch_fit_batch's q) as the SCH verdict."""
        self._call("set_sch_detector", int(detector))

    def sch_fit(self):
        """(q [n_streams], R [n_streams]) float32 of the last search as host numpy arrays: the fit detector's statistic and
        residual; zeros on SCHDET_VALLEY or for a stream that was no candidate (synchronises the context's stream)."""
        d_q, d_R = C.c_void_p(), C.c_void_p()
        self._call("sch_fit", C.byref(d_q), C.byref(d_R))
        self.ctx.synchronize()
        S = self.out.n_streams if self.out is not None else 0
        return _to_host(self.ctx, d_q.value, (S,), "<f4"), _to_host(self.ctx, d_R.value, (S,), "<f4")

    def collect(self):
        """The last search's outputs as host numpy arrays (synchronises the context's stream)."""
        np, o = self.np, self.out
        self.ctx.synchronize()
        S = o.n_streams
        host = lambda p, shape, ts: _to_host(self.ctx, p, shape, ts)
        r = dict(state=host(o.d_state, (S,), "|u1"), fcch_k=host(o.d_fcch_k, (S,), "<i4"), fcch_metric=host(o.d_fcch_metric, (S,), "<f4"),
                 fcch_c=host(o.d_fcch_c, (S, 2), "<f4").view(np.complex64).ravel(), fcch_e=host(o.d_fcch_e, (S,), "<f4"),
                 arg=host(o.d_arg, (S,), "<f4"), omega=host(o.d_omega, (S,), "<f4"), sch_w0=host(o.d_sch_w0, (S,), "<i4"),
                 sch_ptm=host(o.d_sch_ptm, (S,), "<f4"), sch_amp=host(o.d_sch_amp, (S, 2), "<f4").view(np.complex64).ravel(),
                 sch_toa=host(o.d_sch_toa, (S,), "<f4"), soft=host(o.d_soft, (S, o.soft_stride), "<f4"),
                 ok=host(o.d_ok, (S,), "|u1"), bsic=host(o.d_bsic, (S,), "|u1"), rfn=host(o.d_rfn, (S,), "<i4"))
        return r


AIR_MAX_TAPS = 32                                         # TRXSIG_AIR_MAX_TAPS


class Air(_Object):
    """ctypes view of include/trxsig_air.h: the radio channel on the device -- multipath, oscillator offset and counter-based
    Gaussian noise, slot cells -> slot cells (cells) or a carrier's cells -> one stream per handset (stream); and the taps of a
    time-varying, frequency-selective multipath channel for the cell form (fade_profile, fade_columns, fade, fade_params)."""
    _prefix = "trxsig_air"

    def __init__(self, ctx, max_taps=AIR_MAX_TAPS):
        super().__init__(ctx)
        self._create(int(max_taps))
        self._keep = None

    def cells(self, fn, n_arfcn, n_frames, seed, x, slot_stride, arfcn_stride, out=None, out_slot_stride=None, out_arfcn_stride=None,
              taps=None, step=None, phase=None, sigma=None, accumulate=False):
        """x / out: device tensors (complex64 or float32 pairs) or addresses, strides in complex samples; out None: in place.
        taps complex64 [a][t][Lh] (or float32 [a][t][Lh][2]: give n_taps through its shape), step / phase int32-sized words,
        sigma float32, all [a][t] device tensors or None (the stage is skipped)."""
        p = AirCellParams()
        if taps is not None:
            assert taps.is_contiguous()
            p.d_taps = taps.data_ptr()
            p.n_taps = taps.shape[2]
        _fill(p, ("d_step", "d_phase", "d_sigma"), (step, phase, sigma), itemsize=4)
        if out is None:
            out, out_slot_stride, out_arfcn_stride = x, slot_stride, arfcn_stride
        self._call("cells", int(fn), int(n_arfcn), int(n_frames), int(seed), _ptr(x), int(slot_stride), int(arfcn_stride), C.byref(p),
                   _ptr(out), int(out_slot_stride), int(out_arfcn_stride), int(bool(accumulate)))
        self._keep = (taps, step, phase, sigma)

    def stream(self, n_arfcn, n_cells, seed, x, slot_stride, arfcn_stride, out, out_stride, length, arfcn, cut, delay=None, step=None,
               phase=None, gain=None, sigma=None, n0=None):
        """x: the carriers' cells, out: [n_handsets][out_stride] complex samples; arfcn int32, cut int64, delay / sigma float32,
        step / phase / n0 32-bit words, gain complex64 -- device tensors of one entry per handset, or None where optional."""
        p = AirStreamParams()
        p.n_arfcn = int(n_arfcn)
        assert arfcn.element_size() == 4 and cut.element_size() == 8
        keep = _fill(p, None, (arfcn, cut, delay, step, phase, gain, sigma, n0))
        self._call("stream", int(n_cells), int(seed), _ptr(x), int(slot_stride), int(arfcn_stride), int(arfcn.numel()), C.byref(p),
                   int(length), _ptr(out), int(out_stride))
        self._keep = keep


    def fade_profile(self, delay_ns, power, n_sinusoids, n_taps, centre=0, los_share=None, los_cos_q23=None):
        """The fading profile (host sequences, one entry per path): delays in ns, powers, optionally the line-of-sight share of
        each power and its arrival cosine in Q23.  In stream order."""
        np = self.np
        d, w = np.ascontiguousarray(delay_ns, np.int32), np.ascontiguousarray(power, np.float32)
        ls = None if los_share is None else np.ascontiguousarray(los_share, np.float32)
        lc = None if los_cos_q23 is None else np.ascontiguousarray(los_cos_q23, np.int32)
        assert len(w) == len(d) and all(v is None or len(v) == len(d) for v in (ls, lc))
        self._call("fade_profile", len(d), d.ctypes.data, w.ctypes.data, None if ls is None else ls.ctypes.data,
                   None if lc is None else lc.ctypes.data, int(n_sinusoids), int(n_taps), int(centre))
        self.fade_shape = (len(d), int(n_sinusoids), int(n_taps))

    def fade_columns(self, col_khz):
        """The columns' carrier offsets in kHz (a host sequence); as many columns as it has entries.  In stream order."""
        k = self.np.ascontiguousarray(col_khz, self.np.int32)
        self._call("fade_columns", len(k), k.ctypes.data)

    def fade(self, fn, n_arfcn, n_frames, seed, n_links, doppler, taps, link=None):
        """taps: device complex64 [n_arfcn][8 n_frames][n_taps] (or float32 pairs), written; doppler: device uint32-sized words
        [n_links]; link: device int32 [n_arfcn][8 n_frames] or None (link = 8 a + t % 8)."""
        assert doppler.element_size() == 4 and (link is None or link.element_size() == 4)
        self._call("fade", int(fn), int(n_arfcn), int(n_frames), int(seed), _ptr(link), int(n_links), _ptr(doppler), _ptr(taps))
        self._keep = (link, doppler)

    def fade_params(self, seed, n_links, doppler, phase, step):
        """phase / step: device 32-bit words [n_links][P][S + 1], written: the integers behind the taps."""
        assert doppler.element_size() == 4 and phase.element_size() == 4 and step.element_size() == 4
        self._call("fade_params", int(seed), int(n_links), _ptr(doppler), _ptr(phase), _ptr(step))
        self._keep = (doppler,)


TRK_CLIPPED, TRK_UNLOCKED = 1, 2                          # trxsig_l1trk_meas.d_status bits (TRXSIG_TRK_*)
TRK_MAX_FRAMES, TRK_MAX_GATE = 65536, 1 << 24             # TRXSIG_L1TRK_MAX_FRAMES / _MAX_GATE


class L1Trk(_Object):
    """ctypes view of include/trxsig_l1trk.h: the handset's tracking receiver -- acquired streams -> the slot cells TrxGroup.pull
    reads, derotated by an exact NCO (slice), with the AFC measured on every frequency burst passed and the grid moved by the
    TOAs the pull reports (update)."""
    _prefix = "trxsig_l1trk"

    def __init__(self, ctx, phone, c0, max_frames, afc_shift=1, toa_gate=512, fcch_thresh=ACQ_FCCH_THRESH):
        """phone: the phone of every column; c0: every phone's C0 column, -1: none"""
        super().__init__(ctx)
        np = self.np
        phone, c0 = np.ascontiguousarray(phone, np.int32), np.ascontiguousarray(c0, np.int32)
        self.n_cols, self.n_phones = len(phone), len(c0)
        self._create(self.n_phones, self.n_cols, phone.ctypes.data, c0.ctypes.data, int(max_frames), int(afc_shift), int(toa_gate),
                     float(fcch_thresh))
        self.meas = None
        self._keep = None

    def seed(self, acq_out, src):
        """acq_out: the L1AcqOut of a search; src: device int32 [n_phones], the stream each phone was acquired on, -1: leave"""
        assert src.element_size() == 4 and src.numel() == self.n_phones
        self._call("seed", C.byref(acq_out), _ptr(src))
        self._keep = src

    def set(self, phone, locked, fn, pos, step, phase):
        self._call("set", int(phone), int(bool(locked)), int(fn), int(pos), int(step) & 0xffffffff, int(phase) & 0xffffffff)

    def slice(self, streams, stream_stride, n0, n_samples, fn, n_frames, cells, slot_stride, col_stride):
        """streams / cells: device tensors (complex64 or float32 pairs) or addresses; strides in complex samples"""
        out = L1TrkMeas()
        self._call("slice", _ptr(streams), int(stream_stride), int(n0), int(n_samples), int(fn), int(n_frames), _ptr(cells),
                   int(slot_stride), int(col_stride), C.byref(out))
        self.meas = out
        return out

    def update(self, res, fn, use=None):
        """res: the TrxGroupResult of the pull of the cells just sliced; use: device uint8 [n_slots][n_cols] or None"""
        self._call("update", C.byref(res), int(fn), _ptr(use))
        self._keep = use

    def state(self):
        v = L1TrkView()
        self._call("state", C.byref(v))
        return v

    def collect(self):
        """The state, what the last update did and the last slice's records as host numpy arrays (synchronises the stream)."""
        np, v, m = self.np, self.state(), self.meas
        self.ctx.synchronize()
        P = v.n_phones
        host = lambda p, shape, ts: _to_host(self.ctx, p, shape, ts)
        r = dict(fn=host(v.d_fn, (P,), "<i4"), pos=host(v.d_pos, (P,), "<i8"), phase=host(v.d_phase, (P,), "<i4").view(np.uint32),
                 step=host(v.d_step, (P,), "<i4").view(np.uint32), locked=host(v.d_locked, (P,), "|u1"), quiet=host(v.d_quiet, (P,), "<i4"),
                 toa_sum=host(v.d_toa_sum, (P,), "<i8"), toa_n=host(v.d_toa_n, (P,), "<i4"), adj=host(v.d_adj, (P,), "<i8"),
                 afc_n=host(v.d_afc_n, (P,), "<i4"), afc_delta=host(v.d_afc_delta, (P,), "<i8"))
        if m is not None:
            K, n = m.fcch_stride, m.n_fcch
            r.update(status=host(m.d_status, (v.n_cols,), "|u1"), n_fcch=n, fcch_fn=host(m.d_fcch_fn, (P, K), "<i4")[:, :n],
                     fcch_c=host(m.d_fcch_c, (P, K, 2), "<f8")[:, :n].copy().view(np.complex128)[..., 0],
                     fcch_e=host(m.d_fcch_e, (P, K), "<f8")[:, :n], fcch_ok=host(m.d_fcch_ok, (P, K), "|u1")[:, :n])
        return r


A5_OFF, A5_1 = 0, 1                                      # trxsig_l1ciph_set's algo (TRXSIG_A5_*)
L1CIPH_STATE_BYTES = 16                                  # TRXSIG_L1CIPH_STATE_BYTES: uint32 algo, R1, R2, R3


def a5_1_blocks(ctx, kc, count, block1=None, block2=None):
    """trxsig_a5_1_blocks_batch: kc device uint8 [n][8], count device int32 / uint32 [n] -> BLOCK1 / BLOCK2 device uint8
    [n][114], one bit per byte (either may be None).  Enqueued on the context's stream."""
    L = ctx.L
    n = int(count.numel()) if hasattr(count, "numel") else 0
    rc = L.trxsig_a5_1_blocks_batch(ctx.h, n, _ptr(kc), _ptr(count), _ptr(block1), _ptr(block2))
    if rc < 0:
        raise TrxSigError("trxsig_a5_1_blocks_batch: %d (%s)" % (rc, L.trxsig_last_error(ctx.h).decode()))


class L1Ciph(_PlanView):
    """ctypes view of include/trxsig_l1ciph.h: A5/1 ciphering of the dedicated channels' bursts -- bits() on an encoder's burst
    grid before it is sent, soft() on a pull's rows before they are decoded; a key per TCH / XCCH channel (set).
    comb: uint8 [n_arfcn, 8] as L1Rx takes it."""
    _prefix = "trxsig_l1ciph"

    def __init__(self, ctx, comb):
        super().__init__(ctx, comb)

    def set(self, cls, chan, algo, kc=None):
        """algo: A5_OFF or A5_1; kc: 8 key bytes (host).  Takes effect in stream order."""
        key = None if kc is None else (C.c_uint8 * 8)(*[int(x) & 0xff for x in kc])
        self._call("set", int(cls), int(chan), int(algo), key)

    def bits(self, uplink, fn, n_frames, bits, what=None, what_mask=0):
        """bits: device uint8 [n_arfcn][8 n_frames][148] (a tensor or an address: an encoder's d_bits), ciphered in place; what:
        its [n_arfcn][8 n_frames] map or None"""
        self._call("bits", int(bool(uplink)), int(fn), int(n_frames), _ptr(bits), _ptr(what), int(what_mask) & 0xffffffff)

    def soft(self, uplink, res, fn):
        """res: a TrxGroupResult of whole frames from (fn, TN 0); its soft rows are deciphered in place, once"""
        self._call("soft", int(bool(uplink)), C.byref(res), int(fn))

    def collect(self):
        """The channels' records as host numpy arrays uint32 [n_chan][4] per class (synchronises the context's stream)."""
        self.ctx.synchronize()
        return {name: _to_host(self.ctx, self.state(cls), (self.channels(cls), 4), "<i4").view(self.np.uint32)
                for name, cls in (("tch", L1_TCH), ("xcch", L1_XCCH))}


def pdch_map(fn):
    """trxsig_pdch_map_host: frame fn of the packet channel's 52-multiframe -> (block 0..11, burst 0..3), or (-1, -1) on the
    PTCCH (12, 38) and idle (25, 51) frames.  No device, no context."""
    block, burst = C.c_int(), C.c_int()
    rc = lib().trxsig_pdch_map_host(int(fn), C.byref(block), C.byref(burst))
    if rc < 0:
        raise TrxSigError("trxsig_pdch_map_host(%d): %d" % (fn, rc))
    return block.value, burst.value


L1HOP_MAX_N = 64                                         # TRXSIG_L1HOP_MAX_N


def hop_mai(ctx, fn, hsn, maio, n, mai):
    """trxsig_hop_mai_batch: device int32 arrays of equal length, mai[i] = MAI(fn[i], hsn[i], maio[i], n[i]) (GSM 05.02 6.2.3).
    Entries out of range are undefined.  Enqueued on the context's stream."""
    L = ctx.L
    cnt = int(fn.numel()) if hasattr(fn, "numel") else 0
    rc = L.trxsig_hop_mai_batch(ctx.h, cnt, _ptr(fn), _ptr(hsn), _ptr(maio), _ptr(n), _ptr(mai))
    if rc < 0:
        raise TrxSigError("trxsig_hop_mai_batch: %d (%s)" % (rc, L.trxsig_last_error(ctx.h).decode()))


class L1Hop(_Object):
    """ctypes view of include/trxsig_l1hop.h: slow frequency hopping of the dedicated channels -- bits() on an encoder's burst
    grid (in place), cells() on sample cells (out of place), result() on a pull (indices only), map() the radio row of every
    channel row.  comb: uint8 [n_arfcn, 8] as L1Rx takes it; group: int8 [n_arfcn, 8], -1 or a group id; hsn: one per group;
    max_frames: the longest map() / result() call."""
    _prefix = "trxsig_l1hop"

    def __init__(self, ctx, comb, group, hsn, max_frames=104):
        super().__init__(ctx)
        np = self.np
        self.comb = np.ascontiguousarray(comb, np.uint8)
        self.group = np.ascontiguousarray(group, np.int8)
        self.hsn = np.ascontiguousarray(hsn, np.uint8).reshape(-1)
        if self.group.shape != self.comb.shape:
            raise TrxSigError("L1Hop: comb and group differ in shape")
        self.n_arfcn = self.comb.shape[0]
        self._create(self.n_arfcn, self.comb.ctypes.data, self.group.ctypes.data, len(self.hsn),
                     self.hsn.ctypes.data if len(self.hsn) else None, int(max_frames))

    def groups(self):
        return self._call("groups")

    def members(self, g, tn):
        """the rows of group g on timeslot tn, ascending: a row's place in the list is its MAIO"""
        rows = (C.c_int32 * L1HOP_MAX_N)()
        n = self._call("members", int(g), int(tn), rows)
        return list(rows[:n])

    def map(self, fn, n_frames):
        """device int32 [8 n_frames][n_arfcn] (a view of the object's array, valid until the next map): the radio row of channel
        row a in slot t"""
        p = C.c_void_p()
        self._call("map", int(fn), int(n_frames), C.byref(p))
        return _dev_tensor(self.ctx, p.value, (8 * int(n_frames), self.n_arfcn), "<i4")

    def bits(self, to_radio, fn, n_frames, bits, what=None):
        """bits: device uint8 [n_arfcn][8 n_frames][148] (a tensor or an address: an encoder's d_bits), hopped in place together
        with what, its [n_arfcn][8 n_frames] map (or None)"""
        self._call("bits", int(bool(to_radio)), int(fn), int(n_frames), _ptr(bits), _ptr(what))

    def cells(self, to_radio, fn, n_frames, src, in_slot_stride, in_arfcn_stride, dst, out_slot_stride, out_arfcn_stride):
        """src, dst: device complex64 cells (tensors or addresses), strides in samples; out of place"""
        self._call("cells", int(bool(to_radio)), int(fn), int(n_frames), _ptr(src), int(in_slot_stride), int(in_arfcn_stride),
                   _ptr(dst), int(out_slot_stride), int(out_arfcn_stride))

    def result(self, res, fn):
        """res: a TrxGroupResult of whole frames from (fn, TN 0) -> a copy whose d_row is in the channel domain (the object's
        array, valid until the next result; self.row is that array as a tensor)"""
        out = TrxGroupResult()
        self._call("result", int(fn), C.byref(res), C.byref(out))
        self.row = _dev_tensor(self.ctx, out.d_row, (out.n_slots, out.n_arfcn), "<i4")
        return out


L1PDCH_DOWN, L1PDCH_UP = 0, 1                    # TRXSIG_L1PDCH_DOWN / _UP
L1PDCH_PDTCH, L1PDCH_PTCCH = 0, 1                # the channel classes of trxsig_l1pdch.h
L1PDCH_COMB = 13                                 # TRXSIG_L1PDCH_COMB: a packet data channel in comb
L1TX_PDCH = 8                                    # TRXSIG_L1TX_PDCH: the d_what code of a slot L1Pdch wrote
L1PDCH_STATE_BYTES, L1PDCH_RING = 3104, 32       # TRXSIG_L1PDCH_STATE_BYTES, TRXSIG_L1PDCH_RING


class L1Pdch(_Object):
    """ctypes view of include/trxsig_l1pdch.h: packet data channels through L1 -- payloads of the PDCH slots (13 in comb) to timed
    bursts and a Transceiver group pull to payloads, on the device.  direction: L1PDCH_DOWN or L1PDCH_UP."""
    _prefix = "trxsig_l1pdch"

    def __init__(self, ctx, comb, bsic, direction):
        super().__init__(ctx)
        self.comb = self.np.ascontiguousarray(comb, self.np.uint8)
        self._create(self.comb.shape[0], self.comb.ctypes.data, int(bsic), int(direction))
        self.out = self.dec = self._keep = None

    def circuit_plan(self):
        """comb with the packet slots as 0: what L1Tx / L1Rx / L1Ms / L1MsRx and the group take."""
        return self.np.where(self.comb == L1PDCH_COMB, 0, self.comb).astype(self.np.uint8)

    def channels(self, cls):
        return self._call("channels", cls)

    def channel(self, cls, chan):
        """(arfcn, tn) of a channel"""
        v = [C.c_int() for _ in range(2)]
        self._call("channel", cls, chan, *[C.byref(x) for x in v])
        return tuple(x.value for x in v)

    def grid(self, fn, n_frames):
        """(nb_pdtch, nb_ptcch) of an encode call"""
        v = [C.c_int() for _ in range(2)]
        self._call("grid", int(fn), int(n_frames), *[C.byref(x) for x in v])
        return tuple(x.value for x in v)

    def state(self, cls):
        p = C.c_void_p()
        self._call("state", cls, C.byref(p))
        return p.value

    def encode(self, fn, n_frames, pdtch_kind=None, pdtch_cs=None, pdtch_payload=None, ptcch_kind=None, ptcch_payload=None,
               bits_onto=None, what_onto=None):
        """Grids as torch uint8 tensors on the context's device (None for a class without channels); bits_onto / what_onto:
        tensors or device addresses of a grid to overlay (L1Tx's out.d_bits / out.d_what), or None for the object's own grid."""
        ins, out = L1PdchIn(), L1PdchOut()
        keep = _fill(ins, None, (pdtch_kind, pdtch_cs, pdtch_payload, ptcch_kind, ptcch_payload), itemsize=1, empty_as_one=True)
        self._call("encode", int(fn), int(n_frames), C.byref(ins), _ptr(bits_onto), _ptr(what_onto), C.byref(out))
        self._keep = keep + (bits_onto, what_onto)
        self.out = out
        return out

    def decode(self, res, fn, wire=True, cs_force=-1, sibling=None):
        """res: a TrxGroupResult of whole frames from (fn, TN 0)."""
        out = L1PdchDec()
        self._call("decode", C.byref(res), int(fn), int(bool(wire)), int(cs_force), sibling.h if sibling is not None else None,
                   C.byref(out))
        self.dec = out
        return out

    def states(self):
        """{class: the channel records, uint8 [n, L1PDCH_STATE_BYTES]} on the host (synchronises)."""
        self.ctx.synchronize()
        return {cls: _to_host(self.ctx, self.state(cls), (self.channels(cls), L1PDCH_STATE_BYTES), "|u1")
                for cls in (L1PDCH_PDTCH, L1PDCH_PTCCH)}

    def collect(self):
        """The last encode's grid as host numpy arrays (synchronises the context's stream)."""
        o = self.out
        self.ctx.synchronize()
        A, F = o.n_arfcn, o.n_frames
        return dict(bits=_to_host(self.ctx, o.d_bits, (A, 8 * F, 148), "|u1"), what=_to_host(self.ctx, o.d_what, (A, 8 * F), "|u1"))

    def collect_decode(self):
        """The last decode's outputs as host numpy arrays (synchronises the context's stream)."""
        o = self.dec
        self.ctx.synchronize()
        host = lambda p, shape, ts: _to_host(self.ctx, p, shape, ts)
        r = {}
        for name, n, nb, np_ in (("pdtch", o.n_pdtch, o.nb_pdtch, 54), ("ptcch", o.n_ptcch, o.nb_ptcch, 23)):
            get = lambda f: getattr(o, "d_%s_%s" % (name, f))
            r[name] = dict(payload=host(get("payload"), (n, nb, np_), "|u1"), fn=host(get("fn"), (n, nb), "<i4"),
                           rssi=host(get("rssi"), (n,), "<i4"), timing=host(get("timing"), (n,), "<i4"),
                           **{f: host(get(f), (n, nb), "|u1") for f in ("cs", "cs_dist", "ok", "usf", "nb", "granted")})
        return r


L1TX_PACC = 9                                    # TRXSIG_L1TX_PACC: the d_what code of a slot L1Pacc wrote
L1PACC_NONE, L1PACC_PTCCH, L1PACC_PRACH = 0, 1, 2   # d_kind of a frame in L1Pacc.detect's outputs
L1PACC_STATE_BYTES = 144                         # TRXSIG_L1PACC_STATE_BYTES


class L1Pacc(_Object):
    """ctypes view of include/trxsig_l1pacc.h: packet access through L1 -- a handset's access bursts on the PTCCH/U frames and
    PRACH blocks of the PDCH slots (13 in comb) to timed bursts; a base station's detector on those frames of the slot cells, the
    timing advances per TAI and the PTCCH/D message; a handset's reading of that message."""
    _prefix = "trxsig_l1pacc"

    def __init__(self, ctx, comb, bsic):
        super().__init__(ctx)
        self.comb = self.np.ascontiguousarray(comb, self.np.uint8)
        self._create(self.comb.shape[0], self.comb.ctypes.data, int(bsic))
        self.out = self.det = self._keep = None

    def channels(self):
        return self._call("channels")

    def channel(self, chan):
        """(arfcn, tn) of a PDCH"""
        v = [C.c_int() for _ in range(2)]
        self._call("channel", chan, *[C.byref(x) for x in v])
        return tuple(x.value for x in v)

    def grid(self, fn, n_frames):
        """nb: the blocks with a frame in the call"""
        v = C.c_int()
        self._call("grid", int(fn), int(n_frames), C.byref(v))
        return v.value

    def state(self):
        p = C.c_void_p()
        self._call("state", C.byref(p))
        return p.value

    def encode(self, fn, n_frames, ptcch_kind, ptcch_ra, prach_kind, prach_ra, fmt=0, bits_onto=None, what_onto=None):
        """ptcch_kind [n, 16] uint8, ptcch_ra [n, 16] int16, prach_kind [n, nb, 4] uint8, prach_ra [n, nb, 4] int16 (the 16 bits
        of a uint16) on the context's device; bits_onto / what_onto: a grid to overlay, or None for the object's own."""
        ins, out = L1PaccIn(), L1PaccOut()
        ins.fmt = int(fmt)
        keep = _fill(ins, None, (ptcch_kind, ptcch_ra, prach_kind, prach_ra), empty_as_one=True)
        self._call("encode", int(fn), int(n_frames), C.byref(ins), _ptr(bits_onto), _ptr(what_onto), C.byref(out))
        self._keep = keep + (bits_onto, what_onto)
        self.out = out
        return out

    def detect(self, samples, slot_stride, arfcn_stride, fn, n_frames, prach=None, fmt=-1, leg=RACHLEG_DEMOD, detect_thresh=5.0,
               energy_thresh=-1.0, wire=True):
        """samples: the slot cells (a tensor or a device address); prach: a HOST uint8 array [n, nb] (nonzero: a PRACH block) or None."""
        out = L1PaccDet()
        h = None if prach is None else self.np.ascontiguousarray(prach, self.np.uint8)
        self._call("detect", _ptr(samples), int(slot_stride), int(arfcn_stride), int(fn), int(n_frames),
                   None if h is None else h.ctypes.data, int(fmt), int(leg), float(detect_thresh), float(energy_thresh), int(bool(wire)),
                   C.byref(out))
        self.det = out
        return out

    def ta_message(self, kind, payload, nb_pt):
        """kind [n, nb_pt], payload [n, nb_pt, 23] uint8 on the device: L1Pdch.encode's PTCCH inputs."""
        self._call("ta_message", _ptr(kind), _ptr(payload), int(nb_pt))

    def ta_read(self, dec, ta):
        """dec: the L1PdchDec of a handset's decode; ta [n, 16] uint8 on the device, updated where a PTCCH/D block came with ok."""
        self._call("ta_read", C.byref(dec), _ptr(ta))

    def states(self):
        """The PDCHs' tables as dict(ta, fn: int32 [n, 16]; valid: uint8 [n, 16]) on the host (synchronises)."""
        self.ctx.synchronize()
        n = self.channels()
        raw = _to_host(self.ctx, self.state(), (n, L1PACC_STATE_BYTES), "|u1")
        return dict(ta=raw[:, :64].copy().view("<i4"), fn=raw[:, 64:128].copy().view("<i4"), valid=raw[:, 128:].copy())

    def collect(self):
        """The last encode's grid and the last detect's outputs as host numpy arrays (synchronises the context's stream)."""
        self.ctx.synchronize()
        r = {}
        if self.out is not None:
            o = self.out
            A, F = o.n_arfcn, o.n_frames
            r.update(bits=_to_host(self.ctx, o.d_bits, (A, 8 * F, 148), "|u1"), what=_to_host(self.ctx, o.d_what, (A, 8 * F), "|u1"))
        if self.det is not None:
            d = self.det
            shape = (d.n_pdch, d.n_frames)
            for name, ts in (("kind", "|u1"), ("tai", "|i1"), ("det", "|u1"), ("fmt", "|u1"), ("ok", "|u1"), ("toa", "<f4"),
                             ("avgpwr", "<f4"), ("ta", "|u1")):
                r[name] = _to_host(self.ctx, getattr(d, "d_" + name), shape, ts)
            r["amp"] = _to_host(self.ctx, d.d_amp, shape + (2,), "<f4")
            r["ra"] = _to_host(self.ctx, d.d_ra, shape, "<i2").view("<u2")      # (16 bits a word: torch has no unsigned view of them)
        return r
