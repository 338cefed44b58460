"""The binding's shared plumbing on the device: every entry point is typed when the library is loaded (_abi.SIGNATURES), the
eleven object classes share one base (_Object / _PlanView / _PlanObject), and collect() reads the device through one helper
(_to_host).  Every refusal below is a host-side argument check that the stages' own suites make too; nothing is launched for it."""
import ctypes as C
import re

import numpy as np
import pytest

import _pkg

pytestmark = pytest.mark.gpu
PLAN = np.array([[5, 7, 1, 0, 0, 0, 0, 0]], np.uint8)       # one ARFCN: combination V, a VII and a I
BEACON_ONLY = np.array([[5, 0, 0, 0, 0, 0, 0, 0]], np.uint8)   # no TCH at all


def test_binding_plumbing():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    pkg = _pkg.load()
    ctx = pkg.TrxSig(4, 0)
    ctx.use_torch_stream()
    L = ctx.L
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()

    # a raw call before any L1Hop of this function exists: the handle is a 64-bit address, which only a typed call passes whole
    comb = np.array([[5, 1, 0, 0, 0, 0, 0, 0], [0, 1, 0, 0, 0, 0, 0, 0]], np.uint8)
    group = np.full((2, 8), -1, np.int8); group[:, 1] = 0
    hsn = np.array([5], np.uint8)
    h = C.c_void_p()
    assert L.trxsig_l1hop_create(C.byref(h), ctx.h, 2, comb.ctypes.data, group.ctypes.data, 1, hsn.ctypes.data, 2) == 0 and h.value
    assert L.trxsig_l1hop_groups(h) == 1 and L.trxsig_l1hop_groups(h.value) == 1
    L.trxsig_l1hop_destroy(h)

    # one of each class, at the smallest arguments their own suites use
    plan = {"L1Rx": pkg.L1Rx(ctx, PLAN, 1), "L1Tx": pkg.L1Tx(ctx, PLAN, 1), "L1Ms": pkg.L1Ms(ctx, PLAN, 1),
            "L1MsRx": pkg.L1MsRx(ctx, PLAN, 1), "L1Ciph": pkg.L1Ciph(ctx, PLAN)}
    rest = {"L1Acq": pkg.L1Acq(ctx, 2, 1000), "Air": pkg.Air(ctx, 4), "L1Trk": pkg.L1Trk(ctx, [0, 0, 1], [0, 2], 4),
            "L1Hop": pkg.L1Hop(ctx, comb, group, hsn, max_frames=2), "TrxGroup": pkg.TrxGroup(ctx, 1, tsc_leg=pkg.TSCLEG_DEMOD),
            "TrxHost": pkg.TrxHost(4, 0)}
    for name, o in {**plan, **rest}.items():
        assert o.h and o.L is not None and o.np is np, name
        assert name == "TrxHost" or o.ctx is ctx, name
    hop = rest["L1Hop"]
    assert hop.groups() == 1 and hop.members(0, 1) == [0, 1] and (hop.n_arfcn, list(hop.hsn)) == (2, [5])
    assert np.array_equal(hop.comb, comb) and np.array_equal(hop.group, group)
    assert tuple(hop.map(0, 2).shape) == (16, 2)
    assert (rest["L1Trk"].n_cols, rest["L1Trk"].n_phones, rest["TrxGroup"].S, rest["TrxGroup"].n_slots) == (3, 2, 1, 0)

    # the plan as the five plan classes state it: one answer
    rx = plan["L1Rx"]
    for cls in (pkg.L1_TCH, pkg.L1_XCCH):
        n = rx.channels(cls)
        assert n > 0
        where = [rx.channel(cls, i) for i in range(n)]
        assert len(set(where)) == n and all(len(w) == 4 and w[0] == 0 and w[1] in (0, 1, 2) for w in where)
        for name, o in plan.items():
            assert o.channels(cls) == n and [o.channel(cls, i) for i in range(n)] == where, (name, cls)
            assert isinstance(o.state(cls), int) and o.state(cls) != 0, (name, cls)
            assert np.array_equal(o.comb, PLAN), name
    assert len({o.state(pkg.L1_TCH) for o in plan.values()}) == 5        # (each object's own array)
    for name in ("L1Rx", "L1Tx", "L1Ms", "L1MsRx"):
        plan[name].close(pkg.L1_TCH, 0); plan[name].open(pkg.L1_TCH, 0)
    assert not hasattr(plan["L1Ciph"], "open")

    # collect() where a class has no channel: zero-row arrays of the documented dtypes
    ms0, rx0 = pkg.L1Ms(ctx, BEACON_ONLY, 1), pkg.L1Rx(ctx, BEACON_ONLY, 1)
    assert ms0.channels(pkg.L1_TCH) == 0 == rx0.channels(pkg.L1_TCH) and rx0.channels(pkg.L1_XCCH) > 0
    z = dev(np.zeros((64, 64, 33), np.uint8))
    ms0.encode(0, 1, xcch_kind=z, xcch_payload=z, rach_kind=z, rach_ra=z)
    assert ms0._keep[0] is None and ms0._keep[2] is z
    g = ms0.collect()
    X = ms0.channels(pkg.L1_XCCH)
    assert g["tch_state"].shape == (0, pkg.L1MS_STATE_BYTES) and g["tch_state"].dtype == np.uint8
    assert g["xcch_state"].shape == (X, pkg.L1MS_STATE_BYTES) and g["xcch_state"].dtype == np.uint8
    assert g["bits"].shape == (1, 8, 148) and g["bits"].dtype == np.uint8 and g["what"].shape == (1, 8)
    assert g["ms_power"].shape == (X,) and g["ms_power"].dtype == np.int32 and g["ms_ta"].dtype == np.int32
    t = dict(row=dev(np.arange(8, dtype=np.int32).reshape(8, 1)), valid=dev(np.zeros(8, np.uint8)), amp=dev(np.zeros((8, 2), np.float32)),
             toa=dev(np.zeros(8, np.float32)), soft=dev(np.zeros((8, 148), np.float32)))
    res = pkg.TrxGroupResult(n_slots=8, n_arfcn=1, n_rows=8, d_row=t["row"].data_ptr(), d_valid=t["valid"].data_ptr(), d_flags=None,
                             d_amp=t["amp"].data_ptr(), d_toa=t["toa"].data_ptr(), d_avgpwr=None, d_threshold=None,
                             d_soft=t["soft"].data_ptr(), soft_stride=148)
    out = rx0.decode(res, 0)
    assert out is rx0.out and out.n_tch == 0
    g = rx0.collect()
    bt = out.nb_tch
    for key, shape, dtype in (("tch_status", (0, bt), np.uint8), ("tch", (0, bt, 33), np.uint8), ("facch", (0, bt, 23), np.uint8),
                              ("tch_fer", (0, bt), np.float32), ("tch_fn", (0, bt), np.int32), ("tch_rssi", (0,), np.int32),
                              ("tch_timing", (0,), np.int32), ("tch_state", (0, pkg.TCH_RX_STATE_BYTES), np.uint8)):
        assert g[key].shape == shape and g[key].dtype == dtype, key
    assert g["xcch_state"].shape == (out.n_xcch, pkg.XCCH_RX_STATE_BYTES) and g["xcch_fer"].dtype == np.float32
    assert g["xcch_status"].shape == (out.n_xcch, out.nb_xcch) and g["rach"]["ra"].dtype == np.uint8

    # a refusal reads "<call>: <rc> (<the context's last error>)".  trxsig_l1rx_channel records no text of its own, so the
    # bracket holds what the context refused last: a decode from a frame number that is none, made first.
    with pytest.raises(pkg.TrxSigError, match=r"^trxsig_l1rx_decode: -\d+ \(trxsig_l1rx_decode: bad argument.*\)$"):
        rx.decode(res, -1)
    last = L.trxsig_last_error(ctx.h).decode()
    with pytest.raises(pkg.TrxSigError, match=r"^trxsig_l1rx_channel: -\d+ \(.+\)$") as e:
        rx.channel(pkg.L1_TCH, 10 ** 6)
    assert str(e.value) == "trxsig_l1rx_channel: -1 (%s)" % last and re.match(r"^trxsig_l1rx_decode: bad argument", last)
    with pytest.raises(pkg.TrxSigError, match=r"^trxsig_l1rx_create failed \(-1\): .+$"):
        pkg.L1Rx(ctx, PLAN, 64)                              # (a BSIC is six bits)

    # destructors: twice, nothing raised, the handle gone
    for name, o in list(plan.items()) + list(rest.items()) + [("L1Ms", ms0), ("L1Rx", rx0)]:
        end = o.close if name in ("TrxGroup", "TrxHost") else o.destroy
        end(); end()
        assert not o.h, name
    ctx.close(); ctx.close()
    assert not ctx.h
