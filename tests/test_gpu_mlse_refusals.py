"""What the twelve sequence-equaliser entry points of the C ABI refuse, and with which words (trxsig_last_error), on a live context
at sps 1 and 4: one table.  A refusal is TRXSIG_EINVAL, raised as TrxSigError with the entry point's own text -- or, for the
detect-then-equalise calls, the detector's where its check is the one that fires -- and leaves every canaried output as it was
(tests/mlse_run.py's canaries, and 77 / 1.0 in the detector's outputs).  The cases: nsoft 149 and -1, a stride below nsoft, tsc -1
and 8, each required pointer NULL in turn, a loading of -0.1, 16.1 and NaN, and a NaN loading on an empty batch (judged before the
B == 0 return).  Accepted: an empty batch with every pointer NULL (a no-op), nsoft = 0 (no soft or hard bit written), the loadings
0 and 16.  The calls go through the typed C functions and the binding's _chk, so that a NULL d_offset can be passed."""
import numpy as np
import pytest

import mlse_irc_family as ifam
from mlse_run import canaries, ctx, dev, pkg  # noqa: F401  (the fixtures)

pytestmark = pytest.mark.gpu
B = 2
ONE = "x0 off0 len B %s amp toa en chan win soft hard nsoft stride"
ONE_DET = "x0 off0 len B %s dth eth flags_o amp_o toa_o pwr_o chan win soft hard nsoft stride"
TWO = "x0 off0 x1 off1 len B tsc amp toa prim en %s chan2 win soft hard nsoft stride"
TWO_DET = "x0 off0 x1 off1 len B tsc dth eth %s flags_o amp_o toa_o pwr_o sel_o %s chan2 win soft hard nsoft stride"
DETECT_NORMAL, DETECT_RACH = "trxsig_detect_demod_normal_batch: bad argument", "trxsig_detect_demod_rach_batch: bad argument"
# name: (arguments in the header's order, required pointers, its refusal text, the cases that carry `other` instead, other)
ENTRIES = {
    "trxsig_mlse_batch": ((ONE % "tsc").split(), "x0 off0 len amp toa soft", "trxsig_mlse_batch: bad argument", "", None),
    "trxsig_mlse_normal_batch": ((ONE_DET % "tsc").split(), "x0 off0 len flags_o amp_o toa_o soft", "trxsig_mlse_normal_batch: bad argument",
                                 "tsc x0 off0 len flags_o amp_o toa_o", DETECT_NORMAL),
    "trxsig_mlse_access_batch": ((ONE % "").split(), "x0 off0 len amp toa soft", "trxsig_mlse_access_batch: bad argument", "", None),
    "trxsig_mlse_rach_batch": ((ONE_DET % "").split(), "x0 off0 len flags_o amp_o toa_o soft", "trxsig_mlse_rach_batch: bad argument",
                               "x0 off0 len flags_o amp_o toa_o", DETECT_RACH),
    "trxsig_mlse_access_pinv_host": (["pinv"], "pinv", None, "", None),
    "trxsig_mlse_sch_batch": ((ONE % "").split(), "x0 off0 len amp toa soft", "trxsig_mlse_sch_batch: bad argument", "", None),
    "trxsig_mlse_sch_pinv_host": (["pinv"], "pinv", None, "", None),
    "trxsig_sch_fit_batch": ("x0 off0 len B amp toa en chan9 win E R q".split(), "x0 off0 len amp toa", "trxsig_sch_fit_batch: bad argument", "", None),
    "trxsig_mlse_div_batch": ((TWO % "").split(), "x0 off0 x1 off1 len amp toa soft", "trxsig_mlse_div_batch: bad argument", "", None),
    "trxsig_mlse_div_normal_batch": ((TWO_DET % ("", "")).split(), "x0 off0 x1 off1 len flags_o amp_o toa_o sel_o soft",
                                     "trxsig_mlse_div_normal_batch: bad argument", "", None),
    "trxsig_mlse_irc_batch": ((TWO % "loading cov_in cov").split(), "x0 off0 x1 off1 len amp toa soft", "trxsig_mlse_irc_batch: bad argument",
                              "loading", "trxsig_mlse_irc_batch: loading outside 0..16"),
    "trxsig_mlse_irc_normal_batch": ((TWO_DET % ("loading", "cov")).split(), "x0 off0 x1 off1 len flags_o amp_o toa_o sel_o soft",
                                     "trxsig_mlse_irc_normal_batch: bad argument", "", None),
}
CANARY = dict(soft=-1.0, hard=255, chan=-7.0, chan2=-7.0, chan9=-7.0, win=-99, cov=-5.0, E=-7.0, R=-7.0, q=-7.0, flags_o=77, amp_o=1.0, toa_o=1.0,
              pwr_o=1.0, sel_o=9, pinv=-3.0)
EINVAL = -1


def buffers(sps):
    """Every argument by name: two bursts of tests/mlse_irc_family.py's batch on the device, the canaried outputs, the scalars."""
    import torch
    f = ifam.mixed_batch(sps, 2, B, 6400 + sps)
    full = lambda shape, v, ty=torch.float32: torch.full(shape, v, dtype=ty, device="cuda:0")
    a = dict(x0=dev(f["x0"]), off0=dev(f["off0"]), x1=dev(f["x1"]), off1=dev(f["off1"]), len=dev(f["length"]), amp=dev(f["amp"]), toa=dev(f["toa"]),
             prim=dev(np.asarray(f["primary"], np.uint8)), en=None, cov_in=None, B=B, tsc=2, dth=3.0, eth=-1.0, loading=1.0 / 64.0, nsoft=148,
             stride=160, soft=full((B, 160), -1.0), hard=full((B, 160), 255, torch.uint8), chan2=canaries(B, (2, 5))["chan"],
             chan9=canaries(B, (9,))["chan"], flags_o=full((2, B), 77, torch.uint8), amp_o=full((2, B, 2), 1.0), toa_o=full((2, B), 1.0),
             pwr_o=full((2, B), 1.0), sel_o=full((B,), 9, torch.uint8), pinv=full((9, 56), -3.0).cpu(), E=full((B,), -7.0), R=full((B,), -7.0),
             q=full((B,), -7.0))
    a.update(canaries(B, cov=True))
    return a


def call(t, name, a, **change):
    """The entry point on a's arguments with `change` applied; raises TrxSigError with trxsig_last_error's text on a refusal."""
    v = dict(a, **change)
    args = [v[k].data_ptr() if hasattr(v[k], "data_ptr") else v[k] for k in ENTRIES[name][0]]
    if name.endswith("_pinv_host"):
        return getattr(t.L, name)(*args)
    return t._chk(getattr(t.L, name)(t.h, *args), name)


@pytest.mark.parametrize("name", list(ENTRIES))
@pytest.mark.parametrize("sps", [1, 4])
def test_refusals_and_their_words(pkg, ctx, sps, name):
    import torch
    t, a = ctx[sps], buffers(sps)
    arglist, need, text, other_cases, other = ENTRIES[name]
    outputs = {k: a[k].clone() for k in arglist if k in CANARY}
    assert all(bool((v == CANARY[k]).all()) for k, v in outputs.items())

    def untouched(what):
        torch.cuda.synchronize()
        for k, v in outputs.items():
            assert torch.equal(a[k], v), "%s: %s wrote %s" % (name, what, k)

    if text is None:                                           # the two table copies: no context, no text
        assert call(t, name, a, pinv=None) == EINVAL
        untouched("a NULL table")
        assert call(t, name, a) == 0 and not bool((a["pinv"] == -3.0).all())
        return
    cases = [(k, {k: None}) for k in need.split()]
    if "nsoft" in arglist:
        cases += [("nsoft", dict(nsoft=149)), ("nsoft", dict(nsoft=-1)), ("stride", dict(nsoft=148, stride=147))]
    if "tsc" in arglist:
        cases += [("tsc", dict(tsc=-1)), ("tsc", dict(tsc=8))]
    if "loading" in arglist:
        cases += [("loading", dict(loading=v)) for v in (-0.1, 16.1, float("nan"))] + [("loading", dict(loading=float("nan"), B=0))]
    for key, change in cases:
        with pytest.raises(pkg.TrxSigError) as e:
            call(t, name, a, **change)
        want = other if key in other_cases.split() else text
        assert want in str(e.value) and "(%d)" % EINVAL in str(e.value), (name, change, str(e.value))
        untouched("a refused call (%r)" % (change,))
    # accepted: an empty batch with every pointer NULL, nsoft = 0, the loading's bounds
    call(t, name, dict((k, None if hasattr(v, "data_ptr") else v) for k, v in a.items()), B=0)
    untouched("an empty batch")
    if "nsoft" in arglist:
        call(t, name, a, nsoft=0, stride=0)
        torch.cuda.synchronize()
        assert torch.equal(a["soft"], outputs["soft"]) and torch.equal(a["hard"], outputs["hard"]), name + ": nsoft = 0 wrote bits"
    if "loading" in arglist:
        for loading in (0.0, 16.0):
            call(t, name, a, loading=loading)
        torch.cuda.synchronize()
        assert bool((a["soft"][:, :148] >= 0.0).all())
