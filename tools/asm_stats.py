#!/usr/bin/env python3
"""Static instruction mix per kernel from `make -C openbts-ttsou_amd/csrc asm` output, and a check that
every float multiply-add in the kernels belongs to a division / sqrt expansion: the numerical contract
forbids contracted multiply-adds anywhere else.  The intended exceptions are counted apart, each as its own kind: the
marked ones (exact-product, steering, approx-form, soft-tolerance: inline asm with a marker comment), and two that the
compiler emits for code that is not float arithmetic of the kernel's values -- the reciprocal estimate of an integer
division (int-division) and the device library's double log / log10 (libm-log)."""
import re
import sys
from collections import Counter

# every float multiply-add form: v_fma / v_fmac / v_mac / v_mad, the literal forms (v_fmamk / v_fmaak / v_madmk / v_madak),
# packed, legacy and mixed-precision ones (integer v_mad_u32_u24 / v_mad_u64_u32 ... are not float)
FMA = re.compile(r"v_(pk_)?(fma|fmac|mac|mad|fmamk|fmaak|madmk|madak)(_legacy)?_f(16|32|64)|v_(fma|mad)_mix")


def regs(i):
    """the operand fields of an instruction (destination first), modifiers stripped"""
    return [re.sub(r"[-|]", "", x).strip() for x in i.split(None, 1)[1].split(",")] if " " in i else []


def int_division(ins, ops, k):
    """The f32 multiply-adds of the compiler's integer division expansions (AMDGPU's 64-bit udiv / urem and the 24-bit
    div / rem form): a float reciprocal estimate of integer operands, corrected in integer arithmetic afterwards.
      64-bit: hi * 2^32 + lo -> v_rcp_f32, and q_lo = fma(q_hi, -2^32, r) between v_trunc_f32 and v_cvt_u32_f32
      24-bit: r = fma(-q, b, a) with q = v_trunc_f32(a * rcp(b)), then v_cmp_ge_f32 |r|, |b| decides the +-1 step"""
    i, r = ins[k], regs(ins[k])
    if not r or not ops[k].endswith(("f32", "f32_e32", "f32_e64")):
        return False
    near = lambda lo, hi: [(ops[x], regs(ins[x])) for x in range(max(0, lo), min(len(ops), hi))]
    if "0x4f800000" in i:
        return any(o.startswith("v_rcp_f32") and r[0] in rr[1:] for o, rr in near(k + 1, k + 4))
    if "0xcf800000" in i:
        return any(o.startswith("v_trunc_f32") and rr[0] in r[1:] for o, rr in near(k - 3, k)) and \
            any(o.startswith("v_cvt_u32_f32") and r[0] in rr[1:] for o, rr in near(k + 1, k + 4))
    if ops[k] == "v_fma_f32" and len(r) == 4 and "-" in i.split(",")[1]:
        return any(o.startswith("v_trunc_f32") and rr[0] == r[1] for o, rr in near(k - 4, k)) and \
            any(o.startswith("v_cmp_ge_f32") and rr[-2:] == [r[0], r[2]] for o, rr in near(k + 1, k + 4))
    return False


def libm_log(ops, k, span=72):
    """The f64 multiply-adds of the device library's log / log10 (ocml): its range reduction starts with v_frexp_mant_f64 +
    v_frexp_exp_i32_f64, then a reciprocal, a polynomial in s[] coefficients and the reconstruction, within `span`
    instructions"""
    if not ops[k].startswith(("v_fma_f64", "v_fmac_f64")):
        return False
    lo = max(0, k - span)
    starts = [x for x in range(lo, k) if ops[x].startswith("v_frexp_mant_f64")]
    return any(any(o.startswith("v_frexp_exp_i32_f64") for o in ops[x:x + 4]) for x in starts)

path = sys.argv[1] if len(sys.argv) > 1 else "openbts-ttsou_amd/csrc/trxsig_normal.gfx950.s"
only = sys.argv[2] if len(sys.argv) > 2 else ""
text = open(path).read()
for m in re.finditer(r"\n(_Z\w+):.*?\n(.*?)\n\.Lfunc_end", text, flags=re.S):
    name, body = m.group(1), m.group(2)
    if only and only not in name:
        continue
    ins = [l.strip() for l in body.split("\n") if l.startswith("\t") and not l.strip().startswith((".", ";"))]
    ops = [i.split()[0] for i in ins]
    c = Counter()
    for o in ops:
        if o.startswith("v_"): c["valu"] += 1
        elif o.startswith("s_waitcnt"): c["waitcnt"] += 1
        elif o.startswith("s_barrier"): c["barrier"] += 1
        elif o.startswith("s_"): c["salu"] += 1
        elif o.startswith("ds_"): c["lds"] += 1
        elif o.startswith(("global_", "buffer_", "flat_")): c["vmem"] += 1
    # deliberate single-rounding multiply-adds whose product is exact (a tap component of exactly +-1):
    # emitted through inline asm with a marker comment, bit-identical to the separate mul and add
    exact = sum(1 for i in ins if "exact-product" in i)
    # ... and the fused multiply-adds of a steering pass (fma_steer, trxsig_dev.h): approximate values that only select
    # which lags are recomputed exactly
    steer = sum(1 for i in ins if "; steering" in i)
    # ... and those of a form that is approximate by construction and graded with a tolerance (the shared-filter channeliser,
    # trxsig_chan.hip: the per-carrier sums in another order)
    approx = sum(1 for i in ins if "; approx-form" in i)
    # ... and those of the tolerance-mode demodulator (fused_demod_tol, trxsig_demod.h: TRXSIG_SOFT_TOLERANCE -- soft bits within
    # 3.7e-5 of the reference's, hard bits exact; only in kernels instantiated with TOL = true)
    tol = sum(1 for i in ins if "; soft-tolerance" in i)
    fma = [i for i, o in enumerate(ops) if FMA.match(o)
           and "exact-product" not in ins[i] and "; steering" not in ins[i] and "; approx-form" not in ins[i]
           and "; soft-tolerance" not in ins[i]]
    # ... and those the compiler emits for integer division and for the library's double log10 (burst_phy, trxsig_l1rx.hip)
    idiv = [i for i in fma if int_division(ins, ops, i)]
    logm = [i for i in fma if i not in idiv and libm_log(ops, i)]
    fma = [i for i in fma if i not in idiv and i not in logm]
    # hipcc's correctly-rounded division / sqrt expansions keep their fma's next to
    # v_div_scale / v_rcp / v_div_fmas / v_div_fixup / v_sqrt / v_rsq (f32 and f64)
    bad = 0
    for i in fma:
        lo = max(0, i - 24); hi = min(len(ops), i + 24)
        if not any(re.match(r"v_(div_scale|div_fmas|div_fixup|rcp_|sqrt_|rsq_)", o) for o in ops[lo:hi]):
            bad += 1
    kind = re.search(r"\d+(k_\w+?)ILi(\d)", name)
    label = "%s<sps=%s>" % (kind.group(1), kind.group(2)) if kind else name[:50]
    print("%-28s total %5d  %s  fma %d (outside a division: %d)%s" % (
        label, len(ops), dict(c), len(fma), bad, ("  exact-product fma %d" % exact if exact else "") +
        ("  steering fma %d" % steer if steer else "") + ("  approx-form fma %d" % approx if approx else "") +
        ("  soft-tolerance fma %d [%s]" % (tol, name) if tol else "") +
        ("  int-division fma %d" % len(idiv) if idiv else "") + ("  libm-log fma %d" % len(logm) if logm else "")))
