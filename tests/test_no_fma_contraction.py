"""Numerical-contract audit on the generated gfx950 ISA (no GPU needed: hipcc cross-compiles): outside
hipcc's correctly-rounded division / sqrt expansions no kernel may contain a fused multiply-add, except the two
marked kinds (and, in the shared-filter channeliser alone -- an approximate form by construction, off by default, graded with a
tolerance -- the "approx-form" kind; and, in the kernels instantiated for trxsig_set_soft_mode(TRXSIG_SOFT_TOLERANCE) alone, the "soft-tolerance" kind) that tools/asm_stats.py counts apart: the exact-product FMAs of the midamble correlators (a tap
component of exactly +-1: single rounding == separate mul and add) and the FMAs of a steering pass (fma_steer:
approximate correlations that only decide which lags are recomputed with the reference's exact arithmetic), which
may appear in the kernels listed below and nowhere else.  Two more kinds are compiler output for code that is not float
arithmetic of the kernel's values: the reciprocal estimate of an integer division ("int-division": the 64-bit udiv / urem
expansion and the 24-bit div / rem form), allowed in the kernels that divide 64-bit integers, and the device library's double
log10 ("libm-log", burst_phy's RSSI), allowed in k_l1rx_demux alone.  Every kernel file the Makefile builds is audited: the list
comes from csrc/*.hip and must equal the Makefile's KERNELS + TUNEK."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "openbts-ttsou_amd", "csrc")
INT_DIVISION_OK = ("k_l1rx_demux", "k_channelise16", "k_resample", "k_group_expand", "k_group_scatter")   # 64-bit / and %


def kernel_files():
    """The kernel files: csrc/*.hip, checked against the Makefile's KERNELS and TUNEK (a .hip file the Makefile does not build
    or a listed one that does not exist fails here)."""
    hip = sorted(f[:-4] for f in os.listdir(CSRC) if f.endswith(".hip"))
    mk = open(os.path.join(CSRC, "Makefile")).read()
    listed = []
    for var in ("KERNELS", "TUNEK"):
        listed += re.search(r"^%s\s*:=(.*)$" % var, mk, flags=re.M).group(1).split()
    assert sorted(listed) == hip, (listed, hip)
    return hip


def test_kernel_file_list():
    files = kernel_files()
    assert {"trxsig_l1rx", "trxsig_grouptx", "trxsig_chain", "trxsig_fec", "trxsig_normal"} <= set(files)


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="no hipcc")
def test_kernels_have_no_contracted_fma():
    subprocess.check_call(["make", "-s", "-j8", "-C", os.path.join(ROOT, "openbts-ttsou_amd", "csrc"), "asm"],
                          stderr=subprocess.DEVNULL)
    out = ""
    files = kernel_files()
    for f in files:
        o = subprocess.check_output(["python3", os.path.join(ROOT, "tools", "asm_stats.py"), os.path.join(CSRC, f + ".gfx950.s")],
                                    text=True)
        assert "outside a division" in o, f                  # every file's listing holds kernels the audit reads
        out += o
    rows = [l for l in out.splitlines() if "outside a division" in l]
    assert len(rows) >= 23 and any("k_fec_viterbi" in l for l in rows)
    for k in ("k_l1rx_demux", "k_l1rx_finish", "k_group_tx", "k_normal_chain", "k_fec_rx_stream", "k_fec_rx_fold"):
        assert any(k in l for l in rows), k
    steering_ok = ("k_rach_fast", "k_rach_front")
    for l in rows:
        n = int(re.search(r"outside a division: (\d+)", l).group(1))
        assert n == 0, l
        if "steering fma" in l:
            assert any(k in l for k in steering_ok), l
        if "approx-form fma" in l:                           # only the shared-filter channeliser (graded at 1e-4, never the default)
            assert "k_channelise16" in l, l
        if "soft-tolerance fma" in l:                        # only kernels instantiated for TRXSIG_SOFT_TOLERANCE (TOL = true: the last
            sym = re.search(r"\[(\w+)\]", l).group(1)       # template argument of k_demod / k_normal_quad / k_normal_chain)
            assert re.search(r"(7k_demodILi\dELb0ELi148ENS_6SmpC32ELb1EEE|k_normal_quadILi\d.*ELb1EEE|k_normal_chainILi\d.*ELb1EEE|k_demod_rxILi4ELb1EEE)", sym), l
        if "int-division fma" in l:                          # the compiler's integer division: only where 64-bit / and % are
            assert any(k in l for k in INT_DIVISION_OK), l
        if "libm-log fma" in l:                              # the library's double log10: burst_phy's RSSI, k_l1rx_demux alone
            assert "k_l1rx_demux" in l, l
    assert any("steering fma" in l and "k_rach_front" in l for l in rows)
    assert any("int-division fma" in l and "libm-log fma" in l and "k_l1rx_demux" in l for l in rows)
    assert any("approx-form fma" in l and "k_channelise16" in l for l in rows)
    assert any("soft-tolerance fma" in l and "k_demod" in l for l in rows)


def _audit(tmp_path, body):
    p = tmp_path / "k.s"
    p.write_text("\n_Z5k_fooPf:                             ; @k_foo\n" + "".join("\t%s\n" % l for l in body) + ".Lfunc_end0:\n")
    out = subprocess.check_output(["python3", os.path.join(ROOT, "tools", "asm_stats.py"), str(p)], text=True)
    m = re.search(r"fma (\d+) \(outside a division: (\d+)\)", out)
    kinds = {}
    for k in ("int-division", "libm-log"):
        n = re.search(r"%s fma (\d+)" % k, out)
        kinds[k] = int(n.group(1)) if n else 0
    return int(m.group(2)), kinds


def test_audit_rules_on_written_listings(tmp_path):
    """The classifier on small hand-written listings: the compiler's integer division and log10 sequences are their own kinds,
    and a multiply-add that merely resembles them -- or uses a form the old pattern missed (v_fmamk / v_fmaak) -- is a
    contracted one."""
    udiv64 = ["v_cvt_f32_u32_e32 v4, v52", "v_cvt_f32_u32_e32 v40, v39", "v_fmac_f32_e32 v4, 0x4f800000, v40", "v_rcp_f32_e32 v4, v4",
              "v_mul_f32_e32 v4, 0x5f7ffffc, v4", "v_mul_f32_e32 v40, 0x2f800000, v4", "v_trunc_f32_e32 v40, v40",
              "v_fmac_f32_e32 v4, 0xcf800000, v40", "v_cvt_u32_f32_e32 v50, v4"]
    div24 = ["v_cvt_f32_i32_e32 v14, v9", "v_mul_f32_e32 v20, v14, v27", "v_trunc_f32_e32 v20, v20", "v_cvt_i32_f32_e32 v30, v20",
             "v_fma_f32 v14, -v20, v21, v14", "v_cmp_ge_f32_e64 vcc, |v14|, |v21|"]
    log = ["v_frexp_mant_f64_e32 v[36:37], v[34:35]", "v_frexp_exp_i32_f64_e32 v54, v[34:35]"] + ["v_add_f64 v[0:1], v[0:1], v[2:3]"] * 30 + \
          ["v_fmac_f64_e32 v[38:39], s[42:43], v[62:63]", "v_fma_f64 v[40:41], v[38:39], s[48:49], -v[46:47]"]
    filler = ["v_add_f32_e32 v1, v2, v3"] * 30
    assert _audit(tmp_path, udiv64) == (0, {"int-division": 2, "libm-log": 0})
    assert _audit(tmp_path, div24) == (0, {"int-division": 1, "libm-log": 0})
    assert _audit(tmp_path, log) == (0, {"int-division": 0, "libm-log": 2})
    assert _audit(tmp_path, filler + ["v_fmac_f32_e32 v1, v2, v3"] + filler)[0] == 1
    assert _audit(tmp_path, filler + ["v_fmamk_f32 v1, v2, 0x3f800000, v1", "v_fmaak_f32 v1, v2, v3, 0x3f800000"] + filler)[0] == 2
    # +-2^32 without the reciprocal / the conversion around it, the 24-bit form without its compare, log's polynomial far from
    # the range reduction, an f32 multiply-add inside the log window: all contracted
    assert _audit(tmp_path, filler + ["v_fmac_f32_e32 v4, 0x4f800000, v40"] + filler)[0] == 1
    assert _audit(tmp_path, filler + ["v_trunc_f32_e32 v40, v40", "v_fmac_f32_e32 v4, 0xcf800000, v40"] + filler)[0] == 1
    assert _audit(tmp_path, filler + div24[:5] + filler)[0] == 1
    assert _audit(tmp_path, log[:2] + filler * 3 + ["v_fmac_f64_e32 v[38:39], s[42:43], v[62:63]"] + filler)[0] == 1
    assert _audit(tmp_path, log[:2] + ["v_fmac_f32_e32 v1, v2, v3"] + filler)[0] == 1
