"""Interference-rejection combining in the C-ABI: its three entry points exported by libtrxsig.so and libtrxsig_tune.so, declared in
the headers and typed in the binding's table, refused with TRXSIG_EINVAL for a NULL context before anything touches a device;
the contract's words in the header; the kernel file in the Makefile; the binding's methods.  No GPU needed (the refusals that
need a live context -- nsoft, tsc, the loading -- are checked on one in tests/test_gpu_mlse_irc.py and
tests/test_gpu_mlse_irc_group.py)."""
import ctypes

import pytest

import mlse_abi as abi

SYMBOLS = {"trxsig_mlse_irc_batch": "trxsig.h", "trxsig_mlse_irc_normal_batch": "trxsig.h", "trxsig_trxgroup_combine_irc": "trxsig_trxgroup.h"}


@pytest.mark.parametrize("name", abi.LIBS)
def test_irc_in_the_abi(name):
    lib = abi.exported_and_declared(name, SYMBOLS)
    vp, i32, f32 = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
    lib.trxsig_mlse_irc_batch.argtypes = [vp, vp, vp, vp, vp, vp, i32, i32, vp, vp, vp, vp, f32, vp, vp, vp, vp, vp, vp, i32, i32]
    lib.trxsig_mlse_irc_normal_batch.argtypes = [vp, vp, vp, vp, vp, vp, i32, i32, f32, f32, f32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, i32, i32]
    lib.trxsig_trxgroup_combine_irc.argtypes = [vp, vp, vp, vp, f32, vp, vp, vp, vp, vp]
    x = (ctypes.c_float * 16)()
    for nsoft, tsc, loading in ((148, 0, 0.0), (149, 0, 0.0), (148, 8, 0.0), (148, -1, 0.0), (0, 0, 0.0), (148, 0, -1.0), (148, 0, 17.0),
                                (148, 0, float("nan"))):
        assert lib.trxsig_mlse_irc_batch(None, x, x, x, x, x, 1, tsc, x, x, None, None, loading, None, None, None, None, x, None, nsoft, 160) == -1
        assert lib.trxsig_mlse_irc_normal_batch(None, x, x, x, x, x, 1, tsc, 3.0, -1.0, loading, x, x, x, None, x, None, None, None, x, None,
                                                nsoft, 160) == -1
    assert lib.trxsig_mlse_irc_batch(None, None, None, None, None, None, 0, 0, None, None, None, None, 0.0, None, None, None, None, None, None,
                                     0, 0) == -1
    assert lib.trxsig_trxgroup_combine_irc(None, x, None, x, 1.0 / 64.0, None, None, None, None, x) == -1
    abi.table_stays(lib)


def test_headers_state_the_contract():
    h = abi.read("include", "trxsig.h")
    for word in ("S00 += r0.re*r0.re + r0.im*r0.im", "Xi += r0.im*r1.re - r0.re*r1.im", "tt = S00 + S11", "A = S00/tt + loading",
                 "det = A*Bv - (xr*xr + xi*xi)", "v < 0x1p10f", "!(det > 0)", "y1'[n].re = A*y1[n].re - (xr*y0[n].re + xi*y0[n].im)",
                 "y1'[n].im = A*y1[n].im - (xr*y0[n].im - xi*y0[n].re)", "gamma = det*(dr0*dr0 + di0*di0) + (dr1*dr1 + di1*di1)",
                 "(8.0f * E_w)", "0 <= loading <= 16", "d_cov_in", "not symmetric", "tests/mlse_irc_model.py", "tests/mlse_irc_ref.py",
                 "TRXSIG_K_COUNT = 15", "#define TRXSIG_ABI_VERSION 2"):
        assert word in h, word
    g = abi.read("include", "trxsig_trxgroup.h")
    for word in ("trxsig_trxgroup_combine_irc", "k_mlse_irc", "0 <= loading <= 16", "1/64"):
        assert word in g, word


def test_python_binding():
    m, _abi = abi.binding(SYMBOLS, TrxSig=("mlse_irc", "mlse_irc_normal"), TrxGroup=("combine_irc",))
    assert len(_abi.SIGNATURES["trxsig_mlse_irc_batch"][1]) == 21 and len(_abi.SIGNATURES["trxsig_mlse_irc_normal_batch"][1]) == 23
    assert len(_abi.SIGNATURES["trxsig_trxgroup_combine_irc"][1]) == 10
    assert _abi.SIGNATURES["trxsig_mlse_irc_batch"][1][12] is ctypes.c_float and _abi.SIGNATURES["trxsig_trxgroup_combine_irc"][1][4] is ctypes.c_float
    assert m.IRC_LOADING == 1.0 / 64.0


def test_kernel_file_is_built():
    src = abi.kernel_file("trxsig_mlse_irc")
    assert "k_mlse_irc" in src and "amdgpu_waves_per_eu(4)" in src
    for call in ("mlse_symbols<SPS>(", "mlse_window2(", "mlse_trellis2<61, true>(", "#pragma unroll 1"):
        assert call in src, call
    dev = abi.read("openbts-ttsou_amd", "csrc", "trxsig_mlse_dev.h")
    assert "if (WEIGHTED) return det * mlse_gamma(y0, z0) + mlse_gamma(y1, z1);" in dev       # det on antenna 0's metric, and only here


def test_documents_name_the_stage():
    abi.documents_name("trxsig_mlse_irc_batch", "trxsig_trxgroup_combine_irc", "mlse_irc_bench")
    assert "unequal noise power per branch" not in abi.read("README.md")
