"""Two-antenna receive diversity in the C-ABI: its three entry points exported by libtrxsig.so and libtrxsig_tune.so, declared in
the headers and typed in the binding's table, refused with TRXSIG_EINVAL for a NULL context before anything touches a device;
the contract's words in the header; the kernel file in the Makefile; the binding's methods.  No GPU needed (the refusals that
need a live context are in tests/test_gpu_mlse_div.py and tests/test_gpu_mlse_div_group.py)."""
import ctypes
import os
import re

import pytest

import _pkg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = {"trxsig_mlse_div_batch": "trxsig.h", "trxsig_mlse_div_normal_batch": "trxsig.h", "trxsig_trxgroup_combine_div": "trxsig_trxgroup.h"}


@pytest.mark.parametrize("name", ["libtrxsig.so", "libtrxsig_tune.so"])
def test_diversity_in_the_abi(name):
    lib = ctypes.CDLL(os.path.join(ROOT, "openbts-ttsou_amd", name))
    for s, header in SYMBOLS.items():
        assert hasattr(lib, s), s
        assert re.search(r"\bint\s+%s\(" % s, open(os.path.join(ROOT, "include", header)).read()), s
    vp, i32, f32 = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
    lib.trxsig_mlse_div_batch.argtypes = [vp, vp, vp, vp, vp, vp, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp, i32, i32]
    lib.trxsig_mlse_div_normal_batch.argtypes = [vp, vp, vp, vp, vp, vp, i32, i32, f32, f32, vp, vp, vp, vp, vp, vp, vp, vp, vp, i32, i32]
    lib.trxsig_trxgroup_combine_div.argtypes = [vp] * 8
    x = (ctypes.c_float * 16)()
    for nsoft, tsc in ((148, 0), (149, 0), (148, 8), (148, -1), (0, 0)):
        assert lib.trxsig_mlse_div_batch(None, x, x, x, x, x, 1, tsc, x, x, None, None, None, None, x, None, nsoft, 160) == -1      # TRXSIG_EINVAL
        assert lib.trxsig_mlse_div_normal_batch(None, x, x, x, x, x, 1, tsc, 3.0, -1.0, x, x, x, None, x, None, None, x, None, nsoft, 160) == -1
    assert lib.trxsig_mlse_div_batch(None, None, None, None, None, None, 0, 0, None, None, None, None, None, None, None, None, 0, 0) == -1
    assert lib.trxsig_trxgroup_combine_div(None, x, None, x, None, None, None, x) == -1
    # the new kernels have no profiler id: the table (ABI 2) stays where it was
    assert lib.trxsig_kernel_count() == 28
    assert lib.trxsig_abi_version() == 2


def test_header_states_the_contract():
    h = open(os.path.join(ROOT, "include", "trxsig.h")).read()
    for word in ("p[d] = (c_0.re*c_0.re + c_0.im*c_0.im) + (c_1.re*c_1.re + c_1.im*c_1.im)",
                 "gamma = (dr_0*dr_0 + di_0*di_0) + (dr_1*dr_1 + di_1*di_1)", "d_primary", "same noise power",
                 "sel = 1 if v_1 && (!v_0 || n_1 > n_0)", "sel = 0 if v_0", "sel = 2", "ONE window w", "tests/mlse_div_model.py",
                 "tests/mlse_div_ref.py", "B x 2 x 5"):
        assert word in h, word
    g = open(os.path.join(ROOT, "include", "trxsig_trxgroup.h")).read()
    for word in ("1 if v_1 && (!v_0 || n_1 > n_0)", "TRXSIG_TSCLEG_DEMOD is the cheaper choice", "TRXSIG_TSCLEG_EQUALIZE", "fused source",
                 "valid until g0's next pull or combine"):
        assert word in g, word


def test_python_binding():
    m = _pkg.load()
    from openbts_ttsou_amd import _abi
    for name in SYMBOLS:
        assert name in _abi.SIGNATURES, name
    assert len(_abi.SIGNATURES["trxsig_mlse_div_batch"][1]) == 18 and len(_abi.SIGNATURES["trxsig_mlse_div_normal_batch"][1]) == 21
    assert len(_abi.SIGNATURES["trxsig_trxgroup_combine_div"][1]) == 8
    assert callable(getattr(m.TrxSig, "mlse_div", None)) and callable(getattr(m.TrxSig, "mlse_div_normal", None))
    assert callable(getattr(m.TrxGroup, "combine_div", None))


def test_kernel_file_is_built_and_audited():
    mk = open(os.path.join(ROOT, "openbts-ttsou_amd", "csrc", "Makefile")).read()
    assert re.search(r"^KERNELS\s*:=.*\btrxsig_mlse_div\b", mk, re.M)
    assert os.path.exists(os.path.join(ROOT, "openbts-ttsou_amd", "csrc", "trxsig_mlse_div.hip"))


def test_documents_name_the_stage():
    for doc in ("DESIGN.md", "README.md"):
        text = open(os.path.join(ROOT, doc)).read()
        assert "trxsig_mlse_div_batch" in text and "trxsig_trxgroup_combine_div" in text, doc
