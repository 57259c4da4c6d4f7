"""CPU-side checks of the product boundary: the C-ABI library loads, exports every symbol that
include/mi355x_qr.h declares, and refuses to compute without a GPU (no CPU fallback)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest


def test_library_exports_every_declared_symbol(qr):
    names = qr.exported_symbols()
    assert {"mmqr", "explicitQR", "getPanelDims", "dgemm", "identity", "printMat", "qr_thin",
            "qr_geqrf_dev", "qr_applyq_dev", "qr_plan_create"} <= set(names)
    for n in names:
        assert hasattr(qr.lib, n), f"{n} declared in include/mi355x_qr.h but not exported"
    out = subprocess.run(["nm", "-D", qr.LIB_PATH], capture_output=True, text=True).stdout
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    assert set(names) <= exported


def test_drop_in_symbol_set_matches_reference_prototypes(qr):
    """qr.c:15-18 + qr.c:47,55 -- the six external functions of the reference TU."""
    for n in ("printMat", "dgemm", "explicitQR", "identity", "getPanelDims", "mmqr"):
        assert hasattr(qr.lib, n)


def test_host_only_helpers(qr, capfd):
    I = qr.identity(5)                       # qr.c:316-324
    assert np.array_equal(I, np.eye(5))
    nb, ib = qr.get_block_size()
    assert qr.get_panel_dims(512, 128) == (1, -(-128 // nb))
    assert qr.get_panel_dims(16384, 2048) == (1, -(-2048 // nb))             # tall: the default block
    assert qr.get_panel_dims(4096, 4096) == (1, 4096 // 256)                 # wherever the look-ahead schedule pays: 256 (what mmqr really uses)
    assert qr.get_panel_dims(8192, 4096) == (1, 4096 // 256)
    assert qr.get_panel_dims(32768, 8192) == (1, 8192 // 256)                # and from 8192 columns on
    assert qr.get_panel_dims(2048, 2048) == (1, 2048 // 64)                  # small square-ish problems (single stream, all panel): 64
    A = np.asfortranarray(np.arange(6, dtype=np.float64).reshape(2, 3))
    qr.lib.printMat(A.ctypes.data_as(C.POINTER(C.c_double)), 2, 3)   # qr.c:21-33 format
    C.CDLL(None).fflush(None)
    out = capfd.readouterr().out
    assert out.startswith("Matrix 2 x 3, row by row:\n") and " 0.000000  1.000000  2.000000 \n" in out


def test_block_size_validation(qr):
    nb, ib = qr.get_block_size()
    with pytest.raises(qr.QRError):
        qr.set_block_size(100, 32)           # not a multiple of ib
    with pytest.raises(qr.QRError):
        qr.set_block_size(64, 64)            # leaf wider than 32
    qr.set_block_size(nb, ib)


def test_generator_host_matches_scalar_entry(qr):
    M = qr.uniform_matrix_host(7, 5, row_off=3, total_rows=20, seed=12)
    for c in range(5):
        for i in range(7):
            assert M[i, c] == qr.uniform_at(12, c * 20 + i + 3)
    big = qr.uniform_matrix_host(4096, 8, seed=12)
    assert 0.0 <= big.min() and big.max() < 1.0 and abs(big.mean() - 0.5) < 0.01


def test_argument_errors_do_not_need_a_gpu(qr):
    A = np.zeros((4, 6), order="F")
    with pytest.raises(qr.QRError, match="invalid argument"):
        qr.mmqr(A)                            # m < n (the reference asserts, qr.c:465)


def test_no_cpu_fallback_without_device(qr):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(qr.QRError, match="no HIP device"):
        qr.mmqr(np.random.rand(6, 4))
    with pytest.raises(qr.QRError, match="no HIP device"):
        qr.Plan(64, 32)


def test_qr_thin_mgpu_argument_checks(qr):
    """The C-level multi-GPU TSQR entry: argument errors come before anything touches a device; asking for more
    GPUs than are visible is QR_E_ARG on a GPU box and QR_E_NODEVICE where there is none."""
    import torch
    A = np.random.rand(64, 8)
    with pytest.raises(qr.QRError, match="invalid argument"):
        qr.qr_thin_mgpu(A, ngpu=0)
    with pytest.raises(qr.QRError, match="invalid argument"):
        qr.qr_thin_mgpu(np.zeros((4, 6)), ngpu=1)
    ndev = torch.cuda.device_count()
    if ndev == 0:
        with pytest.raises(qr.QRError, match="no HIP device"):
            qr.qr_thin_mgpu(A, ngpu=1)
    else:
        with pytest.raises(qr.QRError, match="invalid argument"):
            qr.qr_thin_mgpu(A, ngpu=ndev + 1)


def test_tsqr_plan_argument_checks(qr):
    """Device-resident TSQR step (qr_tsqr_plan_*, include/mi355x_qr.h): argument errors come before anything touches a device
    or loads RCCL; a valid single-rank request without a GPU is QR_E_NODEVICE (no CPU fallback)."""
    import torch
    h = C.c_void_p()
    E_ARG = -101
    assert qr.lib.qr_tsqr_plan_create(C.byref(h), None, 0, 0, 64, 8, 0) == E_ARG          # no ranks
    assert qr.lib.qr_tsqr_plan_create(C.byref(h), None, 2, 2, 64, 8, 0) == E_ARG          # rank out of range
    assert qr.lib.qr_tsqr_plan_create(C.byref(h), None, 2, 0, 64, 8, 0) == E_ARG          # 2 ranks need a unique id
    assert qr.lib.qr_tsqr_plan_create(C.byref(h), None, 1, 0, 4, 8, 0) == E_ARG           # shard with fewer rows than columns
    assert qr.lib.qr_tsqr_plan_create(None, None, 1, 0, 64, 8, 0) == E_ARG
    assert qr.lib.qr_tsqr_plan_create_comm(C.byref(h), None, 3, 3, 64, 8, 0) == E_ARG
    assert qr.lib.qr_tsqr_factor_dev(None, None, 0, None) == E_ARG
    assert qr.lib.qr_tsqr_formq_dev(None, None, 0, None, 0) == E_ARG
    assert qr.lib.qr_tsqr_stacked_dev(None, None) == E_ARG
    assert qr.lib.qr_tsqr_sync(None) == E_ARG
    assert qr.lib.qr_tsqr_unique_id(None) == E_ARG
    assert qr.lib.qr_tsqr_plan_destroy(None) == 0
    if not torch.cuda.is_available():
        assert qr.lib.qr_tsqr_plan_create(C.byref(h), None, 1, 0, 64, 8, 0) == -103       # QR_E_NODEVICE
        with pytest.raises(qr.QRError, match="no HIP device"):
            qr.TsqrPlan(64, 8)


def test_default_block_size_sizes_tau(qr):
    """mmqr's tau has rowPanels*colPanels*nb entries of the block size THAT SHAPE gets (256 where the look-ahead schedule pays, 64 for
    small square-ish problems), not of the global default: the Python wrapper and C callers size it through qr_default_block_size."""
    # in a fresh process: an earlier qr_set_block_size (test_block_size_validation) pins nb for the rest of this one
    code = ("import sys; sys.path.insert(0, %r); import cuda_qr_amd as qr\n"
            "g = qr.get_block_size()[0]\n"
            "assert qr.default_block_size(512, 128)[0] == g\n"
            "assert qr.default_block_size(1024, 1024)[0] == 64 and qr.tau_len(1024, 1024) == 1024\n"
            "assert qr.default_block_size(4096, 4096)[0] == 256 and qr.default_block_size(3072, 3072)[0] == 256\n"
            "assert qr.default_block_size(2560, 2560)[0] == 64 and qr.default_block_size(16384, 2048)[0] == g\n"
            "assert qr.default_block_size(8192, 1024)[0] == 256 and qr.default_block_size(16384, 1024)[0] == g\n"
            "assert qr.tau_len(2048, 2048) == 2048 and qr.tau_len(1300, 1100) == 1152\n"
            "assert qr.lib.qr_default_block_size(4, 8, None, None) == -101\n"
            "qr.set_block_size(64, 32)\n"
            "assert qr.default_block_size(4096, 4096)[0] == 64 and qr.tau_len(1000, 100) == 128\n") % os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if not k.startswith("MI355XQR_")}
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env)
    assert out.returncode == 0, out.stderr[-2000:]


def test_legacy_shim_panel_dims_and_argument_checks(qr):
    """getPanelDims_legacy = the reference's formula (qr.c:47-53) for a given window; shapes the reference's loops cannot factor
    are refused before anything touches a device."""
    rp, cp = C.c_int(), C.c_int()
    qr.lib.getPanelDims_legacy(512, 128, 64, 8, C.byref(rp), C.byref(cp))
    assert (rp.value, cp.value) == (9, 16)                       # C1 at PR 64 / PC 8
    qr.lib.getPanelDims_legacy(512, 128, 4, 2, C.byref(rp), C.byref(cp))
    assert (rp.value, cp.value) == (255, 64)                     # C1 as committed (PR 4 / PC 2)
    qr.lib.getPanelDims_legacy(6, 4, 4, 2, C.byref(rp), C.byref(cp))
    assert (rp.value, cp.value) == (2, 2)
    A = np.zeros((100, 32), order="F")
    t = C.POINTER(C.c_double)()
    for PR, PC in ((64, 8), (128, 8), (64, 3), (8, 8)):
        assert qr.lib.mmqr_legacy_status(A.ctypes.data_as(C.POINTER(C.c_double)), C.byref(t), 100, 32, PR, PC) == -101


def test_strerror_names_rccl_failures(qr):
    assert "rccl" in qr.strerror(-120).lower()
    assert "argument" not in qr.strerror(-133).lower()          # an RCCL failure (-130 - ncclResult_t) is not an argument error
    assert "argument" in qr.strerror(-7).lower()


@pytest.mark.parametrize("target", ["asan", "tsan"])
def test_host_layer_under_sanitizers(target):
    """SURVEY section 5 (race detection / sanitizers): the C host layer (schedule, plan cache, per-device threads of
    qr_thin_mgpu, TSQR plan) built with AddressSanitizer + UBSan / ThreadSanitizer against the test-only stub device layer
    (tests/c/qrd_stub.c bounds-checks every operand block a launch receives) and run through tests/c/host_sanitize.c.  The same
    targets build and run cuda-qr_amd/tools/stage_sanitize.c over the staging unit of the batched host-pointer twins (csrc/qr_stage.c): the carve
    of its one allocation, every copy and clear inside it, the error path, an overflowing table, no leak."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if not k.startswith("MI355XQR_")}
    out = subprocess.run(["make", "-C", os.path.join(root, "cuda-qr_amd"), target], capture_output=True, text=True, env=env, timeout=600)
    assert out.returncode == 0, (out.stdout[-1500:] + out.stderr[-3000:])
    assert "host layer sanitize run ok" in out.stdout


def test_product_never_touches_the_oracle():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for dp, _, files in os.walk(os.path.join(root, "cuda-qr_amd")):
        for f in files:
            if f.endswith((".py", ".c", ".h", ".hip")):
                txt = open(os.path.join(dp, f)).read()
                assert "oracle" not in txt.lower().replace("no cpu fallback", ""), f"{f} mentions the oracle"


PUBLIC_KNOBS = {"MI355XQR_" + k for k in ("NB", "IB", "PANEL", "GUARD", "LOOKAHEAD", "SPLIT", "CQR_MIN_ROWS", "FUSED_MIN_ROWS", "TSQR_PIPE",
                                          "TSQR_RESERVE_CUS", "PLAN_CACHE", "ROCTX")}


def _knob_strings(path):
    import re
    return set(re.findall(rb"MI355XQR_[A-Z0-9_]+", open(path, "rb").read()))


def test_product_library_reads_only_the_public_knobs(qr):
    """VERDICT r5 item 7 / ADVICE r5: the shipped library must not change what a factorisation does because of a stray measurement
    variable (MI355XQR_NT_CEIL made it return wrong results).  The product build holds the names of the twelve documented knobs and no
    others; the measurement knobs, the results-wrong ceiling variants and the development entry points exist in the lab build only."""
    prod = {s.decode() for s in _knob_strings(os.path.join(os.path.dirname(qr.LIB_PATH), "libmi355xqr.so"))}
    assert prod == PUBLIC_KNOBS, sorted(prod ^ PUBLIC_KNOBS)
    syms = subprocess.run(["nm", "-D", os.path.join(os.path.dirname(qr.LIB_PATH), "libmi355xqr.so")], capture_output=True, text=True).stdout
    assert "qrd_dbg_" not in syms and "gemm_nt4_kernelILb1ELi1E" not in syms and "gemm_nt4_kernelILb1ELi2E" not in syms
    if os.path.exists(qr.LAB_LIB_PATH):
        lab = {s.decode() for s in _knob_strings(qr.LAB_LIB_PATH)}
        assert PUBLIC_KNOBS < lab and "MI355XQR_NT_CEIL" in lab
        assert "qrd_dbg_lu32" in subprocess.run(["nm", "-D", qr.LAB_LIB_PATH], capture_output=True, text=True).stdout


def test_integration_md_documents_exactly_the_public_knobs():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    import re
    txt = open(os.path.join(root, "INTEGRATION.md")).read()
    sec = txt[txt.index("## 6."):]
    sec = sec[:sec.index("\n## ", 5)] if "\n## " in sec[5:] else sec
    table = {m for m in re.findall(r"^\| `(MI355XQR_[A-Z0-9_]+)`", sec, flags=re.M)}
    assert table == PUBLIC_KNOBS, sorted(table ^ PUBLIC_KNOBS)


def test_entry_scripts_compile():
    """bench.py, __graft_entry__.py and the measurement helpers are what the driver and the evidence scripts execute: a syntax error there is
    only seen on the GPU box otherwise."""
    import glob
    import py_compile
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for f in [os.path.join(root, "bench.py"), os.path.join(root, "__graft_entry__.py")] + sorted(glob.glob(os.path.join(root, "devtools", "*.py"))):
        py_compile.compile(f, doraise=True)
