"""CPU-side checks of the singular-value interface (mi355x_qr.h section 7): declared, exported, bound, the Jacobi tournament the device
code runs, and argument errors without a device."""
import ctypes as C
import itertools
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SVD_API = ("qr_jsvd_rounds", "qr_jsvd_round_pairs", "qr_gesvj_dev", "qr_gesvd_dev", "qr_cond_dev", "qr_gelss_dev", "qr_svd", "qr_lstsq_svd")


def test_header_declares_and_library_exports_the_svd_section(qr):
    declared = set(qr.exported_symbols())
    assert set(SVD_API) <= declared
    out = subprocess.run(["nm", "-D", qr.LIB_PATH], capture_output=True, text=True).stdout
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    assert set(SVD_API) <= exported
    for name in SVD_API:
        f = getattr(qr.lib, name)
        assert f.argtypes, name
    txt = open(qr.HEADER).read()
    assert "7. Singular values" in txt
    assert "#define QR_E_NOCONV   (-108)" in txt and "#define QR_JSVD_BLOCK 32" in txt and "#define QR_JSVD_MAX_SWEEPS 30" in txt
    assert qr.QR_E_NOCONV == -108 and qr.JSVD_BLOCK == 32 and qr.JSVD_MAX_SWEEPS == 30
    s = qr.strerror(qr.QR_E_NOCONV)
    assert "Jacobi" in s and s != qr.strerror(-104) and s != qr.strerror(-199)
    for meth in ("gesvj", "gesvd", "cond", "gelss"):
        assert callable(getattr(qr.Plan, meth))
    for fn in ("svd", "svdvals", "cond", "lstsq_svd", "jsvd_rounds", "jsvd_round_pairs"):
        assert callable(getattr(qr, fn))


def test_host_code_stays_out_of_the_stubbed_translation_unit():
    """qr_host.c is compiled against the stub device layer by the sanitizer builds: the new launch wrappers must not be called from it"""
    src = open(os.path.join(ROOT, "cuda-qr_amd", "csrc", "qr_host.c")).read()
    assert "qrd_jsvd" not in src
    mk = open(os.path.join(ROOT, "cuda-qr_amd", "Makefile")).read()
    assert "build/qr_svd_c.o" in mk and "build/lab/qr_svd_c.o" in mk
    assert "csrc/qr_svd.c" in mk and "qr_svd" in mk.split("HIPSRC =")[1].splitlines()[0]
    dev = open(os.path.join(ROOT, "cuda-qr_amd", "csrc", "qr_device.h")).read()
    assert "called from qr_svd.c only" in dev and "qrd_jsvd_round" in dev


@pytest.mark.parametrize("n", [1, 20, 32, 33, 64, 65, 96, 200, 330, 1024])
def test_tournament_covers_every_block_pair_once(qr, n):
    nblk, rounds = qr.jsvd_rounds(n)
    assert nblk == -(-n // 32)
    if nblk == 1:
        assert rounds == 1 and qr.jsvd_round_pairs(n, 0) == [(0, 0)]
        return
    assert rounds == (nblk if nblk % 2 else nblk - 1)
    seen = []
    for r in range(rounds):
        pairs = qr.jsvd_round_pairs(n, r)
        assert len(pairs) == nblk // 2
        blocks = [b for pq in pairs for b in pq]
        assert len(set(blocks)) == len(blocks), "a block appears twice in a round"
        assert all(0 <= p < q < nblk for p, q in pairs)
        seen += pairs
    assert sorted(seen) == list(itertools.combinations(range(nblk), 2)), "a sweep is every unordered pair exactly once"


def test_tournament_rejects_bad_arguments(qr):
    L, E = qr.lib, qr.QR_E_ARG
    buf = (C.c_int * 64)()
    nb, rd = C.c_int(), C.c_int()
    assert L.qr_jsvd_rounds(0, C.byref(nb), C.byref(rd)) == E
    assert L.qr_jsvd_rounds(100, None, None) == 0
    assert L.qr_jsvd_round_pairs(0, 0, buf, 32) == E
    assert L.qr_jsvd_round_pairs(200, -1, buf, 32) == E and L.qr_jsvd_round_pairs(200, 7, buf, 32) == E      # 7 blocks: rounds 0 .. 6
    assert L.qr_jsvd_round_pairs(200, 0, None, 32) == E and L.qr_jsvd_round_pairs(200, 0, buf, 2) == E       # 3 pairs per round
    assert L.qr_jsvd_round_pairs(200, 6, buf, 3) == 3


class _FakePlan(C.Structure):
    """the leading fields of struct qr_plan (csrc/qr_plan_internal.h): m, n, nb, ib, ldv, ldt.  Every call below must reject its
    arguments from these alone, before it reaches a device."""
    _fields_ = [("m", C.c_int), ("n", C.c_int), ("nb", C.c_int), ("ib", C.c_int), ("ldv", C.c_int), ("ldt", C.c_int),
                ("rest", C.c_char * 8192)]


def test_device_entry_points_reject_bad_arguments_without_a_device(qr):
    L = qr.lib
    fp = _FakePlan()
    fp.m, fp.n, fp.nb, fp.ib, fp.ldv, fp.ldt = 1000, 300, 128, 32, 1024, 128
    P = C.cast(C.pointer(fp), C.c_void_p)
    buf = (C.c_double * 16)()
    d = C.cast(buf, C.c_void_p)           # never dereferenced: every call below fails its argument check first
    E = qr.QR_E_ARG
    sw = C.c_int()

    def gesvj(plan=P, jobv=b"V", G=d, r=400, n=300, ldg=400, S=d, V=d, ldv=300):
        return L.qr_gesvj_dev(plan, jobv, G, r, n, ldg, S, V, ldv, C.byref(sw))

    assert gesvj(plan=None) == E and gesvj(G=None) == E and gesvj(S=None) == E
    assert gesvj(V=None) == E and gesvj(jobv=b"v", V=None) == E                  # a NULL dV goes with jobv 'N' only (accepted there: test_gpu_svd)
    assert gesvj(jobv=b"X") == E and gesvj(jobv=b"U") == E
    assert gesvj(n=0) == E and gesvj(r=299, ldg=299) == E                        # r < n
    assert gesvj(n=301, ldv=301) == E and gesvj(r=1001, ldg=1001) == E           # above the plan's
    assert gesvj(ldg=399) == E and gesvj(ldv=299) == E

    def gesvd(plan=P, jobu=b"U", jobv=b"V", A=d, m=1000, n=300, lda=1000, tau=d, S=d, U=d, ldu=1000, V=d, ldv=300):
        return L.qr_gesvd_dev(plan, jobu, jobv, A, m, n, lda, tau, S, U, ldu, V, ldv, C.byref(sw))

    assert gesvd(plan=None) == E and gesvd(A=None) == E and gesvd(tau=None) == E and gesvd(S=None) == E
    assert gesvd(U=None) == E and gesvd(V=None) == E
    assert gesvd(jobu=b"V") == E and gesvd(jobv=b"U") == E and gesvd(jobu=b"A") == E
    assert gesvd(n=0) == E and gesvd(m=299, lda=299, ldu=299) == E               # m < n
    assert gesvd(m=1001, lda=1001, ldu=1001) == E and gesvd(n=301, ldv=301) == E
    assert gesvd(lda=999) == E and gesvd(ldu=999) == E and gesvd(ldv=299) == E

    c = C.c_double()

    def cond(plan=P, A=d, m=1000, n=300, lda=1000, tau=d, out=C.byref(c)):
        return L.qr_cond_dev(plan, A, m, n, lda, tau, out)

    assert cond(plan=None) == E and cond(A=None) == E and cond(tau=None) == E and cond(out=None) == E
    assert cond(n=0) == E and cond(m=299, lda=299) == E and cond(m=1001, lda=1001) == E and cond(n=301) == E and cond(lda=999) == E

    rk = C.c_int()

    def gelss(plan=P, A=d, m=1000, n=300, lda=1000, tau=d, B=d, nrhs=2, ldb=1000, rcond=-1.0, S=d):
        return L.qr_gelss_dev(plan, A, m, n, lda, tau, B, nrhs, ldb, rcond, S, C.byref(rk))

    assert gelss(plan=None) == E and gelss(A=None) == E and gelss(tau=None) == E and gelss(B=None) == E and gelss(S=None) == E
    assert gelss(n=0) == E and gelss(m=299, lda=299, ldb=299) == E and gelss(m=1001, lda=1001, ldb=1001) == E and gelss(n=301) == E
    assert gelss(lda=999) == E and gelss(ldb=999) == E and gelss(nrhs=0) == E


def test_host_twins_reject_bad_arguments_without_a_device(qr):
    dp = C.POINTER(C.c_double)
    a = (C.c_double * 64)()
    p = C.cast(a, dp)
    L, E = qr.lib, qr.QR_E_ARG
    assert L.qr_svd(None, 8, 4, p, None, None) == E and L.qr_svd(p, 8, 4, None, None, None) == E
    assert L.qr_svd(p, 3, 4, p, None, None) == E and L.qr_svd(p, 8, 0, p, None, None) == E

    def ls(A=p, m=8, n=4, B=p, nrhs=1, X=p):
        return L.qr_lstsq_svd(A, m, n, B, nrhs, -1.0, X, None, None, None)

    assert ls(A=None) == E and ls(B=None) == E and ls(X=None) == E
    assert ls(m=3) == E and ls(n=0) == E and ls(nrhs=0) == E
    with pytest.raises(qr.QRError) as ei:
        qr.svd(np.zeros((3, 5)))
    assert ei.value.status == E
    with pytest.raises(qr.QRError) as ei:
        qr.lstsq_svd(np.zeros((5, 3)), np.zeros(4))               # B's height is not A's
    assert ei.value.status == E
