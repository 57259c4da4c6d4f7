"""CPU-side checks of the batched row append / removal (mi355x_qr.h section 8d): declared, exported, bound, the row-limit table, and every
argument error without a device."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UPDATE_API = ("qr_tpqrt_batched_max_rows", "qr_tphqrt_batched_dev", "qr_tpqrt_batched_dev", "qr_tpmqrt_batched_dev",
              "qr_lsacc_batched_create", "qr_lsacc_batched_push_dev", "qr_lsacc_batched_pop_dev", "qr_lsacc_batched_slide_dev",
              "qr_lsacc_batched_factor_dev", "qr_lsacc_batched_solve_dev", "qr_lsacc_batched_reset", "qr_lsacc_batched_destroy",
              "qr_lstsq_rolling_batched")


def test_header_declares_and_library_exports_the_calls(qr):
    declared = set(qr.exported_symbols())
    assert set(UPDATE_API) <= declared
    out = subprocess.run(["nm", "-D", qr.LIB_PATH], capture_output=True, text=True).stdout
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    assert set(UPDATE_API) <= exported
    for name in UPDATE_API:
        assert getattr(qr.lib, name).argtypes, name
    txt = open(qr.HEADER).read()
    assert "8d. Batched row append and removal" in txt and txt.index("8d. Batched row") > txt.index("8c. Batched singular")
    for meth in ("tpqrt_batched", "tphqrt_batched", "tpmqrt_batched"):
        assert callable(getattr(qr.Plan, meth))
    for meth in ("push", "pop", "slide", "factor", "factor_host", "solve", "reset", "close"):
        assert callable(getattr(qr.LsAccumulatorBatched, meth))
    assert callable(qr.lstsq_rolling_batched) and callable(qr.tpqrt_batched_max_rows)


def test_max_rows_table(qr):
    """256: one block row per thread.  226: 64 columns at the leading dimension 226 (2 mod 32) beside the 64 x 65 triangle, tau and the
    partial sums are 64 * (226 + 65) + 72 = 18696 doubles of the 20480 in 160 KiB; at 258 they would be 20744."""
    assert [qr.lib.qr_tpqrt_batched_max_rows(c) for c in (0, 1, 32, 33, 64, 65)] == [0, 256, 256, 226, 226, 0]
    assert [qr.tpqrt_batched_max_rows(c) for c in (0, 1, 32, 33, 64, 65)] == [0, 256, 256, 226, 226, 0]
    assert qr.lib.qr_tpqrt_batched_max_rows(-3) == 0
    ld = lambda p: ((p + 29) // 32) * 32 + 2
    assert ld(226) == 226 and ld(227) == 258 and 64 * (226 + 65) + 72 <= 160 * 1024 // 8 < 64 * (258 + 65) + 72


def test_host_code_stays_out_of_the_stubbed_translation_unit():
    src = open(os.path.join(ROOT, "cuda-qr_amd", "csrc", "qr_host.c")).read()
    assert "qrd_bu_" not in src
    mk = open(os.path.join(ROOT, "cuda-qr_amd", "Makefile")).read()
    assert "build/qr_batched_update_c.o" in mk.split("\nOBJS =")[1].splitlines()[0]
    lab = mk.split("\nLAB_OBJS =")[1]
    assert "build/lab/qr_batched_update_c.o" in lab[:lab.index("$(LAB):")]
    assert "csrc/qr_batched_update.c" in mk and "qr_batched_update" in mk.split("HIPSRC =")[1].splitlines()[0].split()
    dev = open(os.path.join(ROOT, "cuda-qr_amd", "csrc", "qr_device.h")).read()
    for w in ("qrd_bu_update", "qrd_bu_apply", "qrd_bu_solve_prep", "qrd_bu_max_rows"):
        assert w in dev


class _FakePlan(C.Structure):
    """the leading fields of struct qr_plan (csrc/qr_plan_internal.h).  Every call below must reject its arguments before it reaches a
    device, or have batch == 0."""
    _fields_ = [("m", C.c_int), ("n", C.c_int), ("nb", C.c_int), ("ib", C.c_int), ("ldv", C.c_int), ("ldt", C.c_int),
                ("rest", C.c_char * 8192)]


def _plan():
    fp = _FakePlan()
    fp.m, fp.n, fp.nb, fp.ib, fp.ldv, fp.ldt = 16, 4, 4, 4, 128, 4
    return fp


def test_primitives_reject_bad_arguments_without_a_device(qr):
    L = qr.lib
    fp = _plan()
    P = C.cast(C.pointer(fp), C.c_void_p)
    buf = (C.c_double * 16)()
    d = C.cast(buf, C.c_void_p)           # never dereferenced
    ibuf = (C.c_int * 4)()
    di = C.cast(ibuf, C.c_void_p)
    E = qr.QR_E_ARG

    def tph(plan=P, R=d, n=20, ldr=20, sr=400, B=d, pa=6, pd=4, ldb=10, sb=200, tau=d, st=20, C1=d, ldc1=20, sc1=40, C2=d, ldc2=10, sc2=20,
            nrhs=2, info=di, batch=3):
        return L.qr_tphqrt_batched_dev(plan, R, n, ldr, sr, B, pa, pd, ldb, sb, tau, st, C1, ldc1, sc1, C2, ldc2, sc2, nrhs, info, batch)

    assert tph(batch=0) == 0
    assert tph(plan=None) == E and tph(R=None) == E and tph(B=None) == E and tph(tau=None) == E and tph(info=None) == E
    assert tph(C1=None) == E and tph(C2=None) == E
    assert tph(C1=None, C2=None, nrhs=0, batch=0) == 0                       # no right-hand sides: not referenced
    assert tph(n=0) == E and tph(n=-1) == E and tph(nrhs=-1) == E
    assert tph(n=63, ldr=63, sr=63 * 63, sb=630, st=63, ldc1=63, sc1=126, batch=0) == E      # n + nrhs = 65
    assert tph(n=62, ldr=62, sr=62 * 62, sb=620, st=62, ldc1=62, sc1=124, batch=0) == 0      # n + nrhs = 64
    assert tph(n=65, nrhs=0, ldr=65, sr=65 * 65, sb=650, st=65) == E
    assert tph(pa=0, pd=0) == E and tph(pa=-1, pd=11) == E and tph(pa=11, pd=-1) == E
    assert tph(pa=200, pd=56, ldb=256, sb=256 * 20, ldc2=256, sc2=512, batch=0) == 0         # 22 columns: 256 rows
    assert tph(pa=200, pd=57, ldb=257, sb=257 * 20, ldc2=257, sc2=514) == E
    assert tph(n=40, ldr=40, sr=1600, st=40, ldc1=40, sc1=80, pa=226, pd=0, ldb=226, sb=226 * 40, ldc2=226, sc2=452, batch=0) == 0
    assert tph(n=40, ldr=40, sr=1600, st=40, ldc1=40, sc1=80, pa=113, pd=114, ldb=227, sb=227 * 40, ldc2=227, sc2=454) == E
    assert tph(pa=2 ** 31 - 1, pd=2 ** 31 - 1) == E                           # the sum wraps: each count is checked on its own
    assert tph(ldr=19) == E and tph(ldb=9) == E and tph(ldc1=19) == E and tph(ldc2=9) == E
    assert tph(sr=399) == E and tph(sb=199) == E and tph(st=19) == E and tph(sc1=39) == E and tph(sc2=19) == E
    assert tph(ldr=21, sr=419) == E and tph(ldr=21, sr=420, batch=0) == 0
    assert tph(batch=-1) == E
    assert tph(batch=0, R=None) == E                                          # the checks come before the early return

    def tp(plan=P, R=d, n=20, ldr=20, sr=400, B=d, p=10, ldb=10, sb=200, tau=d, st=20, C1=d, ldc1=20, sc1=40, C2=d, ldc2=10, sc2=20, nrhs=2,
           batch=3):
        return L.qr_tpqrt_batched_dev(plan, R, n, ldr, sr, B, p, ldb, sb, tau, st, C1, ldc1, sc1, C2, ldc2, sc2, nrhs, batch)

    assert tp(batch=0) == 0
    assert tp(plan=None) == E and tp(R=None) == E and tp(B=None) == E and tp(tau=None) == E and tp(C1=None) == E and tp(C2=None) == E
    assert tp(n=0) == E and tp(n=63, ldr=63, sr=63 * 63, sb=630, st=63, ldc1=63, sc1=126) == E
    assert tp(p=0) == E and tp(p=-3) == E and tp(p=257, ldb=257, sb=257 * 20, ldc2=257, sc2=514) == E
    assert tp(ldr=19) == E and tp(ldb=9) == E and tp(ldc1=19) == E and tp(ldc2=9) == E
    assert tp(sr=399) == E and tp(sb=199) == E and tp(st=19) == E and tp(sc1=39) == E and tp(sc2=19) == E
    assert tp(batch=-1) == E

    def tpm(plan=P, trans=b"T", V=d, pa=6, pd=4, n=20, ldv=10, sv=200, tau=d, st=20, C1=d, ldc1=20, sc1=100, C2=d, ldc2=10, sc2=50, nrhs=5,
            batch=3):
        return L.qr_tpmqrt_batched_dev(plan, trans, V, pa, pd, n, ldv, sv, tau, st, C1, ldc1, sc1, C2, ldc2, sc2, nrhs, batch)

    assert tpm(batch=0) == 0
    assert tpm(plan=None) == E and tpm(V=None) == E and tpm(tau=None) == E and tpm(C1=None) == E and tpm(C2=None) == E
    assert tpm(trans=b"X") == E and tpm(trans=b"t") == E
    assert tpm(trans=b"N") == E                                               # 'N' with removed rows
    assert tpm(trans=b"N", pa=10, pd=0, batch=0) == 0
    assert tpm(n=0) == E and tpm(n=65, sv=650, st=65, ldc1=65, sc1=325) == E
    assert tpm(nrhs=0) == E and tpm(nrhs=-1) == E
    assert tpm(nrhs=300, sc1=6000, sc2=3000, batch=0) == 0                    # n + nrhs <= 64 binds only the fused calls
    assert tpm(pa=0, pd=0) == E and tpm(pa=-1, pd=11) == E and tpm(pa=257, pd=0, ldv=257, sv=257 * 20, ldc2=257, sc2=257 * 5) == E
    assert tpm(n=64, sv=640, st=64, ldc1=64, sc1=320, pa=227, pd=0, ldv=227, ldc2=227, sc2=227 * 5) == E
    assert tpm(ldv=9) == E and tpm(ldc1=19) == E and tpm(ldc2=9) == E
    assert tpm(sv=199) == E and tpm(st=19) == E and tpm(sc1=99) == E and tpm(sc2=49) == E
    assert tpm(batch=-1) == E
    assert list(ibuf) == [0, 0, 0, 0]


def test_accumulator_and_host_twin_reject_bad_arguments_without_a_device(qr):
    L = qr.lib
    fp = _plan()
    P = C.cast(C.pointer(fp), C.c_void_p)
    buf = (C.c_double * 16)()
    d = C.cast(buf, C.c_void_p)
    ibuf = (C.c_int * 4)()
    di = C.cast(ibuf, C.c_void_p)
    E = qr.QR_E_ARG
    h = C.c_void_p()
    assert L.qr_lsacc_batched_create(None, P, 8, 2, 0) == E and L.qr_lsacc_batched_create(C.byref(h), None, 8, 2, 0) == E
    assert L.qr_lsacc_batched_create(C.byref(h), P, 0, 2, 0) == E and L.qr_lsacc_batched_create(C.byref(h), P, 8, 0, 0) == E
    assert L.qr_lsacc_batched_create(C.byref(h), P, 60, 5, 0) == E and L.qr_lsacc_batched_create(C.byref(h), P, 8, 2, -1) == E
    for fn in ("qr_lsacc_batched_reset", "qr_lsacc_batched_destroy"):
        assert getattr(L, fn)(None) == E
    assert L.qr_lsacc_batched_factor_dev(None, None, None, None, None, None, None, None, None) == E
    # an accumulator over an empty batch allocates nothing and launches nothing: every call reaches its checks, and no device
    assert L.qr_lsacc_batched_create(C.byref(h), P, 8, 2, 0) == 0 and h.value
    a = h

    def push(acc=a, A=d, p=5, lda=5, sa=40, B=d, ldb=5, sb=10):
        return L.qr_lsacc_batched_push_dev(acc, A, p, lda, sa, B, ldb, sb)

    assert push() == 0 and push(p=1000, lda=1000, sa=8000, ldb=1000, sb=2000) == 0          # a push takes any number of rows
    assert push(acc=None) == E and push(A=None) == E and push(B=None) == E and push(p=0) == E and push(p=-1) == E
    assert push(lda=4) == E and push(ldb=4) == E and push(sa=39) == E and push(sb=9) == E

    def pop(acc=a, A=d, p=5, lda=5, sa=40, B=d, ldb=5, sb=10, info=di):
        return L.qr_lsacc_batched_pop_dev(acc, A, p, lda, sa, B, ldb, sb, info)

    assert pop() == 0 and pop(p=256, lda=256, sa=2048, ldb=256, sb=512) == 0
    assert pop(p=257, lda=257, sa=257 * 8, ldb=257, sb=514) == E                           # above the one-launch limit
    assert pop(acc=None) == E and pop(A=None) == E and pop(B=None) == E and pop(info=None) == E and pop(p=0) == E
    assert pop(lda=4) == E and pop(ldb=4) == E and pop(sa=39) == E and pop(sb=9) == E

    def slide(acc=a, An=d, pn=5, ldan=5, san=40, Bn=d, ldbn=5, sbn=10, Ao=d, po=3, ldao=3, sao=24, Bo=d, ldbo=3, sbo=6, info=di):
        return L.qr_lsacc_batched_slide_dev(acc, An, pn, ldan, san, Bn, ldbn, sbn, Ao, po, ldao, sao, Bo, ldbo, sbo, info)

    assert slide() == 0
    assert slide(pn=128, ldan=128, san=1024, ldbn=128, sbn=256, po=128, ldao=128, sao=1024, ldbo=128, sbo=256) == 0
    assert slide(pn=129, ldan=129, san=129 * 8, ldbn=129, sbn=258, po=128, ldao=128, sao=1024, ldbo=128, sbo=256) == E     # 257 rows
    assert slide(acc=None) == E and slide(An=None) == E and slide(Bn=None) == E and slide(Ao=None) == E and slide(Bo=None) == E
    assert slide(info=None) == E and slide(pn=0) == E and slide(po=0) == E and slide(pn=-1) == E
    assert slide(ldan=4) == E and slide(ldbn=4) == E and slide(ldao=2) == E and slide(ldbo=2) == E
    assert slide(san=39) == E and slide(sbn=9) == E and slide(sao=23) == E and slide(sbo=5) == E

    def solve(acc=a, X=d, ldx=8, sx=16, res=d, sres=2, info=di):
        return L.qr_lsacc_batched_solve_dev(acc, X, ldx, sx, res, sres, info)

    assert solve() == 0 and solve(res=None, sres=0) == 0
    assert solve(acc=None) == E and solve(X=None) == E and solve(info=None) == E and solve(ldx=7) == E and solve(sx=15) == E and solve(sres=1) == E
    r, z, s, w = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p()
    ldr, ldz, sr, sz = C.c_int(), C.c_int(), C.c_longlong(), C.c_longlong()
    assert L.qr_lsacc_batched_factor_dev(a, C.byref(r), C.byref(ldr), C.byref(sr), C.byref(z), C.byref(ldz), C.byref(sz), C.byref(s),
                                         C.byref(w)) == 0
    assert (ldr.value, sr.value, ldz.value, sz.value) == (8, 64, 8, 16)
    assert L.qr_lsacc_batched_reset(a) == 0 and L.qr_lsacc_batched_destroy(a) == 0
    # a wide accumulator: the limit is that of n + nrhs columns
    assert L.qr_lsacc_batched_create(C.byref(h), P, 40, 2, 0) == 0
    assert pop(acc=h, p=226, lda=226, sa=226 * 40, ldb=226, sb=452) == 0 and pop(acc=h, p=227, lda=227, sa=227 * 40, ldb=227, sb=454) == E
    assert L.qr_lsacc_batched_destroy(h) == 0

    dp = C.POINTER(C.c_double)
    hb = (C.c_double * 64)()
    p = C.cast(hb, dp)
    inf = (C.c_int * 16)()

    def roll(A=p, m=12, n=2, B=p, nrhs=1, batch=2, window=6, step=2, X=p, resid=None, info=inf):
        return L.qr_lstsq_rolling_batched(A, m, n, B, nrhs, batch, window, step, X, resid, info)

    assert roll(batch=0) == 0
    assert roll(A=None) == E and roll(B=None) == E and roll(X=None) == E and roll(info=None) == E
    assert roll(n=0) == E and roll(nrhs=0) == E and roll(batch=-1) == E and roll(m=0) == E
    assert roll(window=1) == E and roll(step=0) == E and roll(step=7) == E and roll(window=13) == E
    assert roll(n=60, nrhs=5, window=60, m=100) == E                          # n + nrhs > 64
    assert roll(m=1000, window=500, step=129) == E and roll(m=1000, window=500, step=128, batch=0) == 0     # 2 step <= 256
    assert roll(m=1000, n=40, window=500, step=114) == E and roll(m=1000, n=40, window=500, step=113, batch=0) == 0   # 2 step <= 226
    assert list(ibuf) == [0, 0, 0, 0]


def test_python_wrappers_raise_on_bad_shapes(qr):
    with pytest.raises(qr.QRError) as ei:
        qr.lstsq_rolling_batched(np.zeros((12, 2)), np.zeros((3, 12, 1)), 6, 2)               # A 2-D: not a batch
    assert ei.value.status == qr.QR_E_ARG
    with pytest.raises(qr.QRError) as ei:
        qr.lstsq_rolling_batched(np.zeros((3, 12, 2)), np.zeros((2, 12, 1)), 6, 2)            # B's batch is not A's
    assert ei.value.status == qr.QR_E_ARG
    with pytest.raises(qr.QRError) as ei:
        qr.lstsq_rolling_batched(np.zeros((3, 12, 2)), np.zeros((3, 11, 1)), 6, 2)            # B's height is not A's
    assert ei.value.status == qr.QR_E_ARG
    with pytest.raises(qr.QRError, match="invalid argument") as ei:
        qr.lstsq_rolling_batched(np.zeros((3, 12, 2)), np.zeros((3, 12, 1)), 1, 2)            # window < n: rejected by the library
    assert ei.value.status == qr.QR_E_ARG
