"""CPU-side checks of the batched covariance, standard errors and leverages (mi355x_qr.h section 8k): declared, exported, bound, wired
into the build, the row limit against its byte formula, the route predicates, and every argument error without a device."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import batched_stats_ref as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STATS_API = ("qr_stats_batched_max_rows", "qr_covar_batched_dev", "qr_leverage_batched_dev", "qr_gels_stats_batched_dev",
             "qr_lsacc_batched_covar_dev", "qr_lstsq_stats_batched")


def test_header_declares_and_library_exports_the_calls(qr):
    declared = set(qr.exported_symbols())
    assert set(STATS_API) <= declared
    out = subprocess.run(["nm", "-D", qr.LIB_PATH], capture_output=True, text=True).stdout
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    assert set(STATS_API) <= exported
    for name in STATS_API:
        assert getattr(qr.lib, name).argtypes, name
    txt = open(qr.HEADER).read()
    title = "8k. Batched covariance, standard errors and leverages"
    assert title in txt and txt.index(title) > txt.index("8j. Batched robust and weighted")
    assert "leverage and covariance" in txt[txt.index("8j. Batched robust and weighted"):txt.index(title)]      # 8j stays as written
    for name, value in (("QR_COV_UNSCALED", 0), ("QR_COV_SCALED", 1)):
        assert f"#define {name} {value}" in txt and getattr(qr, name) == value
        assert txt.index(f"#define {name} ") > txt.index(title)
    assert callable(qr.lstsq_stats_batched) and callable(qr.stats_batched_max_rows)
    assert callable(qr.Plan.covar_batched) and callable(qr.Plan.leverage_batched) and callable(qr.Plan.gels_stats_batched)
    assert callable(qr.LsAccumulatorBatched.covar)


def test_host_code_stays_out_of_the_stubbed_translation_unit():
    src = open(os.path.join(ROOT, "cuda-qr_amd", "csrc", "qr_host.c")).read()
    assert "qrd_bs_" not in src
    mk = open(os.path.join(ROOT, "cuda-qr_amd", "Makefile")).read()
    assert "build/qr_batched_stats_c.o" in mk.split("\nOBJS =")[1].splitlines()[0]
    lab = mk.split("\nLAB_OBJS =")[1]
    assert "build/lab/qr_batched_stats_c.o" in lab[:lab.index("$(LAB):")]
    assert "csrc/qr_batched_stats.c" in mk.split("\nCSRC =")[1].splitlines()[0]
    assert "qr_batched_stats" in mk.split("HIPSRC =")[1].splitlines()[0].split()
    dev = open(os.path.join(ROOT, "cuda-qr_amd", "csrc", "qr_device.h")).read()
    for w in ("qrd_bs_args", "qrd_bs_lev_args", "qrd_bs_fit_args", "qrd_bs_covar", "qrd_bs_leverage", "qrd_bs_fit", "qrd_bs_max_rows"):
        assert w in dev


def test_max_rows_at_its_edges_and_against_its_byte_formula(qr):
    mr = qr.stats_batched_max_rows
    assert mr(0) == 0 and mr(-1) == 0 and mr(64) == 0 and mr(65) == 0
    assert mr(1) == 512 and mr(8) == 512 and mr(31) == 512 and mr(63) >= 256       # 512 x 31 and 256 x 63 are taken

    def ld(x):
        return ((x + 29) // 32) * 32 + 2

    def nbytes(m, n):
        return 8 * ((n + 1) * ld(m) + n + 72)

    for n in range(1, 64):
        m = mr(n)
        assert m == S.max_rows(n)
        assert n <= m <= 512
        assert nbytes(m, n) <= 160 * 1024
        assert m == 512 or nbytes(m + 1, n) > 160 * 1024
        assert m >= qr.irls_batched_max_rows(n)                                      # the budget is within 8j's
    assert any(mr(n) < 512 for n in range(32, 64))


def test_route_predicates_at_their_edges(qr):
    L = qr.lib
    assert bool(L.qrd_bs_fit_wave_route(64, 31)) and not L.qrd_bs_fit_wave_route(65, 31) and not L.qrd_bs_fit_wave_route(40, 32)
    assert bool(L.qrd_bs_fit_wave_route(1, 1))
    for m in (1, 20, 64, 65, 300):
        for n in (1, 7, 30, 31, 32, 63):
            assert bool(L.qrd_bs_fit_wave_route(m, n)) == S.fit_wave_route(m, n) == bool(L.qrd_ir_wave_route(m, n))
    assert bool(L.qrd_bs_cov_wave_route(1)) and bool(L.qrd_bs_cov_wave_route(32)) and not L.qrd_bs_cov_wave_route(33)
    assert not L.qrd_bs_cov_wave_route(0)
    assert [L.qrd_bs_lev_chunks(k) for k in (0, 1, 256, 257, 1000)] == [0, 1, 1, 2, 4]


class _FakePlan(C.Structure):
    """the leading fields of struct qr_plan (csrc/qr_plan_internal.h).  Every call below must reject its arguments before it reaches a
    device, or have batch == 0."""
    _fields_ = [("m", C.c_int), ("n", C.c_int), ("nb", C.c_int), ("ib", C.c_int), ("ldv", C.c_int), ("ldt", C.c_int),
                ("rest", C.c_char * 8192)]


def _plan():
    fp = _FakePlan()
    fp.m, fp.n, fp.nb, fp.ib, fp.ldv, fp.ldt = 16, 4, 4, 4, 128, 4
    return fp


def test_device_calls_reject_bad_arguments_without_a_device(qr):
    L = qr.lib
    fp = _plan()
    P = C.cast(C.pointer(fp), C.c_void_p)
    buf = (C.c_double * 16)()
    d = C.cast(buf, C.c_void_p)           # never dereferenced
    ibuf = (C.c_int * 4)()
    di = C.cast(ibuf, C.c_void_p)
    E = qr.QR_E_ARG

    def cov(plan=P, R=d, n=8, ldr=20, sr=160, jp=di, sj=8, rk=di, mu=d, Cc=d, ldc=8, sc=64, se=d, sse=8, info=di, batch=3):
        return L.qr_covar_batched_dev(plan, R, n, ldr, sr, jp, sj, rk, mu, Cc, ldc, sc, se, sse, info, batch)

    assert cov(batch=0) == 0 and cov(jp=None, sj=0, rk=None, mu=None, batch=0) == 0
    assert cov(Cc=None, ldc=0, sc=0, batch=0) == 0 and cov(se=None, sse=0, batch=0) == 0 and cov(Cc=None, se=None) == E
    assert cov(plan=None) == E and cov(R=None) == E and cov(info=None) == E and cov(batch=-1) == E
    assert cov(n=0) == E and cov(n=-1) == E and cov(n=65, ldr=65, sr=65 * 65, ldc=65, sc=65 * 65, sse=65, sj=65) == E
    assert cov(n=64, ldr=64, sr=4096, ldc=64, sc=4096, sse=64, sj=64, batch=0) == 0
    assert cov(ldr=7) == E and cov(sr=159) == E and cov(ldr=8, sr=64, batch=0) == 0 and cov(sj=7) == E
    assert cov(ldc=7) == E and cov(sc=63) == E and cov(ldc=9, sc=71) == E and cov(ldc=9, sc=72, batch=0) == 0 and cov(sse=7) == E
    assert cov(batch=0, R=None) == E and cov(batch=0, ldc=7) == E and cov(batch=0, Cc=None, se=None) == E           # the checks come first

    def lev(plan=P, R=d, n=8, ldr=20, sr=160, jp=di, sj=8, rk=di, A=d, mrows=30, lda=30, sa=240, pr=d, spr=30, Hh=d, sh=30, info=di, batch=3):
        return L.qr_leverage_batched_dev(plan, R, n, ldr, sr, jp, sj, rk, A, mrows, lda, sa, pr, spr, Hh, sh, info, batch)

    assert lev(batch=0) == 0 and lev(jp=None, sj=0, rk=None, pr=None, spr=0, batch=0) == 0
    assert lev(plan=None) == E and lev(R=None) == E and lev(A=None) == E and lev(Hh=None) == E and lev(info=None) == E and lev(batch=-1) == E
    assert lev(n=0) == E and lev(n=65, ldr=65, sr=65 * 65, sj=65, sa=30 * 65) == E and lev(ldr=7) == E and lev(sr=159) == E and lev(sj=7) == E
    assert lev(mrows=0, lda=1, sa=8, spr=0, sh=1) == E and lev(lda=29) == E and lev(sa=239) == E and lev(sh=29) == E
    assert lev(spr=29) == E and lev(spr=-1) == E and lev(spr=0, batch=0) == 0 and lev(pr=None, spr=29) == E
    assert lev(mrows=1, lda=1, sa=8, spr=1, sh=1, batch=0) == 0                                                     # one row; below n is fine
    assert lev(mrows=100000, lda=100000, sa=800000, spr=100000, sh=100000, batch=0) == 0                             # not tied to section 8's rows
    assert lev(mrows=100000, lda=100000, sa=800000, spr=100000, sh=100000, batch=2 ** 31 - 1) == E                   # the grid does not fit
    assert lev(batch=0, A=None) == E and lev(batch=0, sh=29) == E

    def fit(plan=P, scaled=1, A=d, m=20, n=8, lda=20, sa=160, B=d, sb=20, pr=d, spr=20, X=d, sx=8, Ee=d, sE=20, Hh=d, sh=20, sg=d, dof=di,
            Cc=d, ldc=8, sc=64, se=d, sse=8, info=di, batch=3):
        return L.qr_gels_stats_batched_dev(plan, scaled, A, m, n, lda, sa, B, sb, pr, spr, X, sx, Ee, sE, Hh, sh, sg, dof, Cc, ldc, sc, se, sse,
                                           info, batch)

    def shaped(m, n, **kw):
        return fit(m=m, n=n, lda=m, sa=m * n, sb=m, spr=m, sx=n, sE=m, sh=m, ldc=n, sc=n * n, sse=n, **kw)

    assert fit(batch=0) == 0 and fit(scaled=0, batch=0) == 0 and fit(scaled=2) == E and fit(scaled=-1) == E
    assert fit(plan=None) == E and fit(A=None) == E and fit(B=None) == E and fit(X=None) == E and fit(info=None) == E and fit(batch=-1) == E
    assert fit(pr=None, Ee=None, sE=0, Hh=None, sh=0, sg=None, dof=None, Cc=None, ldc=0, sc=0, se=None, sse=0, batch=0) == 0
    assert fit(n=0) == E and shaped(70, 64) == E and shaped(70, 63, batch=0) == 0 and shaped(7, 8) == E and shaped(8, 8, batch=0) == 0
    assert shaped(1, 1, batch=0) == 0 and shaped(512, 31, batch=0) == 0 and shaped(513, 31) == E and shaped(256, 63, batch=0) == 0
    mr = L.qr_stats_batched_max_rows(63)
    assert 256 <= mr < 512 and shaped(mr, 63, batch=0) == 0 and shaped(mr + 1, 63) == E
    assert fit(lda=19) == E and fit(sa=159) == E and fit(sb=19) == E and fit(sx=7) == E and fit(sE=19) == E and fit(sh=19) == E
    assert fit(spr=19) == E and fit(spr=0, batch=0) == 0 and fit(pr=None, spr=19) == E
    assert fit(ldc=7) == E and fit(sc=63) == E and fit(sse=7) == E
    assert fit(batch=0, A=None) == E and fit(batch=0, sx=7) == E and fit(batch=0, scaled=5) == E                     # the checks come first

    assert list(ibuf) == [0, 0, 0, 0]


def test_accumulator_call_rejects_bad_arguments_without_a_device(qr):
    L = qr.lib
    E = qr.QR_E_ARG
    buf = (C.c_double * 16)()
    d = C.cast(buf, C.c_void_p)           # never dereferenced
    ibuf = (C.c_int * 4)()
    di = C.cast(ibuf, C.c_void_p)
    f = L.qr_lsacc_batched_covar_dev
    assert f(None, 1, 0, d, 8, 64, d, 8, d, di) == E                                                                 # no accumulator
    fp = _plan()
    acc = C.c_void_p()
    assert L.qr_lsacc_batched_create(C.byref(acc), C.cast(C.pointer(fp), C.c_void_p), 8, 2, 0) == 0                  # batch 0: no device
    try:
        def call(scaled=1, rhs=0, Cc=d, ldc=8, sc=64, se=d, sse=8, sg=d, info=di):
            return f(acc, scaled, rhs, Cc, ldc, sc, se, sse, sg, info)

        assert call() == 0 and call(scaled=0) == 0 and call(rhs=1) == 0 and call(sg=None) == 0
        assert call(Cc=None, ldc=0, sc=0) == 0 and call(se=None, sse=0) == 0 and call(ldc=9, sc=72) == 0
        assert call(scaled=2) == E and call(scaled=-1) == E
        assert call(rhs=-1) == E and call(rhs=2) == E and call(rhs=3) == E                                           # rhs outside 0 .. nrhs-1
        assert call(Cc=None, se=None) == E and call(info=None) == E
        assert call(ldc=7) == E and call(sc=63) == E and call(ldc=9, sc=71) == E and call(sse=7) == E
    finally:
        assert L.qr_lsacc_batched_destroy(acc) == 0
    assert list(ibuf) == [0, 0, 0, 0] and not any(buf)


def test_host_twin_rejects_bad_arguments_without_a_device(qr):
    L = qr.lib
    E = qr.QR_E_ARG
    dp = C.POINTER(C.c_double)
    hb = (C.c_double * 64)()
    p_ = C.cast(hb, dp)
    inf = (C.c_int * 16)()

    def twin(A=p_, m=5, n=3, b=p_, pr=p_, scaled=1, batch=2, X=p_, Ee=p_, Hh=p_, sg=p_, dof=inf, Cc=p_, se=p_, info=inf):
        return L.qr_lstsq_stats_batched(A, m, n, b, pr, scaled, batch, X, Ee, Hh, sg, dof, Cc, se, info)

    assert twin(batch=0) == 0 and twin(batch=0, pr=None, Ee=None, Hh=None, sg=None, dof=None, Cc=None, se=None) == 0
    assert twin(A=None) == E and twin(b=None) == E and twin(X=None) == E and twin(info=None) == E
    assert twin(m=2) == E and twin(n=0) == E and twin(m=70, n=64) == E and twin(batch=-1) == E and twin(scaled=2) == E
    assert twin(m=513, batch=0) == E and twin(m=512, batch=0) == 0 and twin(batch=0, A=None) == E
    assert list(inf) == [0] * 16


def test_python_wrappers_raise_on_bad_shapes(qr):
    z = np.zeros
    bad = [
        lambda: qr.lstsq_stats_batched(z((6, 4)), z((3, 6))),                              # A 2-D: not a batch
        lambda: qr.lstsq_stats_batched(z((3, 6, 4)), z((2, 6))),                           # b's batch is not A's
        lambda: qr.lstsq_stats_batched(z((3, 6, 4)), z((3, 5))),                           # b's height is not A's
        lambda: qr.lstsq_stats_batched(z((3, 6, 4)), z((3, 6, 2))),                        # two right-hand sides
        lambda: qr.lstsq_stats_batched(z((3, 6, 4)), z((3, 6)), weights=z(4)),             # the weights' length is not m
        lambda: qr.lstsq_stats_batched(z((3, 6, 4)), z((3, 6)), weights=z((2, 6))),        # their batch is not A's
    ]
    for f in bad:
        with pytest.raises(qr.QRError) as ei:
            f()
        assert ei.value.status == qr.QR_E_ARG
    with pytest.raises(qr.QRError, match="invalid argument") as ei:
        qr.lstsq_stats_batched(z((3, 3, 4)), z((3, 3)))                                    # m < n: rejected by the library
    assert ei.value.status == qr.QR_E_ARG
