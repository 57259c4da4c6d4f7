"""CPU-side checks of the batched Levenberg-Marquardt solver (mi355x_qr.h section 8m): declared, exported, bound, wired into the build,
the search shared with section 8g, and every argument error and phase-flag error without a device."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cuda-qr_amd", "csrc")
LM_API = ("qr_lm_options_default", "qr_lm_batched_create", "qr_lm_batched_start_dev", "qr_lm_batched_step_dev", "qr_lm_batched_update_dev",
          "qr_lm_batched_view", "qr_lm_batched_running", "qr_lm_batched_destroy", "qr_lm_step_batched_dev", "qr_lstsq_lm_batched")


def test_header_declares_and_library_exports_the_calls(qr):
    declared = set(qr.exported_symbols())
    assert set(LM_API) <= declared
    out = subprocess.run(["nm", "-D", qr.LIB_PATH], capture_output=True, text=True).stdout
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    assert set(LM_API) <= exported
    for name in LM_API:
        assert getattr(qr.lib, name).argtypes, name
    txt = open(qr.HEADER).read()
    assert "8m. Batched Levenberg-Marquardt" in txt and txt.index("8m. Batched Levenberg-Marquardt") > txt.index("8l. Batched inequality")
    assert "Out of scope: the outer Levenberg-Marquardt loop" not in txt          # 8g no longer lists it as missing
    for word in ("qr_lm_batched_state", "qr_lm_options", "qr_lm_fcn", "lmdif", "equal to rounding"):
        assert word in txt[txt.index("8m. Batched Levenberg-Marquardt"):], word
    for meth in ("start", "step", "update", "state", "running", "view"):
        assert callable(getattr(qr.LmBatched, meth))
    assert callable(qr.Plan.lm_step_batched) and callable(qr.lm_batched) and callable(qr.lstsq_lm_batched)


def test_host_code_stays_out_of_the_stubbed_translation_unit():
    src = open(os.path.join(CSRC, "qr_host.c")).read()
    assert "qrd_blm_" not in src
    mk = open(os.path.join(ROOT, "cuda-qr_amd", "Makefile")).read()
    assert "build/qr_batched_lm_c.o" in mk.split("\nOBJS =")[1].splitlines()[0]
    lab = mk.split("\nLAB_OBJS =")[1]
    assert "build/lab/qr_batched_lm_c.o" in lab[:lab.index("$(LAB):")]
    assert "csrc/qr_batched_lm.c" in mk and "qr_batched_lm" in mk.split("HIPSRC =")[1].splitlines()[0].split()
    assert "csrc/qr_batched_trust_dev.h" in mk.split("\nHDRS =")[1].splitlines()[0]
    dev = open(os.path.join(CSRC, "qr_device.h")).read()
    for w in ("qrd_blm_start", "qrd_blm_step", "qrd_blm_update", "qrd_blm_state", "qrd_blm_step_args"):
        assert w in dev
    assert "qr_stage_open" in open(os.path.join(CSRC, "qr_batched_lm.c")).read()    # the twin stages through the shared helper


def test_one_search_for_both_kernel_files():
    """the state, the rules and the search bodies live in the shared header; section 8g's file and section 8m's both call them, and
    neither holds a copy"""
    hdr = open(os.path.join(CSRC, "qr_batched_trust_dev.h")).read()
    trust = open(os.path.join(CSRC, "qr_batched_trust.hip")).read()
    lm = open(os.path.join(CSRC, "qr_batched_lm.hip")).read()
    for fn in ("bt_start", "bt_leave", "bt_update", "bt_wave_core", "bt_wg_core", "bt_wave_solve", "bt_wg_wnorm"):
        assert fn + "(" in hdr, fn
    assert "struct bt_state" in hdr and "struct bt_state" not in trust and "struct bt_state" not in lm
    for f in (trust, lm):
        assert '#include "qr_batched_trust_dev.h"' in f
        for fn in ("bt_wave_core", "bt_wg_core"):
            assert fn in f, fn
        for fn in ("bt_start(", "bt_leave(", "bt_update("):
            assert fn not in f, fn                                                   # reached through the cores only
    assert "bd_wave_elim" in hdr and "bd_wg_elim" in hdr


class _FakePlan(C.Structure):
    """the leading fields of struct qr_plan (csrc/qr_plan_internal.h).  Every call below must reject its arguments before it reaches a
    device, or have batch == 0."""
    _fields_ = [("m", C.c_int), ("n", C.c_int), ("nb", C.c_int), ("ib", C.c_int), ("ldv", C.c_int), ("ldt", C.c_int),
                ("rest", C.c_char * 8192)]


def _plan():
    fp = _FakePlan()
    fp.m, fp.n, fp.nb, fp.ib, fp.ldv, fp.ldt = 16, 4, 4, 4, 128, 4
    return fp


def _ptrs():
    buf = (C.c_double * 16)()
    ibuf = (C.c_int * 4)()
    return buf, C.cast(buf, C.c_void_p), ibuf, C.cast(ibuf, C.c_void_p)     # never dereferenced


NAN = float("nan")


def test_defaults_are_lmder1s(qr):
    o = qr.lm_options()
    assert (o.ftol, o.xtol, o.gtol, o.factor, o.par_rtol) == (float(np.sqrt(np.finfo(float).eps)),) * 2 + (0.0, 100.0, 0.1)
    assert (o.maxfev, o.mode, o.par_maxit) == (0, 1, 10)                       # maxfev 0: 100 (n + 1)
    qr.lib.qr_lm_options_default(None)
    with pytest.raises(qr.QRError) as ei:
        qr.lm_options(tolerance=1.0)
    assert ei.value.status == qr.QR_E_ARG


def test_create_rejects_bad_arguments_without_a_device(qr):
    fp = _plan()
    P = C.cast(C.pointer(fp), C.c_void_p)
    E = qr.QR_E_ARG

    def create(plan=P, m=16, n=3, batch=0, out=True, **opt):
        h = C.c_void_p()
        rc = qr.lib.qr_lm_batched_create(C.byref(h) if out else None, plan, m, n, batch, C.byref(qr.lm_options(**opt)) if opt is not None else None)
        if rc == 0:
            assert qr.lib.qr_lm_batched_destroy(h) == 0
        return rc

    assert create() == 0
    assert create(plan=None) == E and create(out=False) == E and create(batch=-1) == E
    assert create(m=2, n=3) == E and create(m=3, n=3) == 0 and create(n=0) == E and create(m=1, n=1) == 0
    assert create(m=64, n=64) == E and create(m=256, n=63) == 0 and create(m=257, n=63) == E      # m <= qr_batched_max_rows(n + 1)
    assert create(m=512, n=31) == 0 and create(m=513, n=31) == E and create(m=512, n=32) == E and create(m=256, n=32) == 0
    for k in ("ftol", "xtol", "gtol"):
        assert create(**{k: -1e-3}) == E and create(**{k: NAN}) == E and create(**{k: 0.0}) == 0
    assert create(factor=0.0) == E and create(factor=-1.0) == E and create(factor=NAN) == E and create(factor=float("inf")) == E
    assert create(factor=0.1) == 0
    assert create(par_rtol=0.0) == E and create(par_rtol=1.0) == E and create(par_rtol=NAN) == E and create(par_rtol=1e-3) == 0
    assert create(par_maxit=0) == E and create(maxfev=-1) == E and create(maxfev=1) == 0
    assert create(mode=0) == E and create(mode=3) == E and create(mode=2) == 0
    h = C.c_void_p()
    assert qr.lib.qr_lm_batched_create(C.byref(h), P, 16, 3, 0, None) == 0      # no options: the defaults
    assert qr.lib.qr_lm_batched_destroy(h) == 0 and qr.lib.qr_lm_batched_destroy(None) == E


def test_calls_reject_bad_arguments_and_a_wrong_order_without_a_device(qr):
    fp = _plan()
    P = C.cast(C.pointer(fp), C.c_void_p)
    buf, d, ibuf, di = _ptrs()
    E = qr.QR_E_ARG
    lib = qr.lib
    m, n = 16, 3
    for mode in (1, 2):
        h = C.c_void_p()
        assert lib.qr_lm_batched_create(C.byref(h), P, m, n, 0, C.byref(qr.lm_options(mode=mode))) == 0       # batch 0: no device
        try:
            def start(lm=h, X=d, ldx=n, sx=n, D=d, sd=n):
                return lib.qr_lm_batched_start_dev(lm, X, ldx, sx, D, sd)

            def step(lm=h, J=d, ldj=m, sj=m * n, F=d, ldf=m, sf=m):
                return lib.qr_lm_batched_step_dev(lm, J, ldj, sj, F, ldf, sf)

            def fstep(lm=h, R=d, ldr=n, sr=n * n, Z=d, zrows=n, ldz=n, sz=n, rss=None, jp=None, sjp=0):
                return lib.qr_lm_step_batched_dev(lm, R, ldr, sr, Z, zrows, ldz, sz, rss, jp, sjp)

            def update(lm=h, F=d, ldf=m, sf=m):
                return lib.qr_lm_batched_update_dev(lm, F, ldf, sf)

            cnt = C.c_int(7)
            # before start: nothing but start
            assert step() == E and fstep() == E and update() == E and lib.qr_lm_batched_running(h, C.byref(cnt)) == E
            assert start(lm=None) == E and start(X=None) == E and start(ldx=n - 1) == E and start(sx=n - 1) == E
            if mode == 2:
                assert start(D=None) == E and start(sd=n - 1) == E and start(sd=-1) == E and start(sd=0) == 0
            else:
                assert start(D=None, sd=-5) == 0                                   # mode 1: D0 and its stride are not looked at
            assert start() == 0 and start() == 0                                   # a restart is allowed at any time
            assert update() == E                                                   # update before a step
            # argument errors do not move the phase
            assert step(lm=None) == E and step(J=None) == E and step(F=None) == E
            assert step(ldj=m - 1) == E and step(sj=m * n - 1) == E and step(ldf=m - 1) == E and step(sf=m - 1) == E
            assert step() == 0
            assert step() == E and fstep() == E                                    # step twice in a row
            assert update(lm=None) == E and update(F=None) == E and update(ldf=m - 1) == E and update(sf=m - 1) == E
            assert update() == 0
            assert update() == E                                                   # update twice in a row
            assert fstep(R=None) == E and fstep(Z=None) == E and fstep(ldr=n - 1) == E and fstep(sr=n * n - 1) == E
            assert fstep(zrows=n - 1) == E and fstep(zrows=m, ldz=m - 1, sz=m) == E and fstep(zrows=m, ldz=m, sz=m - 1) == E
            assert fstep(jp=di, sjp=n - 1) == E
            assert fstep(zrows=m, ldz=m, sz=m, rss=d, jp=di, sjp=n) == 0
            assert step() == E and update() == 0 and step() == 0 and update() == 0
            assert start() == 0 and update() == E                                  # start puts the solver back in front of a step
            assert lib.qr_lm_batched_running(h, None) == E and lib.qr_lm_batched_running(None, C.byref(cnt)) == E
            assert lib.qr_lm_batched_running(h, C.byref(cnt)) == 0 and cnt.value == 0
            v = qr.LmState()
            assert lib.qr_lm_batched_view(h, C.byref(v)) == 0 and lib.qr_lm_batched_view(h, None) == E
            assert lib.qr_lm_batched_view(None, C.byref(v)) == E
        finally:
            assert lib.qr_lm_batched_destroy(h) == 0
    assert list(ibuf) == [0, 0, 0, 0] and not any(buf)


def test_host_twin_rejects_bad_arguments_without_a_device(qr):
    E = qr.QR_E_ARG
    dp = C.POINTER(C.c_double)
    hb = (C.c_double * 64)()
    p = C.cast(hb, dp)
    inf = (C.c_int * 16)()
    called = []
    fcn = qr.LM_FCN(lambda *a: called.append(a) or 0)

    def twin(f=fcn, m=5, n=3, batch=0, X=p, D=None, info=inf, **opt):
        return qr.lib.qr_lstsq_lm_batched(f, None, m, n, batch, X, D, C.byref(qr.lm_options(**opt)), None, None, None, None, info)

    assert twin() == 0
    assert twin(f=qr.LM_FCN()) == E and twin(X=None) == E and twin(info=None) == E and twin(batch=-1) == E
    assert twin(m=2, n=3) == E and twin(n=0) == E and twin(m=64, n=64) == E and twin(m=257, n=63) == E
    assert twin(mode=2) == E and twin(mode=2, D=p) == 0 and twin(ftol=-1.0) == E and twin(par_rtol=1.0) == E
    assert not called and not any(hb)


def test_python_wrappers_raise_on_bad_shapes(qr):
    with pytest.raises(qr.QRError) as ei:
        qr.lstsq_lm_batched(lambda x: x, lambda x: x, np.zeros(3))                           # x0 1-D: not a batch
    assert ei.value.status == qr.QR_E_ARG
    with pytest.raises(qr.QRError) as ei:
        qr.lstsq_lm_batched(lambda x: x, lambda x: x, np.zeros((2, 3)), m=3, D=np.ones(4))
    assert ei.value.status == qr.QR_E_ARG
    with pytest.raises(qr.QRError) as ei:
        qr.lstsq_lm_batched(lambda x: x, lambda x: x, np.zeros((2, 3)), m=3, tolerance=1.0)
    assert ei.value.status == qr.QR_E_ARG
    with pytest.raises(qr.QRError, match="invalid argument"):
        qr.lstsq_lm_batched(lambda x: x, lambda x: x, np.zeros((2, 3)), m=2)                 # m < n: rejected by the library
    X, fnorm, nfev, njev, status, info = qr.lstsq_lm_batched(lambda x: x, lambda x: x, np.zeros((0, 3)), m=3)
    assert X.shape == (0, 3) and status.shape == (0,)
