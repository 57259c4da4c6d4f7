"""CPU-side checks of the bounded batched Levenberg-Marquardt solver (mi355x_qr.h section 8n): declared, exported, bound, wired into the
build beside the units that run over the stub device layer, the rules of section 8m shared and not copied, and every argument error and
phase-flag error without a device."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cuda-qr_amd", "csrc")
LMB_API = ("qr_lmb_batched_create", "qr_lmb_batched_start_dev", "qr_lmb_batched_step_dev", "qr_lmb_batched_update_dev", "qr_lmb_batched_view",
           "qr_lmb_batched_running", "qr_lmb_batched_destroy", "qr_lstsq_lm_bounded_batched")


def test_header_declares_and_library_exports_the_calls(qr):
    declared = set(qr.exported_symbols())
    assert set(LMB_API) <= declared
    out = subprocess.run(["nm", "-D", qr.LIB_PATH], capture_output=True, text=True).stdout
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    assert set(LMB_API) <= exported
    for name in LMB_API:
        assert getattr(qr.lib, name).argtypes, name
    txt = open(qr.HEADER).read()
    assert "8n. Batched Levenberg-Marquardt with box bounds" in txt
    sec = txt[txt.index("8n. Batched Levenberg-Marquardt with box bounds"):]
    assert txt.index("8n. Batched Levenberg-Marquardt with box bounds") > txt.index("8m. Batched Levenberg-Marquardt")
    for word in ("qr_lmb_batched_state", "peg", "clipped", "alpha", "MPFIT", "general linear constraints", "m < n",
                 "the step from factors that already exist"):
        assert word in sec, word
    for meth in ("start", "step", "update", "state", "running", "view"):
        assert callable(getattr(qr.LmBoundedBatched, meth))
    assert [k for k, _ in qr.LmBoundedState._fields_][:18] == [k for k, _ in qr.LmState._fields_]
    assert [k for k, _ in qr.LmBoundedState._fields_][18:] == ["lo", "hi", "alpha", "peg", "clipped"]


def test_the_unit_is_built_beside_the_stubbed_units_and_shares_the_rules():
    """Sections 8m and 8n are one host unit and one kernel file: the unit runs over the stub device layer with the others, the step is one
    kernel pair instantiated twice, and the rules of section 8m are written once."""
    import glob
    import re
    mk = open(os.path.join(ROOT, "cuda-qr_amd", "Makefile")).read()
    csrc_line = mk.split("\nCSRC =")[1].splitlines()[0].split()
    assert "csrc/qr_batched_lm.c" in csrc_line                                                 # CSRC is what the stub builds compile:
    assert mk.split("\nUNITS_LIB =")[1].splitlines()[0].split() == ["csrc/qr_host.c", "$(CSRC)"]      # UNITS_LIB
    assert "build/qr_batched_lm_c.o" in mk.split("\nOBJS =")[1].splitlines()[0].split()
    lab = mk.split("\nLAB_OBJS =")[1]
    assert "build/lab/qr_batched_lm_c.o" in lab[:lab.index("$(LAB):")].split()
    assert "CSRC_DEVICE_ONLY" not in mk and "qr_batched_lmb" not in mk
    assert "qr_batched_lm" in mk.split("HIPSRC =")[1].splitlines()[0].split()
    assert "csrc/qr_batched_lm_dev.h" in mk.split("\nHDRS =")[1].splitlines()[0]
    for gone in ("qr_batched_lmb.c", "qr_batched_lmb.hip"):
        assert not os.path.exists(os.path.join(CSRC, gone)), gone
    assert "qrd_blmb_" not in open(os.path.join(CSRC, "qr_host.c")).read()
    dev = open(os.path.join(CSRC, "qr_device.h")).read()
    for w in ("qrd_blmb_start", "qrd_blmb_peg", "qrd_blmb_step", "qrd_blmb_update", "qrd_blmb_state", "qrd_blmb_step_args"):
        assert w in dev
    unit = open(os.path.join(CSRC, "qr_batched_lm.c")).read()
    assert "qr_stage_open" in unit and unit.count("qr_stage_open(") == 1                       # one driver loop for both twins
    for call in ("qrd_blmb_peg(", "qrd_b_geqp3(", "qrd_b_ormqr(", "qrd_blm_step(", "qrd_blmb_step(", "qrd_blm_start(", "qrd_blmb_start(",
                 "qrd_blm_update(", "qrd_blmb_update("):
        assert unit.count(call) == 1, call                                                     # every launch is made in one place
    assert unit.index("qrd_blmb_peg(") < unit.index("qrd_b_geqp3(") < unit.index("qrd_b_ormqr(")      # the bounded step path: the peg first
    step = unit[unit.index("static int lm_step("):unit.index("static int lm_update(")]
    assert "qrd_blmb_peg(" in step and "qrd_b_geqp3(" in step and "lm_step_launch(" in step
    hdr = open(os.path.join(CSRC, "qr_batched_lm_dev.h")).read()
    lm = open(os.path.join(CSRC, "qr_batched_lm.hip")).read()
    for fn in ("blm_scalars", "blm_finish", "blm_fail", "blm_update_member", "blm_start_member"):
        assert "void " + fn + "(" in hdr, fn
        assert fn + "(" in lm and "void " + fn + "(" not in lm, fn                            # called in the kernels' file, defined in the header
    assert '#include "qr_batched_lm_dev.h"' in lm
    assert "actred" not in lm and "temp2" not in lm                                            # the update and rule h live in the header alone
    every = "".join(open(f).read() for f in sorted(glob.glob(os.path.join(CSRC, "*"))))
    for kernel in ("blm_step_wave_kernel", "blm_step_wg_kernel"):                              # one kernel pair, two instantiations
        assert len(re.findall(r"__global__\s+void\s+(?:__launch_bounds__\(\d+\)\s+)?" + kernel + r"\b", every)) == 1, kernel
    assert "blmb_step_wave_kernel" not in every and "blmb_step_wg_kernel" not in every
    for core in ("bt_wave_core", "bt_wg_core"):                                                # each search is called exactly once
        assert len(re.findall(core + r"\s*(?:<\w+>)?\(", lm)) == 1, core


class _FakePlan(C.Structure):
    """the leading fields of struct qr_plan (csrc/qr_plan_internal.h).  Every call below must reject its arguments before it reaches a
    device, or have batch == 0."""
    _fields_ = [("m", C.c_int), ("n", C.c_int), ("nb", C.c_int), ("ib", C.c_int), ("ldv", C.c_int), ("ldt", C.c_int),
                ("rest", C.c_char * 8192)]


def _plan():
    fp = _FakePlan()
    fp.m, fp.n, fp.nb, fp.ib, fp.ldv, fp.ldt = 16, 4, 4, 4, 128, 4
    return fp


NAN = float("nan")


def test_create_rejects_bad_arguments_without_a_device(qr):
    fp = _plan()
    P = C.cast(C.pointer(fp), C.c_void_p)
    E = qr.QR_E_ARG

    def create(plan=P, m=16, n=3, batch=0, out=True, **opt):
        h = C.c_void_p()
        rc = qr.lib.qr_lmb_batched_create(C.byref(h) if out else None, plan, m, n, batch, C.byref(qr.lm_options(**opt)))
        if rc == 0:
            assert qr.lib.qr_lmb_batched_destroy(h) == 0
        return rc

    assert create() == 0
    assert create(plan=None) == E and create(out=False) == E and create(batch=-1) == E
    assert create(m=2, n=3) == E and create(m=3, n=3) == 0 and create(n=0) == E and create(m=1, n=1) == 0
    assert create(m=64, n=64) == E and create(m=256, n=63) == 0 and create(m=257, n=63) == E      # the shape limits are section 8m's
    assert create(m=512, n=31) == 0 and create(m=513, n=31) == E and create(m=512, n=32) == E and create(m=256, n=32) == 0
    for k in ("ftol", "xtol", "gtol"):
        assert create(**{k: -1e-3}) == E and create(**{k: NAN}) == E and create(**{k: 0.0}) == 0
    assert create(factor=0.0) == E and create(factor=NAN) == E and create(factor=float("inf")) == E and create(factor=0.1) == 0
    assert create(par_rtol=0.0) == E and create(par_rtol=1.0) == E and create(par_rtol=NAN) == E and create(par_rtol=1e-3) == 0
    assert create(par_maxit=0) == E and create(maxfev=-1) == E and create(maxfev=1) == 0
    assert create(mode=0) == E and create(mode=3) == E and create(mode=2) == 0
    h = C.c_void_p()
    assert qr.lib.qr_lmb_batched_create(C.byref(h), P, 16, 3, 0, None) == 0      # no options: the defaults
    assert qr.lib.qr_lmb_batched_destroy(h) == 0 and qr.lib.qr_lmb_batched_destroy(None) == E


def test_calls_reject_bad_arguments_and_a_wrong_order_without_a_device(qr):
    fp = _plan()
    P = C.cast(C.pointer(fp), C.c_void_p)
    buf = (C.c_double * 16)()
    d = C.cast(buf, C.c_void_p)               # never dereferenced
    E = qr.QR_E_ARG
    lib = qr.lib
    m, n = 16, 3
    for mode in (1, 2):
        h = C.c_void_p()
        assert lib.qr_lmb_batched_create(C.byref(h), P, m, n, 0, C.byref(qr.lm_options(mode=mode))) == 0       # batch 0: no device
        try:
            def start(lm=h, X=d, ldx=n, sx=n, D=d, sd=n, lo=d, slo=n, hi=d, shi=n):
                return lib.qr_lmb_batched_start_dev(lm, X, ldx, sx, D, sd, lo, slo, hi, shi)

            def step(lm=h, J=d, ldj=m, sj=m * n, F=d, ldf=m, sf=m):
                return lib.qr_lmb_batched_step_dev(lm, J, ldj, sj, F, ldf, sf)

            def update(lm=h, F=d, ldf=m, sf=m):
                return lib.qr_lmb_batched_update_dev(lm, F, ldf, sf)

            cnt = C.c_int(7)
            # before start: nothing but start
            assert step() == E and update() == E and lib.qr_lmb_batched_running(h, C.byref(cnt)) == E
            assert start(lm=None) == E and start(X=None) == E and start(ldx=n - 1) == E and start(sx=n - 1) == E
            if mode == 2:
                assert start(D=None) == E and start(sd=n - 1) == E and start(sd=-1) == E and start(sd=0) == 0
            else:
                assert start(D=None, sd=-5) == 0                                   # mode 1: D0 and its stride are not looked at
            assert start(slo=n - 1) == E and start(slo=-1) == E and start(shi=n - 1) == E and start(shi=-1) == E
            assert start(slo=0, shi=0) == 0                                        # one vector shared by all members
            assert start(lo=None, slo=-5) == 0 and start(hi=None, shi=-5) == 0     # a side that is not there: its stride is not looked at
            assert start(lo=None, hi=None) == 0
            assert start() == 0 and start() == 0                                   # a restart is allowed at any time
            assert update() == E                                                   # update before a step
            # argument errors do not move the phase
            assert step(lm=None) == E and step(J=None) == E and step(F=None) == E
            assert step(ldj=m - 1) == E and step(sj=m * n - 1) == E and step(ldf=m - 1) == E and step(sf=m - 1) == E
            assert step() == 0
            assert step() == E                                                     # step twice in a row
            assert update(lm=None) == E and update(F=None) == E and update(ldf=m - 1) == E and update(sf=m - 1) == E
            assert update() == 0
            assert update() == E                                                   # update twice in a row
            assert step() == 0 and update() == 0
            assert start() == 0 and update() == E                                  # start puts the solver back in front of a step
            assert lib.qr_lmb_batched_running(h, None) == E and lib.qr_lmb_batched_running(None, C.byref(cnt)) == E
            assert lib.qr_lmb_batched_running(h, C.byref(cnt)) == 0 and cnt.value == 0
            v = qr.LmBoundedState()
            assert lib.qr_lmb_batched_view(h, C.byref(v)) == 0 and lib.qr_lmb_batched_view(h, None) == E
            assert lib.qr_lmb_batched_view(None, C.byref(v)) == E
        finally:
            assert lib.qr_lmb_batched_destroy(h) == 0
    assert not any(buf)


def test_host_twin_rejects_bad_arguments_without_a_device(qr):
    E = qr.QR_E_ARG
    dp = C.POINTER(C.c_double)
    hb = (C.c_double * 64)()
    p = C.cast(hb, dp)
    inf = (C.c_int * 16)()
    called = []
    fcn = qr.LM_FCN(lambda *a: called.append(a) or 0)

    def twin(f=fcn, m=5, n=3, batch=0, X=p, lo=p, hi=p, D=None, info=inf, **opt):
        return qr.lib.qr_lstsq_lm_bounded_batched(f, None, m, n, batch, X, lo, hi, D, C.byref(qr.lm_options(**opt)), None, None, None, None, info)

    assert twin() == 0 and twin(lo=None) == 0 and twin(hi=None) == 0 and twin(lo=None, hi=None) == 0
    assert twin(f=qr.LM_FCN()) == E and twin(X=None) == E and twin(info=None) == E and twin(batch=-1) == E
    assert twin(m=2, n=3) == E and twin(n=0) == E and twin(m=64, n=64) == E and twin(m=257, n=63) == E
    assert twin(mode=2) == E and twin(mode=2, D=p) == 0 and twin(ftol=-1.0) == E and twin(par_rtol=1.0) == E
    assert not called and not any(hb)


def test_python_wrappers_raise_on_bad_bounds(qr):
    f = lambda x: x
    for bad in ((np.zeros(4), None), (None, np.zeros((3, 3))), (np.zeros((2, 3, 1)), None), 5.0, (0.0,)):
        with pytest.raises(qr.QRError) as ei:
            qr.lstsq_lm_batched(f, f, np.zeros((2, 3)), m=3, bounds=bad)
        assert ei.value.status == qr.QR_E_ARG
    with pytest.raises(qr.QRError, match="invalid argument"):
        qr.lstsq_lm_batched(f, f, np.zeros((2, 3)), m=2, bounds=(0.0, None))                   # m < n: rejected by the library
    X, fnorm, nfev, njev, status, info = qr.lstsq_lm_batched(f, f, np.zeros((0, 3)), m=3, bounds=(-1.0, np.ones(3)))
    assert X.shape == (0, 3) and status.shape == (0,)
