"""The host-pointer twins of the batched sections stage their blocks through csrc/qr_stage.c: every optional output keeps its place in the
one device allocation whether the caller wants it or not, and is handed to the _dev call, and downloaded, only when it is wanted.

Here: the twins that no other file calls both ways (test_gpu_batched_svd.py, _bvls.py, _irls.py and _lsei.py do that for theirs; the thin,
plain least-squares and minimum-norm twins have no optional device block).  Each is called with every optional output NULL, with all of
them given, and with every second one given.  The mandatory outputs and the return code must be identical in all three, and an optional
output the same whenever it is asked for.  No tolerance: the same kernels run on the same data at the same offsets.

Shapes: batch 3 at the smallest shapes of each section's own list that have more than one row and column (batched_damped_ref.SHAPES / WIDE,
test_batched_trust_ref.CASES, batched_lse_ref.SHAPES, batched_stats_ref.FIT_SHAPES; 5 x 3 for sections 8b and 8d); damped and trust once
tall and once wide."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

BATCH = 3
SENTINEL, ISENT = -7.25e300, -12345
DP, IP = C.POINTER(C.c_double), C.POINTER(C.c_int)


class Out:
    def __init__(self, name, shape, optional=False, dtype=np.float64):
        self.name, self.shape, self.optional, self.dtype = name, shape, optional, dtype


def _rng(salt):
    return np.random.default_rng(20240 + salt)


def _pivoted():
    m, n, nrhs, g = 5, 3, 2, _rng(1)
    return "qr_lstsq_pivoted_batched", [g.standard_normal((BATCH, n, m)), m, n, g.standard_normal((BATCH, nrhs, m)), nrhs, BATCH, -1.0, 1,
                                        Out("X", (BATCH, nrhs, n)), Out("resid", (BATCH, nrhs), True), Out("rank", (BATCH,), True, np.intc),
                                        Out("jpvt", (BATCH, n), True, np.intc)]


def _rolling():
    m, n, nrhs, window, step, g = 12, 3, 2, 6, 2, _rng(2)
    nwin = (m - window) // step + 1
    return "qr_lstsq_rolling_batched", [g.standard_normal((BATCH, n, m)), m, n, g.standard_normal((BATCH, nrhs, m)), nrhs, BATCH, window, step,
                                        Out("X", (BATCH, nwin, nrhs, n)), Out("resid", (BATCH, nwin, nrhs), True),
                                        Out("info", (BATCH, nwin), False, np.intc)]


def _damped(m, n, nrhs, with_d):
    nlam, g = 2, _rng(3 + m)
    D = 0.5 + g.random((BATCH, n)) if with_d else None
    lam = np.tile([0.125, 1.5], (BATCH, 1))
    return "qr_lstsq_damped_batched", [g.standard_normal((BATCH, n, m)), m, n, g.standard_normal((BATCH, nrhs, m)), nrhs, BATCH, D, lam, nlam,
                                       Out("X", (BATCH, nlam * nrhs, n)), Out("xnorm", (BATCH, nlam * nrhs), True),
                                       Out("resid", (BATCH, nlam * nrhs), True), Out("info", (BATCH, nlam), False, np.intc)]


def _trust(m, n, with_d):
    g = _rng(20 + m)
    D = 0.5 + g.random((BATCH, n)) if with_d else None
    return "qr_lstsq_trust_batched", [g.standard_normal((BATCH, n, m)), m, n, g.standard_normal((BATCH, m)), BATCH, D, np.full(BATCH, 0.25), None,
                                      0.1, 20, Out("X", (BATCH, n)), Out("lam", (BATCH,)), Out("xnorm", (BATCH,), True),
                                      Out("resid", (BATCH,), True), Out("iter", (BATCH,), True, np.intc), Out("status", (BATCH,), True, np.intc),
                                      Out("info", (BATCH,), False, np.intc)]


def _constrained():
    m, n, p, nrhs, g = 3, 2, 1, 1, _rng(40)
    return "qr_lstsq_constrained_batched", [g.standard_normal((BATCH, n, m)), m, n, g.standard_normal((BATCH, n, p)), p,
                                            g.standard_normal((BATCH, nrhs, m)), g.standard_normal((BATCH, nrhs, p)), nrhs, BATCH,
                                            Out("X", (BATCH, nrhs, n)), Out("L", (BATCH, nrhs, p), True), Out("resid", (BATCH, nrhs), True),
                                            Out("info", (BATCH,), False, np.intc)]


def _stats():
    m, n, g = 5, 3, _rng(50)
    return "qr_lstsq_stats_batched", [g.standard_normal((BATCH, n, m)), m, n, g.standard_normal((BATCH, m)), None, 1, BATCH, Out("X", (BATCH, n)),
                                      Out("E", (BATCH, m), True), Out("H", (BATCH, m), True), Out("sigma2", (BATCH,), True),
                                      Out("dof", (BATCH,), True, np.intc), Out("Cov", (BATCH, n, n), True), Out("se", (BATCH, n), True),
                                      Out("info", (BATCH,), False, np.intc)]


CASES = {
    "pivoted": _pivoted,
    "rolling": _rolling,
    "damped-tall": lambda: _damped(5, 3, 2, True),
    "damped-wide": lambda: _damped(6, 7, 1, False),
    "trust-tall": lambda: _trust(5, 3, True),
    "trust-wide": lambda: _trust(3, 5, False),
    "constrained": _constrained,
    "stats": _stats,
}


def _call(fn, args, wanted):
    """one call of the twin; `wanted`: the names of the optional outputs that are given.  Returns (rc, {name: array})"""
    outs, cargs, keep = {}, [], []
    for a in args:
        if isinstance(a, Out):
            if a.optional and a.name not in wanted:
                cargs.append(None)
                continue
            outs[a.name] = np.full(a.shape, ISENT if a.dtype == np.intc else SENTINEL, dtype=a.dtype)
            cargs.append(outs[a.name].ctypes.data_as(IP if a.dtype == np.intc else DP))
        elif isinstance(a, np.ndarray):
            keep.append(np.ascontiguousarray(a, dtype=np.float64))
            cargs.append(keep[-1].ctypes.data_as(DP))
        else:
            cargs.append(a)
    return fn(*cargs), outs


@pytest.mark.parametrize("case", list(CASES))
def test_optional_outputs_do_not_move_the_others(qr, case):
    name, args = CASES[case]()
    fn = getattr(qr.lib, name)
    optional = [a.name for a in args if isinstance(a, Out) and a.optional]
    mandatory = [a.name for a in args if isinstance(a, Out) and not a.optional]
    assert optional and mandatory
    rc_none, none = _call(fn, args, ())
    rc_all, full = _call(fn, args, optional)
    rc_some, some = _call(fn, args, optional[::2])
    assert rc_none == rc_all == rc_some == 0, (rc_none, rc_all, rc_some)
    if "info" in full:
        assert np.all(full["info"] == 0)
    for k in mandatory + optional:                      # every block the caller gave was downloaded in full
        assert not np.any(full[k] == (ISENT if full[k].dtype == np.intc else SENTINEL)), k
    for k in mandatory:
        assert np.array_equal(none[k], full[k]) and np.array_equal(some[k], full[k]), k
    assert sorted(none) == sorted(mandatory) and sorted(some) == sorted(mandatory + optional[::2])
    for k in optional[::2]:
        assert np.array_equal(some[k], full[k]), k
