"""CPU checks of tests/batched_minnorm_ref.py: every input the GPU test of section 8e uses goes through hp_ref.minnorm, and the float64
instance, measured against the longdouble one, stays under a quarter of each cap (50 kappa eps for the forward error, rows eps for the
residual) -- four times the reference alone then never reaches a cap."""
import numpy as np
import pytest

import batched_minnorm_ref as M
import hp_ref as H


@pytest.mark.parametrize("rows,cols,nrhs,kind", M.CASES)
def test_the_float64_instance_keeps_a_quarter_of_each_cap(rows, cols, nrhs, kind):
    for batch in (M.BATCH, 5) if (rows, cols, nrhs) in ((64, 28, 4), (100, 33, 2), (64, 32, 40), (300, 40, 30)) else (M.BATCH,):
        c = M.case(rows, cols, nrhs, kind, batch) if batch != M.BATCH else M.case(rows, cols, nrhs, kind)
        assert c["F"].shape == (batch, rows, cols) and c["B"].shape == (batch, cols, nrhs)
        if kind == "U":
            assert np.all(np.abs(c["F"]) < 0.5) and np.all(np.abs(c["B"]) < 0.5)
        else:
            assert np.all(np.array([np.linalg.cond(F) for F in c["F"]]) > 0.9e6)
        for q in range(batch):
            Aw = np.ascontiguousarray(c["F"][q].T)
            X64 = H.minnorm(Aw, c["B"][q], np.float64)
            fwd, res = M.measures(Aw, c["B"][q], X64, H.minnorm(Aw, c["B"][q]))
            cf, cr = M.caps(Aw)
            print(f"{rows}x{cols} nrhs={nrhs} {kind} member {q}: forward {fwd / cf:.3f} of its cap, residual {res / cr:.3f} of its cap")
            assert (fwd, res) == c["ref"][q]
            assert fwd <= 0.25 * cf and res <= 0.25 * cr
            assert 4 * fwd <= cf and 4 * res <= cr


@pytest.mark.parametrize("rows,cols", M.AGAIN)
@pytest.mark.parametrize("nrhs", M.AGAIN_NRHS)
def test_the_fresh_right_hand_sides_keep_it_too(rows, cols, nrhs):
    c = M.case(rows, cols, 4 if rows == 64 else 2, batch=5)
    r = M.rhs_case(c["F"], nrhs, 4242 + nrhs)
    assert r["B"].shape == (5, cols, nrhs)
    for q in range(5):
        assert r["ref"][q][0] <= 0.25 * r["caps"][q][0] and r["ref"][q][1] <= 0.25 * r["caps"][q][1]


def test_the_reference_solves_the_system_and_lies_in_the_row_space():
    c = M.case(33, 8, 3)
    for q in range(M.BATCH):
        Aw = np.ascontiguousarray(c["F"][q].T)
        X = np.asarray(c["Xld"][q], dtype=np.float64)
        Xn = np.linalg.lstsq(Aw, c["B"][q], rcond=None)[0]
        assert np.linalg.norm(X - Xn) <= 50 * np.linalg.cond(Aw) * H.EPS * np.linalg.norm(Xn)
        Q = np.linalg.qr(c["F"][q])[0]
        assert np.linalg.norm(X - Q @ (Q.T @ X)) <= 33 * H.EPS * np.linalg.norm(X)


def test_a_one_by_one_and_a_square_member():
    """1 x 1: x = b / a, one rounding; square: the last reflector is the identity (tau == 0)"""
    c = M.case(1, 1, 1)
    for q in range(M.BATCH):
        assert H.minnorm(c["F"][q].T, c["B"][q], np.float64)[0, 0] == c["B"][q][0, 0] / c["F"][q][0, 0]
    F, tau = H.qr(M.case(17, 17, 1)["F"][0], np.float64)
    assert tau[-1] == 0.0
