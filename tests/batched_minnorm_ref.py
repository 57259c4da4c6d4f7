"""Inputs, references and error measures of the batched minimum-norm tests (mi355x_qr.h section 8e; helper module, no fixtures, no GPU).

A case is (rows, cols, nrhs, kind): `batch` tall members F (rows x cols), the wide system of a member is F^T X = B with B cols x nrhs.
kind "U": entries uniform in (-0.5, 0.5) from numpy's default_rng(seed); kind "cond": test_gpu_minnorm._cond_matrix at condition 1e6.
The reference is hp_ref.minnorm in longdouble; the yardstick is the float64 instance of the very same code on the same input.  Measures
per member, both evaluated in longdouble: the forward error ||X - X_ld|| / ||X_ld|| (cap 50 kappa(A) eps) and the residual
||A X - B|| / (||A||_2 ||X||) (cap rows eps), the two bounds of test_gpu_minnorm.py.

A member is kept only if the float64 instance stays under a QUARTER of both caps on it (the next seed is drawn otherwise, in a fixed
order): four times the reference then never reaches a cap, and what the GPU exceeds is the kernel's doing.  tests/
test_batched_minnorm_ref.py asserts that property for every case the GPU file uses.
"""
import functools

import numpy as np

import hp_ref as H

EPS = H.EPS
BATCH = 9

# (rows, cols, nrhs): the shapes of tests/test_gpu_batched_minnorm.py
SHAPES = [(1, 1, 1), (5, 3, 2), (17, 17, 1), (33, 8, 3), (64, 8, 1), (64, 28, 4), (64, 31, 1), (64, 31, 2), (65, 4, 1), (100, 33, 2),
          (256, 60, 4), (512, 30, 2), (64, 32, 40), (300, 40, 30)]
CASES = [s + ("U",) for s in SHAPES] + [(64, 28, 4, "cond")]
# fresh right-hand sides for the solves on existing factors: (rows, cols, nrhs) at the nrhs of the issue
AGAIN_NRHS = (1, 16, 17, 70)
AGAIN = [(64, 28), (100, 33)]


def U(seed, *shape):
    return np.random.default_rng(seed).random(shape) - 0.5


def cond_matrix(m, n, cond, seed):
    """test_gpu_minnorm._cond_matrix"""
    rng = np.random.default_rng(seed)
    Uo, _ = np.linalg.qr(rng.standard_normal((m, n)))
    V, _ = np.linalg.qr(rng.standard_normal((n, n)))
    return (Uo * np.logspace(0, -np.log10(cond), n)) @ V.T


def measures(Aw, B, X, Xld):
    """(forward error, residual) of one member's X, in longdouble; Aw is the wide matrix (cols x rows)"""
    X, Xld = H.arr(X), H.arr(Xld)
    fwd = float(H.norm(X - Xld) / H.norm(Xld))
    res = float(H.norm(H.matmul(Aw, X) - H.arr(B)) / (np.linalg.norm(Aw, 2) * H.norm(X)))
    return fwd, res


def caps(Aw):
    """(50 kappa eps, rows eps); rows is the length of X"""
    return 50.0 * np.linalg.cond(Aw) * EPS, Aw.shape[1] * EPS


def member(rows, cols, nrhs, kind, seed):
    F = U(seed, rows, cols) if kind == "U" else cond_matrix(rows, cols, 1e6, seed)
    B = U(seed + 500000, cols, nrhs)
    Aw = np.ascontiguousarray(F.T)
    Xld = H.minnorm(Aw, B)
    X64 = H.minnorm(Aw, B, np.float64)
    return dict(F=F, B=B, Xld=Xld, ref=measures(Aw, B, X64, Xld), caps=caps(Aw))


def quarter(m):
    return m["ref"][0] <= 0.25 * m["caps"][0] and m["ref"][1] <= 0.25 * m["caps"][1]


@functools.lru_cache(maxsize=None)
def case(rows, cols, nrhs, kind="U", batch=BATCH, salt=0):
    """`batch` kept members: F (batch, rows, cols), B (batch, cols, nrhs), read-only, and per member Xld, ref (the float64 instance's two
    measures) and caps"""
    out, seed = [], 1000 * rows + 10 * cols + nrhs + 77777 * salt + (31 if kind != "U" else 0)
    tries = 0
    while len(out) < batch:
        assert tries < 50 * batch, "no input on which the float64 instance keeps a quarter of the caps"
        m = member(rows, cols, nrhs, kind, seed + 7919 * tries)
        tries += 1
        if quarter(m):
            out.append(m)
    F, B = np.stack([m["F"] for m in out]), np.stack([m["B"] for m in out])
    F.setflags(write=False)
    B.setflags(write=False)
    return dict(F=F, B=B, Xld=[m["Xld"] for m in out], ref=[m["ref"] for m in out], caps=[m["caps"] for m in out])


def rhs_case(F, nrhs, seed):
    """fresh right-hand sides for existing members F (batch, rows, cols): B, and per member Xld, ref, caps -- the same quarter rule, by
    redrawing the right-hand sides"""
    Bs, Xld, ref, cp = [], [], [], []
    for q, Fq in enumerate(np.asarray(F)):
        Aw = np.ascontiguousarray(Fq.T)
        for tries in range(50):
            B = U(seed + 100 * q + 7919 * tries, Fq.shape[1], nrhs)
            xl = H.minnorm(Aw, B)
            r = measures(Aw, B, H.minnorm(Aw, B, np.float64), xl)
            c = caps(Aw)
            if r[0] <= 0.25 * c[0] and r[1] <= 0.25 * c[1]:
                break
        else:
            raise AssertionError("no right-hand side on which the float64 instance keeps a quarter of the caps")
        Bs.append(B); Xld.append(xl); ref.append(r); cp.append(c)
    return dict(B=np.stack(Bs), Xld=Xld, ref=ref, caps=cp)
