"""CPU tests that pin the oracle (oracle/mmqr_oracle.c) to the reference.

(a) against golden fixtures produced by the REAL reference qr.c (oracle/make_golden.py): bitwise;
(b) against the real reference itself (oracle/_ref/*.so) when those binaries are present: bitwise;
(c) the numpy blocked compact-WY mirror (what the HIP kernels implement) against the same golden
    sign-normalised R, to the tolerance the HIP parity tests use.
"""
import hashlib

import numpy as np
import pytest

from conftest import load_golden

CASES = [  # m, n, PR, PC, dtype
    (6, 4, 4, 2, np.float32),
    (6, 4, 4, 2, np.float64),
    (128, 32, 4, 2, np.float64),
    (120, 32, 64, 8, np.float64),
    (64, 20, 16, 4, np.float64),
    (512, 128, 64, 8, np.float64),
    (512, 128, 4, 2, np.float64),
    (1184, 640, 64, 8, np.float64),      # multi-panel fixture for the blocked GPU path (the restatement takes ~5 s on it)
]


def _name(m, n, PR, PC, dtype):
    return f"ref_{m}x{n}_{'f64' if dtype == np.float64 else 'f32'}_{PR}x{PC}"


def _sha(a):
    return hashlib.sha256(np.asfortranarray(a).tobytes(order="F")).hexdigest()


@pytest.mark.parametrize("m,n,PR,PC,dtype", CASES)
def test_generator_matches_reference(oracle, m, n, PR, PC, dtype):
    """srand(12)/rand() input (qr.c:468-474) is reproduced exactly."""
    g = load_golden(_name(m, n, PR, PC, dtype))
    A = oracle.fill_rand(m, n, 12, dtype)
    assert _sha(A) == str(g["sha_A"])
    assert A[0, 0] == g["A00"] and A[1, 0] == g["A10"]
    if (m, n) == (512, 128):   # the numbers SURVEY section 8c recorded from the reference run
        assert _sha(A)[:16] == "7ab1c8a44e80d121"
        assert abs(np.linalg.norm(A) - 147.772783345637) < 1e-9


@pytest.mark.parametrize("m,n,PR,PC,dtype", CASES)
def test_mmqr_restatement_bitwise_vs_golden(oracle, m, n, PR, PC, dtype):
    g = load_golden(_name(m, n, PR, PC, dtype))
    A = oracle.fill_rand(m, n, 12, dtype)
    F, tau, windows = oracle.mmqr(A, PR, PC)
    assert _sha(F) == str(g["sha_F"]), "factored matrix differs from the reference bit pattern"
    assert _sha(tau) == str(g["sha_tau"]), "tau differs from the reference bit pattern"
    if "F" in g:
        assert np.array_equal(F, g["F"]) and np.array_equal(tau, g["tau"])
    assert np.array_equal(np.diag(F[:n, :]), g["diagR"])


@pytest.mark.parametrize("m,n,PR,PC,dtype", [c for c in CASES if c[0] <= 128])
def test_explicit_qr_restatement_bitwise_vs_golden(oracle, m, n, PR, PC, dtype):
    g = load_golden(_name(m, n, PR, PC, dtype))
    Q, R = oracle.explicit_qr(g["F"], g["tau"], PR, PC, faithful=True)
    assert np.array_equal(Q, g["Q"]) and np.array_equal(R, g["R"])
    # the fast builder is the same reflectors as rank-1 updates: equal to rounding
    Q2, R2 = oracle.explicit_qr(g["F"], g["tau"], PR, PC, faithful=False)
    eps = np.finfo(dtype).eps
    assert np.abs(Q2 - Q).max() < 50 * eps and np.array_equal(R2, R)
    A = g["A"].astype(np.float64)
    assert np.linalg.norm(A - Q.astype(np.float64) @ R.astype(np.float64)) / np.linalg.norm(A) < 100 * eps


@pytest.mark.parametrize("m,n,PR,PC,dtype", CASES)
def test_restatement_bitwise_vs_real_reference(oracle, m, n, PR, PC, dtype):
    """Against the real reference where oracle/_ref was built; everywhere, against the digests of its outputs in the fixtures."""
    A = oracle.fill_rand(m, n, 12, dtype)
    F, tau, _ = oracle.mmqr(A, PR, PC)
    g = load_golden(_name(m, n, PR, PC, dtype))
    assert _sha(F) == str(g["sha_F"]) and _sha(tau) == str(g["sha_tau"])
    if oracle.ref_path(dtype, PR, PC) is not None:
        Fr, taur = oracle.ref_mmqr(A, PR, PC)
        assert np.array_equal(F, Fr) and np.array_equal(tau, taur)


def test_known_answers_from_survey(oracle):
    """Numbers recorded from the reference run in SURVEY section 8c."""
    A = oracle.fill_rand(6, 4, 12, np.float64)
    F, tau, windows = oracle.mmqr(A, 4, 2)
    assert windows == 4
    assert abs(F[0, 0] - (-1.41179614086601)) < 1e-13
    assert abs(F[1, 1] - (-0.793205848394169)) < 1e-13
    Ff, tauf, _ = oracle.mmqr(oracle.fill_rand(6, 4, 12, np.float32), 4, 2)
    np.testing.assert_allclose(tauf, [1.105875, 1.437911, 1.556454, 1.382508, 1.629178, 1.088601, 2, 2],
                               rtol=0, atol=5e-7)   # the "tau: ..." lines the committed binary prints
    np.testing.assert_allclose(np.diag(Ff[:4]), [-1.411796, -0.793206, -0.438200, 0.451158], atol=5e-7)
    F1, _, w1 = oracle.mmqr(oracle.fill_rand(512, 128), 64, 8)
    assert w1 == 135
    assert abs(F1[0, 0] - (-12.8905592562288)) < 1e-11 and abs(F1[1, 1] - (-8.1767397360128)) < 1e-11


def test_panel_dims(oracle):
    assert oracle.panel_dims(512, 128, 4, 2) == (255, 64)
    assert oracle.panel_dims(512, 128, 64, 8) == (9, 16)
    assert oracle.panel_dims(6, 4, 4, 2) == (2, 2)
    assert oracle.panel_dims(4, 4, 4, 2) == (1, 2)


@pytest.mark.parametrize("m,n,PR,PC", [(128, 32, 4, 2), (120, 32, 64, 8), (512, 128, 64, 8), (512, 128, 4, 2), (1184, 640, 64, 8)])
@pytest.mark.parametrize("nb", [8, 32])
def test_blocked_mirror_matches_reference_R(oracle, m, n, PR, PC, nb):
    """The blocked compact-WY algorithm (numpy mirror of the HIP path) gives the reference's R
    after sign normalisation -- the implementation-independent golden vector."""
    g = load_golden(_name(m, n, PR, PC, np.float64))
    A = oracle.fill_rand(m, n)
    F, tau, _ = oracle.np_geqrf(A, nb)
    Rn = oracle.sign_normalise(F)
    ref = g["Rn"] if "Rn" in g else None
    if ref is None:
        ref = np.zeros((n, n))
        ref[np.triu_indices(n)] = g["Rn_triu"]
    assert np.linalg.norm(np.triu(Rn) - ref) / np.linalg.norm(ref) <= 1e-13
    Q = oracle.np_orgqr(F, tau, n, nb)
    assert np.linalg.norm(A - Q @ np.triu(F[:n])) / np.linalg.norm(A) < 1e-14
    assert np.linalg.norm(Q.T @ Q - np.eye(n)) < 1e-13


def test_big_square_fixture_is_self_consistent(oracle):
    """ref_2024x2024 (161 s of the real reference, made once by oracle/make_golden.py) holds slices of the sign-normalised
    R plus digests; here: the generator digest, and the slices against LAPACK on the same input (the restatement itself is
    not re-run on it: 160 s)."""
    g = load_golden("ref_2024x2024_f64_64x8")
    A = oracle.fill_rand(2024, 2024)
    assert _sha(A) == str(g["sha_A"])
    Rl = oracle.sign_normalise(np.linalg.qr(A, mode="r"))
    assert np.linalg.norm(Rl[:32] - g["Rn_rows_head"]) / np.linalg.norm(g["Rn_rows_head"]) < 1e-12
    assert np.linalg.norm(Rl[:, -64:] - g["Rn_cols_tail"]) / np.linalg.norm(g["Rn_cols_tail"]) < 1e-12
    assert np.abs(np.diag(Rl) - g["Rn_diag"]).max() < 1e-11 * g["Rn_diag"].max()
    assert abs(np.linalg.norm(Rl) - float(g["Rn_fro"])) < 1e-9


def test_blocked_mirror_tsqr_shard_invariance(oracle):
    rng = np.random.default_rng(3)
    A = rng.random((4 * 96, 24))
    refR = oracle.sign_normalise(np.linalg.qr(A, mode="r"))
    for P in (1, 2, 4):
        R, Qs = oracle.np_tsqr(np.split(A, P), nb=8)
        assert np.linalg.norm(oracle.sign_normalise(R) - refR) / np.linalg.norm(refR) < 1e-13
        Q = np.vstack(Qs)
        assert np.linalg.norm(A - Q @ R) / np.linalg.norm(A) < 1e-14
        assert np.linalg.norm(Q.T @ Q - np.eye(24)) < 1e-13
