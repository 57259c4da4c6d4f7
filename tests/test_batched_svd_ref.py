"""The numpy restatement of the batched SVD (batched_svd_ref.py) checked without a GPU: every shape and input class of
test_gpu_batched_svd.py, R and jpvt from a numpy dlaqp2, Q from its reflectors, the bounds of that test.

Sweep counts of the restatement (the idle last sweep included) over all shapes: Gaussian 1 to 10, condition 1e6 1 to 9, condition
1e12 1 to 8, exact ranks 1 to 9, zero plus duplicated column 1 to 10, the zero matrix and the identity 1, mixed batches 1 to 10.  Every
rank came out exact and the four errors sat at 0.29 of their bounds or less (the largest: |U^T U - I| at n = 64).
"""
import functools

import numpy as np
import pytest

import batched_svd_ref as B


def test_circle_ordering_meets_every_pair_once_per_sweep():
    for n in (1, 2, 3, 8, 17, 32, 33, 64):
        seen = []
        for rd in range(B.rounds(n)):
            pairs = B.circle_pairs(n, rd)
            assert len(pairs) == n // 2
            cols = [c for pq in pairs for c in pq]
            assert len(set(cols)) == len(cols)                   # disjoint within a round
            assert all(0 <= p < q < n for p, q in pairs)
            seen += pairs
        assert sorted(seen) == [(p, q) for p in range(n) for q in range(p + 1, n)]


def test_circle_ordering_is_the_block_tournament_of_section_7(qr):
    for n in (2, 3, 8, 33, 64):                                  # blocks of one column: n * QR_JSVD_BLOCK columns
        for rd in range(B.rounds(n)):
            assert qr.jsvd_round_pairs(n * 32, rd) == B.circle_pairs(n, rd)


@functools.lru_cache(maxsize=None)
def _solved(kind, m, n):
    A, ranks = B.make_batch(kind, m, n)
    out = []
    for q in range(A.shape[0]):
        F, tau, jp = B.dlaqp2(A[q])
        S, V, W, rank, sweeps = B.jsvd_ref(F[:n], jp)
        U = B.form_q(F, tau) @ W
        out.append((S, U, V, rank, sweeps))
    return A, ranks, out


@pytest.mark.parametrize("kind,m,n", B.cases())
def test_restatement_meets_the_bounds(kind, m, n):
    A, ranks, out = _solved(kind, m, n)
    worst, sw = np.zeros(4), []
    for q, (S, U, V, rank, sweeps) in enumerate(out):
        assert sweeps < B.MAX_SWEEPS
        worst = np.maximum(worst, B.check_bounds(A[q], U, S, V, sweeps))
        assert np.all(S[rank:] == 0.0) and np.all(S[:rank] > 0.0)
        if ranks is not None:
            assert rank == ranks[q], (q, rank, ranks[q])
        sw.append(sweeps)
    print(f"restatement {kind} {m}x{n}: sweeps {sw}, fractions of the bounds (rec, sigma, V, U) {np.round(worst, 3)}")


def test_values_do_not_depend_on_the_accumulation():
    A, _ = B.make_batch("mixed", 33, 17)
    for q in range(A.shape[0]):
        F, tau, jp = B.dlaqp2(A[q])
        S, V, W, rank, sweeps = B.jsvd_ref(F[:17], jp)
        S2, V2, _, rank2, sweeps2 = B.jsvd_ref(F[:17], jp, want_w=False)
        assert np.array_equal(S, S2) and np.array_equal(V, V2) and (rank, sweeps) == (rank2, sweeps2)
