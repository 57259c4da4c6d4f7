"""The componentwise bound of tests/gemm_ref.py on the CPU: correct summation orders satisfy it with room, planted faults break it by orders
of magnitude -- on the very shapes of tests/test_gpu_gemm_routes.py whose reference is the longdouble one -- and the padded-buffer layout
puts every element where it says.  No GPU."""
import numpy as np
import pytest

import gemm_ref as G
import hp_ref

SHAPES = G.ld_shapes()
ALPHA, BETA = -1.5, 0.75


_CASE = {}


def _case(M, N, K):
    """operands, the longdouble reference and the envelope of one shape, computed once"""
    if (M, N, K) not in _CASE:
        rng = np.random.default_rng(1000003 * M + 1009 * N + K)
        A, B, C0 = rng.standard_normal((M, K)), rng.standard_normal((K, N)), rng.standard_normal((M, N))
        ref, E, f = G.reference(A, B, ALPHA, BETA, C0)
        assert f == 1 and ref.dtype == hp_ref.LD
        for x in (A, B, C0, E):
            x.setflags(write=False)
        _CASE[(M, N, K)] = (A, B, C0, ref, E)
    return _CASE[(M, N, K)]


def test_the_shape_list_is_the_longdouble_one():
    assert len(SHAPES) >= 20 and all(M * N * K <= G.LD_LIMIT for M, N, K in SHAPES)
    P, _, f = G.product(np.ones((4, 3)), np.ones((3, 5)), False)
    assert f == 1 and P.dtype == hp_ref.LD and np.all(P == 3)
    big = np.ones((1, 10 ** 4 + 1))
    assert G.product(big, np.ones((10 ** 4 + 1, 10 ** 4)), False)[2] == 2           # above 1e8 multiply-adds: float64, f = 2


@pytest.mark.parametrize("M,N,K", SHAPES)
def test_correct_sums_in_any_order_are_within_the_bound(M, N, K):
    """float64 numpy, the reversed order and a 7-way split sum (the split-K shape: partial products, then the partials added)"""
    A, B, C0, ref, E = _case(M, N, K)
    n = G.terms(M, K)
    plain = ALPHA * (A @ B) + BETA * C0
    rev = ALPHA * (A[:, ::-1] @ B[::-1]) + BETA * C0
    parts = [A[:, c] @ B[c] for c in np.array_split(np.arange(K), 7) if len(c)]
    acc = parts[0]
    for p in parts[1:]:
        acc = acc + p
    split = ALPHA * acc + BETA * C0
    r = [G.ratio(x, ref, E, n, 1) for x in (plain, rev, split)]
    print(f"{M} x {N} x {K}: max |err| / bound  numpy {r[0]:.1e}  reversed {r[1]:.1e}  7-way split {r[2]:.1e}")
    assert max(r) <= 1.0


@pytest.mark.parametrize("M,N,K", SHAPES)
def test_planted_faults_are_far_outside_the_bound(M, N, K):
    """Each fault alone on float64 numpy's result.  A dropped term, two swapped rows, beta C0 applied twice and an unwritten strip must exceed
    the bound at least 100 times on every shape.  One operand element rounded to float32 moves one term of K by at most 2^-24 of itself,
    against a bound of (K + 3) 2^-52 times the sum of all K: with |a b| about the mean term that is 2^28 / (K (K + 3)) times the bound at
    the worst rounding and a quarter of that, 2^26 / (K (K + 3)), at the mean one -- at least 100 only while K (K + 3) <= 2^26 / 100, K <= 817.
    Up to there it is asserted at 100 as well; beyond, the bound -- which has to hold for any order of K roundings -- cannot see a
    float32 rounding of one term, and the ratio is printed only."""
    A, B, C0, ref, E = _case(M, N, K)
    n = G.terms(M, K)
    good = ALPHA * (A @ B) + BETA * C0
    i, j = M // 2, N // 3
    out = {}

    x = good.copy()
    x[i, j] -= ALPHA * A[i, K - 1] * B[K - 1, j]
    out["dropped k-term"] = x

    r0, r1 = (0, M - 1) if M > 1 else (0, 0)
    x = good.copy()
    x[[r0, r1]] = x[[r1, r0]]
    if M > 1:
        out["swapped rows"] = x

    x = good + BETA * C0
    out["beta C0 twice"] = x

    x = good.copy()
    x[M - 1:, :] = np.nan
    out["unwritten strip"] = x

    # the largest element of A in the row of the rest of the faults, rounded; the result recomputed with it
    k = int(np.argmax(np.abs(A[i])))
    A32 = A.copy()
    A32[i, k] = np.float32(A[i, k])
    assert A32[i, k] != A[i, k]
    x = good.copy()
    x[i] = ALPHA * (A32[i] @ B) + BETA * C0[i]
    f32 = G.ratio(x, ref, E, n, 1)

    r = {name: G.ratio(x, ref, E, n, 1) for name, x in out.items()}
    print(f"{M} x {N} x {K}: |err| / bound  " + "  ".join(f"{k_} {v:.1e}" for k_, v in r.items()) + f"  float32 operand {f32:.1e}")
    for name, v in r.items():
        assert v >= 100.0, name
    if K * (K + 3) <= 2 ** 26 // 100:
        assert f32 >= 100.0


def test_zero_envelope_demands_exactness_and_tm_is_triangular():
    A, B = np.zeros((3, 4)), np.ones((4, 2))
    ref, E, f = G.reference(A, B)
    assert np.all(E == 0) and G.ratio(np.zeros((3, 2)), ref, E, 7, f) == 0.0
    assert G.ratio(np.full((3, 2), 1e-300), ref, E, 7, f) == np.inf
    rng = np.random.default_rng(3)
    A, B, C0, T = rng.standard_normal((50, 8)), rng.standard_normal((50, 5)), rng.standard_normal((8, 5)), rng.standard_normal((8, 8))
    Tnan = np.triu(T) + np.tril(np.full((8, 8), np.nan), -1)
    with np.errstate(invalid="ignore"):
        ref, E, f = G.reference(A, B, 2.0, -1.0, C0, trans=True, Tm=Tnan)         # what lies below the diagonal is never read
    want = np.triu(T).T @ (2.0 * A.T @ B) - C0
    assert G.ratio(want, ref, E, G.terms(8, 50, tm=True), f) <= 1.0
    assert G.terms(8, 50, tm=True) == 62 and G.terms(8, 50) == 53


@pytest.mark.parametrize("rows,cols,ld,off,batch,stride", [(5, 3, 5, 0, 1, None), (5, 3, 8, 1, 1, None), (4, 2, 7, 1, 3, 20), (4, 2, 4, 0, 3, 0),
                                                          (1, 7, 3, 0, 5, 21), (0, 3, 2, 0, 1, None), (3, 2, 3, 0, 0, None)])
def test_layout_index_arithmetic(rows, cols, ld, off, batch, stride):
    L = G.Layout(rows, cols, ld, off, batch, stride)
    st = cols * ld if stride is None else stride
    assert L.base == G.GUARD + off and L.base % 2 == off          # an aligned allocation + an odd base = 8 bytes off a 16-byte boundary
    assert L.size == 2 * G.GUARD + 1 + L.span and L.base + L.span + G.GUARD <= L.size
    X = np.arange(1, batch * rows * cols + 1, dtype=np.float64).reshape(batch, rows, cols)
    if st == 0 and batch > 1:
        X[:] = X[0]                                               # one shared operand
    flat = L.pack(X if batch != 1 else X[0], G.SENTINEL)
    for z in range(batch):
        for j in range(cols):
            for i in range(rows):
                assert flat[G.GUARD + off + z * st + j * ld + i] == X[z, i, j]
    pad = L.padding()
    distinct = rows * cols * (1 if (st == 0 and batch > 0) else batch)
    assert pad.sum() == L.size - distinct and np.all(flat[pad] == G.SENTINEL) and not np.any(flat[~pad] == G.SENTINEL)
    assert pad[:L.base].all() and pad[L.base + L.span:].all() and pad[:G.GUARD].sum() == G.GUARD and pad[-G.GUARD:].sum() == G.GUARD
    back = L.unpack(flat)
    assert np.array_equal(back, X[0] if batch == 1 else X)
    nanflat = L.pack(X if batch != 1 else X[0], np.nan)
    assert G.same_bits(nanflat, nanflat.copy()) and np.isnan(nanflat[pad]).all()
    if distinct:
        other = nanflat.copy()
        other[L.base] = -other[L.base]
        assert not G.same_bits(nanflat, other)


def test_slab_sum_order():
    """the fixed order of the slab reduction, on values where the order shows: 1, 2^-53, 2^-53, ... gives 1 when the small terms are added one
    by one to the 1, more when they are added to each other first"""
    S = np.zeros((9, 1, 1))
    S[0], S[1:] = 1.0, 2.0 ** -53
    # one row: Mp = 32, nz = 8 groups; group 0 holds slabs 0 and 8 (the tail loop: ((1 + 2^-53) = 1), the others one small term each;
    # the groups are then added in ascending order: 1 + 2^-53 seven times = 1
    assert G.slab_sum(S)[0, 0] == 1.0
    S = np.arange(1.0, 1.0 + 5 * 300 * 2).reshape(5, 300, 2)
    assert np.array_equal(G.slab_sum(S), S.sum(axis=0))           # small integers: any order is exact
