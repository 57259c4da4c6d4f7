"""-m gpu: the kernels of the one-sided block Jacobi SVD (csrc/qr_svd.hip) at the launch layer, one launch at a time.

Through Plan.gesvj the pair kernel only ever runs inside the convergence loop, with the host's tournament pairs; its ragged last block,
its self-pair, the resident (r <= 128) against the streamed route, its "at or below tol: nothing is written" exit, the slot value,
V == NULL and the columns that belong to no pair of the launch are pinned down here, against the float64 instance of
hp_ref.jacobi_pair with every measure evaluated in longdouble.  With tol = sqrt(r) eps as the host sets it, for every pair of a launch:

  (a) its slot is within 64 eps (relative) of the measure of the input's pair;
  (b) V = I on entry, so V's pair columns hold J afterwards: ||G_in J - G_out|| / ||G_in|| and ||J^T J - I|| are at most
      max(4 x the float64 instance's, eps), capped at 20 * 64 eps and 4 * 20 * 64 eps (the plan test's s n eps with its s <= 20, n = 64);
  (c) the measure of G_out's pair is at most max(4 x the float64 instance's, tol) (r is at least the pair's column count everywhere);
  (d) the columns of G and V outside the launch's pairs and all padding (NaN in the rows r .. ldg of G) are bitwise untouched;
  (e) V = NULL gives bitwise the same G and slots;  (f) a repeat is bitwise equal;
  (g) a second launch on the output: its slot is at most 4 x the value of (c), and G is bitwise unchanged when that slot is <= tol;
      a matrix with orthogonal columns (a scaled permutation matrix) is bitwise untouched with a slot of exactly 0;
  (h) exactly zero columns stay exactly zero.

The small kernels (fold, colnorms, gather, permute, normalise, pinv_scale, rt) are checked bitwise, or to r eps for the norms, at their
256-thread strides, along permutation cycles and at the threshold equality of pinv_scale.
"""
import functools

import numpy as np
import pytest
import torch

import hp_ref as H
from gpu_util import Buf, bits, ivec, within

pytestmark = pytest.mark.gpu

EPS = H.EPS
NAN = float("nan")
JB = 32                       # QRD_JSVD_BLOCK
LEAD = 0x40000000             # QRD_JSVD_LEAD

ROUNDS = [(1, 1, ((0, 0),)), (17, 7, ((0, 0),)), (40, 32, ((0, 0),)), (128, 64, ((0, 1),)), (129, 40, ((0, 1),)), (130, 63, ((0, 1),)),
          (257, 64, ((0, 1),)), (300, 100, ((0, 3),)), (300, 128, ((0, 1), (2, 3))), (300, 128, ((0, 3), (1, 2)))]
ZERO_ROUNDS = [(40, 32, ((0, 0),)), (129, 40, ((0, 1),)), (300, 100, ((0, 3),))]

# tag -> the ratio to the float64 reference measured on an MI355X where it exceeds 4 (DESIGN.md has the table and the date); the bound
# of such a case is twice the ratio
MEASURED = {}


@pytest.fixture(scope="module")
def q(qr):
    qr.check(qr.lib.qrd_init(), "qrd_init")
    return qr


def _sync(q):
    q.check(q.lib.qrd_device_sync(), "sync")


def _cols(bp, bq, n):
    """(the columns of the block pair, how many of them are the first block's)"""
    cp = list(range(JB * bp, min(JB * bp + JB, n)))
    return cp + ([] if bq == bp else list(range(JB * bq, min(JB * bq + JB, n)))), len(cp)


def _zero_cols(n, pairs):
    """the second column of the first block and the last column of the last block of the launch"""
    return sorted({min(1, n - 1), _cols(*pairs[-1], n)[0][-1]})


@functools.lru_cache(maxsize=None)
def _round_input(r, n, pairs, zero):
    G = np.random.default_rng(100 * r + n).random((r, n)) - 0.5
    if zero:
        G[:, _zero_cols(n, pairs)] = 0.0
    G.setflags(write=False)
    return G


def _ld(x):
    return float(x)


@functools.lru_cache(maxsize=None)
def _pair_ref(r, n, pairs, zero, i):
    """pair i of the launch: (the measure of the input's pair, and of the float64 instance of jacobi_pair: ||G J - GJ|| / ||G||,
    ||J^T J - I||, the measure of its output), all evaluated in longdouble"""
    cols, wp = _cols(*pairs[i], n)
    Gp = _round_input(r, n, pairs, zero)[:, cols]
    _, GJ, J = H.jacobi_pair(Gp, np.sqrt(r) * EPS, np.float64, wp=wp)
    return (_ld(H.pair_measure(Gp)), _ld(H.norm(H.matmul(Gp, J) - H.arr(GJ)) / H.norm(Gp)),
            _ld(H.norm(H.matmul(J.T, J) - H.arr(np.eye(len(cols))))), _ld(H.pair_measure(GJ)))


def _launch_round(q, G, pairs, tol, with_v=True):
    """one qrd_jsvd_round on sentinel-framed buffers, NaN in G's padding rows, V = I: (bG, bV or None, slots)"""
    r, n = G.shape
    ldg, ldv = (r + 2) | 1, (n + 2) | 1
    bG, bV = Buf(G, ldg, pad=NAN), (Buf(np.eye(n), ldv) if with_v else None)
    pt, pp = ivec([b for pr in pairs for b in pr])
    bs = Buf(np.full((len(pairs), 1), -1.0), len(pairs), extra=0)
    q.check(q.lib.qrd_jsvd_round(None, bG.ptr, ldg, r, n, bV.ptr if with_v else None, ldv if with_v else 0, pp, len(pairs), tol, bs.ptr),
            "qrd_jsvd_round")
    _sync(q)
    return bG, bV, bs.check(np.ones((len(pairs), 1), bool), "slots")[:, 0]


def _round_out(bG, bV, pairs, rotated=True):
    """(G, V) after check (d): only the columns of the launch's pairs may change (nothing at all when rotated is False)"""
    r, n = bG.m, bG.n
    touched = np.zeros(n, bool)
    for pr in pairs:
        touched[_cols(*pr, n)[0]] = rotated
    G = bG.check(np.broadcast_to(touched, (r, n)), "G")
    return G, (bV.check(np.broadcast_to(touched, (n, n)), "V") if bV is not None else None)


def _check_round(q, r, n, pairs, zero=False):
    Gin = _round_input(r, n, pairs, zero)
    tol = np.sqrt(r) * EPS
    bG, bV, slots = _launch_round(q, Gin, pairs, tol)
    G, V = _round_out(bG, bV, pairs)
    assert np.all(np.isfinite(G)) and np.all(np.isfinite(V))
    cvals = []
    for i, pr in enumerate(pairs):
        cols, _ = _cols(*pr, n)
        k = len(cols)
        tag = f"jsvd_round r={r} n={n} pair {pr}" + (" zero columns" if zero else "")
        off, apply64, orth64, c64 = _pair_ref(r, n, pairs, zero, i)
        print(f"{tag}: slot {slots[i]:.17g}, the measure in longdouble {off:.17g}")
        assert abs(slots[i] - off) <= 64 * EPS * off                                                    # (a)
        J = V[np.ix_(cols, cols)]
        rest = np.delete(V[:, cols], cols, axis=0)
        assert np.all(rest == 0.0), "V = I: the rows of V's pair columns outside the pair stay zero"
        Gp = Gin[:, cols]
        e_apply = _ld(H.norm(H.matmul(Gp, J) - H.arr(G[:, cols])) / H.norm(Gp))
        e_orth = _ld(H.norm(H.matmul(J.T, J) - H.arr(np.eye(k))))
        within(f"{tag} G J", e_apply, apply64, 20 * 64 * EPS, MEASURED)                                  # (b)
        within(f"{tag} J^T J", e_orth, orth64, 4 * 20 * 64 * EPS, MEASURED)
        assert r >= k
        cval = _ld(H.pair_measure(G[:, cols]))
        within(f"{tag} measure after", cval, c64, measured=MEASURED, floor=tol)                          # (c)
        cvals.append(cval)
        if off <= tol:
            assert bits(G[:, cols], Gp) and bits(J, np.eye(k)), "at or below tol nothing is written"
    if zero:
        zc = _zero_cols(n, pairs)
        assert np.all(G[:, zc] == 0.0), "exact zero columns stay exactly zero"                            # (h)
    bG2, _, slots2 = _launch_round(q, Gin, pairs, tol, with_v=False)                                     # (e)
    assert bits(_round_out(bG2, None, pairs)[0], G) and bits(slots2, slots), "V = NULL changes neither G nor the slots"
    bG3, bV3, slots3 = _launch_round(q, Gin, pairs, tol)                                                 # (f)
    G3, V3 = _round_out(bG3, bV3, pairs)
    assert bits(G3, G) and bits(V3, V) and bits(slots3, slots), "a repeated launch is bitwise equal"
    bG4, _, slots4 = _launch_round(q, G, pairs, tol, with_v=False)                                       # (g)
    for i, pr in enumerate(pairs):
        print(f"jsvd_round r={r} n={n} pair {pr}: second launch slot {slots4[i] / tol:.3f} tol, the measure in longdouble {cvals[i] / tol:.3f} tol")
        assert slots4[i] <= 4 * cvals[i]
    if np.all(slots4 <= tol):
        _round_out(bG4, None, pairs, rotated=False)
    else:
        _round_out(bG4, None, pairs)


@pytest.mark.parametrize("r,n,pairs", ROUNDS, ids=lambda v: str(v).replace(" ", ""))
def test_one_round_against_the_reference(q, r, n, pairs):
    _check_round(q, r, n, pairs)


@pytest.mark.parametrize("r,n,pairs", ZERO_ROUNDS, ids=lambda v: str(v).replace(" ", ""))
def test_one_round_with_exact_zero_columns(q, r, n, pairs):
    _check_round(q, r, n, pairs, zero=True)


@pytest.mark.parametrize("r,n,pairs", [(40, 32, ((0, 0),)), (130, 63, ((0, 1),)), (300, 100, ((0, 3),))], ids=lambda v: str(v).replace(" ", ""))
def test_orthogonal_columns_are_left_bitwise_alone(q, r, n, pairs):
    """a scaled permutation matrix: every off-diagonal entry of the Gram matrix is exactly 0, so is the slot, and nothing is written"""
    rng = np.random.default_rng(r + n)
    G = np.zeros((r, n))
    G[rng.permutation(r)[:n], np.arange(n)] = np.ldexp(1.0 + rng.random(n), rng.integers(-20, 20, n))
    bG, bV, slots = _launch_round(q, G, pairs, np.sqrt(r) * EPS)
    assert bits(slots, np.zeros(len(pairs)))
    _round_out(bG, bV, pairs, rotated=False)


def test_round_refuses_bad_shapes(q):
    b = Buf(np.zeros((4, 4)), 5)
    pt, pp = ivec([0, 0])
    L = q.lib
    assert L.qrd_jsvd_round(None, b.ptr, 5, 0, 4, None, 0, pp, 1, 1e-15, b.ptr) == -7
    assert L.qrd_jsvd_round(None, b.ptr, 3, 4, 4, None, 0, pp, 1, 1e-15, b.ptr) == -7
    assert L.qrd_jsvd_round(None, b.ptr, 5, 4, 4, b.ptr, 3, pp, 1, 1e-15, b.ptr) == -7
    assert L.qrd_jsvd_round(None, b.ptr, 5, 4, 4, None, 0, pp, 0, 1e-15, b.ptr) == 0                # no pairs: nothing to do
    _sync(q)
    b.check(None, "a refused call")


def _vec(v, fill=-3.5):
    v = np.asarray(v, dtype=np.float64)
    return Buf(v[:, None], len(v), fill=fill, extra=0)


def _vec_out(b):
    return b.check(np.ones((b.m, 1), bool), "vector")[:, 0]


@pytest.mark.parametrize("count", [1, 256, 257, 1000])
@pytest.mark.parametrize("at", ["first", "last", "random"])
def test_fold_is_bitwise_the_maximum(q, count, at):
    rng = np.random.default_rng(count)
    s = rng.random(count)
    s[{"first": 0, "last": count - 1, "random": int(rng.integers(count))}[at]] = 1.5
    bs, bw = _vec(s, fill=9.0), _vec([-1.0])                       # (a sentinel above every slot: reading past count would show)
    q.check(q.lib.qrd_jsvd_fold(None, bs.ptr, count, bw.ptr), "qrd_jsvd_fold")
    _sync(q)
    bs.check(None, "slots")
    assert bits(_vec_out(bw), [s.max()])


@pytest.mark.parametrize("r", [1, 255, 257, 1000])
def test_colnorms(q, r):
    X = np.random.default_rng(r).random((r, 3)) - 0.5
    ldx = (r + 2) | 1
    bX, bo = Buf(X, ldx, pad=NAN), _vec(np.full(3, -1.0))
    q.check(q.lib.qrd_jsvd_colnorms(None, bX.ptr, ldx, r, 3, bo.ptr), "qrd_jsvd_colnorms")
    _sync(q)
    bX.check(None, "X")
    got = _vec_out(bo)
    for c in range(3):
        ref = H.norm(X[:, c])
        e = abs(float((H.arr(got[c]) - ref) / ref))
        print(f"colnorms r={r} column {c}: {e / EPS:.2f} eps (bound {r})")
        assert e <= r * EPS


def _with_leads(perm):
    """the flag on the first (smallest) column of every cycle, fixed points included, as qr_svd.c sets it"""
    n, out = len(perm), np.array(perm, dtype=np.int64)
    for j in range(n):
        k, lead = int(perm[j]), True
        while k != j:
            if k < j:
                lead = False
                break
            k = int(perm[k])
        if lead:
            out[j] |= LEAD
    return out


def _perms(n):
    rng = np.random.default_rng(n)
    mixed = np.arange(n)
    moving = rng.permutation(n)[:max(0, n - n // 3)]                # about a third of the columns stay where they are
    mixed[np.sort(moving)] = moving
    return {"identity": np.arange(n), "one cycle": np.roll(np.arange(n), -1), "random with fixed points": mixed,
            "random": rng.permutation(n)}


@pytest.mark.parametrize("rows", [1, 257])
@pytest.mark.parametrize("n", [1, 2, 33, 200])
def test_gather_and_permute_are_bitwise_a_column_selection(q, n, rows):
    rng = np.random.default_rng(10 * n + rows)
    for name, perm in _perms(n).items():
        assert sorted(perm) == list(range(n))
        M, sig = rng.standard_normal((rows, n)), rng.random(n)
        ld = (rows + 2) | 1
        pt, pp = ivec(_with_leads(perm))
        bM, bsig, bo = Buf(M, ld, pad=NAN), _vec(sig), _vec(np.full(n, -1.0))
        q.check(q.lib.qrd_jsvd_gather(None, bsig.ptr, pp, bo.ptr, n), "qrd_jsvd_gather")
        q.check(q.lib.qrd_jsvd_permute(None, bM.ptr, ld, rows, n, pp), "qrd_jsvd_permute")
        _sync(q)
        bsig.check(None, "sig")
        assert bits(_vec_out(bo), sig[perm]), (name, "gather")
        assert bits(bM.check(np.ones((rows, n), bool), "M"), M[:, perm]), (name, "permute")


@pytest.mark.parametrize("r", [1, 257])
def test_normalise_is_bitwise_numpy_division(q, r):
    rng = np.random.default_rng(r)
    n = 5
    X, sig = rng.standard_normal((r, n)), rng.random(n) + 0.5
    sig[2] = 0.0                                                    # a zero sigma leaves its column alone
    ld = (r + 2) | 1
    bX, bs = Buf(X, ld, pad=NAN), _vec(sig)
    q.check(q.lib.qrd_jsvd_normalise(None, bX.ptr, ld, r, n, bs.ptr), "qrd_jsvd_normalise")
    _sync(q)
    bs.check(None, "sig")
    ref = X.copy()
    ref[:, sig > 0] /= sig[sig > 0]
    assert bits(bX.check(np.ones((r, n), bool), "X"), ref) and bits(ref[:, 2], X[:, 2])


@pytest.mark.parametrize("n", [3, 300])
def test_pinv_scale_at_the_threshold_equality(q, n):
    """powers of two, so that rc sig[0] is exact and some sig[i] equals it: that row is zero (the test is >), the one above it is divided"""
    step = 1 if n == 3 else 8
    sig = np.ldexp(1.5, -(np.arange(n) // step))
    cut = 1 if n == 3 else 20
    rc = np.ldexp(1.0, -cut)
    equal = np.flatnonzero(sig == rc * sig[0])
    assert len(equal) == step and equal[0] == cut * step and sig[equal[0] - 1] > rc * sig[0]
    nrhs = 3
    T1 = np.random.default_rng(n).standard_normal((n, nrhs))
    b1, b2, bs = Buf(T1, n, extra=0), Buf(np.full((n, nrhs), -1.0), n, extra=0), _vec(sig)
    q.check(q.lib.qrd_jsvd_pinv_scale(None, b1.ptr, b2.ptr, n, nrhs, bs.ptr, rc), "qrd_jsvd_pinv_scale")
    _sync(q)
    b1.check(None, "T1")
    bs.check(None, "sig")
    ref = np.where((sig > rc * sig[0])[:, None], T1 / sig[:, None], 0.0)
    got = b2.check(np.ones((n, nrhs), bool), "T2")
    assert bits(got, ref)
    assert np.all(got[equal] == 0.0) and bits(got[equal[0] - 1], T1[equal[0] - 1] / sig[equal[0] - 1])


@pytest.mark.parametrize("n", [1, 33, 257])
def test_rt_is_bitwise_the_transposed_triangle(q, n):
    A = np.random.default_rng(n).standard_normal((n + 3, n))         # the factored matrix: R on and above the diagonal, reflectors below
    lda, ldw = (n + 5) | 1, (n + 2) | 1
    bA, bW = Buf(A, lda, pad=NAN), Buf(np.full((n, n), -1.0), ldw)
    q.check(q.lib.qrd_jsvd_rt(None, bA.ptr, lda, n, bW.ptr, ldw), "qrd_jsvd_rt")
    _sync(q)
    bA.check(None, "A")
    assert bits(bW.check(np.ones((n, n), bool), "W"), np.triu(A[:n]).T)
