"""A plain reference of the dense products of the GEMM launch layer, its componentwise error bound, and the padded-buffer layout of
tests/test_gpu_gemm_routes.py (helper module, no fixtures, no GPU).

    C = alpha op(A) B + beta C0                 op(A) = A (M x K) or A^T (A stored K x M)
    C = Tm^T (alpha A^T B) + beta C0            with the optional upper-triangular Tm (M x M) in front

Up to LD_LIMIT multiply-adds the product is accumulated in hp_ref.LD (longdouble, numpy's own loops: no BLAS); above that in float64
numpy.  Next to the reference comes the elementwise envelope

    E = |alpha| |op(A)| |B| + |beta| |C0|       (with Tm: |Tm|^T (|alpha| |A|^T |B|) + |beta| |C0|)

and the assertion used everywhere is componentwise,

    |got - ref|_ij <= f (K + 3) eps E_ij        (with Tm: K + M + 4 in place of K + 3),

f = 1 against the longdouble reference and f = 2 against the float64 one (which carries the same bound itself).  It is gamma_n E, n the
roundings on the way of one element: K for the sum of K products IN ANY ORDER (Higham, Accuracy and Stability, section 3.1: the bound
on a sum's error does not depend on the order; so any split-K, tile or pairwise order is covered, and an FMA only removes roundings),
one for alpha, one for beta C0, one for the last addition; Tm adds a second sum of at most M terms and its product.  eps = 2^-52 is twice the
unit roundoff, which pays for gamma_n = n u / (1 - n u) against n u and for the reference's own rounding many times over.  Nothing in it
was measured on a kernel.
"""
import numpy as np

import hp_ref

LD_LIMIT = 10 ** 8          # multiply-adds up to which the reference is accumulated in longdouble
EPS = hp_ref.EPS


def product(A, B, trans):
    """(P, Eab, f): P = op(A) B -- hp_ref.LD up to LD_LIMIT multiply-adds (f = 1), float64 numpy above (f = 2) -- and Eab = |op(A)| |B|"""
    A, B = np.asarray(A, dtype=np.float64), np.asarray(B, dtype=np.float64)
    Aop = A.T if trans else A
    M, K = Aop.shape
    assert B.shape[0] == K
    Eab = np.abs(Aop) @ np.abs(B)
    if M * B.shape[1] * K <= LD_LIMIT:
        return hp_ref.arr(Aop) @ hp_ref.arr(B), Eab, 1
    return Aop @ B, Eab, 2


def combine(P, Eab, alpha, beta, C0=None, Tm=None):
    """(ref, E) of alpha P + beta C0 (Tm^T in front of alpha P when Tm, upper triangular, is given); C0 is not read when beta == 0"""
    ld = P.dtype != np.float64
    lift = hp_ref.arr if ld else (lambda x: np.asarray(x, dtype=np.float64))
    ref, E = lift(alpha) * P, abs(alpha) * Eab
    if Tm is not None:
        Tm = np.triu(np.asarray(Tm, dtype=np.float64))
        ref, E = lift(Tm).T @ ref, np.abs(Tm).T @ E
    if beta != 0:
        ref, E = ref + lift(beta) * lift(C0), E + abs(beta) * np.abs(C0)
    return ref, E


def reference(A, B, alpha=1.0, beta=0.0, C0=None, trans=False, Tm=None):
    """(ref, E, f) in one call"""
    P, Eab, f = product(A, B, trans)
    ref, E = combine(P, Eab, alpha, beta, C0, Tm)
    return ref, E, f


def terms(M, K, tm=False):
    """the n of gamma_n: K + 3, with Tm K + M + 4"""
    return K + M + 4 if tm else K + 3


def bound(E, n, f):
    return f * n * EPS * np.asarray(E, dtype=np.float64)


def ratio(got, ref, E, n, f):
    """max_ij |got - ref| / (f n eps E): at most 1 for a correct result.  A NaN or infinity in got gives inf; where the envelope is zero
    (every term of the element is zero) the element must be exact."""
    got = np.asarray(got, dtype=np.float64)
    if not np.isfinite(got).all():
        return np.inf
    ld = ref.dtype != np.float64
    err = np.abs((hp_ref.arr(got) if ld else got) - ref).astype(np.float64)
    b = bound(E, n, f)
    if (err[b == 0] != 0).any():
        return np.inf
    nz = b > 0
    return float((err[nz] / b[nz]).max()) if nz.any() else 0.0


# ---- the padded device buffer of the GPU tests, as index arithmetic on a flat host array ---------------------------------------------
GUARD = 4096            # doubles in front of and behind every buffer
SENTINEL = -7.25        # what an output holds wherever the call must not write


class Layout:
    """`batch` column-major rows x cols matrices of leading dimension ld, matrix z at base + z * stride, inside a flat buffer

        [ GUARD doubles | off | matrices ... | GUARD doubles ]

    base = GUARD + off: the buffer itself is allocated 16-byte aligned (or better) and GUARD is even, so off = 1 puts the base 8 bytes off a
    16-byte boundary.  One spare double keeps the size independent of off.  Element (i, j) of matrix z is flat[base + z stride + j ld + i];
    everything else -- the guard bands, rows >= `rows` of every column, the gaps between strided matrices -- is padding.  A stride of 0
    (every batch member the same operand) is allowed."""

    def __init__(self, rows, cols, ld, off=0, batch=1, stride=None):
        assert off in (0, 1) and ld >= max(rows, 1) and rows >= 0 and cols >= 0 and batch >= 0
        self.rows, self.cols, self.ld, self.off, self.batch = rows, cols, ld, off, batch
        self.stride = cols * ld if stride is None else stride
        self.base = GUARD + off
        self.span = ((batch - 1) * self.stride + cols * ld) if batch > 0 else 0
        self.size = GUARD + 1 + self.span + GUARD

    def index(self):
        """flat indices of the logical elements, shape (batch, cols, rows)"""
        z = np.arange(self.batch, dtype=np.int64)[:, None, None] * self.stride
        j = np.arange(self.cols, dtype=np.int64)[None, :, None] * self.ld
        i = np.arange(self.rows, dtype=np.int64)[None, None, :]
        return self.base + z + j + i

    def pack(self, X, fill):
        """the flat buffer: X (rows x cols, or batch x rows x cols) in place, `fill` everywhere else"""
        X = np.asarray(X, dtype=np.float64)
        X3 = X[None] if X.ndim == 2 else X
        assert X3.shape == (self.batch, self.rows, self.cols), (X3.shape, self.batch, self.rows, self.cols)
        flat = np.full(self.size, fill, dtype=np.float64)
        flat[self.index()] = X3.transpose(0, 2, 1)
        return flat

    def unpack(self, flat):
        """the logical matrices out of a flat buffer: rows x cols for batch == 1, else batch x rows x cols"""
        X3 = np.asarray(flat)[self.index()].transpose(0, 2, 1).copy()
        return X3[0] if self.batch == 1 else X3

    def padding(self):
        """boolean mask over the flat buffer: True on everything that is not a logical element"""
        m = np.ones(self.size, dtype=bool)
        m[self.index()] = False
        return m


def same_bits(a, b):
    """bitwise equality of two float64 arrays (NaN payloads and signed zeros included)"""
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


def slab_sum(S):
    """the fixed-order float64 sum of qrd_slab_reduce's kernel for one row piece layout: S is nslab x M x N, summed per row piece of 256 rows.
    The 256 threads of a workgroup split the slab index nz = 256 / Mp ways (Mp = the piece's rows rounded up to 32); group g adds its
    slabs z = g, g + nz, ... into four interleaved partial sums (s0 + s1) + (s2 + s3), the tail into s0, and the groups are added in
    ascending order from zero."""
    S = np.asarray(S, dtype=np.float64)
    nslab, M, N = S.shape
    out = np.empty((M, N))
    for i0 in range(0, M, 256):
        Mc = min(256, M - i0)
        nz = 256 // ((Mc + 31) & ~31)
        tot = np.zeros((Mc, N))
        for g in range(nz):
            s = [np.zeros((Mc, N)) for _ in range(4)]
            z = g
            while z + 3 * nz < nslab:
                for q in range(4):
                    s[q] = s[q] + S[z + q * nz, i0:i0 + Mc]
                z += 4 * nz
            while z < nslab:
                s[0] = s[0] + S[z, i0:i0 + Mc]
                z += nz
            tot = tot + ((s[0] + s[1]) + (s[2] + s[3]))
        out[i0:i0 + Mc] = tot
    return out


# ---- the shapes of tests/test_gpu_gemm_routes.py (shared with tests/test_gemm_ref.py, which checks the bound's margin on the CPU) ----
# (name, M, N, K): op(A) is M x K.  The route each one is written for stands next to its test.
NN_WHOLE = {44: (2048, 1536), 22: (1024, 768), 11: (64, 64), 41: (12288, 32)}      # the smallest whole-tile shapes that nn_tile gives each tile
NN_STRIPS = {44: (2050, 1538, 128), 22: (1026, 898, 448), 11: (514, 258, 3024), 41: (12290, 32, 1024)}    # M N K >= 4e8, ragged
NN_SHAPES = ([(f"nn{t}_whole", m, n, 16) for t, (m, n) in NN_WHOLE.items()] + [(f"nn{t}_k21", m, n, 21) for t, (m, n) in NN_WHOLE.items()] +
             [(f"nn{t}_strips", *mnk) for t, mnk in NN_STRIPS.items()] +
             [("nn44_below", 2050, 1538, 64), ("nn41_guarded", 12290, 30, 64), ("nn_ld", 200, 96, 48)])
NN_UPDATE_SHAPES = [("up_tile", 128, 128, 16), ("up_whole", 256, 256, 64), ("up_strips", 386, 258, 32), ("up_k40", 256, 256, 40), ("up_m127", 127, 256, 32),
                    ("up_n100", 256, 100, 32), ("up_xcd", 1024, 256, 32), ("up_xcd_strips", 1026, 258, 32)]
TN_SHAPES = [("tn14_a", 32, 256, 4096), ("tn14_b", 24, 256, 2048), ("tn14_c", 32, 256, 4100),
             ("tn22_right", 64, 200, 2048), ("tn22_bottom", 130, 64, 2048), ("tn22_guarded", 130, 60, 2048),
             ("tn11_short", 96, 80, 496), ("tn11_strips", 100, 70, 512),
             ("tn44_whole", 128, 128, 2048), ("tn44_row", 128, 256, 4096), ("tn44_mixed", 130, 131, 4096),
             ("tn_split", 128, 128, 8192), ("tn_split32", 64, 32, 65536), ("tn_split64", 64, 32, 8192),
             ("tm32", 32, 96, 4096), ("tm100", 100, 40, 2048), ("tm256", 256, 64, 1024), ("tm32_one", 32, 96, 64),
             ("tn_krem", 512, 1024, 8200), ("tn_stream", 256, 256, 8192), ("tn_wide", 256, 256, 2048), ("tn_wide_strip", 130, 256, 2048)]
BATCH_SHAPES = [("batch32", 32, 32, 32), ("batch_ragged", 20, 40, 24)]


ALL_SHAPES = []          # distinct (M, N, K); the GPU file takes its operands through a lookup in this list, so it cannot use a shape missing here
for _name, _M, _N, _K in NN_SHAPES + NN_UPDATE_SHAPES + TN_SHAPES + BATCH_SHAPES:
    if (_M, _N, _K) not in ALL_SHAPES:
        ALL_SHAPES.append((_M, _N, _K))


def ld_shapes():
    """the shapes whose reference is the longdouble one"""
    return [(M, N, K) for M, N, K in ALL_SHAPES if M * N * K <= LD_LIMIT]
