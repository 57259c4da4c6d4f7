"""-m gpu: the triangle-aware V*T product (gemm_nn_tri_kernel through qrd_gemm_nn_tri): C = V T with T upper triangular ends the k loop of
every column tile at the diagonal.  Against qrd_gemm_nn on the same operands, bit for bit (up to the sign of zero: the skipped terms are
v * 0, added last); with non-finite V the two differ (inf * 0), which is out of scope."""
import numpy as np
import pytest
import torch

from gpu_util import dev

pytestmark = pytest.mark.gpu

GUARD = 512               # doubles behind the output that must stay as they were
SENTINEL = -7.25


@pytest.fixture(scope="module")
def q(qr):
    qr.check(qr.lib.qrd_init(), "qrd_init")
    return qr


_DATA = {}


def _data(q, M, N, lda):
    """V (unit lower trapezoidal, zeros above, lda >= M rows in memory), T (upper triangular, exact zeros below), T with every entry the
    variant must not read -- column j from row 128 (j // 128 + 1) down -- turned into NaN, and qrd_gemm_nn's V T; once per shape"""
    key = (M, N, lda)
    if key not in _DATA:
        rng = np.random.default_rng(1000 * M + N)
        V = np.tril(rng.standard_normal((lda, N)), -1)
        V[np.arange(N), np.arange(N)] = 1.0
        V[M:] = rng.standard_normal((lda - M, N))          # rows of the array behind the operand: never part of the product
        T = np.triu(rng.standard_normal((N, N)))
        Tp = T.copy()
        i, j = np.indices((N, N))
        Tp[i >= 128 * (j // 128 + 1)] = np.nan
        dV, dT, dTp = dev(V), dev(T), dev(Tp)
        ref = _product(q, lambda *a: q.lib.qrd_gemm_nn(None, M, N, N, 1.0, *a[:4], 0.0, *a[4:]), M, N, lda, dV, dT)
        ref.setflags(write=False)
        _DATA[key] = (dV, dT, dTp, ref, bool(np.isnan(Tp).any()))
    return _DATA[key]


def _product(q, call, M, N, lda, dV, dT):
    """one product into a NaN-filled output (ld lda) with a guard band behind it: rows >= M and the guard band must stay as they were"""
    buf = torch.full((lda * N + GUARD,), float("nan"), dtype=torch.float64, device="cuda")
    buf[lda * N:] = SENTINEL
    torch.cuda.synchronize()
    q.check(call(dV.data_ptr(), lda, dT.data_ptr(), N, buf.data_ptr(), lda))
    q.check(q.lib.qrd_device_sync())
    flat = buf.cpu().numpy()
    assert np.all(flat[lda * N:] == SENTINEL), "guard band behind the output was written"
    out = flat[:lda * N].reshape(N, lda).T
    assert np.isnan(out[M:]).all(), "rows behind the output block were written"
    assert not np.isnan(out[:M]).any(), "an output element was never written"
    return out[:M].copy()


def _check(q, M, N, lda, tile, covered):
    dV, dT, dTp, ref, poison = _data(q, M, N, lda)
    if tile == 0:
        def entry(a, la, b, lb, c, lc):
            return q.lib.qrd_gemm_nn_tri(None, M, N, N, 1.0, a, la, b, lb, 0.0, c, lc)
    else:
        def entry(a, la, b, lb, c, lc):
            return q.lib.qrd_gemm_nn_tri_tile(None, tile, M, N, N, a, la, b, lb, c, lc)
    n0 = q.lib.qrd_vt_tri_launches()
    out = _product(q, entry, M, N, lda, dV, dT)
    assert q.lib.qrd_vt_tri_launches() - n0 == (1 if covered else 0)
    assert np.array_equal(out, ref)
    if poison:          # N > 128: what lies below the 128-row block of the diagonal is never read
        assert covered
        out2 = _product(q, entry, M, N, lda, dV, dTp)
        assert np.array_equal(out2, out)


@pytest.mark.parametrize("M,N,lda,covered", [
    (12288, 256, 12288, True),     # the <4,4> route of the general product
    (6144, 256, 6144, True),       # the <2,2> route
    (256, 256, 256, True),         # one row tile
    (1000, 256, 1008, True),       # ragged bottom tile, leading dimension != rows
    (4096, 128, 4096, True),
    (2048, 64, 2048, True),
    (2048, 96, 2048, True),        # ragged last panel
    (512, 32, 512, False),         # must fall back to the general product
])
def test_vt_tri_matches_the_general_product(q, M, N, lda, covered):
    _check(q, M, N, lda, 0, covered)


@pytest.mark.parametrize("tile", [44, 22, 11])
@pytest.mark.parametrize("M,N,lda", [
    (1000, 256, 1008),             # below 0.4 GFLOP: one guarded launch
    (6200, 256, 6200),             # whole-tile interior + a bottom strip
    (44000, 96, 44000),            # whole-tile interior + a right strip that starts at column 64 (tiles 44, 22) + a bottom strip
])
def test_vt_tri_every_tile(q, M, N, lda, tile):
    _check(q, M, N, lda, tile, True)
