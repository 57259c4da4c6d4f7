"""-m gpu: the trailing update's four-workgroup kernel (gemm_nt4_kernel, qr_gemm_nt.hip) on the cases set for its late-C form (round 26:
accumulators from zero, the C tile fetched as per-lane 16-byte granules behind the last operand tile).  That form was measured and
removed; what it left in the kernel is the K loop's barrier that no longer drains the load queue (KEEP: the tile two ahead stays in
flight across the barrier, on a hand-counted s_waitcnt), and these cases guard exactly what such a barrier can break.

What can go wrong: a ring stage read before its loads have landed or overwritten while still being read (K = 32 and K = 48: the ring
is at its shortest, and wraps; every other case too -- the result is then stale LDS), a lane <-> row-pair mix-up of the C tile (the NaN
test: one 16-byte granule of C is NaN and must come back NaN, alone), rows of C beyond a ragged M read into the result or written.
Every case asserts from the route record that the KEEP kernel is what ran.
"""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from gpu_util import dev, host, rel, zeros

pytestmark = pytest.mark.gpu

ENTRY_NT, TILE_NT4, KEEP = 6, 42, 256          # QRD_ROUTE_ENTRY_NT, the 128 x 64 tile, QRD_ROUTE_KEEP of qr_device.h


@pytest.fixture(scope="module")
def q(qr):
    qr.check(qr.lib.qrd_init(), "qrd_init")
    for name in ("qrd_gemm_last_route", "qrd_gemm_nt_last_route"):
        getattr(qr.lib, name).restype = C.c_int
        getattr(qr.lib, name).argtypes = [C.POINTER(C.c_int)]
    return qr


def _record(q, name):
    out = (C.c_int * 8)()
    getattr(q.lib, name)(out)
    return dict(zip(("entry", "tile", "Mi", "Ni", "ksplit", "piece", "flags", "serial"), out))


def _update(q, M, N, K, gm, A, Bt, C0, lda, ldbt, ldc):
    dA, dB, dC = dev(A), dev(Bt), dev(C0)
    torch.cuda.synchronize()
    q.check(q.lib.qrd_gemm_nt(None, M, N, K, -1, dA.data_ptr(), lda, dB.data_ptr(), ldbt, dC.data_ptr(), ldc, gm, None))
    q.check(q.lib.qrd_device_sync(), "sync")
    r = _record(q, "qrd_gemm_last_route")
    assert (r["entry"], r["tile"], r["Mi"], r["Ni"]) == (ENTRY_NT, TILE_NT4, M, N) and r["flags"] & KEEP, r
    return host(dC)


#            M     N    K
SHAPES = [(128, 64, 32),         # one tile, nk = 4: the ring of three stages wraps once
          (128, 64, 48),         # nk = 6: the ring wraps twice
          (256, 192, 256),       # several tiles
          (130, 64, 64),         # ragged, 2 valid rows in the bottom tile
          (190, 128, 32),        # ragged with the smallest K
          (1150, 320, 256)]      # ragged, many tiles

_CASES = {}


def _case(M, N, K):
    """padded leading dimensions; rows of A beyond a ragged M are NaN (the tile loader reads them, nothing may use them); the numpy
    reference, once per shape and read-only"""
    if (M, N, K) not in _CASES:
        rng = np.random.default_rng(1009 * M + 31 * N + K)
        lda, ldbt, ldc = (M + 127) // 128 * 128 + 128, N + 6, M + 10
        A, Bt, C0 = rng.standard_normal((lda, K)), rng.standard_normal((ldbt, K)), rng.standard_normal((ldc, N))
        if M % 128:
            A[M:] = np.nan
        ref = C0.copy()
        ref[:M] -= A[:M] @ Bt[:N].T
        for x in (A, Bt, C0, ref):
            x.setflags(write=False)
        _CASES[(M, N, K)] = (A, Bt, C0, ref, lda, ldbt, ldc)
    return _CASES[(M, N, K)]


@pytest.mark.parametrize("gm", [0, 8])
@pytest.mark.parametrize("M,N,K", SHAPES)
def test_update_against_numpy(q, M, N, K, gm):
    """C -= A Bt^T: rel < 1e-13 (the tolerance tests/test_gpu_kernels.py holds this kernel to), rows of C beyond M bit-identical."""
    A, Bt, C0, ref, lda, ldbt, ldc = _case(M, N, K)
    assert q.lib.qrd_gemm_nt4_ok(M, N, K, None, lda, None, ldbt, None, ldc) == 1
    out = _update(q, M, N, K, gm, A, Bt, C0, lda, ldbt, ldc)
    err = rel(out[:M], ref[:M])
    print(f"{M} x {N} x {K}, gm {gm}: rel = {err:.2e}")
    assert not np.isnan(out).any()
    assert err < 1e-13
    assert np.array_equal(out[M:], C0[M:])


# (row, column) of the granule's first element: the row is even, the two rows are one lane's 16 bytes.  In wave (wi, wj) of tile
# (i0, j0) the granule (a, c, r) of lane (l4, l15) is rows i0 + 64 wi + 32 c + 2 (l4 + 4 r) + {0, 1} of column j0 + 32 wj + 2 l15 + a.
GRANULES = [(0, 0),                    # wave (0, 0), lane 0, (0, 0, 0)
            (18, 6),                   # l4 = 1, l15 = 3, (0, 0, 2)
            (44, 10),                  # l4 = 2, l15 = 5, (0, 1, 1)
            (62, 7),                   # l4 = 3, l15 = 3, (1, 1, 3)
            (64 + 52, 32 + 30),        # wave (1, 1): l4 = 2, l15 = 15, (0, 1, 2)
            (128 + 64 + 8, 128 + 2),   # tile (1, 2), wave (1, 0), l4 = 0, l15 = 1, (0, 0, 1)
            (254, 191)]                # the last granule of the matrix


@pytest.mark.parametrize("row,col", GRANULES)
def test_nan_in_one_granule_of_c_comes_back_only_there(q, row, col):
    """a lane <-> granule mix-up would move the NaN, or spread it"""
    M, N, K = 256, 192, 256
    A, Bt, C0, ref, lda, ldbt, ldc = _case(M, N, K)
    C1 = C0.copy()
    C1[row:row + 2, col] = np.nan
    out = _update(q, M, N, K, 8, A, Bt, C1, lda, ldbt, ldc)
    where = np.zeros_like(C1, dtype=bool)
    where[row:row + 2, col] = True
    assert np.array_equal(np.isnan(out), where)
    assert rel(out[~where], ref[~where]) < 1e-13


@pytest.mark.parametrize("m,n,nb,la", [(2048, 2048, 128, "0"), (4096, 2048, 256, "1")])
def test_factorisation_on_the_keep_update(q, m, n, nb, la):
    """geqrf on a single stream and on two: residual and orthogonality to the thresholds tests/test_gpu_qr.py holds its largest square
    case to, and the wide update on the nt4 route, KEEP form (qrd_gemm_nt's own record: the products that follow the last wide update leave it
    alone)."""
    os.environ["MI355XQR_LOOKAHEAD"] = la          # read at plan creation
    try:
        p = q.Plan(m, n, nb, 32)
    finally:
        del os.environ["MI355XQR_LOOKAHEAD"]
    dA = zeros(m, n)
    p.fill_uniform(dA, m, m, n, seed=12)
    p.sync()
    dtau, dQ, dR = zeros(n, 1), zeros(m, n), zeros(n, n)
    torch.cuda.synchronize()
    before = _record(q, "qrd_gemm_nt_last_route")["serial"]
    p.geqrf(dA, m, n, m, dtau)
    p.sync()
    r = _record(q, "qrd_gemm_nt_last_route")
    assert r["serial"] > before and (r["entry"], r["tile"]) == (ENTRY_NT, TILE_NT4) and r["flags"] & KEEP, r
    p.extract_r(dA, m, n, m, dR, n, n)
    p.applyq(dA, m, n, m, dtau, dQ, n, m, True)
    dQR, dG = zeros(m, n), zeros(n, n)
    p.gemm("N", m, n, n, 1.0, dQ, m, dR, n, 0.0, dQR, m)
    p.gemm("T", n, n, m, 1.0, dQ, m, dQ, m, 0.0, dG, n)
    p.sync()
    d, a = p.diffnorm(dQR, m, m, n, seed=12)
    o, _ = p.diffnorm(dG, n, n, n, mode=1)
    resid, orth = np.sqrt(d / a), np.sqrt(o)
    print(f"{m} x {n}, nb {nb}, look-ahead {la}: resid = {resid:.2e}  orth = {orth:.2e}")
    assert resid < 5e-14 and orth < 1e-11
    p.close()
