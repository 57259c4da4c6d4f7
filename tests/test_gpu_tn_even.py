"""-m gpu: the even static K split of the wide TN product Wt = A2^T (V T) (qr_tn_even.h; gemm_tn_kernel<.., EVEN> + tile_reduce_kernel),
forced through qrd_gemm_tn_update_even, against float64 numpy -- and one factorisation that runs it."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from gpu_util import dev

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PART = 128 * 128          # doubles of one partial tile
GUARD = 512               # doubles behind the output that must stay as they were
SENTINEL = -7.25


@pytest.fixture(scope="module")
def q(qr):
    qr.check(qr.lib.qrd_init(), "qrd_init")
    lib = qr.lib
    lib.qrd_stream_create_cumask.argtypes = [C.POINTER(C.c_void_p), C.c_int, C.c_int]
    lib.qrd_stream_sync.argtypes = [C.c_void_p]
    lib.qrd_stream_destroy.argtypes = [C.c_void_p]
    lib.qrd_stream_cus.argtypes = [C.c_void_p]
    return qr


_DATA = {}


def _data(M, N, K):
    """operands and the numpy reference, computed once per shape and shared by the tests that use it"""
    if (M, N, K) not in _DATA:
        rng = np.random.default_rng(M + N + K)
        A, B = rng.standard_normal((K, M)), rng.standard_normal((K, N))
        ref = A.T @ B
        ref.setflags(write=False)
        _DATA[(M, N, K)] = (dev(A), dev(B), ref)
    return _DATA[(M, N, K)]


def _run(q, M, N, K, nwg, cap, stream=None, forced=True):
    """two runs, each into a NaN-filled output with a guard band behind it and with a NaN-filled slab buffer; checks the result against numpy,
    run-to-run bit equality and the guard band; returns (even-split launches of the two runs, workgroups of the last one).  forced: through
    qrd_gemm_tn_update_even; else through qrd_gemm_tn_update, the wide update's own entry, where the library's cost model chooses"""
    dA, dB, ref = _data(M, N, K)
    outs = []
    n0 = q.lib.qrd_tn_even_launches()
    for rep in range(2):
        buf = torch.full((M * N + GUARD,), float("nan"), dtype=torch.float64, device="cuda")
        buf[M * N:] = SENTINEL
        slabs = torch.full((cap,), float("nan"), dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        args = (stream, M, N, K, 1.0, dA.data_ptr(), K, dB.data_ptr(), K, 0.0, buf.data_ptr(), M, slabs.data_ptr(), cap)
        q.check(q.lib.qrd_gemm_tn_update_even(*args, nwg) if forced else q.lib.qrd_gemm_tn_update(*args))
        q.check(q.lib.qrd_stream_sync(stream) if stream else q.lib.qrd_device_sync())
        flat = buf.cpu().numpy()
        assert np.all(flat[M * N:] == SENTINEL), "guard band behind the output was written"
        outs.append(flat[:M * N].reshape(N, M).T)
    err, tol = np.abs(outs[0] - ref).max(), 1e-12 * np.sqrt(K) * max(1.0, np.abs(ref).max())
    print(f"even split {M} x {N} x {K}, nwg {nwg}: max error {err:.3e} (tolerance {tol:.3e})")
    assert not np.isnan(outs[0]).any(), "an output element was never written, or a partial that was never written was summed"
    assert err < tol
    assert np.array_equal(outs[0], outs[1])
    return q.lib.qrd_tn_even_launches() - n0, q.lib.qrd_tn_even_last_grid()


@pytest.mark.parametrize("M,N,K,nwg", [
    (128, 128, 112, 3),        # one tile, 7 k-tiles over 3 workgroups: 2 / 2 / 3
    (256, 256, 80, 7),         # 20 units over 7 workgroups: ranges that cross tile boundaries
    (128, 128, 32, 8),         # more workgroups than units: six own nothing
    (256, 256, 64, 1),         # one workgroup walks every tile
    (256, 128, 64, 8),         # workgroup boundaries coincide with tile boundaries
    (512, 128, 32, 3),         # a workgroup that spans three tiles
])
def test_even_split_small_decompositions(q, M, N, K, nwg):
    launches, grid = _run(q, M, N, K, nwg, (nwg + (M // 128) * (N // 128)) * PART)       # exactly G + tiles partial tiles of slab space
    assert launches == 2 and grid == nwg


def test_even_split_grid_follows_the_stream(q):
    """nwg = 0: two workgroups per compute unit of the stream -- the device's on the default stream, 32 on a CU-masked stream of 32"""
    M, N, K = 1280, 256, 4096
    cus = q.lib.qrd_stream_cus(None)
    launches, grid = _run(q, M, N, K, 0, 1 << 24)
    assert launches == 2 and grid == 2 * cus
    st = C.c_void_p()
    q.check(q.lib.qrd_stream_create_cumask(C.byref(st), 0, 32))
    try:
        assert q.lib.qrd_stream_cus(st) == 32
        launches, grid = _run(q, M, N, K, 0, 1 << 24, stream=st)
        assert launches == 2 and grid == 64
    finally:
        q.check(q.lib.qrd_stream_destroy(st))


def test_even_split_falls_back_when_the_partials_do_not_fit(q):
    """slab space one partial tile short of G + tiles: the split-K path runs instead (it needs M N doubles only) and is as right"""
    M, N, K = 1280, 256, 4096
    G, tiles = 2 * q.lib.qrd_stream_cus(None), (M // 128) * (N // 128)
    launches, _ = _run(q, M, N, K, 0, (G + tiles - 1) * PART)
    assert launches == 0


def test_even_split_falls_back_on_ragged_shapes(q):
    """M not a multiple of 128 (K = 129 k-tiles is whole): not eligible"""
    launches, _ = _run(q, 1300, 512, 2064, 0, 1 << 24)
    assert launches == 0


def test_remainder_split_keeps_the_split_k_rule(q):
    """K % 16 != 0 on a product large enough (M N K >= 4e9) for the remainder split -- whole k-tiles on the fast kernel, the last K % 16
    rows accumulated behind them: whole 128 x 128 tiles, but the whole-k-tile part stays on the split-K rule, forced entry or not"""
    M, N, K = 3072, 256, 5128
    assert K % 16 == 8 and M * N * K >= 4e9
    launches, _ = _run(q, M, N, K, 0, 1 << 24)
    assert launches == 0
    launches, _ = _run(q, M, N, K, 0, 1 << 24, forced=False)
    assert launches == 0


def test_product_library_chooses_the_even_split_by_its_model(q, qr):
    """qrd_gemm_tn_update itself, product library, nothing forced: 1408 x 256 x 2048 on a CU-masked stream of 32 CUs (64 slots).  22 tiles:
    the split-K rule's best is 5 slices = 110 workgroups in two rounds (modelled 1066 K rows), the even split 64 workgroups of 44 k-tiles
    (881) -- the smallest shape with so wide a modelled margin (17 %), so the chooser must take the even split, on 64 workgroups"""
    assert not qr.LAB
    st = C.c_void_p()
    q.check(q.lib.qrd_stream_create_cumask(C.byref(st), 0, 32))
    try:
        launches, grid = _run(q, 1408, 256, 2048, 0, 1 << 24, stream=st, forced=False)
        assert launches == 2 and grid == 64
    finally:
        q.check(q.lib.qrd_stream_destroy(st))


_FACTOR_CHILD = r"""
import sys, json
sys.path.insert(0, %r); sys.path.insert(0, %r)
import numpy as np, torch
import cuda_qr_amd as qr
from gpu_util import zeros
m = n = 3072
p = qr.Plan(m, n, 256, 32)
dA = zeros(m, n)
p.fill_uniform(dA, m, m, n, seed=12)
p.sync()
dtau, dQ, dR = zeros(n, 1), zeros(m, n), zeros(n, n)
torch.cuda.synchronize()
n0 = qr.lib.qrd_tn_even_launches()
p.geqrf(dA, m, n, m, dtau)
p.sync()
launches = qr.lib.qrd_tn_even_launches() - n0
# ||A - QR||_F / ||A||_F and ||Q^T Q - I||_F on the device, as the square tests of test_gpu_qr.py compute them
p.extract_r(dA, m, n, m, dR, n, n)
p.applyq(dA, m, n, m, dtau, dQ, n, m, True)
dQR, dG = zeros(m, n), zeros(n, n)
p.gemm("N", m, n, n, 1.0, dQ, m, dR, n, 0.0, dQR, m)
p.gemm("T", n, n, m, 1.0, dQ, m, dQ, m, 0.0, dG, n)
p.sync()
d, a = p.diffnorm(dQR, m, m, n, seed=12)
o, _ = p.diffnorm(dG, n, n, n, mode=1)
print(json.dumps({"even_launches": launches, "resid": float(np.sqrt(d / a)), "orth": float(np.sqrt(o))}))
p.close()
"""


def test_factorisation_on_the_even_split(qr):
    """3072 x 3072 at nb 256 (the smallest look-ahead shape) through qr_geqrf_dev with the even split taken wherever it is eligible
    (MI355XQR_TN_EVEN=1, a measurement knob: lab library, child process): the path ran, residual and orthogonality within the bounds of
    the square tests of test_gpu_qr.py."""
    out = subprocess.run([sys.executable, "-c", _FACTOR_CHILD % (ROOT, os.path.join(ROOT, "tests"))], check=True, timeout=600, capture_output=True,
                         text=True, env=dict(os.environ, CUDA_QR_AMD_LIB="lab", MI355XQR_TN_EVEN="1"))
    rec = json.loads(out.stdout.strip().splitlines()[-1])
    print(rec)
    assert rec["even_launches"] > 0
    assert rec["resid"] < 1e-12 and rec["orth"] < 1e-11
