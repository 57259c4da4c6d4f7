"""-m gpu: a one-rank qr_tsqr_factor_dev writes R straight into the caller's array (no pass through the send buffer, no n x n copy), and the
local / exchange_buffers / stacked steps of the same plan still go through the send buffer."""
import numpy as np
import pytest
import torch

from gpu_util import dev, host

pytestmark = pytest.mark.gpu

SHAPES = [(512, 96), (4096, 256)]


def _nan(n):
    t = torch.full((n, n), float("nan"), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    return t


def _is_r_of(R, F):
    """R is bitwise the upper triangle of the factored array F, exact zeros below"""
    n = R.shape[0]
    assert np.array_equal(np.triu(R), np.triu(F[:n]))
    assert not np.tril(R, -1).any()
    assert not np.isnan(R).any()


@pytest.mark.parametrize("m,n", SHAPES)
def test_one_rank_factor_writes_r_to_the_caller(qr, m, n):
    tp = qr.TsqrPlan(m, n)
    dA, dR = dev(qr.uniform_matrix_host(m, n, seed=5)), _nan(n)
    tp.factor(dA, m, dR)
    tp.sync()
    _is_r_of(host(dR), host(dA))
    tp.close()


@pytest.mark.parametrize("m,n", SHAPES)
def test_back_to_back_factorisations_keep_their_own_r(qr, m, n):
    tp = qr.TsqrPlan(m, n)
    dA = [dev(qr.uniform_matrix_host(m, n, seed=s)) for s in (21, 22)]
    dR = [_nan(n), _nan(n)]
    tp.factor(dA[0], m, dR[0])          # no sync in between: stream order alone keeps the two apart
    tp.factor(dA[1], m, dR[1])
    tp.sync()
    R = [host(r) for r in dR]
    for k in range(2):
        _is_r_of(R[k], host(dA[k]))
    assert not np.array_equal(R[0], R[1])
    tp.close()


@pytest.mark.parametrize("m,n", SHAPES)
def test_local_factor_still_fills_the_send_buffer(qr, m, n):
    from cuda_qr_amd import tsqr as T
    tp = qr.TsqrPlan(m, n)
    send, _ = tp.exchange_buffers()
    sv = T._device_view(send, n * n, "cuda")
    dA, dR = dev(qr.uniform_matrix_host(m, n, seed=5)), _nan(n)
    tp.factor(dA, m, dR)                # (a one-rank factor does not refresh the send buffer; the steps below must)
    dB = dev(qr.uniform_matrix_host(m, n, seed=6))
    tp.local_factor(dB, m)
    tp.sync()
    F = host(dB)
    _is_r_of(sv.cpu().numpy().reshape(n, n).T, F)
    dR2 = _nan(n)
    tp.stacked_factor(dR2)
    tp.sync()
    _is_r_of(host(dR2), F)
    tp.close()
