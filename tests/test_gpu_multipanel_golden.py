"""-m gpu: the FAST path pinned to the reference (missing #1).

The small golden fixtures (n <= 128 = default nb, m <= 512) only ever reach ONE outer panel through the one-workgroup
Householder leaf.  These cases are outputs of the real reference qr.c (oracle/make_golden.py: 1184 x 640 in 5 s, 2024 x 2024 in
161 s, PR = 64 / PC = 8, srand(12) input) factored with 5 / 10 / 16 outer panels, so the CholeskyQR2 + Householder-reconstruction
leaf, the split-K products, the MFMA trailing update, the look-ahead schedule and (2024^2, in a child process with the partition
forced on) the CU-masked streams and the load-balancing share of the panel stream are all compared with reference-made R:
    ||S R_hip - S' R_ref||_F / ||R_ref||_F <= 1e-13     (S = sign(diag R)).
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import load_golden
from gpu_util import dev, host, rel, zeros

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _golden_R(g, n):
    R = np.zeros((n, n))
    R[np.triu_indices(n)] = g["Rn_triu"]
    return R


@pytest.mark.parametrize("la", [None, "1"])          # default for this shape: single-stream schedule; "1": look-ahead on two streams
@pytest.mark.parametrize("nb", [128, 64, 256, 32, 512])
def test_1184x640_blocked_path_vs_reference_R(qr, oracle, nb, la, monkeypatch):
    if la is not None:
        monkeypatch.setenv("MI355XQR_LOOKAHEAD", la)    # read at plan creation
    m, n = 1184, 640
    g = load_golden("ref_1184x640_f64_64x8")
    A = oracle.fill_rand(m, n)
    assert abs(np.linalg.norm(A) - float(g["normA"])) < 1e-9
    p = qr.Plan(m, n, nb, 32)
    dA, dtau, dQ, dR = dev(A), zeros(n, 1), zeros(m, n), zeros(n, n)
    p.geqrf(dA, m, n, m, dtau)
    p.extract_r(dA, m, n, m, dR, n, n)
    p.applyq(dA, m, n, m, dtau, dQ, n, m, True)
    p.sync()
    R, Q = host(dR), host(dQ)
    assert rel(oracle.sign_normalise(R), _golden_R(g, n)) <= 1e-13
    assert np.abs(np.abs(np.diag(R)) - np.abs(g["diagR"])).max() < 1e-12 * np.abs(g["diagR"]).max()
    assert np.linalg.norm(A - Q @ R) / np.linalg.norm(A) < 1e-14 * 4
    assert np.linalg.norm(Q.T @ Q - np.eye(n)) < 1e-12
    p.close()


def test_1184x640_dropin_mmqr_vs_reference_R(qr, oracle):
    """The same through the drop-in host-pointer symbol the reference's caller links (default nb = 128: 5 outer panels)."""
    m, n = 1184, 640
    g = load_golden("ref_1184x640_f64_64x8")
    F, tau = qr.mmqr(oracle.fill_rand(m, n))
    assert rel(oracle.sign_normalise(F), _golden_R(g, n)) <= 1e-13


_PUBLIC_KNOBS = {"MI355XQR_" + k for k in ("NB", "IB", "PANEL", "GUARD", "LOOKAHEAD", "SPLIT", "CQR_MIN_ROWS", "FUSED_MIN_ROWS", "TSQR_PIPE",
                                            "TSQR_RESERVE_CUS", "PLAN_CACHE", "ROCTX")}

_CHILD = r"""
import sys, json, numpy as np, torch
sys.path.insert(0, %r)
import cuda_qr_amd as q
from oracle import oracle as O          # the checker: input generator + sign normalisation only
m = n = 2024
A = O.fill_rand(m, n)
p = q.Plan(m, n, int(sys.argv[2]), 32)
dA = torch.from_numpy(np.ascontiguousarray(A.T)).cuda(); dtau = torch.zeros(n, dtype=torch.float64, device='cuda')
torch.cuda.synchronize()
p.geqrf(dA, m, n, m, dtau); p.sync()
F = np.asfortranarray(dA.cpu().numpy().T)
np.save(sys.argv[1], O.sign_normalise(F))
"""


@pytest.mark.parametrize("nb,env", [
    (128, {}),                                                                        # default schedule (this shape: single stream)
    (128, {"MI355XQR_LOOKAHEAD": "1"}),                                               # look-ahead on two streams, shared CUs
    (128, {"MI355XQR_LOOKAHEAD": "1", "MI355XQR_SPLIT": "64", "MI355XQR_BALANCE": "14,44,0,0"}),   # CU-masked streams + panel-stream share
    (256, {"MI355XQR_LOOKAHEAD": "1", "MI355XQR_SPLIT": "32", "MI355XQR_BALANCE": "14,44,0,0"}),
    (128, {"MI355XQR_LOOKAHEAD": "1", "MI355XQR_SPLIT": "64", "MI355XQR_BALANCE": "14,44,0,0", "MI355XQR_EARLY_NEXT": "0"}),   # look-ahead update never issued early
    (128, {"MI355XQR_LOOKAHEAD": "1", "MI355XQR_SPLIT": "64", "MI355XQR_BALANCE": "14,44,0.05,0.05"}),     # early look-ahead update on some steps only
    (128, {"MI355XQR_PANEL": "tsqr"}),                                                # Householder-TSQR leaf only
    (64, {"MI355XQR_LOOKAHEAD": "0"}),                                                # single-stream schedule
    (512, {}),                                                                        # two-level panels (K = 512 wide update)
    (512, {"MI355XQR_LOOKAHEAD": "1"}),                                               # ... with look-ahead (W_a / W_b pieces, ev_half)
    (512, {"MI355XQR_LOOKAHEAD": "1", "MI355XQR_SPLIT": "64", "MI355XQR_BALANCE": "14,44,0,0", "MI355XQR_NEXT": "update"}),
    (512, {"MI355XQR_LOOKAHEAD": "0"}),
    (128, {"MI355XQR_EP": "0"}),                                                      # in-panel product as a launch of its own (no early product)
    (256, {"MI355XQR_FUSED_MIN_ROWS": "0"}),                                          # round 4: every outer panel in ONE launch (qr_panel_fused.hip)
    (128, {"MI355XQR_FUSED_MIN_ROWS": "0", "MI355XQR_LOOKAHEAD": "0"}),     # ... single-stream schedule
    (64, {"MI355XQR_FUSED_MIN_ROWS": "0", "MI355XQR_LOOKAHEAD": "1", "MI355XQR_SPLIT": "64", "MI355XQR_BALANCE": "14,44,0,0"}),   # ... on a 64-CU panel stream
    (512, {"MI355XQR_FUSED_MIN_ROWS": "0", "MI355XQR_LOOKAHEAD": "0"}),               # ... two-level panels: each half one launch
    (256, {"MI355XQR_LOOKAHEAD": "1", "MI355XQR_SPLIT": "64:0.5,U", "MI355XQR_BALANCE": "14,44,0,0"}),   # late phase: panel chain on an unmasked stream
    (256, {"MI355XQR_LOOKAHEAD": "1", "MI355XQR_SPLIT": "32", "MI355XQR_BALANCE": "14,44,0,0", "MI355XQR_TN_WIDE": "1"}),   # wide-tile TN product
    (256, {"MI355XQR_LOOKAHEAD": "1", "MI355XQR_SPLIT": "32", "MI355XQR_BALANCE": "14,44,0,0", "MI355XQR_KPIPE": "0", "MI355XQR_NT_IL": "0"}),   # plain K loops (round-2 issue order) in the update's two GEMMs
    # schedule variants the stream-order check drives over the stub (tests/test_schedule_order.py; `host_order factor 2024 2024 nb` under the
    # same environment shows the branch taken): at nb 128 on a 32-CU panel stream one panel per factorisation leaves its Gram matrix and T
    # merge to the update stream ...
    (128, {"MI355XQR_LOOKAHEAD": "1", "MI355XQR_SPLIT": "32", "MI355XQR_BALANCE": "14,44,0,0", "MI355XQR_DEFER_T": "0"}),   # ... not here: merged on the panel stream
    (128, {"MI355XQR_LOOKAHEAD": "1", "MI355XQR_SPLIT": "32", "MI355XQR_BALANCE": "14,44,0,0", "MI355XQR_TRSM": "0"}),      # ... merge tree first, then N(s) with the merged T
    (128, {"MI355XQR_LOOKAHEAD": "1", "MI355XQR_SPLIT": "32", "MI355XQR_BALANCE": "14,44,0,0", "MI355XQR_SPLIT_T": "0"}),   # N(s) on the update stream waits for the whole panel (no ev_v)
    (256, {"MI355XQR_LOOKAHEAD": "1", "MI355XQR_SPLIT": "64:0.5,32"}),                                                        # two masked phases: both streams hop, the model follows the phase
    (256, {"MI355XQR_LOOKAHEAD": "1", "MI355XQR_SPLIT": "64", "MI355XQR_NEXT": "panel"}),                                     # N(s) on the panel stream of a partition
])
def test_2024_square_vs_reference_R_slices(qr, oracle, tmp_path, nb, env):
    """16 (nb = 128) / 8 / 32 outer panels: wide update, look-ahead, CU partition, balance_cols -- against slices of the
    reference's sign-normalised R (the whole 2024^2 triangle is 16 MB; the fixture keeps the first 32 rows, the last 64
    columns, the diagonal, the row norms and the Frobenius norm)."""
    g = load_golden("ref_2024x2024_f64_64x8")
    out = str(tmp_path / "rn.npy")
    # the twelve public knobs work in the product library; a case that forces a schedule branch with a measurement knob (the balance
    # model, the look-ahead update's stream, settled kernel A/Bs) runs on the lab build of the same sources
    if set(env) - _PUBLIC_KNOBS:
        env = dict(env, CUDA_QR_AMD_LIB="lab")
    subprocess.run([sys.executable, "-c", _CHILD % ROOT, out, str(nb)], check=True, env=dict(os.environ, **env))
    Rn = np.load(out)
    n = 2024
    assert rel(Rn[:32], g["Rn_rows_head"]) <= 1e-13
    assert rel(Rn[:, -64:], g["Rn_cols_tail"]) <= 1e-13
    assert np.abs(np.diag(Rn) - g["Rn_diag"]).max() <= 1e-13 * g["Rn_diag"].max() * 10
    assert np.abs(np.linalg.norm(Rn, axis=1) - g["Rn_rownorm"]).max() <= 1e-12 * g["Rn_rownorm"].max()
    assert abs(np.linalg.norm(Rn) - float(g["Rn_fro"])) <= 1e-12 * float(g["Rn_fro"])


@pytest.mark.parametrize("cond", [1e2, 1e3, 1e4, 1e5, 1e6, 1e7, 1e8, 1e9, 1e10, 1e11])
@pytest.mark.parametrize("mk,w", [(2048, 32), (20000, 32), (4096, 128)])
def test_cholqr2_guard_threshold_sweep(qr, oracle, cond, mk, w):
    """Leaves whose condition number walks through the region where the CholeskyQR2 route either barely passes its device-side
    guard (max|Q^T Q - I| <= 1/64 after the first pass) or barely fails it and hands the leaf to the Householder TSQR: whichever
    route fires, the result must be Householder-grade (backward error and orthogonality at round-off, R equal to LAPACK's).
    cond = 1e2 .. 1e7 is where CholeskyQR2 loses digits if the guard were too lax (error ~ cond^2 eps of the FIRST pass); 1e9 and
    1e11 sit on either side of the first-pass pivot test.  w = 128: four leaves in one panel, so the in-panel product that runs on Q
    beside the reconstruction (early product) and its redo on the guard route are inside the sweep as well."""
    rng = np.random.default_rng(int(np.log10(cond)) * 7 + mk)
    U, _ = np.linalg.qr(rng.standard_normal((mk, w)))
    V, _ = np.linalg.qr(rng.standard_normal((w, w)))
    A = (U * np.logspace(0, -np.log10(cond), w)) @ V.T
    p = qr.Plan(mk, w, 128 if w > 32 else 32, 32)
    dA, dtau, dQ, dR = dev(A), zeros(w, 1), zeros(mk, w), zeros(w, w)
    p.geqrf(dA, mk, w, mk, dtau)
    p.extract_r(dA, mk, w, mk, dR, w, w)
    p.applyq(dA, mk, w, mk, dtau, dQ, w, mk, True)
    p.sync()
    R, Q = host(dR), host(dQ)
    assert np.isfinite(R).all() and np.isfinite(Q).all()
    assert np.linalg.norm(A - Q @ R) / np.linalg.norm(A) < 2e-15 * np.sqrt(w) * 4
    assert np.linalg.norm(Q.T @ Q - np.eye(w)) < 5e-14 * np.sqrt(w)
    # R against LAPACK, row-wise relative to the row's own scale times cond-independent round-off: |dR| <= c eps |R| column-wise
    Rl = oracle.sign_normalise(np.linalg.qr(A, mode="r"))
    Rn = oracle.sign_normalise(R)
    assert np.linalg.norm(Rn - Rl) / np.linalg.norm(Rl) < 1e-12
    p.close()
