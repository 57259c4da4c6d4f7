"""Batched SVD of small matrices (header section 8c): what one call costs, and beside what.

Writes profiles/r15_batched_svd_perf.txt.  HIP events on the plan's stream (the library's own timing events), one warm-up call, the
minimum of 5 timed calls, everything in one process and on the same Gaussian batch:
  qr_gesvd_batched_dev, values only and with U and V, beside qr_geqp3_batched_dev alone (its first launch);
  torch.linalg.svdvals and torch.linalg.svd (full_matrices=False) on the same batch (torch events on torch's stream).  Where the first
  torch call on 256 of the matrices says the whole batch would take more than TORCH_BUDGET_S per call, torch is timed on those 256 and
  scaled to the batch; the line says which;
  a loop of qr_gesvd_dev (section 7: one matrix per call) over LOOP of the matrices, scaled to the batch.
No ratio is a pass condition: the file records what was measured.

    python devtools/tools_batched_svd_perf.py
"""
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cuda_qr_amd as qr  # noqa: E402
from tools_batched_perf import REPS, Timer  # noqa: E402

SHAPES = [(16, 8, 16384), (64, 32, 16384), (100, 33, 16384), (256, 64, 4096)]
LOOP = 4
TORCH_SUB = 256
TORCH_BUDGET_S = 2.0


def torch_ms(fn, A):
    best = float("inf")
    for r in range(-1, REPS):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn(A)
        e1.record()
        e1.synchronize()
        if r >= 0:
            best = min(best, e0.elapsed_time(e1))
    return best


def torch_scaled(fn, A):
    """(ms for the whole batch, the matrices it was measured on)"""
    batch = A.shape[0]
    sub = A[:TORCH_SUB].contiguous()
    fn(sub)                                                      # (loads the solver library)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn(sub)
    torch.cuda.synchronize()
    if (time.perf_counter() - t0) * batch / TORCH_SUB > TORCH_BUDGET_S:
        return torch_ms(fn, sub) * batch / TORCH_SUB, TORCH_SUB
    return torch_ms(fn, A), batch


def main():
    lines = [f"batched SVD on {qr.device_info()}: min of {REPS} after a warm-up, HIP events, Gaussian batches",
             f"{'shape':>9} {'batch':>6} {'geqp3 ms':>9} {'values ms':>10} {'x geqp3':>8} {'U,S,V ms':>9} {'x geqp3':>8} {'sweeps':>6} "
             f"{'torch svdvals ms':>17} {'torch svd ms':>13} {'(on)':>6} {'svdvals / ours':>14} {'svd / ours':>10} {'gesvd_dev loop ms':>18}"]
    plan = qr.Plan(64, 8, 0, 0)
    timer = Timer(plan)
    g = torch.Generator(device="cuda").manual_seed(15)
    for m, n, batch in SHAPES:
        A0 = torch.randn((batch, n, m), dtype=torch.float64, device="cuda", generator=g)          # packed column-major matrices
        dA, dtau = A0.clone(), torch.zeros((batch, n), dtype=torch.float64, device="cuda")
        dj = torch.zeros((batch, n), dtype=torch.int32, device="cuda")
        dS = torch.zeros((batch, n), dtype=torch.float64, device="cuda")
        dU, dV = torch.zeros((batch, n, m), dtype=torch.float64, device="cuda"), torch.zeros((batch, n, n), dtype=torch.float64, device="cuda")
        dinfo, dsw = torch.zeros(batch, dtype=torch.int32, device="cuda"), torch.zeros(batch, dtype=torch.int32, device="cuda")

        def reset():
            dA.copy_(A0)

        t_qp = timer(reset, lambda: plan.geqp3_batched(dA, m, n, m, m * n, dj, n, dtau, n, batch))
        t_s = timer(reset, lambda: plan.gesvd_batched("N", "N", dA, m, n, m, m * n, dj, n, dtau, n, dS, n, dinfo, batch, dsweeps=dsw))
        t_usv = timer(reset, lambda: plan.gesvd_batched("U", "V", dA, m, n, m, m * n, dj, n, dtau, n, dS, n, dinfo, batch, dU=dU, ldu=m,
                                                        strideU=m * n, dV=dV, ldv=n, strideV=n * n, dsweeps=dsw))
        assert not int(dinfo.max())
        sweeps = int(dsw.max())
        At = A0.transpose(1, 2)                                  # (batch, m, n) views of the same matrices
        ref = torch.linalg.svdvals(At[:8])
        assert float((dS[:8] - ref).abs().max()) <= 1e-12 * float(ref.max())
        t_tv, on = torch_scaled(torch.linalg.svdvals, At)
        t_ts, _ = torch_scaled(lambda X: torch.linalg.svd(X, full_matrices=False), At)
        # section 7, one matrix per call
        p1 = qr.Plan(m, n, 0, 0)
        t1 = Timer(p1)
        d1, tau1, s1 = A0[:LOOP].clone(), torch.zeros((LOOP, n), dtype=torch.float64, device="cuda"), torch.zeros((LOOP, n), dtype=torch.float64, device="cuda")
        u1, v1 = torch.zeros((LOOP, n, m), dtype=torch.float64, device="cuda"), torch.zeros((LOOP, n, n), dtype=torch.float64, device="cuda")

        def loop():
            for q in range(LOOP):
                p1.gesvd("U", "V", d1[q], m, n, m, tau1[q], s1[q], u1[q], m, v1[q], n)

        try:
            t_loop = f"{t1(lambda: d1.copy_(A0[:LOOP]), loop) * batch / LOOP:.0f}"
        except qr.QRError as e:                                  # (a shape section 7 does not take)
            t_loop = f"n/a ({e.status})"
        p1.close()
        lines.append(f"{m:>5}x{n:<3} {batch:>6} {t_qp:>9.4f} {t_s:>10.4f} {t_s / t_qp:>8.2f} {t_usv:>9.4f} {t_usv / t_qp:>8.2f} {sweeps:>6} "
                     f"{t_tv:>17.2f} {t_ts:>13.2f} {on:>6} {t_tv / t_s:>14.1f} {t_ts / t_usv:>10.1f} {t_loop:>18}")
        print(lines[-1], flush=True)
    lines.append(f"(on): the matrices torch was timed on; fewer than the batch means scaled to it.  gesvd_dev loop: {LOOP} calls of "
                 "qr_gesvd_dev with U and V, scaled to the batch")
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "r15_batched_svd_perf.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")
    plan.close()


if __name__ == "__main__":
    main()
