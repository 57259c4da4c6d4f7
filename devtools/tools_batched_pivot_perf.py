"""Batched pivoted QR / rank-deficient least squares: what pivoting costs beside the unpivoted batched calls.

Writes profiles/r14_batched_pivot_perf.txt.  HIP events on the plan's stream (the library's own timing events), one warm-up call, the
minimum of 5 timed calls, everything in one process and on the same full-rank Gaussian batch:
  qr_geqp3_batched_dev beside qr_geqrf_batched_dev;
  qr_gelsy_batched_dev beside qr_gels_batched_dev (one right-hand side, the fused route where the shape allows it);
  one loop of 32 qr_gelsp_dev calls at 256 x 64, scaled to the batch, for scale.
No ratio is a pass condition: the file records what was measured.

    python devtools/tools_batched_pivot_perf.py
"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cuda_qr_amd as qr  # noqa: E402
from tools_batched_perf import REPS, Timer  # noqa: E402

SHAPES = [(16, 8, 16384), (64, 32, 16384), (100, 33, 16384), (256, 64, 4096)]


def main():
    lines = [f"batched pivoted QR on {qr.device_info()}: min of {REPS} after a warm-up, HIP events, full-rank Gaussian batches",
             f"{'shape':>9} {'batch':>6} {'geqrf ms':>9} {'geqp3 ms':>9} {'x geqrf':>8} {'gels ms':>9} {'gelsy ms':>9} {'x gels':>8}"]
    plan = qr.Plan(64, 8, 0, 0)
    timer = Timer(plan)
    g = torch.Generator(device="cuda").manual_seed(14)
    ratios = []
    for m, n, batch in SHAPES:
        A0 = torch.randn((batch, n, m), dtype=torch.float64, device="cuda", generator=g)          # packed column-major matrices
        B0 = torch.randn((batch, 1, m), dtype=torch.float64, device="cuda", generator=g)
        dA, dB, dtau = A0.clone(), B0.clone(), torch.zeros((batch, n), dtype=torch.float64, device="cuda")
        dj = torch.zeros((batch, n), dtype=torch.int32, device="cuda")
        dinfo, drank = torch.zeros(batch, dtype=torch.int32, device="cuda"), torch.zeros(batch, dtype=torch.int32, device="cuda")
        dres = torch.zeros(batch, dtype=torch.float64, device="cuda")

        def reset():
            dA.copy_(A0)
            dB.copy_(B0)

        t_qr = timer(reset, lambda: plan.geqrf_batched(dA, m, n, m, m * n, dtau, n, batch))
        t_qp = timer(reset, lambda: plan.geqp3_batched(dA, m, n, m, m * n, dj, n, dtau, n, batch))
        t_ls = timer(reset, lambda: plan.gels_batched(dA, m, n, m, m * n, dtau, n, dB, 1, m, m, dinfo, batch))
        t_ly = timer(reset, lambda: plan.gelsy_batched(dA, m, n, m, m * n, dj, n, dtau, n, dB, 1, m, m, batch, dresid=dres, drank=drank))
        assert int(drank.min()) == n and not int(dinfo.max())
        ratios.append((t_qp / t_qr, t_ly / t_ls))
        lines.append(f"{m:>5}x{n:<3} {batch:>6} {t_qr:>9.4f} {t_qp:>9.4f} {t_qp / t_qr:>8.2f} {t_ls:>9.4f} {t_ly:>9.4f} {t_ly / t_ls:>8.2f}")
        print(lines[-1], flush=True)
    # for scale: the one-matrix pivoted solve, once per matrix
    m, n, batch, k = 256, 64, 4096, 32
    p1 = qr.Plan(m, n, 0, 0)
    t1 = Timer(p1)
    A0 = torch.randn((k, n, m), dtype=torch.float64, device="cuda", generator=g)
    B0 = torch.randn((k, 1, m), dtype=torch.float64, device="cuda", generator=g)
    d1, b1, tau1 = A0.clone(), B0.clone(), torch.zeros((k, n), dtype=torch.float64, device="cuda")
    j1 = torch.zeros((k, n), dtype=torch.int32, device="cuda")

    def reset1():
        d1.copy_(A0)
        b1.copy_(B0)

    def loop():
        for q in range(k):
            p1.gelsp(d1[q], m, n, m, j1[q], tau1[q], b1[q], 1, m)

    loop_ms = t1(reset1, loop)
    p1.close()
    lines.append(f"a loop of {k} qr_gelsp_dev calls at {m}x{n}: {loop_ms:.2f} ms, {loop_ms / k:.3f} ms per matrix; scaled to {batch} matrices "
                 f"{loop_ms * batch / k:.0f} ms")
    print(lines[-1], flush=True)
    lines.append("pivoting adds, per column: a 6-step arg-max butterfly, the column swap (a select over the register file on the wave "
                 "route, a pass over two LDS columns and one more barrier on the workgroup route), one more barrier to publish the pivot, "
                 "and the norm downdate by wave 0 while the other waves wait; per matrix: one pass for the initial norms")
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "r14_batched_pivot_perf.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")
    plan.close()


if __name__ == "__main__":
    main()
