"""Batched covariance, standard error and leverage timing table (mi355x_qr.h section 8k): HIP events, the minimum of --reps runs after
--warmup warm-up runs, one process.

At m x n = 16 x 8, 64 x 31, 100 x 33 (batch 16384) and 256 x 63 (batch 4096), on standard normal members b = A x* + 0.01 noise with
prior weights in [0.25, 4], on the same GPU and the same A and b:
  all    one qr_gels_stats_batched_dev with every output (x, e, h, sigma2, dof, C, se; QR_COV_SCALED)
  x      the same call with dX alone
  wls    one qr_gels_weighted_batched_dev (x and the residual norm): what the fit alone costs, and the ratio all / wls
  torch  the composition callers use today: one qr_gels_batched_dev on a copy scaled by sqrt(p) (the copy is not timed), then
         torch.linalg.solve_triangular on the batch of R for T, a bmm for C = T T^T, and the row norms of A T for h; the ratio
         torch / all, and the worst ||C_torch - C|| / ||C|| (unscaled)
Then the from-factor calls on their own: qr_covar_batched_dev (C and se) at n = 8, 31, 33, 63 and qr_leverage_batched_dev at 256 rows,
on the triangles of the same batches.

Writes the table to --out (default profiles/r24_batched_stats_perf.txt) as well as to the terminal.  One process, one GPU; give each
invocation a time limit of its own (`timeout -k 10 600 python devtools/tools_batched_stats_perf.py`).
Usage: python devtools/tools_batched_stats_perf.py [--reps K] [--warmup W] [--quick] [--out FILE]
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import argparse  # noqa: E402

import torch  # noqa: E402

import cuda_qr_amd as q  # noqa: E402

_out = None


def say(line):
    print(line, flush=True)
    if _out:
        _out.write(line + "\n")
        _out.flush()


def event_ms(stream, fn, sync):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    fn()
    e1.record(stream)
    sync()
    return e0.elapsed_time(e1)


def best(stream, fn, before, sync, reps, warm):
    ts = []
    for k in range(warm + reps):
        before()
        torch.cuda.synchronize()
        t = event_ms(stream, fn, sync)
        if k >= warm:
            ts.append(t)
    return min(ts)


def row(m, n, batch, reps, warm):
    plan = q.Plan(m, n, 0, 0)
    ps = torch.cuda.ExternalStream(plan.stream)
    gen = torch.Generator(device="cuda").manual_seed(100000 * m + 1000 * n + 24)

    def rnd(*shape):
        return torch.randn(shape, dtype=torch.float64, device="cuda", generator=gen)

    A = rnd(batch, n, m)                                          # column-major members
    xs = rnd(batch, n)
    b = ((A.transpose(1, 2) @ xs[:, :, None])[:, :, 0] + 0.01 * rnd(batch, m)).contiguous()
    p = 0.25 + 3.75 * torch.rand((batch, m), dtype=torch.float64, device="cuda", generator=gen)
    f64 = dict(dtype=torch.float64, device="cuda")
    X, se = torch.empty((batch, n), **f64), torch.empty((batch, n), **f64)
    E, Hh = torch.empty((batch, m), **f64), torch.empty((batch, m), **f64)
    sig, res = torch.empty(batch, **f64), torch.empty(batch, **f64)
    Cv = torch.empty((batch, n, n), **f64)
    dof = torch.zeros(batch, dtype=torch.int32, device="cuda")
    info = torch.zeros(batch, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()

    def fused(scaled=q.QR_COV_SCALED):
        plan.gels_stats_batched(A, m, n, m, m * n, b, m, X, n, info, batch, scaled=scaled, dprior=p, strideprior=m, dE=E, strideE=m, dH=Hh,
                                strideH=m, dsigma2=sig, ddof=dof, dC=Cv, ldc=n, strideC=n * n, dse=se, stridese=n)

    def x_only():
        plan.gels_stats_batched(A, m, n, m, m * n, b, m, X, n, info, batch, dprior=p, strideprior=m)

    def wls():
        plan.gels_weighted_batched(A, m, n, m, m * n, b, m, p, m, X, n, info, batch, dresid=res)

    nothing = lambda: None                                        # noqa: E731
    t_all = best(ps, fused, nothing, plan.sync, reps, warm)
    flagged = int((info != 0).sum().item())
    t_x = best(ps, x_only, nothing, plan.sync, reps, warm)
    t_wls = best(ps, wls, nothing, plan.sync, reps, warm)

    # today's composition: gels on the scaled copy (factored in place: restored before every run, not timed), then torch
    sq = torch.sqrt(p)
    S, r = torch.empty_like(A), torch.empty_like(b)
    tau = torch.empty((batch, n), **f64)
    ginfo = torch.zeros(batch, dtype=torch.int32, device="cuda")
    Ct = torch.empty((batch, n, n), **f64)
    fits = bool(m <= q.lib.qr_batched_max_rows(n + 1))

    def restore():
        torch.mul(A, sq[:, None, :], out=S)
        torch.mul(b, sq, out=r)

    def composed():
        plan.gels_batched(S, m, n, m, m * n, tau, n, r, 1, m, m, ginfo, batch)
        with torch.cuda.stream(ps):
            R = torch.triu(S[:, :, :n].transpose(1, 2))          # (batch, n, n)
            eye = torch.eye(n, **f64).expand(batch, n, n)
            T = torch.linalg.solve_triangular(R, eye, upper=True)
            Ct.copy_(torch.bmm(T, T.transpose(1, 2)))
            Y = torch.bmm(A.transpose(1, 2), T)                   # rows of A T
            hh = p * (Y * Y).sum(dim=2)
            ee = b - (A.transpose(1, 2) @ r[:, :n, None])[:, :, 0]
            _ = (p * ee * ee).sum(dim=1) / (m - n)
            _ = hh.sum()

    t_torch = best(ps, composed, restore, plan.sync, reps, warm) if fits else float("nan")
    fused(q.QR_COV_UNSCALED)
    plan.sync()
    dc = ((Ct - Cv.transpose(1, 2)).flatten(1).norm(dim=1) / Cv.flatten(1).norm(dim=1)).max().item() if fits else float("nan")

    # the from-factor calls on the triangles of the same batch (geqrf factors in place: once, not timed)
    restore()
    plan.geqrf_batched(S, m, n, m, m * n, tau, n, batch)
    plan.sync()

    def covar():
        plan.covar_batched(S, n, m, m * n, info, batch, dC=Cv, ldc=n, strideC=n * n, dse=se, stridese=n)

    t_cov = best(ps, covar, nothing, plan.sync, reps, warm)
    rows = rnd(batch, n, 256)
    H2 = torch.empty((batch, 256), **f64)

    def lever():
        plan.leverage_batched(S, n, m, m * n, rows, 256, 256, 256 * n, H2, 256, info, batch)

    t_lev = best(ps, lever, nothing, plan.sync, reps, warm)
    plan.close()
    say(f"{m:>4} x {n:<3} {batch:>6} | {t_all:>8.3f} {t_x:>8.3f} | {t_wls:>8.3f} {t_all / t_wls:>6.2f} | {t_torch:>9.3f} {t_torch / t_all:>6.2f} {dc:>8.1e} | "
          f"{t_cov:>9.3f} {t_lev:>9.3f}{'' if not flagged else f'   ({flagged} info words)'}")


def main():
    global _out
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--quick", action="store_true", help="small batches only (a check that the tool runs)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r24_batched_stats_perf.txt"))
    a = ap.parse_args()
    _out = open(a.out, "w")
    say(f"device: {q.device_info()}")
    say(f"qr_gels_stats_batched_dev with every output (all) and with dX alone (x); ms by HIP events, minimum of {a.reps} after {a.warmup} warm-up runs")
    say("wls: qr_gels_weighted_batched_dev, all/wls; torch: qr_gels_batched_dev + solve_triangular + bmm + row norms, torch/all, worst "
        "||C_torch - C|| / ||C||; covar: qr_covar_batched_dev (C, se) on the same triangles; lev: qr_leverage_batched_dev, 256 rows")
    say(f"{'m x n':>10} {'batch':>6} | {'all ms':>8} {'x ms':>8} | {'wls ms':>8} {'ratio':>6} | {'torch ms':>9} {'ratio':>6} {'dC':>8} | {'covar ms':>9} {'lev ms':>9}")
    shapes = [(16, 8, 256), (100, 33, 128)] if a.quick else [(16, 8, 16384), (64, 31, 16384), (100, 33, 16384), (256, 63, 4096)]
    for m, n, batch in shapes:
        row(m, n, batch, a.reps, a.warmup)
    _out.close()


if __name__ == "__main__":
    main()
