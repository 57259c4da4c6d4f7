"""Batched robust least squares timing table (mi355x_qr.h section 8j): HIP events, the minimum of --reps runs after --warmup warm-up runs,
one process.

One qr_irls_batched_dev (the reweighting loop of every member in one launch; x, w, scale, resid, iter and status written) at m x n =
  16 x 8, 64 x 31, 100 x 33 (batch 16384) and 256 x 63 (batch 4096)
on planted members with 20 % outliers: standard normal A and x*, b = A x* + 0.01 noise, a fifth of the rows shifted by +-[0.1, 0.5]; the
Huber loss with its defaults (k = 1.345, the MAD scale, tol 1e-8, at most 50 solves).  Beside it, in the same run, on the same GPU and the
same A and b:
  gels   one qr_gels_batched_dev (one factorisation and one solve of the member: what ONE solve costs), and the ratio call / (mean solve
         count x gels): 1 would mean that the launch costs what its solves cost; the slowest member of a workgroup, the refills from A, the
         residual, median and weight passes push it up
  host   the loop this call replaces, on the same stream: per round a copy of the batch scaled by sqrt(w), one qr_gels_batched_dev, the
         residuals, torch.median (the lower median) and the Huber weights as torch elementwise kernels, and one host wait for the
         convergence flag; the batch runs until its slowest member has converged.  Its losses: the rounds, the worst ||x_host - x|| / ||x||

Writes the table to --out (default profiles/r23_batched_irls_perf.txt) as well as to the terminal.  One process, one GPU; give each
invocation a time limit of its own (`timeout -k 10 600 python devtools/tools_batched_irls_perf.py`).
Usage: python devtools/tools_batched_irls_perf.py [--reps K] [--warmup W] [--quick] [--out FILE]
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import argparse  # noqa: E402

import torch  # noqa: E402

import cuda_qr_amd as q  # noqa: E402

_out = None
K_HUBER, MAD, TOL, MAXIT = 1.345, 0.6744897501960817, 1e-8, 50


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


def planted(m, n, batch, gen):
    """A (batch, n, m) column-major members, b (batch, m) with a fifth of the rows shifted, and x* (batch, n)"""
    def rnd(*shape):
        return torch.randn(shape, dtype=torch.float64, device="cuda", generator=gen)

    def uni(*shape):
        return torch.rand(shape, dtype=torch.float64, device="cuda", generator=gen)

    A = rnd(batch, n, m)
    xs = rnd(batch, n)
    b = (A.transpose(1, 2) @ xs[:, :, None])[:, :, 0] + 0.01 * rnd(batch, m)
    k = m // 5
    rows = torch.argsort(uni(batch, m), dim=1)[:, :k]
    shift = (0.1 + 0.4 * uni(batch, k)) * torch.where(uni(batch, k) < 0.5, -1.0, 1.0)
    b.scatter_add_(1, rows, shift)
    return A, b.contiguous(), xs


def row(m, n, batch, reps, warm):
    plan = q.Plan(m, n, 0, 0)
    ps = torch.cuda.ExternalStream(plan.stream)
    gen = torch.Generator(device="cuda").manual_seed(100000 * m + 1000 * n + 23)
    A, b, xs = planted(m, n, batch, gen)
    X = torch.empty((batch, n), dtype=torch.float64, device="cuda")
    W = torch.empty((batch, m), dtype=torch.float64, device="cuda")
    sc = torch.empty(batch, dtype=torch.float64, device="cuda")
    res = torch.empty(batch, dtype=torch.float64, device="cuda")
    it = torch.zeros(batch, dtype=torch.int32, device="cuda")
    st = torch.zeros(batch, dtype=torch.int32, device="cuda")
    info = torch.zeros(batch, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()

    def irls():
        plan.irls_batched(q.QR_LOSS_HUBER, A, m, n, m, m * n, b, m, X, n, info, batch, tol=TOL, dW=W, strideW=m, dscale=sc, dresid=res, diter=it,
                          dstatus=st)

    t_ir = best(ps, irls, lambda: None, plan.sync, reps, warm)
    flagged = int((info != 0).sum().item())
    capped = int((st == 3).sum().item())
    mean_it, max_it = it.to(torch.float64).mean().item(), int(it.max().item())

    # one gels on the same members: factored in place, so A and b are restored before every run (not timed)
    S, r = A.clone(), b.clone()
    tau = torch.empty((batch, n), dtype=torch.float64, device="cuda")
    ginfo = torch.zeros(batch, dtype=torch.int32, device="cuda")

    def restore():
        S.copy_(A)
        r.copy_(b)

    def gels():
        plan.gels_batched(S, m, n, m, m * n, tau, n, r, 1, m, m, ginfo, batch)

    t_gels = best(ps, gels, restore, plan.sync, reps, warm)

    # the host loop this call replaces, on the plan's stream
    Ar = A.transpose(1, 2)                                    # (batch, m, n) view
    Xh = torch.zeros((batch, n), dtype=torch.float64, device="cuda")
    rounds = [0]

    def host_loop():
        with torch.cuda.stream(ps):
            w = torch.ones((batch, m), dtype=torch.float64, device="cuda")
            xold = None
            for k in range(MAXIT):
                sq = torch.sqrt(w)
                torch.mul(A, sq[:, None, :], out=S)           # the scaled copy
                torch.mul(b, sq, out=r)
                plan.gels_batched(S, m, n, m, m * n, tau, n, r, 1, m, m, ginfo, batch)
                x = r[:, :n].clone()
                rr = b - (Ar @ x[:, :, None])[:, :, 0]
                s = torch.median(rr.abs(), dim=1).values / MAD
                u = rr.abs() / s[:, None]
                w = torch.where(u <= K_HUBER, torch.ones_like(u), K_HUBER / u)
                rounds[0] = k + 1
                if xold is not None:
                    done = ((x - xold).abs().amax(dim=1) <= TOL * x.abs().amax(dim=1)).all()
                    if bool(done.item()):                     # the host wait
                        break
                xold = x
            Xh.copy_(x)

    t_host = best(ps, host_loop, lambda: None, plan.sync, max(1, reps // 2), 1)
    dx = ((Xh - X).norm(dim=1) / X.norm(dim=1)).max().item()
    err = ((X - xs).norm(dim=1) / xs.norm(dim=1)).max().item()
    plan.close()
    say(f"{m:>4} x {n:<3} {batch:>6} | {t_ir:>9.3f} | {mean_it:>8.2f} {max_it:>5} | {t_gels:>9.3f} | {t_ir / (mean_it * t_gels):>7.2f} | "
        f"{t_host:>9.3f} {rounds[0]:>6} {dx:>9.1e} | worst ||x - x*|| / ||x*|| {err:.1e}"
        f"{'' if not capped else f'   ({capped} members at 50 solves)'}{'' if not flagged else f'   ({flagged} info words)'}")


def main():
    global _out
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--quick", action="store_true", help="small batches only (a check that the tool runs)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r23_batched_irls_perf.txt"))
    a = ap.parse_args()
    _out = open(a.out, "w")
    say(f"device: {q.device_info()}")
    say(f"one qr_irls_batched_dev (Huber, defaults; x, w, scale, resid, iter, status) on planted members with 20 % outliers; ms by HIP events, "
        f"minimum of {a.reps} after {a.warmup} warm-up runs")
    say("gels: one qr_gels_batched_dev on the same A and b; ratio = irls ms / (mean solves x gels ms); host: the loop it replaces (scaled copy, "
        "gels, torch weights and median, a host wait per round), its rounds and the worst ||x_host - x|| / ||x||")
    say(f"{'m x n':>10} {'batch':>6} | {'irls ms':>9} | {'mean it':>8} {'max':>5} | {'gels ms':>9} | {'ratio':>7} | {'host ms':>9} {'rounds':>6} {'dx':>9} |")
    shapes = [(16, 8, 256), (100, 33, 128)] if a.quick else [(16, 8, 16384), (64, 31, 16384), (100, 33, 16384), (256, 63, 4096)]
    for m, n, batch in shapes:
        row(m, n, batch, a.reps, a.warmup)
    _out.close()


if __name__ == "__main__":
    main()
