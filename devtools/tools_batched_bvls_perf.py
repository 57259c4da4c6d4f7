"""Batched bound-constrained least squares timing table (mi355x_qr.h section 8i): HIP events, the minimum of --reps runs after --warmup
warm-up runs, one process.

One qr_bvls_batched_dev (the active-set loop of every member in one launch; x, w, state, resid and iter written) at m x n =
  16 x 8, 64 x 31, 100 x 33 (batch 16384) and 256 x 63 (batch 4096)
on planted members with about half the variables active: standard normal A, lo in -[0.5, 1.5], hi in +[0.5, 1.5], a random residual made
orthogonal to the free columns, every active variable at lo where a_j^T r < 0 and at hi where it is > 0, x* in [-0.4, 0.4] on the free
ones, b = A x* + r.  Beside it, in the same run, on the same GPU and the same A and b, one qr_gels_batched_dev (one factorisation and one
solve of the whole m x n member: what ONE elimination costs at most).  Columns: the call, the mean and the largest elimination count per
member, the gels call, and the call over (mean eliminations x gels): 1 would mean that the launch costs what its eliminations cost at
full width; the slowest member of a workgroup, the refills from A, the serial solves and the w passes push it up, the free set being
narrower than n pulls it down.

Writes the table to --out (default profiles/r22_batched_bvls_perf.txt) as well as to the terminal.  One process, one GPU; give each
invocation a time limit of its own (`timeout -k 10 600 python devtools/tools_batched_bvls_perf.py`).
Usage: python devtools/tools_batched_bvls_perf.py [--reps K] [--warmup W] [--quick] [--out FILE]
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


def planted(m, n, batch, gen):
    """A (batch, n, m) column-major members, b (batch, m), lo, hi (batch, n) and the planted state (batch, n)"""
    def rnd(*shape):
        return torch.randn(shape, dtype=torch.float64, device="cuda", generator=gen)

    def uni(*shape):
        return torch.rand(shape, dtype=torch.float64, device="cuda", generator=gen)

    A = rnd(batch, n, m)
    Ar = A.transpose(1, 2)                                    # (batch, m, n)
    lo, hi = -0.5 - uni(batch, n), 0.5 + uni(batch, n)
    active = uni(batch, n) < 0.5
    Af = Ar * (~active)[:, None, :]                           # the free columns, zeros elsewhere
    G = Af.transpose(1, 2) @ Af + torch.diag_embed(active.to(torch.float64))
    r = rnd(batch, m, 1)
    for _ in range(2):                                        # r orthogonal to the free columns (twice: the Gram matrix squares kappa)
        r = r - Af @ torch.linalg.solve(G, Af.transpose(1, 2) @ r)
    g = (Ar.transpose(1, 2) @ r)[:, :, 0]
    state = torch.where(active, torch.where(g < 0, -1, 1), 0).to(torch.int32)
    xs = torch.where(active, torch.where(g < 0, lo, hi), 0.8 * (uni(batch, n) - 0.5))
    b = (Ar @ xs[:, :, None] + r)[:, :, 0].contiguous()
    return A, b, lo.contiguous(), hi.contiguous(), state


def row(m, n, batch, reps, warm):
    plan = q.Plan(m, n, 0, 0)
    ps = torch.cuda.ExternalStream(plan.stream)
    gen = torch.Generator(device="cuda").manual_seed(100000 * m + 1000 * n + 22)
    A, b, lo, hi, state = planted(m, n, batch, gen)
    X = torch.empty((batch, n), dtype=torch.float64, device="cuda")
    W = torch.empty((batch, n), dtype=torch.float64, device="cuda")
    res = torch.empty(batch, dtype=torch.float64, device="cuda")
    st = torch.zeros((batch, n), dtype=torch.int32, device="cuda")
    it = torch.zeros(batch, dtype=torch.int32, device="cuda")
    info = torch.zeros(batch, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()

    def bvls():
        plan.bvls_batched(A, m, n, m, m * n, b, m, X, n, info, batch, dlo=lo, dhi=hi, stridebnd=n, dW=W, strideW=n, dstate=st, stridestate=n,
                          dresid=res, diter=it)

    t_bv = best(ps, bvls, lambda: None, plan.sync, reps, warm)
    flagged = int((info != 0).sum().item())
    wrong = int((st != state).any(dim=1).sum().item())
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
    plan.close()
    say(f"{m:>4} x {n:<3} {batch:>6} | {t_bv:>9.3f} | {mean_it:>8.2f} {max_it:>5} | {t_gels:>9.3f} | {t_bv / (mean_it * t_gels):>7.2f}"
        f"   members off the planted state: {wrong}{'' if not flagged else f'   ({flagged} info words)'}")


def main():
    global _out
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--quick", action="store_true", help="small batches only (a check that the tool runs)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r22_batched_bvls_perf.txt"))
    a = ap.parse_args()
    _out = open(a.out, "w")
    say(f"device: {q.device_info()}")
    say(f"one qr_bvls_batched_dev (x, w, state, resid, iter) on planted members, about half the variables active; ms by HIP events, minimum of "
        f"{a.reps} after {a.warmup} warm-up runs")
    say("gels: one qr_gels_batched_dev on the same A and b (a full-width factorisation and solve); ratio = bvls ms / (mean eliminations x gels ms)")
    say(f"{'m x n':>10} {'batch':>6} | {'bvls ms':>9} | {'mean it':>8} {'max':>5} | {'gels ms':>9} | {'ratio':>7}")
    shapes = [(16, 8, 256), (100, 33, 128)] if a.quick else [(16, 8, 16384), (64, 31, 16384), (100, 33, 16384), (256, 63, 4096)]
    for m, n, batch in shapes:
        row(m, n, batch, a.reps, a.warmup)
    _out.close()


if __name__ == "__main__":
    main()
