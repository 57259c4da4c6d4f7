"""Batched trust-region step timing table (mi355x_qr.h section 8g).

Per shape, on factors and Q^T b that one qr_gels_damped_batched_dev call left (lambda = 0, which also yields the Gauss-Newton |D x| the
radii are fractions of; Delta = f x that, f cycling over 2, 1.05, 0.5, 1e-2, 1e-6 by member):
  trust    one qr_trust_batched_dev, rtol 0.1, maxit 10: HIP events on the plan's stream, the minimum of --reps runs;
  loop     the route without it: a host loop of qr_damped_batched_dev with nlam = 1, one device-to-host copy of dxnorm per round and a
           host wait for it, as many rounds as the slowest member of the trust call took: wall time, the minimum of --reps runs.  The
           lambda of the rounds are the trust call's own result (what a host would choose does not change what a round costs);
  iters    the histogram of the iteration counts the trust call returned, and their mean.
Writes the table to --out (default profiles/r20_batched_trust_perf.txt) as well as to the terminal.  One process, one GPU; give each
invocation a time limit of its own (`timeout -k 10 600 python devtools/tools_batched_trust_perf.py`).
Usage: python devtools/tools_batched_trust_perf.py [--reps K] [--quick]
"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import argparse  # noqa: E402

import torch  # noqa: E402

import cuda_qr_amd as q  # noqa: E402

_out = None
FRACS = (2.0, 1.05, 0.5, 1e-2, 1e-6)


def say(line):
    print(line, flush=True)
    if _out:
        _out.write(line + "\n")
        _out.flush()


def event_ms(p, fn):
    s = torch.cuda.ExternalStream(p.stream)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(s)
    fn()
    e1.record(s)
    p.sync()
    return e0.elapsed_time(e1)


def row(m, n, batch, reps, warm):
    plan = q.Plan(m, n, 0, 0)
    gen = torch.Generator(device="cuda").manual_seed(1000 * m + n)

    def rand(*shape):
        return torch.rand(shape, dtype=torch.float64, device="cuda", generator=gen)

    A = rand(batch, n, m) - 0.5                           # member q: m x n column-major, lda = m
    B = rand(batch, 1, m) - 0.5
    d = 0.5 + 1.5 * rand(batch, n)
    tau = torch.empty((batch, n), dtype=torch.float64, device="cuda")
    X = torch.empty((batch, n), dtype=torch.float64, device="cuda")
    lam, xn, rs = (torch.zeros(batch, dtype=torch.float64, device="cuda") for _ in range(3))
    it, st, info = (torch.zeros(batch, dtype=torch.int32, device="cuda") for _ in range(3))
    mn = m * n
    torch.cuda.synchronize()                              # (the plan's stream does not wait for the stream the inputs were made on)
    # factor once; lambda = 0 leaves the Gauss-Newton |D x| in xn
    plan.gels_damped_batched(A, m, n, m, mn, tau, n, B, 1, m, m, lam, 1, 1, X, n, n, info, batch, dD=d, strideD=n, dxnorm=xn)
    plan.sync()
    rss = (B[:, 0, n:] ** 2).sum(dim=1).contiguous()
    frac = torch.tensor([FRACS[k % len(FRACS)] for k in range(batch)], dtype=torch.float64, device="cuda")
    delta = (frac * xn).contiguous()
    torch.cuda.synchronize()

    def trust():
        plan.trust_batched(A, n, m, mn, B, m, m, delta, 1, X, n, n, lam, info, batch, drss=rss, dD=d, strideD=n, rtol=0.1, maxit=10,
                           dxnorm=xn, dresid=rs, diter=it, dstatus=st)

    ts = [event_ms(plan, trust) for _ in range(warm + reps)][warm:]
    t_trust = min(ts)
    iters = it.cpu()
    bad = int((info != 0).sum().item()) + int((st == 3).sum().item())
    rounds = max(int(iters.max().item()), 1)
    host = torch.empty(batch, dtype=torch.float64).pin_memory()
    lam1 = lam.clone()

    def loop():
        for _ in range(rounds):
            plan.damped_batched(A, n, m, mn, B, 1, m, m, lam1, 1, 1, X, n, n, info, batch, drss=rss, dD=d, strideD=n, dxnorm=xn)
            host.copy_(xn, non_blocking=True)             # on the legacy stream: ordered after the plan's, waited for below
            plan.sync()
            torch.cuda.synchronize()                      # the host now holds |D x| of every member and would choose the next lambda

    tl = []
    for k in range(warm + reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        loop()
        if k >= warm:
            tl.append(1e3 * (time.perf_counter() - t0))
    t_loop = min(tl)
    plan.close()
    hist = torch.bincount(iters.to(torch.int64), minlength=rounds + 1).tolist()
    say(f"{m:>3} x {n:<3} {batch:>6} | {t_trust:>9.3f} | {t_loop:>9.3f} ({rounds} rounds) {t_loop / t_trust:>6.2f}x | mean {iters.double().mean().item():.2f} "
        f"hist {hist}{'' if not bad else f'   ({bad} members with an info word or status 3)'}")


def main():
    global _out
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--quick", action="store_true", help="small batches only (a check that the tool runs)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r20_batched_trust_perf.txt"))
    a = ap.parse_args()
    _out = open(a.out, "w")
    say(f"device: {q.device_info()}")
    say(f"one right-hand side, rtol 0.1, maxit 10; ms, minimum of {a.reps} after {a.warmup} warm-up runs")
    say("trust: one qr_trust_batched_dev (HIP events)   loop: rounds x (qr_damped_batched_dev nlam = 1 + copy of dxnorm + host wait), wall")
    say(f"{'m x n':>9} {'batch':>6} | {'trust ms':>9} | {'loop ms':>9} {'':>18} | iterations per member (hist[k]: members with k)")
    shapes = [(16, 8, 256), (100, 33, 128)] if a.quick else [(16, 8, 16384), (64, 32, 16384), (100, 33, 16384), (256, 63, 4096)]
    for m, n, batch in shapes:
        row(m, n, batch, a.reps, a.warmup)
    _out.close()


if __name__ == "__main__":
    main()
