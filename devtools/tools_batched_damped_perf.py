"""Batched damped least-squares timing table (mi355x_qr.h section 8f): HIP events on the plan's stream, the minimum of --reps runs.

For nlam = 1 and 8, one right-hand side, d uniform in [0.5, 2], lambda = 0.3 .. |A|-sized values, at
  16 x 8, 64 x 32, 100 x 33 (batch 16384) and 256 x 63 (batch 4096; 64 columns plus a right-hand side are more than the 64 the call holds)
in the same run and on the same batch:
  fused    one qr_gels_damped_batched_dev: factor and every lambda;
  solve    one qr_damped_batched_dev on the factors and Q^T B the fused call left: what each further list of lambdas costs;
  stacked  the route that exists without section 8f: nlam calls of qr_gels_batched_dev on pre-built stacked matrices [A ; lambda D]
           ((m + n) x n, built outside the timed region), one per lambda.

Writes the table to --out (default profiles/r18_batched_damped_perf.txt) as well as to the terminal.  One process, one GPU; give each
invocation a time limit of its own (`timeout -k 10 600 python devtools/tools_batched_damped_perf.py`).
Usage: python devtools/tools_batched_damped_perf.py [--reps K] [--quick]
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


def event_ms(p, fn):
    s = torch.cuda.ExternalStream(p.stream)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(s)
    fn()
    e1.record(s)
    p.sync()
    return e0.elapsed_time(e1)


def best(plan, fn, before, reps, warm):
    ts = []
    for k in range(warm + reps):
        before()
        torch.cuda.synchronize()
        t = event_ms(plan, fn)
        if k >= warm:
            ts.append(t)
    return min(ts)


def row(m, n, batch, nlam, reps, warm):
    nrhs = 1
    plan = q.Plan(m, n, 0, 0)
    gen = torch.Generator(device="cuda").manual_seed(1000 * m + n)

    def rand(*shape):
        return torch.rand(shape, dtype=torch.float64, device="cuda", generator=gen)

    A0 = rand(batch, n, m) - 0.5                          # member q: m x n column-major, lda = m
    B0 = rand(batch, nrhs, m) - 0.5
    d = 0.5 + 1.5 * rand(batch, n)
    lam = 0.3 * (1.0 + torch.arange(nlam, dtype=torch.float64, device="cuda")).repeat(batch, 1).contiguous()
    A, B = torch.empty_like(A0), torch.empty_like(B0)
    tau = torch.empty((batch, n), dtype=torch.float64, device="cuda")
    X = torch.empty((batch, nlam * nrhs, n), dtype=torch.float64, device="cuda")
    X2 = torch.empty_like(X)
    xn, rs = (torch.empty((batch, nlam * nrhs), dtype=torch.float64, device="cuda") for _ in range(2))
    info = torch.zeros((batch, nlam), dtype=torch.int32, device="cuda")
    mn, ms = m * n, (m + n) * n
    # the stacked matrices of today's route, one per lambda: [A ; lambda D] and [B ; 0]
    S0 = torch.zeros((nlam, batch, n, m + n), dtype=torch.float64, device="cuda")
    S0[:, :, :, :m] = A0
    idx = torch.arange(n, device="cuda")
    for k in range(nlam):
        S0[k, :, idx, m + idx] = lam[:, k:k + 1] * d
    C0 = torch.zeros((nlam, batch, nrhs, m + n), dtype=torch.float64, device="cuda")
    C0[:, :, :, :m] = B0
    S, Cs = torch.empty_like(S0), torch.empty_like(C0)
    ginfo = torch.zeros(batch, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()

    def restore():
        A.copy_(A0)
        B.copy_(B0)

    def restore_stacked():
        S.copy_(S0)
        Cs.copy_(C0)

    def fused():
        plan.gels_damped_batched(A, m, n, m, mn, tau, n, B, nrhs, m, m * nrhs, lam, nlam, nlam, X, n, n * nlam * nrhs, info, batch, dD=d,
                                 strideD=n, dxnorm=xn, dresid=rs)

    def solve():
        plan.damped_batched(A, n, m, mn, B, nrhs, m, m * nrhs, lam, nlam, nlam, X2, n, n * nlam * nrhs, info, batch, dD=d, strideD=n,
                            dxnorm=xn, dresid=rs)

    def stacked():
        for k in range(nlam):
            plan.gels_batched(S[k], m + n, n, m + n, ms, tau, n, Cs[k], nrhs, m + n, (m + n) * nrhs, ginfo, batch)

    t_fused = best(plan, fused, restore, reps, warm)
    bad = int((info != 0).sum().item())
    t_solve = best(plan, solve, lambda: None, reps, warm)          # (A and B hold the factors and Q^T B of the last fused call)
    same = bool(torch.equal(X, X2))
    t_stack, agree = None, float("nan")
    try:
        t_stack = best(plan, stacked, restore_stacked, reps, warm)
        Xs = Cs[:, :, :, :n].permute(1, 0, 2, 3).reshape(batch, nlam * nrhs, n)
        agree = (torch.linalg.norm(Xs - X) / torch.linalg.norm(X)).item()
    except q.QRError as e:   # (a stacked shape that qr_gels_batched_dev does not take)
        say(f"     qr_gels_batched_dev on {m + n} x {n}: {e}")
    plan.close()
    ts = f"{t_stack:>9.3f} {t_stack / t_fused:>7.2f}x {t_stack / t_solve:>7.2f}x" if t_stack is not None else f"{'n/a':>9} {'':>8} {'':>8}"
    say(f"{m:>3} x {n:<3} {batch:>6} {nlam:>4} | {t_fused:>9.3f} | {t_solve:>9.3f} | {ts}   X against stacked: {agree:.1e}, "
        f"solve == fused bitwise: {same}{'' if not bad else f'   ({bad} singular)'}")


def main():
    global _out
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--quick", action="store_true", help="small batches only (a check that the tool runs)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r18_batched_damped_perf.txt"))
    a = ap.parse_args()
    _out = open(a.out, "w")
    say(f"device: {q.device_info()}")
    say(f"one right-hand side; ms, minimum of {a.reps} after {a.warmup} warm-up runs")
    say("fused: qr_gels_damped_batched_dev   solve: qr_damped_batched_dev on its factors   "
        "stacked: nlam x qr_gels_batched_dev on pre-built [A ; lambda D]")
    say(f"{'m x n':>9} {'batch':>6} {'nlam':>4} | {'fused ms':>9} | {'solve ms':>9} | {'stacked':>9} {'/fused':>8} {'/solve':>8}")
    shapes = [(16, 8, 256), (100, 33, 128)] if a.quick else [(16, 8, 16384), (64, 32, 16384), (100, 33, 16384), (256, 63, 4096)]
    for m, n, batch in shapes:
        for nlam in (1, 8):
            row(m, n, batch, nlam, a.reps, a.warmup)
    _out.close()


if __name__ == "__main__":
    main()
