"""Batched equality-constrained least squares timing table (mi355x_qr.h section 8h): HIP events, the minimum of --reps runs after
--warmup warm-up runs, one right-hand side.

One qr_gglse_batched_dev (every member of the batch in one launch, multipliers and resid included) at (m, n, p) =
  (16, 8, 2), (64, 31, 6), (100, 33, 8) (batch 16384) and (256, 63, 16) (batch 4096)
beside, in the same run, on the same GPU and the same data,
  (b) torch.linalg.solve on the batch of KKT matrices [[A^T A, C^T], [C, 0]] (the matrices pre-built; only the solve is timed).  It is
      timed on the first --kkt-members members and SCALED by batch / that number;
  (c) one qr_gels_batched_dev on the pre-built (m + p) x n stack [A ; C] with [b ; d]: a yardstick for cost -- its answer is a different
      one (the constraint is only fitted, not imposed).
The table also reports how far (b)'s x is from the new call's x on the members (b) ran on.

Writes the table to --out (default profiles/r21_batched_lse_perf.txt) as well as to the terminal.  One process, one GPU; give each
invocation a time limit of its own (`timeout -k 10 600 python devtools/tools_batched_lse_perf.py`).
Usage: python devtools/tools_batched_lse_perf.py [--reps K] [--warmup W] [--quick] [--out FILE]
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


def row(m, n, p, batch, reps, warm, kkt_members):
    plan = q.Plan(max(m + p, n), n, 0, 0)
    ps = torch.cuda.ExternalStream(plan.stream)
    gen = torch.Generator(device="cuda").manual_seed(100000 * m + 1000 * n + p)

    def rnd(*shape):
        return torch.randn(shape, dtype=torch.float64, device="cuda", generator=gen)

    # member q of every operand: column-major, packed (the last two axes are (column, row))
    A, Cm, b, d = rnd(batch, n, m), rnd(batch, n, p), rnd(batch, 1, m), rnd(batch, 1, p)
    X = torch.empty((batch, 1, n), dtype=torch.float64, device="cuda")
    L = torch.empty((batch, 1, p), dtype=torch.float64, device="cuda")
    res = torch.empty((batch, 1), dtype=torch.float64, device="cuda")
    info = torch.zeros(batch, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()

    def lse():
        plan.gglse_batched(A, m, n, m, m * n, Cm, p, p, p * n, b, m, m, d, p, p, 1, X, n, n, info, batch, dL=L, ldl=p, strideL=p, dresid=res,
                           strideres=1)

    t_lse = best(ps, lse, lambda: None, plan.sync, reps, warm)
    singular = int((info != 0).sum().item())

    # (b) the KKT systems of the first `members` members, row-major views of the same data
    members = min(kkt_members, batch)
    Ar, Cr = A[:members].transpose(1, 2), Cm[:members].transpose(1, 2)          # (members, m, n), (members, p, n)
    K = torch.zeros((members, n + p, n + p), dtype=torch.float64, device="cuda")
    K[:, :n, :n] = Ar.transpose(1, 2) @ Ar
    K[:, :n, n:] = Cr.transpose(1, 2)
    K[:, n:, :n] = Cr
    rhs = torch.cat([Ar.transpose(1, 2) @ b[:members].transpose(1, 2), d[:members].transpose(1, 2)], dim=1)
    torch.cuda.synchronize()
    cur = torch.cuda.current_stream()
    sol = []

    def kkt():
        sol[:] = [torch.linalg.solve(K, rhs)]

    t_kkt = best(cur, kkt, lambda: None, torch.cuda.synchronize, reps, warm) * batch / members
    xk = sol[0][:, :n, 0]
    xl = X[:members, 0, :]
    apart = (torch.linalg.norm(xk - xl, dim=1) / torch.linalg.norm(xl, dim=1)).max().item()

    # (c) one gels on the stack [A ; C], [b ; d]: factored in place, so the stack is restored before every run (not timed)
    t_gels = None
    if q.batched_max_rows(n + 1) >= m + p or q.lib.qrd_b_fits(m + p, n + 1):
        S0 = torch.cat([A, Cm], dim=2).contiguous()                             # (batch, n, m + p)
        r0 = torch.cat([b, d], dim=2).contiguous()
        S, r = S0.clone(), r0.clone()
        tau = torch.empty((batch, n), dtype=torch.float64, device="cuda")
        mp = m + p

        def restore():
            S.copy_(S0)
            r.copy_(r0)

        def gels():
            plan.gels_batched(S, mp, n, mp, mp * n, tau, n, r, 1, mp, mp, info, batch)

        t_gels = best(ps, gels, restore, plan.sync, reps, warm)
    plan.close()
    tg = f"{t_gels:>9.3f} {t_gels / t_lse:>6.2f}x" if t_gels is not None else f"{'n/a':>9} {'':>7}"
    say(f"({m:>3}, {n:>2}, {p:>2}) {batch:>6} | {t_lse:>9.3f} | {t_kkt:>10.3f} {t_kkt / t_lse:>7.1f}x | {tg}"
        f"   KKT x vs ours on {members} members: {apart:.1e}{'' if not singular else f'   ({singular} singular)'}")


def main():
    global _out
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--kkt-members", type=int, default=1024, help="members torch.linalg.solve is timed on (scaled to the batch)")
    ap.add_argument("--quick", action="store_true", help="small batches only (a check that the tool runs)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r21_batched_lse_perf.txt"))
    a = ap.parse_args()
    _out = open(a.out, "w")
    say(f"device: {q.device_info()}")
    say(f"one qr_gglse_batched_dev (x, multipliers, resid), one right-hand side; ms by HIP events, minimum of {a.reps} after {a.warmup} warm-up runs")
    say(f"(b) torch.linalg.solve on pre-built KKT matrices, timed on {a.kkt_members} members and SCALED by batch / {a.kkt_members}   "
        f"(c) one qr_gels_batched_dev on the pre-built (m + p) x n stack (a different answer: cost yardstick only)")
    say(f"{'(m, n, p)':>13} {'batch':>6} | {'lse ms':>9} | {'(b) ms':>10} {'(b)/lse':>8} | {'(c) ms':>9} {'(c)/lse':>7}")
    shapes = [(16, 8, 2, 256), (100, 33, 8, 128)] if a.quick else [(16, 8, 2, 16384), (64, 31, 6, 16384), (100, 33, 8, 16384), (256, 63, 16, 4096)]
    for m, n, p, batch in shapes:
        row(m, n, p, batch, a.reps, a.warmup, a.kkt_members)
    _out.close()


if __name__ == "__main__":
    main()
