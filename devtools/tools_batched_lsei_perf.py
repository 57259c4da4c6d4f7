"""Batched inequality-constrained least squares timing table (mi355x_qr.h section 8l): HIP events, the minimum of --reps runs after
--warmup warm-up runs, one process.

One qr_lsei_batched_dev (the dual active-set loop of every member in one launch; x, mu, s, state, resid and iter written) at
(m, n, mg) = (16, 8, 12), (64, 31, 40), (100, 33, 64) (batch 16384) and (qr_lsei_batched_max_rows(63, 64), 63, 64) (batch 4096), no
equalities, on planted members: standard normal A and G, x* in [-1, 1], floor(min(n, mg) / 2) rows active with multipliers in [0.5, 1.5],
the other rows with slack in [0.5, 1.5] |G_i|, h = G x* - slack, b = A (x* - z) with (A^T A) z = G^T mu*.  Beside it, in the same run, on
the same GPU and the same A and b, one qr_gglse_batched_dev with the first p rows of every G as equalities, p the mean size of the final
set: what ONE candidate costs at that size.  Columns: the call, the mean and the largest candidate count per member, the gglse call, and
the call over (mean count x gglse): 1 would mean that the launch costs what its candidates cost at the final size; the slowest member of a
workgroup, the refills from A and G, the serial solves and decisions and the s passes push it up, the earlier sets being smaller than the
final one pulls it down.

Writes the table to --out (default profiles/r25_batched_lsei_perf.txt) as well as to the terminal.  One process, one GPU; give each
invocation a time limit of its own (`timeout -k 10 600 python devtools/tools_batched_lsei_perf.py`).
Usage: python devtools/tools_batched_lsei_perf.py [--reps K] [--warmup W] [--quick] [--out FILE]
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


def planted(m, n, mg, batch, gen):
    """A (batch, n, m) and G (batch, n, mg) column-major members, b (batch, m), h (batch, mg) and the planted state (batch, mg)"""
    def rnd(*shape):
        return torch.randn(shape, dtype=torch.float64, device="cuda", generator=gen)

    def uni(*shape):
        return torch.rand(shape, dtype=torch.float64, device="cuda", generator=gen)

    A, G = rnd(batch, n, m), rnd(batch, n, mg)
    Ar, Gr = A.transpose(1, 2), G.transpose(1, 2)             # (batch, m, n), (batch, mg, n)
    xs = 2.0 * uni(batch, n) - 1.0
    na = min(n, mg) // 2
    order = torch.argsort(uni(batch, mg), dim=1)
    state = torch.zeros((batch, mg), dtype=torch.int32, device="cuda")
    state.scatter_(1, order[:, :na], 1)
    act = state.to(torch.float64)
    mus = (0.5 + uni(batch, mg)) * act
    slack = (0.5 + uni(batch, mg)) * torch.linalg.norm(Gr, dim=2) * (1.0 - act)
    h = ((Gr @ xs[:, :, None])[:, :, 0] - slack).contiguous()
    z = torch.linalg.solve(A @ Ar, G @ mus[:, :, None])       # (A^T A) z = G^T mu*
    b = (Ar @ (xs[:, :, None] - z))[:, :, 0].contiguous()
    return A, b, G, h, state, na


def row(m, n, mg, batch, reps, warm):
    plan = q.Plan(m, n, 0, 0)
    ps = torch.cuda.ExternalStream(plan.stream)
    gen = torch.Generator(device="cuda").manual_seed(100000 * m + 1000 * n + mg + 25)
    A, b, G, h, state, na = planted(m, n, mg, batch, gen)
    X = torch.empty((batch, n), dtype=torch.float64, device="cuda")
    MU = torch.empty((batch, mg), dtype=torch.float64, device="cuda")
    S = torch.empty((batch, mg), dtype=torch.float64, device="cuda")
    res = torch.empty(batch, dtype=torch.float64, device="cuda")
    st = torch.zeros((batch, mg), dtype=torch.int32, device="cuda")
    it = torch.zeros(batch, dtype=torch.int32, device="cuda")
    info = torch.zeros(batch, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()

    def lsei():
        plan.lsei_batched(A, m, n, m, m * n, b, m, G, mg, 0, mg, mg * n, h, mg, X, n, info, batch, dMU=MU, strideMU=mg, dS=S, strideS=mg,
                          dstate=st, stridestate=mg, dresid=res, diter=it)

    t_le = best(ps, lsei, lambda: None, plan.sync, reps, warm)
    flagged = int((info != 0).sum().item())
    wrong = int((st != state).any(dim=1).sum().item())
    mean_it, max_it = it.to(torch.float64).mean().item(), int(it.max().item())
    mean_w = st.to(torch.float64).sum(dim=1).mean().item()

    # one gglse on the same A and b with the first p rows of G as equalities (the inputs are read only)
    p = max(1, int(round(mean_w)))
    Cm = G[:, :, :p].contiguous()                             # (batch, n, p): p x n column-major at ldc = p
    d = h[:, :p].contiguous()
    Xg = torch.empty((batch, n), dtype=torch.float64, device="cuda")
    Lg = torch.empty((batch, p), dtype=torch.float64, device="cuda")
    ginfo = torch.zeros(batch, dtype=torch.int32, device="cuda")

    def gglse():
        plan.gglse_batched(A, m, n, m, m * n, Cm, p, p, p * n, b, m, m, d, p, p, 1, Xg, n, n, ginfo, batch, dL=Lg, ldl=p, strideL=p)

    t_gg = best(ps, gglse, lambda: None, plan.sync, reps, warm)
    plan.close()
    say(f"{m:>4} x {n:<3} mg {mg:<3} {batch:>6} | {t_le:>9.3f} | {mean_it:>8.2f} {max_it:>5} | {mean_w:>7.2f} | {t_gg:>9.3f} | "
        f"{t_le / (mean_it * t_gg):>7.2f}   members off the planted set: {wrong}{'' if not flagged else f'   ({flagged} info words)'}")


def main():
    global _out
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--quick", action="store_true", help="small batches only (a check that the tool runs)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r25_batched_lsei_perf.txt"))
    a = ap.parse_args()
    _out = open(a.out, "w")
    say(f"device: {q.device_info()}")
    say(f"one qr_lsei_batched_dev (x, mu, s, state, resid, iter) on planted members, no equalities, half of min(n, mg) rows active; ms by HIP "
        f"events, minimum of {a.reps} after {a.warmup} warm-up runs")
    say("gglse: one qr_gglse_batched_dev on the same A and b with p = the mean |W| rows of G as equalities; ratio = lsei ms / (mean count x gglse ms)")
    say(f"{'m x n':>10} {'mg':>6} {'batch':>6} | {'lsei ms':>9} | {'mean it':>8} {'max':>5} | {'mean W':>7} | {'gglse ms':>9} | {'ratio':>7}")
    mr = q.lsei_batched_max_rows(63, 64)
    shapes = [(16, 8, 12, 256), (100, 33, 64, 128)] if a.quick else [(16, 8, 12, 16384), (64, 31, 40, 16384), (100, 33, 64, 16384),
                                                                     (mr, 63, 64, 4096)]
    for m, n, mg, batch in shapes:
        row(m, n, mg, batch, a.reps, a.warmup)
    _out.close()


if __name__ == "__main__":
    main()
