"""Batched Levenberg-Marquardt timing table (mi355x_qr.h section 8m): one round of the solver against the loop it replaces.

Per shape, on seeded members (J and f uniform in (-0.5, 0.5), x0 likewise; f at the trial point is 0.9 f, so every member accepts), the
first round after a start:
  round    qr_lm_batched_step_dev (geqp3, ormqr 'T', the step) + qr_lm_batched_update_dev: HIP events on the plan's stream around the two
           calls, the minimum of --reps runs;
  parts    the same with the events around the step and around the update alone;
  loop     the route without it: qr_geqp3_batched_dev, qr_ormqr_batched_dev, the rules a to e in torch (norms of the columns of R, D, gnorm),
           qr_trust_batched_dev, then the rules g to i and the update in torch (torch.where per branch), a device-to-host copy of the status
           words and a host wait: wall time, the minimum of --reps runs.  The torch code runs on the plan's stream.
Writes the table to --out (default profiles/r27_batched_lm_perf.txt) as well as to the terminal.  One process, one GPU; give each
invocation a time limit of its own (`timeout -k 10 600 python devtools/tools_batched_lm_perf.py`).
Usage: python devtools/tools_batched_lm_perf.py [--reps K] [--quick]
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


def say(line):
    print(line, flush=True)
    if _out:
        _out.write(line + "\n")
        _out.flush()


def row(m, n, batch, reps, warm):
    """one line of the table.  Everything that lives on the plan's stream -- the events recorded on it, the tensors allocated under it,
    the solver -- is a local of measure() and is gone before the plan (and with it the stream) is closed"""
    plan = q.Plan(m, n, 0, 0)
    try:
        line = measure(plan, m, n, batch, reps, warm)
        torch.cuda.synchronize()
    finally:
        plan.close()
    say(line)


def measure(plan, m, n, batch, reps, warm):
    s = torch.cuda.ExternalStream(plan.stream)
    gen = torch.Generator(device="cuda").manual_seed(1000 * m + n)

    def rand(*shape):
        return torch.rand(shape, dtype=torch.float64, device="cuda", generator=gen) - 0.5

    J0, F0, X0 = rand(batch, n, m), rand(batch, m), rand(batch, n)      # member q: J m x n column-major, ldj = m
    torch.cuda.synchronize()
    mn = m * n
    lm = q.LmBatched(plan, m, n, batch)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
    with torch.cuda.stream(s):
        J, F, Ft = J0.clone(), F0.clone(), 0.9 * F0
        st = lm.state()
        ts = []
        for _ in range(warm + reps):
            J.copy_(J0)
            F.copy_(F0)
            lm.start(X0)
            ev[0].record(s)
            lm.step(J, F)
            ev[1].record(s)
            lm.update(Ft)
            ev[2].record(s)
            plan.sync()
            ts.append((ev[0].elapsed_time(ev[2]), ev[0].elapsed_time(ev[1]), ev[1].elapsed_time(ev[2])))
        t_round, t_step, t_upd = (min(t[k] for t in ts[warm:]) for k in range(3))
        accepted = int(st["accepted"].sum().item())
        bad = int((st["info"] != 0).sum().item())
        par_it = st["par_status"].cpu()

        # the loop it replaces
        jp = torch.zeros((batch, n), dtype=torch.int32, device="cuda")
        tau = torch.zeros((batch, n), dtype=torch.float64, device="cuda")
        P = torch.zeros((batch, n), dtype=torch.float64, device="cuda")
        lam, pn = (torch.zeros(batch, dtype=torch.float64, device="cuda") for _ in range(2))
        info, pst = (torch.zeros(batch, dtype=torch.int32, device="cuda") for _ in range(2))
        host = torch.empty(batch, dtype=torch.int32).pin_memory()
        eps, ftol = 2.220446049250313e-16, 1.4901161193847656e-08

        def loop():
            J.copy_(J0)
            F.copy_(F0)
            plan.geqp3_batched(J, m, n, m, mn, jp, n, tau, n, batch)
            plan.ormqr_batched("T", J, m, n, m, mn, tau, n, F, 1, m, m, batch)
            R = torch.tril(J[:, :, :n])                           # R[q, c, i] = R(i, c)
            z = F[:, :n]
            fnorm = torch.linalg.vector_norm(F, dim=1)
            acn = torch.linalg.vector_norm(R, dim=2)
            jl = jp.long()
            D = torch.empty_like(acn).scatter_(1, jl, torch.where(acn == 0, torch.ones_like(acn), acn))
            xnorm = torch.linalg.vector_norm(D * X0, dim=1)
            delta = torch.where(xnorm == 0, torch.full_like(xnorm, 100.0), 100.0 * xnorm)
            gnorm = ((R * (z / fnorm[:, None])[:, None, :]).sum(2).abs() / acn).max(dim=1).values
            plan.trust_batched(J, n, m, mn, F, m, m, delta, 1, P, n, n, lam, info, batch, djpvt=jp, stridejpvt=n, dD=D, strideD=n, rtol=0.1,
                               maxit=10, dxnorm=pn, dstatus=pst)
            xtrial = X0 - P
            delta = torch.minimum(delta, pn)
            rp = torch.einsum("bci,bc->bi", R, P.gather(1, jl))
            t1 = (torch.linalg.vector_norm(rp, dim=1) / fnorm) ** 2
            t2 = (lam * pn / fnorm) ** 2
            prered, dirder = t1 + t2 / 0.5, -(t1 + t2)
            fnorm1 = torch.linalg.vector_norm(Ft, dim=1)
            ok = torch.isfinite(fnorm1) & (0.1 * fnorm1 < fnorm)
            actred = torch.where(ok, 1.0 - (fnorm1 / fnorm) ** 2, torch.full_like(fnorm, -1.0))
            ratio = torch.where(prered != 0, actred / prered, torch.zeros_like(prered))
            temp = torch.where(actred >= 0, torch.full_like(actred, 0.5), 0.5 * dirder / (dirder + 0.5 * actred))
            temp = torch.where(~ok | (temp < 0.1), torch.full_like(temp, 0.1), temp)
            low, high = ratio <= 0.25, (ratio > 0.25) & ((lam == 0) | (ratio >= 0.75))
            par = lam * lam
            delta = torch.where(low, temp * torch.minimum(delta, pn / 0.1), torch.where(high, pn / 0.5, delta))
            par = torch.where(low, par / temp, torch.where(high, 0.5 * par, par))
            acc = ratio >= 1e-4
            x = torch.where(acc[:, None], xtrial, X0)
            xnorm = torch.where(acc, torch.linalg.vector_norm(D * x, dim=1), xnorm)
            small = 0.5 * ratio <= 1.0
            c1 = (actred.abs() <= ftol) & (prered <= ftol) & small
            c2 = delta <= ftol * xnorm
            stt = torch.where(c1 & c2, 3, torch.where(c2, 2, torch.where(c1, 1, 0)))
            stt = torch.where((stt == 0) & (gnorm <= eps), 8, torch.where((stt == 0) & (delta <= eps * xnorm), 7, stt))
            host.copy_(stt.to(torch.int32), non_blocking=True)
            plan.sync()
            return par

        tl = []
        for k in range(warm + reps):
            plan.sync()
            t0 = time.perf_counter()
            loop()
            if k >= warm:
                tl.append(1e3 * (time.perf_counter() - t0))
        t_loop = min(tl)
        plan.sync()
        lm.close()
        del ev, st, J, F, Ft, jp, tau, P, lam, pn, info, pst, host
    torch.cuda.synchronize()
    hist = torch.bincount(par_it.to(torch.int64), minlength=4).tolist()
    return (f"{m:>3} x {n:<3} {batch:>6} | {t_round:>9.3f} | {t_step:>8.3f} {t_upd:>7.3f} | {t_loop:>9.3f} {t_loop / t_round:>6.2f}x | accepted {accepted}, "
        f"search status hist {hist}{'' if not bad else f'   ({bad} members with an info word)'}")


def main():
    global _out
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--quick", action="store_true", help="small batches only (a check that the tool runs)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r27_batched_lm_perf.txt"))
    a = ap.parse_args()
    _out = open(a.out, "w")
    say(f"device: {q.device_info()}")
    say(f"the first round after a start, defaults (factor 100, par_rtol 0.1, par_maxit 10); ms, minimum of {a.reps} after {a.warmup} warm-up runs")
    say("round: qr_lm_batched_step_dev + qr_lm_batched_update_dev (HIP events)   loop: geqp3 + ormqr + qr_trust_batched_dev + the rules in torch "
        "+ copy of the status words + host wait, wall")
    say(f"{'m x n':>9} {'batch':>6} | {'round ms':>9} | {'step':>8} {'update':>7} | {'loop ms':>9} {'':>7} |")
    shapes = [(16, 8, 256), (100, 33, 128)] if a.quick else [(16, 8, 16384), (64, 31, 16384), (100, 33, 16384), (256, 63, 4096)]
    for m, n, batch in shapes:
        row(m, n, batch, a.reps, a.warmup)
    _out.close()


if __name__ == "__main__":
    main()
