"""Bounded batched Levenberg-Marquardt timing table (mi355x_qr.h section 8n): one bounded round beside one round of section 8m on the
same batch.

Per shape, on seeded members (J and f uniform in (-0.5, 0.5), x0 likewise; f at the trial point is 0.9 f), the first round after a start:
  8m       qr_lm_batched_step_dev + qr_lm_batched_update_dev: HIP events on the plan's stream around the two calls, the minimum of --reps
           runs after --warmup warm-up runs;
  8n       qr_lmb_batched_step_dev (peg, geqp3, ormqr 'T', the step) + qr_lmb_batched_update_dev, the same way, on the box
           [x0 - 0.05, x0 + 0.05] with every fourth entry of lo equal to x0 (on its bound at the start: the peg sums that column and holds
           it where the gradient points outward, and the step is cut);
  free     8n with every bound infinite (the peg launch finds nothing on a bound: the cost of the launch itself).
Writes the table to --out (default profiles/r28_batched_lmb_perf.txt) as well as to the terminal.  One process, one GPU; give each
invocation a time limit of its own (`timeout -k 10 600 python devtools/tools_batched_lmb_perf.py`).
Usage: python devtools/tools_batched_lmb_perf.py [--reps K] [--quick]
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


def row(m, n, batch, reps, warm):
    """one line of the table.  Everything that lives on the plan's stream is a local of measure() and is gone before the plan is closed"""
    plan = q.Plan(m, n, 0, 0)
    try:
        line = measure(plan, m, n, batch, reps, warm)
        torch.cuda.synchronize()
    finally:
        plan.close()
    say(line)


def one_round(plan, s, lm, start, J0, F0, Ft, reps, warm):
    """(round ms, step ms, update ms): the minimum over the measured runs"""
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
    J, F = J0.clone(), F0.clone()
    ts = []
    for _ in range(warm + reps):
        J.copy_(J0)
        F.copy_(F0)
        start()
        ev[0].record(s)
        lm.step(J, F)
        ev[1].record(s)
        lm.update(Ft)
        ev[2].record(s)
        plan.sync()
        ts.append((ev[0].elapsed_time(ev[2]), ev[0].elapsed_time(ev[1]), ev[1].elapsed_time(ev[2])))
    return tuple(min(t[k] for t in ts[warm:]) for k in range(3))


def measure(plan, m, n, batch, reps, warm):
    s = torch.cuda.ExternalStream(plan.stream)
    gen = torch.Generator(device="cuda").manual_seed(1000 * m + n)

    def rand(*shape):
        return torch.rand(shape, dtype=torch.float64, device="cuda", generator=gen) - 0.5

    J0, F0, X0 = rand(batch, n, m), rand(batch, m), rand(batch, n)      # member q: J m x n column-major, ldj = m
    lo, hi = X0 - 0.05, X0 + 0.05
    lo[:, ::4] = X0[:, ::4]
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        Ft = 0.9 * F0
        lm = q.LmBatched(plan, m, n, batch)
        t_m = one_round(plan, s, lm, lambda: lm.start(X0), J0, F0, Ft, reps, warm)
        lm.close()
        lb = q.LmBoundedBatched(plan, m, n, batch)
        t_n = one_round(plan, s, lb, lambda: lb.start(X0, dLo=lo, dHi=hi), J0, F0, Ft, reps, warm)
        st = lb.state()
        held = int((st["peg"] != 0).sum().item())
        clipped = int(st["clipped"].sum().item())
        bad = int((st["info"] != 0).sum().item())
        t_f = one_round(plan, s, lb, lambda: lb.start(X0), J0, F0, Ft, reps, warm)
        plan.sync()
        lb.close()
        del st
    torch.cuda.synchronize()
    return (f"{m:>3} x {n:<3} {batch:>6} | {t_m[0]:>8.3f} {t_m[1]:>8.3f} {t_m[2]:>7.3f} | {t_n[0]:>8.3f} {t_n[1]:>8.3f} {t_n[2]:>7.3f} {t_n[0] / t_m[0]:>5.2f}x | "
            f"{t_f[0]:>8.3f} {t_f[0] / t_m[0]:>5.2f}x | held {held / batch:.1f} columns a member, clipped {clipped}"
            f"{'' if not bad else f'   ({bad} members with an info word)'}")


def main():
    global _out
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--quick", action="store_true", help="small batches only (a check that the tool runs)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r28_batched_lmb_perf.txt"))
    a = ap.parse_args()
    _out = open(a.out, "w")
    say(f"device: {q.device_info()}")
    say(f"the first round after a start, defaults; ms by HIP events, minimum of {a.reps} after {a.warmup} warm-up runs")
    say("8m: qr_lm_batched_step_dev + _update_dev   8n: qr_lmb_batched_step_dev (peg + geqp3 + ormqr + step) + _update_dev on a box   "
        "free: 8n with every bound infinite")
    say(f"{'m x n':>9} {'batch':>6} | {'8m round':>8} {'step':>8} {'update':>7} | {'8n round':>8} {'step':>8} {'update':>7} {'':>6} | {'free':>8} {'':>6} |")
    shapes = [(16, 8, 256), (100, 33, 128)] if a.quick else [(16, 8, 16384), (64, 31, 16384), (100, 33, 16384), (256, 63, 4096)]
    for m, n, batch in shapes:
        row(m, n, batch, a.reps, a.warmup)
    _out.close()


if __name__ == "__main__":
    main()
