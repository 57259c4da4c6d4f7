"""Batched minimum-norm timing table (mi355x_qr.h section 8e): HIP events on the plan's stream, the minimum of --reps runs.

One qr_gels_wide_batched_dev (one right-hand side, every member of the batch in one fused launch) at
  6 x 7, 8 x 16, 31 x 64 (batch 16384) and 60 x 256 (batch 4096)
beside, in the same run and on the same batch,
  (a) the composed route: qr_transpose_batched_dev, qr_geqrf_batched_dev, qr_minnorm_batched_dev (three launches);
  (b) transpose plus geqrf alone: what a caller pays who goes on with qr_gels_batched_dev-style calls of his own;
  (c) torch.linalg.lstsq on the same batch, if it takes wide matrices on this build ("n/a" otherwise);
  (d) a loop of the one-matrix qr_gels_wide_dev over 64 members, wall time, SCALED by batch / 64.

Writes the table to --out (default profiles/r17_batched_minnorm_perf.txt) as well as to the terminal.  One process, one GPU; give each
invocation a time limit of its own (`timeout -k 10 600 python devtools/tools_batched_minnorm_perf.py`).
Usage: python devtools/tools_batched_minnorm_perf.py [--reps K] [--quick]
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
LOOP = 64          # members of the one-matrix loop


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


def row(m, n, batch, reps, warm):
    nrhs = 1
    plan = q.Plan(n, m, 0, 0)
    gen = torch.Generator(device="cuda").manual_seed(1000 * m + n)
    A = torch.rand((batch, n, m), dtype=torch.float64, device="cuda", generator=gen) - 0.5     # member q: m x n column-major, lda = m
    B = torch.zeros((batch, nrhs, n), dtype=torch.float64, device="cuda")                      # n rows tall: B on top of zeros
    B[:, :, :m] = torch.rand((batch, nrhs, m), dtype=torch.float64, device="cuda", generator=gen) - 0.5
    dF = torch.empty((batch, m, n), dtype=torch.float64, device="cuda")
    dX = torch.empty_like(B)
    dtau = torch.empty((batch, m), dtype=torch.float64, device="cuda")
    dinfo = torch.zeros(batch, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    mn = m * n

    def restore():
        dX.copy_(B)

    def fused():
        plan.gels_wide_batched(A, m, n, m, mn, dF, n, mn, dtau, m, dX, nrhs, n, n * nrhs, dinfo, batch)

    def transpose_geqrf():
        plan.transpose_batched(A, m, n, m, mn, dF, n, mn, batch)
        plan.geqrf_batched(dF, n, m, n, mn, dtau, m, batch)

    def composed():
        transpose_geqrf()
        plan.minnorm_batched(dF, n, m, n, mn, dtau, m, dX, nrhs, n, n * nrhs, dinfo, batch)

    t_fused = best(plan, fused, restore, reps, warm)
    singular = int((dinfo != 0).sum().item())
    x_fused = dX.clone()
    t_comp = best(plan, composed, restore, reps, warm)
    agree = (torch.linalg.norm(dX - x_fused) / torch.linalg.norm(x_fused)).item()
    t_tg = best(plan, transpose_geqrf, restore, reps, warm)

    # (c) torch on the same batch: row-major views of the same data
    t_torch = None
    try:
        At = A.transpose(1, 2).contiguous()                  # (batch, m, n)
        Bt = B[:, :, :m].transpose(1, 2).contiguous()        # (batch, m, nrhs)
        ts = []
        for k in range(warm + reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            torch.linalg.lstsq(At, Bt)
            torch.cuda.synchronize()
            if k >= warm:
                ts.append((time.perf_counter() - t0) * 1e3)
        t_torch = min(ts)
    except Exception as e:   # noqa: BLE001  (a build whose lstsq does not take wide matrices on the device)
        say(f"     torch.linalg.lstsq on {m} x {n}: {type(e).__name__}: {str(e).splitlines()[0][:100]}")

    # (d) the one-matrix call, member by member
    members = min(LOOP, batch)
    wF = torch.empty((m, n), dtype=torch.float64, device="cuda")
    wtau = torch.empty(m, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    t_loop = None
    try:
        ts = []
        for k in range(warm + reps):
            restore()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for i in range(members):
                plan.gels_wide(A[i], m, n, m, wF, n, wtau, dX[i], nrhs, n)
            plan.sync()
            if k >= warm:
                ts.append((time.perf_counter() - t0) * 1e3)
        t_loop = min(ts) * batch / members
    except q.QRError as e:   # (a shape the one-matrix call does not take)
        say(f"     qr_gels_wide_dev on {m} x {n}: {e}")
    plan.close()
    tt = f"{t_torch:>9.3f} {t_torch / t_fused:>6.1f}x" if t_torch is not None else f"{'n/a':>9} {'':>7}"
    tl = f"{t_loop:>11.1f} {t_loop / t_fused:>8.0f}x" if t_loop is not None else f"{'n/a':>11} {'':>9}"
    say(f"{m:>3} x {n:<4} {batch:>6} | {t_fused:>9.3f} | {t_comp:>9.3f} {t_comp / t_fused:>6.2f}x | {t_tg:>9.3f} | {tt} | {tl}"
          f"   fused vs composed X: {agree:.1e}{'' if not singular else f'   ({singular} singular)'}")


def main():
    global _out
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--quick", action="store_true", help="small batches only (a check that the tool runs)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r17_batched_minnorm_perf.txt"))
    a = ap.parse_args()
    _out = open(a.out, "w")
    say(f"device: {q.device_info()}")
    say(f"one qr_gels_wide_batched_dev (fused), one right-hand side; ms, minimum of {a.reps} after {a.warmup} warm-up runs")
    say(f"(a) transpose + geqrf + minnorm, same batch   (b) transpose + geqrf alone   (c) torch.linalg.lstsq, wall   "
        f"(d) {LOOP} one-matrix qr_gels_wide_dev calls, wall, SCALED by batch / {LOOP}")
    say(f"{'m x n':>10} {'batch':>6} | {'fused ms':>9} | {'(a) ms':>9} {'(a)/f':>7} | {'(b) ms':>9} | {'(c) ms':>9} {'(c)/f':>7} | {'(d) ms scaled':>11} {'(d)/f':>9}")
    shapes = [(6, 7, 256), (31, 64, 128)] if a.quick else [(6, 7, 16384), (8, 16, 16384), (31, 64, 16384), (60, 256, 4096)]
    for m, n, batch in shapes:
        row(m, n, batch, a.reps, a.warmup)
    _out.close()


if __name__ == "__main__":
    main()
