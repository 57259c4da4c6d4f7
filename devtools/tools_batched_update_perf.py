"""Batched sliding-window update timing table (mi355x_qr.h section 8d): HIP events on the plan's stream, the minimum of --reps runs.

One qr_lsacc_batched_slide_dev (step rows in, step rows out, one right-hand side, every member of the batch in one launch) at
  n = 8, batch 16384, window 64, step 4;   n = 32, batch 16384, window 256, step 8;   n = 63, batch 4096, window 256, step 16
(63 unknowns and the right-hand side are the 64 columns the fused kernels hold) beside, in the same run,
  (a) one qr_gels_batched_dev on the whole window of the same batch: the refactor-every-step alternative (its copy of the window is not
      in its time);
  (b) a loop of the one-matrix qr_lsacc_slide_dev over 64 members, wall time (each call waits for its status word), SCALED by batch / 64.

Writes the table to --out (default profiles/r16_batched_update_perf.txt) as well as to the terminal.  One process, one GPU; give each
invocation a time limit of its own (`timeout -k 10 600 python devtools/tools_batched_update_perf.py`).
Usage: python devtools/tools_batched_update_perf.py [--reps K] [--quick]
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


def row(n, batch, window, step, reps, warm):
    nrhs, runs = 1, warm + reps
    m = window + runs * step
    plan = q.Plan(window, n, 0, 0)
    gen = torch.Generator(device="cuda").manual_seed(1000 * n + step)
    A = torch.randn((batch, n, m), dtype=torch.float64, device="cuda", generator=gen)          # member q: m x n column-major, lda = m
    Y = torch.randn((batch, nrhs, m), dtype=torch.float64, device="cuda", generator=gen)
    dinfo = torch.zeros(batch, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    a0, y0 = A.data_ptr(), Y.data_ptr()
    sa, sy = n * m, nrhs * m

    # the batched accumulator: the first window pushed, then one slide per run
    acc = q.LsAccumulatorBatched(plan, n, nrhs, batch)
    acc.push(a0, window, m, sa, y0, m, sy)
    plan.sync()
    ts = []
    for k in range(1, runs + 1):
        o, e = (k - 1) * step, (k - 1) * step + window
        t = event_ms(plan, lambda: acc.slide(a0 + 8 * e, step, m, sa, y0 + 8 * e, m, sy, a0 + 8 * o, step, m, sa, y0 + 8 * o, m, sy, dinfo))
        if k > warm:
            ts.append(t)
    refused = int((dinfo != 0).sum().item())
    t_slide = min(ts)
    acc.close()

    # (a) the whole window refactored: one fused qr_gels_batched_dev on copies
    dW = torch.empty((batch, n, window), dtype=torch.float64, device="cuda")
    dC = torch.empty((batch, nrhs, window), dtype=torch.float64, device="cuda")
    dtau = torch.empty((batch, n), dtype=torch.float64, device="cuda")
    ts = []
    for k in range(runs):
        dW.copy_(A[:, :, k * step:k * step + window])
        dC.copy_(Y[:, :, k * step:k * step + window])
        torch.cuda.synchronize()
        t = event_ms(plan, lambda: plan.gels_batched(dW, window, n, window, n * window, dtau, n, dC, nrhs, window, nrhs * window, dinfo, batch))
        if k >= warm:
            ts.append(t)
    t_gels = min(ts)

    # (b) the one-matrix accumulator, member by member
    members = min(LOOP, batch)
    accs = [q.LsAccumulator(plan, n, nrhs) for _ in range(members)]
    wA = torch.empty((n, window), dtype=torch.float64, device="cuda")
    wY = torch.empty((nrhs, window), dtype=torch.float64, device="cuda")
    for i, a in enumerate(accs):
        wA.copy_(A[i, :, :window])
        wY.copy_(Y[i, :, :window])
        torch.cuda.synchronize()
        a.push(wA, window, window, wY, window)
        plan.sync()
    ts = []
    for k in range(1, runs + 1):
        o, e = (k - 1) * step, (k - 1) * step + window
        t0 = time.perf_counter()
        for i, a in enumerate(accs):
            ai, yi = a0 + 8 * i * sa, y0 + 8 * i * sy
            a.slide(ai + 8 * e, step, m, yi + 8 * e, m, ai + 8 * o, step, m, yi + 8 * o, m)
        plan.sync()
        if k > warm:
            ts.append((time.perf_counter() - t0) * 1e3)
    t_loop = min(ts) * batch / members
    for a in accs:
        a.close()
    plan.close()
    say(f"{n:>4} {batch:>6} {window:>6} {step:>4} | {t_slide:>9.3f} | {t_gels:>9.3f} {t_gels / t_slide:>6.2f}x | {t_loop:>11.1f} {t_loop / t_slide:>8.0f}x"
        f"{'' if not refused else f'   ({refused} slides refused)'}")


def main():
    global _out
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--quick", action="store_true", help="small batches only (a check that the tool runs)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r16_batched_update_perf.txt"))
    a = ap.parse_args()
    _out = open(a.out, "w")
    say(f"device: {q.device_info()}   qr_tpqrt_batched_max_rows(9, 33, 64) = {[q.tpqrt_batched_max_rows(c) for c in (9, 33, 64)]}")
    say(f"one qr_lsacc_batched_slide_dev, one right-hand side; ms, minimum of {a.reps} after {a.warmup} warm-up runs")
    say(f"(a) one qr_gels_batched_dev on the whole window, same batch   (b) {LOOP} one-matrix qr_lsacc_slide_dev calls, wall, SCALED by batch / {LOOP}")
    say(f"{'n':>4} {'batch':>6} {'window':>6} {'step':>4} | {'slide ms':>9} | {'(a) ms':>9} {'(a)/sl':>7} | {'(b) ms scaled':>11} {'(b)/sl':>9}")
    shapes = [(8, 256, 64, 4), (32, 128, 256, 8)] if a.quick else [(8, 16384, 64, 4), (32, 16384, 256, 8), (63, 4096, 256, 16)]
    for n, batch, window, step in shapes:
        row(n, batch, window, step, a.reps, a.warmup)
    _out.close()


if __name__ == "__main__":
    main()
