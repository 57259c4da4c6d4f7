"""Row-removal timing table (mi355x_qr.h section 6b): wall time around calls that end with their own host wait, after warm-up.

For n = 128, 512, 2048 and a window of 16 n rows held in an accumulator (one right-hand side), with p rows per step (default 64):
  (i)   qr_lsacc_pop_dev of p rows beside qr_lsacc_push_dev of the same p rows (the same launches and bytes by construction; the pop
        also copies R, Z and the sums to its workspace and back, and waits for the status word)
  (ii)  qr_lsacc_slide_dev (p in, p out) beside pop + push of the same rows
  (iii) the slide beside one qr_gels_dev on the whole window -- what a caller without row removal pays per step
Every measured call leaves the accumulator holding the window it started from, to rounding (what was pushed is popped again, a slide is
undone by the opposite slide), so the repetitions time the same state.

Writes the table to --out (default profiles/r12_downdate_perf.txt) as well as to the terminal.  One process, one GPU; give each
invocation a time limit of its own (`timeout -k 10 600 python devtools/tools_downdate_perf.py`).
Usage: python devtools/tools_downdate_perf.py [--reps K] [--rows P] [--quick]
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


def buf(rows, cols):
    t = torch.empty((cols, rows), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    return t


def wall(plan, fn, reps, warm, before=None, after=None):
    """median ms of fn() + a drain of the plan's stream; before() / after() (untimed) run around every call"""
    ts = []
    for i in range(warm + reps):
        if before:
            before()
            torch.cuda.synchronize()
        plan.sync()
        t0 = time.perf_counter()
        fn()
        plan.sync()
        if i >= warm:
            ts.append((time.perf_counter() - t0) * 1e3)
        if after:
            after()
            plan.sync()
    ts.sort()
    return ts[len(ts) // 2]


def table(reps, warm, sizes, p):
    say(f"window = 16 n rows, {p} rows per step, one right-hand side; ms wall, median of {reps}")
    say(f"{'n':>5} {'window':>7} | {'push':>8} {'pop':>8} pop/push | {'slide':>8} {'pop+push':>9} slide/(pop+push) | {'gels':>9} slide/gels")
    for n in sizes:
        w = 16 * n
        plan = q.Plan(w, n, 0, 0)
        acc = q.LsAccumulator(plan, n, 1)
        dW0, dW, db0, db, dtau = buf(w, n), buf(w, n), buf(w, 1), buf(w, 1), buf(n, 1)
        dN0, dN, dbN0, dbN = buf(p, n), buf(p, n), buf(p, 1), buf(p, 1)
        dO, dbO = buf(p, n), buf(p, 1)
        plan.fill_uniform(dW0, w, w, n, seed=5)
        plan.fill_uniform(db0, w, w, 1, seed=6)
        plan.fill_uniform(dN0, p, p, n, seed=7)
        plan.fill_uniform(dbN0, p, p, 1, seed=8)
        plan.sync()
        dO.T.copy_(dW0.T[:p])                     # the oldest p rows of the window
        dbO.T.copy_(db0.T[:p])

        def load_window():
            dW.copy_(dW0)
            db.copy_(db0)

        def load_new():                           # the push uses its arguments as workspace
            dN.copy_(dN0)
            dbN.copy_(dbN0)

        load_window()
        torch.cuda.synchronize()
        acc.push(dW, w, w, db, w)
        plan.sync()
        t_push = wall(plan, lambda: acc.push(dN, p, p, dbN, p), reps, warm, before=load_new, after=lambda: acc.pop(dN0, p, p, dbN0, p))

        def push_new():
            load_new()
            torch.cuda.synchronize()
            acc.push(dN, p, p, dbN, p)

        t_pop = wall(plan, lambda: acc.pop(dN0, p, p, dbN0, p), reps, warm, before=push_new)
        t_slide = wall(plan, lambda: acc.slide(dN0, p, p, dbN0, p, dO, p, p, dbO, p), reps, warm,
                       after=lambda: acc.slide(dO, p, p, dbO, p, dN0, p, p, dbN0, p))

        def pop_push():
            acc.pop(dO, p, p, dbO, p)
            acc.push(dN, p, p, dbN, p)

        t_pp = wall(plan, pop_push, reps, warm, before=load_new, after=lambda: acc.slide(dO, p, p, dbO, p, dN0, p, p, dbN0, p))
        t_gels = wall(plan, lambda: plan.gels(dW, w, n, w, dtau, db, 1, w), reps, warm, before=load_window)
        say(f"{n:>5} {w:>7} | {t_push:>8.3f} {t_pop:>8.3f} {t_pop / t_push:>8.2f} | {t_slide:>8.3f} {t_pp:>9.3f} {t_slide / t_pp:>16.2f} | "
            f"{t_gels:>9.3f} {t_slide / t_gels:>10.3f}")
        assert acc.rows() == w
        acc.close()
        plan.close()


def main():
    global _out
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rows", type=int, default=64, help="rows per step")
    ap.add_argument("--quick", action="store_true", help="n = 128 only (a check that the tool runs)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r12_downdate_perf.txt"))
    a = ap.parse_args()
    _out = open(a.out, "w")
    say(f"device: {q.device_info()}   qr_tpqrt_max_rows() = {q.tpqrt_max_rows()}")
    table(a.reps, a.warmup, (128,) if a.quick else (128, 512, 2048), a.rows)
    _out.close()


if __name__ == "__main__":
    main()
