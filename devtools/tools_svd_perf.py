"""Jacobi SVD timing table (mi355x_qr.h section 7): HIP events on the plan's stream after warm-up, drained between repeats, min and median.

  (i)   qr_gesvj_dev on R^T (the lower triangle of the QR of a uniform 4n x n matrix) for n = 128, 256, 512, 1024, values only and with V:
        sweeps, launches of the pair kernel (sweeps x rounds), ms; beside it, as a comparator only, torch.linalg.svdvals / torch.linalg.svd
        of the same matrix on the same GPU where the installed torch provides them
  (ii)  qr_gesvd_dev (values only, and with U and V) at 262144 x 512 and 16384 x 1024 beside qr_geqrf_dev alone in the same run
  (iii) with --split: nothing is timed; one n = 512 qr_gesvj_dev call with V runs so that
        `rocprofv3 --kernel-trace --stats -- python devtools/tools_svd_perf.py --split` shows the per-kernel split (a run of its own, no
        counters, no events)

Writes the table to --out (default profiles/r11_svd_perf.txt) as well as to the terminal.  One process, one GPU; give each invocation a
time limit of its own (`timeout -k 10 600 python devtools/tools_svd_perf.py`).
Usage: python devtools/tools_svd_perf.py [--reps K] [--quick] [--split]
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


def timed(p, fn, reps, warm, before=None):
    """(min, median) ms of fn() between two HIP events on the plan's stream; before() (untimed) runs ahead of every call"""
    s = torch.cuda.ExternalStream(p.stream)
    out = []
    for i in range(warm + reps):
        if before:
            before()
            torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(s)
        fn()
        e1.record(s)
        p.sync()
        if i >= warm:
            out.append(e0.elapsed_time(e1))
    out.sort()
    return out[0], out[len(out) // 2]


def timed_torch(fn, reps, warm):
    out = []
    for i in range(warm + reps):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        if i >= warm:
            out.append(e0.elapsed_time(e1))
    out.sort()
    return out[0], out[len(out) // 2]


def buf(rows, cols):
    t = torch.empty((cols, rows), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    return t


def triangle_t(n, seed):
    """R^T (n x n, lower triangular) of a uniform 4n x n matrix, from the library itself, as a column-major (n, n) tensor"""
    p = q.Plan(4 * n, n, 0, 0)
    dA, dtau = buf(4 * n, n), buf(n, 1)
    p.fill_uniform(dA, 4 * n, 4 * n, n, seed=seed)
    p.geqrf(dA, 4 * n, n, 4 * n, dtau)
    p.sync()
    Rt = torch.triu(dA.T[:n, :n]).contiguous()          # the (n, n) tensor whose column-major reading is R^T
    p.close()
    return Rt


def table_gesvj(ns, reps, warm):
    say("(i) qr_gesvj_dev on R^T of a uniform 4n x n matrix; torch.linalg on the same matrix as a comparator")
    say(f"{'n':>5} | {'sweeps':>6} {'launches':>8} | {'values ms (min / med)':>22} | {'with V ms (min / med)':>22} | {'torch svdvals ms':>16} | {'torch svd ms':>12}")
    for n in ns:
        Rt = triangle_t(n, 12)
        p = q.Plan(n, n, 0, 0)
        G, S, V = buf(n, n), buf(n, 1), buf(n, n)
        sw = [0]

        def load():
            G.copy_(Rt)

        def run(jobv):
            sw[0] = p.gesvj(jobv, G, n, n, n, S, V if jobv == "V" else None, n)

        t0 = timed(p, lambda: run("N"), reps, warm, before=load)
        t1 = timed(p, lambda: run("V"), reps, warm, before=load)
        _, rounds = q.jsvd_rounds(n)
        tv = tu = (float("nan"), float("nan"))
        M = Rt.T.contiguous()
        try:
            tv = timed_torch(lambda: torch.linalg.svdvals(M), reps, warm)
            tu = timed_torch(lambda: torch.linalg.svd(M, full_matrices=False), reps, warm)
        except Exception as e:      # a torch build without the solver: the comparator column stays empty
            say(f"      (torch.linalg not available here: {type(e).__name__})")
        say(f"{n:>5} | {sw[0]:>6} {sw[0] * rounds:>8} | {t0[0]:>10.3f} / {t0[1]:>9.3f} | {t1[0]:>10.3f} / {t1[1]:>9.3f} | {tv[1]:>16.3f} | {tu[1]:>12.3f}")
        p.close()


def table_gesvd(shapes, reps, warm):
    say("(ii) qr_gesvd_dev beside qr_geqrf_dev alone, same run (matrix resident, refilled before every call)")
    say(f"{'m':>7} {'n':>5} | {'geqrf ms (min / med)':>21} | {'values ms (min / med)':>22} | {'U and V ms (min / med)':>23} | sweeps")
    for m, n in shapes:
        p = q.Plan(m, n, 0, 0)
        dA, dtau, S, U, V = buf(m, n), buf(n, 1), buf(n, 1), buf(m, n), buf(n, n)
        sw = [0]

        def load():
            p.fill_uniform(dA, m, m, n, seed=12)
            p.sync()

        def run(ju, jv):
            sw[0] = p.gesvd(ju, jv, dA, m, n, m, dtau, S, U if ju == "U" else None, m, V if jv == "V" else None, n)

        tq = timed(p, lambda: p.geqrf(dA, m, n, m, dtau), reps, warm, before=load)
        t0 = timed(p, lambda: run("N", "N"), reps, warm, before=load)
        t1 = timed(p, lambda: run("U", "V"), reps, warm, before=load)
        say(f"{m:>7} {n:>5} | {tq[0]:>9.3f} / {tq[1]:>9.3f} | {t0[0]:>10.3f} / {t0[1]:>9.3f} | {t1[0]:>10.3f} / {t1[1]:>10.3f} | {sw[0]}")
        p.close()


def split_run():
    n = 512
    Rt = triangle_t(n, 12)
    p = q.Plan(n, n, 0, 0)
    G, S, V = buf(n, n), buf(n, 1), buf(n, n)
    G.copy_(Rt)
    torch.cuda.synchronize()
    sw = p.gesvj("V", G, n, n, n, S, V, n)
    p.sync()
    print(f"split run: n = {n}, {sw} sweeps")
    p.close()


def main():
    global _out
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--quick", action="store_true", help="n = 128, 512 and the 262144 x 512 shape only, 3 repeats")
    ap.add_argument("--split", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r11_svd_perf.txt"))
    a = ap.parse_args()
    if a.split:
        return split_run()
    reps, warm = (3, 1) if a.quick else (a.reps, 2)
    _out = open(a.out, "w")
    say(f"# Jacobi SVD (mi355x_qr.h section 7): python devtools/tools_svd_perf.py{' --quick' if a.quick else ''}; device: {q.device_info()}")
    say(f"# HIP events on the plan's stream, {warm} warm-up + {reps} timed calls each, min / median; the host waits once per sweep inside the timed region")
    table_gesvj((128, 512) if a.quick else (128, 256, 512, 1024), reps, warm)
    say("")
    table_gesvd(((262144, 512),) if a.quick else ((262144, 512), (16384, 1024)), reps, warm)
    _out.close()


if __name__ == "__main__":
    main()
