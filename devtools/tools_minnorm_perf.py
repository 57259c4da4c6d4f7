"""Minimum-norm solve timing table (mi355x_qr.h section 5): one command, HIP events on the plan's stream after warm-up.

  (i)   qr_solve_rt_dev next to qr_solve_r_dev at n = 4096, 16384, the library's route for each nrhs (the other route with --routes)
  (ii)  qr_transpose_dev in GB/s over 2 rows cols 8 bytes, next to the per-element qrd_transpose and qr_probe_copy_gbps
  (iii) qr_gels_t_dev and qr_gels_wide_dev against qr_geqrf_dev alone, same plan

Writes the table to --out (default profiles/r09_minnorm_perf.txt) as well as to the terminal.  Loads the lab library
(CUDA_QR_AMD_LIB=lab, set here) for the route knob.  Usage: python devtools/tools_minnorm_perf.py [--reps K] [--quick] [--routes]
"""
import os
import sys

os.environ["CUDA_QR_AMD_LIB"] = "lab"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import argparse  # noqa: E402

import torch  # noqa: E402

import cuda_qr_amd as q  # noqa: E402

NRHS = (1, 4, 16, 64, 256)
_out = None


def say(line):
    print(line, flush=True)
    if _out:
        _out.write(line + "\n")
        _out.flush()


def timed(p, fn, reps, warm, before=None):
    """median ms of fn() between two HIP events on the plan's stream; before() (untimed) runs ahead of every call"""
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
    return out[len(out) // 2]


def route(name):
    os.environ["MI355XQR_SOLVE_ROUTE"] = name


def buf(rows, cols):
    t = torch.empty((cols, rows), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    return t


def solve_table(reps, warm, sizes, nrhs_set, routes):
    say("(i) qr_solve_rt_dev (R^T X = B) next to qr_solve_r_dev (R X = B), same factors, same run")
    hdr = f"{'n':>6} {'nrhs':>5} | {'solve_r ms':>10} | {'solve_rt ms':>11} | rt/r"
    if routes:
        hdr += f" | {'r skinny':>8} {'r gemm':>8} | {'rt skinny':>9} {'rt gemm':>8}"
    say(hdr)
    for n in sizes:
        p = q.Plan(n, n, 0, 0)
        dA, dtau = buf(n, n), buf(n, 1)
        p.fill_uniform(dA, n, n, n, seed=12)
        p.geqrf(dA, n, n, n, dtau)
        p.sync()
        for nrhs in nrhs_set:
            B0 = torch.rand((nrhs, n), dtype=torch.float64, device="cuda")
            B = B0.clone()
            reset = lambda: B.copy_(B0)  # noqa: E731
            t_r = timed(p, lambda: p.solve_r(dA, n, n, B, nrhs, n), reps, warm, before=reset)
            t_rt = timed(p, lambda: p.solve_rt(dA, n, n, B, nrhs, n), reps, warm, before=reset)
            line = f"{n:>6} {nrhs:>5} | {t_r:>10.3f} | {t_rt:>11.3f} | {t_rt / t_r:>4.2f}"
            if routes:
                res = {}
                for r in ("skinny", "gemm"):
                    route(r)
                    res["r" + r] = timed(p, lambda: p.solve_r(dA, n, n, B, nrhs, n), reps, warm, before=reset)
                    res["t" + r] = timed(p, lambda: p.solve_rt(dA, n, n, B, nrhs, n), reps, warm, before=reset)
                route("")
                line += f" | {res['rskinny']:>8.3f} {res['rgemm']:>8.3f} | {res['tskinny']:>9.3f} {res['tgemm']:>8.3f}"
            say(line)
        p.close()
        del dA, dtau
        torch.cuda.empty_cache()


def transpose_table(reps, warm, shapes):
    copy = q.probe_copy_gbps()
    say(f"(ii) qr_transpose_dev, GB/s over 2 rows cols 8 bytes; qr_probe_copy_gbps = {copy:.0f} GB/s")
    say(f"{'rows':>6} {'cols':>6} | {'tiled ms':>8} {'GB/s':>6} {'of copy':>7} | {'per-element ms':>14} {'GB/s':>6} | speed-up")
    p = q.Plan(64, 32, 0, 0)
    for rows, cols in shapes:
        S, D = buf(rows, cols), buf(cols, rows)
        p.fill_uniform(S, rows, rows, cols, seed=3)
        p.sync()
        t_new = timed(p, lambda: p.transpose(S, rows, cols, rows, D, cols), reps, warm)
        t_old = timed(p, lambda: q.check(q.lib.qrd_transpose(p.stream, rows, cols, S.data_ptr(), rows, D.data_ptr(), cols)), reps, warm)
        gb = 2.0 * rows * cols * 8 / 1e9
        say(f"{rows:>6} {cols:>6} | {t_new:>8.3f} {gb / t_new * 1e3:>6.0f} {gb / t_new * 1e3 / copy:>7.2f} | {t_old:>14.3f} "
            f"{gb / t_old * 1e3:>6.0f} | {t_old / t_new:>5.1f}x")
        del S, D
        torch.cuda.empty_cache()
    p.close()


def gels_table(reps, warm, shapes, nrhs_set):
    say("(iii) qr_gels_t_dev and qr_gels_wide_dev (on the wide twin n x m, transpose included) against qr_geqrf_dev alone, same plan")
    say(f"{'m':>7} {'n':>6} {'nrhs':>5} | {'geqrf ms':>8} | {'gels_t ms':>9} {'/geqrf':>6} | {'gels_wide ms':>12} {'/geqrf':>6}")
    for m, n in shapes:
        p = q.Plan(m, n, 0, 0)
        dA, dW, dtau = buf(m, n), buf(n, m), buf(n, 1)
        p.fill_uniform(dW, n, n, m, seed=12)             # the wide twin; dA = its transpose, so both paths factor the same matrix
        p.sync()
        fill = lambda: (p.transpose(dW, n, m, n, dA, m), p.sync())  # noqa: E731
        t_qr = timed(p, lambda: p.geqrf(dA, m, n, m, dtau), reps, warm, before=fill)
        for nrhs in nrhs_set:
            B0 = torch.rand((nrhs, m), dtype=torch.float64, device="cuda")
            B = B0.clone()
            t_t = timed(p, lambda: p.gels_t(dA, m, n, m, dtau, B, nrhs, m), reps, warm, before=lambda: (fill(), B.copy_(B0)))
            t_w = timed(p, lambda: p.gels_wide(dW, n, m, n, dA, m, dtau, B, nrhs, m), reps, warm, before=lambda: B.copy_(B0))
            say(f"{m:>7} {n:>6} {nrhs:>5} | {t_qr:>8.2f} | {t_t:>9.2f} {t_t / t_qr:>6.3f} | {t_w:>12.2f} {t_w / t_qr:>6.3f}")
        p.close()
        del dA, dW, dtau
        torch.cuda.empty_cache()


def main():
    global _out
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--quick", action="store_true", help="small shapes only (a check that the tool runs)")
    ap.add_argument("--routes", action="store_true", help="also time both routes of both triangular solves (lab knob MI355XQR_SOLVE_ROUTE)")
    ap.add_argument("--part", default="all", choices=("all", "solve", "transpose", "gels"))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r09_minnorm_perf.txt"))
    a = ap.parse_args()
    if a.quick:
        sizes, tshapes, gshapes, nr = [1024], [(1000, 3000)], [(2048, 512)], (1, 16, 65)
    else:
        sizes, tshapes, gshapes, nr = [4096, 16384], [(16384, 16384), (4096, 65536), (65536, 512)], [(16384, 16384), (262144, 512)], NRHS
    if a.out:
        _out = open(a.out, "w")
    say(f"device {q.device_info()['arch']}; median of {a.reps} after {a.warmup} warm-up calls, HIP events on the plan's stream")
    if a.part in ("all", "solve"):
        solve_table(a.reps, a.warmup, sizes, nr, a.routes)
    if a.part in ("all", "transpose"):
        transpose_table(a.reps, a.warmup, tshapes)
    if a.part in ("all", "gels"):
        gels_table(a.reps, a.warmup, gshapes, (1, 16))
    if _out:
        _out.close()


if __name__ == "__main__":
    main()
