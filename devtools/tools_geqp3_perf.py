#!/usr/bin/env python3
"""Pivoted against unpivoted QR, and the pivoted against the full-rank least-squares solve, event-timed on the plan's stream.

    python devtools/tools_geqp3_perf.py [--reps 7] [--shapes 1024x1024,4096x4096,...] > profiles/r08_geqp3_perf.txt

One process, warm-up run first, median of --reps runs.  The inputs are uniform [0, 1) (the generator of bench.py).  qr_geqp3_dev waits for
the device once per panel, so its event time includes those round trips -- as a caller sees it.  For the per-kernel split run the script
under `rocprofv3 --kernel-trace --stats -- python devtools/tools_geqp3_perf.py --reps 1 --shapes 4096x4096` (a run of its own): the
pv_gemv_kernel row is the hot matrix-vector product, and the bytes it must read are printed here as `gemv_bytes`.
With CUDA_QR_AMD_LIB=lab, MI355XQR_PIVOT_NB=<16..128> sets the panel width (the measurement behind the default).
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import cuda_qr_amd as qr  # noqa: E402


def timed(plan, fn, reps):
    s = torch.cuda.ExternalStream(plan.stream)
    ms = []
    for i in range(reps + 1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        prep = fn(None)
        plan.sync()
        e0.record(s)
        fn(prep)
        e1.record(s)
        plan.sync()
        if i:
            ms.append(e0.elapsed_time(e1))
    return statistics.median(ms), min(ms), max(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--shapes", default="1024x1024,4096x4096,8192x2048,16384x512,65536x128")
    a = ap.parse_args()
    print(f"# device {qr.device_info()}  copy {qr.probe_copy_gbps():.0f} GB/s  panel width {os.environ.get('MI355XQR_PIVOT_NB', 'default')}")
    print("# shape  geqrf_ms  geqp3_ms (min..max)  ratio  gemv_bytes_GB  gels_1/gelsp_1_ms  gels_16/gelsp_16_ms")
    for shp in a.shapes.split(","):
        m, n = (int(x) for x in shp.split("x"))
        p = qr.Plan(m, n, 0, 0)
        src, dA, dtau = qr.colmajor(m, n), qr.colmajor(m, n), qr.colmajor(n, 1)
        dj = torch.zeros(n, dtype=torch.int32, device="cuda")
        p.fill_uniform(src, m, m, n, seed=12)
        p.sync()

        def fresh(_):
            dA.copy_(src)
            torch.cuda.synchronize()

        def run_geqrf(prep):
            if prep is None:
                fresh(0)
                return 1
            p.geqrf(dA, m, n, m, dtau)

        def run_geqp3(prep):
            if prep is None:
                fresh(0)
                return 1
            p.geqp3(dA, m, n, m, dj, dtau)

        t_qr = timed(p, run_geqrf, a.reps)
        t_pv = timed(p, run_geqp3, a.reps)
        gemv_bytes = sum(8.0 * (m - c) * (n - (c // 128) * 128) for c in range(n))
        cols = []
        for nrhs in (1, 16):
            dB0, dB = qr.colmajor(m, nrhs), qr.colmajor(m, nrhs)
            p.fill_uniform(dB0, m, m, nrhs, seed=5)
            p.sync()

            def run_gels(prep, piv=False):
                if prep is None:
                    fresh(0)
                    dB.copy_(dB0)
                    torch.cuda.synchronize()
                    return 1
                if piv:
                    p.gelsp(dA, m, n, m, dj, dtau, dB, nrhs, m)
                else:
                    p.gels(dA, m, n, m, dtau, dB, nrhs, m)

            g = timed(p, run_gels, a.reps)[0]
            gp = timed(p, lambda prep: run_gels(prep, True), a.reps)[0]
            cols.append(f"{g:.3f}/{gp:.3f}")
        print(f"{m}x{n}  {t_qr[0]:.3f}  {t_pv[0]:.3f} ({t_pv[1]:.3f}..{t_pv[2]:.3f})  {t_pv[0] / t_qr[0]:.1f}x  {gemv_bytes / 1e9:.1f}  "
              f"{cols[0]}  {cols[1]}", flush=True)
        p.close()


if __name__ == "__main__":
    main()
