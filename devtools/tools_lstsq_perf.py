"""Least-squares solve timing table (mi355x_qr.h section 3): one command, HIP events on the plan's stream after warm-up.

  (i)   qr_ormqr_dev('T') at 16384^2 and 262144 x 512, T prebuilt, skinny (VALU) route against the MFMA route
        (lab knob MI355XQR_SOLVE_ROUTE), ms and effective GB/s over the compulsory bytes (see ormqr_bytes)
  (ii)  qr_solve_r_dev at n = 4096, 16384, both routes
  (iii) qr_gels_dev against qr_geqrf_dev alone at 4096^2, 16384^2, 262144 x 512

Loads the lab library (CUDA_QR_AMD_LIB=lab, set here) for the route knob.  Usage: python devtools/tools_lstsq_perf.py [--reps K] [--quick]
"""
import os
import sys

os.environ["CUDA_QR_AMD_LIB"] = "lab"
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import argparse  # noqa: E402

import torch  # noqa: E402

import cuda_qr_amd as q  # noqa: E402

NRHS = (1, 4, 16, 32, 64, 256)


def ormqr_bytes(m, n, nb, nrhs):
    """compulsory HBM bytes of Q^T C: V read once, 8 (m n - n^2 / 2), plus C (the panel's mk rows) read and written once per panel"""
    v = 8.0 * (m * n - n * n / 2.0)
    c = sum(16.0 * (m - k) * nrhs for k in range(0, n, nb))
    return v + c


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


def factored(m, n, seed=12):
    p = q.Plan(m, n, 0, 0)
    dA = torch.empty((n, m), dtype=torch.float64, device="cuda")
    dtau = torch.empty(n, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    p.fill_uniform(dA, m, m, n, seed=seed)
    p.geqrf(dA, m, n, m, dtau)
    p.sync()
    return p, dA, dtau


def ormqr_table(reps, warm, shapes, nrhs_set):
    print("(i) qr_ormqr_dev('T'), T prebuilt")
    print(f"{'m':>7} {'n':>6} {'nb':>4} {'nrhs':>5} | {'skinny ms':>9} {'GB/s':>6} | {'gemm ms':>8} {'GB/s':>6} | gemm/skinny")
    for m, n in shapes:
        p, dA, dtau = factored(m, n)
        nb = p.nb
        dT = torch.empty((n, nb), dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        p.build_t(dA, m, n, m, dtau, dT, nb)
        p.sync()
        for nrhs in nrhs_set:
            C = torch.rand((nrhs, m), dtype=torch.float64, device="cuda")
            torch.cuda.synchronize()
            res = {}
            for r in ("skinny", "gemm"):
                route(r)
                res[r] = timed(p, lambda: p.ormqr("T", dA, m, n, m, dtau, C, nrhs, m, dT=dT, ldt=nb), reps, warm)
            route("")
            gb = ormqr_bytes(m, n, nb, nrhs) / 1e9
            print(f"{m:>7} {n:>6} {nb:>4} {nrhs:>5} | {res['skinny']:>9.3f} {gb / res['skinny'] * 1e3:>6.0f} | {res['gemm']:>8.3f} "
                  f"{gb / res['gemm'] * 1e3:>6.0f} | {res['gemm'] / res['skinny']:>5.2f}x", flush=True)
            del C
        p.close()
        del dA, dT, dtau
        torch.cuda.empty_cache()


def solve_r_table(reps, warm, sizes, nrhs_set):
    print("(ii) qr_solve_r_dev")
    print(f"{'n':>6} {'nrhs':>5} | {'skinny ms':>9} | {'gemm ms':>8}")
    for n in sizes:
        p, dA, dtau = factored(n, n)
        for nrhs in nrhs_set:
            B0 = torch.rand((nrhs, n), dtype=torch.float64, device="cuda")
            B = B0.clone()
            res = {}
            for r in ("skinny", "gemm"):
                route(r)
                res[r] = timed(p, lambda: p.solve_r(dA, n, n, B, nrhs, n), reps, warm, before=lambda: B.copy_(B0))
            route("")
            print(f"{n:>6} {nrhs:>5} | {res['skinny']:>9.3f} | {res['gemm']:>8.3f}", flush=True)
        p.close()
        del dA, dtau
        torch.cuda.empty_cache()


def gels_table(reps, warm, shapes, nrhs_set):
    print("(iii) qr_gels_dev against qr_geqrf_dev alone (library's routes)")
    print(f"{'m':>7} {'n':>6} {'nrhs':>5} | {'geqrf ms':>8} | {'gels ms':>8} | gels/geqrf")
    for m, n in shapes:
        p = q.Plan(m, n, 0, 0)
        dA = torch.empty((n, m), dtype=torch.float64, device="cuda")
        dtau = torch.empty(n, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        fill = lambda: (p.fill_uniform(dA, m, m, n, seed=12), p.sync())  # noqa: E731
        t_qr = timed(p, lambda: p.geqrf(dA, m, n, m, dtau), reps, warm, before=fill)
        for nrhs in nrhs_set:
            B0 = torch.rand((nrhs, m), dtype=torch.float64, device="cuda")
            B = B0.clone()
            t_ls = timed(p, lambda: p.gels(dA, m, n, m, dtau, B, nrhs, m), reps, warm, before=lambda: (fill(), B.copy_(B0)))
            print(f"{m:>7} {n:>6} {nrhs:>5} | {t_qr:>8.2f} | {t_ls:>8.2f} | {t_ls / t_qr:>5.3f}", flush=True)
        p.close()
        del dA, dtau
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--quick", action="store_true", help="small shapes only (a check that the tool runs)")
    ap.add_argument("--part", default="all", choices=("all", "ormqr", "solve_r", "gels"))
    a = ap.parse_args()
    if a.quick:
        shapes, sizes, gshapes, nr = [(2048, 512)], [1024], [(2048, 512)], (1, 16, 64)
    else:
        shapes, sizes, gshapes, nr = [(16384, 16384), (262144, 512)], [4096, 16384], [(4096, 4096), (16384, 16384), (262144, 512)], NRHS
    name = q.device_info()["arch"]
    print(f"device {name}; median of {a.reps} after {a.warmup} warm-up calls, HIP events on the plan's stream")
    if a.part in ("all", "ormqr"):
        ormqr_table(a.reps, a.warmup, shapes, nr)
    if a.part in ("all", "solve_r"):
        solve_r_table(a.reps, a.warmup, sizes, nr)
    if a.part in ("all", "gels"):
        gels_table(a.reps, a.warmup, gshapes, (1, 16, 64))


if __name__ == "__main__":
    main()
