"""Batched QR / least squares: time per call against torch.geqrf, a loop of qr_geqrf_dev and the memory floor.

Writes profiles/r13_batched_perf.txt.  HIP events on the plan's stream (the library's own timing events), one warm-up call, the minimum
of 5 timed calls; the comparators run on the same GPU in the same process:
  torch.geqrf on the whole batch (torch's stream, torch events);
  qr_geqrf_dev on 64 of the matrices, one call each on a plan of the matrix's shape, scaled to the batch;
  the memory floor 2 * 8 * m * n * batch bytes (every matrix read once and written once) at the rate qr_probe_copy_gbps reports.
No ratio is a pass condition: the file records what was measured.

    python devtools/tools_batched_perf.py [--max-bytes 2e9]
"""
import argparse
import ctypes as C
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import cuda_qr_amd as qr  # noqa: E402

SHAPES = [(16, 8), (32, 16), (64, 32), (128, 32), (256, 64), (512, 32)]
BATCHES = (1000, 100000)
REPS = 5
_vp = C.c_void_p
for name, args in (("qrd_event_create_timing", [C.POINTER(_vp)]), ("qrd_event_record", [_vp, _vp]), ("qrd_event_sync", [_vp]),
                   ("qrd_event_elapsed_ms", [_vp, _vp, C.POINTER(C.c_float)]), ("qrd_event_destroy", [_vp])):
    f = getattr(qr.lib, name)
    f.restype, f.argtypes = C.c_int, args


def flops(m, n):
    return 2.0 * m * n * n - 2.0 * n ** 3 / 3.0


class Timer:
    """min over REPS of the time between two events on the plan's stream, after one warm-up"""

    def __init__(self, plan):
        self.s = plan.stream
        self.e0, self.e1 = _vp(), _vp()
        qr.check(qr.lib.qrd_event_create_timing(C.byref(self.e0)))
        qr.check(qr.lib.qrd_event_create_timing(C.byref(self.e1)))

    def __call__(self, reset, call):
        best = float("inf")
        for r in range(-1, REPS):
            reset()
            torch.cuda.synchronize()
            qr.check(qr.lib.qrd_event_record(self.e0, self.s))
            call()
            qr.check(qr.lib.qrd_event_record(self.e1, self.s))
            qr.check(qr.lib.qrd_event_sync(self.e1))
            ms = C.c_float()
            qr.check(qr.lib.qrd_event_elapsed_ms(self.e0, self.e1, C.byref(ms)))
            if r >= 0:
                best = min(best, ms.value)
        return best


def torch_ms(A0):
    best = float("inf")
    for r in range(-1, REPS):
        A = A0.clone()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        torch.geqrf(A)
        e1.record()
        e1.synchronize()
        if r >= 0:
            best = min(best, e0.elapsed_time(e1))
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--max-bytes", type=float, default=2e9, help="largest batch buffer; a batch that does not fit is cut down")
    args = ap.parse_args()
    gbps = qr.probe_copy_gbps()
    lines = [f"batched QR on {qr.device_info()}: min of {REPS} after a warm-up, HIP events; copy rate {gbps:.0f} GB/s (qr_probe_copy_gbps)",
             "trailing update shipped: rank-1 (one wave per column), no MFMA blocks",
             f"{'shape':>9} {'batch':>7} {'ms':>9} {'GFLOP/s':>9} {'torch ms':>9} {'x torch':>8} {'loop ms':>10} {'x loop':>8} {'floor ms':>9} {'of floor':>8}"]
    plan = qr.Plan(64, 8, 0, 0)
    timer = Timer(plan)
    g = torch.Generator(device="cuda").manual_seed(13)
    for m, n in SHAPES:
        for want in BATCHES:
            batch = int(min(want, args.max_bytes // (8 * m * n)))
            A0 = torch.randn((batch, n, m), dtype=torch.float64, device="cuda", generator=g)      # packed column-major matrices
            dA, dtau = A0.clone(), torch.zeros((batch, n), dtype=torch.float64, device="cuda")
            ms = timer(lambda: dA.copy_(A0), lambda: plan.geqrf_batched(dA, m, n, m, m * n, dtau, n, batch))
            t_ms = torch_ms(A0.transpose(1, 2))        # (batch, m, n) views of the same data
            p1 = qr.Plan(m, n, 0, 0)
            t1 = Timer(p1)
            k = min(64, batch)
            d1, tau1 = A0[:k].clone(), torch.zeros((k, n), dtype=torch.float64, device="cuda")

            def loop():
                for q in range(k):
                    p1.geqrf(d1[q], m, n, m, tau1[q])

            loop_ms = t1(lambda: d1.copy_(A0[:k]), loop) * batch / k
            p1.close()
            floor_ms = 2 * 8 * m * n * batch / (gbps * 1e9) * 1e3
            lines.append(f"{m:>5}x{n:<3} {batch:>7} {ms:>9.4f} {flops(m, n) * batch / ms / 1e6:>9.1f} {t_ms:>9.3f} {t_ms / ms:>8.2f} "
                         f"{loop_ms:>10.2f} {loop_ms / ms:>8.1f} {floor_ms:>9.4f} {floor_ms / ms:>8.3f}")
            print(lines[-1], flush=True)
    # the fused least squares
    m, n, nrhs = 64, 29, 3
    for want in BATCHES:
        batch = int(min(want, args.max_bytes // (8 * m * (n + nrhs))))
        A0 = torch.randn((batch, n, m), dtype=torch.float64, device="cuda", generator=g)
        B0 = torch.randn((batch, nrhs, m), dtype=torch.float64, device="cuda", generator=g)
        dA, dB, dtau = A0.clone(), B0.clone(), torch.zeros((batch, n), dtype=torch.float64, device="cuda")
        dinfo = torch.zeros(batch, dtype=torch.int32, device="cuda")

        def reset():
            dA.copy_(A0)
            dB.copy_(B0)

        ms = timer(reset, lambda: plan.gels_batched(dA, m, n, m, m * n, dtau, n, dB, nrhs, m, m * nrhs, dinfo, batch))
        floor_ms = 2 * 8 * m * (n + nrhs) * batch / (gbps * 1e9) * 1e3
        lines.append(f"gels {m}x{n}, {nrhs} rhs (fused, one launch), batch {batch}: {ms:.4f} ms, floor {floor_ms:.4f} ms ({floor_ms / ms:.3f} of it)")
        print(lines[-1], flush=True)
    lines.append("where a shape is far from the floor the time is arithmetic and latency, not memory: the wave route spends a 6-step butterfly "
                 "per dot product, the workgroup route three barriers per column and a rank-1 update through LDS")
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "r13_batched_perf.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")
    plan.close()


if __name__ == "__main__":
    main()
