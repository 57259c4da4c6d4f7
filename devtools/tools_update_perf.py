"""Row-append update timing table (mi355x_qr.h section 6): HIP events on the plan's stream after warm-up.

  (i)   qr_tpqrt_dev at (n, p) = (512, 64), (4096, 64), (4096, P), (16384, P) beside the dense route it replaces in the same run: R and B
        copied into an (n + p) x n matrix and qr_geqrf_dev on it
  (ii)  the accumulator over 262144 x 512 with one right-hand side in chunks of 32768 and of 4096 rows beside one qr_gels_dev on the
        whole matrix in the same run (the chunks are resident: views of the matrix's rows, copied to a chunk buffer before each push)
  (iii) with --split: nothing is timed; the primitive runs a few times at (4096, P) so that
        `rocprofv3 --kernel-trace --stats -- python devtools/tools_update_perf.py --split` shows the split between tp_panel_kernel and
        tp_apply_kernel (a run of its own, no events)

Writes the table to --out (default profiles/r10_update_perf.txt) as well as to the terminal.  One process, one GPU; give each
invocation a time limit of its own (`timeout -k 10 600 python devtools/tools_update_perf.py`).
Usage: python devtools/tools_update_perf.py [--reps K] [--quick] [--split]
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


def buf(rows, cols):
    t = torch.empty((cols, rows), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    return t


def triangle(n, seed):
    """a well-conditioned upper triangle: R of a random 2n x n matrix, from the library itself"""
    p = q.Plan(2 * n, n, 0, 0)
    dA, dtau = buf(2 * n, n), buf(n, 1)
    p.fill_uniform(dA, 2 * n, 2 * n, n, seed=seed)
    p.geqrf(dA, 2 * n, n, 2 * n, dtau)
    p.sync()
    R = torch.triu(dA.T[:n, :n]).T.contiguous()        # (n, n) tensor holding R column-major
    p.close()
    return R


def primitive_table(reps, warm, shapes):
    say("(i) qr_tpqrt_dev beside the dense route (copy [R ; B] into an (n + p) x n matrix, qr_geqrf_dev), same run")
    say(f"{'n':>6} {'p':>5} | {'tpqrt ms':>9} | {'dense ms':>9} | tpqrt/dense")
    for n, p_ in shapes:
        R0 = triangle(n, n + p_)
        B0 = torch.rand((n, p_), dtype=torch.float64, device="cuda") - 0.5
        plan = q.Plan(n + p_, n, 0, 0)
        dR, dB, dT = buf(n, n), buf(p_, n), buf(32, n)
        dS, dtau = buf(n + p_, n), buf(n, 1)

        def load():
            dR.copy_(R0)
            dB.copy_(B0)

        def dense():
            S = dS.T
            S[:n].copy_(dR.T)
            S[n:].copy_(dB.T)
            torch.cuda.synchronize()

        t_tp = timed(plan, lambda: plan.tpqrt(dR, n, n, dB, p_, p_, dT, 32), reps, warm, before=load)

        def dense_before():
            load()
            dense()

        t_dn = timed(plan, lambda: plan.geqrf(dS, n + p_, n, n + p_, dtau), reps, warm, before=dense_before)
        say(f"{n:>6} {p_:>5} | {t_tp:>9.3f} | {t_dn:>9.3f} | {t_tp / t_dn:.2f}   (the dense route's copy is not in its time)")
        plan.close()


def accumulator_table(reps, warm, m, n, chunks):
    say(f"(ii) accumulator over {m} x {n}, one right-hand side, beside one qr_gels_dev on the whole matrix, same run")
    plan = q.Plan(m, n, 0, 0)
    dA0, dA, dB0, dB, dtau = buf(m, n), buf(m, n), buf(m, 1), buf(m, 1), buf(n, 1)
    plan.fill_uniform(dA0, m, m, n, seed=5)
    plan.fill_uniform(dB0, m, m, 1, seed=6)
    plan.sync()

    def load():
        dA.copy_(dA0)
        dB.copy_(dB0)

    t_gels = timed(plan, lambda: plan.gels(dA, m, n, m, dtau, dB, 1, m), reps, warm, before=load)
    say(f"qr_gels_dev whole matrix: {t_gels:.3f} ms")
    plan.close()
    for c in chunks:
        pc = q.Plan(max(c, n), n, 0, 0)
        acc = q.LsAccumulator(pc, n, 1)
        dX, dAc, dBc = buf(n, 1), buf(c, n), buf(c, 1)

        def run():
            # each chunk of the resident matrix is copied to the chunk buffer (the push uses its arguments as workspace)
            for r in range(0, m, c):
                h = min(c, m - r)
                dAc.T[:h].copy_(dA0.T[r:r + h])
                dBc.T[:h].copy_(dB0.T[r:r + h])
                torch.cuda.synchronize()
                acc.push(dAc, h, c, dBc, c)
            acc.solve(dX, n)

        def before():
            acc.reset()
            pc.sync()

        # the chunk copies run on torch's stream between the pushes, which events on the plan's stream would not see: wall time of the
        # whole loop, reported as such
        import time
        ts = []
        for i in range(warm + reps):
            before()
            t0 = time.perf_counter()
            run()
            pc.sync()
            if i >= warm:
                ts.append((time.perf_counter() - t0) * 1e3)
        ts.sort()
        t_acc = ts[len(ts) // 2]
        say(f"accumulator chunks of {c:>6}: {t_acc:.3f} ms wall (chunk copies included)   acc/gels {t_acc / t_gels:.2f}")
        acc.close()
        pc.close()


def split_run(n, p_):
    R0 = triangle(n, 3)
    plan = q.Plan(n, n, 0, 0)
    dR, dB, dT = buf(n, n), buf(p_, n), buf(32, n)
    for _ in range(5):
        dR.copy_(R0)
        dB.uniform_(-0.5, 0.5)
        torch.cuda.synchronize()
        plan.tpqrt(dR, n, n, dB, p_, p_, dT, 32)
        plan.sync()
    plan.close()


def main():
    global _out
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--quick", action="store_true", help="small shapes only (a check that the tool runs)")
    ap.add_argument("--split", action="store_true", help="only run the primitive a few times, for rocprofv3 --kernel-trace --stats")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r10_update_perf.txt"))
    a = ap.parse_args()
    P = q.tpqrt_max_rows()
    if a.split:
        split_run(4096, P)
        return
    _out = open(a.out, "w")
    say(f"device: {q.device_info()}   qr_tpqrt_max_rows() = {P}")
    if a.quick:
        primitive_table(a.reps, a.warmup, [(512, 64)])
        accumulator_table(a.reps, a.warmup, 16384, 256, (4096, 128))
    else:
        primitive_table(a.reps, a.warmup, [(512, 64), (4096, 64), (4096, P), (16384, P)])
        accumulator_table(a.reps, a.warmup, 262144, 512, (32768, 4096))
    _out.close()


if __name__ == "__main__":
    main()
