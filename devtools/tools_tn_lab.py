"""isolated rate of the wide TN product Wt = A2^T (V T) (qrd_gemm_tn_update) at update shapes, on the whole chip or on a CU-masked
stream like the update stream of the look-ahead schedule (CUs [first, first + cus)):
   python devtools/tools_tn_lab.py [--cus 224] [--first 32] [--lda 16384] [--cap 16777216] [--even] 15872x256x16128 [more MxNxK]
   (M = columns of A2, N = nb, K = panel height; --lda: A2's leading dimension, default K)
--even: after the library's own choice (qrd_gemm_tn_update: the split-K rule when run as CUDA_QR_AMD_LIB=lab MI355XQR_TN_EVEN=0), also
the even static K split (qrd_gemm_tn_update_even) on one and on two workgroups per slot, in the same process, and the largest
difference of the results."""
import os as _os, sys as _sys
_sys.path.insert(0, _os.path.dirname(_os.path.dirname(_os.path.abspath(__file__))))
import argparse, ctypes as C, time, json
import torch
import cuda_qr_amd as q

ap = argparse.ArgumentParser()
ap.add_argument("--cus", type=int, default=0)
ap.add_argument("--first", type=int, default=32)
ap.add_argument("--lda", type=int, default=0)
ap.add_argument("--cap", type=int, default=1 << 24)
ap.add_argument("--even", action="store_true")
ap.add_argument("shapes", nargs="+")
args = ap.parse_args()

lib = q.lib
lib.qrd_stream_create_cumask.argtypes = [C.POINTER(C.c_void_p), C.c_int, C.c_int]
lib.qrd_stream_sync.argtypes = [C.c_void_p]
lib.qrd_stream_destroy.argtypes = [C.c_void_p]
lib.qrd_stream_cus.argtypes = [C.c_void_p]
st = C.c_void_p()
if args.cus > 0:
    q.check(lib.qrd_stream_create_cumask(C.byref(st), args.first, args.cus))
slots = 2 * lib.qrd_stream_cus(st)


def sync():
    q.check(lib.qrd_stream_sync(st) if st else lib.qrd_device_sync())


for spec in args.shapes:
    M, N, K = (int(x) for x in spec.split("x"))
    lda = args.lda if args.lda >= K else K
    A = torch.rand((M, lda), dtype=torch.float64, device="cuda")        # column-major lda x M, K rows used
    B = torch.rand((N, K), dtype=torch.float64, device="cuda")          # column-major K x N
    slabs = torch.empty(args.cap, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    variants = [("update", None)] + ([("even", 0), ("even_2x", 2 * slots)] if args.even else [])
    outs = {}
    for name, nwg in variants:
        Cc = torch.empty((N, M), dtype=torch.float64, device="cuda")    # column-major M x N
        torch.cuda.synchronize()
        if nwg is None:
            def run():
                q.check(lib.qrd_gemm_tn_update(st, M, N, K, 1.0, A.data_ptr(), lda, B.data_ptr(), K, 0.0, Cc.data_ptr(), M, slabs.data_ptr(), args.cap))
        else:
            def run():
                q.check(lib.qrd_gemm_tn_update_even(st, M, N, K, 1.0, A.data_ptr(), lda, B.data_ptr(), K, 0.0, Cc.data_ptr(), M, slabs.data_ptr(),
                                                    args.cap, nwg))
        n0 = lib.qrd_tn_even_launches() if hasattr(lib, "qrd_tn_even_launches") else 0
        run(); sync()
        took_even = (lib.qrd_tn_even_launches() if hasattr(lib, "qrd_tn_even_launches") else 0) - n0
        best = 1e30
        for _ in range(3):
            t0 = time.perf_counter()
            for _ in range(10):
                run()
            sync()
            best = min(best, (time.perf_counter() - t0) / 10)
        outs[name] = Cc
        rec = {"M": M, "N": N, "K": K, "lda": lda, "cus": slots // 2, "path": name, "even_split": bool(took_even), "ms": round(best * 1e3, 4),
               "tflops": round(2.0 * M * N * K / best / 1e12, 2)}
        if name != "update":
            rec["max_abs_diff_to_update"] = float((Cc - outs["update"]).abs().max())
        print(json.dumps(rec), flush=True)
if st:
    lib.qrd_stream_destroy(st)
