"""isolated time of V*T (T upper triangular) at update shapes on a CU-masked stream like the update stream of the look-ahead schedule:
the general product (qrd_gemm_nn), the triangle-aware one on each tile (qrd_gemm_nn_tri_tile 44 / 22 / 11) and the built-in rule
(qrd_gemm_nn_tri).  Minimum of 3 x 10 launches each.
   python devtools/tools_vt_tri_lab.py [--cus 224] [--first 32] 16384x256 12288x256 8192x256 4096x256 8192x128"""
import os as _os, sys as _sys
_sys.path.insert(0, _os.path.dirname(_os.path.dirname(_os.path.abspath(__file__))))
import argparse, ctypes as C, time, json
import torch
import cuda_qr_amd as q

ap = argparse.ArgumentParser()
ap.add_argument("--cus", type=int, default=224)
ap.add_argument("--first", type=int, default=32)
ap.add_argument("shapes", nargs="+")
args = ap.parse_args()

lib = q.lib
q.check(lib.qrd_init(), "qrd_init")
lib.qrd_stream_create_cumask.argtypes = [C.POINTER(C.c_void_p), C.c_int, C.c_int]
lib.qrd_stream_sync.argtypes = [C.c_void_p]
lib.qrd_stream_destroy.argtypes = [C.c_void_p]
st = C.c_void_p()
if args.cus > 0:
    q.check(lib.qrd_stream_create_cumask(C.byref(st), args.first, args.cus))


def sync():
    q.check(lib.qrd_stream_sync(st) if st else lib.qrd_device_sync())


for spec in args.shapes:
    M, N = (int(x) for x in spec.split("x"))
    V = torch.rand((N, M), dtype=torch.float64, device="cuda")                    # column-major M x N
    T = torch.triu(torch.rand((N, N), dtype=torch.float64, device="cuda")).T.contiguous()   # column-major upper triangular
    outs = {}
    for name, tile in (("generic", -1), ("tri44", 44), ("tri22", 22), ("tri11", 11), ("rule", 0)):
        Cc = torch.empty((N, M), dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()

        def run():
            q.check(lib.qrd_gemm_nn_tri_tile(st, tile, M, N, N, V.data_ptr(), M, T.data_ptr(), N, Cc.data_ptr(), M))
        run(); sync()
        best = 1e30
        for _ in range(3):
            t0 = time.perf_counter()
            for _ in range(10):
                run()
            sync()
            best = min(best, (time.perf_counter() - t0) / 10)
        outs[name] = Cc
        print(json.dumps({"M": M, "N": N, "cus": args.cus, "path": name, "us": round(best * 1e6, 2),
                          "same_bits_as_generic": bool(torch.equal(Cc, outs["generic"]))}), flush=True)
if st:
    lib.qrd_stream_destroy(st)
