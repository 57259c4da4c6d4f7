"""isolated rate of the trailing update A2 -= V Wt^T (qrd_gemm_nt) at update shapes, on the whole chip or on a CU-masked stream:
   python devtools/tools_nt_lab.py [--cus FIRST,COUNT] 16384x16128x256 [more MxNxK]
   (--cus 32,224: the update stream's share of the two-stream schedule.  The lab library's knobs -- MI355XQR_NT_KEEP=0, MI355XQR_NT4=0 --
   are read once per process: one process per variant, CUDA_QR_AMD_LIB=lab)"""
import os as _os, sys as _sys
_sys.path.insert(0, _os.path.dirname(_os.path.dirname(_os.path.abspath(__file__))))
import sys, time, json, ctypes as C
import torch
import cuda_qr_amd as q

f = q.lib.qrd_gemm_nt
f.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p]
args = sys.argv[1:]
stream = C.c_void_p(None)
if args and args[0] == "--cus":
    first, count = (int(x) for x in args[1].split(","))
    q.lib.qrd_stream_create_cumask.argtypes = [C.POINTER(C.c_void_p), C.c_int, C.c_int]
    q.lib.qrd_stream_sync.argtypes = [C.c_void_p]
    q.check(q.lib.qrd_stream_create_cumask(C.byref(stream), first, count))
    args = args[2:]
if hasattr(q.lib, "qrd_gemm_nt4_occupancy"):        # lab library: workgroups per CU of the four instantiations (rag, keep)
    print(json.dumps({"nt4_workgroups_per_cu": {f"rag{r}_keep{l}": q.lib.qrd_gemm_nt4_occupancy(r, l) for r in (0, 1) for l in (0, 1)},
                      "MI355XQR_NT_KEEP": _os.environ.get("MI355XQR_NT_KEEP", "")}), flush=True)


def sync():
    q.check(q.lib.qrd_stream_sync(stream) if stream.value else q.lib.qrd_device_sync())


for spec in args:
    M, N, K = (int(x) for x in spec.split("x"))
    A = torch.rand((K, M), dtype=torch.float64, device="cuda")          # column-major M x K
    Bt = torch.rand((K, N), dtype=torch.float64, device="cuda")         # column-major N x K
    Cc = torch.rand((N, M), dtype=torch.float64, device="cuda")         # column-major M x N
    torch.cuda.synchronize()
    def run():
        q.check(f(stream, M, N, K, -1, A.data_ptr(), M, Bt.data_ptr(), N, Cc.data_ptr(), M, -1, None))
    run(); sync()
    best = 1e30
    for _ in range(3):
        t0 = time.perf_counter()
        for _ in range(10):
            run()
        sync()
        best = min(best, (time.perf_counter() - t0) / 10)
    print(json.dumps({"M": M, "N": N, "K": K, "ms": best * 1e3, "tflops": 2.0 * M * N * K / best / 1e12}), flush=True)
