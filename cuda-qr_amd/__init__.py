"""cuda-qr_amd: thin ctypes binding over the C-ABI library libmi355xqr.so (include/mi355x_qr.h).

This Python layer is plumbing for tests and bench.py -- the product is the C library (C host layer
+ hand-written gfx950 HIP kernels).  There is NO CPU fallback: importing works anywhere the shared
library loads, but every compute entry point needs an MI355X and fails loudly otherwise.

The directory name has a hyphen (it mirrors the reference repo's name), so import it through the
root-level shim:  `import cuda_qr_amd`.
"""
import ctypes as C
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
# CUDA_QR_AMD_LIB=lab (this binding's own switch, not a library knob): load libmi355xqr_lab.so -- the same sources built with -DQR_LAB
# (`make -C cuda-qr_amd lab`), in which the measurement knobs are environment variables and the development entry points of the 32 x 32
# factor core exist.  For devtools/ scripts and the tests that force a schedule branch on a small matrix; everything else (bench.py,
# smoke(), the parity tests) runs the product library.
_which = os.environ.get("CUDA_QR_AMD_LIB", "")
LAB = _which == "lab" or _which.endswith(".so")        # (a path: an experimental build of the lab flavour, devtools/ A/Bs of two kernel versions)
LAB_LIB_PATH = os.path.join(HERE, "libmi355xqr_lab.so")
LIB_PATH = (os.path.join(HERE, _which) if _which.endswith(".so") else LAB_LIB_PATH) if LAB else os.path.join(HERE, "libmi355xqr.so")
HEADER = os.path.join(os.path.dirname(HERE), "include", "mi355x_qr.h")

if not os.path.exists(LIB_PATH):
    raise ImportError(
        f"{LIB_PATH} is missing: build it with `make -C {HERE} all lab` (or python -c 'import __graft_entry__ as g; "
        "g.build()').  The HIP extension is mandatory; there is no CPU fallback.")

# Load order matters when torch is used in the same process (every caller in this repo: device buffers are torch tensors): the torch
# wheel bundles its own libamdhip64, and whichever HIP runtime is mapped first serves both -- with the system one mapped first
# torch.cuda later reports "No HIP GPUs are available".  So torch goes first when it is installed (plumbing only: nothing below uses it).
try:
    import torch  # noqa: F401
except Exception:      # a host without torch: the binding works on raw device pointers
    pass

lib = C.CDLL(LIB_PATH)

QR_PROF_CLASSES = 4
QR_E_ARG = -101
QR_E_SINGULAR = -107
QR_E_NOCONV = -108
QR_E_NOTPD = -109
JSVD_BLOCK = 32         # QR_JSVD_BLOCK: the column-block width of the Jacobi schedule
JSVD_MAX_SWEEPS = 30    # QR_JSVD_MAX_SWEEPS
PROF_NAMES = ("update_nn", "vta_tn", "panel", "vt_misc")


class QRError(RuntimeError):
    def __init__(self, msg, status=0):
        super().__init__(msg)
        self.status = status


class Profile(C.Structure):
    _fields_ = [("ms", C.c_double * QR_PROF_CLASSES), ("flops", C.c_double * QR_PROF_CLASSES),
                ("bytes", C.c_double * QR_PROF_CLASSES), ("launches", C.c_longlong * QR_PROF_CLASSES)]


_dp = C.POINTER(C.c_double)
_vp = C.c_void_p


def _sig(name, restype, *argtypes):
    f = getattr(lib, name)
    f.restype = restype
    f.argtypes = list(argtypes)
    return f


_sig("getPanelDims", None, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int))
_sig("mmqr_status", C.c_int, _dp, C.POINTER(_dp), C.c_int, C.c_int)
_sig("mmqr", None, _dp, C.POINTER(_dp), C.c_int, C.c_int)
_sig("explicitQR_status", C.c_int, _dp, _dp, _dp, _dp, C.c_int, C.c_int)
_sig("explicitQR", None, _dp, _dp, _dp, _dp, C.c_int, C.c_int)
_sig("dgemm_status", C.c_int, _dp, _dp, _dp, C.c_int, C.c_int, C.c_int)
_sig("dgemm", None, _dp, _dp, _dp, C.c_int, C.c_int, C.c_int)
_sig("identity", None, _dp, C.c_int)
_sig("printMat", None, _dp, C.c_int, C.c_int)
_sig("getPanelDims_legacy", None, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int))
_sig("mmqr_legacy_status", C.c_int, _dp, C.POINTER(_dp), C.c_int, C.c_int, C.c_int, C.c_int)
_sig("explicitQR_legacy_status", C.c_int, _dp, _dp, _dp, _dp, C.c_int, C.c_int, C.c_int, C.c_int)
_sig("qr_strerror", C.c_char_p, C.c_int)
_sig("qr_set_block_size", C.c_int, C.c_int, C.c_int)
_sig("qr_get_block_size", None, C.POINTER(C.c_int), C.POINTER(C.c_int))
_sig("qr_default_block_size", C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int))
_sig("qr_thin", C.c_int, _dp, C.c_int, C.c_int, _dp, _dp, C.c_int, C.c_int)
_fp = C.POINTER(C.c_float)
_sig("mmqr_f32_status", C.c_int, _fp, C.POINTER(_fp), C.c_int, C.c_int)
_sig("explicitQR_f32_status", C.c_int, _fp, _fp, _fp, _fp, C.c_int, C.c_int)
_sig("qr_thin_mgpu", C.c_int, _dp, C.c_int, C.c_int, _dp, _dp, C.c_int, C.c_int)
_sig("qr_release_cached_plans", C.c_int)
_sig("qr_tsqr_unique_id", C.c_int, _vp)
_sig("qr_tsqr_plan_create", C.c_int, C.POINTER(_vp), _vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int)
_sig("qr_tsqr_plan_create_comm", C.c_int, C.POINTER(_vp), _vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int)
_sig("qr_tsqr_plan_destroy", C.c_int, _vp)
_sig("qr_tsqr_factor_dev", C.c_int, _vp, _vp, C.c_int, _vp)
_sig("qr_tsqr_formq_dev", C.c_int, _vp, _vp, C.c_int, _vp, C.c_int)
_sig("qr_tsqr_local_dev", C.c_int, _vp, _vp, C.c_int)
_sig("qr_tsqr_exchange_buffers", C.c_int, _vp, C.POINTER(_vp), C.POINTER(_vp))
_sig("qr_tsqr_stacked_dev", C.c_int, _vp, _vp)
_sig("qr_tsqr_is_pipelined", C.c_int, _vp)
_sig("qr_tsqr_set_schedule", C.c_int, _vp, C.c_int)
_sig("qr_tsqr_gather_stats", C.c_int, _vp, C.POINTER(C.c_double))
_sig("qr_tsqr_factor_virtual_dev", C.c_int, C.POINTER(_vp), C.c_int, C.POINTER(_vp), C.c_int, C.POINTER(_vp))
_sig("qr_tsqr_factor_selfgather_dev", C.c_int, _vp, _vp, C.c_int, _vp)
_sig("qr_tsqr_sync", C.c_int, _vp)
_sig("qr_tsqr_stream", _vp, _vp)
_sig("qr_tsqr_comm_ranks", C.c_int, _vp, C.POINTER(C.c_int))
_sig("qr_tsqr_local_plan", _vp, _vp)
_sig("qr_tsqr_stacked_plan", _vp, _vp)
_sig("qr_plan_create", C.c_int, C.POINTER(_vp), C.c_int, C.c_int, C.c_int, C.c_int)
_sig("qr_plan_destroy", C.c_int, _vp)
_sig("qr_geqrf_dev", C.c_int, _vp, _vp, C.c_int, C.c_int, C.c_int, _vp)
_sig("qr_applyq_dev", C.c_int, _vp, _vp, C.c_int, C.c_int, C.c_int, _vp, _vp, C.c_int, C.c_int, C.c_int)
_sig("qr_build_t_dev", C.c_int, _vp, _vp, C.c_int, C.c_int, C.c_int, _vp, _vp, C.c_int)
_sig("qr_ormqr_dev", C.c_int, _vp, C.c_char, _vp, C.c_int, C.c_int, C.c_int, _vp, _vp, C.c_int, _vp, C.c_int, C.c_int)
_sig("qr_solve_r_dev", C.c_int, _vp, _vp, C.c_int, C.c_int, _vp, C.c_int, C.c_int)
_sig("qr_gels_dev", C.c_int, _vp, _vp, C.c_int, C.c_int, C.c_int, _vp, _vp, C.c_int, C.c_int)
_sig("qr_lstsq", C.c_int, _dp, C.c_int, C.c_int, _dp, C.c_int, _dp, _dp)
_ip = C.POINTER(C.c_int)
_sig("qr_geqp3_dev", C.c_int, _vp, _vp, C.c_int, C.c_int, C.c_int, _vp, _vp)
_sig("qr_rank_dev", C.c_int, _vp, _vp, C.c_int, C.c_int, C.c_int, C.c_double, _ip)
_sig("qr_gelsp_dev", C.c_int, _vp, _vp, C.c_int, C.c_int, C.c_int, _vp, _vp, _vp, C.c_int, C.c_int, C.c_double, _vp, _ip)
_sig("qr_lstsq_pivoted", C.c_int, _dp, C.c_int, C.c_int, _dp, C.c_int, C.c_double, _dp, _dp, _ip, _ip)
_sig("qr_solve_rt_dev", C.c_int, _vp, _vp, C.c_int, C.c_int, _vp, C.c_int, C.c_int)
_sig("qr_minnorm_dev", C.c_int, _vp, _vp, C.c_int, C.c_int, C.c_int, _vp, _vp, C.c_int, _vp, C.c_int, C.c_int)
_sig("qr_gels_t_dev", C.c_int, _vp, _vp, C.c_int, C.c_int, C.c_int, _vp, _vp, C.c_int, C.c_int)
_sig("qr_transpose_dev", C.c_int, _vp, _vp, C.c_int, C.c_int, C.c_int, _vp, C.c_int)
_sig("qr_gels_wide_dev", C.c_int, _vp, _vp, C.c_int, C.c_int, C.c_int, _vp, C.c_int, _vp, _vp, C.c_int, C.c_int)
_sig("qr_lstsq_minnorm", C.c_int, _dp, C.c_int, C.c_int, _dp, C.c_int, _dp)
_sig("qr_tpqrt_max_rows", C.c_int)
_sig("qr_tpqrt_dev", C.c_int, _vp, _vp, C.c_int, C.c_int, _vp, C.c_int, C.c_int, _vp, C.c_int)
_sig("qr_tpmqrt_dev", C.c_int, _vp, C.c_char, _vp, C.c_int, C.c_int, C.c_int, _vp, C.c_int, _vp, C.c_int, _vp, C.c_int, C.c_int)
_sig("qr_lsacc_create", C.c_int, C.POINTER(_vp), _vp, C.c_int, C.c_int)
_sig("qr_lsacc_push_dev", C.c_int, _vp, _vp, C.c_int, C.c_int, _vp, C.c_int)
_sig("qr_lsacc_rows", C.c_int, _vp, C.POINTER(C.c_longlong))
_sig("qr_lsacc_factor_dev", C.c_int, _vp, C.POINTER(_vp), _ip, C.POINTER(_vp), _ip)
_sig("qr_lsacc_solve_dev", C.c_int, _vp, _vp, C.c_int, _vp)
_sig("qr_lsacc_reset", C.c_int, _vp)
_sig("qr_lsacc_destroy", C.c_int, _vp)
_sig("qr_lstsq_chunked", C.c_int, _dp, C.c_longlong, C.c_int, C.c_int, _dp, C.c_int, C.c_int, C.c_int, _dp, _dp)
_sig("qr_tphqrt_dev", C.c_int, _vp, _vp, C.c_int, C.c_int, _vp, C.c_int, C.c_int, C.c_int, _vp, C.c_int, _ip)
_sig("qr_tphmqrt_dev", C.c_int, _vp, _vp, C.c_int, C.c_int, C.c_int, C.c_int, _vp, C.c_int, _vp, C.c_int, _vp, C.c_int, C.c_int)
_sig("qr_lsacc_pop_dev", C.c_int, _vp, _vp, C.c_int, C.c_int, _vp, C.c_int)
_sig("qr_lsacc_slide_dev", C.c_int, _vp, _vp, C.c_int, C.c_int, _vp, C.c_int, _vp, C.c_int, C.c_int, _vp, C.c_int)
_sig("qr_lstsq_rolling", C.c_int, _dp, C.c_longlong, C.c_int, C.c_int, _dp, C.c_int, C.c_int, C.c_int, C.c_int, _dp, _dp)
_sig("qr_jsvd_rounds", C.c_int, C.c_int, _ip, _ip)
_sig("qr_jsvd_round_pairs", C.c_int, C.c_int, C.c_int, _ip, C.c_int)
_sig("qr_gesvj_dev", C.c_int, _vp, C.c_char, _vp, C.c_int, C.c_int, C.c_int, _vp, _vp, C.c_int, _ip)
_sig("qr_gesvd_dev", C.c_int, _vp, C.c_char, C.c_char, _vp, C.c_int, C.c_int, C.c_int, _vp, _vp, _vp, C.c_int, _vp, C.c_int, _ip)
_sig("qr_cond_dev", C.c_int, _vp, _vp, C.c_int, C.c_int, C.c_int, _vp, _dp)
_sig("qr_gelss_dev", C.c_int, _vp, _vp, C.c_int, C.c_int, C.c_int, _vp, _vp, C.c_int, C.c_int, C.c_double, _vp, _ip)
_sig("qr_svd", C.c_int, _dp, C.c_int, C.c_int, _dp, _dp, _dp)
_sig("qr_lstsq_svd", C.c_int, _dp, C.c_int, C.c_int, _dp, C.c_int, C.c_double, _dp, _dp, _ip, _dp)
_ll = C.c_longlong
_sig("qr_batched_max_rows", C.c_int, C.c_int)
_sig("qr_geqrf_batched_dev", C.c_int, _vp, _vp, C.c_int, C.c_int, C.c_int, _ll, _vp, _ll, C.c_int)
_sig("qr_ormqr_batched_dev", C.c_int, _vp, C.c_char, _vp, C.c_int, C.c_int, C.c_int, _ll, _vp, _ll, _vp, C.c_int, C.c_int, _ll, C.c_int)
_sig("qr_orgqr_batched_dev", C.c_int, _vp, _vp, C.c_int, C.c_int, C.c_int, _ll, _vp, _ll, _vp, C.c_int, _ll, C.c_int)
_sig("qr_gels_batched_dev", C.c_int, _vp, _vp, C.c_int, C.c_int, C.c_int, _ll, _vp, _ll, _vp, C.c_int, C.c_int, _ll, _vp, C.c_int)
_sig("qr_thin_batched", C.c_int, _dp, C.c_int, C.c_int, C.c_int, _dp, _dp)
_sig("qr_lstsq_batched", C.c_int, _dp, C.c_int, C.c_int, _dp, C.c_int, C.c_int, _dp, _dp, _ip)
_sig("qr_geqp3_batched_dev", C.c_int, _vp, _vp, C.c_int, C.c_int, C.c_int, _ll, _vp, _ll, _vp, _ll, C.c_int)
_sig("qr_rank_batched_dev", C.c_int, _vp, _vp, C.c_int, C.c_int, C.c_int, _ll, C.c_double, _vp, C.c_int)
for _name in ("qr_gelsp_batched_dev", "qr_gelsy_batched_dev"):
    _sig(_name, C.c_int, _vp, _vp, C.c_int, C.c_int, C.c_int, _ll, _vp, _ll, _vp, _ll, _vp, C.c_int, C.c_int, _ll, C.c_double, _vp, _vp, C.c_int)
_sig("qr_thin_pivoted_batched", C.c_int, _dp, C.c_int, C.c_int, C.c_int, _dp, _dp, _ip)
_sig("qr_lstsq_pivoted_batched", C.c_int, _dp, C.c_int, C.c_int, _dp, C.c_int, C.c_int, C.c_double, C.c_int, _dp, _dp, _ip, _ip)
_sig("qr_gesvd_batched_dev", C.c_int, _vp, C.c_char, C.c_char, _vp, C.c_int, C.c_int, C.c_int, _ll, _vp, _ll, _vp, _ll, _vp, _ll, _vp, C.c_int, _ll,
     _vp, C.c_int, _ll, _vp, _vp, _vp, C.c_int)
_sig("qr_svd_batched", C.c_int, _dp, C.c_int, C.c_int, C.c_int, _dp, _dp, _dp, _ip)
_sig("qr_tpqrt_batched_max_rows", C.c_int, C.c_int)
_sig("qr_tphqrt_batched_dev", C.c_int, _vp, _vp, C.c_int, C.c_int, _ll, _vp, C.c_int, C.c_int, C.c_int, _ll, _vp, _ll, _vp, C.c_int, _ll, _vp, C.c_int,
     _ll, C.c_int, _vp, C.c_int)
_sig("qr_tpqrt_batched_dev", C.c_int, _vp, _vp, C.c_int, C.c_int, _ll, _vp, C.c_int, C.c_int, _ll, _vp, _ll, _vp, C.c_int, _ll, _vp, C.c_int, _ll,
     C.c_int, C.c_int)
_sig("qr_tpmqrt_batched_dev", C.c_int, _vp, C.c_char, _vp, C.c_int, C.c_int, C.c_int, C.c_int, _ll, _vp, _ll, _vp, C.c_int, _ll, _vp, C.c_int, _ll,
     C.c_int, C.c_int)
_sig("qr_lsacc_batched_create", C.c_int, C.POINTER(_vp), _vp, C.c_int, C.c_int, C.c_int)
_sig("qr_lsacc_batched_push_dev", C.c_int, _vp, _vp, C.c_int, C.c_int, _ll, _vp, C.c_int, _ll)
_sig("qr_lsacc_batched_pop_dev", C.c_int, _vp, _vp, C.c_int, C.c_int, _ll, _vp, C.c_int, _ll, _vp)
_sig("qr_lsacc_batched_slide_dev", C.c_int, _vp, _vp, C.c_int, C.c_int, _ll, _vp, C.c_int, _ll, _vp, C.c_int, C.c_int, _ll, _vp, C.c_int, _ll, _vp)
_sig("qr_lsacc_batched_factor_dev", C.c_int, _vp, C.POINTER(_vp), _ip, C.POINTER(_ll), C.POINTER(_vp), _ip, C.POINTER(_ll), C.POINTER(_vp),
     C.POINTER(_vp))
_sig("qr_lsacc_batched_solve_dev", C.c_int, _vp, _vp, C.c_int, _ll, _vp, _ll, _vp)
_sig("qr_lsacc_batched_reset", C.c_int, _vp)
_sig("qr_lsacc_batched_destroy", C.c_int, _vp)
_sig("qr_lstsq_rolling_batched", C.c_int, _dp, C.c_int, C.c_int, _dp, C.c_int, C.c_int, C.c_int, C.c_int, _dp, _dp, _ip)
_sig("qr_minnorm_batched_dev", C.c_int, _vp, _vp, C.c_int, C.c_int, C.c_int, _ll, _vp, _ll, _vp, C.c_int, C.c_int, _ll, _vp, C.c_int)
_sig("qr_gels_t_batched_dev", C.c_int, _vp, _vp, C.c_int, C.c_int, C.c_int, _ll, _vp, _ll, _vp, C.c_int, C.c_int, _ll, _vp, C.c_int)
_sig("qr_transpose_batched_dev", C.c_int, _vp, _vp, C.c_int, C.c_int, C.c_int, _ll, _vp, C.c_int, _ll, C.c_int)
_sig("qr_gels_wide_batched_dev", C.c_int, _vp, _vp, C.c_int, C.c_int, C.c_int, _ll, _vp, C.c_int, _ll, _vp, _ll, _vp, C.c_int, C.c_int, _ll, _vp,
     C.c_int)
_sig("qr_lstsq_minnorm_batched", C.c_int, _dp, C.c_int, C.c_int, _dp, C.c_int, C.c_int, _dp, _ip)
_sig("qr_damped_batched_dev", C.c_int, _vp, _vp, C.c_int, C.c_int, _ll, _vp, C.c_int, C.c_int, _ll, _vp, _vp, _ll, _vp, _ll, _vp, C.c_int, _ll,
     C.c_int, _vp, C.c_int, _ll, _vp, _vp, _vp, C.c_int)
_sig("qr_gels_damped_batched_dev", C.c_int, _vp, _vp, C.c_int, C.c_int, C.c_int, _ll, _vp, _ll, _vp, C.c_int, C.c_int, _ll, _vp, _ll, _vp, C.c_int,
     _ll, _vp, C.c_int, _ll, _vp, _vp, _vp, C.c_int)
_sig("qr_gels_damped_wide_batched_dev", C.c_int, _vp, _vp, C.c_int, C.c_int, C.c_int, _ll, _vp, C.c_int, _ll, _vp, _ll, _vp, C.c_int, C.c_int, _ll,
     _vp, C.c_int, _ll, _vp, C.c_int, _ll, _vp, _vp, _vp, C.c_int)
_sig("qr_lsacc_batched_solve_damped_dev", C.c_int, _vp, _vp, _ll, _vp, C.c_int, _ll, _vp, C.c_int, _ll, _vp, _vp, _vp)
_sig("qr_lstsq_damped_batched", C.c_int, _dp, C.c_int, C.c_int, _dp, C.c_int, C.c_int, _dp, _dp, C.c_int, _dp, _dp, _dp, _ip)
_sig("qr_trust_batched_dev", C.c_int, _vp, _vp, C.c_int, C.c_int, _ll, _vp, C.c_int, _ll, _vp, _vp, _ll, _vp, _ll, _vp, _ll, _vp, _ll, C.c_double,
     C.c_int, C.c_int, _vp, C.c_int, _ll, _vp, _vp, _vp, _vp, _vp, _vp, C.c_int)
_sig("qr_gels_trust_batched_dev", C.c_int, _vp, _vp, C.c_int, C.c_int, C.c_int, _ll, _vp, _ll, _vp, C.c_int, _ll, _vp, _ll, _vp, _ll, _vp, _ll,
     C.c_double, C.c_int, _vp, C.c_int, _ll, _vp, _vp, _vp, _vp, _vp, _vp, C.c_int)
_sig("qr_gels_trust_wide_batched_dev", C.c_int, _vp, _vp, C.c_int, C.c_int, C.c_int, _ll, _vp, C.c_int, _ll, _vp, _ll, _vp, C.c_int, _ll, _vp, _ll,
     _vp, _ll, C.c_double, C.c_int, _vp, C.c_int, _ll, _vp, _vp, _vp, _vp, _vp, _vp, C.c_int)
_sig("qr_lsacc_batched_solve_trust_dev", C.c_int, _vp, _vp, _ll, _vp, _ll, _vp, _ll, C.c_double, C.c_int, _vp, C.c_int, _ll, _vp, _vp, _vp, _vp,
     _vp, _vp)
_sig("qr_lstsq_trust_batched", C.c_int, _dp, C.c_int, C.c_int, _dp, C.c_int, _dp, _dp, _dp, C.c_double, C.c_int, _dp, _dp, _dp, _dp, _ip, _ip, _ip)
_sig("qr_gglse_batched_max_rows", C.c_int, C.c_int, C.c_int, C.c_int)
_sig("qr_gglse_batched_dev", C.c_int, _vp, _vp, C.c_int, C.c_int, C.c_int, _ll, _vp, C.c_int, C.c_int, _ll, _vp, C.c_int, _ll, _vp, C.c_int, _ll,
     C.c_int, _vp, C.c_int, _ll, _vp, C.c_int, _ll, _vp, _ll, _vp, C.c_int)
_sig("qr_lstsq_constrained_batched", C.c_int, _dp, C.c_int, C.c_int, _dp, C.c_int, _dp, _dp, C.c_int, C.c_int, _dp, _dp, _dp, _ip)
_sig("qr_bvls_batched_max_rows", C.c_int, C.c_int)
_sig("qr_bvls_batched_dev", C.c_int, _vp, _vp, C.c_int, C.c_int, C.c_int, _ll, _vp, _ll, _vp, _vp, _ll, C.c_int, _vp, _ll, _vp, _ll, _vp, _ll, _vp, _vp,
     _vp, C.c_int)
_sig("qr_lstsq_bounded_batched", C.c_int, _dp, C.c_int, C.c_int, _dp, _dp, _dp, C.c_int, C.c_int, _dp, _dp, _ip, _dp, _ip, _ip)
_sig("qr_lsei_batched_max_rows", C.c_int, C.c_int, C.c_int)
_sig("qr_lsei_batched_dev", C.c_int, _vp, _vp, C.c_int, C.c_int, C.c_int, _ll, _vp, _ll, _vp, C.c_int, C.c_int, C.c_int, _ll, _vp, _ll, C.c_int,
     C.c_double, _vp, _ll, _vp, _ll, _vp, _ll, _vp, _ll, _vp, _vp, _vp, C.c_int)
_sig("qr_lstsq_inequality_batched", C.c_int, _dp, C.c_int, C.c_int, _dp, _dp, C.c_int, C.c_int, _dp, C.c_int, C.c_double, C.c_int, _dp, _dp, _dp,
     _ip, _dp, _ip, _ip)
class LmOptions(C.Structure):
    """qr_lm_options"""
    _fields_ = [("ftol", C.c_double), ("xtol", C.c_double), ("gtol", C.c_double), ("factor", C.c_double), ("par_rtol", C.c_double),
                ("maxfev", C.c_int), ("mode", C.c_int), ("par_maxit", C.c_int)]


class LmState(C.Structure):
    """qr_lm_batched_state: device addresses"""
    _doubles = ("x", "xtrial", "D", "delta", "par", "fnorm", "xnorm", "pnorm", "gnorm", "prered", "dirder")
    _ints = ("iter", "nfev", "njev", "accepted", "status", "info", "par_status")
    _fields_ = [(k, C.c_void_p) for k in _doubles + _ints]


LM_FCN = C.CFUNCTYPE(C.c_int, _vp, C.c_int, _dp, C.c_int, _dp, _dp)
_sig("qr_lm_options_default", None, C.POINTER(LmOptions))
_sig("qr_lm_batched_create", C.c_int, C.POINTER(_vp), _vp, C.c_int, C.c_int, C.c_int, C.POINTER(LmOptions))
_sig("qr_lm_batched_start_dev", C.c_int, _vp, _vp, C.c_int, _ll, _vp, _ll)
_sig("qr_lm_batched_step_dev", C.c_int, _vp, _vp, C.c_int, _ll, _vp, C.c_int, _ll)
_sig("qr_lm_batched_update_dev", C.c_int, _vp, _vp, C.c_int, _ll)
_sig("qr_lm_batched_view", C.c_int, _vp, C.POINTER(LmState))
_sig("qr_lm_batched_running", C.c_int, _vp, C.POINTER(C.c_int))
_sig("qr_lm_batched_destroy", C.c_int, _vp)
_sig("qr_lm_step_batched_dev", C.c_int, _vp, _vp, C.c_int, _ll, _vp, C.c_int, C.c_int, _ll, _vp, _vp, _ll)
_sig("qr_lstsq_lm_batched", C.c_int, LM_FCN, _vp, C.c_int, C.c_int, C.c_int, _dp, _dp, C.POINTER(LmOptions), _dp, _ip, _ip, _ip, _ip)
class LmBoundedState(C.Structure):
    """qr_lmb_batched_state: device addresses"""
    _doubles = LmState._doubles + ("lo", "hi", "alpha")
    _ints = LmState._ints + ("peg", "clipped")
    _fields_ = [(k, C.c_void_p) for k in LmState._doubles + LmState._ints + ("lo", "hi", "alpha", "peg", "clipped")]


_sig("qr_lmb_batched_create", C.c_int, C.POINTER(_vp), _vp, C.c_int, C.c_int, C.c_int, C.POINTER(LmOptions))
_sig("qr_lmb_batched_start_dev", C.c_int, _vp, _vp, C.c_int, _ll, _vp, _ll, _vp, _ll, _vp, _ll)
_sig("qr_lmb_batched_step_dev", C.c_int, _vp, _vp, C.c_int, _ll, _vp, C.c_int, _ll)
_sig("qr_lmb_batched_update_dev", C.c_int, _vp, _vp, C.c_int, _ll)
_sig("qr_lmb_batched_view", C.c_int, _vp, C.POINTER(LmBoundedState))
_sig("qr_lmb_batched_running", C.c_int, _vp, C.POINTER(C.c_int))
_sig("qr_lmb_batched_destroy", C.c_int, _vp)
_sig("qr_lstsq_lm_bounded_batched", C.c_int, LM_FCN, _vp, C.c_int, C.c_int, C.c_int, _dp, _dp, _dp, _dp, C.POINTER(LmOptions), _dp, _ip, _ip, _ip,
     _ip)
_sig("qr_irls_batched_max_rows", C.c_int, C.c_int)
_sig("qr_irls_batched_dev", C.c_int, _vp, C.c_int, C.c_double, _vp, C.c_int, C.c_int, C.c_int, _ll, _vp, _ll, _vp, _ll, _vp, _vp, _ll, C.c_double,
     C.c_int, _vp, _ll, _vp, _ll, _vp, _vp, _vp, _vp, _vp, C.c_int)
_sig("qr_gels_weighted_batched_dev", C.c_int, _vp, _vp, C.c_int, C.c_int, C.c_int, _ll, _vp, _ll, _vp, _ll, _vp, _ll, _vp, _vp, C.c_int)
_sig("qr_lstsq_robust_batched", C.c_int, _dp, C.c_int, C.c_int, _dp, C.c_int, C.c_double, _dp, _dp, _dp, C.c_double, C.c_int, C.c_int, _dp, _dp,
     _dp, _dp, _ip, _ip, _ip)
_sig("qr_stats_batched_max_rows", C.c_int, C.c_int)
_sig("qr_covar_batched_dev", C.c_int, _vp, _vp, C.c_int, C.c_int, _ll, _vp, _ll, _vp, _vp, _vp, C.c_int, _ll, _vp, _ll, _vp, C.c_int)
_sig("qr_leverage_batched_dev", C.c_int, _vp, _vp, C.c_int, C.c_int, _ll, _vp, _ll, _vp, _vp, C.c_int, C.c_int, _ll, _vp, _ll, _vp, _ll, _vp,
     C.c_int)
_sig("qr_gels_stats_batched_dev", C.c_int, _vp, C.c_int, _vp, C.c_int, C.c_int, C.c_int, _ll, _vp, _ll, _vp, _ll, _vp, _ll, _vp, _ll, _vp, _ll,
     _vp, _vp, _vp, C.c_int, _ll, _vp, _ll, _vp, C.c_int)
_sig("qr_lsacc_batched_covar_dev", C.c_int, _vp, C.c_int, C.c_int, _vp, C.c_int, _ll, _vp, _ll, _vp, _vp)
_sig("qr_lstsq_stats_batched", C.c_int, _dp, C.c_int, C.c_int, _dp, _dp, C.c_int, C.c_int, _dp, _dp, _dp, _dp, _ip, _dp, _dp, _ip)
_sig("qr_extract_r_dev", C.c_int, _vp, _vp, C.c_int, C.c_int, C.c_int, _vp, C.c_int, C.c_int)
_sig("qr_gemm_dev", C.c_int, _vp, C.c_char, C.c_int, C.c_int, C.c_int, C.c_double, _vp, C.c_int, _vp, C.c_int,
     C.c_double, _vp, C.c_int)
_sig("qr_fill_uniform_dev", C.c_int, _vp, _vp, C.c_int, C.c_longlong, C.c_int, C.c_longlong, C.c_longlong,
     C.c_ulonglong)
_sig("qr_uniform_at", C.c_double, C.c_ulonglong, C.c_ulonglong)
_sig("qr_diffnorm_dev", C.c_int, _vp, _vp, C.c_int, _vp, C.c_int, C.c_longlong, C.c_int, C.c_longlong,
     C.c_longlong, C.c_ulonglong, C.c_int, _dp)
_sig("qr_device_malloc", C.c_int, C.POINTER(_vp), C.c_size_t)
_sig("qr_device_free", C.c_int, _vp)
_sig("qr_copy_to_device", C.c_int, _vp, _vp, C.c_size_t)
_sig("qr_copy_to_host", C.c_int, _vp, _vp, C.c_size_t)
_sig("qr_plan_sync", C.c_int, _vp)
_sig("qr_plan_stream", _vp, _vp)
_sig("qr_plan_set_guard_mode", C.c_int, _vp, C.c_int)
_sig("qr_plan_route_stats", C.c_int, _vp, C.POINTER(C.c_longlong))
_sig("qr_plan_retry_stats", C.c_int, _vp, C.POINTER(C.c_longlong))
_sig("qr_plan_info", C.c_int, _vp, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int))
_sig("qr_plan_update_cus", C.c_int, _vp)
_sig("qr_plan_set_profile", C.c_int, _vp, C.c_int)
_sig("qr_plan_pause_profile", C.c_int, _vp, C.c_int)
_sig("qr_plan_get_profile", C.c_int, _vp, C.POINTER(Profile))
_sig("qr_plan_get_profile_records", C.c_int, _vp, C.c_int, C.POINTER(C.c_int), _dp, _dp)
_sig("qr_device_info", C.c_int, C.c_char_p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_size_t))
_sig("qr_probe_mfma_f64_tflops", C.c_int, _dp)
_sig("qr_probe_copy_gbps", C.c_int, _dp)
# internal launch layer (kernel unit tests only)
_sig("qrd_gemm_nn", C.c_int, _vp, C.c_int, C.c_int, C.c_int, C.c_double, _vp, C.c_int, _vp, C.c_int, C.c_double,
     _vp, C.c_int)
_sig("qrd_gemm_tn", C.c_int, _vp, C.c_int, C.c_int, C.c_int, C.c_double, _vp, C.c_int, _vp, C.c_int, C.c_double,
     _vp, C.c_int, _vp, C.c_size_t, _vp, C.c_int)
_sig("qrd_gemm_tn_update", C.c_int, _vp, C.c_int, C.c_int, C.c_int, C.c_double, _vp, C.c_int, _vp, C.c_int, C.c_double,
     _vp, C.c_int, _vp, C.c_size_t)
_sig("qrd_gemm_tn_update_wide", C.c_int, _vp, C.c_int, C.c_int, C.c_int, C.c_double, _vp, C.c_int, _vp, C.c_int, C.c_double,
     _vp, C.c_int, _vp, C.c_size_t)
if hasattr(lib, "qrd_gemm_tn_update_even"):        # (absent from libraries of earlier commits loaded for A/B runs through CUDA_QR_AMD_LIB)
    _sig("qrd_gemm_tn_update_even", C.c_int, _vp, C.c_int, C.c_int, C.c_int, C.c_double, _vp, C.c_int, _vp, C.c_int, C.c_double,
         _vp, C.c_int, _vp, C.c_size_t, C.c_int)
    _sig("qrd_tn_even_launches", C.c_longlong)
    _sig("qrd_tn_even_last_grid", C.c_int)
if hasattr(lib, "qrd_gemm_nn_tri"):        # (absent from libraries of earlier commits loaded for A/B runs through CUDA_QR_AMD_LIB)
    _sig("qrd_gemm_nn_tri", C.c_int, _vp, C.c_int, C.c_int, C.c_int, C.c_double, _vp, C.c_int, _vp, C.c_int, C.c_double,
         _vp, C.c_int)
    _sig("qrd_gemm_nn_tri_tile", C.c_int, _vp, C.c_int, C.c_int, C.c_int, C.c_int, _vp, C.c_int, _vp, C.c_int, _vp, C.c_int)
    _sig("qrd_vt_tri_launches", C.c_longlong)
_sig("qrd_gemm_tn_dual", C.c_int, _vp, C.c_int, C.c_int, C.c_int, _vp, C.c_int, _vp, C.c_int, _vp, C.c_int, _vp, C.c_int, _vp, C.c_int, _vp, C.c_int,
     _vp, C.c_size_t)
_sig("qrd_trsm_gt", C.c_int, _vp, C.c_int, C.c_int, _vp, C.c_int, _vp, C.c_int, _vp, C.c_int, _vp, C.c_int)
_sig("qrd_larft", C.c_int, _vp, C.c_int, C.c_int, _vp, C.c_int, _vp, _vp, C.c_int, _vp, C.c_int, _vp, C.c_int)
_sig("qrd_panel_ws_size", C.c_size_t, C.c_int)
_sig("qrd_panel_tsqr", C.c_int, _vp, _vp, C.c_int, C.c_int, C.c_int, _vp, _vp, C.c_int, _vp, C.c_int, _vp, C.c_int)
_sig("qrd_panel_cholqr", C.c_int, _vp, _vp, C.c_int, C.c_int, C.c_int, _vp, _vp, C.c_int, _vp, C.c_int, _vp, C.c_int, _vp, _vp, C.c_size_t, C.c_int)
_sig("qrd_leaf_update_gram", C.c_int, _vp, C.c_int, C.c_int, _vp, C.c_int, _vp, _vp, C.c_int, _vp, C.c_size_t, C.c_int, C.POINTER(C.c_int))
_sig("qrd_gemm_nt", C.c_int, _vp, C.c_int, C.c_int, C.c_int, C.c_int, _vp, C.c_int, _vp, C.c_int, _vp, C.c_int, C.c_int, _vp)
if hasattr(lib, "qrd_gemm_nt4_ok"):        # (absent from libraries of earlier commits loaded for A/B runs through CUDA_QR_AMD_LIB)
    _sig("qrd_gemm_nt4_ok", C.c_int, C.c_int, C.c_int, C.c_int, _vp, C.c_int, _vp, C.c_int, _vp, C.c_int)
_sig("qrd_transpose", C.c_int, _vp, C.c_int, C.c_int, _vp, C.c_int, _vp, C.c_int)
_sig("qrd_copy_block", C.c_int, _vp, _vp, C.c_int, _vp, C.c_int, C.c_int, C.c_int)
_sig("qrd_init", C.c_int)
_sig("qrd_device_sync", C.c_int)
if hasattr(lib, "qrd_tp_panel"):        # (absent from libraries of earlier commits loaded for A/B runs through CUDA_QR_AMD_LIB)
    _sig("qrd_tp_panel", C.c_int, _vp, _vp, C.c_int, _vp, C.c_int, C.c_int, C.c_int, _vp, C.c_int)
    _sig("qrd_tp_apply", C.c_int, _vp, C.c_int, _vp, C.c_int, C.c_int, C.c_int, _vp, C.c_int, _vp, C.c_int, _vp, C.c_int, C.c_int)
    _sig("qrd_tp_colssq_add", C.c_int, _vp, _vp, C.c_int, C.c_int, C.c_int, _vp)
    _sig("qrd_tp_sqrt", C.c_int, _vp, _vp, _vp, C.c_int)
if hasattr(lib, "qrd_th_panel"):
    _sig("qrd_th_panel", C.c_int, _vp, _vp, C.c_int, _vp, C.c_int, C.c_int, C.c_int, C.c_int, _vp, C.c_int, C.c_int, _vp)
    _sig("qrd_th_apply", C.c_int, _vp, _vp, C.c_int, C.c_int, C.c_int, C.c_int, _vp, C.c_int, _vp, C.c_int, _vp, C.c_int, C.c_int, _vp)
    _sig("qrd_th_colssq", C.c_int, _vp, _vp, C.c_int, C.c_int, C.c_int, C.c_int, _vp, _vp)
if hasattr(lib, "qrd_jsvd_round"):
    _sig("qrd_jsvd_round", C.c_int, _vp, _vp, C.c_int, C.c_int, C.c_int, _vp, C.c_int, _vp, C.c_int, C.c_double, _vp)
    _sig("qrd_jsvd_fold", C.c_int, _vp, _vp, C.c_int, _vp)
    _sig("qrd_jsvd_colnorms", C.c_int, _vp, _vp, C.c_int, C.c_int, C.c_int, _vp)
    _sig("qrd_jsvd_gather", C.c_int, _vp, _vp, _vp, _vp, C.c_int)
    _sig("qrd_jsvd_permute", C.c_int, _vp, _vp, C.c_int, C.c_int, C.c_int, _vp)
    _sig("qrd_jsvd_normalise", C.c_int, _vp, _vp, C.c_int, C.c_int, C.c_int, _vp)
    _sig("qrd_jsvd_pinv_scale", C.c_int, _vp, _vp, _vp, C.c_int, C.c_int, _vp, C.c_double)
    _sig("qrd_jsvd_rt", C.c_int, _vp, _vp, C.c_int, C.c_int, _vp, C.c_int)


def strerror(rc):
    return lib.qr_strerror(rc).decode()


def check(rc, what=""):
    if rc != 0:
        raise QRError(f"{what or 'mi355xqr'} failed: {strerror(rc)} ({rc})", rc)


def exported_symbols():
    """Names declared in include/mi355x_qr.h (parsed), for the 'library exports its header' test."""
    import re
    txt = open(HEADER).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    names = re.findall(r"^\s*(?:const\s+)?(?:int|void|double|char\*|void\*|const char\*|qr_plan\*)\s*\*?\s*(\w+)\s*\(", txt, flags=re.M)
    return sorted(set(names))


# ------------------------------------------------------------------------------------------------
# host-pointer drop-in calls (numpy in / numpy out)
# ------------------------------------------------------------------------------------------------
def _f(a):
    return np.asfortranarray(a, dtype=np.float64)


def _p(a):
    return a.ctypes.data_as(_dp)


def get_panel_dims(m, n):
    rp, cp = C.c_int(), C.c_int()
    lib.getPanelDims(m, n, C.byref(rp), C.byref(cp))
    return rp.value, cp.value


def get_block_size():
    nb, ib = C.c_int(), C.c_int()
    lib.qr_get_block_size(C.byref(nb), C.byref(ib))
    return nb.value, ib.value


def default_block_size(m, n):
    """(nb, ib) an m x n problem really gets from mmqr / a default plan (shape-dependent; sizes mmqr's tau)."""
    nb, ib = C.c_int(), C.c_int()
    check(lib.qr_default_block_size(m, n, C.byref(nb), C.byref(ib)), "qr_default_block_size")
    return nb.value, ib.value


def tau_len(m, n):
    """entries of the tau array mmqr mallocs for an m x n problem: rowPanels * colPanels * nb (qr.c:61 sizing rule)."""
    rp, cp = get_panel_dims(m, n)
    return rp * cp * default_block_size(m, n)[0]


def set_block_size(nb, ib):
    check(lib.qr_set_block_size(nb, ib), "qr_set_block_size")


_libc = C.CDLL(None)
_libc.free.argtypes = [C.c_void_p]


def mmqr(A):
    """reference mmqr (qr.c:55): returns (factored copy, tau array of colPanels*nb entries)."""
    F = np.array(A, dtype=np.float64, order="F", copy=True)
    m, n = F.shape
    tptr = _dp()
    check(lib.mmqr_status(_p(F), C.byref(tptr), m, n), "mmqr")
    tau = np.ctypeslib.as_array(tptr, shape=(tau_len(m, n),)).copy()
    _libc.free(C.cast(tptr, C.c_void_p))
    return F, tau


def explicit_qr(F, tau):
    """reference explicitQR (qr.c:330): Q (m x m), R (m x n)."""
    F = _f(F)
    m, n = F.shape
    tau = np.ascontiguousarray(tau, dtype=np.float64)
    if tau.size < n:
        raise QRError(f"explicit_qr: tau has {tau.size} entries, the factorisation of {n} columns has {n}")
    Q = np.empty((m, m), order="F")
    R = np.empty((m, n), order="F")
    check(lib.explicitQR_status(_p(F), _p(tau), _p(Q), _p(R), m, n), "explicitQR")
    return Q, R


def mmqr_legacy(A, PR, PC):
    """The reference's sliding-window MMQR itself (legacy-layout shim): (factored copy, window-indexed tau) for window PR x PC."""
    F = np.array(A, dtype=np.float64, order="F", copy=True)
    m, n = F.shape
    tptr = _dp()
    check(lib.mmqr_legacy_status(_p(F), C.byref(tptr), m, n, PR, PC), "mmqr_legacy")
    rp, cp = C.c_int(), C.c_int()
    lib.getPanelDims_legacy(m, n, PR, PC, C.byref(rp), C.byref(cp))
    tau = np.ctypeslib.as_array(tptr, shape=(rp.value * cp.value * PC,)).copy()
    _libc.free(C.cast(tptr, C.c_void_p))
    return F, tau


def explicit_qr_legacy(F, tau, PR, PC):
    F = _f(F)
    m, n = F.shape
    tau = np.ascontiguousarray(tau, dtype=np.float64)
    Q = np.empty((m, m), order="F")
    R = np.empty((m, n), order="F")
    check(lib.explicitQR_legacy_status(_p(F), _p(tau), _p(Q), _p(R), m, n, PR, PC), "explicitQR_legacy")
    return Q, R


def dgemm(A, B):
    """reference dgemm (qr.c:443): C (k x n) = A (k x m) B (m x n)."""
    A, B = _f(A), _f(B)
    k, m = A.shape
    m2, n = B.shape
    assert m == m2
    Cm = np.empty((k, n), order="F")
    check(lib.dgemm_status(_p(A), _p(B), _p(Cm), k, m, n), "dgemm")
    return Cm


def identity(m):
    A = np.empty((m, m), order="F")
    lib.identity(_p(A), m)
    return A


def qr_thin(A, nb=0, nshards=1):
    A = _f(A)
    m, n = A.shape
    Q = np.empty((m, n), order="F")
    R = np.empty((n, n), order="F")
    check(lib.qr_thin(_p(A), m, n, _p(Q), _p(R), nb, nshards), "qr_thin")
    return Q, R


def mmqr_f32(A):
    """Float instantiation of mmqr (reference Scalar = float, qr.c:11): returns (factored float matrix, float tau)."""
    F = np.asfortranarray(A, dtype=np.float32).copy(order="F")
    m, n = F.shape
    tau = _fp()
    check(lib.mmqr_f32_status(F.ctypes.data_as(_fp), C.byref(tau), m, n), "mmqr_f32")
    t = np.ctypeslib.as_array(tau, shape=(tau_len(m, n),)).copy()
    _libc.free(C.cast(tau, C.c_void_p))
    return F, t


def explicit_qr_f32(F, tau):
    F = np.asfortranarray(F, dtype=np.float32)
    m, n = F.shape
    t = np.ascontiguousarray(tau, dtype=np.float32)
    if t.size < n:
        raise QRError(f"explicit_qr_f32: tau has {t.size} entries, the factorisation of {n} columns has {n}")
    Q = np.empty((m, m), dtype=np.float32, order="F")
    R = np.empty((m, n), dtype=np.float32, order="F")
    check(lib.explicitQR_f32_status(F.ctypes.data_as(_fp), t.ctypes.data_as(_fp), Q.ctypes.data_as(_fp), R.ctypes.data_as(_fp), m, n),
          "explicitQR_f32")
    return Q, R


def qr_thin_mgpu(A, nb=0, ngpu=1):
    """Thin QR over `ngpu` devices of this node through the C-level TSQR entry (one host thread per GPU, one RCCL all-gather)."""
    A = _f(A)
    m, n = A.shape
    Q = np.empty((m, n), order="F")
    R = np.empty((n, n), order="F")
    check(lib.qr_thin_mgpu(_p(A), m, n, _p(Q), _p(R), nb, ngpu), "qr_thin_mgpu")
    return Q, R


def lstsq(A, B):
    """min ||A X - B|| for a full-rank m x n A (m >= n) through qr_lstsq: returns (X, resid), resid[j] = ||A x_j - b_j||.
    A 1-D B is one column (X and resid then 1-D / a scalar).  Raises QRError (status QR_E_SINGULAR) when R has an exactly zero
    diagonal entry."""
    A = _f(A)
    m, n = A.shape
    B = np.asarray(B, dtype=np.float64)
    vec = B.ndim == 1
    B = _f(B.reshape(-1, 1) if vec else B)
    if B.shape[0] != m:
        raise QRError(f"lstsq: B has {B.shape[0]} rows, A has {m}", QR_E_ARG)
    nrhs = B.shape[1]
    X = np.empty((n, nrhs), order="F")
    resid = np.empty(nrhs)
    check(lib.qr_lstsq(_p(A), m, n, _p(B), nrhs, _p(X), _p(resid)), "qr_lstsq")
    return (X[:, 0], resid[0]) if vec else (X, resid)


def lstsq_pivoted(A, B, rcond=None):
    """min ||A X - B|| for an m x n A (m >= n) of any rank through qr_lstsq_pivoted: returns (X, resid, rank, jpvt).  X is the basic
    solution: the rows jpvt[rank:] are zero.  rcond None: max(m, n) eps.  A 1-D B is one column (X and resid then 1-D / a scalar)."""
    A = _f(A)
    m, n = A.shape
    B = np.asarray(B, dtype=np.float64)
    vec = B.ndim == 1
    B = _f(B.reshape(-1, 1) if vec else B)
    if B.shape[0] != m:
        raise QRError(f"lstsq_pivoted: B has {B.shape[0]} rows, A has {m}", QR_E_ARG)
    nrhs = B.shape[1]
    X = np.empty((n, nrhs), order="F")
    resid = np.empty(nrhs)
    jpvt = np.empty(max(n, 1), dtype=np.intc)
    rank = C.c_int()
    check(lib.qr_lstsq_pivoted(_p(A), m, n, _p(B), nrhs, -1.0 if rcond is None else float(rcond), _p(X), _p(resid), C.byref(rank),
                               jpvt.ctypes.data_as(_ip)), "qr_lstsq_pivoted")
    jpvt = jpvt[:n].astype(np.int64)
    return (X[:, 0], resid[0], rank.value, jpvt) if vec else (X, resid, rank.value, jpvt)


def lstsq_minnorm(A, B):
    """The minimum-norm solution of A X = B for a full-rank wide m x n A (m <= n) through qr_lstsq_minnorm: returns X (n x nrhs).
    A 1-D B is one column (X then 1-D).  Raises QRError (status QR_E_SINGULAR) when R of A^T has an exactly zero diagonal entry."""
    A = _f(A)
    m, n = A.shape
    B = np.asarray(B, dtype=np.float64)
    vec = B.ndim == 1
    B = _f(B.reshape(-1, 1) if vec else B)
    if B.shape[0] != m:
        raise QRError(f"lstsq_minnorm: B has {B.shape[0]} rows, A has {m}", QR_E_ARG)
    nrhs = B.shape[1]
    X = np.empty((n, nrhs), order="F")
    check(lib.qr_lstsq_minnorm(_p(A), m, n, _p(B), nrhs, _p(X)), "qr_lstsq_minnorm")
    return X[:, 0] if vec else X


def lstsq_chunked(A, B, chunk_rows):
    """min ||A X - B|| for a full-rank m x n A through qr_lstsq_chunked: chunk_rows rows at a time are uploaded and folded into an
    accumulator (device memory bounded by the chunk): returns (X, resid) as lstsq does.  Raises QRError (status QR_E_SINGULAR) when R
    has an exactly zero diagonal entry or A has fewer rows than columns."""
    A = _f(A)
    m, n = A.shape
    B = np.asarray(B, dtype=np.float64)
    vec = B.ndim == 1
    B = _f(B.reshape(-1, 1) if vec else B)
    if B.shape[0] != m:
        raise QRError(f"lstsq_chunked: B has {B.shape[0]} rows, A has {m}", QR_E_ARG)
    nrhs = B.shape[1]
    X = np.empty((n, nrhs), order="F")
    resid = np.empty(nrhs)
    check(lib.qr_lstsq_chunked(_p(A), m, n, m, _p(B), nrhs, m, int(chunk_rows), _p(X), _p(resid)), "qr_lstsq_chunked")
    return (X[:, 0], resid[0]) if vec else (X, resid)


def lstsq_rolling(A, B, window, step):
    """least squares over the windows A[k step : k step + window], k = 0 .. (m - window) // step, through qr_lstsq_rolling: the first
    window is factored, every later one is one slide (step rows in, step rows out).  Returns (X, resid): X of shape (windows, n, nrhs)
    -- (windows, n) for a vector B --, resid (windows, nrhs) / (windows,).  Raises QRError: QR_E_SINGULAR for a rank-deficient first
    window, QR_E_NOTPD when a later window loses full rank."""
    A = _f(A)
    m, n = A.shape
    B = np.asarray(B, dtype=np.float64)
    vec = B.ndim == 1
    B = _f(B.reshape(-1, 1) if vec else B)
    if B.shape[0] != m:
        raise QRError(f"lstsq_rolling: B has {B.shape[0]} rows, A has {m}", QR_E_ARG)
    nrhs = B.shape[1]
    window, step = int(window), int(step)
    nwin = (m - window) // step + 1 if 1 <= step and n <= window <= m else 1
    X = np.empty((nwin, nrhs, n))                        # window k: the column-major n x nrhs block
    resid = np.empty((nwin, nrhs))
    check(lib.qr_lstsq_rolling(_p(A), m, n, m, _p(B), nrhs, m, window, step, _p(X), _p(resid)), "qr_lstsq_rolling")
    X = X.transpose(0, 2, 1)
    return (X[:, :, 0], resid[:, 0]) if vec else (X, resid)


def batched_max_rows(ncols):
    """the most rows the batched calls take for ncols columns held in LDS (qr_batched_max_rows; 0: too many columns; no device)"""
    return lib.qr_batched_max_rows(int(ncols))


def _packed_batch(A, what):
    """(batch, rows, cols) -> the packed column-major batch (a C-contiguous (batch, cols, rows) array)"""
    A = np.asarray(A, dtype=np.float64)
    if A.ndim != 3:
        raise QRError(f"{what}: expected an array of shape (batch, rows, cols), got {A.shape}", QR_E_ARG)
    return np.ascontiguousarray(A.transpose(0, 2, 1))


def qr_batched(A):
    """the thin QR of every matrix of A (batch, m, n), m >= n, through qr_thin_batched: returns Q (batch, m, n) and R (batch, n, n)"""
    At = _packed_batch(A, "qr_batched")
    batch, n, m = At.shape
    Q = np.empty((batch, n, m))
    R = np.empty((batch, n, n))
    check(lib.qr_thin_batched(_p(At), m, n, batch, _p(Q), _p(R)), "qr_thin_batched")
    return Q.transpose(0, 2, 1), R.transpose(0, 2, 1)


def lstsq_batched(A, B):
    """min ||A_q X_q - B_q|| for every matrix of A (batch, m, n) and B (batch, m, nrhs) through qr_lstsq_batched: returns (X, resid,
    info) with X (batch, n, nrhs), resid[q, j] = ||A_q x_j - b_j|| and info[q] = 0, or i + 1 for the smallest i with R_q(i,i) == 0
    exactly (X[q] then holds no solution; the other matrices are solved).  A singular matrix does not raise."""
    At = _packed_batch(A, "lstsq_batched")
    Bt = _packed_batch(B, "lstsq_batched")
    batch, n, m = At.shape
    if Bt.shape[0] != batch or Bt.shape[2] != m:
        raise QRError(f"lstsq_batched: B is {Bt.shape[0]} matrices of {Bt.shape[2]} rows, A is {batch} of {m}", QR_E_ARG)
    nrhs = Bt.shape[1]
    X = np.empty((batch, nrhs, n))
    resid = np.empty((batch, nrhs))
    info = np.zeros(max(batch, 1), dtype=np.intc)
    rc = lib.qr_lstsq_batched(_p(At), m, n, _p(Bt), nrhs, batch, _p(X), _p(resid), info.ctypes.data_as(_ip))
    if rc != QR_E_SINGULAR:
        check(rc, "qr_lstsq_batched")
    return X.transpose(0, 2, 1), resid, info[:batch].astype(np.int64)


def qr_pivoted_batched(A):
    """the column-pivoted thin QR of every matrix of A (batch, m, n), m >= n, through qr_thin_pivoted_batched: returns Q (batch, m, n),
    R (batch, n, n) and jpvt (batch, n; 0-based) with A[q][:, jpvt[q]] = Q[q] R[q]"""
    At = _packed_batch(A, "qr_pivoted_batched")
    batch, n, m = At.shape
    Q = np.empty((batch, n, m))
    R = np.empty((batch, n, n))
    jpvt = np.zeros((max(batch, 1), max(n, 1)), dtype=np.intc)
    check(lib.qr_thin_pivoted_batched(_p(At), m, n, batch, _p(Q), _p(R), jpvt.ctypes.data_as(_ip)), "qr_thin_pivoted_batched")
    return Q.transpose(0, 2, 1), R.transpose(0, 2, 1), jpvt[:batch, :n].astype(np.int64)


def lstsq_pivoted_batched(A, B, rcond=None, minnorm=True):
    """rank-deficient least squares for every matrix of A (batch, m, n) and B (batch, m, nrhs) through qr_lstsq_pivoted_batched: returns
    (X, resid, rank, jpvt) with X (batch, n, nrhs) the minimum-norm solutions (minnorm=False: the basic ones, zero outside the leading
    rank columns of A P), resid[q, j] = ||A_q x_j - b_j||, rank (batch,) and jpvt (batch, n).  rcond None: max(m, n) eps.  No rank
    raises."""
    At = _packed_batch(A, "lstsq_pivoted_batched")
    Bt = _packed_batch(B, "lstsq_pivoted_batched")
    batch, n, m = At.shape
    if Bt.shape[0] != batch or Bt.shape[2] != m:
        raise QRError(f"lstsq_pivoted_batched: B is {Bt.shape[0]} matrices of {Bt.shape[2]} rows, A is {batch} of {m}", QR_E_ARG)
    nrhs = Bt.shape[1]
    X = np.empty((batch, nrhs, n))
    resid = np.empty((batch, nrhs))
    rank = np.zeros(max(batch, 1), dtype=np.intc)
    jpvt = np.zeros((max(batch, 1), max(n, 1)), dtype=np.intc)
    check(lib.qr_lstsq_pivoted_batched(_p(At), m, n, _p(Bt), nrhs, batch, -1.0 if rcond is None else float(rcond), int(bool(minnorm)),
                                       _p(X), _p(resid), rank.ctypes.data_as(_ip), jpvt.ctypes.data_as(_ip)), "qr_lstsq_pivoted_batched")
    return X.transpose(0, 2, 1), resid, rank[:batch].astype(np.int64), jpvt[:batch, :n].astype(np.int64)


def svd_batched(A, compute_uv=True):
    """the SVD of every matrix of A (batch, m, n), m >= n, through qr_svd_batched: returns (U, S, V, rank) with U (batch, m, n), S (batch, n)
    descending, V (batch, n, n) -- V, not numpy's V^T -- and rank (batch,) = the number of non-zero values, A[q] = U[q] diag(S[q]) V[q]^T;
    compute_uv False: U and V are None"""
    At = _packed_batch(A, "svd_batched")
    batch, n, m = At.shape
    S = np.empty((batch, n))
    rank = np.zeros(max(batch, 1), dtype=np.intc)
    U = np.empty((batch, n, m)) if compute_uv else None
    V = np.empty((batch, n, n)) if compute_uv else None
    check(lib.qr_svd_batched(_p(At), m, n, batch, _p(S), _p(U) if compute_uv else None, _p(V) if compute_uv else None,
                             rank.ctypes.data_as(_ip)), "qr_svd_batched")
    rank = rank[:batch].astype(np.int64)
    if not compute_uv:
        return None, S, None, rank
    return U.transpose(0, 2, 1), S, V.transpose(0, 2, 1), rank


def tpqrt_batched_max_rows(ncols):
    """the most rows p_add + p_del one batched update takes beside ncols = n + nrhs columns (qr_tpqrt_batched_max_rows; 0: too many
    columns; no device)"""
    return lib.qr_tpqrt_batched_max_rows(int(ncols))


def lstsq_rolling_batched(A, B, window, step):
    """least squares over the windows A[q, k step : k step + window] of every series of A (batch, m, n) and B (batch, m, nrhs) through
    qr_lstsq_rolling_batched: the first window is pushed, every later one is one slide for the whole batch.  Returns (X, resid, info):
    X (batch, windows, n, nrhs), resid (batch, windows, nrhs), info (batch, windows) with 0, the failing column + 1 or -1 of a slide, or
    the zero pivot + 1 of a solve.  A non-zero info word does not raise: the other entries are valid."""
    At = _packed_batch(A, "lstsq_rolling_batched")
    Bt = _packed_batch(B, "lstsq_rolling_batched")
    batch, n, m = At.shape
    if Bt.shape[0] != batch or Bt.shape[2] != m:
        raise QRError(f"lstsq_rolling_batched: B is {Bt.shape[0]} series of {Bt.shape[2]} rows, A is {batch} of {m}", QR_E_ARG)
    nrhs = Bt.shape[1]
    window, step = int(window), int(step)
    nwin = (m - window) // step + 1 if 1 <= step and n <= window <= m else 1
    X = np.empty((batch, nwin, nrhs, n))
    resid = np.empty((batch, nwin, nrhs))
    info = np.zeros((max(batch, 1), nwin), dtype=np.intc)
    rc = lib.qr_lstsq_rolling_batched(_p(At), m, n, _p(Bt), nrhs, batch, window, step, _p(X), _p(resid), info.ctypes.data_as(_ip))
    if rc not in (QR_E_SINGULAR, QR_E_NOTPD):
        check(rc, "qr_lstsq_rolling_batched")
    return X.transpose(0, 1, 3, 2), resid, info[:batch].astype(np.int64)


def lstsq_minnorm_batched(A, B):
    """the minimum-norm solution of A_q X_q = B_q for every member of A (batch, m, n), m <= n, and B (batch, m, nrhs) through
    qr_lstsq_minnorm_batched: returns (X, info) with X (batch, n, nrhs) and info[q] = 0, or i + 1 for the smallest i with
    R_q(i,i) == 0 exactly (a zero row of A_q; X[q] then holds no solution, the other members are solved).  A singular member does not
    raise."""
    At = _packed_batch(A, "lstsq_minnorm_batched")
    Bt = _packed_batch(B, "lstsq_minnorm_batched")
    batch, n, m = At.shape
    if Bt.shape[0] != batch or Bt.shape[2] != m:
        raise QRError(f"lstsq_minnorm_batched: B is {Bt.shape[0]} matrices of {Bt.shape[2]} rows, A is {batch} of {m}", QR_E_ARG)
    nrhs = Bt.shape[1]
    X = np.empty((batch, nrhs, n))
    info = np.zeros(max(batch, 1), dtype=np.intc)
    rc = lib.qr_lstsq_minnorm_batched(_p(At), m, n, _p(Bt), nrhs, batch, _p(X), info.ctypes.data_as(_ip))
    if rc != QR_E_SINGULAR:
        check(rc, "qr_lstsq_minnorm_batched")
    return X.transpose(0, 2, 1), info[:batch].astype(np.int64)


def lstsq_damped_batched(A, B, lam, D=None):
    """min ||A_q x - b||^2 + lam^2 ||D_q x||^2 for every member of A (batch, m, n), B (batch, m, nrhs) and every lam of a list, through
    qr_lstsq_damped_batched.  lam: (nlam,) shared by every member, or (batch, nlam); D: None (the identity), (n,) or (batch, n); a wide
    A (m < n) requires D is None.  Returns (X, xnorm, resid, info): X (batch, nlam, n, nrhs), xnorm = ||D x|| and resid = ||A x - b||
    (batch, nlam, nrhs), info (batch, nlam) = 0, or i + 1 for the smallest i with a zero on the damped triangle's diagonal (that X
    holds no solution; the others are solved).  A singular pair does not raise."""
    At = _packed_batch(A, "lstsq_damped_batched")
    Bt = _packed_batch(B, "lstsq_damped_batched")
    batch, n, m = At.shape
    if Bt.shape[0] != batch or Bt.shape[2] != m:
        raise QRError(f"lstsq_damped_batched: B is {Bt.shape[0]} matrices of {Bt.shape[2]} rows, A is {batch} of {m}", QR_E_ARG)
    nrhs = Bt.shape[1]
    lam = np.asarray(lam, dtype=np.float64)
    if lam.ndim == 1:
        lam = np.broadcast_to(lam, (batch, lam.shape[0]))
    if lam.ndim != 2 or lam.shape[0] != batch or lam.shape[1] < 1:
        raise QRError(f"lstsq_damped_batched: lam must be (nlam,) or ({batch}, nlam) with nlam >= 1, got {lam.shape}", QR_E_ARG)
    lam = np.ascontiguousarray(lam)
    nlam = lam.shape[1]
    if D is not None:
        D = np.asarray(D, dtype=np.float64)
        if D.ndim == 1:
            D = np.broadcast_to(D, (batch, D.shape[0]))
        if D.shape != (batch, n):
            raise QRError(f"lstsq_damped_batched: D must be ({n},) or ({batch}, {n}), got {D.shape}", QR_E_ARG)
        D = np.ascontiguousarray(D)
    X = np.empty((batch, nlam, nrhs, n))
    xnorm = np.empty((batch, nlam, nrhs))
    resid = np.empty((batch, nlam, nrhs))
    info = np.zeros((max(batch, 1), nlam), dtype=np.intc)
    rc = lib.qr_lstsq_damped_batched(_p(At), m, n, _p(Bt), nrhs, batch, None if D is None else _p(D), _p(lam), nlam, _p(X), _p(xnorm),
                                     _p(resid), info.ctypes.data_as(_ip))
    if rc != QR_E_SINGULAR:
        check(rc, "qr_lstsq_damped_batched")
    return X.transpose(0, 1, 3, 2), xnorm, resid, info[:batch].astype(np.int64)


def lstsq_trust_batched(A, b, delta, D=None, lam0=None, rtol=0.1, maxit=10):
    """the trust-region step of every member of A (batch, m, n) and b (batch, m) through qr_lstsq_trust_batched: the lam >= 0 and
    x = argmin ||A_q x - b_q||^2 + lam^2 ||D_q x||^2 with | ||D x|| - delta | <= rtol delta, or lam = 0 where the Gauss-Newton step is
    within (1 + rtol) delta (MINPACK lmpar, run on the device).  delta: a scalar or (batch,); D: None (the identity), (n,) or
    (batch, n), and a wide A (m < n) requires D is None; lam0: None, a scalar or (batch,), the starting guess.  Returns (X, lam, xnorm,
    resid, iter, status, info): X (batch, n); status 0 converged, 1 Gauss-Newton step accepted, 2 left by the lower-bound clause,
    3 maxit reached; info 0, i + 1 for a zero on the damped triangle's diagonal, -1 for a delta that is not a finite positive number
    (that member's other outputs hold nothing).  A member with an info word does not raise."""
    At = _packed_batch(A, "lstsq_trust_batched")
    batch, n, m = At.shape
    b = np.asarray(b, dtype=np.float64)
    if b.ndim == 3 and b.shape[2] == 1:
        b = b[:, :, 0]
    if b.shape != (batch, m):
        raise QRError(f"lstsq_trust_batched: b must be ({batch}, {m}), one right-hand side per member, got {b.shape}", QR_E_ARG)
    b = np.ascontiguousarray(b)

    def per_member(v, name):
        v = np.asarray(v, dtype=np.float64)
        if v.ndim == 0:
            v = np.broadcast_to(v, (batch,))
        if v.shape != (batch,):
            raise QRError(f"lstsq_trust_batched: {name} must be a scalar or ({batch},), got {v.shape}", QR_E_ARG)
        return np.ascontiguousarray(v)

    delta = per_member(delta, "delta")
    lam0 = None if lam0 is None else per_member(lam0, "lam0")
    if D is not None:
        D = np.asarray(D, dtype=np.float64)
        if D.ndim == 1:
            D = np.broadcast_to(D, (batch, D.shape[0]))
        if D.shape != (batch, n):
            raise QRError(f"lstsq_trust_batched: D must be ({n},) or ({batch}, {n}), got {D.shape}", QR_E_ARG)
        D = np.ascontiguousarray(D)
    X = np.empty((batch, n))
    lam, xnorm, resid = np.empty(batch), np.empty(batch), np.empty(batch)
    it, status, info = (np.zeros(max(batch, 1), dtype=np.intc) for _ in range(3))
    rc = lib.qr_lstsq_trust_batched(_p(At), m, n, _p(b), batch, None if D is None else _p(D), _p(delta), None if lam0 is None else _p(lam0),
                                    float(rtol), int(maxit), _p(X), _p(lam), _p(xnorm), _p(resid), it.ctypes.data_as(_ip),
                                    status.ctypes.data_as(_ip), info.ctypes.data_as(_ip))
    if rc != QR_E_SINGULAR:
        check(rc, "qr_lstsq_trust_batched")
    return X, lam, xnorm, resid, it[:batch].astype(np.int64), status[:batch].astype(np.int64), info[:batch].astype(np.int64)


def gglse_batched_max_rows(n, p, nrhs):
    """the most rows Plan.gglse_batched takes for p constraints on n unknowns and nrhs right-hand sides (qr_gglse_batched_max_rows; 0:
    the shape is not taken at all; no device)"""
    return lib.qr_gglse_batched_max_rows(int(n), int(p), int(nrhs))


def lstsq_constrained_batched(A, C, b, d):
    """min ||A_q x - b_q|| subject to C_q x = d_q for every member of A (batch, m, n), C (batch, p, n), b (batch, m, nrhs) and d (batch, p,
    nrhs) through qr_lstsq_constrained_batched: returns (X, lam, resid, info) with X (batch, n, nrhs), the Lagrange multipliers lam
    (batch, p, nrhs) of A^T (A x - b) + C^T lam = 0, resid[q, j] = ||A_q x_j - b_j|| and info[q] = 0, i + 1 for the smallest i with
    R_c(i,i) == 0 exactly (a zero row of C_q) or p + i + 1 for the smallest i with R_a(i,i) == 0 exactly (X[q], lam[q] and resid[q] then
    read 0; the other members are solved).  A singular member does not raise."""
    At = _packed_batch(A, "lstsq_constrained_batched")
    Ct = _packed_batch(C, "lstsq_constrained_batched")
    bt = _packed_batch(b, "lstsq_constrained_batched")
    dt = _packed_batch(d, "lstsq_constrained_batched")
    batch, n, m = At.shape
    p, nrhs = Ct.shape[2], bt.shape[1]
    if Ct.shape[0] != batch or bt.shape[0] != batch or dt.shape[0] != batch:
        raise QRError(f"lstsq_constrained_batched: A, C, b and d hold {batch}, {Ct.shape[0]}, {bt.shape[0]} and {dt.shape[0]} members", QR_E_ARG)
    if Ct.shape[1] != n:
        raise QRError(f"lstsq_constrained_batched: C has {Ct.shape[1]} columns, A has {n}", QR_E_ARG)
    if bt.shape[2] != m or dt.shape[2] != p or dt.shape[1] != nrhs:
        raise QRError(f"lstsq_constrained_batched: b must be ({batch}, {m}, nrhs) and d ({batch}, {p}, nrhs), got {bt.shape[::-1][:2]} and "
                      f"{dt.shape[::-1][:2]} per member", QR_E_ARG)
    X = np.empty((batch, nrhs, n))
    lam = np.empty((batch, nrhs, p))
    resid = np.empty((batch, nrhs))
    info = np.zeros(max(batch, 1), dtype=np.intc)
    rc = lib.qr_lstsq_constrained_batched(_p(At), m, n, _p(Ct), p, _p(bt), _p(dt), nrhs, batch, _p(X), _p(lam), _p(resid),
                                          info.ctypes.data_as(_ip))
    if rc != QR_E_SINGULAR:
        check(rc, "qr_lstsq_constrained_batched")
    return X.transpose(0, 2, 1), lam.transpose(0, 2, 1), resid, info[:batch].astype(np.int64)


def bvls_batched_max_rows(n):
    """the most rows Plan.bvls_batched takes for n unknowns (qr_bvls_batched_max_rows; 0: n is not taken at all; no device)"""
    return lib.qr_bvls_batched_max_rows(int(n))


def _bound_batch(v, batch, n, what, name):
    """None, (n,) or (batch, n) -> None or a C-contiguous (batch, n) array"""
    if v is None:
        return None
    v = np.asarray(v, dtype=np.float64)
    if v.shape == (n,):
        v = np.broadcast_to(v, (batch, n))
    if v.shape != (batch, n):
        raise QRError(f"{what}: {name} must be ({n},) or ({batch}, {n}), got {v.shape}", QR_E_ARG)
    return np.ascontiguousarray(v)


def lstsq_bounded_batched(A, b, lo=None, hi=None, maxit=0):
    """min ||A_q x - b_q|| subject to lo <= x <= hi for every member of A (batch, m, n), m >= n, and b (batch, m) through
    qr_lstsq_bounded_batched (bounded-variable least squares, the active-set loop of every member on the device).  lo, hi: None (that
    side is unbounded), (n,) (shared by all members) or (batch, n); entries may be -inf / +inf.  maxit: the most eliminations per member
    (<= 0: 3 n).  Returns (X, w, state, resid, iter, info): X (batch, n) with lo <= X <= hi exactly; w = A^T (b - A x); state -1 at lo,
    0 free, +1 at hi; resid[q] = ||A_q x - b_q||; iter the eliminations taken; info 0, n + 1 at maxit (the last, feasible iterate is
    returned), -1 for bounds that are no box and j + 1 for an exactly zero free column j (the other outputs of such a member read 0).  A
    member with an info word does not raise."""
    At = _packed_batch(A, "lstsq_bounded_batched")
    batch, n, m = At.shape
    b = np.asarray(b, dtype=np.float64)
    if b.ndim == 3 and b.shape[2] == 1:
        b = b[:, :, 0]
    if b.shape != (batch, m):
        raise QRError(f"lstsq_bounded_batched: b must be ({batch}, {m}), one right-hand side per member, got {b.shape}", QR_E_ARG)
    b = np.ascontiguousarray(b)
    lo = _bound_batch(lo, batch, n, "lstsq_bounded_batched", "lo")
    hi = _bound_batch(hi, batch, n, "lstsq_bounded_batched", "hi")
    X = np.empty((batch, n))
    w = np.empty((batch, n))
    resid = np.empty(batch)
    state = np.zeros((max(batch, 1), n), dtype=np.intc)
    it = np.zeros(max(batch, 1), dtype=np.intc)
    info = np.zeros(max(batch, 1), dtype=np.intc)
    rc = lib.qr_lstsq_bounded_batched(_p(At), m, n, _p(b), None if lo is None else _p(lo), None if hi is None else _p(hi), int(maxit), batch,
                                      _p(X), _p(w), state.ctypes.data_as(_ip), _p(resid), it.ctypes.data_as(_ip), info.ctypes.data_as(_ip))
    if rc != QR_E_SINGULAR:
        check(rc, "qr_lstsq_bounded_batched")
    return X, w, state[:batch].astype(np.int64), resid, it[:batch].astype(np.int64), info[:batch].astype(np.int64)


def nnls_batched(A, b, maxit=0):
    """non-negative least squares, min ||A_q x - b_q|| subject to x >= 0, for every member: lstsq_bounded_batched with lo = 0"""
    A = np.asarray(A)
    if A.ndim != 3:
        raise QRError(f"nnls_batched: expected an array of shape (batch, rows, cols), got {A.shape}", QR_E_ARG)
    return lstsq_bounded_batched(A, b, lo=np.zeros(A.shape[2]), hi=None, maxit=maxit)


def lsei_batched_max_rows(n, mg):
    """the most rows Plan.lsei_batched takes for n unknowns and mg constraint rows (qr_lsei_batched_max_rows; 0: (n, mg) is not taken at
    all; no device)"""
    return lib.qr_lsei_batched_max_rows(int(n), int(mg))


def lstsq_inequality_batched(A, b, G, h, neq=0, maxit=0, rcond=0.0):
    """min ||A_q x - b_q|| subject to G_q(0:neq) x = h_q(0:neq), G_q(neq:) x >= h_q(neq:) for every member of A (batch, m, n) and b
    (batch, m) through qr_lstsq_inequality_batched (Lawson & Hanson's LSEI by a dual active-set loop, the loop of every member on the
    device).  G: (mg, n) (shared by all members) or (batch, mg, n); h: (mg,) or (batch, mg); mg <= 64.  maxit: the most candidates per
    member (<= 0: 3 mg + 1); rcond: the dependence test of a row against the set (<= 0: n eps).  Returns (X, mu, s, state, resid, iter,
    info): X (batch, n); mu (batch, mg) with A^T (A x - b) = G^T mu, > 0 on the inequalities of the set and exactly 0 off it; s = G x - h;
    state 1 in the set, else 0; resid[q] = ||A_q x - b_q||; iter the candidates taken; info 0, n + 1 at maxit (the last accepted pair
    is returned, s shows what it still violates), -2 infeasible, -3 equalities exactly dependent, i + 1 an exactly zero R_a(i,i) (the
    other outputs of such a member read 0).  A member with an info word does not raise."""
    what = "lstsq_inequality_batched"
    At = _packed_batch(A, what)
    batch, n, m = At.shape
    b = np.asarray(b, dtype=np.float64)
    if b.ndim == 3 and b.shape[2] == 1:
        b = b[:, :, 0]
    if b.shape != (batch, m):
        raise QRError(f"{what}: b must be ({batch}, {m}), one right-hand side per member, got {b.shape}", QR_E_ARG)
    b = np.ascontiguousarray(b)
    G = np.asarray(G, dtype=np.float64)
    if G.ndim == 2:
        G = np.broadcast_to(G, (batch,) + G.shape)
    if G.ndim != 3 or G.shape[0] != batch or G.shape[2] != n:
        raise QRError(f"{what}: G must be (mg, {n}) or ({batch}, mg, {n}), got {G.shape}", QR_E_ARG)
    mg = G.shape[1]
    Gt = np.ascontiguousarray(G.transpose(0, 2, 1))           # column-major members
    h = _bound_batch(h, batch, mg, what, "h")
    if h is None:
        raise QRError(f"{what}: h is required", QR_E_ARG)
    X = np.empty((batch, n))
    mu = np.empty((batch, mg))
    s = np.empty((batch, mg))
    resid = np.empty(batch)
    state = np.zeros((max(batch, 1), mg), dtype=np.intc)
    it = np.zeros(max(batch, 1), dtype=np.intc)
    info = np.zeros(max(batch, 1), dtype=np.intc)
    rc = lib.qr_lstsq_inequality_batched(_p(At), m, n, _p(b), _p(Gt), mg, int(neq), _p(h), int(maxit), float(rcond), batch, _p(X), _p(mu),
                                         _p(s), state.ctypes.data_as(_ip), _p(resid), it.ctypes.data_as(_ip), info.ctypes.data_as(_ip))
    if rc != QR_E_SINGULAR:
        check(rc, "qr_lstsq_inequality_batched")
    return X, mu, s, state[:batch].astype(np.int64), resid, it[:batch].astype(np.int64), info[:batch].astype(np.int64)


LM_OPTION_NAMES = tuple(k for k, _ in LmOptions._fields_)


def lm_options(**options):
    """qr_lm_options: MINPACK lmder1's defaults (qr_lm_options_default) with the given fields replaced"""
    o = LmOptions()
    lib.qr_lm_options_default(C.byref(o))
    for k, v in options.items():
        if k not in LM_OPTION_NAMES:
            raise QRError(f"lm options: unknown option {k!r} (known: {', '.join(LM_OPTION_NAMES)})", QR_E_ARG)
        setattr(o, k, v)
    return o


def _lm_bounds_host(bounds, batch, n, who):
    """bounds = (lo, hi) -> two packed (batch, n) arrays or None; each of lo, hi: None (unbounded), a scalar, (n,) or (batch, n)"""
    try:
        lo, hi = bounds
    except (TypeError, ValueError):
        raise QRError(f"{who}: bounds must be a pair (lo, hi)", QR_E_ARG)
    out = []
    for v in (lo, hi):
        if v is None:
            out.append(None)
            continue
        v = np.asarray(v, dtype=np.float64)
        if v.ndim == 2 and v.shape != (batch, n) or v.ndim == 1 and v.shape != (n,) or v.ndim > 2:
            raise QRError(f"{who}: a bound must be a scalar, ({n},) or ({batch}, {n}), got {v.shape}", QR_E_ARG)
        out.append(np.ascontiguousarray(np.broadcast_to(v, (batch, n))))
    return out


def lstsq_lm_batched(fun, jac, x0, D=None, m=None, bounds=None, **options):
    """min ||f_q(x)|| for every member by Levenberg-Marquardt (MINPACK lmder's iteration, the loop of every member on the device) through
    qr_lstsq_lm_batched.  fun: numpy (batch, n) -> (batch, m); jac: (batch, n) -> (batch, m, n); x0: (batch, n); D: the scaling of mode 2
    (n,) or (batch, n); m: the number of residuals (None: fun is called once on x0 to find it); options: the fields of qr_lm_options.
    bounds: None, or (lo, hi) for lo <= x <= hi through qr_lstsq_lm_bounded_batched (mi355x_qr.h section 8n; each of lo, hi: None, a
    scalar, (n,) or (batch, n); entries may be infinite).
    Returns (X, fnorm, nfev, njev, status, info): status is MINPACK's info (1 .. 8), or -1 for a member with an info word (which does
    not raise)."""
    x0 = np.asarray(x0, dtype=np.float64)
    if x0.ndim != 2:
        raise QRError(f"lstsq_lm_batched: x0 must be (batch, n), got {x0.shape}", QR_E_ARG)
    batch, n = x0.shape
    if m is None:
        m = int(np.asarray(fun(x0)).shape[1]) if batch else n
    o = lm_options(**options)
    if D is not None:
        D = np.asarray(D, dtype=np.float64)
        if D.ndim == 1:
            D = np.broadcast_to(D, (batch, D.shape[0]))
        if D.shape != (batch, n):
            raise QRError(f"lstsq_lm_batched: D must be ({n},) or ({batch}, {n}), got {D.shape}", QR_E_ARG)
        D = np.ascontiguousarray(D)
    if bounds is not None:
        lo, hi = _lm_bounds_host(bounds, batch, n, "lstsq_lm_batched")
    raised = []

    def model(_user, what, X, nb, F, J):
        try:
            Xn = np.ctypeslib.as_array(X, shape=(nb, n))
            if what == 2:
                np.ctypeslib.as_array(J, shape=(nb, n, m))[...] = np.asarray(jac(Xn), dtype=np.float64).reshape(nb, m, n).transpose(0, 2, 1)
            else:
                np.ctypeslib.as_array(F, shape=(nb, m))[...] = np.asarray(fun(Xn), dtype=np.float64).reshape(nb, m)
            return 0
        except Exception as e:      # (an exception must not cross the C frames)
            raised.append(e)
            return QR_E_ARG

    X = np.ascontiguousarray(x0).copy()
    fnorm = np.zeros(batch)
    nfev, njev, status, info = (np.zeros(max(batch, 1), dtype=np.intc) for _ in range(4))
    tail = (C.byref(o), _p(fnorm), nfev.ctypes.data_as(_ip), njev.ctypes.data_as(_ip), status.ctypes.data_as(_ip), info.ctypes.data_as(_ip))
    Dp = None if D is None else _p(D)
    if bounds is None:
        name, rc = "qr_lstsq_lm_batched", lib.qr_lstsq_lm_batched(LM_FCN(model), None, m, n, batch, _p(X), Dp, *tail)
    else:
        name, rc = "qr_lstsq_lm_bounded_batched", lib.qr_lstsq_lm_bounded_batched(
            LM_FCN(model), None, m, n, batch, _p(X), None if lo is None else _p(lo), None if hi is None else _p(hi), Dp, *tail)
    if raised:
        raise raised[0]
    if rc != QR_E_SINGULAR:
        check(rc, name)
    return X, fnorm, nfev[:batch].astype(np.int64), njev[:batch].astype(np.int64), status[:batch].astype(np.int64), info[:batch].astype(np.int64)


QR_LOSS_LS, QR_LOSS_HUBER, QR_LOSS_BISQUARE = 0, 1, 2
_LOSSES = {"ls": QR_LOSS_LS, "huber": QR_LOSS_HUBER, "bisquare": QR_LOSS_BISQUARE}


def irls_batched_max_rows(n):
    """the most rows Plan.irls_batched takes for n unknowns (qr_irls_batched_max_rows; 0: n is not taken at all; no device)"""
    return lib.qr_irls_batched_max_rows(int(n))


def lstsq_robust_batched(A, b, loss="huber", tune=None, weights=None, scale=None, x0=None, tol=1e-8, maxit=0):
    """A robust fit of every member of A (batch, m, n), m >= n, and b (batch, m) through qr_lstsq_robust_batched (iteratively reweighted
    least squares, the reweighting loop of every member on the device).  loss: "huber", "bisquare" or "ls" (or a QR_LOSS_* value); tune:
    the constant k or c (None: 1.345 / 4.685); weights: None, (m,) (shared by all members) or (batch, m) prior weights >= 0, a zero
    masks the row; scale: None (the MAD scale of every iterate), a scalar or (batch,); x0: None or (batch, n), a warm start; tol: the
    relative change of x that stops; maxit: the most solves per member (<= 0: 50).  Returns (X, w, scale, resid, iter, status, info): X
    (batch, n); the robust weights w (batch, m); resid[q] = ||b_q - A_q x|| over the included rows; status 0 converged, 2 a zero scale,
    3 maxit solves (the last iterate is returned); info 0, -1 for a bad weight or scale, -2 for fewer than n rows of positive weight,
    i + 1 for an exactly zero R(i,i) (the other outputs of such a member read 0).  A member with an info word does not raise."""
    At = _packed_batch(A, "lstsq_robust_batched")
    batch, n, m = At.shape
    b = np.asarray(b, dtype=np.float64)
    if b.ndim == 3 and b.shape[2] == 1:
        b = b[:, :, 0]
    if b.shape != (batch, m):
        raise QRError(f"lstsq_robust_batched: b must be ({batch}, {m}), one right-hand side per member, got {b.shape}", QR_E_ARG)
    b = np.ascontiguousarray(b)
    if isinstance(loss, str):
        if loss not in _LOSSES:
            raise QRError(f"lstsq_robust_batched: loss must be one of {sorted(_LOSSES)}, got {loss!r}", QR_E_ARG)
        loss = _LOSSES[loss]
    weights = _bound_batch(weights, batch, m, "lstsq_robust_batched", "weights")
    x0 = _bound_batch(x0, batch, n, "lstsq_robust_batched", "x0")
    if scale is not None:
        scale = np.asarray(scale, dtype=np.float64)
        if scale.ndim == 0:
            scale = np.broadcast_to(scale, (batch,))
        if scale.shape != (batch,):
            raise QRError(f"lstsq_robust_batched: scale must be a scalar or ({batch},), got {scale.shape}", QR_E_ARG)
        scale = np.ascontiguousarray(scale)
    X = np.empty((batch, n))
    w = np.empty((batch, m))
    sc, resid = np.empty(batch), np.empty(batch)
    it, status, info = (np.zeros(max(batch, 1), dtype=np.intc) for _ in range(3))
    rc = lib.qr_lstsq_robust_batched(_p(At), m, n, _p(b), int(loss), 0.0 if tune is None else float(tune), None if weights is None else _p(weights),
                                     None if scale is None else _p(scale), None if x0 is None else _p(x0), float(tol), int(maxit), batch,
                                     _p(X), _p(w), _p(sc), _p(resid), it.ctypes.data_as(_ip), status.ctypes.data_as(_ip),
                                     info.ctypes.data_as(_ip))
    if rc != QR_E_SINGULAR:
        check(rc, "qr_lstsq_robust_batched")
    return X, w, sc, resid, it[:batch].astype(np.int64), status[:batch].astype(np.int64), info[:batch].astype(np.int64)


def lstsq_weighted_batched(A, b, weights):
    """weighted least squares, min sum_i weights_i (b_q - A_q x)_i^2, for every member: lstsq_robust_batched with the squared loss.
    Returns (X, resid, info)."""
    X, _, _, resid, _, _, info = lstsq_robust_batched(A, b, loss=QR_LOSS_LS, weights=weights)
    return X, resid, info


QR_COV_UNSCALED, QR_COV_SCALED = 0, 1


def stats_batched_max_rows(n):
    """the most rows Plan.gels_stats_batched takes for n unknowns (qr_stats_batched_max_rows; 0: n is not taken at all; no device)"""
    return lib.qr_stats_batched_max_rows(int(n))


def lstsq_stats_batched(A, b, weights=None, scaled=True):
    """The weighted least-squares fit of every member of A (batch, m, n), m >= n, and b (batch, m) with its statistics, through
    qr_lstsq_stats_batched (one launch for the whole batch).  weights: None, (m,) (shared by all members) or (batch, m) prior weights
    >= 0, a zero excludes the row; scaled: the covariance is sigma2 (A^T P A)^-1 (True) or (A^T P A)^-1 (False).  Returns a dict: x
    (batch, n); resid (batch, m), b - A x with exact zeros on excluded rows; leverage (batch, m); sigma2 (batch,), sum p e^2 / dof; dof
    (batch,); cov (batch, n, n); se (batch, n); info (batch,): 0, -1 for a bad weight, -2 for fewer than n rows of positive weight, -3
    for scaled without a degree of freedom, i + 1 for an exactly zero R(i,i) (the other outputs of such a member read 0).  A member
    with an info word does not raise."""
    At = _packed_batch(A, "lstsq_stats_batched")
    batch, n, m = At.shape
    b = np.asarray(b, dtype=np.float64)
    if b.ndim == 3 and b.shape[2] == 1:
        b = b[:, :, 0]
    if b.shape != (batch, m):
        raise QRError(f"lstsq_stats_batched: b must be ({batch}, {m}), one right-hand side per member, got {b.shape}", QR_E_ARG)
    b = np.ascontiguousarray(b)
    weights = _bound_batch(weights, batch, m, "lstsq_stats_batched", "weights")
    X, se = np.empty((batch, n)), np.empty((batch, n))
    E, H = np.empty((batch, m)), np.empty((batch, m))
    sig = np.empty(batch)
    cov = np.empty((batch, n, n))
    dof, info = (np.zeros(max(batch, 1), dtype=np.intc) for _ in range(2))
    rc = lib.qr_lstsq_stats_batched(_p(At), m, n, _p(b), None if weights is None else _p(weights), QR_COV_SCALED if scaled else QR_COV_UNSCALED,
                                    batch, _p(X), _p(E), _p(H), _p(sig), dof.ctypes.data_as(_ip), _p(cov), _p(se), info.ctypes.data_as(_ip))
    if rc != QR_E_SINGULAR:
        check(rc, "qr_lstsq_stats_batched")
    return {"x": X, "resid": E, "leverage": H, "sigma2": sig, "dof": dof[:batch].astype(np.int64), "cov": cov, "se": se,
            "info": info[:batch].astype(np.int64)}


def tpqrt_max_rows():
    """the most rows one Plan.tpqrt / Plan.tpmqrt call takes (qr_tpqrt_max_rows)"""
    return lib.qr_tpqrt_max_rows()


TPQRT_PANEL = 32        # QR_TPQRT_PANEL: rows of the block T that Plan.tpqrt writes


def jsvd_rounds(n):
    """(nblk, rounds) of the Jacobi tournament over the column blocks of an n-column matrix (qr_jsvd_rounds; no device)"""
    nblk, rounds = C.c_int(), C.c_int()
    check(lib.qr_jsvd_rounds(n, C.byref(nblk), C.byref(rounds)), "qr_jsvd_rounds")
    return nblk.value, rounds.value


def jsvd_round_pairs(n, round):
    """[(p, q)] the block pairs of one round, exactly what the device code runs (qr_jsvd_round_pairs; no device)"""
    nblk, _ = jsvd_rounds(n)
    cap = max(1, nblk // 2)
    buf = (C.c_int * (2 * cap))()
    cnt = lib.qr_jsvd_round_pairs(n, round, buf, cap)
    if cnt < 0:
        check(cnt, "qr_jsvd_round_pairs")
    return [(buf[2 * i], buf[2 * i + 1]) for i in range(cnt)]


def _tall(A, what):
    A = _f(A)
    if A.ndim != 2 or A.shape[1] < 1 or A.shape[0] < A.shape[1]:
        raise QRError(f"{what}: {A.shape} (a 2-D array with m >= n >= 1 is required; transpose a wide one)", QR_E_ARG)
    return A


def svd(A, compute_uv=True):
    """The SVD of a tall m x n A (m >= n) through qr_svd: (U m x n, S descending, V n x n) with A = U diag(S) V^T -- V, not numpy's V^T --
    or S alone with compute_uv False."""
    A = _tall(A, "svd")
    m, n = A.shape
    S = np.empty(n)
    if not compute_uv:
        check(lib.qr_svd(_p(A), m, n, _p(S), None, None), "qr_svd")
        return S
    U = np.empty((m, n), order="F")
    V = np.empty((n, n), order="F")
    check(lib.qr_svd(_p(A), m, n, _p(S), _p(U), _p(V)), "qr_svd")
    return U, S, V


def svdvals(A):
    """the singular values of a tall A, descending"""
    return svd(A, compute_uv=False)


def cond(A):
    """the 2-norm condition number sigma_max / sigma_min of a tall A; inf when sigma_min == 0"""
    S = svdvals(A)
    return float(S[0] / S[-1]) if S[-1] > 0.0 else float("inf")


def lstsq_svd(A, B, rcond=None):
    """The minimum-norm solution of min ||A X - B|| for an m x n A (m >= n) of any rank through qr_lstsq_svd (LAPACK dgelss):
    returns (X, resid, rank, S).  rcond None: max(m, n) eps.  A 1-D B is one column (X and resid then 1-D / a scalar)."""
    A = _f(A)
    m, n = A.shape
    B = np.asarray(B, dtype=np.float64)
    vec = B.ndim == 1
    B = _f(B.reshape(-1, 1) if vec else B)
    if B.shape[0] != m:
        raise QRError(f"lstsq_svd: B has {B.shape[0]} rows, A has {m}", QR_E_ARG)
    nrhs = B.shape[1]
    X = np.empty((max(n, 1), nrhs), order="F")
    resid = np.empty(nrhs)
    S = np.empty(max(n, 1))
    rank = C.c_int()
    check(lib.qr_lstsq_svd(_p(A), m, n, _p(B), nrhs, -1.0 if rcond is None else float(rcond), _p(X), _p(resid), C.byref(rank), _p(S)),
          "qr_lstsq_svd")
    return (X[:, 0], resid[0], rank.value, S) if vec else (X, resid, rank.value, S)


def qr_pivoted(A):
    """A[:, jpvt] = Q R with decreasing |diag R| (qr_geqp3_dev): returns (Q m x n, R n x n, jpvt) for a host array."""
    import torch
    A = _f(A)
    m, n = A.shape
    if n < 1 or m < n:
        raise QRError(f"qr_pivoted: {m} x {n} (m >= n >= 1 is required)", QR_E_ARG)
    p = Plan(m, n)
    try:
        dA = to_device_colmajor(A)
        dtau = torch.zeros(n, dtype=torch.float64, device="cuda")
        dj = torch.zeros(n, dtype=torch.int32, device="cuda")
        dQ = torch.zeros((n, m), dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        p.geqp3(dA, m, n, m, dj, dtau)
        p.applyq(dA, m, n, m, dtau, dQ, n, m, True)
        p.sync()
        F = from_device_colmajor(dA)
        return from_device_colmajor(dQ), np.triu(F[:n]), dj.cpu().numpy().astype(np.int64)
    finally:
        p.close()


def release_cached_plans():
    check(lib.qr_release_cached_plans(), "qr_release_cached_plans")


def device_info():
    name = C.create_string_buffer(64)
    cus, clk, mem = C.c_int(), C.c_int(), C.c_size_t()
    check(lib.qr_device_info(name, 64, C.byref(cus), C.byref(clk), C.byref(mem)), "qr_device_info")
    return {"arch": name.value.decode(), "compute_units": cus.value, "clock_khz": clk.value, "hbm_bytes": mem.value}


def probe_mfma_f64_tflops():
    """{mfma_tflops, mfma_clock_ghz, valu_tflops}: sustained fp64 rates measured on this device."""
    v = (C.c_double * 3)()
    check(lib.qr_probe_mfma_f64_tflops(v), "probe")
    return {"mfma_f64_tflops": v[0], "mfma_clock_ghz": v[1], "valu_f64_tflops": v[2]}


def probe_copy_gbps():
    v = C.c_double()
    check(lib.qr_probe_copy_gbps(C.byref(v)), "probe")
    return v.value


# ------------------------------------------------------------------------------------------------
# device-resident API.  Device buffers are anything with .data_ptr() (torch tensors) or raw ints.
# A column-major m x n matrix with leading dimension ld is a flat float64 buffer of ld*n elements;
# `colmajor(m, n)` makes one as a torch tensor of shape (n, m) whose .T is the matrix.
# ------------------------------------------------------------------------------------------------
def _dptr(x):
    if x is None:
        return None
    if isinstance(x, int):
        return x
    return x.data_ptr()


def colmajor(m, n, device="cuda"):
    import torch
    return torch.empty((n, m), dtype=torch.float64, device=device)


def to_device_colmajor(A, device="cuda"):
    """numpy (m x n) -> torch (n, m) buffer holding A column-major."""
    import torch
    t = torch.from_numpy(np.ascontiguousarray(np.asarray(A, dtype=np.float64).T)).to(device)
    torch.cuda.synchronize()      # the copy ran on torch's stream; the plan's streams are not ordered with it
    return t


def from_device_colmajor(t):
    return np.asfortranarray(t.detach().cpu().numpy().T)


class Plan:
    """qr_plan wrapper.  The plan's HIP stream is independent of torch's current stream: call
    torch.cuda.synchronize() (or Plan.sync) at the hand-over points."""

    def __init__(self, m, n, nb=0, ib=0, borrowed=None):
        self.h = None
        self.owned = borrowed is None
        if borrowed is not None:            # a qr_plan that lives inside another object (TsqrPlan): used, never destroyed here
            self.h, self.m, self.n = _vp(borrowed), m, n
            return
        h = _vp()
        check(lib.qr_plan_create(C.byref(h), m, n, nb, ib), "qr_plan_create")
        self.h, self.m, self.n = h, m, n

    def close(self):
        if self.h and self.owned:
            lib.qr_plan_destroy(self.h)
        self.h = None

    __del__ = close

    def sync(self):
        check(lib.qr_plan_sync(self.h), "qr_plan_sync")

    def set_guard_mode(self, latch):
        """latch = True: qr_geqrf_dev never waits for the device; a refused full-width tall panel is reported by sync() (QR_E_REFUSED)"""
        check(lib.qr_plan_set_guard_mode(self.h, int(bool(latch))), "qr_plan_set_guard_mode")

    def route_stats(self):
        out = (C.c_longlong * 4)()
        check(lib.qr_plan_route_stats(self.h, out), "qr_plan_route_stats")
        rt = (C.c_longlong * 2)()
        check(lib.qr_plan_retry_stats(self.h, rt), "qr_plan_retry_stats")
        return {"tall_panels": out[0], "tall_panels_refused": out[1], "fused_leaf_fallbacks": out[2], "fused_stalls": out[3],
                "tall_panels_retried": rt[0], "tall_panels_retry_accepted": rt[1]}

    @property
    def stream(self):
        return lib.qr_plan_stream(self.h)

    def info(self):
        nb, ib, la = C.c_int(), C.c_int(), C.c_int()
        check(lib.qr_plan_info(self.h, C.byref(nb), C.byref(ib), C.byref(la)), "qr_plan_info")
        return nb.value, ib.value, bool(la.value)

    @property
    def nb(self):
        return self.info()[0]

    def geqrf(self, dA, m, n, lda, dtau):
        check(lib.qr_geqrf_dev(self.h, _dptr(dA), m, n, lda, _dptr(dtau)), "qr_geqrf_dev")

    def applyq(self, dA, m, n, lda, dtau, dC, ccols, ldc, identity_start):
        check(lib.qr_applyq_dev(self.h, _dptr(dA), m, n, lda, _dptr(dtau), _dptr(dC), ccols, ldc,
                                int(identity_start)), "qr_applyq_dev")

    def build_t(self, dA, m, n, lda, dtau, dT, ldt):
        """T of every outer block into dT (nb x n, ldt >= nb): qr_build_t_dev"""
        check(lib.qr_build_t_dev(self.h, _dptr(dA), m, n, lda, _dptr(dtau), _dptr(dT), ldt), "qr_build_t_dev")

    def ormqr(self, trans, dA, m, n, lda, dtau, dC, nrhs, ldc, dT=None, ldt=0):
        """dC <- Q^T dC (trans 'T') or Q dC ('N'); dT from build_t, or None: rebuilt panel by panel"""
        check(lib.qr_ormqr_dev(self.h, trans.encode(), _dptr(dA), m, n, lda, _dptr(dtau), _dptr(dT), ldt, _dptr(dC), nrhs, ldc),
              "qr_ormqr_dev")

    def solve_r(self, dA, n, lda, dB, nrhs, ldb):
        """dB (n x nrhs) <- R^-1 dB, R = upper triangle of the factored dA"""
        check(lib.qr_solve_r_dev(self.h, _dptr(dA), n, lda, _dptr(dB), nrhs, ldb), "qr_solve_r_dev")

    def gels(self, dA, m, n, lda, dtau, dB, nrhs, ldb):
        """dgels on the device: factors dA in place, dB rows 0..n-1 = X, rows n..m-1 = the tail of Q^T B"""
        check(lib.qr_gels_dev(self.h, _dptr(dA), m, n, lda, _dptr(dtau), _dptr(dB), nrhs, ldb), "qr_gels_dev")

    def solve_rt(self, dA, n, lda, dB, nrhs, ldb):
        """dB (n x nrhs) <- R^-T dB, R = upper triangle of the factored dA"""
        check(lib.qr_solve_rt_dev(self.h, _dptr(dA), n, lda, _dptr(dB), nrhs, ldb), "qr_solve_rt_dev")

    def minnorm(self, dA, m, n, lda, dtau, dB, nrhs, ldb, dT=None, ldt=0):
        """dB (m x nrhs; rows 0..n-1 = B) <- Q [R^-T B ; 0], the minimum-norm solution of A^T X = B, from existing factors"""
        check(lib.qr_minnorm_dev(self.h, _dptr(dA), m, n, lda, _dptr(dtau), _dptr(dT), ldt, _dptr(dB), nrhs, ldb), "qr_minnorm_dev")

    def gels_t(self, dA, m, n, lda, dtau, dB, nrhs, ldb):
        """dgels('T') on the device: factors dA (m x n, m >= n) in place, dB (m x nrhs; rows 0..n-1 = B) <- minimum-norm X of A^T X = B"""
        check(lib.qr_gels_t_dev(self.h, _dptr(dA), m, n, lda, _dptr(dtau), _dptr(dB), nrhs, ldb), "qr_gels_t_dev")

    def transpose(self, dS, rows, cols, lds, dD, ldd):
        """dD (cols x rows, ldd) = dS (rows x cols, lds)^T, out of place"""
        check(lib.qr_transpose_dev(self.h, _dptr(dS), rows, cols, lds, _dptr(dD), ldd), "qr_transpose_dev")

    def gels_wide(self, dA, m, n, lda, dF, ldf, dtau, dB, nrhs, ldb):
        """dgels('N', m <= n) on a plan for n x m: dA (wide, untouched), dF (n x m) <- factors of A^T, dB (n x nrhs; rows 0..m-1 = B) <- X"""
        check(lib.qr_gels_wide_dev(self.h, _dptr(dA), m, n, lda, _dptr(dF), ldf, _dptr(dtau), _dptr(dB), nrhs, ldb), "qr_gels_wide_dev")

    def tpqrt(self, dR, n, ldr, dB, p, ldb, dT, ldt):
        """dtpqrt (L = 0): [R ; B] = Q' [R' ; 0] in place: dR (n x n upper triangle) <- R', dB (p x n) <- V, dT (32 x n) <- the block T"""
        check(lib.qr_tpqrt_dev(self.h, _dptr(dR), n, ldr, _dptr(dB), p, ldb, _dptr(dT), ldt), "qr_tpqrt_dev")

    def tpmqrt(self, trans, dV, p, n, ldv, dT, ldt, dC1, ldc1, dC2, ldc2, nrhs):
        """dtpmqrt (side 'L'): [C1 ; C2] <- Q'^T [C1 ; C2] (trans 'T') or Q' [C1 ; C2] ('N') with dV, dT from tpqrt"""
        check(lib.qr_tpmqrt_dev(self.h, trans.encode(), _dptr(dV), p, n, ldv, _dptr(dT), ldt, _dptr(dC1), ldc1, _dptr(dC2), ldc2, nrhs),
              "qr_tpmqrt_dev")

    def tphqrt(self, dR, n, ldr, dB, p_add, p_del, ldb, dT, ldt):
        """the signed-row update: dB's first p_add rows are added to the triangle dR, its last p_del rows removed; dB <- V, dT <- the
        block T.  Waits for the result.  Raises QRError (status QR_E_NOTPD, .info = the failing column + 1) when the removal leaves no
        positive-definite triangle."""
        info = C.c_int(0)
        rc = lib.qr_tphqrt_dev(self.h, _dptr(dR), n, ldr, _dptr(dB), p_add, p_del, ldb, _dptr(dT), ldt, C.byref(info))
        if rc != 0:
            e = QRError(f"qr_tphqrt_dev failed: {strerror(rc)} ({rc}), info = {info.value}", rc)
            e.info = info.value
            raise e

    def tphmqrt(self, dV, p_add, p_del, n, ldv, dT, ldt, dC1, ldc1, dC2, ldc2, nrhs):
        """[C1 ; C2] <- the transformation of tphqrt (the one that took [R ; B] to [R' ; 0]) with dV, dT from it"""
        check(lib.qr_tphmqrt_dev(self.h, _dptr(dV), p_add, p_del, n, ldv, _dptr(dT), ldt, _dptr(dC1), ldc1, _dptr(dC2), ldc2, nrhs),
              "qr_tphmqrt_dev")

    def tphqrt_batched(self, dR, n, ldr, strideR, dB, p_add, p_del, ldb, strideB, dtau, stridetau, dinfo, batch, dC1=None, ldc1=0, strideC1=0,
                       dC2=None, ldc2=0, strideC2=0, nrhs=0):
        """the signed-row update of `batch` triangles: dB_q's first p_add rows are added to dR_q, its last p_del rows removed; dB <- V,
        dtau <- tau (n per member); [dC1 ; dC2] (nrhs columns) ride along; dinfo (batch device ints): 0 or the failing column + 1, and
        such a member is left untouched.  Does not wait."""
        check(lib.qr_tphqrt_batched_dev(self.h, _dptr(dR), n, ldr, strideR, _dptr(dB), p_add, p_del, ldb, strideB, _dptr(dtau), stridetau,
                                        _dptr(dC1), ldc1, strideC1, _dptr(dC2), ldc2, strideC2, nrhs, _dptr(dinfo), batch),
              "qr_tphqrt_batched_dev")

    def tpqrt_batched(self, dR, n, ldr, strideR, dB, p, ldb, strideB, dtau, stridetau, batch, dC1=None, ldc1=0, strideC1=0, dC2=None, ldc2=0,
                      strideC2=0, nrhs=0):
        """the row-append update of `batch` triangles (tphqrt_batched with p_del = 0; it cannot fail)"""
        check(lib.qr_tpqrt_batched_dev(self.h, _dptr(dR), n, ldr, strideR, _dptr(dB), p, ldb, strideB, _dptr(dtau), stridetau, _dptr(dC1), ldc1,
                                       strideC1, _dptr(dC2), ldc2, strideC2, nrhs, batch), "qr_tpqrt_batched_dev")

    def tpmqrt_batched(self, trans, dV, p_add, p_del, n, ldv, strideV, dtau, stridetau, dC1, ldc1, strideC1, dC2, ldc2, strideC2, nrhs, batch):
        """[C1 ; C2]_q <- the transformation of tphqrt_batched / tpqrt_batched (trans 'T') or, for p_del == 0, its inverse ('N')"""
        check(lib.qr_tpmqrt_batched_dev(self.h, trans.encode(), _dptr(dV), p_add, p_del, n, ldv, strideV, _dptr(dtau), stridetau, _dptr(dC1),
                                        ldc1, strideC1, _dptr(dC2), ldc2, strideC2, nrhs, batch), "qr_tpmqrt_batched_dev")

    def minnorm_batched(self, dA, m, n, lda, strideA, dtau, stridetau, dB, nrhs, ldb, strideB, dinfo, batch):
        """dB_q (m x nrhs; rows 0..n-1 = B_q on entry) <- the minimum-norm X_q of A_q^T X = B from the factors of geqrf_batched / geqp3_batched;
        dinfo (batch device int32): 0, or i + 1 for the smallest i with R(i,i) == 0 (that member's dB is untouched)"""
        check(lib.qr_minnorm_batched_dev(self.h, _dptr(dA), m, n, lda, strideA, _dptr(dtau), stridetau, _dptr(dB), nrhs, ldb, strideB,
                                         _dptr(dinfo), batch), "qr_minnorm_batched_dev")

    def gels_t_batched(self, dA, m, n, lda, strideA, dtau, stridetau, dB, nrhs, ldb, strideB, dinfo, batch):
        """dgels 'T' (m >= n) of `batch` small matrices: dA factored in place, dB and dinfo as minnorm_batched"""
        check(lib.qr_gels_t_batched_dev(self.h, _dptr(dA), m, n, lda, strideA, _dptr(dtau), stridetau, _dptr(dB), nrhs, ldb, strideB,
                                        _dptr(dinfo), batch), "qr_gels_t_batched_dev")

    def transpose_batched(self, dS, rows, cols, lds, strideS, dD, ldd, strideD, batch):
        """dD_q (cols x rows) <- dS_q^T (rows x cols), out of place, rows and cols <= 512"""
        check(lib.qr_transpose_batched_dev(self.h, _dptr(dS), rows, cols, lds, strideS, _dptr(dD), ldd, strideD, batch),
              "qr_transpose_batched_dev")

    def gels_wide_batched(self, dA, m, n, lda, strideA, dF, ldf, strideF, dtau, stridetau, dB, nrhs, ldb, strideB, dinfo, batch):
        """dgels 'N' (m <= n) of `batch` small wide matrices: dA untouched, dF (n x m) and dtau (m) <- the factors of A_q^T, dB_q (n x nrhs;
        rows 0..m-1 = B_q on entry) <- the minimum-norm X_q; dinfo as minnorm_batched"""
        check(lib.qr_gels_wide_batched_dev(self.h, _dptr(dA), m, n, lda, strideA, _dptr(dF), ldf, strideF, _dptr(dtau), stridetau, _dptr(dB),
                                           nrhs, ldb, strideB, _dptr(dinfo), batch), "qr_gels_wide_batched_dev")

    def damped_batched(self, dR, n, ldr, strideR, dZ, nrhs, ldz, strideZ, dlam, nlam, stridelam, dX, ldx, strideX, dinfo, batch, drss=None,
                       djpvt=None, stridejpvt=0, dD=None, strideD=0, flip=False, dxnorm=None, dresid=None):
        """the damped solves min ||A x - b||^2 + lam_k^2 ||D x||^2 of `batch` members from factors that exist: dR (n x n, upper triangle),
        dZ (n x nrhs, the top of Q^T B), drss (tail sums of squares), djpvt (the factors are geqp3_batched's), flip (the triangle is the
        reversed transpose of R: the wide case).  dX: n x (nlam * nrhs) per member; dinfo: nlam ints per member"""
        check(lib.qr_damped_batched_dev(self.h, _dptr(dR), n, ldr, strideR, _dptr(dZ), nrhs, ldz, strideZ, _dptr(drss), _dptr(djpvt), stridejpvt,
                                        _dptr(dD), strideD, _dptr(dlam), nlam, stridelam, int(bool(flip)), _dptr(dX), ldx, strideX, _dptr(dxnorm),
                                        _dptr(dresid), _dptr(dinfo), batch), "qr_damped_batched_dev")

    def gels_damped_batched(self, dA, m, n, lda, strideA, dtau, stridetau, dB, nrhs, ldb, strideB, dlam, nlam, stridelam, dX, ldx, strideX, dinfo,
                            batch, dD=None, strideD=0, dxnorm=None, dresid=None):
        """m >= n: dA factored in place (as geqrf_batched leaves it), dB <- Q^T B in all rows, the damped solutions of every lam to dX"""
        check(lib.qr_gels_damped_batched_dev(self.h, _dptr(dA), m, n, lda, strideA, _dptr(dtau), stridetau, _dptr(dB), nrhs, ldb, strideB,
                                             _dptr(dD), strideD, _dptr(dlam), nlam, stridelam, _dptr(dX), ldx, strideX, _dptr(dxnorm),
                                             _dptr(dresid), _dptr(dinfo), batch), "qr_gels_damped_batched_dev")

    def gels_damped_wide_batched(self, dA, m, n, lda, strideA, dF, ldf, strideF, dtau, stridetau, dB, nrhs, ldb, strideB, dlam, nlam, stridelam,
                                 dX, ldx, strideX, dinfo, batch, dxnorm=None, dresid=None):
        """m < n, D = I: dA untouched, the factors of A^T to dF and dtau, dB (m x nrhs) read only, the damped solutions (n x (nlam * nrhs))
        to dX"""
        check(lib.qr_gels_damped_wide_batched_dev(self.h, _dptr(dA), m, n, lda, strideA, _dptr(dF), ldf, strideF, _dptr(dtau), stridetau,
                                                  _dptr(dB), nrhs, ldb, strideB, _dptr(dlam), nlam, stridelam, _dptr(dX), ldx, strideX,
                                                  _dptr(dxnorm), _dptr(dresid), _dptr(dinfo), batch), "qr_gels_damped_wide_batched_dev")

    def trust_batched(self, dR, n, ldr, strideR, dZ, ldz, strideZ, ddelta, stridedelta, dX, ldx, strideX, dlam, dinfo, batch, drss=None,
                      djpvt=None, stridejpvt=0, dD=None, strideD=0, dlam0=None, stridelam0=0, rtol=0.1, maxit=10, flip=False, dxnorm=None,
                      dresid=None, diter=None, dstatus=None):
        """the trust-region step of `batch` members from factors that exist (the operands of damped_batched, one right-hand side): per
        member the lam >= 0 to dlam and its x to dX with ||D x|| within rtol of ddelta, found inside one launch; dinfo, diter, dstatus:
        one int per member"""
        check(lib.qr_trust_batched_dev(self.h, _dptr(dR), n, ldr, strideR, _dptr(dZ), ldz, strideZ, _dptr(drss), _dptr(djpvt), stridejpvt,
                                       _dptr(dD), strideD, _dptr(ddelta), stridedelta, _dptr(dlam0), stridelam0, float(rtol), int(maxit),
                                       int(bool(flip)), _dptr(dX), ldx, strideX, _dptr(dlam), _dptr(dxnorm), _dptr(dresid), _dptr(diter),
                                       _dptr(dstatus), _dptr(dinfo), batch), "qr_trust_batched_dev")

    def gels_trust_batched(self, dA, m, n, lda, strideA, dtau, stridetau, dB, ldb, strideB, ddelta, stridedelta, dX, ldx, strideX, dlam, dinfo,
                           batch, dD=None, strideD=0, dlam0=None, stridelam0=0, rtol=0.1, maxit=10, dxnorm=None, dresid=None, diter=None,
                           dstatus=None):
        """m >= n: dA factored in place (as geqrf_batched leaves it), dB (m rows) <- Q^T b in all rows, then the trust-region step"""
        check(lib.qr_gels_trust_batched_dev(self.h, _dptr(dA), m, n, lda, strideA, _dptr(dtau), stridetau, _dptr(dB), ldb, strideB, _dptr(dD),
                                            strideD, _dptr(ddelta), stridedelta, _dptr(dlam0), stridelam0, float(rtol), int(maxit), _dptr(dX),
                                            ldx, strideX, _dptr(dlam), _dptr(dxnorm), _dptr(dresid), _dptr(diter), _dptr(dstatus),
                                            _dptr(dinfo), batch), "qr_gels_trust_batched_dev")

    def gels_trust_wide_batched(self, dA, m, n, lda, strideA, dF, ldf, strideF, dtau, stridetau, dB, ldb, strideB, ddelta, stridedelta, dX, ldx,
                                strideX, dlam, dinfo, batch, dlam0=None, stridelam0=0, rtol=0.1, maxit=10, dxnorm=None, dresid=None,
                                diter=None, dstatus=None):
        """m < n, D = I: dA untouched, the factors of A^T to dF and dtau, dB (m rows) read only, the minimum-norm step of length within
        rtol of ddelta (n rows) to dX"""
        check(lib.qr_gels_trust_wide_batched_dev(self.h, _dptr(dA), m, n, lda, strideA, _dptr(dF), ldf, strideF, _dptr(dtau), stridetau,
                                                 _dptr(dB), ldb, strideB, _dptr(ddelta), stridedelta, _dptr(dlam0), stridelam0, float(rtol),
                                                 int(maxit), _dptr(dX), ldx, strideX, _dptr(dlam), _dptr(dxnorm), _dptr(dresid), _dptr(diter),
                                                 _dptr(dstatus), _dptr(dinfo), batch), "qr_gels_trust_wide_batched_dev")

    def gglse_batched(self, dA, m, n, lda, strideA, dC, p, ldc, strideC, dB, ldb, strideB, dD, ldd, strideD, nrhs, dX, ldx, strideX, dinfo, batch,
                      dL=None, ldl=0, strideL=0, dresid=None, strideres=0):
        """min ||A x - b|| subject to C x = d for `batch` members in one launch: dA (m x n), dC (p x n), dB (m x nrhs) and dD (p x nrhs) are
        read only; x to dX (n x nrhs), the multipliers to dL (p x nrhs) and ||A x - b|| to dresid (nrhs per member) where given; dinfo:
        one int per member (0, i + 1 for R_c(i,i) == 0, p + i + 1 for R_a(i,i) == 0: nothing else is written for that member)"""
        check(lib.qr_gglse_batched_dev(self.h, _dptr(dA), m, n, lda, strideA, _dptr(dC), p, ldc, strideC, _dptr(dB), ldb, strideB, _dptr(dD), ldd,
                                       strideD, nrhs, _dptr(dX), ldx, strideX, _dptr(dL), ldl, strideL, _dptr(dresid), strideres,
                                       _dptr(dinfo), batch), "qr_gglse_batched_dev")

    def bvls_batched(self, dA, m, n, lda, strideA, dB, strideB, dX, strideX, dinfo, batch, dlo=None, dhi=None, stridebnd=0, maxit=0, dW=None,
                     strideW=0, dstate=None, stridestate=0, dresid=None, diter=None):
        """min ||A x - b|| subject to lo <= x <= hi for `batch` members in one launch: dA (m x n, m >= n) and dB (m per member) are read
        only; dlo / dhi (n per member, stridebnd apart, 0: shared; None: that side unbounded); x to dX (n per member), w = A^T (b - A x)
        to dW, the states (int32: -1 at lo, 0 free, +1 at hi) to dstate, ||A x - b|| to dresid and the elimination count (int32) to diter
        where given; maxit <= 0: 3 n; dinfo: one int32 per member (0; n + 1 at maxit, the feasible iterate written; -1 for bad bounds
        and j + 1 for a zero free column j: nothing else is written for that member)"""
        check(lib.qr_bvls_batched_dev(self.h, _dptr(dA), m, n, lda, strideA, _dptr(dB), strideB, _dptr(dlo), _dptr(dhi), stridebnd, int(maxit),
                                      _dptr(dX), strideX, _dptr(dW), strideW, _dptr(dstate), stridestate, _dptr(dresid), _dptr(diter),
                                      _dptr(dinfo), batch), "qr_bvls_batched_dev")

    def lsei_batched(self, dA, m, n, lda, strideA, dB, strideB, dG, mg, neq, ldg, strideG, dH, strideH, dX, strideX, dinfo, batch, maxit=0,
                     rcond=0.0, dMU=None, strideMU=0, dS=None, strideS=0, dstate=None, stridestate=0, dresid=None, diter=None):
        """min ||A x - b|| subject to G(0:neq) x = h(0:neq), G(neq:mg) x >= h(neq:mg) for `batch` members in one launch: dA (m x n), dB (m
        per member), dG (mg x n, strideG 0: shared) and dH (mg per member, strideH 0: shared) are read only; x to dX (n per member), the
        multipliers to dMU, G x - h to dS (mg per member), the set (int32: 1 in it, else 0) to dstate, ||A x - b|| to dresid and the
        candidate count (int32) to diter where given; maxit <= 0: 3 mg + 1; rcond <= 0: n eps; dinfo: one int32 per member (0; n + 1 at
        maxit, the last accepted pair written; -2 infeasible, -3 dependent equalities and i + 1 for a zero R_a(i,i): nothing else is
        written for that member)"""
        check(lib.qr_lsei_batched_dev(self.h, _dptr(dA), m, n, lda, strideA, _dptr(dB), strideB, _dptr(dG), mg, neq, ldg, strideG, _dptr(dH),
                                      strideH, int(maxit), float(rcond), _dptr(dX), strideX, _dptr(dMU), strideMU, _dptr(dS), strideS,
                                      _dptr(dstate), stridestate, _dptr(dresid), _dptr(diter), _dptr(dinfo), batch), "qr_lsei_batched_dev")

    def lm_step_batched(self, lm, dR, ldr, strideR, dZ, zrows, ldz, strideZ, drss=None, djpvt=None, stridejpvt=0):
        """the Levenberg-Marquardt step of every running member of the LmBatched `lm` (created on this plan) from factors that exist, in
        LmBatched.step's place in the protocol: dR (n x n), dZ (the top zrows >= n rows of Q^T f), drss (the squares of the rows that are
        not there, one per member), djpvt (int32, n per member) as for trust_batched"""
        if lm.plan is not self:
            raise QRError("lm_step_batched: the solver was created on another plan", QR_E_ARG)
        check(lib.qr_lm_step_batched_dev(lm.h, _dptr(dR), ldr, strideR, _dptr(dZ), zrows, ldz, strideZ, _dptr(drss), _dptr(djpvt), stridejpvt),
              "qr_lm_step_batched_dev")

    def irls_batched(self, loss, dA, m, n, lda, strideA, dB, strideB, dX, strideX, dinfo, batch, tune=0.0, dprior=None, strideprior=0,
                     dscale_in=None, dX0=None, strideX0=0, tol=1e-8, maxit=0, dW=None, strideW=0, dscale=None, dresid=None, diter=None,
                     dstatus=None):
        """weighted (loss 0), Huber (1) or bisquare (2) fits of `batch` members in one launch: dA (m x n, m >= n) and dB (m per member) are
        read only; dprior (m per member, strideprior apart, 0: shared; None: ones; a zero masks the row); dscale_in (one per member; None:
        the MAD scale); dX0 (n per member; None: a cold start); x to dX (n per member), the robust weights to dW (m per member), the scale
        to dscale, ||b - A x|| to dresid, the solve count and the status (int32: 0 converged, 2 a zero scale, 3 maxit) to diter and
        dstatus where given; tune <= 0: 1.345 / 4.685; maxit <= 0: 50; dinfo: one int32 per member (0; -1 for a bad weight or scale, -2
        for fewer than n rows of positive weight, i + 1 for a zero R(i,i): nothing else is written for that member)"""
        check(lib.qr_irls_batched_dev(self.h, int(loss), float(tune), _dptr(dA), m, n, lda, strideA, _dptr(dB), strideB, _dptr(dprior),
                                      strideprior, _dptr(dscale_in), _dptr(dX0), strideX0, float(tol), int(maxit), _dptr(dX), strideX,
                                      _dptr(dW), strideW, _dptr(dscale), _dptr(dresid), _dptr(diter), _dptr(dstatus), _dptr(dinfo), batch),
              "qr_irls_batched_dev")

    def gels_weighted_batched(self, dA, m, n, lda, strideA, dB, strideB, dprior, strideprior, dX, strideX, dinfo, batch, dresid=None):
        """weighted least squares of `batch` members in one launch (qr_gels_weighted_batched_dev): irls_batched with the squared loss"""
        check(lib.qr_gels_weighted_batched_dev(self.h, _dptr(dA), m, n, lda, strideA, _dptr(dB), strideB, _dptr(dprior), strideprior, _dptr(dX),
                                               strideX, _dptr(dresid), _dptr(dinfo), batch), "qr_gels_weighted_batched_dev")

    def covar_batched(self, dR, n, ldr, strideR, dinfo, batch, dC=None, ldc=0, strideC=0, dse=None, stridese=0, djpvt=None, stridejpvt=0,
                      drank=None, dmult=None):
        """C = mult P [(R11^T R11)^-1 0; 0 0] P^T (to dC, n x n per member) and se = sqrt(diag C) (to dse, n per member) from the upper
        triangle of dR (n x n per member; in-place factors may be passed as they are) in one launch; djpvt (int32, 0-based), drank (int32)
        and dmult (one double per member) default to the identity, n and 1; dinfo: one int32 per member (0; i + 1 for a zero R(i,i); -1 for
        a bad jpvt, rank or multiplier: nothing else is written for that member)"""
        check(lib.qr_covar_batched_dev(self.h, _dptr(dR), n, ldr, strideR, _dptr(djpvt), stridejpvt, _dptr(drank), _dptr(dmult), _dptr(dC), ldc,
                                       strideC, _dptr(dse), stridese, _dptr(dinfo), batch), "qr_covar_batched_dev")

    def leverage_batched(self, dR, n, ldr, strideR, dA, mrows, lda, strideA, dH, strideH, dinfo, batch, dprior=None, strideprior=0, djpvt=None,
                         stridejpvt=0, drank=None):
        """dH[i] = p_i a_i^T (R^T R)^-1 a_i for the mrows rows of dA (the fitted rows or new points; read only) from the upper triangle of
        dR in one launch; dprior (mrows per member, strideprior apart, 0: shared; None: ones; a zero excludes the row); dinfo: one int32
        per member (0; i + 1 for a zero R(i,i); -1 for a bad jpvt, rank or weight)"""
        check(lib.qr_leverage_batched_dev(self.h, _dptr(dR), n, ldr, strideR, _dptr(djpvt), stridejpvt, _dptr(drank), _dptr(dA), mrows, lda,
                                          strideA, _dptr(dprior), strideprior, _dptr(dH), strideH, _dptr(dinfo), batch), "qr_leverage_batched_dev")

    def gels_stats_batched(self, dA, m, n, lda, strideA, dB, strideB, dX, strideX, dinfo, batch, scaled=QR_COV_SCALED, dprior=None, strideprior=0,
                           dE=None, strideE=0, dH=None, strideH=0, dsigma2=None, ddof=None, dC=None, ldc=0, strideC=0, dse=None, stridese=0):
        """the weighted least-squares fit of `batch` members and its statistics in one launch (qr_gels_stats_batched_dev): dA (m x n) and
        dB (m per member) are read only; x to dX, b - A x to dE, the leverages to dH (m per member), sum p e^2 / dof to dsigma2, dof
        (int32) to ddof, the covariance (scaled by sigma2 where scaled) to dC and its standard errors to dse where given; dinfo: one int32
        per member (0; -1 a bad weight, -2 fewer than n rows of positive weight, -3 scaled without a degree of freedom, i + 1 a zero
        R(i,i): nothing else is written for that member)"""
        check(lib.qr_gels_stats_batched_dev(self.h, int(scaled), _dptr(dA), m, n, lda, strideA, _dptr(dB), strideB, _dptr(dprior), strideprior,
                                            _dptr(dX), strideX, _dptr(dE), strideE, _dptr(dH), strideH, _dptr(dsigma2), _dptr(ddof), _dptr(dC), ldc,
                                            strideC, _dptr(dse), stridese, _dptr(dinfo), batch), "qr_gels_stats_batched_dev")

    def geqrf_batched(self, dA, m, n, lda, strideA, dtau, stridetau, batch):
        """dgeqr2 of `batch` small matrices in place (matrix q at dA + q strideA doubles), tau to dtau + q stridetau"""
        check(lib.qr_geqrf_batched_dev(self.h, _dptr(dA), m, n, lda, strideA, _dptr(dtau), stridetau, batch), "qr_geqrf_batched_dev")

    def ormqr_batched(self, trans, dA, m, n, lda, strideA, dtau, stridetau, dC, nrhs, ldc, strideC, batch):
        """dC_q <- Q_q^T dC_q (trans 'T') or Q_q dC_q ('N') with the factors of geqrf_batched"""
        check(lib.qr_ormqr_batched_dev(self.h, trans.encode(), _dptr(dA), m, n, lda, strideA, _dptr(dtau), stridetau, _dptr(dC), nrhs, ldc,
                                       strideC, batch), "qr_ormqr_batched_dev")

    def orgqr_batched(self, dA, m, n, lda, strideA, dtau, stridetau, dQ, ldq, strideQ, batch):
        """the thin m x n Q of every matrix into dQ"""
        check(lib.qr_orgqr_batched_dev(self.h, _dptr(dA), m, n, lda, strideA, _dptr(dtau), stridetau, _dptr(dQ), ldq, strideQ, batch),
              "qr_orgqr_batched_dev")

    def gels_batched(self, dA, m, n, lda, strideA, dtau, stridetau, dB, nrhs, ldb, strideB, dinfo, batch):
        """dgels per matrix: dA factored in place, rows 0..n-1 of dB_q <- X_q; dinfo (batch device ints): 0 or the first zero pivot + 1"""
        check(lib.qr_gels_batched_dev(self.h, _dptr(dA), m, n, lda, strideA, _dptr(dtau), stridetau, _dptr(dB), nrhs, ldb, strideB,
                                      _dptr(dinfo), batch), "qr_gels_batched_dev")

    def geqp3_batched(self, dA, m, n, lda, strideA, djpvt, stridejpvt, dtau, stridetau, batch):
        """dgeqp3 of `batch` small matrices in place: the layout of geqrf_batched, djpvt (int32, n per matrix, 0-based) <- the permutation"""
        check(lib.qr_geqp3_batched_dev(self.h, _dptr(dA), m, n, lda, strideA, _dptr(djpvt), stridejpvt, _dptr(dtau), stridetau, batch),
              "qr_geqp3_batched_dev")

    def rank_batched(self, dA, m, n, lda, strideA, drank, batch, rcond=None):
        """drank (batch device int32) <- the rank of every matrix factored by geqp3_batched; queued, no host wait.  rcond None: max(m, n) eps"""
        check(lib.qr_rank_batched_dev(self.h, _dptr(dA), m, n, lda, strideA, -1.0 if rcond is None else float(rcond), _dptr(drank), batch),
              "qr_rank_batched_dev")

    def _gelsx_batched(self, name, dA, m, n, lda, strideA, djpvt, stridejpvt, dtau, stridetau, dB, nrhs, ldb, strideB, rcond, dresid, drank,
                       batch):
        check(getattr(lib, name)(self.h, _dptr(dA), m, n, lda, strideA, _dptr(djpvt), stridejpvt, _dptr(dtau), stridetau, _dptr(dB), nrhs,
                                 ldb, strideB, -1.0 if rcond is None else float(rcond), _dptr(dresid), _dptr(drank), batch), name)

    def gelsp_batched(self, dA, m, n, lda, strideA, djpvt, stridejpvt, dtau, stridetau, dB, nrhs, ldb, strideB, batch, rcond=None,
                      dresid=None, drank=None):
        """rank-deficient least squares per matrix, the basic solution: rows 0..n-1 of dB_q <- X_q (zero outside the leading rank columns
        of A P); dresid (nrhs per matrix) and drank (batch int32) may be None"""
        self._gelsx_batched("qr_gelsp_batched_dev", dA, m, n, lda, strideA, djpvt, stridejpvt, dtau, stridetau, dB, nrhs, ldb, strideB,
                            rcond, dresid, drank, batch)

    def gelsy_batched(self, dA, m, n, lda, strideA, djpvt, stridejpvt, dtau, stridetau, dB, nrhs, ldb, strideB, batch, rcond=None,
                      dresid=None, drank=None):
        """the same, the minimum-norm solution (LAPACK dgelsy)"""
        self._gelsx_batched("qr_gelsy_batched_dev", dA, m, n, lda, strideA, djpvt, stridejpvt, dtau, stridetau, dB, nrhs, ldb, strideB,
                            rcond, dresid, drank, batch)

    def gesvd_batched(self, jobu, jobv, dA, m, n, lda, strideA, djpvt, stridejpvt, dtau, stridetau, dS, strideS, dinfo, batch, dU=None, ldu=0,
                      strideU=0, dV=None, ldv=0, strideV=0, drank=None, dsweeps=None):
        """the SVD of `batch` small matrices: dA, djpvt, dtau <- the factors of geqp3_batched; dS (n per matrix, descending); jobu 'U': dU
        (m x n per matrix); jobv 'V': dV (n x n per matrix, V itself); drank, dsweeps (int32, optional); dinfo (int32): 1 where the sweep
        limit was reached"""
        check(lib.qr_gesvd_batched_dev(self.h, jobu.encode(), jobv.encode(), _dptr(dA), m, n, lda, strideA, _dptr(djpvt), stridejpvt,
                                       _dptr(dtau), stridetau, _dptr(dS), strideS, _dptr(dU), ldu, strideU, _dptr(dV), ldv, strideV,
                                       _dptr(drank), _dptr(dsweeps), _dptr(dinfo), batch), "qr_gesvd_batched_dev")

    def gesvj(self, jobv, dG, r, n, ldg, dS, dV=None, ldv=0):
        """dgesvj on the device: dG (r x n) <- the left singular vectors, dS <- the values (descending), dV (jobv 'V') <- the right ones;
        returns the sweeps used.  Raises QRError (status QR_E_NOCONV) after JSVD_MAX_SWEEPS sweeps."""
        sw = C.c_int()
        check(lib.qr_gesvj_dev(self.h, jobv.encode(), _dptr(dG), r, n, ldg, _dptr(dS), _dptr(dV), ldv, C.byref(sw)), "qr_gesvj_dev")
        return sw.value

    def gesvd(self, jobu, jobv, dA, m, n, lda, dtau, dS, dU=None, ldu=0, dV=None, ldv=0):
        """the tall SVD on the device: factors dA in place (geqrf's layout), dS <- the values, dU (m x n, jobu 'U'), dV (n x n, jobv 'V');
        returns the sweeps used"""
        sw = C.c_int()
        check(lib.qr_gesvd_dev(self.h, jobu.encode(), jobv.encode(), _dptr(dA), m, n, lda, _dptr(dtau), _dptr(dS), _dptr(dU), ldu,
                               _dptr(dV), ldv, C.byref(sw)), "qr_gesvd_dev")
        return sw.value

    def cond(self, dA, m, n, lda, dtau):
        """sigma_max / sigma_min (inf for a singular matrix); factors dA in place; synchronous"""
        c = C.c_double()
        check(lib.qr_cond_dev(self.h, _dptr(dA), m, n, lda, _dptr(dtau), C.byref(c)), "qr_cond_dev")
        return c.value

    def gelss(self, dA, m, n, lda, dtau, dB, nrhs, ldb, dS, rcond=None):
        """dgelss on the device (minimum-norm solution, any rank): dB rows 0..n-1 = X, dS <- the singular values; returns the rank"""
        r = C.c_int()
        check(lib.qr_gelss_dev(self.h, _dptr(dA), m, n, lda, _dptr(dtau), _dptr(dB), nrhs, ldb, -1.0 if rcond is None else float(rcond),
                               _dptr(dS), C.byref(r)), "qr_gelss_dev")
        return r.value

    def geqp3(self, dA, m, n, lda, djpvt, dtau):
        """column-pivoted QR in place (factors laid out as geqrf's); djpvt: n int32 on the device, 0-based"""
        check(lib.qr_geqp3_dev(self.h, _dptr(dA), m, n, lda, _dptr(djpvt), _dptr(dtau)), "qr_geqp3_dev")

    def rank(self, dA, m, n, lda, rcond=None):
        """numerical rank from geqp3's factors: |R(i,i)| > rcond |R(0,0)| (None: max(m, n) eps); synchronous"""
        r = C.c_int()
        check(lib.qr_rank_dev(self.h, _dptr(dA), m, n, lda, -1.0 if rcond is None else float(rcond), C.byref(r)), "qr_rank_dev")
        return r.value

    def gelsp(self, dA, m, n, lda, djpvt, dtau, dB, nrhs, ldb, rcond=None, dresid=None):
        """rank-deficient least squares on the device (basic solution): dB rows 0..n-1 = X; returns the rank"""
        r = C.c_int()
        check(lib.qr_gelsp_dev(self.h, _dptr(dA), m, n, lda, _dptr(djpvt), _dptr(dtau), _dptr(dB), nrhs, ldb,
                               -1.0 if rcond is None else float(rcond), _dptr(dresid), C.byref(r)), "qr_gelsp_dev")
        return r.value

    def extract_r(self, dA, m, n, lda, dR, rrows, ldr):
        check(lib.qr_extract_r_dev(self.h, _dptr(dA), m, n, lda, _dptr(dR), rrows, ldr), "qr_extract_r_dev")

    def gemm(self, trans, M, N, K, alpha, dA, lda, dB, ldb, beta, dC, ldc):
        check(lib.qr_gemm_dev(self.h, trans.encode(), M, N, K, alpha, _dptr(dA), lda, _dptr(dB), ldb, beta,
                              _dptr(dC), ldc), "qr_gemm_dev")

    def fill_uniform(self, dA, lda, rows, cols, row_off=0, total_rows=None, seed=12):
        check(lib.qr_fill_uniform_dev(self.h, _dptr(dA), lda, rows, cols, row_off,
                                      rows if total_rows is None else total_rows, seed), "qr_fill_uniform_dev")

    def diffnorm(self, dX, ldx, rows, cols, dY=None, ldy=0, row_off=0, total_rows=None, seed=12, mode=0):
        out = (C.c_double * 2)()
        check(lib.qr_diffnorm_dev(self.h, _dptr(dX), ldx, _dptr(dY), ldy, rows, cols, row_off,
                                  rows if total_rows is None else total_rows, seed, mode, out), "qr_diffnorm_dev")
        return out[0], out[1]

    def update_cus(self):
        return lib.qr_plan_update_cus(self.h)

    def set_profile(self, on):
        check(lib.qr_plan_set_profile(self.h, int(on)), "qr_plan_set_profile")

    def pause_profile(self, pause):
        check(lib.qr_plan_pause_profile(self.h, int(bool(pause))), "qr_plan_pause_profile")

    def get_profile_records(self, max_records=65536):
        """[(class, start_ms, end_ms)] of the last profiled run, in issue order (call before get_profile)."""
        cls = (C.c_int * max_records)()
        t0 = (C.c_double * max_records)()
        t1 = (C.c_double * max_records)()
        n = lib.qr_plan_get_profile_records(self.h, max_records, cls, t0, t1)
        if n < 0:
            check(n, "qr_plan_get_profile_records")
        return [(cls[i], t0[i], t1[i]) for i in range(n)]

    def get_profile(self):
        pr = Profile()
        check(lib.qr_plan_get_profile(self.h, C.byref(pr)), "qr_plan_get_profile")
        return {PROF_NAMES[c]: {"ms": pr.ms[c], "flops": pr.flops[c], "bytes": pr.bytes[c],
                                "launches": pr.launches[c]} for c in range(QR_PROF_CLASSES)}


class LsAccumulator:
    """qr_lsacc wrapper: least squares over rows pushed chunk by chunk (R, Q^T b and the residual sums of squares stay on the device).
    The plan must stay open for as long as the accumulator is used."""

    def __init__(self, plan, n, nrhs):
        self.h = None
        h = _vp()
        check(lib.qr_lsacc_create(C.byref(h), plan.h, n, nrhs), "qr_lsacc_create")
        self.h, self.plan, self.n, self.nrhs = h, plan, n, nrhs

    def close(self):
        if self.h and lib is not None and self.plan.h:
            lib.qr_lsacc_destroy(self.h)
        self.h = None

    __del__ = close

    def push(self, dA, p, lda, dB, ldb):
        """fold in p rows [dA | dB]; both buffers are workspace and hold nothing defined afterwards"""
        check(lib.qr_lsacc_push_dev(self.h, _dptr(dA), p, lda, _dptr(dB), ldb), "qr_lsacc_push_dev")

    def pop(self, dA, p, lda, dB, ldb):
        """remove p rows [dA | dB] that were pushed earlier (inputs untouched); QRError with status QR_E_NOTPD leaves the state as it was"""
        check(lib.qr_lsacc_pop_dev(self.h, _dptr(dA), p, lda, _dptr(dB), ldb), "qr_lsacc_pop_dev")

    def slide(self, dAnew, pnew, ldan, dBnew, ldbn, dAold, pold, ldao, dBold, ldbo):
        """add pnew rows and remove pold rows in one pass (inputs untouched); all-or-nothing as pop"""
        check(lib.qr_lsacc_slide_dev(self.h, _dptr(dAnew), pnew, ldan, _dptr(dBnew), ldbn, _dptr(dAold), pold, ldao, _dptr(dBold), ldbo),
              "qr_lsacc_slide_dev")

    def rows(self):
        r = C.c_longlong()
        check(lib.qr_lsacc_rows(self.h, C.byref(r)), "qr_lsacc_rows")
        return r.value

    def factor(self):
        """(dR, ldr, dZ, ldz): device addresses (ints) of the n x n R and the n x nrhs Z = (Q^T b)(0:n)"""
        r, z, ldr, ldz = _vp(), _vp(), C.c_int(), C.c_int()
        check(lib.qr_lsacc_factor_dev(self.h, C.byref(r), C.byref(ldr), C.byref(z), C.byref(ldz)), "qr_lsacc_factor_dev")
        return r.value, ldr.value, z.value, ldz.value

    def factor_host(self):
        """numpy copies (R n x n, Z n x nrhs) of the current state; synchronises the plan"""
        r, ldr, z, ldz = self.factor()
        self.plan.sync()
        R = np.empty((self.n, ldr), order="C")          # the column-major image: row c = column c
        Z = np.empty((self.nrhs, ldz), order="C")
        check(lib.qr_copy_to_host(R.ctypes.data, r, R.nbytes), "qr_copy_to_host")
        check(lib.qr_copy_to_host(Z.ctypes.data, z, Z.nbytes), "qr_copy_to_host")
        return np.asfortranarray(R[:, :self.n].T), np.asfortranarray(Z[:, :self.n].T)

    def solve(self, dX, ldx, dresid=None):
        """dX (n x nrhs) <- the least-squares solution of everything pushed so far; dresid (nrhs) <- the residual norms"""
        check(lib.qr_lsacc_solve_dev(self.h, _dptr(dX), ldx, _dptr(dresid)), "qr_lsacc_solve_dev")

    def reset(self):
        check(lib.qr_lsacc_reset(self.h), "qr_lsacc_reset")


class LsAccumulatorBatched:
    """qr_lsacc_batched wrapper: one least-squares accumulator per member of a batch (R, Q^T b, the residual sums of squares and the row
    counts stay on the device); push, pop and slide are one launch for the whole batch.  The plan must stay open for as long as the
    accumulator is used."""

    def __init__(self, plan, n, nrhs, batch):
        self.h = None
        h = _vp()
        check(lib.qr_lsacc_batched_create(C.byref(h), plan.h, n, nrhs, batch), "qr_lsacc_batched_create")
        self.h, self.plan, self.n, self.nrhs, self.batch = h, plan, n, nrhs, batch

    def close(self):
        if self.h and lib is not None and self.plan.h:
            lib.qr_lsacc_batched_destroy(self.h)
        self.h = None

    __del__ = close

    def push(self, dA, p, lda, strideA, dB, ldb, strideB):
        """fold p rows [dA_q | dB_q] into every member (inputs untouched)"""
        check(lib.qr_lsacc_batched_push_dev(self.h, _dptr(dA), p, lda, strideA, _dptr(dB), ldb, strideB), "qr_lsacc_batched_push_dev")

    def pop(self, dA, p, lda, strideA, dB, ldb, strideB, dinfo):
        """remove p rows that were pushed earlier; dinfo (batch device ints): 0, the failing column + 1, or -1 (fewer than n rows left);
        a member with a non-zero word keeps its state"""
        check(lib.qr_lsacc_batched_pop_dev(self.h, _dptr(dA), p, lda, strideA, _dptr(dB), ldb, strideB, _dptr(dinfo)),
              "qr_lsacc_batched_pop_dev")

    def slide(self, dAnew, pnew, ldan, strideAn, dBnew, ldbn, strideBn, dAold, pold, ldao, strideAo, dBold, ldbo, strideBo, dinfo):
        """add pnew rows and remove pold rows in one launch; dinfo as pop"""
        check(lib.qr_lsacc_batched_slide_dev(self.h, _dptr(dAnew), pnew, ldan, strideAn, _dptr(dBnew), ldbn, strideBn, _dptr(dAold), pold, ldao,
                                             strideAo, _dptr(dBold), ldbo, strideBo, _dptr(dinfo)), "qr_lsacc_batched_slide_dev")

    def factor(self):
        """(dR, ldr, strideR, dZ, ldz, strideZ, drss, drows): device addresses (ints), leading dimensions and strides of the state"""
        r, z, s, w = _vp(), _vp(), _vp(), _vp()
        ldr, ldz, sr, sz = C.c_int(), C.c_int(), _ll(), _ll()
        check(lib.qr_lsacc_batched_factor_dev(self.h, C.byref(r), C.byref(ldr), C.byref(sr), C.byref(z), C.byref(ldz), C.byref(sz), C.byref(s),
                                              C.byref(w)), "qr_lsacc_batched_factor_dev")
        return r.value, ldr.value, sr.value, z.value, ldz.value, sz.value, s.value, w.value

    def factor_host(self):
        """numpy copies (R (batch, n, n), Z (batch, n, nrhs), rss (batch, nrhs), rows (batch,)) of the state; synchronises the plan"""
        r, _, _, z, _, _, s, w = self.factor()
        self.plan.sync()
        R = np.empty((self.batch, self.n, self.n))
        Z = np.empty((self.batch, self.nrhs, self.n))
        rss = np.empty((self.batch, self.nrhs))
        rows = np.zeros(self.batch, dtype=np.intc)
        if self.batch:
            for host, dev in ((R, r), (Z, z), (rss, s), (rows, w)):
                check(lib.qr_copy_to_host(host.ctypes.data, dev, host.nbytes), "qr_copy_to_host")
        return R.transpose(0, 2, 1), Z.transpose(0, 2, 1), rss, rows.astype(np.int64)

    def solve(self, dX, ldx, strideX, dinfo, dresid=None, strideresid=0):
        """dX_q (n x nrhs) <- the least-squares solution of the rows member q holds; dresid (nrhs per member) <- the residual norms;
        dinfo: 0 or the first zero pivot + 1"""
        check(lib.qr_lsacc_batched_solve_dev(self.h, _dptr(dX), ldx, strideX, _dptr(dresid), strideresid, _dptr(dinfo)),
              "qr_lsacc_batched_solve_dev")

    def solve_damped(self, dlam, nlam, stridelam, dX, ldx, strideX, dinfo, dD=None, strideD=0, dxnorm=None, dresid=None):
        """the damped solves of every member from the state, which stays untouched: dX n x (nlam * nrhs) per member, dinfo nlam ints"""
        check(lib.qr_lsacc_batched_solve_damped_dev(self.h, _dptr(dD), strideD, _dptr(dlam), nlam, stridelam, _dptr(dX), ldx, strideX,
                                                    _dptr(dxnorm), _dptr(dresid), _dptr(dinfo)), "qr_lsacc_batched_solve_damped_dev")

    def solve_trust(self, ddelta, stridedelta, dX, ldx, strideX, dlam, dinfo, dD=None, strideD=0, dlam0=None, stridelam0=0, rtol=0.1, maxit=10,
                    dxnorm=None, dresid=None, diter=None, dstatus=None):
        """the trust-region step of every member from the state (nrhs == 1), which stays untouched"""
        check(lib.qr_lsacc_batched_solve_trust_dev(self.h, _dptr(dD), strideD, _dptr(ddelta), stridedelta, _dptr(dlam0), stridelam0, float(rtol),
                                                   int(maxit), _dptr(dX), ldx, strideX, _dptr(dlam), _dptr(dxnorm), _dptr(dresid), _dptr(diter),
                                                   _dptr(dstatus), _dptr(dinfo)), "qr_lsacc_batched_solve_trust_dev")

    def covar(self, dinfo, scaled=QR_COV_SCALED, rhs=0, dC=None, ldc=0, strideC=0, dse=None, stridese=0, dsigma2=None):
        """the covariance (dC, n x n per member) and standard errors (dse) of every member from the state, which stays untouched:
        (R^T R)^-1, times sigma2 = rss[rhs] / (rows - n) where scaled; sigma2 to dsigma2; dinfo: 0, i + 1 for a member that holds fewer
        than n rows, -3 for scaled with rows == n"""
        check(lib.qr_lsacc_batched_covar_dev(self.h, int(scaled), int(rhs), _dptr(dC), ldc, strideC, _dptr(dse), stridese, _dptr(dsigma2),
                                             _dptr(dinfo)), "qr_lsacc_batched_covar_dev")

    def reset(self):
        check(lib.qr_lsacc_batched_reset(self.h), "qr_lsacc_batched_reset")


class _RawDeviceArray:
    """zero-copy torch view of device memory the library owns, through __cuda_array_interface__"""

    def __init__(self, ptr, shape, typestr):
        self.__cuda_array_interface__ = {"shape": tuple(shape), "typestr": typestr, "data": (int(ptr), False), "version": 2}


class LmBatched:
    """qr_lm_batched wrapper: MINPACK lmder's outer loop for every member of a batch, by reverse communication (mi355x_qr.h section 8m).
    start(dX0); then per round: fill J and f at state()["x"], step(dJ, dF); fill f at state()["xtrial"], update(dFtrial); running()
    is the one call that waits on the host.  The calls run on the plan's stream: model code in torch runs there too inside
    `with torch.cuda.stream(torch.cuda.ExternalStream(plan.stream))`.  The plan must stay open for as long as the solver is used."""
    _state = LmState
    _prefix = "qr_lm_batched"          # the C calls are _prefix + "_create", "_start_dev", ..: a subclass names another family

    def _call(self, suffix, *args):
        name = self._prefix + suffix
        check(getattr(lib, name)(self.h, *args), name)

    def __init__(self, plan, m, n, batch, **options):
        self.h = None
        self.options = lm_options(**options)
        h = _vp()
        name = self._prefix + "_create"
        check(getattr(lib, name)(C.byref(h), plan.h, m, n, batch, C.byref(self.options)), name)
        self.h, self.plan, self.m, self.n, self.batch = h, plan, m, n, batch
        self._views = None

    def close(self):
        if self.h and lib is not None and self.plan.h:
            getattr(lib, self._prefix + "_destroy")(self.h)
        self.h = None

    __del__ = close

    def start(self, dX0, ldx=None, strideX=None, dD0=None, strideD=None):
        """x <- dX0 (n per member, packed unless ldx / strideX say otherwise); dD0: the scaling of mode 2 (strideD 0: shared)"""
        ldx = self.n if ldx is None else ldx
        self._call("_start_dev", _dptr(dX0), ldx, ldx if strideX is None else strideX, _dptr(dD0), self.n if strideD is None else strideD)

    def step(self, dJ, dF, ldj=None, strideJ=None, ldf=None, strideF=None):
        """dJ (m x n per member, column-major) <- its pivoted factors, dF (m per member) <- Q^T f, then the step of every running member
        (LmBoundedBatched: the peg on dJ and dF in front, and the step cut to the box)"""
        ldj = self.m if ldj is None else ldj
        ldf = self.m if ldf is None else ldf
        self._call("_step_dev", _dptr(dJ), ldj, ldj * self.n if strideJ is None else strideJ, _dptr(dF), ldf, ldf if strideF is None else strideF)

    def update(self, dFtrial, ldf=None, strideF=None):
        """dFtrial (m per member): f at the trial points"""
        ldf = self.m if ldf is None else ldf
        self._call("_update_dev", _dptr(dFtrial), ldf, ldf if strideF is None else strideF)

    def view(self):
        """the device addresses of the state: a dict of ints"""
        v = self._state()
        self._call("_view", C.byref(v))
        return {k: getattr(v, k) for k, _ in self._state._fields_}

    def state(self, device=None):
        """the state as zero-copy torch views: x, xtrial, D (batch, n) float64; delta, par, fnorm, xnorm, pnorm, gnorm, prered, dirder
        (batch,) float64; iter, nfev, njev, accepted, status, info, par_status (batch,) int32.  Read-only for the caller; reading them on
        the host needs the plan's stream synchronised (running() does)."""
        import torch
        if self._views is None:
            dev = torch.device("cuda", torch.cuda.current_device()) if device is None else device
            ptr = self.view()
            out = {}
            S = self._state
            for k in S._doubles + S._ints:
                shape = (self.batch, self.n) if k in ("x", "xtrial", "D", "lo", "hi", "peg") else (self.batch,)
                if self.batch == 0:
                    out[k] = torch.empty(shape, dtype=torch.float64 if k in S._doubles else torch.int32, device=dev)
                else:
                    out[k] = torch.as_tensor(_RawDeviceArray(ptr[k], shape, "<f8" if k in S._doubles else "<i4"), device=dev)
            self._views = out
        return self._views

    def running(self):
        """the number of members with status == 0 and info == 0; waits for the plan's stream"""
        c = C.c_int()
        self._call("_running", C.byref(c))
        return c.value


class LmBoundedBatched(LmBatched):
    """qr_lmb_batched wrapper: LmBatched's loop with box bounds lo <= x <= hi (mi355x_qr.h section 8n).  The protocol is LmBatched's;
    start takes the bounds, and state() has lo, hi (batch, n) float64, peg (batch, n) int32, alpha (batch,) float64 and clipped (batch,)
    int32 as well."""
    _state = LmBoundedState
    _prefix = "qr_lmb_batched"

    def start(self, dX0, ldx=None, strideX=None, dD0=None, strideD=None, dLo=None, strideLo=None, dHi=None, strideHi=None):
        """x <- dX0, the scaling of mode 2 as in LmBatched.start; dLo, dHi: the bounds, n per member (stride 0: one vector shared by all
        members; None: that side is unbounded)"""
        ldx = self.n if ldx is None else ldx
        self._call("_start_dev", _dptr(dX0), ldx, ldx if strideX is None else strideX, _dptr(dD0), self.n if strideD is None else strideD,
                   _dptr(dLo), self.n if strideLo is None else strideLo, _dptr(dHi), self.n if strideHi is None else strideHi)


def _lm_bounds_dev(bounds, batch, n, device):
    """bounds = (lo, hi) -> two packed (batch, n) device tensors or None"""
    import torch
    try:
        lo, hi = bounds
    except (TypeError, ValueError):
        raise QRError("lm_batched: bounds must be a pair (lo, hi)", QR_E_ARG)
    out = []
    for v in (lo, hi):
        if v is None:
            out.append(None)
            continue
        v = torch.as_tensor(v, dtype=torch.float64, device=device)
        if v.dim() > 2 or (v.dim() == 2 and tuple(v.shape) != (batch, n)) or (v.dim() == 1 and tuple(v.shape) != (n,)):
            raise QRError(f"lm_batched: a bound must be a scalar, ({n},) or ({batch}, {n}), got {tuple(v.shape)}", QR_E_ARG)
        out.append(v.expand(batch, n).contiguous())
    return out


def lm_batched(fun, jac, x0, *, D=None, check_every=1, plan=None, bounds=None, **options):
    """min ||f_q(x)|| for every member by Levenberg-Marquardt with the model in torch: fun maps x (batch, n) to f (batch, m) and jac to
    J (batch, m, n), both on device tensors; x0: (batch, n) on the device; D: the scaling of mode 2, (n,) or (batch, n).  The model runs
    on the plan's stream between the two device calls of a round, the wrapper does the layout copy of J, and running() -- the only host
    wait -- is polled every `check_every` rounds.  options: the fields of qr_lm_options.  bounds: None, or (lo, hi) for lo <= x <= hi
    through LmBoundedBatched (each of lo, hi: None, a scalar, (n,) or (batch, n); entries may be infinite).  Returns a dict of torch
    tensors: the state of LmBatched.state() (copies; LmBoundedBatched.state() with bounds), x first."""
    import torch
    if x0.dim() != 2:
        raise QRError(f"lm_batched: x0 must be (batch, n), got {tuple(x0.shape)}", QR_E_ARG)
    batch, n = x0.shape
    if D is not None:
        options.setdefault("mode", 2)
        D = torch.as_tensor(D, dtype=torch.float64, device=x0.device)
        if D.dim() == 1:
            D = D.expand(batch, n)
        if tuple(D.shape) != (batch, n):
            raise QRError(f"lm_batched: D must be ({n},) or ({batch}, {n}), got {tuple(D.shape)}", QR_E_ARG)
        D = D.contiguous()
    if bounds is not None:
        bounds = _lm_bounds_dev(bounds, batch, n, x0.device)
    torch.cuda.synchronize()                  # x0 and D were made on torch's streams; from here on everything runs on the plan's
    x0 = x0.to(torch.float64).contiguous()
    m = int(fun(x0).shape[1])
    torch.cuda.synchronize()
    own = plan is None
    if own:
        plan = Plan(max(m, 1), n)
    try:
        return _lm_batched_run(plan, fun, jac, x0, D, m, max(int(check_every), 1), options, bounds)
    finally:                                  # (whatever was allocated under the plan's stream is gone before the stream is)
        torch.cuda.synchronize()
        if own:
            plan.close()


def _lm_batched_run(plan, fun, jac, x0, D, m, every, options, bounds=None):
    import torch
    batch, n = x0.shape
    lm = LmBatched(plan, m, n, batch, **options) if bounds is None else LmBoundedBatched(plan, m, n, batch, **options)
    try:
        J = torch.empty((batch, n, m), dtype=torch.float64, device=x0.device)           # member q: J_q column-major
        F = torch.empty((batch, m), dtype=torch.float64, device=x0.device)
        torch.cuda.synchronize()
        with torch.cuda.stream(torch.cuda.ExternalStream(plan.stream)):
            if bounds is None:
                lm.start(x0, dD0=D)
            else:
                lm.start(x0, dD0=D, dLo=bounds[0], dHi=bounds[1])
            st = lm.state(x0.device)
            limit = lm.options.maxfev if lm.options.maxfev > 0 else 100 * (n + 1)     # every round adds 1 to nfev of every running member
            for rounds in range(1, limit + 1 if batch else 1):
                J.copy_(jac(st["x"]).transpose(1, 2))
                F.copy_(fun(st["x"]))
                lm.step(J, F)
                F.copy_(fun(st["xtrial"]))
                lm.update(F)
                if rounds % every == 0 and lm.running() == 0:
                    break
            plan.sync()
        torch.cuda.synchronize()
        return {k: v.clone() for k, v in st.items()}          # copies on the caller's stream: they outlive the solver and the plan
    finally:
        torch.cuda.synchronize()
        lm.close()


class TsqrPlan:
    """qr_tsqr_plan wrapper: the device-resident TSQR step of one rank (include/mi355x_qr.h).  `unique_id`: the 128 bytes
    rank 0 got from tsqr_unique_id(), carried to every rank by the caller; None with nranks = 1; comm="external" builds a
    plan without a communicator (the caller exchanges the R factors itself: local / exchange_buffers / stacked)."""

    def __init__(self, m_local, n, nranks=1, rank=0, nb=0, unique_id=None, comm=None):
        self.h = None
        h = _vp()
        if comm == "external":
            check(lib.qr_tsqr_plan_create_comm(C.byref(h), None, nranks, rank, m_local, n, nb), "qr_tsqr_plan_create_comm")
        else:
            buf = None
            if nranks > 1:
                assert unique_id is not None and len(unique_id) == 128
                buf = C.create_string_buffer(bytes(unique_id), 128)
            check(lib.qr_tsqr_plan_create(C.byref(h), buf, nranks, rank, m_local, n, nb), "qr_tsqr_plan_create")
        self.h, self.m, self.n, self.nranks, self.rank = h, m_local, n, nranks, rank
        self.local = Plan(m_local, n, borrowed=lib.qr_tsqr_local_plan(h))
        sp = lib.qr_tsqr_stacked_plan(h)
        self.stacked = Plan(nranks * n, n, borrowed=sp) if sp else None

    def close(self):
        if self.h and lib is not None:      # (at interpreter shutdown the module's globals may already be gone)
            lib.qr_tsqr_plan_destroy(self.h)
            self.h = None

    __del__ = close

    def factor(self, dA, lda, dR):
        check(lib.qr_tsqr_factor_dev(self.h, _dptr(dA), lda, _dptr(dR)), "qr_tsqr_factor_dev")

    def formq(self, dA, lda, dQ, ldq):
        check(lib.qr_tsqr_formq_dev(self.h, _dptr(dA), lda, _dptr(dQ), ldq), "qr_tsqr_formq_dev")

    def factor_selfgather(self, dA, lda, dR):
        check(lib.qr_tsqr_factor_selfgather_dev(self.h, _dptr(dA), lda, _dptr(dR)), "qr_tsqr_factor_selfgather_dev")

    def set_schedule(self, mode):
        """0 = one collective, 1 = panel-pipelined, 2 = the library's rule; every rank must make the same call"""
        check(lib.qr_tsqr_set_schedule(self.h, int(mode)), "qr_tsqr_set_schedule")

    def is_pipelined(self):
        return bool(lib.qr_tsqr_is_pipelined(self.h))

    def gather_stats(self):
        """the exchange of the last pipelined factor(): per-gather intervals from the stacked stream's events (include/mi355x_qr.h)"""
        out = (C.c_double * 5)()
        check(lib.qr_tsqr_gather_stats(self.h, out), "qr_tsqr_gather_stats")
        return {"gather_ms": out[0], "gather_max_ms": out[1], "call_ms": out[2], "pipelined": bool(out[3]), "fell_back": bool(out[4])}

    def local_factor(self, dA, lda):
        check(lib.qr_tsqr_local_dev(self.h, _dptr(dA), lda), "qr_tsqr_local_dev")

    def exchange_buffers(self):
        s, r = _vp(), _vp()
        check(lib.qr_tsqr_exchange_buffers(self.h, C.byref(s), C.byref(r)), "qr_tsqr_exchange_buffers")
        return s.value, r.value

    def stacked_factor(self, dR):
        check(lib.qr_tsqr_stacked_dev(self.h, _dptr(dR)), "qr_tsqr_stacked_dev")

    def sync(self):
        check(lib.qr_tsqr_sync(self.h), "qr_tsqr_sync")

    def comm_ranks(self):
        n = C.c_int()
        check(lib.qr_tsqr_comm_ranks(self.h, C.byref(n)), "qr_tsqr_comm_ranks")
        return n.value


def tsqr_factor_virtual(plans, shards, lda, Rs):
    """qr_tsqr_factor_virtual_dev: the panel-pipelined schedule over P TsqrPlans of one device (virtual ranks)."""
    P = len(plans)
    hs = (_vp * P)(*[p.h for p in plans])
    As = (_vp * P)(*[_dptr(a) for a in shards])
    Rp = (_vp * P)(*[_dptr(r) for r in Rs])
    check(lib.qr_tsqr_factor_virtual_dev(hs, P, As, lda, Rp), "qr_tsqr_factor_virtual_dev")


def tsqr_unique_id():
    buf = C.create_string_buffer(128)
    check(lib.qr_tsqr_unique_id(buf), "qr_tsqr_unique_id")
    return bytes(buf.raw)


def uniform_at(seed, idx):
    return lib.qr_uniform_at(seed, idx)


def uniform_matrix_host(rows, cols, row_off=0, total_rows=None, seed=12):
    """Host evaluation of the device generator (same hash): numpy (rows x cols)."""
    total = rows if total_rows is None else total_rows
    c = np.arange(cols, dtype=np.uint64)[None, :]
    i = (np.arange(rows, dtype=np.uint64) + np.uint64(row_off))[:, None]
    idx = c * np.uint64(total) + i
    with np.errstate(over="ignore"):
        z = np.uint64(seed) * np.uint64(0x9E3779B97F4A7C15) + (idx + np.uint64(1)) * np.uint64(0xD1B54A32D192ED03)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    return (z >> np.uint64(11)).astype(np.float64) * (1.0 / 9007199254740992.0)


def flops(m, n):
    """Householder QR factorisation flops, 2mn^2 - 2n^3/3."""
    return 2.0 * m * n * n - 2.0 * n ** 3 / 3.0
