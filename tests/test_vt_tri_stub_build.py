"""No GPU: the host layer calls qrd_gemm_nn_tri for V*T, which the stub device layer (tests/c/qrd_stub.c) does not have -- the sanitizer build
must still link and run, through the host layer's weak fallback onto qrd_gemm_nn."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QRDIR = os.path.join(ROOT, "cuda-qr_amd")


def _symbol_kinds(path, *flags):
    nm = subprocess.run(["nm", *flags, path], capture_output=True, text=True, check=True).stdout
    return {ln.split()[-1]: ln.split()[-2] for ln in nm.splitlines() if len(ln.split()) >= 2}


def test_libraries_resolve_to_the_device_layers_definition():
    for lib in ("libmi355xqr.so", "libmi355xqr_lab.so"):
        assert _symbol_kinds(os.path.join(QRDIR, lib), "-D").get("qrd_gemm_nn_tri") == "T", lib


def test_stub_build_factors_through_the_weak_fallback():
    host = open(os.path.join(QRDIR, "csrc", "qr_host.c")).read()
    stub = open(os.path.join(ROOT, "tests", "c", "qrd_stub.c")).read()
    assert "qrd_gemm_nn_tri(stream, mk, wout, wout" in host and "qrd_gemm_nn_tri" not in stub
    env = {k: v for k, v in os.environ.items() if not k.startswith("MI355XQR_")}
    out = subprocess.run(["make", "-C", QRDIR, "asan"], capture_output=True, text=True, env=env, timeout=600)
    assert out.returncode == 0, (out.stdout[-1500:] + out.stderr[-3000:])
    assert "host layer sanitize run ok" in out.stdout
    kinds = _symbol_kinds(os.path.join(QRDIR, "build", "host_asan"))
    assert kinds.get("qrd_gemm_nn_tri") == "W"          # the fallback, and nothing stronger, in the stub build
    assert kinds.get("qrd_gemm_nn") == "T"
