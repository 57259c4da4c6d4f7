"""The seventeen per-interface host units (qr_solve.c ... qr_batched_lm.c, the last one both Levenberg-Marquardt sections, 8m and 8n) over
the stub device layer, checked without a GPU.

The stub (tests/c/qrd_stub.c, tests/c/qrd_stub_units.c) has an entry for every launch these units make: it refuses the shapes the real
launcher refuses, bounds-checks every operand block at the extent qr_device.h documents and stamps it for the stream-order model.  The
driver tests/c/host_units.c reaches every public entry point of every unit, one named configuration per process, with caller-side device
buffers of exactly the documented minimum size (DESIGN "Host units over the stub").  `make -C cuda-qr_amd units_asan units_tsan units_order`
builds and runs them.  Checked here:
  every configuration is silent under AddressSanitizer / UBSan with leak detection, the four-thread run under ThreadSanitizer, 0 order reports;
  malloc failure: each device allocation the library makes fails in turn (QRD_STUB_FAIL_MALLOC=k); the call returns QR_E_ALLOC, nothing
    leaks, and the same call on the same plan then completes;
  shrink sweep: each of those allocations 8 bytes short (QRD_STUB_SHRINK_MALLOC=k) is reported as an out-of-bounds block, except the sites
    listed, each with the reason it has slack, in units_slack_allocations.json;
  coverage gate: gcov over all configurations shows every line of the units that calls a qrd_* launch or copy executed, except the lines
    listed, each with its reason, in units_unreached.json;
  the sizing and route functions the stub restates equal the product's over their whole argument grid.
"""
import ctypes
import json
import os
import re
import subprocess
from concurrent.futures import ThreadPoolExecutor

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QR = os.path.join(ROOT, "cuda-qr_amd")
HERE = os.path.dirname(os.path.abspath(__file__))
UNITS = ["qr_solve", "qr_pivot", "qr_minnorm", "qr_update", "qr_downdate", "qr_svd", "qr_batched", "qr_batched_update", "qr_batched_minnorm",
         "qr_batched_damped", "qr_batched_trust", "qr_batched_lse", "qr_batched_bvls", "qr_batched_irls", "qr_batched_stats",
         "qr_batched_lsei", "qr_batched_lm"]
# the qrd_* functions that launch or copy nothing: sizes, routes, the binding of a workspace
PURE = {"qrd_b_max_rows", "qrd_b_fits", "qrd_b_wave_route", "qrd_bu_max_rows", "qrd_bu_wave_route", "qrd_bd_wave_route", "qrd_bl_max_rows",
        "qrd_bl_wave_route", "qrd_bv_max_rows", "qrd_bv_wave_route", "qrd_ir_max_rows", "qrd_ir_wave_route", "qrd_le_max_rows",
        "qrd_le_wave_route", "qrd_bs_max_rows", "qrd_bs_cov_wave_route", "qrd_bs_fit_wave_route", "qrd_bs_lev_chunks", "qrd_ormqr_skinny_ws",
        "qrd_ormqr_skinny_blocks", "qrd_pivot_ws_doubles", "qrd_pivot_ws_ints", "qrd_pivot_ws_bind", "qrd_gemm_nt_ok", "qrd_gemm_nt4_ok",
        "qrd_malloc", "qrd_free", "qrd_stream_sync"}
# an allocation whose failure the library absorbs: the call completes without it
FAILURE_ABSORBED = {"qr_geqrf_dev:(void**) &p->padA": "the padded copy of an odd-height matrix is optional: qr_geqrf_dev notes the failure and factors in place"}


def _env(**extra):
    env = {k: v for k, v in os.environ.items() if not k.startswith(("MI355XQR_", "QRD_STUB_"))}
    env.update(extra)
    return env


def _make(target, timeout=900):
    out = subprocess.run(["make", "-C", QR, target], capture_output=True, text=True, env=_env(), timeout=timeout)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    return out


@pytest.fixture(scope="module")
def units_build():
    _make("units_order")
    exe = os.path.join(QR, "build", "units", "host_units")
    names = subprocess.run([exe, "list"], capture_output=True, text=True, check=True).stdout.split()
    assert len(names) >= 50
    return {"exe": exe, "cov": os.path.join(QR, "build", "units", "cov", "host_units"), "configs": names,
            "stub": os.path.join(QR, "build", "units", "libqrd_stub.so")}


def _run(exe, config, **extra):
    return subprocess.run([exe, config], capture_output=True, text=True, env=_env(**extra), timeout=120)


@pytest.fixture(scope="module")
def baseline(units_build):
    """every configuration once: {config: [(k, bytes, site), ...]}, the library's allocations in call order"""
    with ThreadPoolExecutor(8) as ex:
        res = list(ex.map(lambda c: _run(units_build["exe"], c), units_build["configs"]))
    allocs = {}
    for c, r in zip(units_build["configs"], res):
        assert r.returncode == 0 and r.stderr == "", (c, r.returncode, r.stderr[-1500:])
        lines = r.stdout.splitlines()
        assert lines[0] == "ORDER 0" and lines[2] == "FAILHITS 0", (c, lines[:3])
        assert int(lines[1].split()[1]) > 50, (c, lines[1])          # the configuration does launch
        allocs[c] = [(int(k), int(b), site) for _, k, b, site in (ln.split(" ", 3) for ln in lines if ln.startswith("ALLOC "))]
    return allocs


def _once_per_site(allocs):
    """the allocations of one configuration, each (site, size) once: a pair already tried is not tried again"""
    seen, todo = set(), []
    for k, b, site in allocs:
        if (site, b) not in seen:
            seen.add((site, b))
            todo.append((k, b, site))
    return todo


def test_every_configuration_is_silent(baseline):
    assert sum(len(a) for a in baseline.values()) > 500          # the configurations do allocate: plans, workspaces, slots, stage blocks


def test_sanitizer_builds_run_clean():
    """`make units_asan` runs every configuration under ASan / UBSan with leak detection, `make units_tsan` the four-thread run"""
    _make("units_asan")
    _make("units_tsan")


def test_malloc_failure_sweep(units_build, baseline):
    """Under the AddressSanitizer build, so that host memory lost on a QR_E_ALLOC path is reported as well (the driver itself ends with
    exit code 6 when a device allocation is still live)."""
    _make("build/units/asan/host_units")
    exe = os.path.join(QR, "build", "units", "asan", "host_units")
    bad = []
    for config in units_build["configs"]:
        todo = _once_per_site(baseline[config])
        with ThreadPoolExecutor(8) as ex:
            res = list(ex.map(lambda t: _run(exe, config, QRD_STUB_FAIL_MALLOC=str(t[0]), ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1"), todo))
        for (k, b, site), r in zip(todo, res):
            hits = "FAILHITS 0" if site in FAILURE_ABSORBED else "FAILHITS 1"          # QR_E_ALLOC came back once and the repeated call completed
            if r.returncode != 0 or r.stderr != "" or hits not in r.stdout or "ORDER 0" not in r.stdout:
                bad.append((config, k, site, r.returncode, r.stdout[:60], r.stderr[-300:]))
    assert not bad, bad[:10]


def test_shrink_sweep(units_build, baseline):
    """Each allocation of the library 8 bytes short in turn: the sites whose shrinking no configuration reports are exactly the committed
    list of allocations with slack."""
    listed = json.load(open(os.path.join(HERE, "units_slack_allocations.json")))
    assert all(isinstance(v, str) and len(v) > 20 for v in listed.values())
    reached, detected = set(), {}
    for config in units_build["configs"]:
        todo = _once_per_site(baseline[config])
        reached |= {site for _, _, site in todo}
        with ThreadPoolExecutor(8) as ex:
            res = list(ex.map(lambda t: _run(units_build["exe"], config, QRD_STUB_SHRINK_MALLOC=str(t[0])), todo))
        for (k, b, site), r in zip(todo, res):
            if r.returncode != 0 and "is not inside a live device allocation" in r.stderr:
                detected.setdefault(site, f"{config} allocation {k} ({b} bytes)")
            else:
                assert r.returncode == 0, (config, k, site, r.stderr[-500:])          # nothing else may go wrong
    undetected = reached - set(detected)
    print("detected:", json.dumps(detected, indent=1))
    assert len(detected) >= 30
    assert undetected == set(listed), {"not listed": sorted(undetected - set(listed)), "listed but detected or never reached": sorted(set(listed) - undetected)}


def _strip_comments(text):
    return re.sub(r"/\*.*?\*/", lambda m: re.sub(r"[^\n]", " ", m.group(0)), text, flags=re.S)


def launch_lines(unit):
    """{line: [names]} of the qrd_* launches and copies unit.c calls (the line the call starts on)"""
    text = _strip_comments(open(os.path.join(QR, "csrc", unit + ".c")).read())
    out = {}
    for m in re.finditer(r"\b(qrd_\w+)\(", text):
        if m.group(1) not in PURE:
            out.setdefault(text.count("\n", 0, m.start()) + 1, []).append(m.group(1))
    return out


def test_every_launch_line_is_reached(units_build):
    listed = json.load(open(os.path.join(HERE, "units_unreached.json")))
    assert all(isinstance(v, str) and len(v) > 20 for v in listed.values())
    cov_dir = os.path.dirname(units_build["cov"])
    for f in os.listdir(cov_dir):
        if f.endswith(".gcda"):
            os.remove(os.path.join(cov_dir, f))
    out = subprocess.run([units_build["cov"], "all"], capture_output=True, text=True, env=_env(), timeout=600)
    assert out.returncode == 0 and out.stdout.startswith("ORDER 0\n"), (out.stdout[:200], out.stderr[-1500:])
    unreached, total = set(), 0
    for unit in UNITS:
        g = subprocess.run(["gcov", "-t", "-o", cov_dir, os.path.join(cov_dir, unit + ".o")], capture_output=True, text=True, cwd=QR, timeout=120)
        assert g.returncode == 0, g.stderr[-2000:]
        counts, in_file = {}, False
        for ln in g.stdout.splitlines():
            m = re.match(r"\s*(\S+):\s*(\d+):(.*)", ln)
            if not m:
                continue
            if m.group(2) == "0":
                if "Source:" in ln:
                    in_file = ln.rstrip().endswith(f"Source:csrc/{unit}.c")
                continue
            if in_file:
                counts[int(m.group(2))] = m.group(1)
        text = open(os.path.join(QR, "csrc", unit + ".c")).read().splitlines()
        for line, names in sorted(launch_lines(unit).items()):
            total += 1
            at = line
            while counts.get(at, "-") == "-" and at > line - 4:          # a call that starts on a continuation line: the statement's first line
                at -= 1
            c = counts.get(at, "-")
            assert c != "-", f"gcov has no count for {unit}.c:{line}"
            if c.startswith("#") or c.startswith("="):
                unreached.add(f"{unit}.c:{'+'.join(names)}:{text[line - 1].strip()[:70]}")
    assert total > 150
    assert unreached == set(listed), {"not listed": sorted(unreached - set(listed)), "listed but reached": sorted(set(listed) - unreached)}


# ---- the sizing and route functions: the stub's restatement against the product, exact equality over the whole grid ----
class _PivotWs(ctypes.Structure):
    _fields_ = [(n, ctypes.c_void_p) for n in ("F", "FT", "P", "vn1", "vn2", "npart", "alpha", "cval", "flag", "cidx", "pend")] + [("ldf", ctypes.c_int)]


def _sig(lib, name, res, nargs):
    f = getattr(lib, name)
    f.restype = res
    f.argtypes = [ctypes.c_int] * nargs
    return f


def test_sizing_functions_equal_the_products(units_build):
    prod_path = os.path.join(QR, "libmi355xqr.so")
    assert os.path.exists(prod_path), "libmi355xqr.so is not built"
    prod = ctypes.CDLL(prod_path, mode=ctypes.RTLD_LOCAL)
    stub = ctypes.CDLL(units_build["stub"], mode=ctypes.RTLD_LOCAL)
    N, R = 66, 514          # one past QRD_B_MAX_N + 1 and QRD_B_MAX_ROWS + 1, from 0 (and -1 where a lower limit is tested)
    grids = {
        "qrd_b_max_rows": (ctypes.c_int, [range(-1, N)]),
        "qrd_b_fits": (ctypes.c_int, [range(-1, R + 1), range(-1, N)]),
        "qrd_b_wave_route": (ctypes.c_int, [range(0, R), range(0, N)]),
        "qrd_bu_max_rows": (ctypes.c_int, [range(-1, N)]),
        "qrd_bu_wave_route": (ctypes.c_int, [range(0, N), range(0, 258)]),
        "qrd_bd_wave_route": (ctypes.c_int, [range(-1, N)]),
        "qrd_bl_wave_route": (ctypes.c_int, [range(0, 67), range(0, N), range(0, N)]),
        "qrd_bl_max_rows": (ctypes.c_int, [range(0, N), range(0, N), range(0, N)]),
        "qrd_bv_wave_route": (ctypes.c_int, [range(0, R), range(0, N)]),
        "qrd_bv_max_rows": (ctypes.c_int, [range(-1, N)]),
        "qrd_ir_wave_route": (ctypes.c_int, [range(0, R), range(0, N)]),
        "qrd_ir_max_rows": (ctypes.c_int, [range(-1, N)]),
        "qrd_le_wave_route": (ctypes.c_int, [range(0, R), range(0, N)]),
        "qrd_le_max_rows": (ctypes.c_int, [range(-1, N), range(-1, 67)]),
        "qrd_bs_cov_wave_route": (ctypes.c_int, [range(-1, N)]),
        "qrd_bs_fit_wave_route": (ctypes.c_int, [range(0, R), range(0, N)]),
        "qrd_bs_max_rows": (ctypes.c_int, [range(-1, N)]),
        "qrd_bs_lev_chunks": (ctypes.c_int, [list(range(-1, 1030)) + [65536, 65537, 2 ** 31 - 1]]),
        # rows past 256 blocks of 64 (16384) and past the next change of the rows per block; every width class and nrhs class
        "qrd_ormqr_skinny_ws": (ctypes.c_size_t, [range(0, 16600), [1, 31, 32, 33, 256, 257], [1, 4, 5, 16, 17]]),
        "qrd_pivot_ws_doubles": (ctypes.c_size_t, [range(1, 1100)]),
        "qrd_pivot_ws_ints": (ctypes.c_size_t, [range(1, 1100)]),
    }
    import itertools
    for name, (res, axes) in grids.items():
        fp, fs = _sig(prod, name, res, len(axes)), _sig(stub, name, res, len(axes))
        count = 0
        for args in itertools.product(*axes):
            a, b = fp(*args), fs(*args)
            assert a == b, f"{name}{args}: the product returns {a}, the stub {b}"
            count += 1
        assert count >= 60, name
    for lib in (prod, stub):
        lib.qrd_ormqr_skinny_blocks.restype = ctypes.c_int
        lib.qrd_ormqr_skinny_blocks.argtypes = [ctypes.c_int, ctypes.POINTER(ctypes.c_int)]
        lib.qrd_pivot_ws_bind.restype = None
        lib.qrd_pivot_ws_bind.argtypes = [ctypes.POINTER(_PivotWs), ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
    for mk in list(range(1, 70000)) + [262144, 262145, 1 << 24, (1 << 24) + 1]:
        ra, rb = ctypes.c_int(-1), ctypes.c_int(-1)
        assert prod.qrd_ormqr_skinny_blocks(mk, ctypes.byref(ra)) == stub.qrd_ormqr_skinny_blocks(mk, ctypes.byref(rb)) and ra.value == rb.value, mk
    for n in range(1, 1100):
        wa, wb = _PivotWs(), _PivotWs()
        prod.qrd_pivot_ws_bind(ctypes.byref(wa), n, 1 << 20, 1 << 30)
        stub.qrd_pivot_ws_bind(ctypes.byref(wb), n, 1 << 20, 1 << 30)
        assert bytes(wa) == bytes(wb), n
