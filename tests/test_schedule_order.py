"""Stream ordering of the host schedule, checked without a GPU.

The stub device layer (tests/c/qrd_stub.c) keeps a happens-before model of streams and events (DESIGN "Stream-order model of the stub"):
every operand block of every launch is stamped with its stream's clock, and two accesses of which one writes, whose elements intersect and
which no record / wait / sync edge orders are reported.  `make -C cuda-qr_amd order` builds
  order_selfcheck   the model's own test: fourteen direct cases with exact report counts;
  host_order        the C host layer over the stub, one schedule configuration per process, every stream_wait_event of qr_host.c naming
                    its site (tests/c/order_sites.h);
  cov/host_order    the same with --coverage.
Checked here: every configuration runs silent; taking out any one wait (QRD_STUB_SKIP_WAIT=k) is reported, except for the sites listed --
each with the edge that implies it -- in schedule_redundant_waits.json; and gcov shows every record and wait line of qr_host.c executed,
except for those listed in schedule_unreached.json.
"""
import json
import os
import re
import subprocess
from concurrent.futures import ThreadPoolExecutor

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QR = os.path.join(ROOT, "cuda-qr_amd")
HOST_C = os.path.join(QR, "csrc", "qr_host.c")
HERE = os.path.dirname(os.path.abspath(__file__))


def _env(**extra):
    env = {k: v for k, v in os.environ.items() if not k.startswith(("MI355XQR_", "QRD_STUB_"))}
    env.update(extra)
    return env


@pytest.fixture(scope="module")
def order_build():
    out = subprocess.run(["make", "-C", QR, "order"], capture_output=True, text=True, env=_env(), timeout=600)
    assert out.returncode == 0, out.stdout[-1500:] + out.stderr[-3000:]
    exe = os.path.join(QR, "build", "order", "host_order")
    names = subprocess.run([exe, "list"], capture_output=True, text=True, check=True).stdout.split()
    assert len(names) >= 30
    return {"make": out.stdout, "exe": exe, "cov": os.path.join(QR, "build", "order", "cov", "host_order"), "configs": names}


def _strip_comments(text):
    """C comments blanked out, newlines kept (line numbers stay right)."""
    return re.sub(r"/\*.*?\*/", lambda m: re.sub(r"[^\n]", " ", m.group(0)), text, flags=re.S)


def _call_args(text, start):
    """the arguments of the call whose '(' is at text[start]"""
    depth, args, cur = 0, [], ""
    for ch in text[start:]:
        if ch == "(":
            depth += 1
            if depth == 1:
                continue
        elif ch == ")":
            depth -= 1
            if depth == 0:
                args.append(cur.strip())
                return args
        if ch == "," and depth == 1:
            args.append(cur.strip())
            cur = ""
        else:
            cur += ch
    raise AssertionError("unbalanced call")


def schedule_sites():
    """Every qrd_event_record / qrd_stream_wait_event call of qr_host.c in source order: kind, line, function, event expression and key.
    key = function:expression for a wait, function:record:expression for a record, '#n' appended to the n-th (n >= 2) call with the same key
    in the file.  The i-th wait (from 0) is the one order_sites.h numbers i."""
    text = _strip_comments(open(HOST_C).read())
    func_at = []          # (offset, name) of every function definition: a line that starts in column 0 and ends its declarator with ')' and '{' below
    for m in re.finditer(r"^(?:[A-Za-z_][\w \*]*?[ \*])?(\w+)\([^;{}]*\)\s*\n\{", text, flags=re.M):
        func_at.append((m.start(), m.group(1)))
    sites, seen = [], {}
    for m in re.finditer(r"\b(qrd_event_record|qrd_stream_wait_event)\(", text):
        func = [name for off, name in func_at if off < m.start()][-1]
        args = _call_args(text, m.end() - 1)
        kind = "record" if m.group(1) == "qrd_event_record" else "wait"
        expr = args[0] if kind == "record" else args[1]
        key = f"{func}:{expr}" if kind == "wait" else f"{func}:record:{expr}"
        seen[key] = seen.get(key, 0) + 1
        if seen[key] > 1:
            key += f"#{seen[key]}"
        sites.append({"kind": kind, "line": text.count("\n", 0, m.start()) + 1, "func": func, "expr": expr, "key": key})
    return sites


def _run(exe, config, skip=None):
    """(reports, [(k, key), ...]) of one configuration; skip: the wait to take out"""
    extra = {"QRD_STUB_SKIP_WAIT": str(skip)} if skip else {}
    out = subprocess.run([exe, config], capture_output=True, text=True, env=_env(**extra), timeout=120)
    assert out.returncode == 0, f"{config} (skip {skip}): exit {out.returncode}\n" + out.stdout[-500:] + out.stderr[-2000:]
    lines = out.stdout.splitlines()
    head = [ln for ln in lines if ln.startswith("ORDER ")]
    assert len(head) == 1, out.stdout[-500:]
    waits = _run.waits
    got = []
    for ln in lines:
        if ln.startswith("WAIT "):
            _, k, site, raw = ln.split(" ", 3)
            w = waits[int(site)]
            assert raw == f"{w['func']}:{w['expr']}", f"wait site {site}: the run says {raw!r}, qr_host.c says {w['func']}:{w['expr']}"
            got.append((int(k), w["key"]))
    assert len(got) == int(head[0].split()[2])
    return int(head[0].split()[1]), got, out.stderr


_run.waits = [s for s in schedule_sites() if s["kind"] == "wait"]


def test_sites_are_found():
    sites = schedule_sites()
    assert len(sites) >= 49 and len({s["key"] for s in sites}) == len(sites)
    funcs = {s["func"] for s in sites}
    assert {"geqrf_issue_inner", "enter_phase", "factor_panel_inner", "apply_small_t"} <= funcs, funcs


def test_order_model_selfcheck(order_build):
    """the fourteen cases of tests/c/order_selfcheck.c, exact counts (the make target runs it; once more for its output)"""
    out = subprocess.run([os.path.join(QR, "build", "order", "order_selfcheck")], capture_output=True, text=True, env=_env(), timeout=60)
    assert out.returncode == 0, out.stdout + out.stderr[-2000:]
    rows = [ln for ln in out.stdout.splitlines() if "expected" in ln]
    assert len(rows) == 14 and not any("WRONG" in ln for ln in rows), out.stdout
    assert [int(re.search(r"expected (\d+)", ln).group(1)) for ln in rows] == [1, 0, 1, 1, 0, 0, 1, 1, 0, 1, 0, 1, 1, 0]
    assert "order self-check ok" in out.stdout


@pytest.fixture(scope="module")
def baseline(order_build):
    """every configuration once, nothing skipped"""
    with ThreadPoolExecutor(8) as ex:
        res = list(ex.map(lambda c: _run(order_build["exe"], c), order_build["configs"]))
    return dict(zip(order_build["configs"], res))


def test_every_configuration_is_silent(baseline):
    bad = {c: (r[0], r[2][:600]) for c, r in baseline.items() if r[0] != 0}
    assert not bad, bad
    assert sum(len(r[1]) for r in baseline.values()) > 1000          # the configurations do wait


def test_wait_removal_sweep(order_build, baseline):
    """Each wait of each configuration taken out in turn (a site already shown detectable is not tried again in later runs): the sites
    whose removal nothing reports are exactly the committed list of redundant waits."""
    listed = json.load(open(os.path.join(HERE, "schedule_redundant_waits.json")))
    assert all(isinstance(v, str) and len(v) > 20 for v in listed.values())          # each with the edge that implies it
    reached, detected = set(), {}
    for config in order_build["configs"]:
        waits = baseline[config][1]
        reached |= {key for _, key in waits}
        todo = [(k, key) for k, key in waits if key not in detected]
        with ThreadPoolExecutor(8) as ex:
            res = list(ex.map(lambda kk: _run(order_build["exe"], config, skip=kk[0])[0], todo))
        for (k, key), reports in zip(todo, res):
            if reports > 0:
                detected.setdefault(key, f"{config} wait {k}: {reports} reports")
    undetected = reached - set(detected)
    print("detected:", json.dumps(detected, indent=1))
    print("undetected:", sorted(undetected))
    assert undetected == set(listed), {"not listed": sorted(undetected - set(listed)), "listed but detected or never reached": sorted(set(listed) - undetected)}


def test_every_record_and_wait_line_is_reached(order_build):
    """gcov over all configurations: every qrd_event_record / qrd_stream_wait_event call of qr_host.c was executed, except the listed ones"""
    listed = json.load(open(os.path.join(HERE, "schedule_unreached.json")))
    cov_dir = os.path.dirname(order_build["cov"])
    for f in os.listdir(cov_dir):
        if f.endswith(".gcda"):
            os.remove(os.path.join(cov_dir, f))
    for config in order_build["configs"]:          # one after the other: they merge their counts into one file
        out = subprocess.run([order_build["cov"], config], capture_output=True, text=True, env=_env(), timeout=120)
        assert out.returncode == 0 and out.stdout.startswith("ORDER 0 "), (config, out.stdout[:200], out.stderr[-1000:])
    out = subprocess.run(["gcov", "-b", "-c", "-t", "-o", cov_dir, os.path.join(cov_dir, "qr_host.o")], capture_output=True, text=True,
                         cwd=QR, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    # per source line of qr_host.c: the "call N ..." records gcov -b prints under it
    calls, cur, in_file = {}, None, False
    for ln in out.stdout.splitlines():
        m = re.match(r"\s*(\S+):\s*(\d+):", ln)
        if m:
            if m.group(2) == "0":
                in_file = ln.rstrip().endswith("Source:csrc/qr_host.c") or (in_file and "Source:" not in ln)
            cur = int(m.group(2)) if in_file else None
            if cur:
                calls.setdefault(cur, [])
        elif cur and ln.startswith("call "):
            calls[cur].append("never executed" not in ln and not re.search(r"returned 0(%|$)", ln))
    unreached = set()
    for s in schedule_sites():
        assert calls.get(s["line"]), f"gcov shows no call on line {s['line']} ({s['key']})"
        if not all(calls[s["line"]]):
            unreached.add(s["key"])
    assert unreached == set(listed), {"not listed": sorted(unreached - set(listed)), "listed but reached": sorted(set(listed) - unreached)}
