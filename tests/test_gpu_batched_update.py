"""-m gpu: batched row append / removal and the batched accumulator (mi355x_qr.h section 8d), member by member.

Inputs as in test_gpu_downdate.py: standard-normal rows from a fixed seed; a member's R is numpy's QR of rows that really contain the
removed ones (scattered among the kept ones); n + 8 rows are kept, so at least that many survive (at least p_add where rows are only
added); the right-hand sides are a fitted part plus noise of the same size.  Shapes (n, nrhs, p_add + p_del): the wave route at each register width and at its edges (32 columns,
64 rows), the first shapes past each edge, and the workgroup route up to qr_tpqrt_batched_max_rows; each with every row added, every row
removed, and half and half; batches of 9, 5 (a partial workgroup on the wave route) and 1.

Bounds (those of test_gpu_downdate.py / test_gpu_update.py): the Gram identity R'^T R' = R^T R + B^T S B to n eps |R^T R|; R' against the
longdouble instance of tests/batched_update_ref.py to 50 kappa(R') eps; the signed column norms |C1|^2 + C2^T S C2 kept to (n + p) eps.
Those kernels are blocked and these are not, so every input is first run through the float64 instance of the restatement on the CPU and
kept only if that stays within HALF of each bound (another seed is drawn otherwise): what the GPU then exceeds is the kernel's doing.
The ratios of both are printed and listed in DESIGN.md section 7k.
"""
import functools

import numpy as np
import pytest
import torch

import batched_update_ref as U
import hp_ref as H

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
SENTINEL = -7.25e33
BATCH = 9


@pytest.fixture(scope="module")
def plan(qr):
    p = qr.Plan(64, 8, 0, 0)              # deliberately small: the batched calls take the plan's stream, not its shape
    yield p
    p.close()


def _up(x):
    t = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    torch.cuda.synchronize()
    return t


def _down(t):
    torch.cuda.synchronize()
    return t.detach().cpu().numpy()


def _pack(A):
    """(batch, rows, cols) -> the packed column-major batch as a (batch, cols, rows) array"""
    return np.ascontiguousarray(np.asarray(A).transpose(0, 2, 1))


def _draw(rng, n, nrhs, p_add, p_del):
    """one member: R of [kept ; removed] with the removed rows scattered, the block [new ; removed], Z = (Q^T y)(0:n), the block's
    right-hand sides, and the surviving rows with theirs"""
    # n + 8 rows are kept wherever rows leave (the hard case of a removal).  Where rows are only added R holds at least as many rows as
    # arrive: the Gram bound is relative to |R^T R| of the triangle that goes in, and its rounding is that of the one that comes out
    nkeep = n + 8 if p_del else max(n + 8, p_add)
    rows = rng.standard_normal((nkeep + p_del, n))
    new = rng.standard_normal((p_add, n))
    x0 = rng.standard_normal((n, nrhs)) / np.sqrt(n)
    y, ynew = rows @ x0 + rng.standard_normal((nkeep + p_del, nrhs)), new @ x0 + rng.standard_normal((p_add, nrhs))
    gone = np.sort(rng.choice(nkeep + p_del, p_del, replace=False))
    mask = np.ones(nkeep + p_del, bool)
    mask[gone] = False
    Q, R = np.linalg.qr(rows)
    return dict(R=np.triu(R), B=np.vstack([new, rows[gone]]), C1=Q.T @ y, C2=np.vstack([ynew, y[gone]]),
                A=np.vstack([rows[mask], new]), Y=np.vstack([y[mask], ynew]))


_measures = U.measures              # the three ratios to their bounds for one member's results


@functools.lru_cache(maxsize=None)
def _case(n, nrhs, p_add, p_del, batch=BATCH):
    """`batch` members whose float64 restatement stays within half of every bound; stacked (batch, rows, cols) arrays, read-only, with
    the longdouble R' and the restatement's worst ratios"""
    members, refs, worst, seed = [], [], np.zeros(3), 0
    while len(members) < batch:
        assert seed < 400 * batch, "no input on which the float64 restatement keeps half the bounds"
        rng = np.random.default_rng(100000 * n + 1000 * nrhs + 10 * (p_add + p_del) + (p_add > 0) + 2 * (p_del > 0) + 7919 * seed)
        seed += 1
        m = _draw(rng, n, nrhs, p_add, p_del)
        Rf, _, _, Zf, Ef, info = U.update(m["R"], m["B"], p_add, m["C1"], m["C2"], np.float64)
        Rld = U.update(m["R"], m["B"], p_add, dtype=H.LD)[0]
        if info:
            continue
        r = np.array(_measures(n, p_add, m, Rf, Zf, Ef, Rld))
        if np.all(r <= 0.5):
            members.append(m)
            refs.append(Rld)
            worst = np.maximum(worst, r)
    out = {k: np.stack([m[k] for m in members]) for k in members[0]}
    for a in out.values():
        a.setflags(write=False)
    out["Rld"], out["ref"] = refs, worst
    return out


def _run(plan, n, nrhs, p_add, p_del, R, B, C1, C2, tpqrt=False):
    """the packed call on a sentinel-filled lower triangle.  Returns the results as (batch, rows, cols) arrays and the device buffers"""
    b, p = len(R), p_add + p_del
    low = np.tril(np.full((n, n), SENTINEL), -1)
    dR, dB = _up(_pack(np.triu(R) + low)), _up(_pack(B))
    dtau, dinfo = _up(np.full((b, n), SENTINEL)), _up(np.full(b, 77, dtype=np.int32))
    d1, d2 = (_up(_pack(C1)), _up(_pack(C2))) if nrhs else (None, None)
    if tpqrt:
        plan.tpqrt_batched(dR, n, n, n * n, dB, p, p, p * n, dtau, n, b, d1, n, n * nrhs, d2, p, p * nrhs, nrhs)
    else:
        plan.tphqrt_batched(dR, n, n, n * n, dB, p_add, p_del, p, p * n, dtau, n, dinfo, b, d1, n, n * nrhs, d2, p, p * nrhs, nrhs)
    plan.sync()
    out = dict(R=_down(dR).transpose(0, 2, 1), V=_down(dB).transpose(0, 2, 1), tau=_down(dtau), info=_down(dinfo),
               C1=_down(d1).transpose(0, 2, 1) if nrhs else np.zeros((b, n, 0)), C2=_down(d2).transpose(0, 2, 1) if nrhs else np.zeros((b, p, 0)))
    return out, (dB, dtau)


def _same(a, b, idx=slice(None), keys=("R", "V", "tau", "info", "C1", "C2")):
    return all(np.array_equal(a[k][idx], b[k]) for k in keys)


WAVE = [(1, 0, 1), (3, 1, 2), (4, 0, 5), (8, 2, 5), (15, 1, 33), (31, 1, 64), (32, 0, 64)]
PAST = [(8, 1, 65), (30, 3, 10), (33, 0, 7)]
WG = [(20, 3, 256), (40, 24, 100), (64, 0, None), (63, 1, None)]
SPLITS = ["added", "removed", "mixed"]


def _split(qr, n, nrhs, p, split):
    p = qr.tpqrt_batched_max_rows(n + nrhs) if p is None else p
    return {"added": (p, 0), "removed": (0, p), "mixed": ((p + 1) // 2, p // 2)}[split]


@pytest.mark.parametrize("split", SPLITS)
@pytest.mark.parametrize("n,nrhs,p", WAVE + PAST + WG)
def test_update_against_the_restatement_and_bitwise_properties(qr, plan, n, nrhs, p, split):
    p_add, p_del = _split(qr, n, nrhs, p, split)
    wave = n + nrhs <= 32 and p_add + p_del <= 64
    assert wave == ((n, nrhs, p) in WAVE)                  # the case sits on the route it is meant for
    p = p_add + p_del
    c = _case(n, nrhs, p_add, p_del)
    args = (c["R"], c["B"], c["C1"], c["C2"])
    out, (dV, dtau) = _run(plan, n, nrhs, p_add, p_del, *args)
    assert np.all(out["info"] == 0)
    assert np.array_equal(np.tril(out["R"], -1), np.broadcast_to(np.tril(np.full((n, n), SENTINEL), -1), out["R"].shape))
    for k in ("R", "V", "tau", "C1", "C2"):
        assert np.all(np.isfinite(np.triu(out[k]) if k == "R" else out[k])), k
    worst = np.zeros(3)
    for q in range(BATCH):
        m = {k: c[k][q] for k in ("R", "B", "C1", "C2")}
        worst = np.maximum(worst, _measures(n, p_add, m, np.triu(out["R"][q]), out["C1"][q], out["C2"][q], c["Rld"][q]))
    print(f"bu ({n},{nrhs},{p_add}+{p_del}) {'wave' if wave else 'wg'}: ratios to the bounds gram / R' / invariant: "
          f"GPU {worst[0]:.3f} {worst[1]:.3f} {worst[2]:.3f}, float64 restatement {c['ref'][0]:.3f} {c['ref'][1]:.3f} {c['ref'][2]:.3f}")
    if nrhs:                                               # the stored reflectors on fresh copies reproduce the ride-along result
        e1, e2 = _up(_pack(c["C1"])), _up(_pack(c["C2"]))
        plan.tpmqrt_batched("T", dV, p_add, p_del, n, p, p * n, dtau, n, e1, n, n * nrhs, e2, p, p * nrhs, nrhs, BATCH)
        plan.sync()
        Y1, Y2 = _down(e1).transpose(0, 2, 1), _down(e2).transpose(0, 2, 1)
        scale = np.sqrt((c["C1"] ** 2).sum(axis=1) + (c["C2"] ** 2).sum(axis=1))
        back = max(np.max(np.abs(Y1 - out["C1"]).max(axis=1) / scale), np.max(np.abs(Y2 - out["C2"]).max(axis=1) / scale))
        assert back <= (n + p) * EPS, back / EPS
    assert worst[0] <= 1.0, "Gram identity"
    assert worst[1] <= 1.0, "R' against the longdouble reference"
    assert worst[2] <= 1.0, "signed column norms"
    # bitwise: a repeat; the first five members as a batch of five; member 7 alone
    assert _same(out, _run(plan, n, nrhs, p_add, p_del, *args)[0])
    assert _same(out, _run(plan, n, nrhs, p_add, p_del, *(a[:5] for a in args))[0], slice(0, 5))
    assert _same(out, _run(plan, n, nrhs, p_add, p_del, *(a[7:8] for a in args))[0], slice(7, 8))
    if p_del == 0:
        assert _same(out, _run(plan, n, nrhs, p_add, 0, *args, tpqrt=True)[0], keys=("R", "V", "tau", "C1", "C2"))


def test_trans_n_undoes_trans_t_for_added_rows(qr, plan):
    n, nrhs, p = 15, 3, 33
    c = _case(n, 1, p, 0)
    _, (dV, dtau) = _run(plan, n, 1, p, 0, c["R"], c["B"], c["C1"], c["C2"])
    rng = np.random.default_rng(1533)
    F1, F2 = rng.standard_normal((BATCH, n, nrhs)), rng.standard_normal((BATCH, p, nrhs))
    e1, e2 = _up(_pack(F1)), _up(_pack(F2))
    plan.tpmqrt_batched("T", dV, p, 0, n, p, p * n, dtau, n, e1, n, n * nrhs, e2, p, p * nrhs, nrhs, BATCH)
    plan.sync()
    assert np.abs(_down(e1).transpose(0, 2, 1) - F1).max() > 0.01
    plan.tpmqrt_batched("N", dV, p, 0, n, p, p * n, dtau, n, e1, n, n * nrhs, e2, p, p * nrhs, nrhs, BATCH)
    plan.sync()
    err = max(np.abs(_down(e1).transpose(0, 2, 1) - F1).max(), np.abs(_down(e2).transpose(0, 2, 1) - F2).max())
    assert err <= (n + p) * EPS * np.sqrt((F1 ** 2).sum(axis=1).max() + (F2 ** 2).sum(axis=1).max())


@pytest.mark.parametrize("n,nrhs,p_add,p_del", [(30, 3, 5, 5), (8, 2, 3, 2)])
def test_padded_layout_is_respected_and_equals_the_packed_call(qr, plan, n, nrhs, p_add, p_del):
    p, batch, tail = p_add + p_del, 5, 13
    c = _case(n, nrhs, p_add, p_del)
    args = [a[:batch] for a in (c["R"], c["B"], c["C1"], c["C2"])]
    want = _run(plan, n, nrhs, p_add, p_del, *args)[0]
    ldr, ldb, ld1, ld2 = n + 3, p + 2, n + 1, p + 4
    sr, sb, st, s1, s2 = ldr * n + 5, ldb * n + 7, n + 2, ld1 * nrhs + 3, ld2 * nrhs + 11
    view = lambda b, s, ld, cols, rows: np.lib.stride_tricks.as_strided(b, (batch, cols, rows), (8 * s, 8 * ld, 8))
    bufs = {k: np.full(batch * s + tail, SENTINEL) for k, s in (("R", sr), ("B", sb), ("tau", st), ("C1", s1), ("C2", s2))}
    geo = {"R": (sr, ldr, n, n), "B": (sb, ldb, n, p), "tau": (st, n, 1, n), "C1": (s1, ld1, nrhs, n), "C2": (s2, ld2, nrhs, p)}
    view(bufs["R"], *geo["R"])[...] = _pack(np.triu(args[0]) + np.tril(np.full((n, n), SENTINEL), -1))
    view(bufs["B"], *geo["B"])[...] = _pack(args[1])
    view(bufs["C1"], *geo["C1"])[...] = _pack(args[2])
    view(bufs["C2"], *geo["C2"])[...] = _pack(args[3])
    dev = {k: _up(v) for k, v in bufs.items()}
    dinfo = _up(np.full(batch, 77, dtype=np.int32))
    plan.tphqrt_batched(dev["R"], n, ldr, sr, dev["B"], p_add, p_del, ldb, sb, dev["tau"], st, dinfo, batch, dev["C1"], ld1, s1, dev["C2"], ld2, s2,
                        nrhs)
    plan.sync()
    got = {k: _down(v).copy() for k, v in dev.items()}
    assert np.all(_down(dinfo) == 0)
    assert np.array_equal(view(got["R"], *geo["R"]).transpose(0, 2, 1), want["R"])           # the strict lower triangle included
    assert np.array_equal(view(got["B"], *geo["B"]).transpose(0, 2, 1), want["V"])
    assert np.array_equal(view(got["tau"], *geo["tau"])[:, 0, :], want["tau"])
    assert np.array_equal(view(got["C1"], *geo["C1"]).transpose(0, 2, 1), want["C1"])
    assert np.array_equal(view(got["C2"], *geo["C2"]).transpose(0, 2, 1), want["C2"])
    for k in got:                                          # gaps and tails came back intact
        view(got[k], *geo[k])[...] = SENTINEL
        assert np.all(got[k] == SENTINEL), k
    # the apply kernel with padded right-hand sides
    F1, F2 = args[2], args[3]
    e1, e2 = np.full(batch * s1 + tail, SENTINEL), np.full(batch * s2 + tail, SENTINEL)
    view(e1, *geo["C1"])[...] = _pack(F1)
    view(e2, *geo["C2"])[...] = _pack(F2)
    d1, d2 = _up(e1), _up(e2)
    plan.tpmqrt_batched("T", dev["B"], p_add, p_del, n, ldb, sb, dev["tau"], st, d1, ld1, s1, d2, ld2, s2, nrhs, batch)
    plan.sync()
    g1, g2 = _down(d1).copy(), _down(d2).copy()
    assert np.abs(view(g1, *geo["C1"]).transpose(0, 2, 1) - want["C1"]).max() <= (n + p) * EPS * np.abs(F1).max() * np.sqrt(n + p)
    view(g1, *geo["C1"])[...] = SENTINEL
    view(g2, *geo["C2"])[...] = SENTINEL
    assert np.all(g1 == SENTINEL) and np.all(g2 == SENTINEL)


def _stranger(c, q, col, p_add):
    """member q's last removed row becomes 100 |R| e_col: a row the matrix never held; the columns before `col` go through (the row is
    zero there, and stays zero), column `col` meets d < 0"""
    B = c["B"].copy()
    B[q, -1, :] = 0.0
    B[q, -1, col] = 100.0 * np.linalg.norm(c["R"][q])
    assert B.shape[1] > p_add
    return B


@pytest.mark.parametrize("n,nrhs,p_add,p_del", [(8, 2, 3, 2), (40, 24, 50, 50)])
def test_scaling_by_powers_of_two_is_bitwise_equivariant(qr, plan, n, nrhs, p_add, p_del):
    """[R ; B] by 2^40, the right-hand sides by 2^-77: R' scales, V and tau do not change, [C1 ; C2] scale; the info words -- member 2
    fails at column 3 -- are the same"""
    c = _case(n, nrhs, p_add, p_del)
    B = _stranger(c, 2, 3, p_add)
    a = _run(plan, n, nrhs, p_add, p_del, c["R"], B, c["C1"], c["C2"])[0]
    s, r = 2.0 ** 40, 2.0 ** -77
    b = _run(plan, n, nrhs, p_add, p_del, s * c["R"], s * B, r * c["C1"], r * c["C2"])[0]
    assert list(a["info"]) == [0, 0, 4, 0, 0, 0, 0, 0, 0] and np.array_equal(a["info"], b["info"])
    ok = a["info"] == 0
    assert np.array_equal(np.triu(b["R"]), s * np.triu(a["R"]))
    assert np.array_equal(b["V"][ok], a["V"][ok]) and np.array_equal(b["tau"][ok], a["tau"][ok])
    assert np.array_equal(b["C1"], r * a["C1"]) and np.array_equal(b["C2"], r * a["C2"])
    assert np.array_equal(b["V"][2], s * a["V"][2])        # the member that failed holds its (scaled) input


@pytest.mark.parametrize("n,nrhs,p_add,p_del", [(8, 2, 3, 2), (33, 0, 4, 3)])
def test_an_exactly_zero_block_column_gives_tau_zero_and_leaves_its_column_alone(qr, plan, n, nrhs, p_add, p_del):
    """column 0 of every added and removed row is zero (so it was zero in those rows of the matrix R came from)"""
    rng = np.random.default_rng(n)
    batch = 5
    kept, old, new = rng.standard_normal((batch, n + 8, n)), rng.standard_normal((batch, p_del, n)), rng.standard_normal((batch, p_add, n))
    old[:, :, 0] = 0.0
    new[:, :, 0] = 0.0
    R = np.stack([np.triu(np.linalg.qr(np.vstack([kept[q], old[q]]), mode="r")) for q in range(batch)])
    B = np.concatenate([new, old], axis=1)
    C1, C2 = rng.standard_normal((batch, n, nrhs)), rng.standard_normal((batch, p_add + p_del, nrhs))
    out = _run(plan, n, nrhs, p_add, p_del, R, B, C1, C2)[0]
    assert np.all(out["info"] == 0)
    assert np.all(out["tau"][:, 0] == 0.0) and np.all(out["V"][:, :, 0] == 0.0)
    Rn = np.triu(out["R"])
    assert np.array_equal(Rn[:, :, 0], R[:, :, 0]) and np.array_equal(Rn[:, 0, :], R[:, 0, :])
    assert np.array_equal(out["C1"][:, 0, :], C1[:, 0, :])
    for q in range(batch):
        G0 = R[q].T @ R[q]
        g = np.linalg.norm(Rn[q].T @ Rn[q] - (G0 + new[q].T @ new[q] - old[q].T @ old[q])) / np.linalg.norm(G0)
        assert g <= n * EPS, (q, g / EPS)


@pytest.mark.parametrize("n,nrhs,p_add,p_del", [(8, 2, 3, 2), (40, 24, 50, 50)])
def test_primitive_failure_is_isolated_to_its_member(qr, plan, n, nrhs, p_add, p_del):
    """member 2 fails at column 3, member 6 at column 0: both are bitwise what they were, the others as in a batch of only them"""
    c = _case(n, nrhs, p_add, p_del)
    B = _stranger(dict(B=_stranger(c, 2, 3, p_add), R=c["R"]), 6, 0, p_add)
    out = _run(plan, n, nrhs, p_add, p_del, c["R"], B, c["C1"], c["C2"])[0]
    assert list(out["info"]) == [0, 0, 4, 0, 0, 0, 1, 0, 0]
    for q, col in ((2, 3), (6, 0)):
        assert U.update(c["R"][q], B[q], p_add, c["C1"][q], c["C2"][q])[5] == col + 1      # the restatement fails at the same column
        assert np.array_equal(np.triu(out["R"][q]), c["R"][q]) and np.array_equal(out["V"][q], B[q])
        assert np.all(out["tau"][q] == SENTINEL)
        assert np.array_equal(out["C1"][q], c["C1"][q]) and np.array_equal(out["C2"][q], c["C2"][q])
    rest = [0, 1, 3, 4, 5, 7, 8]
    alone = _run(plan, n, nrhs, p_add, p_del, c["R"][rest], B[rest], c["C1"][rest], c["C2"][rest])[0]
    assert _same(out, alone, rest)


# ---- the accumulator ----------------------------------------------------------------------------------------------------------------
class _Acc:
    """a batched accumulator over host data: every call uploads packed (batch, rows, cols) arrays"""

    def __init__(self, qr, plan, n, nrhs, batch):
        self.qr, self.plan, self.n, self.nrhs, self.batch = qr, plan, n, nrhs, batch
        self.acc = qr.LsAccumulatorBatched(plan, n, nrhs, batch)
        self.keep = []

    def _dev(self, A, Y):
        dA, dY = _up(_pack(A)), _up(_pack(Y))
        self.keep += [dA, dY]                  # launches are queued, not awaited: the buffers live as long as the accumulator
        return dA, dY, A.shape[1]

    def push(self, A, Y):
        dA, dY, p = self._dev(A, Y)
        self.acc.push(dA, p, p, p * self.n, dY, p, p * self.nrhs)
        self.plan.sync()
        assert np.array_equal(_down(dA), _pack(A)) and np.array_equal(_down(dY), _pack(Y)), "the inputs of a push are untouched"

    def pop(self, A, Y):
        dA, dY, p = self._dev(A, Y)
        dinfo = _up(np.full(self.batch, 77, dtype=np.int32))
        self.acc.pop(dA, p, p, p * self.n, dY, p, p * self.nrhs, dinfo)
        return _down(dinfo)

    def slide(self, An, Yn, Ao, Yo):
        dAn, dYn, pn = self._dev(An, Yn)
        dAo, dYo, po = self._dev(Ao, Yo)
        dinfo = _up(np.full(self.batch, 77, dtype=np.int32))
        self.acc.slide(dAn, pn, pn, pn * self.n, dYn, pn, pn * self.nrhs, dAo, po, po, po * self.n, dYo, po, po * self.nrhs, dinfo)
        return _down(dinfo)

    def solve(self):
        dX, dres = _up(np.full((self.batch, self.nrhs, self.n), SENTINEL)), _up(np.full((self.batch, self.nrhs), SENTINEL))
        dinfo = _up(np.full(self.batch, 77, dtype=np.int32))
        self.acc.solve(dX, self.n, self.n * self.nrhs, dinfo, dres, self.nrhs)
        self.plan.sync()
        return _down(dX).transpose(0, 2, 1), _down(dres), _down(dinfo)

    def state(self):
        return self.acc.factor_host()

    def close(self):
        self.plan.sync()
        self.acc.close()


def _check_ls(A, Y, X, resid):
    """every member against numpy.linalg.lstsq to the bounds test_gpu_batched.py uses for qr_gels_batched_dev: 50 (kappa + kappa^2 |r| /
    (|A| |x|)) eps for X, 100 |A| |x_j| eps |r_j| for the residual sum of squares"""
    wx = 0.0
    for q in range(A.shape[0]):
        Xn = np.linalg.lstsq(A[q], Y[q], rcond=None)[0]
        rn = Y[q] - A[q] @ Xn
        kappa, a2 = np.linalg.cond(A[q]), np.linalg.norm(A[q], 2)
        bound = 50 * (kappa + kappa ** 2 * np.linalg.norm(rn) / (a2 * np.linalg.norm(Xn))) * EPS
        ex = np.linalg.norm(X[q] - Xn) / np.linalg.norm(Xn)
        wx = max(wx, ex / bound)
        assert ex <= bound, (q, ex, bound)
        for j in range(Y.shape[2]):
            rj = np.linalg.norm(rn[:, j])
            assert abs(resid[q, j] ** 2 - rj * rj) <= 100 * a2 * np.linalg.norm(Xn[:, j]) * EPS * rj, (q, j)
    return wx


def _series(seed, batch, m, n, nrhs):
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((batch, m, n))
    x0 = rng.standard_normal((batch, n, nrhs)) / np.sqrt(n)
    return A, A @ x0 + rng.standard_normal((batch, m, nrhs))


@pytest.mark.parametrize("n,nrhs,chunks", [(12, 2, (5, 300, 1, 17)), (40, 3, (30, 230, 7))])
def test_push_in_uneven_chunks_then_solve_matches_numpy(qr, plan, n, nrhs, chunks):
    """one chunk is above the one-launch limit (256 rows beside 14 columns, 226 beside 43) and is split by the library"""
    batch, m = 5, sum(chunks)
    cap = qr.tpqrt_batched_max_rows(n + nrhs)
    assert max(chunks) > cap >= sorted(chunks)[-2]
    launches = sum(-(-k // cap) for k in chunks)
    A, Y = _series(n * m, batch, m, n, nrhs)
    acc = _Acc(qr, plan, n, nrhs, batch)
    o = 0
    for k in chunks:
        acc.push(A[:, o:o + k], Y[:, o:o + k])
        o += k
    X, resid, info = acc.solve()
    R, Z, rss, rows = acc.state()
    assert np.all(info == 0) and np.all(rows == m) and np.all(np.tril(R, -1) == 0.0)
    wx = _check_ls(A, Y, X, resid)
    for q in range(batch):
        G = A[q].T @ A[q]
        assert np.linalg.norm(R[q].T @ R[q] - G) / np.linalg.norm(G) <= launches * n * EPS       # n eps per update, adding linearly
    assert np.array_equal(resid, np.sqrt(rss))
    print(f"batched push n={n} chunks={chunks}: X at {wx:.3f} of its bound")
    X2, resid2, _ = acc.solve()                  # the state is untouched by a solve
    assert np.array_equal(X, X2) and np.array_equal(resid, resid2)
    acc.acc.reset()
    assert np.all(acc.state()[3] == 0) and np.all(acc.state()[0] == 0.0)
    acc.close()


def test_push_pop_push_equals_the_surviving_rows(qr, plan):
    n, nrhs, batch = 20, 3, 5
    A, Y = _series(2020, batch, 4 * n + 40, n, nrhs)
    rng = np.random.default_rng(20)
    gone = np.sort(rng.choice(4 * n, n, replace=False))
    surv = np.concatenate([np.setdiff1d(np.arange(4 * n), gone), np.arange(4 * n, 4 * n + 40)])
    acc = _Acc(qr, plan, n, nrhs, batch)
    acc.push(A[:, :4 * n], Y[:, :4 * n])
    assert np.all(acc.pop(A[:, gone], Y[:, gone]) == 0)
    acc.push(A[:, 4 * n:], Y[:, 4 * n:])
    X, resid, info = acc.solve()
    R, _, _, rows = acc.state()
    assert np.all(info == 0) and np.all(rows == len(surv))
    wx = _check_ls(A[:, surv], Y[:, surv], X, resid)
    for q in range(batch):
        As = A[q][surv]
        G = As.T @ As
        g = np.linalg.norm(R[q].T @ R[q] - G) / np.linalg.norm(G)
        Rl = np.linalg.qr(As, mode="r")
        sg = np.sign(np.diag(Rl)) * np.sign(np.diag(R[q]))
        e = np.linalg.norm(R[q] - sg[:, None] * Rl) / np.linalg.norm(Rl)
        assert g <= n * EPS, (q, g / EPS)
        assert e <= 50 * np.linalg.cond(As) * EPS, (q, e / EPS)
    print(f"batched push/pop/push: X at {wx:.3f} of its bound")
    acc.close()


def test_lstsq_rolling_batched_matches_numpy_on_every_window(qr):
    batch, n, nrhs, window, step, nwin = 5, 6, 2, 40, 4, 8
    m = window + (nwin - 1) * step
    A, Y = _series(640, batch, m, n, nrhs)
    X, resid, info = qr.lstsq_rolling_batched(A, Y, window, step)
    assert X.shape == (batch, nwin, n, nrhs) and resid.shape == (batch, nwin, nrhs) and info.shape == (batch, nwin) and np.all(info == 0)
    worst = 0.0
    for q in range(batch):
        for k in range(nwin):
            Aw, Yw = A[q, k * step:k * step + window], Y[q, k * step:k * step + window]
            kappa = np.linalg.cond(Aw)
            Xn = np.linalg.lstsq(Aw, Yw, rcond=None)[0]
            rn = np.linalg.norm(Aw @ Xn - Yw, axis=0)
            bound = kappa + kappa ** 2 * np.linalg.norm(rn) / (np.linalg.norm(Aw, 2) * np.linalg.norm(Xn))
            e = np.linalg.norm(X[q, k] - Xn) / np.linalg.norm(Xn)
            worst = max(worst, e / (bound * EPS))
            assert e <= 50 * bound * EPS, (q, k)
            assert np.max(np.abs(resid[q, k] - rn) / rn) <= 1e-12, (q, k)
    print(f"rolling batched {nwin} windows x {batch} series: worst X error {worst:.2f} of the perturbation bound (limit 50)")
    X2, resid2, _ = qr.lstsq_rolling_batched(A, Y, window, step)
    assert np.array_equal(X, X2) and np.array_equal(resid, resid2)
    X1 = qr.lstsq_rolling_batched(A[3:4], Y[3:4], window, step)[0]
    assert np.array_equal(X1[0], X[3])             # a series' result does not depend on the batch


def test_gram_drift_after_32_slides(qr, plan):
    """rounding adds at most linearly in the slides: 33 n eps for the push and 32 slides"""
    n, window, step, slides, batch = 32, 128, 8, 32, 3
    m = window + slides * step
    A, Y = _series(32128, batch, m, n, 1)
    acc = _Acc(qr, plan, n, 1, batch)
    acc.push(A[:, :window], Y[:, :window])
    for k in range(1, slides + 1):
        o, e = (k - 1) * step, (k - 1) * step + window
        assert np.all(acc.slide(A[:, e:e + step], Y[:, e:e + step], A[:, o:o + step], Y[:, o:o + step]) == 0), k
    R, _, _, rows = acc.state()
    assert np.all(rows == window)
    worst = 0.0
    for q in range(batch):
        Aw = A[q, m - window:]
        G = Aw.T @ Aw
        g = np.linalg.norm(R[q].T @ R[q] - G) / np.linalg.norm(G)
        worst = max(worst, g)
        assert g <= 33 * n * EPS, (q, g / EPS)
    print(f"batched gram drift after {slides} slides at n={n}: {worst / EPS:.2f} eps (bound {33 * n})")
    X, resid, info = acc.solve()
    assert np.all(info == 0)
    _check_ls(A[:, m - window:], Y[:, m - window:], X, resid)
    acc.close()


@pytest.mark.parametrize("n,nrhs,k2", [(8, 2, 5), (40, 3, 70)])
def test_accumulator_failure_is_isolated_to_its_member(qr, plan, n, nrhs, k2):
    """Nine members hold M rows.  A first pop of k1 rows succeeds for member 6 only (the others are handed rows they never held and keep
    their state).  The second pop, of k2 rows, leaves member 6 with n - 1 rows (-1), hands member 2 a stranger (column 3) and succeeds
    for the other seven, which end bitwise as in an accumulator that holds only them."""
    M = n + 8 + k2
    k1 = M - k2 - (n - 1)
    A, Y = _series(7 * n + k2, BATCH, M, n, nrhs)
    rest = [0, 1, 3, 4, 5, 7, 8]

    def first_pop(members):
        A1, Y1 = A[members][:, :k1].copy(), Y[members][:, :k1].copy()
        for i, q in enumerate(members):
            if q != 6:
                A1[i] *= 100.0
        return A1, Y1

    A2, Y2 = A[:, k1:k1 + k2].copy(), Y[:, k1:k1 + k2].copy()
    A2[2, -1, :] = 0.0
    A2[2, -1, 3] = 100.0 * np.linalg.norm(A[2])
    acc = _Acc(qr, plan, n, nrhs, BATCH)
    acc.push(A, Y)
    i1 = acc.pop(*first_pop(list(range(BATCH))))
    assert i1[6] == 0 and np.all(np.delete(i1, 6) > 0)
    before = acc.state()
    assert list(before[3]) == [M] * 6 + [M - k1] + [M] * 2
    i2 = acc.pop(A2, Y2)
    assert list(i2) == [0, 0, 4, 0, 0, 0, -1, 0, 0]
    after = acc.state()
    for q in (2, 6):
        assert all(np.array_equal(after[i][q], before[i][q]) for i in range(4)), q
    assert list(after[3]) == [M - k2, M - k2, M, M - k2, M - k2, M - k2, M - k1, M - k2, M - k2]
    ref = _Acc(qr, plan, n, nrhs, len(rest))
    ref.push(A[rest], Y[rest])
    assert np.all(ref.pop(*first_pop(rest)) > 0)
    assert np.all(ref.pop(A2[rest], Y2[rest]) == 0)
    alone = ref.state()
    assert all(np.array_equal(after[i][rest], alone[i]) for i in range(4))
    ref.close()
    acc.close()


def test_a_member_with_fewer_than_n_rows_gets_the_info_word_of_the_solve(qr, plan):
    """member 3's second chunk is all zeros: it counts rows but adds nothing, so R(n-1, n-1) == 0 exactly and the back substitution
    reports n; the others solve"""
    n, nrhs, batch = 8, 2, 5
    A, Y = _series(88, batch, n - 1 + 9, n, nrhs)
    A[3, n - 1:] = 0.0
    Y[3, n - 1:] = 0.0
    acc = _Acc(qr, plan, n, nrhs, batch)
    acc.push(A[:, :n - 1], Y[:, :n - 1])
    acc.push(A[:, n - 1:], Y[:, n - 1:])
    X, resid, info = acc.solve()
    assert list(info) == [0, 0, 0, n, 0]
    others = [0, 1, 2, 4]
    _check_ls(A[others], Y[others], X[others], resid[others])
    acc.close()
