"""helpers shared by the -m gpu tests (device buffers are torch tensors holding column-major data)."""
import numpy as np
import torch


def dev(A):
    """numpy (m x n) -> torch cuda tensor of shape (n, m): the column-major image of A."""
    t = torch.from_numpy(np.ascontiguousarray(np.asarray(A, dtype=np.float64).T)).cuda()
    torch.cuda.synchronize()      # torch's stream and the plan's (non-blocking) streams are not ordered
    return t


def host(t):
    """inverse of dev()."""
    torch.cuda.synchronize()
    return np.asfortranarray(t.detach().cpu().numpy().T)


def zeros(m, n):
    t = torch.zeros((n, m), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()      # the fill runs on torch's stream: finish it before a plan stream writes t
    return t


def rel(a, b):
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)


EPS = float(np.finfo(np.float64).eps)


def within(tag, got, ref, cap=float("inf"), measured=None, suffix="", floor=EPS):
    """got <= min(max(FACTOR * ref, floor), cap) with FACTOR = 4, or twice the ratio `measured` (a test file's MEASURED table) records for
    tag: the rule of the tests against the float64 instance of the extended-precision reference.  Prints the ratio."""
    factor = 2.0 * measured[tag] if measured and tag in measured else 4.0
    bound = min(max(factor * ref, floor), cap)
    print(f"RATIO {tag}{suffix}: {got:.3e} is {got / max(ref, EPS / 4):.2f} x the float64 reference {ref:.3e}; bound {bound:.3e}")
    assert np.isfinite(got) and got <= bound, (tag, got, ref, bound)


class Buf:
    """A matrix in a device buffer as the kernel unit tests lay it out: column-major at leading dimension ld, `off` doubles into the
    buffer, `extra` whole columns after it and three doubles behind those, all of it `fill`; the rows m .. ld of its columns hold `pad`
    (default: fill).  out() fetches the whole buffer; check() asserts that every double outside `region` (a boolean m x n mask of the
    entries the launch may write; None: nothing) is bitwise what went in."""

    def __init__(self, A, ld, off=1, fill=-3.5, pad=None, extra=1):
        A = np.asarray(A, dtype=np.float64)
        self.m, self.n, self.ld, self.off, self.cols = A.shape[0], A.shape[1], ld, off, A.shape[1] + extra
        assert ld >= self.m
        self.h = np.full(off + ld * self.cols + 3, float(fill))
        body = self.h[off:off + ld * self.n].reshape(self.n, ld)
        if pad is not None:
            body[:, self.m:] = pad
        body[:, :self.m] = A.T
        self.t = torch.from_numpy(self.h.copy()).cuda()
        torch.cuda.synchronize()
        self.ptr = self.t.data_ptr() + 8 * off

    def out(self):
        torch.cuda.synchronize()
        return self.t.cpu().numpy()

    def mat(self, h=None):
        """the m x n matrix of the buffer image h (default: as fetched now)"""
        h = self.out() if h is None else h
        return np.asfortranarray(h[self.off:self.off + self.ld * self.n].reshape(self.n, self.ld)[:, :self.m].T)

    def check(self, region=None, what="buffer"):
        h = self.out()
        same = h.view(np.uint64) == self.h.view(np.uint64)
        if region is not None:
            body = same[self.off:self.off + self.ld * self.n].reshape(self.n, self.ld)
            body[:, :self.m] |= np.asarray(region, dtype=bool).T
        assert same.all(), f"{what}: written outside its output region at buffer offsets {np.flatnonzero(~same)[:8]}"
        return self.mat(h)


def bits(a, b):
    """bitwise equality of two float64 arrays (NaN payloads and the sign of zero included)"""
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and bool(np.all(a.view(np.uint64) == b.view(np.uint64)))


def ivec(values, sentinel=-9):
    """device int32 vector with a sentinel on either side: (whole tensor, pointer to the first value)"""
    t = torch.tensor([sentinel, *[int(v) for v in values], sentinel], dtype=torch.int32).cuda()
    torch.cuda.synchronize()
    return t, t.data_ptr() + 4


def ivec_out(t, sentinel=-9):
    torch.cuda.synchronize()
    h = t.cpu().numpy()
    assert h[0] == sentinel and h[-1] == sentinel, "written outside the int vector"
    return h[1:-1].copy()
