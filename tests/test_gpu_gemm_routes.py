"""-m gpu: every route of the GEMM launch layer of qr_kernels.hip (launch_nn, launch_tn, gemm_tn_impl, gemm_nn_update_impl, qrd_gemm_nn_batch,
qrd_slab_reduce), element by element.

Each case names the route it was written for -- tile, fast interior, K split, row piece of the reduction, flags -- and asserts it from the
record the launch functions leave (qrd_gemm_last_route), so a case cannot quietly stop reaching its branch.  The rule a case rests on is
quoted next to it; the compute units of the stream enter only the split-K cases, which assert ranges.

Buffers (gemm_ref.Layout): a guard band of 4096 doubles in front and behind, the base optionally 8 bytes off a 16-byte boundary, the
leading dimension given by the case.  Inputs hold NaN everywhere outside the logical operand (guard bands, rows beyond M / K, unused slabs),
so an over-read shows as a NaN in the result; outputs hold a sentinel outside the logical result and, inside, NaN for beta == 0 and C0
otherwise, so an over-write shows as a changed sentinel and an element never written as a NaN.  After each call: the return code, the route,
no NaN in the result, the componentwise bound of gemm_ref (derived, not measured), padding and inputs bit-identical, and a second run on
new buffers bitwise equal to the first.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import gemm_ref as G
import hp_ref

pytestmark = pytest.mark.gpu

NN, NN_UPDATE, TN, NN_BATCH, SLAB_REDUCE = 1, 2, 3, 4, 5                       # out[0] of qrd_gemm_last_route
FAST, MIXED, WIDE, EVEN, KREM, TM, DIRECT, W8 = 1, 2, 4, 8, 16, 32, 64, 128    # QRD_ROUTE_* of qr_device.h
CAP = 1 << 20           # doubles of slab space unless the case says otherwise: room for 64 slabs of 128 x 128, too little for the even split
                        # of a whole-tile product ((2 CUs + tiles) 128 x 128 partials), which has tests of its own (test_gpu_tn_even.py)
_vp, _i, _d, _z = C.c_void_p, C.c_int, C.c_double, C.c_size_t


@pytest.fixture(scope="module")
def q(qr):
    qr.check(qr.lib.qrd_init(), "qrd_init")
    lib = qr.lib
    gemm = [_vp, _i, _i, _i, _d, _vp, _i, _vp, _i, _d, _vp, _i]
    for name, args in (("qrd_gemm_last_route", [C.POINTER(C.c_int)]),
                       ("qrd_gemm_nn_update", gemm), ("qrd_gemm_nn_update2", gemm),
                       ("qrd_gemm_nn_batch", [_vp, _i, _i, _i, _d, _vp, _i, _z, _vp, _i, _z, _d, _vp, _i, _z, _i]),
                       ("qrd_slab_reduce", [_vp, _i, _i, _i, _vp, _i, _z, _vp, _i])):
        getattr(lib, name).restype = C.c_int
        getattr(lib, name).argtypes = args
    lib.qrd_stream_create_cumask.argtypes = [C.POINTER(C.c_void_p), C.c_int, C.c_int]
    lib.qrd_stream_sync.argtypes = [C.c_void_p]
    lib.qrd_stream_destroy.argtypes = [C.c_void_p]
    lib.qrd_stream_cus.argtypes = [C.c_void_p]
    return qr


def _route(q):
    out = (C.c_int * 8)()
    q.lib.qrd_gemm_last_route(out)
    return dict(zip(("entry", "tile", "Mi", "Ni", "ksplit", "piece", "flags", "serial"), out))


def _check_route(r, want, what):
    """want: field -> value, or a predicate; `flags` -> (bits that must be set, bits that must be clear)"""
    for key, v in want.items():
        if key == "flags":
            assert r["flags"] & v[0] == v[0] and r["flags"] & v[1] == 0, (what, "flags", r)
        elif callable(v):
            assert v(r[key]), (what, key, r)
        else:
            assert r[key] == v, (what, key, r)


def _dev(flat):
    t = torch.from_numpy(flat).cuda()
    torch.cuda.synchronize()
    assert t.data_ptr() % 16 == 0
    return t


def _ptr(t, L):
    return t.data_ptr() + 8 * L.base


def _flat(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


_DATA = {}


def _data(M, N, K):
    """operands (op(A) is M x K), the product in the reference precision and its envelope: once per shape, shared and read-only"""
    if (M, N, K) not in _DATA:
        assert (M, N, K) in G.ALL_SHAPES, "a shape of this file that tests/test_gemm_ref.py does not know"
        rng = np.random.default_rng(1000003 * M + 1009 * N + K)
        A, B, C0 = rng.standard_normal((M, K)), rng.standard_normal((K, N)), rng.standard_normal((M, N))
        T = np.triu(rng.standard_normal((M, M))) if M <= 256 else None
        P, Eab, f = G.product(A, B, False)
        plain = A @ B if f == 1 else None           # float64 numpy's own product: its error is printed next to the kernel's, never asserted
        for x in (A, B, C0, T, P, Eab, plain):
            if x is not None:
                x.setflags(write=False)
        _DATA[(M, N, K)] = (A, B, C0, T, P, Eab, f, plain)
    return _DATA[(M, N, K)]


WORST = {}          # entry -> [worst |err| / bound, worst kernel error / numpy error]


def _judge(entry, what, got, ref, E, n, f, plain_result):
    assert not np.isnan(got).any(), f"{what}: an element was never written, or a NaN outside the operands was read"
    r = G.ratio(got, ref, E, n, f)
    vs = float("nan")
    if plain_result is not None:        # longdouble reference: how the kernel's worst error compares with float64 numpy's (printed only)
        ek = float(np.abs(hp_ref.arr(got) - ref).max())
        en = float(np.abs(hp_ref.arr(plain_result) - ref).max())
        vs = ek / en if en > 0 else float("inf") if ek > 0 else 1.0
    print(f"{what}: max |err| / bound = {r:.2e} (f = {f}, n = {n}); kernel error / numpy error = {vs:.2f}")
    w = WORST.setdefault(entry, [0.0, 0.0])
    w[0], w[1] = max(w[0], r), max(w[1], vs if vs == vs else 0.0)
    assert r <= 1.0, what


def _gemm(q, entry, M, N, K, alpha, beta, route, lda=None, ldb=None, ldc=None, offA=0, offB=0, offC=0, tm=False, ldt=None,
          cap=CAP, slabs_null=False, rc=0, slabs_untouched=False, stream=None):
    """one product through `entry` ('nn', 'up', 'up2', 'tn', 'tnu', 'tnw': qrd_gemm_nn, _nn_update, _nn_update2, _tn, _tn_update, _tn_update_wide),
    twice, with every check of the module docstring"""
    trans = entry in ("tn", "tnu", "tnw")
    A, B, C0, T, P, Eab, f, plain = _data(M, N, K)
    LA = G.Layout(K, M, lda or K, offA) if trans else G.Layout(M, K, lda or M, offA)
    LB = G.Layout(K, N, ldb or K, offB)
    LC = G.Layout(M, N, ldc or M, offC)
    fa, fb = LA.pack(A.T if trans else A, np.nan), LB.pack(B, np.nan)
    fc0 = LC.pack(C0 if beta != 0 else np.full((M, N), np.nan), G.SENTINEL)
    dA, dB = _dev(fa), _dev(fb)
    dT = ft = None
    if tm:
        # the contract of slab_reduce_kernel: column i of Tm is read in rows 0 .. i only (T^T(i, p) = T(p, i), p <= i), so what lies below
        # the diagonal -- like the rows beyond M of a padded Tm -- may hold anything: NaN here
        LT = G.Layout(M, M, ldt or M, 0)
        ft = LT.pack(np.triu(T) + np.tril(np.full((M, M), np.nan), -1), np.nan)
        dT = _dev(ft)
    if not trans:
        cap = 0                                     # (no slabs behind the NN entries)
    pad = LC.padding()
    fs0 = np.full(2 * G.GUARD + cap, np.nan)
    fs0[:G.GUARD] = fs0[G.GUARD + cap:] = G.SENTINEL
    what = f"{entry} {M} x {N} x {K} alpha {alpha} beta {beta} lda {LA.ld} ldb {LB.ld} ldc {LC.ld} off {offA}{offB}{offC}" + (" Tm" if tm else "")
    outs = []
    for rep in range(2):
        dC, dS = _dev(fc0), _dev(fs0)
        slabs = None if slabs_null else dS.data_ptr() + 8 * G.GUARD
        base = (stream, M, N, K, alpha, _ptr(dA, LA), LA.ld, _ptr(dB, LB), LB.ld, beta, _ptr(dC, LC), LC.ld)
        if entry == "nn":
            got_rc = q.lib.qrd_gemm_nn(*base)
        elif entry == "up":
            got_rc = q.lib.qrd_gemm_nn_update(*base)
        elif entry == "up2":
            got_rc = q.lib.qrd_gemm_nn_update2(*base)
        elif entry == "tn":
            got_rc = q.lib.qrd_gemm_tn(*base, slabs, 0 if slabs_null else cap, _ptr(dT, LT) if tm else None, LT.ld if tm else 0)
        elif entry == "tnu":
            got_rc = q.lib.qrd_gemm_tn_update(*base, slabs, 0 if slabs_null else cap)
        else:
            got_rc = q.lib.qrd_gemm_tn_update_wide(*base, slabs, 0 if slabs_null else cap)
        r = _route(q)
        q.check(q.lib.qrd_stream_sync(stream) if stream else q.lib.qrd_device_sync(), "sync")
        assert got_rc == rc, (what, got_rc)
        assert r["entry"] == {"nn": NN, "up": NN_UPDATE, "up2": NN_UPDATE}.get(entry, TN), (what, r)
        _check_route(r, route, what)
        fc, fs = _flat(dC), _flat(dS)
        if rc != 0:
            assert G.same_bits(fc, fc0), f"{what}: C was written"
            assert G.same_bits(fs, fs0), f"{what}: the slabs were written"
            continue
        assert G.same_bits(fc[pad], fc0[pad]), f"{what}: guard band or padding of C changed"
        assert G.same_bits(fs[:G.GUARD], fs0[:G.GUARD]) and G.same_bits(fs[G.GUARD + cap:], fs0[G.GUARD + cap:]), f"{what}: slab guards"
        if slabs_untouched:
            assert G.same_bits(fs, fs0), f"{what}: the slab buffer was written"
        outs.append(LC.unpack(fc))
    assert G.same_bits(_flat(dA), fa) and G.same_bits(_flat(dB), fb) and (not tm or G.same_bits(_flat(dT), ft)), f"{what}: an input changed"
    if not outs:
        return r
    ref, E = G.combine(P, Eab, alpha, beta, C0, np.triu(T) if tm else None)
    plain_result = None
    if plain is not None:
        plain_result = (np.triu(T).T @ (alpha * plain) if tm else alpha * plain) + (beta * C0 if beta != 0 else 0.0)
    _judge(entry, what, outs[0], ref, E, G.terms(M, K, tm), f, plain_result)
    assert G.same_bits(outs[0], outs[1]), f"{what}: two runs differ"
    return r


# ---- qrd_gemm_nn ----------------------------------------------------------------------------------------------------------------------
# nn_tile: 44 when M, N > 64 and ceil(M / 128) ceil(N / 128) >= 192; N <= 32: 41 from 12288 rows on, else 11; else 22 when
# ceil(M / 64) ceil(N / 64) >= 192, else 11.  launch_nn: the fast interior (M / BM) BM x (N / BN) BN needs 16-byte aligned A and B, even lda
# and ldb and K % 16 == 0; a ragged product below M N K = 4e8 takes one guarded launch instead of interior + strips.
AB_NN = [(1.0, 0.0), (-1.0, 1.0), (0.5, -2.0), (1.0, 1.0)]
_BLK = {44: (128, 128), 22: (64, 64), 11: (32, 32), 41: (128, 32)}


def _nn_cases():
    cases = []
    for t, (M, N, K) in G.NN_STRIPS.items():
        bm, bn = _BLK[t]
        assert M * N * K >= 4e8
        cases.append((f"tile{t}-interior+strips", M, N, K, {}, dict(tile=t, Mi=M // bm * bm, Ni=N // bn * bn, flags=(FAST, W8))))
    for t, (M, N) in G.NN_WHOLE.items():
        guarded = dict(tile=t, Mi=0, Ni=0, flags=(0, FAST))
        cases += [(f"tile{t}-whole", M, N, 16, {}, dict(tile=t, Mi=M, Ni=N, flags=(FAST, 0))),
                  (f"tile{t}-A-8-bytes-off", M, N, 16, dict(offA=1), guarded),
                  (f"tile{t}-B-8-bytes-off", M, N, 16, dict(offB=1), guarded),
                  (f"tile{t}-odd-lda", M, N, 16, dict(lda=M + 1), guarded),
                  (f"tile{t}-odd-ldb", M, N, 16, dict(ldb=17), guarded),
                  (f"tile{t}-K%16=5", M, N, 21, {}, guarded)]
    cases += [("tile44-ragged-below-4e8", 2050, 1538, 64, {}, dict(tile=44, Mi=0, Ni=0, flags=(0, FAST))),
              ("tile41-no-whole-column-tile", 12290, 30, 64, {}, dict(tile=41, Mi=0, Ni=0, flags=(0, FAST))),
              # ld > rows on A, B and C together (even lda, ldb: still the fast interior; odd ldc and C 8 bytes off: the epilogue is scalar)
              ("tile44-padded-A-B-C", 2050, 1538, 128, dict(lda=2056, ldb=130, ldc=2053, offC=1), dict(tile=44, Mi=2048, Ni=1536, flags=(FAST, 0))),
              ("tile11-padded-A-B-C-guarded", 200, 96, 48, dict(lda=260, ldb=50, ldc=333), dict(tile=11, Mi=0, Ni=0, flags=(0, FAST)))]
    return cases


@pytest.mark.parametrize("name,M,N,K,opts,route", _nn_cases(), ids=[c[0] for c in _nn_cases()])
def test_gemm_nn_routes(q, name, M, N, K, opts, route):
    for alpha, beta in AB_NN:
        _gemm(q, "nn", M, N, K, alpha, beta, route, **opts)


def test_gemm_nn_degenerate_calls(q):
    M, N, K = 64, 64, 16
    C0 = _data(M, N, K)[2]
    L = G.Layout(M, N, M)
    fnan, fc0 = L.pack(np.full((M, N), np.nan), np.nan), L.pack(C0, G.SENTINEL)
    dA, dB = _dev(fnan), _dev(fnan)
    for k, alpha, beta, rc in ((0, 1.0, 1.0, 0),        # K = 0: C = beta C, which beta == 1 makes a no-op ...
                               (0, 1.0, 0.0, -1),       # ... and anything else is refused: there is no scaling kernel behind this entry
                               (K, 0.0, 1.0, 0)):       # alpha == 0, beta == 1: C stays as it is, whatever the operands hold (NaN: 0 * NaN)
        dC = _dev(fc0)
        assert q.lib.qrd_gemm_nn(None, M, N, k, alpha, _ptr(dA, L), M, _ptr(dB, L), M, beta, _ptr(dC, L), M) == rc
        r = _route(q)
        q.check(q.lib.qrd_device_sync(), "sync")
        assert r["entry"] == NN and r["tile"] == 0 and r["flags"] == 0, r
        assert G.same_bits(_flat(dC), fc0), (k, alpha, beta)


# ---- qrd_gemm_nn_update / qrd_gemm_nn_update2 ---------------------------------------------------------------------------------------------
# gemm_nn_update_impl: gemm_nn_w8_kernel<0 / 1> on the 128 x 128 interior and guarded 128 x 128 launches on the right and bottom strips when
# beta == 1, alpha == +-1, A and B 16-byte aligned with even lda, ldb, K % 16 == 0, M >= 128 and N >= 128; anything else: launch_nn<4, 4>.
_UP_W8 = dict(tile=44, flags=(FAST | W8, 0))
_UP_GUARDED = dict(tile=44, Mi=0, Ni=0, flags=(0, FAST | W8))
UP_CASES = [("whole", 256, 256, 64, -1.0, 1.0, {}, dict(_UP_W8, Mi=256, Ni=256)),
            ("whole+", 256, 256, 64, 1.0, 1.0, {}, dict(_UP_W8, Mi=256, Ni=256)),
            ("w8-interior+strips", 386, 258, 32, -1.0, 1.0, {}, dict(_UP_W8, Mi=384, Ni=256)),
            ("w8-interior+strips+", 386, 258, 32, 1.0, 1.0, {}, dict(_UP_W8, Mi=384, Ni=256)),
            ("w8-odd-ldc-C-8-bytes-off", 386, 258, 32, -1.0, 1.0, dict(ldc=389, offC=1, lda=392, ldb=34), dict(_UP_W8, Mi=384, Ni=256)),
            # gemm_nn_w8_kernel<1> (qrd_gemm_nn_update2) renumbers its workgroups over the XCDs when the grid has a multiple of 8 row tiles and at
            # most 8 column tiles; <0> never does: the same cases through both
            ("w8-8-row-tiles", 1024, 256, 32, -1.0, 1.0, {}, dict(_UP_W8, Mi=1024, Ni=256)),
            ("w8-8-row-tiles+strips", 1026, 258, 32, 1.0, 1.0, {}, dict(_UP_W8, Mi=1024, Ni=256)),
            ("fallback-beta-0", 256, 256, 64, -1.0, 0.0, {}, dict(tile=44, Mi=256, Ni=256, flags=(FAST, W8))),
            ("fallback-alpha-0.5", 256, 256, 64, 0.5, 1.0, {}, dict(tile=44, Mi=256, Ni=256, flags=(FAST, W8))),
            ("fallback-K-40", 256, 256, 40, -1.0, 1.0, {}, _UP_GUARDED),
            ("fallback-A-8-bytes-off", 256, 256, 64, -1.0, 1.0, dict(offA=1), _UP_GUARDED),
            ("fallback-B-8-bytes-off", 256, 256, 64, 1.0, 1.0, dict(offB=1), _UP_GUARDED),
            ("fallback-M-127", 127, 256, 32, -1.0, 1.0, {}, _UP_GUARDED),
            ("fallback-N-100", 256, 100, 32, 1.0, 1.0, {}, _UP_GUARDED)]


@pytest.mark.parametrize("entry", ["up", "up2"])
@pytest.mark.parametrize("name,M,N,K,alpha,beta,opts,route", UP_CASES, ids=[c[0] for c in UP_CASES])
def test_gemm_nn_update_routes(q, entry, name, M, N, K, alpha, beta, opts, route):
    _gemm(q, entry, M, N, K, alpha, beta, route, **opts)


def test_gemm_nn_update_one_tile_and_empty(q):
    """one 128 x 128 tile with one k-tile; K = 0 (a panel of no columns): nothing to subtract, nothing launched, C untouched"""
    for entry in ("up", "up2"):
        _gemm(q, entry, 128, 128, 16, -1.0, 1.0, dict(tile=44, Mi=128, Ni=128, flags=(FAST | W8, 0)))
    M = N = 128
    L = G.Layout(M, N, M)
    fc0 = L.pack(_data(128, 128, 16)[2], G.SENTINEL)
    dC, dA = _dev(fc0), _dev(L.pack(np.full((M, N), np.nan), np.nan))
    assert q.lib.qrd_gemm_nn_update(None, M, N, 0, -1.0, _ptr(dA, L), M, _ptr(dA, L), M, 1.0, _ptr(dC, L), M) == 0
    r = _route(q)
    q.check(q.lib.qrd_device_sync(), "sync")
    assert r["entry"] == NN_UPDATE and r["tile"] == 0 and G.same_bits(_flat(dC), fc0)


# ---- qrd_gemm_tn / qrd_gemm_tn_update ---------------------------------------------------------------------------------------------------
# gemm_tn_impl: M <= 32: tile 14 when N is a multiple of 128, else 11; short K (K <= 512, no Tm) on at most 1024 tiles of 32 x 32: 11;
# M <= 64 or N <= 64: 22; else 44.  launch_tn: interior + strips as launch_nn without a size threshold, but 44 ragged = one MIXED launch.
# K split: at most K / 128 slices (256 at most, and slab_cap / (M N)), none for short K, chosen by a cost model over the stream's CUs.
_GUARDED = (0, FAST | MIXED)


def _tn_cases():
    c = []

    def add(name, M, N, K, route, ab=(1.0, 0.0), **opts):
        c.append((name, M, N, K, ab, opts, route))
    # <1, 4>: the leaf products W = V_leaf^T A2
    add("14-whole", 32, 256, 4096, dict(tile=14, Mi=32, Ni=256, flags=(FAST, MIXED | DIRECT | TM), ksplit=lambda k: k > 1, piece=256))
    # (one row of tiles, 2 .. 8 column tiles and 8 or more K slices: gemm_tn_kernel regroups the slices below the last multiple of 8 over the
    # XCDs and leaves the rest as launched -- 12 slices = 8 regrouped + 4 not)
    add("14-12-slices", 32, 256, 4096, dict(tile=14, Mi=32, Ni=256, ksplit=12, piece=256, flags=(FAST, DIRECT)), cap=12 * 32 * 256)
    add("14-M-24-guarded", 24, 256, 2048, dict(tile=14, Mi=0, Ni=0, flags=_GUARDED))
    add("14-K%16=4-guarded", 32, 256, 4100, dict(tile=14, Mi=0, Ni=0, flags=_GUARDED))
    add("14-padded", 32, 256, 4096, dict(tile=14, Mi=32, Ni=256, flags=(FAST, MIXED)), lda=4102, ldb=4098, ldc=35, offC=1)
    add("14-A-8-bytes-off", 32, 256, 4096, dict(tile=14, Mi=0, Ni=0, flags=_GUARDED), offA=1)
    add("14-B-8-bytes-off", 32, 256, 4096, dict(tile=14, Mi=0, Ni=0, flags=_GUARDED), offB=1)
    # <2, 2>
    add("22-interior+right-strip", 64, 200, 2048, dict(tile=22, Mi=64, Ni=192, flags=(FAST, MIXED)))
    add("22-interior+bottom-strip", 130, 64, 2048, dict(tile=22, Mi=128, Ni=64, flags=(FAST, MIXED)))
    add("22-guarded", 130, 60, 2048, dict(tile=22, Mi=0, Ni=0, flags=_GUARDED))
    add("22-padded", 64, 200, 2048, dict(tile=22, Mi=64, Ni=192, flags=(FAST, MIXED)), lda=2054, ldb=2050, ldc=67, offC=1)
    add("22-A-8-bytes-off", 64, 200, 2048, dict(tile=22, Mi=0, Ni=0, flags=_GUARDED), offA=1)
    add("22-odd-ldb", 64, 200, 2048, dict(tile=22, Mi=0, Ni=0, flags=_GUARDED), ldb=2049)
    # <1, 1>, short K: unsplit, C written by the product kernel itself
    add("11-short-K-right-strip", 96, 80, 496, dict(tile=11, Mi=96, Ni=64, ksplit=1, piece=0, flags=(FAST | DIRECT, MIXED)), ab=(2.0, -1.0))
    add("11-short-K-both-strips", 100, 70, 512, dict(tile=11, Mi=96, Ni=64, ksplit=1, piece=0, flags=(FAST | DIRECT, MIXED)))
    add("11-padded", 100, 70, 512, dict(tile=11, Mi=96, Ni=64, ksplit=1, flags=(FAST | DIRECT, MIXED)), ab=(-1.0, 1.0), lda=518, ldb=514, ldc=103,
        offC=1)
    add("11-B-8-bytes-off", 100, 70, 512, dict(tile=11, Mi=0, Ni=0, ksplit=1, flags=(DIRECT, FAST)), ab=(2.0, -1.0), offB=1)
    add("11-odd-lda", 100, 70, 512, dict(tile=11, Mi=0, Ni=0, ksplit=1, flags=(DIRECT, FAST)), lda=513)
    # <4, 4>
    add("44-whole", 128, 128, 2048, dict(tile=44, Mi=128, Ni=128, flags=(FAST, MIXED | EVEN | WIDE)))
    add("44-one-row-of-tiles", 128, 256, 4096, dict(tile=44, Mi=128, Ni=256, ksplit=lambda k: k >= 8, flags=(FAST, MIXED | EVEN | WIDE | DIRECT)))
    add("44-one-row-of-tiles-12-slices", 128, 256, 4096, dict(tile=44, Mi=128, Ni=256, ksplit=12, flags=(FAST, MIXED | EVEN | DIRECT)), ab=(2.0, -1.0),
        cap=12 * 128 * 256)
    add("44-ragged-MIXED", 130, 131, 4096, dict(tile=44, Mi=130, Ni=131, flags=(FAST | MIXED, EVEN | WIDE)))
    add("44-ragged-MIXED-padded", 130, 131, 4096, dict(tile=44, Mi=130, Ni=131, flags=(FAST | MIXED, EVEN)), ab=(-1.0, 1.0), lda=4100, ldb=4098,
        ldc=133, offC=1)
    add("44-A-8-bytes-off", 128, 128, 2048, dict(tile=44, Mi=0, Ni=0, flags=_GUARDED), offA=1)
    add("44-ragged-odd-lda", 130, 131, 4096, dict(tile=44, Mi=0, Ni=0, flags=_GUARDED), lda=4097)
    return c


@pytest.mark.parametrize("entry", ["tn", "tnu"])
@pytest.mark.parametrize("name,M,N,K,ab,opts,route", _tn_cases(), ids=[c[0] for c in _tn_cases()])
def test_gemm_tn_routes(q, entry, name, M, N, K, ab, opts, route):
    _gemm(q, entry, M, N, K, ab[0], ab[1], route, **opts)


AB_TN = [(1.0, 0.0), (-1.0, 1.0), (2.0, -1.0)]


@pytest.mark.parametrize("entry", ["tn", "tnu"])
@pytest.mark.parametrize("alpha,beta", AB_TN)
@pytest.mark.parametrize("M,N,K,tile,ksplit", [
    (128, 128, 8192, 44, lambda k: k > 1),                 # the slabs are summed in row pieces of 256 ...
    (64, 32, 8192, 22, lambda k: 32 <= k < 128),           # ... of 64 from 32 slabs on (M >= 64, no Tm) ...
    (64, 32, 65536, 22, lambda k: k >= 128),               # ... of 32 from 128 on  (32 columns on 64-column tiles: the guarded kernel)
], ids=["split", "piece-64", "piece-32"])
def test_gemm_tn_split_k_with_alpha_and_beta(q, entry, alpha, beta, M, N, K, tile, ksplit):
    """alpha is applied by the product kernel to every slab, beta by slab_reduce_kernel to C: the beta path of the reduction.  The number of
    slabs follows the stream's compute units (asserted as a range); the row piece follows the number of slabs."""
    whole = N >= 64
    r = _gemm(q, entry, M, N, K, alpha, beta, dict(tile=tile, Mi=M if whole else 0, Ni=N if whole else 0, ksplit=ksplit,
                                                   flags=(FAST if whole else 0, DIRECT | MIXED | EVEN | (0 if whole else FAST))))
    assert r["piece"] == (32 if r["ksplit"] >= 128 else 64 if r["ksplit"] >= 32 else 256), r


@pytest.mark.parametrize("entry", ["tn", "tnu"])
def test_gemm_tn_slab_capacity(q, entry):
    """slab_cap < M N: no split, C written directly, the slab buffer untouched; otherwise at most slab_cap / (M N) slices (and nothing behind
    them written: the buffer ends there, in front of its guard band)"""
    M, N, K = 128, 128, 8192
    whole = dict(tile=44, Mi=M, Ni=N)
    for alpha, beta in ((1.0, 0.0), (2.0, -1.0)):
        _gemm(q, entry, M, N, K, alpha, beta, dict(whole, ksplit=lambda k: 1 < k <= 3, piece=256, flags=(FAST, DIRECT)), cap=3 * M * N)
        _gemm(q, entry, M, N, K, alpha, beta, dict(whole, ksplit=2, piece=256, flags=(FAST, DIRECT)), cap=3 * M * N - 1)
        _gemm(q, entry, M, N, K, alpha, beta, dict(whole, ksplit=1, piece=0, flags=(FAST | DIRECT, 0)), cap=M * N - 1, slabs_untouched=True)
        _gemm(q, entry, M, N, K, alpha, beta, dict(whole, ksplit=1, piece=0, flags=(FAST | DIRECT, 0)), slabs_null=True, slabs_untouched=True)


def test_gemm_tn_split_follows_the_compute_units_of_the_stream(q):
    """256 x 256 x 8192, four tiles: the K split is chosen for one round of workgroups on two slots per compute unit OF THE STREAM -- fewer
    slices on a CU-masked stream of 32 than on the whole device, and as right"""
    M, N, K = 256, 256, 8192
    whole = dict(tile=44, Mi=M, Ni=N, flags=(FAST, DIRECT | EVEN))
    cap = 64 * M * N                    # room for the K / 128 slices the rule allows at most
    full = _gemm(q, "tn", M, N, K, 1.0, 0.0, dict(whole, ksplit=lambda k: k > 1), cap=cap)
    st = C.c_void_p()
    q.check(q.lib.qrd_stream_create_cumask(C.byref(st), 0, 32))
    try:
        assert q.lib.qrd_stream_cus(st) == 32 < q.lib.qrd_stream_cus(None)
        masked = _gemm(q, "tn", M, N, K, 1.0, 0.0, dict(whole, ksplit=lambda k: 1 < k <= 16), cap=cap, stream=st)      # 64 slots / 4 tiles
    finally:
        q.check(q.lib.qrd_stream_destroy(st))
    assert masked["ksplit"] < full["ksplit"], (masked, full)


# the wide product's own tile (gemm_tn_wide_kernel, 128 x 256) behind qrd_gemm_tn_update_wide: 44, alpha 1, beta 0, N a multiple of 256, M >= 128,
# K % 16 == 0, aligned operands and slabs; rows beyond the last multiple of 128 on the guarded 128 x 128 kernel; anything else as qrd_gemm_tn_update
WIDE_CASES = [("whole", 256, 256, 2048, (1.0, 0.0), {}, dict(tile=44, Mi=256, Ni=256, flags=(FAST | WIDE, EVEN | MIXED))),
              ("bottom-strip", 130, 256, 2048, (1.0, 0.0), {}, dict(tile=44, Mi=128, Ni=256, flags=(FAST | WIDE, EVEN | MIXED))),
              ("padded", 256, 256, 2048, (1.0, 0.0), dict(lda=2054, ldb=2050, ldc=259, offC=1), dict(tile=44, Mi=256, Ni=256, flags=(FAST | WIDE, EVEN))),
              ("beta-1-not-wide", 256, 256, 2048, (-1.0, 1.0), {}, dict(tile=44, Mi=256, Ni=256, flags=(FAST, WIDE | EVEN))),
              ("A-8-bytes-off-not-wide", 256, 256, 2048, (1.0, 0.0), dict(offA=1), dict(tile=44, Mi=0, Ni=0, flags=(0, FAST | WIDE | EVEN))),
              ("no-slabs-not-wide", 256, 256, 2048, (1.0, 0.0), dict(slabs_null=True, slabs_untouched=True),
               dict(tile=44, Mi=256, Ni=256, ksplit=1, flags=(FAST | DIRECT, WIDE | EVEN)))]


@pytest.mark.parametrize("name,M,N,K,ab,opts,route", WIDE_CASES, ids=[c[0] for c in WIDE_CASES])
def test_gemm_tn_wide_routes(q, name, M, N, K, ab, opts, route):
    _gemm(q, "tnw", M, N, K, ab[0], ab[1], route, **opts)


TM_CASES = [("M-32-many-slices", 32, 96, 4096, 11, lambda k: k > 1, {}),
            ("M-32-one-slice", 32, 96, 64, 11, 1, {}),
            ("M-100-many-slices", 100, 40, 2048, 22, lambda k: k > 1, dict(ldt=104)),
            ("M-256-many-slices", 256, 64, 1024, 22, lambda k: k > 1, dict(ldt=259, ldc=258, lda=1030, ldb=1026))]


@pytest.mark.parametrize("beta", [0.0, 1.0])
@pytest.mark.parametrize("name,M,N,K,tile,ksplit,opts", TM_CASES, ids=[c[0] for c in TM_CASES])
def test_gemm_tn_with_Tm(q, name, M, N, K, tile, ksplit, opts, beta):
    """C = beta C + Tm^T (A^T B): the product always goes through the slabs (one slab when K is a single slice) and the reduction folds Tm in,
    reading its upper triangle only (NaN below the diagonal and in the rows beyond M of a padded Tm)"""
    _gemm(q, "tn", M, N, K, 1.0, beta, dict(tile=tile, ksplit=ksplit, piece=256, flags=(TM, DIRECT)), tm=True, **opts)


def test_gemm_tn_return_codes(q):
    """-2: Tm with more than 256 rows (the reduction holds one column in one workgroup); -3: Tm without slab space.  Nothing is written."""
    quiet = dict(tile=0, Mi=0, Ni=0, ksplit=0, piece=0, flags=(0, 255))
    M, N, K = 257, 33, 64
    rng = np.random.default_rng(1)
    LA, LB, LC, LT = G.Layout(K, M, K), G.Layout(K, N, K), G.Layout(M, N, M), G.Layout(M, M, M)
    fc0 = LC.pack(rng.standard_normal((M, N)), G.SENTINEL)
    dA, dB, dT, dC = _dev(LA.pack(rng.standard_normal((K, M)), np.nan)), _dev(LB.pack(rng.standard_normal((K, N)), np.nan)), \
        _dev(LT.pack(np.triu(rng.standard_normal((M, M))), np.nan)), _dev(fc0)
    dS = _dev(np.full(CAP, np.nan))
    assert q.lib.qrd_gemm_tn(None, M, N, K, 1.0, _ptr(dA, LA), K, _ptr(dB, LB), K, 1.0, _ptr(dC, LC), M, dS.data_ptr(), CAP, _ptr(dT, LT), M) == -2
    r = _route(q)
    _check_route(r, quiet, "-2")
    q.check(q.lib.qrd_device_sync(), "sync")
    assert r["entry"] == TN and G.same_bits(_flat(dC), fc0) and np.isnan(_flat(dS)).all()
    _gemm(q, "tn", 32, 96, 64, 1.0, 1.0, quiet, tm=True, slabs_null=True, rc=-3)
    _gemm(q, "tn", 100, 40, 2048, 1.0, 0.0, quiet, tm=True, cap=100 * 40 - 1, rc=-3)


@pytest.mark.parametrize("alpha,beta", [(-1.0, 1.0), (2.0, -1.0)])
@pytest.mark.parametrize("entry", ["tn", "tnu"])
def test_gemm_tn_k_remainder_split_accumulates_behind_beta(q, entry, alpha, beta):
    """K % 16 != 0 from 4 GFLOP on (aligned operands, no Tm): the whole k-tiles with the caller's beta, then the last K % 16 rows as a guarded
    product accumulated with beta = 1.  The record is the first part's, flagged.  512 x 1024 x 8200, float64 reference: at (-1, 1), and at
    (2, -1), where a second half that applied the caller's beta again would show (at beta = 1 it would not)."""
    M, N, K = 512, 1024, 8200
    assert K % 16 == 8 and M * N * K >= 4e9
    _gemm(q, entry, M, N, K, alpha, beta, dict(tile=44, Mi=M, Ni=N, ksplit=lambda k: k > 1, piece=256, flags=(FAST | KREM, DIRECT | EVEN)), cap=16 * M * N)


# ---- qrd_gemm_nn_batch ------------------------------------------------------------------------------------------------------------------
# fast when A and B are 16-byte aligned with even lda, ldb, sA, sB, K % 16 == 0 and M, N multiples of 32; else the guarded instantiation
BATCH_CASES = [("fast", 32, 32, 32, 5, {}, True),
               ("fast-one-A-for-all", 32, 32, 32, 5, dict(sA=0), True),
               ("fast-one-B-for-all", 32, 32, 32, 5, dict(sB=0), True),
               ("odd-stride-of-A", 32, 32, 32, 5, dict(sA=32 * 32 + 1), False),
               ("odd-stride-of-B", 32, 32, 32, 5, dict(sB=32 * 34 + 3, ldb=34), False),
               ("ragged", 20, 40, 24, 5, {}, False),
               ("padded-C", 32, 32, 32, 5, dict(ldc=37, sC=37 * 32 + 5, lda=34, ldb=36), True),
               ("empty-batch", 32, 32, 32, 0, {}, None)]


@pytest.mark.parametrize("alpha,beta", [(1.0, 0.0), (-1.0, 1.0), (0.5, -2.0)])
@pytest.mark.parametrize("name,M,N,K,batch,opts,fast", BATCH_CASES, ids=[c[0] for c in BATCH_CASES])
def test_gemm_nn_batch_routes(q, name, M, N, K, batch, opts, fast, alpha, beta):
    nb = max(batch, 1)
    rng = np.random.default_rng(97 * M + 89 * N + K)
    lda, ldb, ldc = opts.get("lda", M), opts.get("ldb", K), opts.get("ldc", M)
    sA, sB, sC = opts.get("sA", lda * K), opts.get("sB", ldb * N), opts.get("sC", ldc * N)
    A, B, C0 = rng.standard_normal((1 if sA == 0 else nb, M, K)), rng.standard_normal((1 if sB == 0 else nb, K, N)), rng.standard_normal((nb, M, N))
    LA, LB, LC = G.Layout(M, K, lda, 0, A.shape[0], sA or None), G.Layout(K, N, ldb, 0, B.shape[0], sB or None), G.Layout(M, N, ldc, 0, nb, sC)
    fa, fb = LA.pack(A, np.nan), LB.pack(B, np.nan)
    fc0 = LC.pack(C0 if beta != 0 else np.full((nb, M, N), np.nan), G.SENTINEL)
    dA, dB = _dev(fa), _dev(fb)
    outs = []
    for rep in range(2):
        dC = _dev(fc0)
        q.check(q.lib.qrd_gemm_nn_batch(None, M, N, K, alpha, _ptr(dA, LA), lda, sA, _ptr(dB, LB), ldb, sB, beta, _ptr(dC, LC), ldc, sC, batch))
        r = _route(q)
        q.check(q.lib.qrd_device_sync(), "sync")
        assert r["entry"] == NN_BATCH, r
        fc = _flat(dC)
        if batch == 0:
            assert r["tile"] == 0 and r["flags"] == 0 and G.same_bits(fc, fc0)
            continue
        _check_route(r, dict(tile=11, Mi=M if fast else 0, Ni=N if fast else 0, flags=(FAST, 0) if fast else (0, FAST)), name)
        pad = LC.padding()
        assert G.same_bits(fc[pad], fc0[pad]), "guard band or padding of C changed"
        outs.append(LC.unpack(fc).reshape(nb, M, N))
    assert G.same_bits(_flat(dA), fa) and G.same_bits(_flat(dB), fb), "an input changed"
    if batch == 0:
        return
    for z in range(batch):
        Az, Bz = A[0 if sA == 0 else z], B[0 if sB == 0 else z]
        ref, E, f = G.reference(Az, Bz, alpha, beta, C0[z])
        _judge("nn_batch", f"batch {name} member {z} alpha {alpha} beta {beta}", outs[0][z], ref, E, G.terms(M, K), f, alpha * (Az @ Bz) + beta * C0[z])
    assert G.same_bits(outs[0], outs[1]), "two runs differ"


# ---- qrd_slab_reduce ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nslab", [1, 5])
@pytest.mark.parametrize("M,lds,stride_extra,ldo", [(1, 1, 0, 1), (256, 256, 0, 256), (257, 257, 0, 257), (300, 300, 0, 300),
                                                    (300, 307, 0, 300), (300, 300, 11, 300), (257, 260, 5, 263), (1, 3, 2, 4)])
def test_slab_reduce(q, M, lds, stride_extra, ldo, nslab):
    """out = the sum of nslab slabs, in row pieces of 256 (one workgroup per column and piece): EXACTLY the fixed-order float64 sum of
    gemm_ref.slab_sum, whatever lds, the slab stride and ldo"""
    N = 7
    rng = np.random.default_rng(M + 31 * nslab + lds)
    S = rng.standard_normal((nslab, M, N)) * 10.0 ** rng.integers(-3, 4, (nslab, M, N))      # magnitudes apart: the order of the sum shows
    stride = lds * N + stride_extra
    LS, LO = G.Layout(M, N, lds, 0, nslab, stride), G.Layout(M, N, ldo)
    fs, fo0 = LS.pack(S, np.nan), LO.pack(np.full((M, N), np.nan), G.SENTINEL)
    dS = _dev(fs)
    want = G.slab_sum(S)
    for rep in range(2):
        dO = _dev(fo0)
        q.check(q.lib.qrd_slab_reduce(None, M, N, nslab, _ptr(dS, LS), lds, stride, _ptr(dO, LO), ldo))
        r = _route(q)
        q.check(q.lib.qrd_device_sync(), "sync")
        _check_route(r, dict(entry=SLAB_REDUCE, ksplit=nslab, piece=256, tile=0), "slab_reduce")
        fo = _flat(dO)
        pad = LO.padding()
        assert G.same_bits(fo[pad], fo0[pad]), "guard band or padding of the output changed"
        assert G.same_bits(LO.unpack(fo), want)
    assert G.same_bits(_flat(dS), fs)


def test_zz_worst_ratios():
    """prints what the cases above measured, per entry (for DESIGN.md's table; asserts nothing new)"""
    for entry, (r, vs) in sorted(WORST.items()):
        print(f"worst of {entry}: |err| / bound {r:.2e}, kernel error / numpy error {vs:.2f}")
        assert r <= 1.0
