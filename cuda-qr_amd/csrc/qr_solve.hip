// qr_solve.hip -- kernels of the least-squares solve (qr_solve.c): the block reflector of one outer panel applied to a few
// right-hand sides, and the blocked back substitution with R.
//
//   ormqr_vtc_kernel    P_b = V_b^T C_b           partial sums per row block b, V read in place from the factored matrix
//   ormqr_tw_kernel     W = op(T) sum_b P_b       the partials summed in block order (no atomics: repeated solves are bitwise equal)
//   ormqr_cvw_kernel    C -= V W
//   trsm_step_kernel    rows above a solved 64-row block updated with it, and the next 64-row diagonal block solved by substitution
//
// Memory-bound work with few columns: the products run on the VALU (an MFMA tile would be 15/16 padding at one right-hand side).
// V = the unit lower trapezoid of a panel of the factored matrix: zeros above the diagonal, ones on it, dA below it.
#include "qr_common.h"
#include "qr_device.h"

#define SV_TR 16          // rows of V per LDS tile (ormqr_vtc_kernel)
#define SV_CW 256         // columns of V per pass (one per thread)
#define TRSM_L 64         // rows of a diagonal block of the back substitution

__device__ __forceinline__ double v_at(const double* __restrict__ Ak, int lda, int mk, int r, int c)
{
    if (r >= mk || r < c) return 0.0;
    return r == c ? 1.0 : Ak[(size_t) c * lda + r];
}

// P[(b * nrhs + j) * w + c] = sum over the rows r of block b of V[r, c] C[r, j], for the NC columns j0 .. of blockIdx.y
template <int NC>
__global__ void __launch_bounds__(256) ormqr_vtc_kernel(const double* __restrict__ Ak, int lda, int mk, int w, const double* __restrict__ Cs,
                                                        int ldc, int nrhs, int rpb, double* __restrict__ P)
{
    __shared__ double Vs[SV_CW * (SV_TR + 1)];
    __shared__ double Cl[SV_TR * NC];
    const int t = threadIdx.x, b = blockIdx.x, j0 = blockIdx.y * NC;
    const int nc = min(NC, nrhs - j0);
    const int r_beg = b * rpb, r_end = min(mk, r_beg + rpb);
    for (int cc = 0; cc < w; cc += SV_CW) {
        double acc[NC];
#pragma unroll
        for (int j = 0; j < NC; ++j) acc[j] = 0.0;
        for (int r0 = r_beg; r0 < r_end; r0 += SV_TR) {
            {
                const int rr = t & (SV_TR - 1), cg = t / SV_TR;
#pragma unroll
                for (int i = 0; i < SV_CW / (256 / SV_TR); ++i) {
                    const int c = cg + i * (256 / SV_TR);
                    Vs[c * (SV_TR + 1) + rr] = (cc + c < w) ? v_at(Ak, lda, mk, r0 + rr, cc + c) : 0.0;
                }
            }
            if (t < SV_TR * NC) {
                const int rr = t % SV_TR, j = t / SV_TR, r = r0 + rr;
                Cl[rr * NC + j] = (r < r_end && j < nc) ? Cs[(size_t) (j0 + j) * ldc + r] : 0.0;
            }
            __syncthreads();
#pragma unroll
            for (int rr = 0; rr < SV_TR; ++rr) {
                const double v = Vs[t * (SV_TR + 1) + rr];
#pragma unroll
                for (int j = 0; j < NC; ++j) acc[j] = fma(v, Cl[rr * NC + j], acc[j]);
            }
            __syncthreads();
        }
        const int c = cc + t;
        if (c < w)
            for (int j = 0; j < nc; ++j) P[((size_t) b * nrhs + j0 + j) * w + c] = acc[j];
    }
}

// Wt (w x nrhs, ld w), column j = blockIdx.x: op(T) sum_b P_b[:, j] with op(T) = T^T (trans_t) or T; T upper triangular (ldt)
__global__ void __launch_bounds__(256) ormqr_tw_kernel(const double* __restrict__ P, int nblk, int nrhs, int w, const double* __restrict__ T,
                                                       int ldt, int trans_t, double* __restrict__ Wt)
{
    __shared__ double W0[QRD_SOLVE_MAX_W];
    const int j = blockIdx.x;
    for (int c = threadIdx.x; c < w; c += blockDim.x) {
        double s = 0.0;
        for (int b = 0; b < nblk; ++b) s += P[((size_t) b * nrhs + j) * w + c];
        W0[c] = s;
    }
    __syncthreads();
    for (int c = threadIdx.x; c < w; c += blockDim.x) {
        double s = 0.0;
        if (trans_t) {
#pragma unroll 16
            for (int k = 0; k <= c; ++k) s = fma(T[(size_t) c * ldt + k], W0[k], s);     // (T^T)[c, k] = T[k, c], k <= c
        } else {
#pragma unroll 16
            for (int k = c; k < w; ++k) s = fma(T[(size_t) k * ldt + c], W0[k], s);      // T[c, k], k >= c
        }
        Wt[(size_t) j * w + c] = s;
    }
}

// C[r, j] -= sum_c V[r, c] Wt[c, j]: 64 rows per workgroup, the w columns split over its four waves, their sums added in wave order
template <int NC>
__global__ void __launch_bounds__(256) ormqr_cvw_kernel(const double* __restrict__ Ak, int lda, int mk, int w, const double* __restrict__ Wt,
                                                        double* __restrict__ Cs, int ldc, int nrhs)
{
    extern __shared__ double sm[];
    double* Wl = sm;                       // w x NC
    double* red = sm + (size_t) w * NC;    // 3 waves x 64 rows x NC
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6, j0 = blockIdx.y * NC;
    const int nc = min(NC, nrhs - j0);
    for (int i = t; i < w * NC; i += 256) {
        const int c = i / NC, j = i - c * NC;
        Wl[i] = j < nc ? Wt[(size_t) (j0 + j) * w + c] : 0.0;
    }
    __syncthreads();
    const int r = blockIdx.x * 64 + lane;
    const int cw = (w + 3) / 4, c_beg = wv * cw, c_end = min(w, c_beg + cw);
    double acc[NC];
#pragma unroll
    for (int j = 0; j < NC; ++j) acc[j] = 0.0;
    if (r < mk) {
        const int c_top = min(c_end, r);   // columns c < r read dA; c == r is the unit diagonal; c > r are zeros
        int c = c_beg;
        for (; c + 16 <= c_top; c += 16) {       // 16 loads in flight per lane
            double v[16];
#pragma unroll
            for (int u = 0; u < 16; ++u) v[u] = Ak[(size_t) (c + u) * lda + r];
#pragma unroll
            for (int u = 0; u < 16; ++u)
#pragma unroll
                for (int j = 0; j < NC; ++j) acc[j] = fma(v[u], Wl[(c + u) * NC + j], acc[j]);
        }
        for (; c < c_top; ++c) {
            const double v = Ak[(size_t) c * lda + r];
#pragma unroll
            for (int j = 0; j < NC; ++j) acc[j] = fma(v, Wl[c * NC + j], acc[j]);
        }
        if (r >= c_beg && r < c_end)
#pragma unroll
            for (int j = 0; j < NC; ++j) acc[j] += Wl[r * NC + j];
    }
    if (wv > 0)
#pragma unroll
        for (int j = 0; j < NC; ++j) red[((wv - 1) * 64 + lane) * NC + j] = acc[j];
    __syncthreads();
    if (wv == 0 && r < mk) {
        for (int j = 0; j < nc; ++j) {
            const double s = ((acc[j] + red[(0 * 64 + lane) * NC + j]) + red[(1 * 64 + lane) * NC + j]) + red[(2 * 64 + lane) * NC + j];
            double* cp = Cs + (size_t) (j0 + j) * ldc + r;
            *cp -= s;
        }
    }
}

// One step of the blocked back substitution R X = B (R upper triangular, lda; B ldb; the NC right-hand sides j0 .. of blockIdx.y):
//   rows [row_lo, l1) -= R[rows, x0:x1] B[x0:x1]          (x0 == x1: no update; B[x0:x1] is a block solved by an earlier launch)
//   then block 0 (rows [l0, l1), at most 64) solves R[l0:l1, l0:l1] X = B[l0:l1] by substitution, 16 rows at a time.
// Workgroup 0 owns rows [l0, l1), workgroup b >= 1 the 64 rows [l0 - 64 b, l0 - 64 (b - 1)) clipped to row_lo; the four waves
// split the update's K and their sums are added in wave order.
template <int NC>
__global__ void __launch_bounds__(256) trsm_step_kernel(const double* __restrict__ R, int lda, double* __restrict__ B, int ldb, int nrhs,
                                                        int row_lo, int l0, int l1, int x0, int x1)
{
    // Xs and red serve the update; the leaf's diagonal block Rl (64 x 64) takes their place for the substitution
    constexpr int SM = (TRSM_L * NC + 3 * 64 * NC) > TRSM_L * TRSM_L ? (TRSM_L * NC + 3 * 64 * NC) : TRSM_L * TRSM_L;
    __shared__ double smem[SM];
    __shared__ double Bl[TRSM_L * NC];
    double* Xs = smem;
    double* red = smem + TRSM_L * NC;
    double* Rl = smem;
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6, blk = blockIdx.x, j0 = blockIdx.y * NC;
    const int nc = min(NC, nrhs - j0);
    const int rb = blk == 0 ? l0 : max(row_lo, l0 - 64 * blk);
    const int re = blk == 0 ? l1 : l0 - 64 * (blk - 1);
    const int r = rb + lane;
    const int kx = x1 - x0;
    double acc[NC];
#pragma unroll
    for (int j = 0; j < NC; ++j) acc[j] = 0.0;
    if (kx > 0) {
        for (int i = t; i < kx * NC; i += 256) {
            const int k = i / NC, j = i - k * NC;
            Xs[i] = j < nc ? B[(size_t) (j0 + j) * ldb + x0 + k] : 0.0;
        }
        __syncthreads();
        const int kq = (kx + 3) / 4, k_beg = wv * kq, k_end = min(kx, k_beg + kq);
        if (r < re) {
            double a[TRSM_L / 4];                 // all of this wave's loads in flight at once
#pragma unroll
            for (int u = 0; u < TRSM_L / 4; ++u) a[u] = (k_beg + u < k_end) ? R[(size_t) (x0 + k_beg + u) * lda + r] : 0.0;
#pragma unroll
            for (int u = 0; u < TRSM_L / 4; ++u)
                if (k_beg + u < k_end)
#pragma unroll
                    for (int j = 0; j < NC; ++j) acc[j] = fma(a[u], Xs[(k_beg + u) * NC + j], acc[j]);
        }
        if (wv > 0)
#pragma unroll
            for (int j = 0; j < NC; ++j) red[((wv - 1) * 64 + lane) * NC + j] = acc[j];
        __syncthreads();
    }
    if (wv == 0 && r < re) {
        for (int j = 0; j < nc; ++j) {
            double* bp = B + (size_t) (j0 + j) * ldb + r;
            double v = *bp;
            if (kx > 0) v -= ((acc[j] + red[(0 * 64 + lane) * NC + j]) + red[(1 * 64 + lane) * NC + j]) + red[(2 * 64 + lane) * NC + j];
            if (blk == 0) Bl[lane * NC + j] = v;
            else *bp = v;
        }
    }
    if (blk != 0) return;
    const int h = l1 - l0;
    __syncthreads();                              // (Xs / red are read no more)
    for (int i = t; i < TRSM_L * TRSM_L; i += 256) {
        const int c = i / TRSM_L, rr = i - c * TRSM_L;
        Rl[i] = (rr <= c && c < h) ? R[(size_t) (l0 + c) * lda + l0 + rr] : 0.0;
    }
    __syncthreads();
    const int rr = lane & 15, jj = wv * 4 + (lane >> 4);
    for (int hi = h; hi > 0; hi -= 16) {
        const int s0 = max(0, hi - 16), len = hi - s0;
        const bool act = rr < len && jj < nc;
        double Rd[16];
#pragma unroll
        for (int i = 0; i < 16; ++i)
            Rd[i] = (act && i < len && i >= rr) ? Rl[(s0 + i) * TRSM_L + s0 + rr] : 0.0;
        double b = act ? Bl[(s0 + rr) * NC + jj] : 0.0;
#pragma unroll
        for (int i = 15; i >= 0; --i) {
            if (i < len) {
                if (rr == i && act) b = b / Rd[i];
                const double xi = __shfl(b, (lane & ~15) | i);
                if (rr < i) b = fma(-Rd[i], xi, b);
            }
        }
        if (act) Bl[(s0 + rr) * NC + jj] = b;
        __syncthreads();
        for (int i = t; i < s0 * NC; i += 256) {
            const int row = i % s0, j = i / s0;
            if (j < nc) {
                double s = 0.0;
                for (int q = 0; q < len; ++q) s = fma(Rl[(s0 + q) * TRSM_L + row], Bl[(s0 + q) * NC + j], s);
                Bl[row * NC + j] -= s;
            }
        }
        __syncthreads();
    }
    for (int i = t; i < h * NC; i += 256) {
        const int row = i % h, j = i / h;
        if (j < nc) B[(size_t) (j0 + j) * ldb + l0 + row] = Bl[row * NC + j];
    }
}

static int pick_nc(int nrhs) { return nrhs <= 1 ? 1 : (nrhs <= 4 ? 4 : 16); }

extern "C" {

int qrd_ormqr_skinny_blocks(int mk, int* rpb)
{
    int r = (mk + 255) / 256;
    r = (r + SV_TR - 1) / SV_TR * SV_TR;
    if (r < 64) r = 64;
    if (rpb) *rpb = r;
    return (mk + r - 1) / r;
}

// at most 256 row blocks: ceil(mk / 64) of them up to 16384 rows, of ceil(mk / 256) rows each above
size_t qrd_ormqr_skinny_ws(int m, int w, int nrhs)
{
    const size_t nblk = (size_t) min(256, (m + 63) / 64);
    return (nblk + 1) * (size_t) w * (size_t) nrhs;
}

int qrd_ormqr_skinny(void* stream, const double* Ak, int lda, int mk, int w, const double* T, int ldt, int trans_t, double* Cs, int ldc,
                     int nrhs, double* ws)
{
    if (mk < 1 || w < 1 || w > QRD_SOLVE_MAX_W || w > mk || nrhs < 1) return -7;
    hipStream_t s = (hipStream_t) stream;
    int rpb = 0;
    const int nblk = qrd_ormqr_skinny_blocks(mk, &rpb);
    double* P = ws;
    double* Wt = ws + (size_t) nblk * nrhs * w;
    const int nc = pick_nc(nrhs);
    const dim3 g1(nblk, (nrhs + nc - 1) / nc), g3((mk + 63) / 64, (nrhs + nc - 1) / nc);
    const size_t lds3 = sizeof(double) * ((size_t) w * nc + 3 * 64 * nc);
    if (nc == 1) hipLaunchKernelGGL(ormqr_vtc_kernel<1>, g1, dim3(256), 0, s, Ak, lda, mk, w, Cs, ldc, nrhs, rpb, P);
    else if (nc == 4) hipLaunchKernelGGL(ormqr_vtc_kernel<4>, g1, dim3(256), 0, s, Ak, lda, mk, w, Cs, ldc, nrhs, rpb, P);
    else hipLaunchKernelGGL(ormqr_vtc_kernel<16>, g1, dim3(256), 0, s, Ak, lda, mk, w, Cs, ldc, nrhs, rpb, P);
    int rc = (int) hipGetLastError();
    if (rc) return rc;
    hipLaunchKernelGGL(ormqr_tw_kernel, dim3(nrhs), dim3(256), 0, s, P, nblk, nrhs, w, T, ldt, trans_t, Wt);
    rc = (int) hipGetLastError();
    if (rc) return rc;
    if (nc == 1) hipLaunchKernelGGL(ormqr_cvw_kernel<1>, g3, dim3(256), lds3, s, Ak, lda, mk, w, Wt, Cs, ldc, nrhs);
    else if (nc == 4) hipLaunchKernelGGL(ormqr_cvw_kernel<4>, g3, dim3(256), lds3, s, Ak, lda, mk, w, Wt, Cs, ldc, nrhs);
    else hipLaunchKernelGGL(ormqr_cvw_kernel<16>, g3, dim3(256), lds3, s, Ak, lda, mk, w, Wt, Cs, ldc, nrhs);
    return (int) hipGetLastError();
}

int qrd_trsm_step(void* stream, const double* R, int lda, double* B, int ldb, int nrhs, int row_lo, int l0, int l1, int x0, int x1)
{
    if (l1 - l0 < 1 || l1 - l0 > TRSM_L || x1 - x0 < 0 || x1 - x0 > TRSM_L || row_lo > l0 || nrhs < 1) return -7;
    const int nc = pick_nc(nrhs);
    const dim3 g(1 + (l0 - row_lo + 63) / 64, (nrhs + nc - 1) / nc);
    hipStream_t s = (hipStream_t) stream;
    if (nc == 1) hipLaunchKernelGGL(trsm_step_kernel<1>, g, dim3(256), 0, s, R, lda, B, ldb, nrhs, row_lo, l0, l1, x0, x1);
    else if (nc == 4) hipLaunchKernelGGL(trsm_step_kernel<4>, g, dim3(256), 0, s, R, lda, B, ldb, nrhs, row_lo, l0, l1, x0, x1);
    else hipLaunchKernelGGL(trsm_step_kernel<16>, g, dim3(256), 0, s, R, lda, B, ldb, nrhs, row_lo, l0, l1, x0, x1);
    return (int) hipGetLastError();
}

}   // extern "C"
