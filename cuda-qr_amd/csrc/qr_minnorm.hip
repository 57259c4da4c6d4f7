// qr_minnorm.hip -- kernels of the minimum-norm solve (qr_minnorm.c): forward substitution with R^T, and an out-of-place transpose.
//
//   trsm_t_step_kernel     rows below a solved 64-row block updated with it, and the next 64-row diagonal block of R^T solved by substitution
//   transpose_tile_kernel  D = S^T on 64 x 64 tiles through LDS: the global read and the global write are both contiguous
//
// R^T X = B is not trsm_step_kernel (qr_solve.hip) with its indices swapped.  There the updated row runs along R's contiguous direction,
// so "lane = row" reads R coalesced.  Here the updated entry i needs R[x0:x1, i], up to 64 consecutive doubles of COLUMN i: the lanes of
// a load lie along the block's 64 rows (512 B contiguous per column).  The 64 x 64 block is staged in LDS with a leading dimension of 65
// doubles and read back transposed, lane = updated row, so that the sum over the block's rows is taken by one thread in a fixed order
// (the four waves split it and are added in wave order, as in trsm_step_kernel) -- no cross-lane reduction, no atomics.
//
// LDS banks (8-byte accesses are served per 32-lane half, bank = (byte address / 4) mod 64, two banks per double): lanes along a tile
// row at stride 65 doubles = 130 dwords fall on banks 2 lane + const (mod 64), 32 distinct pairs per half -- conflict-free, like the
// stride-1 accesses along a tile column.  An unpadded stride of 64 doubles would put all 32 lanes of a half on one pair of banks.
#include "qr_common.h"
#include "qr_device.h"

#define TT_L 64             // rows of a diagonal block of the forward substitution
#define TT_LD (TT_L + 1)    // leading dimension of a 64 x 64 block in LDS
#define TP_T 64             // tile edge of the transpose

// One step of the blocked forward substitution R^T X = B (R upper triangular, lda; B ldb; the NC right-hand sides j0 .. of blockIdx.y):
//   rows [l0, row_hi) -= R[x0:x1, rows]^T B[x0:x1]        (x0 == x1: no update; B[x0:x1] is a block solved by an earlier launch, x1 <= l0)
//   then block 0 (rows [l0, l1), at most 64) solves R[l0:l1, l0:l1]^T X = B[l0:l1] by substitution, 16 rows at a time.
// Workgroup 0 owns rows [l0, l1), workgroup b >= 1 the 64 rows [l1 + 64 (b - 1), l1 + 64 b) clipped to row_hi.
template <int NC>
__global__ void __launch_bounds__(256) trsm_t_step_kernel(const double* __restrict__ R, int lda, double* __restrict__ B, int ldb, int nrhs,
                                                          int row_hi, int l0, int l1, int x0, int x1)
{
    // Rt: the block R[x0:x1, rb:re] of the update (column c of the block at Rt + c * TT_LD); then the three upper waves' partial sums
    // (3 * 64 * NC <= 3072 doubles); then, in workgroup 0, the diagonal block
    __shared__ double Rt[TT_L * TT_LD];
    __shared__ double Xs[TT_L * NC];
    __shared__ double Bl[TT_L * NC];
    double* red = Rt;
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6, blk = blockIdx.x, j0 = blockIdx.y * NC;
    const int nc = min(NC, nrhs - j0);
    const int rb = blk == 0 ? l0 : l1 + 64 * (blk - 1);
    const int re = blk == 0 ? l1 : min(row_hi, rb + 64);
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
        {
            double a[TT_L / 4];                   // 16 columns per wave, all of its loads in flight at once; lanes along a column
#pragma unroll
            for (int u = 0; u < TT_L / 4; ++u) {
                const int c = wv + 4 * u;
                a[u] = (lane < kx && rb + c < re) ? R[(size_t) (rb + c) * lda + x0 + lane] : 0.0;
            }
#pragma unroll
            for (int u = 0; u < TT_L / 4; ++u) Rt[(wv + 4 * u) * TT_LD + lane] = a[u];
        }
        __syncthreads();
        const int kq = (kx + 3) / 4, k_beg = wv * kq, k_end = min(kx, k_beg + kq);
        if (r < re) {
#pragma unroll
            for (int u = 0; u < TT_L / 4; ++u)
                if (k_beg + u < k_end) {
                    const double v = Rt[lane * TT_LD + k_beg + u];
#pragma unroll
                    for (int j = 0; j < NC; ++j) acc[j] = fma(v, Xs[(k_beg + u) * NC + j], acc[j]);
                }
        }
        __syncthreads();                          // (every wave has read the block: red takes its place)
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
    __syncthreads();                              // (red is read no more)
    double* Rl = Rt;                              // Rl[c * TT_LD + rr] = R[l0 + rr, l0 + c], the upper triangle; zeros elsewhere
    for (int i = t; i < TT_L * TT_L; i += 256) {
        const int c = i / TT_L, rr = i - c * TT_L;
        Rl[c * TT_LD + rr] = (rr <= c && c < h) ? R[(size_t) (l0 + c) * lda + l0 + rr] : 0.0;
    }
    __syncthreads();
    // L = R[l0:l1, l0:l1]^T is lower triangular: L[row, k] = Rl[row * TT_LD + k].  16 lanes per right-hand side hold 16 rows of L
    const int rr = lane & 15, jj = wv * 4 + (lane >> 4);
    for (int s0 = 0; s0 < h; s0 += 16) {
        const int len = min(16, h - s0);
        const bool act = rr < len && jj < nc;
        double Ld[16];
#pragma unroll
        for (int i = 0; i < 16; ++i)
            Ld[i] = (act && i <= rr) ? Rl[(s0 + rr) * TT_LD + s0 + i] : 0.0;
        double b = act ? Bl[(s0 + rr) * NC + jj] : 0.0;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            if (i < len) {
                if (rr == i && act) b = b / Ld[i];
                const double xi = __shfl(b, (lane & ~15) | i);
                if (rr > i) b = fma(-Ld[i], xi, b);
            }
        }
        if (act) Bl[(s0 + rr) * NC + jj] = b;
        __syncthreads();
        const int e0 = s0 + len, rem = h - e0;    // the rows below the 16 just solved
        for (int i = t; i < rem * NC; i += 256) {
            const int row = e0 + i % rem, j = i / rem;
            if (j < nc) {
                double s = 0.0;
                for (int q = 0; q < len; ++q) s = fma(Rl[row * TT_LD + s0 + q], Bl[(s0 + q) * NC + j], s);
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

// D (cols x rows, ldd) = S (rows x cols, lds)^T, one 64 x 64 tile per workgroup (tile (bi, bj) = blockIdx.x % tr, / tr): each wave reads
// 16 columns of the tile of S, 512 B contiguous per column, and writes 16 columns of the tile of D the same way.  8-byte accesses only:
// any leading dimension and any base address of doubles; elements past a ragged edge are neither read nor written.
__global__ void __launch_bounds__(256) transpose_tile_kernel(int rows, int cols, int tr, const double* __restrict__ S, int lds,
                                                             double* __restrict__ D, int ldd)
{
    __shared__ double tile[TP_T * (TP_T + 1)];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int i0 = (int) (blockIdx.x % (unsigned) tr) * TP_T, j0 = (int) (blockIdx.x / (unsigned) tr) * TP_T;
    double a[TP_T / 4];
#pragma unroll
    for (int u = 0; u < TP_T / 4; ++u) {
        const int i = i0 + lane, j = j0 + wv + 4 * u;
        a[u] = (i < rows && j < cols) ? S[(size_t) j * lds + i] : 0.0;
    }
#pragma unroll
    for (int u = 0; u < TP_T / 4; ++u) tile[(wv + 4 * u) * (TP_T + 1) + lane] = a[u];
    __syncthreads();
#pragma unroll
    for (int u = 0; u < TP_T / 4; ++u) {
        const int i = i0 + wv + 4 * u, j = j0 + lane;
        if (i < rows && j < cols) D[(size_t) i * ldd + j] = tile[lane * (TP_T + 1) + wv + 4 * u];
    }
}

static int pick_nc(int nrhs) { return nrhs <= 1 ? 1 : (nrhs <= 4 ? 4 : 16); }

extern "C" {

int qrd_trsm_t_step(void* stream, const double* R, int lda, double* B, int ldb, int nrhs, int row_hi, int l0, int l1, int x0, int x1)
{
    if (l1 - l0 < 1 || l1 - l0 > TT_L || x0 < 0 || x1 - x0 < 0 || x1 - x0 > TT_L || x1 > l0 || row_hi < l1 || nrhs < 1) return -7;
    const int nc = pick_nc(nrhs);
    const dim3 g(1 + (row_hi - l1 + 63) / 64, (nrhs + nc - 1) / nc);
    hipStream_t s = (hipStream_t) stream;
    if (nc == 1) hipLaunchKernelGGL(trsm_t_step_kernel<1>, g, dim3(256), 0, s, R, lda, B, ldb, nrhs, row_hi, l0, l1, x0, x1);
    else if (nc == 4) hipLaunchKernelGGL(trsm_t_step_kernel<4>, g, dim3(256), 0, s, R, lda, B, ldb, nrhs, row_hi, l0, l1, x0, x1);
    else hipLaunchKernelGGL(trsm_t_step_kernel<16>, g, dim3(256), 0, s, R, lda, B, ldb, nrhs, row_hi, l0, l1, x0, x1);
    return (int) hipGetLastError();
}

int qrd_transpose_tiled(void* stream, int rows, int cols, const double* S, int lds, double* D, int ldd)
{
    if (rows <= 0 || cols <= 0) return 0;
    const int tr = (rows + TP_T - 1) / TP_T, tc = (cols + TP_T - 1) / TP_T;
    if ((long long) tr * tc > 0x7fffffffLL) return -7;
    hipLaunchKernelGGL(transpose_tile_kernel, dim3((unsigned) tr * (unsigned) tc), dim3(256), 0, (hipStream_t) stream, rows, cols, tr, S, lds, D, ldd);
    return (int) hipGetLastError();
}

}   // extern "C"
