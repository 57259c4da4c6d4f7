// qr_update.hip -- kernels of the row-append update (qr_update.c, mi355x_qr.h section 6): QR of a triangle stacked on a block of new rows.
//
//   tp_panel_kernel    one workgroup factors [R_kk (w x w triangle) ; B(:, k:k+w)] column by column with the B panel resident in LDS
//   tp_apply_kernel    one workgroup per slab of 32 columns: W = op(T_k) (C1 + V_k^T C2), C1 -= W, C2 -= V_k W on v_mfma_f64_16x16x4_f64
//   tp_colssq_kernel   per-column sum of squares of a block, added into device accumulators (one workgroup per column, fixed order)
//   tp_sqrt_kernel     out[i] = sqrt(in[i])
//
// Reflector j of a panel is [e_j ; V(:, j)]: the identity on top is never stored or multiplied.  With it V_full^T C = C1 + V^T C2 and
// V_full W = [W ; V W], which is all the apply kernel computes.
//
// LDS images (both kernels): a p x 32 block is kept column-major with a leading dimension of TP_LD = 258 doubles.  8-byte accesses are
// served per 32-lane half, bank = (byte address / 4) mod 64, two banks per double, so a half is conflict-free when its 32 double
// indices are distinct mod 32.  The MFMA operand reads are of two kinds:
//   (lane & 15) along the block's columns, (lane >> 4) along its rows (V^T C2: both operands; the C2 accumulator tiles):
//       index = (lane & 15) * 258 + (lane >> 4) + const = 2 (lane & 15) + {0, 1} (mod 32) -- 32 distinct values;
//   (lane & 15) along the rows, (lane >> 4) along the columns (V as the A operand of V W): the four k of a step are taken 8 columns
//       apart (k-step s = columns s, s + 8, s + 16, s + 24; the B operand W uses the same map), so a half reads rows r .. r + 15 of
//       columns c and c + 8: index = (lane & 15) + {0, 8 * 258 = 16 (mod 32)} -- 32 distinct values.
// The 32 x 32 matrices (R_kk, T_k, W) have a leading dimension of 33.
//
// Fragment maps of v_mfma_f64_16x16x4_f64: A operand lane l = A[row l & 15][k l >> 4], B operand lane l = B[k l >> 4][col l & 15],
// C / D register r of lane l = D[row (l >> 4) + 4 r][col l & 15].
//
// Every sum runs in a fixed order (wave butterflies, waves added in wave order, MFMA chains in k order): repeated launches give
// bitwise-equal results.  No atomics.
#include "qr_common.h"
#include "qr_device.h"

#define TP_W QRD_TP_W
#define TP_P QRD_TP_MAXROWS
#define TP_LD (TP_P + 2)
#define TP_LT (TP_W + 1)
#define TP_PANEL_LDS (sizeof(double) * (TP_W * TP_LD + 2 * TP_W * TP_LT + TP_W + 8))
#define TP_APPLY_LDS (sizeof(double) * (2 * TP_W * TP_LD + 3 * TP_W * TP_LT))

static_assert(TP_W == 32 && TP_P % 16 == 0 && TP_LD % 32 == 2, "the LDS maps above assume 32 columns and a leading dimension of 2 mod 32");
static_assert(TP_APPLY_LDS <= 160 * 1024, "the apply kernel's V panel, C2 slab, T and two W tiles must fit one CU's LDS");

// the same sum in every lane; the order of the additions does not depend on the data
__device__ __forceinline__ double tp_wave_sum(double v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// [R (w x w upper triangle, ldr) ; B (p x w, ldb)] = Q [R' ; 0]: R' over R's triangle (the strict lower triangle is neither read nor
// written), V over B, the w x w upper-triangular T (zeros below its diagonal) to T (ldt).  LAPACK dlarfg per column: beta =
// -sign(alpha) hypot(alpha, |x|), tau = (beta - alpha) / beta, v = x / (alpha - beta); x == 0 exactly: tau = 0, nothing changes.
// An exact zero of B stays an exact zero (v = 0 there, and the update adds -tau w * 0).
__global__ void __launch_bounds__(256) tp_panel_kernel(double* __restrict__ R, int ldr, double* __restrict__ B, int ldb, int p, int w,
                                                       double* __restrict__ T, int ldt)
{
    extern __shared__ __attribute__((aligned(16))) double sm[];
    double* Bs = sm;                        // Bs[c * TP_LD + i] = B[i, c]
    double* Rs = Bs + TP_W * TP_LD;         // Rs[c * TP_LT + r] = R[r, c], r <= c
    double* Ts = Rs + TP_W * TP_LT;         // Ts[c * TP_LT + r] = T[r, c]
    double* dots = Ts + TP_W * TP_LT;       // V[:, c]^T v_j, c < j
    double* red = dots + TP_W;
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    for (int c = wv; c < w; c += 4)
        for (int i = lane; i < p; i += 64) Bs[c * TP_LD + i] = B[(size_t) c * ldb + i];
    for (int idx = t; idx < TP_W * TP_W; idx += 256) {
        const int c = idx >> 5, r = idx & 31;
        Rs[c * TP_LT + r] = (r <= c && c < w) ? R[(size_t) c * ldr + r] : 0.0;
        Ts[c * TP_LT + r] = 0.0;
    }
    __syncthreads();
    for (int j = 0; j < w; ++j) {
        double* vj = Bs + j * TP_LD;
        double s = 0.0;
        for (int i = t; i < p; i += 256) s = fma(vj[i], vj[i], s);
        s = tp_wave_sum(s);
        if (lane == 0) red[wv] = s;
        __syncthreads();
        const double ssq = ((red[0] + red[1]) + red[2]) + red[3];
        if (ssq != 0.0) {                   // (the same value in every thread)
            const double alpha = Rs[j * TP_LT + j];
            const double beta = -copysign(hypot(alpha, sqrt(ssq)), alpha);
            const double tau = (beta - alpha) / beta, scal = 1.0 / (alpha - beta);
            for (int i = t; i < p; i += 256) vj[i] *= scal;
            __syncthreads();
            if (t == 0) Rs[j * TP_LT + j] = beta;
            // wave wv: columns wv, wv + 4, ..: the dot product with v_j, then (to the right of j) that column's update
            for (int c = wv; c < w; c += 4) {
                if (c == j) continue;
                double* bc = Bs + c * TP_LD;
                double d = 0.0;
                for (int i = lane; i < p; i += 64) d = fma(vj[i], bc[i], d);
                d = tp_wave_sum(d);
                if (c < j) {
                    if (lane == 0) dots[c] = d;
                } else {
                    const double tw = tau * (Rs[c * TP_LT + j] + d);
                    if (lane == 0) Rs[c * TP_LT + j] -= tw;
                    for (int i = lane; i < p; i += 64) bc[i] = fma(-tw, vj[i], bc[i]);
                }
            }
            __syncthreads();
            // T[0:j, j] = -tau T[0:j, 0:j] (V[:, 0:j]^T v_j), T[j, j] = tau (dlarft, forward columnwise; the unit tops are orthogonal)
            if (t < j) {
                double a = 0.0;
                for (int l = t; l < j; ++l) a = fma(Ts[l * TP_LT + t], dots[l], a);
                Ts[j * TP_LT + t] = -tau * a;
            } else if (t == j) Ts[j * TP_LT + j] = tau;
        }
        __syncthreads();                    // (red, dots and column j are read no more)
    }
    for (int c = wv; c < w; c += 4)
        for (int i = lane; i < p; i += 64) B[(size_t) c * ldb + i] = Bs[c * TP_LD + i];
    for (int idx = t; idx < TP_W * TP_W; idx += 256) {
        const int c = idx >> 5, r = idx & 31;
        if (c < w && r < w) {
            if (r <= c) R[(size_t) c * ldr + r] = Rs[c * TP_LT + r];
            T[(size_t) c * ldt + r] = Ts[c * TP_LT + r];
        }
    }
}

__device__ __forceinline__ v4d tp_mfma(double a, double b, v4d c) { return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0); }

// Columns [32 b, 32 b + 32) of C (b = blockIdx.x; ncols in all):  W = op(T) (C1 + V^T C2), C1 -= W, C2 -= V W  with V p x w (ldv),
// T w x w upper triangular (ldt; what lies below its diagonal is not read), C1 w x ncols (ldc1), C2 p x ncols (ldc2);
// tr != 0: op(T) = T^T (Q'^T C), else T (Q' C).  V and the C2 slab are staged in LDS with the lanes along a column (contiguous global
// accesses, any leading dimension or base); the slab goes back the same way: C2 is read once and written once.
__global__ void __launch_bounds__(256) tp_apply_kernel(int tr, const double* __restrict__ V, int ldv, int p, int w, const double* __restrict__ T,
                                                       int ldt, double* __restrict__ C1, int ldc1, double* __restrict__ C2, int ldc2, int ncols)
{
    extern __shared__ __attribute__((aligned(16))) double sm[];
    double* Vs = sm;                        // Vs[c * TP_LD + i] = V[i, c], zero for i >= p or c >= w
    double* Cs = Vs + TP_W * TP_LD;         // Cs[c * TP_LD + i] = C2[i, c0 + c], zero outside
    double* Ts = Cs + TP_W * TP_LD;         // Ts[c * TP_LT + r] = T[r, c]
    double* W0 = Ts + TP_W * TP_LT;         // W0[c * TP_LT + r] = (C1 + V^T C2)[r, c]
    double* W1 = W0 + TP_W * TP_LT;         // W
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6, l15 = lane & 15, l4 = lane >> 4;
    const int c0 = (int) blockIdx.x * TP_W, nc = min(TP_W, ncols - c0), p16 = (p + 15) & ~15;
    C1 += (size_t) c0 * ldc1;
    C2 += (size_t) c0 * ldc2;
    for (int c = wv; c < TP_W; c += 4)
        for (int i = lane; i < p16; i += 64) {
            Vs[c * TP_LD + i] = (c < w && i < p) ? V[(size_t) c * ldv + i] : 0.0;
            Cs[c * TP_LD + i] = (c < nc && i < p) ? C2[(size_t) c * ldc2 + i] : 0.0;
        }
    for (int idx = t; idx < TP_W * TP_W; idx += 256) {
        const int c = idx >> 5, r = idx & 31;
        Ts[c * TP_LT + r] = (r <= c && c < w) ? T[(size_t) c * ldt + r] : 0.0;
    }
    __syncthreads();
    // 1. wave wv: the 16 x 16 tile (ti, tj) of V^T C2, K = p16 in four interleaved chains added in a fixed order
    const int ti = wv & 1, tj = wv >> 1;
    const int row0 = 16 * ti + l4, col = 16 * tj + l15;        // this lane's D entries: rows row0 + 4 r, column col
    v4d c1v, w0v;
    {
        const double* va = Vs + (16 * ti + l15) * TP_LD + l4;
        const double* cb = Cs + col * TP_LD + l4;
        v4d a0 = {0.0, 0.0, 0.0, 0.0}, a1 = a0, a2 = a0, a3 = a0;
        for (int i = 0; i < p16; i += 16) {
            a0 = tp_mfma(va[i], cb[i], a0);
            a1 = tp_mfma(va[i + 4], cb[i + 4], a1);
            a2 = tp_mfma(va[i + 8], cb[i + 8], a2);
            a3 = tp_mfma(va[i + 12], cb[i + 12], a3);
        }
        const v4d acc = (a0 + a1) + (a2 + a3);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = row0 + 4 * r;
            c1v[r] = (row < w && col < nc) ? C1[(size_t) col * ldc1 + row] : 0.0;
            w0v[r] = acc[r] + c1v[r];
            W0[col * TP_LT + row] = w0v[r];
        }
    }
    __syncthreads();
    // 2. W = op(T) W0, the same tile; C1 -= W
    {
        v4d wacc = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int ks = 0; ks < TP_W / 4; ++ks) {
            const int k = 4 * ks + l4, ar = 16 * ti + l15;
            const double a = tr ? Ts[ar * TP_LT + k] : Ts[k * TP_LT + ar];
            wacc = tp_mfma(a, W0[col * TP_LT + k], wacc);
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = row0 + 4 * r;
            W1[col * TP_LT + row] = wacc[r];
            if (row < w && col < nc) C1[(size_t) col * ldc1 + row] = c1v[r] - wacc[r];
        }
    }
    __syncthreads();
    // 3. C2 -= V W: wave wv takes the 16-row tiles wv, wv + 4, .. of the slab, both column tiles at once (they share the A operand);
    // k-step ks = columns ks, ks + 8, ks + 16, ks + 24 of V (see the bank note above)
    for (int rt = wv; rt < p16 / 16; rt += 4) {
        double* d0p = Cs + l15 * TP_LD + 16 * rt + l4;
        double* d1p = d0p + 16 * TP_LD;
        v4d d0, d1;
#pragma unroll
        for (int r = 0; r < 4; ++r) { d0[r] = d0p[4 * r]; d1[r] = d1p[4 * r]; }
#pragma unroll
        for (int ks = 0; ks < TP_W / 4; ++ks) {
            const int c = ks + 8 * l4;
            const double a = -Vs[c * TP_LD + 16 * rt + l15];
            d0 = tp_mfma(a, W1[l15 * TP_LT + c], d0);
            d1 = tp_mfma(a, W1[(16 + l15) * TP_LT + c], d1);
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) { d0p[4 * r] = d0[r]; d1p[4 * r] = d1[r]; }
    }
    __syncthreads();
    for (int c = wv; c < nc; c += 4)
        for (int i = lane; i < p; i += 64) C2[(size_t) c * ldc2 + i] = Cs[c * TP_LD + i];
}

// acc[c] += sum over i < rows of X[i, c]^2, c = blockIdx.x: thread-strided partial sums, a wave butterfly, the four waves in wave order
__global__ void __launch_bounds__(256) tp_colssq_kernel(const double* __restrict__ X, int ldx, int rows, double* __restrict__ acc)
{
    __shared__ double red[4];
    const int t = threadIdx.x;
    const double* x = X + (size_t) blockIdx.x * ldx;
    double s = 0.0;
    for (int i = t; i < rows; i += 256) s = fma(x[i], x[i], s);
    s = tp_wave_sum(s);
    if ((t & 63) == 0) red[t >> 6] = s;
    __syncthreads();
    if (t == 0) acc[blockIdx.x] += ((red[0] + red[1]) + red[2]) + red[3];
}

__global__ void tp_sqrt_kernel(const double* __restrict__ in, double* __restrict__ out, int n)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = sqrt(in[i]);
}

// more than 64 KiB of LDS per workgroup has to be allowed per kernel and device, once
static int tp_allow_lds(void)
{
    static int done[64];
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return (int) e;
    if (dev >= 0 && dev < 64 && done[dev]) return 0;
    e = hipFuncSetAttribute(reinterpret_cast<const void*>(tp_panel_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int) TP_PANEL_LDS);
    if (e == hipSuccess)
        e = hipFuncSetAttribute(reinterpret_cast<const void*>(tp_apply_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int) TP_APPLY_LDS);
    if (e == hipSuccess && dev >= 0 && dev < 64) done[dev] = 1;
    return (int) e;
}

extern "C" {

int qrd_tp_panel(void* stream, double* Rkk, int ldr, double* Bk, int ldb, int p, int w, double* Tk, int ldt)
{
    if (p < 1 || p > TP_P || w < 1 || w > TP_W || ldr < w || ldb < p || ldt < w) return -7;
    const int rc = tp_allow_lds();
    if (rc) return rc;
    hipLaunchKernelGGL(tp_panel_kernel, dim3(1), dim3(256), TP_PANEL_LDS, (hipStream_t) stream, Rkk, ldr, Bk, ldb, p, w, Tk, ldt);
    return (int) hipGetLastError();
}

int qrd_tp_apply(void* stream, int trans_t, const double* Vk, int ldv, int p, int w, const double* Tk, int ldt, double* C1k, int ldc1,
                 double* C2, int ldc2, int ncols)
{
    if (ncols <= 0) return 0;
    if (p < 1 || p > TP_P || w < 1 || w > TP_W || ldv < p || ldt < w || ldc1 < w || ldc2 < p) return -7;
    const int rc = tp_allow_lds();
    if (rc) return rc;
    hipLaunchKernelGGL(tp_apply_kernel, dim3((unsigned) ((ncols + TP_W - 1) / TP_W)), dim3(256), TP_APPLY_LDS, (hipStream_t) stream,
                       trans_t, Vk, ldv, p, w, Tk, ldt, C1k, ldc1, C2, ldc2, ncols);
    return (int) hipGetLastError();
}

int qrd_tp_colssq_add(void* stream, const double* X, int ldx, int rows, int cols, double* acc)
{
    if (rows <= 0 || cols <= 0) return 0;
    hipLaunchKernelGGL(tp_colssq_kernel, dim3((unsigned) cols), dim3(256), 0, (hipStream_t) stream, X, ldx, rows, acc);
    return (int) hipGetLastError();
}

int qrd_tp_sqrt(void* stream, const double* in, double* out, int n)
{
    if (n <= 0) return 0;
    hipLaunchKernelGGL(tp_sqrt_kernel, dim3((unsigned) ((n + 255) / 256)), dim3(256), 0, (hipStream_t) stream, in, out, n);
    return (int) hipGetLastError();
}

}   // extern "C"
