// qr_downdate.hip -- kernels of the signed-row update (qr_downdate.c, mi355x_qr.h section 6b): the triangle R stacked on a block whose
// first p_add rows are added and whose last p - p_add rows are removed, R'^T R' = R^T R + B^T S B, S = diag(+1 .. +1, -1 .. -1).
//
//   th_panel_kernel    tp_panel_kernel (qr_update.hip) with every inner product over the block's rows weighted by S, and the test of
//                      d = R(j,j)^2 + b^T S b that ends the call when no positive-definite triangle is left
//   th_apply_kernel    tp_apply_kernel: W = T_k^T (C1 + V_k^T S C2), C1 -= W, C2 -= V_k W on v_mfma_f64_16x16x4_f64
//   th_colssq_kernel   acc[c] = max(0, acc[c] + |X(0:p_add, c)|^2 - |X(p_add:p, c)|^2)
//
// Reflector j is Theta_j = I - tau_j u_j u_j^T Phi, u_j = [e_j ; V(:, j)], Phi = diag(I, S): only the products that contract over the
// block's rows see S (V^T S C2, V^T S V); the rank-one and rank-w corrections V w, V W do not.
//
// LDS images, leading dimensions and the MFMA fragment maps are those of qr_update.hip (a p x 32 block column-major at 258 doubles, the
// 32 x 32 matrices at 33): the bank reasoning written there holds unchanged, because S costs no access -- it is applied to the V operand
// of V^T S C2 in the register it was read into, by the row index the lane already holds (row >= p_add: negate).  It is one product,
// not two.
//
// The status word: one device int, 0 while all is well.  Every kernel here reads it before anything else and returns when it is set
// (the same value in every thread, so whole workgroups leave together, before any barrier).  Only th_panel_kernel writes it -- one
// workgroup, one thread, a plain vector store of the failing global column + 1 -- and launches of one call are ordered on one stream, so
// the first failure is the only one recorded.
//
// Every sum runs in a fixed order (wave butterflies, waves added in wave order, MFMA chains in k order): repeated launches give
// bitwise-equal results.  No atomics.
#include "qr_common.h"
#include "qr_device.h"

#define TH_W QRD_TP_W
#define TH_P QRD_TP_MAXROWS
#define TH_LD (TH_P + 2)
#define TH_LT (TH_W + 1)
#define TH_PANEL_LDS (sizeof(double) * (TH_W * TH_LD + 2 * TH_W * TH_LT + TH_W + 8))
#define TH_APPLY_LDS (sizeof(double) * (2 * TH_W * TH_LD + 3 * TH_W * TH_LT))

static_assert(TH_W == 32 && TH_P % 16 == 0 && TH_LD % 32 == 2 && TH_P <= 256, "32 columns, a leading dimension of 2 mod 32, one row per thread");
static_assert(TH_APPLY_LDS <= 160 * 1024, "the apply kernel's V panel, C2 slab, T and two W tiles must fit one CU's LDS");

// the same sum in every lane; the order of the additions does not depend on the data
__device__ __forceinline__ double th_wave_sum(double v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// [R (w x w upper triangle, ldr) ; B (p x w, ldb)] -> [R' ; 0] under the signs S: R' over R's triangle (the strict lower triangle is
// neither read nor written), V over B, the w x w upper-triangular T to T (ldt).  Per column, with sa / sd the sums of squares of the
// added / removed rows: h = hypot(alpha, sqrt(sa)), d = (h - sqrt(sd)) (h + sqrt(sd)) -- the difference of squares is never formed --,
// beta = -sign(alpha) sqrt(d), tau = (beta - alpha) / beta, v = b / (alpha - beta); b == 0 exactly: tau = 0, nothing changes.
// d <= 0 or not finite: *status = col0 + j + 1, and the launch ends without writing anything back.
__global__ void __launch_bounds__(256) th_panel_kernel(double* __restrict__ R, int ldr, double* __restrict__ B, int ldb, int p, int p_add, int w,
                                                       double* __restrict__ T, int ldt, int col0, int* __restrict__ status)
{
    extern __shared__ __attribute__((aligned(16))) double sm[];
    if (*status != 0) return;
    double* Bs = sm;                        // Bs[c * TH_LD + i] = B[i, c]
    double* Rs = Bs + TH_W * TH_LD;         // Rs[c * TH_LT + r] = R[r, c], r <= c
    double* Ts = Rs + TH_W * TH_LT;         // Ts[c * TH_LT + r] = T[r, c]
    double* dots = Ts + TH_W * TH_LT;       // V[:, c]^T S v_j, c < j
    double* red = dots + TH_W;              // 4 partial sums of the added rows, 4 of the removed ones
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    for (int c = wv; c < w; c += 4)
        for (int i = lane; i < p; i += 64) Bs[c * TH_LD + i] = B[(size_t) c * ldb + i];
    for (int idx = t; idx < TH_W * TH_W; idx += 256) {
        const int c = idx >> 5, r = idx & 31;
        Rs[c * TH_LT + r] = (r <= c && c < w) ? R[(size_t) c * ldr + r] : 0.0;
        Ts[c * TH_LT + r] = 0.0;
    }
    __syncthreads();
    for (int j = 0; j < w; ++j) {
        double* vj = Bs + j * TH_LD;
        // thread t owns row t (p <= 256): its square goes to the sum of its sign
        const double x = t < p ? vj[t] : 0.0, x2 = x * x;
        const double sa_w = th_wave_sum(t < p_add ? x2 : 0.0), sd_w = th_wave_sum(t < p_add ? 0.0 : x2);
        if (lane == 0) { red[wv] = sa_w; red[4 + wv] = sd_w; }
        __syncthreads();
        const double sa = ((red[0] + red[1]) + red[2]) + red[3], sd = ((red[4] + red[5]) + red[6]) + red[7];
        if (sa != 0.0 || sd != 0.0) {       // (the same values in every thread)
            const double alpha = Rs[j * TH_LT + j];
            const double h = hypot(alpha, sqrt(sa)), nd = sqrt(sd), d = (h - nd) * (h + nd);
            if (!(d > 0.0) || !isfinite(d)) {
                if (t == 0) *status = col0 + j + 1;
                return;
            }
            const double beta = -copysign(sqrt(d), alpha);
            const double tau = (beta - alpha) / beta, scal = 1.0 / (alpha - beta);
            if (t < p) vj[t] = x * scal;
            __syncthreads();
            if (t == 0) Rs[j * TH_LT + j] = beta;
            // wave wv: columns wv, wv + 4, ..: the signed dot product with v_j, then (to the right of j) that column's update
            for (int c = wv; c < w; c += 4) {
                if (c == j) continue;
                double* bc = Bs + c * TH_LD;
                double dt = 0.0;
                for (int i = lane; i < p; i += 64) dt = fma(i < p_add ? vj[i] : -vj[i], bc[i], dt);
                dt = th_wave_sum(dt);
                if (c < j) {
                    if (lane == 0) dots[c] = dt;
                } else {
                    const double tw = tau * (Rs[c * TH_LT + j] + dt);
                    if (lane == 0) Rs[c * TH_LT + j] -= tw;
                    for (int i = lane; i < p; i += 64) bc[i] = fma(-tw, vj[i], bc[i]);
                }
            }
            __syncthreads();
            // T[0:j, j] = -tau T[0:j, 0:j] (V[:, 0:j]^T S v_j), T[j, j] = tau: dlarft's recursion on V^T S V (the unit tops are orthogonal)
            if (t < j) {
                double a = 0.0;
                for (int l = t; l < j; ++l) a = fma(Ts[l * TH_LT + t], dots[l], a);
                Ts[j * TH_LT + t] = -tau * a;
            } else if (t == j) Ts[j * TH_LT + j] = tau;
        }
        __syncthreads();                    // (red, dots and column j are read no more)
    }
    for (int c = wv; c < w; c += 4)
        for (int i = lane; i < p; i += 64) B[(size_t) c * ldb + i] = Bs[c * TH_LD + i];
    for (int idx = t; idx < TH_W * TH_W; idx += 256) {
        const int c = idx >> 5, r = idx & 31;
        if (c < w && r < w) {
            if (r <= c) R[(size_t) c * ldr + r] = Rs[c * TH_LT + r];
            T[(size_t) c * ldt + r] = Ts[c * TH_LT + r];
        }
    }
}

__device__ __forceinline__ v4d th_mfma(double a, double b, v4d c) { return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0); }

// Columns [32 b, 32 b + 32) of C (b = blockIdx.x; ncols in all):  W = T^T (C1 + V^T S C2), C1 -= W, C2 -= V W  with V p x w (ldv),
// T w x w upper triangular (ldt; what lies below its diagonal is not read), C1 w x ncols (ldc1), C2 p x ncols (ldc2).  Staging as in
// tp_apply_kernel: lanes along a column, C2 read once and written once.
__global__ void __launch_bounds__(256) th_apply_kernel(const double* __restrict__ V, int ldv, int p, int p_add, int w, const double* __restrict__ T,
                                                       int ldt, double* __restrict__ C1, int ldc1, double* __restrict__ C2, int ldc2, int ncols,
                                                       const int* __restrict__ status)
{
    extern __shared__ __attribute__((aligned(16))) double sm[];
    if (*status != 0) return;
    double* Vs = sm;                        // Vs[c * TH_LD + i] = V[i, c], zero for i >= p or c >= w
    double* Cs = Vs + TH_W * TH_LD;         // Cs[c * TH_LD + i] = C2[i, c0 + c], zero outside
    double* Ts = Cs + TH_W * TH_LD;         // Ts[c * TH_LT + r] = T[r, c]
    double* W0 = Ts + TH_W * TH_LT;         // W0[c * TH_LT + r] = (C1 + V^T S C2)[r, c]
    double* W1 = W0 + TH_W * TH_LT;         // W
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6, l15 = lane & 15, l4 = lane >> 4;
    const int c0 = (int) blockIdx.x * TH_W, nc = min(TH_W, ncols - c0), p16 = (p + 15) & ~15;
    C1 += (size_t) c0 * ldc1;
    C2 += (size_t) c0 * ldc2;
    for (int c = wv; c < TH_W; c += 4)
        for (int i = lane; i < p16; i += 64) {
            Vs[c * TH_LD + i] = (c < w && i < p) ? V[(size_t) c * ldv + i] : 0.0;
            Cs[c * TH_LD + i] = (c < nc && i < p) ? C2[(size_t) c * ldc2 + i] : 0.0;
        }
    for (int idx = t; idx < TH_W * TH_W; idx += 256) {
        const int c = idx >> 5, r = idx & 31;
        Ts[c * TH_LT + r] = (r <= c && c < w) ? T[(size_t) c * ldt + r] : 0.0;
    }
    __syncthreads();
    // 1. wave wv: the 16 x 16 tile (ti, tj) of V^T S C2, K = p16 in four interleaved chains added in a fixed order.  This lane's V
    // operand of chain q at step i is row i + 4 q + l4 of the block: negated from row p_add on.
    const int ti = wv & 1, tj = wv >> 1;
    const int row0 = 16 * ti + l4, col = 16 * tj + l15;        // this lane's D entries: rows row0 + 4 r, column col
    v4d c1v, w0v;
    {
        const double* va = Vs + (16 * ti + l15) * TH_LD + l4;
        const double* cb = Cs + col * TH_LD + l4;
        const int pa = p_add - l4;                             // row i + 4 q + l4 < p_add  <=>  i + 4 q < pa
        v4d a0 = {0.0, 0.0, 0.0, 0.0}, a1 = a0, a2 = a0, a3 = a0;
        for (int i = 0; i < p16; i += 16) {
            a0 = th_mfma(i < pa ? va[i] : -va[i], cb[i], a0);
            a1 = th_mfma(i + 4 < pa ? va[i + 4] : -va[i + 4], cb[i + 4], a1);
            a2 = th_mfma(i + 8 < pa ? va[i + 8] : -va[i + 8], cb[i + 8], a2);
            a3 = th_mfma(i + 12 < pa ? va[i + 12] : -va[i + 12], cb[i + 12], a3);
        }
        const v4d acc = (a0 + a1) + (a2 + a3);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = row0 + 4 * r;
            c1v[r] = (row < w && col < nc) ? C1[(size_t) col * ldc1 + row] : 0.0;
            w0v[r] = acc[r] + c1v[r];
            W0[col * TH_LT + row] = w0v[r];
        }
    }
    __syncthreads();
    // 2. W = T^T W0, the same tile; C1 -= W
    {
        v4d wacc = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int ks = 0; ks < TH_W / 4; ++ks) {
            const int k = 4 * ks + l4, ar = 16 * ti + l15;
            wacc = th_mfma(Ts[ar * TH_LT + k], W0[col * TH_LT + k], wacc);
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = row0 + 4 * r;
            W1[col * TH_LT + row] = wacc[r];
            if (row < w && col < nc) C1[(size_t) col * ldc1 + row] = c1v[r] - wacc[r];
        }
    }
    __syncthreads();
    // 3. C2 -= V W (no signs: the correction is along u_j, not Phi u_j): wave wv takes the 16-row tiles wv, wv + 4, .. of the slab, both
    // column tiles at once; k-step ks = columns ks, ks + 8, ks + 16, ks + 24 of V (the bank note of qr_update.hip)
    for (int rt = wv; rt < p16 / 16; rt += 4) {
        double* d0p = Cs + l15 * TH_LD + 16 * rt + l4;
        double* d1p = d0p + 16 * TH_LD;
        v4d d0, d1;
#pragma unroll
        for (int r = 0; r < 4; ++r) { d0[r] = d0p[4 * r]; d1[r] = d1p[4 * r]; }
#pragma unroll
        for (int ks = 0; ks < TH_W / 4; ++ks) {
            const int c = ks + 8 * l4;
            const double a = -Vs[c * TH_LD + 16 * rt + l15];
            d0 = th_mfma(a, W1[l15 * TH_LT + c], d0);
            d1 = th_mfma(a, W1[(16 + l15) * TH_LT + c], d1);
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) { d0p[4 * r] = d0[r]; d1p[4 * r] = d1[r]; }
    }
    __syncthreads();
    for (int c = wv; c < nc; c += 4)
        for (int i = lane; i < p; i += 64) C2[(size_t) c * ldc2 + i] = Cs[c * TH_LD + i];
}

// acc[c] = max(0, acc[c] + sum over i < p_add of X[i, c]^2 - sum over p_add <= i < p of X[i, c]^2), c = blockIdx.x, p <= 256: one row per
// thread, two wave butterflies, the four waves in wave order
__global__ void __launch_bounds__(256) th_colssq_kernel(const double* __restrict__ X, int ldx, int p, int p_add, double* __restrict__ acc,
                                                        const int* __restrict__ status)
{
    __shared__ double red[8];
    if (*status != 0) return;
    const int t = threadIdx.x;
    const double x = t < p ? X[(size_t) blockIdx.x * ldx + t] : 0.0, x2 = x * x;
    const double sa = th_wave_sum(t < p_add ? x2 : 0.0), sd = th_wave_sum(t < p_add ? 0.0 : x2);
    if ((t & 63) == 0) { red[t >> 6] = sa; red[4 + (t >> 6)] = sd; }
    __syncthreads();
    if (t == 0) {
        const double a = ((red[0] + red[1]) + red[2]) + red[3], d = ((red[4] + red[5]) + red[6]) + red[7];
        acc[blockIdx.x] = fmax(0.0, (acc[blockIdx.x] + a) - d);
    }
}

// more than 64 KiB of LDS per workgroup has to be allowed per kernel and device, once
static int th_allow_lds(void)
{
    static int done[64];
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return (int) e;
    if (dev >= 0 && dev < 64 && done[dev]) return 0;
    e = hipFuncSetAttribute(reinterpret_cast<const void*>(th_panel_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int) TH_PANEL_LDS);
    if (e == hipSuccess)
        e = hipFuncSetAttribute(reinterpret_cast<const void*>(th_apply_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int) TH_APPLY_LDS);
    if (e == hipSuccess && dev >= 0 && dev < 64) done[dev] = 1;
    return (int) e;
}

extern "C" {

int qrd_th_panel(void* stream, double* Rkk, int ldr, double* Bk, int ldb, int p, int p_add, int w, double* Tk, int ldt, int col0, int* status)
{
    if (p < 1 || p > TH_P || p_add < 0 || p_add > p || w < 1 || w > TH_W || ldr < w || ldb < p || ldt < w || col0 < 0 || !status) return -7;
    const int rc = th_allow_lds();
    if (rc) return rc;
    hipLaunchKernelGGL(th_panel_kernel, dim3(1), dim3(256), TH_PANEL_LDS, (hipStream_t) stream, Rkk, ldr, Bk, ldb, p, p_add, w, Tk, ldt, col0,
                       status);
    return (int) hipGetLastError();
}

int qrd_th_apply(void* stream, const double* Vk, int ldv, int p, int p_add, int w, const double* Tk, int ldt, double* C1k, int ldc1,
                 double* C2, int ldc2, int ncols, const int* status)
{
    if (ncols <= 0) return 0;
    if (p < 1 || p > TH_P || p_add < 0 || p_add > p || w < 1 || w > TH_W || ldv < p || ldt < w || ldc1 < w || ldc2 < p || !status) return -7;
    const int rc = th_allow_lds();
    if (rc) return rc;
    hipLaunchKernelGGL(th_apply_kernel, dim3((unsigned) ((ncols + TH_W - 1) / TH_W)), dim3(256), TH_APPLY_LDS, (hipStream_t) stream,
                       Vk, ldv, p, p_add, w, Tk, ldt, C1k, ldc1, C2, ldc2, ncols, status);
    return (int) hipGetLastError();
}

int qrd_th_colssq(void* stream, const double* X, int ldx, int p, int p_add, int cols, double* acc, const int* status)
{
    if (cols <= 0) return 0;
    if (p < 1 || p > TH_P || p_add < 0 || p_add > p || ldx < p || !status) return -7;
    hipLaunchKernelGGL(th_colssq_kernel, dim3((unsigned) cols), dim3(256), 0, (hipStream_t) stream, X, ldx, p, p_add, acc, status);
    return (int) hipGetLastError();
}

}   // extern "C"
