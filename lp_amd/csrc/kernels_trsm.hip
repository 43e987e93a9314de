// kernels_trsm.hip -- Z = B . L^-T: a forward substitution with many right-hand sides on the blocked factor of
// kernels_potrf.hip.  Row r of Z solves L.z = B[r,:]^T.  The tall form with equality rows runs it once per
// iteration with B = the `eq` rows of the resident image and L = the factor of K: Zt = A_eq . L^-T, from which the Schur
// complement S = Zt.Zt^T = A_eq.K^-1.A_eq^T is formed.
//
// Rows of B are independent, so one workgroup owns a strip of 16 rows of Z from beginning to end: one launch, no dependency
// between workgroups, no flags.  The strip lives in Z itself (global memory, re-read through L2) and is solved in place,
// 128-block k of L after 128-block:
//   y_k      = r_k . Inv_k^T                 Inv_k: the plan's inverse of the diagonal block (blk_inv(k)), lower triangular
//   r_below -= y_k . L[below, k]^T
// Both are NT products of 16 x 16 output tiles on v_mfma_f64_16x16x4_f64 (the fragment shape of gemm_tile.hpp: lane l holds
// X[l & 15][k = l >> 4], C row = (l >> 4) + 4 * reg, column = l & 15).  Within a round of 16 k the lane's four k are the
// consecutive ones 4 * (l >> 4) + t, t = 0 .. 3 -- one 32-byte load per operand and round, the same permutation on both
// operands.  Every sum runs in a fixed order that depends on nothing but the position of the element: the result is
// bit-reproducible and does not depend on the grid.
#include "gemm_tile.hpp"

namespace lpipm {

constexpr int TRSM_ROWS = 16;        // rows of Z per workgroup
constexpr int TRSM_MAX_SB = 64;      // diagonal super-blocks of the factor the kernel can be told about (order <= 32768 at 512)
struct TrsmInv { const double* inv[TRSM_MAX_SB]; int super_w; };

__global__ __launch_bounds__(256) void trsm_lt_kernel(const double* B, long long ldb, int rows, int cols, const double* L,
                                                      long long ldl, int n, TrsmInv iv, double* Z, long long ldz) {
    __shared__ __attribute__((aligned(32))) double ys[TRSM_ROWS][NB + 4];     // y_k: the P operand of the update below
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int fr = lane & 15, fq = lane >> 4;
    const int r0 = blockIdx.x * TRSM_ROWS;
    double* Zs = Z + (long long)r0 * ldz;
    // the strip's right-hand sides: rows of B, zeros beyond `rows` and `cols`
    for (int e = threadIdx.x; e < TRSM_ROWS * n; e += 256) {
        const int i = e / n, j = e - i * n;
        Zs[(long long)i * ldz + j] = (r0 + i < rows && j < cols) ? B[(long long)(r0 + i) * ldb + j] : 0.0;
    }
    __syncthreads();
    for (int c0 = 0; c0 < n; c0 += NB) {
        const int sb = c0 / iv.super_w, s0 = sb * iv.super_w, off = c0 - s0;
        const int sz = n - s0 < iv.super_w ? n - s0 : iv.super_w;
        const double* Inv = iv.inv[sb] + (long long)off * sz + off;
        // y_k = r_k . Inv_k^T: eight 16-column tiles, two per wave; column tile cb needs k < 16 * (cb + 1) only, so wave w
        // takes the tiles w and 7 - w: nine rounds of k each (which wave sums a tile does not change its sum)
        d4 acc[2];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int cb = h == 0 ? wave : 7 - wave;
            acc[h] = (d4){0.0, 0.0, 0.0, 0.0};
            const double* ap = Zs + (long long)fr * ldz + c0 + 4 * fq;
            const double* bp = Inv + (long long)(cb * 16 + fr) * sz + 4 * fq;
            for (int kk = 0; kk <= cb; ++kk) {
                const d4 a = *(const d4*)(ap + kk * 16), b = *(const d4*)(bp + kk * 16);
#pragma unroll
                for (int t = 0; t < 4; ++t) acc[h] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[t], b[t], acc[h], 0, 0, 0);
            }
        }
#pragma unroll
        for (int h = 0; h < 2; ++h)
#pragma unroll
            for (int r = 0; r < 4; ++r) ys[fq + 4 * r][(h == 0 ? wave : 7 - wave) * 16 + fr] = acc[h][r];
        __syncthreads();                 // every wave has read r_k; y_k is complete in LDS
#pragma unroll
        for (int h = 0; h < 2; ++h)
#pragma unroll
            for (int r = 0; r < 4; ++r) Zs[(long long)(fq + 4 * r) * ldz + c0 + (h == 0 ? wave : 7 - wave) * 16 + fr] = acc[h][r];
        // r_below -= y_k . L[below, k]^T: 16-column tiles dealt to the waves, k = 0 .. 127 each
        const int ntile = (n - c0 - NB) / 16;
        for (int tl = wave; tl < ntile; tl += 4) {
            const int col0 = c0 + NB + tl * 16;
            d4 s = (d4){0.0, 0.0, 0.0, 0.0};
            const double* bp = L + (long long)(col0 + fr) * ldl + c0 + 4 * fq;
#pragma unroll
            for (int kk = 0; kk < NB / 16; ++kk) {
                const d4 a = *(const d4*)&ys[fr][kk * 16 + 4 * fq], b = *(const d4*)(bp + kk * 16);
#pragma unroll
                for (int t = 0; t < 4; ++t) s = __builtin_amdgcn_mfma_f64_16x16x4f64(a[t], b[t], s, 0, 0, 0);
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) Zs[(long long)(fq + 4 * r) * ldz + col0 + fr] -= s[r];
        }
        __syncthreads();                 // r_{k+1} is complete; ys is free again
    }
}
// The same for every member of a lockstep batch: grid (strips, 1, members).  Member z has its L, its diagonal-block inverses
// and its Z bk.stride bytes * z behind member 0's, as everything else in its arena; B likewise, unless it is the one block
// the batch shares (shared_b: the `eq` rows of the one resident image).  A finished member returns before it touches its Z.
// A kernel of its own, so that the single launch above stays the code it was; the body is that kernel's line for line --
// strip ownership, wave-to-tile assignment (w and 7 - w), k order -- on the member's pointers: member z's bits are those of
// a single launch on its L (tests/test_gpu_tall_eq_batch.py holds the two together).
__global__ __launch_bounds__(256) void trsm_lt_batch_kernel(const double* B, long long ldb, int rows, int cols, const double* L,
                                                            long long ldl, int n, TrsmInv iv, double* Z, long long ldz, BatchK bk,
                                                            int shared_b) {
    if (batch_done(bk)) return;
    if (!shared_b) B = batch_ptr(B, bk);
    L = batch_ptr(L, bk);
    Z = batch_ptr(Z, bk);
    __shared__ __attribute__((aligned(32))) double ys[TRSM_ROWS][NB + 4];     // y_k: the P operand of the update below
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int fr = lane & 15, fq = lane >> 4;
    const int r0 = blockIdx.x * TRSM_ROWS;
    double* Zs = Z + (long long)r0 * ldz;
    // the strip's right-hand sides: rows of B, zeros beyond `rows` and `cols`
    for (int e = threadIdx.x; e < TRSM_ROWS * n; e += 256) {
        const int i = e / n, j = e - i * n;
        Zs[(long long)i * ldz + j] = (r0 + i < rows && j < cols) ? B[(long long)(r0 + i) * ldb + j] : 0.0;
    }
    __syncthreads();
    for (int c0 = 0; c0 < n; c0 += NB) {
        const int sb = c0 / iv.super_w, s0 = sb * iv.super_w, off = c0 - s0;
        const int sz = n - s0 < iv.super_w ? n - s0 : iv.super_w;
        const double* Inv = batch_ptr(iv.inv[sb], bk) + (long long)off * sz + off;
        // y_k = r_k . Inv_k^T: eight 16-column tiles, two per wave; column tile cb needs k < 16 * (cb + 1) only, so wave w
        // takes the tiles w and 7 - w: nine rounds of k each (which wave sums a tile does not change its sum)
        d4 acc[2];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int cb = h == 0 ? wave : 7 - wave;
            acc[h] = (d4){0.0, 0.0, 0.0, 0.0};
            const double* ap = Zs + (long long)fr * ldz + c0 + 4 * fq;
            const double* bp = Inv + (long long)(cb * 16 + fr) * sz + 4 * fq;
            for (int kk = 0; kk <= cb; ++kk) {
                const d4 a = *(const d4*)(ap + kk * 16), b = *(const d4*)(bp + kk * 16);
#pragma unroll
                for (int t = 0; t < 4; ++t) acc[h] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[t], b[t], acc[h], 0, 0, 0);
            }
        }
#pragma unroll
        for (int h = 0; h < 2; ++h)
#pragma unroll
            for (int r = 0; r < 4; ++r) ys[fq + 4 * r][(h == 0 ? wave : 7 - wave) * 16 + fr] = acc[h][r];
        __syncthreads();                 // every wave has read r_k; y_k is complete in LDS
#pragma unroll
        for (int h = 0; h < 2; ++h)
#pragma unroll
            for (int r = 0; r < 4; ++r) Zs[(long long)(fq + 4 * r) * ldz + c0 + (h == 0 ? wave : 7 - wave) * 16 + fr] = acc[h][r];
        // r_below -= y_k . L[below, k]^T: 16-column tiles dealt to the waves, k = 0 .. 127 each
        const int ntile = (n - c0 - NB) / 16;
        for (int tl = wave; tl < ntile; tl += 4) {
            const int col0 = c0 + NB + tl * 16;
            d4 s = (d4){0.0, 0.0, 0.0, 0.0};
            const double* bp = L + (long long)(col0 + fr) * ldl + c0 + 4 * fq;
#pragma unroll
            for (int kk = 0; kk < NB / 16; ++kk) {
                const d4 a = *(const d4*)&ys[fr][kk * 16 + 4 * fq], b = *(const d4*)(bp + kk * 16);
#pragma unroll
                for (int t = 0; t < 4; ++t) s = __builtin_amdgcn_mfma_f64_16x16x4f64(a[t], b[t], s, 0, 0, 0);
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) Zs[(long long)(fq + 4 * r) * ldz + col0 + fr] -= s[r];
        }
        __syncthreads();                 // r_{k+1} is complete; ys is free again
    }
}

hipError_t launch_trsm_lt(const double* B, int64_t ldb, int rows, int cols, const FactorPlan& plan, double* Z, int64_t ldz,
                          hipStream_t st, const Batch& bt, bool shared_b) {
    if (rows <= 0 || bt.count <= 0) return hipSuccess;
    const double* L = plan.L; const int64_t ldl = plan.ld;
    const int n = plan.mp;
    if (n <= 0 || n % NB != 0 || cols > n || ldz < n || ldl < n || (ldz & 3) != 0 || (ldl & 3) != 0 || plan.super_w % NB != 0 ||
        (int)plan.sbs.size() > TRSM_MAX_SB)
        return hipErrorInvalidValue;
    TrsmInv iv{};
    iv.super_w = plan.super_w;
    for (size_t i = 0; i < plan.sbs.size(); ++i) iv.inv[i] = plan.sbs[i].inv;
    const unsigned strips = (unsigned)((rows + TRSM_ROWS - 1) / TRSM_ROWS);
    if (bt.count == 1 && bt.first == 0 && !bt.done) {      // no member dimension: the single kernel, as ever
        hipLaunchKernelGGL(trsm_lt_kernel, dim3(strips), dim3(256), 0, st, B, (long long)ldb, rows, cols, L, (long long)ldl, n, iv, Z,
                           (long long)ldz);
        return hipGetLastError();
    }
    if (bt.count > 65535) return hipErrorInvalidValue;
    hipLaunchKernelGGL(trsm_lt_batch_kernel, dim3(strips, 1, (unsigned)bt.count), dim3(256), 0, st, B, (long long)ldb, rows, cols, L,
                       (long long)ldl, n, iv, Z, (long long)ldz, batch_k(bt), shared_b ? 1 : 0);
    return hipGetLastError();
}

}  // namespace lpipm
