// vec_device.hpp -- device helpers shared by the vector kernels (kernels_vec.hip, kernels_tall.hip): fixed-order
// reductions, the lockstep-batch pointer shifts (vbatch, tbatch) and the (virtual) thread a kernel body is written for.
#pragma once
#include "vec_kernels.hpp"

namespace lpipm {

// ---------------------------------------------------------------- reduction helpers
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}
__device__ __forceinline__ double wave_min(double v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v = fmin(v, __shfl_xor(v, off, 64));
    return v;
}
// max that keeps a NaN once it has met one (a residual that is NaN must not read as small)
__device__ __forceinline__ double max_nan(double a, double b) { return (b > a || b != b) ? b : a; }
__device__ __forceinline__ double wave_max(double v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v = max_nan(v, __shfl_xor(v, off, 64));
    return v;
}
// workgroup (256 threads) reduction of K values; thread 0 writes red[slot0 + k][blockIdx.x]
template <int K, bool IS_MIN>
__device__ __forceinline__ void block_reduce_store(double (&v)[K], double* red, int slot0) {
    __shared__ double sm[4][K];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const double w = IS_MIN ? wave_min(v[k]) : wave_sum(v[k]);
        if (lane == 0) sm[wave][k] = w;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const double r = IS_MIN ? fmin(fmin(sm[0][k], sm[1][k]), fmin(sm[2][k], sm[3][k]))
                                    : (sm[0][k] + sm[1][k]) + (sm[2][k] + sm[3][k]);
            red[(slot0 + k) * RED_STRIDE + blockIdx.x] = r;
        }
    }
}
// one wave folds the nblk partials of a slot in a fixed order; every lane gets the result
__device__ __forceinline__ double fold_sum(const double* red, int slot, int nblk) {
    double s = 0.0;
    for (int b = (int)(threadIdx.x & 63); b < nblk; b += 64) s += red[slot * RED_STRIDE + b];
    return wave_sum(s);
}
__device__ __forceinline__ double fold_min(const double* red, int slot, int nblk, double init) {
    double s = init;
    for (int b = (int)(threadIdx.x & 63); b < nblk; b += 64) s = fmin(s, red[slot * RED_STRIDE + b]);
    return wave_min(s);
}

// workgroup (256 threads) maximum of one value (>= 0 or NaN); thread 0 writes red[slot][blockIdx.x]
__device__ __forceinline__ void block_max_store(double v, double* red, int slot) {
    __shared__ double smx[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const double w = wave_max(v);
    if (lane == 0) smx[wave] = w;
    __syncthreads();
    if (threadIdx.x == 0) red[slot * RED_STRIDE + blockIdx.x] = max_nan(max_nan(smx[0], smx[1]), max_nan(smx[2], smx[3]));
}
__device__ __forceinline__ double fold_max(const double* red, int slot, int nblk, double init) {
    double s = init;
    for (int b = (int)(threadIdx.x & 63); b < nblk; b += 64) s = max_nan(s, red[slot * RED_STRIDE + b]);
    return wave_max(s);
}

// LP blockIdx.z of a lockstep batch.  `check_done`: kernels of the iteration skip an LP that has finished.
__device__ __forceinline__ bool vbatch(VecArgs& a, bool check_done) {
    const BatchK bk{a.bstride, check_done ? a.done_chk : nullptr, 0, a.bfirst};
    if (batch_done(bk)) return false;
    if (blockIdx.z == 0 && a.bfirst == 0) return true;
    a.b = batch_ptr(a.b, bk); a.c = batch_ptr(a.c, bk);
    a.x = batch_ptr(a.x, bk); a.y = batch_ptr(a.y, bk); a.z = batch_ptr(a.z, bk);
    a.dinv = batch_ptr(a.dinv, bk); a.xs = batch_ptr(a.xs, bk); a.r1 = batch_ptr(a.r1, bk); a.rD = batch_ptr(a.rD, bk);
    a.p = batch_ptr(a.p, bk); a.u = batch_ptr(a.u, bk); a.dx = batch_ptr(a.dx, bk); a.dz = batch_ptr(a.dz, bk);
    a.dxdz = batch_ptr(a.dxdz, bk);
    a.rP = batch_ptr(a.rP, bk); a.rP2 = batch_ptr(a.rP2, bk); a.q = batch_ptr(a.q, bk); a.dy = batch_ptr(a.dy, bk);
    a.Ax = batch_ptr(a.Ax, bk); a.W = batch_ptr(a.W, bk); a.R = batch_ptr(a.R, bk); a.ATpart = batch_ptr(a.ATpart, bk);
    a.S = batch_ptr(a.S, bk); a.red = batch_ptr(a.red, bk); a.status = batch_ptr(a.status, bk);
    a.potrf_info = batch_ptr(a.potrf_info, bk); a.flags = batch_ptr(a.flags, bk); a.done = batch_ptr(a.done, bk);
    a.skip_refine = batch_ptr(a.skip_refine, bk);
    a.done_chk = batch_ptr(a.done_chk, bk);
    return true;
}

// The same shift for a kernel of the tall form (kernels_tall.hip): besides the VecArgs, every TallArgs pointer and the raw
// right-hand-side pointers the launch was handed (LP 0's arena addresses; null stays null) move to LP bfirst + blockIdx.z.
// Every pointer such a kernel dereferences goes through here: one that does not reads or writes LP 0's vectors.
__device__ __forceinline__ bool tbatch(VecArgs& a, TallArgs& t, TallRhs& r) {
    const BatchK bk{a.bstride, nullptr, 0, a.bfirst};      // (taken before vbatch moves a's own fields)
    if (!vbatch(a, true)) return false;
    if (blockIdx.z == 0 && a.bfirst == 0) return true;
    t.Ws = batch_ptr(t.Ws, bk); t.Ex = batch_ptr(t.Ex, bk); t.T = batch_ptr(t.T, bk); t.G = batch_ptr(t.G, bk);
    t.Us = batch_ptr(t.Us, bk); t.Ve = batch_ptr(t.Ve, bk);
    r.r1a = batch_ptr(r.r1a, bk); r.r2a = batch_ptr(r.r2a, bk); r.r1b = batch_ptr(r.r1b, bk); r.r2b = batch_ptr(r.r2b, bk);
    return true;
}

// A vector kernel's work is written once, for the thread `vt` of the (virtual) 256-thread block `vb` of `nvb`.
struct VThread { int vb, vt, nvb; };
__device__ __forceinline__ VThread plain_thread() { return VThread{(int)blockIdx.x, (int)threadIdx.x, (int)gridDim.x}; }

}  // namespace lpipm
