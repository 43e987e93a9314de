// kernels_scale.hip -- power-of-two row and column equilibration of the resident matrix (lpipm_set_scaling).
//
// Integer exponents kr[i], kc[j], all zero at the start.  One pass, from the stored structural block X (m x nx):
//   S_ij  = |ldexp(X_ij, kr[i] + kc[j])|            always from the ORIGINAL X_ij, one ldexp by the summed exponent
//   rmax_i = fmax_j S_ij,  cmax_j = fmax_i S_ij     NaNs ignored, both from the same exponents
//   a finite maximum a > 0 with frexp(a) = (f, e) moves its exponent by -(e floordiv 2); every other maximum by 0
// so a maximum in [0.5, 2) is the fixed point.  After the last pass X_ij <- ldexp(X_ij, kr[i] + kc[j]) in place; the slack
// column of `ub` row i, which is not stored, gets kc = -kr[i]: its entry stays exactly 1.
// fmax does not depend on the order of its operands, so the decomposition below is free: no fixed-order reduction is
// needed for bit-reproducible exponents, and no atomics are used.
#include "lpipm_internal.hpp"

namespace lpipm {

namespace {
constexpr int SC_ROWS = 128;                 // rows of a workgroup's block: 32 per wave
constexpr int SC_COLS = 512;                 // columns of it: 4 16-byte loads per lane and row
constexpr int SC_WROWS = SC_ROWS / 4;
constexpr int SC_LOADS = SC_COLS / 128;

__device__ __forceinline__ int exponent_step(double a) {
    if (!(a > 0.0) || isinf(a)) return 0;
    int e;
    (void)frexp(a, &e);
    return -(e >> 1);                         // floor division by 2 (arithmetic shift)
}

// What a lane holds of its block: the columns of its SC_LOADS pairs and their exponents.
struct LaneCols {
    int col[SC_LOADS];
    bool in[SC_LOADS];
    int k[2 * SC_LOADS];
};
__device__ __forceinline__ LaneCols lane_cols(const int32_t* __restrict__ kc, int npa) {
    LaneCols l;
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int t = 0; t < SC_LOADS; ++t) {
        l.col[t] = blockIdx.x * SC_COLS + t * 128 + 2 * lane;
        l.in[t] = l.col[t] < npa;             // npa is even: a pair is inside or outside as a whole
        l.k[2 * t] = l.in[t] ? kc[l.col[t]] : 0;
        l.k[2 * t + 1] = l.in[t] ? kc[l.col[t] + 1] : 0;
    }
    return l;
}

// grid (column chunks, row blocks, exponent sets).  Row maxima of the block's 512 columns by an in-wave reduction into
// rslab[chunk][row]; column maxima of its 128 rows into cslab[row block][column].  k_scale_update folds the slabs.
__global__ __launch_bounds__(256) void k_scale_maxima(const double* __restrict__ A, int mp, int npa, const int32_t* __restrict__ kr,
                                                      const int32_t* __restrict__ kc, long long estride,
                                                      double* __restrict__ rslab, double* __restrict__ cslab, int ncc, int nrb,
                                                      BatchK bk) {
    __shared__ double sm[4][SC_COLS];
    const long long z = batch_lp(bk);
    A = batch_ptr(A, bk);
    kr += z * estride; kc += z * estride;
    rslab += z * (long long)ncc * mp; cslab += z * (long long)nrb * npa;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const LaneCols l = lane_cols(kc, npa);
    double cm[2 * SC_LOADS];
#pragma unroll
    for (int q = 0; q < 2 * SC_LOADS; ++q) cm[q] = 0.0;
    const int r0 = blockIdx.y * SC_ROWS + wave * SC_WROWS;
#pragma unroll 4
    for (int r = 0; r < SC_WROWS; ++r) {
        const int i = r0 + r;
        const int kri = kr[i];
        const double* row = A + (long long)i * npa;
        double rm = 0.0;
#pragma unroll
        for (int t = 0; t < SC_LOADS; ++t) {
            if (!l.in[t]) continue;
            const double2 v = *reinterpret_cast<const double2*>(row + l.col[t]);
            const double s0 = fabs(ldexp(v.x, kri + l.k[2 * t])), s1 = fabs(ldexp(v.y, kri + l.k[2 * t + 1]));
            cm[2 * t] = fmax(cm[2 * t], s0); cm[2 * t + 1] = fmax(cm[2 * t + 1], s1);
            rm = fmax(rm, fmax(s0, s1));
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) rm = fmax(rm, __shfl_xor(rm, o, 64));
        if (lane == 0) rslab[(long long)blockIdx.x * mp + i] = rm;
    }
#pragma unroll
    for (int t = 0; t < SC_LOADS; ++t) { sm[wave][t * 128 + 2 * lane] = cm[2 * t]; sm[wave][t * 128 + 2 * lane + 1] = cm[2 * t + 1]; }
    __syncthreads();
    for (int q = threadIdx.x; q < SC_COLS; q += 256) {
        const int col = blockIdx.x * SC_COLS + q;
        if (col < npa) cslab[(long long)blockIdx.y * npa + col] = fmax(fmax(sm[0][q], sm[1][q]), fmax(sm[2][q], sm[3][q]));
    }
}

// O(m + n): folds the slabs and moves the exponents of the m rows and the nx structural columns.  last: the slack column of
// `ub` row i < ns (column nx + i) gets minus that row's final exponent.
__global__ __launch_bounds__(256) void k_scale_update(int m, int mp, int nx, int npa, int ns, int32_t* __restrict__ kr,
                                                      int32_t* __restrict__ kc, long long estride, const double* __restrict__ rslab,
                                                      const double* __restrict__ cslab, int ncc, int nrb, int last, BatchK bk) {
    const long long z = batch_lp(bk);
    kr += z * estride; kc += z * estride;
    rslab += z * (long long)ncc * mp; cslab += z * (long long)nrb * npa;
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t < m) {
        double a = 0.0;
        for (int ch = 0; ch < ncc; ++ch) a = fmax(a, rslab[(long long)ch * mp + t]);
        const int k = kr[t] + exponent_step(a);
        kr[t] = k;
        if (last && t < ns) kc[nx + t] = -k;
    }
    if (t < nx) {
        double a = 0.0;
        for (int rb = 0; rb < nrb; ++rb) a = fmax(a, cslab[(long long)rb * npa + t]);
        kc[t] += exponent_step(a);
    }
}

// X_ij <- ldexp(X_ij, kr[i] + kc[j]); the grid of k_scale_maxima.  Padding is zero and stays zero.
__global__ __launch_bounds__(256) void k_scale_apply(double* __restrict__ A, int npa, const int32_t* __restrict__ kr,
                                                     const int32_t* __restrict__ kc, long long estride, BatchK bk) {
    const long long z = batch_lp(bk);
    A = batch_ptr(A, bk);
    kr += z * estride; kc += z * estride;
    const LaneCols l = lane_cols(kc, npa);
    const int r0 = blockIdx.y * SC_ROWS + (threadIdx.x >> 6) * SC_WROWS;
#pragma unroll 4
    for (int r = 0; r < SC_WROWS; ++r) {
        const int kri = kr[r0 + r];
        double* row = A + (long long)(r0 + r) * npa;
#pragma unroll
        for (int t = 0; t < SC_LOADS; ++t) {
            if (!l.in[t]) continue;
            double2 v = *reinterpret_cast<double2*>(row + l.col[t]);
            v.x = ldexp(v.x, kri + l.k[2 * t]); v.y = ldexp(v.y, kri + l.k[2 * t + 1]);
            *reinterpret_cast<double2*>(row + l.col[t]) = v;
        }
    }
}

// b_i <- ldexp(b_i, kr[i]) (i < m), c_j <- ldexp(c_j, kc[j]) (j < nc); either vector may be null.  Every member of the
// launch, finished or not: these are the inputs of the next solve.
__global__ __launch_bounds__(256) void k_scale_vectors(double* __restrict__ b, int m, double* __restrict__ c, int nc,
                                                       const int32_t* __restrict__ kr, const int32_t* __restrict__ kc,
                                                       long long estride, BatchK bk) {
    const long long z = batch_lp(bk);
    b = batch_ptr(b, bk); c = batch_ptr(c, bk);
    kr += z * estride; kc += z * estride;
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (b && t < m) b[t] = ldexp(b[t], kr[t]);
    if (c && t < nc) c[t] = ldexp(c[t], kc[t]);
}

// x_j <- ldexp(x_j, kc[j]): the solution of the scaled problem back in the caller's units
__global__ __launch_bounds__(256) void k_unscale_x(double* __restrict__ x, int n, const int32_t* __restrict__ kc, long long estride,
                                                   BatchK bk) {
    x = batch_ptr(x, bk);
    kc += batch_lp(bk) * estride;
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t < n) x[t] = ldexp(x[t], kc[t]);
}

inline int chunks_of(int npa) { return (npa + SC_COLS - 1) / SC_COLS; }
inline size_t exp_bytes(int mp, int np, int sets) { return (size_t)round_up((uint64_t)sets * (size_t)(mp + np) * sizeof(int32_t), 256); }
}  // namespace

size_t scale_buf_bytes(int mp, int np, int npa, int sets) {
    const size_t slabs = (size_t)chunks_of(npa) * mp + (size_t)(mp / SC_ROWS) * npa;
    return exp_bytes(mp, np, sets) + (size_t)sets * slabs * sizeof(double);
}
ScaleBuf scale_buf_place(void* base, int mp, int np, int npa, int sets) {
    ScaleBuf s;
    s.kr = (int32_t*)base; s.kc = s.kr + mp;
    s.estride = sets > 1 ? (long long)(mp + np) : 0;
    s.rslab = (double*)((char*)base + exp_bytes(mp, np, sets));
    s.cslab = s.rslab + (size_t)sets * chunks_of(npa) * mp;
    s.sets = sets;
    return s;
}

hipError_t launch_equilibrate(const ScaleBuf& s, double* A, int m, int mp, int nx, int npa, int ns, int passes, hipStream_t st,
                              const Batch& bt) {
    const int ncc = chunks_of(npa), nrb = mp / SC_ROWS;
    const dim3 grid(ncc, nrb, bt.count), ugrid(((m > nx ? m : nx) + 255) / 256, 1, bt.count);
    const BatchK bk = batch_k(Batch{bt.count, bt.stride, nullptr, bt.first});
    for (int p = 0; p < passes; ++p) {
        hipLaunchKernelGGL(k_scale_maxima, grid, dim3(256), 0, st, A, mp, npa, s.kr, s.kc, s.estride, s.rslab, s.cslab, ncc, nrb, bk);
        hipLaunchKernelGGL(k_scale_update, ugrid, dim3(256), 0, st, m, mp, nx, npa, ns, s.kr, s.kc, s.estride, s.rslab, s.cslab, ncc,
                           nrb, p + 1 == passes ? 1 : 0, bk);
    }
    hipLaunchKernelGGL(k_scale_apply, grid, dim3(256), 0, st, A, npa, s.kr, s.kc, s.estride, bk);
    return hipGetLastError();
}

hipError_t launch_scale_vectors(const ScaleBuf& s, double* b, int m, double* c, int nc, hipStream_t st, const Batch& bt) {
    const int len = (b ? m : 0) > (c ? nc : 0) ? (b ? m : 0) : (c ? nc : 0);
    if (len <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_scale_vectors, dim3((len + 255) / 256, 1, bt.count), dim3(256), 0, st, b, m, c, nc, s.kr, s.kc, s.estride,
                       batch_k(Batch{bt.count, bt.stride, nullptr, bt.first}));
    return hipGetLastError();
}

hipError_t launch_unscale_x(const ScaleBuf& s, double* x, int n, hipStream_t st, const Batch& bt) {
    hipLaunchKernelGGL(k_unscale_x, dim3((n + 255) / 256, 1, bt.count), dim3(256), 0, st, x, n, s.kc, s.estride,
                       batch_k(Batch{bt.count, bt.stride, nullptr, bt.first}));
    return hipGetLastError();
}

}  // namespace lpipm
