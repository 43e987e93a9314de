// kernels_tall.hip -- the vector stage of the tall inequality form (lpipm_upload_ub_tall) and the transpose it starts from.
//
// A pure-`ub` LP, min c^T x, X.x <= b, x >= 0, in slack form A = [X I] with X m x nx and m >> nx.  The normal matrix
// A.D.A^T is m x m; the same Newton system reduces to the nx x nx SPD matrix
//   K = X^T.diag(W_s).X + diag(E_x),   W_s[i] = z_{nx+i} / x_{nx+i},   E_x[j] = z_j / x_j,
// built by the fp64 MFMA A.D.A^T module from the resident transpose Xt (its `A`, contraction over the m rows) with W_s as
// its `dinv`.  sym_solve(r1, r2) (newton_equations.rs:214-225), r1 = [r1_x; r1_s], then reads
//   t   = W_s * r2 + r1_s              k_tall_setup
//   g   = X^T.t - r1_x                 gemv_t over X, slabs folded by k_tall_fold     (r1_x itself, never Dinv * r1)
//   u_x = K^-1 g                       Cholesky chain + super-block solves
//   u_s = r2 - X.u_x                   gemv_n over X (alpha = -1, addend r2)
//   v   = W_s * u_s + r1_s             k_tall_pq_uv / k_tall_uv_corr
//   u   = [u_x; u_s]
// Both u and v come from the reduced solve itself: taking only v from it and u from the dense epilogue Dinv * (A^T.v - r1)
// cancels catastrophically on the slack block.  Everything downstream (d_tau, Delta, ratio test, step,
// residuals, indicators) is the dense path's and sees p, q, u, v where it sees them there.
// Reductions are fixed-order (kernels_vec.hip's two stages, the same slots).  The vector kernels run with gridDim.z = the LPs
// of the launch (a single tall LP, or the members of lpipm_upload_lockstep_shared_ub_tall / lpipm_upload_lockstep_ub_tall): tbatch moves the VecArgs, the
// TallArgs and the right-hand sides to the member and skips a finished one, as vbatch does on the dense path; a member's
// arithmetic and reduction order are those of the single LP.  The kernels of the speculatively enqueued head test the done
// word.
// Equality rows (lpipm_upload_ub_eq_tall, t.me > 0): the image is [X; A_eq], K is built from the ms `ub` rows alone, and between
// the two halves of the solve on K = L.L^T the `eq` rows come in through Zt = A_eq.L^-T and S = Zt.Zt^T (kernels_trsm.hip,
// solver.hip: tall_eq_schur, tall_eq_reduced_solve):
//   w = L^-1 g;  h = r2_e - Zt.w;  v_e = S^-1 h;  w += Zt^T.v_e (k_tall_eq_add_w);  u_x = L^-T w;  v = [W_s * u_s + r1_s; v_e]
// k_tall_setup, k_tall_pq_uv and k_tall_uv_corr are one body each with two instantiations (template <bool EQ>, picked by the host
// wrapper from t.me > 0): under EQ slack quantities loop over ms and row quantities over ms + me, taking v_e from Ve; without it
// ms == m and me == 0, the loops run to m and no line that reads Ve is compiled, so the kernels of every other tall upload do what
// they did before there were equality rows: their bits stay.  k_tall_fold and k_tall_residuals depend on neither count.
#include "vec_kernels.hpp"
#include "vec_device.hpp"

namespace lpipm {

// ---------------------------------------------------------------- resident transpose
// Xt[j][i] = X[i][j], i < m, j < nx, through a 32 x 32 LDS tile (rows padded by one double: the transposed reads walk a
// column of the tile).  Both sides move whole 256-byte row segments.  Xt is zeroed beforehand: nothing outside the m x nx
// block is written.  grid (column tiles of X, row tiles of X, members), 32 x 8 threads: member z of a batch whose members
// own their matrices has its X and its Xt `stride` bytes * z further, as everything else in its arena.
constexpr int TT = 32;
__global__ __launch_bounds__(256) void k_tall_transpose(const double* __restrict__ X, long long ldx, int m, int nx,
                                                        double* __restrict__ Xt, long long ldt, long long stride) {
    __shared__ double tile[TT][TT + 1];
    X = (const double*)((const char*)X + (long long)blockIdx.z * stride);
    Xt = (double*)((char*)Xt + (long long)blockIdx.z * stride);
    const int tx = threadIdx.x, ty = threadIdx.y;
    const long long i0 = (long long)blockIdx.y * TT;
    const int j0 = blockIdx.x * TT;
    for (int r = ty; r < TT; r += 8) {
        const long long i = i0 + r;
        const int j = j0 + tx;
        tile[r][tx] = (i < m && j < nx) ? X[i * ldx + j] : 0.0;
    }
    __syncthreads();
    for (int r = ty; r < TT; r += 8) {
        const int j = j0 + r;
        const long long i = i0 + tx;
        if (j < nx && i < m) Xt[(long long)j * ldt + i] = tile[tx][r];
    }
}
hipError_t tall_transpose(const double* X, int64_t ldx, int m, int nx, double* Xt, int64_t ldt, hipStream_t st, const Batch& bt) {
    if (m <= 0 || nx <= 0 || bt.count <= 0) return hipSuccess;
    const dim3 grid((nx + TT - 1) / TT, (m + TT - 1) / TT, bt.count);
    if (grid.y > 65535u || grid.z > 65535u) return hipErrorInvalidValue;      // m <= 2^20: 32768 row tiles; at most 4096 members
    hipLaunchKernelGGL(k_tall_transpose, grid, dim3(TT, 8), 0, st, X, (long long)ldx, m, nx, Xt, (long long)ldt,
                       bt.count > 1 ? bt.stride : 0LL);
    return hipGetLastError();
}

// ---------------------------------------------------------------- set-up: W_s, E_x, t
// with_scales: W_s = z_s / x_s (i < m; the padding up to mk stays zero) and E_x = z_x / x_x (j < nx) from the iterate.
// t of right-hand side r (r < nrhs): T[r][i] = W_s[i] * r2[i] + r1[nx + i].
// EQ: the same over the ms `ub` rows alone -- only they carry a slack column, K is built from them, and t stays zero on the `eq`
// rows (nothing ever writes it there), so the pass X^T.t over the whole image sees the `ub` rows only.
template <bool EQ>
__global__ __launch_bounds__(256) void k_tall_setup(VecArgs a, TallArgs t, int with_scales, int nrhs, TallRhs rhs) {
    if (!tbatch(a, t, rhs)) return;
    const double *r1a = rhs.r1a, *r2a = rhs.r2a, *r1b = rhs.r1b, *r2b = rhs.r2b;
    const int stride = gridDim.x * 256;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < (EQ ? t.ms : a.m); i += stride) {
        double ws;
        if (with_scales) { ws = a.z[t.nx + i] / a.x[t.nx + i]; t.Ws[i] = ws; }
        else ws = t.Ws[i];
        if (nrhs > 0) t.T[i] = ws * r2a[i] + r1a[t.nx + i];
        if (nrhs > 1) t.T[a.mp + i] = ws * r2b[i] + r1b[t.nx + i];
    }
    if (with_scales)
        for (int j = blockIdx.x * 256 + threadIdx.x; j < t.nx; j += stride) t.Ex[j] = a.z[j] / a.x[j];
}
void tall_setup(const VecArgs& a, const TallArgs& t, bool with_scales, int nrhs, const double* r1a, const double* r2a,
                const double* r1b, const double* r2b, hipStream_t st) {
    hipLaunchKernelGGL(t.me > 0 ? k_tall_setup<true> : k_tall_setup<false>, dim3(a.nblk, 1, a.bcount), dim3(256), 0, st, a, t,
                       with_scales ? 1 : 0, nrhs, TallRhs{r1a, r2a, r1b, r2b});
}

// ---------------------------------------------------------------- right-hand side of the reduced solve
// G[r][j] = sum_s ATpart[s][r][j] - r1[j] for j < nx, 0 for nx <= j < nxp.  A workgroup takes 64 columns; its four waves
// take the four quarters of the row splits, each in index order, and the quarters are added as (w0 + w1) + (w2 + w3): a
// fixed order whatever the launch.  grid (64-column groups of nxp, right-hand sides, LPs).
__global__ __launch_bounds__(256) void k_tall_fold(VecArgs a, TallArgs t, int nrhs, TallRhs rhs) {
    if (!tbatch(a, t, rhs)) return;
    __shared__ double part[4][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int j = blockIdx.x * 64 + lane, r = blockIdx.y;
    const int per = (a.nsplit + 3) / 4;
    const int s0 = wave * per, s1 = s0 + per < a.nsplit ? s0 + per : a.nsplit;
    double s = 0.0;
    if (j < t.nx)
        for (int sp = s0; sp < s1; ++sp) s += a.ATpart[((long long)sp * nrhs + r) * t.npa + j];
    part[wave][lane] = s;
    __syncthreads();
    if (wave != 0 || j >= t.nxp) return;
    const double* r1 = r == 0 ? rhs.r1a : rhs.r1b;
    const double sum = (part[0][lane] + part[1][lane]) + (part[2][lane] + part[3][lane]);
    t.G[(long long)r * t.nxp + j] = j < t.nx ? sum - r1[j] : 0.0;
}
void tall_fold_rhs(const VecArgs& a, const TallArgs& t, int nrhs, const double* r1a, const double* r1b, hipStream_t st) {
    hipLaunchKernelGGL(k_tall_fold, dim3((t.nxp + 63) / 64, nrhs, a.bcount), dim3(256), 0, st, a, t, nrhs,
                       TallRhs{r1a, nullptr, r1b, nullptr});
}

// ---------------------------------------------------------------- epilogues
// Predictor: (p, q) from right-hand side 0, (u, v) from right-hand side 1.  u_x = G, u_s = Us; v = W_s * u_s + r1_s goes
// to R (q into R[0], v into R[1], as the dense solve leaves them) and q to a.q.  The four dots of delta.rs:29-32 go to
// the reduction slots 0 .. 3 and the NaN check of newton_equations.rs:190-194 sets FLAG_NAN_PQ, as k_pq_uv.
// EQ: n = nx + ms columns as above; of the ms + me rows the first ms are v_u = W_s * u_s + r1_s, the others v_e, which the Schur
// solve has left in Ve.  The same dots in the same slots, reduced in the same order.
template <bool EQ>
__global__ __launch_bounds__(256) void k_tall_pq_uv(VecArgs a, TallArgs t, TallRhs rhs) {
    if (!tbatch(a, t, rhs)) return;
    const double *r1a = rhs.r1a, *r1b = rhs.r1b;
    const int stride = gridDim.x * 256;
    double acc[4] = {0, 0, 0, 0};
    int nan = 0;
    for (int j = blockIdx.x * 256 + threadIdx.x; j < a.n; j += stride) {
        double p, u;
        if (j < t.nx) { p = t.G[j]; u = t.G[t.nxp + j]; }
        else          { p = t.Us[j - t.nx]; u = t.Us[a.mp + j - t.nx]; }
        const double cj = a.c[j];
        a.p[j] = p;
        a.u[j] = u;
        acc[0] += cj * p;
        acc[1] += cj * u;
        nan |= (p != p);
    }
    for (int i = blockIdx.x * 256 + threadIdx.x; i < a.m; i += stride) {
        const bool ub = !EQ || i < t.ms;
        const double ws = ub ? t.Ws[i] : 0.0, bi = a.b[i];
        const double q = ub ? ws * t.Us[i] + r1a[t.nx + i] : t.Ve[i - t.ms];
        const double v = ub ? ws * t.Us[a.mp + i] + r1b[t.nx + i] : t.Ve[t.mep + i - t.ms];
        a.q[i] = q;
        a.R[i] = q;
        a.R[a.mp + i] = v;
        acc[2] += bi * q;
        acc[3] += bi * v;
        nan |= (q != q);
    }
    if (nan) atomicOr(a.flags, FLAG_NAN_PQ);
    block_reduce_store<4, false>(acc, a.red, 0);
}
// Corrector: only (u, v) change (k_uv_corr): c.u and b.v into slots 0 and 1, v into R[0].
template <bool EQ>
__global__ __launch_bounds__(256) void k_tall_uv_corr(VecArgs a, TallArgs t, TallRhs rhs) {
    if (!tbatch(a, t, rhs)) return;
    const double* r1a = rhs.r1a;
    const int stride = gridDim.x * 256;
    double acc[2] = {0, 0};
    for (int j = blockIdx.x * 256 + threadIdx.x; j < a.n; j += stride) {
        const double u = j < t.nx ? t.G[j] : t.Us[j - t.nx];
        a.u[j] = u;
        acc[0] += a.c[j] * u;
    }
    for (int i = blockIdx.x * 256 + threadIdx.x; i < a.m; i += stride) {
        const double v = (!EQ || i < t.ms) ? t.Ws[i] * t.Us[i] + r1a[t.nx + i] : t.Ve[i - t.ms];
        a.R[i] = v;
        acc[1] += a.b[i] * v;
    }
    block_reduce_store<2, false>(acc, a.red, 0);
}
// W[r][j] += sum_s ZtPart[s][r][j], j < nxp, slabs in index order.  grid (256-column groups of nxp, right-hand sides, LPs).
__global__ __launch_bounds__(256) void k_tall_eq_add_w(VecArgs a, TallArgs t, int nrhs, double* W, const double* ZtPart) {
    TallRhs ptrs{W, ZtPart, nullptr, nullptr};       // (moved to the member with everything else)
    if (!tbatch(a, t, ptrs)) return;
    const int j = blockIdx.x * 256 + threadIdx.x, r = blockIdx.y;
    if (j >= t.nxp) return;
    double s = 0.0;
    for (int sp = 0; sp < t.mep / GEMVT_ROWS; ++sp) s += ptrs.r2a[((long long)sp * nrhs + r) * t.nxp + j];
    double* w = const_cast<double*>(ptrs.r1a);
    w[(long long)r * t.nxp + j] += s;
}
// More equality rows than columns: S = Zt.Zt^T has rank <= nx < me, so its pivot nx is zero in exact arithmetic whatever the
// data; rounding may leave it a tiny positive number.  The pivot-failure word gets what exact arithmetic gives (the first
// failure recorded wins, as in the factorisation).
__global__ void k_tall_eq_singular(VecArgs a, TallArgs t) {
    TallRhs none;
    if (!tbatch(a, t, none)) return;
    if (threadIdx.x == 0) atomicCAS((int*)a.potrf_info, 0, t.nx + 1);
}
void tall_eq_singular(const VecArgs& a, const TallArgs& t, hipStream_t st) {
    hipLaunchKernelGGL(k_tall_eq_singular, dim3(1, 1, a.bcount), dim3(64), 0, st, a, t);
}
void tall_eq_add_w(const VecArgs& a, const TallArgs& t, int nrhs, double* W, const double* ZtPart, hipStream_t st) {
    hipLaunchKernelGGL(k_tall_eq_add_w, dim3((t.nxp + 255) / 256, nrhs, a.bcount), dim3(256), 0, st, a, t, nrhs, W, ZtPart);
}
void tall_pq_uv(const VecArgs& a, const TallArgs& t, const double* r1a, const double* r1b, hipStream_t st) {
    hipLaunchKernelGGL(t.me > 0 ? k_tall_pq_uv<true> : k_tall_pq_uv<false>, dim3(a.nblk, 1, a.bcount), dim3(256), 0, st, a, t,
                       TallRhs{r1a, nullptr, r1b, nullptr});
}
void tall_uv_corr(const VecArgs& a, const TallArgs& t, const double* r1a, hipStream_t st) {
    hipLaunchKernelGGL(t.me > 0 ? k_tall_uv_corr<true> : k_tall_uv_corr<false>, dim3(a.nblk, 1, a.bcount), dim3(256), 0, st, a, t,
                       TallRhs{r1a, nullptr, nullptr, nullptr});
}

// ---------------------------------------------------------------- residuals at the current point
// k_residuals (residual.rs:22-31, feasible_point.rs:122-123) with the row-split slabs of A^T.y only npa wide: a structural
// column sums its slabs in index order, a slack column's A^T.y is y_i itself.  The same six partial sums in slots 0 .. 5.
__global__ __launch_bounds__(256) void k_tall_residuals(VecArgs a, TallArgs t) {
    TallRhs none;
    if (!tbatch(a, t, none)) return;
    const int stride = gridDim.x * 256;
    const double tau = a.S[S_TAU];
    double acc[6] = {0, 0, 0, 0, 0, 0};
    for (int i = blockIdx.x * 256 + threadIdx.x; i < a.m; i += stride) {
        double ax = a.Ax[i];
        for (int ch = 1; ch < a.ax_chunks; ++ch) ax += a.Ax[(long long)ch * a.mp + i];
        const double r = a.b[i] * tau - ax;
        a.rP[i] = r;
        acc[0] += r * r;
        acc[1] += a.b[i] * a.y[i];
    }
    for (int j = blockIdx.x * 256 + threadIdx.x; j < a.n; j += stride) {
        double aty = 0.0;
        if (j < t.nx) for (int s = 0; s < a.nsplit; ++s) aty += a.ATpart[(long long)s * t.npa + j];
        else aty = a.y[j - t.nx];
        const double xj = a.x[j], zj = a.z[j], cj = a.c[j];
        const double r = cj * tau - aty - zj;
        a.rD[j] = r;
        acc[2] += r * r;
        acc[3] += cj * xj;
        acc[4] += xj * zj;
        acc[5] += cj * (xj / tau);
    }
    block_reduce_store<6, false>(acc, a.red, 0);
}
void tall_residuals(const VecArgs& a, const TallArgs& t, hipStream_t st) {
    hipLaunchKernelGGL(k_tall_residuals, dim3(a.nblk, 1, a.bcount), dim3(256), 0, st, a, t);
}

}  // namespace lpipm
