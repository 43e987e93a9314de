// kernels_box.hip -- the vector stage of the bounded form (lpipm_upload_bounded).
//
// min c^T x, A_ub.x <= b_ub, A_eq.x = b_eq, 0 <= x, x_j <= u_j for the nb columns j of B.  What the iteration works on is the
// explicit LP with one row x_j + w_j = u_j and one slack column w_j per bound,
//   A_ext = [[A, 0], [E_B, I]],   x_ext = [x; w],   z_ext = [z; v],   y_ext = [y; y_b],
// at the extended lengths (a.n = na + nb, a.m = ma + nb) -- but its normal matrix stays ma x ma: the bound block of the
// Newton system is diagonal and is eliminated in closed form.  With dx = x / z, dw = w / v and, on a bounded column,
// s = dx + dw and D~ = 1 / (z / x + v / w) (D~ = dx elsewhere), sym_solve(r1, r2) (newton_equations.rs:214-225),
// r1 = [r1_x; r1_w], r2 = [r2_1; r2_2], reads
//   W_j   = D~_j (r1_x,j - r1_w,j) - (dx_j / s_j) r2_2,j          k_box_setup          (D~_j r1_x,j without a bound)
//   v_1   = M~^-1 (r2_1 + A.W),  M~ = A.diag(D~).A^T               the dense arm: gemv_n, Cholesky chain, super-block solves
//   t     = A^T.v_1                                                gemv_t, row-split slabs
//   g_j   = D~_j (t_j - r1_x,j + r1_w,j)
//   u_x,j = g_j + (dx_j / s_j) r2_2,j,   u_w,j = -g_j + (dw_j / s_j) r2_2,j        (u_x,j = D~_j (t_j - r1_x,j) without a bound)
//   v_2,j = r1_w,j + u_w,j / dw_j                                  k_box_pq_uv / k_box_uv_corr
// u_x and u_w both come from these lines: u_w = r2_2 - u_x cancels once a column sits at its bound, as the dense epilogue
// does on the tall form's slack block.  The bound block itself is never stored and never multiplied: a
// bound row of A_ext.x is x_j + w_j, a bounded column of A_ext^T.y adds y_b, a bound slack column's is y_b.
// Everything downstream (d_tau, Delta, ratio test, step, indicators) is the dense path's and sees p, q, u, v where it sees
// them there.  Reductions are fixed-order (kernels_vec.hip's two stages, the same slots).  The kernels run with gridDim.z =
// the LPs of the launch: bbatch moves the VecArgs, the BoxArgs and the right-hand sides to the member and skips a finished
// one, as vbatch and tbatch do; the index lists are the upload's and are moved with the member's arena like everything else.
// The kernels of the speculatively enqueued head test the done word.
//
// General column bounds (lpipm_upload_bounds) run the same kernels on the primed LP x_j = t_j + sigma_j x'_j,
//   A_ext = [[A', 0, -A'_F], [E_B, I, 0]],   x_ext = [x'; w; x^-],   z_ext = [z; v; z^-]   (a.n = na + nb + nf),
// with one more column x^- per free column j of F (disjoint from B).  On F, with dm = x^- / z^-,
//   D~_j = dx_j + dm_j,  W_j = dx_j r1_x,j - dm_j r1_m,j,  u_x,j = dx_j (t_j - r1_x,j),  u_m,j = dm_j (-t_j - r1_m,j),
// u_m from its own line.  The free block is never stored and never multiplied: a pass over A' reads the NET vector
// (k_box_net: x'_j - x^-_j on F) and the x^- column of A_ext^T.v is -(A'^T.v_1)_j.  Shifts and reflections happen at upload
// (k_box_reflect, the pass A.t) and on the way out (k_box_caller_units); with nf == 0 no kernel here takes an F branch.
#include "vec_kernels.hpp"
#include "vec_device.hpp"

namespace lpipm {

struct BoxRhs { const double *r1a = nullptr, *r2a = nullptr, *r1b = nullptr, *r2b = nullptr; };

__device__ __forceinline__ bool bbatch(VecArgs& a, BoxArgs& bx, BoxRhs& r) {
    const BatchK bk{a.bstride, nullptr, 0, a.bfirst};      // (taken before vbatch moves a's own fields)
    if (!vbatch(a, true)) return false;
    if (blockIdx.z == 0 && a.bfirst == 0) return true;
    bx.bidx = batch_ptr(bx.bidx, bk); bx.binv = batch_ptr(bx.binv, bk);
    bx.Dt = batch_ptr(bx.Dt, bk); bx.Rx = batch_ptr(bx.Rx, bk); bx.Rw = batch_ptr(bx.Rw, bk);
    bx.Wb = batch_ptr(bx.Wb, bk); bx.Rs = batch_ptr(bx.Rs, bk);
    bx.fidx = batch_ptr(bx.fidx, bk); bx.finv = batch_ptr(bx.finv, bk); bx.Xn = batch_ptr(bx.Xn, bk);
    bx.Sg = batch_ptr(bx.Sg, bk); bx.Tj = batch_ptr(bx.Tj, bk);
    r.r1a = batch_ptr(r.r1a, bk); r.r2a = batch_ptr(r.r2a, bk); r.r1b = batch_ptr(r.r1b, bk); r.r2b = batch_ptr(r.r2b, bk);
    return true;
}

// ---------------------------------------------------------------- set-up: D~, dx / s, dw / s, W
// with_scales: a.dinv holds x / z of all na + nb columns (k_pred_setup, the launch in front): D~ = dx on a column without a
// bound, 1 / (z_j / x_j + v_j / w_j) on a bounded one, whose dx / s and dw / s are kept for the epilogues.
// W of right-hand side r (r < nrhs) over the na columns of A; the padding of a row of Wb stays zero.
__global__ __launch_bounds__(256) void k_box_setup(VecArgs a, BoxArgs bx, int with_scales, int nrhs, BoxRhs rhs) {
    if (!bbatch(a, bx, rhs)) return;
    const double *r1a = rhs.r1a, *r2a = rhs.r2a, *r1b = rhs.r1b, *r2b = rhs.r2b;
    const int stride = gridDim.x * 256;
    for (int j = blockIdx.x * 256 + threadIdx.x; j < bx.na; j += stride) {
        const int k = bx.binv[j];
        const int kf = bx.nf > 0 ? bx.finv[j] : -1;
        if (kf >= 0) {       // a free column: D~ = dx + dm, W = dx r1_x - dm r1_m (a.dinv holds x / z throughout the iteration)
            const int jm = bx.na + bx.nb + kf;
            const double dx = a.dinv[j], dm = a.dinv[jm];
            if (with_scales) bx.Dt[j] = dx + dm;
            if (nrhs > 0) bx.Wb[j] = dx * r1a[j] - dm * r1a[jm];
            if (nrhs > 1) bx.Wb[bx.nps + j] = dx * r1b[j] - dm * r1b[jm];
            continue;
        }
        double dt, rx = 0.0;
        if (with_scales) {
            const double dx = a.dinv[j];
            if (k >= 0) {
                const int jw = bx.na + k;
                const double dw = a.dinv[jw], s = dx + dw;
                dt = 1.0 / (a.z[j] / a.x[j] + a.z[jw] / a.x[jw]);
                rx = dx / s;
                bx.Rx[k] = rx;
                bx.Rw[k] = dw / s;
            } else dt = dx;
            bx.Dt[j] = dt;
        } else {
            dt = bx.Dt[j];
            if (k >= 0) rx = bx.Rx[k];
        }
        if (k >= 0) {
            if (nrhs > 0) bx.Wb[j] = dt * (r1a[j] - r1a[bx.na + k]) - rx * r2a[bx.ma + k];
            if (nrhs > 1) bx.Wb[bx.nps + j] = dt * (r1b[j] - r1b[bx.na + k]) - rx * r2b[bx.ma + k];
        } else {
            if (nrhs > 0) bx.Wb[j] = dt * r1a[j];
            if (nrhs > 1) bx.Wb[bx.nps + j] = dt * r1b[j];
        }
    }
}
void box_setup(const VecArgs& a, const BoxArgs& bx, bool with_scales, int nrhs, const double* r1a, const double* r2a,
               const double* r1b, const double* r2b, hipStream_t st) {
    hipLaunchKernelGGL(k_box_setup, dim3(a.nblk, 1, a.bcount), dim3(256), 0, st, a, bx, with_scales ? 1 : 0, nrhs,
                       BoxRhs{r1a, r2a, r1b, r2b});
}

// ---------------------------------------------------------------- epilogues
// u_x, u_w and v_2 of one bounded column from t = (A^T.v_1)_j
struct BoxCol { double ux, uw, v2; };
__device__ __forceinline__ BoxCol box_col(double dt, double rx, double rw, double dw, double t, double r1x, double r1w, double r22) {
    const double g = dt * (t - r1x + r1w);
    BoxCol o;
    o.ux = g + rx * r22;
    o.uw = -g + rw * r22;
    o.v2 = r1w + o.uw / dw;
    return o;
}
// Predictor: (p, q) from right-hand side 0, (u, v) from right-hand side 1, the slabs of A^T.v_1 summed in index order.
// q goes to a.q and R[0], v to R[1], as the dense solve leaves them; the four dots of delta.rs:29-32 go to the reduction
// slots 0 .. 3 and the NaN check of newton_equations.rs:190-194 sets FLAG_NAN_PQ, as k_pq_uv.
__global__ __launch_bounds__(256) void k_box_pq_uv(VecArgs a, BoxArgs bx, BoxRhs rhs) {
    if (!bbatch(a, bx, rhs)) return;
    const double *r1a = rhs.r1a, *r2a = rhs.r2a, *r1b = rhs.r1b, *r2b = rhs.r2b;
    const int stride = gridDim.x * 256;
    double acc[4] = {0, 0, 0, 0};
    int nan = 0;
    for (int j = blockIdx.x * 256 + threadIdx.x; j < bx.na; j += stride) {
        double atq = 0.0, atv = 0.0;
        for (int s = 0; s < a.nsplit; ++s) {
            atq += a.ATpart[((long long)s * 2 + 0) * bx.nps + j];
            atv += a.ATpart[((long long)s * 2 + 1) * bx.nps + j];
        }
        const int k = bx.binv[j];
        const double dt = bx.Dt[j], cj = a.c[j];
        double p, u;
        if (k >= 0) {
            const int jw = bx.na + k, iw = bx.ma + k;
            const double rx = bx.Rx[k], rw = bx.Rw[k], dw = a.dinv[jw], cw = a.c[jw], bw = a.b[iw];
            const BoxCol P = box_col(dt, rx, rw, dw, atq, r1a[j], r1a[jw], r2a[iw]);
            const BoxCol U = box_col(dt, rx, rw, dw, atv, r1b[j], r1b[jw], r2b[iw]);
            p = P.ux; u = U.ux;
            a.p[jw] = P.uw;
            a.u[jw] = U.uw;
            a.q[iw] = P.v2;
            a.R[iw] = P.v2;
            a.R[a.mp + iw] = U.v2;
            acc[0] += cw * P.uw;
            acc[1] += cw * U.uw;
            acc[2] += bw * P.v2;
            acc[3] += bw * U.v2;
            nan |= (P.uw != P.uw) | (P.v2 != P.v2);
        } else if (bx.nf > 0 && bx.finv[j] >= 0) {      // free: u_x = dx (t - r1_x), u_m = dm (-t - r1_m), each from its own line
            const int jm = bx.na + bx.nb + bx.finv[j];
            const double dx = a.dinv[j], dm = a.dinv[jm], cm = a.c[jm];
            const double pm = dm * (-atq - r1a[jm]), um = dm * (-atv - r1b[jm]);
            p = dx * (atq - r1a[j]);
            u = dx * (atv - r1b[j]);
            a.p[jm] = pm;
            a.u[jm] = um;
            acc[0] += cm * pm;
            acc[1] += cm * um;
            nan |= (pm != pm);      // (the check is on p and q, as everywhere: newton_equations.rs:190-194)
        } else {
            p = dt * (atq - r1a[j]);
            u = dt * (atv - r1b[j]);
        }
        a.p[j] = p;
        a.u[j] = u;
        acc[0] += cj * p;
        acc[1] += cj * u;
        nan |= (p != p);
    }
    for (int i = blockIdx.x * 256 + threadIdx.x; i < bx.ma; i += stride) {
        const double q = bx.Rs[i], v = bx.Rs[bx.mps + i], bi = a.b[i];
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
__global__ __launch_bounds__(256) void k_box_uv_corr(VecArgs a, BoxArgs bx, BoxRhs rhs) {
    if (!bbatch(a, bx, rhs)) return;
    const double *r1a = rhs.r1a, *r2a = rhs.r2a;
    const int stride = gridDim.x * 256;
    double acc[2] = {0, 0};
    for (int j = blockIdx.x * 256 + threadIdx.x; j < bx.na; j += stride) {
        double atv = 0.0;
        for (int s = 0; s < a.nsplit; ++s) atv += a.ATpart[(long long)s * bx.nps + j];
        const int k = bx.binv[j];
        const double dt = bx.Dt[j];
        double u;
        if (k >= 0) {
            const int jw = bx.na + k, iw = bx.ma + k;
            const BoxCol U = box_col(dt, bx.Rx[k], bx.Rw[k], a.dinv[jw], atv, r1a[j], r1a[jw], r2a[iw]);
            u = U.ux;
            a.u[jw] = U.uw;
            a.R[iw] = U.v2;
            acc[0] += a.c[jw] * U.uw;
            acc[1] += a.b[iw] * U.v2;
        } else if (bx.nf > 0 && bx.finv[j] >= 0) {
            const int jm = bx.na + bx.nb + bx.finv[j];
            const double um = a.dinv[jm] * (-atv - r1a[jm]);
            u = a.dinv[j] * (atv - r1a[j]);
            a.u[jm] = um;
            acc[0] += a.c[jm] * um;
        } else u = dt * (atv - r1a[j]);
        a.u[j] = u;
        acc[0] += a.c[j] * u;
    }
    for (int i = blockIdx.x * 256 + threadIdx.x; i < bx.ma; i += stride) {
        const double v = bx.Rs[i];
        a.R[i] = v;
        acc[1] += a.b[i] * v;
    }
    block_reduce_store<2, false>(acc, a.red, 0);
}
void box_pq_uv(const VecArgs& a, const BoxArgs& bx, const double* r1a, const double* r2a, const double* r1b, const double* r2b,
               hipStream_t st) {
    hipLaunchKernelGGL(k_box_pq_uv, dim3(a.nblk, 1, a.bcount), dim3(256), 0, st, a, bx, BoxRhs{r1a, r2a, r1b, r2b});
}
void box_uv_corr(const VecArgs& a, const BoxArgs& bx, const double* r1a, const double* r2a, hipStream_t st) {
    hipLaunchKernelGGL(k_box_uv_corr, dim3(a.nblk, 1, a.bcount), dim3(256), 0, st, a, bx, BoxRhs{r1a, r2a, nullptr, nullptr});
}

// ---------------------------------------------------------------- residuals at the current point
// k_residuals (residual.rs:22-31, feasible_point.rs:122-123) on A_ext: the rows and columns of A from the passes over A (chunk
// slabs of A.x mps apart, row-split slabs of A^T.y nps wide, both in index order), a bound row r_P = u_j tau - x_j - w_j, a
// bounded column's A^T.y plus y_b, a bound slack column r_D = -y_b - v.  The same six partial sums in slots 0 .. 5.
__global__ __launch_bounds__(256) void k_box_residuals(VecArgs a, BoxArgs bx) {
    BoxRhs none;
    if (!bbatch(a, bx, none)) return;
    const int stride = gridDim.x * 256;
    const double tau = a.S[S_TAU];
    double acc[6] = {0, 0, 0, 0, 0, 0};
    for (int i = blockIdx.x * 256 + threadIdx.x; i < a.m; i += stride) {
        double ax;
        if (i < bx.ma) {
            ax = a.Ax[i];
            for (int ch = 1; ch < a.ax_chunks; ++ch) ax += a.Ax[(long long)ch * bx.mps + i];
        } else {
            const int k = i - bx.ma;
            ax = a.x[bx.bidx[k]] + a.x[bx.na + k];
        }
        const double r = a.b[i] * tau - ax;
        a.rP[i] = r;
        acc[0] += r * r;
        acc[1] += a.b[i] * a.y[i];
    }
    for (int j = blockIdx.x * 256 + threadIdx.x; j < a.n; j += stride) {
        double aty = 0.0;
        if (j < bx.na) {
            for (int s = 0; s < a.nsplit; ++s) aty += a.ATpart[(long long)s * bx.nps + j];
            const int k = bx.binv[j];
            if (k >= 0) aty += a.y[bx.ma + k];
        } else if (j < bx.na + bx.nb) aty = a.y[bx.ma + j - bx.na];
        else {               // the x^- column of free column f: A_ext's column is -a'_f (c[j] holds -c'_f)
            const int f = bx.fidx[j - bx.na - bx.nb];
            for (int s = 0; s < a.nsplit; ++s) aty += a.ATpart[(long long)s * bx.nps + f];
            aty = -aty;
        }
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
void box_residuals(const VecArgs& a, const BoxArgs& bx, hipStream_t st) {
    hipLaunchKernelGGL(k_box_residuals, dim3(a.nblk, 1, a.bcount), dim3(256), 0, st, a, bx);
}

// ---------------------------------------------------------------- the structural bound block of the passes
// What the passes over A leave, folded in index order and completed by the bound block, which is never stored:
//   (A_ext.w)_i   = sum of the chunk slabs of A.w_x (i < ma);  w_x[B_k] + w_w,k on bound row k
//   (A_ext^T.v)_j = sum of the row-split slabs of A^T.v_1 (+ v_2,k on a bounded column);  v_2,k on bound slack column k
// Either half is skipped when its output is null.  No done test: the kernel entries and the certificates of a finished solve.
__global__ __launch_bounds__(256) void k_box_products(VecArgs a, BoxArgs bx, BoxProducts q) {
    const BatchK bk{a.bstride, nullptr, 0, a.bfirst};
    q.w = batch_ptr(q.w, bk); q.AxPart = batch_ptr(q.AxPart, bk); q.Aw = batch_ptr(q.Aw, bk);
    q.v = batch_ptr(q.v, bk); q.ATpart = batch_ptr(q.ATpart, bk); q.ATv = batch_ptr(q.ATv, bk);
    bx.bidx = batch_ptr(bx.bidx, bk); bx.binv = batch_ptr(bx.binv, bk); bx.fidx = batch_ptr(bx.fidx, bk);
    const int stride = gridDim.x * 256;
    if (q.Aw)
        for (int i = blockIdx.x * 256 + threadIdx.x; i < a.m; i += stride) {
            double s;
            if (i < bx.ma) {
                s = q.AxPart[i];
                for (int ch = 1; ch < q.ax_chunks; ++ch) s += q.AxPart[(long long)ch * bx.mps + i];
            } else {
                const int k = i - bx.ma;
                s = q.w[bx.bidx[k]] + q.w[bx.na + k];
            }
            q.Aw[i] = s;
        }
    if (q.ATv)
        for (int j = blockIdx.x * 256 + threadIdx.x; j < a.n; j += stride) {
            double s = 0.0;
            if (j < bx.na) {
                for (int sp = 0; sp < a.nsplit; ++sp) s += q.ATpart[(long long)sp * q.slab_stride + j];
                const int k = bx.binv[j];
                if (k >= 0) s += q.v[bx.ma + k];
            } else if (j < bx.na + bx.nb) s = q.v[bx.ma + j - bx.na];
            else {
                const int f = bx.fidx[j - bx.na - bx.nb];
                for (int sp = 0; sp < a.nsplit; ++sp) s += q.ATpart[(long long)sp * q.slab_stride + f];
                s = -s;
            }
            q.ATv[j] = s;
        }
}
void box_products(const VecArgs& a, const BoxArgs& bx, const BoxProducts& q, hipStream_t st) {
    hipLaunchKernelGGL(k_box_products, dim3(a.nblk, 1, a.bcount), dim3(256), 0, st, a, bx, q);
}

// Equilibration: the bound row of column j gets kr = -kc[j] and its slack column kc = kc[j], so that the block's entries stay
// exactly 1 (and unstored); u_j <- ldexp(u_j, -kc[j]) then follows from the scaling of b_ext by kr.
__global__ __launch_bounds__(256) void k_box_exponents(BoxArgs bx, int32_t* __restrict__ kr, int32_t* __restrict__ kc) {
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k < bx.nb) {
        const int e = kc[bx.bidx[k]];
        kr[bx.ma + k] = -e;
        kc[bx.na + k] = e;
    }
    if (k < bx.nf) kc[bx.na + bx.nb + k] = kc[bx.fidx[k]];     // the x^- column is its column's negative: the same exponent
}
void box_exponents(const BoxArgs& bx, int32_t* kr, int32_t* kc, hipStream_t st) {
    const int most = bx.nb > bx.nf ? bx.nb : bx.nf;
    if (most > 0) hipLaunchKernelGGL(k_box_exponents, dim3((most + 255) / 256), dim3(256), 0, st, bx, kr, kc);
}

// ---------------------------------------------------------------- general bounds: net vectors, reflection, caller's variables
// The net vector of `rows` extended rows: what a pass over A reads where the explicit form would read [x'; x^-] against
// [A', -A'_F].  check_done: the launch belongs to an iteration (the residual pair's).
__global__ __launch_bounds__(256) void k_box_net(VecArgs a, BoxArgs bx, const double* src, long long lds, double* dst, long long ldd,
                                                 int rows, int check_done) {
    const BatchK bk{a.bstride, check_done ? a.done_chk : nullptr, 0, a.bfirst};
    if (batch_done(bk)) return;
    src = batch_ptr(src, bk); dst = batch_ptr(dst, bk); bx.finv = batch_ptr(bx.finv, bk);
    const int stride = gridDim.x * 256;
    for (int j = blockIdx.x * 256 + threadIdx.x; j < bx.na; j += stride) {
        const int kf = bx.finv[j];
        for (int r = 0; r < rows; ++r) {
            const double* s = src + r * lds;
            dst[r * ldd + j] = kf >= 0 ? s[j] - s[bx.na + bx.nb + kf] : s[j];
        }
    }
}
void box_net(const VecArgs& a, const BoxArgs& bx, const double* src, long long lds, double* dst, long long ldd, int rows,
             bool check_done, hipStream_t st) {
    hipLaunchKernelGGL(k_box_net, dim3(a.nblk, 1, a.bcount), dim3(256), 0, st, a, bx, src, lds, dst, ldd, rows, check_done ? 1 : 0);
}

// A' = A.diag(sigma): the stored structural columns of N negated in the resident image (exact), ahead of the equilibration.
__global__ __launch_bounds__(256) void k_box_reflect(BoxArgs bx, double* __restrict__ A, long long lda, int nx) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= nx || !(bx.Sg[j] < 0.0)) return;
    for (int i = blockIdx.y; i < bx.ma; i += gridDim.y) A[(long long)i * lda + j] = -A[(long long)i * lda + j];
}
void box_reflect(const BoxArgs& bx, double* A, long long lda, int nx, hipStream_t st) {
    const int gy = bx.ma < 1024 ? bx.ma : 1024;
    hipLaunchKernelGGL(k_box_reflect, dim3((nx + 255) / 256, gy), dim3(256), 0, st, bx, A, lda, nx);
}

// One output row of a.n extended entries into the caller's variables, in place (see BOX_OUT_*), one LP.  Only the structural
// entries change: sigma is +1 and t is 0 on every `ub` slack column, and w, x^- keep their places.
__global__ __launch_bounds__(256) void k_box_caller_units(VecArgs a, BoxArgs bx, double* row, int mode) {
    const BatchK bk{a.bstride, nullptr, 0, a.bfirst};
    bx.finv = batch_ptr(bx.finv, bk); bx.Sg = batch_ptr(bx.Sg, bk); bx.Tj = batch_ptr(bx.Tj, bk);
    if (mode == BOX_OUT_CERT) {
        const int kind = (int)batch_ptr(a.red, bk)[2 * RED_STRIDE + 1];
        if (kind == 0) return;
        mode = kind == 1 ? BOX_OUT_Z : BOX_OUT_RAY;
    }
    const int stride = gridDim.x * 256;
    for (int j = blockIdx.x * 256 + threadIdx.x; j < bx.na; j += stride) {
        const double sg = bx.Sg[j], v = row[j];
        const int kf = bx.nf > 0 ? bx.finv[j] : -1;
        if (mode == BOX_OUT_Z) row[j] = sg * v;
        else {
            const double net = kf >= 0 ? v - row[bx.na + bx.nb + kf] : sg * v;
            row[j] = mode == BOX_OUT_X ? bx.Tj[j] + net : net;
        }
    }
}
void box_caller_units(const VecArgs& a, const BoxArgs& bx, double* row, int mode, hipStream_t st) {
    hipLaunchKernelGGL(k_box_caller_units, dim3(a.nblk, 1, 1), dim3(256), 0, st, a, bx, row, mode);
}

}  // namespace lpipm
