// vec_kernels.hpp -- argument block, scalar-slot indices and launchers of kernels_vec.hip.
#pragma once
#include "lpipm_internal.hpp"

namespace lpipm {

constexpr int RED_STRIDE = 512;  // max workgroups of a vector kernel == partials per reduction slot
constexpr int RED_SLOTS  = 8;

// device scalar block S
enum {
    S_TAU = 0, S_KAPPA, S_MU, S_RG, S_GAMMA, S_ETA, S_RHAT_G, S_RHAT_TK, S_DTAU, S_DKAPPA,
    S_ALPHA_PRED, S_ALPHA, S_CP, S_BQ, S_RP0, S_RD0, S_RG0, S_RMU0,
    S_C0,   // the constant of the objective (written at upload; every LP of a batch has its own)
    S_COUNT
};
enum { ST_OPTIMAL = 0, ST_INFEASIBLE = 1, ST_UNBOUNDED = 2, ST_UNFINISHED = 3 };  // indicators.rs:85-90
enum { FLAG_NAN_PQ = 1 };
// Selective refinement (LPIPM_REFINE=1, a measurement mode; the default, LPIPM_REFINE unset, refines nothing; =2 refines every solve): the Cholesky solves of an
// iteration are refined when mu / mu_0 of the point the normal equations are formed at is at most this.  The decision is
// the LP's own (device word skip_refine, mirrored by the host from the status record): the same alone and in a batch.
constexpr double REFINE_BELOW_RHO_MU = 1e-2;
double refine_below();   // REFINE_BELOW_RHO_MU, or LPIPM_REFINE_BELOW from the environment (measurement knob)

// read back once per iteration (96 bytes)
struct StatusRec {
    double alpha, rho_p, rho_d, rho_A, rho_g, rho_mu, obj, tau, kappa;
    int32_t status, potrf_info, flags, pad_;
};

struct VecArgs {
    int n, m, np, mp, nblk, nsplit;
    long long n_total;   // columns of the WHOLE LP (== n unless the LP is split by columns over ranks)
    double* gs;          // n-split mode: globally reduced sums / mins the scalar kernels read instead of `red`
    // problem
    const double *b, *c;
    // iterate
    double *x, *y, *z;
    // work vectors (n-sized: np doubles; m-sized: mp doubles)
    double *dinv, *xs, *r1, *rD, *p, *u, *dx, *dz, *dxdz;   // n
    double *rP, *rP2, *q, *dy, *Ax;                          // m
    double *W;        // [2][np]  gemv_n inputs
    double *R;        // [2][mp]  gemv_n outputs / solve in-out
    const double* ATpart;  // [nsplit][nrhs][np] gemv_t slabs
    double *S, *red;
    StatusRec* status;
    StatusRec* status_pinned;   // nullable: the context's coherent pinned host array, one record per LP of the launch (dense, index
                                //   blockIdx.z).  The kernels that write `status` write the record here too -- payload, system
                                //   fence, then the sequence word pad_ -- so the host can wait for an iteration by watching pad_:
                                //   no D2H copy launch and no event record between the indicators and the next A.D.A^T
    int status_seq;             // what pad_ is set to by the launch this argument block goes to
    int32_t *potrf_info;
    int *flags;
    int *skip_refine; // set by k_scalar_indicators: 1 = the refinement step of this LP's Cholesky solves is skipped in the next
                      //   iteration (the LP has finished, or its normal equations are still well conditioned)
    int *done;        // set by k_scalar_indicators when the LP has reached a final status; cleared by k_blind_start
    const int *done_chk;  // what the kernels of the iteration test before doing anything (nullptr: no test)
    int ax_chunks;    // Ax holds this many slabs of mp doubles whose sum is A.x (1: a plain gemv_n result)
    double refine_below;  // threshold of skip_refine (refine_below())
    int bcount;       // lockstep batch: LPs per launch (gridDim.z); every pointer above is LP 0's,
    long long bstride;//   LP z's is bstride bytes * z further
    int bfirst;       // the launch covers the LPs [bfirst, bfirst + bcount) of the resident batch
};

// n-split mode (a.gs != nullptr): between a vector kernel and the scalar kernel that consumes its
// partial sums, the sums over the split dimension are folded into a.gs and handed to `xr` for the
// cross-rank reduction (op 0 = sum, 1 = min); xr == nullptr / a.gs == nullptr: single-GPU path.
struct XRank {
    int (*fn)(void* self, double* dev_ptr, int count, int op);
    void* self;
};
void vec_blind_start(const VecArgs& a, hipStream_t st);
// with_pred (only where vec_fused(a) holds and xr is null): the launch also does vec_pred_setup for the next iteration
int  vec_residuals(const VecArgs& a, int is_init, int ip_next, double tol, hipStream_t st, const XRank* xr = nullptr,
                   bool with_pred = false);
// the scalar half of vec_residuals' kernel-by-kernel path on its own: for a residual kernel that is not k_residuals (tall form)
void vec_scalar_indicators(const VecArgs& a, int is_init, int ip_next, double tol, hipStream_t st);
void vec_pred_setup(const VecArgs& a, hipStream_t st);
int  vec_pq_uv(const VecArgs& a, hipStream_t st, const XRank* xr = nullptr);
int  vec_uv_corr(const VecArgs& a, hipStream_t st, const XRank* xr = nullptr);
int  vec_delta(const VecArgs& a, int phase, int ip, double alpha0, hipStream_t st, const XRank* xr = nullptr);
void vec_corr_setup(const VecArgs& a, int ip, hipStream_t st);
void vec_step(const VecArgs& a, int ip, double alpha0, hipStream_t st);
// one launch for a run of the kernels above (kernels_vec.hip, "fused vector stage"): vec_fused(a) says whether they apply
bool vec_fused(const VecArgs& a);
void vec_fused_predictor(const VecArgs& a, int ip, hipStream_t st);                  // vec_pq_uv + vec_delta(0) + vec_corr_setup
void vec_fused_corrector(const VecArgs& a, int ip, double alpha0, hipStream_t st);   // vec_uv_corr + vec_delta(1) + vec_step
int  vec_final_x(const VecArgs& a, double* xout, hipStream_t st, const XRank* xr = nullptr);
// The duals of the iterate the arena holds (lpipm_get_duals[_device]): for every member k of the launch whose mask word is
// set, y / tau (m entries) and z / tau (n entries) of the resident problem taken to the caller's units -- y_i by kr[i], z_j by
// -kc[j] (ScaleBuf's exponents, set k's estride * k further; kr null: unscaled) -- into row k - row0 of y (ldy doubles per
// row) and of z (ldz), either of which may be null, and {b.(y / tau) + c0, tau, kappa} into the 3 doubles of row k - row0 of
// info.  a is the resident batch's (bfirst 0, bcount = its count): the grid over a member is a.nblk workgroups whatever the
// count, so the sum has the same bits from a single LP and from any batch.  Reduction slot 0 is used; the iterate is only read.
struct DualsOut {
    double* y; long long ldy;
    double* z; long long ldz;
    double* info;
    long long row0;
    const int32_t* mask;
    const int32_t *kr, *kc; long long estride;
};
void vec_final_duals(const VecArgs& a, const DualsOut& d, hipStream_t st);
// The certificate of the iterate the arena holds (lpipm_get_certificate[_device]).  mask[k] says what member k of the resident
// batch is asked for: CERT_ASK_NOT (skipped by every kernel), CERT_ASK_PLAIN (a status without a certificate: only its info
// record is written), CERT_ASK_INFEASIBLE, CERT_ASK_UNBOUNDED.  vec_cert_rays: s = b.y, respectively -c.x (slots 0 and 1 folded
// in fold_sum's order), kind (1 Farkas, 2 ray, 0 when s <= 0) into slot 2; y^ = y / s into dy, z^ = z / s into dz, x^ = x / s
// into row 0 of W (zeros for the ray the member has not), and to row k - row0 of y (Farkas only) and col (z^, respectively x^) in
// the caller's units: y^ by kr, z^ by -kc, x^ by kc.  The caller then passes over A with W and dy (a.ax_chunks set), and
// vec_cert_residual takes max_j |A^T.y^ + z^| by -kc (the first nxs columns from row-split slabs `slab` doubles wide, the
// columns behind them from y^: a tall form's slack block) or max_i |A.x^| by -kr into slot 3, and writes CERT_INFO_DOUBLES per
// row of info: {s, residual, tau, kappa, kind}, s and residual NaN for CERT_ASK_PLAIN, residual NaN for kind 0.  The grid over
// a member is a.nblk workgroups whatever the count.  Written in the arena: slots 0-3, dy, dz, W below m and n.
enum { CERT_ASK_NOT = 0, CERT_ASK_PLAIN = 1, CERT_ASK_INFEASIBLE = 2, CERT_ASK_UNBOUNDED = 3 };
constexpr int CERT_INFO_DOUBLES = 5;
struct CertOut {
    double* y; long long ldy;
    double* col; long long ldc;
    double* info;
    long long row0;
    const int32_t* mask;
    const int32_t *kr, *kc; long long estride;
    int nxs; long long slab;
};
void vec_cert_rays(const VecArgs& a, const CertOut& d, hipStream_t st);
void vec_cert_residual(const VecArgs& a, const CertOut& d, hipStream_t st);
// Y[q][i] += add_q[i] (i < m): the addend of a column-split A.w after its cross-rank sum
// packed has mp*(mp+128)/2 doubles; dir 0 = M -> packed, 1 = packed -> M (mp a multiple of 128, ld even)
void vec_pack_lower(double* M, long long ld, int mp, double* packed, int dir, hipStream_t st);
void vec_add_rows(int m, int nrhs, double* Y, long long ldy, const double* add0, const double* add1, hipStream_t st);
// tiles[t] = (ti, tj): packed[t][128][128] <-> the 128 x 128 tile of M at (ti, tj); dir 0 = M -> packed, 1 = packed -> M
void vec_pack_tiles(double* M, long long ld, const int2* tiles, int ntiles, double* packed, int dir, hipStream_t st);
// refined Cholesky solve (solver.hip): dst[q][0:mp] = / += src[q][0:mp]; M0 <- lower block-triangle of M
void vec_rows_copy(int mp, int nrhs, double* dst, const double* src, hipStream_t st, const Batch& bt = Batch{});
void vec_rows_add(int mp, int nrhs, double* dst, const double* src, hipStream_t st, const Batch& bt = Batch{});
void vec_copy_lower(const double* M, double* M0, long long ld, int mp, hipStream_t st, const Batch& bt = Batch{});
// Up to SCATTER_SEGS packed row blocks into the arenas in one launch: member z of the launch gets src[z * ld .. + len) at its
// dst (dst is LP 0's pointer; ld in elements, 0 = the same row for every member).  A segment with a null dst is skipped.
// Members are written whether finished or not (lpipm_update_lockstep_vectors; the shared first factor's pivot word).
constexpr int SCATTER_SEGS = 3;
template <typename T> struct ScatterSeg { T* dst = nullptr; const T* src = nullptr; long long ld = 0; int len = 0; };
template <typename T> struct ScatterRows { ScatterSeg<T> seg[SCATTER_SEGS]; };
template <typename T> void vec_scatter_rows(const ScatterRows<T>& a, hipStream_t st, const Batch& bt);

// ---------------------------------------------------------------- tall inequality form (kernels_tall.hip)
// A pure-`ub` LP with many more rows than columns (lpipm_upload_ub_tall): A = [X I], X m x nx.  The Newton system is reduced
// to the nx x nx SPD matrix K = X^T.diag(W_s).X + diag(E_x), W_s = z_s / x_s, E_x = z_x / x_x, and sym_solve(r1, r2)
// (newton_equations.rs:214-225) becomes
//   t = W_s*r2 + r1_s;  g = X^T.t - r1_x;  u_x = K^-1 g;  u_s = r2 - X.u_x;  v = W_s*u_s + r1_s;  u = [u_x; u_s]
// What the kernels of a tall LP work in, next to its VecArgs.  Every pointer is LP 0's, as in VecArgs: member z of a lockstep
// batch has its own bstride bytes * z further (tbatch, vec_device.hpp).
struct TallArgs {
    int nx, npa, nxp, mk;    // structural columns, their count padded to 16 (lda of X), to 128 (order of K), m padded to 16
    double* Ws;              // [mk]      W_s, zeros beyond m: the `dinv` of the A.D.A^T launch that builds K
    double* Ex;              // [nxp]     E_x, added to K's diagonal
    double* T;               // [2][mp]   t of both right-hand sides: the V of gemv_t
    double* G;               // [2][nxp]  g, then u_x: in/out of the Cholesky solve, the W of gemv_n
    double* Us;              // [2][mp]   u_s, from gemv_n (alpha = -1, addend r2)
    // Equality rows (lpipm_upload_ub_eq_tall; me == 0 on every other tall upload, whose kernels read none of these): the image
    // is [X; A_eq], a.m = ms + me rows of which the first ms carry a slack column; K is built from the ms `ub` rows alone.
    int ms, me, mep;         // `ub` rows (= slack columns), `eq` rows, their count padded to 128 (order of S)
    double* Ve;              // [2][mep]  v_e = S^-1.h of both right-hand sides, zeros beyond me
};
// The right-hand sides a tall launch is handed: (r1a, r2a) and (r1b, r2b), r1 n-sized, r2 m-sized, LP 0's addresses in the
// arena (or, for the single LP of the kernel entries, any device buffer); the unused ones are null.
struct TallRhs { const double *r1a = nullptr, *r2a = nullptr, *r1b = nullptr, *r2b = nullptr; };
// Xt (nxp x mk, zeroed beforehand) = X^T for the m x nx block of the resident X (lda = npa); bt: the members of a batch
// that own their matrices (X and Xt are member 0's, the others bt.stride bytes apart), one launch for all
hipError_t tall_transpose(const double* X, int64_t ldx, int m, int nx, double* Xt, int64_t ldt, hipStream_t st,
                          const Batch& bt = Batch{});
// W_s and E_x from the iterate (with_scales), and t for nrhs (0|1|2) right-hand sides (r1a, r2a), (r1b, r2b): r1 n-sized, r2 m-sized
void tall_setup(const VecArgs& a, const TallArgs& t, bool with_scales, int nrhs, const double* r1a, const double* r2a,
                const double* r1b, const double* r2b, hipStream_t st);
// G[r][j] = sum over the row splits of ATpart[s][r][j] (slabs npa wide, in order) - r1{a,b}[j], j < nx; zeros up to nxp
void tall_fold_rhs(const VecArgs& a, const TallArgs& t, int nrhs, const double* r1a, const double* r1b, hipStream_t st);
// Tall counterparts of vec_pq_uv / vec_uv_corr (single GPU: d_tau is folded into k_delta): p, q, u, v -- v into R as the
// dense path leaves it --, the same dots in the same reduction slots, FLAG_NAN_PQ.
void tall_pq_uv(const VecArgs& a, const TallArgs& t, const double* r1a, const double* r1b, hipStream_t st);
void tall_uv_corr(const VecArgs& a, const TallArgs& t, const double* r1a, hipStream_t st);
// (tall_setup, tall_pq_uv and tall_uv_corr launch their kernel's EQ instantiation when t.me > 0: slack quantities over ms, row
// quantities over ms + me with v_e from Ve.)
// Equality rows: W[r][j] += sum over the row splits of ZtPart[s][r][j] (slabs nxp wide, in order), j < nxp: the correction
// Zt^T.v_e of the half-solved right-hand side w = L^-1.g
void tall_eq_add_w(const VecArgs& a, const TallArgs& t, int nrhs, double* W, const double* ZtPart, hipStream_t st);
// me > nx: S is singular by construction (rank <= nx); records the failed pivot nx of exact arithmetic in potrf_info
void tall_eq_singular(const VecArgs& a, const TallArgs& t, hipStream_t st);
// k_residuals for slabs of A^T.y that are npa wide: the slack columns' A^T.y is y itself (what slab 0 holds on the dense
// path, next to zeros: the same bits).  Followed by vec_scalar_indicators.
void tall_residuals(const VecArgs& a, const TallArgs& t, hipStream_t st);

// ---------------------------------------------------------------- bounded form (kernels_box.hip)
// An LP of lpipm_upload_ub_eq with upper bounds on nb of its structural columns (lpipm_upload_bounded).  What is solved is the
// explicit LP A_ext = [[A, 0], [E_B, I]], x_ext = [x; w], y_ext = [y; y_b]: the VecArgs carry the extended lengths (n = na + nb,
// m = ma + nb, np and mp their paddings), the resident image and the normal system stay those of A (ma rows, na columns with
// its slack block).  The bound block is eliminated in closed form: M~ = A.diag(D~).A^T, D~_j = 1 / (z_j / x_j + v_j / w_j) on
// a bounded column and x_j / z_j elsewhere, and sym_solve(r1, r2), r1 = [r1_x; r1_w], r2 = [r2_1; r2_2], reads
//   W_j  = D~_j (r1_x,j - r1_w,j) - (dx_j / s_j) r2_2,j   (j bounded, s = dx + dw;  D~_j r1_x,j elsewhere)     k_box_setup
//   v_1  = M~^-1 (r2_1 + A.W);   t = A^T.v_1                                                        the dense arm's passes
//   g_j  = D~_j (t_j - r1_x,j + r1_w,j);  u_x,j = g_j + (dx_j / s_j) r2_2,j;  u_w,j = -g_j + (dw_j / s_j) r2_2,j
//   v_2,j = r1_w,j + u_w,j / dw_j                                                            k_box_pq_uv / k_box_uv_corr
// Every pointer is LP 0's, as in VecArgs (bbatch, kernels_box.hip, moves them to the member).
struct BoxArgs {
    int nb, na, ma;          // bounded columns; columns and rows of A's slack form (the VecArgs' n - nb and m - nb)
    int nps, mps;            // na padded to 256: width of the A^T.v slabs and of a row of Wb; ma padded to 128: order of M~, row of Rs
    const int* bidx;         // [nb]     the bounded columns, ascending
    const int* binv;         // [na]     k where bidx[k] == j, -1 on a column without a bound
    double* Dt;              // [nps]    D~: the `dinv` of the A.D.A^T launch that builds M~
    double* Rx;              // [nb]     dx / s
    double* Rw;              // [nb]     dw / s
    double* Wb;              // [2][nps] W: the input of the pass A.W
    double* Rs;              // [2][mps] r2_1 + A.W, then v_1: in/out of the Cholesky solve, the V of the pass A^T.v
    // General column bounds (lpipm_upload_bounds): the iteration sees the primed LP x_j = t_j + sigma_j x'_j, with one more
    // column x^-_j (A_ext column -a'_j, cost -c'_j) per free column j of F: x_ext = [x'; w; x^-], n = na + nb + nf.  On F
    //   D~_j = dx_j + dm_j,  W_j = dx_j r1_x,j - dm_j r1_m,j,  u_x,j = dx_j (t_j - r1_x,j),  u_m,j = dm_j (-t_j - r1_m,j)
    // (dm = x^- / z^-), the passes over A read the NET vector (x_j - x^-_j on F), and the x^- column of A_ext^T.v is
    // -(A^T.v_1)_j.  All zero / null on the bounded form itself.
    int nf;                  // free columns
    int gen;                 // a general upload: Sg and Tj are there (a reflection or a shift), and Xn when nf > 0
    const int* fidx;         // [nf]     the free columns, ascending
    const int* finv;         // [na]     k where fidx[k] == j, -1 on every other column
    double* Xn;              // [nps]    the net vector the residual pair's pass over A reads
    const double* Sg;        // [nps]    sigma_j: -1 on a reflected column, +1 elsewhere (0 in the padding)
    const double* Tj;        // [nps]    t_j in the caller's units: lower_j, or upper_j on a reflected column; 0 on F and the slacks
};
// D~, dx / s and dw / s from the iterate (with_scales: a.dinv holds x / z over all n columns, from k_pred_setup), and W for
// nrhs (0|1|2) right-hand sides (r1a, r2a), (r1b, r2b): r1 n-sized, r2 m-sized
void box_setup(const VecArgs& a, const BoxArgs& bx, bool with_scales, int nrhs, const double* r1a, const double* r2a,
               const double* r1b, const double* r2b, hipStream_t st);
// Bounded counterparts of vec_pq_uv / vec_uv_corr (single GPU: d_tau is folded into k_delta): p, q, u, v where the dense
// kernels leave them (q into R[0], v into R[1]; corrector: v into R[0]), the same dots in the same slots, FLAG_NAN_PQ.
void box_pq_uv(const VecArgs& a, const BoxArgs& bx, const double* r1a, const double* r2a, const double* r1b, const double* r2b,
               hipStream_t st);
void box_uv_corr(const VecArgs& a, const BoxArgs& bx, const double* r1a, const double* r2a, hipStream_t st);
// k_residuals with the bound rows and columns: A.x chunk slabs mps apart, A^T.y slabs nps wide.  Followed by vec_scalar_indicators.
void box_residuals(const VecArgs& a, const BoxArgs& bx, hipStream_t st);
// The structural bound block of the passes over A (the kernel entries, the certificates): Aw (m entries) = A_ext.w from the
// ax_chunks chunk slabs of A.w_x (mps apart) and w itself (n entries); ATv (n entries) = A_ext^T.v from the row-split slabs
// of A^T.v_1 (slab_stride doubles apart) and v itself (m entries).  A null output skips its half.  LP 0's pointers.
struct BoxProducts {
    const double* w = nullptr; const double* AxPart = nullptr; int ax_chunks = 1; double* Aw = nullptr;
    const double* v = nullptr; const double* ATpart = nullptr; long long slab_stride = 0; double* ATv = nullptr;
};
void box_products(const VecArgs& a, const BoxArgs& bx, const BoxProducts& q, hipStream_t st);
// kr of the bound rows and kc of the bound slack columns from kc of the bounded columns (one exponent set: a single LP);
// the x^- column of a free column takes its column's kc
void box_exponents(const BoxArgs& bx, int32_t* kr, int32_t* kc, hipStream_t st);
// General bounds.  box_net: dst[j] = src[j] - src[na + nb + finv[j]] on F, src[j] elsewhere, j < na, for each of `rows` rows
// (lds, ldd doubles apart): what a pass over A is handed in place of an extended vector.  check_done: the solve's own launch.
void box_net(const VecArgs& a, const BoxArgs& bx, const double* src, long long lds, double* dst, long long ldd, int rows,
             bool check_done, hipStream_t st);
// Upload time, on the unscaled image (lda doubles a row, nx structural columns, ma rows): the columns of N negated.
void box_reflect(const BoxArgs& bx, double* A, long long lda, int nx, hipStream_t st);
// An output row of n extended entries into the caller's variables, in place, behind the column unscaling:
//   BOX_OUT_X: x_j = t_j + sigma_j x'_j (x'_j - x^-_j on F);  BOX_OUT_RAY: the same without t;  BOX_OUT_Z: z_j = sigma_j z'_j;
//   BOX_OUT_CERT: RAY or Z as the certificate's kind in the reduction block says (nothing without a certificate).
enum { BOX_OUT_X = 0, BOX_OUT_RAY, BOX_OUT_Z, BOX_OUT_CERT };
void box_caller_units(const VecArgs& a, const BoxArgs& bx, double* row, int mode, hipStream_t st);

// ---------------------------------------------------------------- device sources (kernels_pack.hip)
// lpipm_upload_device: the caller's strided device arrays (double or float) into the zeroed resident image.  Strides are in
// ELEMENTS of the source type; `ms` is the member stride of the source (0: one source for the launch), dstride the BYTES
// between the members' arenas (0: one image).  The callers have checked that every address these launches form lies inside
// the caller's allocations (solver.hip, sources_inside).
// A: up to two blocks of rows (the `ub` and `eq` blocks of lpipm_upload_ub_eq; a block of 0 rows is skipped), block s's row i
// going to row row0 + i of the image (ldd doubles per row), columns [0, nx).  mode: a PackMode (device_source.hpp).
struct PackSeg { const void* src = nullptr; long long rs = 0, cs = 0, ms = 0; int rows = 0, row0 = 0, mode = 0; };
struct PackMatrix { PackSeg seg[2]; double* dst = nullptr; long long ldd = 0, dstride = 0; int nx = 0; };
hipError_t launch_pack_matrix(const PackMatrix& a, bool f32, int members, hipStream_t st);
// b and c of every member (segment s: len elements, `stride` apart, into dst of member z's arena), and c0 from a packed
// device array of doubles (c0_src[z] -> c0_dst of member z; null: not written), in one launch.
struct PackVecSeg { const void* src = nullptr; long long stride = 0, ms = 0; double* dst = nullptr; int len = 0; };
struct PackVectors { PackVecSeg seg[2]; const double* c0_src = nullptr; double* c0_dst = nullptr; long long dstride = 0; };
hipError_t launch_pack_vectors(const PackVectors& a, bool f32, int members, hipStream_t st);
// Whether columns [col0, col0 + ns) of every member's m rows are [I; 0]: a thread that finds an element != (i == j ? 1 : 0)
// (a NaN is one) stores 0 into *word, which the caller set to 1 on the same stream.
struct SlackHint { const void* src = nullptr; long long rs = 0, cs = 0, ms = 0, col0 = 0; int m = 0, ns = 0; int* word = nullptr; };
hipError_t launch_slack_hint(const SlackHint& a, bool f32, int members, hipStream_t st);

}  // namespace lpipm
