/*
 * lpipm.h -- C ABI of the MI355X-native interior-point LP hot path (liblpipm.so).
 *
 * Drop-in boundary for the ONE hot path of sebasv/lp (crate `ripped` 0.1.1):
 * `InteriorPoint::solve()` on a slack-form `Problem` -- forming A.diag(x/z).A^T, its Cholesky
 * factor, the triangular solves and the residual / direction GEMVs of the homogeneous self-dual
 * Mehrotra predictor-corrector algorithm -- as hand-written HIP kernels for gfx950.
 *
 * The reference has no FFI; each entry point below names the reference interface it replaces
 * (paths relative to /root/reference/src).  Plain pointers and sizes only; no C++/torch types.
 * The reference-side binding a maintainer would add (a `hip` feature arm next to
 * `cfg(feature = "blas")`, newton_equations.rs:2-13) is shown in INTEGRATION.md and
 * bindings/rust/.
 *
 * Conventions
 *   - every function returns an lpipm_status (0 = Ok) unless stated otherwise;
 *   - the caller owns every host pointer; the library copies in, never retains a host pointer
 *     after return, never calls back, never unwinds across the boundary;
 *   - a ctx is bound to one device and one stream and is not thread-safe; distinct ctxs are
 *     independent (one per GPU for batches);
 *   - matrices are row-major fp64, exactly as `Problem` holds them (ndarray standard layout,
 *     linear_program.rs:145-156).
 */
#ifndef LPIPM_H
#define LPIPM_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* error.rs:10-28 (LinearProgramError) as integers; >= 100 have no reference analogue. */
typedef enum {
    LPIPM_OK                      = 0,
    LPIPM_UNCONSTRAINED           = 1, /* error.rs:12  */
    LPIPM_NUMERICAL_PROBLEM       = 2, /* error.rs:15  */
    LPIPM_INVALID_PARAMETER       = 3, /* error.rs:18  */
    LPIPM_INCOMPATIBLE_DIMENSIONS = 4, /* error.rs:21  */
    LPIPM_INFEASIBLE              = 5, /* error.rs:24  */
    LPIPM_UNBOUNDED               = 6, /* error.rs:27  */
    LPIPM_ITERATION_LIMIT         = 7, /* error.rs:28  IterationLimitExceeded(x / tau): x_out IS filled */
    LPIPM_ERR_HIP                 = 100, /* HIP runtime failure (lpipm_last_error_detail has the text) */
    LPIPM_ERR_NO_PROBLEM          = 101, /* solve before upload */
    LPIPM_ERR_UNSUPPORTED         = 102, /* valid in the reference, not built here (QR arms beyond m = 16384) */
    LPIPM_ERR_BAD_ARGUMENT        = 103  /* null pointer / lda < n / size overflow */
} lpipm_status;

/* solvers/interior_point/newton_equations.rs:37-46 (EquationSolverType) */
enum { LPIPM_SOLVER_CHOLESKY = 0, LPIPM_SOLVER_INVERSE = 1, LPIPM_SOLVER_LEAST_SQUARES = 2 };

/* solvers/interior_point/mod.rs:41-48 (InteriorPointBuilder / InteriorPoint fields) */
typedef struct {
    double   tol;         /* mod.rs:53  default 1e-8    ; must be > 0        (mod.rs:124) */
    double   alpha0;      /* mod.rs:57  default 0.99995 ; 0 < alpha0 < 1     (mod.rs:119) */
    uint64_t max_iter;    /* mod.rs:58  default 1000 */
    int32_t  ip;          /* mod.rs:55  default 1 (alternative initial point) */
    int32_t  solver_type; /* mod.rs:56  default LPIPM_SOLVER_CHOLESKY */
    int32_t  disp;        /* mod.rs:54  default 0; 1 prints the reference's table (mod.rs:208-211,227-229) */
} lpipm_opts;

/* One row of the `disp` table: alpha (mod.rs:228) + Indicators (indicators.rs:8-23). */
typedef struct { double alpha, rho_p, rho_d, rho_A, rho_g, rho_mu, obj; } lpipm_iter_row;
/* The same row of an f32 solve (lpipm_solve_f32). */
typedef struct { float alpha, rho_p, rho_d, rho_A, rho_g, rho_mu, obj; } lpipm_iter_row_f32;

/* Device time per phase of the LAST lpipm_solve on this ctx, from HIP events on the ctx's stream
 * (only filled while profiling is on; recording events costs a few us per phase).  The marks sit on the ctx's stream: what a
 * large single LP runs beside the factorisation's chain on the look-ahead's side stream (trailing updates, merges of the
 * super-block inverses, the predictor's pass over A and the first forward steps of its solve) falls inside the
 * factorisation's interval and is counted in potrf_ms; gemv_passes still counts that pass. */
typedef struct {
    double   adat_ms;      /* sum over iterations of the A.D.A^T kernel launches       */
    double   potrf_ms;     /* Cholesky factorisation (+ diagonal-block inverses)        */
    double   trsv_ms;      /* triangular solves                                        */
    double   gemv_ms;      /* passes over A (GEMV-N / GEMV-T)                           */
    double   vec_ms;       /* O(n) vector / scalar kernels + status read-back          */
    double   total_ms;     /* first kernel to last kernel of the solve                 */
    uint64_t adat_launches; /* A.D.A^T launches made: `iterations`, less one when iteration 1 started from the kept factor, plus
                             * the one that builds a shared-matrix batch's factor ahead of its first solve (its time and
                             * the factorisation's are in adat_ms and potrf_ms of that solve) */
    uint64_t iterations;
    uint64_t gemv_passes;  /* passes over A inside gemv_ms (a 2-vector pass reads A once and counts once) */
} lpipm_phase_times;

typedef struct lpipm_ctx lpipm_ctx; /* opaque: device buffers + stream for one (thread, device) */

/* InteriorPointBuilder::new (mod.rs:50-60) */
void lpipm_default_opts(lpipm_opts* out);
/* Display strings of error.rs:10-28 (+ the >= 100 codes).  Never NULL. */
const char* lpipm_strerror(int status);
/* Text of the last HIP failure on this thread ("" if none). */
const char* lpipm_last_error_detail(void);
/* Number of visible HIP devices (0 when there is no GPU or no driver). */
int lpipm_device_count(void);

/* ProblemBuilder::build (linear_program.rs:125-169): slack form
 *   A = [[A_ub I],[A_eq 0]]  ((m_ub+m_eq) x (n+m_ub)),  b = [b_ub; b_eq],  c = [c; 0].
 * Host-side, O(mn), once per problem.  A_ub / A_eq may be NULL when their row count is 0.
 * Outputs must hold (m_ub+m_eq)*(n+m_ub), (m_ub+m_eq) and (n+m_ub) doubles. */
int lpipm_problem_build(uint64_t n, uint64_t m_ub, const double* A_ub, const double* b_ub,
                        uint64_t m_eq, const double* A_eq, const double* b_eq, const double* c,
                        double* A_out, double* b_out, double* c_out, uint64_t* n_slack_out);

/* One context per (thread, device).  Fails with LPIPM_ERR_HIP when the device is unusable:
 * there is NO CPU fallback anywhere behind this ABI. */
int  lpipm_create(int device, lpipm_ctx** out);
void lpipm_destroy(lpipm_ctx* ctx);

/* Upload the slack-form problem `Problem` holds (accessors A() b() c(), linear_program.rs:42-59;
 * c0 :56-59).  A is m x n row-major with leading dimension lda >= n.  One H2D copy of A; the
 * hot loop never touches host memory again except a 96-byte status read-back per iteration. */
int lpipm_upload(lpipm_ctx* ctx, uint64_t m, uint64_t n, const double* A, uint64_t lda,
                 const double* b, const double* c, double c0);

/* Same upload with the structural hint `Problem` carries (n_slack, linear_program.rs:161): the last
 * n_slack columns of A are the slack block [I; 0] of `ub` constraints (linear_program.rs:147-156).
 * They are then neither copied to the device nor multiplied: M = A_x D_x A_x^T + diag(D_s), A.w adds
 * w_s, A^T.v copies v.  The hint is verified; a matrix without that structure is treated as dense.
 * Results agree with lpipm_upload to rounding (same iteration counts on every test). */
int lpipm_upload_slack(lpipm_ctx* ctx, uint64_t m, uint64_t n, const double* A, uint64_t lda,
                       const double* b, const double* c, double c0, uint64_t n_slack);

/* Device-side assembly of the slack form (ProblemBuilder::build, linear_program.rs:125-169, without its
 * (m_ub+m_eq) x (n+m_ub) host matrix): the `ub` and `eq` blocks go to the device as they are -- rows of A_ub
 * first, then rows of A_eq (linear_program.rs:145-156) -- b = [b_ub; b_eq] (:157-158), c = [c; 0] (:159-160),
 * and the slack block [I; 0] is never formed anywhere.  Equivalent to lpipm_problem_build + lpipm_upload_slack
 * (bit-identical solves); x_slack_out of lpipm_solve then has n + m_ub entries, slack values last.
 * Either block may be absent (m_ub or m_eq 0, pointer NULL); both absent -> LPIPM_UNCONSTRAINED (:134-136). */
int lpipm_upload_ub_eq(lpipm_ctx* ctx, uint64_t n, uint64_t m_ub, const double* A_ub, uint64_t lda_ub,
                       const double* b_ub, uint64_t m_eq, const double* A_eq, uint64_t lda_eq, const double* b_eq,
                       const double* c, double c0);

/* The tall inequality form: a pure-`ub` LP, min c^T x, A_ub.x <= b_ub, x >= 0, with many more rows than columns (cover and
 * resource models, L1 / L-infinity fits, scenario cuts, discretised semi-infinite constraints).  Arguments as lpipm_upload_ub_eq
 * without its `eq` block.  The slack form is A = [X I], X = A_ub (m_ub x n), and its normal matrix X.D_x.X^T + D_s has one row
 * per constraint; after this upload lpipm_solve / lpipm_solve_device factor instead the n x n SPD matrix
 *   K = X^T.diag(W_s).X + diag(E_x),   W_s = z_s / x_s (slack part of the iterate),   E_x = z_x / x_x (structural part),
 * and sym_solve(r1, r2) (newton_equations.rs:214-225), r1 = [r1_x; r1_s], reads
 *   t = W_s*r2 + r1_s;  g = X^T.t - r1_x;  u_x = K^-1 g;  u_s = r2 - X.u_x;  v = W_s*u_s + r1_s;  u = [u_x; u_s]
 * -- the same Newton system, so every solve agrees with lpipm_upload_ub_eq on the same LP to rounding (same status and
 * iteration count on every test; no bit-identity).  K is built by the A.D.A^T kernels from a resident transpose of X (written
 * once per upload, after the equilibration of lpipm_set_scaling, which works as for any upload: both copies carry the same
 * exponents) and factored by the Cholesky chain; nothing the context holds grows as m_ub^2 (lpipm_get_resident_bytes counts the
 * transpose).  x_slack_out has n + m_ub entries, slack values last; return codes, fun, the iteration log, the `disp` table and
 * the phase times are as after lpipm_upload_ub_eq (K's build in adat_ms, its factorisation in potrf_ms; a failed pivot of K is
 * LPIPM_NUMERICAL_PROBLEM, as a failed pivot of M is).  m_ub = 0: LPIPM_UNCONSTRAINED.
 * Scope.  Cholesky arm only: lpipm_solve with solver_type 1 or 2 returns LPIPM_ERR_UNSUPPORTED, and so do
 * lpipm_update_vectors (as after lpipm_upload_ub_eq), this upload on a context of a column split (lpipm_set_collective with
 * world > 1) or with the opt-in refined solves, and lpipm_k_adat (there is no M; lpipm_k_tall_normal returns K).  The first
 * iteration's factor is not kept (as for the QR arms).  `eq` rows go through lpipm_upload_ub_eq_tall (below: a Schur
 * complement on K's factor); many tall LPs over one A_ub are a lockstep batch (lpipm_upload_lockstep_shared_ub_tall, below).
 * lpipm_k_iteration, lpipm_k_gemv_n, lpipm_k_gemv_t and lpipm_k_gemv_dual work as on any other upload. */
int lpipm_upload_ub_tall(lpipm_ctx* ctx, uint64_t n, uint64_t m_ub, const double* A_ub, uint64_t lda_ub, const double* b_ub,
                         const double* c, double c0);

/* The tall form with equality rows: min c^T x, A_ub.x <= b_ub, A_eq.x = b_eq, x >= 0, m_ub >> n and a few `eq` rows (a budget
 * or normalisation row, an interpolation constraint, a conservation row).  The arguments of lpipm_upload_ub_eq.  K stays the
 * n x n SPD matrix of lpipm_upload_ub_tall, built from the `ub` rows alone; the m_eq equality rows go through a Schur complement
 * on its factor.  Once per iteration, after K = L.L^T:
 *   Zt = A_eq.L^-T  (m_eq x n),   S = Zt.Zt^T = A_eq.K^-1.A_eq^T  (m_eq x m_eq, SPD),   S = L_S.L_S^T
 * and sym_solve(r1, r2), r2 = [r2_u; r2_e], reads
 *   t = W_s*r2_u + r1_s;  g = X^T.t - r1_x;  w = L^-1.g;  h = r2_e - Zt.w;  v_e = S^-1.h;  w += Zt^T.v_e;  u_x = L^-T.w;
 *   u_s = r2_u - X.u_x;  v_u = W_s*u_s + r1_s;  u = [u_x; u_s];  v = [v_u; v_e]
 * Afterwards lpipm_solve / lpipm_solve_device run that.  x_slack_out has n + m_ub entries, slack values last; return codes, fun,
 * the iteration log and the `disp` table are as after lpipm_upload_ub_eq, and the contract against it on the same LP is the
 * same status and iteration count and x to rounding (no bit-identity).  A failed pivot of K or of S is
 * LPIPM_NUMERICAL_PROBLEM: linearly dependent equality rows, and m_eq > n, end there.  Phase times: adat_ms and adat_launches
 * count the build of K only; potrf_ms holds the factorisation of K, then Zt, then S and its factorisation; trsv_ms all
 * triangular solves, the two on S included.  The resident image is lpipm_upload_ub_eq's (rows of A_ub, then rows of A_eq),
 * the transpose is of the `ub` rows only; Zt, S with its inverses and the work vectors of the Schur solve are counted by
 * lpipm_get_resident_bytes, and nothing grows as m_ub^2.  lpipm_set_scaling works as on any upload (the image with its `eq`
 * rows is equilibrated before the transpose is written, Zt comes from the scaled image, x comes back in the caller's units).
 * m_eq == 0: exactly lpipm_upload_ub_tall on the same arguments -- the same request, the same bits.
 * Refusals.  m_ub == 0 and m_eq == 0: LPIPM_UNCONSTRAINED.  Null pointers or lda < n: LPIPM_ERR_BAD_ARGUMENT.  m_ub == 0 < m_eq
 * (not a tall LP: lpipm_upload_ub_eq is its entry), a column-split context or one with the refined solves, solver_type 1 or
 * 2, lpipm_update_vectors[_device] and lpipm_k_adat: LPIPM_ERR_UNSUPPORTED, as on every tall upload.
 * Many such LPs over one [A_ub; A_eq] are a lockstep batch: lpipm_upload_lockstep_shared_ub_eq_tall, below.
 * Out of scope: such LPs with their own matrices as a batch; lpipm_upload_device (its form value 3 stays
 * LPIPM_ERR_BAD_ARGUMENT); a kept K_1; the QR arms.  No first factor is kept. */
int lpipm_upload_ub_eq_tall(lpipm_ctx* ctx, uint64_t n, uint64_t m_ub, const double* A_ub, uint64_t lda_ub,
                            const double* b_ub, uint64_t m_eq, const double* A_eq, uint64_t lda_eq, const double* b_eq,
                            const double* c, double c0);

/* The bounded form: min c^T x, A_ub.x <= b_ub, A_eq.x = b_eq, 0 <= x, x_j <= upper[j] -- capacities, 0-1 relaxations, box
 * constraints, trust regions.  The arguments of lpipm_upload_ub_eq, plus upper[n]: +inf means no bound; B is the ascending list
 * of the nb columns with a finite one.  Written as `ub` rows the bounds would grow the normal matrix from m x m to
 * (m + nb) x (m + nb), m = m_ub + m_eq.  Here the LP that is solved is that explicit one,
 *   A_ext = [[A, 0], [E_B, I_nb]]   b_ext = [b; u_B]   c_ext = [c; 0]   x_ext = [x; w]   z_ext = [z; v]   y_ext = [y; y_b]
 * (A the slack form of lpipm_upload_ub_eq, w the bound slacks, v their reduced costs, y_b = -v at a solution), by the unchanged
 * algorithm on the extended vectors -- but the bound block of the Newton system is diagonal and is eliminated in closed form.
 * With dx = x / z, dw = w / v, s = dx_j + dw_j and D~_j = 1 / (z_j / x_j + v_j / w_j) for j in B, D~_j = dx_j elsewhere,
 * sym_solve(r1, r2) (newton_equations.rs:214-225), r1 = [r1_x; r1_w], r2 = [r2_1; r2_2], reads
 *   M~   = A.diag(D~).A^T                    m x m: the A.D.A^T build with D~ for dinv (+ diag(D_s) on the `ub` rows, as always)
 *   W_j  = D~_j (r1_x,j - r1_w,j) - (dx_j / s) r2_2,j        j in B;   W_j = dx_j r1_x,j otherwise
 *   v_1  = M~^-1 (r2_1 + A.W);   t = A^T.v_1                 one pass A.w, one solve, one pass A^T.v: the dense arm's
 *   g_j  = D~_j (t_j - r1_x,j + r1_w,j);  u_x,j = g_j + (dx_j / s) r2_2,j;  u_w,j = -g_j + (dw_j / s) r2_2,j     j in B
 *   u_x,j = dx_j (t_j - r1_x,j) otherwise;   v_2,j = r1_w,j + u_w,j / dw_j;   u = [u_x; u_w],  v = [v_1; v_2]
 * (u_w never as r2_2 - u_x: that cancels once a column sits at its bound.)  The bound block is never stored and never
 * multiplied; an iteration makes as many passes over A as after lpipm_upload_ub_eq.
 * Outputs.  x_slack_out of lpipm_solve[_device] has n + m_ub + nb entries: the structural values, the `ub` slacks, then the
 * bound slacks w in ascending column order.  lpipm_get_duals[_device] and lpipm_get_certificate[_device] serve the upload:
 * y has m + nb entries, the bound rows last (a bound row's multiplier is <= 0 and equals -v_j up to the dual residual); z and
 * col are as long as x_slack_out.
 * Contract against the explicit form -- the same LP with its bound rows appended to A_ub, through lpipm_upload_ub_eq: the same
 * status and iteration count, x and fun to rounding (no bit-identity).  nb == 0 (upper NULL or all +inf): exactly
 * lpipm_upload_ub_eq on the same arguments -- the same request, the same bits.
 * Memory: nothing the context holds grows as (m + nb)^2; lpipm_get_resident_bytes counts the index lists.  Phase times are as
 * after lpipm_upload_ub_eq.  lpipm_set_scaling works as on any upload: exponents from the stored structural block; the bound
 * row of column j gets kr = -kc[j] and its slack column kc = kc[j] (its entries stay exactly 1, the block unstored),
 * u_j <- ldexp(u_j, -kc[j]), x_j and w_j come back by ldexp(., kc[j]); lpipm_get_scaling returns m + nb row exponents and
 * n + m_ub + nb column exponents.
 * Refusals (a refused call leaves the resident problem as it was).  An upper[j] that is NaN or -inf: LPIPM_ERR_BAD_ARGUMENT (any
 * finite value is accepted, as the explicit form accepts it).  Both blocks absent: LPIPM_UNCONSTRAINED.  solver_type 1 or 2 at
 * solve time, a column-split context, a context with the refined solves, lpipm_update_vectors[_device] and lpipm_k_adat:
 * LPIPM_ERR_UNSUPPORTED.  lpipm_k_iteration, lpipm_k_gemv_n, lpipm_k_gemv_t and lpipm_k_gemv_dual see A_ext with its extended
 * lengths.  No first factor is kept.
 * Out of scope: lockstep and shared-matrix batches of bounded LPs; lpipm_upload_device and lpipm_solve_batch*; a kept first
 * factor (M~_1 depends on A and B alone: a follow-up); the QR arms; f32; bounds on the tall forms (there a bound is one more
 * cheap row already); lower bounds other than 0 and free columns (lpipm_upload_bounds, next, has them). */
int lpipm_upload_bounded(lpipm_ctx* ctx, uint64_t n, uint64_t m_ub, const double* A_ub, uint64_t lda_ub, const double* b_ub,
                         uint64_t m_eq, const double* A_eq, uint64_t lda_eq, const double* b_eq, const double* c, double c0,
                         const double* upper);

/* General column bounds: min c.x + c0, A_ub x <= b_ub, A_eq x = b_eq, lower_j <= x_j <= upper_j, with lower_j real or -inf
 * (NULL: all 0) and upper_j real or +inf (NULL: all +inf), one pair per structural column.  The normal matrix still has the
 * order m = m_ub + m_eq, and no column of A is stored or read twice.  Per column:
 *   P  lower finite, upper +inf    the shift x_j = lower_j + x'_j          (lower_j = 0: the ordinary column)
 *   B  both finite                 the shift, then lpipm_upload_bounded's column with u'_j = upper_j - lower_j
 *   N  lower -inf, upper finite    the reflection x_j = upper_j - x'_j     (sigma_j = -1, t_j = upper_j)
 *   F  lower -inf, upper +inf      free: x_j = x'_j - x^-_j, both halves >= 0, ONE stored column
 * With sigma_j = +1 outside N and t_j = 0 on F the iteration sees the primed LP A' = A.diag(sigma), b' = b - A.t, c' = sigma c,
 * c0' = c0 + c.t, extended as lpipm_upload_bounded extends it plus one column per free column (F ascending, nf of them):
 *   A_ext = [[A', 0, -A'_F], [E_B, I_nb, 0]]   b_ext = [b'; u'_B]   c_ext = [c'; 0; -c'_F]   x_ext = [x'; w; x^-]   z_ext = [z; v; z^-]
 * Only sym_solve changes, on F (dm = x^- / z^-, r1 = [r1_x; r1_w; r1_m], t = A'^T.v_1):
 *   D~_j = dx_j + dm_j;   W_j = dx_j r1_x,j - dm_j r1_m,j;   u_x,j = dx_j (t_j - r1_x,j);   u_m,j = dm_j (-t_j - r1_m,j)
 * The free block is never stored and never multiplied: a pass over A' reads the net vector (x'_j - x^-_j on F), and the x^-
 * column of A_ext^T.v is -(A'^T.v_1)_j.  The two halves of a free column are determined only up to a common shift: the contract
 * is on their difference.
 * Outputs.  x_slack_out of lpipm_solve[_device] has n + m_ub + nb + nf entries: the structural values IN THE CALLER'S VARIABLES
 * (x_j = t_j + sigma_j x'_j; x'_j - x^-_j on F), the `ub` slacks, the bound slacks w, then the negative parts x^- in ascending
 * column order (a diagnostic: the positive part is x_j + x^-_j).  fun = c.x + c0 in the caller's variables.
 * lpipm_get_duals[_device]: y has m + nb entries (a column transform does not change a row's multiplier); z is as long as
 * x_slack_out, z_j = sigma_j z'_j on the structural columns, so that A^T y + z = c holds in the caller's orientation up to the
 * dual residual (z_j <= 0 on N, z_j ~ 0 on F), v and z^- behind them; dual_fun is that of the primed LP (b'.y + u'.y_b + c0').
 * lpipm_get_certificate[_device]: as on the bounded form.  The improving ray comes in the caller's orientation (sigma applied,
 * the free halves netted: A x ~ 0, c.x = -1, x_j >= 0 outside N and F, x_j <= 0 on N); the Farkas ray is normalised against the
 * SHIFTED right-hand side, b'.y + u'.y_b = 1 with b' = b - A.t, and its z comes with sigma applied.
 * lpipm_get_scaling returns m + nb row exponents and n + m_ub + nb + nf column exponents (an x^- column has its column's).
 * Refusals (a refused call leaves the resident problem as it was).  NaN, lower_j = +inf or upper_j = -inf: LPIPM_ERR_BAD_ARGUMENT;
 * lower_j > upper_j: LPIPM_INFEASIBLE, returned by the upload; lower_j == upper_j is class B with width 0 and behaves as the
 * explicit form does.  Everything lpipm_upload_bounded refuses with LPIPM_ERR_UNSUPPORTED is refused here.  The
 * lpipm_k_bounded_* entries, lpipm_k_iteration and lpipm_k_gemv_n/_t/_dual see A_ext at the new lengths.  No first factor is kept.
 * Without a free column, a reflection or a non-zero shift this is lpipm_upload_bounded's request itself: the same launches,
 * the same bits.
 * Out of scope: lockstep and shared-matrix batches; lpipm_upload_device and lpipm_solve_batch*; the tall forms; f32; the QR
 * arms; a kept first factor; eliminating fixed columns; ranged rows. */
int lpipm_upload_bounds(lpipm_ctx* ctx, uint64_t n, uint64_t m_ub, const double* A_ub, uint64_t lda_ub, const double* b_ub,
                        uint64_t m_eq, const double* A_eq, uint64_t lda_eq, const double* b_eq, const double* c, double c0,
                        const double* lower, const double* upper);

/* New b and c for the resident problem of lpipm_upload / lpipm_upload_slack: b[m] and c[n] in that upload's own form (c with
 * its slack entries).  A stays where it is, so a sweep over right-hand sides or costs, or a sequence of LPs over one
 * constraint matrix, pays for the upload of A once -- and, with it, for the first iteration's factor (below), which depends
 * on A alone and is kept.  The next lpipm_solve is bit-identical to lpipm_upload(A, b, c) + lpipm_solve; c0 stays.
 * LPIPM_ERR_NO_PROBLEM without an upload; LPIPM_ERR_UNSUPPORTED after lpipm_upload_ub_eq (its b and c come in parts), for a
 * lockstep batch and for a column-split context. */
int lpipm_update_vectors(lpipm_ctx* ctx, const double* b, const double* c);

/* New b, c and (optionally) c0 for EVERY member of the resident lockstep batch, whichever lpipm_upload_lockstep* made it, in
 * that upload's own form: b[i][m] and c[i][n] (c with its slack entries); after lpipm_upload_lockstep_shared_ub_eq
 * b[i] = [b_ub_i; b_eq_i] and c[i] = the n structural costs (the slack costs stay 0), after
 * lpipm_upload_lockstep_shared_ub_tall and lpipm_upload_lockstep_ub_tall b[i] of m_ub doubles and c[i] = the n structural costs,
 * after lpipm_upload_lockstep_shared_ub_eq_tall b[i] = [b_ub_i; b_eq_i] and c[i] = the n structural costs.  b or c may be NULL as a whole: those
 * vectors stay (a right-hand-side sweep sends no costs); c0 == NULL: the constants stay.  A, the layout, the half-batch views
 * and the kept first factor(s) are not touched, and the padding beyond m and n stays zero: the next lpipm_solve_lockstep[_device]
 * is bit-identical to a fresh upload of the same members followed by a solve.  The host arrays are staged in one pinned block
 * of the context, sent with one copy and distributed by one kernel launch; the call returns when they are free again.
 * The _device variant reads packed row blocks that are already on the device, on the context's stream (they must be
 * complete when it is called): member i's b at b_dev + i * ldb doubles (ldb >= m), its c at c_dev + i * ldc (ldc >= the
 * length of c[i] above); c0 stays a host array.  A scenario generator on the GPU never touches the host.
 * LPIPM_ERR_NO_PROBLEM without an upload; LPIPM_ERR_BAD_ARGUMENT for a null context, b and c both NULL, count other than
 * the resident member count, or ldb / ldc too small; LPIPM_ERR_UNSUPPORTED for a column-split context and after the
 * single-LP lpipm_upload_ub_eq (as lpipm_update_vectors).  The staging block (count * (m + n + 1) doubles on each side) is
 * not part of lpipm_get_resident_bytes. */
int lpipm_update_lockstep_vectors(lpipm_ctx* ctx, uint64_t count, const double* const* b /* nullable */,
                                  const double* const* c /* nullable */, const double* c0 /* nullable: stays */);
int lpipm_update_lockstep_vectors_device(lpipm_ctx* ctx, uint64_t count, const void* b_dev /* nullable */, uint64_t ldb,
                                         const void* c_dev /* nullable */, uint64_t ldc,
                                         const double* c0 /* host, nullable: stays */);

/* Every solve starts from x = z = 1 (feasible_point.rs:24-31), so the normal matrix of its first iteration is A.A^T (+ I on
 * the rows of a structural slack block): that matrix, its Cholesky factor, the inverses of the factor's diagonal blocks and
 * the pivot-failure word are functions of A alone.  The Cholesky arm keeps them per upload -- a single LP's, and every
 * member's of a lockstep batch whose members own their matrices -- and every solve after the first on the same upload starts
 * from them instead of running A.D.A^T and the factorisation again.  A shared-matrix batch (lpipm_upload_lockstep_shared*)
 * keeps ONE set next to its one A: it is formed and factored once, ahead of the first solve after the upload, and every
 * member of every solve, the first included, starts from it; in that iteration each block of the factor and of its inverses
 * is read once per group of members.  No result changes by a bit.  Any upload drops what is kept.  Not used by the QR arms,
 * column-split contexts, lpipm_solve_f32 and lpipm_solve_batch (which uploads on every call).
 * Cost per resident LP -- once per shared-matrix batch, which adds a vector of ones over the padded columns (8 np bytes
 * rounded up to 4096, np = n rounded up to 16) --, with mp = m rounded up to 128 and s_k the widths of the diagonal
 * super-blocks (512 each up to mp = 2048, 1024 beyond; the last one what is left of mp):  8 mp^2 + 16 sum_k s_k^2 + 4096
 * bytes (lpipm_get_resident_bytes counts them).  A single LP with mp >= 4096 -- not a batch, not a column split -- solves
 * through the coupled backward sweep, and its kept factor has blocks of its own for that: the products H_k (s_k x s_k+1, one
 * per super-block but the last) and the transposed copy of every block column k of the factor below super-block k + 1
 * (s_k x (mp - r_k+2), r_j the first row of super-block j): 8 (sum_k s_k s_k+1 + sum_k s_k (mp - r_k+2)) bytes more, 48 MiB
 * at mp = 4096.  on = 0 gives that memory back: the kept factor is no longer used from the
 * next solve on, and the buffers go (or, with on = 1 again, come back) with the next upload; a shared-matrix batch uploaded
 * with on = 0 has no shared set, and every member forms and factors its own iteration 1.  Default: on. */
int lpipm_set_first_factor_cache(lpipm_ctx* ctx, int on);

/* Power-of-two row and column equilibration of the resident matrix, for problems that mix units (the reference has none; it
 * leaves a comment slot, mod.rs:164).  With integer exponents kr[i], kc[j], all zero at the start, and X the stored structural
 * block of A (the slack columns of a verified hint or of an *_ub_eq upload are not part of it), one pass takes
 * S_ij = |ldexp(X_ij, kr[i] + kc[j])| from the original X_ij, the row and column maxima of S (NaNs ignored), and for every
 * finite maximum a > 0 with frexp(a) = (f, e) adds -(e floordiv 2) to that row's or column's exponent; a maximum in [0.5, 2)
 * stays.  After the last pass A_ij <- ldexp(A_ij, kr[i] + kc[j]), b_i <- ldexp(b_i, kr[i]), c_j <- ldexp(c_j, kc[j]) on the
 * device; the slack column of `ub` row i gets kc = -kr[i], so its entry stays exactly 1 and the block [I; 0] stays unstored.
 * The solve then runs unchanged on the scaled problem: it is bit-identical to an ordinary solve of the same LP scaled on the
 * host with these exponents (powers of two: exact), and x_j / tau is returned as ldexp(x_j / tau, kc[j]) to every
 * destination.  `fun` is computed from the scaled vectors (the same number); the iteration log, the `disp` table and `tol`
 * refer to the SCALED problem.  The kept first factor is that of the scaled matrix; lpipm_update_vectors and
 * lpipm_update_lockstep_vectors[_device] scale the new b and c with the kept exponents.  A lockstep batch whose members own
 * their matrices has one set of exponents per member, a shared-matrix batch one set.  lpipm_solve_batch* passes the switch on
 * to every member.  The lpipm_k_* entries that work on the uploaded problem see the scaled one.  lpipm_solve_f32 ignores the
 * switch; lpipm_upload_nsplit with scaling on returns LPIPM_ERR_UNSUPPORTED.  The exponents (4 (mp + np) bytes per set) and the
 * slabs of the maxima pass live in an allocation of their own, made only while scaling is on (lpipm_get_resident_bytes
 * counts it).
 * passes = 0: off (default).  1..64: that many equilibration passes at every later upload on this ctx.  Takes effect
 * with the next upload, like lpipm_set_first_factor_cache.  > 64 or < 0: LPIPM_ERR_BAD_ARGUMENT. */
int lpipm_set_scaling(lpipm_ctx* ctx, int passes);
/* The exponents in use for resident member `member` (0 for a single LP and for a shared-matrix batch): row_exp_out[m],
 * col_exp_out[n] (int32; n counts slack columns too).  All zero when scaling is off.  LPIPM_ERR_NO_PROBLEM before an upload. */
int lpipm_get_scaling(const lpipm_ctx* ctx, uint64_t member, int32_t* row_exp_out, int32_t* col_exp_out);

/* InteriorPoint::solve_normal_form + the `fun` of solve (mod.rs:199-240, :165).
 *   x_slack_out[n] : x / tau  (mod.rs:231); ALSO filled for LPIPM_ITERATION_LIMIT (mod.rs:237-239)
 *   fun_out        : c . x_slack + c0  (linear_program.rs:61-63)
 *   iterations_out : iteration at which the status was decided (mod.rs:213,231)
 *   log            : nullable; one row per iteration, at most max_iter rows
 * Dropping the n_slack tail (denormalize_x_into, linear_program.rs:65-69) stays with the caller,
 * where the reference has it (mod.rs:166).  Option validation mirrors mod.rs:118-128. */
int lpipm_solve(lpipm_ctx* ctx, const lpipm_opts* opts, double* x_slack_out, double* fun_out,
                uint64_t* iterations_out, lpipm_iter_row* log);

/* Same solve, solution left in HBM: copies x / tau (n doubles) to a DEVICE pointer on the ctx's
 * stream (for the one RCCL gather of a sharded batch); x_dev_out may be NULL. */
int lpipm_solve_device(lpipm_ctx* ctx, const lpipm_opts* opts, void* x_dev_out, double* fun_out,
                       uint64_t* iterations_out, lpipm_iter_row* log);

/* A shard of independent LPs on ONE device (BASELINE config 4): problem i is m[i] x n[i] with
 * A[i] (lda = n[i]), b[i], c[i], c0[i]; results go to x_slack_out[i] (n[i] doubles), fun_out[i],
 * iterations_out[i], status_out[i].  Returns the first non-Ok *runtime* status (>= 100) or Ok;
 * per-problem solver outcomes (Infeasible, ...) are reported in status_out only.
 * Members of equal shape are solved as lockstep batches (below), the others one at a time on worker contexts.
 * The call replaces the context's uploaded problem: upload again before a later lpipm_solve on this context. */
int lpipm_solve_batch(lpipm_ctx* ctx, uint64_t count, const uint64_t* m, const uint64_t* n,
                      const double* const* A, const double* const* b, const double* const* c,
                      const double* c0, const lpipm_opts* opts, double* const* x_slack_out,
                      double* fun_out, uint64_t* iterations_out, int32_t* status_out);

/* ---- one LP split by COLUMNS over several ranks / GPUs (BASELINE config C5) -----------------------------
 * Rank g holds the column block A[:, J_g] (m x n_local), c[J_g] and the matching slices of x, z; b and y
 * are replicated.  Per iteration the partial normal equations M_g = A_g D_g A_g^T are summed over ranks
 * (the "all-reduce on A.D.A^T panels"), as are A_g.w_g (m doubles) and a handful of dot products / ratio-test
 * minima; the factorisation runs replicated on every rank.  The library never links a communication
 * library: the caller supplies the all-reduce (RCCL `ncclAllReduce` on `stream` from Rust/C++, a
 * torch.distributed call from the Python harness).
 *   fn(user, dev_ptr, count, op, stream): in-place all-reduce of `count` doubles at device pointer dev_ptr,
 *   op 0 = sum, 1 = min; the stream has been drained before the call; return 0 when the result is in place. */
typedef int (*lpipm_allreduce_fn)(void* user, void* dev_ptr, uint64_t count, int op, void* stream);
int lpipm_set_collective(lpipm_ctx* ctx, int rank, int world, lpipm_allreduce_fn fn, void* user);
/* on = 1: the library no longer drains its stream before calling fn; fn must ENQUEUE the reduction on the stream it
 * is handed (RCCL: ncclAllReduce(ptr, ptr, count, ncclDouble, op, comm, (hipStream_t)stream)) and may return at once --
 * stream order makes the result visible to the kernels that follow, and nothing on the host waits (the one
 * status read-back per iteration excepted).  on = 0 (default): the drained contract described above. */
int lpipm_set_collective_on_stream(lpipm_ctx* ctx, int on);
/* Upload this rank's column block; afterwards lpipm_solve / lpipm_solve_device run the n-split algorithm and
 * return this rank's slice of x / tau (n_local doubles); fun, iterations and the log are global. */
int lpipm_upload_nsplit(lpipm_ctx* ctx, uint64_t m, uint64_t n_total, uint64_t n_local, const double* A_local,
                        uint64_t lda, const double* b, const double* c_local, double c0);

/* Lockstep batch: `count` LPs of ONE shape (m x n; dense, or with the slack hint of lpipm_upload_lockstep_slack) resident on the device at once; every kernel launch of
 * the iteration covers all of them, so the ~100 dependent launches per iteration are paid once per batch
 * instead of once per LP.  lpipm_upload_lockstep replaces the context's problem; lpipm_solve_lockstep returns
 * per-LP status (0 / LinearProgramError variants), fun, iterations and x / tau, exactly as `count` calls of
 * lpipm_solve would (Cholesky arm only: LPIPM_ERR_UNSUPPORTED otherwise).  A[i]: m x n row-major, lda = n. */
int lpipm_upload_lockstep(lpipm_ctx* ctx, uint64_t count, uint64_t m, uint64_t n, const double* const* A,
                          const double* const* b, const double* const* c, const double* c0 /* nullable */);
/* lpipm_upload_lockstep with the structural hint of lpipm_upload_slack (n_slack, linear_program.rs:161): the last n_slack
 * columns of EVERY member are the slack block [I; 0] of its `ub` rows (linear_program.rs:145-161) and are then neither
 * copied nor multiplied.  The hint is verified on every member; if one member's columns are not [I; 0] the whole upload is
 * treated as dense (and still returns Ok); n_slack == n is ignored.  Each member comes out bit-identical to
 * lpipm_upload_slack (same hint) + lpipm_solve of that member alone.  n_slack = 0: exactly lpipm_upload_lockstep. */
int lpipm_upload_lockstep_slack(lpipm_ctx* ctx, uint64_t count, uint64_t m, uint64_t n, const double* const* A,
                                const double* const* b, const double* const* c, const double* c0 /* nullable */,
                                uint64_t n_slack);
int lpipm_solve_lockstep(lpipm_ctx* ctx, const lpipm_opts* opts, double* const* x_slack_out, double* fun_out,
                         uint64_t* iterations_out, int32_t* status_out);
/* The same with the solutions left in HBM: x / tau of LP i goes to the DEVICE row x_dev_out + i * row_stride doubles
 * (row_stride >= n), device to device on the ctx's stream -- the packed block a sharded batch then all-gathers (RCCL)
 * without a host round trip.  Rows of members without a solution (Infeasible, ...) are left untouched. */
int lpipm_solve_lockstep_device(lpipm_ctx* ctx, const lpipm_opts* opts, void* x_dev_out, uint64_t row_stride,
                                double* fun_out, uint64_t* iterations_out, int32_t* status_out);
/* Lockstep batch of `count` LPs that share ONE constraint matrix A (m x n row-major, lda >= n): member i is
 * (A, b[i], c[i], c0[i]).  A is copied to the device once and is not part of any member's arena; every pass over A
 * serves the whole batch.  Solve with lpipm_solve_lockstep / lpipm_solve_lockstep_device, exactly as after
 * lpipm_upload_lockstep: each member comes out bit-identical to lpipm_upload + lpipm_solve of (A, b[i], c[i], c0[i]).
 * Validation and return codes as lpipm_upload_lockstep (Cholesky arm only).  This entry takes A as a dense matrix; the
 * two below keep its slack block structural. */
int lpipm_upload_lockstep_shared(lpipm_ctx* ctx, uint64_t count, uint64_t m, uint64_t n, const double* A, uint64_t lda,
                                 const double* const* b, const double* const* c, const double* c0 /* nullable */);
/* lpipm_upload_lockstep_shared with the structural hint of lpipm_upload_slack (linear_program.rs:145-161): the one shared A
 * is given with its n_slack slack columns [I; 0], which are verified and then neither copied nor multiplied (a matrix
 * without them is treated as dense; n_slack == n is ignored).  Each member bit-identical to lpipm_upload_slack (same hint) +
 * lpipm_solve of (A, b[i], c[i], c0[i]).  n_slack = 0: exactly lpipm_upload_lockstep_shared. */
int lpipm_upload_lockstep_shared_slack(lpipm_ctx* ctx, uint64_t count, uint64_t m, uint64_t n, const double* A, uint64_t lda,
                                       const double* const* b, const double* const* c, const double* c0 /* nullable */,
                                       uint64_t n_slack);
/* Device-side assembly (as lpipm_upload_ub_eq; ProblemBuilder::build, linear_program.rs:145-161) of a shared-matrix batch:
 * the ub / eq blocks are given once (either may be absent: row count 0, pointer NULL; both absent -> LPIPM_UNCONSTRAINED).
 * b[i] = [b_ub_i; b_eq_i] (m_ub + m_eq doubles), c[i] = the n structural costs.  No (m_ub+m_eq) x (n+m_ub) host matrix
 * exists anywhere.  x of lpipm_solve_lockstep has n + m_ub entries, slack values last; each member bit-identical to
 * lpipm_upload_ub_eq + lpipm_solve of that member alone. */
int lpipm_upload_lockstep_shared_ub_eq(lpipm_ctx* ctx, uint64_t count, uint64_t n, uint64_t m_ub, const double* A_ub,
                                       uint64_t lda_ub, uint64_t m_eq, const double* A_eq, uint64_t lda_eq,
                                       const double* const* b, const double* const* c, const double* c0 /* nullable */);
/* A lockstep batch of tall inequality-form LPs (lpipm_upload_ub_tall) over ONE A_ub: L1 / L-infinity fits of many response
 * vectors on one design matrix, quantile regression at many quantiles, scenario cuts under many right-hand sides.  Member i is
 * (A_ub, b[i] (m_ub doubles), c[i] (the n structural costs), c0[i]); the arguments are those of
 * lpipm_upload_lockstep_shared_ub_eq without its `eq` block.  X = A_ub and its transpose are resident ONCE for the batch
 * (the transpose written once per upload, behind the equilibration); a member holds its vectors, its own n x n matrix K with
 * the factor's inverses and its slabs -- nothing of a member grows as m_ub^2 and nothing of it is a copy of X.  Every pass over
 * X and the launch that builds the members' K read the one copy for a group of members.
 * Solve with lpipm_solve_lockstep / lpipm_solve_lockstep_device: x has n + m_ub entries, slack values last; status, fun and
 * iterations per member.  Every member is bit-identical to lpipm_upload_ub_tall + lpipm_solve of that member alone -- x, fun,
 * status and iteration count -- whatever the count, whichever members have finished, as one view or two half-batch views.
 * lpipm_update_lockstep_vectors[_device] replace b[i] (m_ub doubles), c[i] (the n structural costs) and c0 in place: X and its
 * transpose stay, and the next solve is bit-identical to a fresh upload of the same members.  lpipm_set_scaling works as for any
 * shared-matrix batch: one set of exponents (lpipm_get_scaling with member 0), X equilibrated once, b and c of the upload and
 * of later updates scaled with the kept exponents, x in the caller's units.  No first factor is kept
 * (lpipm_set_first_factor_cache changes nothing here); lpipm_get_resident_bytes counts X and its transpose once.
 * Return codes: m_ub == 0 LPIPM_UNCONSTRAINED; null pointers, count == 0 (or > 4096), lda_ub < n LPIPM_ERR_BAD_ARGUMENT; a
 * column-split context or one with the refined solves LPIPM_ERR_UNSUPPORTED (as lpipm_upload_ub_tall); solver_type 1 or 2
 * LPIPM_ERR_UNSUPPORTED (as every lockstep batch); lpipm_k_tall_normal, lpipm_k_tall_sym_solve, lpipm_k_iteration and
 * lpipm_k_adat on such a batch LPIPM_ERR_UNSUPPORTED.
 * Tall LPs of one shape that each have their own matrix: lpipm_upload_lockstep_ub_tall, below.
 * The same batch with `eq` rows in the one image: lpipm_upload_lockstep_shared_ub_eq_tall, below.
 * Not built: a kept K_1 = X^T.X + I, fused small-LP vector kernels for the tall form, tall members inside
 * lpipm_solve_batch / lpipm_solve_batch_slack (lpipm_solve_batch_ub_tall is their entry). */
int lpipm_upload_lockstep_shared_ub_tall(lpipm_ctx* ctx, uint64_t count, uint64_t n, uint64_t m_ub, const double* A_ub,
                                         uint64_t lda_ub, const double* const* b, const double* const* c,
                                         const double* c0 /* nullable */);
/* A lockstep batch of tall LPs with equality rows (lpipm_upload_ub_eq_tall) over ONE pair (A_ub, A_eq): the batches of
 * lpipm_upload_lockstep_shared_ub_tall whose members also carry a sum-to-one, budget, interpolation or conservation row.  The
 * arguments are those of lpipm_upload_lockstep_shared_ub_eq: member i is (A_ub, A_eq, b[i] = [b_ub_i; b_eq_i] (m_ub + m_eq
 * doubles), c[i] (the n structural costs), c0[i]).  Resident once: the image [A_ub; A_eq] and the transpose of its `ub` rows.
 * In each member's arena, beside its K, tall vectors and slabs: Zt = A_eq.L^-T, S with its factor's inverses and the words
 * and slabs of the launch that builds it, the work vectors of the Schur solve and the n ones that launch scales by.  Nothing
 * of a member is a copy of A_ub or A_eq, nothing of it grows as m_ub^2.  Once per iteration one launch forms every running
 * member's Zt from the one block of `eq` rows and the member's own factor of K; S, its factorisation and the solves follow
 * as lockstep launches.  A failed pivot of K or of S (dependent equality rows, m_eq > n) is that member's
 * LPIPM_NUMERICAL_PROBLEM; the others go on.
 * Solve with lpipm_solve_lockstep / lpipm_solve_lockstep_device: x has n + m_ub entries, slack values last.  Every member is
 * bit-identical to lpipm_upload_ub_eq_tall + lpipm_solve of that member alone -- x, fun, status and iteration count --
 * whatever the count, whichever members have finished, as one view or two half-batch views.
 * lpipm_update_lockstep_vectors[_device] replace b[i] (m_ub + m_eq doubles), c[i] (the n structural costs) and c0 in place,
 * the next solve bit-identical to a fresh upload of the same members.  lpipm_set_scaling works as for any shared-matrix
 * batch: one set of exponents (lpipm_get_scaling with member 0), the image with its `eq` rows equilibrated once, before the
 * transpose is written, Zt formed from the scaled image, updates scaled with the kept exponents, x in the caller's units.
 * No first factor is kept.
 * m_eq == 0: exactly lpipm_upload_lockstep_shared_ub_tall on the same arguments -- the same request, the same bits.
 * Refusals.  m_ub == 0 and m_eq == 0: LPIPM_UNCONSTRAINED.  m_ub == 0 < m_eq: LPIPM_ERR_UNSUPPORTED.  Null pointers, count == 0
 * (or > 4096), lda_ub < n or lda_eq < n: LPIPM_ERR_BAD_ARGUMENT.  A column-split context or one with the refined solves,
 * solver_type 1 or 2 at solve time, and lpipm_k_tall_normal, lpipm_k_tall_schur, lpipm_k_tall_sym_solve, lpipm_k_iteration and
 * lpipm_k_adat on such a batch: LPIPM_ERR_UNSUPPORTED.  A refused call leaves the resident problem as it was.
 * Out of scope: members with their own A_ub and A_eq, tall members with `eq` rows inside lpipm_solve_batch*, a kept first
 * factor, lpipm_upload_device (its form value 3 stays LPIPM_ERR_BAD_ARGUMENT). */
int lpipm_upload_lockstep_shared_ub_eq_tall(lpipm_ctx* ctx, uint64_t count, uint64_t n, uint64_t m_ub, const double* A_ub,
                                            uint64_t lda_ub, uint64_t m_eq, const double* A_eq, uint64_t lda_eq,
                                            const double* const* b, const double* const* c, const double* c0 /* nullable */);
/* A lockstep batch of `count` independent tall inequality-form LPs of one shape, each with its OWN matrix: one L-infinity fit or
 * cover model per customer or time window, per-scenario cut sets.  Member i is (A_ub[i] (m_ub x n row-major, lda_ub), b[i] (m_ub
 * doubles), c[i] (the n structural costs), c0[i]): the arguments of lpipm_upload_lockstep_shared_ub_tall with one matrix per
 * member.  Member i's arena holds its own X_i, its own transpose (made for all members by one launch, behind the per-member
 * equilibration) and its own K beside its tall vectors; nothing of a member grows as m_ub^2 and nothing is shared.
 * Solve with lpipm_solve_lockstep / lpipm_solve_lockstep_device: x has n + m_ub entries, slack values last.  Every member is
 * bit-identical to lpipm_upload_ub_tall + lpipm_solve of that member alone -- x, fun, status and iteration count -- whatever the
 * count, wherever the member sits, whichever members have finished, as one view or two half-batch views.
 * lpipm_update_lockstep_vectors[_device] replace b[i] (m_ub doubles), c[i] (the n structural costs) and c0 in place, the next
 * solve bit-identical to a fresh upload of the same members.  lpipm_set_scaling keeps one set of exponents per member
 * (lpipm_get_scaling with the member's index), as for any batch whose members own their matrices.  No first factor is kept.
 * Return codes and refusals are those of lpipm_upload_lockstep_shared_ub_tall, A_ub[i] counting among the pointers. */
int lpipm_upload_lockstep_ub_tall(lpipm_ctx* ctx, uint64_t count, uint64_t n, uint64_t m_ub, const double* const* A_ub,
                                  uint64_t lda_ub, const double* const* b, const double* const* c,
                                  const double* c0 /* nullable */);
/* ---- problems that are already in device memory ----------------------------------------------------------
 * Every upload above reads the caller's HOST arrays.  lpipm_upload_device makes the same problems resident from DEVICE memory
 * -- a torch model's cut sets, a design matrix a kernel built, members sliced out of one big tensor -- with no host copy of A,
 * b or c: one descriptor covers every form the host entries cover.
 *   form, shared, count select the host entry the call is equivalent to:
 *     SLACK    shared 0  count 1    lpipm_upload_slack                    UB_TALL  shared 0  count 1    lpipm_upload_ub_tall
 *     SLACK    shared 0  count > 1  lpipm_upload_lockstep_slack           UB_TALL  shared 0  count > 1  lpipm_upload_lockstep_ub_tall
 *     SLACK    shared 1  any        lpipm_upload_lockstep_shared_slack    UB_TALL  shared 1  any        lpipm_upload_lockstep_shared_ub_tall
 *     UB_EQ    shared 0  count 1    lpipm_upload_ub_eq                    UB_EQ    shared 1  any        lpipm_upload_lockstep_shared_ub_eq
 *   (UB_EQ members with their own matrices have no host entry: LPIPM_ERR_UNSUPPORTED).  After a successful call the context is
 *   in exactly the state that entry leaves for the same numbers -- geometry, lpipm_get_resident_bytes, scaling exponents, the
 *   kept first factor -- and every later call (solves, lpipm_update_vectors, lpipm_update_lockstep_vectors[_device],
 *   lpipm_get_scaling, the lpipm_k_* entries) gives the same bits and the same return codes: an upload is a copy.
 * Source layout.  Element (i, j) of member k of a matrix is at ptr + k * member_stride + i * row_stride + j * col_stride
 *   ELEMENTS (of src_type: LPIPM_SRC_F32 is widened to double, which is exact); element i of member k of a vector at
 *   ptr + k * member_stride + i * stride.  Every stride that is read must be >= 1; member_stride is not read for a shared
 *   matrix or count == 1.  A row-major block with a leading dimension, a column-major one and a slice of a larger tensor all go
 *   in as they are; ptr needs no alignment beyond its element type's.  b of member k: m entries (UB_EQ: [b_ub; b_eq],
 *   m + m_eq); c: n entries (UB_EQ / UB_TALL: the n structural costs).  c0 is a HOST array of count doubles (NULL: zeros).
 *   A with unit col_stride is moved as whole row segments (16 bytes per lane when base and pitches allow, else 8), one with
 *   unit row_stride through an LDS tile; any other pair of strides is gathered element by element -- correct, not fast.
 * Stream contract (as lpipm_update_lockstep_vectors_device): the sources must be complete when the call is made; they are read on
 *   the context's stream; the call returns when they are free again.
 * The slack hint (SLACK, 0 < n_slack < n) is verified ON THE DEVICE over the last n_slack columns of every member (of the one
 *   matrix when shared), with lpipm_upload_slack's comparison (a NaN fails it); one 4-byte word is read back before the
 *   geometry is chosen.  A hint that fails gives a dense upload and still returns Ok.  The word lives in an allocation of the
 *   context that lpipm_get_resident_bytes does not count.
 * Nothing reaches a kernel that could make it read outside the caller's allocations: before any launch every source pointer
 *   is looked up with the runtime, must be device memory of the context's device, and the farthest element its strides and
 *   extents address must lie inside that allocation; otherwise LPIPM_ERR_BAD_ARGUMENT, with nothing enqueued and the resident
 *   problem untouched.
 * Return codes: a null context or descriptor, struct_size other than sizeof(lpipm_device_problem), an unknown form or
 *   src_type, shared > 1, count 0 or > 4096, a stride < 1 LPIPM_ERR_BAD_ARGUMENT; then what the equivalent host entry returns
 *   for null pointers, m == 0 (LPIPM_UNCONSTRAINED), n == 0, n_slack > n or > m, m > 2^20, n > 2^24 and a tall form on a
 *   context with the refined solves; a column-split context (lpipm_set_collective, world > 1) LPIPM_ERR_UNSUPPORTED
 *   (lpipm_upload_nsplit stays host-only). */
enum { LPIPM_FORM_SLACK = 0, LPIPM_FORM_UB_EQ = 1, LPIPM_FORM_UB_TALL = 2 };
enum { LPIPM_SRC_F64 = 0, LPIPM_SRC_F32 = 1 };          /* element type of A, A_eq, b, c on the device */
typedef struct { const void* ptr; int64_t row_stride, col_stride, member_stride; } lpipm_dev_matrix; /* strides in ELEMENTS */
typedef struct { const void* ptr; int64_t stride, member_stride; } lpipm_dev_vector;
typedef struct {
    uint32_t struct_size;   /* sizeof(lpipm_device_problem): anything else is LPIPM_ERR_BAD_ARGUMENT */
    uint32_t form, src_type, shared;   /* shared = 1: ONE matrix (A, A_eq) for all `count` members */
    uint64_t count;         /* 1..4096 */
    uint64_t m;             /* rows of A: SLACK all rows; UB_EQ / UB_TALL the `ub` rows */
    uint64_t m_eq;          /* rows of A_eq (UB_EQ only, else 0) */
    uint64_t n;             /* columns of A (SLACK: slack columns included) */
    uint64_t n_slack;       /* SLACK only: the hint of lpipm_upload_slack, verified ON THE DEVICE */
    lpipm_dev_matrix A, A_eq;
    lpipm_dev_vector b;     /* per member: SLACK m; UB_EQ [b_ub; b_eq] of m + m_eq; UB_TALL m */
    lpipm_dev_vector c;     /* per member: SLACK n; UB_EQ / UB_TALL the n structural costs */
    const double* c0;       /* HOST array of `count`, nullable: zeros (as lpipm_update_lockstep_vectors_device) */
} lpipm_device_problem;
int lpipm_upload_device(lpipm_ctx* ctx, const lpipm_device_problem* d);
/* lpipm_update_vectors with b[m] and c[n] read from DEVICE memory (doubles, contiguous), on the context's stream and under the
 * stream contract above; the pointers are looked up as lpipm_upload_device's are.  Same refusals; the next solve is
 * bit-identical to one after lpipm_update_vectors with the same values. */
int lpipm_update_vectors_device(lpipm_ctx* ctx, const void* b_dev, const void* c_dev);

/* ---- dual values and reduced costs of the LAST solve ------------------------------------------------------------------
 * Every solve above hands back x / tau, fun and the iteration count; the multipliers y of the rows and the reduced costs z of
 * the columns of the same iterate stay in the context and are fetched here, after the solve: a Benders or scenario cut is y,
 * the sensitivity of fun to b_i is y_i, column pricing is z.  No solve entry, no arena layout and no bit of any solve changes.
 * Definition.  (x, y, z, tau, kappa) is the iterate at which the member's status was decided -- the one x_slack_out was
 *   formed from, for LPIPM_OK and for LPIPM_ITERATION_LIMIT alike.  In the resident (possibly scaled) problem yh = y / tau,
 *   zh = z / tau; with kr, kc the kept exponents of lpipm_get_scaling the values returned are y_i = ldexp(yh_i, kr[i]) and
 *   z_j = ldexp(zh_j, -kc[j]) (the slack column of `ub` row i carries kc = -kr[i]: its z gets +kr[i]) -- the division first, the
 *   power of two second, as for x: exact unless a value under- or overflows.  dual_fun = b.yh + c0 from the resident vectors,
 *   as fun is; tau and kappa are the iterate's.  Convention (residual.rs:23-29, r_D = c.tau - A^T.y - z): A^T.y + z = c,
 *   z >= 0, d fun / d b_i = y_i; the multiplier of a `ub` row is <= 0 and equals minus its slack's reduced cost up to the
 *   dual residual.
 * Lengths and order.  y: the m rows of the upload (*_ub_eq and *_ub_eq_tall: m_ub + m_eq, `ub` first); z: exactly as long as
 *   x_slack_out of that upload (structural entries, then the slack entries where the form has them).
 * lpipm_get_duals: resident member `member` (0 for a single LP), to host arrays (each nullable).  A member whose last status
 *   has no solution: that status (LPIPM_INFEASIBLE, ...) is returned and nothing is written.
 * lpipm_get_duals_device: all members at once, left in HBM on the context's stream (complete on return): member i's y at
 *   y_dev + i * ldy doubles, its z at z_dev + i * ldz (ldy >= the length of y, ldz >= that of z; either pointer may be NULL).
 *   Returns LPIPM_OK; the rows of a member without a solution stay untouched and its info is {NaN, NaN, NaN, status}.
 *   info_out: a host array of one record per resident member (nullable).  The destinations are looked up with the runtime
 *   and checked against their allocation before any launch, as lpipm_upload_device checks its sources.
 * The context keeps the per-member return codes of its last solve, whichever entry ran it (both half-batch views of a large
 *   lockstep batch record into it), and every member comes out bit-identical -- y, z, dual_fun, tau, kappa -- to the single
 *   upload + lpipm_solve + lpipm_get_duals of that member alone, by either entry.
 * Validity.  LPIPM_ERR_BAD_ARGUMENT: a null context, member >= the resident count, ldy or ldz too small, a destination that
 *   is not device memory of the context's device or does not hold every row.  LPIPM_ERR_UNSUPPORTED: a column-split context.
 *   LPIPM_ERR_NO_PROBLEM: nothing resident, or no solve has completed since the last event that changes what the iterate
 *   means: any upload, lpipm_update_vectors[_device], lpipm_update_lockstep_vectors[_device] (b and c are new, the iterate is
 *   old), an lpipm_k_* entry that writes the iterate (lpipm_k_iteration, lpipm_k_tall_normal, lpipm_k_tall_schur,
 *   lpipm_k_tall_sym_solve, lpipm_k_bounded_normal, lpipm_k_bounded_sym_solve), a solve that returned a runtime code (>= 100), lpipm_solve_batch* (which replace the resident
 *   problem with whichever chunk or member the context solved last: that is nobody's to ask about).  All three solver arms qualify.  Not served: lpipm_solve_batch*, lpipm_solve_f32, column-split contexts.
 * Cost: one vector launch and one scalar launch over the batch (gridDim.z = the resident count; the grid over a member
 *   depends on m and n alone), reduction slot 0, and for host destinations a staging block of the context that
 *   lpipm_get_resident_bytes does not count (the block of lpipm_update_lockstep_vectors).  The iterate is only read. */
typedef struct { double dual_fun, tau, kappa; int32_t status; int32_t reserved; } lpipm_dual_info;   /* 32 bytes */
int lpipm_get_duals(lpipm_ctx* ctx, uint64_t member, double* y_out /* nullable */, double* z_out /* nullable */,
                    lpipm_dual_info* info_out /* nullable */);
int lpipm_get_duals_device(lpipm_ctx* ctx, void* y_dev /* nullable */, uint64_t ldy, void* z_dev /* nullable */, uint64_t ldz,
                           lpipm_dual_info* info_out /* host array, one per resident member, nullable */);

/* ---- infeasibility and unboundedness certificates of the LAST solve ------------------------------------------------------
 * A member that ends LPIPM_INFEASIBLE or LPIPM_UNBOUNDED has no x and no duals; what a Benders or scenario loop needs from it is
 * the ray: the Farkas multipliers for a feasibility cut, or the improving direction.  Both are the homogeneous iterate
 * (x, y, z, tau, kappa) at which indicators.rs:66-76 decided the status, which stays in the context, normalised here after the
 * solve.  No solve entry, no arena layout, no lpipm_get_resident_bytes value and no bit of any solve changes.
 * Definition, in the resident (possibly scaled) problem:
 *   LPIPM_INFEASIBLE: kind = LPIPM_CERT_FARKAS, s = b.y (> tol by indicators.rs:72), yh = y / s, zh = z / s; y_out gets yh,
 *     col_out gets zh.  A^T.yh + zh ~ 0, zh >= 0, b.yh = 1: A x = b, x >= 0 has no solution.  The multiplier of a `ub` row is
 *     <= 0 and equals minus its slack's zh up to the residual.
 *   LPIPM_UNBOUNDED: s = -c.x.  s > 0: kind = LPIPM_CERT_RAY, xh = x / s, col_out gets xh, y_out is untouched.  A.xh ~ 0,
 *     xh >= 0, c.xh = -1: the dual is infeasible, the primal unbounded wherever it is feasible.  s <= 0 (the reference says
 *     Unbounded whenever b.y <= tol, so nothing is proved): kind = LPIPM_CERT_NONE, nothing is written.
 *   Any other status (Ok, iteration limit, numerical problem): kind = LPIPM_CERT_NONE, nothing is written, scale and residual
 *     are NaN.
 *   info: status is the member's last return code, tau and kappa the iterate's, scale = s.
 * Caller's units: the mapping of lpipm_get_duals, the division first and the power of two second: yh_i -> ldexp(., kr[i]),
 *   zh_j -> ldexp(., -kc[j]), xh_j -> ldexp(., kc[j]) (as x).  b.y and c.x are invariant under the equilibration: s needs no
 *   correction.  Lengths and order are those of lpipm_get_duals: y_out the m rows of the upload (`ub` first), col_out as long
 *   as x_slack_out, slack entries included.
 * residual, in the caller's units, computed on the device by one pass over the resident image (the residual pair's pass):
 *   Farkas max_j |ldexp((A^T.yh + zh)_j, -kc[j])| over all n columns (a slack column contributes yh_i + zh_s,i), ray
 *   max_i |ldexp((A.xh)_i, -kr[i])| over the m rows.
 * lpipm_get_certificate: resident member `member` (0 for a single LP) to host arrays (each nullable; info_out required).
 * lpipm_get_certificate_device: all members at once, member i's yh at y_dev + i * ldy doubles, its zh or xh at
 *   col_dev + i * ldc (ldy >= m, ldc >= n; either pointer may be NULL), complete on return; the rows of a kind NONE member stay
 *   untouched.  info_out: a host array of one record per resident member (required).
 * Every member comes out bit-identical -- y, col and the whole record -- to the single upload + lpipm_solve +
 *   lpipm_get_certificate of that member alone, by either entry.
 * Return codes.  First lpipm_get_duals's checks in its order: a null context LPIPM_ERR_BAD_ARGUMENT, nothing resident
 *   LPIPM_ERR_NO_PROBLEM, a column-split context LPIPM_ERR_UNSUPPORTED, no completed solve since the last event that changes
 *   what the iterate means (the list above) LPIPM_ERR_NO_PROBLEM.  Then LPIPM_ERR_BAD_ARGUMENT: member >= the resident count, a
 *   null info_out, ldy < m, ldc < n, a device destination that is not device memory of the context's device or does not hold
 *   every row (checked before anything is enqueued).  Otherwise LPIPM_OK, and info.kind says what was written.
 * Served: every resident form and solver arm lpipm_get_duals serves.  Not served: lpipm_solve_batch*, lpipm_solve_f32,
 *   column-split contexts.
 * Cost: five short launches and one pass over the resident image (shared images: one read per group of members).  In the
 *   arenas it writes reduction slots 0-3, the slabs of the pass and three work vectors below m and n, all of which every
 *   iteration rewrites before it reads them; the iterate, b, c and every padding are only read: lpipm_get_duals and the next
 *   solve find what they would have found. */
enum { LPIPM_CERT_NONE = 0, LPIPM_CERT_FARKAS = 1, LPIPM_CERT_RAY = 2 };
typedef struct { double scale, residual, tau, kappa; int32_t kind, status; } lpipm_cert_info;   /* 40 bytes */
int lpipm_get_certificate(lpipm_ctx* ctx, uint64_t member, double* y_out /* m, nullable */, double* col_out /* n, nullable */,
                          lpipm_cert_info* info_out /* required */);
int lpipm_get_certificate_device(lpipm_ctx* ctx, void* y_dev /* nullable */, uint64_t ldy, void* col_dev /* nullable */,
                                 uint64_t ldc, lpipm_cert_info* info_out /* host, one per resident member, required */);

/* Device bytes the context holds for its resident problem(s) (arenas + shared matrix with the batch's one kept first factor +
 * factor workspace, and the exponent block of lpipm_set_scaling while scaling is on); 0 before any upload. */
int lpipm_get_resident_bytes(const lpipm_ctx* ctx, uint64_t* bytes_out);
/* lpipm_solve_batch with device-resident results: member i's x / tau goes to x_dev_out + i * row_stride doubles
 * (row_stride >= max n[i]); everything else as lpipm_solve_batch. */
int lpipm_solve_batch_device(lpipm_ctx* ctx, uint64_t count, const uint64_t* m, const uint64_t* n,
                             const double* const* A, const double* const* b, const double* const* c,
                             const double* c0 /* nullable */, const lpipm_opts* opts, void* x_dev_out,
                             uint64_t row_stride, double* fun_out /* nullable */, uint64_t* iterations_out /* nullable */,
                             int32_t* status_out);
/* lpipm_solve_batch / lpipm_solve_batch_device with a per-member structural hint (n_slack nullable = all 0; semantics of
 * lpipm_upload_slack, linear_program.rs:145-161).  Each member's hint is verified first; members are then grouped into
 * lockstep batches by (m, n, the hint that holds), and members solved one at a time are uploaded with their hint.
 * Exactly one of x_slack_out (host rows, as lpipm_solve_batch) and x_dev_out (+ row_stride, as lpipm_solve_batch_device)
 * is non-null.  Each member bit-identical to lpipm_upload_slack (its hint) + lpipm_solve. */
int lpipm_solve_batch_slack(lpipm_ctx* ctx, uint64_t count, const uint64_t* m, const uint64_t* n, const uint64_t* n_slack,
                            const double* const* A, const double* const* b, const double* const* c,
                            const double* c0 /* nullable */, const lpipm_opts* opts, double* const* x_slack_out,
                            void* x_dev_out, uint64_t row_stride, double* fun_out, uint64_t* iterations_out,
                            int32_t* status_out);
/* A shard of independent tall inequality-form LPs (pure `ub`): member i is A_ub[i] (m_ub[i] x n[i] row-major, lda = n[i]),
 * b_ub[i] (m_ub[i] doubles), c[i] (the n[i] structural costs), c0[i].  Output conventions of lpipm_solve_batch_slack: exactly
 * one of x_slack_out and x_dev_out (+ row_stride) is non-null, member i's x has n[i] + m_ub[i] entries, slack values last, and
 * row_stride is at least the largest of those lengths.  Members of equal (m_ub, n) are solved as lockstep chunks of
 * lpipm_upload_lockstep_ub_tall, the others one at a time through lpipm_upload_ub_tall on the worker contexts; chunk sizes, the
 * two-context upload pipeline, lpipm_set_batch_lockstep, lpipm_set_batch_concurrency and the treatment of a member's bad
 * arguments, of m_ub[i] == 0 (LPIPM_UNCONSTRAINED in status_out[i]) and of runtime codes are those of lpipm_solve_batch.  Each
 * member bit-identical to lpipm_upload_ub_tall + lpipm_solve, at every max_group. */
int lpipm_solve_batch_ub_tall(lpipm_ctx* ctx, uint64_t count, const uint64_t* m_ub, const uint64_t* n,
                              const double* const* A_ub, const double* const* b_ub, const double* const* c,
                              const double* c0 /* nullable */, const lpipm_opts* opts, double* const* x_slack_out,
                              void* x_dev_out, uint64_t row_stride, double* fun_out, uint64_t* iterations_out,
                              int32_t* status_out);
/* lpipm_solve_batch groups members of equal shape into lockstep batches: max_group -1 = auto (default: chunks
 * of up to 32 within the memory budget, the upload of one chunk overlapping the solve of the previous one), 0 = never, > 0 = largest group. */
int lpipm_set_batch_lockstep(lpipm_ctx* ctx, int max_group);

/* Number of LPs of a batch in flight at once on the device (0 = auto, the default: 8 for members up
 * to m = 2048, else 2; 1 = strictly one after the other).  Members of a batch are independent, each in-flight member has its own stream and buffers. */
int lpipm_set_batch_concurrency(lpipm_ctx* ctx, int nworkers);

/* Profiling switch (off by default) and the per-phase device times of the last solve: HIP events on the
 * context's own stream.  on = 1: every phase (~14 events per iteration); on = 2: only the A.D.A^T launches
 * (2 events per iteration; the other phases are lumped into vec_ms). */
int lpipm_set_profiling(lpipm_ctx* ctx, int on);
int lpipm_get_phase_times(const lpipm_ctx* ctx, lpipm_phase_times* out);

/* ---- kernel-granularity entry points ---------------------------------------------------------
 * Each runs ONE stage of the hot path on the uploaded problem / the given operands so that the
 * parity tests can compare it with the oracle's restatement of the cited reference lines.
 * Host pointers in, host pointers out (copies are outside any timing the library reports).
 * An `ms_out` (nullable) is device time between two HIP events on the context's stream, taken in one of two ways:
 *   per repeat    what the entry launches is bracketed and the stream drained `repeats` (>= 1) times over, one after the other;
 *                 the mean of the brackets.  lpipm_k_adat, lpipm_k_potrf, lpipm_k_chol_solve, lpipm_k_gemv_n, lpipm_k_gemv_t,
 *                 lpipm_k_gemv_dual, lpipm_k_mfma_f64_probe (three repeats) and lpipm_k_qr_solve (one).  What a repeat needs put
 *                 back first (the matrix lpipm_k_potrf factors in place, the right-hand sides lpipm_k_chol_solve overwrites) is
 *                 enqueued ahead of its bracket.
 *   back to back  one bracket around `repeats` launches enqueued without a drain between them, divided by `repeats`.
 *                 lpipm_k_pack_matrix only. */

/* newton_equations.rs:54-57:  M = A . diag(dinv) . A^T.  dinv[n]; M_out m x m row-major, LOWER
 * triangle valid (the strict upper triangle is unspecified).  ms_out: the launches of one build, per repeat. */
int lpipm_k_adat(lpipm_ctx* ctx, const double* dinv, double* M_out, int repeats, double* ms_out);   /* tall upload: LPIPM_ERR_UNSUPPORTED */
/* The resident image of the stored structural block of member `member` (0 for a single LP and for a shared-matrix batch), as
 * the solves read it: mp x npa doubles (rows padded to 128, stored columns to 16, zeros beyond m and the stored columns), after
 * any equilibration.  Copies its top-left rows x cols to out (leading dimension ld >= cols) and reports the padded shape in
 * mp_out / npa_out (nullable).  rows > mp, cols > npa, ld < cols or a member that does not exist: LPIPM_ERR_BAD_ARGUMENT;
 * LPIPM_ERR_NO_PROBLEM without an upload. */
int lpipm_k_resident_matrix(lpipm_ctx* ctx, uint64_t member, uint64_t rows, uint64_t cols, double* out, uint64_t ld,
                            uint64_t* mp_out, uint64_t* npa_out);
/* The launch of lpipm_upload_device that moves A (both blocks of the UB_EQ form) into the resident image, alone and timed:
 * `repeats` (>= 1) back-to-back launches between two HIP events, the mean per launch in pack_ms_out; then, the same way, as
 * many hipMemcpyDtoDAsync calls over as many bytes as one launch reads and writes together (half of them each way) between two
 * scratch allocations, in copy_ms_out: the runtime's copy is the yardstick of the kernel (profiles/device_upload.md).  The
 * resident problem must be the one lpipm_upload_device made from this very descriptor -- the image is rewritten with the
 * values it holds; another shape is LPIPM_ERR_BAD_ARGUMENT, a scaled upload or a column-split context
 * LPIPM_ERR_UNSUPPORTED.  The descriptor is checked as lpipm_upload_device checks it. */
int lpipm_k_pack_matrix(lpipm_ctx* ctx, const lpipm_device_problem* d, int repeats, double* pack_ms_out, double* copy_ms_out);
/* On a single tall upload (lpipm_upload_ub_tall or lpipm_upload_ub_eq_tall; not a batch), with nx its structural columns, m_ub
 * its `ub` rows, n = nx + m_ub and dinv[n] = x / z:
 * K_out (nx x nx row-major, LOWER triangle valid) = X^T.diag(1 / dinv_s).X + diag(1 / dinv_x), from the `ub` rows.  Any other
 * upload: LPIPM_ERR_UNSUPPORTED. */
int lpipm_k_tall_normal(lpipm_ctx* ctx, const double* dinv, double* K_out);
/* The reduced sym_solve (newton_equations.rs:214-225) on a tall upload at the given dinv[n], for nrhs (1|2) right-hand sides:
 * R1 nrhs x n, R2 nrhs x m -> U_out nrhs x n, V_out nrhs x m, with M.V = R2 + A.(dinv * R1), U = dinv * (A^T.V - R1) in exact
 * arithmetic.  info_out (nullable): pivot failure of K as lpipm_k_potrf.  The iterate of the context is overwritten.
 * After lpipm_upload_ub_eq_tall m = m_ub + m_eq: R2 and V_out carry the `eq` entries behind the `ub` ones, and info_out also
 * reports a failed pivot of S. */
int lpipm_k_tall_sym_solve(lpipm_ctx* ctx, const double* dinv, int nrhs, const double* R1, const double* R2, double* U_out,
                           double* V_out, int32_t* info_out);
/* After lpipm_upload_ub_eq_tall with m_eq > 0: builds K at dinv[n], factors it and returns the Schur complement
 * S_out (m_eq x m_eq row-major, LOWER triangle valid) = A_eq.K^-1.A_eq^T, as built (before its own factorisation).  Any other
 * upload, a batch of such LPs included: LPIPM_ERR_UNSUPPORTED.  The iterate of the context is overwritten. */
int lpipm_k_tall_schur(lpipm_ctx* ctx, const double* dinv, double* S_out);
/* On a bounded upload (lpipm_upload_bounded with nb > 0), with m = m_ub + m_eq, n = nx + m_ub and dinv_ext[n + nb] = x / z of
 * the explicit LP's columns (the bound slacks last): M_out (m x m row-major, LOWER triangle valid) = M~ = A.diag(D~).A^T,
 * D~_j = 1 / (1 / dinv_ext[j] + 1 / dinv_ext[n + k]) on the k-th bounded column, dinv_ext[j] elsewhere.  Any other upload:
 * LPIPM_ERR_UNSUPPORTED.  The iterate of the context is overwritten. */
int lpipm_k_bounded_normal(lpipm_ctx* ctx, const double* dinv_ext, double* M_out);
/* The reduced sym_solve on a bounded upload at the given dinv_ext[n + nb], for nrhs (1|2) right-hand sides of the explicit LP:
 * R1 nrhs x (n + nb), R2 nrhs x (m + nb) -> U_out nrhs x (n + nb), V_out nrhs x (m + nb), with M_ext.V = R2 + A_ext.(dinv_ext * R1),
 * U = dinv_ext * (A_ext^T.V - R1) in exact arithmetic.  info_out (nullable): pivot failure of M~ as lpipm_k_potrf.  The iterate
 * of the context is overwritten. */
int lpipm_k_bounded_sym_solve(lpipm_ctx* ctx, const double* dinv_ext, int nrhs, const double* R1, const double* R2, double* U_out,
                              double* V_out, int32_t* info_out);
/* newton_equations.rs:129-131: in-place lower Cholesky of the m x m row-major matrix M (lower
 * triangle read, lower triangle written).  info_out: 0, or k+1 for the first non-positive pivot.
 * ms_out: the factorisation's launches, per repeat. */
int lpipm_k_potrf(lpipm_ctx* ctx, uint64_t m, double* M_inout, int32_t* info_out, int repeats,
                  double* ms_out);
/* After lpipm_k_potrf at size m on this ctx: the explicit inverses of the factor's diagonal super-blocks as the solves read
 * them.  inv_out, invT_out: mp x mp row-major (mp = m rounded up to 128), zero but for the diagonal super-blocks, which
 * hold inv(L_ss) and inv(L_ss)^T.  super_w_out (nullable): the super-block width. */
int lpipm_k_factor_inverses(lpipm_ctx* ctx, uint64_t m, double* inv_out, double* invT_out, int32_t* super_w_out);
/* lpipm_k_potrf of `count` (1..64) m x m matrices (Ms_inout: count x m x m) as ONE lockstep batch: the launches of a lockstep
 * solve's factorisation, every member in its own arena.  infos_out[count]. */
int lpipm_k_potrf_lockstep(lpipm_ctx* ctx, uint64_t m, int count, double* Ms_inout, int32_t* infos_out);
/* Z = B . L^-T with a member dimension, as a lockstep batch of tall LPs with equality rows forms its members' Zt: factors the
 * `count` (1..64) n x n SPD matrices Ms (count x n x n) as lpipm_k_potrf_lockstep does, then runs ONE substitution launch over
 * the members.  B: one rows x cols block (row-major, ld ldb, cols <= n) for all members when shared_b, else `count` of them
 * rows * ldb doubles apart.  Z_inout: count blocks of round_up(rows, 16) x round_up(n, 128) doubles (row r of block q solves
 * L_q.z = B_q[r, :]^T; columns beyond n and rows beyond `rows` come back zero).  What a block holds on entry is what that
 * member's Z holds before the launch.  done_mask (nullable): one int per member, non-zero marks it finished -- its block comes
 * back as it went in.  Member q's Z is bit-identical to a call with count == 1 on Ms[q], whatever the count and the mask.
 * infos_out[count]: the factorisations' pivot words. */
int lpipm_k_trsm_lt_lockstep(lpipm_ctx* ctx, uint64_t n, int count, int rows, int cols, int shared_b, const double* Ms,
                             const double* B, uint64_t ldb, double* Z_inout, int32_t* infos_out,
                             const int32_t* done_mask /* nullable */);
/* newton_equations.rs:151-169: V[r] = L^-T L^-1 R[r] for nrhs (1 or 2) right-hand sides, with
 * L = the factor of a preceding lpipm_k_potrf on this ctx (kept on device).  R, V: nrhs x m.
 * ms_out: the sweep's launches, per repeat. */
int lpipm_k_chol_solve(lpipm_ctx* ctx, uint64_t m, int nrhs, const double* R, double* V,
                       int repeats, double* ms_out);
/* The same solve as two calls of the sweep: the forward steps [0, split) of the super-blocks, then the rest of the forward
 * sweep and the backward one (how the solver runs the predictor's first steps beside the factorisation).  Same bits as
 * lpipm_k_chol_solve whatever the split. */
int lpipm_k_chol_solve_split(lpipm_ctx* ctx, uint64_t m, int nrhs, const double* R, double* V, int split);
/* The launches of the triangular sweep for an m x m factor with super-blocks of width super_w (a multiple of 128), as numbers;
 * needs no device.  coupled: 0 the plain sweep, 1 both sweeps coupled, 2 the backward one alone (the solver's choice for a
 * single LP from m = 4096; the forward sweep is then the plain recurrence, listed as two launches per step), 3 the forward
 * one alone (the plain backward sweep is not listed).
 * out (cap int32): nsb, coupled (0 when the shape has one super-block), the number of launches; then per
 * launch {0 forward | 1 backward, super-block of the step, pieces, workgroups} and per piece {rows, columns of the first term,
 * columns of the second term (0: none), first vector's offset, whether it is in the scratch, second vector's offset (-1:
 * none), in the scratch, addend's offset (-1: none), in the scratch, output's offset, in the scratch, first workgroup}; then per
 * super-block {first row of its transposed block column (-1: none), that copy's row length, has H, has G}.  An uncoupled plan
 * has no launches listed.  count_out: numbers written.  coupling_bytes_out (nullable): bytes of the coupling blocks. */
int lpipm_k_sweep_plan(uint64_t m, int super_w, int coupled, int32_t* out, int cap, int32_t* count_out,
                       uint64_t* coupling_bytes_out);
/* The residual of the refinement step of the Cholesky solve (solver.hip chol_solve_refined): Rho[q] = R0[q] - M.V[q],
 * q < nrhs (1|2), for a symmetric m x m row-major M of which only the LOWER triangle is read.  V, R0, Rho: nrhs x m. */
int lpipm_k_symv_residual(lpipm_ctx* ctx, uint64_t m, const double* M, int nrhs, const double* V, const double* R0, double* Rho);
/* newton_equations.rs:133-149, :155-166 (the Inverse / LeastSquares arms): V[r] = R^-1 Q^T R[r] with
 * M = QR a Householder factorisation of the symmetric m x m matrix M (row-major; only the lower
 * triangle is read), nrhs 1|2, m <= 16384.  info_out: 0, or k+1 for a zero column / zero R[k][k].
 * ms_out: factorisation and solves in one bracket (one repeat). */
int lpipm_k_qr_solve(lpipm_ctx* ctx, uint64_t m, const double* M, int nrhs, const double* R, double* V,
                     int32_t* info_out, double* ms_out);
/* A.w (feasible_point.rs:122, newton_equations.rs:220, residual.rs:23): nrhs (1|2) vectors,
 * W nrhs x n -> Y nrhs x m.  ms_out (also of lpipm_k_gemv_t and lpipm_k_gemv_dual): one pass, per repeat. */
int lpipm_k_gemv_n(lpipm_ctx* ctx, int nrhs, const double* W, double* Y, int repeats, double* ms_out);
/* A^T.v (feasible_point.rs:123, newton_equations.rs:223, residual.rs:25): V nrhs x m -> U nrhs x n */
int lpipm_k_gemv_t(lpipm_ctx* ctx, int nrhs, const double* V, double* U, int repeats, double* ms_out);
/* One loop body of solve_normal_form (mod.rs:215-222) on the uploaded problem from a GIVEN iterate: get_delta
 * (feasible_point.rs:110-152: residuals, normal equations + factor, Rhat::predictor / corrector, Delta::compute twice,
 * update_gamma), the step length (mod.rs:216-221, feasible_point.rs:53-72) and do_step (:76-106).
 * In/out: x[n], y[m], z[n], *tau, *kappa.  Out: the corrector's direction d_x[n], d_y[m], d_z[n],
 * d_tk = {d_tau, d_kappa}, *alpha, *info (pivot failure as lpipm_k_potrf).  Differential tests of the vector stage.
 * On a column-split context (lpipm_upload_nsplit) every rank must call it together: x, z, d_x, d_z are the rank's
 * slices of n_local elements; y[m], tau, kappa and every other output are replicated, bit-identical on all ranks.
 * A group wait of the pipelined reduction of M that gave up is reported as in lpipm_solve (LPIPM_ERR_HIP).
 * A lockstep batch is refused (LPIPM_ERR_UNSUPPORTED). */
int lpipm_k_iteration(lpipm_ctx* ctx, const lpipm_opts* opts, int ip, double* x, double* y, double* z, double* tau,
                      double* kappa, double* d_x, double* d_y, double* d_z, double* d_tk, double* alpha_out,
                      int32_t* info_out);
/* residual.rs:23,25 / feasible_point.rs:122-123 in ONE read of A: Aw_out[m] = A.w, ATv_out[n] = A^T.v (w[n], v[m]). */
int lpipm_k_gemv_dual(lpipm_ctx* ctx, const double* w, const double* v, double* Aw_out, double* ATv_out, int repeats,
                      double* ms_out);
/* ---- InteriorPoint<f32> ------------------------------------------------------------------------
 * src/float.rs:42-43 (`impl Float for f32`): the reference's solver is generic over F; with F = f32 every operation of
 * interior_point/mod.rs:161-168, :199-240 runs in f32.  lpipm_solve_f32 is that instantiation: the same algorithm as
 * lpipm_solve with every operation in f32, on generic (scalar-type-templated) HIP kernels -- correctness first, like the
 * QR arms; the hand-written fp64 path is the fast one.  The slack-form problem (A m x n row-major, lda >= n) is uploaded,
 * solved and released inside the call.  opts: tol and alpha0 are converted to f32; only the Cholesky arm (the default).
 * Return codes as lpipm_solve; x_slack_out[n] = x / tau (also for LPIPM_ITERATION_LIMIT); log nullable, max_iter rows.
 * NOTE (reference behaviour, not a property of this backend): with the default tol = 1e-8 an f32 solve cannot satisfy the
 * optimality test (f32 epsilon is 6e-8): it ends in IterationLimitExceeded or NumericalProblem; pass a tolerance f32 can
 * reach (1e-4 .. 1e-5). */
int lpipm_solve_f32(lpipm_ctx* ctx, uint64_t m, uint64_t n, const float* A_rowmajor, uint64_t lda, const float* b,
                    const float* c, float c0, const lpipm_opts* opts, float* x_slack_out, float* fun_out,
                    uint64_t* iterations_out, lpipm_iter_row_f32* log);
/* Test hook: the SAME generic kernels instantiated for double (solver_generic.hip), so that they can be checked against
 * the fp64 oracle to 1e-8 -- which f32 arithmetic itself cannot show. */
int lpipm_k_generic_solve_f64(lpipm_ctx* ctx, uint64_t m, uint64_t n, const double* A_rowmajor, uint64_t lda, const double* b,
                              const double* c, double c0, const lpipm_opts* opts, double* x_slack_out, double* fun_out,
                              uint64_t* iterations_out, lpipm_iter_row* log);

/* fp64 MFMA issue-rate probe (v_mfma_f64_16x16x4_f64 back to back, operands in registers):
 * tflops_out = achieved TFLOP/s over the whole chip; used to confirm the roofline denominator.  ms_out: one launch, per
 * repeat, three repeats. */
int lpipm_k_mfma_f64_probe(lpipm_ctx* ctx, int iters, double* tflops_out, double* ms_out);

/* ---- synthetic inputs (SURVEY.md 8d / BASELINE.md 3) -----------------------------------------
 * Equality-form planted LP with a strictly complementary optimum: A_ij ~ N(0,1); basis B of m
 * columns; x*_B ~ U(1,2), x*_N = 0; y* ~ N(0,1); z*_N ~ U(1,2), z*_B = 0; b = A x*, c = A^T y* + z*.
 * splitmix64 -> xoshiro256**, Box-Muller, Fisher-Yates.  Host-side; A m x n row-major.
 * xstar_out (n) is nullable. */
int lpipm_synth_planted_lp(uint64_t seed, uint64_t m, uint64_t n, double* A_out, double* b_out,
                           double* c_out, double* xstar_out);

#ifdef __cplusplus
}
#endif
#endif /* LPIPM_H */
