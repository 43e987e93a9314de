//! `extern "C"` surface of include/lpipm.h (only what the shim calls).
//! The crate denies `unsafe_code` (.cargo/config.toml:6); this module is the one scoped exception.
#![allow(unsafe_code, non_camel_case_types)]

use std::os::raw::{c_char, c_int, c_void};

#[repr(C)]
pub struct lpipm_ctx {
    _private: [u8; 0],
}

/// include/lpipm.h `lpipm_opts` == InteriorPointBuilder fields (interior_point/mod.rs:41-48)
#[repr(C)]
#[derive(Clone, Copy)]
pub struct lpipm_opts {
    pub tol: f64,
    pub alpha0: f64,
    pub max_iter: u64,
    pub ip: i32,
    pub solver_type: i32,
    pub disp: i32,
}

/// include/lpipm.h `lpipm_dual_info` (32 bytes): dual_fun = b.(y / tau) + c0, the iterate's tau and kappa, the member's status
#[repr(C)]
#[derive(Clone, Copy, Default)]
pub struct lpipm_dual_info {
    pub dual_fun: f64,
    pub tau: f64,
    pub kappa: f64,
    pub status: i32,
    pub reserved: i32,
}

/// include/lpipm.h `lpipm_cert_info` (40 bytes): scale = b.y or -c.x, the ray's residual in the caller's units, the iterate's
/// tau and kappa, kind (LPIPM_CERT_*), the member's status
#[repr(C)]
#[derive(Clone, Copy, Default)]
pub struct lpipm_cert_info {
    pub scale: f64,
    pub residual: f64,
    pub tau: f64,
    pub kappa: f64,
    pub kind: i32,
    pub status: i32,
}
pub const LPIPM_CERT_NONE: i32 = 0;
pub const LPIPM_CERT_FARKAS: i32 = 1;
pub const LPIPM_CERT_RAY: i32 = 2;

/// include/lpipm.h `lpipm_iter_row` (indicators.rs:8-23 + alpha)
#[repr(C)]
#[derive(Clone, Copy, Default)]
pub struct lpipm_iter_row {
    pub alpha: f64,
    pub rho_p: f64,
    pub rho_d: f64,
    pub rho_a: f64,
    pub rho_g: f64,
    pub rho_mu: f64,
    pub obj: f64,
}

/// include/lpipm.h `lpipm_dev_matrix`: a strided matrix in device memory (strides in elements of the source type)
#[repr(C)]
#[derive(Clone, Copy)]
pub struct lpipm_dev_matrix {
    pub ptr: *const c_void,
    pub row_stride: i64,
    pub col_stride: i64,
    pub member_stride: i64,
}

/// include/lpipm.h `lpipm_dev_vector`
#[repr(C)]
#[derive(Clone, Copy)]
pub struct lpipm_dev_vector {
    pub ptr: *const c_void,
    pub stride: i64,
    pub member_stride: i64,
}

/// include/lpipm.h `lpipm_device_problem`: what lpipm_upload_device makes resident (struct_size = size_of::<Self>())
#[repr(C)]
#[derive(Clone, Copy)]
pub struct lpipm_device_problem {
    pub struct_size: u32,
    pub form: u32,
    pub src_type: u32,
    pub shared: u32,
    pub count: u64,
    pub m: u64,
    pub m_eq: u64,
    pub n: u64,
    pub n_slack: u64,
    pub a: lpipm_dev_matrix,
    pub a_eq: lpipm_dev_matrix,
    pub b: lpipm_dev_vector,
    pub c: lpipm_dev_vector,
    pub c0: *const f64,
}

pub const LPIPM_FORM_SLACK: u32 = 0;
pub const LPIPM_FORM_UB_EQ: u32 = 1;
pub const LPIPM_FORM_UB_TALL: u32 = 2;
pub const LPIPM_SRC_F64: u32 = 0;
pub const LPIPM_SRC_F32: u32 = 1;

pub const LPIPM_OK: c_int = 0;
pub const LPIPM_UNCONSTRAINED: c_int = 1;
pub const LPIPM_NUMERICAL_PROBLEM: c_int = 2;
pub const LPIPM_INVALID_PARAMETER: c_int = 3;
pub const LPIPM_INCOMPATIBLE_DIMENSIONS: c_int = 4;
pub const LPIPM_INFEASIBLE: c_int = 5;
pub const LPIPM_UNBOUNDED: c_int = 6;
pub const LPIPM_ITERATION_LIMIT: c_int = 7;

extern "C" {
    pub fn lpipm_create(device: c_int, out: *mut *mut lpipm_ctx) -> c_int;
    pub fn lpipm_destroy(ctx: *mut lpipm_ctx);
    pub fn lpipm_upload(
        ctx: *mut lpipm_ctx, m: u64, n: u64, a: *const f64, lda: u64, b: *const f64, c: *const f64, c0: f64,
    ) -> c_int;
    pub fn lpipm_upload_slack(
        ctx: *mut lpipm_ctx, m: u64, n: u64, a: *const f64, lda: u64, b: *const f64, c: *const f64, c0: f64,
        n_slack: u64,
    ) -> c_int;
    pub fn lpipm_upload_ub_eq(
        ctx: *mut lpipm_ctx, n: u64, m_ub: u64, a_ub: *const f64, lda_ub: u64, b_ub: *const f64, m_eq: u64,
        a_eq: *const f64, lda_eq: u64, b_eq: *const f64, c: *const f64, c0: f64,
    ) -> c_int;
    /// The tall inequality form: `ub` rows only, many more rows than columns; lpipm_solve then factors the n x n reduced
    /// system K = X^T W_s X + E_x instead of the m_ub x m_ub normal matrix (Cholesky arm only; see include/lpipm.h).
    pub fn lpipm_upload_ub_tall(
        ctx: *mut lpipm_ctx, n: u64, m_ub: u64, a_ub: *const f64, lda_ub: u64, b_ub: *const f64, c: *const f64, c0: f64,
    ) -> c_int;
    /// The tall form with equality rows: K on the `ub` rows as lpipm_upload_ub_tall, the m_eq `eq` rows through the Schur
    /// complement S = A_eq K^-1 A_eq^T on K's factor (arguments of lpipm_upload_ub_eq; m_eq == 0: lpipm_upload_ub_tall itself).
    pub fn lpipm_upload_ub_eq_tall(
        ctx: *mut lpipm_ctx, n: u64, m_ub: u64, a_ub: *const f64, lda_ub: u64, b_ub: *const f64, m_eq: u64,
        a_eq: *const f64, lda_eq: u64, b_eq: *const f64, c: *const f64, c0: f64,
    ) -> c_int;
    /// The bounded form: lpipm_upload_ub_eq's LP with upper bounds on nb of its structural columns (upper[n], +inf = none).  The
    /// bound block is eliminated in closed form, so the normal matrix stays m x m; x_slack has n + m_ub + nb entries, the bound
    /// slacks last, y of lpipm_get_duals m + nb (Cholesky arm only; nb == 0 is lpipm_upload_ub_eq itself; see include/lpipm.h).
    pub fn lpipm_upload_bounded(
        ctx: *mut lpipm_ctx, n: u64, m_ub: u64, a_ub: *const f64, lda_ub: u64, b_ub: *const f64, m_eq: u64,
        a_eq: *const f64, lda_eq: u64, b_eq: *const f64, c: *const f64, c0: f64, upper: *const f64,
    ) -> c_int;
    /// General column bounds lower[n] <= x <= upper[n] (null lower: zeros, null upper: +inf; -inf / +inf = no such end): shifts,
    /// reflections and free columns without growing the normal matrix or storing a column twice.  x_slack has n + m_ub + nb + nf
    /// entries -- the structural values in the caller's variables, the `ub` slacks, the bound slacks, the free columns' negative
    /// parts --, y of lpipm_get_duals m + nb.  lower_j > upper_j: LPIPM_INFEASIBLE from the upload (see include/lpipm.h).
    pub fn lpipm_upload_bounds(
        ctx: *mut lpipm_ctx, n: u64, m_ub: u64, a_ub: *const f64, lda_ub: u64, b_ub: *const f64, m_eq: u64,
        a_eq: *const f64, lda_eq: u64, b_eq: *const f64, c: *const f64, c0: f64, lower: *const f64, upper: *const f64,
    ) -> c_int;
    /// Kernel entries of a bounded upload: M~ (m x m, lower triangle) at dinv_ext[n + nb], and its reduced sym_solve.
    pub fn lpipm_k_bounded_normal(ctx: *mut lpipm_ctx, dinv_ext: *const f64, m_out: *mut f64) -> c_int;
    pub fn lpipm_k_bounded_sym_solve(
        ctx: *mut lpipm_ctx, dinv_ext: *const f64, nrhs: c_int, r1: *const f64, r2: *const f64, u_out: *mut f64,
        v_out: *mut f64, info_out: *mut i32,
    ) -> c_int;
    pub fn lpipm_solve(
        ctx: *mut lpipm_ctx, opts: *const lpipm_opts, x_slack_out: *mut f64, fun_out: *mut f64,
        iterations_out: *mut u64, log: *mut lpipm_iter_row,
    ) -> c_int;
    /// InteriorPoint<f32> (src/float.rs:42-43): the same algorithm with every operation in f32; upload + solve in one call
    pub fn lpipm_solve_f32(
        ctx: *mut lpipm_ctx, m: u64, n: u64, a: *const f32, lda: u64, b: *const f32, c: *const f32, c0: f32,
        opts: *const lpipm_opts, x_slack_out: *mut f32, fun_out: *mut f32, iterations_out: *mut u64, log: *mut c_void,
    ) -> c_int;
    pub fn lpipm_strerror(status: c_int) -> *const c_char;
    pub fn lpipm_last_error_detail() -> *const c_char;

    // A batch of independent LPs on one device (BASELINE config 4): members of equal shape advance as
    // lockstep batches, one kernel launch covering all of them.
    pub fn lpipm_solve_batch(
        ctx: *mut lpipm_ctx, count: u64, m: *const u64, n: *const u64, a: *const *const f64,
        b: *const *const f64, c: *const *const f64, c0: *const f64, opts: *const lpipm_opts,
        x_slack_out: *const *mut f64, fun_out: *mut f64, iterations_out: *mut u64, status_out: *mut i32,
    ) -> c_int;
    pub fn lpipm_upload_lockstep(
        ctx: *mut lpipm_ctx, count: u64, m: u64, n: u64, a: *const *const f64, b: *const *const f64,
        c: *const *const f64, c0: *const f64,
    ) -> c_int;
    pub fn lpipm_solve_lockstep(
        ctx: *mut lpipm_ctx, opts: *const lpipm_opts, x_slack_out: *const *mut f64, fun_out: *mut f64,
        iterations_out: *mut u64, status_out: *mut i32,
    ) -> c_int;
    // A lockstep batch whose members share ONE constraint matrix (member i = (A, b[i], c[i], c0[i])): A resident once,
    // every pass over it serving the whole batch; solved with lpipm_solve_lockstep, members bit-identical to single solves.
    pub fn lpipm_upload_lockstep_shared(
        ctx: *mut lpipm_ctx, count: u64, m: u64, n: u64, a: *const f64, lda: u64, b: *const *const f64,
        c: *const *const f64, c0: *const f64,
    ) -> c_int;
    // The same batches with the structural hint of lpipm_upload_slack (linear_program.rs:145-161): the slack block [I; 0]
    // of the `ub` rows is verified, then neither stored nor multiplied; members bit-identical to lpipm_upload_slack + lpipm_solve.
    pub fn lpipm_upload_lockstep_slack(
        ctx: *mut lpipm_ctx, count: u64, m: u64, n: u64, a: *const *const f64, b: *const *const f64,
        c: *const *const f64, c0: *const f64, n_slack: u64,
    ) -> c_int;
    pub fn lpipm_upload_lockstep_shared_slack(
        ctx: *mut lpipm_ctx, count: u64, m: u64, n: u64, a: *const f64, lda: u64, b: *const *const f64,
        c: *const *const f64, c0: *const f64, n_slack: u64,
    ) -> c_int;
    // Device-side assembly of a shared-matrix batch: the ub / eq blocks once, b[i] = [b_ub_i; b_eq_i], c[i] = n structural costs.
    pub fn lpipm_upload_lockstep_shared_ub_eq(
        ctx: *mut lpipm_ctx, count: u64, n: u64, m_ub: u64, a_ub: *const f64, lda_ub: u64, m_eq: u64, a_eq: *const f64,
        lda_eq: u64, b: *const *const f64, c: *const *const f64, c0: *const f64,
    ) -> c_int;
    // A lockstep batch of tall inequality-form LPs over ONE A_ub (b[i]: m_ub doubles, c[i]: the n structural costs): A_ub and
    // its transpose resident once, every member factoring its own n x n reduced system; each member bit-identical to
    // lpipm_upload_ub_tall + lpipm_solve of that member alone.
    pub fn lpipm_upload_lockstep_shared_ub_tall(
        ctx: *mut lpipm_ctx, count: u64, n: u64, m_ub: u64, a_ub: *const f64, lda_ub: u64, b: *const *const f64,
        c: *const *const f64, c0: *const f64,
    ) -> c_int;
    // The same batch with `eq` rows in the one image (b[i] = [b_ub_i; b_eq_i]): every member a tall LP with equality rows, its
    // own K and its own Schur complement; each member bit-identical to lpipm_upload_ub_eq_tall + lpipm_solve of that member alone.
    pub fn lpipm_upload_lockstep_shared_ub_eq_tall(
        ctx: *mut lpipm_ctx, count: u64, n: u64, m_ub: u64, a_ub: *const f64, lda_ub: u64, m_eq: u64, a_eq: *const f64,
        lda_eq: u64, b: *const *const f64, c: *const *const f64, c0: *const f64,
    ) -> c_int;
    // The same with one matrix per member (a_ub[i]: m_ub x n, lda_ub): every member keeps its own X, transpose and K.
    pub fn lpipm_upload_lockstep_ub_tall(
        ctx: *mut lpipm_ctx, count: u64, n: u64, m_ub: u64, a_ub: *const *const f64, lda_ub: u64, b: *const *const f64,
        c: *const *const f64, c0: *const f64,
    ) -> c_int;
    // New b / c / c0 (each nullable: stays) for every member of the resident lockstep batch, in its upload's own form; A and
    // the kept first factor stay.  _device: packed row blocks on the device, member i at b_dev + i * ldb doubles.
    pub fn lpipm_update_lockstep_vectors(
        ctx: *mut lpipm_ctx, count: u64, b: *const *const f64, c: *const *const f64, c0: *const f64,
    ) -> c_int;
    pub fn lpipm_update_lockstep_vectors_device(
        ctx: *mut lpipm_ctx, count: u64, b_dev: *const c_void, ldb: u64, c_dev: *const c_void, ldc: u64, c0: *const f64,
    ) -> c_int;
    // Any of the uploads above from DEVICE memory, strided, double or float: (form, shared, count) select the host entry the
    // call is equivalent to; every source pointer is checked against its allocation before anything is launched.
    pub fn lpipm_upload_device(ctx: *mut lpipm_ctx, d: *const lpipm_device_problem) -> c_int;
    // lpipm_update_vectors with b[m], c[n] (doubles, contiguous) in device memory.
    pub fn lpipm_update_vectors_device(ctx: *mut lpipm_ctx, b_dev: *const c_void, c_dev: *const c_void) -> c_int;
    // Test hook: the top-left rows x cols of member's padded resident image (mp x npa) to the host.
    pub fn lpipm_k_resident_matrix(
        ctx: *mut lpipm_ctx, member: u64, rows: u64, cols: u64, out: *mut f64, ld: u64, mp_out: *mut u64, npa_out: *mut u64,
    ) -> c_int;
    // Measuring hook: the launch that packs A, `repeats` times between two events, beside the runtime's copy of as many bytes.
    pub fn lpipm_k_pack_matrix(
        ctx: *mut lpipm_ctx, d: *const lpipm_device_problem, repeats: c_int, pack_ms_out: *mut f64, copy_ms_out: *mut f64,
    ) -> c_int;
    // lpipm_solve_batch with a per-member hint (n_slack nullable); exactly one of x_slack_out and x_dev_out is non-null.
    pub fn lpipm_solve_batch_slack(
        ctx: *mut lpipm_ctx, count: u64, m: *const u64, n: *const u64, n_slack: *const u64, a: *const *const f64,
        b: *const *const f64, c: *const *const f64, c0: *const f64, opts: *const lpipm_opts,
        x_slack_out: *const *mut f64, x_dev_out: *mut c_void, row_stride: u64, fun_out: *mut f64,
        iterations_out: *mut u64, status_out: *mut i32,
    ) -> c_int;
    // A shard of tall inequality-form LPs (a_ub[i]: m_ub[i] x n[i], lda = n[i]; x: n[i] + m_ub[i] entries, slack values last):
    // members of equal shape as lockstep chunks of lpipm_upload_lockstep_ub_tall, the others through lpipm_upload_ub_tall.
    pub fn lpipm_solve_batch_ub_tall(
        ctx: *mut lpipm_ctx, count: u64, m_ub: *const u64, n: *const u64, a_ub: *const *const f64,
        b_ub: *const *const f64, c: *const *const f64, c0: *const f64, opts: *const lpipm_opts,
        x_slack_out: *const *mut f64, x_dev_out: *mut c_void, row_stride: u64, fun_out: *mut f64,
        iterations_out: *mut u64, status_out: *mut i32,
    ) -> c_int;
    // Device bytes held for the resident problem(s): arenas + shared matrix + factor workspace.
    pub fn lpipm_get_resident_bytes(ctx: *const lpipm_ctx, bytes_out: *mut u64) -> c_int;
    // Dual values and reduced costs of the LAST solve on the context, in the caller's units: y_out[m] (rows of the upload, `ub`
    // first), z_out[n] (as long as x_slack_out), each nullable; A^T.y + z = c, z >= 0, d fun / d b_i = y_i.  A member without
    // a solution: its own status is returned and nothing is written.  _device: every resident member at once, member i's y at
    // y_dev + i * ldy doubles, its z at z_dev + i * ldz; info_out a host array of one record per member.
    pub fn lpipm_get_duals(
        ctx: *mut lpipm_ctx, member: u64, y_out: *mut f64, z_out: *mut f64, info_out: *mut lpipm_dual_info,
    ) -> c_int;
    pub fn lpipm_get_duals_device(
        ctx: *mut lpipm_ctx, y_dev: *mut c_void, ldy: u64, z_dev: *mut c_void, ldz: u64, info_out: *mut lpipm_dual_info,
    ) -> c_int;
    // The certificate of the LAST solve on the context for a member that ended Infeasible (kind FARKAS: y_out[m] = y / b.y,
    // col_out[n] = z / b.y; A^T.y + z ~ 0, z >= 0, b.y = 1) or Unbounded (kind RAY: col_out[n] = x / (-c.x); A.x ~ 0, x >= 0,
    // c.x = -1), in the caller's units; kind NONE (any other status, or c.x >= 0): nothing is written.  info_out is required.
    // _device: every resident member at once, member i's y at y_dev + i * ldy doubles, its z or x at col_dev + i * ldc.
    pub fn lpipm_get_certificate(
        ctx: *mut lpipm_ctx, member: u64, y_out: *mut f64, col_out: *mut f64, info_out: *mut lpipm_cert_info,
    ) -> c_int;
    pub fn lpipm_get_certificate_device(
        ctx: *mut lpipm_ctx, y_dev: *mut c_void, ldy: u64, col_dev: *mut c_void, ldc: u64, info_out: *mut lpipm_cert_info,
    ) -> c_int;
    // Power-of-two row / column equilibration of every later upload (passes 1..64; 0 = off, the default), and the int32
    // exponents in use for a resident member: row_exp_out[m], col_exp_out[n].  x comes back in the caller's units.
    pub fn lpipm_set_scaling(ctx: *mut lpipm_ctx, passes: c_int) -> c_int;
    pub fn lpipm_get_scaling(ctx: *const lpipm_ctx, member: u64, row_exp_out: *mut i32, col_exp_out: *mut i32) -> c_int;

    // One LP split by columns over ranks (BASELINE config 5): the caller supplies the all-reduce
    // (e.g. ncclAllReduce on `stream`); op 0 = sum, 1 = min.
    pub fn lpipm_set_collective(
        ctx: *mut lpipm_ctx, rank: c_int, world: c_int,
        f: Option<unsafe extern "C" fn(user: *mut c_void, dev_ptr: *mut c_void, count: u64, op: c_int, stream: *mut c_void) -> c_int>,
        user: *mut c_void,
    ) -> c_int;
    pub fn lpipm_upload_nsplit(
        ctx: *mut lpipm_ctx, m: u64, n_total: u64, n_local: u64, a_local: *const f64, lda: u64,
        b: *const f64, c_local: *const f64, c0: f64,
    ) -> c_int;
}
