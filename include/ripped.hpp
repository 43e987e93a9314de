// ripped.hpp -- header-only C++17 host-side mirror of the public API of sebasv/lp (crate `ripped`
// 0.1.1) for the one path liblpipm.so accelerates, written over the C ABI of lpipm.h.
//
// The reference is compiled Rust and this image has no Rust toolchain, so the host side above the
// C ABI is mirrored in C++ (and in Python, lp_amd/__init__.py): same names, same argument meaning,
// same error behaviour.  A Rust `Result::Err(e)` is a thrown ripped::LinearProgramError whose
// `kind()` is the variant of src/error.rs:10-28.
//
//   reference (Rust)                                      here
//   Problem::target(&c).ub(&A,&b).eq(&A,&b).build()?      Problem::target(c).ub(A,b).eq(A,b).build()
//   InteriorPoint::custom().tol(1e-8)....build()?          InteriorPoint::custom().tol(1e-8)....build()
//   solver.solve(&problem)? -> OptimizeResult              solver.solve(problem) -> OptimizeResult
//   res.x() / res.fun() / res.iteration()                  res.x() / res.fun() / res.iteration()
//
// Matrices are row-major std::vector<F> + (rows, cols), the layout ndarray gives `Problem`.
// The reference is generic over `F: Float` (src/float.rs:8-43, f64 and f32): the classes below are templates over the
// scalar type with the f64 instantiation under the reference's plain names (Problem, Matrix, OptimizeResult) and the f32 one
// as ProblemF32 / MatrixF32 / OptimizeResultF32; InteriorPoint::solve takes either (f64: the hand-written fp64 path,
// f32: lpipm_solve_f32).
#pragma once
#include <type_traits>
#include <cstdint>
#include <stdexcept>
#include <string>
#include <utility>
#include <limits>
#include <vector>

#include "lpipm.h"

namespace ripped {

// src/error.rs:10-28
enum class ErrorKind {
    Unconstrained = LPIPM_UNCONSTRAINED,
    NumericalProblem = LPIPM_NUMERICAL_PROBLEM,
    InvalidParameter = LPIPM_INVALID_PARAMETER,
    IncompatibleInputDimensions = LPIPM_INCOMPATIBLE_DIMENSIONS,
    Infeasible = LPIPM_INFEASIBLE,
    Unbounded = LPIPM_UNBOUNDED,
    IterationLimitExceeded = LPIPM_ITERATION_LIMIT,
    Backend = LPIPM_ERR_HIP  // HIP / driver failure: no analogue in the reference, never swallowed
};

class LinearProgramError : public std::runtime_error {
public:
    LinearProgramError(ErrorKind k, const std::string& msg, std::vector<double> x = {})
        : std::runtime_error(msg), kind_(k), x_(std::move(x)) {}
    ErrorKind kind() const { return kind_; }
    // IterationLimitExceeded(x / tau): error.rs:26-28, interior_point/mod.rs:237-239
    const std::vector<double>& best_x() const { return x_; }

private:
    ErrorKind kind_;
    std::vector<double> x_;
};

// What InteriorPoint::solve_with_certificate hands back with an Infeasible or Unbounded error (lpipm_get_certificate), split as
// ProblemBuilder::build stacks the rows.  kind LPIPM_CERT_FARKAS: y_ub (<= 0), y_eq and z (>= 0, the structural columns) with
// A_ub^T y_ub + A_eq^T y_eq + z ~ 0 and b_ub.y_ub + b_eq.y_eq = 1 -- a feasibility cut.  kind LPIPM_CERT_RAY: x (>= 0, the
// structural columns) with A_ub x <= 0, A_eq x ~ 0, c.x = -1.  kind LPIPM_CERT_NONE: an Unbounded call that proves nothing.
// residual: max |A^T y + z|, respectively max |A x|, over the slack form.  The vectors a kind does not have are empty.
struct Certificate {
    int kind = LPIPM_CERT_NONE;
    std::vector<double> y_ub, y_eq, z, x;
    double scale = 0.0, residual = 0.0;
};
class CertifiedError : public LinearProgramError {
public:
    CertifiedError(ErrorKind k, const std::string& msg, Certificate c) : LinearProgramError(k, msg), cert_(std::move(c)) {}
    const Certificate& certificate() const { return cert_; }

private:
    Certificate cert_;
};

inline void raise_for(int status, std::vector<double> x = {}) {
    if (status == LPIPM_OK) return;
    std::string msg = lpipm_strerror(status);
    if (status >= 100) {
        msg += ": ";
        msg += lpipm_last_error_detail();
        throw LinearProgramError(ErrorKind::Backend, msg);
    }
    throw LinearProgramError(static_cast<ErrorKind>(status), msg, std::move(x));
}

template <class F> struct BasicMatrix {  // row-major, the layout of ndarray's standard Array2
    static_assert(std::is_same<F, double>::value || std::is_same<F, float>::value, "src/float.rs:33-43: f64 and f32");
    std::vector<F> data;
    uint64_t rows = 0, cols = 0;
};

template <class F> class BasicProblemBuilder;

// src/linear_program.rs:24-70
template <class F> class BasicProblem {
public:
    static BasicProblemBuilder<F> target(const std::vector<F>& c);   // :37-39
    const BasicMatrix<F>& A() const { return A_; }                   // :42-44
    const std::vector<F>& b() const { return b_; }                   // :47-49
    const std::vector<F>& c() const { return c_; }                   // :52-54
    F c0() const { return c0_; }                                     // :57-59
    uint64_t n_slack() const { return n_slack_; }
    // Not in the reference: the upper bounds of the structural columns given to ProblemBuilder::upper (+inf: none; empty: no
    // bounds at all) and how many of them are finite.  A(), b() and c() stay the slack form WITHOUT the bounds.
    const std::vector<F>& upper() const { return upper_; }
    uint64_t n_bounded() const { return n_bounded_; }
    // Likewise the lower bounds given to ProblemBuilder::lower (-inf: none; empty: all 0), the columns with neither end, and
    // whether any lower end is not 0: InteriorPoint then uploads through lpipm_upload_bounds.  n_bounded() counts the columns
    // with both ends finite.
    const std::vector<F>& lower() const { return lower_; }
    uint64_t n_free() const { return n_free_; }
    bool general_bounds() const { return general_; }
    // what follows the structural columns in the upload's column vectors: `ub` slacks, bound slacks, negative parts
    uint64_t tail() const { return n_slack_ + n_bounded_ + n_free_; }
    std::vector<F> denormalize_x_into(std::vector<F> x_slack) const {  // :65-69
        x_slack.resize(x_slack.size() - tail());      // (a bounded solve's x_slack ends with the bound slacks, then the x^-)
        return x_slack;
    }

private:
    friend class BasicProblemBuilder<F>;
    BasicMatrix<F> A_;
    std::vector<F> b_, c_;
    F c0_ = 0;
    uint64_t n_slack_ = 0;
    std::vector<F> upper_, lower_;
    uint64_t n_bounded_ = 0, n_free_ = 0;
    bool general_ = false;
};

// src/linear_program.rs:72-170
template <class F> class BasicProblemBuilder {
public:
    explicit BasicProblemBuilder(const std::vector<F>& c) : c_(c) {}
    BasicProblemBuilder& ub(const BasicMatrix<F>& A, const std::vector<F>& b) { ub_A_ = &A; ub_b_ = &b; return *this; }  // :93-96
    BasicProblemBuilder& eq(const BasicMatrix<F>& A, const std::vector<F>& b) { eq_A_ = &A; eq_b_ = &b; return *this; }  // :102-105
    // Not in the reference: upper bounds x_j <= u[j] on the structural columns, one entry per column, +infinity where there is
    // none.  InteriorPoint::solve then runs the bounded form (lpipm_upload_bounded): the normal matrix keeps its order.  f64 only.
    BasicProblemBuilder& upper(const std::vector<F>& u) { upper_ = &u; return *this; }
    // Not in the reference: lower bounds l[j] <= x_j, one entry per column, -infinity where there is none (without this call every
    // lower bound is 0); a column with neither end is free.  InteriorPoint::solve then runs lpipm_upload_bounds and returns x,
    // fun, the duals and the certificates in these variables.  f64 only.
    BasicProblemBuilder& lower(const std::vector<F>& l) { lower_ = &l; return *this; }
    BasicProblem<F> build() const {                                                                               // :125-169
        const uint64_t n = c_.size();
        const uint64_t m_ub = ub_A_ ? ub_A_->rows : 0, m_eq = eq_A_ ? eq_A_->rows : 0;
        if (m_ub + m_eq == 0) raise_for(LPIPM_UNCONSTRAINED);                                                     // :134-136
        if ((ub_A_ && (ub_A_->cols != n || ub_b_->size() != m_ub || ub_A_->data.size() != m_ub * n)) ||
            (eq_A_ && (eq_A_->cols != n || eq_b_->size() != m_eq || eq_A_->data.size() != m_eq * n)))
            raise_for(LPIPM_INCOMPATIBLE_DIMENSIONS);                                                             // :137-143
        BasicProblem<F> p;
        p.A_.rows = m_ub + m_eq;
        p.A_.cols = n + m_ub;
        p.A_.data.assign(p.A_.rows * p.A_.cols, F(0));
        p.b_.resize(p.A_.rows);
        p.c_.assign(p.A_.cols, F(0));
        if constexpr (std::is_same<F, double>::value) {
            raise_for(lpipm_problem_build(n, m_ub, ub_A_ ? ub_A_->data.data() : nullptr, ub_b_ ? ub_b_->data() : nullptr,
                                          m_eq, eq_A_ ? eq_A_->data.data() : nullptr, eq_b_ ? eq_b_->data() : nullptr,
                                          c_.data(), p.A_.data.data(), p.b_.data(), p.c_.data(), &p.n_slack_));
        } else {
            // the slack form of linear_program.rs:145-160 (the C ABI's lpipm_problem_build is the f64 instantiation):
            //   A = [[A_ub, I], [A_eq, 0]], b = [b_ub; b_eq], c = [c; 0]
            const uint64_t nn = p.A_.cols;
            for (uint64_t i = 0; i < m_ub; ++i) {
                for (uint64_t j = 0; j < n; ++j) p.A_.data[i * nn + j] = ub_A_->data[i * n + j];
                p.A_.data[i * nn + n + i] = F(1);
                p.b_[i] = (*ub_b_)[i];
            }
            for (uint64_t i = 0; i < m_eq; ++i) {
                for (uint64_t j = 0; j < n; ++j) p.A_.data[(m_ub + i) * nn + j] = eq_A_->data[i * n + j];
                p.b_[m_ub + i] = (*eq_b_)[i];
            }
            for (uint64_t j = 0; j < n; ++j) p.c_[j] = c_[j];
            p.n_slack_ = m_ub;
        }
        if (upper_ || lower_) {
            const F inf = std::numeric_limits<F>::infinity();
            if ((upper_ && upper_->size() != n) || (lower_ && lower_->size() != n)) raise_for(LPIPM_INCOMPATIBLE_DIMENSIONS);
            p.upper_ = upper_ ? *upper_ : std::vector<F>(n, inf);
            if (lower_) p.lower_ = *lower_;
            for (uint64_t j = 0; j < n; ++j) {
                const F u = p.upper_[j], l = lower_ ? p.lower_[j] : F(0);
                if (u != u || u == -inf || l != l || l == inf) raise_for(LPIPM_INVALID_PARAMETER);
                if (u != inf && l != -inf) ++p.n_bounded_;
                if (u == inf && l == -inf) ++p.n_free_;
                if (l != F(0)) p.general_ = true;
            }
        }
        return p;
    }

private:
    const std::vector<F>& c_;
    const BasicMatrix<F>* ub_A_ = nullptr;
    const std::vector<F>* ub_b_ = nullptr;
    const BasicMatrix<F>* eq_A_ = nullptr;
    const std::vector<F>* eq_b_ = nullptr;
    const std::vector<F>* upper_ = nullptr;
    const std::vector<F>* lower_ = nullptr;
};
template <class F> inline BasicProblemBuilder<F> BasicProblem<F>::target(const std::vector<F>& c) { return BasicProblemBuilder<F>(c); }

// src/solvers/mod.rs:19-49
template <class F> class BasicOptimizeResult {
public:
    BasicOptimizeResult(std::vector<F> x, F fun, uint64_t iteration) : x_(std::move(x)), fun_(fun), iteration_(iteration) {}
    uint64_t iteration() const { return iteration_; }
    F fun() const { return fun_; }
    const std::vector<F>& x() const { return x_; }

private:
    std::vector<F> x_;
    F fun_;
    uint64_t iteration_;
};

using Matrix = BasicMatrix<double>;                 // the reference's Problem<f64>, ...
using Problem = BasicProblem<double>;
using ProblemBuilder = BasicProblemBuilder<double>;
using OptimizeResult = BasicOptimizeResult<double>;
using MatrixF32 = BasicMatrix<float>;               // ... and Problem<f32>
using ProblemF32 = BasicProblem<float>;
using ProblemBuilderF32 = BasicProblemBuilder<float>;
using OptimizeResultF32 = BasicOptimizeResult<float>;

enum class EquationSolverType { Cholesky = 0, Inverse = 1, LeastSquares = 2 };  // newton_equations.rs:37-46

class InteriorPoint;

// src/solvers/interior_point/mod.rs:41-138
class InteriorPointBuilder {
public:
    InteriorPointBuilder() { lpipm_default_opts(&o_); }  // mod.rs:50-60
    InteriorPointBuilder& tol(double v) { o_.tol = v; return *this; }
    InteriorPointBuilder& disp(bool v) { o_.disp = v; return *this; }
    InteriorPointBuilder& ip(bool v) { o_.ip = v; return *this; }
    InteriorPointBuilder& solver_type(EquationSolverType v) { o_.solver_type = static_cast<int32_t>(v); return *this; }
    InteriorPointBuilder& alpha0(double v) { o_.alpha0 = v; return *this; }
    InteriorPointBuilder& max_iter(uint64_t v) { o_.max_iter = v; return *this; }
    InteriorPoint build() const;  // mod.rs:118-137

private:
    lpipm_opts o_;
};

// src/solvers/mod.rs:12-16 (trait Solver) + interior_point/mod.rs:140-241
class InteriorPoint {
public:
    explicit InteriorPoint(const lpipm_opts& o, int device = 0) : o_(o), device_(device) {}
    static InteriorPoint default_() { return InteriorPointBuilder().build(); }  // mod.rs:154-159
    static InteriorPointBuilder custom() { return InteriorPointBuilder(); }     // mod.rs:195-197
    bool operator==(const InteriorPoint& r) const {                             // derive(PartialEq), mod.rs:140
        return o_.tol == r.o_.tol && o_.alpha0 == r.o_.alpha0 && o_.max_iter == r.o_.max_iter && o_.ip == r.o_.ip &&
               o_.solver_type == r.o_.solver_type && o_.disp == r.o_.disp;
    }
    const lpipm_opts& opts() const { return o_; }
    // Opt-in (not in the reference): a problem built from `ub` rows only is uploaded in the tall inequality form
    // (lpipm_upload_ub_tall) -- the solve factors the n x n reduced system instead of the m_ub x m_ub normal matrix.  For LPs
    // with many more rows than columns; Cholesky arm only.  Problems with `eq` rows are solved as before.
    InteriorPoint& tall_form(bool on = true) { tall_ = on; return *this; }
    // A separate opt-in: a problem with `ub` rows and any `eq` rows goes through lpipm_upload_ub_eq_tall -- the n x n reduced
    // system of the `ub` rows, the `eq` rows through a Schur complement on its factor.  For many more `ub` rows than columns and
    // a few `eq` rows; Cholesky arm only.  tall_form() alone keeps solving problems with `eq` rows as before.
    InteriorPoint& tall_eq_form(bool on = true) { tall_eq_ = on; return *this; }

    // mod.rs:161-168.  One context (stream + device buffers) per call keeps `solve(&self)` stateless
    // and re-entrant like the reference; callers that solve many problems can hold an lpipm_ctx.
    OptimizeResult solve(const Problem& problem) const {
        lpipm_ctx* ctx = nullptr;
        raise_for(lpipm_create(device_, &ctx));
        struct Guard { lpipm_ctx* c; ~Guard() { lpipm_destroy(c); } } guard{ctx};
        std::vector<double> x;
        double fun = 0.0;
        uint64_t it = 0;
        upload_and_solve(ctx, problem, x, fun, it);
        return OptimizeResult(problem.denormalize_x_into(std::move(x)), fun, it);  // mod.rs:165-167
    }
    // solve() with the duals of its last iterate (lpipm_get_duals on the same context; tall_form() / tall_eq_form() are
    // honoured): y_ub, y_eq the multipliers of the `ub` and `eq` rows as ProblemBuilder::build stacks them
    // (linear_program.rs:145-158; d fun / d b), reduced_costs those of the structural columns, dual_fun = b.y + c0.
    // A^T y + z = c with z >= 0; the multiplier of a `ub` row is <= 0.  Not in the reference.
    struct DualResult {
        OptimizeResult result;
        std::vector<double> y_ub, y_eq, reduced_costs;
        double dual_fun;
    };
    DualResult solve_with_duals(const Problem& problem) const {
        lpipm_ctx* ctx = nullptr;
        raise_for(lpipm_create(device_, &ctx));
        struct Guard { lpipm_ctx* c; ~Guard() { lpipm_destroy(c); } } guard{ctx};
        std::vector<double> x;
        double fun = 0.0;
        uint64_t it = 0;
        upload_and_solve(ctx, problem, x, fun, it);
        const Matrix& A = problem.A();
        const std::size_t ns = problem.n_slack(), nb = problem.n_bounded();     // (bounded: the bound rows and their slacks come last)
        const std::size_t nf = problem.n_free();                                 // (general bounds: then the negative parts)
        std::vector<double> y(A.rows + nb), z(A.cols + nb + nf);
        lpipm_dual_info info{};
        raise_for(lpipm_get_duals(ctx, 0, y.data(), z.data(), &info));
        return DualResult{OptimizeResult(problem.denormalize_x_into(std::move(x)), fun, it),
                          std::vector<double>(y.begin(), y.begin() + ns), std::vector<double>(y.begin() + ns, y.end() - nb),
                          std::vector<double>(z.begin(), z.end() - ns - nb - nf), info.dual_fun};
    }
    // solve(), but an Infeasible or Unbounded problem throws a CertifiedError (a LinearProgramError of the same kind) that
    // carries the certificate of the solve's last iterate (lpipm_get_certificate on the same context; tall_form() /
    // tall_eq_form() are honoured).  Every other outcome is solve()'s.  Not in the reference.
    OptimizeResult solve_with_certificate(const Problem& problem) const {
        lpipm_ctx* ctx = nullptr;
        raise_for(lpipm_create(device_, &ctx));
        struct Guard { lpipm_ctx* c; ~Guard() { lpipm_destroy(c); } } guard{ctx};
        std::vector<double> x;
        double fun = 0.0;
        uint64_t it = 0;
        const int rc = upload_and_solve_rc(ctx, problem, x, fun, it);
        if (rc == LPIPM_INFEASIBLE || rc == LPIPM_UNBOUNDED) {
            const Matrix& A = problem.A();
            const std::size_t ns = problem.n_slack(), nb = problem.n_bounded();
            const std::size_t nf = problem.n_free();
            std::vector<double> y(A.rows + nb), col(A.cols + nb + nf);
            lpipm_cert_info info{};
            raise_for(lpipm_get_certificate(ctx, 0, y.data(), col.data(), &info));
            Certificate cert;
            cert.kind = info.kind; cert.scale = info.scale; cert.residual = info.residual;
            if (info.kind == LPIPM_CERT_FARKAS) {
                cert.y_ub.assign(y.begin(), y.begin() + ns); cert.y_eq.assign(y.begin() + ns, y.end() - nb);
                cert.z.assign(col.begin(), col.end() - ns - nb - nf);
            } else if (info.kind == LPIPM_CERT_RAY)
                cert.x.assign(col.begin(), col.end() - ns - nb - nf);
            throw CertifiedError(static_cast<ErrorKind>(rc), lpipm_strerror(rc), std::move(cert));
        }
        if (rc == LPIPM_ITERATION_LIMIT) raise_for(rc, x);          // payload: x / tau, mod.rs:237-239
        raise_for(rc);
        return OptimizeResult(problem.denormalize_x_into(std::move(x)), fun, it);
    }
    // The f32 instantiation of the same `solve` (src/float.rs:42-43): every operation in f32, lpipm_solve_f32.  With the
    // default tol = 1e-8 an f32 solve cannot satisfy the optimality test (the reference's behaviour): pass 1e-4 .. 1e-5.
    OptimizeResultF32 solve(const ProblemF32& problem) const {
        lpipm_ctx* ctx = nullptr;
        raise_for(lpipm_create(device_, &ctx));
        struct Guard { lpipm_ctx* c; ~Guard() { lpipm_destroy(c); } } guard{ctx};
        if (problem.n_bounded() > 0 || problem.general_bounds()) raise_for(LPIPM_ERR_UNSUPPORTED);     // the bounded forms have no f32 arm
        const MatrixF32& A = problem.A();
        std::vector<float> x(A.cols);
        float fun = 0.0f;
        uint64_t it = 0;
        const int rc = lpipm_solve_f32(ctx, A.rows, A.cols, A.data.data(), A.cols, problem.b().data(), problem.c().data(),
                                       problem.c0(), &o_, x.data(), &fun, &it, nullptr);
        if (rc == LPIPM_ITERATION_LIMIT) raise_for(rc, std::vector<double>(x.begin(), x.end()));
        raise_for(rc);
        return OptimizeResultF32(problem.denormalize_x_into(std::move(x)), fun, it);
    }

private:
    // What solve() and solve_with_duals() share: upload_and_solve_rc, every status but Ok thrown.
    void upload_and_solve(lpipm_ctx* ctx, const Problem& problem, std::vector<double>& x, double& fun, uint64_t& it) const {
        const int rc = upload_and_solve_rc(ctx, problem, x, fun, it);
        if (rc == LPIPM_ITERATION_LIMIT) raise_for(rc, x);          // payload: x / tau, mod.rs:237-239
        raise_for(rc);
    }
    // The upload of `problem` in the form the opt-ins select, and lpipm_solve.  -> the solve's status
    int upload_and_solve_rc(lpipm_ctx* ctx, const Problem& problem, std::vector<double>& x, double& fun, uint64_t& it) const {
        const Matrix& A = problem.A();
        if (problem.general_bounds()) {
            // general column bounds, whatever the opt-ins say: the blocks of A = [[A_ub I], [A_eq 0]] with lda = cols, both
            // bound vectors as given; x_slack comes back in the caller's variables and ends with the bound slacks and the x^-
            const std::size_t m_ub = problem.n_slack(), m_eq = A.rows - m_ub;
            raise_for(lpipm_upload_bounds(ctx, A.cols - m_ub, m_ub, m_ub ? A.data.data() : nullptr, A.cols,
                                          m_ub ? problem.b().data() : nullptr, m_eq, m_eq ? A.data.data() + m_ub * A.cols : nullptr,
                                          A.cols, m_eq ? problem.b().data() + m_ub : nullptr, problem.c().data(), problem.c0(),
                                          problem.lower().data(), problem.upper().data()));
            x.assign(A.cols + problem.n_bounded() + problem.n_free(), 0.0);
            return lpipm_solve(ctx, &o_, x.data(), &fun, &it, nullptr);
        }
        if (problem.n_bounded() > 0) {
            // the bounded form, whatever the opt-ins say (on a tall form a bound is one more `ub` row): the blocks of
            // A = [[A_ub I], [A_eq 0]] with lda = cols, the bounds as given; x_slack ends with the nb bound slacks
            const std::size_t m_ub = problem.n_slack(), m_eq = A.rows - m_ub;
            raise_for(lpipm_upload_bounded(ctx, A.cols - m_ub, m_ub, m_ub ? A.data.data() : nullptr, A.cols,
                                           m_ub ? problem.b().data() : nullptr, m_eq, m_eq ? A.data.data() + m_ub * A.cols : nullptr,
                                           A.cols, m_eq ? problem.b().data() + m_ub : nullptr, problem.c().data(), problem.c0(),
                                           problem.upper().data()));
            x.assign(A.cols + problem.n_bounded(), 0.0);
            return lpipm_solve(ctx, &o_, x.data(), &fun, &it, nullptr);
        }
        if (tall_eq_ && problem.n_slack() > 0 && problem.n_slack() <= A.rows && problem.n_slack() < A.cols) {
            // A = [[X I], [A_eq 0]]: the `ub` block is the first n_slack rows, the `eq` block the rest, both with lda = cols
            const std::size_t m_ub = problem.n_slack(), m_eq = A.rows - m_ub;
            raise_for(lpipm_upload_ub_eq_tall(ctx, A.cols - m_ub, m_ub, A.data.data(), A.cols, problem.b().data(), m_eq,
                                              m_eq ? A.data.data() + m_ub * A.cols : nullptr, A.cols,
                                              m_eq ? problem.b().data() + m_ub : nullptr, problem.c().data(), problem.c0()));
        } else if (tall_ && problem.n_slack() == A.rows && problem.n_slack() < A.cols)
            // `ub` rows only: A = [X I], X = the first cols - n_slack columns (lda = cols); the slack costs are zero
            raise_for(lpipm_upload_ub_tall(ctx, A.cols - problem.n_slack(), A.rows, A.data.data(), A.cols, problem.b().data(),
                                           problem.c().data(), problem.c0()));
        else
        // n_slack tells the backend that the last columns are the [I; 0] slack block (linear_program.rs:147-161)
        raise_for(lpipm_upload_slack(ctx, A.rows, A.cols, A.data.data(), A.cols, problem.b().data(),
                                     problem.c().data(), problem.c0(), problem.n_slack()));
        x.assign(A.cols, 0.0);
        return lpipm_solve(ctx, &o_, x.data(), &fun, &it, nullptr);
    }
    lpipm_opts o_;
    int device_;
    bool tall_ = false, tall_eq_ = false;
};

inline InteriorPoint InteriorPointBuilder::build() const {
    if (!(o_.alpha0 > 0.0) || !(o_.alpha0 < 1.0))   // mod.rs:119-123
        throw LinearProgramError(ErrorKind::InvalidParameter,
                                 "A parameter was set to an invalid value: Alpha0 must be between 0 and 1 (exclusive)");
    if (!(o_.tol > 0.0))                            // mod.rs:124-128
        throw LinearProgramError(ErrorKind::InvalidParameter,
                                 "A parameter was set to an invalid value: The tolerance must be nonnegative.");
    return InteriorPoint(o_);
}

}  // namespace ripped
