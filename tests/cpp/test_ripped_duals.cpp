// test_ripped_duals.cpp -- InteriorPoint::solve_with_duals() of include/ripped.hpp, through liblpipm.so on device 0: the README
// LP (two `ub` rows, one `eq` row; src/lib.rs:84-96, known answer [1, 0]) in the slack form and in the tall-eq form.  The duals
// must be the known ones, close the dual residual of the caller's own arrays, have z >= 0, `ub` multipliers <= 0 and dual_fun at
// fun; and they must meet identity 1 of the getter's contract against the solve's own log (check_identity).
#include <cmath>
#include <cstdio>
#include <vector>

#include "ripped.hpp"

using namespace ripped;

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); ++failures; } } while (0)

// |c - A_ub^T y_ub - A_eq^T y_eq - z|_2 over the structural columns, and |0 - y_ub[i] - z_slack[i]| over the slack ones: the
// slack form's A^T y + z = c, with the slack columns' reduced costs taken as -y_ub (what the identity then leaves is 0 there)
static double dual_residual(const Matrix& A_ub, const Matrix& A_eq, const std::vector<double>& c,
                            const InteriorPoint::DualResult& d) {
    double s = 0.0;
    for (uint64_t j = 0; j < c.size(); ++j) {
        double r = c[j] - d.reduced_costs[j];
        for (uint64_t i = 0; i < A_ub.rows; ++i) r -= A_ub.data[i * A_ub.cols + j] * d.y_ub[i];
        for (uint64_t i = 0; i < A_eq.rows; ++i) r -= A_eq.data[i * A_eq.cols + j] * d.y_eq[i];
        s += r * r;
    }
    return std::sqrt(s);
}

static void check(const char* what, const Matrix& A_ub, const Matrix& A_eq, const std::vector<double>& c,
                  const InteriorPoint::DualResult& d, const OptimizeResult& plain) {
    const double res = dual_residual(A_ub, A_eq, c, d);
    std::printf("%s: x = [%.9f, %.9f], fun %.9f, dual_fun %.9f, |c - A^T y - z| %.3g, y_ub [%.6f, %.6f], y_eq [%.6f]\n", what,
                d.result.x()[0], d.result.x()[1], d.result.fun(), d.dual_fun, res, d.y_ub[0], d.y_ub[1], d.y_eq[0]);
    CHECK(d.y_ub.size() == 2 && d.y_eq.size() == 1 && d.reduced_costs.size() == 2);
    CHECK(std::fabs(d.result.x()[0] - 1.0) <= 1e-6 && std::fabs(d.result.x()[1]) <= 1e-6);
    CHECK(std::fabs(d.result.fun() - plain.fun()) <= 1e-6 && d.result.iteration() == plain.iteration());
    CHECK(res <= 1e-6);
    CHECK(std::fabs(d.dual_fun - d.result.fun()) <= 1e-6);
    for (double v : d.reduced_costs) CHECK(v > 0.0);
    for (double v : d.y_ub) CHECK(v <= 1e-6);               // minus the slack's (positive) reduced cost, up to the dual residual
    // the known answer: x = [1, 0] is optimal with the `eq` row's multiplier -1 (c_1 = -1 = y_eq, x_1 basic) and no active `ub` row
    CHECK(std::fabs(d.y_eq[0] + 1.0) <= 1e-6 && std::fabs(d.y_ub[0]) <= 1e-6 && std::fabs(d.y_ub[1]) <= 1e-6);
    CHECK(std::fabs(d.reduced_costs[0]) <= 1e-6 && std::fabs(d.reduced_costs[1] - 5.0) <= 1e-6);
}

// Identity 1 of the duals' contract, on the slack form the Problem holds: |c - A^T y - z|_2 = rho_d max(1, |c - 1|_2) / tau, with
// rho_d the last row of the solve's log and tau the getter's.  The same upload, solve and getter as solve_with_duals makes,
// through the C ABI (which has the log): the duals must be solve_with_duals's, bit for bit.  Allowance: the standard summation
// bound, 2 gamma_k sum|terms| per side with k = number of terms + 2.
static void check_identity(const char* what, const Problem& p, bool tall_eq, const InteriorPoint::DualResult& d) {
    const Matrix& A = p.A();
    const uint64_t m = A.rows, n = A.cols, ns = p.n_slack();
    lpipm_ctx* ctx = nullptr;
    CHECK(lpipm_create(0, &ctx) == LPIPM_OK);
    if (!ctx) return;
    const int up = tall_eq ? lpipm_upload_ub_eq_tall(ctx, n - ns, ns, A.data.data(), n, p.b().data(), m - ns, A.data.data() + ns * n, n,
                                                     p.b().data() + ns, p.c().data(), p.c0())
                           : lpipm_upload_slack(ctx, m, n, A.data.data(), n, p.b().data(), p.c().data(), p.c0(), ns);
    CHECK(up == LPIPM_OK);
    lpipm_opts o;
    lpipm_default_opts(&o);
    std::vector<double> x(n), y(m), z(n);
    std::vector<lpipm_iter_row> log(o.max_iter);
    double fun = 0.0;
    uint64_t it = 0;
    lpipm_dual_info info{};
    CHECK(lpipm_get_duals(ctx, 0, y.data(), z.data(), &info) == LPIPM_ERR_NO_PROBLEM);       // no solve yet
    CHECK(lpipm_solve(ctx, &o, x.data(), &fun, &it, log.data()) == LPIPM_OK);
    CHECK(lpipm_get_duals(ctx, 0, y.data(), z.data(), &info) == LPIPM_OK);
    lpipm_destroy(ctx);
    CHECK(it >= 1 && info.status == LPIPM_OK && info.tau > 0.0 && info.dual_fun == d.dual_fun);
    for (uint64_t i = 0; i < m; ++i) CHECK(y[i] == (i < ns ? d.y_ub[i] : d.y_eq[i - ns]));
    for (uint64_t j = 0; j < n - ns; ++j) CHECK(z[j] == d.reduced_costs[j]);
    double lhs = 0.0, mag = 0.0, cn = 0.0;
    for (uint64_t j = 0; j < n; ++j) {
        double r = p.c()[j] - z[j], a = std::fabs(p.c()[j]) + std::fabs(z[j]);
        for (uint64_t i = 0; i < m; ++i) { r -= A.data[i * n + j] * y[i]; a += std::fabs(A.data[i * n + j] * y[i]); }
        lhs += r * r; mag += a * a; cn += (p.c()[j] - 1.0) * (p.c()[j] - 1.0);
        CHECK(z[j] > 0.0);
    }
    lhs = std::sqrt(lhs); mag = std::sqrt(mag); cn = std::fmax(1.0, std::sqrt(cn));
    const double rhs = log[it - 1].rho_d * cn / info.tau;
    const double k = double(m + 2 + n + 2), eps = std::ldexp(1.0, -53), tol = 4.0 * (k * eps / (1.0 - k * eps)) * mag;
    std::printf("%s: identity 1: lhs %.6g, rhs %.6g, |lhs - rhs| %.3g, allowance %.3g\n", what, lhs, rhs, std::fabs(lhs - rhs), tol);
    CHECK(std::fabs(lhs - rhs) <= tol);
}

int main() {
    const Matrix A_ub{{-3, 1, 1, 2}, 2, 2}, A_eq{{1, 1}, 1, 2};
    const std::vector<double> b_ub{6, 4}, b_eq{1}, c{-1, 4};
    const Problem with_eq = Problem::target(c).ub(A_ub, b_ub).eq(A_eq, b_eq).build();
    try {
        const OptimizeResult plain = InteriorPoint::default_().solve(with_eq);
        check("slack form", A_ub, A_eq, c, InteriorPoint::default_().solve_with_duals(with_eq), plain);
        check("tall-eq form", A_ub, A_eq, c, InteriorPoint::default_().tall_eq_form().solve_with_duals(with_eq), plain);
        check_identity("slack form", with_eq, false, InteriorPoint::default_().solve_with_duals(with_eq));
        check_identity("tall-eq form", with_eq, true, InteriorPoint::default_().tall_eq_form().solve_with_duals(with_eq));
        // the same solve: solve_with_duals changes no bit of x or fun
        const InteriorPoint::DualResult d = InteriorPoint::default_().solve_with_duals(with_eq);
        CHECK(d.result.x() == plain.x() && d.result.fun() == plain.fun());
    } catch (const LinearProgramError& e) {
        std::printf("FAIL: %s\n", e.what());
        ++failures;
    }
    std::printf(failures ? "%d failure(s)\n" : "ok\n", failures);
    return failures ? 1 : 0;
}
