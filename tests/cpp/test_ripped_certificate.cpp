// test_ripped_certificate.cpp -- InteriorPoint::solve_with_certificate() of include/ripped.hpp, through liblpipm.so on device 0,
// in the slack form and in the tall-eq form: an infeasible LP (x0 + x1 <= -1 over x >= 0) must throw Infeasible with a Farkas
// ray that closes A^T y + z = 0 on the caller's own arrays with b.y = 1, z >= 0 and `ub` multipliers <= 0; an unbounded one
// (min -x0 with x0 in no binding row) must throw Unbounded with a ray x >= 0, A_ub x <= 0, A_eq x = 0, c.x = -1; the README LP
// must come back as solve() returns it.
#include <cmath>
#include <cstdio>
#include <vector>

#include "ripped.hpp"

using namespace ripped;

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); ++failures; } } while (0)

static double dot_col(const Matrix& A, const std::vector<double>& y, uint64_t j) {
    double s = 0.0;
    for (uint64_t i = 0; i < A.rows; ++i) s += A.data[i * A.cols + j] * y[i];
    return s;
}
static double dot_row(const Matrix& A, const std::vector<double>& x, uint64_t i) {
    double s = 0.0;
    for (uint64_t j = 0; j < A.cols; ++j) s += A.data[i * A.cols + j] * x[j];
    return s;
}

static void run(const char* what, const InteriorPoint& solver) {
    const Matrix A_eq{{1, -1, 0}, 1, 3};
    const std::vector<double> b_eq{0.5};
    {   // infeasible: row 0 asks for x0 + x1 + x2 <= -1
        const Matrix A_ub{{1, 1, 1, -1, 2, 1}, 2, 3};
        const std::vector<double> b_ub{-1, 4}, c{1, 2, 3};
        const Problem p = Problem::target(c).ub(A_ub, b_ub).eq(A_eq, b_eq).build();
        bool thrown = false;
        try {
            solver.solve_with_certificate(p);
        } catch (const CertifiedError& e) {
            thrown = true;
            const Certificate& k = e.certificate();
            CHECK(e.kind() == ErrorKind::Infeasible && k.kind == LPIPM_CERT_FARKAS);
            CHECK(k.y_ub.size() == 2 && k.y_eq.size() == 1 && k.z.size() == 3 && k.x.empty());
            double by = b_eq[0] * k.y_eq[0], worst = 0.0;
            for (uint64_t i = 0; i < 2; ++i) { by += b_ub[i] * k.y_ub[i]; CHECK(k.y_ub[i] <= 1e-6); }
            for (uint64_t j = 0; j < 3; ++j) {
                CHECK(k.z[j] >= 0.0);
                worst = std::fmax(worst, std::fabs(dot_col(A_ub, k.y_ub, j) + dot_col(A_eq, k.y_eq, j) + k.z[j]));
            }
            std::printf("%s, infeasible: b.y %.12f, |A^T y + z| %.3g, residual %.3g, scale %.6g\n", what, by, worst, k.residual, k.scale);
            CHECK(std::fabs(by - 1.0) <= 1e-6 && worst <= 1e-6 && k.residual <= 1e-6 && k.scale > 0.0);
        }
        CHECK(thrown);
        try { solver.solve(p); CHECK(false); } catch (const LinearProgramError& e) { CHECK(e.kind() == ErrorKind::Infeasible); }
    }
    {   // unbounded: x2 is in no `eq` row, loosens both `ub` rows and pays -1
        const Matrix A_ub{{1, 1, -1, -1, 2, -2}, 2, 3};
        const std::vector<double> b_ub{3, 4}, c{1, 2, -1};
        const Problem p = Problem::target(c).ub(A_ub, b_ub).eq(A_eq, b_eq).build();
        bool thrown = false;
        try {
            solver.solve_with_certificate(p);
        } catch (const CertifiedError& e) {
            thrown = true;
            const Certificate& k = e.certificate();
            CHECK(e.kind() == ErrorKind::Unbounded && k.kind == LPIPM_CERT_RAY);
            CHECK(k.x.size() == 3 && k.y_ub.empty() && k.y_eq.empty() && k.z.empty());
            double cx = 0.0;
            for (uint64_t j = 0; j < 3; ++j) { cx += c[j] * k.x[j]; CHECK(k.x[j] >= 0.0); }
            for (uint64_t i = 0; i < 2; ++i) CHECK(dot_row(A_ub, k.x, i) <= 1e-6);
            std::printf("%s, unbounded: c.x %.12f, A_eq x %.3g, residual %.3g, scale %.6g\n", what, cx, dot_row(A_eq, k.x, 0), k.residual, k.scale);
            CHECK(std::fabs(cx + 1.0) <= 1e-6 && std::fabs(dot_row(A_eq, k.x, 0)) <= 1e-6 && k.residual <= 1e-6 && k.scale > 0.0);
        }
        CHECK(thrown);
    }
    {   // the README LP: what solve() returns, bit for bit
        const Matrix A_ub{{-3, 1, 1, 2}, 2, 2}, A1{{1, 1}, 1, 2};
        const Problem p = Problem::target({-1, 4}).ub(A_ub, {6, 4}).eq(A1, {1}).build();
        const OptimizeResult a = solver.solve(p), b = solver.solve_with_certificate(p);
        CHECK(a.x() == b.x() && a.fun() == b.fun() && a.iteration() == b.iteration());
    }
}

int main() {
    try {
        run("slack form", InteriorPoint::default_());
        run("tall-eq form", InteriorPoint::default_().tall_eq_form());
    } catch (const LinearProgramError& e) {
        std::printf("FAIL: %s\n", e.what());
        ++failures;
    }
    std::printf(failures ? "%d failure(s)\n" : "ok\n", failures);
    return failures ? 1 : 0;
}
