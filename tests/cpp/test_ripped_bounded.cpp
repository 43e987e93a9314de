// test_ripped_bounded.cpp -- ProblemBuilder::upper of include/ripped.hpp, through liblpipm.so on device 0: an LP that only its
// bounds keep bounded (min -x1 - x2, x1 - x2 <= 1, u = (3, 2)) comes back with x = (3, 2) through lpipm_upload_bounded; the same
// bounds written as `ub` rows give the same answer and iteration count; the duals carry one entry per `ub` row and column; the
// README LP with bounds that are not active keeps its answer; an LP infeasible by its bounds throws with a Farkas certificate.
#include <cmath>
#include <cstdio>
#include <limits>
#include <vector>

#include "ripped.hpp"

using namespace ripped;

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); ++failures; } } while (0)

static bool close(const std::vector<double>& a, const std::vector<double>& b, double eps) {
    if (a.size() != b.size()) return false;
    for (size_t i = 0; i < a.size(); ++i)
        if (!(std::fabs(a[i] - b[i]) <= eps)) return false;
    return true;
}

int main() {
    const double inf = std::numeric_limits<double>::infinity();
    const Matrix A_ub{{1, -1}, 1, 2}, A_rows{{1, -1, 1, 0, 0, 1}, 3, 2};
    const std::vector<double> b_ub{1}, b_rows{1, 3, 2}, c{-1, -1}, u{3, 2};
    const Problem boxed = Problem::target(c).ub(A_ub, b_ub).upper(u).build();
    const Problem rows = Problem::target(c).ub(A_rows, b_rows).build();
    CHECK(boxed.n_bounded() == 2 && rows.n_bounded() == 0 && boxed.A().rows == 1 && boxed.A().cols == 3);
    try {
        const OptimizeResult got = InteriorPoint::default_().solve(boxed);
        const OptimizeResult want = InteriorPoint::default_().solve(rows);
        CHECK(close(got.x(), {3.0, 2.0}, 1e-6) && std::fabs(got.fun() + 5.0) <= 1e-6);
        CHECK(close(got.x(), want.x(), 1e-6) && got.iteration() == want.iteration());
        const InteriorPoint::DualResult d = InteriorPoint::default_().solve_with_duals(boxed);
        CHECK(d.y_ub.size() == 1 && d.y_eq.empty() && d.reduced_costs.size() == 2);
        CHECK(std::fabs(d.dual_fun - d.result.fun()) <= 1e-6);
        // the README LP (src/lib.rs:84-96) with one inactive bound and one column without: the known answer
        const Matrix R_ub{{-3, 1, 1, 2}, 2, 2}, R_eq{{1, 1}, 1, 2};
        const std::vector<double> rb_ub{6, 4}, rb_eq{1}, rc{-1, 4}, ru{5, inf};
        const OptimizeResult readme = InteriorPoint::default_().solve(Problem::target(rc).ub(R_ub, rb_ub).eq(R_eq, rb_eq).upper(ru).build());
        CHECK(close(readme.x(), {1.0, 0.0}, 1e-6));
    } catch (const LinearProgramError& e) {
        std::printf("FAIL: %s\n", e.what());
        ++failures;
    }
    // x1 + x2 + x3 = 10 with u = 1: infeasible by its bounds
    const Matrix S_eq{{1, 1, 1}, 1, 3};
    const std::vector<double> sb{10}, sc{1, 1, 1}, su{1, 1, 1};
    bool thrown = false;
    try {
        (void)InteriorPoint::default_().solve_with_certificate(Problem::target(sc).eq(S_eq, sb).upper(su).build());
    } catch (const CertifiedError& e) {
        thrown = e.kind() == ErrorKind::Infeasible && e.certificate().kind == LPIPM_CERT_FARKAS && e.certificate().y_eq.size() == 1 &&
                 e.certificate().z.size() == 3 && e.certificate().residual <= 1e-6;
    } catch (const LinearProgramError& e) {
        std::printf("FAIL: %s\n", e.what());
    }
    CHECK(thrown);
    std::printf(failures ? "%d failure(s)\n" : "ok\n", failures);
    return failures ? 1 : 0;
}
