// The host-only steps of lpipm_solve_batch* (lp_amd/csrc/batch_plan.hpp) against their rules: hints, groups, chunk sizes, chunks.
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "batch_plan.hpp"

using namespace lpipm;

#define CHECK(cond) do { if (!(cond)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); std::exit(1); } } while (0)

// The chunk rule as lpipm_set_batch_lockstep documents it, written out on its own.
static size_t expected_chunk(size_t group, int max_group, size_t fit) {
    size_t want = max_group > 0 ? (size_t)max_group : group > 32 ? 32 : group >= 16 ? (group + 1) / 2 : group;
    return want < fit ? want : fit;
}

static void check_chunks() {
    const size_t sizes[] = {0, 1, 2, 5, 15, 16, 17, 32, 33, 65};
    const int maxima[] = {-1, 0, 2, 3, 4096};
    const size_t fits[] = {0, 1, 2, 3, 8, 1000};
    for (size_t size : sizes) for (int max_group : maxima) for (size_t fit : fits) {
        std::vector<uint64_t> grp(size), rest{777};                       // member ids 100, 103, ...: not their positions
        for (size_t k = 0; k < size; ++k) grp[k] = 100 + 3 * k;
        const size_t chunk = chunk_size(size, max_group, fit);
        CHECK(chunk == expected_chunk(size, max_group, fit));
        CHECK(chunk <= fit);
        const std::vector<Span> spans = split_chunks(grp, chunk, rest);
        CHECK(rest[0] == 777);                                            // what was there stays
        std::vector<int> seen(size, 0);                                   // every member in exactly one chunk or in rest
        for (const Span& s : spans) {
            CHECK(s.g >= 2 && s.g <= chunk && s.k0 + s.g <= size);
            for (size_t k = s.k0; k < s.k0 + s.g; ++k) ++seen[k];
        }
        for (size_t r = 1; r < rest.size(); ++r) {
            CHECK(rest[r] >= 100 && (rest[r] - 100) % 3 == 0 && (rest[r] - 100) / 3 < size);
            ++seen[(rest[r] - 100) / 3];
        }
        for (size_t k = 0; k < size; ++k) CHECK(seen[k] == 1);
        if (chunk < 2) CHECK(spans.empty() && rest.size() == 1 + size);   // nothing fits (or a maximum below two): all one by one
        else {
            CHECK(spans.size() == size / chunk + (size % chunk >= 2 ? 1 : 0));
            CHECK(rest.size() == 1 + (size % chunk == 1 ? 1 : 0));        // a last chunk of one member is no chunk
            for (size_t q = 0; q < spans.size(); ++q) CHECK(spans[q].k0 == q * chunk);
        }
    }
}

static void check_hints_and_groups() {
    // six members: 0, 2, 5 are 3 x 5 with [I; 0] in their last two columns; 1 is 3 x 5 without; 3 is 2 x 4; 4 has no rows
    const uint64_t m[] = {3, 3, 3, 2, 0, 3}, n[] = {5, 5, 5, 4, 5, 5};
    std::vector<std::vector<double>> mats;
    for (int i = 0; i < 6; ++i) {
        std::vector<double> a(m[i] * n[i], 0.25);
        if (i == 0 || i == 2 || i == 5)
            for (uint64_t r = 0; r < 3; ++r) for (uint64_t j = 0; j < 2; ++j) a[r * 5 + 3 + j] = r == j ? 1.0 : 0.0;
        mats.push_back(a);
    }
    const double* A[6];
    for (int i = 0; i < 6; ++i) A[i] = mats[i].data();
    {   // no hints at all: every 3 x 5 member in one group
        std::vector<char> taken(6, 0);
        const std::vector<uint64_t> ns = verify_hints(6, m, n, nullptr, A, taken);
        for (int i = 0; i < 6; ++i) CHECK(ns[i] == 0 && !taken[i]);
        const auto groups = group_members(6, m, n, ns, taken);
        CHECK(groups.size() == 1 && groups[0] == (std::vector<uint64_t>{0, 1, 2, 5}));
        CHECK(taken[0] && taken[1] && taken[2] && !taken[3] && !taken[4] && taken[5]);
    }
    {   // hints: 2 holds on 0 and 2, not on 1; 3 > m on member 3 (refused); a hint on the member without rows is not looked at;
        // 6 > n on member 5 (refused)
        const uint64_t hint[] = {2, 2, 2, 3, 9, 6};
        std::vector<char> taken(6, 0);
        const std::vector<uint64_t> ns = verify_hints(6, m, n, hint, A, taken);
        CHECK(ns == (std::vector<uint64_t>{2, 0, 2, 0, 0, 0}));
        CHECK(!taken[0] && !taken[1] && !taken[2] && taken[3] && !taken[4] && taken[5]);
        const auto groups = group_members(6, m, n, ns, taken);
        CHECK(groups.size() == 1 && groups[0] == (std::vector<uint64_t>{0, 2}));      // 1 is alone with its hint of 0
        CHECK(!taken[1] && !taken[4]);
    }
    {   // a null matrix is left to its upload; n_slack == n is no hint; count == 0
        const uint64_t hint[] = {2, 0, 0, 0, 0, 2};
        const double* B[6] = {nullptr, A[1], A[2], A[3], A[4], A[5]};
        std::vector<char> taken(6, 0);
        const std::vector<uint64_t> ns = verify_hints(6, m, n, hint, B, taken);
        CHECK(ns == (std::vector<uint64_t>{0, 0, 0, 0, 0, 2}));
        for (int i = 0; i < 6; ++i) CHECK(!taken[i]);
        const double eye[] = {1, 1, 0, 0, 0, 0};                          // 3 x 2: its last column is [1; 0; 0]; n_slack == n is no hint, whatever the matrix
        const double* E[1] = {eye};
        CHECK(!slack_hint_holds(1, 3, 2, E, 2, 2) && slack_hint_holds(1, 3, 2, E, 2, 1) && !slack_hint_holds(1, 3, 2, E, 2, 0));
        std::vector<char> none;
        CHECK(verify_hints(0, nullptr, nullptr, nullptr, nullptr, none).empty());
        CHECK(group_members(0, nullptr, nullptr, {}, none).empty());
    }
    {   // two shapes interleaved: groups in order of their first member, ascending inside
        const uint64_t m2[] = {4, 7, 4, 7, 4}, n2[] = {9, 9, 9, 9, 8};
        std::vector<char> taken(5, 0);
        const auto groups = group_members(5, m2, n2, std::vector<uint64_t>(5, 0), taken);
        CHECK(groups.size() == 2 && groups[0] == (std::vector<uint64_t>{0, 2}) && groups[1] == (std::vector<uint64_t>{1, 3}));
        CHECK(!taken[4]);
    }
}

int main() {
    check_chunks();
    check_hints_and_groups();
    std::printf("batch plan ok\n");
    return 0;
}
