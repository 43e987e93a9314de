// batch_plan.hpp -- how lpipm_solve_batch* divides a list of LPs into lockstep chunks and a rest that is solved one by one.
// Plain C++ on the caller's arrays: no device, no HIP call, so a host-only program can include and check it
// (tests/cpp/test_batch_plan.cpp).
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

namespace lpipm {

// Whether the last n_slack columns of every one of the `count` m x n matrices are [I; 0] (n_slack == n: not a hint).
inline bool slack_hint_holds(uint64_t count, uint64_t m, uint64_t n, const double* const* A, uint64_t lda, uint64_t n_slack) {
    if (n_slack == 0 || n_slack == n) return false;
    for (uint64_t k = 0; k < count; ++k)
        for (uint64_t i = 0; i < m; ++i) {
            const double* row = A[k] + i * lda + (n - n_slack);
            for (uint64_t j = 0; j < n_slack; ++j)
                if (row[j] != ((i == j) ? 1.0 : 0.0)) return false;
        }
    return true;
}

// The hint that holds, per member (0: none; n_slack null: none anywhere), verified once on the member's own matrix.  A hint
// larger than the member's n or m is that member's error, as it is lpipm_upload_slack's: refused[i] is set and the member takes
// no further part.  A member without rows, without a hint or without a matrix is left to its upload's answer.
inline std::vector<uint64_t> verify_hints(uint64_t count, const uint64_t* m, const uint64_t* n, const uint64_t* n_slack,
                                          const double* const* A, std::vector<char>& refused) {
    std::vector<uint64_t> ns(count, 0);
    for (uint64_t i = 0; i < count && n_slack; ++i) {
        if (m[i] == 0 || n_slack[i] == 0 || !A[i]) continue;
        if (n_slack[i] > n[i] || n_slack[i] > m[i]) refused[i] = 1;
        else if (slack_hint_holds(1, m[i], n[i], &A[i], n[i], n_slack[i])) ns[i] = n_slack[i];
    }
    return ns;
}

// The members not yet taken, grouped by (m, n, hint that holds): every group of two or more, ascending inside and ordered by
// first member; its members are marked taken.  A member alone in its group stays untaken.
inline std::vector<std::vector<uint64_t>> group_members(uint64_t count, const uint64_t* m, const uint64_t* n,
                                                        const std::vector<uint64_t>& ns, std::vector<char>& taken) {
    std::vector<std::vector<uint64_t>> groups;
    for (uint64_t i = 0; i < count; ++i) {
        if (taken[i]) continue;
        std::vector<uint64_t> grp;
        for (uint64_t j = i; j < count; ++j)
            if (!taken[j] && m[j] == m[i] && n[j] == n[i] && ns[j] == ns[i]) grp.push_back(j);
        if (grp.size() < 2) continue;
        for (uint64_t j : grp) taken[j] = 1;
        groups.push_back(std::move(grp));
    }
    return groups;
}

// Members per chunk of a group: the configured maximum (lpipm_set_batch_lockstep > 0), else 32 above 32 members, else two
// chunks from 16 members on (the second upload hides behind the first solve), else the whole group -- and never more than
// `fit`, the members whose arenas fit the memory budget.
inline size_t chunk_size(size_t group, int lockstep_max, size_t fit) {
    size_t chunk;
    if (lockstep_max > 0) chunk = (size_t)lockstep_max;
    else if (group > 32) chunk = 32;
    else if (group >= 16) chunk = (group + 1) / 2;
    else chunk = group;
    return chunk > fit ? fit : chunk;
}

// The chunks [k0, k0 + g) of a group cut `chunk` members at a time.  A last chunk of one member, and the whole group when
// `chunk` is below two, go to `rest`: the one-by-one path.
struct Span { size_t k0, g; };
inline std::vector<Span> split_chunks(const std::vector<uint64_t>& grp, size_t chunk, std::vector<uint64_t>& rest) {
    std::vector<Span> spans;
    if (chunk < 2) { rest.insert(rest.end(), grp.begin(), grp.end()); return spans; }
    for (size_t k0 = 0; k0 < grp.size(); k0 += chunk) {
        const size_t g = (k0 + chunk < grp.size() ? k0 + chunk : grp.size()) - k0;
        if (g < 2) rest.push_back(grp[k0]);
        else spans.push_back(Span{k0, g});
    }
    return spans;
}

}  // namespace lpipm
