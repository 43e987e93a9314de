// The host-only part of lpipm_upload_device (lp_amd/csrc/device_source.hpp): descriptor -> host entry, the refusals that need
// no device, the farthest-element computation with its overflow checks, and the choice of copy mode.  No device, no HIP.
#include <cstdio>
#include <cstdint>
#include <initializer_list>
#include "device_source.hpp"

using namespace lpipm;

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); ++failures; } } while (0)

static lpipm_device_problem good(uint32_t form, uint32_t shared, uint64_t count) {
    lpipm_device_problem d{};
    d.struct_size = (uint32_t)sizeof(d); d.form = form; d.src_type = LPIPM_SRC_F64; d.shared = shared; d.count = count;
    d.m = 5; d.n = 7; d.m_eq = form == LPIPM_FORM_UB_EQ ? 2 : 0;
    d.A = {nullptr, 7, 1, 35}; d.A_eq = {nullptr, 7, 1, 0}; d.b = {nullptr, 1, 7}; d.c = {nullptr, 1, 7};
    return d;
}
static HostEntry entry(uint32_t form, uint32_t shared, uint64_t count, int* rc) {
    const lpipm_device_problem d = good(form, shared, count);
    HostEntry e;
    *rc = entry_of(&d, &e);
    return e;
}

int main() {
    int rc = 0;
    // every (form, shared, count) and the entry it stands for
    CHECK(entry(LPIPM_FORM_SLACK, 0, 1, &rc) == HostEntry::Slack && rc == LPIPM_OK);
    CHECK(entry(LPIPM_FORM_SLACK, 0, 2, &rc) == HostEntry::LockstepSlack && rc == LPIPM_OK);
    CHECK(entry(LPIPM_FORM_SLACK, 0, 4096, &rc) == HostEntry::LockstepSlack && rc == LPIPM_OK);
    CHECK(entry(LPIPM_FORM_SLACK, 1, 1, &rc) == HostEntry::SharedSlack && rc == LPIPM_OK);
    CHECK(entry(LPIPM_FORM_SLACK, 1, 9, &rc) == HostEntry::SharedSlack && rc == LPIPM_OK);
    CHECK(entry(LPIPM_FORM_UB_EQ, 0, 1, &rc) == HostEntry::UbEq && rc == LPIPM_OK);
    CHECK(entry(LPIPM_FORM_UB_EQ, 1, 1, &rc) == HostEntry::SharedUbEq && rc == LPIPM_OK);
    CHECK(entry(LPIPM_FORM_UB_EQ, 1, 5, &rc) == HostEntry::SharedUbEq && rc == LPIPM_OK);
    CHECK(entry(LPIPM_FORM_UB_EQ, 0, 3, &rc) == HostEntry::None && rc == LPIPM_ERR_UNSUPPORTED);
    CHECK(entry(LPIPM_FORM_UB_TALL, 0, 1, &rc) == HostEntry::UbTall && rc == LPIPM_OK);
    CHECK(entry(LPIPM_FORM_UB_TALL, 0, 3, &rc) == HostEntry::LockstepUbTall && rc == LPIPM_OK);
    CHECK(entry(LPIPM_FORM_UB_TALL, 1, 1, &rc) == HostEntry::SharedUbTall && rc == LPIPM_OK);
    CHECK(entry(LPIPM_FORM_UB_TALL, 1, 3, &rc) == HostEntry::SharedUbTall && rc == LPIPM_OK);
    CHECK(entry_shared(HostEntry::SharedSlack) && entry_shared(HostEntry::SharedUbEq) && entry_shared(HostEntry::SharedUbTall));
    CHECK(!entry_shared(HostEntry::Slack) && !entry_shared(HostEntry::LockstepUbTall) && !entry_shared(HostEntry::UbEq));

    // what is refused without a look at the shape
    HostEntry e;
    CHECK(entry_of(nullptr, &e) == LPIPM_ERR_BAD_ARGUMENT && e == HostEntry::None);
    for (uint64_t count : {(uint64_t)0, (uint64_t)4097, ~(uint64_t)0})
        for (uint32_t form : {LPIPM_FORM_SLACK, LPIPM_FORM_UB_EQ, LPIPM_FORM_UB_TALL}) {
            (void)entry(form, 0, count, &rc);
            CHECK(rc == LPIPM_ERR_BAD_ARGUMENT);       // (UB_EQ with its own matrices included: the count comes first)
        }
    { lpipm_device_problem d = good(LPIPM_FORM_SLACK, 0, 1); d.struct_size -= 8; CHECK(entry_of(&d, &e) == LPIPM_ERR_BAD_ARGUMENT); }
    { lpipm_device_problem d = good(LPIPM_FORM_SLACK, 0, 1); d.struct_size += 8; CHECK(entry_of(&d, &e) == LPIPM_ERR_BAD_ARGUMENT); }
    { lpipm_device_problem d = good(LPIPM_FORM_SLACK, 0, 1); d.struct_size = 0; CHECK(entry_of(&d, &e) == LPIPM_ERR_BAD_ARGUMENT); }
    { lpipm_device_problem d = good(3, 0, 1); CHECK(entry_of(&d, &e) == LPIPM_ERR_BAD_ARGUMENT); }
    { lpipm_device_problem d = good(LPIPM_FORM_SLACK, 0, 1); d.src_type = 2; CHECK(entry_of(&d, &e) == LPIPM_ERR_BAD_ARGUMENT); }
    { lpipm_device_problem d = good(LPIPM_FORM_SLACK, 2, 1); CHECK(entry_of(&d, &e) == LPIPM_ERR_BAD_ARGUMENT); }

    // strides: every one that is read must be >= 1, the others may be anything
    { lpipm_device_problem d = good(LPIPM_FORM_SLACK, 0, 3); CHECK(strides_ok(&d)); }
    { lpipm_device_problem d = good(LPIPM_FORM_SLACK, 0, 3); d.A.row_stride = 0; CHECK(!strides_ok(&d)); }
    { lpipm_device_problem d = good(LPIPM_FORM_SLACK, 0, 3); d.A.col_stride = -1; CHECK(!strides_ok(&d)); }
    { lpipm_device_problem d = good(LPIPM_FORM_SLACK, 0, 3); d.A.member_stride = 0; CHECK(!strides_ok(&d)); }
    { lpipm_device_problem d = good(LPIPM_FORM_SLACK, 0, 1); d.A.member_stride = 0; d.b.member_stride = d.c.member_stride = -5; CHECK(strides_ok(&d)); }
    { lpipm_device_problem d = good(LPIPM_FORM_SLACK, 1, 3); d.A.member_stride = 0; CHECK(strides_ok(&d)); }
    { lpipm_device_problem d = good(LPIPM_FORM_SLACK, 1, 3); d.b.member_stride = 0; CHECK(!strides_ok(&d)); }
    { lpipm_device_problem d = good(LPIPM_FORM_SLACK, 1, 3); d.c.member_stride = 0; CHECK(!strides_ok(&d)); }
    { lpipm_device_problem d = good(LPIPM_FORM_SLACK, 0, 1); d.b.stride = 0; CHECK(!strides_ok(&d)); }
    { lpipm_device_problem d = good(LPIPM_FORM_SLACK, 0, 1); d.c.stride = 0; CHECK(!strides_ok(&d)); }
    { lpipm_device_problem d = good(LPIPM_FORM_SLACK, 0, 1); d.A_eq.row_stride = 0; CHECK(strides_ok(&d)); }       // A_eq is not read
    { lpipm_device_problem d = good(LPIPM_FORM_UB_EQ, 0, 1); d.A_eq.row_stride = 0; CHECK(!strides_ok(&d)); }
    { lpipm_device_problem d = good(LPIPM_FORM_UB_EQ, 0, 1); d.A_eq.col_stride = 0; CHECK(!strides_ok(&d)); }
    { lpipm_device_problem d = good(LPIPM_FORM_UB_EQ, 0, 1); d.m_eq = 0; d.A_eq.col_stride = 0; CHECK(strides_ok(&d)); }

    // the farthest element
    uint64_t span = 0, bytes = 0;
    { const Dim d[2] = {{5, 7}, {7, 1}}; CHECK(span_elements(d, 2, &span) && span == 35); }
    { const Dim d[2] = {{5, 10}, {7, 1}}; CHECK(span_elements(d, 2, &span) && span == 47); }                     // a pitch
    { const Dim d[2] = {{5, 1}, {7, 5}}; CHECK(span_elements(d, 2, &span) && span == 35); }                      // column-major
    { const Dim d[3] = {{3, 70}, {5, 14}, {3, 3}}; CHECK(span_elements(d, 3, &span) && span == 2 * 70 + 4 * 14 + 2 * 3 + 1); }
    { const Dim d[2] = {{0, 7}, {7, 1}}; CHECK(span_elements(d, 2, &span) && span == 0); }                       // nothing is read
    { const Dim d[1] = {{1, INT64_MAX}}; CHECK(span_elements(d, 1, &span) && span == 1); }                       // extent 1: the stride is not used
    { const Dim d[2] = {{(uint64_t)1 << 40, 8}, {8, 1}}; CHECK(span_bytes(d, 2, 8, &bytes) && bytes == ((((uint64_t)1 << 40) - 1) * 8 + 8) * 8); }
    // ... near 2^63: the product, the sum, the + 1 and the bytes each overflow on their own
    { const Dim d[1] = {{3, INT64_MAX / 2 + 1}}; CHECK(!span_elements(d, 1, &span)); }
    { const Dim d[1] = {{3, INT64_MAX / 2}}; CHECK(span_elements(d, 1, &span) && span == (uint64_t)INT64_MAX); }
    { const Dim d[2] = {{2, INT64_MAX - 1}, {3, 1}}; CHECK(!span_elements(d, 2, &span)); }
    { const Dim d[2] = {{2, INT64_MAX - 2}, {3, 1}}; CHECK(!span_elements(d, 2, &span)); }                       // far == 2^63 - 1: no room for the + 1
    { const Dim d[2] = {{2, INT64_MAX - 3}, {3, 1}}; CHECK(span_elements(d, 2, &span) && span == (uint64_t)INT64_MAX); }
    { const Dim d[1] = {{~(uint64_t)0, 2}}; CHECK(!span_elements(d, 1, &span)); }
    { const Dim d[1] = {{5, -1}}; CHECK(!span_elements(d, 1, &span)); }
    { const Dim d[1] = {{((uint64_t)1 << 60) + 1, 1}}; CHECK(span_bytes(d, 1, 4, &bytes) && !span_bytes(d, 1, 8, &bytes) && bytes == 0); }
    CHECK(inside(1000, 100, 1000, 100) && inside(1040, 60, 1000, 100) && !inside(1040, 61, 1000, 100));
    CHECK(!inside(999, 1, 1000, 100) && !inside(1101, 0, 1000, 100) && inside(1100, 0, 1000, 100));
    CHECK(!inside(1000, ~(uint64_t)0, 1000, 100));

    // the copy mode: the three layouts, and the row-major one when a base or a pitch is not a multiple of two elements
    CHECK(pack_mode(4096, 8, 128, 1, 0, false) == PackMode::RowWide);
    CHECK(pack_mode(4096 + 8, 8, 128, 1, 0, false) == PackMode::Row);                // an odd element offset
    CHECK(pack_mode(4096, 8, 129, 1, 0, false) == PackMode::Row);                    // an odd pitch
    CHECK(pack_mode(4096, 8, 128, 1, 1025, true) == PackMode::Row);                  // an odd member stride
    CHECK(pack_mode(4096, 8, 128, 1, 1025, false) == PackMode::RowWide);             // ... that is not read
    CHECK(pack_mode(4096 + 8, 4, 128, 1, 0, false) == PackMode::RowWide);            // float: 8 bytes are two elements
    CHECK(pack_mode(4096 + 4, 4, 128, 1, 0, false) == PackMode::Row);
    CHECK(pack_mode(4096, 8, 1, 200, 0, false) == PackMode::Col);
    CHECK(pack_mode(4096 + 8, 4, 1, 200, 0, false) == PackMode::Col);
    CHECK(pack_mode(4096, 8, 1, 1, 0, false) == PackMode::Row);                      // both unit (a single row): the row walk
    CHECK(pack_mode(4096, 8, 400, 3, 0, false) == PackMode::Gather);
    CHECK(pack_mode(4096, 8, 2, 2, 0, false) == PackMode::Gather);

    if (failures) { std::printf("%d check(s) failed\n", failures); return 1; }
    std::printf("device_source: ok\n");
    return 0;
}
