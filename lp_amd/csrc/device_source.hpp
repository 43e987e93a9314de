// device_source.hpp -- the host-only part of lpipm_upload_device: what a descriptor asks for, whether it may be asked, how far
// its strides reach and which copy kernel serves its layout.  Plain C++ on the descriptor's numbers: no device, no HIP call and
// no pointer is dereferenced, so a host-only program can include and check it (tests/cpp/test_device_source.cpp).
#pragma once
#include <cstddef>
#include <cstdint>
#include "../../include/lpipm.h"

namespace lpipm {

// The host entry a descriptor stands for (lpipm.h, the table at lpipm_upload_device).
enum class HostEntry { None, Slack, LockstepSlack, SharedSlack, UbEq, SharedUbEq, UbTall, LockstepUbTall, SharedUbTall };

inline size_t src_elem_bytes(uint32_t src_type) { return src_type == LPIPM_SRC_F32 ? sizeof(float) : sizeof(double); }

// What can be said of a descriptor without looking at the shape or the pointers: its size word, form, element type and
// member count, and the entry (form, shared, count) selects.  UB_EQ members with their own matrices have no host entry.
inline int entry_of(const lpipm_device_problem* d, HostEntry* out) {
    *out = HostEntry::None;
    if (!d || d->struct_size != sizeof(lpipm_device_problem)) return LPIPM_ERR_BAD_ARGUMENT;
    if (d->form > LPIPM_FORM_UB_TALL || d->src_type > LPIPM_SRC_F32 || d->shared > 1) return LPIPM_ERR_BAD_ARGUMENT;
    if (d->count < 1 || d->count > 4096) return LPIPM_ERR_BAD_ARGUMENT;
    const bool one = d->count == 1;
    switch (d->form) {
    case LPIPM_FORM_SLACK:   *out = d->shared ? HostEntry::SharedSlack : one ? HostEntry::Slack : HostEntry::LockstepSlack; break;
    case LPIPM_FORM_UB_EQ:   if (!d->shared && !one) return LPIPM_ERR_UNSUPPORTED;
                             *out = d->shared ? HostEntry::SharedUbEq : HostEntry::UbEq; break;
    default:                 *out = d->shared ? HostEntry::SharedUbTall : one ? HostEntry::UbTall : HostEntry::LockstepUbTall; break;
    }
    return LPIPM_OK;
}
inline bool entry_shared(HostEntry e) { return e == HostEntry::SharedSlack || e == HostEntry::SharedUbEq || e == HostEntry::SharedUbTall; }

// Whether the matrix has one image per member (else one for the call), and whether a member stride is read at all.
inline bool member_strided(const lpipm_device_problem* d) { return !d->shared && d->count > 1; }

// Every stride that will be used is >= 1.  A_eq counts only where it is read (UB_EQ with m_eq rows); a matrix's member stride
// only for members that own their matrices, a vector's for more than one member.
inline bool strides_ok(const lpipm_device_problem* d) {
    const bool eq = d->form == LPIPM_FORM_UB_EQ && d->m_eq > 0;
    if (d->A.row_stride < 1 || d->A.col_stride < 1 || (member_strided(d) && d->A.member_stride < 1)) return false;
    if (eq && (d->A_eq.row_stride < 1 || d->A_eq.col_stride < 1)) return false;
    if (d->b.stride < 1 || d->c.stride < 1) return false;
    if (d->count > 1 && (d->b.member_stride < 1 || d->c.member_stride < 1)) return false;
    return true;
}

// One past the farthest element the extents and strides address, in elements from the base pointer: the sum over the
// dimensions of (extent - 1) * stride, plus one.  Dimensions of extent 0 make the whole thing empty (*span_out = 0).
// False when the sum does not fit 63 bits (strides are positive here: nothing is subtracted).
struct Dim { uint64_t extent; int64_t stride; };
inline bool span_elements(const Dim* dims, int ndims, uint64_t* span_out) {
    *span_out = 0;
    for (int k = 0; k < ndims; ++k) if (dims[k].extent == 0) return true;
    const uint64_t lim = (uint64_t)INT64_MAX;
    uint64_t far = 0;
    for (int k = 0; k < ndims; ++k) {
        if (dims[k].stride < 0) return false;
        const uint64_t e = dims[k].extent - 1, s = (uint64_t)dims[k].stride;
        if (e != 0 && s > lim / e) return false;
        const uint64_t term = e * s;
        if (term > lim - far) return false;
        far += term;
    }
    if (far == lim) return false;
    *span_out = far + 1;
    return true;
}
// The same in bytes from the base pointer; false on overflow.
inline bool span_bytes(const Dim* dims, int ndims, size_t elem, uint64_t* bytes_out) {
    uint64_t span = 0;
    *bytes_out = 0;
    if (!span_elements(dims, ndims, &span)) return false;
    if (span > (uint64_t)INT64_MAX / elem) return false;
    *bytes_out = span * elem;
    return true;
}
// Whether [ptr, ptr + bytes) lies inside the allocation [base, base + size).
inline bool inside(uintptr_t ptr, uint64_t bytes, uintptr_t base, uint64_t size) {
    if (ptr < base) return false;
    const uint64_t off = (uint64_t)(ptr - base);
    return off <= size && bytes <= size - off;
}

// How k_pack_matrix reads a source (kernels_pack.hip).  RowWide: unit column stride, two elements per lane and load -- the
// base and every row and member pitch are multiples of two elements (16 bytes for double).  Row: unit column stride, one
// element per lane and load.  Col: unit row stride (a column-major source), through an LDS tile.  Gather: anything else.
enum class PackMode { RowWide, Row, Col, Gather };
inline PackMode pack_mode(uintptr_t ptr, size_t elem, int64_t row_stride, int64_t col_stride, int64_t member_stride, bool members) {
    if (col_stride == 1) {
        const bool wide = ptr % (2 * elem) == 0 && row_stride % 2 == 0 && (!members || member_stride % 2 == 0);
        return wide ? PackMode::RowWide : PackMode::Row;
    }
    return row_stride == 1 ? PackMode::Col : PackMode::Gather;
}

}  // namespace lpipm
