// Where the slots of a row live in the two column-major formats: slot i of `row` is element
// first + i * step of the column / value arrays, for i < len.  One struct per format, passed to the
// product kernels of formats.hip and complex_formats.hip by value; the kernels are templated on it.
#pragma once
#include "common.hpp"

namespace gkoc {

// ELL: k slots per row, column i of all rows is one run of `stride` elements
struct ell_rows {
    int64_t k;
    int64_t stride;
    __device__ __forceinline__ void locate(int64_t row, int64_t& len, int64_t& first, int64_t& step) const
    {
        len = k;
        first = row;
        step = stride;
    }
};

// SELL-P: slices of slice_size rows; slice g holds lengths[g] columns, the first of them at column
// sets[g] of the slice-column-major arrays.  `row` must be a row of the matrix (its slice exists).
struct sellp_rows {
    int64_t slice_size;
    const uint64_t* __restrict__ sets;
    const uint64_t* __restrict__ lengths;
    __device__ __forceinline__ void locate(int64_t row, int64_t& len, int64_t& first, int64_t& step) const
    {
        const int64_t slice = row / slice_size;
        len = int64_t(lengths[slice]);
        first = int64_t(sets[slice]) * slice_size + (row - slice * slice_size);
        step = slice_size;
    }
};

}  // namespace gkoc
