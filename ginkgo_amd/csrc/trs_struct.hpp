// The level schedule of a triangular solve (trs.hip builds and owns it; factorization.hip walks the
// lower one: row i of an ILU(0) / IC(0) factor depends on exactly the rows the lower solve depends on).
#pragma once
#include <cstdint>
#include <vector>

struct gkoc_trs_struct_s {
    int64_t n_rows;
    int64_t nnz;             // row_ptrs[n_rows] at generate
    int is_upper;
    int64_t n_levels;
    int64_t* level_ptrs;     // device, n_levels + 1
    int64_t* level_rows;     // device, n_rows
    struct segment {
        int64_t first, last; // levels [first, last)
        int64_t offset;      // level_ptrs[first]
        int64_t rows;        // wide: rows of the level; narrow: the largest level of the run
        bool wide;
    };
    std::vector<segment> schedule;
};
