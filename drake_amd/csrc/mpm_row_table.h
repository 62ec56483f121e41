// Vertex row tables: the one data structure behind bending (k_bend, k_bend_eval), hinge damping (k_bend_damp,
// k_bend_damp_eval), links (k_link, k_link_eval), pressure (k_pressure, k_pressure_eval), shell bending (k_hinge_gather,
// k_hinge_gather_eval) and the report's bending energy (measure_bend_row).  Host only, no HIP
// header: a plain C++17 program can include it (tests/test_row_tables.py does, under the address and undefined-behaviour
// sanitizers).
//
// A table holds one row per vertex that has something to add, in ascending original vertex id; row r belongs to the
// particle row_pid[r] (faces in front + vertex).  Its records are stored in sliced ELL: slices of 64 rows -- one wave --,
// a slice as wide as its longest row, its records column-major: record e of the slice's lane l is at
// ent[slice_off[s] + 64 e + l], so a wave reads contiguous records per step, and slice_off[s + 1] - slice_off[s] is 64
// times the slice's width.  slice_off has one more element than there are slices; its last is the number of records.  A
// row shorter than its slice is padded with a record that must evaluate to an EXACT zero whatever the state and must name
// a particle the row may read: each table pads with the row's own id and zero coefficients (the shell table's records
// name hinge records, not particles: its padding is a word that no record can be, and is skipped).  The lanes of the last slice
// past the last row are never read; they hold the last row's padding.  Three device arrays carry a table (row_pid,
// slice_off, ent: BendArgs, LinkArgs; uploaded by rows_upload, mpm_cloth_host.h).
#pragma once
#include <math.h>
#include <stddef.h>

#include <algorithm>
#include <vector>

namespace mpm {

// A table on the host: what sliced_ell fills and rows_upload (mpm_cloth_host.h) copies to the device
template <class Record>
struct RowTable {
    std::vector<int> row_pid;          // [row] particle id (faces in front + vertex) of the row's vertex, ascending
    std::vector<unsigned> slice_off;   // [slices + 1]
    std::vector<Record> ent;
};

// Lays n_rows rows out: len(r) records get(r, 0 .. len(r) - 1) for row r, pad(r) behind them up to the slice's width.
// `slice`: rows per slice (64 on the device; the tests pass less).  No rows: slice_off = {0}, ent empty.  false, with
// nothing usable in the outputs: a slice would end at or past 2^31 records (the caller words the refusal).
template <class Record, class Len, class Get, class Pad>
inline bool sliced_ell(size_t n_rows, size_t slice, Len len, Get get, Pad pad, std::vector<unsigned>& slice_off,
                       std::vector<Record>& ent) {
    const size_t n_slices = (n_rows + slice - 1) / slice;
    slice_off.assign(n_slices + 1, 0u);
    for (size_t s = 0; s < n_slices; ++s) {
        size_t width = 0;
        for (size_t r = s * slice; r < std::min(n_rows, (s + 1) * slice); ++r) width = std::max(width, (size_t)len(r));
        if (!((size_t)slice_off[s] + width * slice < (size_t)1 << 31)) return false;
        slice_off[s + 1] = slice_off[s] + (unsigned)(width * slice);
    }
    ent.resize(slice_off[n_slices]);
    for (size_t s = 0; s < n_slices; ++s) {
        const size_t width = (slice_off[s + 1] - slice_off[s]) / slice;
        for (size_t l = 0, r = s * slice; l < slice; ++l, ++r)
            for (size_t q = 0; q < width; ++q)
                ent[slice_off[s] + q * slice + l] = r < n_rows && q < (size_t)len(r) ? get(r, q) : pad(std::min(r, n_rows - 1));
    }
    return true;
}

// The rate of a stability guard (Gershgorin on the lumped system): max over the rows with sum[r] > 0 of
// scale * sum[r] / mass(r); INFINITY where such a row's mass is not positive, 0 where no row counts.
template <class Mass>
inline double max_row_rate(const double* sum, size_t n_rows, double scale, Mass mass) {
    double worst = 0.0;
    for (size_t r = 0; r < n_rows; ++r)
        if (sum[r] > 0.0) {
            const double m = (double)mass(r);
            worst = std::max(worst, m > 0.0 ? scale * sum[r] / m : (double)INFINITY);
        }
    return worst;
}

}  // namespace mpm
