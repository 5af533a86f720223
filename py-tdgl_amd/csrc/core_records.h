// The records of vortex cores taken inside the time loops (census.inc, DESIGN.md section 3, "Cores in the loop"), as the
// host puts them together after a flush: plain C++, no HIP headers (csrc/census.inc includes it for the flush and for
// the host entry point tdgl_host_core_records_assemble; a stand-alone host program can include it alone).
//
// Between two flushes the kernels append one record per charged triangle of every recorded step to a pool, through a
// cursor: the launches are ordered on the stream, so the records of consecutive steps are contiguous, in the order of
// the steps -- and within a step in whatever order the wavefronts reserved their slots.  The census rows of the window
// say how many each step has (n_plus + n_minus), hence where its segment begins.  A record whose slot is at or beyond
// the capacity was not written.
//
//   a step whose segment ends within the capacity is complete: its records, sorted by triangle number (a triangle
//     has at most one record per step, so the order is total and two runs give the same bytes)
//   a step whose segment reaches beyond the capacity is incomplete and delivers no records -- which of them fitted
//     depends on the scheduling --, and so is every later recorded step of the window, whatever its count
#pragma once

#include <algorithm>
#include <cstdint>

namespace tdgl_cores {

struct Record {  // 24 bytes, what a hit lane writes
    int32_t triangle, charge;  // a row of the caller's triangles (reference numbering), +1 / -1
    double x, y;               // the zero of the linear interpolant of psi on that triangle
};

// rows: [n_rows][ncol] int32 census rows of the window (columns 0, 1: n_plus, n_minus); recorded: [n_rows], nonzero for
// the steps that recorded cores; pool: the first min(sum of their counts, capacity) records of the device's pool.
// Per recorded step k, in the order of the rows: row[k] its row in the window, offset[k] .. offset[k + 1] its records in
// out (offset has one entry more than there are recorded steps), complete[k].  out holds at most min(sum, capacity)
// records.  Returns the number of recorded steps.
inline int64_t assemble(int64_t n_rows, int32_t ncol, const int32_t *rows, const uint8_t *recorded, const Record *pool,
                        int64_t capacity, int64_t *row, int64_t *offset, uint8_t *complete, Record *out) {
    int64_t steps = 0, begin = 0, kept = 0;  // begin: where the step's segment starts in the pool
    bool overflowed = false;
    offset[0] = 0;
    for (int64_t r = 0; r < n_rows; ++r) {
        if (!recorded[r]) continue;
        const int64_t count = (int64_t)rows[r * ncol] + (int64_t)rows[r * ncol + 1];
        if (begin + count > capacity) overflowed = true;
        row[steps] = r;
        complete[steps] = overflowed ? 0 : 1;
        if (!overflowed && count > 0) {
            std::copy(pool + begin, pool + begin + count, out + kept);
            std::sort(out + kept, out + kept + count, [](const Record &a, const Record &b) { return a.triangle < b.triangle; });
            kept += count;
        }
        begin += count;
        offset[++steps] = kept;
    }
    return steps;
}

}  // namespace tdgl_cores
