// Point location on a triangulation through a uniform grid of cells: plain C++, no HIP headers (csrc/sample.inc
// includes it for the host entry point and for the kernel; a stand-alone host program can include it alone).
//
// The answer for a point p is the LOWEST-NUMBERED triangle whose three barycentric coordinates are all >= -1e-12
// ("Currents between the sites"), with triinterp.py's formula: per triangle (a, b, c) the inverse
// of the edge matrix [b - a, c - a] is precomputed, inv = (e2y, -e2x, -e1y, e1x) / det, and
//     l1 = inv0 dx + inv1 dy,   l2 = inv2 dx + inv3 dy,   l0 = (1 - l1) - l2,      (dx, dy) = p - a
// every product and sum rounded on its own.  A triangle with det == 0 (or a non-finite inverse) is never chosen.
//
// The grid only narrows the candidates.  A cell lists, in ascending order, every triangle whose bounding box, inflated
// by 1e-9 of the triangle's larger extent, overlaps it; a point's cell comes from the same monotone function of its
// coordinate that placed the boxes, so a point inside an inflated box always finds that triangle in its cell's list, and
// a point that passes the test above lies inside the inflated box (the tolerance moves it out of the triangle by 1e-12
// of an edge at the most).  Walking the list in order and stopping at the first hit is therefore the exhaustive search.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>

#if defined(__HIPCC__)
#define TDGL_SAMPLE_HD __host__ __device__
#else
#define TDGL_SAMPLE_HD
#endif

namespace tdgl_sample {

constexpr double LOCATE_TOL = 1e-12;
constexpr double BOX_INFLATE = 1e-9;
constexpr int64_t GRID_CAP = 16;  // the cells' lists hold at most GRID_CAP * n_tri entries

// What the search reads, as plain pointers (host vectors or device buffers).
struct GridView {
    double x0 = 0.0, y0 = 0.0, inv_hx = 0.0, inv_hy = 0.0;
    int32_t nx = 1, ny = 1;
    const int64_t *cell_ptr = nullptr;  // [nx * ny + 1]
    const int32_t *cell_tri = nullptr;  // [cell_ptr[nx * ny]], ascending within a cell
    const double *tri = nullptr;        // [n_tri][6]: a.x, a.y, inv0 .. inv3
};

// cell number along one axis: monotone in v, clamped to the border cells (a NaN product, 0 * inf, goes to cell 0)
TDGL_SAMPLE_HD inline int32_t grid_cell(double v, double v0, double inv_h, int32_t n) {
    const double f = floor((v - v0) * inv_h);
    if (!(f >= 0.0)) return 0;
    if (f >= (double)n) return n - 1;
    return (int32_t)f;
}

// The triangle of (px, py) and its weights (l0, l1, l2); -1 and zeros when it is in none.
TDGL_SAMPLE_HD inline int32_t locate_point(const GridView &g, double px, double py, double *w) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const int32_t cx = grid_cell(px, g.x0, g.inv_hx, g.nx), cy = grid_cell(py, g.y0, g.inv_hy, g.ny);
    const int64_t cell = (int64_t)cy * g.nx + cx;
    for (int64_t k = g.cell_ptr[cell]; k < g.cell_ptr[cell + 1]; ++k) {
        const int32_t t = g.cell_tri[k];
        const double *q = g.tri + 6 * (int64_t)t;
        const double dx = px - q[0], dy = py - q[1];
        const double l1 = q[2] * dx + q[3] * dy;
        const double l2 = q[4] * dx + q[5] * dy;
        const double l0 = (1.0 - l1) - l2;
        if (l0 >= -LOCATE_TOL && l1 >= -LOCATE_TOL && l2 >= -LOCATE_TOL) {
            w[0] = l0, w[1] = l1, w[2] = l2;
            return t;
        }
    }
    w[0] = w[1] = w[2] = 0.0;
    return -1;
}

struct Grid {
    double x0 = 0.0, y0 = 0.0, inv_hx = 0.0, inv_hy = 0.0;
    int32_t nx = 1, ny = 1;
    std::vector<int64_t> cell_ptr;
    std::vector<int32_t> cell_tri;
    std::vector<double> tri;
    GridView view() const {
        GridView v;
        v.x0 = x0, v.y0 = y0, v.inv_hx = inv_hx, v.inv_hy = inv_hy, v.nx = nx, v.ny = ny;
        v.cell_ptr = cell_ptr.data(), v.cell_tri = cell_tri.data(), v.tri = tri.data();
        return v;
    }
};

namespace detail {
struct CellBox {
    int32_t cx0, cx1, cy0, cy1;
};

inline void set_axes(Grid &g, double w, double h, int32_t nx, int32_t ny) {
    g.nx = nx, g.ny = ny;
    g.inv_hx = (w > 0.0 && nx > 1) ? (double)nx / w : 0.0;
    g.inv_hy = (h > 0.0 && ny > 1) ? (double)ny / h : 0.0;
}
}  // namespace detail

// sites_xy [n_sites][2] finite, elements [n_tri][3] in range (the caller has checked both).  Deterministic: the
// lists come from a counting sort over the triangles in ascending order.
inline Grid build_grid(int64_t n_sites, const double *sites_xy, int64_t n_tri, const int32_t *elements) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    Grid g;
    double xmin = sites_xy[0], xmax = xmin, ymin = sites_xy[1], ymax = ymin;
    for (int64_t i = 1; i < n_sites; ++i) {
        xmin = std::min(xmin, sites_xy[2 * i]), xmax = std::max(xmax, sites_xy[2 * i]);
        ymin = std::min(ymin, sites_xy[2 * i + 1]), ymax = std::max(ymax, sites_xy[2 * i + 1]);
    }
    g.x0 = xmin, g.y0 = ymin;
    const double w = xmax - xmin, h = ymax - ymin;
    // per triangle: the corner a and the inverse edge matrix, as triinterp.py forms them; the inflated box
    g.tri.assign((size_t)(6 * n_tri), 0.0);
    std::vector<double> box((size_t)(4 * n_tri));
    std::vector<char> usable((size_t)n_tri, 0);
    for (int64_t t = 0; t < n_tri; ++t) {
        const double *a = sites_xy + 2 * (int64_t)elements[3 * t], *b = sites_xy + 2 * (int64_t)elements[3 * t + 1],
                     *c = sites_xy + 2 * (int64_t)elements[3 * t + 2];
        const double e1x = b[0] - a[0], e1y = b[1] - a[1], e2x = c[0] - a[0], e2y = c[1] - a[1];
        const double det = e1x * e2y - e1y * e2x;
        double *q = g.tri.data() + 6 * t;
        q[0] = a[0], q[1] = a[1];
        q[2] = e2y / det, q[3] = -e2x / det, q[4] = -e1y / det, q[5] = e1x / det;
        usable[t] = det != 0.0 && std::isfinite(q[2]) && std::isfinite(q[3]) && std::isfinite(q[4]) && std::isfinite(q[5]);
        const double bx0 = std::min(a[0], std::min(b[0], c[0])), bx1 = std::max(a[0], std::max(b[0], c[0]));
        const double by0 = std::min(a[1], std::min(b[1], c[1])), by1 = std::max(a[1], std::max(b[1], c[1]));
        const double pad = BOX_INFLATE * std::max(bx1 - bx0, by1 - by0);
        box[4 * t] = bx0 - pad, box[4 * t + 1] = bx1 + pad, box[4 * t + 2] = by0 - pad, box[4 * t + 3] = by1 + pad;
    }
    // about one cell per triangle, square cells; then coarsen until the lists respect the cap
    const double cells = (double)std::max<int64_t>(n_tri, 1);
    int32_t nx = 1, ny = 1;
    const double limit = 32768.0;
    if (w > 0.0 && h > 0.0) {
        const double side = std::sqrt(w * h / cells);
        nx = (int32_t)std::min(limit, std::max(1.0, std::ceil(w / side)));
        ny = (int32_t)std::min(limit, std::max(1.0, std::ceil(h / side)));
    } else if (w > 0.0) {
        nx = (int32_t)std::min(limit, cells);
    } else if (h > 0.0) {
        ny = (int32_t)std::min(limit, cells);
    }
    std::vector<detail::CellBox> cb((size_t)n_tri);
    for (;;) {
        detail::set_axes(g, w, h, nx, ny);
        int64_t entries = 0;
        for (int64_t t = 0; t < n_tri; ++t) {
            if (!usable[t]) continue;
            detail::CellBox &r = cb[t];
            r.cx0 = grid_cell(box[4 * t], g.x0, g.inv_hx, nx), r.cx1 = grid_cell(box[4 * t + 1], g.x0, g.inv_hx, nx);
            r.cy0 = grid_cell(box[4 * t + 2], g.y0, g.inv_hy, ny), r.cy1 = grid_cell(box[4 * t + 3], g.y0, g.inv_hy, ny);
            entries += (int64_t)(r.cx1 - r.cx0 + 1) * (r.cy1 - r.cy0 + 1);
        }
        if (entries <= GRID_CAP * std::max<int64_t>(n_tri, 1) || (nx == 1 && ny == 1)) break;
        nx = (nx + 1) / 2, ny = (ny + 1) / 2;
    }
    const int64_t n_cells = (int64_t)nx * ny;
    g.cell_ptr.assign((size_t)(n_cells + 1), 0);
    for (int64_t t = 0; t < n_tri; ++t) {
        if (!usable[t]) continue;
        for (int32_t cy = cb[t].cy0; cy <= cb[t].cy1; ++cy)
            for (int32_t cx = cb[t].cx0; cx <= cb[t].cx1; ++cx) ++g.cell_ptr[(size_t)((int64_t)cy * nx + cx) + 1];
    }
    for (int64_t c = 0; c < n_cells; ++c) g.cell_ptr[c + 1] += g.cell_ptr[c];
    g.cell_tri.assign((size_t)g.cell_ptr[n_cells], 0);
    std::vector<int64_t> fill(g.cell_ptr.begin(), g.cell_ptr.end() - 1);
    for (int64_t t = 0; t < n_tri; ++t) {  // ascending t: every list comes out ascending
        if (!usable[t]) continue;
        for (int32_t cy = cb[t].cy0; cy <= cb[t].cy1; ++cy)
            for (int32_t cx = cb[t].cx0; cx <= cb[t].cx1; ++cx) g.cell_tri[(size_t)fill[(int64_t)cy * nx + cx]++] = (int32_t)t;
    }
    return g;
}

}  // namespace tdgl_sample
