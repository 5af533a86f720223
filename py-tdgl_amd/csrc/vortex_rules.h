// The two integer rules of DESIGN.md section 3, "Vortex cores and windings", as device functions: the charge of a
// triangle and the winding around a closed loop of sites -- and the position of the core inside a charged triangle.
// One copy for the kernels of vortices.inc (saved order parameters) and of census.inc (the live state inside the time
// loops); tdgl_amd/vortices.py restates them in NumPy.
//
// Every sign decision compares two separately rounded products p = u.re v.im and q = u.im v.re and never takes the
// sign of a difference, so a contraction of p - q into an FMA cannot change a decision.
#pragma once

namespace tdgl {

__device__ inline int vortex_sign(double p, double q) { return (p > q) - (p < q); }

// +1 / -1 when psi winds once around the triangle (a, b, c) in the order given, 0 otherwise (also for a vertex that
// is zero or NaN: every comparison is then false)
__device__ inline int vortex_triangle_winding(double2 a, double2 b, double2 c) {
    const int sab = vortex_sign(a.x * b.y, a.y * b.x);
    const int sbc = vortex_sign(b.x * c.y, b.y * c.x);
    const int sca = vortex_sign(c.x * a.y, c.y * a.x);
    if (sab > 0 && sbc > 0 && sca > 0) return 1;
    if (sab < 0 && sbc < 0 && sca < 0) return -1;
    return 0;
}

// The zero of the linear interpolant of psi on the triangle with values (a, b, c) at the corners (ra, rb, rc): the
// crosses ca = b x c, cb = c x a, cc = a x b, S = (ca + cb) + cc, the weights c / S, and (la ra + lb rb) + lc rc per
// coordinate.  The only place that takes p - q; positions are compared within the bound of DESIGN.md section 3.
__device__ inline double2 vortex_core_position(double2 a, double2 b, double2 c, double2 ra, double2 rb, double2 rc) {
    const double ca = b.x * c.y - b.y * c.x, cb = c.x * a.y - c.y * a.x, cc = a.x * b.y - a.y * b.x;
    const double S = (ca + cb) + cc;
    const double la = ca / S, lb = cb / S, lc = cc / S;
    return make_double2((la * ra.x + lb * rb.x) + lc * rc.x, (la * ra.y + lb * rb.y) + lc * rc.y);
}

// One wavefront, all 64 lanes taking part: Sunday's crossing rule around the origin over the edges u -> v of the
// closed loop loop_sites[e0 .. e1) of z, lanes striding over the edges.  Every lane returns the winding, or
// TDGL_WINDING_UNDEFINED when a vertex is zero or not finite or an edge is a segment through the origin.
__device__ inline int vortex_loop_winding(const double2 *__restrict__ z, const int32_t *__restrict__ loop_sites,
                                          int64_t e0, int64_t e1, int lane) {
    int w = 0, undefined = 0;
    for (int64_t e = e0 + lane; e < e1; e += WAVE) {
        const double2 u = z[loop_sites[e]];
        const double2 v = z[loop_sites[e + 1 < e1 ? e + 1 : e0]];
        if ((u.x == 0.0 && u.y == 0.0) || !isfinite(u.x) || !isfinite(u.y)) undefined = 1;
        const double p = u.x * v.y, q = u.y * v.x;
        const double rr = u.x * v.x, ii = u.y * v.y;
        if (p == q && (rr < 0.0 || ii < 0.0)) undefined = 1;
        if (u.y <= 0.0 && v.y > 0.0 && p > q) ++w;
        if (u.y > 0.0 && v.y <= 0.0 && p < q) --w;
    }
#pragma unroll
    for (int d = WAVE / 2; d > 0; d >>= 1) {
        w += __shfl_xor(w, d, WAVE);
        undefined |= __shfl_xor(undefined, d, WAVE);
    }
    return undefined ? TDGL_WINDING_UNDEFINED : w;
}

}  // namespace tdgl
