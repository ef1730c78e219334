// qhull_margin.h -- how Qhull sees a sign of the 2-D Delaunay triangulation, as ONE definition for the two triangulators that answer
// for it: the host's (delaunay.cpp, worst_margin) and the device's (delaunay_dev.hip).  Both must judge a quad or a hull corner by the
// very same arithmetic, or one of them would answer where the other refuses.
//
// Qhull lifts (x, y) to z = x*x + y*y WITHOUT centring, scales z to the range [0, m], m = the largest |x| or |y| ('Qbb'), and takes a
// point for coplanar with a facet when its distance from the facet's plane is within a few DISTround = eps * (3 * sqrt(3) * 1.01 + 1) * m;
// z itself carries eps * z of rounding before the scaling.  A ratio (distance / allowance) far above one is a sign Qhull cannot get
// wrong; same_amd/delaunay.py:GUARD is how far above.
// Plain C++ for the host compiler and __host__ __device__ under hipcc; -ffp-contract=off in both builds (the Makefile), so every
// expression below is evaluated as written wherever it is compiled.
#pragma once
#include <cmath>

#if defined(__HIPCC__)
#define QM_HD __host__ __device__ inline
#else
#define QM_HD inline
#endif

namespace qm {

constexpr double EPS = 2.220446049250313e-16;

QM_HD double max2(double a, double b) { return a < b ? b : a; }   // std::max's semantics, on both sides

// Qbb's scale of the lifted coordinate and the plane distance Qhull cannot tell from zero, for a set with largest |x| or |y| m and
// lifted range [zmin, zmax]
struct Scale {
    double s, allow;
};
QM_HD Scale scale(double m, double zmin, double zmax) {
    const double s = zmax > zmin ? m / (zmax - zmin) : 1.0;
    const double allow = EPS * (6.25 * m + zmax * s);
    return Scale{s, allow};
}

// per triangle (x0, y0), (x0 + dx, y0 + dy), (x0 + ex, y0 + ey): the plane of the lifted triangle is z = 2 c . x + const, c its
// circumcentre -- slope 2 |c| before the scaling; a thin triangle's plane is known that much worse (longest side over height); the
// distance of a point with in-circle determinant det is s * det / (2 area) / sqrt(1 + slope^2).  -> the factor that turns |det| into
// distance / allowance
QM_HD double judge(double x0, double y0, double dx, double dy, double ex, double ey, Scale sc) {
    const double bl = dx * dx + dy * dy, cl = ex * ex + ey * ey, d = dx * ey - dy * ex, area2 = std::fabs(d);
    const double ccx = x0 + (ey * bl - dy * cl) * 0.5 / d, ccy = y0 + (dx * cl - ex * bl) * 0.5 / d;
    const double slope2 = 4 * sc.s * sc.s * (ccx * ccx + ccy * ccy);
    const double l2 = max2(bl, max2(cl, (ex - dx) * (ex - dx) + (ey - dy) * (ey - dy)));
    return sc.s / (area2 * std::sqrt(1 + slope2) * sc.allow * max2(1.0, l2 / area2));
}

// a hull edge or chord of length `edge` and a point at twice-area `area2` from it (in plain coordinates: the facet next to a hull
// edge is vertical, it holds Qhull's point at infinity 'Qz') -> distance / allowance
QM_HD double plain_ratio(double area2, double edge, Scale sc) { return area2 / edge / sc.allow; }

}  // namespace qm
