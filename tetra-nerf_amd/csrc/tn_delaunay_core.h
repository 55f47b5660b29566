// tn_delaunay_core.h -- the per-face arithmetic of the Delaunay monitor (tn_delaunay_check) and the per-tetrahedron rule of the
// state transfer (tn_remap_tet_values), written once for the kernels (tn_delaunay.hip) and the CPU emulation
// (tests/host/delaunay_emul.cpp), the way tn_vertex_guard_core.h states the limiter.  The same statements in numpy float64:
// geometry.py (delaunay_face_statement, remap_tet_values_statement).
//
// The predicate.  An interior face with the tetrahedra t0 = (p0, p1, p2, p3) and t1 on its two sides is
// locally Delaunay iff e, the vertex of t1 that t0 does not name, is not strictly inside the circumsphere of t0.  With
//     I = | p0-e  |p0-e|^2 |           O = | p0-p3 |
//         | p1-e  |p1-e|^2 |               | p1-p3 |
//         | p2-e  |p2-e|^2 |               | p2-p3 |
//         | p3-e  |p3-e|^2 |
// e is inside iff I and O have the same sign (O > 0 is a tetrahedron whose ((p1-p0) x (p2-p0)) . (p3-p0) is negative).  Both are
// evaluated in double on the fp32 coordinates by the stage-A expressions of J. R. Shewchuk, "Adaptive Precision Floating-Point
// Arithmetic and Fast Robust Geometric Predicates" (1997), each beside its permanent (the same expression with every term taken
// in magnitude), one rounding per operation in the order written.  The a-priori bounds of that paper,
//     |I - exact| <= (16 + 224 eps) eps perm_I,      |O - exact| <= (7 + 56 eps) eps perm_O,      eps = 2^-53,
// cover the rounding of the differences, so a determinant whose magnitude exceeds its bound has the exact sign.  A face where
// either does not is UNCERTAIN -- cospherical points and zero-volume tetrahedra land there, NaN too -- and nothing decides it
// on the device.
#pragma once
#include <cstdint>
#include <cmath>

#if !defined(TN_HD)
#if defined(__HIPCC__)
#define TN_HD __host__ __device__ __forceinline__
#else
#define TN_HD inline
#endif
#endif

namespace tn {
namespace delaunay {

constexpr double EPS = 1.0 / 9007199254740992.0;             // 2^-53
constexpr double INSPHERE_BOUND = (16.0 + 224.0 * EPS) * EPS;   // Shewchuk's isperrboundA
constexpr double ORIENT_BOUND = (7.0 + 56.0 * EPS) * EPS;       // Shewchuk's o3derrboundA

enum State : int {
    HULL = 0,        // one tetrahedron only: nothing to test
    REGULAR = 1,     // both signs certain, e not inside
    VIOLATED = 2,    // both signs certain, e strictly inside the circumsphere of t0
    UNCERTAIN = 3,   // a determinant within its error bound (or NaN)
};

struct Det { double det, perm; };
struct Verdict { int state; bool inverted; };   // inverted: VIOLATED and t0 certainly of negative orientation as stored

// O and its permanent: the 3 x 3 orientation determinant translated by p3
TN_HD Det orient_det(const float p[4][3]) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const double adx = (double)p[0][0] - (double)p[3][0], ady = (double)p[0][1] - (double)p[3][1], adz = (double)p[0][2] - (double)p[3][2];
    const double bdx = (double)p[1][0] - (double)p[3][0], bdy = (double)p[1][1] - (double)p[3][1], bdz = (double)p[1][2] - (double)p[3][2];
    const double cdx = (double)p[2][0] - (double)p[3][0], cdy = (double)p[2][1] - (double)p[3][1], cdz = (double)p[2][2] - (double)p[3][2];
    const double bdxcdy = bdx * cdy, cdxbdy = cdx * bdy;
    const double cdxady = cdx * ady, adxcdy = adx * cdy;
    const double adxbdy = adx * bdy, bdxady = bdx * ady;
    const double det = (adz * (bdxcdy - cdxbdy) + bdz * (cdxady - adxcdy)) + cdz * (adxbdy - bdxady);
    const double perm = ((fabs(bdxcdy) + fabs(cdxbdy)) * fabs(adz) + (fabs(cdxady) + fabs(adxcdy)) * fabs(bdz)) +
                        (fabs(adxbdy) + fabs(bdxady)) * fabs(cdz);
    return Det{det, perm};
}

// I and its permanent: the 4 x 4 in-sphere determinant translated by e
TN_HD Det insphere_det(const float p[4][3], const float e[3]) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const double aex = (double)p[0][0] - (double)e[0], aey = (double)p[0][1] - (double)e[1], aez = (double)p[0][2] - (double)e[2];
    const double bex = (double)p[1][0] - (double)e[0], bey = (double)p[1][1] - (double)e[1], bez = (double)p[1][2] - (double)e[2];
    const double cex = (double)p[2][0] - (double)e[0], cey = (double)p[2][1] - (double)e[1], cez = (double)p[2][2] - (double)e[2];
    const double dex = (double)p[3][0] - (double)e[0], dey = (double)p[3][1] - (double)e[1], dez = (double)p[3][2] - (double)e[2];
    const double aexbey = aex * bey, bexaey = bex * aey, ab = aexbey - bexaey;
    const double bexcey = bex * cey, cexbey = cex * bey, bc = bexcey - cexbey;
    const double cexdey = cex * dey, dexcey = dex * cey, cd = cexdey - dexcey;
    const double dexaey = dex * aey, aexdey = aex * dey, da = dexaey - aexdey;
    const double aexcey = aex * cey, cexaey = cex * aey, ac = aexcey - cexaey;
    const double bexdey = bex * dey, dexbey = dex * bey, bd = bexdey - dexbey;
    const double abc = (aez * bc - bez * ac) + cez * ab;
    const double bcd = (bez * cd - cez * bd) + dez * bc;
    const double cda = (cez * da + dez * ac) + aez * cd;
    const double dab = (dez * ab + aez * bd) + bez * da;
    const double alift = (aex * aex + aey * aey) + aez * aez;
    const double blift = (bex * bex + bey * bey) + bez * bez;
    const double clift = (cex * cex + cey * cey) + cez * cez;
    const double dlift = (dex * dex + dey * dey) + dez * dez;
    const double det = (dlift * abc - clift * dab) + (blift * cda - alift * bcd);
    const double aezp = fabs(aez), bezp = fabs(bez), cezp = fabs(cez), dezp = fabs(dez);
    const double abp = fabs(aexbey) + fabs(bexaey), bcp = fabs(bexcey) + fabs(cexbey), cdp = fabs(cexdey) + fabs(dexcey);
    const double dap = fabs(dexaey) + fabs(aexdey), acp = fabs(aexcey) + fabs(cexaey), bdp = fabs(bexdey) + fabs(dexbey);
    const double perm = (((cdp * bezp + bdp * cezp) + bcp * dezp) * alift + ((dap * cezp + acp * dezp) + cdp * aezp) * blift) +
                        (((abp * dezp + bdp * aezp) + dap * bezp) * clift + ((bcp * aezp + acp * bezp) + abp * cezp) * dlift);
    return Det{det, perm};
}

// the verdict on one interior face: p = the corners of t0 in stored order, e = the vertex of t1 that t0 does not name
TN_HD Verdict face_verdict(const float p[4][3], const float e[3]) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const Det in = insphere_det(p, e), orr = orient_det(p);
    const bool certain = fabs(in.det) > INSPHERE_BOUND * in.perm && fabs(orr.det) > ORIENT_BOUND * orr.perm;   // false for NaN
    if (!certain) return Verdict{UNCERTAIN, false};
    const bool inside = (in.det > 0.0) == (orr.det > 0.0);
    return Verdict{inside ? VIOLATED : REGULAR, inside && orr.det > 0.0};
}

// which vertex of c1 is `e`: the first one c0 does not name (a valid face has exactly one; where c0 names all four the last is
// taken, every difference of one row is then zero and the face comes out UNCERTAIN)
TN_HD uint32_t opposite_vertex(const uint32_t c0[4], const uint32_t c1[4]) {
    uint32_t e = c1[3];
    for (int k = 2; k >= 0; --k) {
        const uint32_t v = c1[k];
        if (v != c0[0] && v != c0[1] && v != c0[2] && v != c0[3]) e = v;
    }
    return e;
}

// the transfer's rule: the larger of two per-tetrahedron values by their bit patterns as unsigned integers.  For non-negative
// floats (+0 and +inf included) that is the larger float.  NaN and negative values are outside the contract: by this rule a set
// sign bit beats everything and a positive NaN beats every number.
TN_HD uint32_t max_bits(uint32_t a, uint32_t b) { return a > b ? a : b; }

}  // namespace delaunay
}  // namespace tn
