// mvosr_score_math.hpp — the 3 x 4 pose arithmetic of mvosr_score.hip, in plain C++ so that a host compiler builds the very same
// operations (no contraction: the including file is built with -ffp-contract=off; an FMA is written fma()).
#pragma once

#include <math.h>

#if defined(__HIPCC__)
#define MVOSR_HD __host__ __device__
#else
#define MVOSR_HD
#endif

namespace mvosr {

struct Pose { double m[12]; };

MVOSR_HD inline Pose pose_load(const double *p) {
    Pose a;
    for (int k = 0; k < 12; ++k) a.m[k] = p[k];
    return a;
}

MVOSR_HD inline bool pose_rotation_is_zero(const Pose &a) {
    bool z = true;
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) z = z && a.m[4 * r + c] == 0.0;
    return z;
}

// one row of A * B (B's last row is 0 0 0 1)
MVOSR_HD inline void pose_row_mul(const double a[4], const double *b, double out[4]) {
    for (int j = 0; j < 4; ++j)
        out[j] = ((a[0] * b[j] + a[1] * b[4 + j]) + a[2] * b[8 + j]) + a[3] * (j == 3 ? 1.0 : 0.0);
}

MVOSR_HD inline Pose pose_mul(const Pose &a, const Pose &b) {
    Pose o;
    for (int r = 0; r < 3; ++r) pose_row_mul(&a.m[4 * r], b.m, &o.m[4 * r]);
    return o;
}

MVOSR_HD inline Pose pose_inverse(const Pose &a) {
    const double r00 = a.m[0], r01 = a.m[1], r02 = a.m[2], r10 = a.m[4], r11 = a.m[5], r12 = a.m[6], r20 = a.m[8], r21 = a.m[9], r22 = a.m[10];
    const double c00 = r11 * r22 - r12 * r21, c01 = r02 * r21 - r01 * r22, c02 = r01 * r12 - r02 * r11;
    const double c10 = r12 * r20 - r10 * r22, c11 = r00 * r22 - r02 * r20, c12 = r02 * r10 - r00 * r12;
    const double c20 = r10 * r21 - r11 * r20, c21 = r01 * r20 - r00 * r21, c22 = r00 * r11 - r01 * r10;
    const double det = (r00 * c00 + r01 * c10) + r02 * c20;
    Pose o;
    o.m[0] = c00 / det; o.m[1] = c01 / det; o.m[2] = c02 / det;
    o.m[4] = c10 / det; o.m[5] = c11 / det; o.m[6] = c12 / det;
    o.m[8] = c20 / det; o.m[9] = c21 / det; o.m[10] = c22 / det;
    const double t0 = a.m[3], t1 = a.m[7], t2 = a.m[11];
    for (int r = 0; r < 3; ++r) o.m[4 * r + 3] = -((o.m[4 * r] * t0 + o.m[4 * r + 1] * t1) + o.m[4 * r + 2] * t2);
    return o;
}

MVOSR_HD inline double norm3(double x, double y, double z) { return sqrt((x * x + y * y) + z * z); }

// ---- the segment error, in double-double -------------------------------------------------------------------------------------
// r_err = acos(0.5 (trace(e) - 1)) of a small angle multiplies every rounding of trace(e) by 1 / sin(r_err) — a few hundred on a
// 100 m segment — and the per-length means add the roundings of hundreds of segments up: evaluated in plain doubles, the kernel's
// own rounding noise (another inverse and another product order than LAPACK's and BLAS's) is as large as the reference's.  So the
// chain q = inv(P_first) P_last, e = inv(q) g is carried as unevaluated sums hi + lo of two doubles (error-free products by fma,
// error-free sums): about 100 bits, rounded to a double once, in front of acos and sqrt.  Same formulas, same inputs.
struct dd { double hi, lo; };

MVOSR_HD inline dd dd_two_sum(double a, double b) {
    const double s = a + b, bb = s - a;
    return {s, (a - (s - bb)) + (b - bb)};
}
MVOSR_HD inline dd dd_quick(double a, double b) {          // |a| >= |b|
    const double s = a + b;
    return {s, b - (s - a)};
}
MVOSR_HD inline dd dd_prod(double a, double b) {
    const double p = a * b;
    return {p, fma(a, b, -p)};
}
MVOSR_HD inline dd dd_add(dd a, dd b) {
    dd s = dd_two_sum(a.hi, b.hi);
    const dd t = dd_two_sum(a.lo, b.lo);
    s = dd_quick(s.hi, s.lo + t.hi);
    return dd_quick(s.hi, s.lo + t.lo);
}
MVOSR_HD inline dd dd_neg(dd a) { return {-a.hi, -a.lo}; }
MVOSR_HD inline dd dd_sub(dd a, dd b) { return dd_add(a, dd_neg(b)); }
MVOSR_HD inline dd dd_mul(dd a, dd b) {
    dd p = dd_prod(a.hi, b.hi);
    p.lo = p.lo + (a.hi * b.lo + a.lo * b.hi);
    return dd_quick(p.hi, p.lo);
}
MVOSR_HD inline dd dd_div(dd a, dd b) {
    const double q1 = a.hi / b.hi;
    dd r = dd_sub(a, dd_mul(b, dd{q1, 0.0}));
    const double q2 = r.hi / b.hi;
    r = dd_sub(r, dd_mul(b, dd{q2, 0.0}));
    const double q3 = r.hi / b.hi;
    return dd_add(dd_quick(q1, q2), dd{q3, 0.0});
}

struct PoseDD { dd m[12]; };

MVOSR_HD inline PoseDD pose_widen(const Pose &a) {
    PoseDD o;
    for (int k = 0; k < 12; ++k) o.m[k] = {a.m[k], 0.0};
    return o;
}
MVOSR_HD inline PoseDD pose_join(const double *hi, const double *lo) {
    PoseDD o;
    for (int k = 0; k < 12; ++k) o.m[k] = {hi[k], lo[k]};
    return o;
}

MVOSR_HD inline PoseDD pose_mul(const PoseDD &a, const PoseDD &b) {
    PoseDD o;
    for (int r = 0; r < 3; ++r)
        for (int j = 0; j < 4; ++j) {
            dd s = dd_add(dd_add(dd_mul(a.m[4 * r], b.m[j]), dd_mul(a.m[4 * r + 1], b.m[4 + j])), dd_mul(a.m[4 * r + 2], b.m[8 + j]));
            o.m[4 * r + j] = j == 3 ? dd_add(s, a.m[4 * r + 3]) : s;
        }
    return o;
}

MVOSR_HD inline PoseDD pose_inverse(const PoseDD &a) {
    const dd r00 = a.m[0], r01 = a.m[1], r02 = a.m[2], r10 = a.m[4], r11 = a.m[5], r12 = a.m[6], r20 = a.m[8], r21 = a.m[9], r22 = a.m[10];
    const dd c00 = dd_sub(dd_mul(r11, r22), dd_mul(r12, r21)), c01 = dd_sub(dd_mul(r02, r21), dd_mul(r01, r22)), c02 = dd_sub(dd_mul(r01, r12), dd_mul(r02, r11));
    const dd c10 = dd_sub(dd_mul(r12, r20), dd_mul(r10, r22)), c11 = dd_sub(dd_mul(r00, r22), dd_mul(r02, r20)), c12 = dd_sub(dd_mul(r02, r10), dd_mul(r00, r12));
    const dd c20 = dd_sub(dd_mul(r10, r21), dd_mul(r11, r20)), c21 = dd_sub(dd_mul(r01, r20), dd_mul(r00, r21)), c22 = dd_sub(dd_mul(r00, r11), dd_mul(r01, r10));
    const dd det = dd_add(dd_add(dd_mul(r00, c00), dd_mul(r01, c10)), dd_mul(r02, c20));
    PoseDD o;
    o.m[0] = dd_div(c00, det); o.m[1] = dd_div(c01, det); o.m[2] = dd_div(c02, det);
    o.m[4] = dd_div(c10, det); o.m[5] = dd_div(c11, det); o.m[6] = dd_div(c12, det);
    o.m[8] = dd_div(c20, det); o.m[9] = dd_div(c21, det); o.m[10] = dd_div(c22, det);
    for (int r = 0; r < 3; ++r)
        o.m[4 * r + 3] = dd_neg(dd_add(dd_add(dd_mul(o.m[4 * r], a.m[3]), dd_mul(o.m[4 * r + 1], a.m[7])), dd_mul(o.m[4 * r + 2], a.m[11])));
    return o;
}

// the ground truth's delta inv(G_first) G_last of a segment, kept as hi and lo
MVOSR_HD inline PoseDD ground_delta(const Pose &first, const Pose &last) { return pose_mul(pose_inverse(pose_widen(first)), pose_widen(last)); }

// evaluate_vo.py:66-67, 21-33 for one segment: q = inv(P_first) P_last, e = inv(q) g; the rotation and translation error, each over
// the segment's length
MVOSR_HD inline void segment_error(const Pose &pf, const Pose &pl, const PoseDD &g, double length, double *r_err, double *t_err,
                                   bool *zero_block) {
    const PoseDD q = pose_mul(pose_inverse(pose_widen(pf)), pose_widen(pl));
    bool qz = true;
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) qz = qz && q.m[4 * r + c].hi == 0.0;
    *zero_block = pose_rotation_is_zero(pf) || qz;
    const PoseDD e = pose_mul(pose_inverse(q), g);
    const dd trace = dd_add(dd_add(e.m[0], e.m[5]), e.m[10]);
    const dd d2 = dd_add(trace, dd{-1.0, 0.0});                       // 0.5 (trace - 1): the halving is exact
    const double d = 0.5 * (d2.hi + d2.lo);
    *r_err = acos(fmax(fmin(d, 1.0), -1.0)) / length;
    const dd sq = dd_add(dd_add(dd_mul(e.m[3], e.m[3]), dd_mul(e.m[7], e.m[7])), dd_mul(e.m[11], e.m[11]));
    *t_err = sqrt(sq.hi + sq.lo) / length;
}

}  // namespace mvosr
