// fg_psis_dd.h -- double-double arithmetic (an unevaluated sum hi + lo of two doubles, about 106 bits) for the Pareto fit of
// fg_psis.hip: sums, products, quotients, sqrt, exp, expm1, log and log1p to about 1e-30 relative.  The rule of DESIGN 3.22 is stated in
// IEEE double, where l_j multiplies the rounding of a profile mean by M ahead of a softmax; the device evaluates the same formulas
// in this arithmetic, in the same fixed orders, and rounds each word once at the end, so what it reports sits at the exact value of
// the rule on the table's cells rather than one more double evaluation away from it.  Error-free transformations (Dekker, Knuth)
// with fma for the product; the unit is compiled with -ffp-contract=off, which they rely on.  Host and device (the plan driver
// checks the functions against long double).
#pragma once
#include <cmath>

#ifdef __HIPCC__
#define FG_DD_HD __host__ __device__ inline
#else
#define FG_DD_HD inline
#endif

struct FgDD { double hi, lo; };

FG_DD_HD FgDD fg_dd(double a) { FgDD r; r.hi = a; r.lo = 0.0; return r; }
FG_DD_HD bool fg_dd_finite(double a) { return a - a == 0.0; }
// a + b exactly (a non-finite sum carries no low part)
FG_DD_HD FgDD fg_dd_two_sum(double a, double b) {
    FgDD r;
    r.hi = a + b;
    const double bb = r.hi - a;
    r.lo = (a - (r.hi - bb)) + (b - bb);
    if (!fg_dd_finite(r.hi)) r.lo = 0.0;
    return r;
}
// the same for |a| >= |b|
FG_DD_HD FgDD fg_dd_fast_sum(double a, double b) {
    FgDD r;
    r.hi = a + b;
    r.lo = b - (r.hi - a);
    if (!fg_dd_finite(r.hi)) r.lo = 0.0;
    return r;
}
FG_DD_HD FgDD fg_dd_add(FgDD a, FgDD b) {
    FgDD s = fg_dd_two_sum(a.hi, b.hi);
    const FgDD t = fg_dd_two_sum(a.lo, b.lo);
    s.lo += t.hi;
    s = fg_dd_fast_sum(s.hi, s.lo);
    s.lo += t.lo;
    return fg_dd_fast_sum(s.hi, s.lo);
}
FG_DD_HD FgDD fg_dd_neg(FgDD a) { FgDD r; r.hi = -a.hi; r.lo = -a.lo; return r; }
FG_DD_HD FgDD fg_dd_sub(FgDD a, FgDD b) { return fg_dd_add(a, fg_dd_neg(b)); }
FG_DD_HD FgDD fg_dd_add_d(FgDD a, double b) { return fg_dd_add(a, fg_dd(b)); }
FG_DD_HD FgDD fg_dd_mul(FgDD a, FgDD b) {
    const double p = a.hi * b.hi;
    double e = fma(a.hi, b.hi, -p);
    e += a.hi * b.lo + a.lo * b.hi;
    return fg_dd_fast_sum(p, e);
}
FG_DD_HD FgDD fg_dd_mul_d(FgDD a, double b) {
    const double p = a.hi * b;
    double e = fma(a.hi, b, -p);
    e += a.lo * b;
    return fg_dd_fast_sum(p, e);
}
// by a power of two: exact
FG_DD_HD FgDD fg_dd_scale(FgDD a, double p2) { FgDD r; r.hi = a.hi * p2; r.lo = a.lo * p2; return r; }
FG_DD_HD FgDD fg_dd_div(FgDD a, FgDD b) {
    const double q1 = a.hi / b.hi;
    if (!fg_dd_finite(q1)) return fg_dd(q1);
    FgDD r = fg_dd_sub(a, fg_dd_mul_d(b, q1));
    const double q2 = r.hi / b.hi;
    r = fg_dd_sub(r, fg_dd_mul_d(b, q2));
    const double q3 = r.hi / b.hi;
    return fg_dd_add_d(fg_dd_fast_sum(q1, q2), q3);
}
FG_DD_HD FgDD fg_dd_sqrt(FgDD a) {                         // Karp and Markstein; a > 0
    const double x = 1.0 / sqrt(a.hi), ax = a.hi * x;
    const FgDD d = fg_dd_sub(a, fg_dd_mul(fg_dd(ax), fg_dd(ax)));
    return fg_dd_two_sum(ax, d.hi * (x * 0.5));
}
FG_DD_HD double fg_dd_round(FgDD a) { return a.hi + a.lo; }
FG_DD_HD bool fg_dd_gt(FgDD a, FgDD b) { return a.hi > b.hi || (a.hi == b.hi && a.lo > b.lo); }

// expm1 for |a| <= 0.35: the argument over 512, the series to the eighth power, nine doublings s <- 2 s + s^2
FG_DD_HD FgDD fg_dd_expm1_core(FgDD a) {
    const FgDD m = fg_dd_scale(a, 1.0 / 512.0);
    FgDD q = fg_dd(1.0 / 40320.0);
    q = fg_dd_add_d(fg_dd_mul(q, m), 1.0 / 5040.0);
    q = fg_dd_add_d(fg_dd_mul(q, m), 1.0 / 720.0);
    q = fg_dd_add_d(fg_dd_mul(q, m), 1.0 / 120.0);
    q = fg_dd_add_d(fg_dd_mul(q, m), 1.0 / 24.0);
    q = fg_dd_add(fg_dd_mul(q, m), fg_dd_div(fg_dd(1.0), fg_dd(6.0)));
    q = fg_dd_add_d(fg_dd_mul(q, m), 0.5);
    FgDD s = fg_dd_add(m, fg_dd_mul(fg_dd_mul(m, m), q));
    for (int i = 0; i < 9; ++i) s = fg_dd_add(fg_dd_scale(s, 2.0), fg_dd_mul(s, s));
    return s;
}
#define FG_DD_LN2_HI 6.931471805599452862e-01
#define FG_DD_LN2_LO 2.319046813846299558e-17
FG_DD_HD FgDD fg_dd_exp(FgDD a) {
    if (a.hi != a.hi) return fg_dd(a.hi);
    if (a.hi <= -745.2) return fg_dd(0.0);
    if (a.hi >= 709.79) return fg_dd(INFINITY);
    const double k = rint(a.hi * 1.4426950408889634);
    FgDD ln2; ln2.hi = FG_DD_LN2_HI; ln2.lo = FG_DD_LN2_LO;
    const FgDD r = fg_dd_sub(a, fg_dd_mul_d(ln2, k));
    const FgDD e = fg_dd_add_d(fg_dd_expm1_core(r), 1.0);
    const int ki = (int)k;
    FgDD out; out.hi = ldexp(e.hi, ki); out.lo = ldexp(e.lo, ki);
    return out;
}
FG_DD_HD FgDD fg_dd_expm1(FgDD a) {
    if (fabs(a.hi) <= 0.34) return fg_dd_expm1_core(a);
    return fg_dd_add_d(fg_dd_exp(a), -1.0);
}
// one Newton step on exp from the double logarithm: x + a exp(-x) - 1
FG_DD_HD FgDD fg_dd_log(FgDD a) {
    if (a.hi != a.hi || a.hi < 0.0) return fg_dd(NAN);
    if (a.hi == 0.0) return fg_dd(-INFINITY);
    if (!fg_dd_finite(a.hi)) return fg_dd(a.hi);
    const FgDD x = fg_dd(log(a.hi));
    const FgDD y = fg_dd_mul(a, fg_dd_exp(fg_dd_neg(x)));
    return fg_dd_add(x, fg_dd_add_d(y, -1.0));
}
FG_DD_HD FgDD fg_dd_log1p(FgDD a) { return fg_dd_log(fg_dd_add_d(a, 1.0)); }
