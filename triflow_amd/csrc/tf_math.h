// Scalar arithmetic helpers used by the generated stencil bodies and the kernel
// skeletons.  Included before the generated per-model code.
#pragma once
#ifndef TF_DEVICE
#error "define TF_DEVICE before including tf_math.h"
#endif
// streaming store of write-once data (Jacobian planes, F): bypasses cache
// allocation on the device, plain store in the host build
#ifndef TF_STORE_STREAM
#define TF_STORE_STREAM(ptr, val) (*(ptr) = (val))
#endif
#ifndef TF_DEVICE_M          // qualifier of in-class functions
#define TF_DEVICE_M TF_DEVICE
#endif

// ---------------------------------------------------------------- arithmetic
// The stencil bodies are compiled with -ffp-contract=off and mirror the
// operation tree NumPy evaluates, so F and J agree bit for bit with the
// reference's numpy-compiler path for + - * / sqrt and integer powers.
TF_DEVICE double tf_sq(double a) { return a * a; }

// correctly rounded (up to double rounding, ~2^-50) small integer powers via
// double-double products -- what a correctly rounded libm pow() returns
TF_DEVICE double tf_powi(double x, int n) {
    bool neg = n < 0;
    if (neg) n = -n;
    double hi = 1.0, lo = 0.0;
    for (int k = 0; k < n; ++k) {
        double p = hi * x;
        double e = __builtin_fma(hi, x, -p);
        e = __builtin_fma(lo, x, e);
        double s = p + e;
        lo = e - (s - p);
        hi = s;
    }
    if (!neg) return hi + lo;
    // 1 / (hi + lo), corrected with the exact residual of the rounded quotient
    double q = 1.0 / hi;
    double r = __builtin_fma(-hi, q, 1.0);
    r = __builtin_fma(-lo, q, r);
    return __builtin_fma(r, q, q);
}
// x / d for a divisor d that is the same for every node of a thread (dx, dx**2,
// scalar parameters): rd = RN(1/d) is computed once per thread, the quotient is
//   q = RN(x*rd);  r = x - q*d (exact, FMA);  q' = RN(q + r*rd)
// which is the correctly rounded x/d (Markstein's theorem) for finite operands in
// the normal range, the one exception being a divisor whose significand is all
// ones (probability 2^-52 for a grid spacing): there the result is still within
// one ulp of the quotient (before its last rounding q + r*rd equals x/d to a
// relative 2^-104, so q' is a faithful rounding; measured on 2 x 200 such divisors
// over 600 binades: 0.5 ulp, none differs from IEEE division,
// profiles/r08_vocabulary.txt).  Replaces the ~35-instruction fp64
// division expansion by 3 instructions without changing a bit of the result
// (checked against NumPy on every F/J parity vector).  Non-finite inputs give
// NaN where IEEE division would give inf: the run has failed either way.
TF_DEVICE double tf_div_u(double x, double d, double rd) {
    const double q = x * rd;
    const double r = __builtin_fma(-q, d, x);
    return __builtin_fma(r, rd, q);
}
// tf_div_u for the exact mode of the models, where an infinite state is a legitimate
// input (a Piecewise or a Heaviside may keep it out of the result, and NumPy's bits are promised there too):
// x * rd is already IEEE's quotient when it is not finite (+-inf with the sign of x / d, or the NaN), where
// the residual correction would turn it into a NaN, and when x is a zero (the zero with the sign of x / d,
// which the correction's +0 residual would make +0: a tie of Max(U, 0) is such a numerator).  On the device
// that is what v_div_fixup_f64 does to a quotient, given divisor and numerator: one instruction more than
// tf_div_u (the selects written out cost six per quotient, a third of the F+J sweep of the Burgers model of
// DESIGN.md section 20); it returns the quotient of finite non-zero operands as it is.  The host build (the
// tests' emulation) has no such instruction and takes IEEE's own division for every operand pair with a NaN,
// an infinity or a zero in it -- the same case table, d == 0 and d == inf included.  The two still differ where
// the fixup flushes a quotient below the denormal range or saturates one whose operands' exponents are more
// than 1075 apart: operands outside the normal range, which tf_div_u does not promise either.
TF_DEVICE double tf_div_x(double x, double d, double rd) {
    const double q = x * rd;
    const double r = __builtin_fma(-q, d, x);
    const double s = __builtin_fma(r, rd, q);
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_div_fixup(s, d, x);
#else
    const bool ordinary = (x - x) == 0.0 && x != 0.0 && (d - d) == 0.0 && d != 0.0;
    return ordinary ? s : x / d;
#endif
}
// np.maximum / np.minimum: a NaN operand wins; of two zeros of either sign (they compare equal) the
// second operand comes back with its own sign bit, tf_max(+0, -0) = -0 and tf_max(-0, +0) = +0, likewise
// tf_min -- what NumPy's loops return, pinned in tests/test_vocabulary.py
TF_DEVICE double tf_max(double a, double b) { return (a > b || a != a) ? a : b; }
TF_DEVICE double tf_min(double a, double b) { return (a < b || a != a) ? a : b; }
// np.sign: +1, -1, +0.0 for a zero of either sign (never -0.0: 1/sign(u) and a comparison of bytes
// would see it), the NaN itself for a NaN
TF_DEVICE double tf_sign(double a) { return a > 0 ? 1.0 : (a < 0 ? -1.0 : (a == 0 ? 0.0 : a)); }
// np.heaviside(a, h0), the exact mode of the models: 0 below zero, 1 above, h0 at a
// zero of either sign, the NaN itself for a NaN.  A straight chain of unconditional selects: a nested
// conditional is a branch to the compiler, which it flattens in some kernels and not in others.
TF_DEVICE double tf_heaviside(double a, double h0) {
    double r = a;
    r = (a == 0.0) ? h0 : r;
    r = (a < 0.0) ? 0.0 : r;
    r = (a > 0.0) ? 1.0 : r;
    return r;
}
// one link of np.select: both values are arguments, so both are evaluated, as NumPy evaluates every
// branch of a Piecewise; the result is one of them, bit for bit
TF_DEVICE double tf_select(bool c, double a, double b) { return c ? a : b; }
// np.nan, the value of a Piecewise none of whose conditions holds
TF_DEVICE double tf_nan() { return __builtin_nan(""); }
TF_DEVICE double tf_fma(double a, double b, double c) { return __builtin_fma(a, b, c); }
TF_DEVICE double tf_abs(double a) { return __builtin_fabs(a); }
TF_DEVICE bool tf_finite(double a) { return (a - a) == 0.0; }

