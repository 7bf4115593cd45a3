"""TEST-ONLY: the referee and the inputs the CPU and GPU tests of the device spectra share.

The referee is the discrete Fourier transform in extended precision: ``r = (m * g) mod N`` in int64 (exact),
the angle ``2 * pi * r / N``, the products and ``np.sum`` in ``np.longdouble`` with pi from a 36-digit literal
(mpmath at 40 digits where the platform's long double has no 64-bit significand).  The twiddles of one ``N``
are a table over ``r``, computed once.

Accuracy is asserted per mode as ``|c - c_ref| <= BOUND_ULPS * 2**-53 * sum_g |v_g|``.  In these units
``np.fft.fft`` itself is within 1.5 of the referee, a NumPy model of the kernels' arithmetic (octant
twiddles, two-level product, sums of 8, then a tree) within 0.8, and twiddles from ``np.exp(-2j * pi * m * g
/ N)`` with the product formed in floating point are off by 15 to 79 at the modes >= N // 4 of N >= 4099: so
8 is five times what the reference library needs and half of what the bug it is meant to catch produces.
"""
import numpy as np

BOUND_ULPS = 8.0
UNIT = 2.0 ** -53
_PI = "3.14159265358979323846264338327950288"
_EXTENDED = np.finfo(np.longdouble).nmant >= 63
_TABLES = {}


def twiddle_table(N):
    """exp(-2 pi i r / N) for r = 0 ... N - 1 as (cos, -sin), two ``np.longdouble`` arrays."""
    if N not in _TABLES:
        if _EXTENDED:
            ang = 2 * np.longdouble(_PI) * np.arange(N, dtype=np.int64).astype(np.longdouble) / np.longdouble(N)
            _TABLES[N] = (np.cos(ang), -np.sin(ang))
        else:
            import mpmath
            with mpmath.workdps(40):
                pi = mpmath.mpf(_PI)
                ang = [2 * pi * r / N for r in range(N)]
                _TABLES[N] = (np.array([np.longdouble(str(mpmath.cos(a))) for a in ang]),
                              np.array([np.longdouble(str(-mpmath.sin(a))) for a in ang]))
    return _TABLES[N]


def twiddle_exact(r, N):
    """One twiddle of the referee, (re, im) as ``np.longdouble`` -- any N, no table."""
    if _EXTENDED:
        ang = 2 * np.longdouble(_PI) * np.longdouble(int(r)) / np.longdouble(int(N))
        return np.cos(ang), -np.sin(ang)
    import mpmath
    with mpmath.workdps(40):
        ang = 2 * mpmath.mpf(_PI) * int(r) / int(N)
        return np.longdouble(str(mpmath.cos(ang))), np.longdouble(str(-mpmath.sin(ang)))


def referee(v, modes):
    """``sum_g v_g exp(-2 pi i m g / N)`` for the modes ``m``: (re, im), ``np.longdouble`` [nmodes], or
    [rows, nmodes] for ``v [rows, N]`` (the twiddles of a mode are gathered once for all rows)."""
    v = np.asarray(v, dtype=float)
    N = v.shape[-1]
    c, s = twiddle_table(N)
    vl = v.astype(np.longdouble)
    g = np.arange(N, dtype=np.int64)
    re, im = [], []
    for m in modes:
        r = (np.int64(m) * g) % np.int64(N)
        re.append(np.sum(vl * c[r], axis=-1))
        im.append(np.sum(vl * s[r], axis=-1))
    return np.stack(re, axis=-1), np.stack(im, axis=-1)


def ratios(got, v, modes):
    """``|got - referee| / (2**-53 * sum |v|)`` per mode (``got``: complex128 [nmodes], or [rows, nmodes]
    for ``v [rows, N]``)."""
    got = np.asarray(got)
    re, im = referee(v, modes)
    err = np.hypot(got.real.astype(np.longdouble) - re, got.imag.astype(np.longdouble) - im)
    scale = np.longdouble(UNIT) * np.sum(np.abs(np.asarray(v, dtype=float)).astype(np.longdouble), axis=-1)
    return np.asarray(err / np.asarray(scale)[..., None], dtype=float)


def mode_set(N):
    """Low modes, the quarter and the top of the spectrum: where twiddles from a floating-point product
    of m and g lose the most."""
    return sorted({0, 1, 5, 7, min(31, N // 2), N // 4, N // 2 - 1, N // 2})


def low_and_top_modes(N, low=32):
    """``low`` low modes plus N // 4, N // 2 - 1 and N // 2."""
    return sorted(set(range(low)) | {N // 4, N // 2 - 1, N // 2})


def signal(N, seed=3):
    """``1 + 0.3 cos(2 pi 5 x) + 0.05 N(0, 1)`` on x = g / N."""
    x = np.arange(N) / float(N)
    return 1.0 + 0.3 * np.cos(2 * np.pi * 5 * x) + 0.05 * np.random.RandomState(seed).standard_normal(N)
