// Device spectra: amplitudes of chosen Fourier modes of model expressions (which wavenumber grows, at what
// rate, where the harmonics saturate), one row per record.
//
// A spectrum is an expression in the model's string language, lowered by codegen.lower_spectra to one case
// of tf_eval_spectrum (same emitter as tf_eval_F, tf_eval_probe, tf_eval_record and tf_eval_stat: the
// per-node values are the bits the reference's lambdified NumPy code computes), and a list of modes m_i in
// a device buffer.  A row is c[i] = sum_g v_g exp(-2 pi i m_i g / N) over the natural nodes g of a system:
// np.fft.fft(v)[m_i], unnormalised.  The generated spectrum block defines TF_NSPEC, TF_NSPEC_HC,
// TF_SPEC_USES_X and tf_eval_spectrum before this header is read: it is the tail of a spectrum code object's
// translation unit and of no other.
//
// The twiddle function and the walk of one thread (on the node window the spectra share with the other
// observers, tf_node.h) are what the host harness of the test suite (tests/spectrum_host/) also compiles
// with g++; the kernels are at the end of the file.
#pragma once
#include "tf_node.h"

// exp(-2 pi i r / N) for 0 <= r < N < 2^31: (*re, *im) = (cos, -sin) of 2 pi r / N.  The turn is cut into
// octants with integers -- q = 8 r / N, rem = 8 r - q N, both exact -- and libm only ever sees
// (pi / 4) rem / N, or (pi / 4) (N - rem) / N in the odd octants where the angle is measured back from the
// octant's end: an argument in [0, pi / 4] that carries three roundings, whatever r is.  The octant is put
// back with swaps and sign changes, which are exact; so multiples of a quarter turn give exactly +-1 and
// 0, and no zero is negative (0.0 - x, never -x).  cos(2 pi m g / N) with the product formed in floating
// point is wrong by about m g / N ulps instead.
TF_DEVICE void tf_spec_twiddle(int64_t r, int64_t N, double* re, double* im) {
    const int64_t r8 = 8 * r;
    const int q = (int)(r8 / N);
    const int64_t rem = r8 - (int64_t)q * N;
    const int64_t num = (q & 1) ? N - rem : rem;
    const double arg = 0.78539816339744830961566084581988 * ((double)num / (double)N);
    const double c = cos(arg), s = sin(arg);
    // angle = (q + 1) pi / 4 - arg in the odd octants, q pi / 4 + arg in the even ones
    const bool swap = ((q + 1) >> 1) & 1;              // octants 1, 2, 5, 6: the angle is off a half-turn axis
    const double ac = swap ? s : c, as = swap ? c : s; // |cos|, |sin| of the angle
    const bool cneg = q >= 2 && q <= 5, sneg = q >= 4;
    *re = cneg ? 0.0 - ac : ac;
    *im = sneg ? as : 0.0 - as;
}

// The step twiddles of mode m: w^(m j) for the nodes j = 0 ... TF_PROBE_SEG - 1 of a segment, step[j *
// stride] = (re, im).  One table per workgroup (LDS) serves every thread: a thread's nodes are g0 + j.
TF_DEVICE void tf_spec_step(int m, int j, int N, double* out) {
    tf_spec_twiddle(((int64_t)m * j) % N, N, out, out + 1);
}

// One thread, segment sg (TF_PROBE_SEG nodes) of chunk p of system e: the expression at the n nodes of
// the segment (0 ... TF_PROBE_SEG, the return value) into v in node order, *g0: the natural index of the
// first of them.  The state is read here, once, whatever the number of modes.
TF_DEVICE int tf_spectrum_values(const TfSpectrumArgs& a, int e, int p, int sg, double (&v)[TF_PROBE_SEG],
                                 int* g0) {
    const TfLayout& L = a.L;
    const int len = tf_len(L, p);
    const int i0 = sg * TF_PROBE_SEG;
    *g0 = tf_start(L, p) + i0;
    if (i0 >= len) return 0;
    TfNodeWindow<TF_NSPEC_HC, TF_SPEC_USES_X> W(a, e);
    W.prime(p, len, i0);
    int n = 0;
#pragma unroll
    for (int j = 0; j < TF_PROBE_SEG; ++j) {
        const int i = i0 + j;
        v[j] = 0.0;
        if (i >= len) continue;
        W.advance(p, len, i);
        v[j] = tf_eval_spectrum(a.which, W.w, W.par, W.hc, W.dx, W.xc);
        n = j + 1;
    }
    return n;
}

// +0.0 for finite values, NaN once one of them is a NaN or an infinity: added to both parts of every mode, it
// makes a row with a non-finite node NaN throughout.  (An infinity times a twiddle is an infinity of either
// sign or, at a twiddle's exact zero, a NaN: left alone, a row would hold whichever the mode's twiddles make
// of it.  Adding +0.0 changes no finite sum.)
TF_DEVICE double tf_spectrum_poison(int n, const double (&v)[TF_PROBE_SEG]) {
    double z = 0.0;
#pragma unroll
    for (int j = 0; j < TF_PROBE_SEG; ++j)
        if (j < n) z = z + v[j] * 0.0;
    return z;
}

// Mode m of the n values of a segment that starts at natural node g0: w^(m (g0 + j)) = w^(m g0) w^(m j),
// the two-level product.  u = sum_j v_j w^(m j) is accumulated in node order from the step table (two
// multiplies and two adds per node and mode); the base twiddle w^(m g0), with m g0 mod N in 64-bit
// integers, multiplies the sum once.  No recurrence: no twiddle is computed from another one.
// poison (tf_spectrum_poison of the same values) is added to both parts.
TF_DEVICE void tf_spectrum_mode(int m, int g0, int N, int n, const double (&v)[TF_PROBE_SEG], double poison,
                                const double* step, int stride, double* re, double* im) {
    double ur = 0.0, ui = 0.0;
#pragma unroll
    for (int j = 0; j < TF_PROBE_SEG; ++j)
        if (j < n) {
            ur = ur + v[j] * step[j * stride];
            ui = ui + v[j] * step[j * stride + 1];
        }
    double br, bi;
    tf_spec_twiddle(((int64_t)m * g0) % N, N, &br, &bi);
    *re = (br * ur - bi * ui) + poison;
    *im = (br * ui + bi * ur) + poison;
}

#if defined(__HIPCC__)
// grid (nsys * nblk, nseg), 256 threads, one launch per spectrum that is due: thread x of workgroup blk
// walks segment blockIdx.y of chunk blk * 256 + x, as in tfk_probe_partial -- the lanes of a wavefront
// sit over neighbouring chunks, so every load of the state is 512 contiguous bytes.  The segment's values
// stay in registers; per mode, the thread's (re, im) goes through the 64-lane xor tree (every lane ends
// with the same value: the partner sums are the same two operands) and LDS across the four wavefronts, in
// a fixed order; one pair per workgroup, mode and system leaves with plain stores.  Threads without nodes
// add +0.0.  No atomics on floating-point data: the series are bitwise reproducible.
extern "C" __global__ void __launch_bounds__(256) tfk_spectrum_partial(TfSpectrumArgs a) {
    __shared__ double step[TF_PROBE_SEG][TF_SPEC_MAX_MODES][2];
    __shared__ double part[4][TF_SPEC_MAX_MODES][2];
    const int e = blockIdx.x / a.nblk, blk = blockIdx.x - e * a.nblk, sg = blockIdx.y;
    const int p = blk * 256 + threadIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int nm = a.nmodes < TF_SPEC_MAX_MODES ? a.nmodes : TF_SPEC_MAX_MODES;
    const int N = a.L.N;
    for (int t = threadIdx.x; t < TF_PROBE_SEG * nm; t += 256) {
        const int j = t / nm, k = t - j * nm;
        tf_spec_step(a.modes[k], j, N, &step[j][k][0]);
    }
    double v[TF_PROBE_SEG];
    int n = 0, g0 = 0;
    if (p < a.L.P) n = tf_spectrum_values(a, e, p, sg, v, &g0);
    const double poison = tf_spectrum_poison(n, v);
    __syncthreads();
    for (int k = 0; k < nm; ++k) {
        double re = 0.0, im = 0.0;
        if (n > 0) tf_spectrum_mode(a.modes[k], g0, N, n, v, poison, &step[0][k][0], 2 * TF_SPEC_MAX_MODES, &re, &im);
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            re = re + __shfl_xor(re, off, 64);
            im = im + __shfl_xor(im, off, 64);
        }
        if (lane == 0) { part[wave][k][0] = re; part[wave][k][1] = im; }
    }
    __syncthreads();
    if ((int)threadIdx.x < nm) {
        const int k = threadIdx.x;
        double re = part[0][k][0], im = part[0][k][1];
        for (int w = 1; w < 4; ++w) { re = re + part[w][k][0]; im = im + part[w][k][1]; }
        double* out = a.partial + (((int64_t)e * nm + k) * a.nseg * a.nblk + sg * a.nblk + blk) * 2;
        out[0] = re;
        out[1] = im;
    }
}
// grid (nsys), 256 threads: wavefront w reduces modes w, w + 4, ... of one system -- the partials in a
// fixed order, strided over the lanes with eight loads in flight (as tfk_probe_final), then the shuffle
// tree -- and lane 0 writes the pair into row a.row of the ring.  The row comes by value, from the host's
// count of the rows: the launch is queued on the solver's stream between the steps, never inside a
// captured graph (a replay would write every row where it was captured).
extern "C" __global__ void __launch_bounds__(256) tfk_spectrum_final(TfSpectrumArgs a) {
    const int e = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int nb = a.nblk * a.nseg;
    for (int k = wave; k < a.nmodes; k += 4) {
        const double* part = a.partial + ((int64_t)e * a.nmodes + k) * nb * 2;
        double re = 0.0, im = 0.0;
        for (int b0 = lane; b0 < nb; b0 += 64 * 8) {
            double vr[8], vi[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int b = b0 + 64 * j;
                vr[j] = b < nb ? part[2 * b] : 0.0;
                vi[j] = b < nb ? part[2 * b + 1] : 0.0;
            }
#pragma unroll
            for (int j = 0; j < 8; ++j)
                if (b0 + 64 * j < nb) { re = re + vr[j]; im = im + vi[j]; }
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            re = re + __shfl_xor(re, off, 64);
            im = im + __shfl_xor(im, off, 64);
        }
        if (lane == 0 && a.row >= 0 && a.row < a.capacity) {
            double* out = a.ring + (((int64_t)a.row * a.L.nsys + e) * a.nmodes + k) * 2;
            out[0] = re;
            out[1] = im;
        }
    }
}
#endif
