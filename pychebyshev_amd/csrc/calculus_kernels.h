// calculus_kernels.h -- batched roots, minima and maxima of 1-D Chebyshev interpolants (gfx950).
//
// The device half of roots() / minimize() / maximize() (reference _calculus.py:198-297).  One wavefront per fibre
// (the n <= 64 values of a 1-D interpolant at its ascending type-I nodes), everything in LDS:
//
//   1. min/max: f = D v (D the fibre's differentiation matrix), roots: f = v
//   2. Chebyshev coefficients of f: the DCT-II of the reversed values / n with c_0 halved, as a matrix product over a
//      cosine table of the 4n reduced angles
//   3. trim trailing coefficients that are exactly zero (NumPy as_series); < 2 left: no roots, 2: -c_0 / c_1
//   4. else the colleague matrix of NumPy's chebcompanion, m = degree <= 63, flipped as chebroots flips it
//      ([::-1, ::-1]: lower Hessenberg with a dense first column), then LAPACK dgeev's path for it: dgebal's power-of-two
//      scaling loop (its permutation step finds nothing to isolate: every off-diagonal neighbour is 1/2 or sqrt(1/2))
//      and dgehd2's Householder reduction to upper Hessenberg form.  The flip and the reduction matter: when the trailing
//      coefficients are round-off, the last column holds entries near 1e16, and the unflipped, unreduced matrix gives
//      roots some 1e-8 away from NumPy's (which are then accurate to ~1e-15)
//   5. eigenvalues by the Francis double-shift QR of LAPACK dlahqr (eigenvalues only): deflation on a negligible
//      subdiagonal, exceptional shifts every 10 iterations, 30 max(10, m) iterations at most, 2 x 2 blocks by dlanv2
//   6. keep |imag| < 1e-10 and -1 - 1e-10 <= re <= 1 + 1e-10; an eigenvalue within 1e-10 of +-1, on either side, is
//      that end and gives exactly lo or hi (the reference clips only from outside, so a root at an end came back a few
//      ulp inside it as often as not); the others are mapped to [lo, hi]; rank-sort, drop a root that does not exceed
//      its predecessor by more than 1e-10 (hi - lo + 1)
//   7. min/max: the candidates [lo, critical points..., hi] evaluated barycentrically on v (first node within 1e-14
//      -> that node's value), the first best one wins (a NaN wins, as in np.argmin / np.argmax)
//
// Every decision (deflation, shifts, trimming, counts) is computed by all lanes from the same LDS data, so it is uniform
// across the wave; the lanes share only the O(m) row and column updates of each reflector and the O(n^2) products.
// No atomics: a row's result depends on its own fibre only, bit for bit, whatever the batch.
//
// The solver is written once for both compilation passes: on the device the CALC_LANES loops are strided over the 64
// lanes and CALC_SYNC is a workgroup barrier (a workgroup is one wave, and every branch around a barrier is uniform);
// on the host they are plain loops, which lets the arithmetic be checked on a CPU.
#pragma once

#include "pcx_common.h"

#include <float.h>
#include <math.h>

#pragma clang fp contract(off)     // no fused multiply-add: the same roundings as the NumPy statements restated here

#define PCX_CALC_MAX_N 64          // fibre length limit (the reference's max_n default)
#define PCX_CALC_EXTRA (12 * 64 + 256)   // LDS doubles besides the matrix: vectors of 64 and the 4n-entry cosine table

#define CALC_FN __host__ __device__ inline
#if defined(__HIP_DEVICE_COMPILE__)
#define CALC_LANES(j, lo, hi) for (int j = (lo) + (int)(threadIdx.x & 63); j < (hi); j += 64)
#define CALC_ONE if ((threadIdx.x & 63) == 0)
#define CALC_SYNC() __syncthreads()
#else
#define CALC_LANES(j, lo, hi) for (int j = (lo); j < (hi); ++j)
#define CALC_ONE
#define CALC_SYNC() ((void)0)
#endif

struct CalcArgs {
    int n;                    // fibre length, 1 .. PCX_CALC_MAX_N
    int mode;                 // 0 roots, 1 minimize, 2 maximize
    int W;                    // roots row stride: max(n - 1, 1)
    double lo, hi;            // the fibre's physical interval
    const double *nodes;      // n ascending nodes
    const double *wts;        // n barycentric weights
    const double *diff;       // n x n differentiation matrix, row-major (modes 1, 2)
    const double *vals;       // rows x n fibre values
    double *roots;            // rows x W, ascending, NaN-padded (mode 0)
    int32_t *counts;          // rows: roots / critical points found, -1 = failed
    double *val, *loc;        // rows (modes 1, 2)
};

// LAPACK dlapy2: sqrt(x^2 + y^2) without needless overflow
CALC_FN double calc_lapy2(double x, double y) {
    if (x != x) return x;
    if (y != y) return y;
    const double xa = fabs(x), ya = fabs(y);
    const double w = fmax(xa, ya), z = fmin(xa, ya);
    if (z == 0.0 || w > DBL_MAX) return w;
    const double q = z / w;
    return w * sqrt(1.0 + q * q);
}

// LAPACK dlarfg for a reflector of order nr <= 3: alpha in, beta out; (x1, x2) -- x2 only when nr == 3 -- become
// v(2:nr); returns tau
CALC_FN double calc_larfg(int nr, double &alpha, double &x1, double &x2) {
    if (nr <= 1) return 0.0;
    double xnorm = nr == 2 ? fabs(x1) : calc_lapy2(x1, x2);
    if (xnorm == 0.0) return 0.0;
    double beta = -copysign(calc_lapy2(alpha, xnorm), alpha);
    const double safmin = DBL_MIN / (DBL_EPSILON * 0.5);       // dlamch('S') / dlamch('E')
    int knt = 0;
    if (fabs(beta) < safmin) {
        const double rsafmn = 1.0 / safmin;
        do {
            ++knt;
            x1 *= rsafmn;
            if (nr == 3) x2 *= rsafmn;
            beta *= rsafmn;
            alpha *= rsafmn;
        } while (fabs(beta) < safmin && knt < 20);
        xnorm = nr == 2 ? fabs(x1) : calc_lapy2(x1, x2);
        beta = -copysign(calc_lapy2(alpha, xnorm), alpha);
    }
    const double tau = (beta - alpha) / beta;
    const double sc = 1.0 / (alpha - beta);
    x1 *= sc;
    if (nr == 3) x2 *= sc;
    for (int q = 0; q < knt; ++q) beta *= safmin;
    alpha = beta;
    return tau;
}

// LAPACK dlanv2: eigenvalues (rt1r + i rt1i, rt2r + i rt2i) of the 2 x 2 block [a b; c d] in standard form
CALC_FN void calc_lanv2(double a, double b, double c, double d, double &rt1r, double &rt1i, double &rt2r, double &rt2i) {
    const double eps = DBL_EPSILON;                            // dlamch('P')
    const double safmn2 = 0x1p-485, safmx2 = 0x1p485;         // base^int(log(safmin / eps) / log(base) / 2)
    if (c == 0.0) {
    } else if (b == 0.0) {
        const double t = d;
        d = a;
        a = t;
        b = -c;
        c = 0.0;
    } else if ((a - d) == 0.0 && copysign(1.0, b) != copysign(1.0, c)) {
    } else {
        double temp = a - d;
        double p = 0.5 * temp;
        const double bcmax = fmax(fabs(b), fabs(c));
        const double bcmis = fmin(fabs(b), fabs(c)) * copysign(1.0, b) * copysign(1.0, c);
        double scale = fmax(fabs(p), bcmax);
        double z = (p / scale) * p + (bcmax / scale) * bcmis;
        if (z >= 4.0 * eps) {                                  // real eigenvalues
            z = p + copysign(sqrt(scale) * sqrt(z), p);
            a = d + z;
            d = d - (bcmax / z) * bcmis;
            b = b - c;
            c = 0.0;
        } else {                                               // complex, or real and nearly equal
            double sigma = b + c;
            for (int count = 1; count <= 21; ++count) {
                scale = fmax(fabs(temp), fabs(sigma));
                if (scale >= safmx2) { sigma *= safmn2; temp *= safmn2; continue; }
                if (scale <= safmn2) { sigma *= safmx2; temp *= safmx2; continue; }
                break;
            }
            p = 0.5 * temp;
            double tau = calc_lapy2(sigma, temp);
            const double cs = sqrt(0.5 * (1.0 + fabs(sigma) / tau));
            const double sn = -(p / (tau * cs)) * copysign(1.0, sigma);
            const double aa = a * cs + b * sn, bb = -a * sn + b * cs;
            const double cc = c * cs + d * sn, dd = -c * sn + d * cs;
            a = aa * cs + cc * sn;
            b = bb * cs + dd * sn;
            c = -aa * sn + cc * cs;
            d = -bb * sn + dd * cs;
            temp = 0.5 * (a + d);
            a = temp;
            d = temp;
            if (c != 0.0) {
                if (b != 0.0) {
                    if (copysign(1.0, b) == copysign(1.0, c)) {   // real eigenvalues
                        const double sab = sqrt(fabs(b)), sac = sqrt(fabs(c));
                        p = copysign(sab * sac, c);
                        a = temp + p;
                        d = temp - p;
                        b = b - c;
                        c = 0.0;
                    }
                } else {
                    b = -c;
                    c = 0.0;
                }
            }
        }
    }
    rt1r = a;
    rt2r = d;
    if (c == 0.0) {
        rt1i = rt2i = 0.0;
    } else {
        rt1i = sqrt(fabs(b)) * sqrt(fabs(c));
        rt2i = -rt1i;
    }
}

#define CALC_H(r, q) H[(r) * S + (q)]

// LAPACK dgebal's scaling loop (job 'S': no permutations) on the m x m matrix H; sc: m scratch doubles
template <int S>
CALC_FN void calc_balance(double *H, int m, double *sc) {
    const double sfmin1 = 0x1p-970, sfmax1 = 0x1p970;          // dlamch('S') / dlamch('P') and its inverse
    const double sfmin2 = sfmin1 * 2.0, sfmax2 = 1.0 / sfmin2;
    CALC_LANES(i, 0, m) sc[i] = 1.0;
    CALC_SYNC();
    for (int sweep = 0; sweep < 200; ++sweep) {
        bool noconv = false;
        for (int i = 0; i < m; ++i) {
            double ca = 0.0, ra = 0.0;
            for (int k = 0; k < m; ++k) {
                ca = fmax(ca, fabs(CALC_H(k, i)));
                ra = fmax(ra, fabs(CALC_H(i, k)));
            }
            if (ca == 0.0 || ra == 0.0) continue;
            double c = 0.0, r = 0.0;                           // 2-norms of column and row i (scaled sums)
            for (int k = 0; k < m; ++k) {
                const double x = CALC_H(k, i) / ca, y = CALC_H(i, k) / ra;
                c += x * x;
                r += y * y;
            }
            c = ca * sqrt(c);
            r = ra * sqrt(r);
            double g = r / 2.0, f = 1.0;
            const double s = c + r;
            while (c < g && fmax(f, fmax(c, ca)) < sfmax2 && fmin(r, fmin(g, ra)) > sfmin2) {
                f *= 2.0; c *= 2.0; ca *= 2.0; r /= 2.0; g /= 2.0; ra /= 2.0;
            }
            g = c / 2.0;
            while (g >= r && fmax(r, ra) < sfmax2 && fmin(fmin(f, c), fmin(g, ca)) > sfmin2) {
                f /= 2.0; c /= 2.0; g /= 2.0; ca /= 2.0; r *= 2.0; ra *= 2.0;
            }
            if ((c + r) >= 0.95 * s) continue;
            const double sci = sc[i];
            if (f < 1.0 && sci < 1.0 && f * sci <= sfmin1) continue;
            if (f > 1.0 && sci > 1.0 && sci >= sfmax1 / f) continue;
            g = 1.0 / f;
            noconv = true;
            CALC_SYNC();                                       // every lane has read row / column i
            CALC_LANES(k, 0, m) {
                if (k != i) {
                    CALC_H(i, k) *= g;
                    CALC_H(k, i) *= f;
                }
            }
            CALC_ONE sc[i] = sci * f;
            CALC_SYNC();
        }
        if (!noconv) break;
    }
}

// LAPACK dgehd2 (ilo = 0, ihi = m - 1): Householder reduction of H to upper Hessenberg form, eigenvalues only (the
// reflectors are not kept: the entries below the subdiagonal are zeroed).  v: m scratch doubles.
template <int S>
CALC_FN void calc_hessenberg(double *H, int m, double *v) {
    for (int i = 0; i + 1 < m; ++i) {
        const int L = m - 1 - i;                              // reflector order: rows i+1 .. m-1 of column i
        if (L < 2) break;                                     // dlarfg of order 1: tau = 0
        double xs = 0.0;                                      // dnrm2 of rows i+2 .. m-1 (scaled sum)
        for (int r = i + 2; r < m; ++r) xs = fmax(xs, fabs(CALC_H(r, i)));
        double xnorm = 0.0;
        if (xs > 0.0) {
            for (int r = i + 2; r < m; ++r) {
                const double q = CALC_H(r, i) / xs;
                xnorm += q * q;
            }
            xnorm = xs * sqrt(xnorm);
        }
        if (xnorm == 0.0) continue;                           // tau = 0: H = I
        const double alpha = CALC_H(i + 1, i);
        const double beta = -copysign(calc_lapy2(alpha, xnorm), alpha);
        const double tau = (beta - alpha) / beta;
        const double sc = 1.0 / (alpha - beta);
        CALC_SYNC();                                          // every lane has read column i
        CALC_LANES(r, i + 1, m) v[r - i - 1] = r == i + 1 ? 1.0 : CALC_H(r, i) * sc;
        CALC_SYNC();
        CALC_LANES(r, i + 1, m) CALC_H(r, i) = r == i + 1 ? beta : 0.0;
        CALC_LANES(r, 0, m) {                                 // from the right: columns i+1 .. m-1, a lane per row
            double w = 0.0;
            for (int j = 0; j < L; ++j) w += CALC_H(r, i + 1 + j) * v[j];
            for (int j = 0; j < L; ++j) CALC_H(r, i + 1 + j) = CALC_H(r, i + 1 + j) - (tau * w) * v[j];
        }
        CALC_SYNC();
        CALC_LANES(c, i + 1, m) {                             // from the left: rows i+1 .. m-1, a lane per column
            double w = 0.0;
            for (int j = 0; j < L; ++j) w += v[j] * CALC_H(i + 1 + j, c);
            for (int j = 0; j < L; ++j) CALC_H(i + 1 + j, c) = CALC_H(i + 1 + j, c) - (tau * v[j]) * w;
        }
        CALC_SYNC();
    }
}

// LAPACK dlahqr (wantt = wantz = false, ilo = 0, ihi = m - 1): eigenvalues of the upper Hessenberg H into wr / wi.
// False when an eigenvalue did not converge within 30 max(10, m) iterations.
template <int S>
CALC_FN bool calc_hqr(double *H, int m, double *wr, double *wi) {
    const double ulp = DBL_EPSILON;                            // dlamch('P')
    const double smlnum = DBL_MIN * ((double)m / ulp);
    const int itmax = 30 * (m > 10 ? m : 10);
    int kdefl = 0;
    int i = m - 1;
    while (i >= 0) {
        int l = 0;
        bool conv = false;
        for (int its = 0; its <= itmax; ++its) {
            int k;
            for (k = i; k > l; --k) {                          // a negligible subdiagonal entry
                if (fabs(CALC_H(k, k - 1)) <= smlnum) break;
                double tst = fabs(CALC_H(k - 1, k - 1)) + fabs(CALC_H(k, k));
                if (tst == 0.0) {
                    if (k - 2 >= 0) tst += fabs(CALC_H(k - 1, k - 2));
                    if (k + 1 <= m - 1) tst += fabs(CALC_H(k + 1, k));
                }
                if (fabs(CALC_H(k, k - 1)) <= ulp * tst) {
                    const double ab = fmax(fabs(CALC_H(k, k - 1)), fabs(CALC_H(k - 1, k)));
                    const double ba = fmin(fabs(CALC_H(k, k - 1)), fabs(CALC_H(k - 1, k)));
                    const double aa = fmax(fabs(CALC_H(k, k)), fabs(CALC_H(k - 1, k - 1) - CALC_H(k, k)));
                    const double bb = fmin(fabs(CALC_H(k, k)), fabs(CALC_H(k - 1, k - 1) - CALC_H(k, k)));
                    const double s = aa + ab;
                    if (ba * (ab / s) <= fmax(smlnum, ulp * (bb * (aa / s)))) break;
                }
            }
            l = k;
            if (l > 0) {
                CALC_SYNC();
                CALC_ONE CALC_H(l, l - 1) = 0.0;
                CALC_SYNC();
            }
            if (l >= i - 1) { conv = true; break; }
            ++kdefl;
            double h11, h12, h21, h22, s;
            if (kdefl % 20 == 0) {                             // exceptional shifts
                s = fabs(CALC_H(i, i - 1)) + fabs(CALC_H(i - 1, i - 2));
                h11 = 0.75 * s + CALC_H(i, i);
                h12 = -0.4375 * s;
                h21 = s;
                h22 = h11;
            } else if (kdefl % 10 == 0) {
                s = fabs(CALC_H(l + 1, l)) + fabs(CALC_H(l + 2, l + 1));
                h11 = 0.75 * s + CALC_H(l, l);
                h12 = -0.4375 * s;
                h21 = s;
                h22 = h11;
            } else {                                           // Wilkinson's double shift
                h11 = CALC_H(i - 1, i - 1);
                h21 = CALC_H(i, i - 1);
                h12 = CALC_H(i - 1, i);
                h22 = CALC_H(i, i);
            }
            s = fabs(h11) + fabs(h12) + fabs(h21) + fabs(h22);
            double rt1r, rt1i, rt2r, rt2i;
            if (s == 0.0) {
                rt1r = rt1i = rt2r = rt2i = 0.0;
            } else {
                h11 /= s; h21 /= s; h12 /= s; h22 /= s;
                const double tr = (h11 + h22) / 2.0;
                const double det = (h11 - tr) * (h22 - tr) - h12 * h21;
                const double rtdisc = sqrt(fabs(det));
                if (det >= 0.0) {
                    rt1r = tr * s;
                    rt2r = rt1r;
                    rt1i = rtdisc * s;
                    rt2i = -rt1i;
                } else {
                    rt1r = tr + rtdisc;
                    rt2r = tr - rtdisc;
                    if (fabs(rt1r - h22) <= fabs(rt2r - h22)) { rt1r *= s; rt2r = rt1r; }
                    else { rt2r *= s; rt1r = rt2r; }
                    rt1i = rt2i = 0.0;
                }
            }
            int mm;                                            // two consecutive small subdiagonal entries
            double v0 = 0.0, v1 = 0.0, v2 = 0.0;
            for (mm = i - 2; mm >= l; --mm) {
                double h21s = CALC_H(mm + 1, mm);
                s = fabs(CALC_H(mm, mm) - rt2r) + fabs(rt2i) + fabs(h21s);
                h21s = CALC_H(mm + 1, mm) / s;
                v0 = h21s * CALC_H(mm, mm + 1) + (CALC_H(mm, mm) - rt1r) * ((CALC_H(mm, mm) - rt2r) / s) - rt1i * (rt2i / s);
                v1 = h21s * (CALC_H(mm, mm) + CALC_H(mm + 1, mm + 1) - rt1r - rt2r);
                v2 = h21s * CALC_H(mm + 2, mm + 1);
                s = fabs(v0) + fabs(v1) + fabs(v2);
                v0 /= s; v1 /= s; v2 /= s;
                if (mm == l) break;
                const double h00 = fabs(CALC_H(mm, mm - 1)) * (fabs(v1) + fabs(v2));
                const double h01 = fabs(v0) * (fabs(CALC_H(mm - 1, mm - 1)) + fabs(CALC_H(mm, mm)) + fabs(CALC_H(mm + 1, mm + 1)));
                if (h00 <= ulp * h01) break;
            }
            for (k = mm; k <= i - 1; ++k) {                    // the double-shift QR step: chase the bulge
                const int nr = (i - k + 1) < 3 ? (i - k + 1) : 3;
                if (k > mm) {
                    v0 = CALC_H(k, k - 1);
                    v1 = CALC_H(k + 1, k - 1);
                    if (nr == 3) v2 = CALC_H(k + 2, k - 1);
                }
                const double t1 = calc_larfg(nr, v0, v1, v2);
                CALC_SYNC();                                   // every lane has read column k - 1
                if (k > mm) {
                    CALC_ONE {
                        CALC_H(k, k - 1) = v0;
                        CALC_H(k + 1, k - 1) = 0.0;
                        if (k < i - 1) CALC_H(k + 2, k - 1) = 0.0;
                    }
                } else if (mm > l) {
                    CALC_ONE CALC_H(k, k - 1) = CALC_H(k, k - 1) * (1.0 - t1);
                }
                CALC_SYNC();
                const double u2 = v1, t2 = t1 * u2;
                if (nr == 3) {
                    const double u3 = v2, t3 = t1 * u3;
                    CALC_LANES(j, k, i + 1) {                  // rows k .. k+2, a lane per column
                        const double sum = CALC_H(k, j) + u2 * CALC_H(k + 1, j) + u3 * CALC_H(k + 2, j);
                        CALC_H(k, j) = CALC_H(k, j) - sum * t1;
                        CALC_H(k + 1, j) = CALC_H(k + 1, j) - sum * t2;
                        CALC_H(k + 2, j) = CALC_H(k + 2, j) - sum * t3;
                    }
                    CALC_SYNC();
                    const int jhi = (k + 3 < i ? k + 3 : i) + 1;
                    CALC_LANES(j, l, jhi) {                    // columns k .. k+2, a lane per row
                        const double sum = CALC_H(j, k) + u2 * CALC_H(j, k + 1) + u3 * CALC_H(j, k + 2);
                        CALC_H(j, k) = CALC_H(j, k) - sum * t1;
                        CALC_H(j, k + 1) = CALC_H(j, k + 1) - sum * t2;
                        CALC_H(j, k + 2) = CALC_H(j, k + 2) - sum * t3;
                    }
                    CALC_SYNC();
                } else if (nr == 2) {
                    CALC_LANES(j, k, i + 1) {
                        const double sum = CALC_H(k, j) + u2 * CALC_H(k + 1, j);
                        CALC_H(k, j) = CALC_H(k, j) - sum * t1;
                        CALC_H(k + 1, j) = CALC_H(k + 1, j) - sum * t2;
                    }
                    CALC_SYNC();
                    CALC_LANES(j, l, i + 1) {
                        const double sum = CALC_H(j, k) + u2 * CALC_H(j, k + 1);
                        CALC_H(j, k) = CALC_H(j, k) - sum * t1;
                        CALC_H(j, k + 1) = CALC_H(j, k + 1) - sum * t2;
                    }
                    CALC_SYNC();
                }
            }
        }
        if (!conv) return false;
        if (l == i) {
            CALC_ONE { wr[i] = CALC_H(i, i); wi[i] = 0.0; }
        } else {                                               // l == i - 1: a 2 x 2 block
            double r1r, r1i, r2r, r2i;
            calc_lanv2(CALC_H(i - 1, i - 1), CALC_H(i - 1, i), CALC_H(i, i - 1), CALC_H(i, i), r1r, r1i, r2r, r2i);
            CALC_ONE { wr[i - 1] = r1r; wi[i - 1] = r1i; wr[i] = r2r; wi[i] = r2i; }
        }
        CALC_SYNC();
        kdefl = 0;
        i = l - 1;
    }
    return true;
}

// Per-wave LDS layout (doubles): the matrix (MP rows of stride MP + 1), then twelve vectors of 64 and the cosine table.
struct CalcLds {
    double *H, *v, *f, *c, *wr, *wi, *key, *srt, *rs, *nd, *wt, *cv, *tab;
};

template <int S>
CALC_FN CalcLds calc_lds(double *base, int mp) {
    CalcLds L;
    L.H = base;
    double *p = base + (size_t)mp * S;
    L.v = p; L.f = p + 64; L.c = p + 128; L.wr = p + 192; L.wi = p + 256; L.key = p + 320; L.srt = p + 384;
    L.rs = p + 448; L.nd = p + 512; L.wt = p + 576; L.cv = p + 640;   // cv: 128 (up to n + 1 candidates)
    L.tab = p + 768;
    return L;
}

// Real roots in [lo, hi] of the interpolant through L.f[0 .. n) (reference _roots_1d) -> L.rs[0 .. count), ascending.
// -1 when the colleague matrix is not finite or the QR iteration does not converge.
template <int S>
CALC_FN int calc_roots(const CalcLds &L, int n, double lo, double hi) {
    double *H = L.H;
    const int n4 = 4 * n;
    CALC_LANES(q, 0, n4) L.tab[q] = cos(M_PI * (double)q / (2.0 * (double)n));
    CALC_SYNC();
    CALC_LANES(k, 0, n) {                                      // c_k = (sum_j 2 cos(pi k (2j+1) / 2n) f_(n-1-j)) / n
        double s = 0.0;
        for (int j = 0; j < n; ++j) s += (2.0 * L.tab[(k * (2 * j + 1)) % n4]) * L.f[n - 1 - j];
        double ck = s / (double)n;
        if (k == 0) ck = ck / 2.0;
        L.c[k] = ck;
    }
    CALC_SYNC();
    int nc = 0;                                                // trailing exact zeros trimmed (as_series)
    for (int k = n - 1; k >= 0; --k)
        if (L.c[k] != 0.0) { nc = k + 1; break; }
    int m = 0;
    if (nc == 2) {
        CALC_ONE { L.wr[0] = -L.c[0] / L.c[1]; L.wi[0] = 0.0; }
        CALC_SYNC();
        m = 1;
    } else if (nc >= 3) {
        m = nc - 1;                  // the flipped colleague matrix F = chebcompanion(c)[::-1, ::-1], a lane per column
        const double sh = sqrt(0.5);
        CALC_LANES(j, 0, m) {                                  // tridiagonal part: 1/2, sqrt(1/2) at the flipped corner
            for (int r = 0; r < m; ++r) {
                double e = 0.0;
                if (r == j + 1 || j == r + 1) e = (r + j == 2 * m - 3) ? sh : 0.5;
                CALC_H(r, j) = e;
            }
        }
        CALC_SYNC();
        const double cm = L.c[m];
        CALC_LANES(r, 0, m) {       // mat[:, -1] -= (c[:-1] / c[-1]) * (scl / scl[-1]) * .5, flipped: column 0, row m-1-q
            const int q = m - 1 - r;
            const double scl = q == 0 ? 1.0 : sh;
            CALC_H(r, 0) = CALC_H(r, 0) - ((L.c[q] / cm) * (scl / sh)) * 0.5;
        }
        CALC_SYNC();
        for (int r = 0; r < m; ++r)
            if (!isfinite(CALC_H(r, 0))) return -1;            // NumPy's eigvals refuses infs and NaNs
        calc_balance<S>(H, m, L.key);
        calc_hessenberg<S>(H, m, L.srt);
        if (!calc_hqr<S>(H, m, L.wr, L.wi)) return -1;
    }
    const double tol = 1e-10;
    CALC_LANES(e, 0, m) {                                      // filter, snap to an end within tol of it, map
        const double re = L.wr[e];
        const bool ok = fabs(L.wi[e]) < tol && -1.0 - tol <= re && re <= 1.0 + tol;
        const double x = 0.5 * (lo + hi) + 0.5 * (hi - lo) * re;
        L.key[e] = !ok ? NAN : (re >= 1.0 - tol ? hi : (re <= tol - 1.0 ? lo : x));
    }
    CALC_SYNC();
    int cnt = 0;
    for (int e = 0; e < m; ++e) cnt += L.key[e] == L.key[e];
    CALC_LANES(e, 0, m) {                                      // rank sort (ties by index)
        const double x = L.key[e];
        if (x == x) {
            int r = 0;
            for (int q = 0; q < m; ++q) {
                const double y = L.key[q];
                r += (y == y) && (y < x || (y == x && q < e));
            }
            L.srt[r] = x;
        }
    }
    CALC_SYNC();
    const double dtol = 1e-10 * (hi - lo + 1.0);
    CALC_LANES(r, 0, cnt) {                                    // keep r when it exceeds r - 1 by more than dtol
        if (r == 0 || (L.srt[r] - L.srt[r - 1]) > dtol) {
            int pos = 0;
            for (int q = 0; q < r; ++q) pos += (q == 0 || (L.srt[q] - L.srt[q - 1]) > dtol);
            L.rs[pos] = L.srt[r];
        }
    }
    CALC_SYNC();
    int kept = 0;
    for (int r = 0; r < cnt; ++r) kept += (r == 0 || (L.srt[r] - L.srt[r - 1]) > dtol);
    return kept;
}

// One fibre, row `row` of the batch: roots into a.roots, or the first best candidate into a.val / a.loc.
template <int S>
CALC_FN void calc_row(const CalcArgs &a, long row, double *lds, int mp) {
    const CalcLds L = calc_lds<S>(lds, mp);
    const int n = a.n;
    const double *vals = a.vals + (size_t)row * n;
    CALC_LANES(j, 0, n) {
        L.v[j] = vals[j];
        L.nd[j] = a.nodes[j];
        L.wt[j] = a.wts[j];
    }
    CALC_SYNC();
    CALC_LANES(i, 0, n) {
        if (a.mode == 0) {
            L.f[i] = L.v[i];
        } else {                                               // D @ values
            const double *Di = a.diff + (size_t)i * n;
            double s = 0.0;
            for (int j = 0; j < n; ++j) s += Di[j] * L.v[j];
            L.f[i] = s;
        }
    }
    CALC_SYNC();
    const int cnt = calc_roots<S>(L, n, a.lo, a.hi);
    if (a.mode == 0) {
        double *out = a.roots + (size_t)row * a.W;
        CALC_LANES(q, 0, a.W) out[q] = q < cnt ? L.rs[q] : NAN;
        CALC_ONE a.counts[row] = cnt;
        return;
    }
    if (cnt < 0) {
        CALC_ONE { a.counts[row] = -1; a.val[row] = NAN; a.loc[row] = NAN; }
        return;
    }
    const int nc = cnt + 2;                                    // candidates [lo, critical..., hi]
    CALC_LANES(q, 0, nc) {
        const double x = q == 0 ? a.lo : (q == nc - 1 ? a.hi : L.rs[q - 1]);
        int exact = -1;
        double num = 0.0, den = 0.0;
        for (int j = 0; j < n; ++j) {
            const double dx = x - L.nd[j];
            if (fabs(dx) < 1e-14) {
                if (exact < 0) exact = j;
            } else {
                const double t = L.wt[j] / dx;
                num += t * L.v[j];
                den += t;
            }
        }
        L.cv[q] = exact >= 0 ? L.v[exact] : num / den;
    }
    CALC_SYNC();
    int best = 0;
    double bv = L.cv[0];
    for (int q = 1; q < nc && bv == bv; ++q) {
        const double x = L.cv[q];
        if (x != x || (a.mode == 1 ? x < bv : x > bv)) { best = q; bv = x; }
    }
    CALC_ONE {
        a.counts[row] = cnt;
        a.val[row] = bv;
        a.loc[row] = best == 0 ? a.lo : (best == nc - 1 ? a.hi : L.rs[best - 1]);
    }
}

#undef CALC_H

#if defined(__HIPCC__)
// One wave (workgroup) per fibre; MP bounds the colleague matrix (m <= MP), which sizes the LDS: 16 -> 10.1 KiB,
// 32 -> 16.3 KiB, 64 -> 40.5 KiB per workgroup, so several workgroups share a CU.
template <int MP>
__global__ __launch_bounds__(64) void k_cheb1d_calculus(CalcArgs a) {
    __shared__ double lds[MP * (MP + 1) + PCX_CALC_EXTRA];
    calc_row<MP + 1>(a, (long)blockIdx.x, lds, MP);
}

// Fibre points: row r, node j -> point r n + j with the fixed values of row r in every column but `dim` (in
// increasing column order) and the node value x_j, copied bit for bit, in column `dim`.
__global__ __launch_bounds__(256) void k_calc_expand(const double *__restrict__ fixed, long rows, int d, int dim, int n,
                                                     const double *__restrict__ nodes, double *__restrict__ pts) {
    const long total = rows * n * d;
    for (long idx = (long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long)gridDim.x * blockDim.x) {
        const int e = (int)(idx % d);
        const long p = idx / d;
        const int j = (int)(p % n);
        const long r = p / n;
        pts[idx] = e == dim ? nodes[j] : fixed[r * (d - 1) + (e < dim ? e : e - 1)];
    }
}
#endif
