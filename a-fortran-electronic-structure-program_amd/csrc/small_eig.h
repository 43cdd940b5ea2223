// small_eig.h -- eigenvalues and right eigenvectors of a small real general matrix on the host (the projected matrix of the EOM
// Davidson iteration, eom_so.h: n is at most a few hundred).  Householder reduction to Hessenberg form, the shifted double-step QR
// iteration on it with the transformations accumulated, and back-substitution for the vectors of the quasi-triangular form (the
// classical orthes / hqr2 pair: Wilkinson and Reinsch, Handbook for Automatic Computation II, 1971), and the partial-pivot LU solve of
// the projected linear systems of its linear mode (davidson_so.h).  Host code only; the library links no LAPACK.
#pragma once
#include <algorithm>
#include <cmath>
#include <numeric>
#include <vector>

namespace afesp {

namespace small_eig_detail {

inline void cdiv(double xr, double xi, double yr, double yi, double& cr, double& ci)
{
    double r, d;
    if (std::fabs(yr) > std::fabs(yi)) {
        r = yi / yr;
        d = yr + r * yi;
        cr = (xr + r * xi) / d;
        ci = (xi - r * xr) / d;
    } else {
        r = yr / yi;
        d = yi + r * yr;
        cr = (r * xr + xi) / d;
        ci = (r * xi - xr) / d;
    }
}

struct Work {
    int n;
    std::vector<double> h, v, d, e, ort;   // h, v row-major n x n
    double& H(int i, int j) { return h[(size_t)i * n + j]; }
    double& V(int i, int j) { return v[(size_t)i * n + j]; }
};

inline void orthes(Work& w)
{
    const int n = w.n, low = 0, high = n - 1;
    std::vector<double>& ort = w.ort;
    for (int m = low + 1; m <= high - 1; ++m) {
        double scale = 0.0;
        for (int i = m; i <= high; ++i) scale += std::fabs(w.H(i, m - 1));
        if (scale != 0.0) {
            double h = 0.0;
            for (int i = high; i >= m; --i) {
                ort[i] = w.H(i, m - 1) / scale;
                h += ort[i] * ort[i];
            }
            double g = std::sqrt(h);
            if (ort[m] > 0.0) g = -g;
            h -= ort[m] * g;
            ort[m] -= g;
            for (int j = m; j < n; ++j) {
                double f = 0.0;
                for (int i = high; i >= m; --i) f += ort[i] * w.H(i, j);
                f /= h;
                for (int i = m; i <= high; ++i) w.H(i, j) -= f * ort[i];
            }
            for (int i = 0; i <= high; ++i) {
                double f = 0.0;
                for (int j = high; j >= m; --j) f += ort[j] * w.H(i, j);
                f /= h;
                for (int j = m; j <= high; ++j) w.H(i, j) -= f * ort[j];
            }
            ort[m] = scale * ort[m];
            w.H(m, m - 1) = scale * g;
        }
    }
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < n; ++j) w.V(i, j) = i == j ? 1.0 : 0.0;
    for (int m = high - 1; m >= low + 1; --m) {
        if (w.H(m, m - 1) != 0.0) {
            for (int i = m + 1; i <= high; ++i) ort[i] = w.H(i, m - 1);
            for (int j = m; j <= high; ++j) {
                double g = 0.0;
                for (int i = m; i <= high; ++i) g += ort[i] * w.V(i, j);
                g = (g / ort[m]) / w.H(m, m - 1);   // (double division avoids a possible underflow)
                for (int i = m; i <= high; ++i) w.V(i, j) += g * ort[i];
            }
        }
    }
}

// -> false when a root needs more than 60 QR sweeps
inline bool hqr2(Work& w)
{
    const int nn = w.n, low = 0, high = nn - 1;
    int n = nn - 1;
    const double eps = std::ldexp(1.0, -52);
    double exshift = 0.0, p = 0, q = 0, r = 0, s = 0, z = 0, t, ww, x, y;
    std::vector<double>&d = w.d, &e = w.e;
    double norm = 0.0;
    for (int i = 0; i < nn; ++i)
        for (int j = std::max(i - 1, 0); j < nn; ++j) norm += std::fabs(w.H(i, j));
    int iter = 0;
    while (n >= low) {
        int l = n;
        while (l > low) {
            s = std::fabs(w.H(l - 1, l - 1)) + std::fabs(w.H(l, l));
            if (s == 0.0) s = norm;
            if (std::fabs(w.H(l, l - 1)) <= eps * s) break;   // (<=: a zero matrix deflates too)
            --l;
        }
        if (l == n) {   // one root
            w.H(n, n) += exshift;
            d[n] = w.H(n, n);
            e[n] = 0.0;
            --n;
            iter = 0;
        } else if (l == n - 1) {   // two roots
            ww = w.H(n, n - 1) * w.H(n - 1, n);
            p = (w.H(n - 1, n - 1) - w.H(n, n)) / 2.0;
            q = p * p + ww;
            z = std::sqrt(std::fabs(q));
            w.H(n, n) += exshift;
            w.H(n - 1, n - 1) += exshift;
            x = w.H(n, n);
            if (q >= 0.0) {   // a real pair
                z = p >= 0.0 ? p + z : p - z;
                d[n - 1] = x + z;
                d[n] = d[n - 1];
                if (z != 0.0) d[n] = x - ww / z;
                e[n - 1] = e[n] = 0.0;
                x = w.H(n, n - 1);
                s = std::fabs(x) + std::fabs(z);
                p = x / s;
                q = z / s;
                r = std::sqrt(p * p + q * q);
                p /= r;
                q /= r;
                for (int j = n - 1; j < nn; ++j) {
                    z = w.H(n - 1, j);
                    w.H(n - 1, j) = q * z + p * w.H(n, j);
                    w.H(n, j) = q * w.H(n, j) - p * z;
                }
                for (int i = 0; i <= n; ++i) {
                    z = w.H(i, n - 1);
                    w.H(i, n - 1) = q * z + p * w.H(i, n);
                    w.H(i, n) = q * w.H(i, n) - p * z;
                }
                for (int i = low; i <= high; ++i) {
                    z = w.V(i, n - 1);
                    w.V(i, n - 1) = q * z + p * w.V(i, n);
                    w.V(i, n) = q * w.V(i, n) - p * z;
                }
            } else {   // a complex pair
                d[n - 1] = x + p;
                d[n] = x + p;
                e[n - 1] = z;
                e[n] = -z;
            }
            n -= 2;
            iter = 0;
        } else {
            x = w.H(n, n);
            y = 0.0;
            ww = 0.0;
            if (l < n) {
                y = w.H(n - 1, n - 1);
                ww = w.H(n, n - 1) * w.H(n - 1, n);
            }
            if (iter == 10) {   // Wilkinson's exceptional shift
                exshift += x;
                for (int i = low; i <= n; ++i) w.H(i, i) -= x;
                s = std::fabs(w.H(n, n - 1)) + std::fabs(w.H(n - 1, n - 2));
                x = y = 0.75 * s;
                ww = -0.4375 * s * s;
            }
            if (iter == 30) {   // a second exceptional shift
                s = (y - x) / 2.0;
                s = s * s + ww;
                if (s > 0.0) {
                    s = std::sqrt(s);
                    if (y < x) s = -s;
                    s = x - ww / ((y - x) / 2.0 + s);
                    for (int i = low; i <= n; ++i) w.H(i, i) -= s;
                    exshift += s;
                    x = y = ww = 0.964;
                }
            }
            if (++iter > 60) return false;
            int m = n - 2;   // two consecutive small sub-diagonal elements
            while (m >= l) {
                z = w.H(m, m);
                r = x - z;
                s = y - z;
                p = (r * s - ww) / w.H(m + 1, m) + w.H(m, m + 1);
                q = w.H(m + 1, m + 1) - z - r - s;
                r = w.H(m + 2, m + 1);
                s = std::fabs(p) + std::fabs(q) + std::fabs(r);
                p /= s;
                q /= s;
                r /= s;
                if (m == l) break;
                if (std::fabs(w.H(m, m - 1)) * (std::fabs(q) + std::fabs(r)) <
                    eps * (std::fabs(p) * (std::fabs(w.H(m - 1, m - 1)) + std::fabs(z) + std::fabs(w.H(m + 1, m + 1)))))
                    break;
                --m;
            }
            for (int i = m + 2; i <= n; ++i) {
                w.H(i, i - 2) = 0.0;
                if (i > m + 2) w.H(i, i - 3) = 0.0;
            }
            for (int k = m; k <= n - 1; ++k) {   // the double QR step on rows l .. n and columns m .. n
                const bool notlast = k != n - 1;
                if (k != m) {
                    p = w.H(k, k - 1);
                    q = w.H(k + 1, k - 1);
                    r = notlast ? w.H(k + 2, k - 1) : 0.0;
                    x = std::fabs(p) + std::fabs(q) + std::fabs(r);
                    if (x == 0.0) continue;
                    p /= x;
                    q /= x;
                    r /= x;
                }
                s = std::sqrt(p * p + q * q + r * r);
                if (p < 0.0) s = -s;
                if (s != 0.0) {
                    if (k != m) w.H(k, k - 1) = -s * x;
                    else if (l != m) w.H(k, k - 1) = -w.H(k, k - 1);
                    p += s;
                    x = p / s;
                    y = q / s;
                    z = r / s;
                    q /= p;
                    r /= p;
                    for (int j = k; j < nn; ++j) {
                        p = w.H(k, j) + q * w.H(k + 1, j);
                        if (notlast) {
                            p += r * w.H(k + 2, j);
                            w.H(k + 2, j) -= p * z;
                        }
                        w.H(k, j) -= p * x;
                        w.H(k + 1, j) -= p * y;
                    }
                    for (int i = 0; i <= std::min(n, k + 3); ++i) {
                        p = x * w.H(i, k) + y * w.H(i, k + 1);
                        if (notlast) {
                            p += z * w.H(i, k + 2);
                            w.H(i, k + 2) -= p * r;
                        }
                        w.H(i, k) -= p;
                        w.H(i, k + 1) -= p * q;
                    }
                    for (int i = low; i <= high; ++i) {
                        p = x * w.V(i, k) + y * w.V(i, k + 1);
                        if (notlast) {
                            p += z * w.V(i, k + 2);
                            w.V(i, k + 2) -= p * r;
                        }
                        w.V(i, k) -= p;
                        w.V(i, k + 1) -= p * q;
                    }
                }
            }
        }
    }
    if (norm == 0.0) return true;
    // back-substitution: the vectors of the quasi-triangular form
    for (n = nn - 1; n >= 0; --n) {
        p = d[n];
        q = e[n];
        if (q == 0.0) {   // a real vector
            int l = n;
            w.H(n, n) = 1.0;
            for (int i = n - 1; i >= 0; --i) {
                ww = w.H(i, i) - p;
                r = 0.0;
                for (int j = l; j <= n; ++j) r += w.H(i, j) * w.H(j, n);
                if (e[i] < 0.0) {
                    z = ww;
                    s = r;
                } else {
                    l = i;
                    if (e[i] == 0.0) {
                        w.H(i, n) = ww != 0.0 ? -r / ww : -r / (eps * norm);
                    } else {   // two real equations
                        x = w.H(i, i + 1);
                        y = w.H(i + 1, i);
                        q = (d[i] - p) * (d[i] - p) + e[i] * e[i];
                        t = (x * s - z * r) / q;
                        w.H(i, n) = t;
                        w.H(i + 1, n) = std::fabs(x) > std::fabs(z) ? (-r - ww * t) / x : (-s - y * t) / z;
                    }
                    t = std::fabs(w.H(i, n));   // overflow control
                    if ((eps * t) * t > 1.0)
                        for (int j = i; j <= n; ++j) w.H(j, n) /= t;
                }
            }
        } else if (q < 0.0) {   // a complex vector: columns n - 1 (real part) and n (imaginary part) of the root d[n-1] + i e[n-1]
            int l = n - 1;
            double cr, ci, ra, sa, vr, vi;
            if (std::fabs(w.H(n, n - 1)) > std::fabs(w.H(n - 1, n))) {
                w.H(n - 1, n - 1) = q / w.H(n, n - 1);
                w.H(n - 1, n) = -(w.H(n, n) - p) / w.H(n, n - 1);
            } else {
                cdiv(0.0, -w.H(n - 1, n), w.H(n - 1, n - 1) - p, q, cr, ci);
                w.H(n - 1, n - 1) = cr;
                w.H(n - 1, n) = ci;
            }
            w.H(n, n - 1) = 0.0;
            w.H(n, n) = 1.0;
            for (int i = n - 2; i >= 0; --i) {
                ra = 0.0;
                sa = 0.0;
                for (int j = l; j <= n; ++j) {
                    ra += w.H(i, j) * w.H(j, n - 1);
                    sa += w.H(i, j) * w.H(j, n);
                }
                ww = w.H(i, i) - p;
                if (e[i] < 0.0) {
                    z = ww;
                    r = ra;
                    s = sa;
                } else {
                    l = i;
                    if (e[i] == 0.0) {
                        cdiv(-ra, -sa, ww, q, cr, ci);
                        w.H(i, n - 1) = cr;
                        w.H(i, n) = ci;
                    } else {   // two complex equations
                        x = w.H(i, i + 1);
                        y = w.H(i + 1, i);
                        vr = (d[i] - p) * (d[i] - p) + e[i] * e[i] - q * q;
                        vi = (d[i] - p) * 2.0 * q;
                        if (vr == 0.0 && vi == 0.0)
                            vr = eps * norm * (std::fabs(ww) + std::fabs(q) + std::fabs(x) + std::fabs(y) + std::fabs(z));
                        cdiv(x * r - z * ra + q * sa, x * s - z * sa - q * ra, vr, vi, cr, ci);
                        w.H(i, n - 1) = cr;
                        w.H(i, n) = ci;
                        if (std::fabs(x) > std::fabs(z) + std::fabs(q)) {
                            w.H(i + 1, n - 1) = (-ra - ww * w.H(i, n - 1) + q * w.H(i, n)) / x;
                            w.H(i + 1, n) = (-sa - ww * w.H(i, n) - q * w.H(i, n - 1)) / x;
                        } else {
                            cdiv(-r - y * w.H(i, n - 1), -s - y * w.H(i, n), z, q, cr, ci);
                            w.H(i + 1, n - 1) = cr;
                            w.H(i + 1, n) = ci;
                        }
                    }
                    t = std::max(std::fabs(w.H(i, n - 1)), std::fabs(w.H(i, n)));   // overflow control
                    if ((eps * t) * t > 1.0)
                        for (int j = i; j <= n; ++j) {
                            w.H(j, n - 1) /= t;
                            w.H(j, n) /= t;
                        }
                }
            }
        }
    }
    // back to the vectors of the original matrix
    for (int j = nn - 1; j >= low; --j)
        for (int i = low; i <= high; ++i) {
            z = 0.0;
            for (int k = low; k <= std::min(j, high); ++k) z += w.V(i, k) * w.H(k, j);
            w.V(i, j) = z;
        }
    return true;
}

}  // namespace small_eig_detail

// Eigenvalues wr + i wi and right eigenvectors of the real n x n matrix a (column-major, leading dimension lda; not changed), ordered by
// real part with ties broken by the order in which the QR iteration deflated them -- a complex pair stays adjacent, the root with
// wi > 0 first.  vr is n x n column-major: column k belongs to root k and has unit Euclidean norm; for a complex pair the column of
// the root with wi > 0 holds the real part of its vector and the next column the imaginary part (together of unit norm).
// -> 0, 1 on a bad argument, 2 when the QR iteration does not converge.
inline int eig_general(int n, const double* a, int lda, double* wr, double* wi, double* vr)
{
    using namespace small_eig_detail;
    if (n < 1 || !a || lda < n || !wr || !wi || !vr) return 1;
    Work w;
    w.n = n;
    w.h.resize((size_t)n * n);
    w.v.resize((size_t)n * n);
    w.d.assign(n, 0.0);
    w.e.assign(n, 0.0);
    w.ort.assign(n, 0.0);
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < n; ++j) {
            const double x = a[i + (size_t)lda * j];
            if (!std::isfinite(x)) return 1;
            w.H(i, j) = x;
        }
    orthes(w);
    if (!hqr2(w)) return 2;
    std::vector<int> order(n);
    std::iota(order.begin(), order.end(), 0);
    std::stable_sort(order.begin(), order.end(), [&](int p, int q) { return w.d[p] < w.d[q]; });
    for (int k = 0; k < n; ++k) {
        const int c = order[k];
        wr[k] = w.d[c];
        wi[k] = w.e[c];
        // the norm of the vector this column is (part of): a real one alone, a pair's two columns together
        const int c0 = w.e[c] < 0.0 ? c - 1 : c, c1 = w.e[c] > 0.0 ? c + 1 : c;
        double s = 0.0;
        for (int i = 0; i < n; ++i)
            for (int cc = c0; cc <= c1; ++cc) s += w.V(i, cc) * w.V(i, cc);
        s = s > 0.0 ? 1.0 / std::sqrt(s) : 0.0;
        for (int i = 0; i < n; ++i) vr[i + (size_t)n * k] = w.V(i, c) * s;
    }
    return 0;
}

// a x = b for nrhs right-hand sides by LU with partial pivoting, in place: a (n x n, column-major, leading dimension lda) is overwritten
// by its factors and b (n x nrhs, leading dimension ldb) by the solutions.  -> 0, 1 on a bad argument, 2 when a pivot is not above
// `floor` in magnitude (floor = 0: an exactly singular matrix) -- a and b then hold a partial elimination.
inline int lu_solve(int n, double* a, int lda, int nrhs, double* b, int ldb, double floor)
{
    if (n < 1 || nrhs < 0 || !a || lda < n || (nrhs > 0 && (!b || ldb < n)) || !(floor >= 0.0)) return 1;
    for (int k = 0; k < n; ++k) {
        int p = k;
        for (int i = k + 1; i < n; ++i)
            if (std::fabs(a[i + (size_t)lda * k]) > std::fabs(a[p + (size_t)lda * k])) p = i;
        if (!(std::fabs(a[p + (size_t)lda * k]) > floor)) return 2;
        if (p != k) {
            for (int j = 0; j < n; ++j) std::swap(a[k + (size_t)lda * j], a[p + (size_t)lda * j]);
            for (int j = 0; j < nrhs; ++j) std::swap(b[k + (size_t)ldb * j], b[p + (size_t)ldb * j]);
        }
        const double piv = a[k + (size_t)lda * k];
        for (int i = k + 1; i < n; ++i) {
            const double l = a[i + (size_t)lda * k] / piv;
            if (l == 0.0) continue;
            a[i + (size_t)lda * k] = l;
            for (int j = k + 1; j < n; ++j) a[i + (size_t)lda * j] -= l * a[k + (size_t)lda * j];
            for (int j = 0; j < nrhs; ++j) b[i + (size_t)ldb * j] -= l * b[k + (size_t)ldb * j];
        }
    }
    for (int j = 0; j < nrhs; ++j)
        for (int k = n - 1; k >= 0; --k) {
            double x = b[k + (size_t)ldb * j];
            for (int i = k + 1; i < n; ++i) x -= a[k + (size_t)lda * i] * b[i + (size_t)ldb * j];
            b[k + (size_t)ldb * j] = x / a[k + (size_t)lda * k];
        }
    return 0;
}

// lu_solve for a complex matrix and complex right-hand sides: a and b hold (re, im) pairs, element (i, j) of a at a[2 (i + lda j)] and
// a[2 (i + lda j) + 1], b likewise with ldb.  Pivoting is on |pivot| (hypot); -> 2 when |pivot| is not above `floor`.  The products and
// quotients are written out on the parts -- (a + ib)(c + id) = (ac - bd) + i(ad + bc), (a + ib) / (c + id) = [(ac + bd) + i(bc - ad)] /
// (c^2 + d^2) -- so that a system whose imaginary parts are all zero is solved with imaginary parts that are exactly zero.
inline int lu_solve_complex(int n, double* a, int lda, int nrhs, double* b, int ldb, double floor)
{
    if (n < 1 || nrhs < 0 || !a || lda < n || (nrhs > 0 && (!b || ldb < n)) || !(floor >= 0.0)) return 1;
    auto A = [&](int i, int j) { return a + 2 * (i + (size_t)lda * j); };
    auto Bv = [&](int i, int j) { return b + 2 * (i + (size_t)ldb * j); };
    auto mag = [](const double* z) { return std::hypot(z[0], z[1]); };
    // z -= l w
    auto submul = [](double* z, const double* l, const double* w) {
        z[0] -= l[0] * w[0] - l[1] * w[1];
        z[1] -= l[0] * w[1] + l[1] * w[0];
    };
    auto div = [](const double* x, const double* y, double* q) {
        const double m2 = y[0] * y[0] + y[1] * y[1];
        const double re = (x[0] * y[0] + x[1] * y[1]) / m2, im = (x[1] * y[0] - x[0] * y[1]) / m2;
        q[0] = re;
        q[1] = im;
    };
    for (int k = 0; k < n; ++k) {
        int p = k;
        for (int i = k + 1; i < n; ++i)
            if (mag(A(i, k)) > mag(A(p, k))) p = i;
        if (!(mag(A(p, k)) > floor)) return 2;
        if (p != k) {
            for (int j = 0; j < n; ++j) {
                std::swap(A(k, j)[0], A(p, j)[0]);
                std::swap(A(k, j)[1], A(p, j)[1]);
            }
            for (int j = 0; j < nrhs; ++j) {
                std::swap(Bv(k, j)[0], Bv(p, j)[0]);
                std::swap(Bv(k, j)[1], Bv(p, j)[1]);
            }
        }
        for (int i = k + 1; i < n; ++i) {
            double l[2];
            div(A(i, k), A(k, k), l);
            if (l[0] == 0.0 && l[1] == 0.0) continue;
            A(i, k)[0] = l[0];
            A(i, k)[1] = l[1];
            for (int j = k + 1; j < n; ++j) submul(A(i, j), l, A(k, j));
            for (int j = 0; j < nrhs; ++j) submul(Bv(i, j), l, Bv(k, j));
        }
    }
    for (int j = 0; j < nrhs; ++j)
        for (int k = n - 1; k >= 0; --k) {
            double x[2] = {Bv(k, j)[0], Bv(k, j)[1]};
            for (int i = k + 1; i < n; ++i) submul(x, A(k, i), Bv(i, j));
            div(x, A(k, k), Bv(k, j));
        }
    return 0;
}

}  // namespace afesp
