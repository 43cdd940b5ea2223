// small_eig_check.cpp -- stand-alone check of csrc/small_eig.h (host code only; meant to be built with -fsanitize=address,undefined):
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined tools/small_eig_check.cpp -o small_eig_check && ./small_eig_check
// Random matrices of n = 1 .. 96, a block matrix with known complex pairs, a symmetric one and a nearly defective one: every root's
// residual |A v - w v| (complex arithmetic for a pair) stays below 1e-10 |A|, and the trace equals the sum of the roots.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../a-fortran-electronic-structure-program_amd/csrc/small_eig.h"

static uint64_t state = 0x9E3779B97F4A7C15ull;
static double uniform()
{
    state = state * 6364136223846793005ull + 1442695040888963407ull;
    return (double)(state >> 11) * (1.0 / 9007199254740992.0) * 2.0 - 1.0;
}

static int check(const char* what, int n, const std::vector<double>& a)
{
    std::vector<double> wr(n), wi(n), vr((size_t)n * n);
    const int rc = afesp::eig_general(n, a.data(), n, wr.data(), wi.data(), vr.data());
    if (rc) {
        printf("%s n=%d: status %d\n", what, n, rc);
        return 1;
    }
    double norm = 0.0, trace = 0.0, sum = 0.0, worst = 0.0;
    for (double x : a) norm += x * x;
    norm = std::sqrt(norm);
    for (int i = 0; i < n; ++i) trace += a[i + (size_t)n * i], sum += wr[i];
    int bad = 0;
    for (int k = 0; k < n; ++k) {
        if (k && wr[k] < wr[k - 1]) bad = 1;
        const double* re = wi[k] < 0.0 ? &vr[(size_t)n * (k - 1)] : &vr[(size_t)n * k];
        const double* im = wi[k] > 0.0 ? &vr[(size_t)n * (k + 1)] : (wi[k] < 0.0 ? &vr[(size_t)n * k] : nullptr);
        const double sgn = wi[k] < 0.0 ? -1.0 : 1.0;   // the conjugate root takes the conjugate vector
        double res = 0.0;
        for (int i = 0; i < n; ++i) {
            double ar = 0.0, ai = 0.0;
            for (int j = 0; j < n; ++j) {
                ar += a[i + (size_t)n * j] * re[j];
                if (im) ai += a[i + (size_t)n * j] * sgn * im[j];
            }
            const double vi = im ? sgn * im[i] : 0.0;
            const double dr = ar - (wr[k] * re[i] - wi[k] * vi), di = ai - (wr[k] * vi + wi[k] * re[i]);
            res += dr * dr + di * di;
        }
        worst = std::max(worst, std::sqrt(res));
    }
    const double bound = 1e-10 * std::max(norm, 1e-300);
    if (worst > bound || std::fabs(trace - sum) > 1e-10 * std::max(1.0, norm)) bad = 1;
    printf("%-16s n=%3d  worst residual %.2e  (bound %.2e)  trace - sum %.1e  %s\n", what, n, worst, bound, trace - sum, bad ? "FAILED" : "ok");
    return bad;
}

int main()
{
    int bad = 0;
    for (int n : {1, 2, 3, 5, 8, 24, 64, 96}) {
        std::vector<double> a((size_t)n * n);
        for (double& x : a) x = uniform();
        bad += check("random", n, a);
    }
    {   // rotation blocks hidden by a similarity: roots 1 +- 2i, -0.5 +- 0.25i, 3
        const int n = 5;
        std::vector<double> d((size_t)n * n, 0.0), s((size_t)n * n), a((size_t)n * n, 0.0);
        d[0 + n * 0] = 1.0; d[0 + n * 1] = 2.0; d[1 + n * 0] = -2.0; d[1 + n * 1] = 1.0;
        d[2 + n * 2] = -0.5; d[2 + n * 3] = 0.25; d[3 + n * 2] = -0.25; d[3 + n * 3] = -0.5;
        d[4 + n * 4] = 3.0;
        for (int i = 0; i < n; ++i)
            for (int j = 0; j < n; ++j) s[i + n * j] = (i == j ? 2.0 : 0.0) + 0.3 * uniform();
        // a = s d s^-1 is checked through its residuals alone; here a = s d (another general matrix with complex roots)
        for (int i = 0; i < n; ++i)
            for (int j = 0; j < n; ++j)
                for (int k = 0; k < n; ++k) a[i + n * j] += s[i + n * k] * d[k + n * j];
        bad += check("complex pairs", n, d);
        bad += check("complex mixed", n, a);
    }
    {
        const int n = 12;
        std::vector<double> a((size_t)n * n);
        for (int i = 0; i < n; ++i)
            for (int j = 0; j <= i; ++j) a[i + n * j] = a[j + n * i] = uniform();
        bad += check("symmetric", n, a);
    }
    {   // a Jordan block perturbed at 1e-10: the roots split by 1e-10^(1/4), the residuals stay small
        const int n = 4;
        std::vector<double> a((size_t)n * n, 0.0);
        for (int i = 0; i < n; ++i) a[i + n * i] = 1.0;
        for (int i = 0; i + 1 < n; ++i) a[i + n * (i + 1)] = 1.0;
        a[(n - 1) + n * 0] = 1e-10;
        bad += check("nearly defective", n, a);
    }
    {
        std::vector<double> a(9, 0.0);
        bad += check("zero", 3, a);
    }
    printf(bad ? "FAILED\n" : "all ok\n");
    return bad ? 1 : 0;
}
