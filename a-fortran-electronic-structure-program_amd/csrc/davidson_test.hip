// davidson_test.hip -- the test entry of davidson_test.h: a Davidson state whose operator is the data A = diag(d) + U V^T.  The sigma
// build is two plain kernels around the unit's own fixed-order reduction (davidson_reduce_blocks / davidson_reduce_final), so a run gives
// the same bits every time; tests/test_gpu_davidson.py checks it element by element and trusts nothing of it.
#include "davidson_test.h"
#include "device_util.h"

#include <cstring>

namespace afesp {
namespace {

constexpr int DT_MAXR = 64;

// partial[j nblk + blk] = the block's share of <V_j, x>  (block (blk, j))
__global__ void davidson_test_vtx_kernel(double* partial, const double* V, const double* x, int64_t nvec)
{
    __shared__ double sm[4];
    const double* v = V + nvec * blockIdx.y;
    double acc[1] = {0.0};
    GRID_STRIDE(e, nvec) acc[0] += v[e] * x[e];
    block_sum<1>(acc, sm);
    if (threadIdx.x == 0) partial[(int64_t)blockIdx.y * gridDim.x + blockIdx.x] = acc[0];
}

// s = d o x + sum_j U_j t_j
__global__ void davidson_test_apply_kernel(double* s, const double* d, const double* U, const double* t, const double* x, int r, int64_t nvec)
{
    GRID_STRIDE(e, nvec)
    {
        double a = d[e] * x[e];
        for (int j = 0; j < r; ++j) a = __fma_rn(U[nvec * j + e], t[j], a);
        s[e] = a;
    }
}

void upload(Context& cx, double* dev, const double* host, int64_t n)
{
    if (n > 0) AFESP_HIP(hipMemcpyAsync(dev, host, sizeof(double) * n, hipMemcpyHostToDevice, cx.stream));
}

int64_t give(double* out, int64_t capacity, const double* src, int64_t n, const char* what)
{
    if (n > capacity) throw Error(1, std::string("afesp_test_davidson_fetch: capacity is below the ") + std::to_string(n) + " doubles of " + what);
    if (n > 0) memcpy(out, src, sizeof(double) * n);
    return n;
}

}  // namespace

DavidsonTest& davidson_test_need(Context& cx, const char* who)
{
    if (!cx.dav_test) throw Error(1, std::string(who) + ": no Davidson test state (call afesp_test_davidson_create first)");
    return *cx.dav_test;
}

void davidson_test_destroy(Context& cx)
{
    DavidsonTest* T = cx.dav_test;
    if (!T) return;
    davidson_free(cx, T->d);
    double* bufs[] = {T->dd, T->U, T->V, T->vpart, T->vt, T->rhs};
    for (double* b : bufs) cx.release(b);
    delete T;
    cx.dav_test = nullptr;
}

void davidson_test_create(Context& cx, int64_t n1, int64_t nvec, double w2, int follow, int nroots, int max_space, int r, const double* d,
                          const double* U, const double* V, const double* diag)
{
    const char* who = "afesp_test_davidson_create";
    if (nvec < 1 || n1 < 0 || n1 > nvec || !(w2 > 0.0)) throw Error(1, std::string(who) + ": needs nvec >= 1, 0 <= n1 <= nvec and w2 > 0");
    if (nroots < 1 || nroots > nvec) throw Error(1, std::string(who) + ": needs 1 <= nroots <= nvec");
    if (max_space < 2 * nroots || max_space > 4096) throw Error(1, std::string(who) + ": needs 2 nroots <= max_space <= 4096");
    if (r < 0 || r > DT_MAXR || !d || !diag || (r > 0 && (!U || !V))) throw Error(1, std::string(who) + ": needs 0 <= r <= 64 and d, diag (and U, V)");
    davidson_test_destroy(cx);
    DavidsonTest* T = cx.dav_test = new DavidsonTest();
    try {
        T->r = r;
        T->dd = cx.alloc(nvec);
        T->U = cx.alloc(nvec * r);
        T->V = cx.alloc(nvec * r);
        T->vpart = cx.alloc((int64_t)std::max(r, 1) * davidson_reduce_blocks(nvec));
        T->vt = cx.alloc(std::max(r, 1));
        upload(cx, T->dd, d, nvec);
        upload(cx, T->U, U, nvec * r);
        upload(cx, T->V, V, nvec * r);
        davidson_alloc(cx, T->d, n1, nvec, w2, follow != 0, nroots, max_space, [&](double* dg) { upload(cx, dg, diag, nvec); });
        cx.sync();
    } catch (...) {
        davidson_test_destroy(cx);
        throw;
    }
}

void davidson_test_sigma(Context& cx, DavidsonTest& T, const double* x, double* s)
{
    const int64_t nvec = T.d.nvec;
    const int nblk = davidson_reduce_blocks(nvec);
    if (T.r > 0) {
        LAUNCH(davidson_test_vtx_kernel, dim3(nblk, T.r), T.vpart, T.V, x, nvec);
        davidson_reduce_final(cx, T.vt, T.vpart, T.r, nblk);
    }
    LAUNCH(davidson_test_apply_kernel, grid_for(nvec), s, T.dd, T.U, T.vt, x, T.r, nvec);
}

void davidson_test_set_guess(Context& cx, int k, const double* x1, const double* x2)
{
    DavidsonTest& T = davidson_test_need(cx, "afesp_test_davidson_set_guess");
    davidson_set_pending_from_host(cx, T.d, "afesp_test_davidson_", k, x1, x2);
    T.linear = false;
}

int davidson_test_iterate(Context& cx, double tol)
{
    DavidsonTest& T = davidson_test_need(cx, "afesp_test_davidson_iterate");
    if (!(tol > 0.0)) throw Error(1, "afesp_test_davidson_iterate: tol must be positive");
    if (T.linear) throw Error(1, "afesp_test_davidson_iterate: the state is in linear mode (call afesp_test_davidson_set_guess first)");
    T.y_nb = -1;
    const int conv = davidson_iterate(cx, T.d, "afesp_test_davidson_", tol, [&](const double* x, double* s) { davidson_test_sigma(cx, T, x, s); });
    T.y_nb = T.d.nb;
    return conv;
}

void davidson_test_linear_start(Context& cx, int nrhs, const double* rhs_host, const double* shifts)
{
    DavidsonTest& T = davidson_test_need(cx, "afesp_test_davidson_linear_start");
    if (nrhs < 1 || nrhs > T.d.nroots || !rhs_host || !shifts)
        throw Error(1, "afesp_test_davidson_linear_start: needs 1 <= nrhs <= nroots right-hand sides and nroots shifts");
    cx.release(T.rhs);
    T.rhs = nullptr;
    T.d.rhs = nullptr;
    T.rhs = cx.alloc(T.d.nvec * nrhs);
    upload(cx, T.rhs, rhs_host, T.d.nvec * nrhs);
    davidson_linear_start(cx, T.d, T.rhs, nrhs, shifts);
    T.linear = true;
}

void davidson_test_linear_start_complex(Context& cx, int nrhs, const double* rhs_host, const double* shift_re, const double* shift_im)
{
    const char* who = "afesp_test_davidson_linear_start_complex";
    DavidsonTest& T = davidson_test_need(cx, who);
    if (nrhs < 1 || nrhs > T.d.nroots || !rhs_host || !shift_re || !shift_im)
        throw Error(1, std::string(who) + ": needs 1 <= nrhs <= nroots right-hand sides and nroots complex shifts");
    if (T.d.max_space < 4 * T.d.nroots || T.d.nroots > 64) throw Error(1, std::string(who) + ": needs 4 nroots <= max_space and nroots <= 64");
    if (!T.d.wide) {   // the state again with two columns per system, the diagonal carried over
        Davidson wide;
        try {
            davidson_alloc(cx, wide, T.d.n1, T.d.nvec, T.d.w2, T.d.follow, T.d.nroots, T.d.max_space, [&](double* dg) { k_copy(cx, dg, T.d.diag, T.d.nvec); }, true);
            cx.sync();
        } catch (...) {
            davidson_free(cx, wide);
            throw;
        }
        davidson_free(cx, T.d);
        T.d = wide;
    }
    cx.release(T.rhs);
    T.rhs = nullptr;
    T.d.rhs = nullptr;
    T.rhs = cx.alloc(T.d.nvec * nrhs);
    upload(cx, T.rhs, rhs_host, T.d.nvec * nrhs);
    davidson_linear_start_complex(cx, T.d, T.rhs, nrhs, shift_re, shift_im);
    T.linear = true;
}

int davidson_test_linear_iterate(Context& cx, double tol)
{
    DavidsonTest& T = davidson_test_need(cx, "afesp_test_davidson_linear_iterate");
    if (!(tol > 0.0)) throw Error(1, "afesp_test_davidson_linear_iterate: tol must be positive");
    if (!T.linear) throw Error(1, "afesp_test_davidson_linear_iterate: no right-hand sides (call afesp_test_davidson_linear_start first)");
    T.y_nb = -1;   // (a throw at a pole leaves a larger basis and the coefficients of the step before: not to be fetched)
    const int conv = davidson_linear_iterate(cx, T.d, "afesp_test_davidson_linear_", tol, [&](const double* x, double* s) { davidson_test_sigma(cx, T, x, s); });
    T.y_nb = T.d.nb;
    return conv;
}

void davidson_test_get_vector(Context& cx, int k, double* x1, double* x2)
{
    DavidsonTest& T = davidson_test_need(cx, "afesp_test_davidson_get_vector");
    davidson_get_vector(cx, T.d, "afesp_test_davidson_", k, x1, x2);
}

int64_t davidson_test_fetch(Context& cx, const char* what, double* out, int64_t capacity)
{
    DavidsonTest& T = davidson_test_need(cx, "afesp_test_davidson_fetch");
    Davidson& E = T.d;
    if (!what || !out || capacity < 0) throw Error(1, "afesp_test_davidson_fetch: NULL argument");
    const std::string w = what;
    const int nb = E.nb, ms = E.max_space;
    const int nr = T.linear ? E.nroots : std::min(E.nroots, nb);
    const int ncol = E.cplx ? 2 : 1;   // complex linear mode: real and imaginary columns
    const double* dev = nullptr;
    int64_t n = 0;
    if (w == "B") dev = E.B, n = E.nvec * nb;
    else if (w == "S") dev = E.S, n = E.nvec * nb;
    else if (w == "pend") dev = E.pend, n = E.nvec * E.npend;
    else if (w == "x") dev = E.x, n = E.nvec * E.nroots * ncol;
    else if (w == "sx") dev = E.sx, n = E.nvec * E.nroots * ncol;
    else if (w == "corr") dev = E.corr, n = E.nvec * E.nroots * ncol;
    else if (w == "diag") dev = E.diag, n = E.nvec;
    else if (w == "y") {
        if (!E.ritz || T.y_nb != nb) throw Error(1, "afesp_test_davidson_fetch: no coefficients: no step has finished on the present basis");
        dev = E.coef, n = ((int64_t)nb * nr + nr) * ncol;
    }
    if (dev) {
        if (n > capacity) throw Error(1, "afesp_test_davidson_fetch: capacity is below the " + std::to_string(n) + " doubles of " + w);
        if (n > 0) AFESP_HIP(hipMemcpyAsync(out, dev, sizeof(double) * n, hipMemcpyDeviceToHost, cx.stream));
        cx.sync();
        return n;
    }
    if (w == "G") {
        std::vector<double> g((size_t)nb * nb);
        for (int q = 0; q < nb; ++q)
            for (int p = 0; p < nb; ++p) g[p + (size_t)nb * q] = E.G[p + (size_t)ms * q];
        return give(out, capacity, g.data(), (int64_t)g.size(), what);
    }
    if (w == "prhs") {
        if (!T.linear) throw Error(1, "afesp_test_davidson_fetch: prhs belongs to the linear mode");
        std::vector<double> g((size_t)nb * E.nrhs);
        for (int a = 0; a < E.nrhs; ++a)
            for (int p = 0; p < nb; ++p) g[p + (size_t)nb * a] = E.prhs[p + (size_t)ms * a];
        return give(out, capacity, g.data(), (int64_t)g.size(), what);
    }
    if (w == "target") return give(out, capacity, E.target.data(), (int64_t)E.target.size(), what);
    if (w == "counts") {
        const double c[4] = {(double)E.nsigma, (double)E.ncollapse, (double)E.nb, (double)E.npend};
        return give(out, capacity, c, 4, what);
    }
    throw Error(1, "afesp_test_davidson_fetch: what is one of B, S, pend, x, sx, corr, diag, G, prhs, y, target, counts");
}

}  // namespace afesp
