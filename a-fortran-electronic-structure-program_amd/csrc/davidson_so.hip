// davidson_so.hip -- the block Davidson iteration of davidson_so.h.  Launches are plain call-by-call ones.  Every
// reduction is block partials on a grid fixed by the vector length, then an ordered final sum: the same input gives the same bits on
// every run.
#include "davidson_so.h"
#include "device_util.h"
#include "small_eig.h"

#include <cmath>
#include <numeric>

namespace afesp {
namespace {

constexpr int DAV_MAXBLK = 128;   // blocks of a reduction (at most TB: davidson_final_kernel sums them in one block)
constexpr int DAV_RCHUNK = 8;     // roots one launch of the Ritz pass forms
constexpr double DAV_DROP = 1e-10, DAV_CLAMP = 1e-4;
constexpr double DAV_POLE = 1e-10;   // linear mode: a pivot below this times max(|G|_max, |shift|) is a pole

// The Gram panel of one vector pair (bq, sq) against ncol stored columns, in one launch -- block (blk, p):
//   p < ncol:  <b_p, sq>, <s_p, bq>, <b_p, bq>        p = ncol:  <bq, sq>, the same again, <bq, bq>
// with the weights 1 on the first n1 elements and w2 behind them; partial[(q (ncol + 1) + p) nblk + blk], q = 0, 1, 2.  sq null: the
// overlaps alone (q = 2; the others are written as zero).
__global__ void davidson_panel_kernel(double* partial, const double* B, const double* S, int64_t stride, int ncol, const double* bq,
                                      const double* sq, int64_t nvec, int64_t n1, double w2)
{
    __shared__ double sm[3 * 4];
    const int p = blockIdx.y, nblk = gridDim.x;
    const double* bp = p < ncol ? B + stride * p : bq;
    const double* sp = sq ? (p < ncol ? S + stride * p : sq) : nullptr;
    double acc[3] = {0.0, 0.0, 0.0};
    GRID_STRIDE(x, nvec)
    {
        const double w = x < n1 ? 1.0 : w2, b = bp[x], q = bq[x];
        if (sp) {
            acc[0] += w * b * sq[x];
            acc[1] += w * sp[x] * q;
        }
        acc[2] += w * b * q;
    }
    block_sum<3>(acc, sm);
    if (threadIdx.x == 0)
        for (int q = 0; q < 3; ++q) partial[((int64_t)q * (ncol + 1) + p) * nblk + blockIdx.x] = acc[q];
}

// out[b] = the sum of partial[b nblk .. (b + 1) nblk) in a fixed order (nblk <= TB)
__global__ void davidson_final_kernel(double* out, const double* partial, int nblk)
{
    __shared__ double red[TB];
    block_tree_sum((int)threadIdx.x < nblk ? partial[(int64_t)blockIdx.x * nblk + threadIdx.x] : 0.0, red);
    if (threadIdx.x == 0) out[blockIdx.x] = red[0];
}

// one projection pass: x -= sum_p coef[p] b_p, and the companion sx -= sum_p coef[p] s_p where given
__global__ void davidson_project_kernel(double* x, double* sx, const double* B, const double* S, int64_t stride, int ncol, const double* coef,
                                        int64_t nvec)
{
    GRID_STRIDE(e, nvec)
    {
        double a = x[e], sa = sx ? sx[e] : 0.0;
        for (int p = 0; p < ncol; ++p) {
            const double c = coef[p];
            a = __fma_rn(-c, B[stride * p + e], a);
            if (sx) sa = __fma_rn(-c, S[stride * p + e], sa);
        }
        x[e] = a;
        if (sx) sx[e] = sa;
    }
}

__global__ void davidson_scale_kernel(double* dst, const double* src, double* dst2, const double* src2, double scale, int64_t nvec)
{
    GRID_STRIDE(e, nvec)
    {
        dst[e] = __dmul_rn(scale, src[e]);
        if (src2) dst2[e] = __dmul_rn(scale, src2[e]);
    }
}

// The Ritz pass for the roots k0 .. k0 + nr (nr <= DAV_RCHUNK): every stored b_p and sigma_p is read once and gives
//   x_k = sum_p y(p,k) b_p,  sx_k = sum_p y(p,k) sigma_p,  rho_k = sx_k - omega_k x_k,  corr_k = rho_k / (omega_k - diag)
// (|omega_k - diag| clamped below at DAV_CLAMP, keeping its sign) and the block partials of <rho_k, rho_k> at
// partial[(k0 + k) nblk + blk].  y: nb x nroots column-major.  rhs non-null: the fused pass of the linear mode -- omega holds the shifts
// and rho_k = rhs_(k % nrhs) + (sx_k - omega_k x_k); rhs null is the Ritz pass, with the arithmetic it always had.
__global__ void davidson_ritz_kernel(double* X, double* SX, double* corr, double* partial, const double* B, const double* S, int64_t stride, int nb,
                                     const double* y, const double* omega, const double* diag, int64_t n1, double w2, int64_t nvec, int k0, int nr,
                                     const double* rhs, int nrhs)
{
    __shared__ double sm[DAV_RCHUNK * 4];
    double nrm[DAV_RCHUNK];
#pragma unroll
    for (int k = 0; k < DAV_RCHUNK; ++k) nrm[k] = 0.0;
    GRID_STRIDE(e, nvec)
    {
        double xa[DAV_RCHUNK], sa[DAV_RCHUNK];
#pragma unroll
        for (int k = 0; k < DAV_RCHUNK; ++k) xa[k] = sa[k] = 0.0;
        for (int p = 0; p < nb; ++p) {
            const double b = B[stride * p + e], s = S[stride * p + e];
#pragma unroll
            for (int k = 0; k < DAV_RCHUNK; ++k)
                if (k < nr) {
                    const double c = y[p + (int64_t)nb * (k0 + k)];
                    xa[k] = __fma_rn(c, b, xa[k]);
                    sa[k] = __fma_rn(c, s, sa[k]);
                }
        }
        const double D = diag[e], w = e < n1 ? 1.0 : w2;
#pragma unroll
        for (int k = 0; k < DAV_RCHUNK; ++k)
            if (k < nr) {
                const double om = omega[k0 + k];
                double rho = __fma_rn(-om, xa[k], sa[k]);
                if (rhs) rho = __dadd_rn(rhs[stride * ((k0 + k) % nrhs) + e], rho);
                double den = om - D;
                if (fabs(den) < DAV_CLAMP) den = den < 0.0 ? -DAV_CLAMP : DAV_CLAMP;
                X[stride * (k0 + k) + e] = xa[k];
                SX[stride * (k0 + k) + e] = sa[k];
                corr[stride * (k0 + k) + e] = rho / den;
                nrm[k] += w * rho * rho;
            }
    }
    block_sum<DAV_RCHUNK>(nrm, sm);
    if (threadIdx.x == 0)
        for (int k = 0; k < nr; ++k) partial[(int64_t)(k0 + k) * gridDim.x + blockIdx.x] = nrm[k];
}

// pend_j = rhs_(j % nrhs) / (shift_j - diag), j < nsys: the first pending vectors of the linear mode
__global__ void davidson_precondition_kernel(double* pend, const double* rhs, int nrhs, const double* shift, const double* diag, int64_t stride,
                                             int nsys, int64_t nvec)
{
    GRID_STRIDE(e, nvec)
    {
        const double D = diag[e];
        for (int j = 0; j < nsys; ++j) {
            double den = shift[j] - D;
            if (fabs(den) < DAV_CLAMP) den = den < 0.0 ? -DAV_CLAMP : DAV_CLAMP;
            pend[stride * j + e] = rhs[stride * (j % nrhs) + e] / den;
        }
    }
}

// the guarded denominator z - diag of the complex linear mode: inside DAV_CLAMP of zero it is the real +-DAV_CLAMP, with the sign of its
// real part (+ for zero)
__device__ inline void davidson_cden(double om, double ga, double D, double& dr, double& di)
{
    dr = om - D;
    di = ga;
    if (dr * dr + di * di < DAV_CLAMP * DAV_CLAMP) {
        dr = dr < 0.0 ? -DAV_CLAMP : DAV_CLAMP;
        di = 0.0;
    }
}

// The fused pass of the complex linear mode for the systems k0 .. k0 + nr (nr <= DAV_CCHUNK): every stored b_p and sigma_p is read once
// and gives, with y_k = yre_k + i yim_k, z_k = om_k + i ga_k,
//   P_k = sum_p yre(p,k) b_p,  Q_k = sum_p yim(p,k) b_p,  SP_k, SQ_k the same of sigma_p      -> columns 2 k and 2 k + 1 of X and SX
//   rho_re = rhs_(k % nrhs) + SP_k - om_k P_k + ga_k Q_k,   rho_im = SQ_k - om_k Q_k - ga_k P_k
//   corr_k = rho_k / (z_k - diag)                                                              -> columns 2 k and 2 k + 1 of corr
// and the block partials of <rho_re, rho_re> + <rho_im, rho_im> at partial[(k0 + k) nblk + blk].  yre, yim: nb x nsys column-major.
constexpr int DAV_CCHUNK = DAV_RCHUNK;   // complex systems of one launch: B and S are read as often per system as the real pass reads them
__global__ void davidson_cfused_kernel(double* X, double* SX, double* corr, double* partial, const double* B, const double* S, int64_t stride,
                                       int nb, const double* yre, const double* yim, const double* om, const double* ga, const double* diag,
                                       int64_t n1, double w2, int64_t nvec, int k0, int nr, const double* rhs, int nrhs)
{
    __shared__ double sm[DAV_CCHUNK * 4];
    double nrm[DAV_CCHUNK];
#pragma unroll
    for (int k = 0; k < DAV_CCHUNK; ++k) nrm[k] = 0.0;
    GRID_STRIDE(e, nvec)
    {
        double pr[DAV_CCHUNK], qi[DAV_CCHUNK], spr[DAV_CCHUNK], sqi[DAV_CCHUNK];
#pragma unroll
        for (int k = 0; k < DAV_CCHUNK; ++k) pr[k] = qi[k] = spr[k] = sqi[k] = 0.0;
        for (int p = 0; p < nb; ++p) {
            const double b = B[stride * p + e], s = S[stride * p + e];
#pragma unroll
            for (int k = 0; k < DAV_CCHUNK; ++k)
                if (k < nr) {
                    const double cr = yre[p + (int64_t)nb * (k0 + k)], ci = yim[p + (int64_t)nb * (k0 + k)];
                    pr[k] = __fma_rn(cr, b, pr[k]);
                    qi[k] = __fma_rn(ci, b, qi[k]);
                    spr[k] = __fma_rn(cr, s, spr[k]);
                    sqi[k] = __fma_rn(ci, s, sqi[k]);
                }
        }
        const double D = diag[e], w = e < n1 ? 1.0 : w2;
#pragma unroll
        for (int k = 0; k < DAV_CCHUNK; ++k)
            if (k < nr) {
                const double o = om[k0 + k], g = ga[k0 + k];
                double rre = __fma_rn(g, qi[k], __fma_rn(-o, pr[k], spr[k]));
                rre = __dadd_rn(rhs[stride * ((k0 + k) % nrhs) + e], rre);
                const double rim = __fma_rn(-g, pr[k], __fma_rn(-o, qi[k], sqi[k]));
                double dr, di;
                davidson_cden(o, g, D, dr, di);
                const double m2 = dr * dr + di * di;
                const int64_t c0 = stride * 2 * (k0 + k) + e, c1 = c0 + stride;
                X[c0] = pr[k];
                X[c1] = qi[k];
                SX[c0] = spr[k];
                SX[c1] = sqi[k];
                corr[c0] = (rre * dr + rim * di) / m2;
                corr[c1] = (rim * dr - rre * di) / m2;
                nrm[k] += w * (rre * rre + rim * rim);
            }
    }
    block_sum<DAV_CCHUNK>(nrm, sm);
    if (threadIdx.x == 0)
        for (int k = 0; k < nr; ++k) partial[(int64_t)(k0 + k) * gridDim.x + blockIdx.x] = nrm[k];
}

// pend_(2 j), pend_(2 j + 1) = Re, Im of rhs_(j % nrhs) / (z_j - diag), j < nsys: the first pending vectors of the complex linear mode
__global__ void davidson_cprecondition_kernel(double* pend, const double* rhs, int nrhs, const double* om, const double* ga, const double* diag,
                                              int64_t stride, int nsys, int64_t nvec)
{
    GRID_STRIDE(e, nvec)
    {
        const double D = diag[e];
        for (int j = 0; j < nsys; ++j) {
            double dr, di;
            davidson_cden(om[j], ga[j], D, dr, di);
            const double m2 = dr * dr + di * di, r = rhs[stride * (j % nrhs) + e];
            pend[stride * 2 * j + e] = r * dr / m2;
            pend[stride * (2 * j + 1) + e] = -(r * di) / m2;
        }
    }
}

void preload_davidson_so()
{
    static const bool loaded = [] {
        first_use_touch(reinterpret_cast<const void*>(davidson_panel_kernel));
        first_use_touch(reinterpret_cast<const void*>(davidson_final_kernel));
        first_use_touch(reinterpret_cast<const void*>(davidson_project_kernel));
        first_use_touch(reinterpret_cast<const void*>(davidson_scale_kernel));
        first_use_touch(reinterpret_cast<const void*>(davidson_ritz_kernel));
        first_use_touch(reinterpret_cast<const void*>(davidson_precondition_kernel));
        first_use_touch(reinterpret_cast<const void*>(davidson_cfused_kernel));
        first_use_touch(reinterpret_cast<const void*>(davidson_cprecondition_kernel));
        (void)hipGetLastError();
        return true;
    }();
    (void)loaded;
}

void read_back(Context& cx, double* host, const double* dev, int64_t n)
{
    AFESP_HIP(hipMemcpyAsync(host, dev, sizeof(double) * n, hipMemcpyDeviceToHost, cx.stream));
    cx.sync();
}

// the panel of (bq, sq) against the first ncol columns, summed: E.sums[q (ncol + 1) + p]
void panel(Context& cx, Davidson& E, int ncol, const double* bq, const double* sq)
{
    const int nblk = davidson_reduce_blocks(E.nvec);
    LAUNCH(davidson_panel_kernel, dim3(nblk, ncol + 1), E.partial, E.B, E.S, E.nvec, ncol, bq, sq, E.nvec, E.n1, E.w2);
    LAUNCH(davidson_final_kernel, dim3(3 * (ncol + 1)), E.sums, E.partial, nblk);
}

// Two passes of projection of x (and its companion sx) against the first nb columns through the panel, then x / |x| -> column nb of B
// (sx / |x| -> column nb of S).  -> false: the norm after projection is below DAV_DROP, nothing was stored
bool orthonormalise(Context& cx, Davidson& E, double* x, double* sx)
{
    const int nb = E.nb;
    if (nb > 0)
        for (int pass = 0; pass < 2; ++pass) {
            panel(cx, E, nb, x, nullptr);
            LAUNCH(davidson_project_kernel, grid_for(E.nvec), x, sx, E.B, E.S, E.nvec, nb, E.sums + 2 * (nb + 1), E.nvec);
        }
    panel(cx, E, 0, x, nullptr);
    double nrm2 = 0.0;
    read_back(cx, &nrm2, E.sums + 2, 1);
    const double nrm = std::sqrt(nrm2);
    if (!(nrm >= DAV_DROP)) return false;
    LAUNCH(davidson_scale_kernel, grid_for(E.nvec), E.B + E.nvec * nb, x, sx ? E.S + E.nvec * nb : nullptr, sx, 1.0 / nrm, E.nvec);
    return true;
}

// column nb of B and S is there: its row and column of the projected matrix, then nb + 1 columns
void extend_projected(Context& cx, Davidson& E)
{
    const int q = E.nb, ms = E.max_space;
    panel(cx, E, q, E.B + E.nvec * q, E.S + E.nvec * q);
    std::vector<double> h(3 * (q + 1));
    read_back(cx, h.data(), E.sums, 3 * (q + 1));
    for (int p = 0; p <= q; ++p) E.G[p + (size_t)ms * q] = h[p];
    for (int p = 0; p < q; ++p) E.G[q + (size_t)ms * p] = h[(q + 1) + p];
    E.nb = q + 1;
}

// linear mode: extend_projected, and row q of the projected right-hand sides <b_q, rhs_a> through the same panel kernel (the right-hand
// sides in the place of the stored columns, overlaps alone)
void extend_linear(Context& cx, Davidson& E)
{
    const int q = E.nb, ms = E.max_space, nr = E.nrhs;
    extend_projected(cx, E);
    const int nblk = davidson_reduce_blocks(E.nvec);
    LAUNCH(davidson_panel_kernel, dim3(nblk, nr + 1), E.partial, E.rhs, (const double*)nullptr, E.nvec, nr, E.B + E.nvec * q, (const double*)nullptr,
           E.nvec, E.n1, E.w2);
    LAUNCH(davidson_final_kernel, dim3(3 * (nr + 1)), E.sums, E.partial, nblk);
    std::vector<double> h(nr);
    read_back(cx, h.data(), E.sums + 2 * (nr + 1), nr);
    for (int a = 0; a < nr; ++a) E.prhs[q + (size_t)ms * a] = h[a];
}

}  // namespace

int davidson_reduce_blocks(int64_t nvec) { return (int)std::max<int64_t>(1, std::min<int64_t>((nvec + TB - 1) / TB, DAV_MAXBLK)); }

void davidson_reduce_final(Context& cx, double* out, const double* partial, int nout, int nblk)
{
    LAUNCH(davidson_final_kernel, dim3(nout), out, partial, nblk);
}

double davidson_bytes(double nvec, int nroots, int max_space)
{
    // b_p and sigma_p; the pending vectors, the Ritz vectors, their sigma and the corrections; the diagonal; the reduction buffers
    return 8.0 * ((2.0 * max_space + 4.0 * nroots + 1.0) * nvec + 3.0 * (max_space + 1.0) * (DAV_MAXBLK + 1.0) +
                  (double)nroots * (DAV_MAXBLK + 2.0) + (double)max_space * nroots);
}

double davidson_bytes_complex(double nvec, int nsys, int max_space)
{
    // four more columns per system, and the imaginary parts of the coefficients and shifts
    return davidson_bytes(nvec, nsys, max_space) + 8.0 * (4.0 * nsys * nvec + (double)max_space * nsys + nsys);
}

void davidson_alloc(Context& cx, Davidson& E, int64_t n1, int64_t nvec, double w2, bool follow, int nroots, int max_space,
                    const std::function<void(double* diag)>& fill_diag, bool wide)
{
    preload_davidson_so();
    const int64_t ncol = wide ? 2 * nroots : nroots;
    E.nroots = nroots;
    E.max_space = max_space;
    E.n1 = n1;
    E.nvec = nvec;
    E.w2 = w2;
    E.follow = follow;
    E.wide = wide;
    E.cplx = false;
    E.B = cx.alloc(nvec * max_space);
    E.S = cx.alloc(nvec * max_space);
    E.pend = cx.alloc(nvec * ncol);
    E.x = cx.alloc(nvec * ncol);
    E.sx = cx.alloc(nvec * ncol);
    E.corr = cx.alloc(nvec * ncol);
    E.partial = cx.alloc(std::max<int64_t>(3 * (max_space + 1), nroots) * DAV_MAXBLK);
    E.sums = cx.alloc(std::max<int64_t>(3 * (max_space + 1), nroots));
    E.coef = cx.alloc((int64_t)max_space * ncol + ncol);
    E.diag = cx.alloc(nvec);
    fill_diag(E.diag);
    E.G.assign((size_t)max_space * max_space, 0.0);
    E.omega.assign(nroots, 0.0);
    E.resnorm.assign(nroots, 0.0);
    E.flags.assign(nroots, 0);
}

void davidson_free(Context& cx, Davidson& E)
{
    double* bufs[] = {E.B, E.S, E.pend, E.x, E.sx, E.corr, E.partial, E.sums, E.coef, E.diag};
    for (double* b : bufs) cx.release(b);
}

void davidson_restart(Davidson& E)
{
    E.nb = 0;
    E.npend = 0;
    E.ritz = false;
    E.user_guess = false;
    E.cplx = false;
    E.target.clear();
    E.nsigma = E.ncollapse = 0;
    std::fill(E.flags.begin(), E.flags.end(), 0);
}

void davidson_set_pending_from_host(Context& cx, Davidson& E, const std::string& prefix, int k, const double* r1, const double* r2)
{
    if (k < 0 || k >= E.nroots || !r1 || !r2) throw Error(1, prefix + "set_guess: k outside 0 .. nroots - 1, or a NULL vector");
    if (E.nb > 0 || !E.user_guess) {   // the first of a block of the caller's guesses starts over: a running iteration, the unit guesses
        davidson_restart(E);
        k_fill(cx, E.pend, E.nvec * E.nroots, 0.0);   // (a column the caller leaves out stays zero and is dropped)
        E.user_guess = true;
    }
    AFESP_HIP(hipMemcpyAsync(E.pend + E.nvec * k, r1, sizeof(double) * E.n1, hipMemcpyHostToDevice, cx.stream));
    AFESP_HIP(hipMemcpyAsync(E.pend + E.nvec * k + E.n1, r2, sizeof(double) * (E.nvec - E.n1), hipMemcpyHostToDevice, cx.stream));
    cx.sync();
    E.npend = std::max(E.npend, k + 1);
}

int davidson_iterate(Context& cx, Davidson& E, const std::string& prefix, double tol, const DavidsonSigma& sigma)
{
    const std::string who = prefix + "iterate";
    const int64_t nvec = E.nvec;
    const int ms = E.max_space;
    if (E.nb == 0 && E.npend == 0) throw Error(1, who + ": no guess vectors (call " + prefix + "guess or " + prefix + "set_guess first)");
    const bool guess_step = E.nb == 0;
    // ---- collapse: restart from the Ritz vectors, their sigma being the same combination of the stored sigma (no new sigma builds)
    if (E.nb + E.npend > ms) {
        const int nr = std::min(E.nroots, E.nb);
        E.nb = 0;
        for (int k = 0; k < nr; ++k)
            if (orthonormalise(cx, E, E.x + nvec * k, E.sx + nvec * k)) extend_projected(cx, E);
        ++E.ncollapse;
    }
    // ---- the pending vectors: orthonormalise, sigma, one more row and column of the projected matrix <b_p, sigma(b_q)>
    for (int k = 0; k < E.npend && E.nb < ms; ++k) {
        if (!orthonormalise(cx, E, E.pend + nvec * k, nullptr)) continue;
        sigma(E.B + nvec * E.nb, E.S + nvec * E.nb);
        ++E.nsigma;
        extend_projected(cx, E);
    }
    E.npend = 0;
    if (E.nb == 0) throw Error(1, who + ": every guess vector vanished");
    // ---- the projected problem on the host
    const int nb = E.nb, nr = std::min(E.nroots, nb);
    std::vector<double> g((size_t)nb * nb), wr(nb), wi(nb), vr((size_t)nb * nb), up((size_t)nb * nr + nr);
    for (int q = 0; q < nb; ++q)
        for (int p = 0; p < nb; ++p) g[p + (size_t)nb * q] = E.G[p + (size_t)ms * q];
    const int rc = eig_general(nb, g.data(), nb, wr.data(), wi.data(), vr.data());
    if (rc) throw Error(1, who + ": the eigenvalues of the projected matrix were not found (status " + std::to_string(rc) + ")");
    // The roots taken: the lowest nr -- or, for a following state from the caller's guesses, those nearest to the Ritz values of its guess
    // step, target by target in their order, each root once, then by ascending omega.  A lower root of another symmetry, which only
    // rounding brings into the basis and the iteration then amplifies, takes no place that way.
    std::vector<int> sel(nr);
    std::iota(sel.begin(), sel.end(), 0);
    if (guess_step && E.follow && E.user_guess) E.target.assign(wr.begin(), wr.begin() + nr);
    else if (!E.target.empty() && nb > nr) {
        std::vector<char> used(nb, 0);
        const int nt = std::min<int>(nr, (int)E.target.size());
        for (int k = 0; k < nr; ++k) {
            int best = -1;
            for (int c = 0; c < nb; ++c) {
                if (used[c]) continue;
                // (beyond the targets -- a guess was dropped --: the lowest root not yet taken)
                if (best < 0 || (k < nt && std::fabs(wr[c] - E.target[k]) < std::fabs(wr[best] - E.target[k]))) best = c;
            }
            used[best] = 1;
            sel[k] = best;
        }
        std::sort(sel.begin(), sel.end());
    }
    for (int k = 0; k < nr; ++k) {
        const int c = sel[k];
        // a root with an imaginary part: the real part of its vector (the column of the pair's root with wi > 0)
        const double* col = vr.data() + (size_t)nb * (wi[c] < 0.0 && c > 0 ? c - 1 : c);
        double n2 = 0.0;
        for (int p = 0; p < nb; ++p) n2 += col[p] * col[p];
        const double sc = n2 > 0.0 ? 1.0 / std::sqrt(n2) : 0.0;   // <x, x> = sum_p y_p^2: the basis is orthonormal
        for (int p = 0; p < nb; ++p) up[p + (size_t)nb * k] = sc * col[p];
        up[(size_t)nb * nr + k] = wr[c];
        E.omega[k] = wr[c];
        E.flags[k] = wi[c] != 0.0 ? EOM_FLAG_COMPLEX : 0;
    }
    AFESP_HIP(hipMemcpyAsync(E.coef, up.data(), sizeof(double) * up.size(), hipMemcpyHostToDevice, cx.stream));
    // ---- Ritz pass
    const int nblk = davidson_reduce_blocks(nvec);
    for (int k0 = 0; k0 < nr; k0 += DAV_RCHUNK)
        LAUNCH(davidson_ritz_kernel, dim3(nblk), E.x, E.sx, E.corr, E.partial, E.B, E.S, nvec, nb, E.coef, E.coef + (size_t)nb * nr, E.diag, E.n1, E.w2,
               nvec, k0, std::min(DAV_RCHUNK, nr - k0), (const double*)nullptr, 1);
    LAUNCH(davidson_final_kernel, dim3(nr), E.sums, E.partial, nblk);
    std::vector<double> nrm(nr);
    read_back(cx, nrm.data(), E.sums, nr);   // (also: `up` is no longer read)
    E.ritz = true;
    int all = nr == E.nroots ? 1 : 0;
    for (int k = 0; k < E.nroots; ++k) {
        if (k >= nr) {   // fewer basis vectors than roots: not found (yet)
            E.omega[k] = 0.0;
            E.resnorm[k] = HUGE_VAL;
            E.flags[k] = 0;
            continue;
        }
        E.resnorm[k] = std::sqrt(nrm[k]);
        if (E.resnorm[k] < tol) E.flags[k] |= EOM_FLAG_CONVERGED;
        else {
            all = 0;
            k_copy(cx, E.pend + nvec * E.npend, E.corr + nvec * k, nvec);
            ++E.npend;
        }
    }
    return all;
}

void davidson_linear_start(Context& cx, Davidson& E, const double* rhs, int nrhs, const double* shifts)
{
    if (!rhs || nrhs < 1 || nrhs > E.nroots || !shifts) throw Error(1, "davidson_linear_start: no right-hand sides or shifts");
    davidson_restart(E);
    E.rhs = rhs;
    E.nrhs = nrhs;
    E.shift.assign(shifts, shifts + E.nroots);
    E.prhs.assign((size_t)E.max_space * nrhs, 0.0);
    std::fill(E.resnorm.begin(), E.resnorm.end(), HUGE_VAL);
    AFESP_HIP(hipMemcpyAsync(E.coef, E.shift.data(), sizeof(double) * E.nroots, hipMemcpyHostToDevice, cx.stream));
    LAUNCH(davidson_precondition_kernel, grid_for(E.nvec), E.pend, rhs, nrhs, E.coef, E.diag, E.nvec, E.nroots, E.nvec);
    cx.sync();   // (E.coef is written again by the first step)
    E.npend = E.nroots;
}

void davidson_linear_start_complex(Context& cx, Davidson& E, const double* rhs, int nrhs, const double* shift_re, const double* shift_im)
{
    const char* who = "davidson_linear_start_complex";
    if (!rhs || nrhs < 1 || nrhs > E.nroots || !shift_re || !shift_im) throw Error(1, std::string(who) + ": no right-hand sides or shifts");
    if (!E.wide || E.max_space < 4 * E.nroots || E.nroots > 64)
        throw Error(1, std::string(who) + ": needs a state with two columns per system, 4 nsys <= max_space and nsys <= 64");
    const int ns = E.nroots;
    davidson_restart(E);
    E.cplx = true;
    E.rhs = rhs;
    E.nrhs = nrhs;
    E.shift.assign(shift_re, shift_re + ns);
    E.shift_im.assign(shift_im, shift_im + ns);
    E.prhs.assign((size_t)E.max_space * nrhs, 0.0);
    std::fill(E.resnorm.begin(), E.resnorm.end(), HUGE_VAL);
    AFESP_HIP(hipMemcpyAsync(E.coef, E.shift.data(), sizeof(double) * ns, hipMemcpyHostToDevice, cx.stream));
    AFESP_HIP(hipMemcpyAsync(E.coef + ns, E.shift_im.data(), sizeof(double) * ns, hipMemcpyHostToDevice, cx.stream));
    LAUNCH(davidson_cprecondition_kernel, grid_for(E.nvec), E.pend, rhs, nrhs, E.coef, E.coef + ns, E.diag, E.nvec, ns, E.nvec);
    cx.sync();   // (E.coef is written again by the first step)
    E.npend = 2 * ns;
}

namespace {

// davidson_linear_iterate of a state in the complex mode (davidson_so.h)
int linear_iterate_complex(Context& cx, Davidson& E, const std::string& prefix, double tol, const DavidsonSigma& sigma)
{
    const std::string who = prefix + "iterate";
    const int64_t nvec = E.nvec;
    const int ms = E.max_space, ns = E.nroots;
    if (!E.rhs || (E.nb == 0 && E.npend == 0)) throw Error(1, who + ": no right-hand sides (call " + prefix + "init first)");
    // ---- collapse onto Re x_j, Im x_j of every system, in column order (no new sigma builds)
    if (E.nb + E.npend > ms) {
        E.nb = 0;
        for (int k = 0; k < 2 * ns; ++k)
            if (orthonormalise(cx, E, E.x + nvec * k, E.sx + nvec * k)) extend_linear(cx, E);
        ++E.ncollapse;
    }
    // ---- the pending vectors, as in the real mode
    for (int k = 0; k < E.npend && E.nb < ms; ++k) {
        if (!orthonormalise(cx, E, E.pend + nvec * k, nullptr)) continue;
        sigma(E.B + nvec * E.nb, E.S + nvec * E.nb);
        ++E.nsigma;
        extend_linear(cx, E);
    }
    E.npend = 0;
    if (E.nb == 0) throw Error(1, who + ": every right-hand side vanished");
    // ---- (G - z_j) y_j = -B^T rhs_j on the host; up: Re y (nb x ns), Im y (nb x ns), omega (ns), gamma (ns)
    const int nb = E.nb;
    double gmax = 0.0;
    for (int q = 0; q < nb; ++q)
        for (int p = 0; p < nb; ++p) gmax = std::max(gmax, std::fabs(E.G[p + (size_t)ms * q]));
    std::vector<double> m(2 * (size_t)nb * nb), y(2 * (size_t)nb), up(2 * ((size_t)nb * ns + ns));
    double *yre = up.data(), *yim = yre + (size_t)nb * ns, *uom = yim + (size_t)nb * ns, *uga = uom + ns;
    for (int j = 0; j < ns; ++j) {
        const double om = E.shift[j], ga = E.shift_im[j];
        for (int q = 0; q < nb; ++q)
            for (int p = 0; p < nb; ++p) {
                m[2 * (p + (size_t)nb * q)] = E.G[p + (size_t)ms * q] - (p == q ? om : 0.0);
                m[2 * (p + (size_t)nb * q) + 1] = p == q ? -ga : 0.0;
            }
        for (int p = 0; p < nb; ++p) {
            y[2 * p] = -E.prhs[p + (size_t)ms * (j % E.nrhs)];
            y[2 * p + 1] = 0.0;
        }
        const int rc = lu_solve_complex(nb, m.data(), nb, 1, y.data(), nb, DAV_POLE * std::max(gmax, std::hypot(om, ga)));
        if (rc == 2)
            throw Error(DAVIDSON_ERR_POLE, who + ": frequency at a pole: system " + std::to_string(j) + " (shift " + std::to_string(om) + " + " +
                                               std::to_string(ga) + " i) is singular in the projected space of " + std::to_string(nb) + " vectors");
        if (rc) throw Error(1, who + ": the projected system was not solved (status " + std::to_string(rc) + ")");
        for (int p = 0; p < nb; ++p) {
            yre[p + (size_t)nb * j] = y[2 * p];
            yim[p + (size_t)nb * j] = y[2 * p + 1];
        }
        uom[j] = om;
        uga[j] = ga;
    }
    AFESP_HIP(hipMemcpyAsync(E.coef, up.data(), sizeof(double) * up.size(), hipMemcpyHostToDevice, cx.stream));
    // ---- the fused pass
    const int nblk = davidson_reduce_blocks(nvec);
    const double* dco = E.coef;
    for (int k0 = 0; k0 < ns; k0 += DAV_CCHUNK)
        LAUNCH(davidson_cfused_kernel, dim3(nblk), E.x, E.sx, E.corr, E.partial, E.B, E.S, nvec, nb, dco, dco + (size_t)nb * ns,
               dco + 2 * (size_t)nb * ns, dco + 2 * (size_t)nb * ns + ns, E.diag, E.n1, E.w2, nvec, k0, std::min(DAV_CCHUNK, ns - k0), E.rhs, E.nrhs);
    LAUNCH(davidson_final_kernel, dim3(ns), E.sums, E.partial, nblk);
    std::vector<double> nrm(ns);
    read_back(cx, nrm.data(), E.sums, ns);   // (also: `up` is no longer read)
    E.ritz = true;
    int all = 1;
    for (int j = 0; j < ns; ++j) {
        E.omega[j] = E.shift[j];
        E.resnorm[j] = std::sqrt(nrm[j]);
        E.flags[j] = E.resnorm[j] < tol ? EOM_FLAG_CONVERGED : 0;
        if (E.flags[j]) continue;
        all = 0;
        LAUNCH(davidson_scale_kernel, grid_for(nvec), E.pend + nvec * E.npend, E.corr + nvec * 2 * j, E.pend + nvec * (E.npend + 1),
               E.corr + nvec * (2 * j + 1), 1.0 / E.resnorm[j], nvec);
        E.npend += 2;
    }
    return all;
}

}  // namespace

int davidson_linear_iterate(Context& cx, Davidson& E, const std::string& prefix, double tol, const DavidsonSigma& sigma)
{
    if (E.cplx) return linear_iterate_complex(cx, E, prefix, tol, sigma);
    const std::string who = prefix + "iterate";
    const int64_t nvec = E.nvec;
    const int ms = E.max_space, ns = E.nroots;
    if (!E.rhs || (E.nb == 0 && E.npend == 0)) throw Error(1, who + ": no right-hand sides (call " + prefix + "init first)");
    // ---- collapse onto the current solutions, their sigma being the same combination of the stored sigma (no new sigma builds)
    if (E.nb + E.npend > ms) {
        E.nb = 0;
        for (int k = 0; k < ns; ++k)
            if (orthonormalise(cx, E, E.x + nvec * k, E.sx + nvec * k)) extend_linear(cx, E);
        ++E.ncollapse;
    }
    // ---- the pending vectors: orthonormalise, ONE sigma build each for all systems, the projected matrix and right-hand sides
    for (int k = 0; k < E.npend && E.nb < ms; ++k) {
        if (!orthonormalise(cx, E, E.pend + nvec * k, nullptr)) continue;
        sigma(E.B + nvec * E.nb, E.S + nvec * E.nb);
        ++E.nsigma;
        extend_linear(cx, E);
    }
    E.npend = 0;
    if (E.nb == 0) throw Error(1, who + ": every right-hand side vanished");
    // ---- (G - shift_j) y_j = -B^T rhs_j on the host
    const int nb = E.nb;
    double gmax = 0.0;
    for (int q = 0; q < nb; ++q)
        for (int p = 0; p < nb; ++p) gmax = std::max(gmax, std::fabs(E.G[p + (size_t)ms * q]));
    std::vector<double> m((size_t)nb * nb), up((size_t)nb * ns + ns);
    for (int j = 0; j < ns; ++j) {
        const double om = E.shift[j];
        for (int q = 0; q < nb; ++q)
            for (int p = 0; p < nb; ++p) m[p + (size_t)nb * q] = E.G[p + (size_t)ms * q] - (p == q ? om : 0.0);
        double* y = up.data() + (size_t)nb * j;
        for (int p = 0; p < nb; ++p) y[p] = -E.prhs[p + (size_t)ms * (j % E.nrhs)];
        const int rc = lu_solve(nb, m.data(), nb, 1, y, nb, DAV_POLE * std::max(gmax, std::fabs(om)));
        if (rc == 2)
            throw Error(DAVIDSON_ERR_POLE, who + ": frequency at a pole: system " + std::to_string(j) + " (shift " + std::to_string(om) +
                                               ") is singular in the projected space of " + std::to_string(nb) + " vectors");
        if (rc) throw Error(1, who + ": the projected system was not solved (status " + std::to_string(rc) + ")");
        up[(size_t)nb * ns + j] = om;
    }
    AFESP_HIP(hipMemcpyAsync(E.coef, up.data(), sizeof(double) * up.size(), hipMemcpyHostToDevice, cx.stream));
    // ---- the fused pass: the Ritz kernel with the right-hand sides
    const int nblk = davidson_reduce_blocks(nvec);
    for (int k0 = 0; k0 < ns; k0 += DAV_RCHUNK)
        LAUNCH(davidson_ritz_kernel, dim3(nblk), E.x, E.sx, E.corr, E.partial, E.B, E.S, nvec, nb, E.coef, E.coef + (size_t)nb * ns, E.diag, E.n1,
               E.w2, nvec, k0, std::min(DAV_RCHUNK, ns - k0), E.rhs, E.nrhs);
    LAUNCH(davidson_final_kernel, dim3(ns), E.sums, E.partial, nblk);
    std::vector<double> nrm(ns);
    read_back(cx, nrm.data(), E.sums, ns);   // (also: `up` is no longer read)
    E.ritz = true;
    int all = 1;
    for (int j = 0; j < ns; ++j) {
        E.omega[j] = E.shift[j];
        E.resnorm[j] = std::sqrt(nrm[j]);
        E.flags[j] = E.resnorm[j] < tol ? EOM_FLAG_CONVERGED : 0;
        if (E.flags[j]) continue;
        all = 0;
        // (scaled by 1 / |rho_j|: the drop threshold of the orthonormalisation is absolute, and a correction of a nearly converged system
        // is as small as its residual)
        LAUNCH(davidson_scale_kernel, grid_for(nvec), E.pend + nvec * E.npend, E.corr + nvec * j, (double*)nullptr, (const double*)nullptr,
               1.0 / E.resnorm[j], nvec);
        ++E.npend;
    }
    return all;
}

void davidson_get_vector(Context& cx, Davidson& E, const std::string& prefix, int k, double* r1, double* r2)
{
    if (!E.ritz || k < 0 || k >= std::min(E.nroots, E.nb) || !r1 || !r2)
        throw Error(1, prefix + "get_vector: no Ritz vector k (iterate first; k in 0 .. nroots - 1), or a NULL vector");
    AFESP_HIP(hipMemcpyAsync(r1, E.x + E.nvec * k, sizeof(double) * E.n1, hipMemcpyDeviceToHost, cx.stream));
    AFESP_HIP(hipMemcpyAsync(r2, E.x + E.nvec * k + E.n1, sizeof(double) * (E.nvec - E.n1), hipMemcpyDeviceToHost, cx.stream));
    cx.sync();
}

}  // namespace afesp
