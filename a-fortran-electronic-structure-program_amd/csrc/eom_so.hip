// eom_so.hip -- EOM-EE-CCSD on the spin-orbital CCSD state (eom_so.h): the sigma build sigma(r) = A r, term by term in
// the letters of tests/np_eom.py (sigma_explicit) over the H-bar elements of the live Lambda state, and a block Davidson iteration for the
// lowest eigenvalues of the non-symmetric A.  Launches are plain call-by-call ones, as Lambda's.  Every reduction is block partials on a
// grid fixed by the vector length, then an ordered final sum: the same input gives the same bits on every run.
#include "device_util.h"
#include "eom_so.h"
#include "small_eig.h"

#include <cmath>
#include <numeric>

namespace afesp {
namespace {

constexpr int EOM_MAXBLK = 128;   // blocks of a reduction (at most TB: eom_final_kernel sums them in one block)
constexpr int EOM_RCHUNK = 8;     // roots one launch of the Ritz pass forms
constexpr double EOM_DROP = 1e-10, EOM_CLAMP = 1e-4;

// sigma2 from the ladder block and the three permutation carriers, and sigma1's diagonal term (threads x < o v):
//   sigma2 = lad + P(ij)P(ab) AB + P(ij) A + P(ab) Bm - D2 r2,   sigma1 -= D1 r1.
// lad is antisymmetric in both pairs, A in a,b and Bm in i,j -- as sums of products only up to rounding.  With c = 1/4 lad + AB +
// 1/2 (A + Bm) the value is (c(ijab) + c(jiba)) - (c(jiab) + c(ijba)): exchanging i and j, or a and b, exchanges the two brackets, so the
// value is negated to the bit and vanishes on the diagonals; D2 enters as the mean of its four images for the same reason.
__device__ __forceinline__ double eom_carrier(const double* lad, const double* AB, const double* A, const double* Bm, int64_t p)
{
    return __dadd_rn(__dadd_rn(__dmul_rn(0.25, lad[p]), AB[p]), __dmul_rn(0.5, __dadd_rn(A[p], Bm[p])));
}
__global__ void eom_sigma_assemble_kernel(double* s2, double* s1, const double* lad, const double* AB, const double* A, const double* Bm,
                                          const double* r2, const double* r1, const double* D2, const double* D1, int o, int v)
{
    const int64_t n2 = (int64_t)o * o * v * v, n1 = (int64_t)o * v;
    GRID_STRIDE(x, n2)
    {
        const int i = (int)(x % o), j = (int)((x / o) % o), a = (int)((x / ((int64_t)o * o)) % v), b = (int)(x / ((int64_t)o * o * v));
        const int64_t ji = j + (int64_t)o * (i + (int64_t)o * (a + (int64_t)v * b));
        const int64_t ba = i + (int64_t)o * (j + (int64_t)o * (b + (int64_t)v * a));
        const int64_t jiba = j + (int64_t)o * (i + (int64_t)o * (b + (int64_t)v * a));
        const double same = __dadd_rn(eom_carrier(lad, AB, A, Bm, x), eom_carrier(lad, AB, A, Bm, jiba));
        const double swapped = __dadd_rn(eom_carrier(lad, AB, A, Bm, ji), eom_carrier(lad, AB, A, Bm, ba));
        const double d = __dmul_rn(0.25, __dadd_rn(__dadd_rn(D2[x], D2[jiba]), __dadd_rn(D2[ji], D2[ba])));
        s2[x] = __dadd_rn(__dadd_rn(same, -swapped), -__dmul_rn(d, r2[x]));
        if (x < n1) s1[x] = __dadd_rn(s1[x], -__dmul_rn(D1[x], r1[x]));   // (o v <= o^2 v^2: every single has its thread)
    }
}

// The Gram panel of one vector pair (bq, sq) against ncol stored columns, in one launch -- block (blk, p):
//   p < ncol:  <b_p, sq>, <s_p, bq>, <b_p, bq>        p = ncol:  <bq, sq>, the same again, <bq, bq>
// with the weights 1 on the first n1 elements and 1/4 behind them; partial[(q (ncol + 1) + p) nblk + blk], q = 0, 1, 2.  sq null: the
// overlaps alone (q = 2; the others are written as zero).
__global__ void eom_panel_kernel(double* partial, const double* B, const double* S, int64_t stride, int ncol, const double* bq, const double* sq,
                                 int64_t nvec, int64_t n1)
{
    __shared__ double sm[3 * 4];
    const int p = blockIdx.y, nblk = gridDim.x;
    const double* bp = p < ncol ? B + stride * p : bq;
    const double* sp = sq ? (p < ncol ? S + stride * p : sq) : nullptr;
    double acc[3] = {0.0, 0.0, 0.0};
    GRID_STRIDE(x, nvec)
    {
        const double w = x < n1 ? 1.0 : 0.25, b = bp[x], q = bq[x];
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
__global__ void eom_final_kernel(double* out, const double* partial, int nblk)
{
    __shared__ double red[TB];
    red[threadIdx.x] = (int)threadIdx.x < nblk ? partial[(int64_t)blockIdx.x * nblk + threadIdx.x] : 0.0;
    __syncthreads();
    for (int w = TB / 2; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[blockIdx.x] = red[0];
}

// one projection pass: x -= sum_p coef[p] b_p, and the companion sx -= sum_p coef[p] s_p where given
__global__ void eom_project_kernel(double* x, double* sx, const double* B, const double* S, int64_t stride, int ncol, const double* coef, int64_t nvec)
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

__global__ void eom_scale_kernel(double* dst, const double* src, double* dst2, const double* src2, double scale, int64_t nvec)
{
    GRID_STRIDE(e, nvec)
    {
        dst[e] = __dmul_rn(scale, src[e]);
        if (src2) dst2[e] = __dmul_rn(scale, src2[e]);
    }
}

// a guess: +1 at i0 and i1, -1 at i2 and i3 (negative index: none) of a vector that is zero otherwise
__global__ void eom_unit_kernel(double* x, int64_t nvec, int64_t i0, int64_t i1, int64_t i2, int64_t i3)
{
    GRID_STRIDE(e, nvec) x[e] = (e == i0 || e == i1) ? 1.0 : ((e == i2 || e == i3) ? -1.0 : 0.0);
}

// The Ritz pass for the roots k0 .. k0 + nr (nr <= EOM_RCHUNK): every stored b_p and sigma_p is read once and gives
//   x_k = sum_p y(p,k) b_p,  sx_k = sum_p y(p,k) sigma_p,  rho_k = sx_k - omega_k x_k,  corr_k = rho_k / (omega_k + D)
// (|omega_k + D| clamped below at EOM_CLAMP, keeping its sign; -D is the diagonal guess of A) and the block partials of <rho_k, rho_k>
// at partial[(k0 + k) nblk + blk].  y: nb x nroots column-major.
__global__ void eom_ritz_kernel(double* X, double* SX, double* corr, double* partial, const double* B, const double* S, int64_t stride, int nb,
                                const double* y, const double* omega, const double* D1, const double* D2, int o, int v, int64_t nvec, int k0, int nr)
{
    __shared__ double sm[EOM_RCHUNK * 4];
    const int64_t n1 = (int64_t)o * v;
    double nrm[EOM_RCHUNK];
#pragma unroll
    for (int k = 0; k < EOM_RCHUNK; ++k) nrm[k] = 0.0;
    GRID_STRIDE(e, nvec)
    {
        double xa[EOM_RCHUNK], sa[EOM_RCHUNK];
#pragma unroll
        for (int k = 0; k < EOM_RCHUNK; ++k) xa[k] = sa[k] = 0.0;
        for (int p = 0; p < nb; ++p) {
            const double b = B[stride * p + e], s = S[stride * p + e];
#pragma unroll
            for (int k = 0; k < EOM_RCHUNK; ++k)
                if (k < nr) {
                    const double c = y[p + (int64_t)nb * (k0 + k)];
                    xa[k] = __fma_rn(c, b, xa[k]);
                    sa[k] = __fma_rn(c, s, sa[k]);
                }
        }
        // (D2 is summed as ((e_i + e_j) - e_a) - e_b: symmetric in i,j to the bit, in a,b only with its image -- the corrections stay
        // antisymmetric to the bit as the basis vectors are)
        double D;
        if (e < n1) D = D1[e];
        else {
            const int64_t x = e - n1, ij = x % ((int64_t)o * o);
            const int a = (int)((x / ((int64_t)o * o)) % v), b = (int)(x / ((int64_t)o * o * v));
            D = __dmul_rn(0.5, __dadd_rn(D2[x], D2[ij + (int64_t)o * o * (b + (int64_t)v * a)]));
        }
        const double w = e < n1 ? 1.0 : 0.25;
#pragma unroll
        for (int k = 0; k < EOM_RCHUNK; ++k)
            if (k < nr) {
                const double om = omega[k0 + k];
                const double rho = __fma_rn(-om, xa[k], sa[k]);
                double den = om + D;
                if (fabs(den) < EOM_CLAMP) den = den < 0.0 ? -EOM_CLAMP : EOM_CLAMP;
                X[stride * (k0 + k) + e] = xa[k];
                SX[stride * (k0 + k) + e] = sa[k];
                corr[stride * (k0 + k) + e] = rho / den;
                nrm[k] += w * rho * rho;
            }
    }
    block_sum<EOM_RCHUNK>(nrm, sm);
    if (threadIdx.x == 0)
        for (int k = 0; k < nr; ++k) partial[(int64_t)(k0 + k) * gridDim.x + blockIdx.x] = nrm[k];
}

void need_plain(Context& cx)
{
    if (cx.rec) throw Error(1, "so_eom: the EOM equations are not part of a recorded (launch-fused) sequence");
}

inline int eom_nblk(int64_t nvec) { return (int)std::max<int64_t>(1, std::min<int64_t>((nvec + TB - 1) / TB, EOM_MAXBLK)); }

void read_back(Context& cx, double* host, const double* dev, int64_t n)
{
    AFESP_HIP(hipMemcpyAsync(host, dev, sizeof(double) * n, hipMemcpyDeviceToHost, cx.stream));
    cx.sync();
}

// the panel of (bq, sq) against the first ncol columns, summed: E.sums[q (ncol + 1) + p]
void panel(Context& cx, SOEom& E, int ncol, const double* bq, const double* sq, int64_t n1)
{
    const int nblk = eom_nblk(E.nvec);
    LAUNCH(eom_panel_kernel, dim3(nblk, ncol + 1), E.partial, E.B, E.S, E.nvec, ncol, bq, sq, E.nvec, n1);
    LAUNCH(eom_final_kernel, dim3(3 * (ncol + 1)), E.sums, E.partial, nblk);
}

// Two passes of projection of x (and its companion sx) against the first nb columns through the panel, then x / |x| -> column nb of B
// (sx / |x| -> column nb of S).  -> false: the norm after projection is below EOM_DROP, nothing was stored
bool orthonormalise(Context& cx, SOEom& E, double* x, double* sx, int64_t n1)
{
    const int nb = E.nb;
    if (nb > 0)
        for (int pass = 0; pass < 2; ++pass) {
            panel(cx, E, nb, x, nullptr, n1);
            LAUNCH(eom_project_kernel, grid_for(E.nvec), x, sx, E.B, E.S, E.nvec, nb, E.sums + 2 * (nb + 1), E.nvec);
        }
    panel(cx, E, 0, x, nullptr, n1);
    double nrm2 = 0.0;
    read_back(cx, &nrm2, E.sums + 2, 1);
    const double nrm = std::sqrt(nrm2);
    if (!(nrm >= EOM_DROP)) return false;
    LAUNCH(eom_scale_kernel, grid_for(E.nvec), E.B + E.nvec * nb, x, sx ? E.S + E.nvec * nb : nullptr, sx, 1.0 / nrm, E.nvec);
    return true;
}

// column nb of B and S is there: its row and column of the projected matrix, then nb + 1 columns
void extend_projected(Context& cx, SOEom& E, int64_t n1)
{
    const int q = E.nb, ms = E.max_space;
    panel(cx, E, q, E.B + E.nvec * q, E.S + E.nvec * q, n1);
    std::vector<double> h(3 * (q + 1));
    read_back(cx, h.data(), E.sums, 3 * (q + 1));
    for (int p = 0; p <= q; ++p) E.G[p + (size_t)ms * q] = h[p];
    for (int p = 0; p < q; ++p) E.G[q + (size_t)ms * p] = h[(q + 1) + p];
    E.nb = q + 1;
}

void free_buffers(Context& cx, SOEom& E)
{
    double* bufs[] = {E.B, E.S, E.pend, E.x, E.sx, E.corr, E.partial, E.sums, E.coef};
    for (double* b : bufs) cx.release(b);
}

}  // namespace

void preload_eom_so()
{
    first_use_touch(reinterpret_cast<const void*>(eom_sigma_assemble_kernel));
    first_use_touch(reinterpret_cast<const void*>(eom_panel_kernel));
    first_use_touch(reinterpret_cast<const void*>(eom_final_kernel));
    first_use_touch(reinterpret_cast<const void*>(eom_project_kernel));
    first_use_touch(reinterpret_cast<const void*>(eom_scale_kernel));
    first_use_touch(reinterpret_cast<const void*>(eom_unit_kernel));
    first_use_touch(reinterpret_cast<const void*>(eom_ritz_kernel));
    (void)hipGetLastError();
}

int so_eom_reduce_blocks(int64_t nvec) { return eom_nblk(nvec); }

void so_eom_reduce_final(Context& cx, double* out, const double* partial, int nout, int nblk)
{
    LAUNCH(eom_final_kernel, dim3(nout), out, partial, nblk);
}

double so_eom_bytes(int64_t o, int64_t v, int nroots, int max_space)
{
    const double O = (double)o, V = (double)v, o2v2 = O * O * V * V, nvec = O * V + o2v2;
    // b_p and sigma_p; the pending vectors, the Ritz vectors, their sigma and the corrections; the reduction buffers; the scratch of a
    // sigma build (lad, AB, A, B, Z, the o^4 product, Y_vv, Y_oo) and the two staging vectors of the host entry
    const double doubles = (2.0 * max_space + 4.0 * nroots) * nvec + 3.0 * (max_space + 1.0) * (EOM_MAXBLK + 1.0) + (double)nroots * (EOM_MAXBLK + 2.0) +
                           (double)max_space * nroots + 4.0 * o2v2 + O * O * O * V + O * O * O * O + V * V + O * O + 2.0 * nvec;
    return 8.0 * doubles;
}

// the right-hand and the left-hand Davidson state are one type and one code: `left` chooses the slot, the sigma build and the names
static SOEom*& eom_slot(SOState& s, bool left) { return left ? s.eom_left : s.eom; }
static std::string eom_name(bool left, const char* call) { return std::string(left ? "afesp_ccsd_so_eom_left_" : "afesp_ccsd_so_eom_") + call; }

static void eom_free_one(Context& cx, SOState& s, bool left)
{
    SOEom*& e = eom_slot(s, left);
    if (!e) return;
    free_buffers(cx, *e);
    delete e;
    e = nullptr;
}

void so_eom_free(Context& cx, SOState& s)
{
    eom_free_one(cx, s, false);
    eom_free_one(cx, s, true);
}

SOEom& so_eom_need(SOState& s, const char* who, bool left)
{
    so_lambda_need(s, who);
    SOEom* e = eom_slot(s, left);
    if (!e || e->epoch != s.amp_epoch)
        throw Error(LAMBDA_ERR_STALE, std::string(who) + (left ? ": no left EOM state for the live Lambda state (call afesp_ccsd_so_eom_left_init first)"
                                                               : ": no EOM state for the live Lambda state (call afesp_ccsd_so_eom_init first)"));
    return *e;
}

void so_eom_init(Context& cx, SOState& s, int nroots, int max_space, bool left)
{
    need_plain(cx);
    const std::string who = eom_name(left, "init");
    SOLambda& L = so_lambda_need(s, who.c_str());
    const int64_t O = s.o, V = s.v, nvec = O * V + O * O * V * V, nunique = O * V + (O * (O - 1) / 2) * (V * (V - 1) / 2);
    if (nroots < 1 || (int64_t)nroots > nunique)
        throw Error(1, who + ": nroots must be in 1 .. " + std::to_string(nunique) + " (the unique singles and doubles)");
    if ((int64_t)max_space < 2 * (int64_t)nroots || max_space > 4096)
        throw Error(1, who + ": max_space must be in 2 nroots .. 4096");
    eom_free_one(cx, s, left);
    if (!cx.fits(left ? so_eom_left_bytes(O, V, nroots, max_space) : so_eom_bytes(O, V, nroots, max_space)))
        throw Error(1, who + ": the EOM state of this system (" + std::to_string(max_space) + " basis vectors) does not fit the free device memory");
    static const bool loaded = (preload_eom_so(), true);
    (void)loaded;
    if (left) {
        static const bool loaded_left = (preload_eom_left_so(), true);
        (void)loaded_left;
    }
    eom_slot(s, left) = new SOEom();
    SOEom& E = *eom_slot(s, left);
    try {
        E.left = left;
        E.nroots = nroots;
        E.max_space = max_space;
        E.nvec = nvec;
        E.B = cx.alloc(nvec * max_space);
        E.S = cx.alloc(nvec * max_space);
        E.pend = cx.alloc(nvec * nroots);
        E.x = cx.alloc(nvec * nroots);
        E.sx = cx.alloc(nvec * nroots);
        E.corr = cx.alloc(nvec * nroots);
        E.partial = cx.alloc(std::max<int64_t>(3 * (max_space + 1), nroots) * EOM_MAXBLK);
        E.sums = cx.alloc(std::max<int64_t>(3 * (max_space + 1), nroots));
        E.coef = cx.alloc((int64_t)max_space * nroots + nroots);
        E.G.assign((size_t)max_space * max_space, 0.0);
        E.omega.assign(nroots, 0.0);
        E.resnorm.assign(nroots, 0.0);
        E.flags.assign(nroots, 0);
        E.epoch = L.epoch;
        cx.sync();
    } catch (...) {
        try { cx.quiesce(); eom_free_one(cx, s, left); } catch (...) {}
        throw;
    }
}

void so_eom_sigma(Context& cx, SOState& s, const double* r, double* sigma)
{
    need_plain(cx);
    SOLambda& L = so_lambda_need(s, "afesp_ccsd_so_eom_sigma");
    auto C = [&](double al, const Tensor& A, const char* la, const Tensor& B, const char* lb, double be, const Tensor& Cc,
                 const char* lc) { contract(cx, al, A, la, B, lb, be, Cc, lc); };
    const int o = s.o, v = s.v;
    const int64_t O = o, V = v, ov = O * V, o2v2 = O * O * V * V;
    const Tensor r1 = view(const_cast<double*>(r), {O, V}), r2 = view(const_cast<double*>(r) + ov, {O, O, V, V});
    const Tensor s1 = view(sigma, {O, V});
    const Tensor &t1 = s.t1, &t2 = s.t2;
    // ---- sigma1: H_ae r_ie - H_mi r_ma + H_me r_imae + H_maei r_me - 1/2 H_mnie r_mnae + 1/2 H_amef r_imef  (- D1 r1: the assemble kernel)
    C(1.0, L.Hvv, "ae", r1, "ie", 0.0, s1, "ia");
    C(-1.0, L.Hoo, "mi", r1, "ma", 1.0, s1, "ia");
    C(1.0, r2, "imae", L.Hov, "me", 1.0, s1, "ia");
    C(1.0, L.Hovvo, "maei", r1, "me", 1.0, s1, "ia");
    C(-0.5, r2, "mnae", L.Hooov, "mnie", 1.0, s1, "ia");
    C(0.5, r2, "imef", L.Hvovv, "amef", 1.0, s1, "ia");
    // ---- Y_be = H_bmef r_mf - 1/2 <mn||ef> r_mnbf,  Y_mj = H_mnje r_ne + 1/2 <mn||ef> r_jnef
    Tensor Yvv = view(cx.scratch("eom_Yvv", V * V), {V, V}), Yoo = view(cx.scratch("eom_Yoo", O * O), {O, O});
    C(1.0, L.Hvovv, "bmef", r1, "mf", 0.0, Yvv, "be");
    C(-0.5, s.oovv, "mnef", r2, "mnbf", 1.0, Yvv, "be");
    C(1.0, L.Hooov, "mnje", r1, "ne", 0.0, Yoo, "mj");
    C(0.5, s.oovv, "mnef", r2, "jnef", 1.0, Yoo, "mj");
    // ---- sigma2
    Tensor lad = view(cx.scratch("eom_lad", o2v2), {O, O, V, V});
    Tensor AB = view(cx.scratch("so_AB", o2v2), {O, O, V, V}), A = view(cx.scratch("so_A", o2v2), {O, O, V, V});
    Tensor Bm = view(cx.scratch("so_B", o2v2), {O, O, V, V});
    Tensor Z = view(cx.scratch("eom_Z", O * O * V * O), {O, O, V, O});
    Tensor Roo = view(cx.scratch("eom_Roo", O * O * O * O), {O, O, O, O});
    // 1/2 r_ijef W_abef as so_ladder treats 1/2 tau_ijef W_abef: the bare part over antisymmetric pairs against va, the t1 parts through
    // Z(i,j,a,m) = 1/2 r_ijef <am||ef>, the tau part as (r . <mn||ef> over ef) -> o^4, then x tau;  + 1/2 H_mnij r_mnab
    so_ladder_bare(cx, s, r2, lad);
    C(0.5, r2, "ijef", s.vovv, "amef", 0.0, Z, "ijam");
    C(-1.0, Z, "ijam", t1, "mb", 1.0, lad, "ijab");
    C(1.0, Z, "ijbm", t1, "ma", 1.0, lad, "ijab");
    C(1.0, r2, "ijef", s.oovv, "mnef", 0.0, Roo, "ijmn");
    C(0.25, Roo, "ijmn", L.tau, "mnab", 1.0, lad, "ijab");
    C(0.5, L.Hoooo, "mnij", r2, "mnab", 1.0, lad, "ijab");
    // P(ij)P(ab) H_mbej r_imae
    C(1.0, r2, "imae", L.Hovvo, "mbej", 0.0, AB, "ijab");
    // P(ij) [ -H_mj r_imab + H_abej r_ie - Y_mj t_imab ]  (H_abej stored (j,e,a,b))
    C(-1.0, L.Hoo, "mj", r2, "imab", 0.0, A, "ijab");
    C(1.0, r1, "ie", L.Hvvvo, "jeab", 1.0, A, "ijab");
    C(-1.0, Yoo, "mj", t2, "imab", 1.0, A, "ijab");
    // P(ab) [ H_be r_ijae - H_mbij r_ma + Y_be t_ijae ]
    C(1.0, r2, "ijae", L.Hvv, "be", 0.0, Bm, "ijab");
    C(-1.0, L.Hovoo, "mbij", r1, "ma", 1.0, Bm, "ijab");
    C(1.0, t2, "ijae", Yvv, "be", 1.0, Bm, "ijab");
    LAUNCH(eom_sigma_assemble_kernel, grid_for(o2v2), sigma + ov, sigma, lad.d, AB.d, A.d, Bm.d, r2.d, r1.d, s.D2.d, s.D1.d, o, v);
}

void so_eom_sigma_host(Context& cx, SOState& s, int nvec, const double* r1, const double* r2, double* s1, double* s2)
{
    need_plain(cx);
    so_lambda_need(s, "afesp_ccsd_so_eom_sigma");
    if (nvec < 1 || !r1 || !r2 || !s1 || !s2) throw Error(1, "afesp_ccsd_so_eom_sigma: nvec < 1 or a NULL vector");
    const int64_t O = s.o, V = s.v, ov = O * V, o2v2 = O * O * V * V;
    double* r = cx.scratch("eom_r_stage", ov + o2v2);
    double* sg = cx.scratch("eom_s_stage", ov + o2v2);
    for (int k = 0; k < nvec; ++k) {
        AFESP_HIP(hipMemcpyAsync(r, r1 + ov * k, sizeof(double) * ov, hipMemcpyHostToDevice, cx.stream));
        AFESP_HIP(hipMemcpyAsync(r + ov, r2 + o2v2 * k, sizeof(double) * o2v2, hipMemcpyHostToDevice, cx.stream));
        so_eom_sigma(cx, s, r, sg);
        AFESP_HIP(hipMemcpyAsync(s1 + ov * k, sg, sizeof(double) * ov, hipMemcpyDeviceToHost, cx.stream));
        AFESP_HIP(hipMemcpyAsync(s2 + o2v2 * k, sg + ov, sizeof(double) * o2v2, hipMemcpyDeviceToHost, cx.stream));
        cx.sync();
    }
}

static void eom_restart(SOEom& E)
{
    E.nb = 0;
    E.npend = 0;
    E.ritz = false;
    E.user_guess = false;
    E.target.clear();
    E.nsigma = E.ncollapse = 0;
    std::fill(E.flags.begin(), E.flags.end(), 0);
}

void so_eom_guess(Context& cx, SOState& s, bool left)
{
    need_plain(cx);
    SOEom& E = so_eom_need(s, eom_name(left, "guess").c_str(), left);
    const int64_t O = s.o, V = s.v, ov = O * V, o2v2 = O * O * V * V;
    std::vector<double> D(ov + o2v2);
    AFESP_HIP(hipMemcpyAsync(D.data(), s.D1.d, sizeof(double) * ov, hipMemcpyDeviceToHost, cx.stream));
    AFESP_HIP(hipMemcpyAsync(D.data() + ov, s.D2.d, sizeof(double) * o2v2, hipMemcpyDeviceToHost, cx.stream));
    cx.sync();
    // the unique amplitudes by ascending -D, ties by flat index
    std::vector<int64_t> idx;
    idx.reserve(ov + (O * (O - 1) / 2) * (V * (V - 1) / 2));
    for (int64_t x = 0; x < ov; ++x) idx.push_back(x);
    for (int64_t b = 0; b < V; ++b)
        for (int64_t a = 0; a < b; ++a)
            for (int64_t j = 0; j < O; ++j)
                for (int64_t i = 0; i < j; ++i) idx.push_back(ov + i + O * (j + O * (a + V * b)));
    const int nr = E.nroots;
    std::partial_sort(idx.begin(), idx.begin() + nr, idx.end(), [&](int64_t p, int64_t q) { return -D[p] != -D[q] ? -D[p] < -D[q] : p < q; });
    eom_restart(E);
    for (int k = 0; k < nr; ++k) {
        int64_t i0 = idx[k], i1 = -1, i2 = -1, i3 = -1;
        if (i0 >= ov) {
            const int64_t x = i0 - ov, i = x % O, j = (x / O) % O, a = (x / (O * O)) % V, b = x / (O * O * V);
            i1 = ov + j + O * (i + O * (b + V * a));
            i2 = ov + j + O * (i + O * (a + V * b));
            i3 = ov + i + O * (j + O * (b + V * a));
        }
        LAUNCH(eom_unit_kernel, grid_for(E.nvec), E.pend + E.nvec * k, E.nvec, i0, i1, i2, i3);
    }
    E.npend = nr;
    cx.sync();
}

void so_eom_set_guess(Context& cx, SOState& s, int k, const double* r1, const double* r2, bool left)
{
    need_plain(cx);
    SOEom& E = so_eom_need(s, eom_name(left, "set_guess").c_str(), left);
    if (k < 0 || k >= E.nroots || !r1 || !r2) throw Error(1, eom_name(left, "set_guess") + ": k outside 0 .. nroots - 1, or a NULL vector");
    const int64_t ov = (int64_t)s.o * s.v;
    if (E.nb > 0 || !E.user_guess) {   // the first of a block of the caller's guesses starts over: a running iteration, the unit guesses
        eom_restart(E);
        k_fill(cx, E.pend, E.nvec * E.nroots, 0.0);   // (a column the caller leaves out stays zero and is dropped)
        E.user_guess = true;
    }
    AFESP_HIP(hipMemcpyAsync(E.pend + E.nvec * k, r1, sizeof(double) * ov, hipMemcpyHostToDevice, cx.stream));
    AFESP_HIP(hipMemcpyAsync(E.pend + E.nvec * k + ov, r2, sizeof(double) * (E.nvec - ov), hipMemcpyHostToDevice, cx.stream));
    cx.sync();
    E.npend = std::max(E.npend, k + 1);
}

int so_eom_iterate(Context& cx, SOState& s, double tol, bool left)
{
    need_plain(cx);
    const std::string who = eom_name(left, "iterate");
    SOEom& E = so_eom_need(s, who.c_str(), left);
    const int64_t n1 = (int64_t)s.o * s.v, nvec = E.nvec;
    const int ms = E.max_space;
    if (E.nb == 0 && E.npend == 0) throw Error(1, who + ": no guess vectors (call " + eom_name(left, "guess") + " or " + eom_name(left, "set_guess") + " first)");
    const bool guess_step = E.nb == 0;
    // ---- collapse: restart from the Ritz vectors, their sigma being the same combination of the stored sigma (no new sigma builds)
    if (E.nb + E.npend > ms) {
        const int nr = std::min(E.nroots, E.nb);
        E.nb = 0;
        for (int k = 0; k < nr; ++k)
            if (orthonormalise(cx, E, E.x + nvec * k, E.sx + nvec * k, n1)) extend_projected(cx, E, n1);
        ++E.ncollapse;
    }
    // ---- the pending vectors: orthonormalise, sigma, one more row and column of the projected matrix
    for (int k = 0; k < E.npend && E.nb < ms; ++k) {
        if (!orthonormalise(cx, E, E.pend + nvec * k, nullptr, n1)) continue;
        if (left) so_eom_lsigma(cx, s, E.B + nvec * E.nb, E.S + nvec * E.nb);   // the projected matrix is then <b_p, sigma_L(b_q)>
        else so_eom_sigma(cx, s, E.B + nvec * E.nb, E.S + nvec * E.nb);
        ++E.nsigma;
        extend_projected(cx, E, n1);
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
    // The roots taken: the lowest nr -- or, for the left state from the caller's guesses, those nearest to the Ritz values of its guess step,
    // target by target in their order, each root once, then by ascending omega.  A lower root of another symmetry, which only rounding
    // brings into the basis and the iteration then amplifies, takes no place that way.
    std::vector<int> sel(nr);
    std::iota(sel.begin(), sel.end(), 0);
    if (guess_step && left && E.user_guess) E.target.assign(wr.begin(), wr.begin() + nr);
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
    const int nblk = eom_nblk(nvec);
    for (int k0 = 0; k0 < nr; k0 += EOM_RCHUNK)
        LAUNCH(eom_ritz_kernel, dim3(nblk), E.x, E.sx, E.corr, E.partial, E.B, E.S, nvec, nb, E.coef, E.coef + (size_t)nb * nr, s.D1.d, s.D2.d, s.o, s.v,
               nvec, k0, std::min(EOM_RCHUNK, nr - k0));
    LAUNCH(eom_final_kernel, dim3(nr), E.sums, E.partial, nblk);
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

void so_eom_get_vector(Context& cx, SOState& s, int k, double* r1, double* r2, bool left)
{
    need_plain(cx);
    SOEom& E = so_eom_need(s, eom_name(left, "get_vector").c_str(), left);
    if (!E.ritz || k < 0 || k >= std::min(E.nroots, E.nb) || !r1 || !r2)
        throw Error(1, eom_name(left, "get_vector") + ": no Ritz vector k (iterate first; k in 0 .. nroots - 1), or a NULL vector");
    const int64_t ov = (int64_t)s.o * s.v;
    AFESP_HIP(hipMemcpyAsync(r1, E.x + E.nvec * k, sizeof(double) * ov, hipMemcpyDeviceToHost, cx.stream));
    AFESP_HIP(hipMemcpyAsync(r2, E.x + E.nvec * k + ov, sizeof(double) * (E.nvec - ov), hipMemcpyDeviceToHost, cx.stream));
    cx.sync();
}

}  // namespace afesp
