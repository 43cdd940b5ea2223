// ccsd_so.hip -- spin-orbital CCSD (Stanton, Gauss, Watts, Bartlett 1991 as coded in the reference's src/ccsd.f90).
// Every contraction the reference writes as reshape + dgemm or as a loop nest is one label-driven contract() here;
// the index letters are the reference's.
#include "device_util.h"
#include "fused.h"
#include "lambda_so.h"   // (ccsd_so.h, and the contractor() of the spin-orbital units)

#include <cmath>

namespace afesp {
namespace {

// ccsd.f90:108-143,193-207: out(p,q,r,s) = <p+b0 q+b1 || r+b2 s+b3> over spin orbitals x = 2 X + spin, from the packed
// chemist MO integrals: <pq|rs> = (PR|QS) [sp = sr][sq = ss]
__global__ void slice_asym_kernel(double* out, const double* packed, int d0, int d1, int d2, int d3, int b0, int b1, int b2, int b3)
{
    const int64_t n = (int64_t)d0 * d1 * d2 * d3;
    GRID_STRIDE(x, n)
    {
        const int p = (int)(x % d0) + b0;
        int64_t y = x / d0;
        const int q = (int)(y % d1) + b1;
        y /= d1;
        const int r = (int)(y % d2) + b2, s = (int)(y / d2) + b3;
        const int P = p >> 1, Q = q >> 1, R = r >> 1, S = s >> 1;
        double val = 0.0;
        if ((p & 1) == (r & 1) && (q & 1) == (s & 1)) val += packed[tri(tri(P, R), tri(Q, S))];
        if ((p & 1) == (s & 1) && (q & 1) == (r & 1)) val -= packed[tri(tri(P, S), tri(Q, R))];
        out[x] = val;
    }
}

// The same slices from the UHF blocks: spin orbital x is spatial orbital tab[x] / 2 of spin tab[x] & 1 (0 alpha, 1 beta; so_init_uhf),
// <pq|rs> = (PR|QS)_{sp sq} [sp = sr][sq = ss] read from aa (both alpha), bb (both beta) or ab (alpha-beta; beta-alpha transposed)
__device__ __forceinline__ double uhf_chem(const double* aa, const double* bb, const double* ab, int64_t np, int sl, int P, int R, int sr,
                                           int Q, int S)
{
    const int64_t pr = tri(P, R), qs = tri(Q, S);
    if (sl == sr) return (sl ? bb : aa)[tri(pr, qs)];
    return sl == 0 ? ab[pr * np + qs] : ab[qs * np + pr];
}
__global__ void slice_asym_uhf_kernel(double* out, const double* aa, const double* bb, const double* ab, const int* tab, int64_t np, int d0,
                                      int d1, int d2, int d3, int b0, int b1, int b2, int b3)
{
    const int64_t n = (int64_t)d0 * d1 * d2 * d3;
    GRID_STRIDE(x, n)
    {
        const int p = tab[(int)(x % d0) + b0];
        int64_t y = x / d0;
        const int q = tab[(int)(y % d1) + b1];
        y /= d1;
        const int r = tab[(int)(y % d2) + b2], s = tab[(int)(y / d2) + b3];
        const int sp = p & 1, sq = q & 1, sr = r & 1, ss = s & 1;
        double val = 0.0;
        if (sp == sr && sq == ss) val += uhf_chem(aa, bb, ab, np, sp, p >> 1, r >> 1, sq, q >> 1, s >> 1);
        if (sp == ss && sq == sr) val -= uhf_chem(aa, bb, ab, np, sp, p >> 1, s >> 1, sq, q >> 1, r >> 1);
        out[x] = val;
    }
}
// D from the level of every spin orbital (lev: occupied first)
__global__ void so_denominators_lev_kernel(double* D1, double* D2, const double* lev, int o, int v)
{
    const int64_t n2 = (int64_t)o * o * v * v, n1 = (int64_t)o * v;
    GRID_STRIDE(x, n2)
    {
        const auto [i, j, a, b] = oovv_decode(x, o, v);
        D2[x] = lev[i] + lev[j] - lev[o + a] - lev[o + b];
        if (x < n1) D1[x] = lev[(int)(x % o)] - lev[o + (int)(x / o)];
    }
}

// ccsd.f90:437-448
}  // namespace
static void preload_ccsd_so_fock();
void preload_ccsd_so()
{
    first_use_touch(reinterpret_cast<const void*>(slice_asym_kernel));
    first_use_touch(reinterpret_cast<const void*>(slice_asym_uhf_kernel));
    first_use_touch(reinterpret_cast<const void*>(so_denominators_lev_kernel));
    (void)hipGetLastError();
    preload_ccsd_so_fock();
}
namespace {
__global__ void so_denominators_kernel(double* D1, double* D2, const double* e, int o, int v)
{
    const int64_t n2 = (int64_t)o * o * v * v, n1 = (int64_t)o * v;
    const int os = o / 2;
    GRID_STRIDE(x, n2)
    {
        const auto [i, j, a, b] = oovv_decode(x, o, v);
        D2[x] = e[i / 2] + e[j / 2] - e[a / 2 + os] - e[b / 2 + os];
        if (x < n1) D1[x] = e[(int)(x % o) / 2] - e[(int)(x / o) / 2 + os];
    }
}

// ccsd.f90:678-714
__global__ void so_tau_kernel(double* tau, double* tau_t, const double* t1, const double* t2, int o, int v, double* t1_w)
{
    const int64_t n2 = (int64_t)o * o * v * v;
    GRID_STRIDE(x, n2)
    {
        if (x < (int64_t)o * v) t1_w[x] = t1[x];   // the t1 these intermediates belong to (so_build_W_vvvv forms W_abef from it on request)
        const auto [i, j, a, b] = oovv_decode(x, o, v);
        const double y = t1[i + o * a] * t1[j + o * b] - t1[i + o * b] * t1[j + o * a];
        const double tt = t2[x] + 0.5 * y;
        tau_t[x] = tt;
        tau[x] = tt + 0.5 * y;
    }
}

// ccsd.f90:877-887: scratch(n,f,j,b) = 1/2 t2(j,n,f,b) + t1(j,f) t1(n,b)
__global__ void so_ring_operand_kernel(double* out, const double* t1, const double* t2, int o, int v)
{
    const int64_t n2 = (int64_t)o * v * o * v;
    GRID_STRIDE(x, n2)
    {
        const int n = (int)(x % o), f = (int)((x / o) % v), j = (int)((x / ((int64_t)o * v)) % o), b = (int)(x / ((int64_t)o * v * o));
        out[x] = 0.5 * t2[j + (int64_t)o * (n + (int64_t)o * (f + (int64_t)v * b))] + t1[j + o * f] * t1[n + o * b];
    }
}

// ccsd.f90:1783-1806 (unrestricted branch): out[0] = 1/4 sum <ij||ab> (t2 + 2 t1 t1), out[1] = sum (t2 - t2_old)^2;
// t2_old <- t2.  One block-partial per block, summed by so_sum2.
__global__ void so_energy_kernel(double* partial, const double* oovv, const double* t1, const double* t2, double* t2_old, int o, int v)
{
    __shared__ double red[2 * 4];
    const int64_t n2 = (int64_t)o * o * v * v;
    double e = 0.0, r = 0.0;
    GRID_STRIDE(x, n2)
    {
        const auto [i, j, a, b] = oovv_decode(x, o, v);
        const double t = t2[x];
        e += 0.25 * oovv[x] * (t + 2.0 * t1[i + o * a] * t1[j + o * b]);
        const double d = t - t2_old[x];
        r += d * d;
        t2_old[x] = t;
    }
    double s[2] = {e, r};
    block_sum_down<2>(s, red);
    if (threadIdx.x == 0) {
        partial[blockIdx.x] = s[0];
        partial[gridDim.x + blockIdx.x] = s[1];
    }
}

// out[b] = sum of partial[b nblk .. (b + 1) nblk) in a fixed order; block 0 adds sum f(x) l1(x) where f is given (the Lambda pseudo energy)
__global__ void so_sum2_kernel(double* out, const double* partial, int nblk, const double* f_ov, const double* l1, int64_t n1)
{
    __shared__ double red[TB];
    const double* p = partial + (int64_t)blockIdx.x * nblk;
    double s = 0.0;
    for (int x = threadIdx.x; x < nblk; x += TB) s += p[x];
    if (blockIdx.x == 0 && f_ov)
        for (int64_t x = threadIdx.x; x < n1; x += TB) s += f_ov[x] * l1[x];
    block_tree_sum(s, red);
    if (threadIdx.x == 0) out[blockIdx.x] = red[0];
}

// ccsd.f90:969-1034 assembled in one pass: r2 holds the two ladder terms; AB carries P(ij)P(ab), A carries P(ij), Bm
// carries P(ab):  t2 = [<ij||ab> + r2 + P(ij)P(ab) AB + P(ij) A + P(ab) Bm] / D
__global__ void so_t2_assemble_kernel(double* t2, const double* r2, const double* oovv, const double* AB, const double* A, const double* Bm,
                                      const double* D2, int o, int v)
{
    const int64_t n2 = (int64_t)o * o * v * v;
    GRID_STRIDE(x, n2)
    {
        const auto [i, j, a, b] = oovv_decode(x, o, v);
        const auto [ji, ba, jiba] = oovv_images(i, j, a, b, o, v);
        const double val = oovv[x] + r2[x] + (AB[x] - AB[ji] - AB[ba] + AB[jiba]) + (A[x] - A[ji]) + (Bm[x] - Bm[ba]);
        t2[x] = val / D2[x];
    }
}

// F_oo helper: G(m,i) = F_oo(m,i) + 1/2 Y(i,m)
__global__ void so_g_kernel(double* G, const double* F_oo, const double* Y, int o)
{
    GRID_STRIDE(x, (int64_t)o * o)
    {
        const int m = (int)(x % o), i = (int)(x / o);
        G[x] = F_oo[x] + 0.5 * Y[i + o * m];
    }
}

// ---- the Fock terms of a state with a full Fock matrix (so_init_fock), Stanton et al. Eqs. 3-5: the element-wise parts
// F_vv(a,e) += f_ae (a != e; the diagonal of f_vv is stored as zero), F_oo(m,i) += f_mi likewise, F_ov(m,e) += f_me
__global__ void so_fock_f_kernel(double* F_vv, double* F_oo, double* F_ov, const double* f_vv, const double* f_oo, const double* f_ov, int o, int v)
{
    const int64_t nvv = (int64_t)v * v, noo = (int64_t)o * o, nov = (int64_t)o * v;
    GRID_STRIDE(x, nvv + noo + nov)
    {
        if (x < nvv) F_vv[x] += f_vv[x];
        else if (x < nvv + noo) F_oo[x - nvv] += f_oo[x - nvv];
        else F_ov[x - nvv - noo] += f_ov[x - nvv - noo];
    }
}
// y += x (the f_ia of the T1 residual, Eq. 1)
__global__ void so_add_kernel(double* y, const double* x, int64_t n)
{
    GRID_STRIDE(i, n) y[i] += x[i];
}
// out[0] += sum f_ia t_ia behind so_energy_kernel / so_sum2_kernel: one block, a fixed order (a launch of its own: inside so_sum2_kernel
// the terms would join the partials before the tree, another order of the published energy)
__global__ void so_energy_fock_kernel(double* out, const double* f_ov, const double* t1, int64_t n)
{
    __shared__ double red[TB];
    double s = 0.0;
    for (int64_t x = threadIdx.x; x < n; x += TB) s += f_ov[x] * t1[x];
    block_tree_sum(s, red);
    if (threadIdx.x == 0) out[0] += red[0];
}
// partial[block] = sum f_ia^2 / D_ia (x < o v) + 1/4 sum <ij||ab>^2 / D_ijab over the block's elements; summed by so_sum2_kernel
__global__ void so_mp2_fock_kernel(double* partial, const double* oovv, const double* D2, const double* f_ov, const double* D1, int o, int v)
{
    __shared__ double red[TB];
    const int64_t n2 = (int64_t)o * o * v * v, n1 = (int64_t)o * v;
    double e = 0.0;
    GRID_STRIDE(x, n2)
    {
        e += 0.25 * oovv[x] * oovv[x] / D2[x];
        if (x < n1) e += f_ov[x] * f_ov[x] / D1[x];
    }
    block_tree_sum(e, red);
    if (threadIdx.x == 0) partial[blockIdx.x] = red[0];
}

// va(ef, ab) = <ab||ef>, e < f, a < b, leading dimension ka
__global__ void so_vvvv_asympack_kernel(double* va, const double* vvvv, int v, int64_t ka)
{
    const int64_t V = v, np = V * (V - 1) / 2;
    GRID_STRIDE(x, np * np)
    {
        int e, f, a, b;
        unpair_lt(x % np, e, f);
        unpair_lt(x / np, a, b);
        va[x % np + ka * (x / np)] = vvvv[a + V * (b + V * (e + V * f))];
    }
}
// ta(ij, ef) = tau(i,j,e,f), i < j, e < f, leading dimension na
__global__ void so_tau_asympack_kernel(double* ta, const double* tau, int o, int v, int64_t na)
{
    const int64_t O = o, V = v, npo = O * (O - 1) / 2, npv = V * (V - 1) / 2;
    GRID_STRIDE(x, npo * npv)
    {
        int i, j, e, f;
        unpair_lt(x % npo, i, j);
        unpair_lt(x / npo, e, f);
        ta[x % npo + na * (x / npo)] = tau[i + O * (j + O * (e + V * f))];
    }
}
// r2(i,j,a,b) = +- pa(ij, ab): + for (i < j, a < b) and (j < i, b < a), - when exactly one pair is exchanged, 0 on the diagonals
__global__ void so_ladder_expand_kernel(double* r2, const double* pa, int o, int v, int64_t na)
{
    const int64_t n2 = (int64_t)o * o * v * v;
    GRID_STRIDE(x, n2)
    {
        const auto [i, j, a, b] = oovv_decode(x, o, v);
        double val = 0.0;
        if (i != j && a != b) {
            const int il = min(i, j), ih = max(i, j), al = min(a, b), ah = max(a, b);
            const double p = pa[(int64_t)ih * (ih - 1) / 2 + il + na * ((int64_t)ah * (ah - 1) / 2 + al)];
            val = ((i < j) == (a < b)) ? p : -p;
        }
        r2[x] = val;
    }
}

}  // namespace
// ... and the kernels only a state with a full Fock matrix launches (so_init_fock)
static void preload_ccsd_so_fock()
{
    first_use_touch(reinterpret_cast<const void*>(so_fock_f_kernel));
    first_use_touch(reinterpret_cast<const void*>(so_add_kernel));
    first_use_touch(reinterpret_cast<const void*>(so_energy_fock_kernel));
    first_use_touch(reinterpret_cast<const void*>(so_mp2_fock_kernel));
    (void)hipGetLastError();
}
namespace {
// an element-wise kernel over n elements; nothing where there are none (a state without an occupied or a virtual pair)
#define SO_LAUNCH(kernel, n, ...)                                                \
    do {                                                                         \
        if ((n) > 0) LAUNCH(kernel, grid_for(n, SO_GRID_CAP), __VA_ARGS__);      \
    } while (0)

// ... or, while a call sequence is being recorded for the levelled path (fused.h), noted with the memory it reads and writes (replayed on
// the context it is given, which LAUNCH reads as `cx`)
#define SO_KERNEL(READS, WRITES, kernel, n, ...)                                                                                     \
    do {                                                                                                                             \
        if (cx.rec) {                                                                                                                \
            if ((n) > 0)                                                                                                             \
                cx.rec->opaque(READS, WRITES, [=](Context& cx) { LAUNCH(kernel, grid_for(n, SO_GRID_CAP), __VA_ARGS__); });          \
        } else {                                                                                                                     \
            SO_LAUNCH(kernel, n, __VA_ARGS__);                                                                                       \
        }                                                                                                                            \
    } while (0)
#define FR(p, n) frange(p, n)
typedef std::vector<FusedRange> Ranges;

}  // namespace

static void so_init_tail(Context& cx, SOState& s, int diis_nerr);

void so_init(Context& cx, SOState& s, int nbasis, int nel, const double* eri_mo_dev, const double* e_host, int diis_nerr,
             bool foo_as_published)
{
    if (nbasis <= 0 || nel <= 0 || (nel & 1) || nel >= 2 * nbasis)
        throw Error(1, "ccsd_so_init: need an even electron count with at least one occupied and one virtual spatial orbital");
    so_free(cx, s);
    const int o = nel, v = 2 * nbasis - nel;
    s.o = o; s.v = v; s.n = nbasis;
    s.foo_as_published = foo_as_published;
    const int64_t O = o, V = v, o2v2 = O * O * V * V;
    s.e = cx.alloc(nbasis);
    AFESP_HIP(hipMemcpyAsync(s.e, e_host, sizeof(double) * nbasis, hipMemcpyHostToDevice, cx.stream));
    cx.sync();
    s.oooo = cx.tensor({O, O, O, O}); s.ooov = cx.tensor({O, O, O, V}); s.ovoo = cx.tensor({O, V, O, O});
    s.oovo = cx.tensor({O, O, V, O}); s.oovv = cx.tensor({O, O, V, V}); s.ovvo = cx.tensor({O, V, V, O});
    s.ovvv = cx.tensor({O, V, V, V}); s.vovv = cx.tensor({V, O, V, V}); s.vvvv = cx.tensor({V, V, V, V});
    auto slice = [&](const Tensor& t, int b0, int b1, int b2, int b3) {
        SO_LAUNCH(slice_asym_kernel, t.size(), t.d, eri_mo_dev, (int)t.dim[0], (int)t.dim[1], (int)t.dim[2], (int)t.dim[3], b0, b1, b2, b3);
    };
    slice(s.oooo, 0, 0, 0, 0); slice(s.ooov, 0, 0, 0, o); slice(s.ovoo, 0, o, 0, 0); slice(s.oovo, 0, 0, o, 0);
    slice(s.oovv, 0, 0, o, o); slice(s.ovvo, 0, o, o, 0); slice(s.ovvv, 0, o, o, o); slice(s.vovv, o, 0, o, o);
    slice(s.vvvv, o, o, o, o);
    s.D1 = cx.tensor({O, V}); s.D2 = cx.tensor({O, O, V, V});
    SO_LAUNCH(so_denominators_kernel, o2v2, s.D1.d, s.D2.d, s.e, o, v);
    so_init_tail(cx, s, diis_nerr);
}

// what follows the integrals and the denominators, for either source
static void so_init_tail(Context& cx, SOState& s, int diis_nerr)
{
    const int o = s.o, v = s.v;
    const int64_t O = o, V = v, ov = O * V, o2v2 = O * O * V * V;
    s.nvec = ov + o2v2;
    s.amp = cx.alloc(s.nvec);
    s.t1 = view(s.amp, {O, V}); s.t2 = view(s.amp + ov, {O, O, V, V});
    double* res = cx.alloc(s.nvec);
    s.r1 = view(res, {O, V}); s.r2 = view(res + ov, {O, O, V, V});
    s.t2_old = cx.tensor({O, O, V, V});
    s.F_vv = cx.tensor({V, V}); s.F_oo = cx.tensor({O, O}); s.F_ov = cx.tensor({O, V});
    s.W_oooo = cx.tensor({O, O, O, O}); s.W_ovvo = cx.tensor({O, V, V, O});   // (W_vvvv: so_build_W_vvvv, on request only)
    {
        // the bare part of 1/2 tau W_abef over antisymmetric pairs (so_ladder)
        auto even = [](int64_t x) { return (x + 1) & ~(int64_t)1; };
        const int64_t npv = V * (V - 1) / 2, npo = O * (O - 1) / 2, ka = even(std::max<int64_t>(npv, 1)), na = even(std::max<int64_t>(npo, 1));
        s.lad_ka = ka; s.lad_na = na;
        if (npv > 0 && npo > 0) {
            s.va = cx.alloc(ka * npv); s.ta = cx.alloc(na * ka); s.pa = cx.alloc(na * npv);
            SO_LAUNCH(so_vvvv_asympack_kernel, npv * npv, s.va, s.vvvv.d, v, ka);
            // [ k (also n) | ka*m | na*k | na*m ]
            std::vector<int64_t> tab;
            const int64_t kn = std::max(ka, na);
            for (int64_t k = 0; k < kn; ++k) tab.push_back(k);
            for (int64_t m = 0; m < npv; ++m) tab.push_back(ka * m);
            for (int64_t k = 0; k < ka; ++k) tab.push_back(na * k);
            for (int64_t m = 0; m < npv; ++m) tab.push_back(na * m);
            s.lad_tab = cx.alloc_i64((int64_t)tab.size());
            AFESP_HIP(hipMemcpyAsync(s.lad_tab, tab.data(), tab.size() * sizeof(int64_t), hipMemcpyHostToDevice, cx.stream));
            cx.sync();
        }
    }
    s.tau = cx.tensor({O, O, V, V}); s.tau_t = cx.tensor({O, O, V, V}); s.t1_w = cx.tensor({O, V});
    k_div(cx, s.t2.d, s.oovv.d, s.D2.d, o2v2);   // ccsd.f90:516 (t1 = 0 from the zero-filled allocation, :472)
    diis_alloc(cx, s, diis_nerr);
    s.energy = s.energy_old = s.rms = 0.0;
    s.ready = true;
    cx.sync();
}

void so_init_uhf(Context& cx, SOState& s, int nbasis, int na, int nb, const double* aa, const double* bb, const double* ab,
                 const double* ea_host, const double* eb_host, int diis_nerr)
{
    if (nbasis <= 0 || na < 0 || nb < 0 || na > nbasis || nb > nbasis || na + nb <= 0 || na + nb >= 2 * nbasis)
        throw Error(1, "ccsd_uso_init: need 0 <= nalpha, nbeta <= nbasis with at least one occupied and one virtual spin orbital");
    so_free(cx, s);
    const int n = nbasis, o = na + nb, v = 2 * nbasis - o;
    s.o = o; s.v = v; s.n = nbasis;
    s.foo_as_published = true;
    const int64_t O = o, V = v, o2v2 = O * O * V * V, np = (int64_t)n * (n + 1) / 2;
    // spin-orbital table (2 orbital + spin) and levels, in the order of the header
    std::vector<int> tab((size_t)(o + v));
    std::vector<double> lev((size_t)(o + v));
    for (int x = 0; x < o + v; ++x) {
        int orb, sp;
        if (x < na) { orb = x; sp = 0; }
        else if (x < o) { orb = x - na; sp = 1; }
        else if (x < o + n - na) { orb = na + (x - o); sp = 0; }
        else { orb = nb + (x - o - (n - na)); sp = 1; }
        tab[(size_t)x] = 2 * orb + sp;
        lev[(size_t)x] = sp ? eb_host[orb] : ea_host[orb];
    }
    s.lev = cx.alloc(O + V);
    AFESP_HIP(hipMemcpyAsync(s.lev, lev.data(), sizeof(double) * (O + V), hipMemcpyHostToDevice, cx.stream));
    int* tab_dev = (int*)cx.scratch("so_uhf_tab", (O + V + 1) / 2 + 1);
    AFESP_HIP(hipMemcpyAsync(tab_dev, tab.data(), sizeof(int) * (O + V), hipMemcpyHostToDevice, cx.stream));
    s.oooo = cx.tensor({O, O, O, O}); s.ooov = cx.tensor({O, O, O, V}); s.ovoo = cx.tensor({O, V, O, O});
    s.oovo = cx.tensor({O, O, V, O}); s.oovv = cx.tensor({O, O, V, V}); s.ovvo = cx.tensor({O, V, V, O});
    s.ovvv = cx.tensor({O, V, V, V}); s.vovv = cx.tensor({V, O, V, V}); s.vvvv = cx.tensor({V, V, V, V});
    auto slice = [&](const Tensor& t, int b0, int b1, int b2, int b3) {
        SO_LAUNCH(slice_asym_uhf_kernel, t.size(), t.d, aa, bb, ab, tab_dev, np, (int)t.dim[0], (int)t.dim[1], (int)t.dim[2], (int)t.dim[3],
                  b0, b1, b2, b3);
    };
    slice(s.oooo, 0, 0, 0, 0); slice(s.ooov, 0, 0, 0, o); slice(s.ovoo, 0, o, 0, 0); slice(s.oovo, 0, 0, o, 0);
    slice(s.oovv, 0, 0, o, o); slice(s.ovvo, 0, o, o, 0); slice(s.ovvv, 0, o, o, o); slice(s.vovv, o, 0, o, o);
    slice(s.vvvv, o, o, o, o);
    s.D1 = cx.tensor({O, V}); s.D2 = cx.tensor({O, O, V, V});
    SO_LAUNCH(so_denominators_lev_kernel, o2v2, s.D1.d, s.D2.d, s.lev, o, v);
    cx.sync();   // (the host images of the table and the levels)
    so_init_tail(cx, s, diis_nerr);
}

static double so_init_fock_terms(Context& cx, SOState& s, int n, int na, int nb, const double* fa_host, const double* fb_host);
double so_init_fock(Context& cx, SOState& s, int nbasis, int na, int nb, const double* aa, const double* bb, const double* ab,
                    const double* fa_host, const double* fb_host, int diis_nerr)
{
    const int n = nbasis;
    std::vector<double> ea((size_t)std::max(n, 1)), eb((size_t)std::max(n, 1));
    for (int p = 0; p < n; ++p) {
        ea[(size_t)p] = fa_host[p + (int64_t)n * p];
        eb[(size_t)p] = fb_host[p + (int64_t)n * p];
    }
    so_init_uhf(cx, s, nbasis, na, nb, aa, bb, ab, ea.data(), eb.data(), diis_nerr);   // (checks the extents)
    // so_init_uhf leaves a ready state WITHOUT the Fock terms: it must not survive a failure of what follows
    s.ready = false;
    try {
        return so_init_fock_terms(cx, s, nbasis, na, nb, fa_host, fb_host);
    } catch (...) {
        try { so_free(cx, s); } catch (...) {}
        throw;
    }
}

static double so_init_fock_terms(Context& cx, SOState& s, int n, int na, int nb, const double* fa_host, const double* fb_host)
{
    const int o = s.o, v = s.v;
    const int64_t O = o, V = v, ov = O * V, o2v2 = O * O * V * V;
    // spin orbital x of the state: (orbital, spin), in so_init_uhf's order
    auto orb_of = [&](int x, int& orb, int& sp) {
        if (x < na) { orb = x; sp = 0; }
        else if (x < o) { orb = x - na; sp = 1; }
        else if (x < o + n - na) { orb = na + (x - o); sp = 0; }
        else { orb = nb + (x - o - (n - na)); sp = 1; }
    };
    auto f_of = [&](int x, int y) {
        int px, sx, py, sy;
        orb_of(x, px, sx);
        orb_of(y, py, sy);
        if (sx != sy) return 0.0;
        return (sx ? fb_host : fa_host)[px + (int64_t)n * py];
    };
    std::vector<double> fov((size_t)ov), foo((size_t)(O * O)), fvv((size_t)(V * V));
    double off = 0.0;
    for (int a = 0; a < v; ++a)
        for (int i = 0; i < o; ++i) fov[(size_t)(i + O * a)] = f_of(i, o + a);
    for (int i = 0; i < o; ++i)
        for (int m = 0; m < o; ++m) {
            const double x = m == i ? 0.0 : f_of(m, i);
            foo[(size_t)(m + O * i)] = x;
            off = std::max(off, std::fabs(x));
        }
    for (int e = 0; e < v; ++e)
        for (int a = 0; a < v; ++a) {
            const double x = a == e ? 0.0 : f_of(o + a, o + e);
            fvv[(size_t)(a + V * e)] = x;
            off = std::max(off, std::fabs(x));
        }
    s.f_ov = cx.tensor({O, V}); s.f_oo = cx.tensor({O, O}); s.f_vv = cx.tensor({V, V});
    AFESP_HIP(hipMemcpyAsync(s.f_ov.d, fov.data(), sizeof(double) * ov, hipMemcpyHostToDevice, cx.stream));
    AFESP_HIP(hipMemcpyAsync(s.f_oo.d, foo.data(), sizeof(double) * O * O, hipMemcpyHostToDevice, cx.stream));
    AFESP_HIP(hipMemcpyAsync(s.f_vv.d, fvv.data(), sizeof(double) * V * V, hipMemcpyHostToDevice, cx.stream));
    s.fock = true;
    s.f_offdiag = off;
    k_div(cx, s.t1.d, s.f_ov.d, s.D1.d, ov);   // t1 = f_ia / D_ia beside so_init_tail's t2 = <ij||ab> / D_ijab
    const int nblk = (int)std::min<int64_t>((o2v2 + TB - 1) / TB, 1024);
    double e2 = 0.0;
    if (o2v2 > 0) {
        double* partial = cx.scratch("so_energy_partial", 2 * 1024);
        LAUNCH(so_mp2_fock_kernel, nblk, partial, s.oovv.d, s.D2.d, s.f_ov.d, s.D1.d, o, v);
        so_sum2(cx, cx.scal, partial, 1, nblk);
        e2 = host_scalars(cx, 1)[0];
    }
    cx.sync();   // (the host images of the Fock blocks)
    s.ready = true;
    return e2;
}

double so_state_bytes(int64_t o, int64_t v, int diis_nerr)
{
    const double O = (double)o, V = (double)v, npv = V * (V - 1) / 2;
    // slices, the W_abef pair operand va, the o^2 v^2 tensors of the state and the iteration's scratch, the DIIS history, and the
    // (T) operands (vt / tt / vs)
    const double doubles = V * V * V * V + 2 * O * V * V * V + O * O * O * O + 4 * O * O * O * V + npv * npv + (16.0 + 2.0 * diis_nerr) * O * O * V * V +
                           (V + O + 16) * (V * V * O + V * O * O) + O * O * O * V + (V * V + O * O + O * V);   // (last: f_vv, f_oo, f_ov of so_init_fock)
    return 8.0 * doubles;
}

void so_free(Context& cx, SOState& s)
{
    if (!s.o) return;
    double* bufs[] = {s.e, s.lev, s.oooo.d, s.ooov.d, s.ovoo.d, s.oovo.d, s.oovv.d, s.ovvo.d, s.ovvv.d, s.vovv.d, s.vvvv.d, s.D1.d,
                      s.D2.d, s.amp, s.r1.d, s.t2_old.d, s.F_vv.d, s.F_oo.d, s.F_ov.d, s.W_oooo.d, s.W_vvvv.d, s.W_ovvo.d,
                      s.tau.d, s.tau_t.d, s.amp_s, s.hist_t, s.hist_e, s.coef, s.bmat, s.va, s.ta, s.pa, (double*)s.lad_tab, s.t1_w.d,
                      s.f_ov.d, s.f_oo.d, s.f_vv.d};
    for (double* b : bufs) cx.release(b);
    cx.drop_scratch();
    so_triples_plan_free(s);
    so_lambda_free(cx, s);
    s = SOState();
}

void so_intermediates(Context& cx, SOState& s)
{
    const auto C = contractor(cx);
    auto P = [&](double al, const Tensor& in, const char* li, double be, const Tensor& out, const char* lo) {
        permute_add(cx, al, in, li, be, out, lo);
    };
    const int o = s.o, v = s.v;
    const int64_t O = o, V = v;
    SO_KERNEL((Ranges{FR(s.t1.d, O * V), FR(s.t2.d, s.t2.size())}), (Ranges{FR(s.tau.d, s.t2.size()), FR(s.tau_t.d, s.t2.size()), FR(s.t1_w.d, O * V)}),
              so_tau_kernel, s.t2.size(), s.tau.d, s.tau_t.d, s.t1.d, s.t2.d, o, v, s.t1_w.d);
    // ---- build_F, ccsd.f90:716-797
    C(1.0, s.ovvv, "mafe", s.t1, "mf", 0.0, s.F_vv, "ae");             // :749-759
    C(0.5, s.tau_t, "mnaf", s.oovv, "mnfe", 1.0, s.F_vv, "ae");        // :783-786 (tmp_4_1(a,m,n,f) = tau~(m,n,a,f))
    C(-1.0, s.ooov, "nmie", s.t1, "ne", 0.0, s.F_oo, "mi");            // :757-767
    // :789-794: dgemm('N','N',nocc,nocc,...,tau_tilde,tmp_4_1,F_oo) yields C(i,m) = 1/2 sum tau~(i,n,e,f) <mn||ef>
    // and adds it to F_oo(i,m) although F_oo is read as (m,i) everywhere; kept as coded unless the context asks for
    // Stanton's Eq. 4 order, which is what the reference's shipped ref_out (2022) was computed with.
    C(0.5, s.tau_t, "inef", s.oovv, "mnef", 1.0, s.F_oo, s.foo_as_published ? "mi" : "im");
    C(1.0, s.oovv, "mnef", s.t1, "nf", 0.0, s.F_ov, "me");             // :770-780
    if (s.fock) {   // Stanton Eqs. 3-5 with f: F_ae += (1 - d_ae) f_ae - 1/2 f_me t_ma, F_mi += (1 - d_mi) f_mi + 1/2 t_ie f_me, F_me += f_me
        C(-0.5, s.t1, "ma", s.f_ov, "me", 1.0, s.F_vv, "ae");
        C(0.5, s.f_ov, "me", s.t1, "ie", 1.0, s.F_oo, "mi");
        SO_KERNEL((Ranges{FR(s.f_vv.d, V * V), FR(s.f_oo.d, O * O), FR(s.f_ov.d, O * V), FR(s.F_vv.d, V * V), FR(s.F_oo.d, O * O), FR(s.F_ov.d, O * V)}),
                  (Ranges{FR(s.F_vv.d, V * V), FR(s.F_oo.d, O * O), FR(s.F_ov.d, O * V)}), so_fock_f_kernel, V * V + O * O + O * V, s.F_vv.d,
                  s.F_oo.d, s.F_ov.d, s.f_vv.d, s.f_oo.d, s.f_ov.d, o, v);
    }
    // ---- build_W, ccsd.f90:799-905
    // Eq. 6, stored W(i,j,m,n) (:842-846)
    Tensor sc = view(cx.scratch("so_sc_oooo", O * O * O * O), {O, O, O, O});
    C(1.0, s.ooov, "mnie", s.t1, "je", 0.0, sc, "mnij");               // :826
    P(1.0, s.oooo, "mnij", 0.0, s.W_oooo, "ijmn");
    P(1.0, sc, "mnij", 1.0, s.W_oooo, "ijmn");
    P(-1.0, sc, "mnji", 1.0, s.W_oooo, "ijmn");                        // :827-828
    C(0.5, s.oovv, "mnef", s.tau, "ijef", 1.0, s.W_oooo, "ijmn");      // :832-836
    // Eq. 7, W_abef (:852-861), is not stored: so_amplitudes contracts tau with its three terms one by one (so_ladder)
    // Eq. 8 (:866-902)
    k_copy(cx, s.W_ovvo.d, s.ovvo.d, s.ovvo.size());
    C(1.0, s.ovvv, "mbef", s.t1, "jf", 1.0, s.W_ovvo, "mbej");         // :867
    C(1.0, s.t1, "nb", s.oovo, "nmej", 1.0, s.W_ovvo, "mbej");         // :871-877
    Tensor ro = view(cx.scratch("so_ring_operand", O * V * O * V), {O, V, O, V});
    SO_KERNEL((Ranges{FR(s.t1.d, O * V), FR(s.t2.d, s.t2.size())}), (Ranges{FR(ro.d, ro.size())}), so_ring_operand_kernel, ro.size(), ro.d, s.t1.d,
              s.t2.d, o, v);
    C(-1.0, s.oovv, "mnef", ro, "nfjb", 1.0, s.W_ovvo, "mbej");        // :883-901
}

// W_abef = <ab||ef> - P(ab) t(m,b) <ma||ef> as a tensor W(e,f,a,b) (ccsd.f90:852-861): tests / afesp_ccsd_so_get_tensor only
void so_build_W_vvvv(Context& cx, SOState& s)
{
    const int64_t V = s.v;
    if (!s.W_vvvv.d) s.W_vvvv = cx.tensor({V, V, V, V});
    Tensor sv = view(cx.scratch("so_sc_vvvv", V * V * V * V), {V, V, V, V});
    contract(cx, 1.0, s.t1_w, "mb", s.ovvv, "maef", 0.0, sv, "baef");             // :853 (t1 as of the last so_intermediates)
    permute_add(cx, 1.0, s.vvvv, "abef", 0.0, s.W_vvvv, "efab");
    permute_add(cx, 1.0, sv, "baef", 1.0, s.W_vvvv, "efab");                      // + reshape_scratch(a,b,e,f) = scratch(b,a,e,f)
    permute_add(cx, -1.0, sv, "abef", 1.0, s.W_vvvv, "efab");                     // - scratch(a,b,e,f)
}

// r2(ijab) = 1/2 sum_ef tau(ijef) W(efab) (ccsd.f90:1021-1024) without forming W_abef -- at the H2O/cc-pVTZ shape (v = 106 spin
// orbitals) building it was three permuting passes over v^4 = 1 GB plus a v^4 scratch, 2.6 of the 4.3 ms of an iteration, and the
// product read it once more.  With W(efab) = <ab||ef> + t(m,b) <ma||ef> - t(m,a) <mb||ef>:
//   bare part   sum_{e<f} tau(ijef) <ab||ef> for i < j, a < b only -- tau and the integrals are antisymmetric in each pair -- one
//               product over pair indices, an eighth of the o^2 v^4 multiply-adds, against va(ef, ab) built once (so_init);
//   t1 parts    1/2 sum_m [ t(m,b) Z(ijma) - t(m,a) Z(ijmb) ],  Z(ijma) = sum_ef tau(ijef) <ma||ef>  (o^3 v^3 and two K = o products).
// the bare part: out(ijab) = sum_{e<f} x(ijef) <ab||ef> for any x antisymmetric in each pair (tau here; lambda_2 in lambda_so.hip, whose
// 1/2 l_ijef <ef||ab> it is)
void so_ladder_bare(Context& cx, SOState& s, const Tensor& x, const Tensor& out)
{
    const int o = s.o, v = s.v;
    const int64_t O = o, V = v, npv = V * (V - 1) / 2, npo = O * (O - 1) / 2, ka = s.lad_ka, na = s.lad_na;
    if (npv == 0 || npo == 0) {
        k_fill(cx, out.d, out.size(), 0.0);
    } else {
        SO_KERNEL((Ranges{FR(x.d, x.size())}), (Ranges{FR(s.ta, na * ka)}), so_tau_asympack_kernel, npo * npv, s.ta, x.d, o, v, na);
        const int64_t* t = s.lad_tab;
        const int64_t kn = std::max(ka, na);
        GettProblem gp;
        gp.alpha = 1.0; gp.beta = 0.0;
        gp.nbatch = 1; gp.batchA = gp.batchB = gp.batchC = nullptr;
        gp.a_kcontig = true; gp.b_kcontig = false;
        gp.wide = true;
        gp.A = s.va; gp.B = s.ta; gp.C = s.pa;
        gp.offAk = t; gp.offBn = gp.offCn = t;
        gp.offAm = t + kn; gp.offBk = t + kn + npv; gp.offCm = t + kn + npv + ka;
        gp.M = (int)npv; gp.N = (int)na; gp.K = (int)ka;
        if (cx.rec) cx.rec->product(gp, ka * npv, na * ka, na * npv);
        else AFESP_HIP(gett_launch(gp, cx.ws, cx.stream));
        SO_KERNEL((Ranges{FR(s.pa, na * npv)}), (Ranges{FR(out.d, out.size())}), so_ladder_expand_kernel, out.size(), out.d, s.pa, o, v, na);
    }
}

// xa(ij, ef) = x(i,j,e,f), i < j, e < f, in the layout of ta (leading dimension lad_na): the ladder's packer on a caller's buffer
void so_pair_pack(Context& cx, SOState& s, const Tensor& x, double* xa)
{
    const int64_t O = s.o, V = s.v, npv = V * (V - 1) / 2, npo = O * (O - 1) / 2;
    SO_KERNEL((Ranges{FR(x.d, x.size())}), (Ranges{FR(xa, s.lad_na * npv)}), so_tau_asympack_kernel, npo * npv, xa, x.d, s.o, s.v, s.lad_na);
}

static void so_ladder(Context& cx, SOState& s)
{
    const int64_t O = s.o, V = s.v;
    so_ladder_bare(cx, s, s.tau, s.r2);
    Tensor Z = view(cx.scratch("so_Z", O * O * O * V), {O, O, O, V});
    contract(cx, 1.0, s.tau, "ijef", s.ovvv, "maef", 0.0, Z, "ijma");
    contract(cx, 0.5, Z, "ijma", s.t1, "mb", 1.0, s.r2, "ijab");
    contract(cx, -0.5, Z, "ijmb", s.t1, "ma", 1.0, s.r2, "ijab");
}

void so_amplitudes(Context& cx, SOState& s)
{
    const auto C = contractor(cx);
    const int o = s.o, v = s.v;
    const int64_t O = o, V = v, o2v2 = O * O * V * V;
    // ---- T1, ccsd.f90:931-957
    C(1.0, s.t1, "ie", s.F_vv, "ae", 0.0, s.r1, "ia");
    C(-1.0, s.F_oo, "mi", s.t1, "ma", 1.0, s.r1, "ia");
    C(1.0, s.t1, "me", s.ovvo, "maei", 1.0, s.r1, "ia");
    C(1.0, s.t2, "miea", s.F_ov, "me", 1.0, s.r1, "ia");
    C(0.5, s.t2, "mife", s.ovvv, "mafe", 1.0, s.r1, "ia");
    C(-0.5, s.t2, "mnea", s.oovo, "mnei", 1.0, s.r1, "ia");
    if (s.fock)   // Eq. 1: + f_ia
        SO_KERNEL((Ranges{FR(s.f_ov.d, O * V), FR(s.r1.d, O * V)}), (Ranges{FR(s.r1.d, O * V)}), so_add_kernel, O * V, s.r1.d, s.f_ov.d, O * V);
    // ---- T2, ccsd.f90:959-1034
    Tensor AB = view(cx.scratch("so_AB", o2v2), {O, O, V, V}), A = view(cx.scratch("so_A", o2v2), {O, O, V, V});
    Tensor Bm = view(cx.scratch("so_B", o2v2), {O, O, V, V});
    Tensor Q = view(cx.scratch("so_Q", O * V * O * O), {O, V, O, O});
    Tensor X = view(cx.scratch("so_X", V * V), {V, V}), Y = view(cx.scratch("so_Y", O * O), {O, O});
    Tensor G = view(cx.scratch("so_G", O * O), {O, O});
    // P(ij)P(ab) [ t_imae W_mbej - t_ie t_ma <mb||ej> ]  (:973-994)
    C(1.0, s.ovvo, "mbej", s.t1, "ie", 0.0, Q, "mbij");
    C(-1.0, s.t1, "ma", Q, "mbij", 0.0, AB, "ijab");
    C(1.0, s.t2, "miea", s.W_ovvo, "mbej", 1.0, AB, "ijab");
    // P(ab) [ t_ijae (F_be - 1/2 t_mb F_me) ]  (:996-1003)  and  -P(ab) t_ma <mb||ij> = -P(ab) Z(ijab)  (:1012-1016)
    k_copy(cx, X.d, s.F_vv.d, V * V);
    C(-0.5, s.t1, "mb", s.F_ov, "me", 1.0, X, "be");
    C(1.0, s.t2, "ijae", X, "be", 0.0, Bm, "ijab");
    C(-1.0, s.oovo, "ijam", s.t1, "mb", 1.0, Bm, "ijab");
    // -P(ij) [ t_imab (F_mj + 1/2 t_je F_me) ]  (:1004-1007,:1017-1020)  and  P(ij) t_ie <ej||ab>  (:1008-1011)
    C(1.0, s.t1, "je", s.F_ov, "me", 0.0, Y, "jm");
    SO_KERNEL((Ranges{FR(s.F_oo.d, O * O), FR(Y.d, O * O)}), (Ranges{FR(G.d, O * O)}), so_g_kernel, O * O, G.d, s.F_oo.d, Y.d, o);
    C(-1.0, G, "mi", s.t2, "mjab", 0.0, A, "ijab");
    C(1.0, s.t1, "ie", s.vovv, "ejab", 1.0, A, "ijab");
    // 1/2 tau_mnab W_mnij + 1/2 tau_ijef W_abef  (:1021-1024)
    so_ladder(cx, s);
    C(0.5, s.W_oooo, "ijmn", s.tau, "mnab", 1.0, s.r2, "ijab");
    // :1027-1028 (t1 first: r1 / D_ia)
    k_div(cx, s.t1.d, s.r1.d, s.D1.d, O * V);
    SO_KERNEL((Ranges{FR(s.r2.d, o2v2), FR(s.oovv.d, o2v2), FR(AB.d, o2v2), FR(A.d, o2v2), FR(Bm.d, o2v2), FR(s.D2.d, o2v2)}), (Ranges{FR(s.t2.d, o2v2)}),
              so_t2_assemble_kernel, o2v2, s.t2.d, s.r2.d, s.oovv.d, AB.d, A.d, Bm.d, s.D2.d, o, v);
}

void so_sum2(Context& cx, double* out, const double* partial, int nout, int nblk, const double* f_ov, const double* l1, int64_t n1)
{
    LAUNCH(so_sum2_kernel, nout, out, partial, nblk, f_ov, l1, n1);
}

int so_energy(Context& cx, SOState& s, double e_tol, double t_tol)
{
    const int64_t n2 = s.t2.size();
    const int nblk = (int)std::min<int64_t>((n2 + TB - 1) / TB, 1024);
    double* partial = cx.scratch("so_energy_partial", 2 * 1024);
    LAUNCH(so_energy_kernel, nblk, partial, s.oovv.d, s.t1.d, s.t2.d, s.t2_old.d, s.o, s.v);
    so_sum2(cx, cx.scal, partial, 2, nblk);
    if (s.fock)   // + sum f_ia t_ia
        LAUNCH(so_energy_fock_kernel, 1, cx.scal, s.f_ov.d, s.t1.d, (int64_t)s.o * s.v);
    double* h = host_scalars(cx, DIIS_FLAG_SLOT + 1);
    diis_check_flag(cx, h);
    s.energy_old = s.energy;
    s.energy = h[0];
    s.rms = h[1];
    return (std::sqrt(h[1]) < t_tol && std::fabs(s.energy - s.energy_old) < e_tol) ? 1 : 0;
}

}  // namespace afesp
