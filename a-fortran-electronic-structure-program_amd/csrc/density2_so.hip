// density2_so.hip -- the two-particle density of spin-orbital CCSD (density2_so.h), term by term as
// tests/np_density2.py restates it (carriers, gamma_explicit).  Per block family: the products into one carrier through contract() /
// permute_add(), then one assemble kernel that adds the disconnected terms and sums the carrier over the images of the element with their
// signs, so that the stored block is antisymmetric / pair-symmetric to the bit.  Launches are plain call-by-call ones.
#include "device_util.h"
#include "density2_so.h"

#include <cmath>
#include <cstring>

namespace afesp {
namespace {

constexpr int D2_MAXBLK = 1024;
constexpr int D2_NFAM = 6;

// oooo(i,j,k,l) = 1/16 [images of Y],  Y(i,j,k,l) = tau_ijef l_klef: the antisymmetriser in each pair and the (ij)<->(kl) symmetriser
__global__ void d2_oooo_kernel(double* G, const double* Y, int o)
{
    const int64_t O = o, n = O * O * O * O;
    GRID_STRIDE(x, n)
    {
        const int64_t i = x % O, j = (x / O) % O, k = (x / (O * O)) % O, l = x / (O * O * O);
#define D2_Y(P_, Q_, R_, S_) Y[(P_) + O * ((Q_) + O * ((R_) + O * (S_)))]
        const double a = D2_Y(i, j, k, l) - D2_Y(j, i, k, l), b = D2_Y(i, j, l, k) - D2_Y(j, i, l, k);
        const double c = D2_Y(k, l, i, j) - D2_Y(l, k, i, j), d = D2_Y(k, l, j, i) - D2_Y(l, k, j, i);
#undef D2_Y
        G[x] = 0.0625 * ((a - b) + (c - d));
    }
}

// ooov(i,j,k,a) = 1/8 [c(i,j,k,a) - c(j,i,k,a)],  c = carrier - 4 G_oo(i,k) t1(j,a)
__global__ void d2_ooov_kernel(double* G, const double* Cr, const double* Goo, const double* t1, int o, int v)
{
    const int64_t O = o, n = O * O * O * v;
    GRID_STRIDE(x, n)
    {
        const int64_t i = x % O, j = (x / O) % O, k = (x / (O * O)) % O, a = x / (O * O * O);
        const double c1 = __dsub_rn(Cr[x], 4.0 * __dmul_rn(Goo[i + O * k], t1[j + O * a]));
        const double c2 = __dsub_rn(Cr[j + O * (i + O * (k + O * a))], 4.0 * __dmul_rn(Goo[j + O * k], t1[i + O * a]));
        G[x] = 0.125 * (c1 - c2);
    }
}

// oovv(i,j,a,b) = 1/8 [c(ijab) - c(jiab) - c(ijba) + c(jiba)],  c = carrier + tau + l2 + 4 s1(i,a) t1(j,b)
__global__ void d2_oovv_kernel(double* G, const double* Cr, const double* tau, const double* l2, const double* s1, const double* t1, int o, int v)
{
    const int64_t O = o, V = v, n = O * O * V * V;
    GRID_STRIDE(x, n)
    {
        const int64_t i = x % O, j = (x / O) % O, a = (x / (O * O)) % V, b = x / (O * O * V);
        auto c = [&](int64_t p, int64_t q, int64_t e, int64_t f) {
            const int64_t y = p + O * (q + O * (e + V * f));
            return __dadd_rn(__dadd_rn(__dadd_rn(Cr[y], tau[y]), l2[y]), 4.0 * __dmul_rn(s1[p + O * e], t1[q + O * f]));
        };
        G[x] = 0.125 * ((c(i, j, a, b) - c(j, i, a, b)) - (c(i, j, b, a) - c(j, i, b, a)));
    }
}

// ovov(i,a,j,b) = 1/8 [c(i,a,j,b) + c(j,b,i,a)],  c = carrier - 4 l1(j,a) t1(i,b)
__global__ void d2_ovov_kernel(double* G, const double* Cr, const double* l1, const double* t1, int o, int v)
{
    const int64_t O = o, V = v, n = O * V * O * V;
    GRID_STRIDE(x, n)
    {
        const int64_t i = x % O, a = (x / O) % V, j = (x / (O * V)) % O, b = x / (O * V * O);
        const double c1 = __dsub_rn(Cr[x], 4.0 * __dmul_rn(l1[j + O * a], t1[i + O * b]));
        const double c2 = __dsub_rn(Cr[j + O * (b + V * (i + O * a))], 4.0 * __dmul_rn(l1[i + O * b], t1[j + O * a]));
        G[x] = 0.125 * (c1 + c2);
    }
}

// ovvv(i,a,b,c) = 1/8 [c(i,a,b,c) - c(i,a,c,b)],  c = carrier - 4 G_vv(a,c) t1(i,b)
__global__ void d2_ovvv_kernel(double* G, const double* Cr, const double* Gvv, const double* t1, int o, int v)
{
    const int64_t O = o, V = v, n = O * V * V * V;
    GRID_STRIDE(x, n)
    {
        const int64_t i = x % O, a = (x / O) % V, b = (x / (O * V)) % V, c = x / (O * V * V);
        const double c1 = __dsub_rn(Cr[x], 4.0 * __dmul_rn(Gvv[a + V * c], t1[i + O * b]));
        const double c2 = __dsub_rn(Cr[i + O * (a + V * (c + V * b))], 4.0 * __dmul_rn(Gvv[a + V * b], t1[i + O * c]));
        G[x] = 0.125 * (c1 - c2);
    }
}

// ga(p, q) = ga(q, p) = 1/2 (w(p, q) + w(q, p)) in place, one thread per unordered pair of pair indices
__global__ void d2_pair_symmetrise_kernel(double* ga, int64_t npv, int64_t ka)
{
    GRID_STRIDE(y, npv * npv)
    {
        const int64_t p = y % npv, q = y / npv;
        if (p > q) continue;
        const double s = 0.5 * (ga[p + ka * q] + ga[q + ka * p]);
        ga[p + ka * q] = s;
        ga[q + ka * p] = s;
    }
}

// One walk over a stored block: every element times the sum over its images, with their signs, of either the state's own integrals
// (A == nullptr: g is the slice in the block's layout -- <ia||bj> stored (i,a,b,j) for ovov, va for the pair form -- and `weight` the
// number of images over four) or A_pr B_qs (two caller matrices, (o+v)^2 column-major).  Block partials in a fixed order.
struct D2Walk {
    const double* G;
    const double* g;
    const double* A;
    const double* B;
    double weight;
    int64_t n, ld;
    int fam, o, v;
};
__device__ __forceinline__ double d2_ab(const double* A, const double* B, int64_t N, int64_t p, int64_t q, int64_t r, int64_t s)
{
    return A[p + N * r] * B[q + N * s];
}
__global__ void d2_walk_kernel(double* partial, D2Walk w)
{
    const int64_t O = w.o, V = w.v, N = O + V;
    double sum = 0.0;
    GRID_STRIDE(x, w.n)
    {
        double val, wt;
        int64_t p, q, r, s;
        if (w.fam == 5) {
            const int64_t npv = V * (V - 1) / 2;
            int a, b, c, d;
            unpair_lt(x % npv, a, b);
            unpair_lt(x / npv, c, d);
            val = w.G[x % npv + w.ld * (x / npv)];
            wt = w.A ? 0.0 : w.g[x % npv + w.ld * (x / npv)];
            p = O + a; q = O + b; r = O + c; s = O + d;
        } else {
            const bool qv = w.fam == 3 || w.fam == 4, rv = w.fam == 2 || w.fam == 4;
            const int64_t d0 = O, d1 = qv ? V : O, d2 = rv ? V : O;
            const int64_t x0 = x % d0, x1 = (x / d0) % d1, x2 = (x / (d0 * d1)) % d2, x3 = x / (d0 * d1 * d2);
            val = w.G[x];
            // <ia||jb> = -<ia||bj>, the state's ovvo slice (i,a,b,j)
            wt = w.A ? 0.0 : (w.fam == 3 ? -w.g[x0 + O * (x1 + V * (x3 + V * x2))] : w.g[x]);
            p = x0;
            q = x1 + (qv ? O : 0);
            r = x2 + (rv ? O : 0);
            s = x3 + (w.fam == 0 ? 0 : O);
        }
        if (w.A) {
            const double* A = w.A;
            const double* B = w.B;
            switch (w.fam) {
            case 0: wt = d2_ab(A, B, N, p, q, r, s); break;
            case 1: wt = (d2_ab(A, B, N, p, q, r, s) - d2_ab(A, B, N, p, q, s, r)) + (d2_ab(A, B, N, r, s, p, q) - d2_ab(A, B, N, s, r, p, q)); break;
            case 2: wt = d2_ab(A, B, N, p, q, r, s) + d2_ab(A, B, N, r, s, p, q); break;
            case 4: wt = (d2_ab(A, B, N, p, q, r, s) - d2_ab(A, B, N, q, p, r, s)) + (d2_ab(A, B, N, r, s, p, q) - d2_ab(A, B, N, r, s, q, p)); break;
            default:   // ovov and the pair form: the four images inside one orientation (the transposed pair is a stored element itself)
                wt = (d2_ab(A, B, N, p, q, r, s) - d2_ab(A, B, N, q, p, r, s)) - (d2_ab(A, B, N, p, q, s, r) - d2_ab(A, B, N, q, p, s, r));
                break;
            }
        }
        sum += val * wt;
    }
    __shared__ double red[4];
    double t[1] = {sum};
    block_sum_down<1>(t, red);   // (the order of the CCSD and Lambda energies)
    if (threadIdx.x == 0) partial[blockIdx.x] = w.weight * t[0];
}

// out[f] = the ordered sum of family f's block partials partial[f D2_MAXBLK .. + nblk[f])
struct D2Counts { int nblk[D2_NFAM]; };
__global__ void d2_final_sum_kernel(double* out, const double* partial, D2Counts cnt)
{
    __shared__ double red[TB];
    const double* p = partial + (int64_t)blockIdx.x * D2_MAXBLK;
    const int nblk = cnt.nblk[blockIdx.x];
    double s = 0.0;
    for (int x = threadIdx.x; x < nblk; x += TB) s += p[x];
    block_tree_sum(s, red);
    if (threadIdx.x == 0) out[blockIdx.x] = red[0];
}

constexpr const char* D2_PLAIN = "the two-particle density is";   // (so_need_plain)

// the six family sums of one walk each, on the host in family order
void walk_all(Context& cx, SOState& s, SODensity2& G, const double* A, const double* B, double* out)
{
    const int o = s.o, v = s.v;
    const int64_t O = o, V = v, npv = pair_count(V), npo = pair_count(O);
    double* partial = cx.scratch("d2_partial", (int64_t)D2_NFAM * D2_MAXBLK);
    const double* blocks[D2_NFAM] = {G.oooo.d, G.ooov.d, G.oovv.d, G.ovov.d, G.ovvv.d, G.ga};
    const double* slices[D2_NFAM] = {s.oooo.d, s.ooov.d, s.oovv.d, s.ovvo.d, s.ovvv.d, s.va};
    const int64_t counts[D2_NFAM] = {O * O * O * O, O * O * O * V, O * O * V * V, O * V * O * V, O * V * V * V, npv * npv};
    const double images[D2_NFAM] = {1.0, 4.0, 2.0, 4.0, 4.0, 4.0};   // (pair form: the four images of a stored a < b, c < d element)
    D2Counts cnt;
    for (int f = 0; f < D2_NFAM; ++f) {
        // (the pair form of a state without an occupied pair is zero and its integral side va is not built)
        const bool empty = counts[f] == 0 || (f == 5 && (!G.ga || (!A && (npo == 0 || !s.va))));
        cnt.nblk[f] = empty ? 0 : (int)std::min<int64_t>((counts[f] + TB - 1) / TB, D2_MAXBLK);
        if (empty) continue;
        D2Walk w{blocks[f], slices[f], A, B, A ? 1.0 : 0.25 * images[f], counts[f], s.lad_ka, f, o, v};
        LAUNCH(d2_walk_kernel, cnt.nblk[f], partial + (int64_t)f * D2_MAXBLK, w);
    }
    LAUNCH(d2_final_sum_kernel, D2_NFAM, cx.scal, partial, cnt);
    const double* h = host_scalars(cx, D2_NFAM);
    for (int f = 0; f < D2_NFAM; ++f) out[f] = h[f];
}

}  // namespace

void preload_density2_so()
{
    static const bool loaded = [] {
        first_use_touch(reinterpret_cast<const void*>(d2_oooo_kernel));
        first_use_touch(reinterpret_cast<const void*>(d2_ooov_kernel));
        first_use_touch(reinterpret_cast<const void*>(d2_oovv_kernel));
        first_use_touch(reinterpret_cast<const void*>(d2_ovov_kernel));
        first_use_touch(reinterpret_cast<const void*>(d2_ovvv_kernel));
        first_use_touch(reinterpret_cast<const void*>(d2_pair_symmetrise_kernel));
        first_use_touch(reinterpret_cast<const void*>(d2_walk_kernel));
        first_use_touch(reinterpret_cast<const void*>(d2_final_sum_kernel));
        (void)hipGetLastError();
        return true;
    }();
    (void)loaded;
}

SODensity2& so_density2_need(SOState& s, const char* who)
{
    SOLambda& L = so_lambda_need(s, who);
    if (!L.d2 || L.d2->epoch != s.amp_epoch || L.d2->stamp != L.stamp)
        throw Error(LAMBDA_ERR_STALE, std::string(who) + ": no two-particle density of the current t and lambda (call afesp_ccsd_so_density2_build; "
                                                         "whatever writes t1 / t2 or l1 / l2 makes an earlier build stale)");
    return *L.d2;
}

double so_density2_bytes(int64_t o, int64_t v)
{
    const double O = (double)o, V = (double)v, o2v2 = O * O * V * V;
    auto even = [](double x) { return x + std::fmod(x, 2.0); };
    const double npv = V * (V - 1) / 2, ka = even(std::max(npv, 1.0)), na = even(std::max(O * (O - 1) / 2, 1.0));
    // the stored blocks; Y, M, Lt, Mt, the four carriers, the two packed pair operands, the one-body pieces and the block partials
    const double stored = O * O * O * O + O * O * O * V + 2.0 * o2v2 + O * V * V * V + ka * npv;
    const double work = O * O * O * O + o2v2 + 2.0 * O * O * O * V + O * O * O * V + 2.0 * o2v2 + O * V * V * V + 2.0 * na * ka + O * O + V * V + O * V +
                        (O + V) * (O + V) * 3.0 + (double)D2_NFAM * D2_MAXBLK;
    return 8.0 * (stored + work);
}

void so_density2_free(Context& cx, SOLambda& L)
{
    if (!L.d2) return;
    double* bufs[] = {L.d2->oooo.d, L.d2->ooov.d, L.d2->oovv.d, L.d2->ovov.d, L.d2->ovvv.d, L.d2->ga};
    for (double* b : bufs) cx.release(b);
    delete L.d2;
    L.d2 = nullptr;
}

void so_density2_build(Context& cx, SOState& s)
{
    so_need_plain(cx, "afesp_ccsd_so_density2_build", D2_PLAIN);
    if (!s.foo_as_published)
        throw Error(LAMBDA_ERR_FOO, "afesp_ccsd_so_density2_build: this state keeps the reference's transposed F_mi term, whose equations have no consistent "
                                    "Lagrangian (initialise it with AFESP_SO_FOO_AS_PUBLISHED=1)");
    SOLambda& L = so_lambda_need(s, "afesp_ccsd_so_density2_build");
    const int o = s.o, v = s.v;
    const int64_t O = o, V = v, npv = pair_count(V), npo = pair_count(O), ka = s.lad_ka, na = s.lad_na;
    if (!L.d2) {
        if (!cx.fits(so_density2_bytes(o, v)))
            throw Error(LAMBDA_ERR_CAPACITY, "afesp_ccsd_so_density2_build: the two-particle density of this system does not fit the free device memory");
        L.d2 = new SODensity2();
        SODensity2& G = *L.d2;
        try {
            G.oooo = cx.tensor({O, O, O, O}); G.ooov = cx.tensor({O, O, O, V}); G.oovv = cx.tensor({O, O, V, V});
            G.ovov = cx.tensor({O, V, O, V}); G.ovvv = cx.tensor({O, V, V, V});
            if (npv > 0) G.ga = cx.alloc(ka * npv);
        } catch (...) {
            try { so_density2_free(cx, L); } catch (...) {}
            throw;
        }
    }
    preload_density2_so();
    SODensity2& G = *L.d2;
    G.epoch = G.stamp = -1;   // (stale until the last launch is queued)
    const auto C = contractor(cx);
    const Tensor &t1 = s.t1, &t2 = s.t2, &l1 = L.l1, &l2 = L.l2, &tau = L.tau;
    // G_vv / G_oo of the current l2 (as so_density)
    C(-0.5, t2, "mnef", l2, "mnaf", 0.0, L.Gvv, "ae");
    C(0.5, t2, "mnef", l2, "inef", 0.0, L.Goo, "mi");
    Tensor Y = view(cx.scratch("d2_Y", O * O * O * O), {O, O, O, O}), M = view(cx.scratch("d2_M", O * V * O * V), {O, V, O, V});
    Tensor Lt = view(cx.scratch("d2_Lt", O * O * O * V), {O, O, O, V}), Mt = view(cx.scratch("d2_Mt", O * V * O * O), {O, V, O, O});
    Tensor Xoo = view(cx.scratch("d2_Xoo", O * O), {O, O}), Xvv = view(cx.scratch("d2_Xvv", V * V), {V, V}), s1 = view(cx.scratch("d2_s1", O * V), {O, V});
    // ---- what the families share: Y_ijkl = tau_ijef l_klef (o^4 v^2), the ring product M_iakf = t_imae l_kmfe (o^3 v^3), Lt_mnia = l_mnae t_ie
    C(1.0, tau, "ijef", l2, "klef", 0.0, Y, "ijkl");
    C(1.0, t2, "imae", l2, "kmfe", 0.0, M, "iakf");
    C(1.0, l2, "mnae", t1, "ie", 0.0, Lt, "mnia");
    C(1.0, l1, "me", t1, "je", 0.0, Xoo, "mj");
    C(1.0, l1, "me", t1, "mb", 0.0, Xvv, "eb");
    C(1.0, l1, "me", t2, "imae", 0.0, s1, "ia");
    // ---- oooo
    LAUNCH(d2_oooo_kernel, grid_for(G.oooo.size(), SO_GRID_CAP), G.oooo.d, Y.d, o);
    // ---- ooov: -2 l_ke tau_ijea + Y_ijkm t_ma + 4 M_iakf t_jf + 2 l_ijae t_ke  (- 4 G_ik t_ja in the kernel)
    Tensor c1 = view(cx.scratch("d2_c_ooov", O * O * O * V), {O, O, O, V});
    C(-2.0, l1, "ke", tau, "ijea", 0.0, c1, "ijka");
    C(1.0, Y, "ijkm", t1, "ma", 1.0, c1, "ijka");
    C(4.0, M, "iakf", t1, "jf", 1.0, c1, "ijka");
    C(2.0, l2, "ijae", t1, "ke", 1.0, c1, "ijka");
    LAUNCH(d2_ooov_kernel, grid_for(G.ooov.size(), SO_GRID_CAP), G.ooov.d, c1.d, L.Goo.d, t1.d, o, v);
    // ---- ovvv: 2 l_ma tau_imbc + Lt_mnia tau_mnbc - 4 M_icna t_nb + 2 l_imbc t_ma  (- 4 G_ac t_ib in the kernel).  Lt first: the product
    // l_mnae tau_mnbc itself would be the v^4 array times t1
    Tensor c4 = view(cx.scratch("d2_c_ovvv", O * V * V * V), {O, V, V, V});
    C(2.0, l1, "ma", tau, "imbc", 0.0, c4, "iabc");
    C(1.0, Lt, "mnia", tau, "mnbc", 1.0, c4, "iabc");
    C(-4.0, M, "icna", t1, "nb", 1.0, c4, "iabc");
    C(2.0, l2, "imbc", t1, "ma", 1.0, c4, "iabc");
    LAUNCH(d2_ovvv_kernel, grid_for(G.ovvv.size(), SO_GRID_CAP), G.ovvv.d, c4.d, L.Gvv.d, t1.d, o, v);
    // ---- ovov: -4 M_ibja + 4 Lt_jmia t_mb  (- 4 l_ja t_ib in the kernel)
    Tensor c3 = view(cx.scratch("d2_c_ovov", O * V * O * V), {O, V, O, V});
    permute_add(cx, -4.0, M, "ibja", 0.0, c3, "iajb");
    C(4.0, Lt, "jmia", t1, "mb", 1.0, c3, "iajb");
    LAUNCH(d2_ovov_kernel, grid_for(G.ovov.size(), SO_GRID_CAP), G.ovov.d, c3.d, l1.d, t1.d, o, v);
    // ---- oovv: -2 X_mj t_imab + 2 X_eb tau_ijea - 2 G_in tau_njab + 2 G_fb tau_ijaf + 1/4 Y_ijmn tau_mnab + 2 M_ibnf t_njaf + 4 (M_ibnf t_jf) t_na
    // (+ tau + l2 + 4 s_ia t_jb in the kernel)
    Tensor c2 = view(cx.scratch("d2_c_oovv", O * O * V * V), {O, O, V, V});
    C(1.0, M, "ibnf", t1, "jf", 0.0, Mt, "ibnj");
    C(-2.0, Xoo, "mj", t2, "imab", 0.0, c2, "ijab");
    C(2.0, Xvv, "eb", tau, "ijea", 1.0, c2, "ijab");
    C(-2.0, L.Goo, "in", tau, "njab", 1.0, c2, "ijab");
    C(2.0, L.Gvv, "fb", tau, "ijaf", 1.0, c2, "ijab");
    C(0.25, Y, "ijmn", tau, "mnab", 1.0, c2, "ijab");
    C(2.0, M, "ibnf", t2, "njaf", 1.0, c2, "ijab");
    C(4.0, Mt, "ibnj", t1, "na", 1.0, c2, "ijab");
    LAUNCH(d2_oovv_kernel, grid_for(G.oovv.size(), SO_GRID_CAP), G.oovv.d, c2.d, tau.d, l2.d, s1.d, t1.d, o, v);
    // ---- vvvv, pair form only: w(ab, cd) = sum_{i<j} l_ijab tau_ijcd, one product with K = o (o - 1) / 2 on the packed operands, then
    // ga = 1/2 (w + w^T) in place
    if (npv > 0) {
        if (npo == 0) {
            k_fill(cx, G.ga, ka * npv, 0.0);
        } else {
            double* la = cx.scratch("d2_la", na * npv);
            double* ta = cx.scratch("d2_ta", na * npv);
            so_pair_pack(cx, s, l2, la);   // (the ladder's packer and pair layout)
            so_pair_pack(cx, s, tau, ta);
            Tensor LA = view(la, {npo, npv}), TA = view(ta, {npo, npv}), GA = view(G.ga, {npv, npv});
            LA.stride[1] = TA.stride[1] = na;
            GA.stride[1] = ka;
            C(1.0, LA, "kp", TA, "kq", 0.0, GA, "pq");
            LAUNCH(d2_pair_symmetrise_kernel, grid_for(npv * npv, SO_GRID_CAP), G.ga, npv, ka);
        }
    }
    cx.sync();
    G.epoch = s.amp_epoch;
    G.stamp = L.stamp;
}

void so_density2_get(Context& cx, SOState& s, const char* name, double* out, int64_t capacity)
{
    so_need_plain(cx, "afesp_ccsd_so_density2_get", D2_PLAIN);
    if (!name || !out) throw Error(1, "afesp_ccsd_so_density2_get: NULL argument");
    SODensity2& G = so_density2_need(s, "afesp_ccsd_so_density2_get");
    const int64_t O = s.o, V = s.v, N = O + V, npv = pair_count(V), ka = s.lad_ka;
    auto need = [&](int64_t n) {
        if (capacity < n)
            throw Error(LAMBDA_ERR_CAPACITY, std::string("afesp_ccsd_so_density2_get: the buffer holds ") + std::to_string(capacity) + " doubles, " + name +
                                                 " needs " + std::to_string(n));
    };
    auto fetch = [&](double* dst, const Tensor& t) {
        if (t.size() > 0) AFESP_HIP(hipMemcpyAsync(dst, t.d, sizeof(double) * t.size(), hipMemcpyDeviceToHost, cx.stream));
    };
    auto fetch_pairs = [&](double* dst) {
        if (npv > 0)
            AFESP_HIP(hipMemcpy2DAsync(dst, sizeof(double) * npv, G.ga, sizeof(double) * ka, sizeof(double) * npv, npv, hipMemcpyDeviceToHost, cx.stream));
        cx.sync();
    };
    struct { const char* n; const Tensor* t; } tab[] = {{"oooo", &G.oooo}, {"ooov", &G.ooov}, {"oovv", &G.oovv}, {"ovov", &G.ovov}, {"ovvv", &G.ovvv}};
    for (auto& e : tab)
        if (!strcmp(e.n, name)) {
            need(e.t->size());
            fetch(out, *e.t);
            cx.sync();
            return;
        }
    if (!strcmp(name, "vvvv_pairs")) {
        need(npv * npv);
        fetch_pairs(out);
        return;
    }
    const bool full = !strcmp(name, "full");
    if (!full && strcmp(name, "vvvv")) throw Error(1, std::string("afesp_ccsd_so_density2_get: unknown name ") + name);
    need(full ? N * N * N * N : V * V * V * V);
    // the expansions, written on the host for the caller: no dense v^4 array exists on the device
    std::vector<double> ga((size_t)(npv * npv));
    fetch_pairs(ga.data());
    const int64_t n4 = full ? N : V, off = full ? O : 0;
    auto at = [&](int64_t p, int64_t q, int64_t r, int64_t t) -> double& { return out[p + n4 * (q + n4 * (r + n4 * t))]; };
    std::fill(out, out + n4 * n4 * n4 * n4, 0.0);
    auto pidx = [](int64_t a, int64_t b) { return a + b * (b - 1) / 2; };
    for (int64_t d = 1; d < V; ++d)
        for (int64_t c = 0; c < d; ++c)
            for (int64_t b = 1; b < V; ++b)
                for (int64_t a = 0; a < b; ++a) {
                    const double x = ga[(size_t)(pidx(a, b) + npv * pidx(c, d))];
                    at(off + a, off + b, off + c, off + d) = at(off + b, off + a, off + d, off + c) = x;
                    at(off + b, off + a, off + c, off + d) = at(off + a, off + b, off + d, off + c) = -x;
                }
    if (!full) return;
    std::vector<double> h;
    auto host = [&](const Tensor& t) {
        h.resize((size_t)t.size());
        fetch(h.data(), t);
        cx.sync();
    };
    host(G.oooo);
    for (int64_t x = 0; x < G.oooo.size(); ++x) at(x % O, (x / O) % O, (x / (O * O)) % O, x / (O * O * O)) = h[(size_t)x];
    host(G.ooov);
    for (int64_t x = 0; x < G.ooov.size(); ++x) {
        const int64_t i = x % O, j = (x / O) % O, k = (x / (O * O)) % O, a = O + x / (O * O * O);
        at(i, j, k, a) = at(k, a, i, j) = h[(size_t)x];
        at(i, j, a, k) = at(a, k, i, j) = -h[(size_t)x];
    }
    host(G.oovv);
    for (int64_t x = 0; x < G.oovv.size(); ++x) {
        const int64_t i = x % O, j = (x / O) % O, a = O + (x / (O * O)) % V, b = O + x / (O * O * V);
        at(i, j, a, b) = at(a, b, i, j) = h[(size_t)x];
    }
    host(G.ovov);
    for (int64_t x = 0; x < G.ovov.size(); ++x) {
        const int64_t i = x % O, a = O + (x / O) % V, j = (x / (O * V)) % O, b = O + x / (O * V * O);
        at(i, a, j, b) = at(a, i, b, j) = h[(size_t)x];
        at(a, i, j, b) = at(i, a, b, j) = -h[(size_t)x];
    }
    host(G.ovvv);
    for (int64_t x = 0; x < G.ovvv.size(); ++x) {
        const int64_t i = x % O, a = O + (x / O) % V, b = O + (x / (O * V)) % V, c = O + x / (O * V * V);
        at(i, a, b, c) = at(b, c, i, a) = h[(size_t)x];
        at(a, i, b, c) = at(b, c, a, i) = -h[(size_t)x];
    }
}

void so_density2_energy(Context& cx, SOState& s, double* e)
{
    so_need_plain(cx, "afesp_ccsd_so_density2_energy", D2_PLAIN);
    if (!e) throw Error(1, "afesp_ccsd_so_density2_energy: NULL argument");
    SODensity2& G = so_density2_need(s, "afesp_ccsd_so_density2_energy");
    const int64_t O = s.o, V = s.v, N = O + V;
    // sum f D with the state's f: the levels on the diagonal, f_ov / f_oo / f_vv where the state has them (one-body algebra, on the host)
    std::vector<double> D((size_t)(N * N)), lev((size_t)N), fov, foo, fvv;
    so_density(cx, s, D.data(), N * N);
    if (s.lev) {
        AFESP_HIP(hipMemcpyAsync(lev.data(), s.lev, sizeof(double) * N, hipMemcpyDeviceToHost, cx.stream));
        cx.sync();
    } else {
        std::vector<double> es((size_t)s.n);
        AFESP_HIP(hipMemcpyAsync(es.data(), s.e, sizeof(double) * s.n, hipMemcpyDeviceToHost, cx.stream));
        cx.sync();
        for (int64_t p = 0; p < N; ++p) lev[(size_t)p] = es[(size_t)(p / 2)];   // (the interleaved order of the RHF-fed state)
    }
    double e0 = 0.0;
    for (int64_t p = 0; p < N; ++p) e0 += lev[(size_t)p] * D[(size_t)(p + N * p)];
    if (s.fock) {
        fov.resize((size_t)(O * V)); foo.resize((size_t)(O * O)); fvv.resize((size_t)(V * V));
        AFESP_HIP(hipMemcpyAsync(fov.data(), s.f_ov.d, sizeof(double) * O * V, hipMemcpyDeviceToHost, cx.stream));
        AFESP_HIP(hipMemcpyAsync(foo.data(), s.f_oo.d, sizeof(double) * O * O, hipMemcpyDeviceToHost, cx.stream));
        AFESP_HIP(hipMemcpyAsync(fvv.data(), s.f_vv.d, sizeof(double) * V * V, hipMemcpyDeviceToHost, cx.stream));
        cx.sync();
        for (int64_t i = 0; i < O; ++i)
            for (int64_t m = 0; m < O; ++m)
                if (m != i) e0 += foo[(size_t)(m + O * i)] * D[(size_t)(m + N * i)];
        for (int64_t c = 0; c < V; ++c)
            for (int64_t a = 0; a < V; ++a)
                if (a != c) e0 += fvv[(size_t)(a + V * c)] * D[(size_t)(O + a + N * (O + c))];
        for (int64_t a = 0; a < V; ++a)
            for (int64_t i = 0; i < O; ++i) e0 += 2.0 * fov[(size_t)(i + O * a)] * D[(size_t)(i + N * (O + a))];
    }
    e[0] = e0;
    walk_all(cx, s, G, nullptr, nullptr, e + 1);
    e[7] = ((((e[1] + e[2]) + e[3]) + e[4]) + e[5]) + e[6];
}

double so_density2_expect(Context& cx, SOState& s, const double* A, const double* B)
{
    so_need_plain(cx, "afesp_ccsd_so_density2_expect", D2_PLAIN);
    if (!A || !B) throw Error(1, "afesp_ccsd_so_density2_expect: NULL argument");
    SODensity2& G = so_density2_need(s, "afesp_ccsd_so_density2_expect");
    const int64_t N = (int64_t)s.o + s.v;
    double* ab = cx.scratch("d2_AB", 2 * N * N);
    AFESP_HIP(hipMemcpyAsync(ab, A, sizeof(double) * N * N, hipMemcpyHostToDevice, cx.stream));
    AFESP_HIP(hipMemcpyAsync(ab + N * N, B, sizeof(double) * N * N, hipMemcpyHostToDevice, cx.stream));
    double f[D2_NFAM];
    walk_all(cx, s, G, ab, ab + N * N, f);
    return ((((f[0] + f[1]) + f[2]) + f[3]) + f[4]) + f[5];
}

}  // namespace afesp
