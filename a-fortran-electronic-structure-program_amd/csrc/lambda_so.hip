// lambda_so.hip -- spin-orbital CCSD Lambda equations and the unrelaxed one-particle density (lambda_so.h).
// Every term is one label-driven contract(), in the letters of Gauss and Stanton (1995) as restated in tests/np_lambda.py
// (hbar, lambda_rhs_explicit, density_explicit); launches are plain call-by-call ones -- the levelled / recorded path of fused.h is
// not extended to them.
#include "device_util.h"
#include "lambda_so.h"
#include "density2_so.h"

#include <cmath>

namespace afesp {
namespace {

constexpr int MAXBLK = 1024;
constexpr const char *LAM_WHO = "so_lambda", *LAM_PLAIN = "the Lambda equations are";   // (so_need_plain)

// tau(i,j,a,b) = t2 + t1(i,a) t1(j,b) - t1(i,b) t1(j,a)
__global__ void lam_tau_kernel(double* tau, const double* t1, const double* t2, int o, int v)
{
    const int64_t n2 = (int64_t)o * o * v * v;
    GRID_STRIDE(x, n2)
    {
        const auto [i, j, a, b] = oovv_decode(x, o, v);
        tau[x] = t2[x] + t1[i + o * a] * t1[j + o * b] - t1[i + o * b] * t1[j + o * a];
    }
}

// the ring operand of H_mbej with the whole t2 (W_mbej of the T iteration takes half of it): out(n,f,j,b) = t2(j,n,f,b) + t1(j,f) t1(n,b)
__global__ void lam_ring_operand_kernel(double* out, const double* t1, const double* t2, int o, int v)
{
    const int64_t n2 = (int64_t)o * v * o * v;
    GRID_STRIDE(x, n2)
    {
        const int n = (int)(x % o), f = (int)((x / o) % v), j = (int)((x / ((int64_t)o * v)) % o), b = (int)(x / ((int64_t)o * v * o));
        out[x] = t2[j + (int64_t)o * (n + (int64_t)o * (f + (int64_t)v * b))] + t1[j + o * f] * t1[n + o * b];
    }
}

// block sums of a pair of per-thread values, in the order of so_energy_kernel: partial[block] and partial[gridDim.x + block]
__device__ __forceinline__ void lam_block_sums(double* partial, double e, double r)
{
    __shared__ double red[2 * 4];
    double s[2] = {e, r};
    block_sum_down<2>(s, red);
    if (threadIdx.x == 0) {
        partial[blockIdx.x] = s[0];
        partial[gridDim.x + blockIdx.x] = s[1];
    }
}

// The l2 update in one pass: x2 holds the ladder terms; AB carries P(ij)P(ab) together with the disconnected l1(i,a) H_jb, A carries
// P(ij), Bm carries P(ab):
//   l2 = [<ij||ab> + x2 + P(ij)P(ab) (AB + l1 Hov) + P(ij) A + P(ab) Bm] / D
// and the block partials of the pseudo energy 1/4 sum <ij||ab> l2 and of sum (l2 - l2_old)^2; l2_old <- l2.  l1 is the one the
// iteration started from (its own division follows this kernel).
__global__ void lam_l2_assemble_kernel(double* l2, double* l2_old, double* partial, const double* x2, const double* oovv, const double* AB,
                                       const double* A, const double* Bm, const double* l1, const double* Hov, const double* D2, int o, int v)
{
    const int64_t n2 = (int64_t)o * o * v * v;
    double e = 0.0, r = 0.0;
    GRID_STRIDE(x, n2)
    {
        const auto [i, j, a, b] = oovv_decode(x, o, v);
        const auto [ji, ba, jiba] = oovv_images(i, j, a, b, o, v);
        // (rounded products, grouped so that exchanging i and j or a and b negates the term to the bit: it vanishes on the diagonals)
        const double disc = (__dmul_rn(l1[i + o * a], Hov[j + o * b]) + __dmul_rn(l1[j + o * b], Hov[i + o * a])) -
                            (__dmul_rn(l1[j + o * a], Hov[i + o * b]) + __dmul_rn(l1[i + o * b], Hov[j + o * a]));
        const double val = oovv[x] + x2[x] + (AB[x] - AB[ji] - AB[ba] + AB[jiba]) + disc + (A[x] - A[ji]) + (Bm[x] - Bm[ba]);
        const double l = val / D2[x];
        l2[x] = l;
        e += 0.25 * oovv[x] * l;
        const double d = l - l2_old[x];
        r += d * d;
        l2_old[x] = l;
    }
    lam_block_sums(partial, e, r);
}

// the same two sums of an l2 that is already there (so_lambda_energy); l2_old <- l2
__global__ void lam_energy_kernel(double* partial, const double* oovv, const double* l2, double* l2_old, int64_t n2)
{
    double e = 0.0, r = 0.0;
    GRID_STRIDE(x, n2)
    {
        const double l = l2[x];
        e += 0.25 * oovv[x] * l;
        const double d = l - l2_old[x];
        r += d * d;
        l2_old[x] = l;
    }
    lam_block_sums(partial, e, r);
}

// so_density_assemble (lambda_so.h), one element per thread.  (The ground state's w = 1: __fma_rn(1, t1, dov) is the once-rounded dov + t1.)
__global__ void so_density_assemble_kernel(double* D, const double* doo, const double* dvv, const double* dov, const double* t1,
                                           const double* r1, const double* L1, double w, double l0, int o, int v)
{
    const int n = o + v;
    GRID_STRIDE(x, (int64_t)n * n)
    {
        const int p = (int)(x % n), q = (int)(x / n);
        double val;
        if (p < o && q < o) val = 0.5 * (doo[p + o * q] + doo[q + o * p]);
        else if (p >= o && q >= o) val = 0.5 * (dvv[(p - o) + v * (q - o)] + dvv[(q - o) + v * (p - o)]);
        else {
            const int m = p < o ? p : q, e = (p < o ? q : p) - o;
            double sum = __fma_rn(w, t1[m + o * e], dov[m + o * e]);
            if (r1) sum = __fma_rn(l0, r1[m + o * e], sum);
            if (L1) sum += L1[m + o * e];
            val = 0.5 * sum;
        }
        D[x] = val;
    }
}

// G_vv / G_oo of the current l2
void build_G(Context& cx, SOState& s, SOLambda& L)
{
    contract(cx, -0.5, s.t2, "mnef", L.l2, "mnaf", 0.0, L.Gvv, "ae");
    contract(cx, 0.5, s.t2, "mnef", L.l2, "inef", 0.0, L.Goo, "mi");
}

void free_buffers(Context& cx, SOLambda& L)
{
    double* bufs[] = {L.amp, L.x1.d, L.l2_old.d, L.tau.d, L.Hov.d, L.Hoo.d, L.Hvv.d, L.Hoooo.d, L.Hvovv.d, L.Hooov.d, L.Hovvo.d, L.Hvvvo.d,
                      L.Hovoo.d, L.Gvv.d, L.Goo.d, L.amp_s, L.hist_t, L.hist_e, L.coef, L.bmat};
    for (double* b : bufs) cx.release(b);
}

}  // namespace

void preload_lambda_so()
{
    static const bool loaded = [] {
        first_use_touch(reinterpret_cast<const void*>(lam_tau_kernel));
        first_use_touch(reinterpret_cast<const void*>(lam_ring_operand_kernel));
        first_use_touch(reinterpret_cast<const void*>(lam_l2_assemble_kernel));
        first_use_touch(reinterpret_cast<const void*>(lam_energy_kernel));
        first_use_touch(reinterpret_cast<const void*>(so_density_assemble_kernel));
        (void)hipGetLastError();
        return true;
    }();
    (void)loaded;
}

double so_lambda_bytes(int64_t o, int64_t v, int diis_nerr)
{
    const double O = (double)o, V = (double)v, o2v2 = O * O * V * V, nvec = O * V + o2v2;
    // [l1; l2], X, l2_old, tau, Hovvo and the DIIS ring; the two- and four-index H-bar elements; the scratch of the build and of an
    // iteration (AB, A, B, q, Zv / ring operand, p1, p2, Lt, two o^4); the Lambda-side operand pair of Lambda-(T) (lt_vt / lt_tt, as
    // so_state_bytes counts vt / tt -- its second block pool is checked where it is allocated, so_lambda_triples)
    const double doubles = (2.0 + (diis_nerr >= 2 ? 1.0 + 2.0 * diis_nerr : 0.0)) * nvec + 3.0 * o2v2 + 2.0 * (O * V + O * O + V * V) +
                           O * O * O * O + 2.0 * O * V * V * V + 2.0 * O * O * O * V + 5.0 * o2v2 + O * V * V * V + 2.0 * O * O * O * V +
                           2.0 * O * O * O * O + (V + O + 16) * (V * V * O + V * O * O);
    return 8.0 * doubles;
}

void so_lambda_free(Context& cx, SOState& s)
{
    so_eom_free(cx, s);   // (they borrow this state's H-bar elements)
    so_response_free(cx, s);
    if (!s.lam) return;
    so_density2_free(cx, *s.lam);
    so_relax_free(cx, *s.lam);
    free_buffers(cx, *s.lam);
    delete s.lam;
    s.lam = nullptr;
}

SOLambda& so_lambda_need(SOState& s, const char* who)
{
    if (!s.lam) throw Error(LAMBDA_ERR_STALE, std::string(who) + ": no Lambda state (call afesp_ccsd_so_lambda_init first)");
    if (s.lam->epoch != s.amp_epoch)
        throw Error(LAMBDA_ERR_STALE, std::string(who) + ": the Lambda state is stale: t1 / t2 may have changed since afesp_ccsd_so_lambda_init (call it again)");
    return *s.lam;
}

void so_lambda_init(Context& cx, SOState& s, int diis_nerr)
{
    so_need_plain(cx, LAM_WHO, LAM_PLAIN);
    if (!s.foo_as_published)
        throw Error(LAMBDA_ERR_FOO,
                    "afesp_ccsd_so_lambda_init: this state keeps the reference's transposed F_mi term, whose equations have no consistent "
                    "Lagrangian (initialise it with AFESP_SO_FOO_AS_PUBLISHED=1)");
    if (diis_nerr < 0 || diis_nerr > 15) throw Error(1, "afesp_ccsd_so_lambda_init: diis_n_errmat must be in 0 .. 15");
    so_lambda_free(cx, s);
    if (!cx.fits(so_lambda_bytes(s.o, s.v, diis_nerr)))
        throw Error(1, "afesp_ccsd_so_lambda_init: the Lambda state of this system does not fit the free device memory");
    preload_lambda_so();
    const auto C = contractor(cx);
    auto P = [&](double al, const Tensor& in, const char* li, double be, const Tensor& out, const char* lo) {
        permute_add(cx, al, in, li, be, out, lo);
    };
    const int o = s.o, v = s.v;
    const int64_t O = o, V = v, ov = O * V, o2v2 = O * O * V * V;
    s.lam = new SOLambda();
    SOLambda& L = *s.lam;
    try {
        L.nvec = ov + o2v2;
        L.amp = cx.alloc(L.nvec);
        L.l1 = view(L.amp, {O, V}); L.l2 = view(L.amp + ov, {O, O, V, V});
        double* res = cx.alloc(L.nvec);
        L.x1 = view(res, {O, V}); L.x2 = view(res + ov, {O, O, V, V});
        L.l2_old = cx.tensor({O, O, V, V});
        L.tau = cx.tensor({O, O, V, V});
        L.Hov = cx.tensor({O, V}); L.Hoo = cx.tensor({O, O}); L.Hvv = cx.tensor({V, V});
        L.Hoooo = cx.tensor({O, O, O, O});
        L.Hvovv = cx.tensor({V, O, V, V}); L.Hooov = cx.tensor({O, O, O, V});
        L.Hovvo = cx.tensor({O, V, V, O});
        L.Hvvvo = cx.tensor({O, V, V, V});
        L.Hovoo = cx.tensor({O, V, O, O});
        L.Gvv = cx.tensor({V, V}); L.Goo = cx.tensor({O, O});
        diis_alloc(cx, L, diis_nerr);

        const Tensor &t1 = s.t1, &t2 = s.t2, &tau = L.tau;
        // (every state has o, v >= 1 -- so_init, so_init_uhf -- so no element-wise launch of this unit is empty)
        LAUNCH(lam_tau_kernel, grid_for(o2v2, SO_GRID_CAP), L.tau.d, t1.d, t2.d, o, v);
        // ---- one-body elements
        C(1.0, s.oovv, "mnef", t1, "nf", 0.0, L.Hov, "me");
        C(1.0, s.ooov, "mnie", t1, "ne", 0.0, L.Hoo, "mi");
        C(0.5, tau, "inef", s.oovv, "mnef", 1.0, L.Hoo, "mi");
        C(1.0, s.ovvv, "mafe", t1, "mf", 0.0, L.Hvv, "ae");
        C(-0.5, tau, "mnaf", s.oovv, "mnef", 1.0, L.Hvv, "ae");
        if (s.fock) {
            k_axpby(cx, L.Hov.d, 1.0, s.f_ov.d, 1.0, ov);
            C(1.0, s.f_ov, "me", t1, "ie", 1.0, L.Hoo, "mi");
            k_axpby(cx, L.Hoo.d, 1.0, s.f_oo.d, 1.0, O * O);
            C(-1.0, t1, "ma", s.f_ov, "me", 1.0, L.Hvv, "ae");
            k_axpby(cx, L.Hvv.d, 1.0, s.f_vv.d, 1.0, V * V);
        }
        // ---- H_mnij = <mn||ij> + P(ij) t_je <mn||ie> + 1/2 tau_ijef <mn||ef>
        Tensor sc = view(cx.scratch("lam_sc_oooo", O * O * O * O), {O, O, O, O});
        C(1.0, s.ooov, "mnie", t1, "je", 0.0, sc, "mnij");
        k_copy(cx, L.Hoooo.d, s.oooo.d, s.oooo.size());
        P(1.0, sc, "mnij", 1.0, L.Hoooo, "mnij");
        P(-1.0, sc, "mnji", 1.0, L.Hoooo, "mnij");
        C(0.5, s.oovv, "mnef", tau, "ijef", 1.0, L.Hoooo, "mnij");
        // ---- H_amef = <am||ef> - t_na <nm||ef>,  H_mnie = <mn||ie> + t_if <mn||fe>
        k_copy(cx, L.Hvovv.d, s.vovv.d, s.vovv.size());
        C(-1.0, t1, "na", s.oovv, "nmef", 1.0, L.Hvovv, "amef");
        k_copy(cx, L.Hooov.d, s.ooov.d, s.ooov.size());
        C(-1.0, s.oovv, "mnef", t1, "if", 1.0, L.Hooov, "mnie");
        // ---- H_mbej = <mb||ej> + t_jf <mb||ef> - t_nb <mn||ej> - (t_jnfb + t_jf t_nb) <mn||ef>
        Tensor ro = view(cx.scratch("lam_ring_operand", o2v2), {O, V, O, V});
        k_copy(cx, L.Hovvo.d, s.ovvo.d, s.ovvo.size());
        C(1.0, s.ovvv, "mbef", t1, "jf", 1.0, L.Hovvo, "mbej");
        C(1.0, t1, "nb", s.oovo, "nmej", 1.0, L.Hovvo, "mbej");
        LAUNCH(lam_ring_operand_kernel, grid_for(o2v2, SO_GRID_CAP), ro.d, t1.d, t2.d, o, v);
        C(-1.0, s.oovv, "mnef", ro, "nfjb", 1.0, L.Hovvo, "mbej");
        // ---- what H_abei and H_mbij share: q(m,b,e,i) = <mb||ei> - t_nibf <mn||ef>
        Tensor q = view(cx.scratch("lam_q", o2v2), {O, V, V, O});
        k_copy(cx, q.d, s.ovvo.d, s.ovvo.size());
        C(-1.0, s.oovv, "mnef", t2, "nibf", 1.0, q, "mbei");
        // ---- H_abei, stored (i,e,a,b):  <ab||ei> - H_me t_miab + t_if W_abef + 1/2 tau_mnab <mn||ei> - P(ab) t_miaf <mb||ef> - P(ab) t_ma q_mbei.
        // W_abef is not formed: its bare part is the one o v^4 product of the Lambda equations (done once, here, on vvvv itself), its
        // t1 parts go through Zv(m,i,a,e) = t_if <am||ef>, and its tau part joins 1/2 tau_mnab <mn||ei> as -1/2 tau_mnab H_mnie
        Tensor Zv = view(cx.scratch("lam_Zv", o2v2), {O, O, V, V});
        Tensor p1 = view(cx.scratch("lam_p1", O * V * V * V), {O, V, V, V});
        C(1.0, t1, "if", s.vovv, "amef", 0.0, Zv, "miae");
        P(1.0, s.vovv, "eiab", 0.0, L.Hvvvo, "ieab");
        C(-1.0, L.Hov, "me", t2, "miab", 1.0, L.Hvvvo, "ieab");
        C(1.0, t1, "if", s.vvvv, "abef", 1.0, L.Hvvvo, "ieab");
        C(-0.5, tau, "mnab", L.Hooov, "mnie", 1.0, L.Hvvvo, "ieab");
        C(-1.0, t2, "miaf", s.ovvv, "mbef", 0.0, p1, "ieab");
        C(-1.0, t1, "ma", q, "mbei", 1.0, p1, "ieab");
        C(-1.0, t1, "mb", Zv, "miae", 1.0, p1, "ieab");
        P(1.0, p1, "ieab", 1.0, L.Hvvvo, "ieab");
        P(-1.0, p1, "ieba", 1.0, L.Hvvvo, "ieab");
        // ---- H_mbij = <mb||ij> - H_me t_ijbe - t_nb H_mnij + 1/2 tau_ijef <mb||ef> + P(ij) t_jnbe <mn||ie> + P(ij) t_ie q_mbej
        Tensor p2 = view(cx.scratch("lam_p2", O * V * O * O), {O, V, O, O});
        k_copy(cx, L.Hovoo.d, s.ovoo.d, s.ovoo.size());
        C(-1.0, L.Hov, "me", t2, "ijbe", 1.0, L.Hovoo, "mbij");
        C(-1.0, t1, "nb", L.Hoooo, "mnij", 1.0, L.Hovoo, "mbij");
        C(0.5, tau, "ijef", s.ovvv, "mbef", 1.0, L.Hovoo, "mbij");
        C(1.0, t2, "jnbe", s.ooov, "mnie", 0.0, p2, "mbij");
        C(1.0, t1, "ie", q, "mbej", 1.0, p2, "mbij");
        P(1.0, p2, "mbij", 1.0, L.Hovoo, "mbij");
        P(-1.0, p2, "mbji", 1.0, L.Hovoo, "mbij");
        // ---- start: l = t (l2_old = 0 from the zero-filled allocation, as the T iteration's t2_old)
        k_copy(cx, L.amp, s.amp, L.nvec);
        L.pseudo = L.pseudo_old = L.rms = 0.0;
        L.epoch = s.amp_epoch;
        L.stamp = ++cx.lam_clock;
        cx.sync();
    } catch (...) {
        try { cx.quiesce(); so_lambda_free(cx, s); } catch (...) {}
        throw;
    }
}

void so_lambda_iterate(Context& cx, SOState& s)
{
    so_need_plain(cx, LAM_WHO, LAM_PLAIN);
    SOLambda& L = so_lambda_need(s, "afesp_ccsd_so_lambda_iterate");
    const auto C = contractor(cx);
    const int o = s.o, v = s.v;
    const int64_t O = o, V = v, ov = O * V, o2v2 = O * O * V * V;
    const Tensor &l1 = L.l1, &l2 = L.l2;
    L.stamp = ++cx.lam_clock;
    diis_save(cx, L);
    build_G(cx, s, L);
    // ---- l1: H_ia + l_ie H_ea - l_ma H_im + l_me H_ieam + 1/2 l_imef H_efam - 1/2 l_mnae H_iemn - G_ef H_eifa - G_mn H_mina
    k_copy(cx, L.x1.d, L.Hov.d, ov);
    C(1.0, l1, "ie", L.Hvv, "ea", 1.0, L.x1, "ia");
    C(-1.0, L.Hoo, "im", l1, "ma", 1.0, L.x1, "ia");
    C(1.0, l1, "me", L.Hovvo, "ieam", 1.0, L.x1, "ia");
    C(0.5, l2, "imef", L.Hvvvo, "maef", 1.0, L.x1, "ia");
    C(-0.5, l2, "mnae", L.Hovoo, "iemn", 1.0, L.x1, "ia");
    C(-1.0, L.Gvv, "ef", L.Hvovv, "eifa", 1.0, L.x1, "ia");
    C(-1.0, L.Goo, "mn", L.Hooov, "mina", 1.0, L.x1, "ia");
    // ---- l2
    Tensor AB = view(cx.scratch("so_AB", o2v2), {O, O, V, V}), A = view(cx.scratch("so_A", o2v2), {O, O, V, V});
    Tensor Bm = view(cx.scratch("so_B", o2v2), {O, O, V, V});
    Tensor Lt = view(cx.scratch("lam_Lt", O * O * O * V), {O, O, O, V});
    Tensor Loo = view(cx.scratch("lam_Loo", O * O * O * O), {O, O, O, O});
    // 1/2 l_ijef H_efab as so_ladder treats 1/2 tau_ijef W_abef: the bare part over antisymmetric pairs against va, the t1 parts
    // through Lt(i,j,m,e) = l_ijef t_mf, the tau part as (l . tau over ef) -> o^4, then x <mn||ab>;  + 1/2 l_mnab H_ijmn
    so_ladder_bare(cx, s, l2, L.x2);
    C(1.0, l2, "ijef", s.t1, "mf", 0.0, Lt, "ijme");
    C(-1.0, Lt, "ijme", s.vovv, "emab", 1.0, L.x2, "ijab");
    C(1.0, l2, "ijef", L.tau, "mnef", 0.0, Loo, "ijmn");
    C(0.25, Loo, "ijmn", s.oovv, "mnab", 1.0, L.x2, "ijab");
    C(0.5, L.Hoooo, "ijmn", l2, "mnab", 1.0, L.x2, "ijab");
    // P(ij)P(ab) l_imae H_jebm  (the disconnected l_ia H_jb joins it in the assemble kernel)
    C(1.0, l2, "imae", L.Hovvo, "jebm", 0.0, AB, "ijab");
    // P(ij) [ -l_imab H_jm + l_ie H_ejab - <im||ab> G_mj ]
    C(-1.0, L.Hoo, "jm", l2, "imab", 0.0, A, "ijab");
    C(1.0, l1, "ie", L.Hvovv, "ejab", 1.0, A, "ijab");
    C(-1.0, s.oovv, "imab", L.Goo, "mj", 1.0, A, "ijab");
    // P(ab) [ l_ijae H_eb - l_ma H_ijmb + <ij||ae> G_be ]
    C(1.0, l2, "ijae", L.Hvv, "eb", 0.0, Bm, "ijab");
    C(-1.0, L.Hooov, "ijmb", l1, "ma", 1.0, Bm, "ijab");
    C(1.0, s.oovv, "ijae", L.Gvv, "be", 1.0, Bm, "ijab");
    // l2 first (it reads the l1 the iteration started from), then l1 = x1 / D, then the fixed-order sums
    const int nblk = (int)std::min<int64_t>((o2v2 + TB - 1) / TB, MAXBLK);
    double* partial = cx.scratch("lam_partial", 2 * MAXBLK);
    LAUNCH(lam_l2_assemble_kernel, nblk, L.l2.d, L.l2_old.d, partial, L.x2.d, s.oovv.d, AB.d, A.d, Bm.d, L.l1.d, L.Hov.d, s.D2.d, o, v);
    k_div(cx, L.l1.d, L.x1.d, s.D1.d, ov);
    so_sum2(cx, cx.scal, partial, 2, nblk, s.fock ? s.f_ov.d : (const double*)nullptr, L.l1.d, ov);
}

void so_lambda_energy(Context& cx, SOState& s)
{
    so_need_plain(cx, LAM_WHO, LAM_PLAIN);
    SOLambda& L = so_lambda_need(s, "afesp_ccsd_so_lambda_energy");
    const int64_t n2 = L.l2.size();
    const int nblk = (int)std::min<int64_t>((n2 + TB - 1) / TB, MAXBLK);
    double* partial = cx.scratch("lam_partial", 2 * MAXBLK);
    LAUNCH(lam_energy_kernel, nblk, partial, s.oovv.d, L.l2.d, L.l2_old.d, n2);
    so_sum2(cx, cx.scal, partial, 2, nblk, s.fock ? s.f_ov.d : (const double*)nullptr, L.l1.d, (int64_t)s.o * s.v);
}

int so_lambda_read(Context& cx, SOState& s, double e_tol, double l_tol)
{
    SOLambda& L = so_lambda_need(s, "afesp_ccsd_so_lambda");
    double* h = host_scalars(cx, DIIS_FLAG_SLOT + 1);
    diis_check_flag(cx, h);
    L.pseudo_old = L.pseudo;
    L.pseudo = h[0];
    L.rms = h[1];
    return (std::sqrt(h[1]) < l_tol && std::fabs(L.pseudo - L.pseudo_old) < e_tol) ? 1 : 0;
}

double* so_density_device(Context& cx, SOState& s, const char* who)
{
    SOLambda& L = so_lambda_need(s, who);
    const int o = s.o, v = s.v;
    const int64_t O = o, V = v, N = O + V;
    const auto C = contractor(cx);
    Tensor doo = view(cx.scratch("lam_doo", O * O), {O, O}), dvv = view(cx.scratch("lam_dvv", V * V), {V, V});
    Tensor dov = view(cx.scratch("lam_dov", O * V), {O, V});
    double* D = cx.scratch("lam_density", N * N);
    build_G(cx, s, L);
    // dL/df_mi = -l_ia t_ma - G_mi;  dL/df_ae = l_ia t_ie - G_ae;
    // dL/df_me = t_me + l_me + l_ia t_imae - l_ia t_ie t_ma + G_be t_mb - G_mj t_je  (the two middle terms: -t_mb dL/df_be)
    C(-1.0, s.t1, "ma", L.l1, "ia", 0.0, doo, "mi");
    k_axpby(cx, doo.d, -1.0, L.Goo.d, 1.0, O * O);
    C(1.0, L.l1, "ia", s.t1, "ie", 0.0, dvv, "ae");
    k_axpby(cx, dvv.d, -1.0, L.Gvv.d, 1.0, V * V);
    C(1.0, L.l1, "ia", s.t2, "imae", 0.0, dov, "me");
    C(-1.0, s.t1, "mb", dvv, "be", 1.0, dov, "me");
    C(-1.0, L.Goo, "mj", s.t1, "je", 1.0, dov, "me");
    so_density_assemble(cx, s, D, doo.d, dvv.d, dov.d, nullptr, L.l1.d, 1.0, 0.0);
    return D;
}

void so_density_assemble(Context& cx, SOState& s, double* D, const double* doo, const double* dvv, const double* dov, const double* r1,
                         const double* L1, double w, double l0)
{
    const int64_t N = (int64_t)s.o + s.v;
    // (a state holds v^4 integrals, so N^2 elements stay far below either cap of grid_for: one block per TB elements, whoever calls)
    LAUNCH(so_density_assemble_kernel, grid_for(N * N, SO_GRID_CAP), D, doo, dvv, dov, s.t1.d, r1, L1, w, l0, s.o, s.v);
}

void so_density(Context& cx, SOState& s, double* d_host, int64_t capacity)
{
    so_need_plain(cx, LAM_WHO, LAM_PLAIN);
    so_lambda_need(s, "afesp_ccsd_so_density");
    const int64_t N = (int64_t)s.o + s.v;
    if (!d_host || capacity < N * N)
        throw Error(LAMBDA_ERR_CAPACITY, "afesp_ccsd_so_density: the buffer holds " + std::to_string(d_host ? capacity : 0) + " doubles, the density needs (o + v)^2 = " +
                                             std::to_string(N * N));
    const double* D = so_density_device(cx, s, "afesp_ccsd_so_density");
    AFESP_HIP(hipMemcpyAsync(d_host, D, sizeof(double) * N * N, hipMemcpyDeviceToHost, cx.stream));
    cx.sync();
}

}  // namespace afesp
