// eom_left_so.hip -- the left-hand side of EOM-EE-CCSD on the spin-orbital CCSD state (eom_so.h): the left sigma build
// sigma_L(l) = A^T l, the coupling of right vectors to the reference, and the one-particle density as a bilinear form of a left pair
// (l0, l) and a right pair (r0, r).  Term by term in the letters of tests/np_eom_left.py (lsigma_explicit, density_explicit) over the
// H-bar elements of the live Lambda state, which are borrowed and never written.  The left Davidson state is a second user of
// davidson_so.h (eom_so.hip).  Launches are plain call-by-call ones; every reduction is block partials, then an ordered final sum.
#include "device_util.h"
#include "eom_so.h"

namespace afesp {
namespace {

// sigma2 from the ladder block and the three permutation carriers, and sigma1's diagonal term (threads x < o v):
//   sigma2 = lad + P(ij)P(ab) (AB + l1 Hov) + P(ij) A + P(ab) Bm - D2 l2,   sigma1 -= D1 l1.
// lad is antisymmetric in both pairs, A in a,b and Bm in i,j -- as sums of products only up to rounding.  With c = 1/4 lad + AB +
// l_ia H_jb + 1/2 (A + Bm) the value is (c(ijab) + c(jiba)) - (c(jiab) + c(ijba)): the weights make that sum the P-form, and exchanging
// i and j, or a and b, exchanges the two brackets, so the value is negated to the bit and vanishes on the diagonals; D2 enters as the
// mean of its four images for the same reason.
__device__ __forceinline__ double eom_lcarrier(const double* lad, const double* AB, const double* A, const double* Bm, const double* l1,
                                               const double* Hov, int64_t p, int i, int j, int a, int b, int o)
{
    const double conn = __dadd_rn(__dadd_rn(__dmul_rn(0.25, lad[p]), AB[p]), __dmul_rn(0.5, __dadd_rn(A[p], Bm[p])));
    return __dadd_rn(conn, __dmul_rn(l1[i + o * a], Hov[j + o * b]));
}
__global__ void eom_lsigma_assemble_kernel(double* s2, double* s1, const double* lad, const double* AB, const double* A, const double* Bm,
                                           const double* l2, const double* l1, const double* Hov, const double* D2, const double* D1, int o, int v)
{
    const int64_t n2 = (int64_t)o * o * v * v, n1 = (int64_t)o * v;
    GRID_STRIDE(x, n2)
    {
        const auto [i, j, a, b] = oovv_decode(x, o, v);
        const auto [ji, ba, jiba] = oovv_images(i, j, a, b, o, v);
        const double same = __dadd_rn(eom_lcarrier(lad, AB, A, Bm, l1, Hov, x, i, j, a, b, o), eom_lcarrier(lad, AB, A, Bm, l1, Hov, jiba, j, i, b, a, o));
        const double swapped = __dadd_rn(eom_lcarrier(lad, AB, A, Bm, l1, Hov, ji, j, i, a, b, o), eom_lcarrier(lad, AB, A, Bm, l1, Hov, ba, i, j, b, a, o));
        const double d = __dmul_rn(0.25, __dadd_rn(__dadd_rn(D2[x], D2[jiba]), __dadd_rn(D2[ji], D2[ba])));
        s2[x] = __dadd_rn(__dadd_rn(same, -swapped), -__dmul_rn(d, l2[x]));
        if (x < n1) s1[x] = __dadd_rn(s1[x], -__dmul_rn(D1[x], l1[x]));   // (o v <= o^2 v^2: every single has its thread)
    }
}

// block partials of so_eom_wdot (eom_so.h)
__global__ void eom_wdot_kernel(double* partial, const double* a1, const double* a2, const double* y, int64_t n1, int64_t n2)
{
    __shared__ double sm[4];
    double acc[1] = {0.0};
    GRID_STRIDE(x, n1 + n2) acc[0] += x < n1 ? a1[x] * y[x] : 0.25 * a2[x - n1] * y[x];
    block_sum<1>(acc, sm);
    if (threadIdx.x == 0) partial[blockIdx.x] = acc[0];
}

// G_vv / G_oo of (x2, l2) into buffers of the caller: G_ae = -1/2 x_mnef l_mnaf, G_mi = 1/2 x_mnef l_inef
void build_G(Context& cx, const Tensor& x2, const Tensor& l2, const Tensor& Gvv, const Tensor& Goo)
{
    contract(cx, -0.5, x2, "mnef", l2, "mnaf", 0.0, Gvv, "ae");
    contract(cx, 0.5, x2, "mnef", l2, "inef", 0.0, Goo, "mi");
}

}  // namespace

const double* so_eom_wdot(Context& cx, const double* a1, const double* a2, const double* y, int64_t n1, int64_t n2)
{
    preload_eom_left_so();
    const int nblk = davidson_reduce_blocks(n1 + n2);
    double* partial = cx.scratch("eoml_partial", nblk + 1);   // (the sum behind the partials)
    LAUNCH(eom_wdot_kernel, dim3(nblk), partial, a1, a2, y, n1, n2);
    davidson_reduce_final(cx, partial + nblk, partial, 1, nblk);
    return partial + nblk;
}

void preload_eom_left_so()
{
    static const bool loaded = [] {
        first_use_touch(reinterpret_cast<const void*>(eom_lsigma_assemble_kernel));
        first_use_touch(reinterpret_cast<const void*>(eom_wdot_kernel));
        (void)hipGetLastError();
        return true;
    }();
    (void)loaded;
}

double so_eom_left_bytes(int64_t o, int64_t v, int nroots, int max_space)
{
    const double O = (double)o, V = (double)v, nvec = O * V + O * O * V * V;
    // the Davidson state and the scratch of a sigma build are those of the right-hand side (lad, AB, A, B, Lt for Z, the o^4 product, G_vv,
    // G_oo, two staging vectors); a density call adds two staging vectors, four G, three blocks, d_vv of t, L1 and the matrix
    return so_eom_bytes(o, v, nroots, max_space) + 8.0 * (2.0 * nvec + 6.0 * (V * V + O * O) + 2.0 * O * V + (O + V) * (O + V) + 256.0);
}

void so_eom_lsigma(Context& cx, SOState& s, const double* l, double* sigma)
{
    so_need_plain(cx, EOM_WHO, EOM_PLAIN);
    SOLambda& L = so_lambda_need(s, "afesp_ccsd_so_eom_lsigma");
    preload_eom_left_so();
    const auto C = contractor(cx);
    const int o = s.o, v = s.v;
    const int64_t O = o, V = v, ov = O * V, o2v2 = O * O * V * V;
    const Tensor l1 = view(const_cast<double*>(l), {O, V}), l2 = view(const_cast<double*>(l) + ov, {O, O, V, V});
    const Tensor s1 = view(sigma, {O, V});
    // G_vv / G_oo of this l2, in buffers of this build (the Lambda state's own are those of its l2)
    Tensor Gvv = view(cx.scratch("eoml_Gvv", V * V), {V, V}), Goo = view(cx.scratch("eoml_Goo", O * O), {O, O});
    build_G(cx, s.t2, l2, Gvv, Goo);
    // ---- sigma1: l_ie H_ea - l_ma H_im + l_me H_ieam + 1/2 l_imef H_efam - 1/2 l_mnae H_iemn - G_ef H_eifa - G_mn H_mina
    //      (- D1 l1: the assemble kernel; no H_ia: sigma is linear)
    C(1.0, l1, "ie", L.Hvv, "ea", 0.0, s1, "ia");
    C(-1.0, L.Hoo, "im", l1, "ma", 1.0, s1, "ia");
    C(1.0, l1, "me", L.Hovvo, "ieam", 1.0, s1, "ia");
    C(0.5, l2, "imef", L.Hvvvo, "maef", 1.0, s1, "ia");
    C(-0.5, l2, "mnae", L.Hovoo, "iemn", 1.0, s1, "ia");
    C(-1.0, Gvv, "ef", L.Hvovv, "eifa", 1.0, s1, "ia");
    C(-1.0, Goo, "mn", L.Hooov, "mina", 1.0, s1, "ia");
    // ---- sigma2
    Tensor lad = view(cx.scratch("eom_lad", o2v2), {O, O, V, V});
    Tensor AB = view(cx.scratch("so_AB", o2v2), {O, O, V, V}), A = view(cx.scratch("so_A", o2v2), {O, O, V, V});
    Tensor Bm = view(cx.scratch("so_B", o2v2), {O, O, V, V});
    Tensor Lt = view(cx.scratch("lam_Lt", O * O * O * V), {O, O, O, V});
    Tensor Loo = view(cx.scratch("lam_Loo", O * O * O * O), {O, O, O, O});
    // 1/2 l_ijef H_efab as the Lambda iteration treats it: the bare part over antisymmetric pairs against va, the t1 parts through
    // Lt(i,j,m,e) = l_ijef t_mf, the tau part as (l . tau over ef) -> o^4, then x <mn||ab>;  + 1/2 l_mnab H_ijmn
    so_ladder_bare(cx, s, l2, lad);
    C(1.0, l2, "ijef", s.t1, "mf", 0.0, Lt, "ijme");
    C(-1.0, Lt, "ijme", s.vovv, "emab", 1.0, lad, "ijab");
    C(1.0, l2, "ijef", L.tau, "mnef", 0.0, Loo, "ijmn");
    C(0.25, Loo, "ijmn", s.oovv, "mnab", 1.0, lad, "ijab");
    C(0.5, L.Hoooo, "ijmn", l2, "mnab", 1.0, lad, "ijab");
    // P(ij)P(ab) l_imae H_jebm  (the disconnected l_ia H_jb joins it in the assemble kernel)
    C(1.0, l2, "imae", L.Hovvo, "jebm", 0.0, AB, "ijab");
    // P(ij) [ -l_imab H_jm + l_ie H_ejab - <im||ab> G_mj ]
    C(-1.0, L.Hoo, "jm", l2, "imab", 0.0, A, "ijab");
    C(1.0, l1, "ie", L.Hvovv, "ejab", 1.0, A, "ijab");
    C(-1.0, s.oovv, "imab", Goo, "mj", 1.0, A, "ijab");
    // P(ab) [ l_ijae H_eb - l_ma H_ijmb + <ij||ae> G_be ]
    C(1.0, l2, "ijae", L.Hvv, "eb", 0.0, Bm, "ijab");
    C(-1.0, L.Hooov, "ijmb", l1, "ma", 1.0, Bm, "ijab");
    C(1.0, s.oovv, "ijae", Gvv, "be", 1.0, Bm, "ijab");
    LAUNCH(eom_lsigma_assemble_kernel, grid_for(o2v2), sigma + ov, sigma, lad.d, AB.d, A.d, Bm.d, l2.d, l1.d, L.Hov.d, s.D2.d, s.D1.d, o, v);
}

void so_eom_ref_coupling(Context& cx, SOState& s, int nvec, const double* r1, const double* r2, double* c)
{
    so_need_plain(cx, EOM_WHO, EOM_PLAIN);
    SOLambda& L = so_lambda_need(s, "afesp_ccsd_so_eom_ref_coupling");
    if (nvec < 1 || !r1 || !r2 || !c) throw Error(1, "afesp_ccsd_so_eom_ref_coupling: nvec < 1 or a NULL vector");
    preload_eom_left_so();
    const int64_t O = s.o, V = s.v, ov = O * V, o2v2 = O * O * V * V;
    double* r = cx.scratch("eom_r_stage", ov + o2v2);
    for (int k = 0; k < nvec; ++k) {
        AFESP_HIP(hipMemcpyAsync(r, r1 + ov * k, sizeof(double) * ov, hipMemcpyHostToDevice, cx.stream));
        AFESP_HIP(hipMemcpyAsync(r + ov, r2 + o2v2 * k, sizeof(double) * o2v2, hipMemcpyHostToDevice, cx.stream));
        const double* out = so_eom_wdot(cx, L.Hov.d, s.oovv.d, r, ov, o2v2);
        AFESP_HIP(hipMemcpyAsync(c + k, out, sizeof(double), hipMemcpyDeviceToHost, cx.stream));
        cx.sync();
    }
}

void so_eom_density(Context& cx, SOState& s, double l0, const double* l1h, const double* l2h, double r0, const double* r1h, const double* r2h,
                    double* d_host, int64_t capacity)
{
    so_need_plain(cx, EOM_WHO, EOM_PLAIN);
    so_lambda_need(s, "afesp_ccsd_so_eom_density");
    const int o = s.o, v = s.v;
    const int64_t O = o, V = v, N = O + V, ov = O * V, o2v2 = O * O * V * V;
    if ((l1h == nullptr) != (l2h == nullptr) || (r1h == nullptr) != (r2h == nullptr))
        throw Error(1, "afesp_ccsd_so_eom_density: l1 / l2 are both NULL or both given, and so are r1 / r2");
    if (!d_host || capacity < N * N)
        throw Error(LAMBDA_ERR_CAPACITY, "afesp_ccsd_so_eom_density: the buffer holds " + std::to_string(d_host ? capacity : 0) +
                                             " doubles, the density needs (o + v)^2 = " + std::to_string(N * N));
    preload_eom_left_so();
    const auto C = contractor(cx);
    const bool hasl = l1h != nullptr, hasr = r1h != nullptr;
    Tensor l1, l2, r1, r2;
    if (hasl) {
        double* l = cx.scratch("eoml_l_stage", ov + o2v2);
        AFESP_HIP(hipMemcpyAsync(l, l1h, sizeof(double) * ov, hipMemcpyHostToDevice, cx.stream));
        AFESP_HIP(hipMemcpyAsync(l + ov, l2h, sizeof(double) * o2v2, hipMemcpyHostToDevice, cx.stream));
        l1 = view(l, {O, V}); l2 = view(l + ov, {O, O, V, V});
    }
    if (hasr) {
        double* r = cx.scratch("eom_r_stage", ov + o2v2);
        AFESP_HIP(hipMemcpyAsync(r, r1h, sizeof(double) * ov, hipMemcpyHostToDevice, cx.stream));
        AFESP_HIP(hipMemcpyAsync(r + ov, r2h, sizeof(double) * o2v2, hipMemcpyHostToDevice, cx.stream));
        r1 = view(r, {O, V}); r2 = view(r + ov, {O, O, V, V});
    }
    // ---- w = l0 r0 + <l, r>: the weight of the lone t_me term
    double w = l0 * r0;
    if (hasl && hasr) {
        double lr = 0.0;
        const double* out = so_eom_wdot(cx, l1.d, l2.d, r1.d, ov, o2v2);
        AFESP_HIP(hipMemcpyAsync(&lr, out, sizeof(double), hipMemcpyDeviceToHost, cx.stream));
        cx.sync();
        w += lr;
    }
    const Tensor &t1 = s.t1, &t2 = s.t2;
    Tensor doo = view(cx.scratch("eoml_doo", O * O), {O, O}), dvv = view(cx.scratch("eoml_dvv", V * V), {V, V});
    Tensor dov = view(cx.scratch("eoml_dov", ov), {O, V});
    double* D = cx.scratch("eoml_density", N * N);
    k_fill(cx, doo.d, O * O, 0.0);
    k_fill(cx, dvv.d, V * V, 0.0);
    k_fill(cx, dov.d, ov, 0.0);
    Tensor L1;
    if (hasl) {
        Tensor GvvT = view(cx.scratch("eoml_GvvT", V * V), {V, V}), GooT = view(cx.scratch("eoml_GooT", O * O), {O, O});
        L1 = view(cx.scratch("eoml_L1", ov), {O, V});
        build_G(cx, t2, l2, GvvT, GooT);
        // ---- the lambda part: the ground-state formulas with lambda -> (L1, r0 l2), L1 = r0 l1 + y, where y_jb = l_ijab r_ia carries the
        // disconnected term (it multiplies R1 as a lambda_1 does)
        k_fill(cx, L1.d, ov, 0.0);
        k_axpby(cx, L1.d, r0, l1.d, 1.0, ov);
        if (hasr) C(1.0, l2, "ijab", r1, "ia", 1.0, L1, "jb");
        C(-1.0, t1, "ma", L1, "ia", 1.0, doo, "mi");
        k_axpby(cx, doo.d, -r0, GooT.d, 1.0, O * O);
        C(1.0, L1, "ia", t1, "ie", 1.0, dvv, "ae");
        k_axpby(cx, dvv.d, -r0, GvvT.d, 1.0, V * V);
        C(1.0, L1, "ia", t2, "imae", 1.0, dov, "me");
        C(-r0, GooT, "mj", t1, "je", 1.0, dov, "me");
        if (hasr) {
            // ---- the sigma part: the derivative of the lambda part along r.  oo and vv blocks from l1 . r1 and l2 . r2 ...
            Tensor GvvR = view(cx.scratch("eoml_GvvR", V * V), {V, V}), GooR = view(cx.scratch("eoml_GooR", O * O), {O, O});
            Tensor dvvT = view(cx.scratch("eoml_dvvT", V * V), {V, V});
            build_G(cx, r2, l2, GvvR, GooR);
            C(-1.0, r1, "ma", l1, "ia", 1.0, doo, "mi");
            k_axpby(cx, doo.d, -1.0, GooR.d, 1.0, O * O);
            C(1.0, l1, "ia", r1, "ie", 1.0, dvv, "ae");
            k_axpby(cx, dvv.d, -1.0, GvvR.d, 1.0, V * V);
            // ... and the ov-block chains through t1 / t2: l_ia r_imae - r_mb (l_ia t_ie - G_be(t)) - G_mj(r) t_je - G_mj(t) r_je
            C(1.0, l1, "ia", t1, "ie", 0.0, dvvT, "ae");
            k_axpby(cx, dvvT.d, -1.0, GvvT.d, 1.0, V * V);
            C(1.0, l1, "ia", r2, "imae", 1.0, dov, "me");
            C(-1.0, r1, "mb", dvvT, "be", 1.0, dov, "me");
            C(-1.0, GooR, "mj", t1, "je", 1.0, dov, "me");
            C(-1.0, GooT, "mj", r1, "je", 1.0, dov, "me");
        }
        C(-1.0, t1, "mb", dvv, "be", 1.0, dov, "me");   // (the whole vv block, both parts: -t_mb d_be)
    }
    so_density_assemble(cx, s, D, doo.d, dvv.d, dov.d, hasr ? r1.d : (const double*)nullptr, hasl ? L1.d : (const double*)nullptr, w, l0);
    AFESP_HIP(hipMemcpyAsync(d_host, D, sizeof(double) * N * N, hipMemcpyDeviceToHost, cx.stream));
    cx.sync();
}

}  // namespace afesp
