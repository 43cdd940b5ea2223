// eom_so.hip -- EOM-EE-CCSD on the spin-orbital CCSD state (eom_so.h): the sigma build sigma(r) = A r, term by term in
// the letters of tests/np_eom.py (sigma_explicit) over the H-bar elements of the live Lambda state, the diagonal and the guesses, for the
// block Davidson iteration of davidson_so.h on the non-symmetric A.  Launches are plain call-by-call ones, as Lambda's.
#include "device_util.h"
#include "eom_so.h"

namespace afesp {
namespace {

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

// a guess: +1 at i0 and i1, -1 at i2 and i3 (negative index: none) of a vector that is zero otherwise
__global__ void eom_unit_kernel(double* x, int64_t nvec, int64_t i0, int64_t i1, int64_t i2, int64_t i3)
{
    GRID_STRIDE(e, nvec) x[e] = (e == i0 || e == i1) ? 1.0 : ((e == i2 || e == i3) ? -1.0 : 0.0);
}

// The diagonal guess of A as the Davidson unit reads it (corr = rho / (omega - diag)): diag = -D, D = D1 on the singles and the mean of D2
// and its a,b image behind them.  (D2 is summed as ((e_i + e_j) - e_a) - e_b: symmetric in i,j to the bit, in a,b only with its image -- the
// corrections stay antisymmetric to the bit as the basis vectors are.)
__global__ void eom_diag_kernel(double* diag, const double* D1, const double* D2, int o, int v, int64_t nvec)
{
    const int64_t n1 = (int64_t)o * v;
    GRID_STRIDE(e, nvec)
    {
        double D;
        if (e < n1) D = D1[e];
        else {
            const int64_t x = e - n1, ij = x % ((int64_t)o * o);
            const int a = (int)((x / ((int64_t)o * o)) % v), b = (int)(x / ((int64_t)o * o * v));
            D = __dmul_rn(0.5, __dadd_rn(D2[x], D2[ij + (int64_t)o * o * (b + (int64_t)v * a)]));
        }
        diag[e] = -D;
    }
}

void need_plain(Context& cx)
{
    if (cx.rec) throw Error(1, "so_eom: the EOM equations are not part of a recorded (launch-fused) sequence");
}

}  // namespace

void preload_eom_so()
{
    first_use_touch(reinterpret_cast<const void*>(eom_sigma_assemble_kernel));
    first_use_touch(reinterpret_cast<const void*>(eom_unit_kernel));
    first_use_touch(reinterpret_cast<const void*>(eom_diag_kernel));
    (void)hipGetLastError();
}

double so_eom_bytes(int64_t o, int64_t v, int nroots, int max_space)
{
    const double O = (double)o, V = (double)v, o2v2 = O * O * V * V, nvec = O * V + o2v2;
    // the Davidson state; the scratch of a sigma build (lad, AB, A, B, Z, the o^4 product, Y_vv, Y_oo) and the two staging vectors of the
    // host entry
    return davidson_bytes(nvec, nroots, max_space) + 8.0 * (4.0 * o2v2 + O * O * O * V + O * O * O * O + V * V + O * O + 2.0 * nvec);
}

// the right-hand and the left-hand Davidson state are one type and one code: `left` chooses the slot, the sigma build and the names
static SOEom*& eom_slot(SOState& s, bool left) { return left ? s.eom_left : s.eom; }
static std::string eom_name(bool left, const char* call = "") { return std::string(left ? "afesp_ccsd_so_eom_left_" : "afesp_ccsd_so_eom_") + call; }

static void eom_free_one(Context& cx, SOState& s, bool left)
{
    SOEom*& e = eom_slot(s, left);
    if (!e) return;
    davidson_free(cx, e->d);
    delete e;
    e = nullptr;
}

void so_eom_free(Context& cx, SOState& s)
{
    eom_free_one(cx, s, false);
    eom_free_one(cx, s, true);
}

void so_eom_fill_diag(Context& cx, SOState& s, double* diag)
{
    const int64_t nvec = (int64_t)s.o * s.v + (int64_t)s.o * s.o * s.v * s.v;
    LAUNCH(eom_diag_kernel, grid_for(nvec), diag, s.D1.d, s.D2.d, s.o, s.v, nvec);
}

SOEom& so_eom_need(SOState& s, const char* who, bool left)
{
    so_lambda_need(s, who);
    SOEom* e = eom_slot(s, left);
    if (!e || e->d.epoch != s.amp_epoch)
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
        davidson_alloc(cx, E.d, O * V, nvec, 0.25, left, nroots, max_space,
                       [&](double* diag) { so_eom_fill_diag(cx, s, diag); });
        E.d.epoch = L.epoch;
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

void so_eom_guess(Context& cx, SOState& s, bool left)
{
    need_plain(cx);
    Davidson& E = so_eom_need(s, eom_name(left, "guess").c_str(), left).d;
    const int64_t O = s.o, V = s.v, ov = O * V, o2v2 = O * O * V * V;
    // (the raw D1 / D2, not the unit's symmetrised diagonal: the two can differ in the last bit, and a tie broken differently is another guess set)
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
    davidson_restart(E);
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
    davidson_set_pending_from_host(cx, so_eom_need(s, eom_name(left, "set_guess").c_str(), left).d, eom_name(left), k, r1, r2);
}

int so_eom_iterate(Context& cx, SOState& s, double tol, bool left)
{
    need_plain(cx);
    Davidson& E = so_eom_need(s, eom_name(left, "iterate").c_str(), left).d;
    return davidson_iterate(cx, E, eom_name(left), tol, [&](const double* r, double* sigma) {
        if (left) so_eom_lsigma(cx, s, r, sigma);   // the projected matrix is then <b_p, sigma_L(b_q)>
        else so_eom_sigma(cx, s, r, sigma);
    });
}

void so_eom_get_vector(Context& cx, SOState& s, int k, double* r1, double* r2, bool left)
{
    need_plain(cx);
    davidson_get_vector(cx, so_eom_need(s, eom_name(left, "get_vector").c_str(), left).d, eom_name(left), k, r1, r2);
}

}  // namespace afesp
