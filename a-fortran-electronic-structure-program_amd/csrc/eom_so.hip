// eom_so.hip -- EOM-EE-CCSD on the spin-orbital CCSD state (eom_so.h): the sigma build sigma(r) = A r, term by term in
// the letters of tests/np_eom.py (sigma_explicit) over the H-bar elements of the live Lambda state, the diagonal and the guesses, for the
// block Davidson iteration of davidson_so.h on the non-symmetric A; and the one driver of the six EOM eigenproblems (EE, IP, EA, their left sides)
// over a descriptor per kind.  Launches are plain call-by-call ones, as Lambda's.
#include "device_util.h"
#include "eom_ipea_so.h"

#include <algorithm>

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
        const auto [i, j, a, b] = oovv_decode(x, o, v);
        const auto [ji, ba, jiba] = oovv_images(i, j, a, b, o, v);
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

}  // namespace

void preload_eom_so()
{
    static const bool loaded = [] {
        first_use_touch(reinterpret_cast<const void*>(eom_sigma_assemble_kernel));
        first_use_touch(reinterpret_cast<const void*>(eom_unit_kernel));
        first_use_touch(reinterpret_cast<const void*>(eom_diag_kernel));
        (void)hipGetLastError();
        return true;
    }();
    (void)loaded;
}

double so_eom_bytes(int64_t o, int64_t v, int nroots, int max_space)
{
    const double O = (double)o, V = (double)v, o2v2 = O * O * V * V, nvec = O * V + o2v2;
    // the Davidson state; the scratch of a sigma build (lad, AB, A, B, Z, the o^4 product, Y_vv, Y_oo) and the two staging vectors of the
    // host entry
    return davidson_bytes(nvec, nroots, max_space) + 8.0 * (4.0 * o2v2 + O * O * O * V + O * O * O * O + V * V + O * O + 2.0 * nvec);
}

void so_eom_fill_diag(Context& cx, SOState& s, double* diag)
{
    const int64_t nvec = (int64_t)s.o * s.v + (int64_t)s.o * s.o * s.v * s.v;
    LAUNCH(eom_diag_kernel, grid_for(nvec), diag, s.D1.d, s.D2.d, s.o, s.v, nvec);
}

void so_eom_sigma(Context& cx, SOState& s, const double* r, double* sigma)
{
    so_need_plain(cx, EOM_WHO, EOM_PLAIN);
    SOLambda& L = so_lambda_need(s, "afesp_ccsd_so_eom_sigma");
    const auto C = contractor(cx);
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

// ---- the driver of the six eigenproblems (eom_so.h).  What differs per kind, and nothing else:
namespace {

struct EomProblem {
    std::string prefix;              // of the kind's C entry points: messages name prefix + "init", "guess", "iterate", ...
    const char* state;               // "no <state> state for the live Lambda state"
    const char* space;               // what bounds nroots
    const char* sigma_entry;         // the host sigma entry
    const char *r_stage, *s_stage;   // ... and its staging buffers (Context::scratch caches by name: kinds of different lengths keep their own)
    int64_t n1, n2, nunique;
    double w2;                       // weight of the n2 elements in the metric
    bool follow;                     // the state follows the states of the caller's guesses
    std::function<double(int nroots, int max_space)> bytes;
    void (*preload)();
    std::function<void(Context&, SOState&, double* diag)> fill_diag;
    std::function<void(Context&, SOState&, const double* r, double* sigma)> sigma;
    // the guess: the host sort key of every element, the unique elements behind the first n1 in flat-index order, the unit vector on one
    std::function<std::vector<double>(Context&, SOState&, const Davidson&)> sort_key;
    std::function<void(const SOState&, std::vector<int64_t>&)> unique;
    std::function<void(Context&, SOState&, double* x, int64_t p)> unit;
};

// EE, both sides: -D from the raw D1 / D2, not the unit's symmetrised diagonal -- the two can differ in the last bit, and a tie broken
// differently is another guess set (-D is the diagonal of A^T too: the same unit vectors)
std::vector<double> ee_sort_key(Context& cx, SOState& s, const Davidson&)
{
    const int64_t O = s.o, V = s.v, ov = O * V, o2v2 = O * O * V * V;
    std::vector<double> D(ov + o2v2);
    AFESP_HIP(hipMemcpyAsync(D.data(), s.D1.d, sizeof(double) * ov, hipMemcpyDeviceToHost, cx.stream));
    AFESP_HIP(hipMemcpyAsync(D.data() + ov, s.D2.d, sizeof(double) * o2v2, hipMemcpyDeviceToHost, cx.stream));
    cx.sync();
    for (double& d : D) d = -d;
    return D;
}

void ee_unique(const SOState& s, std::vector<int64_t>& idx)
{
    const int64_t O = s.o, V = s.v;
    for (int64_t b = 0; b < V; ++b)
        for (int64_t a = 0; a < b; ++a)
            for (int64_t j = 0; j < O; ++j)
                for (int64_t i = 0; i < j; ++i) idx.push_back(O * V + i + O * (j + O * (a + V * b)));
}

void ee_unit(Context& cx, SOState& s, double* x, int64_t i0)
{
    const int64_t O = s.o, V = s.v, ov = O * V, nvec = ov + O * O * V * V;
    int64_t i1 = -1, i2 = -1, i3 = -1;
    if (i0 >= ov) {
        const int64_t y = i0 - ov, i = y % O, j = (y / O) % O, a = (y / (O * O)) % V, b = y / (O * O * V);
        i1 = ov + j + O * (i + O * (b + V * a));
        i2 = ov + j + O * (i + O * (a + V * b));
        i3 = ov + i + O * (j + O * (b + V * a));
    }
    LAUNCH(eom_unit_kernel, grid_for(nvec), x, nvec, i0, i1, i2, i3);
}

// IP / EA: the unit's own diagonal
std::vector<double> diag_sort_key(Context& cx, SOState&, const Davidson& E)
{
    std::vector<double> D(E.nvec);
    AFESP_HIP(hipMemcpyAsync(D.data(), E.diag, sizeof(double) * E.nvec, hipMemcpyDeviceToHost, cx.stream));
    cx.sync();
    return D;
}

void preload_eom_both_sides() { preload_eom_so(); preload_eom_left_so(); }
void preload_eom_ipea_both_sides() { preload_eom_ipea_so(); preload_eom_ipea_left_so(); }

EomProblem eom_problem(const SOState& s, EomKind kind)
{
    const int64_t O = s.o, V = s.v;
    EomProblem P;
    if (kind == EOM_KIND_EE || kind == EOM_KIND_EE_LEFT) {
        const bool left = kind == EOM_KIND_EE_LEFT;
        P.prefix = left ? "afesp_ccsd_so_eom_left_" : "afesp_ccsd_so_eom_";
        P.state = left ? "left EOM" : "EOM";
        P.space = "the unique singles and doubles";
        P.sigma_entry = left ? "afesp_ccsd_so_eom_lsigma" : "afesp_ccsd_so_eom_sigma";
        P.r_stage = "eom_r_stage"; P.s_stage = "eom_s_stage";
        P.n1 = O * V; P.n2 = O * O * V * V; P.nunique = O * V + (O * (O - 1) / 2) * (V * (V - 1) / 2);
        P.w2 = 0.25; P.follow = left;
        P.bytes = [=](int nroots, int max_space) { return (left ? so_eom_left_bytes : so_eom_bytes)(O, V, nroots, max_space); };
        P.preload = left ? preload_eom_both_sides : preload_eom_so;
        P.fill_diag = so_eom_fill_diag;
        P.sigma = left ? so_eom_lsigma : so_eom_sigma;   // (left: the projected matrix is then <b_p, sigma_L(b_q)>)
        P.sort_key = ee_sort_key; P.unique = ee_unique; P.unit = ee_unit;
    } else {
        const bool ip = kind == EOM_KIND_IP || kind == EOM_KIND_IP_LEFT, left = kind == EOM_KIND_IP_LEFT || kind == EOM_KIND_EA_LEFT;
        const int sector = ip ? EOM_SECTOR_IP : EOM_SECTOR_EA;
        P.prefix = left ? "afesp_ccsd_so_eom_ipea_left_" : "afesp_ccsd_so_eom_ipea_";
        P.state = left ? (ip ? "left EOM-IP" : "left EOM-EA") : (ip ? "EOM-IP" : "EOM-EA");
        P.space = ip ? "the unique amplitudes of the EOM-IP sector" : "the unique amplitudes of the EOM-EA sector";
        P.sigma_entry = left ? "afesp_ccsd_so_eom_ipea_lsigma" : "afesp_ccsd_so_eom_ipea_sigma";
        P.r_stage = left ? "ipeal_r_stage" : "ipea_r_stage"; P.s_stage = left ? "ipeal_s_stage" : "ipea_s_stage";
        P.n1 = ip ? O : V; P.n2 = ip ? O * O * V : O * V * V; P.nunique = ip ? O + (O * (O - 1) / 2) * V : V + O * (V * (V - 1) / 2);
        P.w2 = 0.5; P.follow = left;
        P.bytes = [=](int nroots, int max_space) { return (left ? so_eom_ipea_left_bytes : so_eom_ipea_bytes)(O, V, sector, nroots, max_space); };
        P.preload = left ? preload_eom_ipea_both_sides : preload_eom_ipea_so;
        P.fill_diag = [=](Context& cx, SOState& st, double* diag) { so_eom_ipea_fill_diag(cx, st, sector, diag); };
        // (left: -D is the diagonal of A^T too -- the same diagonal, unique amplitudes and unit vectors with the admixture)
        P.sigma = [=](Context& cx, SOState& st, const double* r, double* sigma) {
            (left ? so_eom_ipea_lsigma : so_eom_ipea_sigma)(cx, st, sector, r, sigma);
        };
        P.sort_key = diag_sort_key;
        P.unique = [=](const SOState& st, std::vector<int64_t>& idx) { so_eom_ipea_unique(st, sector, idx); };
        P.unit = [=](Context& cx, SOState& st, double* x, int64_t p) { so_eom_ipea_unit(cx, st, sector, x, p); };
    }
    return P;
}

void eom_free_one(Context& cx, SOState& s, EomKind kind)
{
    SOEom*& e = s.eom[kind];
    if (!e) return;
    davidson_free(cx, e->d);
    delete e;
    e = nullptr;
}

}  // namespace

void so_eom_free(Context& cx, SOState& s)
{
    for (int kind = 0; kind < EOM_KINDS; ++kind) eom_free_one(cx, s, (EomKind)kind);
}

SOEom& so_eom_need(SOState& s, EomKind kind, const char* who)
{
    so_lambda_need(s, who);
    SOEom* e = s.eom[kind];
    if (!e || e->d.epoch != s.amp_epoch) {
        const EomProblem P = eom_problem(s, kind);
        throw Error(LAMBDA_ERR_STALE, std::string(who) + ": no " + P.state + " state for the live Lambda state (call " + P.prefix + "init first)");
    }
    return *e;
}

void so_eom_init(Context& cx, SOState& s, EomKind kind, int nroots, int max_space)
{
    so_need_plain(cx, EOM_WHO, EOM_PLAIN);
    const EomProblem P = eom_problem(s, kind);
    const std::string who = P.prefix + "init";
    SOLambda& L = so_lambda_need(s, who.c_str());
    if (nroots < 1 || (int64_t)nroots > P.nunique)
        throw Error(1, who + ": nroots must be in 1 .. " + std::to_string(P.nunique) + " (" + P.space + ")");
    if ((int64_t)max_space < 2 * (int64_t)nroots || max_space > 4096)
        throw Error(1, who + ": max_space must be in 2 nroots .. 4096");
    eom_free_one(cx, s, kind);
    if (!cx.fits(P.bytes(nroots, max_space)))
        throw Error(1, who + ": the " + P.state + " state of this system (" + std::to_string(max_space) + " basis vectors) does not fit the free device memory");
    P.preload();
    s.eom[kind] = new SOEom();
    SOEom& E = *s.eom[kind];
    try {
        E.kind = kind;
        davidson_alloc(cx, E.d, P.n1, P.n1 + P.n2, P.w2, P.follow, nroots, max_space, [&](double* diag) { P.fill_diag(cx, s, diag); });
        E.d.epoch = L.epoch;
        cx.sync();
    } catch (...) {
        try { cx.quiesce(); eom_free_one(cx, s, kind); } catch (...) {}
        throw;
    }
}

void so_eom_sigma_host(Context& cx, SOState& s, EomKind kind, int nvec, const double* r1, const double* r2, double* s1, double* s2)
{
    so_need_plain(cx, EOM_WHO, EOM_PLAIN);
    const EomProblem P = eom_problem(s, kind);
    so_lambda_need(s, P.sigma_entry);
    if (nvec < 1 || !r1 || !r2 || !s1 || !s2) throw Error(1, std::string(P.sigma_entry) + ": nvec < 1 or a NULL vector");
    const int64_t n1 = P.n1, n2 = P.n2;
    double* r = cx.scratch(P.r_stage, n1 + n2);
    double* sg = cx.scratch(P.s_stage, n1 + n2);
    for (int k = 0; k < nvec; ++k) {
        AFESP_HIP(hipMemcpyAsync(r, r1 + n1 * k, sizeof(double) * n1, hipMemcpyHostToDevice, cx.stream));
        AFESP_HIP(hipMemcpyAsync(r + n1, r2 + n2 * k, sizeof(double) * n2, hipMemcpyHostToDevice, cx.stream));
        P.sigma(cx, s, r, sg);
        AFESP_HIP(hipMemcpyAsync(s1 + n1 * k, sg, sizeof(double) * n1, hipMemcpyDeviceToHost, cx.stream));
        AFESP_HIP(hipMemcpyAsync(s2 + n2 * k, sg + n1, sizeof(double) * n2, hipMemcpyDeviceToHost, cx.stream));
        cx.sync();
    }
}

void so_eom_guess(Context& cx, SOState& s, EomKind kind)
{
    so_need_plain(cx, EOM_WHO, EOM_PLAIN);
    const EomProblem P = eom_problem(s, kind);
    Davidson& E = so_eom_need(s, kind, (P.prefix + "guess").c_str()).d;
    const std::vector<double> key = P.sort_key(cx, s, E);
    // the unique amplitudes by ascending key, ties by flat index
    std::vector<int64_t> idx;
    idx.reserve(P.nunique);
    for (int64_t x = 0; x < P.n1; ++x) idx.push_back(x);
    P.unique(s, idx);
    const int nr = E.nroots;
    std::partial_sort(idx.begin(), idx.begin() + nr, idx.end(), [&](int64_t p, int64_t q) { return key[p] != key[q] ? key[p] < key[q] : p < q; });
    davidson_restart(E);
    for (int k = 0; k < nr; ++k) P.unit(cx, s, E.pend + E.nvec * k, idx[k]);
    E.npend = nr;
    cx.sync();
}

void so_eom_set_guess(Context& cx, SOState& s, EomKind kind, int k, const double* r1, const double* r2)
{
    so_need_plain(cx, EOM_WHO, EOM_PLAIN);
    const EomProblem P = eom_problem(s, kind);
    davidson_set_pending_from_host(cx, so_eom_need(s, kind, (P.prefix + "set_guess").c_str()).d, P.prefix, k, r1, r2);
}

int so_eom_iterate(Context& cx, SOState& s, EomKind kind, double tol)
{
    so_need_plain(cx, EOM_WHO, EOM_PLAIN);
    const EomProblem P = eom_problem(s, kind);
    Davidson& E = so_eom_need(s, kind, (P.prefix + "iterate").c_str()).d;
    return davidson_iterate(cx, E, P.prefix, tol, [&](const double* r, double* sigma) { P.sigma(cx, s, r, sigma); });
}

void so_eom_get_vector(Context& cx, SOState& s, EomKind kind, int k, double* r1, double* r2)
{
    so_need_plain(cx, EOM_WHO, EOM_PLAIN);
    const EomProblem P = eom_problem(s, kind);
    davidson_get_vector(cx, so_eom_need(s, kind, (P.prefix + "get_vector").c_str()).d, P.prefix, k, r1, r2);
}

}  // namespace afesp
