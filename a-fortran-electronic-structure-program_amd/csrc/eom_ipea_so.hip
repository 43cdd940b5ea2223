// eom_ipea_so.hip -- EOM-IP-CCSD and EOM-EA-CCSD on the spin-orbital CCSD state (eom_ipea_so.h): the sigma build of either
// sector, term by term in the letters of tests/np_eom_ipea.py (ip_sigma_explicit, ea_sigma_explicit) over the H-bar elements of the live
// Lambda state, the diagonal and the guesses, for the block Davidson iteration of davidson_so.h on a vector described by (n1, n2, weight
// 1/2).  Launches are plain call-by-call ones.
#include "device_util.h"
#include "eom_ipea_so.h"
#include "tall.h"

namespace afesp {
namespace {

constexpr double IPEA_SEED = 1e-3;   // weight of the guesses' admixture of every unique amplitude (ipea_unit_kernel)

__global__ void ipea_diag_kernel(double* diag, int sector, const double* e, const double* lev, int o, int v, int64_t nvec)
{
    GRID_STRIDE(x, nvec) diag[x] = ipea_diag(sector, e, lev, o, v, x);
}

// sigma of a sector from the carriers of its sigma build, one thread per element of [sigma1; sigma2]:
//   IP   sigma2(i,j,a) = W + P(ij) A + diag r2      EA   sigma2(i,a,b) = W + P(ab) A + diag r2      sigma1 += diag r1
// W is antisymmetric in the pair as a sum of products only up to rounding.  With c = 1/2 W + A the value is c(pair) - c(pair exchanged):
// exchanging the pair negates it to the bit and it vanishes on the diagonal; diag is symmetric in the pair to the bit (ipea_diag).
__global__ void ipea_assemble_kernel(double* s, const double* W, const double* A, const double* r, int sector, const double* e, const double* lev,
                                     int o, int v)
{
    const bool ip = sector == EOM_SECTOR_IP;
    const int64_t n1 = ip ? o : v, n2 = ip ? (int64_t)o * o * v : (int64_t)o * v * v;
    GRID_STRIDE(x, n1 + n2)
    {
        const double d = ipea_diag(sector, e, lev, o, v, x);
        if (x < n1) {
            s[x] = __dadd_rn(s[x], __dmul_rn(d, r[x]));
            continue;
        }
        const int64_t y = x - n1;
        int64_t z;   // the image with the pair exchanged
        if (ip) {
            const int i = (int)(y % o), j = (int)((y / o) % o);
            z = j + (int64_t)o * (i + (y / ((int64_t)o * o)) * o);
        } else {
            const int i = (int)(y % o), a = (int)((y / o) % v), b = (int)(y / ((int64_t)o * v));
            z = i + (int64_t)o * (b + (int64_t)v * a);
        }
        const double cy = __dadd_rn(__dmul_rn(0.5, W[y]), A[y]), cz = __dadd_rn(__dmul_rn(0.5, W[z]), A[z]);
        s[x] = __dadd_rn(__dadd_rn(cy, -cz), __dmul_rn(d, r[x]));
    }
}

// ra(i, ef) = r(i,e,f) for e < f, leading dimension na; rows o .. oa and pairs npv .. ka are written as zero (the product reads them)
__global__ void ipea_ea_pack_kernel(double* ra, const double* r2, int o, int v, int64_t na, int64_t oa, int64_t ka)
{
    const int64_t npv = (int64_t)v * (v - 1) / 2;
    GRID_STRIDE(x, oa * ka)
    {
        const int64_t i = x % oa, p = x / oa;
        double val = 0.0;
        if (i < o && p < npv) {
            int e, f;
            unpair_lt(p, e, f);
            val = r2[i + (int64_t)o * (e + (int64_t)v * f)];
        }
        ra[i + na * p] = val;
    }
}
// W(i,a,b) = +- pa(i, ab): + for a < b, - for b < a, 0 on the diagonal
__global__ void ipea_ea_expand_kernel(double* W, const double* pa, int o, int v, int64_t na)
{
    GRID_STRIDE(x, (int64_t)o * v * v)
    {
        const int i = (int)(x % o), a = (int)((x / o) % v), b = (int)(x / ((int64_t)o * v));
        double val = 0.0;
        if (a != b) {
            const int al = min(a, b), ah = max(a, b);
            const double p = pa[i + na * ((int64_t)ah * (ah - 1) / 2 + al)];
            val = a < b ? p : -p;
        }
        W[x] = val;
    }
}

// A guess: +1 at ip, -1 at im (negative index: none), and on every unique amplitude the admixture IPEA_SEED (frac((q + 1) phi) - 1/2)
// with q the flat index of its i < j / a < b element and phi the golden ratio's fraction (the image carries the opposite sign, the
// diagonal zero).  sigma couples neither different Ms nor different irreducible representations and a unit vector lies in one block of
// each: without the admixture a wanted root in a block that holds none of the smallest diagonal elements -- the Ms = -+3/2 components of
// a 2h1p quartet, a hole in an orbital of another symmetry -- is never found, or only when rounding noise has grown into it.
__global__ void ipea_unit_kernel(double* x, int64_t nvec, int64_t ip, int64_t im, int sector, int o, int v)
{
    const int64_t n1 = sector == EOM_SECTOR_IP ? o : v;
    GRID_STRIDE(e, nvec)
    {
        int64_t q = e;
        double sign = 1.0;
        if (e >= n1) {
            const int64_t y = e - n1;
            int64_t z;
            if (sector == EOM_SECTOR_IP) z = (y / o) % o + (int64_t)o * (y % o + (y / ((int64_t)o * o)) * o);
            else z = y % o + (int64_t)o * (y / ((int64_t)o * v) + (int64_t)v * ((y / o) % v));
            sign = z == y ? 0.0 : (y < z ? 1.0 : -1.0);
            q = n1 + (y < z ? y : z);
        }
        const double t = __dmul_rn((double)(q + 1), 0.6180339887498949);
        const double seed = __dmul_rn(__dmul_rn(IPEA_SEED, sign), __dadd_rn(__dadd_rn(t, -floor(t)), -0.5));
        x[e] = __dadd_rn(e == ip ? 1.0 : (e == im ? -1.0 : 0.0), seed);
    }
}

}  // namespace

void preload_eom_ipea_so()
{
    static const bool loaded = [] {
        first_use_touch(reinterpret_cast<const void*>(ipea_diag_kernel));
        first_use_touch(reinterpret_cast<const void*>(ipea_assemble_kernel));
        first_use_touch(reinterpret_cast<const void*>(ipea_ea_pack_kernel));
        first_use_touch(reinterpret_cast<const void*>(ipea_ea_expand_kernel));
        first_use_touch(reinterpret_cast<const void*>(ipea_unit_kernel));
        (void)hipGetLastError();
        return true;
    }();
    (void)loaded;
}

// W(i,a,b) = sum_{e<f} <ab||ef> r(i,e,f) = 1/2 sum_ef: the bare ladder over the antisymmetric pair (e,f) against the pair-form va the T
// iteration built at init, in that iteration's own pair buffers ta / pa and with its offset table -- r is packed as ra(i, ef) on ta's
// leading dimension, a tall x skinny product M = K = v (v - 1) / 2, N = o.  That needs o <= o (o - 1) / 2, so that r fills rows of ta the T
// iteration fills too and its zero padding stays zero: o >= 3.  A state with o = 2, or without va (o = 1: the T iteration has no pair of
// occupied orbitals), contracts against <ab||ef> itself.
void so_eom_ea_ladder_bare(Context& cx, SOState& s, const Tensor& r2, const Tensor& W)
{
    preload_eom_ipea_so();
    const int o = s.o, v = s.v;
    const int64_t V = v, npv = V * (V - 1) / 2, ka = s.lad_ka, na = s.lad_na, oa = (o + 1) & ~1;
    if (npv == 0) {
        k_fill(cx, W.d, W.size(), 0.0);
        return;
    }
    if (!s.va || o > (int64_t)o * (o - 1) / 2) {
        contract(cx, 0.5, r2, "ief", s.vvvv, "abef", 0.0, W, "iab");
        return;
    }
    LAUNCH(ipea_ea_pack_kernel, grid_for(oa * ka), s.ta, r2.d, o, v, na, oa, ka);
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
    gp.M = (int)npv; gp.N = (int)oa; gp.K = (int)ka;
    const bool tall = tall_eligible(gp);   // the launcher's own choice, as contract() makes it
    ++(tall ? cx.n_tall : cx.n_gett);
    AFESP_HIP(tall ? tall_launch(gp, cx.stream) : gett_launch(gp, cx.ws, cx.stream));
    LAUNCH(ipea_ea_expand_kernel, grid_for(W.size()), W.d, s.pa, o, v, na);
}

double so_eom_ipea_bytes(int64_t o, int64_t v, int sector, int nroots, int max_space)
{
    const bool ip = sector == EOM_SECTOR_IP;
    const double O = (double)o, V = (double)v;
    const double n1 = ip ? O : V, n2 = ip ? O * O * V : O * V * V, nvec = n1 + n2;
    // the Davidson state; the scratch of a sigma build (W and the permutation carrier, y; EA: Z and the o^3 product) and the two staging
    // vectors of the host entry
    const double scratch = 2.0 * n2 + (ip ? V : O + O * V * O + O * O * O);
    return davidson_bytes(nvec, nroots, max_space) + 8.0 * (scratch + 2.0 * nvec);
}

void so_eom_ipea_sigma(Context& cx, SOState& s, int sector, const double* r, double* sigma)
{
    so_need_plain(cx, EOM_WHO, EOM_PLAIN);
    SOLambda& L = so_lambda_need(s, "afesp_ccsd_so_eom_ipea_sigma");
    preload_eom_ipea_so();
    const auto C = contractor(cx);
    const int o = s.o, v = s.v;
    const int64_t O = o, V = v;
    const Tensor &t1 = s.t1, &t2 = s.t2;
    double* rr = const_cast<double*>(r);
    if (sector == EOM_SECTOR_IP) {
        const int64_t n2 = O * O * V;
        const Tensor r1 = view(rr, {O}), r2 = view(rr + O, {O, O, V}), s1 = view(sigma, {O});
        // ---- sigma1: -H_mi r_m - H_me r_ime + 1/2 H_mnie r_mne  (- e_i r_i: the assemble kernel)
        C(-1.0, L.Hoo, "mi", r1, "m", 0.0, s1, "i");
        C(-1.0, r2, "ime", L.Hov, "me", 1.0, s1, "i");
        C(0.5, L.Hooov, "mnie", r2, "mne", 1.0, s1, "i");
        // ---- y_e = 1/2 <mn||ef> r_mnf
        Tensor y = view(cx.scratch("ipea_y", V), {V});
        C(0.5, s.oovv, "mnef", r2, "mnf", 0.0, y, "e");
        // ---- sigma2: W = 1/2 H_mnij r_mna + H_ae r_ije + H_maij r_m + y_e t_ijae;  P(ij) [ H_maej r_ime - H_mj r_ima ]
        Tensor W = view(cx.scratch("ipea_W", n2), {O, O, V}), A = view(cx.scratch("ipea_A", n2), {O, O, V});
        C(0.5, L.Hoooo, "mnij", r2, "mna", 0.0, W, "ija");
        C(1.0, r2, "ije", L.Hvv, "ae", 1.0, W, "ija");
        C(1.0, L.Hovoo, "maij", r1, "m", 1.0, W, "ija");
        C(1.0, t2, "ijae", y, "e", 1.0, W, "ija");
        C(1.0, r2, "ime", L.Hovvo, "maej", 0.0, A, "ija");
        C(-1.0, r2, "ima", L.Hoo, "mj", 1.0, A, "ija");
        LAUNCH(ipea_assemble_kernel, grid_for(O + n2), sigma, W.d, A.d, r, sector, s.e, s.lev, o, v);
    } else {
        const int64_t n2 = O * V * V;
        const Tensor r1 = view(rr, {V}), r2 = view(rr + V, {O, V, V}), s1 = view(sigma, {V});
        // ---- sigma1: H_ae r_e - H_me r_mae - 1/2 H_amef r_mef  (+ e_a r_a: the assemble kernel)
        C(1.0, L.Hvv, "ae", r1, "e", 0.0, s1, "a");
        C(-1.0, r2, "mae", L.Hov, "me", 1.0, s1, "a");
        C(-0.5, L.Hvovv, "amef", r2, "mef", 1.0, s1, "a");
        // ---- y_m = 1/2 <mn||ef> r_nef,  Z_iam = 1/2 r_ief <am||ef>,  Q_imn = r_ief <mn||ef>
        Tensor y = view(cx.scratch("ipea_y", O), {O}), Z = view(cx.scratch("ipea_Z", O * V * O), {O, V, O});
        Tensor Q = view(cx.scratch("ipea_Q", O * O * O), {O, O, O});
        C(0.5, s.oovv, "mnef", r2, "nef", 0.0, y, "m");
        C(0.5, r2, "ief", s.vovv, "amef", 0.0, Z, "iam");
        C(1.0, r2, "ief", s.oovv, "mnef", 0.0, Q, "imn");
        // ---- sigma2: W = bare ladder + 1/4 Q_imn tau_mnab + y_m t_imab - H_mi r_mab - H_abei r_e  (H_abei stored (i,e,a,b));
        //      P(ab) [ -t_mb Z_iam + H_mbei r_mae + H_be r_iae ]
        Tensor W = view(cx.scratch("ipea_W", n2), {O, V, V}), A = view(cx.scratch("ipea_A", n2), {O, V, V});
        so_eom_ea_ladder_bare(cx, s, r2, W);
        C(0.25, Q, "imn", L.tau, "mnab", 1.0, W, "iab");
        C(1.0, t2, "imab", y, "m", 1.0, W, "iab");
        C(-1.0, L.Hoo, "mi", r2, "mab", 1.0, W, "iab");
        C(-1.0, L.Hvvvo, "ieab", r1, "e", 1.0, W, "iab");
        C(-1.0, Z, "iam", t1, "mb", 0.0, A, "iab");
        C(1.0, r2, "mae", L.Hovvo, "mbei", 1.0, A, "iab");
        C(1.0, r2, "iae", L.Hvv, "be", 1.0, A, "iab");
        LAUNCH(ipea_assemble_kernel, grid_for(V + n2), sigma, W.d, A.d, r, sector, s.e, s.lev, o, v);
    }
}

void so_eom_ipea_fill_diag(Context& cx, SOState& s, int sector, double* diag)
{
    const int64_t O = s.o, V = s.v, nvec = sector == EOM_SECTOR_IP ? O + O * O * V : V + O * V * V;
    LAUNCH(ipea_diag_kernel, grid_for(nvec), diag, sector, s.e, s.lev, s.o, s.v, nvec);
}

void so_eom_ipea_unique(const SOState& s, int sector, std::vector<int64_t>& idx)
{
    const int64_t O = s.o, V = s.v;
    if (sector == EOM_SECTOR_IP) {
        for (int64_t a = 0; a < V; ++a)
            for (int64_t j = 0; j < O; ++j)
                for (int64_t i = 0; i < j; ++i) idx.push_back(O + i + O * (j + O * a));
    } else {
        for (int64_t b = 0; b < V; ++b)
            for (int64_t a = 0; a < b; ++a)
                for (int64_t i = 0; i < O; ++i) idx.push_back(V + i + O * (a + V * b));
    }
}

void so_eom_ipea_unit(Context& cx, SOState& s, int sector, double* x, int64_t p)
{
    const bool ip = sector == EOM_SECTOR_IP;
    const int64_t O = s.o, V = s.v, n1 = ip ? O : V, nvec = n1 + (ip ? O * O * V : O * V * V);
    int64_t im = -1;   // the image with the pair exchanged
    if (p >= n1) {
        const int64_t y = p - n1;
        if (ip) im = n1 + (y / O) % O + O * (y % O + O * (y / (O * O)));
        else im = n1 + y % O + O * (y / (O * V) + V * ((y / O) % V));
    }
    LAUNCH(ipea_unit_kernel, grid_for(nvec), x, nvec, p, im, sector, s.o, s.v);
}

}  // namespace afesp
