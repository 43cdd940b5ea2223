// eom_ipea_left_so.hip -- the left-hand side of EOM-IP-CCSD and EOM-EA-CCSD on the spin-orbital CCSD state (eom_ipea_so.h):
// the left sigma build sigma_L(l) = A^T l of either sector, transposed in the sector's metric <x, y> = sum x1 y1 + 1/2 sum x2 y2, and the
// Dyson orbitals of left and right vectors.  Term by term in the letters of tests/np_eom_ipea_left.py (ip_lsigma_explicit,
// ea_lsigma_explicit, dyson_explicit) over the H-bar elements of the live Lambda state, which are borrowed and never written.  The left
// Davidson states are two more kinds of eom_so.hip's driver.  Launches are plain call-by-call ones; every sum has a fixed order.
#include "device_util.h"
#include "eom_ipea_so.h"

namespace afesp {
namespace {

// sigma_L of a sector from the carriers of its build, one thread per element of [sigma_L1; sigma_L2]:
//   IP   sigma_L2(m,n,e) = W + P(mn) [A - l_m H_ne] + diag l2      EA   sigma_L2(i,a,e) = W + P(ae) [A - l_a H_ie] + diag l2
//   sigma_L1 += diag l1
// W is antisymmetric in the pair as a sum of products only up to rounding.  With c = 1/2 W + A - l1 H_ov the value is c(pair) - c(pair
// exchanged): exchanging the pair negates it to the bit and it vanishes on the diagonal; diag (ipea_diag: -D is the diagonal of A^T too) is
// symmetric in the pair to the bit.
__device__ __forceinline__ double ipea_lcarrier(const double* W, const double* A, const double* l1, const double* Hov, int64_t y, int one, int ov_o,
                                                int ov_v, int o)
{
    // (two explicit fused operations: the carrier of an element has the same bits whichever thread forms it, and as whichever operand)
    return fma(-l1[one], Hov[ov_o + (int64_t)o * ov_v], fma(0.5, W[y], A[y]));
}
__global__ void ipea_lassemble_kernel(double* s, const double* W, const double* A, const double* l, const double* Hov, int sector, const double* e,
                                      const double* lev, int o, int v)
{
    const bool ip = sector == EOM_SECTOR_IP;
    const int64_t n1 = ip ? o : v, n2 = ip ? (int64_t)o * o * v : (int64_t)o * v * v;
    GRID_STRIDE(x, n1 + n2)
    {
        const double d = ipea_diag(sector, e, lev, o, v, x);
        if (x < n1) {
            s[x] = __dadd_rn(s[x], __dmul_rn(d, l[x]));
            continue;
        }
        const int64_t y = x - n1;
        double cy, cz;   // the carrier and its image with the pair exchanged
        if (ip) {
            const int m = (int)(y % o), n = (int)((y / o) % o), c = (int)(y / ((int64_t)o * o));
            const int64_t z = n + (int64_t)o * (m + (int64_t)c * o);
            cy = ipea_lcarrier(W, A, l, Hov, y, m, n, c, o);
            cz = ipea_lcarrier(W, A, l, Hov, z, n, m, c, o);
        } else {
            const int i = (int)(y % o), a = (int)((y / o) % v), c = (int)(y / ((int64_t)o * v));
            const int64_t z = i + (int64_t)o * (c + (int64_t)v * a);
            cy = ipea_lcarrier(W, A, l, Hov, y, a, i, c, o);
            cz = ipea_lcarrier(W, A, l, Hov, z, c, i, a, o);
        }
        s[x] = __dadd_rn(__dadd_rn(cy, -cz), __dmul_rn(d, l[x]));
    }
}

// One Dyson vector element per block: out(p, k), p over the o + v spin orbitals, k over the vectors x(:, k) = [x1; x2] of length nlen.
// P(:, k) is the product of x2 with the four-index array (t2 for the left vectors, lambda2 for the right ones), G the o x o / v x v product of
// t2 and lambda2 the right vectors meet; the sums over one and two indices are made here, strided over the block and summed in a fixed order.
//   IP left    p = i: l_i                                  p = o + a: P_a + sum_i l_i t_ia                    (P_a = -1/2 l_mnf t_mnaf)
//   IP right   p = o + a: u_a = P_a + sum_i lam_ia r_i      (P_a = -1/2 lam_mnaf r_mnf)
//              p = m: r_m + sum_ia lam_ia (r_ima - t_ma r_i) - sum_a t_ma P_a - sum_j G_mj r_j                 (G_mj = 1/2 t_mnef lam_jnef)
//   EA left    p = o + a: l_a                              p = m: P_m - sum_a l_a t_ma                        (P_m = 1/2 l_nef t_mnef)
//   EA right   p = i: u_i = P_i - sum_a lam_ia r_a          (P_i = 1/2 lam_inef r_nef)
//              p = o + e: r_e + sum_ia lam_ia (r_iae - t_ie r_a) + sum_j P_j t_je - sum_b r_b G_be             (G_be = 1/2 t_mnef lam_mnbf)
__global__ void ipea_dyson_kernel(double* out, const double* x, const double* P, const double* G, const double* t1, const double* lam1,
                                  int right, int sector, int o, int v, int64_t nlen)
{
    __shared__ double sm[4];
    const int N = o + v, p = (int)(blockIdx.x % N);
    const int64_t k = blockIdx.x / N;
    const bool ip = sector == EOM_SECTOR_IP;
    const int np = ip ? v : o;                        // the length of P(:, k)
    const double *x1 = x + nlen * k, *x2 = x1 + (ip ? o : v), *Pk = P + (int64_t)np * k;
    const int64_t ov = (int64_t)o * v;
    double base = 0.0, acc[1] = {0.0};
    if (ip) {
        if (!right) {
            if (p < o) base = x1[p];
            else {
                const int a = p - o;
                base = Pk[a];
                for (int i = threadIdx.x; i < o; i += blockDim.x) acc[0] += x1[i] * t1[i + (int64_t)o * a];
            }
        } else if (p >= o) {
            const int a = p - o;
            base = Pk[a];
            for (int i = threadIdx.x; i < o; i += blockDim.x) acc[0] += lam1[i + (int64_t)o * a] * x1[i];
        } else {
            const int m = p;
            base = x1[m];
            for (int64_t q = threadIdx.x; q < ov + v + o; q += blockDim.x) {
                if (q < ov) {
                    const int i = (int)(q % o), a = (int)(q / o);
                    acc[0] += lam1[q] * (x2[i + (int64_t)o * (m + (int64_t)o * a)] - t1[m + (int64_t)o * a] * x1[i]);
                } else if (q < ov + v) {
                    const int a = (int)(q - ov);
                    acc[0] -= t1[m + (int64_t)o * a] * Pk[a];
                } else {
                    const int j = (int)(q - ov - v);
                    acc[0] -= G[m + (int64_t)o * j] * x1[j];
                }
            }
        }
    } else {
        if (!right) {
            if (p >= o) base = x1[p - o];
            else {
                base = Pk[p];
                for (int a = threadIdx.x; a < v; a += blockDim.x) acc[0] -= x1[a] * t1[p + (int64_t)o * a];
            }
        } else if (p < o) {
            base = Pk[p];
            for (int a = threadIdx.x; a < v; a += blockDim.x) acc[0] -= lam1[p + (int64_t)o * a] * x1[a];
        } else {
            const int e = p - o;
            base = x1[e];
            for (int64_t q = threadIdx.x; q < ov + o + v; q += blockDim.x) {
                if (q < ov) {
                    const int i = (int)(q % o), a = (int)(q / o);
                    acc[0] += lam1[q] * (x2[i + (int64_t)o * (a + (int64_t)v * e)] - t1[i + (int64_t)o * e] * x1[a]);
                } else if (q < ov + o) {
                    const int j = (int)(q - ov);
                    acc[0] += Pk[j] * t1[j + (int64_t)o * e];
                } else {
                    const int b = (int)(q - ov - o);
                    acc[0] -= x1[b] * G[b + (int64_t)v * e];
                }
            }
        }
    }
    block_sum<1>(acc, sm);
    if (threadIdx.x == 0) out[p + (int64_t)N * k] = base + acc[0];
}

}  // namespace

void preload_eom_ipea_left_so()
{
    static const bool loaded = [] {
        first_use_touch(reinterpret_cast<const void*>(ipea_lassemble_kernel));
        first_use_touch(reinterpret_cast<const void*>(ipea_dyson_kernel));
        (void)hipGetLastError();
        return true;
    }();
    (void)loaded;
}

double so_eom_ipea_left_bytes(int64_t o, int64_t v, int sector, int nroots, int max_space)
{
    const bool ip = sector == EOM_SECTOR_IP;
    const double O = (double)o, V = (double)v;
    const double n1 = ip ? O : V, n2 = ip ? O * O * V : O * V * V, nvec = n1 + n2;
    // the Davidson state; the scratch of a left sigma build (W and the permutation carrier, G; EA: Xt and the o^3 product) and the two
    // staging vectors of the host entry
    const double scratch = 2.0 * n2 + (ip ? V : O + O * V * O + O * O * O);
    return davidson_bytes(nvec, nroots, max_space) + 8.0 * (scratch + 2.0 * nvec);
}

void so_eom_ipea_lsigma(Context& cx, SOState& s, int sector, const double* l, double* sigma)
{
    so_need_plain(cx, EOM_WHO, EOM_PLAIN);
    SOLambda& L = so_lambda_need(s, "afesp_ccsd_so_eom_ipea_lsigma");
    preload_eom_ipea_left_so();
    const auto C = contractor(cx);
    const int o = s.o, v = s.v;
    const int64_t O = o, V = v;
    const Tensor &t1 = s.t1, &t2 = s.t2;
    double* ll = const_cast<double*>(l);
    if (sector == EOM_SECTOR_IP) {
        const int64_t n2 = O * O * V;
        const Tensor l1 = view(ll, {O}), l2 = view(ll + O, {O, O, V}), s1 = view(sigma, {O});
        // ---- sigma_L1: -H_mi l_i + 1/2 H_maij l_ija  (- e_m l_m: the assemble kernel)
        C(-1.0, L.Hoo, "mi", l1, "i", 0.0, s1, "m");
        C(0.5, L.Hovoo, "maij", l2, "ija", 1.0, s1, "m");
        // ---- G_e = 1/2 l_ija t_ijae
        Tensor G = view(cx.scratch("ipeal_G", V), {V});
        C(0.5, t2, "ijae", l2, "ija", 0.0, G, "e");
        // ---- sigma_L2: W = 1/2 H_mnij l_ije + l_mna H_ae + H_mnie l_i + G_a <mn||ae>;  P(mn) [ l_mja H_naej - l_mje H_nj - l_m H_ne ]
        //      (the disconnected l_m H_ne joins in the assemble kernel)
        Tensor W = view(cx.scratch("ipeal_W", n2), {O, O, V}), A = view(cx.scratch("ipeal_A", n2), {O, O, V});
        C(0.5, L.Hoooo, "mnij", l2, "ije", 0.0, W, "mne");
        C(1.0, l2, "mna", L.Hvv, "ae", 1.0, W, "mne");
        C(1.0, L.Hooov, "mnie", l1, "i", 1.0, W, "mne");
        C(1.0, s.oovv, "mnae", G, "a", 1.0, W, "mne");
        C(1.0, l2, "mja", L.Hovvo, "naej", 0.0, A, "mne");
        C(-1.0, l2, "mje", L.Hoo, "nj", 1.0, A, "mne");
        LAUNCH(ipea_lassemble_kernel, grid_for(O + n2), sigma, W.d, A.d, l, L.Hov.d, sector, s.e, s.lev, o, v);
    } else {
        const int64_t n2 = O * V * V;
        const Tensor l1 = view(ll, {V}), l2 = view(ll + V, {O, V, V}), s1 = view(sigma, {V});
        // ---- sigma_L1: H_ae l_a - 1/2 H_abei l_iab  (+ e_e l_e: the assemble kernel; H_abei stored (i,e,a,b))
        C(1.0, L.Hvv, "ae", l1, "a", 0.0, s1, "e");
        C(-0.5, L.Hvvvo, "ieab", l2, "iab", 1.0, s1, "e");
        // ---- G_m = 1/2 l_iab t_imab,  Xt_iam = l_iab t_mb,  Q_imn = l_iab tau_mnab
        Tensor G = view(cx.scratch("ipeal_G", O), {O}), Xt = view(cx.scratch("ipeal_Xt", O * V * O), {O, V, O});
        Tensor Q = view(cx.scratch("ipeal_Q", O * O * O), {O, O, O});
        C(0.5, t2, "imab", l2, "iab", 0.0, G, "m");
        C(1.0, l2, "iab", t1, "mb", 0.0, Xt, "iam");
        C(1.0, l2, "iab", L.tau, "mnab", 0.0, Q, "imn");
        // ---- sigma_L2: W = bare ladder + 1/4 Q_imn <mn||ef> + G_m <mi||ef> - H_im l_mef - H_aief l_a - Xt_iam <am||ef>;
        //      P(ae) [ l_mab H_ibem + l_iab H_be - l_a H_ie ]  (the disconnected l_a H_ie joins in the assemble kernel)
        Tensor W = view(cx.scratch("ipeal_W", n2), {O, V, V}), A = view(cx.scratch("ipeal_A", n2), {O, V, V});
        so_eom_ea_ladder_bare(cx, s, l2, W);
        C(0.25, Q, "imn", s.oovv, "mnef", 1.0, W, "ief");
        C(1.0, s.oovv, "mief", G, "m", 1.0, W, "ief");
        C(-1.0, L.Hoo, "im", l2, "mef", 1.0, W, "ief");
        C(-1.0, L.Hvovv, "aief", l1, "a", 1.0, W, "ief");
        C(-1.0, Xt, "iam", s.vovv, "amef", 1.0, W, "ief");
        C(1.0, l2, "mab", L.Hovvo, "ibem", 0.0, A, "iae");
        C(1.0, l2, "iab", L.Hvv, "be", 1.0, A, "iae");
        LAUNCH(ipea_lassemble_kernel, grid_for(V + n2), sigma, W.d, A.d, l, L.Hov.d, sector, s.e, s.lev, o, v);
    }
}

void so_eom_ipea_dyson(Context& cx, SOState& s, int sector, int nvec, const double* l1h, const double* l2h, const double* r1h, const double* r2h,
                       double* dl, double* dr)
{
    const char* who = "afesp_ccsd_so_eom_ipea_dyson";
    so_need_plain(cx, EOM_WHO, EOM_PLAIN);
    SOLambda& L = so_lambda_need(s, who);
    if (nvec < 1) throw Error(1, std::string(who) + ": nvec < 1");
    if ((l1h == nullptr) != (l2h == nullptr) || (r1h == nullptr) != (r2h == nullptr))
        throw Error(1, std::string(who) + ": l1 / l2 are both NULL or both given, and so are r1 / r2");
    const bool hasl = l1h != nullptr, hasr = r1h != nullptr;
    if ((hasl && !dl) || (hasr && !dr)) throw Error(1, std::string(who) + ": vectors are given and the Dyson vectors of their side are NULL");
    if (!hasl && !hasr) return;
    preload_eom_ipea_left_so();
    const auto C = contractor(cx);
    const bool ip = sector == EOM_SECTOR_IP;
    const int o = s.o, v = s.v;
    const int64_t O = o, V = v, N = O + V, n1 = ip ? O : V, n2 = ip ? O * O * V : O * V * V, nlen = n1 + n2, np = ip ? V : O;
    const Tensor &t2 = s.t2;
    double* x = cx.scratch("ipeal_x_stage", nlen * nvec);
    double* P = cx.scratch("ipeal_P", np * nvec);
    double* out = cx.scratch("ipeal_dyson", N * nvec);
    auto doubles = [&](int k) { return ip ? view(x + nlen * k + n1, {O, O, V}) : view(x + nlen * k + n1, {O, V, V}); };
    auto stage = [&](const double* x1h, const double* x2h) {
        for (int k = 0; k < nvec; ++k) {
            AFESP_HIP(hipMemcpyAsync(x + nlen * k, x1h + n1 * k, sizeof(double) * n1, hipMemcpyHostToDevice, cx.stream));
            AFESP_HIP(hipMemcpyAsync(x + nlen * k + n1, x2h + n2 * k, sizeof(double) * n2, hipMemcpyHostToDevice, cx.stream));
        }
    };
    auto finish = [&](int right, const double* G, double* d_host) {
        LAUNCH(ipea_dyson_kernel, dim3((unsigned)(N * nvec)), out, x, P, G, s.t1.d, L.l1.d, right, sector, o, v, nlen);
        AFESP_HIP(hipMemcpyAsync(d_host, out, sizeof(double) * N * nvec, hipMemcpyDeviceToHost, cx.stream));
        cx.sync();   // (the staging buffers serve the other side next)
    };
    if (hasl) {
        stage(l1h, l2h);
        for (int k = 0; k < nvec; ++k) {
            const Tensor x2 = doubles(k), Pk = view(P + np * k, {np});
            if (ip) C(-0.5, t2, "mnaf", x2, "mnf", 0.0, Pk, "a");
            else C(0.5, t2, "mnef", x2, "nef", 0.0, Pk, "m");
        }
        finish(0, nullptr, dl);
    }
    if (hasr) {
        stage(r1h, r2h);
        // G of t2 and lambda2, in a buffer of this unit (the Lambda state's own G are its iteration's)
        Tensor G = ip ? view(cx.scratch("ipeal_Goo", O * O), {O, O}) : view(cx.scratch("ipeal_Gvv", V * V), {V, V});
        if (ip) C(0.5, t2, "mnef", L.l2, "jnef", 0.0, G, "mj");
        else C(0.5, t2, "mnef", L.l2, "mnbf", 0.0, G, "be");
        for (int k = 0; k < nvec; ++k) {
            const Tensor x2 = doubles(k), Pk = view(P + np * k, {np});
            if (ip) C(-0.5, L.l2, "mnaf", x2, "mnf", 0.0, Pk, "a");
            else C(0.5, L.l2, "inef", x2, "nef", 0.0, Pk, "i");
        }
        finish(1, G.d, dr);
    }
}

}  // namespace afesp
