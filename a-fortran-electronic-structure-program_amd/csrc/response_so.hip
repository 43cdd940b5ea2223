// response_so.hip -- EOM-CCSD linear response on the spin-orbital CCSD state (response_so.h): the operator vectors xi^X in
// the letters of tests/np_response.py (xi_explicit), the response state on the linear mode of davidson_so.h with so_eom_sigma as its
// matrix, and the response function from the resident solutions through so_eom_density.  Launches are plain call-by-call ones; every sum
// is in a fixed order.
#include "response_so.h"

#include "device_util.h"

#include <cmath>

namespace afesp {
namespace {

constexpr int RSP_CT = 32;      // virtual indices of one staged piece of a row of X~_vv
constexpr int RSP_KT = 8;       // rows k of X~_oo staged at a time, fewer where o rows of RSP_KT exceed ...
constexpr int RSP_OO = 2048;    // ... the doubles of the staging buffer: kt = min(o, RSP_KT, RSP_OO / o)
constexpr int RSP_PAB = TB / 64;   // virtual pairs of a block: one per wave, 64 occupied pairs each
constexpr const char *RSP_WHO = "so_response", *RSP_PLAIN = "the response equations are";   // (so_need_plain)

// The dressed operators and xi1 of every operator of the batch (blockIdx.y), one element per thread and every sum in a fixed order:
//   X~_kj = X_kj + sum_c X_kc t_jc                  -> Xoo[k + o j]
//   X~_bc = X_bc - sum_k t_kb X_kc                  -> XvvT[c + v b]  (transposed: the assemble kernel reads rows b)
//   xi_ia = X_ai + sum_b X_ab t_ib - sum_j t_ja X_ji + sum_jb X_jb (t_ijab - t_ib t_ja)
__global__ void response_dress_kernel(double* Xoo, double* XvvT, double* xi, const double* X, const double* t1, const double* t2, int o, int v,
                                      int64_t nvec)
{
    const int N = o + v, op = blockIdx.y;
    const int64_t oo = (int64_t)o * o, vv = (int64_t)v * v, ov = (int64_t)o * v;
    const double* Xp = X + (int64_t)op * N * N;
    double *xoo = Xoo + op * oo, *xvv = XvvT + op * vv, *x1 = xi + op * nvec;
    GRID_STRIDE(e, oo + vv + ov)
    {
        if (e < oo) {
            const int k = (int)(e % o), j = (int)(e / o);
            double s = Xp[k + (int64_t)N * j];
            for (int c = 0; c < v; ++c) s = __fma_rn(Xp[k + (int64_t)N * (o + c)], t1[j + o * c], s);
            xoo[e] = s;
        } else if (e < oo + vv) {
            const int64_t x = e - oo;
            const int c = (int)(x % v), b = (int)(x / v);
            double s = Xp[(o + b) + (int64_t)N * (o + c)];
            for (int k = 0; k < o; ++k) s = __fma_rn(-t1[k + o * b], Xp[k + (int64_t)N * (o + c)], s);
            xvv[x] = s;
        } else {
            const int64_t x = e - oo - vv;
            const int i = (int)(x % o), a = (int)(x / o);
            double s = Xp[(o + a) + (int64_t)N * i];
            for (int b = 0; b < v; ++b) s = __fma_rn(Xp[(o + a) + (int64_t)N * (o + b)], t1[i + o * b], s);
            for (int j = 0; j < o; ++j) s = __fma_rn(-t1[j + o * a], Xp[j + (int64_t)N * i], s);
            for (int b = 0; b < v; ++b)
                for (int j = 0; j < o; ++j)
                    s = __fma_rn(Xp[j + (int64_t)N * (o + b)], __fma_rn(-t1[i + o * b], t1[j + o * a], t2[i + o * (j + o * (a + (int64_t)v * b))]), s);
            x1[x] = s;
        }
    }
}

// xi2 of every operator of the batch (blockIdx.y).  A thread owns one unique (i < j, a < b): lane = occupied pair (i fastest, so that a
// wave reads t2 along its fastest index), wave = virtual pair.  It forms
//   xi_ijab = sum_c [X~_bc t_ijac - X~_ac t_ijbc] - sum_k [X~_kj t_ikab - X~_ki t_jkab]
// once -- c ascending, then k ascending -- and writes the four images with the sign flipped: antisymmetric to the bit; the diagonals are
// the zeros the buffer was filled with.  Rows a and b of X~_vv are staged per wave in pieces of RSP_CT, kt rows k of X~_oo per block.
__global__ void response_xi2_kernel(double* xi, const double* Xoo, const double* XvvT, const double* t2, int o, int v, int kt, int nbij,
                                    int64_t nvec)
{
    __shared__ double sv[RSP_PAB][2][RSP_CT];
    __shared__ double soo[RSP_OO];
    const int op = blockIdx.y, lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int64_t oo = (int64_t)o * o, npo = (int64_t)o * (o - 1) / 2, npv = (int64_t)v * (v - 1) / 2;
    const int64_t pij = (int64_t)(blockIdx.x % nbij) * 64 + lane, pab = (int64_t)(blockIdx.x / nbij) * RSP_PAB + wv;
    const bool wave_ok = pab < npv, ok = wave_ok && pij < npo;
    int i = 0, j = 1, a = 0, b = 1, h;
    if (pij < npo) { unpair(pij, i, h); j = h + 1; }
    if (wave_ok) { unpair(pab, a, h); b = h + 1; }
    const double *xoo = Xoo + op * oo, *xvv = XvvT + (int64_t)op * v * v;
    const int64_t ij = i + (int64_t)o * j, ab = a + (int64_t)v * b;
    double acc = 0.0;
    for (int c0 = 0; c0 < v; c0 += RSP_CT) {
        const int cn = min(RSP_CT, v - c0);
        __syncthreads();
        if (wave_ok)
            for (int c = lane; c < cn; c += 64) {
                sv[wv][0][c] = xvv[(c0 + c) + (int64_t)v * a];
                sv[wv][1][c] = xvv[(c0 + c) + (int64_t)v * b];
            }
        __syncthreads();
        if (ok)
            for (int c = 0; c < cn; ++c) {
                acc = __fma_rn(sv[wv][1][c], t2[ij + oo * (a + (int64_t)v * (c0 + c))], acc);
                acc = __fma_rn(-sv[wv][0][c], t2[ij + oo * (b + (int64_t)v * (c0 + c))], acc);
            }
    }
    for (int k0 = 0; k0 < o; k0 += kt) {
        const int kn = min(kt, o - k0);
        __syncthreads();
        for (int e = threadIdx.x; e < kn * o; e += TB) {
            const int kk = e % kn, jj = e / kn;
            soo[kk + kt * jj] = xoo[(k0 + kk) + (int64_t)o * jj];
        }
        __syncthreads();
        if (ok)
            for (int kk = 0; kk < kn; ++kk) {
                acc = __fma_rn(-soo[kk + kt * j], t2[i + (int64_t)o * (k0 + kk) + oo * ab], acc);
                acc = __fma_rn(soo[kk + kt * i], t2[j + (int64_t)o * (k0 + kk) + oo * ab], acc);
            }
    }
    if (ok) {
        double* x2 = xi + op * nvec + (int64_t)o * v;
        const int64_t ba = b + (int64_t)v * a;
        x2[i + (int64_t)o * j + oo * ab] = acc;
        x2[j + (int64_t)o * i + oo * ba] = acc;
        x2[j + (int64_t)o * i + oo * ab] = -acc;
        x2[i + (int64_t)o * j + oo * ba] = -acc;
    }
}

void check_count(const char* who, int nop, const double* x)
{
    if (nop < 1 || nop > RESPONSE_MAX_SYSTEMS || !x)
        throw Error(1, std::string(who) + ": nop must be in 1 .. " + std::to_string(RESPONSE_MAX_SYSTEMS) + ", and the operators given");
}

void check_operators(const char* who, int nop, const double* x, int64_t N)
{
    check_count(who, nop, x);
    for (int a = 0; a < nop; ++a) {
        const double* m = x + (int64_t)a * N * N;
        double big = 1.0;
        for (int64_t e = 0; e < N * N; ++e) {
            if (!std::isfinite(m[e])) throw Error(1, std::string(who) + ": operator " + std::to_string(a) + " has a non-finite element");
            big = std::max(big, std::fabs(m[e]));
        }
        for (int64_t q = 0; q < N; ++q)
            for (int64_t p = 0; p < q; ++p)
                if (std::fabs(m[p + N * q] - m[q + N * p]) > 1e-12 * big)
                    throw Error(1, std::string(who) + ": operator " + std::to_string(a) + " is not symmetric (elements " + std::to_string(p) + "," +
                                       std::to_string(q) + ")");
    }
}

int64_t vec_len(const SOState& s) { return (int64_t)s.o * s.v + (int64_t)s.o * s.o * s.v * s.v; }

}  // namespace

void preload_response_so()
{
    static const bool loaded = [] {
        first_use_touch(reinterpret_cast<const void*>(response_dress_kernel));
        first_use_touch(reinterpret_cast<const void*>(response_xi2_kernel));
        (void)hipGetLastError();
        return true;
    }();
    (void)loaded;
}

double so_response_bytes(int64_t o, int64_t v, int nop, int nsys, int max_space, bool cplx)
{
    const double O = (double)o, V = (double)v, nvec = O * V + O * O * V * V;
    // the Davidson state and the scratch of a sigma build and of a density call as the left EOM state counts them; the xi vectors, the
    // operators and their dressed blocks; complex frequencies: what the second column of every system adds to the Davidson state
    return so_eom_left_bytes(o, v, nsys, max_space) + 8.0 * nop * (nvec + (O + V) * (O + V) + O * O + V * V) +
           (cplx ? davidson_bytes_complex(nvec, nsys, max_space) - davidson_bytes(nvec, nsys, max_space) : 0.0);
}

// so_response_xi behind its argument check
static void xi_build(Context& cx, SOState& s, int nop, const double* x_host, double* xi)
{
    preload_response_so();
    const int o = s.o, v = s.v;
    const int64_t O = o, V = v, N = O + V, nvec = vec_len(s);
    if (O > RSP_OO) throw Error(1, "afesp_ccsd_so_response_xi: more occupied spin orbitals than the assemble kernel stages");
    double* X = cx.scratch("rsp_X", nop * N * N);
    double* Xoo = cx.scratch("rsp_Xoo", nop * O * O);
    double* XvvT = cx.scratch("rsp_XvvT", nop * V * V);
    AFESP_HIP(hipMemcpyAsync(X, x_host, sizeof(double) * nop * N * N, hipMemcpyHostToDevice, cx.stream));
    k_fill(cx, xi, nvec * nop, 0.0);
    LAUNCH(response_dress_kernel, dim3(grid_for(O * O + V * V + O * V), nop), Xoo, XvvT, xi, X, s.t1.d, s.t2.d, o, v, nvec);
    const int64_t npo = O * (O - 1) / 2, npv = V * (V - 1) / 2;
    if (npo > 0 && npv > 0) {
        const int64_t nbij = (npo + 63) / 64, nbab = (npv + RSP_PAB - 1) / RSP_PAB;
        if (nbij * nbab > 0x7fffffff) throw Error(1, "afesp_ccsd_so_response_xi: the pair space exceeds one launch");
        const int kt = (int)std::min<int64_t>(std::min<int64_t>(O, RSP_KT), RSP_OO / O);
        LAUNCH(response_xi2_kernel, dim3((unsigned)(nbij * nbab), nop), xi, Xoo, XvvT, s.t2.d, o, v, kt, (int)nbij, nvec);
    }
    cx.sync();   // (x_host is the caller's)
}

void so_response_xi(Context& cx, SOState& s, int nop, const double* x_host, double* xi)
{
    so_need_plain(cx, RSP_WHO, RSP_PLAIN);
    check_operators("afesp_ccsd_so_response_xi", nop, x_host, (int64_t)s.o + s.v);
    xi_build(cx, s, nop, x_host, xi);
}

void so_response_xi_host(Context& cx, SOState& s, int nop, const double* x, double* xi1, double* xi2)
{
    so_need_plain(cx, RSP_WHO, RSP_PLAIN);
    if (!xi1 || !xi2) throw Error(1, "afesp_ccsd_so_response_xi: a NULL vector");
    const int64_t O = s.o, V = s.v, ov = O * V, o2v2 = O * O * V * V, nvec = ov + o2v2;
    check_count("afesp_ccsd_so_response_xi", nop, x);   // (it sizes the staging buffer; the matrices themselves: so_response_xi)
    double* xi = cx.scratch("rsp_xi_stage", nvec * nop);
    so_response_xi(cx, s, nop, x, xi);
    for (int a = 0; a < nop; ++a) {
        AFESP_HIP(hipMemcpyAsync(xi1 + ov * a, xi + nvec * a, sizeof(double) * ov, hipMemcpyDeviceToHost, cx.stream));
        AFESP_HIP(hipMemcpyAsync(xi2 + o2v2 * a, xi + nvec * a + ov, sizeof(double) * o2v2, hipMemcpyDeviceToHost, cx.stream));
    }
    cx.sync();
}

void so_response_free(Context& cx, SOState& s)
{
    SOResponse* r = s.resp;
    if (!r) return;
    davidson_free(cx, r->d);
    cx.release(r->xi);
    delete r;
    s.resp = nullptr;
}

SOResponse& so_response_need(SOState& s, const char* who)
{
    SOLambda& L = so_lambda_need(s, who);
    SOResponse* r = s.resp;
    if (!r || r->d.epoch != s.amp_epoch)
        throw Error(LAMBDA_ERR_STALE, std::string(who) + ": no response state for the live Lambda state (call afesp_ccsd_so_response_init first)");
    if (r->lam_stamp != L.stamp)
        throw Error(LAMBDA_ERR_STALE, std::string(who) + ": the response state is stale: l1 / l2 may have changed since afesp_ccsd_so_response_init (call it again)");
    return *r;
}

// so_response_init (gamma null: real frequencies omega[f]) and so_response_init_complex (omega[f] + i gamma[f], both with stride `inc`)
static void response_init(Context& cx, SOState& s, const char* who, int nop, const double* x, int nfreq, const double* omega, const double* gamma,
                          int inc, int max_space)
{
    so_need_plain(cx, RSP_WHO, RSP_PLAIN);
    const bool cplx = gamma != nullptr;
    SOLambda& L = so_lambda_need(s, who);
    const int64_t O = s.o, V = s.v, N = O + V, nvec = vec_len(s);
    check_operators(who, nop, x, N);
    if (nfreq < 1 || !omega || (int64_t)nop * nfreq > RESPONSE_MAX_SYSTEMS)
        throw Error(1, std::string(who) + ": nfreq_signed must be at least 1 and nop nfreq_signed at most " + std::to_string(RESPONSE_MAX_SYSTEMS));
    for (int f = 0; f < nfreq; ++f)
        if (!std::isfinite(omega[inc * f]) || (cplx && !std::isfinite(gamma[inc * f]))) throw Error(1, std::string(who) + ": a frequency is not finite");
    const int nsys = nop * nfreq;
    if (max_space < (cplx ? 4 : 2) * nsys || max_space > 4096)
        throw Error(1, std::string(who) + ": max_space must be in " + (cplx ? "4" : "2") + " nop nfreq_signed .. 4096");
    so_response_free(cx, s);
    if (!cx.fits(so_response_bytes(O, V, nop, nsys, max_space, cplx)))
        throw Error(1, std::string(who) + ": the response state of this system (" + std::to_string(max_space) + " basis vectors) does not fit the free device memory");
    preload_eom_so();   // (the diagonal is the EE state's)
    preload_response_so();
    s.resp = new SOResponse();
    SOResponse& R = *s.resp;
    try {
        R.nop = nop;
        R.nfreq = nfreq;
        R.x.assign(x, x + (int64_t)nop * N * N);
        R.cplx = cplx;
        R.omega.resize(nfreq);
        R.gamma.assign(nfreq, 0.0);
        for (int f = 0; f < nfreq; ++f) {
            R.omega[f] = omega[inc * f];
            if (cplx) R.gamma[f] = gamma[inc * f];
        }
        R.phi.assign((size_t)nop * nsys, 0.0);
        R.phi_im.assign(cplx ? (size_t)nop * nsys : 0, 0.0);
        R.have_phi.assign(nsys, 0);
        R.xi = cx.alloc(nvec * nop);
        xi_build(cx, s, nop, x, R.xi);   // (checked above)
        davidson_alloc(cx, R.d, O * V, nvec, 0.25, false, nsys, max_space, [&](double* diag) { so_eom_fill_diag(cx, s, diag); }, cplx);
        std::vector<double> shifts(nsys), shifts_im(nsys);
        for (int j = 0; j < nsys; ++j) shifts[j] = R.omega[j / nop], shifts_im[j] = R.gamma[j / nop];
        if (cplx) davidson_linear_start_complex(cx, R.d, R.xi, nop, shifts.data(), shifts_im.data());
        else davidson_linear_start(cx, R.d, R.xi, nop, shifts.data());
        R.d.epoch = L.epoch;
        R.lam_stamp = L.stamp;
        cx.sync();
    } catch (...) {
        try { cx.quiesce(); so_response_free(cx, s); } catch (...) {}
        throw;
    }
}

void so_response_init(Context& cx, SOState& s, int nop, const double* x, int nfreq, const double* omega, int max_space)
{
    response_init(cx, s, "afesp_ccsd_so_response_init", nop, x, nfreq, omega, nullptr, 1, max_space);
}

void so_response_init_complex(Context& cx, SOState& s, int nop, const double* x, int nfreq, const double* z, int max_space)
{
    response_init(cx, s, "afesp_ccsd_so_response_init_complex", nop, x, nfreq, z, z ? z + 1 : nullptr, 2, max_space);
}

// status 1 where the state is not of the kind the entry point `who` works on
static void need_mode(const SOResponse& R, bool cplx, const char* who)
{
    if (R.cplx != cplx)
        throw Error(1, std::string(who) + ": the response state was made for " + (R.cplx ? "complex" : "real") + " frequencies (use the " +
                           (R.cplx ? "_complex entry points" : "entry points without _complex") + ", or initialise it again)");
}

int so_response_iterate(Context& cx, SOState& s, double tol)
{
    so_need_plain(cx, RSP_WHO, RSP_PLAIN);
    SOResponse& R = so_response_need(s, "afesp_ccsd_so_response_iterate");
    std::fill(R.have_phi.begin(), R.have_phi.end(), 0);   // (the solutions move with every step)
    const int conv = davidson_linear_iterate(cx, R.d, "afesp_ccsd_so_response_", tol, [&](const double* r, double* sigma) { so_eom_sigma(cx, s, r, sigma); });
    R.stepped = true;
    return conv;
}

void so_response_get_vector(Context& cx, SOState& s, int iop, int ifreq, double* r1, double* r2)
{
    so_need_plain(cx, RSP_WHO, RSP_PLAIN);
    SOResponse& R = so_response_need(s, "afesp_ccsd_so_response_get_vector");
    need_mode(R, false, "afesp_ccsd_so_response_get_vector");
    if (!R.stepped || iop < 0 || iop >= R.nop || ifreq < 0 || ifreq >= R.nfreq || !r1 || !r2)
        throw Error(1, "afesp_ccsd_so_response_get_vector: no solution (iop, ifreq) (iterate first; iop in 0 .. nop - 1, ifreq in 0 .. nfreq_signed - 1), or a NULL vector");
    const Davidson& E = R.d;
    const double* x = E.x + E.nvec * (iop + R.nop * ifreq);
    AFESP_HIP(hipMemcpyAsync(r1, x, sizeof(double) * E.n1, hipMemcpyDeviceToHost, cx.stream));
    AFESP_HIP(hipMemcpyAsync(r2, x + E.n1, sizeof(double) * (E.nvec - E.n1), hipMemcpyDeviceToHost, cx.stream));
    cx.sync();
}

void so_response_get_vector_complex(Context& cx, SOState& s, int iop, int ifreq, double* r1_re, double* r2_re, double* r1_im, double* r2_im)
{
    so_need_plain(cx, RSP_WHO, RSP_PLAIN);
    const char* who = "afesp_ccsd_so_response_get_vector_complex";
    SOResponse& R = so_response_need(s, who);
    need_mode(R, true, who);
    if (!R.stepped || iop < 0 || iop >= R.nop || ifreq < 0 || ifreq >= R.nfreq || !r1_re || !r2_re || !r1_im || !r2_im)
        throw Error(1, std::string(who) + ": no solution (iop, ifreq) (iterate first; iop in 0 .. nop - 1, ifreq in 0 .. nfreq_signed - 1), or a NULL vector");
    const Davidson& E = R.d;
    const double* p = E.x + E.nvec * 2 * (iop + R.nop * ifreq);
    const double* q = p + E.nvec;
    AFESP_HIP(hipMemcpyAsync(r1_re, p, sizeof(double) * E.n1, hipMemcpyDeviceToHost, cx.stream));
    AFESP_HIP(hipMemcpyAsync(r2_re, p + E.n1, sizeof(double) * (E.nvec - E.n1), hipMemcpyDeviceToHost, cx.stream));
    AFESP_HIP(hipMemcpyAsync(r1_im, q, sizeof(double) * E.n1, hipMemcpyDeviceToHost, cx.stream));
    AFESP_HIP(hipMemcpyAsync(r2_im, q + E.n1, sizeof(double) * (E.nvec - E.n1), hipMemcpyDeviceToHost, cx.stream));
    cx.sync();
}

namespace {

// Phi[X_a, r] of one device vector r for every operator of the state: one density call, the traces on the host in a fixed order.  The
// host copy of lambda, D and Tr(X_a D) are made at the first call and kept for the later ones of one response function.
struct PhiWork {
    std::vector<double> lam, r, D, gam, trD;

    void column(Context& cx, SOState& s, SOResponse& R, const double* xj, double* phi /* nop, stride 1 */)
    {
        SOLambda& L = *s.lam;
        const int nop = R.nop;
        const int64_t O = s.o, V = s.v, N = O + V, ov = O * V, o2v2 = O * O * V * V, nvec = ov + o2v2;
        if (lam.empty()) {
            lam.resize(nvec);
            r.resize(nvec);
            D.resize(N * N);
            gam.resize(N * N);
            trD.resize(nop);
            AFESP_HIP(hipMemcpyAsync(lam.data(), L.l1.d, sizeof(double) * ov, hipMemcpyDeviceToHost, cx.stream));
            AFESP_HIP(hipMemcpyAsync(lam.data() + ov, L.l2.d, sizeof(double) * o2v2, hipMemcpyDeviceToHost, cx.stream));
            cx.sync();
            so_density(cx, s, D.data(), N * N);
            for (int a = 0; a < nop; ++a) {
                double t = 0.0;
                for (int64_t e = 0; e < N * N; ++e) t += R.x[(int64_t)a * N * N + e] * D[e];
                trD[a] = t;
            }
        }
        double lr = 0.0;   // <lambda, x_j>
        AFESP_HIP(hipMemcpyAsync(&lr, so_eom_wdot(cx, L.l1.d, L.l2.d, xj, ov, o2v2), sizeof(double), hipMemcpyDeviceToHost, cx.stream));
        AFESP_HIP(hipMemcpyAsync(r.data(), xj, sizeof(double) * nvec, hipMemcpyDeviceToHost, cx.stream));
        cx.sync();
        so_eom_density(cx, s, 1.0, lam.data(), lam.data() + ov, 0.0, r.data(), r.data() + ov, gam.data(), N * N);
        for (int a = 0; a < nop; ++a) {
            double t = 0.0;
            for (int64_t e = 0; e < N * N; ++e) t += R.x[(int64_t)a * N * N + e] * gam[e];
            phi[a] = t - trD[a] * lr;
        }
    }
};

void need_converged(const SOResponse& R, const char* who, int g)
{
    for (int a = 0; a < R.nop; ++a)
        if (!R.stepped || !(R.d.flags[a + R.nop * g] & EOM_FLAG_CONVERGED))
            throw Error(RESPONSE_ERR_NOT_CONVERGED, std::string(who) + ": the solution of operator " + std::to_string(a) + " at frequency " +
                                                        std::to_string(R.omega[g]) + (R.cplx ? " + " + std::to_string(R.gamma[g]) + " i" : "") +
                                                        " has not converged (residual " +
                                                        std::to_string(R.stepped ? R.d.resnorm[a + R.nop * g] : HUGE_VAL) + ")");
}

}  // namespace

void so_response_function_complex(Context& cx, SOState& s, int nfreq, const double* z, double* out)
{
    so_need_plain(cx, RSP_WHO, RSP_PLAIN);
    const char* who = "afesp_ccsd_so_response_function_complex";
    SOResponse& R = so_response_need(s, who);
    need_mode(R, true, who);
    if (nfreq < 1 || !z || !out) throw Error(1, std::string(who) + ": nfreq < 1 or a NULL argument");
    const int nop = R.nop;
    const int64_t nvec = vec_len(s);
    // ---- which stored frequency serves z and -z of every request: -z itself, or the conjugate of the solution at -conj(z)
    std::vector<int> plus(nfreq, -1), minus(nfreq, -1);
    std::vector<char> conj(nfreq, 0);
    for (int f = 0; f < nfreq; ++f) {
        const double re = z[2 * f], im = z[2 * f + 1];
        int partner = -1;
        for (int g = R.nfreq - 1; g >= 0; --g) {
            if (R.omega[g] == re && R.gamma[g] == im) plus[f] = g;
            if (R.omega[g] == -re && R.gamma[g] == -im) minus[f] = g;
            if (R.omega[g] == -re && R.gamma[g] == im) partner = g;
        }
        if (minus[f] < 0 && partner >= 0) minus[f] = partner, conj[f] = 1;
        if (plus[f] < 0 || minus[f] < 0)
            throw Error(1, std::string(who) + ": the frequency " + std::to_string(re) + " + " + std::to_string(im) +
                               " i was not solved at z and at -z (or -conj z) by this response state");
    }
    for (int f = 0; f < nfreq; ++f)
        for (int g : {plus[f], minus[f]}) need_converged(R, who, g);
    // ---- Phi[X_a, P_j] and Phi[X_a, Q_j] of the systems that lack them: two density calls per solution
    PhiWork work;
    for (int f = 0; f < nfreq; ++f)
        for (int g : {plus[f], minus[f]})
            for (int b = 0; b < nop; ++b) {
                const int j = b + nop * g;
                if (R.have_phi[j]) continue;
                work.column(cx, s, R, R.d.x + nvec * 2 * j, R.phi.data() + (size_t)nop * j);
                work.column(cx, s, R, R.d.x + nvec * (2 * j + 1), R.phi_im.data() + (size_t)nop * j);
                R.have_phi[j] = 1;
            }
    for (int f = 0; f < nfreq; ++f)
        for (int a = 0; a < nop; ++a)
            for (int b = 0; b < nop; ++b) {
                const size_t jp = a + (size_t)nop * (b + nop * plus[f]), jm = b + (size_t)nop * (a + nop * minus[f]);
                double* o2 = out + 2 * (((size_t)f * nop + a) * nop + b);
                o2[0] = R.phi[jp] + R.phi[jm];
                o2[1] = R.phi_im[jp] + (conj[f] ? -R.phi_im[jm] : R.phi_im[jm]);
            }
}

void so_response_function(Context& cx, SOState& s, int nfreq, const double* omega, double* out)
{
    so_need_plain(cx, RSP_WHO, RSP_PLAIN);
    const char* who = "afesp_ccsd_so_response_function";
    SOResponse& R = so_response_need(s, who);
    need_mode(R, false, who);
    if (nfreq < 1 || !omega || !out) throw Error(1, std::string(who) + ": nfreq < 1 or a NULL argument");
    const int nop = R.nop;
    const int64_t nvec = vec_len(s);
    // ---- which stored frequency serves +omega and -omega of every request; all of them solved and converged?
    std::vector<int> plus(nfreq, -1), minus(nfreq, -1);
    for (int f = 0; f < nfreq; ++f) {
        for (int g = R.nfreq - 1; g >= 0; --g) {
            if (R.omega[g] == omega[f]) plus[f] = g;
            if (R.omega[g] == -omega[f]) minus[f] = g;
        }
        if (plus[f] < 0 || minus[f] < 0)
            throw Error(1, std::string(who) + ": the frequency " + std::to_string(omega[f]) + " was not solved at both signs by this response state");
    }
    for (int f = 0; f < nfreq; ++f)
        for (int g : {plus[f], minus[f]}) need_converged(R, who, g);
    // ---- Phi[X_a, R_j] of the systems that lack it: one density per solution, the traces on the host in a fixed order
    PhiWork work;
    for (int f = 0; f < nfreq; ++f)
        for (int g : {plus[f], minus[f]})
            for (int b = 0; b < nop; ++b) {
                const int j = b + nop * g;
                if (R.have_phi[j]) continue;
                work.column(cx, s, R, R.d.x + nvec * j, R.phi.data() + (size_t)nop * j);
                R.have_phi[j] = 1;
            }
    for (int f = 0; f < nfreq; ++f)
        for (int a = 0; a < nop; ++a)
            for (int b = 0; b < nop; ++b)
                out[((size_t)f * nop + a) * nop + b] = R.phi[a + (size_t)nop * (b + nop * plus[f])] + R.phi[b + (size_t)nop * (a + nop * minus[f])];
}

}  // namespace afesp
