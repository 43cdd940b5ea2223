// relax_so.hip -- the orbital gradient of the CCSD Lagrangian, the Z-vector equations and the relaxed one-particle density of the
// spin-orbital state (relax_so.h), term by term as tests/np_relax.py restates it (gradient_blocks).  The two o v^4 terms run
// on the pair-stored arrays through relax_pair_row_kernel; the dense terms through contract(); the solve is preconditioned conjugate
// gradients with the vectors resident and its three scalars per iteration read on the host.  Launches are plain call-by-call ones.
#include "device_util.h"
#include "relax_so.h"

#include <cmath>
#include <cstdio>

namespace afesp {
namespace {

constexpr int RX_MCAP = 6016;    // doubles of one pair column (or a segment of it) in LDS: v <= 110 holds a whole column
constexpr int RX_QCAP = 2048;    // doubles of one (i,b) slice of Q in LDS, i padded to a multiple of RX_IT; larger slices are read through the caches
constexpr int RX_IT = 8;         // occupied indices per work item
constexpr int RX_SPLIT = 512;    // blocks over the pair columns (c<d): two per compute unit
constexpr const char* RX_PLAIN = "orbital relaxation is";   // (so_need_plain)

// partial[blockIdx.x][i + o a] = sum over the block's pair columns (c<d) of sum_b P(ab; cd) Q(i,b,c,d).  P(., cd) is one column of the
// pair matrix (a<b at a + b(b-1)/2, leading dimension ld), read from memory once into LDS and used there for both of its images
// P(ab) = -P(ba); the (i,b) slice of Q of the column is staged beside it (STAGED) and read as a broadcast by the work items, each of which
// holds one row a and RX_IT occupied indices in registers.  Work items [item0, item0 + 256) of v ceil(o / RX_IT) per launch.  A column that
// exceeds mcap <= RX_MCAP doubles is walked in segments of whole b (each at least one b: v - 1 <= mcap is the launcher's to check).  The
// order of every sum is fixed by (o, v) and mcap alone.
template <bool STAGED>
__global__ __launch_bounds__(TB) void relax_pair_row_kernel(double* __restrict__ partial, const double* __restrict__ P, int64_t ld,
                                                            const double* __restrict__ Q, int o, int v, int64_t npv, int64_t chunk, int item0,
                                                            int nitems, int mcap)
{
    __shared__ double Msh[RX_MCAP];
    __shared__ __attribute__((aligned(16))) double Qsh[STAGED ? RX_QCAP : 2];
    const int64_t O = o, V = v;
    const int op = (o + RX_IT - 1) / RX_IT * RX_IT;   // the staged slice is (op, v), zero beyond o: whole 16-byte reads per work item
    const int item = item0 + (int)threadIdx.x;
    const bool active = item < nitems;
    const int r = active ? item % v : 0, i0 = active ? (item / v) * RX_IT : 0;
    int ii[RX_IT];
#pragma unroll
    for (int k = 0; k < RX_IT; ++k) ii[k] = min(i0 + k, o - 1);
    double acc[RX_IT];
#pragma unroll
    for (int k = 0; k < RX_IT; ++k) acc[k] = 0.0;
    const int64_t cd0 = (int64_t)blockIdx.x * chunk, cd1 = min(npv, cd0 + chunk);
    int c = 0, d = 1;
    if (cd0 < cd1) unpair_lt(cd0, c, d);
    const int rb = r * (r - 1) / 2;   // (v <= RX_MCAP + 1: every pair index fits 32 bits)
    for (int64_t cd = cd0; cd < cd1; ++cd) {
        const double* col = P + ld * cd;
        const double* qg = Q + O * V * ((int64_t)c + V * d);
        __syncthreads();   // (the slice and the last segment of the column before are done with)
        if (STAGED)
            for (int x = threadIdx.x; x < op * v; x += TB) {
                const int i = x % op, b = x / op;
                Qsh[x] = i < o ? qg[i + O * b] : 0.0;
            }
        int b0 = 1;
        while (b0 < v) {
            const int sb = b0 * (b0 - 1) / 2;
            int b1 = b0 + 1;
            while (b1 < v && (b1 + 1) * b1 / 2 - sb <= mcap) ++b1;   // pairs with b in [b0, b1)
            const int count = b1 * (b1 - 1) / 2 - sb;
            if (b0 > 1) __syncthreads();
            for (int x = threadIdx.x; x < count; x += TB) Msh[x] = col[sb + x];
            __syncthreads();
            if (active && r < b1) {
                // every b < b1 in turn, the same b in all lanes (the slice is read as a broadcast); a lane takes P(b r) = -P(r b) below
                // its row -- stored in this segment when r is --, P(r b) above it, and zero where the element is not in the segment
                const bool rin = r >= b0;
                int tb = 0;   // b (b - 1) / 2
#pragma unroll 4
                for (int b = 0; b < b1; ++b) {
                    const bool below = b < r;
                    const bool valid = below ? rin : (b > r && b >= b0);
                    const int idx = valid ? (below ? rb + b : tb + r) - sb : 0;
                    double m = Msh[idx];
                    m = below ? -m : m;
                    m = valid ? m : 0.0;
                    if (STAGED) {
                        const double2* q = reinterpret_cast<const double2*>(Qsh + i0 + op * b);
#pragma unroll
                        for (int k = 0; k < RX_IT / 2; ++k) {
                            const double2 qq = q[k];
                            acc[2 * k] = fma(m, qq.x, acc[2 * k]);
                            acc[2 * k + 1] = fma(m, qq.y, acc[2 * k + 1]);
                        }
                    } else {
#pragma unroll
                        for (int k = 0; k < RX_IT; ++k) acc[k] = fma(m, qg[ii[k] + O * b], acc[k]);
                    }
                    tb += b;
                }
            }
            b0 = b1;
        }
        if (++c == d) { c = 0; ++d; }
    }
    if (active) {
        double* out = partial + (int64_t)blockIdx.x * O * V;
#pragma unroll
        for (int k = 0; k < RX_IT; ++k)
            if (i0 + k < o) out[(i0 + k) + O * r] = acc[k];
    }
}

// F(p,q) over all o + v spin orbitals: the levels on the diagonal, f_ov / f_oo / f_vv (off-diagonal) where the state has them
__global__ void relax_fock_kernel(double* F, const double* lev, const double* e, const double* fov, const double* foo, const double* fvv, int o, int v)
{
    const int64_t O = o, V = v, N = O + V;
    GRID_STRIDE(x, N * N)
    {
        const int64_t p = x % N, q = x / N;
        double val = 0.0;
        if (p == q) val = lev ? lev[p] : e[p / 2];
        else if (fov) {
            if (p < O && q < O) val = foo[p + O * q];
            else if (p >= O && q >= O) val = fvv[(p - O) + V * (q - O)];
            else val = p < O ? fov[p + O * (q - O)] : fov[q + O * (p - O)];
        }
        F[x] = val;
    }
}

// w(i,a) = 2 [x(i,a) + (F D)(a,i) - (F D)(i,a) + sum_k p1[k](i,a) - sum_k p2[k](i,a)], the split sums in the order of k
__global__ void relax_assemble_kernel(double* w, const double* x, const double* FD, const double* p1, const double* p2, int nsplit, int o, int v)
{
    const int64_t O = o, V = v, N = O + V;
    GRID_STRIDE(y, O * V)
    {
        const int64_t i = y % O, a = y / O;
        double s1 = 0.0, s2 = 0.0;
        for (int k = 0; k < nsplit; ++k) {
            s1 += p1[(int64_t)k * O * V + y];
            s2 += p2[(int64_t)k * O * V + y];
        }
        w[y] = 2.0 * (((x[y] + (FD[(O + a) + N * i] - FD[i + N * (O + a)])) + s1) - s2);
    }
}

__global__ void relax_split_sum_kernel(double* out, const double* p, int nsplit, int64_t n)
{
    GRID_STRIDE(y, n)
    {
        double s = 0.0;
        for (int k = 0; k < nsplit; ++k) s += p[(int64_t)k * n + y];
        out[y] = s;
    }
}

// y(i,a) -= D1(i,a) x(i,a): the diagonal (e_a - e_i) of the Z-vector operator
__global__ void relax_diag_kernel(double* y, const double* D1, const double* x, int64_t n)
{
    GRID_STRIDE(k, n) y[k] = fma(-D1[k], x[k], y[k]);
}

// out[0] = a . b, out[1] = c . d, one block, fixed order
__global__ void relax_dot2_kernel(double* out, const double* a, const double* b, const double* c, const double* d, int64_t n)
{
    __shared__ double sm[8];
    double s[2] = {0.0, 0.0};
    for (int64_t k = threadIdx.x; k < n; k += TB) {
        s[0] = fma(a[k], b[k], s[0]);
        s[1] = fma(c[k], d[k], s[1]);
    }
    block_sum<2>(s, sm);
    if (threadIdx.x == 0) {
        out[0] = s[0];
        out[1] = s[1];
    }
}

// The interleaved (RHF-fed) order holds spin orbital 2 P + spin: exchanging the two spins of (i,a) is (i ^ 1, a ^ 1) (o is even there).
// out = 1/2 (x + sgn x with the spins exchanged): the part of x that is symmetric (sgn = 1) or antisymmetric (-1) under the exchange,
// to the bit; sgn = 0 copies
__global__ void relax_spin_part_kernel(double* out, const double* x, int sgn, int o, int64_t n)
{
    GRID_STRIDE(k, n)
    {
        const int64_t i = k % o, a = k / o;
        out[k] = sgn ? 0.5 * (x[k] + (double)sgn * x[(i ^ 1) + (int64_t)o * (a ^ 1)]) : x[k];
    }
}

// r = -b, zz = r / (e_a - e_i), p = zz
__global__ void relax_cg_start_kernel(double* r, double* p, double* zz, const double* b, const double* D1, int64_t n)
{
    GRID_STRIDE(k, n)
    {
        const double rk = -b[k], m = -rk / D1[k];
        r[k] = rk;
        zz[k] = m;
        p[k] = m;
    }
}

// z += alpha p, r -= alpha Ap, zz = r / (e_a - e_i)
__global__ void relax_cg_step_kernel(double* z, double* r, double* zz, const double* p, const double* Ap, const double* D1, double alpha, int64_t n)
{
    GRID_STRIDE(k, n)
    {
        z[k] = fma(alpha, p[k], z[k]);
        const double rk = fma(-alpha, Ap[k], r[k]);
        r[k] = rk;
        zz[k] = -rk / D1[k];
    }
}

__global__ void relax_cg_dir_kernel(double* p, const double* zz, double beta, int64_t n)
{
    GRID_STRIDE(k, n) p[k] = fma(beta, p[k], zz[k]);
}

// D_rel = D with 1/2 z(i,a) added to (i, o+a) and written to both images
__global__ void relax_density_kernel(double* out, const double* D, const double* z, int o, int v)
{
    const int64_t O = o, V = v, N = O + V;
    GRID_STRIDE(x, N * N)
    {
        const int64_t p = x % N, q = x / N;
        double val = D[x];
        if ((p < O) != (q < O)) {
            const int64_t i = p < O ? p : q, a = (p < O ? q : p) - O;
            val = fma(0.5, z[i + O * a], D[i + N * (O + a)]);
        }
        out[x] = val;
    }
}

struct Split { int64_t chunk; int nsplit; };
Split split_of(int64_t npv)
{
    const int64_t chunk = std::max<int64_t>(1, (npv + RX_SPLIT - 1) / RX_SPLIT);
    return {chunk, (int)((npv + chunk - 1) / chunk)};
}

// the split partials of out(i,a) = sum_b sum_{c<d} P(ab; cd) Q(i,b,c,d) -> number of splits (0: no pairs, nothing launched)
int pair_row(Context& cx, SOState& s, const double* P, const double* Q, double* partial)
{
    const int o = s.o, v = s.v;
    const int64_t npv = pair_count(v);
    if (npv == 0 || !P) return 0;
    if (v - 1 > RX_MCAP) throw Error(1, "orbital gradient: more than " + std::to_string(RX_MCAP + 1) + " virtual spin orbitals are not supported by the pair-row kernel");
    const int mcap = std::max(v - 1, std::min(knobs().relax_mcap, RX_MCAP));   // (a segment holds at least the longest b)
    const Split sp = split_of(npv);
    const int nitems = v * ((o + RX_IT - 1) / RX_IT);
    const bool staged = (int64_t)((o + RX_IT - 1) / RX_IT * RX_IT) * v <= std::min(knobs().relax_qcap, RX_QCAP);
    for (int item0 = 0; item0 < nitems; item0 += TB) {
        if (staged) LAUNCH(relax_pair_row_kernel<true>, sp.nsplit, partial, P, s.lad_ka, Q, o, v, npv, sp.chunk, item0, nitems, mcap);
        else LAUNCH(relax_pair_row_kernel<false>, sp.nsplit, partial, P, s.lad_ka, Q, o, v, npv, sp.chunk, item0, nitems, mcap);
    }
    return sp.nsplit;
}

SORelax& relax_of(Context& cx, SOState& s, SOLambda& L, const char* who)
{
    if (L.rx) return *L.rx;
    if (!cx.fits(so_relax_bytes(s.o, s.v)))
        throw Error(LAMBDA_ERR_CAPACITY, std::string(who) + ": the orbital gradient of this system does not fit the free device memory");
    preload_relax_so();
    L.rx = new SORelax();
    try {
        L.rx->vec = cx.alloc(6 * (int64_t)s.o * s.v);
    } catch (...) {
        delete L.rx;
        L.rx = nullptr;
        throw;
    }
    return *L.rx;
}

// w(i,a) on the device
void gradient(Context& cx, SOState& s, SODensity2& G, int fock_response, double* w, const char* who)
{
    const int o = s.o, v = s.v;
    const int64_t O = o, V = v, N = O + V, npv = pair_count(V);
    const auto C = contractor(cx);
    double* D = so_density_device(cx, s, who);
    double* F = cx.scratch("rx_F", N * N);
    Tensor FD = view(cx.scratch("rx_FD", N * N), {N, N}), X = view(cx.scratch("rx_X", O * V), {O, V});
    LAUNCH(relax_fock_kernel, grid_for(N * N, SO_GRID_CAP), F, (const double*)s.lev, (const double*)s.e, s.fock ? (const double*)s.f_ov.d : nullptr,
              s.fock ? (const double*)s.f_oo.d : nullptr, s.fock ? (const double*)s.f_vv.d : nullptr, o, v);
    C(1.0, view(F, {N, N}), "pr", view(D, {N, N}), "rq", 0.0, FD, "pq");
    // ---- the dense terms of X_ai - X_ia over the stored blocks of Gamma (np_relax.gradient_blocks, in its order)
    C(-0.5, s.ooov, "klja", G.oooo, "ijkl", 0.0, X, "ia");
    C(1.0, s.ovvo, "jabk", G.ooov, "ijkb", 1.0, X, "ia");
    C(-0.5, s.ovvv, "jabc", G.oovv, "ijbc", 1.0, X, "ia");
    C(0.5, s.oovv, "jkab", G.ooov, "jkib", 1.0, X, "ia");
    C(1.0, s.ovvv, "jcab", G.ovov, "ibjc", 1.0, X, "ia");
    C(0.5, s.oooo, "ijkl", G.ooov, "klja", 1.0, X, "ia");
    C(1.0, s.ooov, "ijkb", G.ovov, "jakb", 1.0, X, "ia");
    C(0.5, s.oovv, "ijbc", G.ovvv, "jabc", 1.0, X, "ia");
    C(-0.5, s.ooov, "jkib", G.oovv, "jkab", 1.0, X, "ia");
    C(1.0, s.ovvo, "ibcj", G.ovvv, "jcab", 1.0, X, "ia");
    if (fock_response) {
        // 2 sum_pq D_pq <pa||qi>: the oo, ov (twice) and vv blocks of D as strided views of the matrix
        Tensor doo = view(D, {O, O}), dov = view(D + N * O, {O, V}), dvv = view(D + N * O + O, {V, V});
        doo.stride[1] = dov.stride[1] = dvv.stride[1] = N;
        C(1.0, doo, "jk", s.ooov, "kija", 1.0, X, "ia");
        C(1.0, dov, "jb", s.ovvo, "jabi", 1.0, X, "ia");
        C(1.0, dov, "jb", s.oovv, "jiba", 1.0, X, "ia");
        C(1.0, dvv, "bc", s.ovvv, "icab", 1.0, X, "ia");
    }
    // ---- the two pair-row terms: <ab||cd> Gamma_ibcd and <ib||cd> Gamma_abcd
    const Split sp = split_of(std::max<int64_t>(npv, 1));
    double* p1 = cx.scratch("rx_p1", (int64_t)sp.nsplit * O * V);
    double* p2 = cx.scratch("rx_p2", (int64_t)sp.nsplit * O * V);
    // (a state without an occupied pair has no va: Gamma_ovvv and ga are zero there, as density2_so.hip leaves them)
    const int n1 = pair_row(cx, s, s.va, G.ovvv.d, p1);
    const int n2 = pair_row(cx, s, G.ga, s.ovvv.d, p2);
    if (n1 != n2) {   // one of the pair arrays is missing: its term is zero
        if (!n1) k_fill(cx, p1, (int64_t)n2 * O * V, 0.0);
        if (!n2) k_fill(cx, p2, (int64_t)n1 * O * V, 0.0);
    }
    LAUNCH(relax_assemble_kernel, grid_for(O * V, SO_GRID_CAP), w, X.d, FD.d, p1, p2, std::max(n1, n2), o, v);
}

// y = A x on the device, (i,a) arrays
void apply(Context& cx, SOState& s, const double* x, double* y)
{
    const int64_t O = s.o, V = s.v;
    Tensor Xt = view(const_cast<double*>(x), {O, V}), Yt = view(y, {O, V});
    contract(cx, 1.0, s.oovv, "ijab", Xt, "jb", 0.0, Yt, "ia");
    contract(cx, 1.0, s.ovvo, "jabi", Xt, "jb", 1.0, Yt, "ia");
    LAUNCH(relax_diag_kernel, grid_for(O * V, SO_GRID_CAP), y, s.D1.d, x, O * V);
}

}  // namespace

void preload_relax_so()
{
    static const bool loaded = [] {
        first_use_touch(reinterpret_cast<const void*>(relax_pair_row_kernel<true>));
        first_use_touch(reinterpret_cast<const void*>(relax_pair_row_kernel<false>));
        first_use_touch(reinterpret_cast<const void*>(relax_fock_kernel));
        first_use_touch(reinterpret_cast<const void*>(relax_assemble_kernel));
        first_use_touch(reinterpret_cast<const void*>(relax_split_sum_kernel));
        first_use_touch(reinterpret_cast<const void*>(relax_diag_kernel));
        first_use_touch(reinterpret_cast<const void*>(relax_dot2_kernel));
        first_use_touch(reinterpret_cast<const void*>(relax_spin_part_kernel));
        first_use_touch(reinterpret_cast<const void*>(relax_cg_start_kernel));
        first_use_touch(reinterpret_cast<const void*>(relax_cg_step_kernel));
        first_use_touch(reinterpret_cast<const void*>(relax_cg_dir_kernel));
        first_use_touch(reinterpret_cast<const void*>(relax_density_kernel));
        (void)hipGetLastError();
        return true;
    }();
    (void)loaded;
}

double so_relax_bytes(int64_t o, int64_t v)
{
    const double O = (double)o, V = (double)v, N = O + V;
    // the six vectors; F, F D, X, the host mirrors of x / y; the split partials of the two pair-row terms; the relaxed matrix
    return 8.0 * (6.0 * O * V + 3.0 * N * N + 3.0 * O * V + 2.0 * RX_SPLIT * O * V);
}

void so_relax_free(Context& cx, SOLambda& L)
{
    if (!L.rx) return;
    cx.release(L.rx->vec);
    delete L.rx;
    L.rx = nullptr;
}

void so_orbital_gradient(Context& cx, SOState& s, int fock_response, double* w_host, int64_t capacity)
{
    const char* who = "afesp_ccsd_so_orbital_gradient";
    so_need_plain(cx, who, RX_PLAIN);
    if (fock_response != 0 && fock_response != 1) throw Error(1, std::string(who) + ": fock_response must be 0 or 1");
    SODensity2& G = so_density2_need(s, who);
    const int64_t n = (int64_t)s.o * s.v;
    if (!w_host || capacity < n)
        throw Error(LAMBDA_ERR_CAPACITY, std::string(who) + ": the buffer holds " + std::to_string(w_host ? capacity : 0) + " doubles, the gradient needs o v = " +
                                             std::to_string(n));
    SORelax& R = relax_of(cx, s, *s.lam, who);
    // (into the work vector Ap, not w: a converged solve keeps the right-hand side it was made from)
    double* w = R.vec + 4 * n;
    gradient(cx, s, G, fock_response, w, who);
    AFESP_HIP(hipMemcpyAsync(w_host, w, sizeof(double) * n, hipMemcpyDeviceToHost, cx.stream));
    cx.sync();
}

void so_zvector_apply(Context& cx, SOState& s, const double* x_host, double* y_host)
{
    const char* who = "afesp_ccsd_so_zvector_apply";
    so_need_plain(cx, who, RX_PLAIN);
    if (!x_host || !y_host) throw Error(1, std::string(who) + ": NULL argument");
    so_density2_need(s, who);
    const int64_t n = (int64_t)s.o * s.v;
    relax_of(cx, s, *s.lam, who);
    double* xy = cx.scratch("rx_xy", 2 * n);
    AFESP_HIP(hipMemcpyAsync(xy, x_host, sizeof(double) * n, hipMemcpyHostToDevice, cx.stream));
    apply(cx, s, xy, xy + n);
    AFESP_HIP(hipMemcpyAsync(y_host, xy + n, sizeof(double) * n, hipMemcpyDeviceToHost, cx.stream));
    cx.sync();
}

void so_zvector_solve(Context& cx, SOState& s, double tol, int maxiter, double* z_host, int* iters, double* resid)
{
    const char* who = "afesp_ccsd_so_zvector_solve";
    so_need_plain(cx, who, RX_PLAIN);
    if (!(tol > 0.0) || maxiter < 1) throw Error(1, std::string(who) + ": tol must be positive and maxiter at least 1");
    SODensity2& G = so_density2_need(s, who);
    if (s.fock)
        throw Error(RELAX_ERR_NOT_HF, std::string(who) + ": the reference of a state made by afesp_ccsd_uso_init_fock is not stationary in the spin-orbital "
                                                         "rotations (a restricted open-shell Z-vector is not built)");
    SOLambda& L = *s.lam;
    SORelax& R = relax_of(cx, s, L, who);
    const int64_t n = (int64_t)s.o * s.v;
    double *w = R.vec, *z = w + n, *r = z + n, *p = r + n, *Ap = p + n, *zz = Ap + n;
    R.epoch = R.stamp = -1;
    R.iters = R.negative = 0;
    gradient(cx, s, G, 1, w, who);
    k_fill(cx, z, n, 0.0);
    // The operator of the interleaved (RHF-fed) state commutes with the exchange of the two spins, so the equations fall into a symmetric
    // and an antisymmetric part.  They are solved one after the other, each iteration kept in its part to the bit (A p is projected; the
    // element-wise updates preserve the symmetry): a reference with a triplet instability has negative eigenvalues in the antisymmetric
    // part, which rounding noise of a spin-pure right-hand side must not reach (it grows there by the residual polynomial's value at a
    // negative eigenvalue, exponentially in the iteration count).  A part whose right-hand side is below its share of tol is converged as
    // it stands.  Every other state: one pass over the whole space.
    const int nparts = s.lev ? 1 : 2;
    const double part_tol = tol / std::sqrt((double)nparts);
    double rr_sum = 0.0;
    bool converged = true;
    std::string trouble;
    char num[64];
    for (int part = 0; part < nparts && trouble.empty(); ++part) {
        const int sgn = nparts == 1 ? 0 : (part == 0 ? 1 : -1);
        LAUNCH(relax_spin_part_kernel, grid_for(n, SO_GRID_CAP), Ap, w, sgn, s.o, n);
        LAUNCH(relax_cg_start_kernel, grid_for(n, SO_GRID_CAP), r, p, zz, Ap, s.D1.d, n);
        LAUNCH(relax_dot2_kernel, 1, cx.scal, r, zz, r, r, n);
        const double* h = host_scalars(cx, 2);
        double rz = h[0], rr = h[1];
        bool done = std::sqrt(rr) < part_tol;
        while (!done && R.iters < maxiter) {
            apply(cx, s, p, zz);   // (zz is free between the direction update and the next step)
            LAUNCH(relax_spin_part_kernel, grid_for(n, SO_GRID_CAP), Ap, zz, sgn, s.o, n);
            LAUNCH(relax_dot2_kernel, 1, cx.scal, p, Ap, p, Ap, n);
            const double pAp = host_scalars(cx, 1)[0];
            // Negative curvature alone does not stop the iteration: at a saddle point of the SCF energy (an unstable but stationary
            // reference) A is indefinite and the equations still have their solution.  A breakdown does: p A p = 0 is a singular A
            // (an instability threshold); a nearly singular one stagnates and ends at maxiter.
            if (pAp == 0.0 || !std::isfinite(pAp)) {
                snprintf(num, sizeof num, "%.3e", pAp);
                trouble = std::string(" (a direction with p A p = ") + num + ": the orbital Hessian of the reference is singular)";
                break;
            }
            if (pAp < 0.0) ++R.negative;
            const double alpha = rz / pAp;
            LAUNCH(relax_cg_step_kernel, grid_for(n, SO_GRID_CAP), z, r, zz, p, Ap, s.D1.d, alpha, n);
            LAUNCH(relax_dot2_kernel, 1, cx.scal, r, zz, r, r, n);
            h = host_scalars(cx, 2);
            const double rz_new = h[0];
            rr = h[1];
            ++R.iters;
            done = std::sqrt(rr) < part_tol;
            if (done) break;
            LAUNCH(relax_cg_dir_kernel, grid_for(n, SO_GRID_CAP), p, zz, rz_new / rz, n);
            rz = rz_new;
        }
        rr_sum += rr;
        converged = converged && done;
    }
    const double rr = rr_sum;
    R.resid = std::sqrt(rr);
    if (iters) *iters = R.iters;
    if (resid) *resid = R.resid;
    if (!converged)
    {
        snprintf(num, sizeof num, "%.3e", R.resid);
        throw Error(RELAX_ERR_NOT_CONVERGED, std::string(who) + ": residual " + num + " after " + std::to_string(R.iters) + " iterations, tol not reached" + trouble);
    }
    if (z_host) AFESP_HIP(hipMemcpyAsync(z_host, z, sizeof(double) * n, hipMemcpyDeviceToHost, cx.stream));
    cx.sync();
    R.epoch = s.amp_epoch;
    R.stamp = L.stamp;
}

void so_relaxed_density(Context& cx, SOState& s, double* d_host, int64_t capacity)
{
    const char* who = "afesp_ccsd_so_relaxed_density";
    so_need_plain(cx, who, RX_PLAIN);
    so_density2_need(s, who);
    if (s.fock)
        throw Error(RELAX_ERR_NOT_HF, std::string(who) + ": the reference of a state made by afesp_ccsd_uso_init_fock is not stationary in the spin-orbital "
                                                         "rotations (a restricted open-shell Z-vector is not built)");
    SOLambda& L = *s.lam;
    if (!L.rx || L.rx->epoch != s.amp_epoch || L.rx->stamp != L.stamp)
        throw Error(LAMBDA_ERR_STALE, std::string(who) + ": no converged Z-vector of the current t and lambda (call afesp_ccsd_so_zvector_solve)");
    const int64_t O = s.o, V = s.v, N = O + V;
    if (!d_host || capacity < N * N)
        throw Error(LAMBDA_ERR_CAPACITY, std::string(who) + ": the buffer holds " + std::to_string(d_host ? capacity : 0) + " doubles, the density needs (o + v)^2 = " +
                                             std::to_string(N * N));
    const double* D = so_density_device(cx, s, who);
    double* out = cx.scratch("rx_Drel", N * N);
    LAUNCH(relax_density_kernel, grid_for(N * N, SO_GRID_CAP), out, D, L.rx->vec + O * V, s.o, s.v);
    AFESP_HIP(hipMemcpyAsync(d_host, out, sizeof(double) * N * N, hipMemcpyDeviceToHost, cx.stream));
    cx.sync();
}

double so_relax_pair_row(Context& cx, SOState& s, int which, double* out_host, int reps)
{
    const char* who = "afesp_ccsd_so_relax_pair_row";
    so_need_plain(cx, who, RX_PLAIN);
    if (which != 0 && which != 1) throw Error(1, std::string(who) + ": which must be 0 or 1");
    SODensity2& G = so_density2_need(s, who);
    relax_of(cx, s, *s.lam, who);
    const int64_t n = (int64_t)s.o * s.v;
    const Split sp = split_of(std::max<int64_t>(pair_count(s.v), 1));
    double* p1 = cx.scratch("rx_p1", (int64_t)sp.nsplit * n);
    double* out = cx.scratch("rx_xy", 2 * n);
    const double* P = which ? G.ga : s.va;
    const double* Q = which ? s.ovvv.d : G.ovvv.d;
    struct Event { hipEvent_t e = nullptr; ~Event() { if (e) (void)hipEventDestroy(e); } } a, b;
    AFESP_HIP(hipEventCreate(&a.e));
    AFESP_HIP(hipEventCreate(&b.e));
    int ns = pair_row(cx, s, P, Q, p1);   // the warm call
    AFESP_HIP(hipEventRecord(a.e, cx.stream));
    for (int k = 0; k < reps; ++k) ns = pair_row(cx, s, P, Q, p1);
    AFESP_HIP(hipEventRecord(b.e, cx.stream));
    LAUNCH(relax_split_sum_kernel, grid_for(n, SO_GRID_CAP), out, p1, ns, n);
    if (out_host) AFESP_HIP(hipMemcpyAsync(out_host, out, sizeof(double) * n, hipMemcpyDeviceToHost, cx.stream));
    cx.sync();
    float ms = 0.f;
    if (reps > 0) AFESP_HIP(hipEventElapsedTime(&ms, a.e, b.e));
    return reps > 0 ? (double)ms / reps : 0.0;
}

}  // namespace afesp
