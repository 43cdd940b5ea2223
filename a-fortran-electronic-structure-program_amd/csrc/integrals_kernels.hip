// integrals_kernels.hip -- the kernels of the integral layer (integrals_kernels.h lists them; host side: integrals.hip).
// All tensors are Fortran column-major (first index fastest); lanes run along the fastest index.
#include "device_util.h"
#include "fcidump_parse.h"
#include "integrals_kernels.h"

using namespace afesp;

extern "C" {   // (the names these kernels have in profiles: plain, as the entry points' own)
// ---- a quarter transform on the LDS-DMA GEMM (tgemm.h): out(x2, m, S) = sum_x1 C(m, x1) in(x1, x2, S)
// The transformed index is the fastest one of `in`, so every column (x2, S) of the product is a contiguous run of n doubles: both
// operands are contiguous along the summation index (C goes in as a zero-padded transpose), which is all that kernel asks for.
// The result comes out with x2 fastest and the new index second -- the layout the NEXT quarter transform wants for its input
// (and the one the old path produced after two of them: (p,q,K), (r,s,P)).  Needs an even n (16-byte chunks, pairs of columns).
__global__ __launch_bounds__(256) void ao2mo_ct_kernel(double* ct, const double* c, int n, int Kc)
{
    for (int x = blockIdx.x * blockDim.x + threadIdx.x; x < n * Kc; x += gridDim.x * blockDim.x) {
        const int m = x / Kc, k = x % Kc;
        ct[x] = k < n ? c[m + n * k] : 0.0;
    }
}
// rowA[m] = byte offset of row m of the padded transpose; colB[c] = byte offset of column c = x2 + n Sloc of a slab of `in`;
// offCm[m] = ld m; offCn[c] = x2 + ld n Sloc (elements); the pads behind them (tgemm.h) are zero.
// ld: the temporaries' columns are ld doubles long (n of them data, the rest zero): ld = Kc puts every column on a 128-byte line
__global__ __launch_bounds__(256) void ao2mo_tables_kernel(uint32_t* rowA, uint32_t* colB, int64_t* offCm, int64_t* offCn, int n, int Kc, int64_t ncol, int64_t ld)
{
    for (int64_t x = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; x < ncol + 256; x += (int64_t)gridDim.x * blockDim.x) {
        if (x < n + 256) rowA[x] = x < n ? (uint32_t)(8 * Kc * x) : 0u;
        if (x < n + 128) offCm[x] = x < n ? ld * x : 0;
        colB[x] = x < ncol ? (uint32_t)(8 * ld * x) : 0u;
        if (x < ncol + 128) offCn[x] = x < ncol ? (x % n) + ld * n * (x / n) : 0;
    }
}

// The second pair of transforms is only needed where the packed result has an entry: (rs|PQ) for RS <= PQ, i.e. r <= p(PQ).  The
// last transform therefore runs over the columns (r, PQ) with r <= p only -- p + 1 of them per pair PQ = tri(p, q), rounded up to
// an even count (pairs of columns are stored together) -- about half of all: colB / offCn list them pair by pair, relative to
// the pair's slab (cstart[PQ] = first column of the pair).
__global__ __launch_bounds__(256) void ao2mo_tables_tri_kernel(uint32_t* colB, int64_t* offCn, const int64_t* cstart, int n, int64_t np, int64_t sl, int64_t ld)
{
    for (int64_t P = blockIdx.x; P < np; P += gridDim.x) {
        const int64_t c0 = cstart[P], cnt = cstart[P + 1] - c0, rel = P % sl;
        for (int64_t r = threadIdx.x; r < cnt; r += blockDim.x) {
            colB[c0 + r] = (uint32_t)(8 * ld * (r + (int64_t)n * rel));
            offCn[c0 + r] = r + ld * n * rel;
        }
    }
}

// columns (x2, S) with x2 < TG_BM only (the pair transposition behind the second transform reads its result (x2, m, S) for
// x2 <= m only: the rows m < 128 are needed for these columns only), relative to a slab: column c = x2 + 128 Sloc
__global__ __launch_bounds__(256) void ao2mo_tables_lo_kernel(uint32_t* colB, int64_t* offCn, int n, int cnt, int64_t ncol, int64_t ld)
{
    for (int64_t x = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; x < ncol + 256; x += (int64_t)gridDim.x * blockDim.x) {
        const int64_t x2 = x % cnt, sloc = x / cnt;
        colB[x] = x < ncol ? (uint32_t)(8 * ld * (x2 + (int64_t)n * sloc)) : 0u;
        if (x < ncol + 128) offCn[x] = x < ncol ? x2 + ld * n * sloc : 0;
    }
}
// ---- the two spin Fock operators of a restricted determinant (afesp_mo_fock_ro, afesp_read_fcidump_rohf) out of ONE packed MO array:
//   F_a(p,q) = h(p,q) + sum_{i < na} [(pq|ii) - (pi|qi)] + sum_{i < nb} (pq|ii),   F_b: na and nb exchanged
// One wave per pair p >= q, as k_fock_mo: lane l takes i = l, l + 64, ... in rising order -- the Coulomb sum over the doubly occupied
// orbitals i < nb, the one over the singly occupied ones nb <= i < na and the two exchange sums are kept apart -- the 64 partial sums are
// added in a fixed butterfly order and both triangles are written from one register: symmetric to the bit, the same on every run.
// (The butterfly is this kernel's own: wave_sum adds in another order, and the ROHF operators are kept to the bit.)
__global__ __launch_bounds__(256) void fock_ro_kernel(double* __restrict__ fa, double* __restrict__ fb, const double* __restrict__ h,
                                                      const double* __restrict__ packed, int n, int na, int nb)
{
    const int lane = threadIdx.x & 63;
    const int64_t np = (int64_t)n * (n + 1) / 2, w = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (w >= np) return;   // (whole waves leave)
    int64_t q, p;
    unpair(w, q, p);
    double jd = 0.0, js = 0.0, kd = 0.0, ks = 0.0;   // Coulomb / exchange over the doubly / the singly occupied orbitals
    for (int64_t i = lane; i < na; i += 64) {
        const double J = packed[tri(w, tri(i, i))], K = packed[tri(tri(p, i), tri(q, i))];
        if (i < nb) { jd += J; kd += K; }
        else { js += J; ks += K; }
    }
    for (int off = 32; off > 0; off >>= 1) {
        jd += __shfl_xor(jd, off, 64);
        js += __shfl_xor(js, off, 64);
        kd += __shfl_xor(kd, off, 64);
        ks += __shfl_xor(ks, off, 64);
    }
    if (lane == 0) {
        const int64_t lo = p + (int64_t)n * q, up = q + (int64_t)n * p;
        const double h0 = h[lo], jj = (jd + jd) + js;
        const double va = h0 + (jj - (kd + ks)), vb = h0 + (jj - kd);
        fa[lo] = va; fa[up] = va;
        fb[lo] = vb; fb[up] = vb;
    }
}
}  // extern "C"

namespace afesp {

namespace {
// mp2.f90:418-440 on the <ij|ab> slice
__global__ __launch_bounds__(TB) void mp2_energy_kernel(double* partial, const double* voovv, const double* D2, int o, int v)
{
    __shared__ double sm[4];
    const int64_t n = (int64_t)o * o * v * v;
    double acc[1] = {0.0};
    GRID_STRIDE(x, n)
    {
        int i = (int)(x % o);
        int64_t r = x / o;
        int j = (int)(r % o);
        r /= o;
        int a = (int)(r % v), b = (int)(r / v);
        double vx = voovv[i + (int64_t)o * (j + (int64_t)o * (b + (int64_t)v * a))];
        acc[0] += voovv[x] * (2.0 * voovv[x] - vx) / D2[x];
    }
    block_sum<1>(acc, sm);
    if (threadIdx.x == 0) partial[blockIdx.x] = acc[0];
}
// The same sum straight from the packed MO integrals (<ij|ab> = (ia|jb): mp2.f90:418-440 with the slice and the denominators formed on
// the fly), the ordered sum of the block partials by whichever block finishes last, and the result into the host's publishing
// area (contract.hip, host_scalars_slot): ONE launch where a small system's MP2 energy took five (slice, denominators, sum, final
// sum, publication: 29 of the 163 us of an AO->MO + MP2 call at n = 58).
struct Mp2Levels { double e[256]; };   // orbital energies by value (kernel arguments) when they fit: no upload in front of the launch
template <bool BYVAL>
__global__ __launch_bounds__(TB) void mp2_packed_kernel(double* partial, unsigned* counter, double* scal, double* pub, double seq,
                                                        const double* __restrict__ eri, const double* __restrict__ e_dev, Mp2Levels lv, int o, int v)
{
    __shared__ double sm[4];
    __shared__ bool last;
    __shared__ double e[BYVAL ? 256 : 1];
    if (BYVAL) {
        if ((int)threadIdx.x < o + v) e[threadIdx.x] = lv.e[threadIdx.x];
        __syncthreads();
    }
    const double* ep = BYVAL ? e : e_dev;
    const int64_t n = (int64_t)o * o * v * v;
    double acc[1] = {0.0};
    GRID_STRIDE(x, n)
    {
        const int i = (int)(x % o);
        int64_t r = x / o;
        const int j = (int)(r % o);
        r /= o;
        const int a = (int)(r % v), b = (int)(r / v);
        const int64_t ia = tri(o + a, i), jb = tri(o + b, j), ib = tri(o + b, i), ja = tri(o + a, j);
        const double vx = eri[tri(ia, jb)], vex = eri[tri(ib, ja)];
        acc[0] += vx * (2.0 * vx - vex) / (ep[i] + ep[j] - ep[o + a] - ep[o + b]);
    }
    block_sum<1>(acc, sm);
    if (threadIdx.x == 0) {
        partial[blockIdx.x] = acc[0];
        __threadfence();
        last = atomicInc(counter, gridDim.x - 1) == gridDim.x - 1;   // (wraps to zero: ready for the next call)
    }
    __syncthreads();
    if (!last) return;
    __threadfence();
    double tot[1] = {0.0};
    for (int b = threadIdx.x; b < (int)gridDim.x; b += blockDim.x) tot[0] += __builtin_nontemporal_load(&partial[b]);
    block_sum<1>(tot, sm);
    if (threadIdx.x == 0) {
        scal[0] = tot[0];
        if (pub) {
            pub[0] = tot[0];
            __threadfence_system();
            __hip_atomic_store(&pub[64], seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
        }
    }
}

// build_fock (hf.f90:349-385): F(i,j) = H(i,j) + sum_kl D(k,l) [2 (ij|kl) - (ik|jl)].  Both sums run over the half-unpacked
// integrals u(x,y,P) = (xy|ab), P = tri(a,b), a >= b -- the first stage of the AO->MO transform, built once per SCF -- so
// every unique pair slab is read once per sum, in 8-byte-per-lane coalesced rows, and every partial sum is combined in a
// fixed order (bit-reproducible run to run):
//   J(x,y)  = sum_P u(x,y,P) dv(P),  dv(P) = D(a,b) + D(b,a)  (D(a,a) on a == b)           fock_j_kernel, FOCK_CHUNKS partial sums
//   K(x,a) += sum_y u(x,y,P) D(y,b),   K(x,b) += sum_y u(x,y,P) D(y,a)  (a != b)              fock_k_kernel, one workgroup per slab
constexpr int FOCK_CHUNKS = 64;
__global__ void fock_dv_kernel(double* dv, const double* dens, int n)
{
    const int64_t np = (int64_t)n * (n + 1) / 2;
    GRID_STRIDE(p, np)
    {
        int b, a;
        unpair(p, b, a);
        dv[p] = a == b ? dens[a + (int64_t)n * a] : dens[a + (int64_t)n * b] + dens[b + (int64_t)n * a];
    }
}
// (ld: leading dimension of u(x, y, P), n or -- where afesp_ao2mo_mp2 will run its transforms on the LDS-DMA GEMM -- n rounded up to
// whole K steps, integrals.h: Ao2moForm)
__global__ __launch_bounds__(256) void fock_j_kernel(double* jpart, const double* u, const double* dv, int n, int ld)
{
    const int64_t n2 = (int64_t)n * n, np = (int64_t)n * (n + 1) / 2, pl = (int64_t)ld * n;
    const int64_t xy = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t per = (np + FOCK_CHUNKS - 1) / FOCK_CHUNKS, p0 = blockIdx.y * per, p1 = p0 + per < np ? p0 + per : np;
    if (xy >= n2) return;
    const int64_t at = xy % n + (int64_t)ld * (xy / n);
    double acc = 0.0;
#pragma unroll 8
    for (int64_t p = p0; p < p1; ++p) acc += u[at + pl * p] * dv[p];
    jpart[(int64_t)blockIdx.y * n2 + xy] = acc;
}
__global__ __launch_bounds__(256) void fock_k_kernel(double* kp1, double* kp2, const double* u, const double* dens, int n, int ld)
{
    extern __shared__ double dcol[];   // D(:,b) then D(:,a)
    const int64_t n2 = (int64_t)ld * n, p = blockIdx.x;
    int b, a;
    unpair(p, b, a);
    for (int y = threadIdx.x; y < n; y += 256) {
        dcol[y] = dens[y + (int64_t)n * b];
        dcol[n + y] = dens[y + (int64_t)n * a];
    }
    __syncthreads();
    const double* m = u + n2 * p;
    for (int x = threadIdx.x; x < n; x += 256) {
        double w1 = 0.0, w2 = 0.0;
#pragma unroll 8
        for (int y = 0; y < n; ++y) {
            const double v = m[x + (int64_t)ld * y];
            w1 += v * dcol[y];
            w2 += v * dcol[n + y];
        }
        kp1[p * n + x] = w1;
        kp2[p * n + x] = w2;
    }
}
// F(x,a) = H(x,a) + 2 sum_c jpart[c](x,a) - sum_{b<=a} kp1[tri(a,b)](x) - sum_{b>a} kp2[tri(b,a)](x)
__global__ void fock_reduce_kernel(double* fock, const double* hcore, const double* jpart, const double* kp1, const double* kp2, int n)
{
    const int64_t n2 = (int64_t)n * n;
    GRID_STRIDE(xa, n2)
    {
        const int x = (int)(xa % n), a = (int)(xa / n);
        double j = 0.0, k = 0.0;
        for (int c = 0; c < FOCK_CHUNKS; ++c) j += jpart[(int64_t)c * n2 + xa];
        for (int b = 0; b <= a; ++b) k += kp1[((int64_t)a * (a + 1) / 2 + b) * n + x];
        for (int b = a + 1; b < n; ++b) k += kp2[((int64_t)b * (b + 1) / 2 + a) * n + x];
        fock[xa] = hcore[xa] + 2.0 * j - k;
    }
}
// The unrestricted Fock matrices  F_s = H + J[Da + Db] - K[D_s]  (s = a, b) on the same half-unpacked integrals: J is one pass of
// fock_j_kernel with dv of the total density; the exchange kernel carries both spins' density columns, so every slab is read
// once for the two of them.  With Da = Db = D every partial sum is twice (J) or exactly (K) the one of k_build_fock, so the
// result is the RHF Fock matrix bit for bit.
__global__ void fock_dv_uhf_kernel(double* dv, const double* da, const double* db, int n)
{
    const int64_t np = (int64_t)n * (n + 1) / 2;
    GRID_STRIDE(p, np)
    {
        int b, a;
        unpair(p, b, a);
        const int64_t ab = a + (int64_t)n * b, ba = b + (int64_t)n * a;
        dv[p] = a == b ? da[ab] + db[ab] : (da[ab] + db[ab]) + (da[ba] + db[ba]);
    }
}
// kp[s][0]: sum_y u(x,y,P) D_s(y,b), kp[s][1]: sum_y u(x,y,P) D_s(y,a) -- each in fock_k_kernel's order
__global__ __launch_bounds__(256) void fock_k_uhf_kernel(double* kp1a, double* kp2a, double* kp1b, double* kp2b, const double* u,
                                                         const double* da, const double* db, int n, int ld)
{
    extern __shared__ double dcol[];   // Da(:,b), Da(:,a), Db(:,b), Db(:,a)
    const int64_t n2 = (int64_t)ld * n, p = blockIdx.x;
    int b, a;
    unpair(p, b, a);
    for (int y = threadIdx.x; y < n; y += 256) {
        dcol[y] = da[y + (int64_t)n * b];
        dcol[n + y] = da[y + (int64_t)n * a];
        dcol[2 * n + y] = db[y + (int64_t)n * b];
        dcol[3 * n + y] = db[y + (int64_t)n * a];
    }
    __syncthreads();
    const double* m = u + n2 * p;
    for (int x = threadIdx.x; x < n; x += 256) {
        double w1 = 0.0, w2 = 0.0, w3 = 0.0, w4 = 0.0;
#pragma unroll 8
        for (int y = 0; y < n; ++y) {
            const double v = m[x + (int64_t)ld * y];
            w1 += v * dcol[y];
            w2 += v * dcol[n + y];
            w3 += v * dcol[2 * n + y];
            w4 += v * dcol[3 * n + y];
        }
        kp1a[p * n + x] = w1;
        kp2a[p * n + x] = w2;
        kp1b[p * n + x] = w3;
        kp2b[p * n + x] = w4;
    }
}
__global__ void fock_reduce_uhf_kernel(double* fa, double* fb, const double* hcore, const double* jpart, const double* kp1a,
                                       const double* kp2a, const double* kp1b, const double* kp2b, int n)
{
    const int64_t n2 = (int64_t)n * n;
    GRID_STRIDE(xa, n2)
    {
        const int x = (int)(xa % n), a = (int)(xa / n);
        double j = 0.0, ka = 0.0, kb = 0.0;
        for (int c = 0; c < FOCK_CHUNKS; ++c) j += jpart[(int64_t)c * n2 + xa];
        for (int b = 0; b <= a; ++b) {
            const int64_t at = ((int64_t)a * (a + 1) / 2 + b) * n + x;
            ka += kp1a[at];
            kb += kp1b[at];
        }
        for (int b = a + 1; b < n; ++b) {
            const int64_t at = ((int64_t)b * (b + 1) / 2 + a) * n + x;
            ka += kp2a[at];
            kb += kp2b[at];
        }
        fa[xa] = hcore[xa] + j - ka;
        fb[xa] = hcore[xa] + j - kb;
    }
}
// UMP2 straight from the three resident blocks of afesp_ao2mo_ump2 (the analogue of mp2_packed_kernel, same last-block reduction):
//   E = 1/4 sum_{ijab in a} [(ia|jb) - (ib|ja)]^2 / D  +  the same in b  +  sum_{ia in a, jb in b} (ia|jb)^2 / D
// aa / bb: 8-fold packed (spatial MO index: occupied first), ab: ab[tri(p,q) np + tri(r,s)] = (pq|rs), pq alpha, rs beta
__global__ __launch_bounds__(TB) void ump2_kernel(double* partial, unsigned* counter, double* scal, const double* __restrict__ aa,
                                                  const double* __restrict__ bb, const double* __restrict__ ab,
                                                  const double* __restrict__ ea, const double* __restrict__ eb, int n, int na, int nb)
{
    __shared__ double sm[4];
    __shared__ bool last;
    const int va = n - na, vb = n - nb;
    const int64_t np = (int64_t)n * (n + 1) / 2;
    const int64_t naa = (int64_t)na * na * va * va, nbb = (int64_t)nb * nb * vb * vb, nab = (int64_t)na * nb * va * vb;
    double acc[1] = {0.0};
    GRID_STRIDE(x, naa + nbb + nab)
    {
        if (x < naa + nbb) {
            const bool beta = x >= naa;
            const int o = beta ? nb : na, v = beta ? vb : va;
            const double* P = beta ? bb : aa;
            const double* e = beta ? eb : ea;
            int64_t r = beta ? x - naa : x;
            const int i = (int)(r % o);
            r /= o;
            const int j = (int)(r % o);
            r /= o;
            const int a = (int)(r % v), b = (int)(r / v);
            const double d = P[tri(tri(o + a, i), tri(o + b, j))] - P[tri(tri(o + b, i), tri(o + a, j))];
            acc[0] += 0.25 * d * d / (e[i] + e[j] - e[o + a] - e[o + b]);
        } else {
            int64_t r = x - naa - nbb;
            const int i = (int)(r % na);
            r /= na;
            const int a = (int)(r % va);
            r /= va;
            const int j = (int)(r % nb), b = (int)(r / nb);
            const double g = ab[tri(na + a, i) * np + tri(nb + b, j)];
            acc[0] += g * g / (ea[i] + eb[j] - ea[na + a] - eb[nb + b]);
        }
    }
    block_sum<1>(acc, sm);
    if (threadIdx.x == 0) {
        partial[blockIdx.x] = acc[0];
        __threadfence();
        last = atomicInc(counter, gridDim.x - 1) == gridDim.x - 1;   // (wraps to zero: ready for the next call)
    }
    __syncthreads();
    if (!last) return;
    __threadfence();
    double tot[1] = {0.0};
    for (int b = threadIdx.x; b < (int)gridDim.x; b += blockDim.x) tot[0] += __builtin_nontemporal_load(&partial[b]);
    block_sum<1>(tot, sm);
    if (threadIdx.x == 0) scal[0] = tot[0];
}
}  // namespace

// E(MP2) of the packed MO integrals on the host; e_dev: the n orbital energies on the device
double k_mp2_packed(Context& cx, const double* eri_packed, const double* e_host, int o, int v)
{
    double seq = 0.0;
    double* pub = host_scalars_slot(cx, &seq);
    unsigned* counter = reinterpret_cast<unsigned*>(cx.scal + 56);   // (zero between launches: atomicInc wraps)
    const int nblk = (int)grid_for((int64_t)o * o * v * v, RED_BLOCKS);
    Mp2Levels lv;
    if (o + v <= 256) {
        for (int q = 0; q < o + v; ++q) lv.e[q] = e_host[q];
        LAUNCH(mp2_packed_kernel<true>, dim3(nblk), partials(cx), counter, cx.scal, pub, seq, eri_packed, (const double*)nullptr, lv, o, v);
    } else {
        double* e_dev = cx.scratch("ao2mo_e", o + v);
        AFESP_HIP(hipMemcpyAsync(e_dev, e_host, sizeof(double) * (o + v), hipMemcpyHostToDevice, cx.stream));
        LAUNCH(mp2_packed_kernel<false>, dim3(nblk), partials(cx), counter, cx.scal, pub, seq, eri_packed, e_dev, lv, o, v);
    }
    return pub ? host_scalars_wait(cx, 1, seq)[0] : host_scalars(cx, 1)[0];
}
void k_mp2_energy(Context& cx, double* out1, const double* v_oovv, const double* D2, int o, int v)
{
    LAUNCH(mp2_energy_kernel, dim3(RED_BLOCKS), partials(cx), v_oovv, D2, o, v);
    k_final_sum(cx, out1, 1, false);
}
// ---- pair-symmetric AO->MO (integrals.hip, ao2mo_mp2): the three layout steps between the quarter transforms
// Both steps have the shape  out(x,y,C) = src(C, tri(x,y)):  a pair index is squared up into the two leading (fastest)
// indices of the result while the other pair index C moves from fastest (in src) to slowest.  A workgroup stages a
// 16 x 16 x 16 tile through LDS so that both the reads (16 consecutive C, or 16 consecutive members of the packed pair)
// and the writes (16 consecutive x) are 128-byte runs; the tile and its mirror image (x and y exchanged) come from one read.
//   MODE 0  unpack_half:     out(i,j,KL) = packed[tri(tri(i,j), KL)]          (ij|kl) with ij squared up, for every pair KL
//   MODE 1  pair_transpose:  out(k,l,PQ) = in(q,p,tri(k,l)), PQ = tri(p,q)    (pq|kl) -> (kl|PQ), kl squared up, p >= q
//   MODE 2  out(k,l,P) = g(P, tri(k,l)), g a plain [np x np] array         the same from the pair-packed half-transformed integrals
// The C blocks [c_begin, c_end) of the result are produced (c_begin a multiple of 16), at out(x,y,C - c_begin): the blocked
// transform of afesp_ao2mo_mp2 works on slabs of C.
// ld >= n: leading dimension of `out` (and of MODE 1's source): the LDS-DMA transforms of a basis size that is no multiple of 16 keep
// their temporaries with columns of ld = 16 ceil(n / 16) doubles, so that every column -- a 128-byte line per K step of the GEMM,
// a 128-byte run of this kernel -- starts on a line (round 6; n = 220: 39.2 -> 36 ms per transform).
template <int MODE>
__global__ __launch_bounds__(256) void pair_square_kernel(double* out, const double* src, int n, int64_t c_begin, int64_t c_end, int ld)
{
    constexpr int T = 16, TP = T + 1, SC = T * TP + 3;   // rows padded: the mirrored tile is read out of LDS along y
    __shared__ double tile[T * SC];
    const int64_t N = n, np = N * (N + 1) / 2, L = ld;
    const int nb = (n + T - 1) / T, nbp = nb * (nb + 1) / 2;
    // a workgroup owns the tile pair (x-block xb >= y-block yb) of one C block: src(C, tri(x,y)) is read once and written
    // to out(x,y,C) and to its mirror image out(y,x,C)
    const int64_t cb = (int64_t)blockIdx.x / nbp;
    int yb, xb;
    unpair((int64_t)blockIdx.x % nbp, yb, xb);
    const int x0 = xb * T, y0 = yb * T;
    const int64_t c0 = c_begin + cb * T;
    // which tile direction is contiguous in src: C (dir 0) or y (dir 1: the whole tile lies in rows C of the packed triangle,
    // where the members x >= y of a pair run along y)
    int dir = 0;
    if (MODE == 0 && tri(min(x0 + T, n) - 1, min(y0 + T, n) - 1) <= c0) dir = 1;
    const int lane = threadIdx.x % T, row = threadIdx.x / T;
    int64_t pq_off = 0;
    if (MODE == 1 && c0 + lane < c_end) {
        int q, p;
        unpair(c0 + lane, q, p);
        pq_off = q + L * p;
    }
#pragma unroll 4
    for (int it = 0; it < T; ++it) {
        const int c = dir == 0 ? lane : row, yi = dir == 0 ? it : lane, xi = dir == 0 ? row : it;
        const int X = x0 + xi, Y = y0 + yi;
        if (X < n && Y < n && c0 + c < c_end)
            tile[c * SC + yi * TP + xi] = MODE == 0 ? src[tri(tri(X, Y), c0 + c)]
                                        : MODE == 1 ? src[pq_off + L * N * tri(X, Y)] : src[(c0 + c) + np * tri(X, Y)];
    }
    __syncthreads();
    const int64_t cr = c0 - c_begin;   // position of the block in the slab
    {
        const int X = x0 + lane, Y = y0 + row;          // out(x,y,C): lanes along x
        if (X < n && Y < n) {
#pragma unroll 4
            for (int c = 0; c < T; ++c)
                if (c0 + c < c_end) out[X + L * Y + L * N * (cr + c)] = tile[c * SC + row * TP + lane];
        }
    }
    if (xb != yb) {
        const int X = y0 + lane, Y = x0 + row;          // the mirror image out(y,x,C): lanes along y
        if (X < n && Y < n) {
#pragma unroll 4
            for (int c = 0; c < T; ++c)
                if (c0 + c < c_end) out[X + L * Y + L * N * (cr + c)] = tile[c * SC + lane * TP + row];
        }
    }
}
// packed[tri(PQ,RS)] = full(s,r,PQ - p_begin) for RS = tri(r,s) <= PQ, PQ in [p_begin, p_end)  (mp2.f90:388-410 on the
// pair-packed result; the whole range in one call, or slab by slab)
__global__ void pack_pairs_kernel(double* packed, const double* full, int n, int64_t p_begin, int64_t p_end, int ld)
{
    const int64_t N = n, np = N * (N + 1) / 2, tot = np * (p_end - p_begin), L = ld;
    GRID_STRIDE(x, tot)
    {
        const int64_t rs = x % np, pq = p_begin + x / np;
        if (rs > pq) continue;
        int s_, r_;
        unpair(rs, s_, r_);
        packed[pq * (pq + 1) / 2 + rs] = full[s_ + L * r_ + L * N * (pq - p_begin)];
    }
}
// cols[PQ np + RS] = full(s,r,PQ) for every RS = tri(r,s) (the full column: afesp_ao2mo_ump2's alpha-beta block)
__global__ void pack_cols_kernel(double* cols, const double* full, int n)
{
    const int64_t N = n, np = N * (N + 1) / 2;
    GRID_STRIDE(x, np * np)
    {
        const int64_t rs = x % np, pq = x / np;
        int s_, r_;
        unpair(rs, s_, r_);
        cols[x] = full[s_ + N * r_ + N * N * pq];
    }
}
// g(PQ, K) = half(q, p, K - k_begin), PQ = tri(p,q) over p >= q, K in [k_begin, k_end): the half-transformed integrals of a slab
// of (kl) pairs, pair-packed in (pq), into the [np x np] array the second pair of transforms gathers from
__global__ void tri_pack_kernel(double* g, const double* half, int n, int64_t k_begin, int64_t k_end)
{
    const int64_t N = n, np = N * (N + 1) / 2, tot = np * (k_end - k_begin);
    GRID_STRIDE(x, tot)
    {
        const int64_t pq = x % np, k = x / np;
        int q, p;
        unpair(pq, q, p);
        g[pq + np * (k_begin + k)] = half[q + N * p + N * N * k];
    }
}
// Active orbital window [lo, lo + n_act) of the packed MO integrals (afesp_mo_window): dst[ijkl(p,q,r,s)] = src[ijkl(p+lo,q+lo,r+lo,s+lo)],
// dst packed over n_act orbitals, src over n.  Shifting all four indices by lo keeps p >= q, r >= s and PQ >= RS, so every element is
// read where it lies: a pure gather, one destination element per thread (contiguous writes; reads are runs along s).  64-bit flat
// indices throughout (neri(220) = 2.96e8, neri(1024) = 1.4e11).
__global__ void window_pack_kernel(double* __restrict__ dst, const double* __restrict__ src, int lo, int64_t total)
{
    GRID_STRIDE(x, total)
    {
        // x = PQ(PQ+1)/2 + RS, RS <= PQ: the same triangular inverse, on 64-bit pair indices
        int64_t rs, pq;
        unpair(x, rs, pq);
        int q, p, s, r;
        unpair(pq, q, p);
        unpair(rs, s, r);
        dst[x] = src[packed_index(p + lo, q + lo, r + lo, s + lo)];
    }
}
// The same for the alpha-beta block of the open-shell path, a full [npair x npair] matrix (afesp_umo_window):
// dst[tri(p,q) np_act + tri(r,s)] = src[tri(p+lo,q+lo) np + tri(r+lo,s+lo)]
__global__ void window_pairs_kernel(double* __restrict__ dst, const double* __restrict__ src, int n_act, int n, int lo)
{
    const int64_t npa = (int64_t)n_act * (n_act + 1) / 2, np = (int64_t)n * (n + 1) / 2;
    GRID_STRIDE(x, npa * npa)
    {
        const int64_t rs = x % npa, pq = x / npa;
        int q, p, s, r;
        unpair(pq, q, p);
        unpair(rs, s, r);
        dst[x] = src[tri(p + lo, q + lo) * np + tri(r + lo, s + lo)];
    }
}
static unsigned pair_square_grid(int n, int64_t c_begin, int64_t c_end)
{
    const int64_t nb = (n + 15) / 16;
    return (unsigned)(nb * (nb + 1) / 2 * ((c_end - c_begin + 15) / 16));
}
void k_unpack_half(Context& cx, double* u, const double* packed, int n, int64_t c_begin, int64_t c_end, int ld)
{
    const int64_t np = (int64_t)n * (n + 1) / 2;
    if (c_end < 0) c_end = np;
    if (c_end > c_begin) LAUNCH(pair_square_kernel<0>, dim3(pair_square_grid(n, c_begin, c_end)), u, packed, n, c_begin, c_end, ld > 0 ? ld : n);
}
// zeroes rows [n, ld) of every column of x(ld, ncol): the padding of the LDS-DMA transforms' temporaries (read as K padding, times zero)
__global__ __launch_bounds__(256) void pad_rows_zero_kernel(double* x, int n, int ld, int64_t ncol)
{
    const int w = ld - n;
    GRID_STRIDE(i, ncol * w) x[(i / w) * ld + n + (i % w)] = 0.0;
}
void k_pad_rows_zero(Context& cx, double* x, int n, int ld, int64_t ncol)
{
    if (ld > n && ncol > 0) LAUNCH(pad_rows_zero_kernel, dim3(grid_for(ncol * (ld - n), 65536)), x, n, ld, ncol);
}
// ---- both quarter transforms of a pair index in ONE kernel, for bases of up to 64 functions (mp2.f90:321-348 resp. :357-385):
//   out(:, :, S) = C in(:, :, S) C^T   for every pair S, in(:, :, S) symmetric
// A workgroup owns one S: the n x n block goes to LDS once (zero-padded to 64 x 64), T1 = C U is formed by the four waves
// (32 x 32 quadrants, 2 x 2 accumulators of v_mfma_f64_16x16x4_f64), written back over U in the layout the second product reads
// its A fragments in, and T2 = T1 C^T leaves through its transpose -- T2 is symmetric -- so that the lanes of a store run along the
// fastest index.  The coefficient fragments come straight from memory (C is 27 KB at n = 58: L1 / L2 resident), all of them
// requested before the first product starts.  No intermediate touches HBM: the two gather-GEMM launches per pair, their K-slice
// reductions and 2 x 8 n^2 npair bytes of traffic become one launch.
constexpr int PX = 64, PXS = 66;   // padded extent, LDS row stride
// MODE 0: in = u(a, b, S) squares (n x n per pair), out = squares            (the transform between the layout kernels)
// MODE 1: in = the 8-fold packed AO integrals, block S gathered through the packed index; out = pair columns g(PQ, S), p >= q
// MODE 2: in = pair columns h(KL, S);  out = the packed MO integrals, run S: packed[S (S + 1) / 2 + RS], RS <= S
// MODE 3: in as MODE 2;  out = the full column of S: out[np S + RS] for every RS (afesp_ao2mo_ump2: (ab|ab) with C of the other
//         spin in the second pair, where the 8-fold symmetry is gone)
// -- with modes 1 and 2 and one transposition of the npair x npair matrix between them the whole AO->MO transform of a small basis
// is three launches and moves 8 (2 neri + 4 npair^2) bytes: no squared-up copy of the integrals exists at any point.
template <int MODE>
__global__ __launch_bounds__(256, 2) void pair_xform_kernel(double* __restrict__ out, const double* __restrict__ in, const double* __restrict__ C,
                                                            int n)
{
    typedef double v4d_t __attribute__((ext_vector_type(4)));
    __shared__ double S[PX * PXS];
    const int64_t nn = (int64_t)n * n, np = (int64_t)n * (n + 1) / 2, blk = blockIdx.x;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, wm = wave >> 1, wn = wave & 1, lm = lane & 15, lk = lane >> 4;
    // coefficient fragments: as A operand of the first product (row p, k = i) and as B operand of the second (column q, k = j)
    double ca[16][2], cb[16][2];
#pragma unroll
    for (int s = 0; s < 16; ++s) {
        const int k = min(4 * s + lk, n - 1);
#pragma unroll
        for (int f = 0; f < 2; ++f) {
            ca[s][f] = C[min(32 * wm + 16 * f + lm, n - 1) + (int64_t)n * k];
            cb[s][f] = C[min(32 * wn + 16 * f + lm, n - 1) + (int64_t)n * k];
        }
    }
    // U into LDS, zero-padded; (a, b) and (b, a) are the same number, so the lanes run along the fastest index on both sides
    // (clamped addresses, the padding zeroed afterwards: a load under a condition would be waited for on its own, sixteen round
    // trips instead of one)
    double ur[PX * PX / 256];
#pragma unroll
    for (int r = 0; r < PX * PX / 256; ++r) {
        const int e = t + 256 * r, a = min(e & 63, n - 1), b = min(e >> 6, n - 1);
        if (MODE == 0) ur[r] = in[nn * blk + a + (int64_t)n * b];
        else if (MODE == 1) ur[r] = in[tri(tri(a, b), blk)];
        else ur[r] = in[np * blk + tri(a, b)];
    }
#pragma unroll
    for (int r = 0; r < PX * PX / 256; ++r) {
        const int e = t + 256 * r, a = e & 63, b = e >> 6;
        S[b * PXS + a] = (a < n && b < n) ? ur[r] : 0.0;
    }
    __syncthreads();
    v4d_t acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = (v4d_t){0.0, 0.0, 0.0, 0.0};
    // T1(p, j) = sum_i C(p, i) U(i, j)
#pragma unroll
    for (int s = 0; s < 16; ++s) {
        double bf[2];
#pragma unroll
        for (int j = 0; j < 2; ++j) bf[j] = S[(4 * s + lk) * PXS + 32 * wn + 16 * j + lm];
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(ca[s][i], bf[j], acc[i][j], 0, 0, 0);
    }
    __syncthreads();   // every wave has read U
    // T1 over U, k-major for the second product's A fragments: S[j][p]  (C/D layout: column = lane & 15, row = (lane >> 4) + 4 r)
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) S[(32 * wn + 16 * j + lm) * PXS + 32 * wm + 16 * i + lk + 4 * r] = acc[i][j][r];
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = (v4d_t){0.0, 0.0, 0.0, 0.0};
    // T2(p, q) = sum_j T1(p, j) C(q, j); the k >= n rows of T1 are zero (U's padding), so the clamped coefficient rows do no harm
#pragma unroll
    for (int s = 0; s < 16; ++s) {
        double af[2];
#pragma unroll
        for (int i = 0; i < 2; ++i) af[i] = S[(4 * s + lk) * PXS + 32 * wm + 16 * i + lm];
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(af[i], cb[s][j], acc[i][j], 0, 0, 0);
    }
    // T2 is symmetric: (row, col) of an accumulator is written as element (col, row) so that the lanes of a store run along the
    // fastest index of the destination -- squares: out(q, p); pair columns / packed runs: the pair (p, q) for q <= p
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int p = 32 * wm + 16 * i + lk + 4 * r;
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int q = 32 * wn + 16 * j + lm;
                if (MODE == 0) {
                    if (p < n && q < n) out[nn * blk + q + (int64_t)n * p] = acc[i][j][r];
                } else if (MODE == 1 || MODE == 3) {
                    if (p < n && q <= p) out[np * blk + (int64_t)p * (p + 1) / 2 + q] = acc[i][j][r];
                } else {
                    const int64_t rs = (int64_t)p * (p + 1) / 2 + q;
                    if (p < n && q <= p && rs <= blk) out[blk * (blk + 1) / 2 + rs] = acc[i][j][r];
                }
            }
        }
}
// out(y, x) = in(x, y), n x n: 32 x 32 tiles through LDS
__global__ __launch_bounds__(256) void square_transpose_kernel(double* __restrict__ out, const double* __restrict__ in, int64_t n)
{
    __shared__ double tile[32][33];
    const int64_t tiles = (n + 31) / 32, bx = blockIdx.x % tiles, by = blockIdx.x / tiles;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int64_t x = bx * 32 + tx, y = by * 32 + ty + 8 * r;
        if (x < n && y < n) tile[ty + 8 * r][tx] = in[x + n * y];
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int64_t y = by * 32 + tx, x = bx * 32 + ty + 8 * r;
        if (x < n && y < n) out[y + n * x] = tile[tx][ty + 8 * r];
    }
}
void k_pair_xform(Context& cx, double* out, const double* in, const double* C, int n, int64_t npairs, int mode)
{
    if (n > PX) throw Error(3, "k_pair_xform: more than 64 basis functions");
    if (npairs <= 0) return;
    if (mode == 0) AFESP_KLAUNCH(pair_xform_kernel<0>, dim3((unsigned)npairs), dim3(256), 0, cx.stream, out, in, C, n);
    else if (mode == 1) AFESP_KLAUNCH(pair_xform_kernel<1>, dim3((unsigned)npairs), dim3(256), 0, cx.stream, out, in, C, n);
    else if (mode == 2) AFESP_KLAUNCH(pair_xform_kernel<2>, dim3((unsigned)npairs), dim3(256), 0, cx.stream, out, in, C, n);
    else AFESP_KLAUNCH(pair_xform_kernel<3>, dim3((unsigned)npairs), dim3(256), 0, cx.stream, out, in, C, n);
    AFESP_HIP(hipGetLastError());
}
void k_square_transpose(Context& cx, double* out, const double* in, int64_t n)
{
    const int64_t tiles = (n + 31) / 32;
    if (n > 0) LAUNCH(square_transpose_kernel, dim3((unsigned)(tiles * tiles)), out, in, n);
}
void k_pair_transpose(Context& cx, double* out, const double* in, int n, int ld)
{
    const int64_t np = (int64_t)n * (n + 1) / 2;
    LAUNCH(pair_square_kernel<1>, dim3(pair_square_grid(n, 0, np)), out, in, n, (int64_t)0, np, ld > 0 ? ld : n);
}
void k_pair_square_packed(Context& cx, double* out, const double* g, int n, int64_t c_begin, int64_t c_end)
{
    if (c_end > c_begin) LAUNCH(pair_square_kernel<2>, dim3(pair_square_grid(n, c_begin, c_end)), out, g, n, c_begin, c_end, n);
}
void k_tri_pack(Context& cx, double* g, const double* half, int n, int64_t k_begin, int64_t k_end)
{
    const int64_t np = (int64_t)n * (n + 1) / 2;
    if (k_end > k_begin) LAUNCH(tri_pack_kernel, dim3(grid_for(np * (k_end - k_begin), 65536)), g, half, n, k_begin, k_end);
}
void k_pack_pairs(Context& cx, double* packed, const double* full, int n, int64_t p_begin, int64_t p_end, int ld)
{
    const int64_t np = (int64_t)n * (n + 1) / 2;
    if (p_end < 0) p_end = np;
    if (p_end > p_begin) LAUNCH(pack_pairs_kernel, dim3(grid_for(np * (p_end - p_begin), 65536)), packed, full, n, p_begin, p_end, ld > 0 ? ld : n);
}
void k_pack_cols(Context& cx, double* cols, const double* full, int n)
{
    const int64_t np = (int64_t)n * (n + 1) / 2;
    LAUNCH(pack_cols_kernel, dim3(grid_for(np * np, 65536)), cols, full, n);
}
void k_window_pack(Context& cx, double* dst, const double* src, int n_act, int lo)
{
    const int64_t npa = (int64_t)n_act * (n_act + 1) / 2, total = npa * (npa + 1) / 2;
    if (total > 0) LAUNCH(window_pack_kernel, dim3(grid_for(total, 65536)), dst, src, lo, total);
}
void k_window_pairs(Context& cx, double* dst, const double* src, int n_act, int n, int lo)
{
    const int64_t npa = (int64_t)n_act * (n_act + 1) / 2;
    if (npa > 0) LAUNCH(window_pairs_kernel, dim3(grid_for(npa * npa, 65536)), dst, src, n_act, n, lo);
}
// ---- the tables and the padded coefficient transpose of the LDS-DMA quarter transforms (the extern "C" kernels above)
void k_ao2mo_ct(Context& cx, double* ct, const double* c, int n, int Kc) { LAUNCH(ao2mo_ct_kernel, dim3((unsigned)(((int64_t)n * Kc + 255) / 256)), ct, c, n, Kc); }
void k_ao2mo_tables(Context& cx, uint32_t* rowA, uint32_t* colB, int64_t* offCm, int64_t* offCn, int n, int Kc, int64_t ncol, int64_t ld)
{
    LAUNCH(ao2mo_tables_kernel, dim3((unsigned)std::min<int64_t>((ncol + 256 + 255) / 256, 65536)), rowA, colB, offCm, offCn, n, Kc, ncol, ld);
}
void k_ao2mo_tables_tri(Context& cx, uint32_t* colB, int64_t* offCn, const int64_t* cstart, int n, int64_t np, int64_t sl, int64_t ld)
{
    LAUNCH(ao2mo_tables_tri_kernel, dim3((unsigned)std::min<int64_t>(np, 65536)), colB, offCn, cstart, n, np, sl, ld);
}
void k_ao2mo_tables_lo(Context& cx, uint32_t* colB, int64_t* offCn, int n, int cnt, int64_t ncol, int64_t ld)
{
    LAUNCH(ao2mo_tables_lo_kernel, dim3((unsigned)std::min<int64_t>((ncol + 256 + 255) / 256, 65536)), colB, offCn, n, cnt, ncol, ld);
}
// ---- MP1 amplitude operands of the virtual-virtual MP2 density (afesp_mp2_vv_density / afesp_ump2_vv_density)
// One destination element per thread, x = j + o (i + o (c + v a)): the contraction index (j,i,c) of D = T~^T T runs fastest in the
// operand (contiguous writes, both operands K-contiguous for the GEMM), and j fastest of all, because (ia|jc) lies at
// tri(tri(A,I), tri(C,J)) in the 8-fold packed array -- for PQ >= RS a run along j (window_pack_kernel's argument; the exchange partner
// (ic|ja) and the PQ < RS half are gathers).  Orbitals: I = nfc + i, A = nfc + o + a.  64-bit flat indices (o^2 v^2 = 3.2e7 at n = 220,
// 8.5e9 at o = 100, v = 924).  Tt != nullptr (closed shell): T = t(i,j,a,c) = (ia|jc) / D, Tt = 2 t(i,j,a,c) - t(i,j,c,a), the block's
// share of sum (ia|jc) Tt = E(MP2); Tt == nullptr (one spin of an open shell): T = [(ia|jc) - (ic|ja)] / D, share of 1/4 sum d T.
// Fixed grid of RED_BLOCKS blocks, per-block partials, ordered final sum (k_final_sum): deterministic.
__global__ __launch_bounds__(TB) void fno_amps_kernel(double* partial, double* __restrict__ T, double* __restrict__ Tt,
                                                      const double* __restrict__ packed, const double* __restrict__ e, int nfc, int o, int v)
{
    __shared__ double sm[4];
    const int64_t total = (int64_t)o * o * v * v;
    const int no = nfc + o;
    double acc[1] = {0.0};
    GRID_STRIDE(x, total)
    {
        const int j = (int)(x % o);
        int64_t r = x / o;
        const int i = (int)(r % o);
        r /= o;
        const int c = (int)(r % v), a = (int)(r / v);
        const int64_t I = nfc + i, J = nfc + j, A = no + a, Cc = no + c;
        const double g = packed[packed_index(A, I, Cc, J)], gx = packed[packed_index(Cc, I, A, J)];
        const double den = e[I] + e[J] - e[A] - e[Cc];
        if (Tt) {
            const double t = g / den, tt = 2.0 * t - gx / den;
            T[x] = t;
            Tt[x] = tt;
            acc[0] += g * tt;
        } else {
            const double d = g - gx, t = d / den;
            T[x] = t;
            acc[0] += 0.25 * d * t;
        }
    }
    block_sum<1>(acc, sm);
    if (threadIdx.x == 0) partial[blockIdx.x] = acc[0];
}
// The opposite-spin amplitudes t(i,J,a,B) = (ia|JB) / D out of the alpha-beta block ab[tri(A,I) np + tri(B,J)] (alpha pair: row).  J runs
// fastest on both sides -- tri(B,J) is a run along J in the block's fastest index --
//   BETA_COLS = false: x = J + ob (B + vb (i + oa a)), rows (J,B,i) of column a: the operand of D alpha
//   BETA_COLS = true:  x = J + ob (i + oa (a + va B)), rows (J,i,a) of column B: the operand of D beta
// and the block's share of sum (ia|JB) t, the opposite-spin part of E(UMP2).
template <bool BETA_COLS>
__global__ __launch_bounds__(TB) void fno_amps_ab_kernel(double* partial, double* __restrict__ T, const double* __restrict__ ab,
                                                         const double* __restrict__ ea, const double* __restrict__ eb, int n, int nfc, int oa,
                                                         int ob, int va, int vb)
{
    __shared__ double sm[4];
    const int64_t total = (int64_t)oa * ob * va * vb, np = (int64_t)n * (n + 1) / 2;
    const int na = nfc + oa, nb = nfc + ob;
    double acc[1] = {0.0};
    GRID_STRIDE(x, total)
    {
        const int j = (int)(x % ob);
        int64_t r = x / ob;
        int i, a, b;
        if (BETA_COLS) {
            i = (int)(r % oa);
            r /= oa;
            a = (int)(r % va);
            b = (int)(r / va);
        } else {
            b = (int)(r % vb);
            r /= vb;
            i = (int)(r % oa);
            a = (int)(r / oa);
        }
        const int64_t I = nfc + i, J = nfc + j, A = na + a, B = nb + b;
        const double g = ab[tri(A, I) * np + tri(B, J)];
        const double t = g / (ea[I] + eb[J] - ea[A] - eb[B]);
        T[x] = t;
        acc[0] += g * t;
    }
    block_sum<1>(acc, sm);
    if (threadIdx.x == 0) partial[blockIdx.x] = acc[0];
}
void k_fno_amps(Context& cx, double* T, double* Tt, const double* packed, const double* e_dev, int nfc, int o, int v, int slot)
{
    LAUNCH(fno_amps_kernel, dim3(RED_BLOCKS), partials(cx), T, Tt, packed, e_dev, nfc, o, v);
    k_final_sum(cx, cx.scal + slot, 1, false);
}
void k_fno_amps_ab(Context& cx, double* T, const double* ab, const double* ea_dev, const double* eb_dev, int n, int nfc, int oa, int ob, int va,
                   int vb, bool beta_cols, int slot)
{
    if (beta_cols) LAUNCH(fno_amps_ab_kernel<true>, dim3(RED_BLOCKS), partials(cx), T, ab, ea_dev, eb_dev, n, nfc, oa, ob, va, vb);
    else LAUNCH(fno_amps_ab_kernel<false>, dim3(RED_BLOCKS), partials(cx), T, ab, ea_dev, eb_dev, n, nfc, oa, ob, va, vb);
    k_final_sum(cx, cx.scal + slot, 1, false);
}
// ---- the field of the frozen core on the active window (afesp_core_operator / afesp_ucore_operator)
// One wave per active pair (p >= q), P = nfc + p, Q = nfc + q: h_act(p,q) = h_mo(P,Q) + sum_c [wj (PQ|cc) - (Pc|Qc)] over the nfc frozen
// orbitals -- lane l takes c = l, l + 64, ... in rising order and the 64 partial sums are added in wave_sum's fixed order, so the result
// does not depend on the launch -- written to both triangles from one register (symmetric to the bit; h_mo enters as the mean of its two
// triangles, which the GEMMs leave equal only to rounding).  The wave after the last pair forms the core energy
// e_core = eh sum_c h_mo(c,c) + e2 sum_cd [wj (cc|dd) - (cd|cd)].  Closed shell: wj = 2, eh = 2, e2 = 1; one spin of an open shell:
// wj = 1, eh = 1, e2 = 1/2.  64-bit flat indices (packed_index).
__global__ __launch_bounds__(TB) void core_fold_kernel(double* __restrict__ h_act, double* __restrict__ e_core, const double* __restrict__ hmo,
                                                       const double* __restrict__ packed, int n, int nfc, int n_act, double wj, double eh,
                                                       double e2)
{
    const int lane = threadIdx.x & 63;
    const int64_t npa = (int64_t)n_act * (n_act + 1) / 2, w = (int64_t)blockIdx.x * (TB / 64) + (threadIdx.x >> 6);
    if (w > npa) return;   // (whole waves leave)
    double acc = 0.0;
    if (w < npa) {
        int q, p;
        unpair(w, q, p);
        const int64_t P = p + nfc, Q = q + nfc;
        for (int64_t c = lane; c < nfc; c += 64) acc += wj * packed[packed_index(P, Q, c, c)] - packed[packed_index(P, c, Q, c)];
        acc = wave_sum(acc);
        if (lane == 0) {
            const double val = 0.5 * (hmo[P + (int64_t)n * Q] + hmo[Q + (int64_t)n * P]) + acc;
            h_act[p + (int64_t)n_act * q] = val;
            h_act[q + (int64_t)n_act * p] = val;
        }
    } else {
        double one = 0.0;
        for (int64_t x = lane; x < (int64_t)nfc * nfc; x += 64) {
            const int64_t c = x % nfc, d = x / nfc;
            acc += wj * packed[packed_index(c, c, d, d)] - packed[packed_index(c, d, c, d)];
        }
        for (int64_t c = lane; c < nfc; c += 64) one += hmo[c + (int64_t)n * c];
        acc = wave_sum(acc);
        one = wave_sum(one);
        if (lane == 0) *e_core = eh * one + e2 * acc;
    }
}
// The opposite-spin share out of the alpha-beta block ab[tri(p,q) np + tri(r,s)] (alpha pair: row), added to what core_fold_kernel wrote:
// h_a(p,q) += sum_C (PQ|CC), h_b(p,q) += sum_c (cc|PQ); the last wave: e_core = sum_cD (cc|DD).
__global__ __launch_bounds__(TB) void core_fold_ab_kernel(double* __restrict__ h_a, double* __restrict__ h_b, double* __restrict__ e_core,
                                                          const double* __restrict__ ab, int n, int nfc, int n_act)
{
    const int lane = threadIdx.x & 63;
    const int64_t npa = (int64_t)n_act * (n_act + 1) / 2, np = (int64_t)n * (n + 1) / 2;
    const int64_t w = (int64_t)blockIdx.x * (TB / 64) + (threadIdx.x >> 6);
    if (w > npa) return;
    if (w < npa) {
        int q, p;
        unpair(w, q, p);
        const int64_t PQ = tri(p + nfc, q + nfc);
        double fa = 0.0, fb = 0.0;
        for (int64_t c = lane; c < nfc; c += 64) {
            fa += ab[PQ * np + tri(c, c)];
            fb += ab[tri(c, c) * np + PQ];
        }
        fa = wave_sum(fa);
        fb = wave_sum(fb);
        if (lane == 0) {
            const int64_t lo = p + (int64_t)n_act * q, up = q + (int64_t)n_act * p;
            const double va = h_a[lo] + fa, vb = h_b[lo] + fb;
            h_a[lo] = va; h_a[up] = va;
            h_b[lo] = vb; h_b[up] = vb;
        }
    } else {
        double acc = 0.0;
        for (int64_t x = lane; x < (int64_t)nfc * nfc; x += 64) acc += ab[tri(x % nfc, x % nfc) * np + tri(x / nfc, x / nfc)];
        acc = wave_sum(acc);
        if (lane == 0) *e_core = acc;
    }
}
void k_core_fold(Context& cx, double* h_act, double* e_core, const double* hmo, const double* packed, int n, int nfc, int n_act, bool one_spin)
{
    const int64_t waves = (int64_t)n_act * (n_act + 1) / 2 + 1;
    LAUNCH(core_fold_kernel, dim3((unsigned)((waves + TB / 64 - 1) / (TB / 64))), h_act, e_core, hmo, packed, n, nfc, n_act,
           one_spin ? 1.0 : 2.0, one_spin ? 1.0 : 2.0, one_spin ? 0.5 : 1.0);
}
void k_core_fold_ab(Context& cx, double* h_a, double* h_b, double* e_core, const double* ab, int n, int nfc, int n_act)
{
    const int64_t waves = (int64_t)n_act * (n_act + 1) / 2 + 1;
    LAUNCH(core_fold_ab_kernel, dim3((unsigned)((waves + TB / 64 - 1) / (TB / 64))), h_a, h_b, e_core, ab, n, nfc, n_act);
}

// ---- the FCIDUMP reader (afesp_read_fcidump / _uhf): records -> slots, and the Fock operator of the file's determinant
// One record per lane: canonicalise (packed_index / tri do), route, act.  Targets and the bit of the visited map (one bit per slot):
//   closed shell: packed [0, ne) | h, bit ne + tri(i,j) | core energy
//   open shell:   aa [0, ne) | bb | ab, row = alpha pair, the (bb|aa) form transposed | h_a | h_b | core energy
// (odd spin-orbital numbers are alpha, spatial orbital (x + 1) / 2 - 1).  The host has checked every record (fcidump_parse.h: classify);
// a record that fails here nevertheless is counted as an error and never dereferenced.
namespace {
struct FcSlot {
    double *a, *mirror;
    int64_t bit;
};
__device__ __forceinline__ bool fc_route(const FcidumpTargets& T, const fcidump::Record& r, FcSlot& s)
{
    const int64_t norb = T.uhf ? 2 * T.n : T.n;
    const int64_t i = r.idx[0], j = r.idx[1], k = r.idx[2], l = r.idx[3];
    s.mirror = nullptr;
    if (i < 0 || j < 0 || k < 0 || l < 0 || i > norb || j > norb || k > norb || l > norb) return false;
    if (i == 0 || j == 0) {
        if (i | j | k | l) return false;
        s.a = T.ecore;
        s.bit = T.nslots - 1;
        return true;
    }
    if ((k == 0) != (l == 0)) return false;
    if (!T.uhf) {
        if (k == 0) {
            s.a = T.h[0] + (i - 1) + T.n * (j - 1);
            s.mirror = T.h[0] + (j - 1) + T.n * (i - 1);
            s.bit = T.ne + tri(i - 1, j - 1);
        } else {
            s.bit = packed_index(i - 1, j - 1, k - 1, l - 1);
            s.a = T.eri[0] + s.bit;
        }
        return true;
    }
    const int64_t p = (i + 1) / 2 - 1, q = (j + 1) / 2 - 1;
    const int b1 = !(i & 1);
    if (((i ^ j) & 1) || ((k ^ l) & 1)) return false;
    if (k == 0) {
        s.a = T.h[b1] + p + T.n * q;
        s.mirror = T.h[b1] + q + T.n * p;
        s.bit = 2 * T.ne + T.np * T.np + b1 * T.np + tri(p, q);
        return true;
    }
    const int64_t t = (k + 1) / 2 - 1, u = (l + 1) / 2 - 1;
    const int b2 = !(k & 1);
    if (b1 == b2) {
        const int64_t x = packed_index(p, q, t, u);
        s.a = T.eri[b1] + x;
        s.bit = b1 * T.ne + x;
    } else {
        const int64_t x = b1 ? tri(t, u) * T.np + tri(p, q) : tri(p, q) * T.np + tri(t, u);
        s.a = T.eri[2] + x;
        s.bit = 2 * T.ne + x;
    }
    return true;
}
__device__ __forceinline__ void fc_flag(const FcidumpTargets& T, int64_t line)
{
    atomicAdd(T.err, 1ull);
    atomicMin(T.err + 1, (unsigned long long)line);
}
// PASS 0: a record whose slot an EARLIER chunk visited compares its bits with the resident value.  PASS 1: store, mark visited.
// PASS 2: every record reads its slot back (a one-electron record both triangles): of two records of this chunk that disagree, at
// least one finds the other's bits in a location it stored to.
template <int PASS>
__global__ __launch_bounds__(TB) void fcidump_scatter_kernel(FcidumpTargets T, const fcidump::Record* __restrict__ rec, int64_t count)
{
    GRID_STRIDE(x, count)
    {
        const fcidump::Record r = rec[x];
        FcSlot s;
        if (!fc_route(T, r, s) || s.bit < 0 || s.bit >= T.nslots) {
            if (PASS == 0) fc_flag(T, r.line);
            continue;
        }
        uint32_t* word = T.visited + (s.bit >> 5);
        const uint32_t mask = 1u << (s.bit & 31);
        if (PASS == 0) {
            if ((*word & mask) && (__double_as_longlong(*s.a) != __double_as_longlong(r.value) ||
                                   (s.mirror && __double_as_longlong(*s.mirror) != __double_as_longlong(r.value))))
                fc_flag(T, r.line);
        } else if (PASS == 1) {
            *s.a = r.value;
            if (s.mirror) *s.mirror = r.value;
            atomicOr(word, mask);
        } else {   // (a one-electron record stored both triangles: both are read back, whichever order the stores landed in)
            if (__double_as_longlong(*s.a) != __double_as_longlong(r.value) ||
                (s.mirror && __double_as_longlong(*s.mirror) != __double_as_longlong(r.value)))
                fc_flag(T, r.line);
        }
    }
}
// The Fock operator of the determinant that fills the first nocc orbitals, over ALL n orbitals (the all-orbital analogue of
// core_fold_kernel): one wave per pair p >= q, F(p,q) = h(p,q) + sum_{i < nocc} [wj (pq|ii) - (pi|qi)] -- lane l takes i = l, l + 64, ...
// in rising order, wave_sum adds the 64 partial sums in its fixed order, both triangles are written from one register.  wj = 2 closed
// shell, 1 for one spin of an open shell.
__global__ __launch_bounds__(TB) void fock_mo_kernel(double* __restrict__ F, const double* __restrict__ h, const double* __restrict__ packed, int n,
                                                     int nocc, double wj)
{
    const int lane = threadIdx.x & 63;
    const int64_t np = (int64_t)n * (n + 1) / 2, w = (int64_t)blockIdx.x * (TB / 64) + (threadIdx.x >> 6);
    if (w >= np) return;   // (whole waves leave)
    int q, p;
    unpair(w, q, p);
    double acc = 0.0;
    for (int64_t i = lane; i < nocc; i += 64) acc += wj * packed[packed_index(p, q, i, i)] - packed[packed_index(p, i, q, i)];
    acc = wave_sum(acc);
    if (lane == 0) {
        const double val = h[p + (int64_t)n * q] + acc;
        F[p + (int64_t)n * q] = val;
        F[q + (int64_t)n * p] = val;
    }
}
// ... and the opposite-spin Coulomb terms out of ab[tri(p,q) np + tri(r,s)] (alpha pair: row), added to what fock_mo_kernel wrote:
// F_a(p,q) += sum_{I < nb} (pq|II), F_b(p,q) += sum_{i < na} (ii|pq)
__global__ __launch_bounds__(TB) void fock_mo_ab_kernel(double* __restrict__ fa, double* __restrict__ fb, const double* __restrict__ ab, int n,
                                                        int na, int nb)
{
    const int lane = threadIdx.x & 63;
    const int64_t np = (int64_t)n * (n + 1) / 2, w = (int64_t)blockIdx.x * (TB / 64) + (threadIdx.x >> 6);
    if (w >= np) return;
    int q, p;
    unpair(w, q, p);
    double ja = 0.0, jb = 0.0;
    for (int64_t i = lane; i < nb; i += 64) ja += ab[w * np + tri(i, i)];
    for (int64_t i = lane; i < na; i += 64) jb += ab[tri(i, i) * np + w];
    ja = wave_sum(ja);
    jb = wave_sum(jb);
    if (lane == 0) {
        const int64_t lo = p + (int64_t)n * q, up = q + (int64_t)n * p;
        const double va = fa[lo] + ja, vb = fb[lo] + jb;
        fa[lo] = va; fa[up] = va;
        fb[lo] = vb; fb[up] = vb;
    }
}
}  // namespace
void k_fcidump_scatter(Context& cx, const FcidumpTargets& T, const fcidump::Record* rec, int64_t count)
{
    if (count <= 0) return;
    const dim3 grid(grid_for(count, 65536));
    LAUNCH(fcidump_scatter_kernel<0>, grid, T, rec, count);
    LAUNCH(fcidump_scatter_kernel<1>, grid, T, rec, count);
    LAUNCH(fcidump_scatter_kernel<2>, grid, T, rec, count);
}
void k_fock_mo(Context& cx, double* F, const double* h, const double* packed, int n, int nocc, double wj)
{
    const int64_t waves = (int64_t)n * (n + 1) / 2;
    LAUNCH(fock_mo_kernel, dim3((unsigned)((waves + TB / 64 - 1) / (TB / 64))), F, h, packed, n, nocc, wj);
}
void k_fock_mo_ab(Context& cx, double* fa, double* fb, const double* ab, int n, int na, int nb)
{
    const int64_t waves = (int64_t)n * (n + 1) / 2;
    LAUNCH(fock_mo_ab_kernel, dim3((unsigned)((waves + TB / 64 - 1) / (TB / 64))), fa, fb, ab, n, na, nb);
}
void k_fock_ro(Context& cx, double* fa, double* fb, const double* h, const double* packed, int n, int na, int nb)
{
    const int64_t waves = (int64_t)n * (n + 1) / 2;
    LAUNCH(fock_ro_kernel, dim3((unsigned)((waves + 3) / 4)), fa, fb, h, packed, n, na, nb);
}

// ---- order-preserving stream compaction of an integral array (afesp_write_fcidump_active / _uactive): the elements with
// |x| > thr as (flat index, value) pairs in rising index order, so that only they cross to the host.  A wave owns a run of
// COMPACT_CHUNK = 64 x 32 consecutive elements (chunk c = [c CHUNK, (c + 1) CHUNK): the owner of a chunk depends on its number alone,
// not on the grid) and walks it 64 elements at a time -- one coalesced 512-byte load per step.
//   count:   counts[c] = sum over the steps of popcount(ballot(|x| > thr))
//   scan:    counts -> exclusive prefix sums in place, counts[nchunks] = number of survivors (one workgroup: 1.4e5 chunks at n = 220)
//   scatter: the same walk; a survivor's slot = prefix[c] + survivors of the earlier steps + lanes below it in this step's ballot (mbcnt)
// A threshold of 0 keeps everything except exact zeros (and NaNs, which no comparison keeps).
constexpr int COMPACT_ITEMS = 32;
constexpr int64_t COMPACT_CHUNK = 64 * COMPACT_ITEMS;
__global__ __launch_bounds__(TB) void compact_count_kernel(int64_t* __restrict__ counts, const double* __restrict__ x, int64_t total,
                                                           int64_t nchunks, double thr)
{
    const int lane = threadIdx.x & 63;
    for (int64_t c = (int64_t)blockIdx.x * (TB / 64) + (threadIdx.x >> 6); c < nchunks; c += (int64_t)gridDim.x * (TB / 64)) {
        const int64_t base = c * COMPACT_CHUNK;
        int64_t cnt = 0;
#pragma unroll 4
        for (int it = 0; it < COMPACT_ITEMS; ++it) {
            const int64_t i = base + 64 * it + lane;
            const bool keep = i < total && fabs(x[i]) > thr;
            cnt += __popcll(__ballot(keep));
        }
        if (lane == 0) counts[c] = cnt;
    }
}
__global__ __launch_bounds__(TB) void compact_scan_kernel(int64_t* counts, int64_t nchunks)
{
    __shared__ int64_t part[TB];
    const int64_t seg = (nchunks + TB - 1) / TB;   // thread t scans chunks [t seg, (t + 1) seg)
    const int64_t lo = seg * threadIdx.x < nchunks ? seg * threadIdx.x : nchunks, hi = lo + seg < nchunks ? lo + seg : nchunks;
    int64_t s = 0;
    for (int64_t i = lo; i < hi; ++i) s += counts[i];
    part[threadIdx.x] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        int64_t run = 0;
        for (int t = 0; t < TB; ++t) {
            const int64_t v = part[t];
            part[t] = run;
            run += v;
        }
        counts[nchunks] = run;
    }
    __syncthreads();
    int64_t run = part[threadIdx.x];
    for (int64_t i = lo; i < hi; ++i) {
        const int64_t v = counts[i];
        counts[i] = run;
        run += v;
    }
}
__global__ __launch_bounds__(TB) void compact_scatter_kernel(int64_t* __restrict__ out_idx, double* __restrict__ out_val,
                                                             const int64_t* __restrict__ prefix, const double* __restrict__ x, int64_t total,
                                                             int64_t nchunks, double thr)
{
    const int lane = threadIdx.x & 63;
    for (int64_t c = (int64_t)blockIdx.x * (TB / 64) + (threadIdx.x >> 6); c < nchunks; c += (int64_t)gridDim.x * (TB / 64)) {
        const int64_t base = c * COMPACT_CHUNK;
        int64_t off = prefix[c];
        if (prefix[c + 1] == off) continue;   // (nothing survives in this chunk: wave-uniform)
#pragma unroll 4
        for (int it = 0; it < COMPACT_ITEMS; ++it) {
            const int64_t i = base + 64 * it + lane;
            const double v = i < total ? x[i] : 0.0;
            const bool keep = i < total && fabs(v) > thr;
            const unsigned long long m = __ballot(keep);
            const int below = __builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
            if (keep) {
                out_idx[off + below] = i;
                out_val[off + below] = v;
            }
            off += __popcll(m);
        }
    }
}
int64_t k_compact_chunks(int64_t total) { return (total + COMPACT_CHUNK - 1) / COMPACT_CHUNK; }
void k_compact_count(Context& cx, int64_t* counts, const double* x, int64_t total, double thr)
{
    const int64_t nchunks = k_compact_chunks(total);
    if (nchunks > 0) LAUNCH(compact_count_kernel, dim3(grid_for(nchunks * 64, 65536)), counts, x, total, nchunks, thr);
    LAUNCH(compact_scan_kernel, dim3(1), counts, nchunks);
}
void k_compact_scatter(Context& cx, int64_t* out_idx, double* out_val, const int64_t* prefix, const double* x, int64_t total, double thr)
{
    const int64_t nchunks = k_compact_chunks(total);
    if (nchunks > 0) LAUNCH(compact_scatter_kernel, dim3(grid_for(nchunks * 64, 65536)), out_idx, out_val, prefix, x, total, nchunks, thr);
}

void k_build_fock(Context& cx, double* fock, const double* hcore, const double* dens, const double* u, double* work, int n, int ld)
{
    if (ld <= 0) ld = n;
    // work: [ dv (npair) | jpart (FOCK_CHUNKS n^2) | kp1 (npair n) | kp2 (npair n) ]
    const int64_t n2 = (int64_t)n * n, np = (int64_t)n * (n + 1) / 2;
    double *dv = work, *jpart = dv + np, *kp1 = jpart + FOCK_CHUNKS * n2, *kp2 = kp1 + np * n;
    LAUNCH(fock_dv_kernel, dim3(grid_for(np)), dv, dens, n);
    LAUNCH(fock_j_kernel, dim3((unsigned)((n2 + 255) / 256), FOCK_CHUNKS), jpart, u, dv, n, ld);
    AFESP_KLAUNCH(fock_k_kernel, dim3((unsigned)np), dim3(256), 2 * n * sizeof(double), cx.stream, kp1, kp2, u, dens, n, ld);
    AFESP_HIP(hipGetLastError());
    LAUNCH(fock_reduce_kernel, dim3(grid_for(n2)), fock, hcore, jpart, kp1, kp2, n);
}
void k_build_fock_uhf(Context& cx, double* fa, double* fb, const double* hcore, const double* da, const double* db, const double* u,
                      double* work, int n, int ld)
{
    if (ld <= 0) ld = n;
    // work: [ dv (npair) | jpart (FOCK_CHUNKS n^2) | kp1a, kp2a, kp1b, kp2b (npair n each) ]
    const int64_t n2 = (int64_t)n * n, np = (int64_t)n * (n + 1) / 2;
    double *dv = work, *jpart = dv + np, *kp = jpart + FOCK_CHUNKS * n2;
    LAUNCH(fock_dv_uhf_kernel, dim3(grid_for(np)), dv, da, db, n);
    LAUNCH(fock_j_kernel, dim3((unsigned)((n2 + 255) / 256), FOCK_CHUNKS), jpart, u, dv, n, ld);
    AFESP_KLAUNCH(fock_k_uhf_kernel, dim3((unsigned)np), dim3(256), 4 * n * sizeof(double), cx.stream, kp, kp + np * n, kp + 2 * np * n,
                  kp + 3 * np * n, u, da, db, n, ld);
    AFESP_HIP(hipGetLastError());
    LAUNCH(fock_reduce_uhf_kernel, dim3(grid_for(n2)), fa, fb, hcore, jpart, kp, kp + np * n, kp + 2 * np * n, kp + 3 * np * n, n);
}
int64_t k_build_fock_uhf_work(int n)
{
    const int64_t n2 = (int64_t)n * n, np = (int64_t)n * (n + 1) / 2;
    return np + FOCK_CHUNKS * n2 + 4 * np * n;
}
double k_ump2(Context& cx, const double* aa, const double* bb, const double* ab, const double* ea_dev, const double* eb_dev, int n, int na,
              int nb)
{
    unsigned* counter = reinterpret_cast<unsigned*>(cx.scal + 56);   // (shared with mp2_packed_kernel: zero between launches)
    const int64_t va = n - na, vb = n - nb;
    const int64_t tot = (int64_t)na * na * va * va + (int64_t)nb * nb * vb * vb + (int64_t)na * nb * va * vb;
    if (tot == 0) return 0.0;
    const int nblk = (int)grid_for(tot, RED_BLOCKS);
    LAUNCH(ump2_kernel, dim3(nblk), partials(cx), counter, cx.scal, aa, bb, ab, ea_dev, eb_dev, n, na, nb);
    return host_scalars(cx, 1)[0];
}
int64_t k_build_fock_work(int n)
{
    const int64_t n2 = (int64_t)n * n, np = (int64_t)n * (n + 1) / 2;
    return np + FOCK_CHUNKS * n2 + 2 * np * n;
}

// per-kernel first-use resolution (first_use.h) of what a small system's AO->MO transform and MP2 launch, of the open-shell set-up
// (afesp_build_fock_uhf, afesp_ao2mo_ump2) and of the restricted open-shell Fock operators
void preload_integrals()
{
    const void* fns[] = {reinterpret_cast<const void*>(mp2_energy_kernel), reinterpret_cast<const void*>(mp2_packed_kernel<true>),
                         reinterpret_cast<const void*>(pair_xform_kernel<1>), reinterpret_cast<const void*>(pair_xform_kernel<2>),
                         reinterpret_cast<const void*>(square_transpose_kernel), reinterpret_cast<const void*>(fock_dv_uhf_kernel),
                         reinterpret_cast<const void*>(fock_k_uhf_kernel), reinterpret_cast<const void*>(fock_reduce_uhf_kernel),
                         reinterpret_cast<const void*>(ump2_kernel), reinterpret_cast<const void*>(pair_xform_kernel<3>),
                         reinterpret_cast<const void*>(pack_cols_kernel), reinterpret_cast<const void*>(fock_ro_kernel)};
    for (const void* f : fns) first_use_touch(f);   // (each under the process-wide first-use lock, first_use.h)
    (void)hipGetLastError();
}

}  // namespace afesp
