// integrals.hip -- the integral layer (integrals.h), host side: the resident AO / MO integrals and their validity records, the Fock builds,
// the AO->MO transform in its forms (pair kernels, gather GEMM, LDS-DMA GEMM, slab-blocked), the orbital windows, the frozen-core operator,
// the text reader and the FCIDUMP reader and writers.  No device code: the layer's kernels are integrals_kernels.hip's.
#include <cmath>
#include <cstdlib>
#include <cstring>

#include "fcidump_format.h"
#include "fcidump_parse.h"
#include "integrals.h"
#include "integrals_kernels.h"
#include "solver.h"
#include "tgemm.h"

using namespace afesp;

namespace {
struct Ao2moTg {
    int64_t n = 0, Kc = 0, sl = 0;   // basis size, padded summation length, (S) pairs per slab (one TgGroup each)
    int64_t ld = 0;                  // leading dimension of the temporaries: Kc (ao2mo_ld), or n
    double* ct = nullptr;
    uint32_t *rowA = nullptr, *colB = nullptr;
    int64_t *offCm = nullptr, *offCn = nullptr;
    TgGroup* groups = nullptr;       // room for the descriptors of every transform of one call (no host synchronisation between them)
    int64_t groups_cap = 0, groups_used = 0;
    std::vector<std::vector<TgGroup>> host;   // ... whose host copies live until the call's final synchronisation
    // columns (r, PQ), r <= p(PQ) only (ao2mo_tables_tri_kernel)
    uint32_t* colB_tri = nullptr;
    int64_t* offCn_tri = nullptr;
    std::vector<int64_t> cstart;     // [np + 1], host copy
    int64_t p_split = 0;             // first pair PQ with p >= TG_BM (the pairs below it need the first 128 rows only)
    uint32_t* colB_lo = nullptr;     // columns x2 < TG_BM (ao2mo_tables_lo_kernel)
    int64_t* offCn_lo = nullptr;
};

// tables and the padded transpose of the coefficient matrix for basis size n (cached scratch: rebuilt per call, microseconds)
static Ao2moTg ao2mo_tg_prepare(Context& cx, const double* Cm, int64_t n, int64_t np, int64_t ld)
{
    Ao2moTg t;
    t.n = n;
    t.ld = ld;
    t.Kc = (n + 15) / 16 * 16;
    // a slab's columns are addressed with 32-bit byte offsets: n * sl columns of n doubles each below 4 GiB
    t.sl = std::min<int64_t>(np, std::min<int64_t>(8192, (((int64_t)1 << 32) - 4096) / (8 * t.ld * n)));
    const int64_t ncol = n * t.sl;
    t.ct = cx.scratch("ao2mo_ct", n * t.Kc);
    t.rowA = (uint32_t*)cx.scratch("ao2mo_t32", (n + 256 + ncol + 256) / 2 + 2);
    t.colB = t.rowA + n + 256;
    t.offCm = (int64_t*)cx.scratch("ao2mo_t64", n + 128 + ncol + 128 + 2);
    t.offCn = t.offCm + n + 128;
    k_ao2mo_ct(cx, t.ct, Cm, (int)n, (int)t.Kc);
    k_ao2mo_tables(cx, t.rowA, t.colB, t.offCm, t.offCn, (int)n, (int)t.Kc, ncol, t.ld);
    const int64_t ng = (np + t.sl - 1) / t.sl;
    t.groups_cap = 8 * (ng + 2);
    t.groups = (TgGroup*)cx.scratch("ao2mo_tg", (int64_t)(t.groups_cap * sizeof(TgGroup) / sizeof(double) + 1));
    // the triangular column list of the last transform
    t.cstart.assign((size_t)np + 1, 0);
    for (int64_t pp = 0, P = 0; pp < n; ++pp)
        for (int64_t q = 0; q <= pp; ++q, ++P) t.cstart[(size_t)P + 1] = t.cstart[(size_t)P] + ((pp + 2) & ~(int64_t)1);
    t.p_split = std::min<int64_t>(np, (int64_t)TG_BM * (TG_BM + 1) / 2);
    const int64_t ctot = t.cstart[(size_t)np];
    t.colB_tri = (uint32_t*)cx.scratch("ao2mo_t32t", (ctot + 256) / 2 + 2);
    t.offCn_tri = (int64_t*)cx.scratch("ao2mo_t64t", ctot + 128 + 2);
    int64_t* cs_dev = (int64_t*)cx.scratch("ao2mo_cs", np + 2);
    AFESP_HIP(hipMemcpyAsync(cs_dev, t.cstart.data(), (size_t)(np + 1) * sizeof(int64_t), hipMemcpyHostToDevice, cx.stream));
    AFESP_HIP(hipMemsetAsync(t.colB_tri + ctot, 0, 256 * sizeof(uint32_t), cx.stream));
    AFESP_HIP(hipMemsetAsync(t.offCn_tri + ctot, 0, 128 * sizeof(int64_t), cx.stream));
    k_ao2mo_tables_tri(cx, t.colB_tri, t.offCn_tri, cs_dev, (int)n, np, t.sl, t.ld);
    if (n > TG_BM) {
        const int64_t nlo = (int64_t)TG_BM * t.sl;
        t.colB_lo = (uint32_t*)cx.scratch("ao2mo_t32h", (nlo + 256) / 2 + 2);
        t.offCn_lo = (int64_t*)cx.scratch("ao2mo_t64h", nlo + 128 + 2);
        k_ao2mo_tables_lo(cx, t.colB_lo, t.offCn_lo, (int)n, (int)TG_BM, nlo, t.ld);
    }
    return t;
}

// one quarter transform over the pairs S in [s_begin, s_end) of `in` (n x n x np), rows row0 <= m < row0 + M of the result only;
// cols: 0 every column (x2, S), 1 only x2 <= p(S), 2 only x2 < 128 (the rest of `out` is left untouched)
static void ao2mo_tg_xform(Context& cx, Ao2moTg& t, const double* in, double* out, int64_t s_begin, int64_t s_end, int64_t M, int cols,
                    int64_t row0 = 0)
{
    if (s_end <= s_begin || M <= 0) return;
    const bool tri = cols == 1, lo = cols == 2;
    const int64_t nlo = TG_BM;
    const int64_t n = t.n, g_lo = s_begin / t.sl, g_hi = (s_end - 1) / t.sl;
    const int mt = (int)((M + TG_BM - 1) / TG_BM);
    t.host.emplace_back();
    std::vector<TgGroup>& hv = t.host.back();
    int mx = 0, tile = 0;
    auto ncols = [&](int64_t s0, int64_t s1) { return tri ? t.cstart[(size_t)s1] - t.cstart[(size_t)s0] : (lo ? nlo : n) * (s1 - s0); };
    for (int64_t g = g_lo; g <= g_hi; ++g) {
        const int64_t s0 = std::max(s_begin, g * t.sl), s1 = std::min(s_end, (g + 1) * t.sl);
        mx = std::max(mx, (int)((ncols(s0, s1) + TG_BN - 1) / TG_BN));
    }
    const int gm = tgemm_group_m((int)M, mx);
    for (int64_t g = g_lo; g <= g_hi; ++g) {
        const int64_t s0 = std::max(s_begin, g * t.sl), s1 = std::min(s_end, (g + 1) * t.sl);
        TgGroup d{};
        d.a1 = d.a2 = 0;
        d.b1 = d.b2 = t.ld * n * g * t.sl;       // (the tables are relative to the slab's first pair; columns are ld doubles long)
        d.c0 = t.ld * n * g * t.sl;
        d.colB = tri ? t.colB_tri + t.cstart[(size_t)s0] : lo ? t.colB_lo + nlo * (s0 - g * t.sl) : t.colB + n * (s0 - g * t.sl);
        d.offCn = tri ? t.offCn_tri + t.cstart[(size_t)s0] : lo ? t.offCn_lo + nlo * (s0 - g * t.sl) : t.offCn + n * (s0 - g * t.sl);
        d.N = (int)ncols(s0, s1);
        d.ntiles = (d.N + TG_BN - 1) / TG_BN;
        d.tile_start = tile;
        d.nk1 = d.nk = (int)(t.Kc / TG_BK);
        d.inv_width = tgemm_inverse(gm * d.ntiles);
        if ((int64_t)mt * d.ntiles * gm * d.ntiles >= ((int64_t)1 << 32)) throw Error(2, "ao2mo: tile walk out of range");
        tile += mt * d.ntiles;
        hv.push_back(d);
    }
    TgGroup end{};
    end.tile_start = tile;
    hv.push_back(end);
    const int ng = (int)hv.size() - 1;
    if (t.groups_used + (int64_t)hv.size() > t.groups_cap) throw Error(2, "ao2mo: descriptor buffer too small");
    TgGroup* dev = t.groups + t.groups_used;
    t.groups_used += (int64_t)hv.size();
    AFESP_HIP(hipMemcpyAsync(dev, hv.data(), hv.size() * sizeof(TgGroup), hipMemcpyHostToDevice, cx.stream));
    TgProblem p{t.ct, in, out, t.rowA + row0, t.offCm + row0, (int)M, true, (int)((n - (t.Kc - TG_BK) + 3) / 4)};
    p.tag = 2;
    // (rows that end at most 96 past a multiple of 128 -- n = 220: 92 -- take a 96-row last tile: three quarters of its MFMAs, tgemm.h)
    const int bm = (knobs().ao2mo_mixed && M % TG_BM != 0 && M % TG_BM <= 96) ? TG_BM : 0;
    AFESP_HIP(tgemm_launch(p, dev, ng, tile, mx, cx.stream, cx.tg, bm));
}
// MP2 energy on the <ij|ab> slice of packed MO integrals over o + v orbitals (mp2.f90:418-440); levels: their o + v orbital energies (host)
double mp2_of_packed(Context& cx, const double* packed, const double* levels, int64_t o, int64_t v)
{
    const int64_t n = o + v;
    // small systems: one launch, straight from the packed array (the slice and the denominators are formed on the fly)
    // (AFESP_MP2_PACKED=0: the five-launch form at every size, A/B runs)
    if (o * o * v * v <= ((int64_t)1 << 22) && knobs().mp2_packed) return k_mp2_packed(cx, packed, levels, (int)o, (int)v);
    double* e_dev = cx.scratch("ao2mo_e", n);
    AFESP_HIP(hipMemcpyAsync(e_dev, levels, sizeof(double) * n, hipMemcpyHostToDevice, cx.stream));
    Tensor voovv = view(cx.scratch("ao2mo_v", o * o * v * v), {o, o, v, v}), D1 = view(cx.scratch("ao2mo_d1", o * v), {o, v}),
           D2 = view(cx.scratch("ao2mo_d2", o * o * v * v), {o, o, v, v});
    k_slice_phys(cx, voovv.d, packed, (int)o, (int)o, (int)v, (int)v, 0, 0, (int)o, (int)o);
    k_denominators(cx, D1.d, D2.d, e_dev, (int)o, (int)v);
    k_mp2_energy(cx, cx.scal, voovv.d, D2.d, (int)o, (int)v);
    return host_scalars(cx, 1)[0];
}

// ---- the steps of a transform (src/mp2.f90:261-449), each written once.  Four quarter transforms as MFMA GEMMs; each pass contracts the
// leading AO index with C(MO,AO) and the planner writes the result with the new MO index in place: (ij|K) in a -> (pq|K) in a, by way of b
void first_pair(Context& cx, const Tensor& C, const Tensor& a, const Tensor& b)
{
    contract(cx, 1.0, C, "pi", a, "ijK", 0.0, b, "pjK");   // mp2.f90:321-333
    contract(cx, 1.0, C, "qj", b, "pjK", 0.0, a, "pqK");   // mp2.f90:338-348
}
// gather-GEMM, second pair: (kl|P) in `in` -> (rs|P) in `out`, by way of tmp
void second_pair(Context& cx, const Tensor& C, const Tensor& in, const Tensor& tmp, const Tensor& out)
{
    contract(cx, 1.0, C, "rk", in, "klP", 0.0, tmp, "rlP");    // mp2.f90:357-367
    contract(cx, 1.0, C, "sl", tmp, "rlP", 0.0, out, "rsP");   // mp2.f90:375-385
}
// pair kernels (both quarter transforms of a pair index in one kernel with the n x n block resident in LDS), first pair: straight from the
// packed AO integrals to pair columns, one transposition -- g(K, PQ) in a (a / b hold the two npair^2 matrices, no squared-up copy)
void pair_half(Context& cx, const double* ao, const Tensor& C, const Tensor& a, const Tensor& b)
{
    const int64_t n = C.dim[0], np = npair_of(n);
    k_pair_xform(cx, b.d, ao, C.d, (int)n, np, 1);   // (ij|K) -> g(PQ, K)       mp2.f90:321-348
    k_square_transpose(cx, a.d, b.d, np);            // g(K, PQ)
}

// Small bases: the whole tensor at once.  The two temporaries are cached scratch: a second transform in the same context reuses them,
// the next afesp_ccsd_init / afesp_ccsd_so_init gives them back.
void transform_dense(Context& cx, Integrals& in, const Ao2moForm& form, double* packed, const double* ao, const Tensor& Cm, bool have_u)
{
    const int64_t n = Cm.dim[0], np = npair_of(n), L = form.ld;
    Tensor Ta = view(cx.scratch("ao2mo_a", Integrals::temp_size(n, L)), {n, n, np}),
           Tb = view(cx.scratch("ao2mo_b", Integrals::temp_size(n, L)), {n, n, np});
    if (!have_u && !form.pair) k_unpack_half(cx, Ta.d, ao, (int)n, 0, -1, (int)L);   // (ij|KL), ij squared up
    in.half_overwritten();
    if (form.use_tg) {
        AFESP_HIP(hipMemsetAsync(Ta.d + L * n * np, 0, 16 * sizeof(double), cx.stream));
        AFESP_HIP(hipMemsetAsync(Tb.d + L * n * np, 0, 16 * sizeof(double), cx.stream));
        in.zero_padding(cx, Ta.d, Tb.d, n, L);
        Ao2moTg tg = ao2mo_tg_prepare(cx, Cm.d, n, np, L);
        ao2mo_tg_xform(cx, tg, Ta.d, Tb.d, 0, np, n, 0);         // (ij|K) -> (j p|K)        mp2.f90:321-333
        // (jp|K) -> (x2 m|K), mp2.f90:338-348: the transposition below reads x2 <= m only -- the rows m < 128 are computed
        // for the columns x2 < 128 only
        if (n > TG_BM) {
            ao2mo_tg_xform(cx, tg, Tb.d, Ta.d, 0, np, n - TG_BM, 0, TG_BM);
            ao2mo_tg_xform(cx, tg, Tb.d, Ta.d, 0, np, TG_BM, 2);
        } else {
            ao2mo_tg_xform(cx, tg, Tb.d, Ta.d, 0, np, n, 0);
        }
        k_pair_transpose(cx, Tb.d, Ta.d, (int)n, (int)L);       // (kl|PQ), kl squared up, p >= q
        // Second pair: only (rs|PQ) with RS <= PQ is packed (mp2.f90:388-410), i.e. r <= p and s <= r.  Rows beyond the
        // first 128 are therefore skipped for the pairs with p < 128, and the last transform runs over the columns
        // (r, PQ) with r <= p only -- 2.6 n^5 flop in 128-row tiles instead of 4 (the reference: 8).
        const int64_t ps = tg.p_split, m_lo = std::min<int64_t>(n, TG_BM);
        ao2mo_tg_xform(cx, tg, Tb.d, Ta.d, 0, ps, m_lo, 0);      // (kl|P) -> (l r|P)        mp2.f90:357-367
        ao2mo_tg_xform(cx, tg, Tb.d, Ta.d, ps, np, n, 0);
        ao2mo_tg_xform(cx, tg, Ta.d, Tb.d, 0, ps, m_lo, 1);      // (lr|P) -> (r s|P)        mp2.f90:375-385
        ao2mo_tg_xform(cx, tg, Ta.d, Tb.d, ps, np, n, 1);
        k_pack_pairs(cx, packed, Tb.d, (int)n, 0, -1, (int)L);   // mp2.f90:388-410
        cx.sync();                                               // (the descriptors' host copies die with tg)
        return;
    }
    in.padding_overwritten();
    if (form.pair) {   // every bundled input, the H2O/cc-pVTZ shape: three launches
        pair_half(cx, ao, Cm, Ta, Tb);
        k_pair_xform(cx, packed, Ta.d, Cm.d, (int)n, np, 2);   // (kl|P) -> (rs|P), RS <= P  mp2.f90:357-410
    } else {
        first_pair(cx, Cm, Ta, Tb);
        k_pair_transpose(cx, Tb.d, Ta.d, (int)n);   // (kl|PQ), kl squared up, p >= q
        second_pair(cx, Cm, Tb, Ta, Tb);
        k_pack_pairs(cx, packed, Tb.d, (int)n);     // mp2.f90:388-410
    }
}

// Large bases: slab by slab.  The first pair of transforms acts on every (kl) pair separately and the second on every (pq) pair, so only
// the half-transformed integrals have to exist as a whole -- pair-packed, g(PQ,K), np^2 doubles (4.7 GB at n = 220) -- and the n^2 npair
// temporaries (2 x 9.4 GB) shrink to two slabs of S pairs.  S is chosen so that a slab's column tiles fill whole rounds of the persistent
// GEMM grid.  From temporaries of 16 GiB each (n >= 256): at n = 220 this form is 5 % slower (58.9 against 55.8 ms: one more pass over
// the half-transformed integrals) for 12.5 GB less -- it is there for the sizes where 2 n^2 npair doubles no longer fit beside the rest
// (n = 400: 2 x 103 GB)
void transform_blocked(Context& cx, Integrals& in, double* packed, const double* ao, const Tensor& Cm, bool have_u)
{
    const int64_t n = Cm.dim[0], np = npair_of(n);
    in.padding_overwritten();
    int64_t S = std::max<int64_t>(16, ((int64_t)256 * 128 * 14 / n) / 16 * 16);
    if (S > np) S = (np + 15) / 16 * 16;
    double* g = cx.scratch("ao2mo_g", np * np);
    double* sa = have_u ? nullptr : cx.scratch("ao2mo_a", n * n * S);   // (with (ij|KL) left by the Fock build: its slabs, in place)
    double* sb = cx.scratch("ao2mo_b", n * n * S);
    double* u = have_u ? cx.scratch("ao2mo_a", n * n * np) : nullptr;
    in.half_overwritten();
    for (int64_t k0 = 0; k0 < np; k0 += S) {
        const int64_t k1 = std::min(np, k0 + S), len = k1 - k0;
        double* a_s = have_u ? u + n * n * k0 : sa;
        if (!have_u) k_unpack_half(cx, a_s, ao, (int)n, k0, k1);   // (ij|K), ij squared up, K in the slab
        first_pair(cx, Cm, view(a_s, {n, n, len}), view(sb, {n, n, len}));
        k_tri_pack(cx, g, a_s, (int)n, k0, k1);                    // g(PQ,K), p >= q
    }
    if (have_u) sa = u;   // (dead now: its first slab serves the second pair)
    for (int64_t p0 = 0; p0 < np; p0 += S) {
        const int64_t p1 = std::min(np, p0 + S), len = p1 - p0;
        k_pair_square_packed(cx, sb, g, (int)n, p0, p1);           // (kl|P), kl squared up, P in the slab
        Tensor Ta = view(sa, {n, n, len}), Tb = view(sb, {n, n, len});
        second_pair(cx, Cm, Tb, Ta, Tb);
        k_pack_pairs(cx, packed, sb, (int)n, p0, p1);              // mp2.f90:388-410
    }
}

// read_integrals_in, two-body part (src/integrals.f90:146-161): lines "i j a b value", 1-based, any blank separation, in
// any order; a later line for the same packed slot overwrites an earlier one; slots never mentioned stay 0.
int64_t parse_eri_text(FILE* f, int64_t nbasis, std::vector<double>& host)
{
    std::vector<char> buf((size_t)(8 << 20) + 1);
    size_t keep = 0;
    int64_t lines = 0;
    auto tri = [](int64_t i, int64_t j) { return i >= j ? i * (i + 1) / 2 + j : j * (j + 1) / 2 + i; };
    for (;;) {
        const size_t got = fread(buf.data() + keep, 1, buf.size() - 1 - keep, f);
        const size_t have = keep + got;
        if (have == 0) break;
        buf[have] = 0;
        // parse whole lines only; the tail (an incomplete line) is carried into the next block
        size_t end = have;
        if (got > 0) {
            while (end > 0 && buf[end - 1] != '\n') --end;
            if (end == 0 && have == buf.size() - 1) return -1;   // a "line" longer than the buffer
        }
        const size_t stop = got > 0 ? end : have;
        char* p = buf.data();
        char* const lim = buf.data() + stop;
        const char saved = *lim;
        *lim = 0;
        while (p < lim) {
            while (p < lim && (*p == ' ' || *p == '\t' || *p == '\r' || *p == '\n')) ++p;
            if (p >= lim) break;
            // list-directed input (src/integrals.f90:150 `read (ir, *) i, j, a, b, val`): fields are separated by blanks
            // and/or one comma, a real may carry a Fortran D exponent ("1.0D-05"); whatever follows the fifth field on
            // the record is ignored, as the reference's read does
            auto sep = [&](char*& c) {
                while (c < lim && (*c == ' ' || *c == '\t' || *c == '\r')) ++c;
                if (c < lim && *c == ',') ++c;
                while (c < lim && (*c == ' ' || *c == '\t' || *c == '\r')) ++c;
            };
            char* q;
            long idx[4];
            bool ok = true;
            for (int k = 0; k < 4 && ok; ++k) {
                if (*p == '\n') { ok = false; break; }
                idx[k] = strtol(p, &q, 10);
                ok = (q != p) && (q >= lim || *q == ' ' || *q == '\t' || *q == ',' || *q == '\r') && idx[k] >= 1 && idx[k] <= nbasis;
                p = q;
                if (ok) sep(p);
            }
            if (!ok || *p == '\n') return -1;
            char tok[64];
            size_t len = 0;
            while (p + len < lim && len < sizeof(tok) - 1 && p[len] != ' ' && p[len] != '\t' && p[len] != ',' && p[len] != '\r' &&
                   p[len] != '\n') {
                const char ch = p[len];
                tok[len] = (ch == 'D' || ch == 'd') ? 'E' : ch;
                ++len;
            }
            tok[len] = 0;
            char* tq = nullptr;
            const double val = strtod(tok, &tq);
            if (len == 0 || tq != tok + len) return -1;   // the whole token is the number
            p += len;
            host[(size_t)tri(tri(idx[0] - 1, idx[1] - 1), tri(idx[2] - 1, idx[3] - 1))] = val;
            ++lines;
            while (p < lim && *p != '\n') ++p;   // ignore anything else on the line
        }
        *lim = saved;
        if (got == 0) break;
        keep = have - stop;
        memmove(buf.data(), buf.data() + stop, keep);
    }
    return lines;
}

}  // namespace

namespace afesp {

Ao2moForm::Ao2moForm(int64_t n, bool open_shell)
{
    const Knobs& k = knobs();
    blocked = k.ao2mo_blocked >= 0 ? k.ao2mo_blocked == 1 : n * n * npair_of(n) >= ((int64_t)1 << 31);
    use_tg = !open_shell && !blocked && n % 2 == 0 && n >= 16 && (k.ao2mo_tg >= 0 ? k.ao2mo_tg == 1 : n >= 96);
    pair = !blocked && !use_tg && n <= 64 && (open_shell || k.ao2mo_pair);
    ld = use_tg && k.ao2mo_pad ? (n + 15) / 16 * 16 : n;
}

double* Integrals::adopt_ao(Context& cx, int64_t n)
{
    if (ao) cx.release(ao);
    ao = nullptr;
    half_n = 0;
    ao = cx.alloc(neri_of(n));
    ao_n = n;
    return ao;
}

void Integrals::upload_ao(Context& cx, int64_t n, const double* host)
{
    AFESP_HIP(hipMemcpyAsync(adopt_ao(cx, n), host, sizeof(double) * neri_of(n), hipMemcpyHostToDevice, cx.stream));
    cx.sync();
}

const double* Integrals::half_unpacked(Context& cx, int64_t n, int64_t& ld)
{
    ld = Ao2moForm(n).ld;
    double* u = cx.scratch("ao2mo_a", temp_size(n, ld));
    if (!half_valid(cx, n, ld)) {
        if (pad_n != n || pad_ld != ld) pad_n = 0;   // (another layout lands in the buffer the transforms share)
        k_unpack_half(cx, u, ao, (int)n, 0, -1, (int)ld);
        half_n = n; half_ld = ld; half_epoch = cx.scratch_epoch;
    }
    return u;
}

// (rows n .. ld - 1 of every column are K padding of the products -- read, times the zero padding of C: finite, so zero.  No kernel of
// the LDS-DMA form or of the Fock builds writes them, so they are zeroed once per (buffers, n, ld): 0.2 ms each)
void Integrals::zero_padding(Context& cx, double* a, double* b, int64_t n, int64_t ld)
{
    if (pad_a == a && pad_b == b && pad_n == n && pad_ld == ld && pad_epoch == cx.scratch_epoch) return;
    k_pad_rows_zero(cx, a, (int)n, (int)ld, n * npair_of(n));
    k_pad_rows_zero(cx, b, (int)n, (int)ld, n * npair_of(n));
    pad_a = a; pad_b = b; pad_n = n; pad_ld = ld; pad_epoch = cx.scratch_epoch;
}

void Integrals::release_uhf(Context& cx)
{
    cx.release(uhf_aa); cx.release(uhf_bb); cx.release(uhf_ab);
    uhf_aa = uhf_bb = uhf_ab = nullptr;
    uhf_n = 0;
}

void Integrals::adopt_uhf(Context& cx, int64_t n)
{
    if (uhf_n == n && uhf_aa) return;
    release_uhf(cx);
    uhf_aa = cx.alloc_raw(neri_of(n));
    uhf_bb = cx.alloc_raw(neri_of(n));
    uhf_ab = cx.alloc_raw(npair_of(n) * npair_of(n));
    uhf_n = n;
}

// the orbitals [lo, lo + n_act) of the three blocks: block by block, each full block back to the arena before the next window is asked for
void Integrals::window_uhf(Context& cx, int64_t n_act, int64_t lo)
{
    const int64_t n = uhf_n, nea = neri_of(n_act), npa = npair_of(n_act);
    for (double** blk : {&uhf_aa, &uhf_bb, &uhf_ab}) {
        double* w = cx.alloc_raw(blk == &uhf_ab ? npa * npa : nea);
        if (blk == &uhf_ab) k_window_pairs(cx, w, uhf_ab, (int)n_act, (int)n, (int)lo);
        else k_window_pack(cx, w, *blk, (int)n_act, (int)lo);
        cx.release(*blk);
        *blk = w;
        uhf_n = 0;   // (from here on the blocks are of mixed extents until all three are done)
    }
    uhf_n = n_act;
}

void Integrals::swap_uhf(Context& cx, double* aa, double* bb, double* ab, int64_t n)
{
    release_uhf(cx);
    uhf_aa = aa; uhf_bb = bb; uhf_ab = ab;
    uhf_n = n;
}

void Integrals::drop_mo(Context& cx, Solver& sv)
{
    sv.eri_gone(mo);
    if (mo) cx.release(mo);
    set_mo(nullptr, 0);
}

double* Integrals::replace_mo(Context& cx, Solver& sv, int64_t n)
{
    if (mo && mo_n == n) {   // a transform of the same basis size overwrites the previous result
        sv.eri_gone(mo);
        return mo;
    }
    drop_mo(cx, sv);
    return cx.alloc_raw(neri_of(n));
}

// build_fock (src/hf.f90:349-385) on the resident packed AO integrals
void build_fock(Context& cx, Integrals& in, int64_t n, const double* density, const double* hcore, double* fock)
{
    const int64_t n2 = n * n;
    double* buf = cx.scratch("fock_io", 3 * n2);
    AFESP_HIP(hipMemcpyAsync(buf, density, sizeof(double) * n2, hipMemcpyHostToDevice, cx.stream));
    AFESP_HIP(hipMemcpyAsync(buf + n2, hcore, sizeof(double) * n2, hipMemcpyHostToDevice, cx.stream));
    int64_t L = 0;
    const double* u = in.half_unpacked(cx, n, L);
    double* work = cx.scratch("fock_work", k_build_fock_work((int)n));
    in.half_restamp(cx);
    k_build_fock(cx, buf + 2 * n2, buf + n2, buf, u, work, (int)n, (int)L);
    AFESP_HIP(hipMemcpyAsync(fock, buf + 2 * n2, sizeof(double) * n2, hipMemcpyDeviceToHost, cx.stream));
    cx.sync();
}

void build_fock_uhf(Context& cx, Integrals& in, int64_t n, const double* dens_a, const double* dens_b, const double* hcore, double* fock_a,
                    double* fock_b)
{
    const int64_t n2 = n * n;
    double* buf = cx.scratch("fock_uio", 5 * n2);   // [ Da | Db | H | Fa | Fb ]
    AFESP_HIP(hipMemcpyAsync(buf, dens_a, sizeof(double) * n2, hipMemcpyHostToDevice, cx.stream));
    AFESP_HIP(hipMemcpyAsync(buf + n2, dens_b, sizeof(double) * n2, hipMemcpyHostToDevice, cx.stream));
    AFESP_HIP(hipMemcpyAsync(buf + 2 * n2, hcore, sizeof(double) * n2, hipMemcpyHostToDevice, cx.stream));
    // the half-unpacked integrals build_fock keeps (same buffer, same validity)
    int64_t L = 0;
    const double* u = in.half_unpacked(cx, n, L);
    double* work = cx.scratch("fock_uwork", k_build_fock_uhf_work((int)n));
    in.half_restamp(cx);
    k_build_fock_uhf(cx, buf + 3 * n2, buf + 4 * n2, buf + 2 * n2, buf, buf + n2, u, work, (int)n, (int)L);
    AFESP_HIP(hipMemcpyAsync(fock_a, buf + 3 * n2, sizeof(double) * n2, hipMemcpyDeviceToHost, cx.stream));
    AFESP_HIP(hipMemcpyAsync(fock_b, buf + 4 * n2, sizeof(double) * n2, hipMemcpyDeviceToHost, cx.stream));
    cx.sync();
}

double ao2mo_mp2(Context& cx, Integrals& in, Solver& sv, int64_t n, int64_t o, const double* coeff, const double* levels,
                 const double* eri_packed, double* eri_mo_packed)
{
    const int64_t ne = neri_of(n);
    if (!eri_packed && (!in.ao || in.ao_n != n))
        throw Error(1, "afesp_ao2mo_mp2: eri_packed is NULL and no AO integrals were read onto the device for this basis size");
    cx.drop_scratch("t_");   // the (T) pool of a previous system holds the blocks the two temporaries below were
    in.release_uhf(cx);      // an RHF transform ends the open-shell calculation: its integral blocks go back to the arena
    double* packed = in.replace_mo(cx, sv, n);
    const double* ao = in.ao;   // NULL source: transformed where afesp_read_eri_text / afesp_set_eri left them
    if (eri_packed) {           // upload buffer, then the packed MO integrals
        AFESP_HIP(hipMemcpyAsync(packed, eri_packed, sizeof(double) * ne, hipMemcpyHostToDevice, cx.stream));
        ao = packed;
    }
    Tensor Cm = view(cx.scratch("ao2mo_c", n * n), {n, n});
    AFESP_HIP(hipMemcpyAsync(Cm.d, coeff, sizeof(double) * n * n, hipMemcpyHostToDevice, cx.stream));
    // Pair symmetry: (ij|kl) is transformed for the n(n+1)/2 pairs k >= l only, the half-transformed (pq|kl) kept for
    // p >= q only -- 4 n^5 flop and two buffers of n^2 x npair instead of 8 n^5 and two of n^4.
    const Ao2moForm form(n);
    const bool have_u = ao == in.ao && in.half_valid(cx, n, form.ld);   // a Fock build left (ij|KL)
    if (form.blocked) transform_blocked(cx, in, packed, ao, Cm, have_u);
    else transform_dense(cx, in, form, packed, ao, Cm, have_u);
    in.set_mo(packed, n);
    const double emp2 = mp2_of_packed(cx, packed, levels, o, n - o);
    if (eri_mo_packed) {
        AFESP_HIP(hipMemcpyAsync(eri_mo_packed, packed, sizeof(double) * ne, hipMemcpyDeviceToHost, cx.stream));
        cx.sync();
    }
    return emp2;
}

// (aa|aa), (bb|bb) and (aa|bb) from one set of AO integrals: the first pair of quarter transforms with C_a is shared by the first and
// the third block, the second pair runs with C_a (packed, RS <= PQ) and with C_b (every RS: no 8-fold symmetry is left), then the whole
// transform once more with C_b.
// The launches of that transform, for whichever packed source `src` (the AO integrals: afesp_ao2mo_ump2; the resident MO integrals:
// afesp_mo_rotate_uhf) and coefficient pair on the host; the three blocks are the resident ones
static void uhf_blocks_from_packed(Context& cx, Integrals& in, const Ao2moForm& form, int64_t n, const double* src, const double* coeff_a,
                                   const double* coeff_b)
{
    const int64_t np = npair_of(n);
    double *aa = in.uhf_aa, *bb = in.uhf_bb, *ab = in.uhf_ab;
    const double* ao = src;
    Tensor Ca = view(cx.scratch("ao2mo_c", n * n), {n, n}), Cb = view(cx.scratch("ao2mo_cb", n * n), {n, n});
    AFESP_HIP(hipMemcpyAsync(Ca.d, coeff_a, sizeof(double) * n * n, hipMemcpyHostToDevice, cx.stream));
    AFESP_HIP(hipMemcpyAsync(Cb.d, coeff_b, sizeof(double) * n * n, hipMemcpyHostToDevice, cx.stream));
    // the temporaries are the RHF transform's (dense columns of n): whatever the Fock build or an LDS-DMA transform left there is gone
    in.half_overwritten();
    in.padding_overwritten();
    Tensor Ta = view(cx.scratch("ao2mo_a", Integrals::temp_size(n, form.ld)), {n, n, np}),
           Tb = view(cx.scratch("ao2mo_b", Integrals::temp_size(n, form.ld)), {n, n, np});
    if (form.pair) {
        pair_half(cx, ao, Ca, Ta, Tb);                          // g(K, PQ), C_a
        k_pair_xform(cx, aa, Ta.d, Ca.d, (int)n, np, 2);        // (rs|PQ), RS <= PQ, C_a
        k_pair_xform(cx, ab, Ta.d, Cb.d, (int)n, np, 3);        // (rs|PQ), every RS, C_b
        pair_half(cx, ao, Cb, Ta, Tb);                          // and the beta-beta block
        k_pair_xform(cx, bb, Ta.d, Cb.d, (int)n, np, 2);
    } else {
        Tensor Tc = view(cx.scratch("ao2mo_c3", n * n * np), {n, n, np});
        k_unpack_half(cx, Ta.d, ao, (int)n);
        first_pair(cx, Ca, Ta, Tb);
        k_pair_transpose(cx, Tb.d, Ta.d, (int)n);                // (kl|PQ), alpha PQ
        second_pair(cx, Ca, Tb, Ta, Tc);
        k_pack_pairs(cx, aa, Tc.d, (int)n);
        second_pair(cx, Cb, Tb, Ta, Tc);
        k_pack_cols(cx, ab, Tc.d, (int)n);
        k_unpack_half(cx, Ta.d, ao, (int)n);
        first_pair(cx, Cb, Ta, Tb);
        k_pair_transpose(cx, Tb.d, Ta.d, (int)n);
        second_pair(cx, Cb, Tb, Ta, Tc);
        k_pack_pairs(cx, bb, Tc.d, (int)n);
    }
}
// device memory of that transform: the temporaries (two npair^2 for the pair form, three n^2 npair for the gather-GEMM form) and, for a
// new basis size, the three result blocks, against what the device has free plus what the context's arena holds idle
static void uhf_blocks_fit(Context& cx, Integrals& in, const Ao2moForm& form, int64_t n, const char* who)
{
    const int64_t ne = neri_of(n), np = npair_of(n);
    const double tmp = form.pair ? 2.0 * np * np : 3.0 * n * n * np;
    const double blocks = (in.uhf_n == n && in.uhf_aa) ? 0.0 : 2.0 * ne + (double)np * np;
    if (in.uhf_n != n) in.release_uhf(cx);   // (blocks of another basis size: returned before their successors are sized)
    if (!cx.fits(8.0 * (tmp + blocks + 4.0 * n * n)))
        throw Error(1, std::string(who) + ": the open-shell transform of this basis does not fit the free device memory");
}

double ao2mo_ump2(Context& cx, Integrals& in, int64_t n, int64_t na, int64_t nb, const double* coeff_a, const double* coeff_b,
                  const double* levels_a, const double* levels_b, const double* eri_packed, double* eri_aa, double* eri_ab, double* eri_bb)
{
    const Ao2moForm form(n, true);
    if (form.blocked)
        throw Error(1, "afesp_ao2mo_ump2: basis too large (only the slab-blocked transform fits, and it has no open-shell form)");
    if (!eri_packed && (!in.ao || in.ao_n != n))
        throw Error(1, "afesp_ao2mo_ump2: eri_packed is NULL and no AO integrals were read onto the device for this basis size");
    cx.drop_scratch("t_");
    cx.drop_scratch("ao2mo_");   // (the temporaries are sized below; what they held goes back to the arena)
    const int64_t ne = neri_of(n);
    uhf_blocks_fit(cx, in, form, n, "afesp_ao2mo_ump2");
    in.adopt_uhf(cx, n);
    const double* ao = in.ao;
    if (eri_packed) {   // (into the beta-beta block: every read of the AO integrals precedes its one write)
        AFESP_HIP(hipMemcpyAsync(in.uhf_bb, eri_packed, sizeof(double) * ne, hipMemcpyHostToDevice, cx.stream));
        ao = in.uhf_bb;
    }
    uhf_blocks_from_packed(cx, in, form, n, ao, coeff_a, coeff_b);
    return ump2_of_blocks(cx, in, levels_a, levels_b, na, nb, eri_aa, eri_ab, eri_bb);
}

// E(UMP2) of the three resident blocks (levels on the host, for their basis size) and the blocks themselves for whoever asks
double ump2_of_blocks(Context& cx, const Integrals& in, const double* levels_a, const double* levels_b, int64_t oa, int64_t ob, double* eri_aa,
                      double* eri_ab, double* eri_bb)
{
    const int64_t n = in.uhf_n, ne = neri_of(n), np = npair_of(n);
    double* ea = cx.scratch("ao2mo_ea", 2 * n);
    AFESP_HIP(hipMemcpyAsync(ea, levels_a, sizeof(double) * n, hipMemcpyHostToDevice, cx.stream));
    AFESP_HIP(hipMemcpyAsync(ea + n, levels_b, sizeof(double) * n, hipMemcpyHostToDevice, cx.stream));
    const double e2 = k_ump2(cx, in.uhf_aa, in.uhf_bb, in.uhf_ab, ea, ea + n, (int)n, (int)oa, (int)ob);
    if (eri_aa) AFESP_HIP(hipMemcpyAsync(eri_aa, in.uhf_aa, sizeof(double) * ne, hipMemcpyDeviceToHost, cx.stream));
    if (eri_bb) AFESP_HIP(hipMemcpyAsync(eri_bb, in.uhf_bb, sizeof(double) * ne, hipMemcpyDeviceToHost, cx.stream));
    if (eri_ab) AFESP_HIP(hipMemcpyAsync(eri_ab, in.uhf_ab, sizeof(double) * np * np, hipMemcpyDeviceToHost, cx.stream));
    cx.sync();
    return e2;
}

// The resident packed MO integrals in two new orbital sets, one per spin (afesp_mo_rotate_uhf): the mixed-spin transform
// above with the packed MO array in the place of the AO integrals and u_s (new orbital, old orbital) in the place of the coefficients.
// The source is only read; the three blocks are left resident as ao2mo_ump2 leaves them.
void mo_rotate_uhf(Context& cx, Integrals& in, int64_t n, const double* u_a, const double* u_b, double* eri_aa, double* eri_ab, double* eri_bb)
{
    const Ao2moForm form(n, true);
    if (form.blocked)
        throw Error(1, "afesp_mo_rotate_uhf: basis too large (only the slab-blocked transform fits, and it has no open-shell form)");
    if (!in.mo || in.mo_n != n)
        throw Error(1, "afesp_mo_rotate_uhf: no packed MO integrals resident for this basis size (afesp_ao2mo_mp2 / afesp_read_fcidump / "
                       "afesp_read_fcidump_rohf)");
    cx.drop_scratch("t_");
    cx.drop_scratch("ao2mo_");
    uhf_blocks_fit(cx, in, form, n, "afesp_mo_rotate_uhf");
    in.adopt_uhf(cx, n);
    uhf_blocks_from_packed(cx, in, form, n, in.mo, u_a, u_b);
    const int64_t ne = neri_of(n), np = npair_of(n);
    if (eri_aa) AFESP_HIP(hipMemcpyAsync(eri_aa, in.uhf_aa, sizeof(double) * ne, hipMemcpyDeviceToHost, cx.stream));
    if (eri_bb) AFESP_HIP(hipMemcpyAsync(eri_bb, in.uhf_bb, sizeof(double) * ne, hipMemcpyDeviceToHost, cx.stream));
    if (eri_ab) AFESP_HIP(hipMemcpyAsync(eri_ab, in.uhf_ab, sizeof(double) * np * np, hipMemcpyDeviceToHost, cx.stream));
    cx.sync();
}

// 1/2 sum_{i < na} [h + F_a](i,i) + 1/2 sum_{i < nb} [h + F_b](i,i), host matrices
static double ro_reference_energy(const double* h, const double* fa, const double* fb, int64_t n, int64_t na, int64_t nb)
{
    double ea = 0.0, eb = 0.0;
    for (int64_t i = 0; i < na; ++i) ea += h[i + n * i] + fa[i + n * i];
    for (int64_t i = 0; i < nb; ++i) eb += h[i + n * i] + fb[i + n * i];
    return 0.5 * ea + 0.5 * eb;
}

double mo_fock_ro(Context& cx, const Integrals& in, int64_t n, int64_t na, int64_t nb, const double* h_mo, double* fock_a, double* fock_b)
{
    const int64_t n2 = (n * n + 15) / 16 * 16;
    double* buf = cx.alloc_raw(3 * n2);   // h | F_a | F_b; back to the arena before the call ends, on every path
    try {
        AFESP_HIP(hipMemcpyAsync(buf, h_mo, sizeof(double) * n * n, hipMemcpyHostToDevice, cx.stream));
        k_fock_ro(cx, buf + n2, buf + 2 * n2, buf, in.mo, (int)n, (int)na, (int)nb);
        AFESP_HIP(hipMemcpyAsync(fock_a, buf + n2, sizeof(double) * n * n, hipMemcpyDeviceToHost, cx.stream));
        AFESP_HIP(hipMemcpyAsync(fock_b, buf + 2 * n2, sizeof(double) * n * n, hipMemcpyDeviceToHost, cx.stream));
        cx.sync();
    } catch (...) {
        (void)hipStreamSynchronize(cx.stream);
        try { cx.release(buf); } catch (...) {}
        throw;
    }
    cx.release(buf);
    return ro_reference_energy(h_mo, fock_a, fock_b, n, na, nb);
}

// The active orbital window [nfc, n - nfv) of the resident (or handed-in) packed MO integrals: a gather after the full transform
// (DESIGN.md), left resident as afesp_ao2mo_mp2 leaves a basis of n_act functions; the full array goes back to the arena here.
double mo_window(Context& cx, Integrals& in, Solver& sv, int64_t n, int64_t nocc, int64_t nfc, int64_t nfv, const double* levels,
                 const double* eri_mo_packed, double* eri_act)
{
    const int64_t na = n - nfc - nfv, o = nocc - nfc, v = na - o, ne = neri_of(n), nea = neri_of(na);
    double* full = in.mo;
    if (eri_mo_packed) {   // from the host: whatever was resident is replaced, as a transform would replace it
        in.drop_mo(cx, sv);
        full = cx.alloc_raw(ne);
        AFESP_HIP(hipMemcpyAsync(full, eri_mo_packed, sizeof(double) * ne, hipMemcpyHostToDevice, cx.stream));
    }
    double* act = full;
    if (na != n) {   // (the whole basis: the array stays where it is, bit for bit)
        try {
            act = cx.alloc_raw(nea);
            k_window_pack(cx, act, full, (int)na, (int)nfc);
        } catch (...) {
            if (act != full) cx.release(act);
            if (eri_mo_packed) cx.release(full);   // (resident integrals stay as they were)
            throw;
        }
        if (eri_mo_packed) cx.release(full);   // (waits for the gather) a context never keeps two packed arrays past the call
        else in.drop_mo(cx, sv);
    }
    in.set_mo(act, na);
    const double emp2 = mp2_of_packed(cx, act, levels + nfc, o, v);
    if (eri_act) {
        AFESP_HIP(hipMemcpyAsync(eri_act, act, sizeof(double) * nea, hipMemcpyDeviceToHost, cx.stream));
        cx.sync();
    }
    return emp2;
}

// ---- the virtual-virtual block of the MP2 one-particle density (frozen natural orbitals)
namespace {
inline int64_t up16(int64_t x) { return (x + 15) / 16 * 16; }   // (every piece of the scratch block starts on a 128-byte line)
// One block from the arena for the amplitude operands, D and the levels: refused (status 1) where it does not fit what the device has free
// plus what the arena holds idle -- as afesp_ao2mo_ump2 refuses -- and given back when the call ends, on every path.
struct FnoScratch {
    Context& cx;
    double* base = nullptr;
    FnoScratch(Context& c, int64_t ndoubles, const char* who, const char* what = "the amplitude operands of this system") : cx(c)
    {
        if (!cx.fits(8.0 * (double)ndoubles))
            throw Error(1, std::string(who) + ": " + what + " do not fit the free device memory");
        base = cx.alloc_raw(ndoubles);
    }
    ~FnoScratch()
    {
        try {
            cx.release(base);   // (waits for the stream)
        } catch (...) {
        }
    }
};
// D (+)= alpha A^T B over the rows: A, B dense (K x v), the contraction index fastest in both; the planner picks the kernel for the shape
void fno_product(Context& cx, double alpha, double* A, double* B, double* D, int64_t K, int64_t v)
{
    if (K <= 0 || v <= 0) return;
    contract(cx, alpha, view(A, {K, v}), "ka", view(B, {K, v}), "kb", 1.0, view(D, {v, v}), "ab");
}
// D -> host, symmetrised there (v^2 numbers): 1/2 (D(a,b) + D(b,a)) is the same number for both orders
void fno_fetch_symmetric(Context& cx, const double* D, int64_t v, double* host)
{
    if (v <= 0) return;
    AFESP_HIP(hipMemcpyAsync(host, D, sizeof(double) * v * v, hipMemcpyDeviceToHost, cx.stream));
    cx.sync();
    for (int64_t b = 0; b < v; ++b)
        for (int64_t a = 0; a < b; ++a) host[a + v * b] = host[b + v * a] = 0.5 * (host[a + v * b] + host[b + v * a]);
}
}  // namespace

double mp2_vv_density(Context& cx, const Integrals& in, int64_t n, int64_t nocc, int64_t nfc, const double* levels, double* d_vv)
{
    const int64_t o = nocc - nfc, v = n - nocc, sz = up16(o * o * v * v), K = o * o * v;
    FnoScratch s(cx, 2 * sz + up16(v * v) + up16(n), "afesp_mp2_vv_density");
    double *T = s.base, *Tt = T + sz, *D = Tt + sz, *e_dev = D + up16(v * v);
    AFESP_HIP(hipMemcpyAsync(e_dev, levels, sizeof(double) * n, hipMemcpyHostToDevice, cx.stream));
    AFESP_HIP(hipMemsetAsync(D, 0, sizeof(double) * v * v, cx.stream));
    k_fno_amps(cx, T, Tt, in.mo, e_dev, (int)nfc, (int)o, (int)v, 0);
    const double e2 = host_scalars(cx, 1)[0];
    fno_product(cx, 1.0, Tt, T, D, K, v);
    fno_fetch_symmetric(cx, D, v, d_vv);
    return e2;
}

double ump2_vv_density(Context& cx, const Integrals& in, int64_t n, int64_t na, int64_t nb, int64_t nfc, const double* levels_a,
                       const double* levels_b, double* d_a, double* d_b)
{
    const int64_t oa = na - nfc, ob = nb - nfc, va = n - na, vb = n - nb;
    const int64_t saa = up16(oa * oa * va * va), sbb = up16(ob * ob * vb * vb), sab = up16(oa * ob * va * vb), sss = std::max(saa, sbb);
    const int64_t vmax = std::max(va, vb);
    // one spin after the other in the same two operands: same-spin amplitudes, opposite-spin amplitudes
    FnoScratch s(cx, sss + sab + up16(vmax * vmax) + up16(2 * n), "afesp_ump2_vv_density");
    double *Tss = s.base, *Tos = Tss + sss, *D = Tos + sab, *ea = D + up16(vmax * vmax), *eb = ea + n;
    AFESP_HIP(hipMemcpyAsync(ea, levels_a, sizeof(double) * n, hipMemcpyHostToDevice, cx.stream));
    AFESP_HIP(hipMemcpyAsync(eb, levels_b, sizeof(double) * n, hipMemcpyHostToDevice, cx.stream));
    double e2 = 0.0;
    for (int beta = 0; beta < 2; ++beta) {
        const int64_t o = beta ? ob : oa, v = beta ? vb : va, Kss = o * o * v, Kos = beta ? oa * ob * va : oa * ob * vb;
        if (v <= 0) continue;
        AFESP_HIP(hipMemsetAsync(D, 0, sizeof(double) * v * v, cx.stream));
        if (Kss > 0) {
            k_fno_amps(cx, Tss, nullptr, beta ? in.uhf_bb : in.uhf_aa, beta ? eb : ea, (int)nfc, (int)o, (int)v, 0);
            e2 += host_scalars(cx, 1)[0];
            fno_product(cx, 0.5, Tss, Tss, D, Kss, v);
        }
        if (Kos > 0) {
            k_fno_amps_ab(cx, Tos, in.uhf_ab, ea, eb, (int)n, (int)nfc, (int)oa, (int)ob, (int)va, (int)vb, beta != 0, 0);
            if (!beta) e2 += host_scalars(cx, 1)[0];   // (the opposite-spin energy once)
            fno_product(cx, 1.0, Tos, Tos, D, Kos, v);
        }
        fno_fetch_symmetric(cx, D, v, beta ? d_b : d_a);
    }
    // (a spin without virtuals contributes its opposite-spin energy through the other spin's pass; without virtuals in alpha that pass is
    // skipped above and the opposite-spin energy is zero anyway: no alpha virtual, no (ia|JB))
    return e2;
}

// ---- the frozen-core operator of the active window and the core energy
namespace {
// h_mo = C h_ao C^T on the device: C is (MO, AO), so h_mo(p,q) = sum_ab C(p,a) h(a,b) C(q,b); hao and tmp are n x n scratch
void core_h_mo(Context& cx, const double* coeff_host, double* Cm, double* hao, double* tmp, double* hmo, int64_t n)
{
    AFESP_HIP(hipMemcpyAsync(Cm, coeff_host, sizeof(double) * n * n, hipMemcpyHostToDevice, cx.stream));
    contract(cx, 1.0, view(Cm, {n, n}), "pa", view(hao, {n, n}), "ab", 0.0, view(tmp, {n, n}), "pb");
    contract(cx, 1.0, view(Cm, {n, n}), "qb", view(tmp, {n, n}), "pb", 0.0, view(hmo, {n, n}), "pq");
}
}  // namespace

void core_operator(Context& cx, const Integrals& in, int64_t n, int64_t nfc, int64_t nfv, const double* coeff, const double* h_ao, double* h_act,
                   double* e_core)
{
    const int64_t na = n - nfc - nfv, n2 = up16(n * n);
    FnoScratch s(cx, 4 * n2 + up16(na * na) + 16, "afesp_core_operator", "the one-electron matrices of this system");
    double *Cm = s.base, *hao = Cm + n2, *tmp = hao + n2, *hmo = tmp + n2, *hact = hmo + n2, *e_dev = hact + up16(na * na);
    AFESP_HIP(hipMemcpyAsync(hao, h_ao, sizeof(double) * n * n, hipMemcpyHostToDevice, cx.stream));
    core_h_mo(cx, coeff, Cm, hao, tmp, hmo, n);
    k_core_fold(cx, hact, e_dev, hmo, in.mo, (int)n, (int)nfc, (int)na, false);
    AFESP_HIP(hipMemcpyAsync(h_act, hact, sizeof(double) * na * na, hipMemcpyDeviceToHost, cx.stream));
    AFESP_HIP(hipMemcpyAsync(e_core, e_dev, sizeof(double), hipMemcpyDeviceToHost, cx.stream));
    cx.sync();
}

void ucore_operator(Context& cx, const Integrals& in, int64_t n, int64_t nfc, int64_t nfv, const double* coeff_a, const double* coeff_b,
                    const double* h_ao, double* h_act_a, double* h_act_b, double* e_core)
{
    const int64_t na = n - nfc - nfv, n2 = up16(n * n), a2 = up16(na * na);
    FnoScratch s(cx, 4 * n2 + 2 * a2 + 16, "afesp_ucore_operator", "the one-electron matrices of this system");
    double *Cm = s.base, *hao = Cm + n2, *tmp = hao + n2, *hmo = tmp + n2, *ha = hmo + n2, *hb = ha + a2, *e_dev = hb + a2;
    AFESP_HIP(hipMemcpyAsync(hao, h_ao, sizeof(double) * n * n, hipMemcpyHostToDevice, cx.stream));
    core_h_mo(cx, coeff_a, Cm, hao, tmp, hmo, n);
    k_core_fold(cx, ha, e_dev, hmo, in.uhf_aa, (int)n, (int)nfc, (int)na, true);
    core_h_mo(cx, coeff_b, Cm, hao, tmp, hmo, n);
    k_core_fold(cx, hb, e_dev + 1, hmo, in.uhf_bb, (int)n, (int)nfc, (int)na, true);
    k_core_fold_ab(cx, ha, hb, e_dev + 2, in.uhf_ab, (int)n, (int)nfc, (int)na);
    double e[3] = {0.0, 0.0, 0.0};
    AFESP_HIP(hipMemcpyAsync(h_act_a, ha, sizeof(double) * na * na, hipMemcpyDeviceToHost, cx.stream));
    AFESP_HIP(hipMemcpyAsync(h_act_b, hb, sizeof(double) * na * na, hipMemcpyDeviceToHost, cx.stream));
    AFESP_HIP(hipMemcpyAsync(e, e_dev, 3 * sizeof(double), hipMemcpyDeviceToHost, cx.stream));
    cx.sync();
    *e_core = (e[0] + e[1]) + e[2];
}

// ---- the standard FCIDUMP of the resident integrals
namespace {
struct File {
    FILE* f;
    explicit File(FILE* g) : f(g) {}
    ~File() { if (f) fclose(f); }
};
// the survivors |x| > threshold of a device array, compacted there (integrals_kernels.hip) and written as two-electron lines; returns their number
int64_t dump_block(Context& cx, FILE* f, const char* who, const double* x, int64_t total, double threshold, fcidump::Block b, int64_t np)
{
    const int64_t nchunks = k_compact_chunks(total);
    FnoScratch counts(cx, nchunks + 1, who, "the compaction counters");
    int64_t* prefix = reinterpret_cast<int64_t*>(counts.base);
    k_compact_count(cx, prefix, x, total, threshold);
    int64_t kept = 0;
    AFESP_HIP(hipMemcpyAsync(&kept, prefix + nchunks, sizeof(int64_t), hipMemcpyDeviceToHost, cx.stream));
    cx.sync();
    if (kept == 0) return 0;
    FnoScratch pairs(cx, 2 * kept, who, "the compacted integrals");
    int64_t* idx_dev = reinterpret_cast<int64_t*>(pairs.base);
    double* val_dev = pairs.base + kept;
    k_compact_scatter(cx, idx_dev, val_dev, prefix, x, total, threshold);
    std::vector<int64_t> idx((size_t)kept);
    std::vector<double> val((size_t)kept);
    AFESP_HIP(hipMemcpyAsync(idx.data(), idx_dev, sizeof(int64_t) * kept, hipMemcpyDeviceToHost, cx.stream));
    AFESP_HIP(hipMemcpyAsync(val.data(), val_dev, sizeof(double) * kept, hipMemcpyDeviceToHost, cx.stream));
    cx.sync();
    if (!fcidump::write_two_electron(f, b, np, idx.data(), val.data(), kept, fcidump::thread_count(kept)))
        throw Error(2, std::string(who) + ": write failed");
    return kept;
}
}  // namespace

int64_t write_fcidump_active(Context& cx, const Integrals& in, const char* path, int64_t n_act, int64_t nelec, int64_t ms2, const double* h_act,
                             double e_core_total, double threshold)
{
    const char* who = "afesp_write_fcidump_active";
    File out(fopen(path, "w"));
    if (!out.f) throw Error(2, std::string(who) + ": cannot open " + path);
    if (!fcidump::write_header(out.f, n_act, nelec, ms2, false)) throw Error(2, std::string(who) + ": write failed");
    int64_t lines = dump_block(cx, out.f, who, in.mo, neri_of(n_act), threshold, fcidump::SPATIAL, 0);
    const int64_t one = fcidump::write_one_electron(out.f, h_act, n_act, threshold, false, false);
    if (one < 0 || !fcidump::write_core_energy(out.f, e_core_total)) throw Error(2, std::string(who) + ": write failed");
    lines += one + 1;
    FILE* f = out.f;
    out.f = nullptr;
    if (fclose(f) != 0) throw Error(2, std::string(who) + ": write failed");
    return lines;
}

int64_t write_fcidump_uactive(Context& cx, const Integrals& in, const char* path, int64_t n_act, int64_t nalpha, int64_t nbeta,
                              const double* h_act_a, const double* h_act_b, double e_core_total, double threshold)
{
    const char* who = "afesp_write_fcidump_uactive";
    const int64_t np = npair_of(n_act);
    File out(fopen(path, "w"));
    if (!out.f) throw Error(2, std::string(who) + ": cannot open " + path);
    if (!fcidump::write_header(out.f, 2 * n_act, nalpha + nbeta, nalpha - nbeta, true)) throw Error(2, std::string(who) + ": write failed");
    int64_t lines = dump_block(cx, out.f, who, in.uhf_aa, neri_of(n_act), threshold, fcidump::ALPHA_ALPHA, 0);
    lines += dump_block(cx, out.f, who, in.uhf_bb, neri_of(n_act), threshold, fcidump::BETA_BETA, 0);
    lines += dump_block(cx, out.f, who, in.uhf_ab, np * np, threshold, fcidump::ALPHA_BETA, np);
    const int64_t one_a = fcidump::write_one_electron(out.f, h_act_a, n_act, threshold, true, false);
    const int64_t one_b = one_a < 0 ? -1 : fcidump::write_one_electron(out.f, h_act_b, n_act, threshold, true, true);
    if (one_b < 0 || !fcidump::write_core_energy(out.f, e_core_total)) throw Error(2, std::string(who) + ": write failed");
    lines += one_a + one_b + 1;
    FILE* f = out.f;
    out.f = nullptr;
    if (fclose(f) != 0) throw Error(2, std::string(who) + ": write failed");
    return lines;
}

// ---- a standard FCIDUMP as input: text -> records on the host (fcidump_parse.h), records -> slots on the device
namespace {
// the header (fcidump_parse.h: read_header); leaves the file positioned at the body
void fcidump_open_header(FILE* f, const char* who, const char* path, fcidump::Header& h)
{
    std::string why;
    if (!fcidump::read_header(f, h, why)) throw Error(1, std::string(who) + ": " + why + " in " + path);
}
// everything a read allocates: back to the arena / the driver on every path, after the stream has drained
struct ReadScratch {
    Context& cx;
    std::vector<void*> dev;
    void* pinned[2] = {nullptr, nullptr};
    hipEvent_t ev[2] = {nullptr, nullptr};
    explicit ReadScratch(Context& c) : cx(c) {}
    double* get(int64_t ndoubles)
    {
        double* p = cx.alloc_raw(ndoubles);
        dev.push_back(p);
        return p;
    }
    void keep(void* p)   // the caller takes it over
    {
        for (void*& q : dev)
            if (q == p) q = nullptr;
    }
    ~ReadScratch()
    {
        (void)hipStreamSynchronize(cx.stream);
        for (void* p : dev) {
            try {
                if (p) cx.release(p);
            } catch (...) {
            }
        }
        for (int b = 0; b < 2; ++b) {
            if (pinned[b]) (void)hipHostFree(pinned[b]);
            if (ev[b]) (void)hipEventDestroy(ev[b]);
        }
    }
};
struct FcidumpRead {
    double e_core = 0.0;
    int64_t nread = 0;
};
// The body of `f` into the targets (zeroed here).  Throws status 1 with the line number for everything the file can do wrong.
FcidumpRead fcidump_read_body(Context& cx, ReadScratch& rs, FILE* f, const char* who, const fcidump::Header& h, FcidumpTargets& T)
{
    const size_t chunk = (size_t)knobs().fcidump_chunk_kib << 10;
    const int64_t max_rec = (int64_t)(chunk / 8 + 2);
    for (int b = 0; b < 2; ++b) {
        AFESP_HIP(hipHostMalloc(&rs.pinned[b], (size_t)max_rec * sizeof(fcidump::Record), hipHostMallocDefault));
        AFESP_HIP(hipEventCreateWithFlags(&rs.ev[b], hipEventDisableTiming));
    }
    fcidump::Record* rec_dev = reinterpret_cast<fcidump::Record*>(rs.get(max_rec * 4));
    T.visited = reinterpret_cast<uint32_t*>(rs.get((T.nslots + 63) / 64 + 1));
    T.err = reinterpret_cast<unsigned long long*>(rs.get(2));
    AFESP_HIP(hipMemsetAsync(T.visited, 0, (size_t)((T.nslots + 63) / 64 + 1) * 8, cx.stream));
    const unsigned long long err0[2] = {0ull, ~0ull};
    AFESP_HIP(hipMemcpyAsync(T.err, err0, sizeof(err0), hipMemcpyHostToDevice, cx.stream));
    cx.sync();   // (err0 is on this frame)
    FcidumpRead out;
    bool used[2] = {false, false};
    // the chunk loop is fcidump_parse.h's: the host parses round k + 1 into one pinned buffer while the device scatters round k
    const fcidump::ParseError perr = fcidump::read_body(
        f, h, chunk, fcidump::reader_threads(),
        [&](int b) {
            if (used[b]) AFESP_HIP(hipEventSynchronize(rs.ev[b]));   // the copy out of this buffer two rounds ago
            return static_cast<fcidump::Record*>(rs.pinned[b]);
        },
        [&](const fcidump::Record* rec, int64_t count, int b) {
            AFESP_HIP(hipMemcpyAsync(rec_dev, rec, (size_t)count * sizeof(fcidump::Record), hipMemcpyHostToDevice, cx.stream));
            AFESP_HIP(hipEventRecord(rs.ev[b], cx.stream));
            used[b] = true;
            k_fcidump_scatter(cx, T, rec_dev, count);
        },
        &out.nread);
    if (perr.line) throw Error(1, std::string(who) + ": line " + std::to_string(perr.line) + ": " + perr.why);
    if (ferror(f)) throw Error(1, std::string(who) + ": read error");
    unsigned long long err[2] = {0, 0};
    AFESP_HIP(hipMemcpyAsync(err, T.err, sizeof(err), hipMemcpyDeviceToHost, cx.stream));
    AFESP_HIP(hipMemcpyAsync(&out.e_core, T.ecore, sizeof(double), hipMemcpyDeviceToHost, cx.stream));
    cx.sync();
    if (err[0])
        throw Error(1, std::string(who) + ": line " + std::to_string(err[1]) + ": a duplicate that disagrees with another line for the same integral (" +
                           std::to_string(err[0]) + " mismatches)");
    return out;
}
void fcidump_fit(Context& cx, const char* who, double ndoubles)
{
    if (!cx.fits(8.0 * ndoubles))
        throw Error(1, std::string(who) + ": the integrals of this file do not fit the free device memory");
}
double offdiag_max(const double* F, int64_t n)
{
    double m = 0.0;
    for (int64_t q = 0; q < n; ++q)
        for (int64_t p = 0; p < n; ++p)
            if (p != q) m = std::max(m, std::fabs(F[p + n * q]));
    return m;
}
}  // namespace

int fcidump_scan(const char* path, int64_t* norb, int64_t* nelec, int64_t* ms2, int* uhf, int64_t* nlines)
{
    if (!path) return 1;
    File in(fopen(path, "rb"));
    if (!in.f) return 1;
    fcidump::Header h;
    try {
        fcidump_open_header(in.f, "afesp_fcidump_scan", path, h);
    } catch (const std::exception&) {
        return 1;
    }
    int64_t lines = 0;
    std::vector<char> blk(1 << 20);
    bool ink = false;   // the current line has a non-blank character
    for (size_t got; (got = fread(blk.data(), 1, blk.size(), in.f)) > 0;)
        for (size_t i = 0; i < got; ++i) {
            const char c = blk[i];
            if (c == '\n') { lines += ink; ink = false; }
            else if (!fcidump::detail::blank(c)) ink = true;
        }
    lines += ink;
    if (norb) *norb = h.norb;
    if (nelec) *nelec = h.nelec;
    if (ms2) *ms2 = h.ms2;
    if (uhf) *uhf = h.uhf ? 1 : 0;
    if (nlines) *nlines = lines;
    return 0;
}

namespace {
// What afesp_read_fcidump and afesp_read_fcidump_rohf share once the header has passed their own checks: the body of a restricted file
// into a new packed array and h, the Fock operator(s) of the determinant that fills the first na (alpha) / nb (beta) orbitals -- ro:
// the two spin operators (k_fock_ro), else the closed-shell one (na == nb) -- and, only when all of that was good, residency.
void read_restricted(Context& cx, Integrals& in, Solver& sv, FILE* f, const char* who, const fcidump::Header& h, int64_t n, int64_t na,
                     int64_t nb, bool ro, FcidumpResult& r)
{
    const int64_t ne = neri_of(n), np = npair_of(n), n2 = up16(n * n), nf = ro ? 2 : 1;
    FcidumpTargets T{};
    T.n = n; T.np = np; T.ne = ne; T.uhf = 0;
    T.nslots = ne + np + 1;
    fcidump_fit(cx, who, (double)ne + (double)T.nslots / 64 + (1.0 + nf) * n2 + ((double)knobs().fcidump_chunk_kib * 1024 / 2));
    ReadScratch rs(cx);
    double* packed = rs.get(ne);
    double* small = rs.get((1 + nf) * n2 + 16);   // h | F (| F_b) | core energy
    T.eri[0] = packed;
    T.h[0] = small;
    T.ecore = small + (1 + nf) * n2;
    AFESP_HIP(hipMemsetAsync(packed, 0, sizeof(double) * ne, cx.stream));
    AFESP_HIP(hipMemsetAsync(small, 0, sizeof(double) * ((1 + nf) * n2 + 16), cx.stream));
    const FcidumpRead got = fcidump_read_body(cx, rs, f, who, h, T);
    double* F = small + n2;
    if (ro) k_fock_ro(cx, F, F + n2, T.h[0], packed, (int)n, (int)na, (int)nb);
    else k_fock_mo(cx, F, T.h[0], packed, (int)n, (int)na, 2.0);
    std::vector<double> hh((size_t)(n * n)), ff[2];
    AFESP_HIP(hipMemcpyAsync(hh.data(), T.h[0], sizeof(double) * n * n, hipMemcpyDeviceToHost, cx.stream));
    for (int64_t s = 0; s < nf; ++s) {
        ff[s].resize((size_t)(n * n));
        AFESP_HIP(hipMemcpyAsync(ff[s].data(), F + s * n2, sizeof(double) * n * n, hipMemcpyDeviceToHost, cx.stream));
    }
    if (r.eri[0]) AFESP_HIP(hipMemcpyAsync(r.eri[0], packed, sizeof(double) * ne, hipMemcpyDeviceToHost, cx.stream));
    cx.sync();
    // from here on nothing fails: the new array takes the place of the resident one, as a transform's result would
    cx.drop_scratch("t_");
    in.release_uhf(cx);
    in.drop_mo(cx, sv);
    rs.keep(packed);
    in.set_mo(packed, n);
    if (r.h[0]) memcpy(r.h[0], hh.data(), sizeof(double) * n * n);
    for (int64_t s = 0; s < nf; ++s)
        if (r.fock[s]) memcpy(r.fock[s], ff[s].data(), sizeof(double) * n * n);
    r.e_core = got.e_core;
    r.nread = got.nread;
    if (ro) {
        r.e_ref = got.e_core + ro_reference_energy(hh.data(), ff[0].data(), ff[1].data(), n, na, nb);
        // largest |F| of either spin among the occupied-occupied off-diagonal, the virtual-virtual off-diagonal and the occupied-virtual elements
        for (int k = 0; k < 3; ++k) r.fock_offdiag3[k] = 0.0;
        for (int s = 0; s < 2; ++s) {
            const int64_t o = s ? nb : na;
            for (int64_t q = 0; q < n; ++q)
                for (int64_t p = 0; p < n; ++p) {
                    if (p == q) continue;
                    const int k = (p < o && q < o) ? 0 : (p >= o && q >= o) ? 1 : 2;
                    r.fock_offdiag3[k] = std::max(r.fock_offdiag3[k], std::fabs(ff[s][(size_t)(p + n * q)]));
                }
        }
        return;
    }
    double e = got.e_core;
    for (int64_t i = 0; i < na; ++i) e += hh[(size_t)(i + n * i)] + ff[0][(size_t)(i + n * i)];
    if (r.levels[0])
        for (int64_t p = 0; p < n; ++p) r.levels[0][p] = ff[0][(size_t)(p + n * p)];
    r.e_ref = e;
    r.fock_offdiag = offdiag_max(ff[0].data(), n);
}
}  // namespace

void read_fcidump(Context& cx, Integrals& in, Solver& sv, const char* path, int64_t n, int64_t nocc, FcidumpResult& r)
{
    const char* who = "afesp_read_fcidump";
    File file(fopen(path, "rb"));
    if (!file.f) throw Error(1, std::string(who) + ": cannot open " + path);
    fcidump::Header h;
    fcidump_open_header(file.f, who, path, h);
    if (h.uhf) throw Error(1, std::string(who) + ": the file says UHF=.TRUE. (afesp_read_fcidump_uhf reads it)");
    if (h.norb != n || h.nelec != 2 * nocc || h.ms2 != 0)
        throw Error(1, std::string(who) + ": the header (NORB " + std::to_string(h.norb) + ", NELEC " + std::to_string(h.nelec) + ", MS2 " +
                           std::to_string(h.ms2) + ") disagrees with nbasis " + std::to_string(n) + ", nocc " + std::to_string(nocc));
    read_restricted(cx, in, sv, file.f, who, h, n, nocc, nocc, false, r);
}

// The restricted open-shell file (no UHF flag, MS2 = nalpha - nbeta >= 0): one set of orbitals and integrals, two spin Fock operators
void read_fcidump_rohf(Context& cx, Integrals& in, Solver& sv, const char* path, int64_t n, int64_t na, int64_t nb, FcidumpResult& r)
{
    const char* who = "afesp_read_fcidump_rohf";
    File file(fopen(path, "rb"));
    if (!file.f) throw Error(1, std::string(who) + ": cannot open " + path);
    fcidump::Header h;
    fcidump_open_header(file.f, who, path, h);
    if (h.uhf) throw Error(1, std::string(who) + ": the file says UHF=.TRUE. (afesp_read_fcidump_uhf reads it)");
    if (h.ms2 < 0) throw Error(1, std::string(who) + ": MS2 " + std::to_string(h.ms2) + " is negative (more beta than alpha electrons)");
    if (h.norb != n || h.nelec != na + nb || h.ms2 != na - nb)
        throw Error(1, std::string(who) + ": the header (NORB " + std::to_string(h.norb) + ", NELEC " + std::to_string(h.nelec) + ", MS2 " +
                           std::to_string(h.ms2) + ") disagrees with nbasis " + std::to_string(n) + ", nalpha " + std::to_string(na) + ", nbeta " +
                           std::to_string(nb));
    read_restricted(cx, in, sv, file.f, who, h, n, na, nb, true, r);
}

void read_fcidump_uhf(Context& cx, Integrals& in, const char* path, int64_t n, int64_t na, int64_t nb, FcidumpResult& r)
{
    const char* who = "afesp_read_fcidump_uhf";
    File file(fopen(path, "rb"));
    if (!file.f) throw Error(1, std::string(who) + ": cannot open " + path);
    fcidump::Header h;
    fcidump_open_header(file.f, who, path, h);
    if (!h.uhf) throw Error(1, std::string(who) + ": the file does not say UHF=.TRUE. (afesp_read_fcidump reads it)");
    if (h.norb != 2 * n || h.nelec != na + nb || h.ms2 != na - nb)
        throw Error(1, std::string(who) + ": the header (NORB " + std::to_string(h.norb) + ", NELEC " + std::to_string(h.nelec) + ", MS2 " +
                           std::to_string(h.ms2) + ") disagrees with nbasis " + std::to_string(n) + ", nalpha " + std::to_string(na) + ", nbeta " +
                           std::to_string(nb));
    const int64_t ne = neri_of(n), np = npair_of(n), n2 = up16(n * n);
    FcidumpTargets T{};
    T.n = n; T.np = np; T.ne = ne; T.uhf = 1;
    T.nslots = 2 * ne + np * np + 2 * np + 1;
    fcidump_fit(cx, who, 2.0 * ne + (double)np * np + (double)T.nslots / 64 + 4.0 * n2 + ((double)knobs().fcidump_chunk_kib * 1024 / 2));
    ReadScratch rs(cx);
    double *aa = rs.get(ne), *bb = rs.get(ne), *ab = rs.get(np * np);
    double* small = rs.get(4 * n2 + 16);   // h_a | h_b | F_a | F_b | core energy
    T.eri[0] = aa; T.eri[1] = bb; T.eri[2] = ab;
    T.h[0] = small; T.h[1] = small + n2;
    T.ecore = small + 4 * n2;
    AFESP_HIP(hipMemsetAsync(aa, 0, sizeof(double) * ne, cx.stream));
    AFESP_HIP(hipMemsetAsync(bb, 0, sizeof(double) * ne, cx.stream));
    AFESP_HIP(hipMemsetAsync(ab, 0, sizeof(double) * np * np, cx.stream));
    AFESP_HIP(hipMemsetAsync(small, 0, sizeof(double) * (4 * n2 + 16), cx.stream));
    const FcidumpRead got = fcidump_read_body(cx, rs, file.f, who, h, T);
    double *Fa = small + 2 * n2, *Fb = small + 3 * n2;
    k_fock_mo(cx, Fa, T.h[0], aa, (int)n, (int)na, 1.0);
    k_fock_mo(cx, Fb, T.h[1], bb, (int)n, (int)nb, 1.0);
    k_fock_mo_ab(cx, Fa, Fb, ab, (int)n, (int)na, (int)nb);
    std::vector<double> hh[2], ff[2];
    for (int s = 0; s < 2; ++s) {
        hh[s].resize((size_t)(n * n));
        ff[s].resize((size_t)(n * n));
        AFESP_HIP(hipMemcpyAsync(hh[s].data(), T.h[s], sizeof(double) * n * n, hipMemcpyDeviceToHost, cx.stream));
        AFESP_HIP(hipMemcpyAsync(ff[s].data(), s ? Fb : Fa, sizeof(double) * n * n, hipMemcpyDeviceToHost, cx.stream));
    }
    if (r.eri[0]) AFESP_HIP(hipMemcpyAsync(r.eri[0], aa, sizeof(double) * ne, hipMemcpyDeviceToHost, cx.stream));
    if (r.eri[1]) AFESP_HIP(hipMemcpyAsync(r.eri[1], bb, sizeof(double) * ne, hipMemcpyDeviceToHost, cx.stream));
    if (r.eri[2]) AFESP_HIP(hipMemcpyAsync(r.eri[2], ab, sizeof(double) * np * np, hipMemcpyDeviceToHost, cx.stream));
    cx.sync();
    cx.drop_scratch("t_");
    rs.keep(aa); rs.keep(bb); rs.keep(ab);
    in.swap_uhf(cx, aa, bb, ab, n);
    double ea = 0.0, eb = 0.0;
    for (int64_t i = 0; i < na; ++i) ea += hh[0][(size_t)(i + n * i)] + ff[0][(size_t)(i + n * i)];
    for (int64_t i = 0; i < nb; ++i) eb += hh[1][(size_t)(i + n * i)] + ff[1][(size_t)(i + n * i)];
    for (int s = 0; s < 2; ++s) {
        if (r.h[s]) memcpy(r.h[s], hh[s].data(), sizeof(double) * n * n);
        if (r.fock[s]) memcpy(r.fock[s], ff[s].data(), sizeof(double) * n * n);
        if (r.levels[s])
            for (int64_t p = 0; p < n; ++p) r.levels[s][p] = ff[s][(size_t)(p + n * p)];
    }
    r.e_core = got.e_core;
    r.e_ref = got.e_core + 0.5 * ea + 0.5 * eb;
    r.fock_offdiag = std::max(offdiag_max(ff[0].data(), n), offdiag_max(ff[1].data(), n));
    r.nread = got.nread;
}

int64_t read_eri_text(Context& cx, Integrals& in, const char* path, int64_t nbasis, double* eri_packed)
{
    FILE* f = fopen(path, "rb");
    if (!f) throw Error(2, std::string("afesp_read_eri_text: cannot open ") + path);
    std::vector<double> host((size_t)neri_of(nbasis), 0.0);
    const int64_t lines = parse_eri_text(f, nbasis, host);
    fclose(f);
    if (lines < 0) throw Error(2, std::string("afesp_read_eri_text: malformed line or index outside 1..nbasis in ") + path);
    in.upload_ao(cx, nbasis, host.data());
    if (eri_packed) memcpy(eri_packed, host.data(), sizeof(double) * host.size());
    return lines;
}

// write_fcidump (src/mp2.f90:451-487): the packed MO integrals in canonical order, one line "p q r s value" in format
// (I3,I3,I3,I3,ES17.9) for every |value| > 1e-7 (no header, no one-electron part -- as the reference writes it).
int64_t write_fcidump(Context& cx, const Integrals& in, const char* path, int64_t nbasis)
{
    std::vector<double> host((size_t)neri_of(nbasis));
    AFESP_HIP(hipMemcpyAsync(host.data(), in.mo, sizeof(double) * host.size(), hipMemcpyDeviceToHost, cx.stream));
    cx.sync();
    FILE* f = fopen(path, "w");
    if (!f) throw Error(2, std::string("afesp_write_fcidump: cannot open ") + path);
    int64_t pqrs = 0, lines = 0;
    for (int64_t p = 1; p <= nbasis; ++p)
        for (int64_t q = 1; q <= p; ++q)
            for (int64_t r = 1; r <= p; ++r) {
                const int64_t s_up = (p == r) ? q : r;
                for (int64_t s = 1; s <= s_up; ++s) {
                    const double x = host[(size_t)pqrs++];
                    if (std::fabs(x) > 1e-7) {
                        fprintf(f, "%3d%3d%3d%3d%17.9E\n", (int)p, (int)q, (int)r, (int)s, x);
                        ++lines;
                    }
                }
            }
    fclose(f);
    return lines;
}

}  // namespace afesp
