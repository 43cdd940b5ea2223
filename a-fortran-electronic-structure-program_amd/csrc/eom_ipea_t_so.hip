// eom_ipea_t_so.hip -- the non-iterative triples correction to EOM-IP-CCSD and EOM-EA-CCSD roots (eom_ipea_t_so.h), in the
// letters of tests/np_eom_ipea_t.py (per_item_explicit).
//
// Every numerator is a signed sum of "images", and every image is a v x v tile (IP) or a v^3 cube (EA) that one group of products fills:
//   IP  image (p;q,r), three per triple: +(i;j,k), -(j;i,k), -(k;j,i).  With U_fpb = sum_l r_l <fp||bl>, Y_mqr = sum_l r_l <ml||qr>
//         Q_r[b,a] = 1/2 sum_f <fp||ba> r_qrf - 1/2 sum_m t_mpab Y_mqr + sum_m r_mpb <ma||qr> - sum_f U_fpb t_qraf
//         Q_l[b,a] = 1/2 sum_f <fp||ba> l_qrf + sum_m l_mpb <ma||qr>
//       and the numerators of the triple are  sum+- (Q[b,a] - Q[a,b])  (the first two products are antisymmetric in a,b: hence the halves),
//       the left one with  l_p <qr||ab> + [f_pa l_qrb - f_pb l_qra]  added by the contraction kernel.
//   EA  image (p,q), two per pair: +(i,j), -(j,i), and the pair-symmetric part S(i,j).  With U_fbc = sum_d <fd||bc> r_d, Y_mar = sum_d <ma||dr> r_d
//         Q_r(p,q)[b,c,a] = sum_f <fp||bc> r_qaf + sum_m t_mpcb Y_maq        S_r(i,j)[b,c,a] = sum_m r_mcb <ma||ji> - sum_f U_fbc t_jiaf
//         Q_l(p,q)[b,c,a] = sum_f <fp||bc> l_qaf                              S_l(i,j)[b,c,a] = sum_m l_mcb <ma||ji>
//       m = Q_r(i,j) - Q_r(j,i) + S_r,  l = Q_l(i,j) - Q_l(j,i) + S_l + l_a <ij||bc> + [f_ia l_jbc - f_ja l_ibc].
// The images of a chunk of items are columns of one buffer per side, sorted by p, so that all images of one p are ONE product of the
// p-slice of a resident operand (<fp||bc>, t_mp.., r_mp., U_fp.) with the columns a build kernel gathered for them (r_qrf, Y_mqr, <ma||qr>,
// t_qraf, ...): contract() calls with beta = 1 for the terms that share a tile, no new GEMM kernel and no padded operand.  Every ordered
// (p; q<r) with p outside the pair (IP) and every ordered p != q (EA) is used by exactly one item, so no product is computed twice or in vain.
// Chunks of items bound the scratch by the (T) pool knob; the two contraction kernels leave one partial per block, summed in a fixed order.
#include <cstdio>
#include <vector>

#include "device_util.h"
#include "eom_ipea_t_so.h"
#include "knobs.h"
#include "lambda_so.h"

namespace afesp {
namespace {

struct IpeaTCol { int p, q, r, pad; };      // IP: image (p;q,r).  EA: image (p,q) with r = -1; pair-symmetric part of (i,j): p = o, q = i, r = j
struct IpeaTItem { int c0, c1, c2, pad; };  // the columns of an item's images: IP (i;j,k), (j;i,k), (k;j,i); EA (i,j), (j,i), S(i,j)

// The gathered column operands of one chunk, zero-free: every element of every buffer is written.
//   IP, column c = (p;q,r):  xr[f,c] = r2(q,r,f)   xl[f,c] = l2(q,r,f)   yy[m,c] = Y(m,q,r)   bo[m,a,c] = <ma||qr>   bt[f,a,c] = t2(q,r,a,f)
__global__ __launch_bounds__(TB) void ipt_build_ip_kernel(double* __restrict__ xr, double* __restrict__ xl, double* __restrict__ yy,
                                                          double* __restrict__ bo, double* __restrict__ bt, const IpeaTCol* __restrict__ cols,
                                                          int64_t ncol, const double* __restrict__ r2, const double* __restrict__ l2,
                                                          const double* __restrict__ Y, const double* __restrict__ ovoo,
                                                          const double* __restrict__ t2, int o, int v)
{
    const int64_t O = o, V = v, W = 2 * V + O + O * V + V * V;
    GRID_STRIDE(x, ncol * W)
    {
        const int64_t c = x / W;
        int64_t y = x % W;
        const int64_t q = cols[c].q, r = cols[c].r;
        if (y < V) { xr[y + V * c] = r2[q + O * (r + O * y)]; continue; }
        y -= V;
        if (y < V) { xl[y + V * c] = l2[q + O * (r + O * y)]; continue; }
        y -= V;
        if (y < O) { yy[y + O * c] = Y[y + O * (q + O * r)]; continue; }
        y -= O;
        if (y < O * V) { bo[y + O * V * c] = ovoo[y + O * V * (q + O * r)]; continue; }
        y -= O * V;
        const int64_t f = y % V, a = y / V;
        bt[y + V * V * c] = t2[q + O * (r + O * (a + V * f))];
    }
}

//   EA, image column c < nimg = (p,q):  xr[f,a,c] = r2(q,a,f)   xl[f,a,c] = l2(q,a,f)   yy[m,a,c] = Y(m,a,q)
//       pair column c >= nimg = S(i,j):  bo[m,a,c-nimg] = <ma||ji>   bt[f,a,c-nimg] = t2(j,i,a,f)
__global__ __launch_bounds__(TB) void ipt_build_ea_kernel(double* __restrict__ xr, double* __restrict__ xl, double* __restrict__ yy,
                                                          double* __restrict__ bo, double* __restrict__ bt, const IpeaTCol* __restrict__ cols,
                                                          int64_t nimg, int64_t npair, const double* __restrict__ r2, const double* __restrict__ l2,
                                                          const double* __restrict__ Y, const double* __restrict__ ovoo,
                                                          const double* __restrict__ t2, int o, int v)
{
    const int64_t O = o, V = v, W1 = 2 * V * V + O * V, W2 = O * V + V * V;
    GRID_STRIDE(x, nimg * W1 + npair * W2)
    {
        if (x < nimg * W1) {
            const int64_t c = x / W1;
            int64_t y = x % W1;
            const int64_t q = cols[c].q;
            if (y < 2 * V * V) {
                const bool left = y >= V * V;
                if (left) y -= V * V;
                const int64_t f = y % V, a = y / V;
                (left ? xl : xr)[y + V * V * c] = (left ? l2 : r2)[q + O * (a + V * f)];
            } else {
                y -= 2 * V * V;
                yy[y + O * V * c] = Y[y + O * V * q];
            }
        } else {
            const int64_t z = x - nimg * W1, c = z / W2;
            int64_t y = z % W2;
            const int64_t i = cols[nimg + c].q, j = cols[nimg + c].r;
            if (y < O * V) bo[y + O * V * c] = ovoo[y + O * V * (j + O * i)];
            else {
                y -= O * V;
                const int64_t f = y % V, a = y / V;
                bt[y + V * V * c] = t2[j + O * (i + O * (a + V * f))];
            }
        }
    }
}

struct IpeaTIn {
    const double *e, *lev;      // the levels of either kind of state (ipea_level)
    const double *l1, *l2;      // the left vector of the state at hand (device)
    const double *oovv, *f_ov;  // <ij||ab>; f(i,a) of a Fock state
    int o, v;
};

// IP: block (x, item) sums  L[a,b] M[a,b] / (e_i + e_j + e_k - e_a - e_b + w)  over its share of a<b; one partial per block.
template <bool FOCK>
__global__ __launch_bounds__(TB) void ipt_contract_ip_kernel(double* __restrict__ partial, const double* __restrict__ Qr, const double* __restrict__ Ql,
                                                             const IpeaTCol* __restrict__ cols, const IpeaTItem* __restrict__ items, IpeaTIn in, double omega)
{
    __shared__ double sm[4];
    const int o = in.o, v = in.v;
    const int64_t O = o, V = v, v2 = V * V;
    const IpeaTItem it = items[blockIdx.y];
    const int col[3] = {it.c0, it.c1, it.c2};
    const IpeaTCol first = cols[it.c0];
    const int i = first.p, j = first.q, k = first.r;
    const double eo = (ipea_level(in.e, in.lev, o, i) + ipea_level(in.e, in.lev, o, j)) + ipea_level(in.e, in.lev, o, k);
    double acc[1] = {0.0};
    for (int64_t x = (int64_t)blockIdx.x * TB + threadIdx.x; x < v2; x += (int64_t)gridDim.x * TB) {
        const int b = (int)(x % V), a = (int)(x / V);
        if (a >= b) continue;
        const int64_t ba = b + V * a, ab = a + V * b;
        double m = 0.0, l = 0.0;
#pragma unroll
        for (int im = 0; im < 3; ++im) {
            const IpeaTCol c = cols[col[im]];
            const double* qr = Qr + v2 * col[im];
            const double* ql = Ql + v2 * col[im];
            double li = (ql[ba] - ql[ab]) + in.l1[c.p] * in.oovv[c.q + O * (c.r + O * ab)];
            if (FOCK)
                li += in.f_ov[c.p + O * a] * in.l2[c.q + O * (c.r + O * b)] - in.f_ov[c.p + O * b] * in.l2[c.q + O * (c.r + O * a)];
            const double mi = qr[ba] - qr[ab];
            if (im == 0) { m = mi; l = li; }
            else { m -= mi; l -= li; }
        }
        const double d = ((eo - ipea_level(in.e, in.lev, o, o + a)) - ipea_level(in.e, in.lev, o, o + b)) + omega;
        acc[0] += l * m / d;
    }
    block_sum<1>(acc, sm);
    if (threadIdx.x == 0) partial[(int64_t)blockIdx.y * gridDim.x + blockIdx.x] = acc[0];
}

// EA: block (x, item) sums  P(l) P(m) / (e_i + e_j - e_a - e_b - e_c + w)  over its share of a<b<c,  P(y) = y(abc) - y(bac) - y(cba); an
// image holds y(abc) at [b,c,a].
template <bool FOCK>
__global__ __launch_bounds__(TB) void ipt_contract_ea_kernel(double* __restrict__ partial, const double* __restrict__ Qr, const double* __restrict__ Ql,
                                                             const IpeaTCol* __restrict__ cols, const IpeaTItem* __restrict__ items, IpeaTIn in, double omega)
{
    __shared__ double sm[4];
    const int o = in.o, v = in.v;
    const int64_t O = o, V = v, v3 = V * V * V;
    const IpeaTItem it = items[blockIdx.y];
    const IpeaTCol first = cols[it.c0];
    const int i = first.p, j = first.q;
    const double *r0 = Qr + v3 * it.c0, *r1 = Qr + v3 * it.c1, *r2 = Qr + v3 * it.c2;
    const double *l0 = Ql + v3 * it.c0, *l1 = Ql + v3 * it.c1, *l2 = Ql + v3 * it.c2;
    const double eo = ipea_level(in.e, in.lev, o, i) + ipea_level(in.e, in.lev, o, j);
    auto mnum = [&](int a, int b, int c) {
        const int64_t y = b + V * (c + V * a);
        return (r0[y] - r1[y]) + r2[y];
    };
    auto lnum = [&](int a, int b, int c) {
        const int64_t y = b + V * (c + V * a);
        double val = ((l0[y] - l1[y]) + l2[y]) + in.l1[a] * in.oovv[i + O * (j + O * (b + V * c))];
        if (FOCK) val += in.f_ov[i + O * a] * in.l2[j + O * (b + V * c)] - in.f_ov[j + O * a] * in.l2[i + O * (b + V * c)];
        return val;
    };
    double acc[1] = {0.0};
    for (int64_t x = (int64_t)blockIdx.x * TB + threadIdx.x; x < v3; x += (int64_t)gridDim.x * TB) {
        const int b = (int)(x % V), c = (int)((x / V) % V), a = (int)(x / (V * V));
        if (!(a < b && b < c)) continue;
        const double pm = (mnum(a, b, c) - mnum(b, a, c)) - mnum(c, b, a);
        const double pl = (lnum(a, b, c) - lnum(b, a, c)) - lnum(c, b, a);
        const double d = (((eo - ipea_level(in.e, in.lev, o, o + a)) - ipea_level(in.e, in.lev, o, o + b)) - ipea_level(in.e, in.lev, o, o + c)) + omega;
        acc[0] += pl * pm / d;
    }
    block_sum<1>(acc, sm);
    if (threadIdx.x == 0) partial[(int64_t)blockIdx.y * gridDim.x + blockIdx.x] = acc[0];
}

// one chunk of items on the host: its columns (images sorted by p, EA: the pair columns behind them), its items, the column range per p
struct IpeaTChunk {
    int64_t col_off = 0, item_off = 0;   // into the uploaded tables
    int64_t ncol = 0, nimg = 0, nitem = 0;
    struct Group { int p; int64_t c0, n; };
    std::vector<Group> groups;           // images only
};

}  // namespace

int64_t so_eom_ipea_t_items(int sector, int o)
{
    if (o < 0) return 0;
    return sector == EOM_SECTOR_IP ? so_triples_count(o) : pair_count(o);
}

void preload_eom_ipea_t_so()
{
    static const bool loaded = [] {
        first_use_touch(reinterpret_cast<const void*>(ipt_build_ip_kernel));
        first_use_touch(reinterpret_cast<const void*>(ipt_build_ea_kernel));
        first_use_touch(reinterpret_cast<const void*>(ipt_contract_ip_kernel<false>));
        first_use_touch(reinterpret_cast<const void*>(ipt_contract_ip_kernel<true>));
        first_use_touch(reinterpret_cast<const void*>(ipt_contract_ea_kernel<false>));
        first_use_touch(reinterpret_cast<const void*>(ipt_contract_ea_kernel<true>));
        (void)hipGetLastError();
        return true;
    }();
    (void)loaded;
}

void so_eom_ipea_triples(Context& cx, SOState& s, int sector, int nstates, const double* omega, const double* l1, const double* l2,
                         const double* r1, const double* r2, int64_t begin, int64_t end, double* delta)
{
    const char* who = "afesp_ccsd_so_eom_ipea_t";
    if (cx.rec) throw Error(1, std::string(who) + ": the EOM-IP/EA triples correction is not part of a recorded (launch-fused) sequence");
    if (!s.ready) throw Error(1, std::string(who) + ": no converged spin-orbital CCSD state in this context");
    if (!so_eom_sector_ok(sector)) throw Error(1, std::string(who) + ": sector is neither 1 (IP) nor 2 (EA)");
    if (nstates < 1 || !omega || !l1 || !l2 || !r1 || !r2 || !delta) throw Error(1, std::string(who) + ": nstates < 1 or a NULL argument");
    so_triples_guard(s, who);
    const bool ip = sector == EOM_SECTOR_IP;
    const int o = s.o, v = s.v;
    const int64_t O = o, V = v, v2 = V * V, v3 = v2 * V;
    for (int st = 0; st < nstates; ++st) delta[st] = 0.0;
    begin = std::max<int64_t>(0, begin);
    end = std::min<int64_t>(so_eom_ipea_t_items(sector, o), end);
    if ((ip ? (o < 3 || v < 2) : (o < 2 || v < 3)) || end <= begin) return;
    preload_eom_ipea_t_so();
    const int64_t n1 = ip ? O : V, n2 = ip ? O * O * V : O * V * V;   // the sector's vector
    const int64_t tile = ip ? v2 : v3;                              // one image

    // ---- chunking: the doubles an item costs (three image tiles per side and the gathered columns) against the (T) pool budget
    const int64_t per_item = ip ? 3 * (2 * tile + 2 * V + O + O * V + v2) : 6 * tile + 2 * (2 * v2 + O * V) + (O * V + v2);
    // (an item is a row of the contraction kernels' grids: at most 65535 of them)
    const int64_t nb = std::max<int64_t>(1, std::min<int64_t>({end - begin, device_pool_budget() / (8 * per_item), (int64_t)65535}));
    // the resident operands, the state's vectors and intermediates
    const int64_t fixed = O * v3 + O * O * v2 + 2 * (n1 + n2) + (ip ? 2 * O * O * V + V * V * O + O * O * O : v3 + O * V * O);
    {
        // (scratch that does not fit is refused before anything is allocated; buffers this size from an earlier call are there already)
        auto have = [&](const char* name, int64_t n) {
            auto it = cx.cache.find(name);
            return it != cx.cache.end() && it->second.second >= (size_t)n * sizeof(double);
        };
        const bool cached = have("ipt_qr", 3 * nb * tile) && have("ipt_ql", 3 * nb * tile) && have("ipt_vp", O * v3);
        if (!cached && !cx.fits(8.0 * ((double)nb * (double)per_item + (double)fixed)))
            throw Error(1, std::string(who) + ": the image buffers of a chunk do not fit the free device memory (lower AFESP_T_POOL_GIB)");
    }

    // ---- the tables of every chunk
    std::vector<IpeaTCol> hcols;
    std::vector<IpeaTItem> hitems;
    std::vector<IpeaTChunk> chunks;
    {
        std::vector<IpeaTCol> its;   // the items of the range as (i, j, k) / (i, j)
        if (ip) {
            int64_t t = 0;
            for (int i = 0; i < o && t < end; ++i)
                for (int j = i + 1; j < o && t < end; ++j)
                    for (int k = j + 1; k < o && t < end; ++k, ++t)
                        if (t >= begin) its.push_back({i, j, k, 0});
        } else {
            int64_t t = 0;
            for (int j = 1; j < o && t < end; ++j)
                for (int i = 0; i < j && t < end; ++i, ++t)
                    if (t >= begin) its.push_back({i, j, -1, 0});
        }
        if ((int64_t)its.size() != end - begin) throw Error(2, std::string(who) + ": item enumeration");
        for (int64_t t0 = 0; t0 < end - begin; t0 += nb) {
            IpeaTChunk ch;
            ch.col_off = (int64_t)hcols.size();
            ch.item_off = (int64_t)hitems.size();
            ch.nitem = std::min<int64_t>(nb, end - begin - t0);
            ch.nimg = (ip ? 3 : 2) * ch.nitem;
            ch.ncol = 3 * ch.nitem;
            // images with the item and the slot they belong to, sorted by p (stable: the order inside a p is the items')
            struct Img { IpeaTCol c; int64_t item; int slot; };
            std::vector<Img> imgs;
            for (int64_t t = 0; t < ch.nitem; ++t) {
                const IpeaTCol x = its[(size_t)(t0 + t)];
                if (ip) {
                    imgs.push_back({{x.p, x.q, x.r, 0}, t, 0});
                    imgs.push_back({{x.q, x.p, x.r, 0}, t, 1});
                    imgs.push_back({{x.r, x.q, x.p, 0}, t, 2});
                } else {
                    imgs.push_back({{x.p, x.q, -1, 0}, t, 0});
                    imgs.push_back({{x.q, x.p, -1, 0}, t, 1});
                }
            }
            std::stable_sort(imgs.begin(), imgs.end(), [](const Img& a, const Img& b) { return a.c.p < b.c.p; });
            std::vector<IpeaTItem> itab((size_t)ch.nitem, IpeaTItem{0, 0, 0, 0});
            for (int64_t c = 0; c < (int64_t)imgs.size(); ++c) {
                const Img& im = imgs[(size_t)c];
                hcols.push_back(im.c);
                (im.slot == 0 ? itab[(size_t)im.item].c0 : im.slot == 1 ? itab[(size_t)im.item].c1 : itab[(size_t)im.item].c2) = (int)c;
                if (ch.groups.empty() || ch.groups.back().p != im.c.p) ch.groups.push_back({im.c.p, c, 0});
                ++ch.groups.back().n;
            }
            if (!ip)
                for (int64_t t = 0; t < ch.nitem; ++t) {
                    const IpeaTCol x = its[(size_t)(t0 + t)];
                    hcols.push_back({o, x.p, x.q, 0});
                    itab[(size_t)t].c2 = (int)(ch.nimg + t);
                }
            hitems.insert(hitems.end(), itab.begin(), itab.end());
            chunks.push_back(std::move(ch));
        }
    }

    // ---- every cached buffer first (a buffer that grows bumps the scratch epoch)
    double* Qr = cx.scratch("ipt_qr", 3 * nb * tile);
    double* Ql = cx.scratch("ipt_ql", 3 * nb * tile);
    const int64_t nimg_max = (ip ? 3 : 2) * nb;
    double* xr = cx.scratch("ipt_xr", nimg_max * (ip ? V : v2));
    double* xl = cx.scratch("ipt_xl", nimg_max * (ip ? V : v2));
    double* yy = cx.scratch("ipt_yy", nimg_max * (ip ? O : O * V));
    double* bo = cx.scratch("ipt_bo", (ip ? 3 : 1) * nb * O * V);
    double* bt = cx.scratch("ipt_bt", (ip ? 3 : 1) * nb * v2);
    const int nblk = (int)std::max<int64_t>(1, std::min<int64_t>((tile + TB - 1) / TB, 64));   // blocks per item of a contraction kernel
    double* partial = cx.scratch("ipt_partial", std::max<int64_t>(nblk * nb, 512));
    double* sum_tmp = cx.scratch("ipt_sum_tmp", 128);
    IpeaTCol* dcols = (IpeaTCol*)cx.scratch("ipt_cols", (int64_t)hcols.size() * 2 + 2);
    IpeaTItem* ditems = (IpeaTItem*)cx.scratch("ipt_items", (int64_t)hitems.size() * 2 + 2);
    Tensor Vp = view(cx.scratch("ipt_vp", O * v3), {V, V, V, O});       // Vp(f,b,c;p) = <fp||bc>
    Tensor Tp = view(cx.scratch("ipt_tp", O * O * v2), {O, V, V, O});   // Tp(m,a,b;p) = t2(m,p,a,b)
    double* dl = cx.scratch("ipt_l", n1 + n2);
    double* dr = cx.scratch("ipt_r", n1 + n2);
    // IP: the vectors' doubles with p last, U(f,b;p), Y(m,q,r).  EA: U(f,b,c), Y(m,a,r)
    Tensor Xrp, Xlp, U, Y;
    if (ip) {
        Xrp = view(cx.scratch("ipt_xrp", O * O * V), {O, V, O});
        Xlp = view(cx.scratch("ipt_xlp", O * O * V), {O, V, O});
        U = view(cx.scratch("ipt_u", v2 * O), {V, V, O});
        Y = view(cx.scratch("ipt_y", O * O * O), {O, O, O});
    } else {
        U = view(cx.scratch("ipt_u", v3), {V, V, V});
        Y = view(cx.scratch("ipt_y", O * V * O), {O, V, O});
    }
    AFESP_HIP(hipMemcpyAsync(dcols, hcols.data(), hcols.size() * sizeof(IpeaTCol), hipMemcpyHostToDevice, cx.stream));
    AFESP_HIP(hipMemcpyAsync(ditems, hitems.data(), hitems.size() * sizeof(IpeaTItem), hipMemcpyHostToDevice, cx.stream));
    cx.sync();   // the host tables may die with an exception below

    const auto C = contractor(cx);
    permute_add(cx, 1.0, s.vovv, "fpbc", 0.0, Vp, "fbcp");
    permute_add(cx, 1.0, s.t2, "mpab", 0.0, Tp, "mabp");
    const Tensor r1d = view(dr, {n1});
    const Tensor l2d = ip ? view(dl + n1, {O, O, V}) : view(dl + n1, {O, V, V});
    const Tensor r2d = ip ? view(dr + n1, {O, O, V}) : view(dr + n1, {O, V, V});
    const IpeaTIn in{s.e, s.lev, dl, dl + n1, s.oovv.d, s.fock ? s.f_ov.d : nullptr, o, v};

    SOStamps prof(cx);   // afesp_profile: the build kernel and the products as the GEMM part, the contraction kernel as the orbit pass
    for (int st = 0; st < nstates; ++st) {
        AFESP_HIP(hipMemcpyAsync(dl, l1 + st * n1, sizeof(double) * n1, hipMemcpyHostToDevice, cx.stream));
        AFESP_HIP(hipMemcpyAsync(dl + n1, l2 + st * n2, sizeof(double) * n2, hipMemcpyHostToDevice, cx.stream));
        AFESP_HIP(hipMemcpyAsync(dr, r1 + st * n1, sizeof(double) * n1, hipMemcpyHostToDevice, cx.stream));
        AFESP_HIP(hipMemcpyAsync(dr + n1, r2 + st * n2, sizeof(double) * n2, hipMemcpyHostToDevice, cx.stream));
        if (ip) {
            permute_add(cx, 1.0, r2d, "mpb", 0.0, Xrp, "mbp");
            permute_add(cx, 1.0, l2d, "mpb", 0.0, Xlp, "mbp");
            // U_fpb = sum_l r_l <fp||bl>  (<fp||bl> = -<pf||bl>),   Y_mqr = sum_l r_l <ml||qr>
            C(-1.0, s.ovvo, "pfbl", r1d, "l", 0.0, U, "fbp");
            C(1.0, s.oooo, "mlqr", r1d, "l", 0.0, Y, "mqr");
        } else {
            // U_fbc = sum_d <fd||bc> r_d,   Y_mar = sum_d <ma||dr> r_d
            C(1.0, s.vvvv, "fdbc", r1d, "d", 0.0, U, "fbc");
            C(1.0, s.ovvo, "madr", r1d, "d", 0.0, Y, "mar");
        }
        k_fill(cx, cx.scal, 1, 0.0);
        for (const IpeaTChunk& ch : chunks) {
            const IpeaTCol* cols = dcols + ch.col_off;
            const IpeaTItem* items = ditems + ch.item_off;
            prof.stamp();
            if (ip) {
                LAUNCH(ipt_build_ip_kernel, grid_for(ch.ncol * (2 * V + O + O * V + v2)), xr, xl, yy, bo, bt, cols, ch.ncol, r2d.d, l2d.d, Y.d, s.ovoo.d,
                       s.t2.d, o, v);
                for (const IpeaTChunk::Group& g : ch.groups) {
                    const int64_t p = g.p, c0 = g.c0, n = g.n;
                    const Tensor Vs = view(Vp.d + p * v3, {V, V, V}), Ts = view(Tp.d + p * O * v2, {O, V, V});
                    const Tensor Xr = view(Xrp.d + p * O * V, {O, V}), Xl = view(Xlp.d + p * O * V, {O, V}), Us = view(U.d + p * v2, {V, V});
                    const Tensor qr = view(Qr + c0 * v2, {V, V, n}), ql = view(Ql + c0 * v2, {V, V, n});
                    const Tensor bxr = view(xr + c0 * V, {V, n}), bxl = view(xl + c0 * V, {V, n}), byy = view(yy + c0 * O, {O, n});
                    const Tensor bbo = view(bo + c0 * O * V, {O, V, n}), bbt = view(bt + c0 * v2, {V, V, n});
                    C(0.5, Vs, "fba", bxr, "fx", 0.0, qr, "bax");
                    C(-0.5, Ts, "mab", byy, "mx", 1.0, qr, "bax");
                    C(1.0, Xr, "mb", bbo, "max", 1.0, qr, "bax");
                    C(-1.0, Us, "fb", bbt, "fax", 1.0, qr, "bax");
                    C(0.5, Vs, "fba", bxl, "fx", 0.0, ql, "bax");
                    C(1.0, Xl, "mb", bbo, "max", 1.0, ql, "bax");
                }
                prof.stamp();
                if (s.fock) LAUNCH((ipt_contract_ip_kernel<true>), dim3(nblk, (unsigned)ch.nitem), partial, Qr, Ql, cols, items, in, omega[st]);
                else LAUNCH((ipt_contract_ip_kernel<false>), dim3(nblk, (unsigned)ch.nitem), partial, Qr, Ql, cols, items, in, omega[st]);
            } else {
                LAUNCH(ipt_build_ea_kernel, grid_for(ch.nimg * (2 * v2 + O * V) + ch.nitem * (O * V + v2)), xr, xl, yy, bo, bt, cols, ch.nimg, ch.nitem,
                       r2d.d, l2d.d, Y.d, s.ovoo.d, s.t2.d, o, v);
                for (const IpeaTChunk::Group& g : ch.groups) {
                    const int64_t p = g.p, c0 = g.c0, n = g.n;
                    const Tensor Vs = view(Vp.d + p * v3, {V, V, V}), Ts = view(Tp.d + p * O * v2, {O, V, V});
                    const Tensor qr = view(Qr + c0 * v3, {V, V, V, n}), ql = view(Ql + c0 * v3, {V, V, V, n});
                    const Tensor bxr = view(xr + c0 * v2, {V, V, n}), bxl = view(xl + c0 * v2, {V, V, n}), byy = view(yy + c0 * O * V, {O, V, n});
                    C(1.0, Vs, "fbc", bxr, "fax", 0.0, qr, "bcax");
                    C(1.0, Ts, "mcb", byy, "max", 1.0, qr, "bcax");
                    C(1.0, Vs, "fbc", bxl, "fax", 0.0, ql, "bcax");
                }
                {
                    const int64_t n = ch.nitem;
                    const Tensor qr = view(Qr + ch.nimg * v3, {V, V, V, n}), ql = view(Ql + ch.nimg * v3, {V, V, V, n});
                    const Tensor bbo = view(bo, {O, V, n}), bbt = view(bt, {V, V, n});
                    C(1.0, r2d, "mcb", bbo, "max", 0.0, qr, "bcax");
                    C(-1.0, U, "fbc", bbt, "fax", 1.0, qr, "bcax");
                    C(1.0, l2d, "mcb", bbo, "max", 0.0, ql, "bcax");
                }
                prof.stamp();
                if (s.fock) LAUNCH((ipt_contract_ea_kernel<true>), dim3(nblk, (unsigned)ch.nitem), partial, Qr, Ql, cols, items, in, omega[st]);
                else LAUNCH((ipt_contract_ea_kernel<false>), dim3(nblk, (unsigned)ch.nitem), partial, Qr, Ql, cols, items, in, omega[st]);
            }
            prof.stamp();
            sum_partials(cx, cx.scal, partial, 1, (int)(nblk * ch.nitem), sum_tmp);
        }
        delta[st] = host_scalars(cx, 1)[0];   // (synchronises: the next state's uploads overwrite ipt_l / ipt_r after this state's readers)
    }
    prof.read();
    if (knobs().t_debug)
        fprintf(stderr, "afesp EOM-%s-(T): o %d v %d states %d items %lld per chunk %lld chunks %zu\n", ip ? "IP" : "EA", o, v, nstates,
                (long long)(end - begin), (long long)nb, chunks.size());
}

}  // namespace afesp
