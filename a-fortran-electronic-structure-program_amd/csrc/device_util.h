// device_util.h -- the device helpers every kernel unit shares, written once: the block size, grid size and grid-stride loop of the
// element-wise kernels; the fixed-order block sums (block_sum over wave_sum, block_sum_down, block_tree_sum: two orders of the wave sum, see
// block_sum_down); the triangular pair indices and their inverses (tri / unpair for x <= y, pair_count / unpair_lt for x < y); the decode of
// an (o, o, v, v) element with its three images; the reduction partials of a context and the LAUNCH macro.  Everything has internal linkage
// (an unnamed namespace per unit); no __global__ function lives here.
#pragma once
#include <algorithm>

#include "afesp_internal.h"

namespace afesp {

namespace {
constexpr int TB = 256;
// the grid cap of the spin-orbital CCSD, Lambda, two-particle-density and relaxation maps (beside grid_for's own 4096): where a kernel
// leaves block partials, the cap decides how they are grouped
constexpr int SO_GRID_CAP = 65536;
inline unsigned grid_for(int64_t n, int cap = 4096) { return (unsigned)std::max<int64_t>(1, std::min<int64_t>((n + TB - 1) / TB, cap)); }
#define GRID_STRIDE(IDX_, n) for (int64_t IDX_ = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; IDX_ < (n); IDX_ += (int64_t)gridDim.x * blockDim.x)

// Sum over the 64 lanes of a wave, the same value in every lane, in a fixed order (bit-reproducible).  Four butterfly steps inside
// each row of 16 lanes as DPP moves (one VALU instruction per 32-bit half; a __shfl is a ds_bpermute plus ~8 instructions of lane
// arithmetic -- eighteen sums of a block reduction were ~2000 instructions per wave), then the four row sums through v_readlane.
template <int CTRL>
__device__ __forceinline__ double dpp_permuted(double v)
{
    const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), CTRL, 0xf, 0xf, true);
    const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), CTRL, 0xf, 0xf, true);
    return __hiloint2double(hi, lo);
}
__device__ __forceinline__ double lane_value(double v, int from)   // `from` uniform: the value lands in scalar registers
{
    const int lo = __builtin_amdgcn_readlane(__double2loint(v), from), hi = __builtin_amdgcn_readlane(__double2hiint(v), from);
    return __hiloint2double(hi, lo);
}
__device__ __forceinline__ double wave_sum(double v)
{
    v += dpp_permuted<0xB1>(v);    // quad_perm [1,0,3,2]
    v += dpp_permuted<0x4E>(v);    // quad_perm [2,3,0,1]
    v += dpp_permuted<0x141>(v);   // row_half_mirror
    v += dpp_permuted<0x140>(v);   // row_mirror: every lane of a row holds the row's sum
    return ((lane_value(v, 0) + lane_value(v, 16)) + lane_value(v, 32)) + lane_value(v, 48);
}
// block-wide sum of up to NV values; result valid in thread 0
template <int NV>
__device__ __forceinline__ void block_sum(double (&v)[NV], double* sm /* [NV*4] */)
{
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
    for (int q = 0; q < NV; ++q) {
        v[q] = wave_sum(v[q]);
        if (lane == 0) sm[q * 4 + w] = v[q];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int q = 0; q < NV; ++q) v[q] = sm[q * 4] + sm[q * 4 + 1] + sm[q * 4 + 2] + sm[q * 4 + 3];
    }
}

// The same block-wide sum in the order of the CCSD, Lambda and two-particle-density energies: a __shfl_down tree over each wave, then the
// four wave values added 0, 1, 2, 3 by thread 0.  The two trees pair the lanes differently, so the last bit of a sum differs between
// them: a kernel stays with the order its published numbers were made in (block_sum: the Davidson, EOM, response and Z-vector
// reductions).  Result valid in thread 0.
template <int NV>
__device__ __forceinline__ void block_sum_down(double (&v)[NV], double* sm /* [NV*4] */)
{
    for (int off = 32; off > 0; off >>= 1) {
#pragma unroll
        for (int q = 0; q < NV; ++q) v[q] += __shfl_down(v[q], off, 64);
    }
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int q = 0; q < NV; ++q) sm[q * 4 + (threadIdx.x >> 6)] = v[q];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int q = 0; q < NV; ++q) v[q] = 0.0;
        for (int w = 0; w < TB / 64; ++w) {
#pragma unroll
            for (int q = 0; q < NV; ++q) v[q] += sm[q * 4 + w];
        }
    }
}
// the sum of one value per thread through a halving tree in LDS (the ordered final sum of block partials) -> red[0], for every thread
__device__ __forceinline__ void block_tree_sum(double s, double (&red)[TB])
{
    red[threadIdx.x] = s;
    __syncthreads();
    for (int w = TB / 2; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
        __syncthreads();
    }
}

__device__ __forceinline__ int64_t tri(int64_t i, int64_t j) { return i >= j ? i * (i + 1) / 2 + j : j * (j + 1) / 2 + i; }
// where (pq|rs) lies in the 8-fold packed array, for the four indices in any order (the one place that canonicalises them)
__device__ __forceinline__ int64_t packed_index(int64_t p, int64_t q, int64_t r, int64_t s) { return tri(tri(p, q), tri(r, s)); }
// pair index of x <= y: y(y+1)/2 + x; inverse of it (the 64-bit form: a pair of pairs -- neri(1024) = 1.4e11 -- or indices used as such)
__device__ __forceinline__ void unpair(int64_t p, int64_t& lo, int64_t& hi)
{
    int64_t h = (int64_t)((sqrt(8.0 * (double)p + 1.0) - 1.0) * 0.5);
    while (h * (h + 1) / 2 > p) --h;
    while ((h + 1) * (h + 2) / 2 <= p) ++h;
    hi = h;
    lo = p - h * (h + 1) / 2;
}
__device__ __forceinline__ void unpair(int64_t p, int& lo, int& hi)
{
    int64_t l, h;
    unpair(p, l, h);
    hi = (int)h;
    lo = (int)l;
}
// pairs x < y are numbered y(y-1)/2 + x: how many of n indices, and the inverse
__host__ __device__ inline int64_t pair_count(int64_t n) { return n * (n - 1) / 2; }
__device__ __forceinline__ void unpair_lt(int64_t p, int& lo, int& hi)
{
    int64_t h = (int64_t)((1.0 + sqrt(1.0 + 8.0 * (double)p)) * 0.5);
    while (h * (h - 1) / 2 > p) --h;
    while ((h + 1) * h / 2 <= p) ++h;
    hi = (int)h;
    lo = (int)(p - h * (h - 1) / 2);
}

// element x = i + o (j + o (a + v b)) of an (o, o, v, v) array: `const auto [i, j, a, b] = oovv_decode(x, o, v);` ...
struct OOVV { int i, j, a, b; };
__device__ __forceinline__ OOVV oovv_decode(int64_t x, int o, int v)
{
    return {(int)(x % o), (int)((x / o) % o), (int)((x / ((int64_t)o * o)) % v), (int)(x / ((int64_t)o * o * v))};
}
// ... and where its images under i <-> j, under a <-> b and under both lie: `const auto [ji, ba, jiba] = oovv_images(i, j, a, b, o, v);`
struct OOVVImages { int64_t ji, ba, jiba; };
__device__ __forceinline__ OOVVImages oovv_images(int i, int j, int a, int b, int o, int v)
{
    return {j + (int64_t)o * (i + (int64_t)o * (a + (int64_t)v * b)), i + (int64_t)o * (j + (int64_t)o * (b + (int64_t)v * a)),
            j + (int64_t)o * (i + (int64_t)o * (b + (int64_t)v * a))};
}

// the fixed grid of the deterministic reductions: per-block partials, ordered final sum (k_final_sum)
constexpr int RED_BLOCKS = 512;
// partial sums live at cx.scal + 64 (2*RED_BLOCKS doubles reserved by the context)
inline double* partials(Context& cx) { return cx.scal + 64; }
}  // namespace

#define LAUNCH(kernel, grid, ...)                                               \
    do {                                                                        \
        AFESP_KLAUNCH(kernel, grid, dim3(TB), 0, cx.stream, __VA_ARGS__);  \
        AFESP_HIP(hipGetLastError());                                           \
    } while (0)

}  // namespace afesp
