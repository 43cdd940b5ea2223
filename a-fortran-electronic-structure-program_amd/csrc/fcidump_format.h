// fcidump_format.h -- host side of the active-space FCIDUMP writer (afesp_write_fcidump_active / _uactive): the inverse
// of the flat packed index, the spin-orbital numbering and the text formatting.  Plain C++ with no GPU call, so that it also builds into
// the stand-alone check program tools/fcidump_format_check.cpp (run under the address and undefined-behaviour sanitizers).
//
// File: a namelist header (&FCI NORB=,NELEC=,MS2=, / ORBSYM=1,...,1, / ISYM=1, [/ UHF=.TRUE.,] / &END), then one line per number,
// "value i j k l": the value as %23.15E, four blank-separated 1-based indices in chemists' notation (ij|kl); two-electron lines in the
// canonical order of the packed array, then h(i,j) i j 0 0 for i >= j, last the core energy with four zeros.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <string>
#include <thread>
#include <vector>

namespace afesp {
namespace fcidump {

enum Block { SPATIAL = 0, ALPHA_ALPHA = 1, BETA_BETA = 2, ALPHA_BETA = 3 };
constexpr int MAX_THREADS = 16;
constexpr int64_t SLAB = (int64_t)1 << 16;   // lines one thread formats per round
constexpr int LINE_BYTES = 64;                 // bytes of one line at most (23 + 4 x (1 + 10) + newline)

// x = hi (hi + 1) / 2 + lo with lo <= hi (0-based)
inline void unpair(int64_t x, int64_t& hi, int64_t& lo)
{
    int64_t h = (int64_t)((std::sqrt(8.0 * (double)x + 1.0) - 1.0) * 0.5);
    while (h * (h + 1) / 2 > x) --h;
    while ((h + 1) * (h + 2) / 2 <= x) ++h;
    hi = h;
    lo = x - h * (h + 1) / 2;
}
// flat index -> spatial (p, q, r, s), 0-based, p >= q, r >= s.  np == 0: the 8-fold packed array, x = PQ (PQ + 1) / 2 + RS;
// np > 0: the npair x npair alpha-beta block, x = PQ np + RS
inline void unflatten(int64_t x, int64_t np, int64_t out[4])
{
    int64_t pq, rs;
    if (np > 0) {
        pq = x / np;
        rs = x % np;
    } else {
        unpair(x, pq, rs);
    }
    unpair(pq, out[0], out[1]);
    unpair(rs, out[2], out[3]);
}
// the number written for 0-based spatial orbital p: p + 1, or the interleaved spin orbital 2p + 1 (alpha) / 2p + 2 (beta)
inline int64_t label(int64_t p, bool spin, bool beta) { return spin ? 2 * p + (beta ? 2 : 1) : p + 1; }
inline int format_line(char* dst, double value, int64_t i, int64_t j, int64_t k, int64_t l)
{
    return std::snprintf(dst, LINE_BYTES, "%23.15E %4lld %4lld %4lld %4lld\n", value, (long long)i, (long long)j, (long long)k, (long long)l);
}
inline int format_two_electron(char* dst, Block b, int64_t np, int64_t flat, double value)
{
    int64_t o[4];
    unflatten(flat, b == ALPHA_BETA ? np : 0, o);
    const bool spin = b != SPATIAL;
    return format_line(dst, value, label(o[0], spin, b == BETA_BETA), label(o[1], spin, b == BETA_BETA),
                       label(o[2], spin, b == BETA_BETA || b == ALPHA_BETA), label(o[3], spin, b == BETA_BETA || b == ALPHA_BETA));
}

inline int thread_count(int64_t lines)
{
    const unsigned hw = std::thread::hardware_concurrency();
    const int64_t want = (lines + SLAB - 1) / SLAB;
    int64_t t = hw ? (int64_t)hw : 1;
    if (t > MAX_THREADS) t = MAX_THREADS;
    if (t > want) t = want;
    return t < 1 ? 1 : (int)t;
}

// The `count` two-electron lines of the (flat index, value) pairs, in their order.  Rounds of nthreads slabs: every thread formats its
// slab into a buffer of its own, the buffers go to the file in slab order -- the bytes do not depend on the number of threads.
inline bool write_two_electron(FILE* f, Block b, int64_t np, const int64_t* flat, const double* value, int64_t count, int nthreads)
{
    if (nthreads < 1) nthreads = 1;
    std::vector<std::vector<char>> buf((size_t)nthreads);
    std::vector<size_t> used((size_t)nthreads, 0);
    auto work = [&](int t, int64_t lo, int64_t hi) {
        std::vector<char>& mine = buf[(size_t)t];
        mine.resize((size_t)(hi - lo) * LINE_BYTES);
        size_t at = 0;
        for (int64_t x = lo; x < hi; ++x) at += (size_t)format_two_electron(mine.data() + at, b, np, flat[x], value[x]);
        used[(size_t)t] = at;
    };
    for (int64_t base = 0; base < count; base += SLAB * nthreads) {
        std::vector<std::thread> pool;
        int active = 0;
        for (int t = 0; t < nthreads; ++t) {
            const int64_t lo = base + SLAB * t, hi = lo + SLAB < count ? lo + SLAB : count;
            if (lo >= count) break;
            ++active;
            if (t > 0) pool.emplace_back(work, t, lo, hi);
        }
        work(0, base, base + SLAB < count ? base + SLAB : count);
        for (std::thread& th : pool) th.join();
        for (int t = 0; t < active; ++t)
            if (std::fwrite(buf[(size_t)t].data(), 1, used[(size_t)t], f) != used[(size_t)t]) return false;
    }
    return true;
}

// h(i,j) i j 0 0 for i >= j, |h| > threshold; h: n x n column-major.  Returns the number of lines, -1 if the file refused them.
inline int64_t write_one_electron(FILE* f, const double* h, int64_t n, double threshold, bool spin, bool beta)
{
    char line[LINE_BYTES];
    int64_t lines = 0;
    for (int64_t i = 0; i < n; ++i)
        for (int64_t j = 0; j <= i; ++j) {
            const double x = h[i + n * j];
            if (!(std::fabs(x) > threshold)) continue;
            const int len = format_line(line, x, label(i, spin, beta), label(j, spin, beta), 0, 0);
            if (std::fwrite(line, 1, (size_t)len, f) != (size_t)len) return -1;
            ++lines;
        }
    return lines;
}

inline bool write_core_energy(FILE* f, double e_core_total)
{
    char line[LINE_BYTES];
    const int len = format_line(line, e_core_total, 0, 0, 0, 0);
    return std::fwrite(line, 1, (size_t)len, f) == (size_t)len;
}

inline bool write_header(FILE* f, int64_t norb, int64_t nelec, int64_t ms2, bool uhf)
{
    std::string s = " &FCI NORB=" + std::to_string(norb) + ",NELEC=" + std::to_string(nelec) + ",MS2=" + std::to_string(ms2) + ",\n  ORBSYM=";
    for (int64_t i = 0; i < norb; ++i) s += "1,";
    s += "\n  ISYM=1,\n";
    if (uhf) s += "  UHF=.TRUE.,\n";
    s += " &END\n";
    return std::fwrite(s.data(), 1, s.size(), f) == s.size();
}

}  // namespace fcidump
}  // namespace afesp
