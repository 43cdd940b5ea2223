// fcidump_format_check -- stand-alone check of the host side of the active-space FCIDUMP writer (csrc/fcidump_format.h: index inversion,
// spin-orbital numbering, chunked formatting).  No GPU call; meant to be built with the sanitizers and run on the CPU:
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -pthread tools/fcidump_format_check.cpp \
//       -o tools/fcidump_format_check_bin && tools/fcidump_format_check_bin [n] [directory for the scratch files]
// Every flat index of the packed array over n orbitals (default 100: four-digit spin-orbital numbers, three-digit spatial ones) goes
// through the inversion and back; a sample of lines is formatted on 1, 3 and 16 threads, the files must be the same bytes and every line
// must parse back to its index and value.  Exit status 0 and "ok" on success.
#include <cinttypes>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <sstream>

#include "../a-fortran-electronic-structure-program_amd/csrc/fcidump_format.h"

using namespace afesp::fcidump;

static int64_t tri(int64_t a, int64_t b) { return a >= b ? a * (a + 1) / 2 + b : b * (b + 1) / 2 + a; }
static int fail(const std::string& what)
{
    std::cerr << "FAILED: " << what << "\n";
    return 1;
}
static std::string slurp(const std::string& path)
{
    std::ifstream in(path, std::ios::binary);
    std::ostringstream ss;
    ss << in.rdbuf();
    return ss.str();
}

int main(int argc, char** argv)
{
    const int64_t n = argc > 1 ? std::atoll(argv[1]) : 100;
    const std::string dir = argc > 2 ? argv[2] : ".";
    const int64_t np = n * (n + 1) / 2, total = np * (np + 1) / 2;
    // 1. the inversion of every flat index, packed and alpha-beta (the latter on a stride: np^2 of them)
    int64_t largest = 0;
    for (int64_t x = 0; x < total; ++x) {
        int64_t o[4];
        unflatten(x, 0, o);
        if (!(o[0] >= o[1] && o[2] >= o[3] && o[0] < n && o[1] >= 0 && o[3] >= 0) || tri(o[0], o[1]) < tri(o[2], o[3]) ||
            tri(tri(o[0], o[1]), tri(o[2], o[3])) != x)
            return fail("packed inversion at " + std::to_string(x));
        if (o[0] + 1 > largest) largest = o[0] + 1;
    }
    if (largest != n) return fail("largest orbital");
    for (int64_t x = 0; x < np * np; x += 7) {
        int64_t o[4];
        unflatten(x, np, o);
        if (!(o[0] >= o[1] && o[2] >= o[3] && o[0] < n && o[2] < n) || tri(o[0], o[1]) * np + tri(o[2], o[3]) != x)
            return fail("pair-matrix inversion at " + std::to_string(x));
    }
    // 2. a sample of survivors (every 11th element, the first and the last: more than one round of 16 slabs
    std::vector<int64_t> flat;
    std::vector<double> value;
    for (int64_t x = 0; x < total; x += 11) flat.push_back(x);
    if (flat.back() != total - 1) flat.push_back(total - 1);
    for (size_t k = 0; k < flat.size(); ++k) value.push_back((k % 2 ? -1.0 : 1.0) * std::ldexp(1.0 + 1e-3 * (double)(k % 997), (int)(k % 600) - 300));
    const Block blocks[4] = {SPATIAL, ALPHA_ALPHA, BETA_BETA, ALPHA_BETA};
    for (Block b : blocks) {
        std::string first;
        for (int threads : {1, 3, 16}) {
            const std::string path = dir + "/fcidump_format_check." + std::to_string((int)b) + "." + std::to_string(threads);
            FILE* f = std::fopen(path.c_str(), "w");
            if (!f) return fail("cannot open " + path);
            std::vector<int64_t> use = flat;
            if (b == ALPHA_BETA)
                for (int64_t& x : use) x = (x * 2) % (np * np);   // (any index of the square block; order is the caller's)
            std::vector<double> h((size_t)(n * n));
            for (int64_t i = 0; i < n; ++i)
                for (int64_t j = 0; j < n; ++j) h[(size_t)(i + n * j)] = (i + j) % 3 ? 0.25 * (double)(i + j + 1) : 0.0;
            bool ok = write_header(f, b == SPATIAL ? n : 2 * n, 10, b == SPATIAL ? 0 : 2, b != SPATIAL);
            ok = ok && write_two_electron(f, b, np, use.data(), value.data(), (int64_t)use.size(), threads);
            const int64_t one = write_one_electron(f, h.data(), n, 0.0, b != SPATIAL, b == BETA_BETA);
            ok = ok && one >= 0 && write_core_energy(f, -76.0);
            if (std::fclose(f) != 0 || !ok) return fail("write " + path);
            const std::string bytes = slurp(path);
            std::remove(path.c_str());
            if (threads == 1) first = bytes;
            else if (bytes != first) return fail("the file depends on the number of threads, block " + std::to_string((int)b));
            if (threads != 16) continue;
            // parse back
            std::istringstream in(bytes);
            std::string line;
            while (std::getline(in, line) && line.find("&END") == std::string::npos) {}
            int64_t two = 0, ones = 0, biggest = 0;
            while (std::getline(in, line)) {
                double v;
                long long i, j, k, l;
                char extra;
                if (std::sscanf(line.c_str(), "%lf %lld %lld %lld %lld %c", &v, &i, &j, &k, &l, &extra) != 5) return fail("line does not split into five fields: " + line);
                for (long long q : {i, j, k, l}) biggest = q > biggest ? q : biggest;
                if (k == 0) { ++ones; continue; }
                if (two >= (int64_t)use.size()) return fail("too many two-electron lines");
                int64_t o[4];
                unflatten(use[(size_t)two], b == ALPHA_BETA ? np : 0, o);
                const bool spin = b != SPATIAL, b12 = b == BETA_BETA, b34 = b == BETA_BETA || b == ALPHA_BETA;
                if (i != label(o[0], spin, b12) || j != label(o[1], spin, b12) || k != label(o[2], spin, b34) || l != label(o[3], spin, b34) ||
                    std::fabs(v - value[(size_t)two]) > 2e-15 * std::fabs(value[(size_t)two]))   // (16 significant digits are written)
                    return fail("line " + std::to_string(two) + " of block " + std::to_string((int)b) + ": " + line);
                ++two;
            }
            if (two != (int64_t)use.size() || ones != one + 1) return fail("line counts");
            if (b == SPATIAL && biggest != n) return fail("largest index read back");
        }
    }
    std::printf("ok: n = %" PRId64 ", %" PRId64 " packed indices inverted, %zu lines per block on 1, 3 and 16 threads\n", n, total, flat.size());
    return 0;
}
