// fcidump_parse_check.cpp -- the host half of the FCIDUMP reader (csrc/fcidump_parse.h) as a stand-alone program: read_header and
// read_body -- the very chunk loop, carried-over tail, threaded block parser and per-record checks that csrc/integrals.hip calls -- with
// a host map in place of the device scatter (slot -> bits; a duplicate that disagrees is an error).  No GPU call: build it with the address and
// undefined-behaviour sanitizers and feed it good and malformed files:
//   clang++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -pthread tools/fcidump_parse_check.cpp -o fcidump_parse_check
//   ./fcidump_parse_check FILE [CHUNK_BYTES [THREADS]]      prints "ok ..." (exit 0) or "refused: line N: why" (exit 1)
#include <cstdio>
#include <cstring>
#include <map>
#include <string>
#include <tuple>
#include <vector>

#include "../a-fortran-electronic-structure-program_amd/csrc/fcidump_parse.h"

using namespace afesp::fcidump;

static int64_t tri(int64_t i, int64_t j) { return i >= j ? i * (i + 1) / 2 + j : j * (j + 1) / 2 + i; }

int main(int argc, char** argv)
{
    if (argc < 2) return 2;
    const size_t chunk = argc > 2 ? (size_t)std::atoll(argv[2]) : (size_t)4 << 20;
    const int threads = argc > 3 ? std::atoi(argv[3]) : reader_threads();
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) { std::printf("refused: cannot open\n"); return 1; }
    Header h;
    std::string why;
    if (!read_header(f, h, why)) { std::printf("refused: %s\n", why.c_str()); std::fclose(f); return 1; }
    std::vector<Record> rec[2] = {std::vector<Record>(chunk / 8 + 2), std::vector<Record>(chunk / 8 + 2)};
    std::map<std::tuple<int, int64_t>, std::pair<uint64_t, int64_t>> slots;   // (target, slot) -> (bits, line)
    int64_t nread = 0, dup_line = 0, dup_first = 0;
    const ParseError perr = read_body(
        f, h, chunk, threads, [&](int b) { return rec[b].data(); },
        [&](const Record* recs, int64_t count, int) {
            for (int64_t x = 0; x < count && !dup_line; ++x) {
                const Record& r = recs[x];
                const int64_t i = r.idx[0], j = r.idx[1], k = r.idx[2], l = r.idx[3];
                std::tuple<int, int64_t> key;
                if (i == 0) key = {0, 0};
                else if (!h.uhf) key = k == 0 ? std::make_tuple(1, tri(i, j)) : std::make_tuple(2, tri(tri(i, j), tri(k, l)));
                else if (k == 0) key = {3 + (int)(~i & 1), tri(i, j)};
                else if ((i & 1) == (k & 1)) key = {5 + (int)(~i & 1), tri(tri(i, j), tri(k, l))};
                else key = (i & 1) ? std::make_tuple(7, tri(i, j) * ((int64_t)1 << 31) + tri(k, l)) : std::make_tuple(7, tri(k, l) * ((int64_t)1 << 31) + tri(i, j));
                uint64_t bits;
                std::memcpy(&bits, &r.value, 8);
                auto it = slots.find(key);
                if (it == slots.end()) slots[key] = {bits, r.line};
                else if (it->second.first != bits) { dup_line = r.line; dup_first = it->second.second; }
            }
        },
        &nread);
    if (perr.line) { std::printf("refused: line %lld: %s\n", (long long)perr.line, perr.why); std::fclose(f); return 1; }
    if (dup_line) {
        std::printf("refused: line %lld: a duplicate that disagrees with line %lld\n", (long long)dup_line, (long long)dup_first);
        std::fclose(f);
        return 1;
    }
    std::fclose(f);
    std::printf("ok NORB %lld NELEC %lld MS2 %lld UHF %d lines %lld slots %zu\n", (long long)h.norb, (long long)h.nelec, (long long)h.ms2, (int)h.uhf,
                (long long)nread, slots.size());
    return 0;
}
