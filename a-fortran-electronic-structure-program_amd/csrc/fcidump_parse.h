// fcidump_parse.h -- host side of the FCIDUMP reader (afesp_fcidump_scan / afesp_read_fcidump / _uhf): the namelist
// header, one body line -> one fixed-size record, the checks a record can fail on its own, and the split of a block of text over threads.
// Plain C++ with no GPU call (like fcidump_format.h beside it), so that it also builds into a stand-alone program and runs under the
// address and undefined-behaviour sanitizers.
//
// Accepted: "&FCI ... &END" or "&FCI ... /"; keys in any letter case, over any number of lines, in any order; ORBSYM, ISYM and unknown
// keys ignored; MS2 missing = 0; UHF=.TRUE. = the writer's spin-orbital numbering (spatial orbital p is 2p - 1 for alpha, 2p for beta).
// Body: "value i j k l", fields separated by blanks and/or one comma, reals with E or D exponents, blank lines and \r tolerated.
#pragma once
#include <cctype>
#include <cmath>
#include <cstdio>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <string>
#include <system_error>
#include <thread>
#include <vector>

namespace afesp {
namespace fcidump {

struct Header {
    int64_t norb = 0, nelec = 0, ms2 = 0;
    bool uhf = false;
    size_t body = 0;     // offset of the first byte after the terminator's line
    int64_t lines = 0;   // lines the header takes (the body's first line is number lines + 1)
};

// one body line: 32 bytes, the unit that crosses to the device
struct Record {
    double value;
    int32_t idx[4];   // as written: 1-based, 0 where the file says 0
    int64_t line;     // line number in the file, 1-based
};
static_assert(sizeof(Record) == 32, "Record is 32 bytes");

enum Kind { CORE = 0, ONE = 1, TWO = 2 };
enum LineStatus { LINE_BLANK = 0, LINE_OK = 1, LINE_MALFORMED = -1 };

namespace detail {
inline bool ieq(const char* a, const char* b, size_t n)
{
    for (size_t i = 0; i < n; ++i)
        if (std::toupper((unsigned char)a[i]) != std::toupper((unsigned char)b[i])) return false;
    return true;
}
inline bool word_char(char c) { return std::isalnum((unsigned char)c) || c == '_'; }
// the one definition of a blank inside a body line: the line count of afesp_fcidump_scan and the records of the reader agree through it
inline bool blank(char c) { return c == ' ' || c == '\t' || c == '\r' || c == '\f' || c == '\v'; }
// the text after "KEY =" for the first whole-word, case-blind occurrence of KEY in [p, end); nullptr if there is none
inline const char* after_key(const char* p, const char* end, const char* key)
{
    const size_t k = std::strlen(key);
    for (const char* c = p; c + k <= end; ++c) {
        if (!ieq(c, key, k) || (c > p && word_char(c[-1]))) continue;
        const char* v = c + k;
        while (v < end && std::isspace((unsigned char)*v)) ++v;
        if (v < end && *v == '=') {
            ++v;
            while (v < end && std::isspace((unsigned char)*v)) ++v;
            return v;
        }
    }
    return nullptr;
}
inline bool key_int(const char* p, const char* end, const char* key, int64_t& out)
{
    const char* v = after_key(p, end, key);
    if (!v || v >= end) return false;
    char tok[24];
    size_t n = 0;
    if (*v == '-' || *v == '+') tok[n++] = *v++;
    while (v < end && std::isdigit((unsigned char)*v) && n < sizeof(tok) - 1) tok[n++] = *v++;
    tok[n] = 0;
    if (n == 0 || (n == 1 && !std::isdigit((unsigned char)tok[0]))) return false;
    out = std::strtoll(tok, nullptr, 10);
    return true;
}
}  // namespace detail

// The header in text[0, len).  0: parsed.  1: the terminator is not in these bytes (read more, or give up at the end of the file).
// -1: the text does not begin with &FCI, or NORB / NELEC is missing or not positive: err says which.
inline int parse_header(const char* text, size_t len, Header& h, std::string& err)
{
    const char* const end = text + len;
    const char* p = text;
    while (p < end && std::isspace((unsigned char)*p)) ++p;
    if (end - p < 4) {
        if (len > 0 && p < end && *p != '&') { err = "no &FCI header"; return -1; }
        return 1;
    }
    if (!detail::ieq(p, "&FCI", 4)) { err = "no &FCI header"; return -1; }
    const char* const keys = p + 4;
    const char* term = nullptr;
    for (const char* c = keys; c < end; ++c) {
        if (*c == '/') { term = c; break; }
        if (*c == '&' && end - c >= 4 && detail::ieq(c, "&END", 4)) { term = c; break; }
        if (*c == '&' && end - c < 4) return 1;   // (possibly a cut "&END")
    }
    if (!term) return 1;
    const char* nl = term;
    while (nl < end && *nl != '\n') ++nl;
    if (nl == end) return 1;   // the terminator's line is not complete yet (the caller appends a newline at the end of the file)
    h = Header();
    h.body = (size_t)(nl + 1 - text);
    for (const char* c = text; c <= nl; ++c) h.lines += *c == '\n';
    if (!detail::key_int(keys, term, "NORB", h.norb) || h.norb <= 0) { err = "no NORB in the header"; return -1; }
    if (!detail::key_int(keys, term, "NELEC", h.nelec) || h.nelec < 0) { err = "no NELEC in the header"; return -1; }
    if (!detail::key_int(keys, term, "MS2", h.ms2)) h.ms2 = 0;
    const char* u = detail::after_key(keys, term, "UHF");
    if (u && u < term && *u == '.') ++u;
    h.uhf = u && u < term && (*u == 'T' || *u == 't');
    return 0;
}

// One line [p, end) without its newline.  The value by strtod on the token (D exponents turned into E): correctly rounded, the bits
// Python's float() gives.  Only digits, sign, point and exponent letters make a value (no "inf", "nan" or hexadecimal forms); an index
// is a non-negative decimal integer.  Whatever follows the fifth field must be blank.
inline LineStatus parse_line(const char* p, const char* end, Record& r)
{
    using detail::blank;
    while (p < end && blank(*p)) ++p;
    if (p >= end) return LINE_BLANK;
    char tok[64];
    size_t n = 0;
    while (p < end && !blank(*p) && *p != ',') {
        const char c = *p++;
        if (n >= sizeof(tok) - 1) return LINE_MALFORMED;
        if (c == 'D' || c == 'd') tok[n++] = 'E';
        else if (std::isdigit((unsigned char)c) || c == '+' || c == '-' || c == '.' || c == 'E' || c == 'e') tok[n++] = c;
        else return LINE_MALFORMED;
    }
    tok[n] = 0;
    char* q = nullptr;
    r.value = std::strtod(tok, &q);
    if (n == 0 || q != tok + n || !std::isfinite(r.value)) return LINE_MALFORMED;   // (an overflow such as 1E999 is no value either)
    for (int k = 0; k < 4; ++k) {
        while (p < end && blank(*p)) ++p;
        if (p < end && *p == ',') ++p;
        while (p < end && blank(*p)) ++p;
        int64_t v = 0;
        int digits = 0;
        while (p < end && std::isdigit((unsigned char)*p)) {
            if (++digits > 9) return LINE_MALFORMED;
            v = 10 * v + (*p++ - '0');
        }
        if (digits == 0 || (p < end && !blank(*p) && *p != ',')) return LINE_MALFORMED;
        r.idx[k] = (int32_t)v;
    }
    while (p < end && blank(*p)) ++p;
    return p == end ? LINE_OK : LINE_MALFORMED;
}

// What a record is, and the checks it can fail on its own.  Returns the kind, or -1 with `why` set.
inline int classify(const Record& r, int64_t norb, bool uhf, const char*& why)
{
    const int32_t i = r.idx[0], j = r.idx[1], k = r.idx[2], l = r.idx[3];
    if (i < 0 || j < 0 || k < 0 || l < 0 || i > norb || j > norb || k > norb || l > norb) { why = "an index outside 0..NORB"; return -1; }
    int kind;
    if (i > 0 && j > 0 && k > 0 && l > 0) kind = TWO;
    else if (i > 0 && j > 0 && k == 0 && l == 0) kind = ONE;
    else if (i == 0 && j == 0 && k == 0 && l == 0) kind = CORE;
    else { why = "neither a two-electron, a one-electron nor the core-energy line"; return -1; }
    if (uhf && kind != CORE) {   // odd spin-orbital numbers are alpha, even ones beta
        if ((i ^ j) & 1) { why = kind == ONE ? "a one-electron element between an alpha and a beta spin orbital" : "a spin-forbidden two-electron integral"; return -1; }
        if (kind == TWO && ((k ^ l) & 1)) { why = "a spin-forbidden two-electron integral"; return -1; }
    }
    return kind;
}

struct ParseError {
    int64_t line = 0;   // 0: none
    const char* why = nullptr;
};

// The whole lines of text[0, len) (len ends behind a newline, or at the end of the file) as records, written to out[0 ..] in file order
// (room for len / 8 + 2 of them: a line takes ten bytes at least); first_line = the number of the first line.  Up to `nthreads` threads,
// each on a run of whole lines, in two rounds that are each started and joined: the first counts every run's lines and non-blank lines,
// the second parses straight into the run's place in `out` with the final line numbers -- no second pass over the records, and no thread
// ever waits for another, so a run whose thread cannot be started is simply done by the caller.  The records and the error reported (the
// one on the smallest line) do not depend on the number of threads.  Core-energy lines are counted into ncore across
// calls, the second one's line number kept.  Where an error is reported the contents of `out` are not to be used.
struct BlockResult {
    int64_t lines = 0, records = 0;
};
inline BlockResult parse_block(const char* text, size_t len, int64_t first_line, int64_t norb, bool uhf, int nthreads, Record* out,
                               int64_t& ncore, int64_t& second_core_line, ParseError& err)
{
    if (nthreads < 1) nthreads = 1;
    if (len < ((size_t)nthreads << 16)) nthreads = (int)(len >> 16) > 0 ? (int)(len >> 16) : 1;   // 64 KiB per thread at least
    struct Part {
        size_t lo = 0, hi = 0;
        int64_t lines = 0, slots = 0;      // lines, non-blank lines
        int64_t core[2] = {0, 0}, ncore = 0;   // line numbers of the first two core-energy lines
        ParseError err;
    };
    using detail::blank;
    std::vector<Part> parts((size_t)nthreads);
    for (int t = 1; t < nthreads; ++t) {
        size_t cut = len * (size_t)t / (size_t)nthreads;
        while (cut > 0 && cut < len && text[cut - 1] != '\n') ++cut;
        parts[(size_t)t].lo = parts[(size_t)t - 1].hi = cut;
    }
    parts.back().hi = len;
    auto count = [&](int t) {
        Part& part = parts[(size_t)t];
        const char* const end = text + part.hi;
        for (const char* p = text + part.lo; p < end;) {
            const char* nl = (const char*)std::memchr(p, '\n', (size_t)(end - p));
            const char* stop = nl ? nl : end;
            ++part.lines;
            while (p < stop && blank(*p)) ++p;
            part.slots += p < stop;
            p = stop + 1;
        }
    };
    auto parse = [&](int t) {
        Part& part = parts[(size_t)t];
        const char* const end = text + part.hi;
        int64_t line = first_line, at = 0;
        for (int u = 0; u < t; ++u) {
            line += parts[(size_t)u].lines;
            at += parts[(size_t)u].slots;
        }
        for (const char* p = text + part.lo; p < end; ++line) {
            const char* nl = (const char*)std::memchr(p, '\n', (size_t)(end - p));
            const char* stop = nl ? nl : end;
            Record r;
            const LineStatus st = parse_line(p, stop, r);
            if (st == LINE_OK) {
                r.line = line;
                const char* why = nullptr;
                if (classify(r, norb, uhf, why) >= 0) {
                    if (r.idx[0] == 0 && part.ncore++ < 2) part.core[part.ncore - 1] = line;
                    out[at++] = r;
                } else if (!part.err.line) {
                    part.err.line = line;
                    part.err.why = why;
                }
            } else if (st == LINE_MALFORMED && !part.err.line) {
                part.err.line = line;
                part.err.why = "a malformed line";
            }
            p = stop + 1;
        }
    };
    std::vector<std::thread> pool;
    pool.reserve((size_t)nthreads);
    auto on_all_parts = [&](const std::function<void(int)>& fn) {
        int started = 1;
        try {
            for (; started < nthreads; ++started) pool.emplace_back(fn, started);
        } catch (const std::system_error&) {   // no further thread to be had: the caller does those runs itself
        }
        fn(0);
        for (int t = started; t < nthreads; ++t) fn(t);
        for (std::thread& th : pool) th.join();
        pool.clear();
    };
    on_all_parts(count);
    on_all_parts(parse);
    BlockResult res;
    for (const Part& part : parts) {
        if (part.err.line && !err.line) err = part.err;
        for (int c = 0; c < 2 && c < part.ncore; ++c)
            if (++ncore == 2) second_core_line = part.core[c];
        if (part.ncore > 2) ncore += part.ncore - 2;
        res.lines += part.lines;
        res.records += part.slots;
    }
    return res;
}

inline int reader_threads()
{
    const unsigned hw = std::thread::hardware_concurrency();
    const int t = hw ? (int)hw : 1;
    return t > 16 ? 16 : t;
}

// The header at the start of `f`, read block by block until its terminator's line is whole; the file is left positioned at the body.
// A header may take HEADER_MAX bytes at most (ORBSYM of 2048 orbitals is 4 KiB), so a file without a terminator is refused after one
// bounded scan.  Returns false with `why` set.
constexpr size_t HEADER_MAX = (size_t)256 << 10;
inline bool read_header(FILE* f, Header& h, std::string& why)
{
    std::string text;
    std::vector<char> blk(1 << 14);
    for (bool eof = false;;) {
        const size_t got = eof ? 0 : std::fread(blk.data(), 1, blk.size(), f);
        text.append(blk.data(), got);
        if (got == 0 && !eof) { eof = true; text.push_back('\n'); }   // (a terminator on the last line, without a newline)
        const int st = parse_header(text.data(), text.size(), h, why);
        if (st == 0) break;
        if (st < 0) return false;
        if (eof || text.size() > HEADER_MAX) { why = "no &FCI ... &END (or /) header"; return false; }
    }
    if (std::fseek(f, (long)h.body, SEEK_SET) != 0) { why = "cannot seek"; return false; }
    return true;
}

// The body of `f` (positioned behind the header) chunk by chunk: at most `chunk` bytes of text per round, an incomplete last line carried
// into the next round.  acquire(b) hands out the record buffer of round parity b (room for chunk / 8 + 2 records; it may wait until an
// earlier round's records have left it), sink(records, count, b) takes a round's records.  Stops at the first round with an error:
// returns it (line 0: none) -- a malformed line, a failed check of classify, a second core-energy line, a line longer than a chunk.
// *nread = the records handed to sink.
template <class Acquire, class Sink>
inline ParseError read_body(FILE* f, const Header& h, size_t chunk, int nthreads, Acquire&& acquire, Sink&& sink, int64_t* nread)
{
    std::vector<char> buf(chunk + 1);
    size_t keep = 0;
    int64_t line_no = h.lines + 1, ncore = 0, second_core = 0;
    *nread = 0;
    for (int b = 0;;) {
        const size_t got = std::fread(buf.data() + keep, 1, chunk - keep, f);
        const size_t have = keep + got;
        if (have == 0) break;
        const bool eof = got == 0;
        size_t stop = have;   // (at the end of the file the last line may lack its newline)
        if (!eof) {
            while (stop > 0 && buf[stop - 1] != '\n') --stop;
            if (stop == 0) {
                if (have == chunk) return ParseError{line_no, "a line longer than a chunk"};
                keep = have;
                continue;
            }
        }
        Record* rec = acquire(b);
        ParseError perr;
        const BlockResult res = parse_block(buf.data(), stop, line_no, h.norb, h.uhf, nthreads, rec, ncore, second_core, perr);
        if (ncore >= 2 && (!perr.line || second_core < perr.line)) perr = ParseError{second_core, "more than one core-energy line"};
        if (perr.line) return perr;
        if (res.records > 0) sink(rec, res.records, b);
        *nread += res.records;
        line_no += res.lines;
        keep = have - stop;
        std::memmove(buf.data(), buf.data() + stop, keep);
        b ^= 1;
        if (eof) break;
    }
    return ParseError();
}

}  // namespace fcidump
}  // namespace afesp
