// CPU test binary for the HIP-free pieces of eagle_vcf_to_bed (csrc/eagle_host.h: vcf_next_line, vcf_whole_lines, vcf_split_tabs,
// vcf_header_error, vcf_verdict, vcf_count_fields, vcf_window_bytes, vcf_line_fits, vcf_window_lines), built by tests/test_vcf_abi.py
// with -fsanitize=address,undefined.  Every text lives in a heap block of exactly its size, so that a read past a line that ends at
// the buffer end, or past a field at the last byte, is an ASan report.  Exit code 0 = every check passed.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>

#include "../../eagleeverything_amd/csrc/eagle_host.h"

static int g_fail = 0;
#define CHECK(cond)                                                                  \
    do {                                                                             \
        if (!(cond)) { fprintf(stderr, "FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); g_fail++; } \
    } while (0)

// a heap copy of exactly s.size() bytes (no terminator)
struct Exact {
    char* p;
    size_t n;
    explicit Exact(const std::string& s) : p((char*)malloc(s.size() ? s.size() : 1)), n(s.size()) { memcpy(p, s.data(), s.size()); }
    ~Exact() { free(p); }
};

static std::string str(const VcfSpan& s) { return std::string(s.p, (size_t)s.len); }

// the lines of a buffer as the window loop walks them
static std::vector<std::string> lines_of(const std::string& text, bool last, size_t* stop) {
    Exact x(text);
    std::vector<std::string> out;
    size_t p = 0, b, e, next;
    while (vcf_next_line(x.p, x.n, p, last, &b, &e, &next)) {
        CHECK(b == p && e >= b && e <= x.n && next > p && next <= x.n);
        out.emplace_back(x.p + b, e - b);
        p = next;
    }
    *stop = p;
    return out;
}

static void test_lines() {
    size_t stop;
    auto v = lines_of("ab\ncd\r\n\n\r\nef", true, &stop);
    CHECK(v.size() == 5 && v[0] == "ab" && v[1] == "cd" && v[2].empty() && v[3].empty() && v[4] == "ef" && stop == 12);
    v = lines_of("ab\ncd\r\n\n\r\nef", false, &stop);           // the tail is not a whole line
    CHECK(v.size() == 4 && stop == 10);
    v = lines_of("ab\n", true, &stop);                           // the line ends exactly at the buffer end
    CHECK(v.size() == 1 && v[0] == "ab" && stop == 3);
    v = lines_of("ab\r\n", false, &stop);
    CHECK(v.size() == 1 && v[0] == "ab" && stop == 4);
    v = lines_of("\n", true, &stop);
    CHECK(v.size() == 1 && v[0].empty() && stop == 1);
    v = lines_of("\r", true, &stop);                             // a lone '\r' at the last byte of the file: an empty line
    CHECK(v.size() == 1 && v[0].empty() && stop == 1);
    v = lines_of("x", true, &stop);
    CHECK(v.size() == 1 && v[0] == "x" && stop == 1);
    v = lines_of("x", false, &stop);
    CHECK(v.empty() && stop == 0);
    v = lines_of("", true, &stop);
    CHECK(v.empty() && stop == 0);
    for (const char* t : {"", "abc", "abc\n", "a\nbc", "a\nb\nc\n", "\n", "\n\nabc"}) {
        Exact x(t);
        size_t want = 0;
        for (size_t i = 0; i < x.n; i++) if (x.p[i] == '\n') want = i + 1;
        CHECK(vcf_whole_lines(x.p, x.n) == want);
    }
}

static void test_tabs() {
    VcfSpan f[9];
    const char* rest;
    {
        Exact x("1\t100\trs1\tA\tC\t.\tPASS\t.\tGT\t0/1\t1");   // the last sample field is the last byte
        CHECK(vcf_split_tabs(x.p, x.p + x.n, f, 9, &rest) == 9 && rest == x.p + 26);
        CHECK(str(f[0]) == "1" && str(f[1]) == "100" && str(f[2]) == "rs1" && str(f[3]) == "A" && str(f[4]) == "C" && str(f[8]) == "GT");
        CHECK(vcf_count_fields(rest, x.p + x.n) == 2);
        CHECK(vcf_verdict(f, 0) == VCF_KEEP && vcf_verdict(f, VCF_SNPS_ONLY | VCF_PASS_ONLY) == VCF_KEEP);
    }
    {
        Exact x("1\t100\trs1\tA\tC\t.\tPASS\t.\tGT");             // nine fields and the line ends: no sample field
        CHECK(vcf_split_tabs(x.p, x.p + x.n, f, 9, &rest) == 9 && rest == nullptr && str(f[8]) == "GT");
    }
    {
        Exact x("1\t100\trs1\tA\tC\t.\tPASS\t.\tGT\t");           // a tab at the last byte: one empty sample field
        CHECK(vcf_split_tabs(x.p, x.p + x.n, f, 9, &rest) == 9 && rest == x.p + x.n && vcf_count_fields(rest, x.p + x.n) == 1);
    }
    {
        Exact x("1\t100\trs1\tA");
        CHECK(vcf_split_tabs(x.p, x.p + x.n, f, 9, &rest) == 4 && rest == nullptr && str(f[3]) == "A");
    }
    {
        Exact x("\t\t");
        CHECK(vcf_split_tabs(x.p, x.p + x.n, f, 9, &rest) == 3 && rest == nullptr && f[0].len == 0 && f[2].len == 0 && f[2].p == x.p + 2);
        CHECK(vcf_count_fields(x.p, x.p + x.n) == 3 && vcf_count_fields(x.p, x.p) == 1);
    }
    {
        Exact x("");
        CHECK(vcf_split_tabs(x.p, x.p, f, 9, &rest) == 1 && rest == nullptr && f[0].len == 0);
    }
}

static VcfVerdict verdict(const char* ref, const char* alt, const char* filter, const char* format, int flags) {
    const std::string line = std::string("7\t5\t.\t") + ref + "\t" + alt + "\t.\t" + filter + "\t.\t" + format;   // FORMAT ends the buffer
    Exact x(line);
    VcfSpan f[9];
    const char* rest;
    CHECK(vcf_split_tabs(x.p, x.p + x.n, f, 9, &rest) == 9);
    return vcf_verdict(f, flags);
}

static void test_verdicts() {
    const int all = VCF_SNPS_ONLY | VCF_PASS_ONLY;
    CHECK(verdict("A", "C", "PASS", "GT", all) == VCF_KEEP && verdict("a", "t", ".", "GT:DP", all) == VCF_KEEP);
    CHECK(verdict("A", "C", "PASS", "GT:", all) == VCF_KEEP);
    CHECK(verdict("A", "C,G", "PASS", "GT", 0) == VCF_MULTIALLELIC && verdict("A", ",", "q", "DP", all) == VCF_MULTIALLELIC);
    CHECK(verdict("A", ".", "PASS", "GT", 0) == VCF_NO_ALT && verdict("AT", ".", "q", "DP", all) == VCF_NO_ALT);
    CHECK(verdict("A", "C", "PASS", "DP:GT", 0) == VCF_NO_GT && verdict("A", "C", "PASS", "GTX", 0) == VCF_NO_GT);
    CHECK(verdict("A", "C", "PASS", "G", 0) == VCF_NO_GT && verdict("A", "C", "PASS", "", 0) == VCF_NO_GT);
    CHECK(verdict("AT", "A", "q", "DP", all) == VCF_NO_GT);                                    // the first reason that holds
    CHECK(verdict("AT", "A", "PASS", "GT", 0) == VCF_KEEP && verdict("AT", "A", "PASS", "GT", VCF_SNPS_ONLY) == VCF_NOT_SNP);
    CHECK(verdict("A", "N", "PASS", "GT", VCF_SNPS_ONLY) == VCF_NOT_SNP && verdict("A", "", "PASS", "GT", VCF_SNPS_ONLY) == VCF_NOT_SNP);
    CHECK(verdict("A", "<DEL>", "q", "GT", all) == VCF_NOT_SNP);
    CHECK(verdict("A", "C", "q10", "GT", 0) == VCF_KEEP && verdict("A", "C", "q10", "GT", VCF_PASS_ONLY) == VCF_FILTERED);
    CHECK(verdict("A", "C", "PASSED", "GT", VCF_PASS_ONLY) == VCF_FILTERED && verdict("A", "C", "", "GT", VCF_PASS_ONLY) == VCF_FILTERED);
    CHECK(verdict("A", "C", "pass", "GT", VCF_PASS_ONLY) == VCF_FILTERED);
}

static const char* header(const std::string& line, std::vector<std::string>* names = nullptr) {
    Exact x(line);
    std::vector<VcfSpan> spans;
    const char* e = vcf_header_error(x.p, x.p + x.n, spans);
    if (names) { names->clear(); for (const VcfSpan& s : spans) names->push_back(str(s)); }
    return e;
}
static bool says(const char* got, const char* part) { return got && strstr(got, part); }

static void test_header() {
    const std::string nine = "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT";
    std::vector<std::string> names;
    CHECK(header(nine + "\tA", &names) == nullptr && names.size() == 1 && names[0] == "A");   // the name is the last byte
    CHECK(header(nine + "\tS1\tS-2\tx.y", &names) == nullptr && names.size() == 3 && names[1] == "S-2" && names[2] == "x.y");
    CHECK(says(header(nine), "fewer than 10 columns") && says(header("#CHROM"), "fewer than 10 columns"));
    CHECK(says(header("#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO"), "fewer than 10 columns"));
    CHECK(says(header(nine + "\t"), "empty sample name") && says(header(nine + "\tA\t"), "empty sample name"));
    CHECK(says(header(nine + "\tA\t\tB"), "empty sample name") && says(header(nine + "\tA b"), "blank"));
    CHECK(says(header("1\t5\t.\tA\tC\t.\t.\t.\tGT\t0/0"), "#CHROM") && says(header("#CHRO"), "#CHROM") && says(header("#"), "#CHROM"));
}

static void test_windows() {
    CHECK(vcf_window_bytes(1, 8.0) == 1 && vcf_window_bytes(12345, 0.0) == 12345);
    CHECK(vcf_window_bytes(0, 8.0) == 67108864 && vcf_window_bytes(0, 0.0) == 67108864);
    CHECK(vcf_window_bytes(0, 0.03125) == 7812500 && vcf_window_bytes(0, 1e-9) == 4096);
    CHECK(vcf_line_fits(1000, 8.0) && vcf_line_fits(1L << 30, 0.0) && !vcf_line_fits(7812501, 0.03125) && vcf_line_fits(7812500, 0.03125));
    // a kept line of n fields takes at least 2 n - 1 sample bytes behind 19 bytes of fixed fields: the bound holds the lines of a window
    for (long n : {1L, 2L, 5L, 4099L})
        for (long cap : {1L, 40L, 4096L, 1L << 26}) CHECK(vcf_window_lines(cap, n) >= cap / (2 * n - 1 + 19 + 1) + 1);
}

int main() {
    test_lines();
    test_tabs();
    test_verdicts();
    test_header();
    test_windows();
    if (g_fail) { fprintf(stderr, "%d checks failed\n", g_fail); return 1; }
    printf("vcf host checks passed\n");
    return 0;
}
