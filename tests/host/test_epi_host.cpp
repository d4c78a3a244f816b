// CPU test binary for the HIP-free pieces of eagle_epistasis_loci / eagle_epistasis_pairs (csrc/eagle_host.h: epi_arg_error,
// epi_loci_arg_error, epi_pairs_arg_error, epi_digits, epi_t53, epi_stat, epi_pair_tested), built by tests/test_epistasis_abi.py with
// -fsanitize=address,undefined.  Its own checks run first; then every line "n Y T si qi ui sj qj uj d e f h z" of the file argv[1] is
// answered on stdout with "Delta Sxx Sxy Syy <the statistic's 64 bits in hex>", which the test compares with Python-int results.
#include <inttypes.h>
#include <stdio.h>
#include <stdlib.h>

#include <string>
#include <vector>

#include "../../eagleeverything_amd/csrc/eagle_host.h"

#define CHECK(c)                                                          \
    do {                                                                  \
        if (!(c)) {                                                       \
            printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c);         \
            return 1;                                                     \
        }                                                                 \
    } while (0)

static std::string dec(epi_i128 x) {
    if (x == 0) return "0";
    const bool neg = x < 0;
    unsigned __int128 m = neg ? (unsigned __int128)0 - (unsigned __int128)x : (unsigned __int128)x;
    std::string s;
    while (m) { s.insert(s.begin(), (char)('0' + (int)(m % 10))); m /= 10; }
    return neg ? "-" + s : s;
}

static int own_checks() {
    // digits: every |y| <= 10^6 is three balanced base-128 digits, and so are the ends of their range
    for (int32_t y = -EPI_YMAX; y <= EPI_YMAX; y++) {
        int8_t d[3];
        CHECK(epi_digits(y, d) == 0);
        CHECK(d[0] >= -64 && d[0] <= 63 && d[1] >= -64 && d[1] <= 63 && d[2] >= -64 && d[2] <= 63);
        CHECK(d[0] + 128 * d[1] + 16384 * d[2] == y);
    }
    int8_t d[3];
    CHECK(epi_digits(1040319, d) == 0 && d[0] == 63 && d[1] == 63 && d[2] == 63);
    CHECK(epi_digits(-1056832, d) == 0 && d[0] == -64 && d[1] == -64 && d[2] == -64);
    CHECK(epi_digits(1040320, d) != 0 && epi_digits(-1056833, d) != 0);
    for (int32_t y : {63, 64, 65, 8127, 8128, 8256}) {
        CHECK(epi_digits(y, d) == 0 && d[0] + 128 * d[1] + 16384 * d[2] == y);
        CHECK(epi_digits(-y, d) == 0 && d[0] + 128 * d[1] + 16384 * d[2] == -y);
    }
    // t53
    CHECK(epi_t53(0) == 0.0 && epi_t53(1) == 1.0 && epi_t53(-1) == -1.0);
    const epi_i128 p53 = (epi_i128)1 << 53;
    CHECK(epi_t53(p53 - 1) == 9007199254740991.0 && epi_t53(p53) == 9007199254740992.0 && epi_t53(p53 + 1) == 9007199254740992.0);
    CHECK(epi_t53(-(p53 + 1)) == -9007199254740992.0 && epi_t53(p53 + 3) == 9007199254740994.0);
    CHECK(epi_t53(((epi_i128)1 << 110) - 1) == ldexp(9007199254740991.0, 57));
    CHECK(epi_t53(-(((epi_i128)1 << 126) + 1)) == -ldexp(1.0, 126));
    // the argument rules
    std::vector<int32_t> y(8, 5);
    CHECK(!epi_arg_error(8, 3, y.data()) && !epi_arg_error(EPI_MAX_N, 3, nullptr));
    CHECK(epi_arg_error(0, 3, nullptr) && epi_arg_error(8, 0, nullptr) && epi_arg_error(-1, -1, nullptr));
    CHECK(epi_arg_error(EPI_MAX_N + 1, 3, nullptr) && epi_arg_error(8, 0x80000000L, nullptr));
    y[7] = EPI_YMAX;
    y[0] = -EPI_YMAX;
    CHECK(!epi_arg_error(8, 3, y.data()));
    y[7] = EPI_YMAX + 1;
    CHECK(epi_arg_error(8, 3, y.data()));
    y[7] = 0;
    y[0] = -EPI_YMAX - 1;
    CHECK(epi_arg_error(8, 3, y.data()));
    const long loci[3] = {0, 9, 9};
    CHECK(!epi_loci_arg_error(10, loci, 3) && epi_loci_arg_error(9, loci, 3) && epi_loci_arg_error(10, loci, 0) && epi_loci_arg_error(10, loci, 65));
    const long neg[1] = {-1};
    CHECK(epi_loci_arg_error(10, neg, 1));
    CHECK(!epi_pairs_arg_error(0, 0.0, 0, false) && !epi_pairs_arg_error(3, -INFINITY, 5, true) && !epi_pairs_arg_error(0, INFINITY, 0, true));
    CHECK(epi_pairs_arg_error(-1, 0.0, 0, false) && epi_pairs_arg_error(0, NAN, 0, false) && epi_pairs_arg_error(0, 0.0, -1, true) &&
          epi_pairs_arg_error(0, 0.0, 1, false));
    // the gap rule
    const int32_t chrom[5] = {1, 1, 1, 2, 2};
    CHECK(epi_pair_tested(0, 1, nullptr, 0) && !epi_pair_tested(0, 1, nullptr, 1) && epi_pair_tested(0, 2, nullptr, 1));
    CHECK(!epi_pair_tested(0, 2, chrom, 2) && epi_pair_tested(2, 3, chrom, 2) && !epi_pair_tested(3, 4, chrom, 2) && epi_pair_tested(0, 4, chrom, 100));
    return 0;
}

int main(int argc, char** argv) {
    if (own_checks()) return 1;
    if (argc > 1) {
        FILE* f = fopen(argv[1], "r");
        if (!f) { printf("FAILED: cannot open %s\n", argv[1]); return 1; }
        long n;
        long long v[13];
        while (fscanf(f, "%ld %lld %lld %lld %lld %lld %lld %lld %lld %lld %lld %lld %lld %lld", &n, &v[0], &v[1], &v[2], &v[3], &v[4], &v[5], &v[6],
                      &v[7], &v[8], &v[9], &v[10], &v[11], &v[12]) == 14) {
            const EpiTrait t = {n, v[0], v[1]};
            const EpiMarker a = {v[2], v[3], v[4]}, b = {v[5], v[6], v[7]};
            epi_i128 S[4];
            const double st = epi_stat(t, a, b, v[8], v[9], v[10], v[11], v[12], S);
            uint64_t bits;
            memcpy(&bits, &st, sizeof bits);
            printf("%s %s %s %s %016" PRIx64 "\n", dec(S[0]).c_str(), dec(S[1]).c_str(), dec(S[2]).c_str(), dec(S[3]).c_str(), bits);
        }
        fclose(f);
    }
    printf("epi host checks passed\n");
    return 0;
}
