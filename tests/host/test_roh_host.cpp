// CPU test binary for the HIP-free pieces of eagle_roh / eagle_bed_roh (csrc/eagle_host.h: roh_arg_error, roh_block_table, roh_pos_check,
// roh_offsets), built by tests/test_roh_abi.py with -fsanitize=address,undefined.  Exit code 0 = every check passed.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../eagleeverything_amd/csrc/eagle_host.h"

static int g_fail = 0;
#define CHECK(cond)                                                                  \
    do {                                                                             \
        if (!(cond)) { fprintf(stderr, "FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); g_fail++; } \
    } while (0)

static bool says(const char* got, const char* part) { return got && strstr(got, part); }

// the defaults with field k replaced by v
static const char* rule(int k, int64_t v, long markers = 1000, long seg_cap = 0, bool has_seg = false) {
    int64_t p[9] = {50, 1, 5, 3277, 100, 0, 0, 0, -1};
    if (k >= 0) p[k] = v;
    return roh_arg_error(p, markers, seg_cap, has_seg);
}

// chrom / pos live in heap blocks of exactly `markers` entries, so that a read past them is an ASan report
static std::vector<int32_t> table(const std::vector<int32_t>& chrom, bool null_chrom = false) {
    int32_t* c = (int32_t*)malloc(sizeof(int32_t) * (chrom.size() ? chrom.size() : 1));
    for (size_t i = 0; i < chrom.size(); i++) c[i] = chrom[i];
    std::vector<int32_t> blk;
    roh_block_table(null_chrom ? nullptr : c, (long)chrom.size(), blk);
    free(c);
    return blk;
}
static long pos_check(const std::vector<int64_t>& pos, const std::vector<int32_t>& blk) {
    int64_t* p = (int64_t*)malloc(sizeof(int64_t) * (pos.size() ? pos.size() : 1));
    for (size_t i = 0; i < pos.size(); i++) p[i] = pos[i];
    const long r = roh_pos_check(p, blk);
    free(p);
    return r;
}

int main() {
    CHECK(rule(-1, 0) == nullptr);
    CHECK(says(rule(0, 0), "w must be") && says(rule(0, 65), "w must be") && rule(0, 1) == nullptr && rule(0, 64) == nullptr);
    CHECK(says(rule(1, -1), "win_het") && rule(1, 0) == nullptr && rule(1, 1000) == nullptr);
    CHECK(says(rule(2, -1), "win_miss") && rule(2, 0) == nullptr);
    CHECK(says(rule(3, -1), "thr16") && says(rule(3, 65537), "thr16") && rule(3, 0) == nullptr && rule(3, 65536) == nullptr);
    CHECK(says(rule(4, 0), "min_snp") && rule(4, 1) == nullptr);
    CHECK(says(rule(5, -1), "min_len") && rule(5, 0) == nullptr && rule(5, 0x7fffffffffffffffL) == nullptr);
    CHECK(says(rule(6, -1), "max_gap") && rule(6, 0) == nullptr);
    CHECK(says(rule(7, -1), "max_density") && says(rule(7, (1L << 31) + 1), "max_density") && rule(7, 1L << 31) == nullptr);
    CHECK(rule(8, -5) == nullptr && rule(8, 0) == nullptr && rule(8, 7) == nullptr);
    CHECK(says(rule(-1, 0, 1L << 31), "2^31") && rule(-1, 0, (1L << 31) - 1) == nullptr);
    CHECK(says(rule(-1, 0, 1000, -1, true), "seg_cap"));
    CHECK(says(rule(-1, 0, 1000, 1, false), "NULL") && rule(-1, 0, 1000, 1, true) == nullptr && rule(-1, 0, 1000, 0, false) == nullptr);

    // block table: maximal runs of equal chrom, any coding; a chromosome that comes back is a new block
    CHECK((table({3, 3, 3, 3}) == std::vector<int32_t>{0, 4}));
    CHECK((table({3, 3, 1, 1, 1, 3}) == std::vector<int32_t>{0, 2, 5, 6}));
    CHECK((table({1, 2, 3}) == std::vector<int32_t>{0, 1, 2, 3}));
    CHECK((table({7}) == std::vector<int32_t>{0, 1}));
    CHECK((table({1, 2, 3, 4, 5}, true) == std::vector<int32_t>{0, 5}));
    CHECK((table({-1, -1, 0x7fffffff, 0x7fffffff}) == std::vector<int32_t>{0, 2, 4}));

    // pos: non-decreasing inside every block, free across block edges; ties pass
    const std::vector<int32_t> blk = {0, 3, 5, 6};
    CHECK(roh_pos_check(nullptr, blk) == -1);
    CHECK(pos_check({10, 20, 30, 5, 6, 1}, blk) == -1);            // every block edge goes down: not compared
    CHECK(pos_check({10, 10, 10, 5, 5, 1}, blk) == -1);
    CHECK(pos_check({10, 9, 30, 5, 6, 1}, blk) == 1);
    CHECK(pos_check({10, 20, 19, 5, 6, 1}, blk) == 2);             // the last marker of a block
    CHECK(pos_check({10, 20, 30, 5, 4, 1}, blk) == 4);             // the second marker of a block: the pair right after the edge
    CHECK(pos_check({10, 9, 8, 5, 4, 1}, blk) == 1);               // the first violation is reported
    CHECK(pos_check({-5, -4, 0x7fffffffffffffffL, 0, 0, 0}, blk) == -1);
    CHECK(pos_check({1, 0}, {0, 2}) == 1 && pos_check({1, 0}, {0, 1, 2}) == -1);
    CHECK(pos_check({4}, {0, 1}) == -1);

    // exclusive scan by (individual, block)
    {
        int32_t* cnt = (int32_t*)malloc(sizeof(int32_t) * 5);
        int64_t* offs = (int64_t*)malloc(sizeof(int64_t) * 5);
        const int32_t v[5] = {2, 0, 3, 0, 1};
        memcpy(cnt, v, sizeof v);
        CHECK(roh_offsets(cnt, 5, offs) == 6);
        CHECK(offs[0] == 0 && offs[1] == 2 && offs[2] == 2 && offs[3] == 5 && offs[4] == 5);
        CHECK(roh_offsets(cnt, 0, offs) == 0);
        free(cnt);
        free(offs);
    }
    if (g_fail) {
        fprintf(stderr, "%d roh host checks FAILED\n", g_fail);
        return 1;
    }
    printf("roh host checks passed\n");
    return 0;
}
