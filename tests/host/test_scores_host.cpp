// CPU test binary for the HIP-free rules of eagle_sample_scores / eagle_marker_scores (csrc/eagle_host.h: scores_arg_error, score_digits,
// score_digit), built by tests/test_scores_abi.py with -fsanitize=address,undefined.  Exit code 0 = every check passed.
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

// the weights live in a heap block of exactly T * line_len words, so that a read past them is an ASan report
static const char* with_weights(long lines, long line_len, long T, const std::vector<int32_t>& w, int* mask = nullptr) {
    int32_t* p = (int32_t*)malloc(sizeof(int32_t) * (w.size() ? w.size() : 1));
    for (size_t i = 0; i < w.size(); i++) p[i] = w[i];
    const char* r = scores_arg_error(lines, line_len, T, p, mask);
    free(p);
    return r;
}

static long long rebuild(const int8_t d[4]) { return d[0] + 256LL * d[1] + 65536LL * d[2] + 16777216LL * d[3]; }

int main() {
    const int32_t W = 1 << 30;
    const int32_t edges[] = {0, 1, -1, 127, 128, -128, -129, 32639, 32640, -32896, -32897, 8355711, 8355712, -8421504, -8421505, W - 1, W, -W};
    for (int32_t x : edges) {
        int8_t d[4];
        CHECK(score_digits(x, d) == 0);
        CHECK(rebuild(d) == x);
        for (int p = 0; p < 4; p++) CHECK(score_digit(x, p) == d[p]);
    }
    unsigned long long s = 88172645463325252ULL;   // xorshift64: 10^5 weights across the whole range
    for (int i = 0; i < 100000; i++) {
        s ^= s << 13; s ^= s >> 7; s ^= s << 17;
        const int32_t x = (int32_t)((long long)(s % (2ULL * W + 1)) - W);
        int8_t d[4];
        CHECK(score_digits(x, d) == 0 && rebuild(d) == x);
        CHECK(score_digit(x, 3) == d[3] && score_digit(x, 0) == d[0]);
    }
    { int8_t d[4]; (void)score_digits(127, d); CHECK(d[0] == 127 && !d[1] && !d[2] && !d[3]); }
    { int8_t d[4]; (void)score_digits(128, d); CHECK(d[0] == -128 && d[1] == 1 && !d[2] && !d[3]); }
    { int8_t d[4]; (void)score_digits(-129, d); CHECK(d[0] == 127 && d[1] == -1 && !d[2] && !d[3]); }
    { int8_t d[4]; (void)score_digits(W, d); CHECK(!d[0] && !d[1] && !d[2] && d[3] == 64); }

    CHECK(scores_arg_error(10, 20, 1, nullptr, nullptr) == nullptr);
    CHECK(says(scores_arg_error(0, 20, 1, nullptr, nullptr), "dims") && says(scores_arg_error(10, -1, 1, nullptr, nullptr), "dims"));
    CHECK(says(scores_arg_error(10, 20, 0, nullptr, nullptr), "T outside") && says(scores_arg_error(10, 20, 65, nullptr, nullptr), "T outside"));
    CHECK(scores_arg_error(10, 20, 64, nullptr, nullptr) == nullptr);
    CHECK(says(scores_arg_error(10, SCORES_MAX_LINE + 1, 1, nullptr, nullptr), "EAGLE_SCORES_MAX_LINE"));
    CHECK(scores_arg_error(10, SCORES_MAX_LINE, 64, nullptr, nullptr) == nullptr);
    CHECK(says(scores_arg_error(1L << 31, 20, 1, nullptr, nullptr), "2^31") && scores_arg_error((1L << 31) - 1, 20, 1, nullptr, nullptr) == nullptr);
    // the shape is judged before a weight is read: one word of weights behind shapes that would read far more
    CHECK(says(with_weights(10, SCORES_MAX_LINE + 1, 1, {1}), "EAGLE_SCORES_MAX_LINE") && says(with_weights(10, 20, 65, {1}), "T outside"));
    int mask = -1;
    CHECK(with_weights(10, 3, 2, {1, -2, 3, 127, -128, 0}, &mask) == nullptr && mask == 1);
    CHECK(with_weights(10, 3, 1, {256, -512, 0}, &mask) == nullptr && mask == 2);
    CHECK(with_weights(10, 3, 1, {0, 0, 0}, &mask) == nullptr && mask == 0);
    CHECK(with_weights(10, 2, 1, {W, -W}, &mask) == nullptr && mask == 8);
    CHECK(with_weights(10, 2, 1, {W - 1, 0}, &mask) == nullptr && mask == 9);      // 2^30 - 1 = -1 + 64 * 256^3
    CHECK(with_weights(10, 2, 1, {0, 0x01020304}, &mask) == nullptr && mask == 15);
    CHECK(with_weights(10, 1, 1, {128}, &mask) == nullptr && mask == 3);
    CHECK(says(with_weights(10, 2, 2, {0, 0, 0, W + 1}), "2^30") && says(with_weights(10, 2, 2, {-W - 1, 0, 0, 0}), "2^30"));
    CHECK(says(with_weights(10, 1, 1, {INT32_MIN}), "2^30") && says(with_weights(10, 1, 1, {INT32_MAX}), "2^30"));
    if (g_fail) { fprintf(stderr, "%d check(s) failed\n", g_fail); return 1; }
    printf("scores host checks passed\n");
    return 0;
}
