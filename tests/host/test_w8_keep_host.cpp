// CPU test binary for the rule by which the int8 W engine keeps what it made from S alone (csrc/eagle_host.h: W8Keep, w8_keep_valid,
// w8_keep_forget, W8Declared, w8_declared_gen), built by tests/test_w8_keep_host.py with -fsanitize=address,undefined.
// Exit code 0 = every check passed.
#include <stdio.h>
#include <stdlib.h>

#include "../../eagleeverything_amd/csrc/eagle_host.h"

static int g_fail = 0;
#define CHECK(cond)                                                                  \
    do {                                                                             \
        if (!(cond)) { fprintf(stderr, "FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); g_fail++; } \
    } while (0)

int main() {
    double S1[4], S2[4], ws1[4], ws2[4];
    int st1, st2;
    W8Keep k;
    // nothing recorded: never valid, whatever the call says
    CHECK(!w8_keep_valid(k, S1, 700, 768, ws1, 1, 5, &st1));
    CHECK(!w8_keep_valid(k, nullptr, 0, 0, nullptr, 0, 0, nullptr));
    k.Sa = S1; k.n = 700; k.np = 768; k.ws = ws1; k.ws_gen = 3; k.s_gen = 5; k.stream = &st1;
    CHECK(w8_keep_valid(k, S1, 700, 768, ws1, 3, 5, &st1));
    // the truth table: one field off at a time
    CHECK(!w8_keep_valid(k, S2, 700, 768, ws1, 3, 5, &st1));    // another image
    CHECK(!w8_keep_valid(k, S1, 701, 768, ws1, 3, 5, &st1));    // n
    CHECK(!w8_keep_valid(k, S1, 700, 1024, ws1, 3, 5, &st1));   // n_pad
    CHECK(!w8_keep_valid(k, S1, 700, 768, ws2, 3, 5, &st1));    // another workspace block
    CHECK(!w8_keep_valid(k, S1, 700, 768, ws1, 4, 5, &st1));    // the same address after a re-allocation
    CHECK(!w8_keep_valid(k, S1, 700, 768, ws1, 3, 6, &st1));    // a new S in the same buffer
    CHECK(!w8_keep_valid(k, S1, 700, 768, ws1, 3, 0, &st1));    // nobody vouches for S (no declaration, EAGLE_HIP_NO_SCACHE)
    CHECK(!w8_keep_valid(k, S1, 700, 768, ws1, 3, 5, &st2));    // another stream: what was kept may not have been written yet
    CHECK(!w8_keep_valid(k, S1, 700, 768, nullptr, 3, 5, &st1));
    // a record made without a number is never valid, not even against a call without one
    W8Keep z = k;
    z.s_gen = 0;
    CHECK(!w8_keep_valid(z, S1, 700, 768, ws1, 3, 0, &st1));
    // every combination of two fields off
    for (int m = 0; m < 128; m++) {
        const bool ok = w8_keep_valid(k, (m & 1) ? S2 : S1, (m & 2) ? 699 : 700, (m & 4) ? 1024 : 768, (m & 8) ? ws2 : ws1, (m & 16) ? 9ul : 3ul,
                                      (m & 32) ? 7ul : 5ul, (m & 64) ? (const void*)&st2 : (const void*)&st1);
        CHECK(ok == (m == 0));
    }
    // forget (drop_workspaces, eagle_dev_forget_s, a declined call)
    w8_keep_forget(k);
    CHECK(!w8_keep_valid(k, S1, 700, 768, ws1, 3, 5, &st1));
    CHECK(k.Sa == nullptr && k.ws == nullptr && k.s_gen == 0 && k.n == 0 && k.np == 0);

    // the declaration vouches for exactly (image, n, n_pad)
    W8Declared d;
    CHECK(w8_declared_gen(d, S1, 700, 768) == 0);
    CHECK(w8_declared_gen(d, nullptr, 0, 0) == 0);               // (nothing declared matches nothing)
    d.Sa = S1; d.n = 700; d.np = 768; d.s_gen = 11;
    CHECK(w8_declared_gen(d, S1, 700, 768) == 11);
    CHECK(w8_declared_gen(d, S2, 700, 768) == 0);
    CHECK(w8_declared_gen(d, S1, 699, 768) == 0);
    CHECK(w8_declared_gen(d, S1, 700, 1024) == 0);
    // declare -> keep -> declare again (a new S in the same buffer) -> the record is void; forget -> nothing vouched for
    k.Sa = S1; k.n = 700; k.np = 768; k.ws = ws1; k.ws_gen = 3; k.s_gen = w8_declared_gen(d, S1, 700, 768); k.stream = &st1;
    CHECK(w8_keep_valid(k, S1, 700, 768, ws1, 3, w8_declared_gen(d, S1, 700, 768), &st1));
    d.s_gen = 12;
    CHECK(!w8_keep_valid(k, S1, 700, 768, ws1, 3, w8_declared_gen(d, S1, 700, 768), &st1));
    d = W8Declared();
    CHECK(!w8_keep_valid(k, S1, 700, 768, ws1, 3, w8_declared_gen(d, S1, 700, 768), &st1));

    if (g_fail) { fprintf(stderr, "%d check(s) failed\n", g_fail); return 1; }
    printf("w8 keep host checks passed\n");
    return 0;
}
