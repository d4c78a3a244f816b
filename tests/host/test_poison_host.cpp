// CPU test binary for the value of EAGLE_HIP_POISON (csrc/eagle_host.h: poison_parse), built by tests/test_poison_host.py with
// -fsanitize=address,undefined.  The hook fills every allocation with the byte the value names; a value it does not understand must
// leave it off, never select some other byte.  The strings come in as literals and, for the cases the tests set, through the environment
// as the library reads it.  Exit code 0 = every check passed.
#include <stdio.h>
#include <stdlib.h>

#include "../../eagleeverything_amd/csrc/eagle_host.h"

static int g_fail = 0;
#define CHECK(cond)                                                                  \
    do {                                                                             \
        if (!(cond)) { fprintf(stderr, "FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); g_fail++; } \
    } while (0)

static int from_env(const char* value) {
    if (value) setenv("EAGLE_HIP_POISON", value, 1);
    else unsetenv("EAGLE_HIP_POISON");
    return poison_parse(getenv("EAGLE_HIP_POISON"));
}

int main() {
    // unset and empty: off
    CHECK(poison_parse(nullptr) == -1);
    CHECK(poison_parse("") == -1);
    // every byte, with and without leading zeros
    char buf[16];
    for (int v = 0; v <= 255; v++) {
        snprintf(buf, sizeof buf, "%d", v);
        CHECK(poison_parse(buf) == v);
        snprintf(buf, sizeof buf, "%03d", v);
        CHECK(poison_parse(buf) == v);
    }
    CHECK(poison_parse("0") == 0);
    CHECK(poison_parse("255") == 255);
    CHECK(poison_parse("127") == 0x7F);
    CHECK(poison_parse("85") == 0x55);
    // out of range: off, not a byte modulo 256
    CHECK(poison_parse("256") == -1);
    CHECK(poison_parse("999") == -1);
    CHECK(poison_parse("1000") == -1);
    CHECK(poison_parse("0255") == -1);   // four characters
    CHECK(poison_parse("4294967551") == -1);   // 2^32 + 255
    CHECK(poison_parse("99999999999999999999999999") == -1);
    // garbage: off, not the digits in front of it
    const char* garbage[] = {"-1", "+1", " 1", "1 ", "0x55", "0xFF", "ff", "1e2", "1.0", "12a", "a12", "yes", "on", "\t7", "7\n", "-", "2 5 5"};
    for (const char* g : garbage) CHECK(poison_parse(g) == -1);
    // as the library reads it
    CHECK(from_env(nullptr) == -1);
    CHECK(from_env("") == -1);
    CHECK(from_env("0") == 0);
    CHECK(from_env("255") == 255);
    CHECK(from_env("256") == -1);
    CHECK(from_env("poison") == -1);
    CHECK(from_env(nullptr) == -1);   // and off again once it is unset
    if (g_fail) { fprintf(stderr, "%d check(s) failed\n", g_fail); return 1; }
    printf("poison host checks passed\n");
    return 0;
}
