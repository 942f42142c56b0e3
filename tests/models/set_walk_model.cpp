// Host model of the set walk: infidex_amd/csrc/set_walk.h, UNCHANGED.  The flag words, the zero-byte test, the member predicate and the code reader of a
// thread's 16 documents are held to a definition written byte by byte.  Flags and codes live in heap blocks of exactly n elements and the program is built with
// -fsanitize=address,undefined: a read at or beyond n ends the run.  tests/test_set_walk_model.py compiles and runs it.
//   set_walk_model         runs every case, prints "OK <groups> <flag patterns> <documents compared>" or the first mismatch (exit 1)
// Walked: every n from 1 to 48, every group of 16 that begins below n and the first one beyond (a thread past the corpus: no member, nothing read out of
// bounds); a null mask and, for the group that holds document n - 1, all 2^16 flag patterns, for the others 4096 random ones; flag bytes of several non-zero
// values; codes that name their document (never zero, so a code that was not loaded shows), and a null column.
#define SW_FN static inline
#include "set_walk.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>

typedef unsigned long long u64;
static u64 g_seed = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() { g_seed ^= g_seed << 13; g_seed ^= g_seed >> 7; g_seed ^= g_seed << 17; return (uint32_t)(g_seed >> 16); }

static u64 g_groups = 0, g_patterns = 0, g_docs = 0;

// the definition: document d is a member when it lies in the corpus and its flag, if there are flags, is zero
static bool member_def(const uint8_t* mask, int32_t n, int64_t d) { return d < n && (!mask || mask[d] == 0); }

static bool check(const uint8_t* mask, const uint32_t* col, int32_t n, int64_t d0, const char* what) {
    uint32_t m[4], cc[SW_GROUP], zz[SW_GROUP];
    sw_flags16(mask, n, d0, m);
    const bool any = sw_codes16(col, n, d0, m, cc), anyNull = sw_codes16(nullptr, n, d0, m, zz);
    bool anyDef = false;
    for (int q = 0; q < 4; q++) {
        bool some = false;
        for (int t = 0; t < 4; t++) some = some || member_def(mask, n, d0 + 4 * q + t);
        anyDef = anyDef || some;
        if (sw_any4(m[q]) != some) { printf("FAIL %s: n %d, group %lld, four %d: word %08x, a member among them: %d\n", what, n, (long long)d0, q, m[q], (int)some); return false; }
        for (int t = 0; t < 4; t++) {
            const int j = 4 * q + t; const int64_t d = d0 + j;
            const bool in = member_def(mask, n, d), byteSet = ((m[q] >> (8 * t)) & 0xFFu) != 0;
            if (byteSet == in || sw_member(m, j) != in) { printf("FAIL %s: n %d, document %lld: flag byte %02x, member %d, defined %d\n", what, n, (long long)d, (m[q] >> (8 * t)) & 0xFFu, (int)sw_member(m, j), (int)in); return false; }
            const uint32_t want = some && d < n ? col[d] : 0u;              // a four without a member is not loaded and reads as zeros
            if (cc[j] != want || zz[j] != 0u) { printf("FAIL %s: n %d, document %lld: code %u (null column: %u), expected %u\n", what, n, (long long)d, cc[j], zz[j], want); return false; }
            g_docs++;
        }
    }
    if (any != anyDef || anyNull != anyDef) { printf("FAIL %s: n %d, group %lld: a member among the 16: %d / %d, defined %d\n", what, n, (long long)d0, (int)any, (int)anyNull, (int)anyDef); return false; }
    g_patterns++;
    return true;
}

int main() {
    static const uint8_t shades[4] = {0x01, 0x80, 0xFF, 0x5A};             // a flag is any non-zero byte
    for (int32_t n = 1; n <= 48; n++) {
        uint8_t* mask = (uint8_t*)malloc((size_t)n);                        // exactly n elements each (malloc aligns them to 16 bytes, as the device's buffers are)
        uint32_t* col = (uint32_t*)malloc((size_t)n * 4);
        if (!mask || !col) return 2;
        for (int32_t d = 0; d < n; d++) { mask[d] = (uint8_t)(rnd() & 1u); col[d] = 0x51000000u + 977u * (uint32_t)d + 1u; }
        const int64_t past = ((int64_t)n + SW_GROUP - 1) / SW_GROUP * SW_GROUP;
        for (int64_t d0 = 0; d0 <= past; d0 += SW_GROUP) {
            const int32_t here = (int32_t)(d0 >= n ? 0 : (n - d0 < SW_GROUP ? n - d0 : SW_GROUP));      // documents of the group inside the corpus
            const bool last = d0 < n && d0 + SW_GROUP >= n;
            if (!check(nullptr, col, n, d0, "null mask")) return 1;
            const uint32_t patterns = last ? 65536u : (here ? 4096u : 16u);
            for (uint32_t p = 0; p < patterns; p++) {
                const uint32_t bits = last ? p : rnd() & 0xFFFFu, tone = rnd();
                for (int32_t j = 0; j < here; j++) mask[d0 + j] = (bits >> j) & 1u ? shades[(tone >> (2 * j)) & 3u] : 0;
                if (!check(mask, col, n, d0, last ? "the group of the last document" : (here ? "a whole group" : "past the corpus"))) return 1;
            }
            g_groups++;
        }
        free(mask); free(col);
    }
    printf("OK %llu %llu %llu\n", g_groups, g_patterns, g_docs);
    return 0;
}
