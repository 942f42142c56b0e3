// Host check of the wide entry point of the device introsort (bcl_introsort_wide in infidex_amd/csrc/bclsort.hip.inc, the sort k_postproc_wide runs over
// up to 1024 rows): the SAME source file compiled for the host, element for element against the oracle's restatement of
// ArraySortHelper<T>.IntrospectiveSort (oracle/dotnet.hpp IntroSorter), with the three comparisons of k_postproc — score descending (float.CompareTo, NaN
// lowest, -0 == +0) and the sort key ascending / descending with null lowest — at n in {65, 127, 128, 129, 255, 256, 257, 511, 512, 1000, 1023, 1024} on
// tie-heavy random inputs (2-5 distinct values), and on a McIlroy adversary input at n = 1024 that exhausts the depth limit.  The frame stack is as
// long as the device's (BCL_WIDE_MAX_FRAMES); a write past it aborts.
// Prints "OK <sorts> <insertion> <partition> <heapsort> <deepest stack>".  "dump <seed> <rounds>" prints random cases of every size with their sorted
// order instead, for the Python port (tests/bcl_sort.py).  Test infrastructure (tests/test_bclsort_wide_model.py).
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>
static long long g_branch[3];
static int g_deepest;
static const int SIZES[] = {65, 127, 128, 129, 255, 256, 257, 511, 512, 1000, 1023, 1024};
#define BCL_FN static inline
#define BCL_BRANCH(w) (g_branch[w]++)
#include "../../infidex_amd/csrc/bclsort.hip.inc"
#include "../../oracle/dotnet.hpp"

// the comparison of k_postproc on row indices: mode 0 score descending, 1 key ascending, 2 key descending (key 0 = null)
struct Rows { std::vector<float> sc; std::vector<uint32_t> key; int mode; };
static int cmp_rows(const Rows& R, int a, int b) {
    if (R.mode == 0) return bcl_cmp_float(R.sc[b], R.sc[a]);
    return R.mode == 1 ? bcl_cmp_u32(R.key[a], R.key[b]) : bcl_cmp_u32(R.key[b], R.key[a]);
}
struct HostSeq {                       // the accessor of bclsort.hip.inc over host arrays
    const Rows* R; int* k; int frames[BCL_WIDE_MAX_FRAMES];
    int get(int i) const { return k[i]; }
    void set(int i, int v) { k[i] = v; }
    int fget(int i) const { return frames[i]; }
    void fset(int i, int v) { if (i < 0 || i >= BCL_WIDE_MAX_FRAMES) abort(); frames[i] = v; if (i + 1 > g_deepest) g_deepest = i + 1; }
    int cmp(int a, int b) const { return cmp_rows(*R, a, b); }
};
static std::vector<int> product_sort(const Rows& R, int n) {
    std::vector<int> p(n); for (int i = 0; i < n; i++) p[i] = i;
    HostSeq s{&R, p.data(), {}}; bcl_introsort_wide(s, n);
    return p;
}
static std::vector<int> oracle_sort(const Rows& R, int n) {
    std::vector<int> p(n); for (int i = 0; i < n; i++) p[i] = i;
    orc::dotnet::sort(p, [&](int a, int b) { return cmp_rows(R, a, b); });
    return p;
}
static Rows random_rows(std::mt19937& rng, int n, int mode) {
    Rows R; R.mode = mode; R.sc.resize(n); R.key.resize(n);
    const int distinct = 2 + (int)(rng() % 4);
    float vals[5];
    for (int v = 0; v < distinct; v++) {
        const int kind = (int)(rng() % 8);
        vals[v] = kind == 0 ? NAN : kind == 1 ? -0.0f : kind == 2 ? 0.0f : (float)(rng() % 7) * 0.25f + 0.5f;
    }
    for (int i = 0; i < n; i++) { R.sc[i] = vals[rng() % distinct]; R.key[i] = (uint32_t)(rng() % distinct); }    // key 0 = null
    return R;
}
// McIlroy, "A killer adversary for quicksort" (1999): values are fixed lazily so that every pivot is as bad as possible; the values it ends with are an
// input on which the same sort (any sort following the same compares) goes quadratic -> introsort reaches its depth limit and heapsorts
static std::vector<uint32_t> adversary_keys(int n) {
    std::vector<int> val(n, n); int solid = 0, candidate = 0;
    auto freeze = [&](int x) { val[x] = solid++; };
    std::vector<int> p(n); for (int i = 0; i < n; i++) p[i] = i;
    orc::dotnet::sort(p, [&](int x, int y) {
        if (val[x] == n && val[y] == n) { if (x == candidate) freeze(x); else freeze(y); }
        if (val[x] == n) candidate = x; else if (val[y] == n) candidate = y;
        return val[x] < val[y] ? -1 : (val[x] > val[y] ? 1 : 0);
    });
    std::vector<uint32_t> k(n); for (int i = 0; i < n; i++) k[i] = 1u + (uint32_t)val[i];
    return k;
}
static int check(const Rows& R, int n, long long& sorts) {
    const std::vector<int> a = product_sort(R, n), b = oracle_sort(R, n);
    sorts++;
    if (a != b) {
        printf("MISMATCH mode %d n %d\n", R.mode, n);
        for (int i = 0; i < n; i++) printf("%d:%d/%d ", i, a[i], b[i]);
        printf("\n");
        return 1;
    }
    return 0;
}
int main(int argc, char** argv) {
    if (argc > 1 && !strcmp(argv[1], "dump")) {       // <mode> <n> then n values (score bits as hex / keys), then the sorted order
        std::mt19937 rng((unsigned)atoi(argv[2])); const int rounds = atoi(argv[3]);
        for (int r = 0; r < rounds; r++) for (int n : SIZES) for (int mode = 0; mode < 3; mode++) {
            const Rows R = random_rows(rng, n, mode);
            const std::vector<int> p = product_sort(R, n);
            printf("%d %d", mode, n);
            for (int i = 0; i < n; i++) { if (mode == 0) { uint32_t u; memcpy(&u, &R.sc[i], 4); printf(" %08x", u); } else printf(" %u", R.key[i]); }
            printf(" |");
            for (int i = 0; i < n; i++) printf(" %d", p[i]);
            printf("\n");
        }
        return 0;
    }
    const int rounds = argc > 1 ? atoi(argv[1]) : 20;
    std::mt19937 rng(20261017);
    long long sorts = 0; int bad = 0;
    for (int n : SIZES)
        for (int mode = 0; mode < 3; mode++)
            for (int r = 0; r < rounds; r++) { bad += check(random_rows(rng, n, mode), n, sorts); if (bad > 3) return 1; }
    const long long heapBefore = g_branch[2];
    for (int mode = 1; mode <= 2; mode++) {
        Rows R; R.mode = mode; R.sc.assign(BCL_WIDE_MAX_N, 0.f); R.key = adversary_keys(BCL_WIDE_MAX_N);
        if (mode == 2) for (auto& k : R.key) k = (uint32_t)BCL_WIDE_MAX_N + 1 - k;       // the same sequence of compares under the reversed comparison
        bad += check(R, BCL_WIDE_MAX_N, sorts);
    }
    if (g_branch[2] == heapBefore) { printf("the adversary input did not reach the heapsort fallback\n"); return 1; }
    if (bad) return 1;
    printf("OK %lld %lld %lld %lld %d\n", sorts, g_branch[0], g_branch[1], g_branch[2], g_deepest);
    return 0;
}
