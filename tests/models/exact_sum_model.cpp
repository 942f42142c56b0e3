// Host model of field_stats' exact sums: infidex_amd/csrc/exact_sum.h, UNCHANGED, doing on the host what k_field_stats and the engine do with it — the
// column's scale, every value's limbs added into signed 64-bit sums, the sums recombined and rounded.  tests/test_exact_sum_model.py compiles it, feeds it
// cases and checks every figure against fractions.Fraction and math.fsum.
//   stdin    per case:  <kind> <n>  then n lines  <raw value, 16 hex digits> <times it occurs>
//   stdout   per case:  <summable> <scale> <nlimbs> <S0> <S1> <S2> <S3> <count> <nan> <+inf> <-inf> <sum bits> <mean bits or -> <int128 hi> <int128 lo>
//            (hex for the bit patterns and the int128 halves; a case that is not summable prints its first three figures only)
#define XS_FN static inline
#include "exact_sum.h"

#include <cinttypes>
#include <cstdio>
#include <vector>

int main() {
    int kind; unsigned long long n;
    while (scanf("%d %llu", &kind, &n) == 2) {
        std::vector<uint64_t> vals(n); std::vector<uint64_t> times(n);
        for (unsigned long long i = 0; i < n; i++) { unsigned long long v, t; if (scanf("%llx %llu", &v, &t) != 2) return 2; vals[i] = v; times[i] = t; }
        XsScale sc;
        const bool ok = xs_column_scale(vals.data(), n, kind, &sc);
        if (!ok) { printf("0 %d %u\n", sc.scale, sc.nlimbs); continue; }
        int64_t S[XS_MAX_LIMBS] = {0, 0, 0, 0}; uint64_t cls[4] = {0, 0, 0, 0};
        for (unsigned long long i = 0; i < n; i++) {
            uint32_t neg, limb[XS_MAX_LIMBS];
            const uint32_t c = xs_limbs(vals[i], kind, sc.scale, &neg, limb);
            cls[c] += times[i];
            if (c != XS_FINITE) continue;
            for (uint32_t k = sc.nlimbs; k < XS_MAX_LIMBS; k++) if (limb[k]) return 3;      // nothing above the column's width
            for (uint32_t k = 0; k < sc.nlimbs; k++) { const int64_t x = (int64_t)((uint64_t)limb[k] * times[i]); S[k] += neg ? -x : x; }
        }
        const uint32_t count = (uint32_t)(cls[XS_FINITE] + cls[XS_PINF] + cls[XS_NINF]);
        const XsWide W = xs_recombine(S, sc.nlimbs);
        uint64_t lo; int64_t hi; xs_sum_int128(W, &lo, &hi);
        printf("1 %d %u %" PRId64 " %" PRId64 " %" PRId64 " %" PRId64 " %u %" PRIu64 " %" PRIu64 " %" PRIu64 " %016" PRIx64 " ", sc.scale, sc.nlimbs, S[0], S[1], S[2], S[3], count,
               cls[XS_NAN], cls[XS_PINF], cls[XS_NINF], xs_sum_bits(W, sc.scale, (uint32_t)cls[XS_PINF], (uint32_t)cls[XS_NINF]));
        if (count) printf("%016" PRIx64, xs_mean_bits(W, sc.scale, count, (uint32_t)cls[XS_PINF], (uint32_t)cls[XS_NINF])); else printf("-");
        printf(" %016" PRIx64 " %016" PRIx64 "\n", (uint64_t)hi, lo);
    }
    return 0;
}
