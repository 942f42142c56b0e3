// Host model of list_group_members' slot walk: infidex_amd/csrc/group_members.h, UNCHANGED, over std::atomic slots whose "minimum into memory, return what was
// there" is a compare-and-swap loop.  Every run ends with its slots held to std::sort: slot j is the j-th smallest composite of the stream, the slots beyond
// the stream are empty.  tests/test_group_members_model.py compiles and runs it plain, under -fsanitize=thread and under -fsanitize=address,undefined.
//   single thread   every permutation of 7 distinct composites into N = 1 .. 4 slots; random streams of 0, 1, N-1, N, N+1 and 5000 composites with many equal
//                   keys for N in {1, 2, 3, 7, 16}
//   eight threads   one row fed from eight threads at once; and the kernel's two levels: four groups of two threads, each group with a table of its own
//                   ("LDS"), merged by the group's threads into one shared table ("global") with the same gm_insert while the other groups still run
// Prints "OK <permutation runs> <single-thread streams> <eight-thread runs> <two-level runs>"; any mismatch prints it and exits 1.
#define GH_FN static inline
#define GM_FN static inline
#include "group_members.h"

#include <algorithm>
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <random>
#include <thread>
#include <vector>

struct Slots {
    std::atomic<uint64_t>* s;
    uint64_t read(uint32_t j) const { return s[j].load(std::memory_order_relaxed); }
    uint64_t take_min(uint32_t j, uint64_t v) const {
        uint64_t old = s[j].load(std::memory_order_relaxed);
        while (old > v && !s[j].compare_exchange_weak(old, v, std::memory_order_relaxed)) {}
        return old;
    }
};
struct Row {
    uint32_t n; std::unique_ptr<std::atomic<uint64_t>[]> s;
    explicit Row(uint32_t n_) : n(n_), s(new std::atomic<uint64_t>[n_]) { for (uint32_t j = 0; j < n; j++) s[j].store(GH_EMPTY); }
    Slots mem() const { return Slots{s.get()}; }
};

static void die(const char* what, uint32_t N, size_t len, uint32_t j, uint64_t got, uint64_t want) {
    std::printf("MISMATCH %s N=%u stream=%zu slot=%u got=%016llx want=%016llx\n", what, N, len, j, (unsigned long long)got, (unsigned long long)want);
    std::exit(1);
}
// the row against the sorted stream, slot by slot, empties behind
static void hold(const char* what, const Row& R, std::vector<uint64_t> stream) {
    std::sort(stream.begin(), stream.end());
    for (uint32_t j = 0; j < R.n; j++) {
        const uint64_t want = j < stream.size() ? stream[j] : GH_EMPTY, got = R.s[j].load();
        if (got != want) die(what, R.n, stream.size(), j, got, want);
    }
}
// len composites with distinct documents and keys from 1 .. keys (many ties), in random order
static std::vector<uint64_t> stream_of(std::mt19937_64& rng, size_t len, uint32_t keys) {
    std::vector<uint64_t> v(len);
    std::vector<uint32_t> doc(len);
    for (size_t i = 0; i < len; i++) doc[i] = (uint32_t)i * 3u + 1u;
    std::shuffle(doc.begin(), doc.end(), rng);
    for (size_t i = 0; i < len; i++) v[i] = gh_composite(1u + (uint32_t)(rng() % keys), doc[i]);
    return v;
}

int main() {
    std::mt19937_64 rng(20240611);
    long perms = 0, streams = 0, flat = 0, two = 0;
    // every permutation of seven composites, two of them sharing each key
    for (uint32_t N = 1; N <= 4; N++) {
        std::vector<uint64_t> v;
        for (uint32_t i = 0; i < 7; i++) v.push_back(gh_composite(1u + i / 2u, 10u + ((i * 5u) % 7u)));
        std::sort(v.begin(), v.end());
        do {
            Row R(N);
            for (uint64_t c : v) gm_insert(R.mem(), N, c);
            hold("permutation", R, v);
            perms++;
        } while (std::next_permutation(v.begin(), v.end()));
    }
    const uint32_t NS[] = {1, 2, 3, 7, 16};
    for (uint32_t N : NS) {
        const size_t lens[] = {0, 1, N - 1, N, N + 1, 5000};
        for (size_t len : lens)
            for (uint32_t keys : {1u, 3u, 50u}) {
                const std::vector<uint64_t> v = stream_of(rng, len, keys);
                Row R(N);
                for (uint64_t c : v) gm_insert(R.mem(), N, c);
                hold("stream", R, v);
                streams++;
            }
    }
    // eight threads, one row
    const uint32_t MT[] = {1, 2, 3, 4, 7, 16};
    for (uint32_t N : MT) {
        const size_t lens[] = {0, 1, N, N + 1, 100, 5000};
        for (size_t len : lens)
            for (uint32_t keys : {1u, 4u}) {
                const std::vector<uint64_t> v = stream_of(rng, len, keys);
                {
                    Row R(N);
                    std::vector<std::thread> th;
                    for (size_t t = 0; t < 8; t++)
                        th.emplace_back([&, t] { for (size_t i = t; i < v.size(); i += 8) gm_insert(R.mem(), N, v[i]); });
                    for (auto& x : th) x.join();
                    hold("eight threads", R, v);
                    flat++;
                }
                {
                    // four groups of two threads: a table per group, merged into the shared one by the group's own threads
                    Row G(N);
                    std::vector<std::thread> groups;
                    for (size_t g = 0; g < 4; g++)
                        groups.emplace_back([&, g] {
                            Row L(N);
                            std::thread a([&] { for (size_t i = 2 * g; i < v.size(); i += 8) gm_insert(L.mem(), N, v[i]); });
                            std::thread b([&] { for (size_t i = 2 * g + 1; i < v.size(); i += 8) gm_insert(L.mem(), N, v[i]); });
                            a.join(); b.join();                                        // (the workgroup's barrier)
                            auto merge = [&](uint32_t first) { for (uint32_t j = first; j < N; j += 2) { const uint64_t c = L.s[j].load(); if (c != GH_EMPTY) gm_insert(G.mem(), N, c); } };
                            std::thread c([&] { merge(0); });
                            std::thread d([&] { merge(1); });
                            c.join(); d.join();
                        });
                    for (auto& x : groups) x.join();
                    hold("two levels", G, v);
                    two++;
                }
            }
    }
    std::printf("OK %ld %ld %ld %ld\n", perms, streams, flat, two);
    return 0;
}
