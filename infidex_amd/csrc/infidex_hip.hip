// libinfidex_hip.so — device side + C ABI (include/infidex_hip.h). gfx950 (MI355X) only.
//
// Replaces, for a BATCH of queries on a device-resident index shard:
//   Bm25Scorer.Search + TieredCandidateSelector.SelectCandidates   (Indexing/Bm25Scorer.cs:56-193,
//        Scoring/TieredCandidateSelector.cs:53-237)        -> k_accumulate + k_select
//   CoverageEngine.CalculateFeatures + FusionScorer.Calculate      (Coverage/CoverageEngine.cs:174-382,
//        Scoring/FusionScorer.cs:19-236)                    -> k_stage2   (stage2.hip.inc)
//
// Stage-1 design (HBM-bound integer/byte streaming, no MFMA): the doc-id space is cut into ranges of R docs. One
// wave (= one 64-thread workgroup) owns one (query, range): the fp32 partial scores and the tier flags of the R docs
// live in LDS; every posting list of the query is read exactly once, coalesced, from the slice that falls in the
// range (located through a per-term range skip table); a wave executes its LDS read-modify-writes in program order, so
// the per-document accumulation order is the reference's term order with no barriers and no atomics. Candidate tiers
// (quirk Q11) are evaluated from per-doc flags; a range that holds no candidate-generating posting exits before it
// streams anything else (range-granular WAND skip). Survivors are compacted with wave ballots into a batch arena and
// k_select picks the top-`depth` per query with an LDS radix select + bitonic sort.
#include <type_traits>
#include <cstring>
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>
#include <stdio.h>
#include <string>
#include <vector>
#include <unordered_map>
#include <algorithm>
#include <map>
#include <mutex>
#include <chrono>
#include <thread>
#include <dlfcn.h>
#include <rccl/rccl.h>          // types and enums only: the functions are resolved with dlopen (rccl_api)
#include "../../include/infidex_hip.h"
#include "unicode_tables.h"        // generated: BMP simple case mappings, letter set (tools/gen_unicode_tables.py)

#define WAVE 64
#define FILT_MAXCOL 64

static thread_local std::string g_err;
static int32_t fail(int32_t code, const char* fmt, const char* a = "") {
    char buf[512]; snprintf(buf, sizeof buf, fmt, a); g_err = buf; return code;
}
#define HIPCHK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) return fail(INFX_EHIP, #x ": %s", hipGetErrorString(e_)); } while (0)
// Start of an API call: select the index's device and drop whatever error an EARLIER runtime call of this thread left behind — the library checks
// hipGetLastError() after its launches, and a stale error of someone else's call (torch next door leaves "invalid device ordinal" / "peer access already
// enabled" behind as a matter of course) would otherwise be reported as the failure of the first launch that follows.
static inline hipError_t enter_device(int device) { const hipError_t e = hipSetDevice(device); (void)hipGetLastError(); return e; }

// ---------------------------------------------------------------------------------------------------------------
struct DevIndex {
    int32_t N, T, R, rshift, nRanges, docBase, totalDocs;
    const uint64_t* postOff; const int32_t* postDoc; const uint8_t* postW;
    const float* docNorm;      // K1*((1-B) + (B/avgdl)*dl) — the 8-lane formula of Bm25Scorer.cs:413-416
    const float* docLen;       // VectorModel._docLengths (the scalar-tail formula of ComputeTermScore needs dl / avgdl, k_exact1)
    const uint8_t* deleted;    // Document.Deleted per GLOBAL internal id (nullptr = nothing deleted)
    const int64_t* docKey;
    const uint64_t* textOff; const uint16_t* text;
    const uint32_t* skipIdx;   // per term: first entry in skipTbl, or 0xFFFFFFFF
    const uint32_t* skipTbl;   // nRanges+1 offsets (relative to postOff[t]) per skipped term
    const uint32_t* psSkip;    // per prefix DocSet: first entry in psSkipTbl, or 0xFFFFFFFF
    const uint32_t* psSkipTbl; // nRanges+1 offsets (relative to psOff[k]) per skipped set
    const int32_t* wmExact;    // WordMatcher exact-word doc lists (infx_upload_wordmatcher), global ids
    const int32_t* wmLd1;      // WordMatcher symmetric-delete doc lists
    const int64_t* docKeyAll;  // DocumentKey by GLOBAL internal id (== docKey when unsharded)
    int packed;                // 1: postDoc entries are (doc << 8) | tf (shards below 2^24 - 1 documents), 0: plain doc ids + postW
    const uint64_t* psOff; const int32_t* psDocs; uint32_t nSets;
    // Pre-filters (infx_stream_set_doc_masks): per query of the batch its own Deleted flags — the mask of its pre-filter, or `deleted` for a query without
    // one — by GLOBAL internal id; entries [0, nd) belong to the Stage-1 queries, [nd, nd + nq) to the fused queries.  nullptr unless the batch has a
    // pre-filtered query: every query then reads `deleted`.
    const uint8_t* const* qDeleted;
};
// Document.Deleted flags of query q (nullptr = nothing deleted).  Wave-uniform: read once per wave / workgroup, never per posting.
__device__ __forceinline__ const uint8_t* q_deleted(const DevIndex& ix, uint32_t q) { return ix.qDeleted ? ix.qDeleted[q] : ix.deleted; }

// Main streams of the sessions, one pool per device for the whole process.  The runtime serves the streams of a process from a pool of hardware queues per
// priority (4 by default): a stream created once that pool is full is put on the queue with the fewest streams, busy or idle, the most recently created first
// among equals, and kernels of streams on one queue run one after the other.  With a stream per session created as the sessions came, the engine's own (idle)
// session and the null stream held two of the four queues and the main streams of four sessions shared the other two (profiles/hwqueues_default.md).  The first
// infx_create on a device therefore creates the main streams up front, before the uploads touch the null stream, and every session of every index on that device
// draws the one with the fewest users: four sessions, four queues.  PRECONDITION: nothing else in the process has created HIP streams on the device before that
// first infx_create; where a host program has, the pool's streams are placed by the runtime's sharing rule like any others and may share queues.  Users beyond
// the pool share a stream, which is what the runtime would do with their queues.  INFX_MAIN_STREAMS (1..32, default 4) sizes the pool for processes that run
// with more queues.  The streams live as long as the process.
struct MainPool { std::mutex mu; std::vector<hipStream_t> st; std::vector<int> users; };
static int32_t main_pool(int device, MainPool** out);

struct infx_index {
    infx_config cfg;
    DevIndex d{};
    std::vector<void*> allocs;
    bool havePostings = false, haveDocs = false, haveWm = false;
    uint64_t nWmExact = 0, nWmLd1 = 0;
    float avgdl = 0.f;
    std::vector<uint64_t> hPostOff;   // host copy of the (padded) list starts
    std::vector<uint64_t> hPostLen;   // true list lengths
    std::vector<int32_t> hDf;
    std::vector<uint32_t> hSkipIdx;   // host copy of DevIndex::skipIdx (filled by infx_upload_postings)
    uint8_t* dDeleted = nullptr;      // device copy of the global Document.Deleted flags (infx_set_deleted)
    int32_t* dFirstLive = nullptr; uint32_t firstLiveCap = 0; const int32_t* firstLive = nullptr;      // first live document of each document's key, by GLOBAL internal id (infx_set_first_live; nullptr: keys are unique)
    const uint32_t* colCodes[FILT_MAXCOL] = {}; uint32_t colValues[FILT_MAXCOL] = {}; uint32_t colDocs[FILT_MAXCOL] = {}; uint32_t colCap[FILT_MAXCOL] = {};   // device-resident columns (infx_upload_column)
    const uint32_t* colRank[FILT_MAXCOL] = {}; uint32_t colRankCap[FILT_MAXCOL] = {}; bool colRankOk[FILT_MAXCOL] = {};     // sort ranks of their codes (infx_upload_sort_rank); a column re-upload voids its rank
    const uint32_t* colTie[FILT_MAXCOL] = {}; uint32_t colTieCap[FILT_MAXCOL] = {}; bool colTieOk[FILT_MAXCOL] = {};        // facet tie order of their codes (infx_upload_group_rank, for infx_top_groups); a column re-upload voids it
    // raw values of their codes with the scale field_stats sums them at (infx_upload_column_values); a column re-upload voids them too
    const uint64_t* colBits[FILT_MAXCOL] = {}; uint32_t colBitsCap[FILT_MAXCOL] = {}; bool colBitsOk[FILT_MAXCOL] = {}; int32_t colKind[FILT_MAXCOL] = {}, colScale[FILT_MAXCOL] = {}; uint32_t colLimbs[FILT_MAXCOL] = {};
    // list columns (infx_upload_list_column): the CSR pair of each, and the staging buffer of infx_list_leaf_build's leaf bitmaps
    const uint32_t* listOff[INFX_MAX_LIST_COLS] = {}; const uint32_t* listCode[INFX_MAX_LIST_COLS] = {}; uint32_t listDocs[INFX_MAX_LIST_COLS] = {}, listValues[INFX_MAX_LIST_COLS] = {};
    size_t listOffCap[INFX_MAX_LIST_COLS] = {}, listCodeCap[INFX_MAX_LIST_COLS] = {}; uint32_t* listMaps = nullptr; size_t listMapsCap = 0;
    std::vector<uint64_t> hPsOff;
    int rank = 0, nranks = 1;
    ncclComm_t comm = nullptr;         // infx_set_shard_comm
    struct DevLookup* lk = nullptr;    // dictionaries / term trie of the device-side planning lookups (lookup.hip.inc); owned, freed by infx_destroy
    // Turnstile of the full-width phase (k_accumulate .. k_select) between the streams of an index: see infx_search_fused
    std::mutex turnMu; hipEvent_t turnEvent = nullptr;
    struct MainPool* pool = nullptr;   // the device's main streams (below); owned by the process
    bool haveDict = false, haveTrie = false;
    uint32_t postRows = INFX_FILTER_MAX_ROWS;      // rows per query the post-filter / facets / boosts / sort-by / browse accept (infx_set_post_rows)
    bool hasAlias = false;            // the corpus text holds one of the 22 OrdinalIgnoreCase alias characters (infx_upload_docs counts them): Stage 2 runs its ALIAS instantiation
};

template <class Tp> static hipError_t dalloc(infx_index* ix, Tp** p, size_t n) {
    void* v = nullptr; hipError_t e = hipMalloc(&v, std::max<size_t>(n, 1) * sizeof(Tp));
    if (e == hipSuccess) { ix->allocs.push_back(v); *p = (Tp*)v; }
    return e;
}

template <class Tp> static int32_t dcopy(infx_index* ix, const Tp** out, const Tp* src, size_t n) {
    Tp* d = nullptr;
    HIPCHK(dalloc(ix, &d, n));
    if (n) HIPCHK(hipMemcpy(d, src, n * sizeof(Tp), hipMemcpyHostToDevice));
    *out = d; return INFX_OK;
}

// ---------------------------------------------------------------------------------------------------------------
// Device posting layout: every list starts on a 16-byte boundary and is padded to a multiple of 4 postings with the sentinel doc id
// 0x7F7F7F7F (beyond any real id).  k_accumulate streams lists with 16-byte loads from an aligned-down address; with this layout the
// extra elements of a group are either postings of the SAME list outside the block's doc range or sentinels, so a plain range check
// replaces the per-posting index check.  One thread per posting: find its list (upper bound in the unpadded offsets), copy.
__global__ void k_pad_lists(const uint64_t* __restrict__ offs, const uint64_t* __restrict__ offs2, uint32_t T, uint64_t P,
                            const int32_t* __restrict__ inDoc, const uint8_t* __restrict__ inW, int32_t* __restrict__ outDoc, uint8_t* __restrict__ outW, int packed) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= P) return;
    uint64_t lo = 0, hi = (uint64_t)T + 1;                      // first index with offs[idx] > i
    while (lo < hi) { uint64_t m = (lo + hi) >> 1; if (offs[m] <= i) lo = m + 1; else hi = m; }
    const uint64_t t = lo - 1;
    const uint64_t dst = offs2[t] + (i - offs[t]);
    outDoc[dst] = packed ? (int32_t)(((uint32_t)inDoc[i] << 8) | inW[i]) : inDoc[i]; outW[dst] = inW[i];
}

// skip table build: one thread per (skipped term, range boundary)
__global__ void k_build_skip(const uint64_t* postOff, const int32_t* postDoc, const uint32_t* skipTerms, uint32_t nSkip,
                             uint32_t* skipTbl, int nRanges, int rshift, int packed) {
    uint64_t gid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    uint64_t per = (uint64_t)nRanges + 1;
    if (gid >= (uint64_t)nSkip * per) return;
    uint32_t s = (uint32_t)(gid / per); int r = (int)(gid % per);
    uint32_t t = skipTerms[s];
    uint64_t lo = postOff[t], hi = postOff[t + 1];
    int64_t target = (int64_t)r << rshift;
    uint64_t a = lo, b = hi;
    while (a < b) { uint64_t m = (a + b) >> 1; if ((int64_t)(packed ? (int32_t)((uint32_t)postDoc[m] >> 8) : postDoc[m]) < target) a = m + 1; else b = m; }
    skipTbl[(uint64_t)s * per + r] = (uint32_t)(a - lo);
}

__global__ void k_doc_norm(const float* docLen, float* norm, int n, float bDivAvg) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float k1 = 1.2f, minDl = 1.f - 0.75f;
    float t1 = bDivAvg * docLen[i];
    float t2 = minDl + t1;
    norm[i] = k1 * t2;
}

// ---------------------------------------------------------------------------------------------------------------
struct DevTerm {           // per (query term), device layout
    uint64_t begin, end;   // absolute posting slice in postDoc/postW, or in extraDocs for virtual terms
    float idf;
    uint32_t skip;         // skipTbl base or 0xFFFFFFFF
    uint8_t role, rank, isVirtual, pad;   // pad = fuzzy-union dedupe group (member-list terms), 0 = none
    uint16_t refIdx, pad2; // position of the term in the query's Bm25Scorer order (member lists share their virtual term's position)
};
struct DevQuery {
    uint32_t termOff, numTerms;
    int32_t mode, prefixSet, depth, nAnd;
    uint32_t refOff, numRef;   // the query's terms as the caller passed them (Bm25Scorer order): DevRefTerm[refOff .. +numRef)
};
struct SelRule {           // decided on the host from the (global) class counts
    int32_t mode;          // INFX_MODE_*
    int32_t cutoffRank;    // DISJ: include class&0x7F <= cutoff
    uint32_t classMask;    // AND: include if (class & classMask) != 0
    int32_t depth;
    uint32_t total;        // upper bound on the number of entries the rule lets through
    uint32_t pad;
};

template <class Tp> __device__ __forceinline__ Tp rfl(Tp v) { return v; }
__device__ __forceinline__ int rfl_i(int v) { return __builtin_amdgcn_readfirstlane(v); }
__device__ __forceinline__ uint64_t rfl_u64(uint64_t v) {
    uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)v), hi = __builtin_amdgcn_readfirstlane((uint32_t)(v >> 32));
    return ((uint64_t)hi << 32) | lo;
}

// posting lists of a packed index hold (doc << 8) | tf; sentinels are 0xFFFFFFFF
__device__ __forceinline__ int32_t post_doc(int32_t v, int packed) { return packed ? (int32_t)((uint32_t)v >> 8) : v; }
__device__ __forceinline__ uint64_t lower_bound_post(const int32_t* a, uint64_t lo, uint64_t hi, int32_t target, int packed) {
    while (lo < hi) { uint64_t m = (lo + hi) >> 1; if (post_doc(a[m], packed) < target) lo = m + 1; else hi = m; }
    return lo;
}
__device__ __forceinline__ uint64_t lower_bound_i32(const int32_t* a, uint64_t lo, uint64_t hi, int32_t target) {
    while (lo < hi) { uint64_t m = (lo + hi) >> 1; if (a[m] < target) lo = m + 1; else hi = m; }
    return lo;
}

#include "stage1.hip.inc"
#include "stage1_sparse.hip.inc"
#include "exact1.hip.inc"
#include "exact3.hip.inc"
#include "exactsh.hip.inc"
#include "stage2.hip.inc"

// TieredCandidateSelector tier rules evaluated from class counts (see header of this file / DESIGN.md)
__host__ __device__ static inline SelRule make_rule0(const infx_query& Q, const uint32_t* c) {
    SelRule r{}; r.mode = Q.mode; r.depth = Q.depth; r.cutoffRank = 127; r.classMask = 0xFFFFFFFFu;
    const long k = Q.depth;
    if (Q.mode == INFX_MODE_AND) {
        unsigned long long t0 = 0, t1 = 0;
        for (int i = 0; i < 16; i++) { if (i & 1) t0 += c[i]; if (i & 2) t1 += c[i]; }
        if ((long)t0 >= k * 2) { r.classMask = 1; return r; }                       // Tier 0 alone (:160-161)
        unsigned long long g = t0; uint32_t gmask = 1;
        if (Q.n_and >= 3 && (long)t0 < k * 3) { g = t1; gmask = 2 | 1; }            // Tier 1 (:165-171); T1 contains T0
        if ((long)g < k * 5) {                                                      // Tier 2 (:174-234)
            if (Q.df_s1 <= 0) { r.classMask = gmask; return r; }
            if ((long)Q.df_s1 >= k * 10 || Q.df_s2 <= 0) { r.classMask = 4 | gmask; return r; }   // G u S1 == S1
            r.classMask = 4 | 8 | gmask; return r;
        }
        r.classMask = gmask; return r;
    }
    if (Q.mode == INFX_MODE_DISJ) {
        // SelectCandidatesDisjunctive (:260-319): ranks [0, n_and) are not low-quality, the rest are
        int nElig = Q.n_and; bool hasSel = false; long local = 0; int cutoff = -1;
        int nRanks = 0; for (int i = 127; i >= 0; i--) if (c[i]) { nRanks = i + 1; break; }
        int totalRanks = nRanks > Q.df_s1 ? nRanks : Q.df_s1;   // df_s1 carries the number of ranks in DISJ mode
        for (int i = 0; i < totalRanks; i++) {
            bool lowq = i >= nElig;
            if (totalRanks > 1 && lowq && hasSel) continue;
            cutoff = i; local += c[i];
            if (!lowq && local > 0) hasSel = true;
            if (local >= k * 100) break;
        }
        r.cutoffRank = cutoff; return r;
    }
    return r;
}

__host__ __device__ static inline SelRule make_rule(const infx_query& Q, const uint32_t* c) {
    SelRule r = make_rule0(Q, c);
    unsigned long long tot = 0;
    if (Q.mode == INFX_MODE_AND) { for (int i = 0; i < 16; i++) if (i & r.classMask) tot += c[i]; }
    else if (Q.mode == INFX_MODE_DISJ) { for (int i = 0; i <= r.cutoffRank && i < 128; i++) tot += c[i]; tot += 128; /* pre-seen docs (< 100) are not in the histogram */ }
    else tot = c[1];
    r.total = (uint32_t)(tot < 0xFFFFFFFFull ? tot : 0xFFFFFFFFull); r.pad = 0;
    return r;
}

#include "fused.hip.inc"
#include "lookup.hip.inc"
#include "filter.hip.inc"
#include "browse.hip.inc"
#include "facets_filtered.hip.inc"
#include "list_columns.hip.inc"
#include "listing.hip.inc"
#include "ranges.hip.inc"
#include "stats.hip.inc"
#include "bucket_stats.hip.inc"
#include "groups.hip.inc"
#include "group_members.hip.inc"
#include "top_groups.hip.inc"
#include "distinct.hip.inc"
#include "quantiles.hip.inc"
#include "bclsort.hip.inc"
#include "postproc.hip.inc"
#include "collapse.hip.inc"
#include "highlight.hip.inc"

// ---------------------------------------------------------------------------------------------------------------
struct infx_filter {
    infx_index* ix; DevFilter d{}; uint32_t nops = 0, nleaves = 0; void *dOps = nullptr, *dLeaves = nullptr, *dTables = nullptr;
    std::vector<infx_filter_leaf> hLeaves;      // host copy of the leaves: the columns k_filter_count_multi loads for it
};
static int32_t check_filter_prog(infx_index* ix, uint32_t nops, const infx_filter_op* ops, uint32_t nleaves, const infx_filter_leaf* leaves, uint32_t ntable_words);

// The filter programs of one launch sequence on their way to the device; nothing else knows how they are laid out.  An entry is either
//   - packed: its ops, leaves and tables lie in `code`, each 16-byte aligned (opsOff / leavesOff / tablesOff: byte offsets into code), or
//   - resident: an infx_filter, whose device copy is the program and whose hLeaves are its host leaves.
// On the device a table is DevFilter[size()] and, wherever the caller puts it, the code the packed entries point into.  The usual blob is the table,
// padded to 16 bytes, then the code (blob_bytes / put_blob, table_upload); the finalize places the two parts inside its own upload (put).
struct ProgTable {
    struct Entry { uint32_t nops, nleaves, opsOff, leavesOff, tablesOff; const infx_filter* resident; };
    std::vector<Entry> progs; std::vector<uint8_t> code;
    static size_t al16(size_t x) { return (x + 15) & ~(size_t)15; }
    uint32_t size() const { return (uint32_t)progs.size(); }
    void clear() { progs.clear(); code.clear(); }
    void add(const infx_filter* f) { progs.push_back(Entry{0, 0, 0, 0, 0, f}); }
    // replaces the table by programs [0, n), packed, each validated as infx_filter_create does
    int32_t pack(infx_index* ix, uint32_t n, const infx_filter_prog* src) {
        clear();
        auto put = [&](const void* p, size_t bytes) { const size_t o = al16(code.size()); code.resize(o + bytes); if (bytes) std::memcpy(code.data() + o, p, bytes); return (uint32_t)o; };
        for (uint32_t i = 0; i < n; i++) {
            const infx_filter_prog& P = src[i];
            if (!P.nops || !P.ops || (P.nleaves && (!P.leaves || !P.tables))) return fail(INFX_EINVAL, "null filter program%s");
            { int32_t rc_ = check_filter_prog(ix, P.nops, P.ops, P.nleaves, P.leaves, P.ntable_words); if (rc_) return rc_; }
            Entry Q{P.nops, P.nleaves, 0, 0, 0, nullptr};
            Q.opsOff = put(P.ops, (size_t)P.nops * sizeof(infx_filter_op));
            Q.leavesOff = put(P.leaves, (size_t)P.nleaves * sizeof(infx_filter_leaf));
            Q.tablesOff = put(P.tables, (size_t)P.ntable_words * 4);
            progs.push_back(Q);
        }
        if (code.size() > 0xFFFFFFF0ull) return fail(INFX_ECAPACITY, "the batch's filter programs exceed 4 GiB%s");
        return INFX_OK;
    }
    // program p as the kernels read it, the code at dCode on the device
    DevFilter dev(uint32_t p, const char* dCode) const {
        const Entry& P = progs[p];
        if (P.resident) return P.resident->d;
        return DevFilter{(const infx_filter_op*)(dCode + P.opsOff), P.nops, (const infx_filter_leaf*)(dCode + P.leavesOff), P.nleaves, (const uint32_t*)(dCode + P.tablesOff)};
    }
    // adds the columns program p reads to cc, each once, in the order they are met (the kernels load a document's codes of these columns once for all programs)
    void add_columns(DevCountCols& cc, uint32_t p) const {
        const Entry& P = progs[p];
        const infx_filter_leaf* L = P.resident ? P.resident->hLeaves.data() : (const infx_filter_leaf*)(code.data() + P.leavesOff);
        const uint32_t nl = P.resident ? (uint32_t)P.resident->hLeaves.size() : P.nleaves;
        for (uint32_t l = 0; l < nl; l++) {
            const uint32_t c = L[l].col;
            if (c < FILT_MAXCOL && !(cc.slot[c] < cc.nUsed && cc.col[cc.slot[c]] == c)) { cc.slot[c] = (uint8_t)cc.nUsed; cc.col[cc.nUsed++] = c; }
        }
    }
    DevCountCols columns(uint32_t first, uint32_t n) const { DevCountCols cc{}; for (uint32_t p = 0; p < n; p++) add_columns(cc, first + p); return cc; }
    size_t table_bytes() const { return progs.size() * sizeof(DevFilter); }
    void put(uint8_t* hTable, uint8_t* hCode, const char* dCode) const {
        for (uint32_t p = 0; p < size(); p++) { const DevFilter f = dev(p, dCode); std::memcpy(hTable + (size_t)p * sizeof(DevFilter), &f, sizeof f); }
        if (!code.empty()) std::memcpy(hCode, code.data(), code.size());
    }
    size_t blob_bytes() const { return al16(table_bytes()) + code.size(); }
    void put_blob(uint8_t* h, const char* d) const { put(h, h + al16(table_bytes()), d + al16(table_bytes())); }
};

// The kinds of calls over document sets ("requests over document sets" below), what a stream keeps of each (ws | out | raw) and what info[] counts of the last call:
enum SetKind {
    SK_LIST,          // infx_list_ordered: select states, histograms, range counts, page composites | the rows.  Histogram passes, kernel launches
    SK_RANGE,         // infx_range_counts: the requests' thresholds | counters, largest and smallest ranks.  Requests, k_range_counts launches
    SK_STATS,         // infx_field_stats: - | the requests' slots and smallest ranks | their host copy.  Requests, k_field_stats launches
    SK_QUANT,         // infx_field_quantiles: quantiles, targets and one pass's rows | counts and ranks | their host copy.  Requests, histogram passes, launches, digit width,
                      // request-passes with rows in LDS / in global memory
    SK_GROUPED,       // infx_list_grouped (its pages in SK_LIST's buffers): a spec's head table and heads mask; per request the page's sorted codes, rows, group codes and sizes | -.
                      // Head passes, histogram passes, kernel launches
    SK_TOP,           // infx_top_groups: [a table's slots and smallest ranks | its requests' composites | histograms | select states] | the requests' pages | their host copy.
                      // Requests, accumulate passes, select passes, launches, tables in a workgroup's LDS / a CU's whole LDS / global memory
    SK_DISTINCT,      // infx_field_distinct: one spec's pair set at a time — [rows | union row] or [hash set | side row] | every spec's [sizes | distinct | whole | overflow] |
                      // their host copy.  Requests, kernel launches, specs marked in LDS / in a global bitmap / in a hash set
    SK_MEMBERS,       // infx_list_group_members (its pages in SK_LIST's buffers): SK_GROUPED's workspace | per request its slots, limit and per_group, the members'
                      // keys, documents and codes, the rows' member counts.  Head passes, histogram passes, member walks, kernel launches
    SK_BUCKETS,       // infx_bucket_stats: the requests' thresholds | the requests' slots and smallest ranks | their host copy.  Requests, k_bucket_stats launches, requests
                      // with slots in a workgroup's LDS / a CU's whole LDS / global memory
    SK_KINDS
};
struct SetKindState {
    void *ws = nullptr, *out = nullptr; size_t capWs = 0, capOut = 0;      // the workspace and the output on the device
    std::vector<uint32_t> raw;                                             // the output as the host unpacks it
    uint32_t info[7] = {0, 0, 0, 0, 0, 0, 0};                              // the counters of the kind's last call, in the order of its infx_last_* reader
};

struct infx_stream {
    infx_index* ix;
    // post-filter / facets (infx_stream_set_postfilter): applied to the rows of every fused / sharded finalize on this stream
    infx_filter* postFilter = nullptr; uint32_t nFacet = 0; uint32_t facetCols[INFX_MAX_FACET_COLS] = {};
    void *dFDocs = nullptr, *dFacetCols = nullptr, *dFacCodes = nullptr, *dFacCounts = nullptr, *dFacN = nullptr;
    size_t capFDocs = 0, capFacCodes = 0, capFacCounts = 0, capFacN = 0;
    std::vector<uint32_t> hFacCodes, hFacCounts, hFacN; uint32_t facetNq = 0, facetNFacet = 0, facetRows = 0;     // facets of the last batch: nq, facet columns, pairs held per (query, column)
    // boosts / sort-by (infx_stream_set_boosts / _set_sort): applied after the post-filter (k_postproc)
    infx_filter* boosts[INFX_MAX_BOOSTS] = {}; int32_t boostStrength[INFX_MAX_BOOSTS] = {}; uint32_t nBoost = 0;
    uint32_t sortCol = 0; bool sortOn = false, sortAsc = false;
    // per-query post-processing of the NEXT batch (infx_stream_set_query_post), consumed by its finalize: the batch's programs,
    // the boost list, one descriptor per query, the programs [0, qpNCount) to count
    bool qpOn = false; uint32_t qpNq = 0, qpNFacet = 0, qpFacetCols[INFX_MAX_FACET_COLS] = {}, qpNCount = 0; uint32_t* qpCountsOut = nullptr;
    ProgTable qpTable; std::vector<DevQBoost> qpBoosts; std::vector<DevQPost> qpDesc;
    uint32_t lastCountK = 0, lastCountLaunches = 0;     // the filter programs the last finalize counted, and its k_filter_count_multi launches
    void* dPostBlob = nullptr; size_t capPostBlob = 0;     // the batch's DevPostBatch + program table + boost list + descriptors (+ packed programs)
    void* dQCount = nullptr; size_t capQCount = 0;
    // pre-filter masks: the stream's mask slots (infx_stream_mask_slot), a staged build (infx_filter_masks, enqueued by the next
    // batch or by infx_stream_wait), the per-query flags of the next batch (infx_stream_set_doc_masks) and their device table (DevIndex::qDeleted while qDelOn)
    uint8_t* dMask[INFX_MAX_PREFILTERS] = {}; size_t capMask[INFX_MAX_PREFILTERS] = {};
    bool mkStaged = false; ProgTable mkTable; DevMaskOut mkOut{}; uint32_t* mkCountsOut = nullptr;
    void* dMaskBlob = nullptr; size_t capMaskBlob = 0; void* dMaskCnt = nullptr; size_t capMaskCnt = 0;
    uint32_t lastMaskBuilt = 0, lastMaskLaunches = 0;
    std::vector<const uint8_t*> docMasks; void* dQDel = nullptr; size_t capQDel = 0; bool qDelOn = false;
    // browse queries (INFX_FQ_BROWSE) of the batch being staged: (query, rows asked), recorded by the prep stage and consumed by the finalize
    std::vector<std::pair<uint32_t, uint32_t>> browseQ;
    std::vector<int32_t> qpRows;      // max_results of each fused query of the batch, kept only by an index with more than INFX_FILTER_MAX_ROWS post rows
    void *dBrwBlob = nullptr, *dBrwWork = nullptr; size_t capBrwBlob = 0, capBrwWork = 0;
    uint32_t lastBrowseGroups = 0, lastBrowseLaunches = 0;      // groups and k_browse_scan launches of the last finalize
    // Query.collapse_by of the NEXT batch (infx_stream_set_query_collapse), consumed by its finalize; the windows and what k_collapse keeps (dClp: one blob);
    // of the last batch: each query's slot (-1: none), the stride, per slot the groups and rows of its list and the rows k_collapse wrote, per such row its document, code and size
    bool clpOn = false; std::vector<infx_collapse_req> clpReq;
    void* dClp = nullptr; size_t capClp = 0;
    std::vector<int32_t> clpSlot, clpDocs, clpFinalDocs; std::vector<uint32_t> clpCodes, clpSizes, clpGroups, clpRanked, clpReturned, clpCounts; uint32_t clpStride = 0; bool clpPosted = false;
    uint32_t lastClpQueries = 0, lastClpLaunches = 0;
    // Query.highlight of the NEXT batch (infx_stream_set_query_highlight), consumed by its finalize.  dHl: one blob — each query's slot and width, then the rows
    // k_highlight writes.  Of the last batch: each query's slot (-1: it did not ask), the strides, the rows as downloaded, each query's row count.
    // hlCs / hlAlias: the matcher settings and the alias flag the batch's Stage 2 ran with (fused_enqueue_prep_stage2 notes them: Stage 2 consumes the settings).
    bool hlOn = false; std::vector<int32_t> hlReq;
    void* dHl = nullptr; size_t capHl = 0;
    std::vector<int32_t> hlSlot; std::vector<uint16_t> hlRows; std::vector<uint32_t> hlCounts; uint32_t hlStride = 0, hlTermStride = 0, hlSnipStride = 0;
    uint32_t lastHlQueries = 0, lastHlLaunches = 0; uint64_t lastHlBytes = 0;
    infx_stage2_setup hlCs{}; bool hlAlias = false; std::vector<int32_t> hlWords;      // hlWords: per query of the batch its Stage-2 word count, -1 for a long query
    hipEvent_t evH0 = nullptr, evH1 = nullptr; bool timedHl = false;      // around k_highlight (created by the first batch that highlights)
    hipEvent_t evK0 = nullptr, evK1 = nullptr; bool timedClp = false;      // around k_collapse (created by the first batch that collapses): evF0 .. evK0 is k_finalize_win
    void* dFacAll = nullptr; size_t capFacAll = 0;              // infx_facets_all counters
    void* dLfCnt = nullptr; size_t capLfCnt = 0;      // infx_list_facets: counters [k][num_values]
    void *dFfBlob = nullptr, *dFfCnt = nullptr; size_t capFfBlob = 0, capFfCnt = 0;      // infx_facets_filtered: the programs' blob; counters [k][sum of num_values] + totals [k]
    uint32_t lastFfProgs = 0, lastFfLaunches = 0;              // programs and k_facets_filtered launches of the last infx_facets_filtered
    SetKindState kind[SK_KINDS];                               // the set calls (infx_list_ordered .. infx_field_distinct): per kind its buffers, raw host copy and counters
    hipStream_t st = nullptr;
    // Planning kernels (k_ld1, k_union count pass) are tiny and the host WAITS for their results (idf needs the union cardinalities): queued behind the
    // streaming kernels of the other batches in flight they came back after 10-15 ms (measured: plan_ms 14.9 per batch of which ~2 ms host work).  They
    // run on a stream of their own with the highest priority the device offers, so their few hundred waves are placed as soon as any CU has room.
    hipStream_t stPlan = nullptr, stMain = nullptr; hipEvent_t evPlan = nullptr;
    int mainSlot = -1;                                             // stMain is the device's MainPool::st[mainSlot]: owned by the process, shared with the users beyond the pool
    hipEvent_t evTurn = nullptr;                                   // end of this stream's k_select: what the next batch's k_accumulate (another stream) waits for
    hipStream_t stAux = nullptr; hipEvent_t evJoin = nullptr;      // INFX_REPLAY_AUX=1 only: the replay's workgroup k_ex_chunk launches run beside the one-wave launch (all are tail-bound)
    hipEvent_t evA0, evA1, evS0, evS1, evC0, evC1, evP0, evP1, evF0, evF1, evX0, evX1, evSync;
    hipEvent_t evXa, evXb, evXc; bool timedReplayParts = false; float msReplayParts[4] = {0, 0, 0, 0};      // inside the replay: after the scan (k_ex_walk x2, k_ex_prefix, k_ex_theta), after the k_ex_chunk launches, after k_ex_heap
    bool timedReplay = false; float msReplay = 0.f; uint32_t lastFlagWhy[4] = {0, 0, 0, 0};     // exact replay of the last batch: kernel time, why its queries were flagged
    // fused pipeline workspaces
    void *dFQ = nullptr, *dFLists = nullptr, *dFOwned = nullptr, *dFS1 = nullptr, *dFMeta = nullptr, *dFQueries = nullptr, *dFKeys = nullptr, *dFScores = nullptr, *dFTies = nullptr, *dFCounts = nullptr, *dFFlags = nullptr, *dFErr = nullptr, *dFHitsAll = nullptr, *dFHcAll = nullptr, *dFPairs = nullptr;
    size_t capFQ = 0, capFLists = 0, capFOwned = 0, capFS1 = 0, capFMeta = 0, capFQueries = 0, capFKeys = 0, capFScores = 0, capFTies = 0, capFCounts = 0, capFFlags = 0, capFErr = 0, capFHitsAll = 0, capFHcAll = 0, capFPairs = 0;
    uint64_t fusedS1 = 0, fusedCands = 0, fusedTextBytes = 0;
    uint32_t fusedNq = 0; int fusedDepth = 0; bool fusedDebug = false, timedFused = false; float msFused[5] = {0, 0, 0, 0, 0};
    // device workspaces (grown on demand)
    void* dQueries = nullptr; size_t capQueries = 0;
    void* dTerms = nullptr; size_t capTerms = 0;
    void* dExtra = nullptr; size_t capExtra = 0;
    void* dRules = nullptr; size_t capRules = 0;
    void* dHits = nullptr; size_t capHits = 0;
    void* dHitCount = nullptr; size_t capHitCount = 0;
    void* dBlockOut = nullptr; size_t capBlockOut = 0;
    void* dBlockOutHi = nullptr; size_t capBlockOutHi = 0;
    void* dQBytes = nullptr; size_t capQBytes = 0; uint32_t lastNqAlloc = 0;
    void* dUOffs = nullptr; size_t capUOffs = 0; void* dUMem = nullptr; size_t capUMem = 0; void* dUCnt = nullptr; size_t capUCnt = 0;
    void* dURange = nullptr; size_t capURange = 0; void* dUBase = nullptr; size_t capUBase = 0; void* dUDocs = nullptr; size_t capUDocs = 0;
    struct PinChunk { char* base; size_t cap, off; }; std::vector<PinChunk> pins;      // pinned staging arena
    struct PendingOut { void* dst; const void* src; size_t bytes; }; std::vector<PendingOut> pendingOut; bool unsynced = false;
    std::vector<uint32_t> unionCount; std::vector<unsigned long long> unionBase{0};   // device-resident unions of the last infx_union_build
    void* dCounts = nullptr; size_t capCounts = 0;
    void* dDense = nullptr; size_t capDense = 0;      // k_accumulate_sparse -> k_accumulate hand-over flags, one byte per (query, stripe)
    void* dCovQ = nullptr; size_t capCovQ = 0;
    void* dCovQL = nullptr; size_t capCovQL = 0; uint32_t nLongQ = 0;      // infx_stage2_long_queries: the long-query table of the next Stage-2 call
    // infx_stream_set_coverage: the matcher settings of the next Stage-2 call (csOn: they differ from the defaults -> the custom-setup instantiations) and the
    // per-query truncation records of the next finalize (finOn; else dFin holds finDefaultN default records)
    bool csOn = false; infx_stage2_setup cs{}; bool finOn = false; std::vector<infx_finalize_setup> finH; void* dFin = nullptr; size_t capFin = 0; uint32_t finDefaultN = 0;
    void* dCovC = nullptr; size_t capCovC = 0;
    void* dCovO = nullptr; size_t capCovO = 0;
    void* dCovF = nullptr; size_t capCovF = 0;
    int32_t* arDoc = nullptr; float* arScore = nullptr; uint8_t* arCls = nullptr; size_t arCap = 0;
    bool accLayoutBad = false;
    bool batchAlias = false, longAlias = false;      // ... or the coverage queries of the batch / its long-query table do
    unsigned long long* arMask = nullptr; size_t arMaskCap = 0; int maskWords = 0;     // per-row hit masks of the last accumulate launch
    void* dWideQ = nullptr; size_t capWideQ = 0; uint32_t nWide = 0;                     // queries of the batch with more than 64 reference terms: beyond the masks, never replayed
    uint32_t* arExc = nullptr; uint32_t* exCand = nullptr; infx_hit* exOut = nullptr; size_t exCap = 0;       // tf exception records, candidate lists, replay rows (arena-sized)
    void* exChunks = nullptr; size_t capExChunks = 0; void* exQueries = nullptr; size_t capExQueries = 0; void* exTasks = nullptr; size_t capExTasks = 0; uint32_t* exCounters = nullptr;
    void* dSelOrder = nullptr; size_t capSelOrder = 0;        // k_select_order: the batch's queries by row count, descending
    void* dAccOrder = nullptr; size_t capAccOrder = 0; uint32_t nAccHeavy = 0xFFFFFFFFu;      // k_accumulate: the batch's queries by row bound, descending, and how many of them go first (~0: query order)
    uint32_t nBoundGiants = 0;                               // queries of the batch whose row bound reaches k_select's multi-workgroup threshold
    void* dSelG = nullptr; size_t capSelG = 0;                // k_selg_hist / k_selg_gather: global histograms, key lists and flags of the batch's largest queries
    void* exContEnd = nullptr; size_t capExContEnd = 0;      // k_ex_cand: candidates up to the end of every (query, container)
    uint32_t exChunkCap = 0; size_t arBound = 0; unsigned long long maxQueryBound = 0;
    void* dDir = nullptr; size_t capDir = 0;
    void* dRefTerms = nullptr; size_t capRefTerms = 0; void* dExactFlag = nullptr; size_t capExactFlag = 0; uint32_t* dExactStat = nullptr;   // k_exact1 inputs
    uint32_t lastExact2[2] = {0, 0};                                                     // last batch: queries replayed exactly, of them by the sequential fallback                                            // (query, range) chunk directory
    unsigned long long* dCursor = nullptr;   // [0]=cursor [1]=algBytes
    uint32_t* dOverflow = nullptr;
    std::vector<infx_query> lastQ;            // kept between accumulate and select
    uint32_t lastNq = 0;
    float msAcc = 0, msSel = 0, msCov = 0;
    uint64_t lastAlgBytes = 0, lastCandTotal = 0;
    bool timedAcc = false, timedSel = false, timedCov = false;
    void* dStats = nullptr;      // k_accumulate profiling counters (INFX_ACC_SKIP=8)
    void* dExProf = nullptr; size_t capExProf = 0;      // INFX_EXACT_PROF: per-query cycle counters of the replay kernels (EXP_WORDS u64 per query)
    // exact replay across document shards (exactsh.hip.inc)
    void *dNext = nullptr, *dPrior = nullptr, *shBlob = nullptr, *dAllBlobs = nullptr, *dAllNext = nullptr, *dChainState = nullptr, *dChainNeed = nullptr;
    size_t capNext = 0, capPrior = 0, capShBlob = 0, capAllBlobs = 0, capAllNext = 0, capChainState = 0, capChainNeed = 0;
    uint32_t shHead[4] = {0, 0, 0, 0}; uint32_t shNd = 0; int shDepth = 0; bool shSelected = false;
    void* scratch[16] = {}; size_t capScratch[16] = {};      // infx_stream_scratch
    std::vector<void*> parked;                                // outgrown workspaces of a sharded stream (see grow)
    void *dHugeWs = nullptr, *dHugeCnt = nullptr; size_t capHugeWs = 0, capHugeCnt = 0;      // k_stage2's global-workspace pass
    ncclComm_t comm = nullptr;                                 // infx_stream_comm: this stream's own communicator (several batches in flight per rank)
    void *dLWordOff = nullptr, *dLChars = nullptr, *dLMembers = nullptr, *dLCount = nullptr; size_t capLWordOff = 0, capLChars = 0, capLMembers = 0, capLCount = 0;   // infx_ld1_expand
};

#define S2_HUGE_POOL_U16 (32u << 20)      // token-table pool of k_stage2's over-long-document pass: 64 MB per stream (a 700-word row takes 7.1 KB, a 32 768-token one 332 KB)
static int32_t grow(infx_stream* s, void** p, size_t* cap, size_t need);
static int32_t s2_huge_ready(infx_stream* s) {      // pool + bump counter of the over-long-document pass (allocated at the stream's first Stage-2 launch)
    int32_t rc = grow(s, &s->dHugeWs, &s->capHugeWs, (size_t)S2_HUGE_POOL_U16 * 2); if (rc) return rc;
    rc = grow(s, &s->dHugeCnt, &s->capHugeCnt, 16); if (rc) return rc;
    if (hipMemsetAsync(s->dHugeCnt, 0, 4, s->st) != hipSuccess) return fail(INFX_EHIP, "hipMemsetAsync failed%s");
    return INFX_OK;
}
// hipFree synchronises the whole device: it returns when EVERY stream has drained.  With several sessions in flight the others keep refilling the device, so a
// session that outgrows a workspace in the middle of a stream waited in hipFree until the run ended (measured, round 4: one batch of a 20-batch run 12 % larger
// than its session's earlier batches sat 290 ms in grow() — 310 ms instead of 250 ms for the run); and on a document shard another session's collective may be
// in flight at that moment, spinning until the peer rank's matching collective runs, while on the peer the roles are swapped: neither rank can enqueue what the
// other waits for.  Workspaces are therefore never freed while their stream lives: the outgrown buffer is parked on the stream (freed by infx_stream_destroy);
// growth is geometric, so the parked buffers add up to less than the live one.
static void ws_release(infx_stream* s, void* p);
static int32_t grow(infx_stream* s, void** p, size_t* cap, size_t need) {
    if (need <= *cap) return INFX_OK;
    if (*p) s->parked.push_back(*p);
    // a quarter of headroom: batches of one workload differ by a few per cent, and a reallocation (hipFree + hipMalloc synchronise the device) in a
    // stream's second batch would stall every other stream's batch in flight
    size_t n = std::max(need + need / 4 + 4096, *cap * 2);
    static const bool dbgGrow = getenv("INFX_DEBUG_GROW") != nullptr;
    const auto tg0 = std::chrono::steady_clock::now();
    if (hipMalloc(p, n) != hipSuccess) { *p = nullptr; *cap = 0; return fail(INFX_ENOMEM, "hipMalloc workspace failed%s"); }
    if (dbgGrow) fprintf(stderr, "[infx] grow: %zu -> %zu bytes (need %zu), hipMalloc took %.2f ms\n", *cap, n, need, std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - tg0).count());
    *cap = n; return INFX_OK;
}
static void ws_release(infx_stream* s, void* p) { if (p) s->parked.push_back(p); }
#define GROW(p, cap, need) do { int32_t rc_ = grow(s, (void**)&(p), &(cap), (need)); if (rc_) return rc_; } while (0)      /* `s`: the stream of the enclosing call */
// The index as a launch on stream s sees it: every kernel that takes DevIndex by value takes it from here.  qDeleted is the stream's per-query flags table
// while a batch with a pre-filtered query is being enqueued (infx_search_fused), else nullptr: the kernels then read the index's Deleted flags.
static inline DevIndex dev_index(const infx_stream* s) { DevIndex d = s->ix->d; d.qDeleted = s->qDelOn ? (const uint8_t* const*)s->dQDel : nullptr; return d; }

// Stage-2 launches: the register budget of the fast variant is selectable for tuning (INFX_S2_WAVES = 2, 4 or 6 waves per SIMD)
static int s2_waves() { static const int w = [] { const char* e = getenv("INFX_S2_WAVES"); int v = e ? atoi(e) : 0; return (v == 2 || v == 4 || v == 6 || v == 8) ? v : S2_MIN_WAVES; }(); return w; }
// LDS pool of the fast launch: UTF-16 units of document text per 64-candidate workgroup (INFX_S2_POOL overrides; 0 = texts stay in global memory)
static int s2_pool() { static const int w = [] { const char* e = getenv("INFX_S2_POOL"); int v = e ? atoi(e) : S2_POOL_CHARS; return (v < 0 || v > 32768) ? S2_POOL_CHARS : v; }(); return w; }
// INFX_S2_CUSTOM=1 (measurement, like the two above): a stream that is handed matcher settings (infx_stream_set_coverage; the engine does so for every batch) runs the
// custom-setup instantiations of k_stage2 also when the settings are CoverageSetup's defaults — what the settings cost as kernel arguments against compile-time
// constants, same results (profiles/coverage_setup.md)
static bool s2_force_custom() { static const bool f = [] { const char* e = getenv("INFX_S2_CUSTOM"); return e && e[0] == '1'; }(); return f; }
#define S2_GRID(lds) (ncand + S2_THREADS - 1) / S2_THREADS, S2_THREADS, (lds), s->st
#define S2_FAST_TAIL pool_, (uint16_t*)nullptr, (uint32_t*)nullptr, 0u, (const infx_cov_query_long*)nullptr, s->nLongQ      /* the first launch tells long-query rows apart (and checks their table index) */
// AL: the ALIAS instantiation (stage2.hip.inc: OrdinalIgnoreCase sites compare class representatives) — whenever the corpus or the batch's queries hold one of the 22 alias
// characters; else the plain one (every comparison `==`, exact without them)
#define S2_AL (s->ix->hasAlias || s->batchAlias)
// CS: the custom-setup instantiations (stage2.hip.inc), whenever the stream holds matcher settings that differ from CoverageSetup's defaults.  The fast launch — where
// the time goes — exists in the plain and the ALIAS form; the retry, huge-pool and long-query launches only in the ALIAS form (exact with or without alias characters)
#define S2_CS (s->csOn)
#define S2_NOHUGE (uint16_t*)nullptr, (uint32_t*)nullptr, 0u
#define S2_HUGEWS (uint16_t*)s->dHugeWs, (uint32_t*)s->dHugeCnt, (uint32_t)S2_HUGE_POOL_U16
#define S2_NOLONG (const infx_cov_query_long*)nullptr, 0u
#define S2_LONGT (const infx_cov_query_long*)s->dCovQL, s->nLongQ
#define S2_LAUNCH_FAST(...) do { const int pool_ = s2_pool(); if (S2_CS) { if (S2_AL) k_stage2<S2_FASTD, 6, false, false, true, true><<<S2_GRID(pool_ * 2)>>>(__VA_ARGS__, S2_FAST_TAIL, s->cs); \
                                              else k_stage2<S2_FASTD, 6, false, false, false, true><<<S2_GRID(pool_ * 2)>>>(__VA_ARGS__, S2_FAST_TAIL, s->cs); break; } \
                                 if (S2_AL) { k_stage2<S2_FASTD, 6, false, false, true><<<S2_GRID(pool_ * 2)>>>(__VA_ARGS__, S2_FAST_TAIL); break; } \
                                 switch (s2_waves()) { case 2: k_stage2<S2_FASTD, 2><<<S2_GRID(pool_ * 2)>>>(__VA_ARGS__, S2_FAST_TAIL); break; case 6: k_stage2<S2_FASTD, 6><<<S2_GRID(pool_ * 2)>>>(__VA_ARGS__, S2_FAST_TAIL); break; \
                                                     case 8: k_stage2<S2_FASTD, 8><<<S2_GRID(pool_ * 2)>>>(__VA_ARGS__, S2_FAST_TAIL); break; default: k_stage2<S2_FASTD, 4><<<S2_GRID(pool_ * 2)>>>(__VA_ARGS__, S2_FAST_TAIL); break; } } while (0)
#define S2_LAUNCH_SLOW(...) do { if (S2_CS) k_stage2<S2_MAXD, 4, false, false, true, true><<<S2_GRID(0)>>>(__VA_ARGS__, 0, S2_NOHUGE, S2_NOLONG, s->cs); else if (S2_AL) k_stage2<S2_MAXD, 4, false, false, true><<<S2_GRID(0)>>>(__VA_ARGS__, 0); else k_stage2<S2_MAXD, 4><<<S2_GRID(0)>>>(__VA_ARGS__, 0); } while (0)
#define S2_LAUNCH_HUGE(...) do { if (S2_CS) k_stage2<S2_HUGE_TOKENS, 1, true, false, true, true><<<S2_GRID(0)>>>(__VA_ARGS__, 0, S2_HUGEWS, S2_NOLONG, s->cs); else if (S2_AL) k_stage2<S2_HUGE_TOKENS, 1, true, false, true><<<S2_GRID(0)>>>(__VA_ARGS__, 0, (uint16_t*)s->dHugeWs, (uint32_t*)s->dHugeCnt, (uint32_t)S2_HUGE_POOL_U16); \
                                 else k_stage2<S2_HUGE_TOKENS, 1, true><<<S2_GRID(0)>>>(__VA_ARGS__, 0, (uint16_t*)s->dHugeWs, (uint32_t*)s->dHugeCnt, (uint32_t)S2_HUGE_POOL_U16); } while (0)
// rows of long queries (marked by the first launch): documents up to S2_MAXD words, then the rest through the global-workspace pass; nothing is launched for a batch without long queries.
// The table is consumed: the next Stage-2 call starts without one.
#define S2_LAUNCH_LONGQ(...) do { if (s->nLongQ) { \
    if (S2_CS) k_stage2<S2_MAXD, 2, false, true, true, true><<<S2_GRID(0)>>>(__VA_ARGS__, 0, S2_NOHUGE, S2_LONGT, s->cs); \
    else if (S2_AL) k_stage2<S2_MAXD, 2, false, true, true><<<S2_GRID(0)>>>(__VA_ARGS__, 0, (uint16_t*)nullptr, (uint32_t*)nullptr, 0u, (const infx_cov_query_long*)s->dCovQL, s->nLongQ); \
    else k_stage2<S2_MAXD, 2, false, true><<<S2_GRID(0)>>>(__VA_ARGS__, 0, (uint16_t*)nullptr, (uint32_t*)nullptr, 0u, (const infx_cov_query_long*)s->dCovQL, s->nLongQ); \
    (void)hipMemsetAsync(s->dHugeCnt, 0, 4, s->st);      /* the long-query rows get the whole token-table pool, not what the ordinary rows' pool pass left of it */ \
    if (S2_CS) k_stage2<S2_HUGE_TOKENS, 1, true, true, true, true><<<S2_GRID(0)>>>(__VA_ARGS__, 0, S2_HUGEWS, S2_LONGT, s->cs); \
    else if (S2_AL) k_stage2<S2_HUGE_TOKENS, 1, true, true, true><<<S2_GRID(0)>>>(__VA_ARGS__, 0, (uint16_t*)s->dHugeWs, (uint32_t*)s->dHugeCnt, (uint32_t)S2_HUGE_POOL_U16, (const infx_cov_query_long*)s->dCovQL, s->nLongQ); \
    else k_stage2<S2_HUGE_TOKENS, 1, true, true><<<S2_GRID(0)>>>(__VA_ARGS__, 0, (uint16_t*)s->dHugeWs, (uint32_t*)s->dHugeCnt, (uint32_t)S2_HUGE_POOL_U16, (const infx_cov_query_long*)s->dCovQL, s->nLongQ); \
    s->nLongQ = 0; s->longAlias = false; } s->csOn = false;      /* the matcher settings are consumed with the call's last launch */ } while (0)
static int32_t s2_huge_ready(infx_stream* s);

// ---- host <-> device transfers through pinned staging -------------------------------------------------------------------
// The C ABI takes plain (pageable) host pointers.  Handing those to hipMemcpyAsync makes the runtime pin/unpin the caller's pages
// per copy, which takes the process-wide address-space lock and stalls every host thread that page-faults meanwhile (observed:
// 50-70 ms stalls of unrelated planning threads with three sessions in flight).  Each stream therefore owns a pinned arena:
// inputs are copied into it and DMA'd from there; outputs are DMA'd into it and copied out after the stream synchronises.
static void* pin_take(infx_stream* s, size_t bytes) {
    bytes = (bytes + 255) & ~(size_t)255;
    for (auto& c : s->pins) if (c.cap - c.off >= bytes) { void* p = c.base + c.off; c.off += bytes; return p; }
    size_t cap = std::max<size_t>(bytes, s->pins.empty() ? (size_t)8 << 20 : s->pins.back().cap * 2);
    void* b = nullptr;
    if (hipHostMalloc(&b, cap, hipHostMallocDefault) != hipSuccess) return nullptr;
    s->pins.push_back({(char*)b, cap, bytes});
    return b;
}
static int comm_timeout_s() { static const int v = [] { const char* e = getenv("INFX_COMM_TIMEOUT_S"); const int x = e ? atoi(e) : 0; return x > 0 ? x : 120; }(); return v; }
static int32_t stream_sync(infx_stream* s) {
    // blocking wait (interrupt-driven) instead of hipStreamSynchronize's busy poll: a waiting host thread must not burn a core of a
    // CPU-quota-limited container while the planner pool of another session (or another rank's process) needs it
    HIPCHK(hipEventRecord(s->evSync, s->st));
    static const bool pollAlways = [] { const char* e = getenv("INFX_SYNC_POLL"); return e && e[0] == '1'; }();
    if (pollAlways || (s->ix->nranks > 1 && (s->comm || s->ix->comm))) {
        // A stream that carries RCCL collectives waits with a deadline: a peer that died or fell out of step leaves the collective kernel spinning for ever,
        // and an unbounded wait would turn that into a hung job.  INFX_COMM_TIMEOUT_S (default 120) -> INFX_ENCCL.
        const auto t0 = std::chrono::steady_clock::now(); const double limit = (double)comm_timeout_s();
        for (unsigned spin = 0;; spin++) {
            const hipError_t q = hipEventQuery(s->evSync);
            if (q == hipSuccess) break;
            if (q != hipErrorNotReady) return fail(INFX_EHIP, "hipEventQuery: %s", hipGetErrorString(q));
            if (std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() > limit) {
                s->pendingOut.clear();
                return fail(INFX_ENCCL, "a collective (or the kernels behind it) did not complete within INFX_COMM_TIMEOUT_S seconds: a peer rank is gone or out of step%s");
            }
            if (spin < 200) std::this_thread::yield(); else std::this_thread::sleep_for(std::chrono::microseconds(spin < 2000 ? 20 : 200));
        }
    } else
    HIPCHK(hipEventSynchronize(s->evSync));
    for (auto& d : s->pendingOut) std::memcpy(d.dst, d.src, d.bytes);
    s->pendingOut.clear(); s->unsynced = false;
    return INFX_OK;
}
static int32_t pin_reset(infx_stream* s) {     // start of an API call: the staging of the previous call must have been consumed
    // Outputs still pending here belong to a call that returned before its own synchronisation (an error path): their destinations
    // (often that call's stack variables) are gone, so they are dropped, never copied.
    s->pendingOut.clear();
    if (s->unsynced) { int32_t rc = stream_sync(s); if (rc) return rc; }
    for (auto& c : s->pins) c.off = 0;
    return INFX_OK;
}
static int32_t up(infx_stream* s, void* dst, const void* src, size_t bytes) {
    if (!bytes) return INFX_OK;
    void* p = pin_take(s, bytes); if (!p) return fail(INFX_ENOMEM, "hipHostMalloc staging failed%s");
    std::memcpy(p, src, bytes);
    HIPCHK(hipMemcpyAsync(dst, p, bytes, hipMemcpyHostToDevice, s->st)); s->unsynced = true;
    return INFX_OK;
}
static int32_t down(infx_stream* s, void* dstHost, const void* srcDev, size_t bytes) {   // lands in dstHost at the next stream_sync
    if (!bytes) return INFX_OK;
    void* p = pin_take(s, bytes); if (!p) return fail(INFX_ENOMEM, "hipHostMalloc staging failed%s");
    HIPCHK(hipMemcpyAsync(p, srcDev, bytes, hipMemcpyDeviceToHost, s->st)); s->unsynced = true;
    s->pendingOut.push_back({dstHost, p, bytes});
    return INFX_OK;
}
// Exchange buffers of the sharded stage API may live on the device (e.g. torch CUDA tensors handed to RCCL): those are copied
// device-to-device on the stream instead of being staged through the pinned arena.
static bool is_device_ptr(const void* p) {
    if (!p) return false;
    hipPointerAttribute_t a;
    if (hipPointerGetAttributes(&a, p) != hipSuccess) { (void)hipGetLastError(); return false; }     // plain pageable host memory
    return a.type == hipMemoryTypeDevice;
}
static int32_t upx(infx_stream* s, void* dst, const void* src, size_t bytes) {
    if (!bytes) return INFX_OK;
    if (!is_device_ptr(src)) return up(s, dst, src, bytes);
    HIPCHK(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, s->st)); s->unsynced = true;
    return INFX_OK;
}
static int32_t downx(infx_stream* s, void* dst, const void* srcDev, size_t bytes) {
    if (!bytes) return INFX_OK;
    if (!is_device_ptr(dst)) return down(s, dst, srcDev, bytes);
    HIPCHK(hipMemcpyAsync(dst, srcDev, bytes, hipMemcpyDeviceToDevice, s->st)); s->unsynced = true;
    return INFX_OK;
}
// Planning calls (infx_ld1_expand, infx_union_build) run on the stream's high-priority companion: every helper above works on s->st, which is swapped
// for the duration of the call; leave() makes the main stream wait for what the planning stream still has queued (the union write pass).
struct PlanStream {
    infx_stream* s; bool on;
    explicit PlanStream(infx_stream* x) : s(x), on(x->stPlan != nullptr) { if (on) s->st = s->stPlan; }
    int32_t leave() {
        if (!on) return INFX_OK;
        on = false; s->st = s->stMain;
        HIPCHK(hipEventRecord(s->evPlan, s->stPlan));
        HIPCHK(hipStreamWaitEvent(s->stMain, s->evPlan, 0));
        return INFX_OK;
    }
    ~PlanStream() { if (on) s->st = s->stMain; }
};
#define UPX(dst, src, n) do { int32_t rc_ = upx(s, (dst), (src), (n)); if (rc_) return rc_; } while (0)
#define DOWNX(dst, src, n) do { int32_t rc_ = downx(s, (dst), (src), (n)); if (rc_) return rc_; } while (0)
#define UP(dst, src, n) do { int32_t rc_ = up(s, (dst), (src), (n)); if (rc_) return rc_; } while (0)
#define DOWN(dst, src, n) do { int32_t rc_ = down(s, (dst), (src), (n)); if (rc_) return rc_; } while (0)
#define SYNC() do { int32_t rc_ = stream_sync(s); if (rc_) return rc_; } while (0)
// the table as one blob in *buf, grown to fit: one upload
static int32_t table_upload(infx_stream* s, const ProgTable& T, void** buf, size_t* cap) {
    const size_t total = T.blob_bytes();
    { int32_t rc_ = grow(s, buf, cap, total); if (rc_) return rc_; }
    std::vector<uint8_t> H(total, 0);
    T.put_blob(H.data(), (const char*)*buf);
    return up(s, *buf, H.data(), total);
}
// Columns are indexed by GLOBAL internal id: whatever reads them by document needs every uploaded column (col < 0), or column col, to hold documents [0, n)
#define COLS_COVER_CORPUS "a column holds fewer rows than the corpus has documents%s"
#define COLS_COVER_COUNTED "a column holds fewer rows than the counted documents%s"
static int32_t columns_cover(const infx_index* ix, int64_t n, const char* msg, int col = -1) {
    for (int c = std::max(col, 0); c < (col < 0 ? FILT_MAXCOL : col + 1); c++)
        if (ix->colCodes[c] && (uint64_t)ix->colDocs[c] < (uint64_t)std::max<int64_t>(n, 0)) return fail(INFX_EINVAL, msg);
    return INFX_OK;
}
static DevColumns dev_columns(const infx_index* ix) { DevColumns cols; for (int c = 0; c < FILT_MAXCOL; c++) cols.codes[c] = ix->colCodes[c]; return cols; }
// Raises kernel fn's dynamic-LDS limit for a launch of lds bytes on `device`, when that is more than the 64 KiB every kernel may have.  Sessions launch from
// several threads: the attribute is raised under a lock, and only past its high-water mark — one mark per (device, function), because a function's
// attributes belong to the device that is current when they are set.
static hipError_t lds_limit(const void* fn, int device, size_t lds) {
    if (lds <= 64 * 1024) return hipSuccess;
    static std::mutex mu; static std::map<std::pair<int, const void*>, size_t> mark;
    std::lock_guard<std::mutex> lk(mu);
    size_t& hw = mark[{device, fn}];
    if (lds > hw) { const hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds); if (e != hipSuccess) return e; hw = lds; }
    return hipSuccess;
}

template <int R> static void launch_union(infx_stream* s, uint32_t nv, const uint32_t* dBeg, const uint32_t* dEnd, const int32_t* dMembers, uint32_t* dRangeCount,
                                            const unsigned long long* dBase, int32_t* outDocs) {
    uint64_t blocks = (uint64_t)nv * s->ix->d.nRanges;
    k_union<R><<<dim3((unsigned)blocks), dim3(WAVE), 0, s->st>>>(dev_index(s), dBeg, dEnd, dMembers, nv, dRangeCount, dBase, outDocs);
}
static void launch_union_any(infx_stream* s, uint32_t nv, const uint32_t* dBeg, const uint32_t* dEnd, const int32_t* dMembers, uint32_t* dRangeCount,
                             const unsigned long long* dBase, int32_t* outDocs) {
    switch (s->ix->d.R) {
        case 512: launch_union<512>(s, nv, dBeg, dEnd, dMembers, dRangeCount, dBase, outDocs); break;
        case 1024: launch_union<1024>(s, nv, dBeg, dEnd, dMembers, dRangeCount, dBase, outDocs); break;
        case 2048: launch_union<2048>(s, nv, dBeg, dEnd, dMembers, dRangeCount, dBase, outDocs); break;
        case 4096: launch_union<4096>(s, nv, dBeg, dEnd, dMembers, dRangeCount, dBase, outDocs); break;
        case 8192: launch_union<8192>(s, nv, dBeg, dEnd, dMembers, dRangeCount, dBase, outDocs); break;
        default: launch_union<16384>(s, nv, dBeg, dEnd, dMembers, dRangeCount, dBase, outDocs); break;
    }
}
// exact replay of the reference's Stage-1 order effects (k_exact1) — on unless INFX_EXACT=0
static bool exact_enabled(const infx_index* ix) { static const bool v = [] { const char* e = getenv("INFX_EXACT"); return !(e && e[0] == '0'); }(); return v && !(ix->cfg.flags & INFX_CFG_NO_EXACT_REPLAY); }
static Arena make_arena(infx_stream* s) {
    return Arena{s->arDoc, s->arScore, s->arCls, s->arMask, s->arExc, (const unsigned long long*)s->dBlockOut, (uint32_t*)s->dBlockOutHi,
                 (uint32_t*)s->dCounts, s->dOverflow, (unsigned long long*)s->dQBytes, (uint32_t*)((unsigned long long*)s->dQBytes + s->lastNqAlloc), (uint2*)s->dDir, s->maskWords};
}
static int acc_stripe() { static const int v = [] { const char* e = getenv("INFX_ACC_STRIPE"); int x = e ? atoi(e) : 0; return (x >= 1 && x <= 64) ? x : 4; }(); return v; }
// LDS8 (stage1.hip.inc) addresses the tf array by raw LDS offset: true only while k_accumulate owns no static __shared__ data, i.e. its dynamic
// LDS starts at address 0.  Checked once per instantiation against the code object; a violation fails the search loudly.
template <int R> static bool acc_lds_layout_ok() {
    static const bool ok = [] {
        hipFuncAttributes a1{}, a2{}, a4{};
        if (hipFuncGetAttributes(&a1, (const void*)k_accumulate<R, 1>) != hipSuccess || hipFuncGetAttributes(&a2, (const void*)k_accumulate<R, 2>) != hipSuccess ||
            hipFuncGetAttributes(&a4, (const void*)k_accumulate<R, 4>) != hipSuccess) return false;
        return a1.sharedSizeBytes == 0 && a2.sharedSizeBytes == 0 && a4.sharedSizeBytes == 0;
    }();
    return ok;
}
// Two kernels share the (query, stripe) pairs of a batch by candidate density (INFX_ACC_SPARSE_T candidates per stripe, default 96 — measured 64: 6.27, 96: 6.18, 128: 6.20, 192: 6.31, 256: 6.41, 512: 6.85 ms for the pair; 0: one kernel, 7.21 ms):
//   k_accumulate_sparse (stage1_sparse.hip.inc)  stripes of <= T candidates: the candidates look their postings up (binary search of the stripe slice, one per lane)
//   k_accumulate        (stage1.hip.inc)         the rest: byte scatter + probe per (list, range) — cheapest per candidate once a range holds dozens of them
static int acc_sparse_t() { static const int v = [] { const char* e = getenv("INFX_ACC_SPARSE_T"); const int x = e ? atoi(e) : 96; return std::max(0, std::min(4096, x)); }(); return v; }
template <int R> static void launch_acc(infx_stream* s, uint32_t nq, Arena ar, int maxT, int useGrp, int maxRef) {
    (void)maxRef;
    if (!acc_lds_layout_ok<R>()) { s->accLayoutBad = true; return; }
    static const int dbgSkip = [] { const char* e = getenv("INFX_ACC_SKIP"); return e ? atoi(e) : 0; }();     // kernel ablation for profiling only
    const int sparseT = s->ix->hPostOff.empty() || s->ix->hPostOff.back() + 4 <= 0xFFFFFFF0ull ? acc_sparse_t() : 0;      // (k_accumulate_sparse indexes a shard's postings with 32 bits)
    const int stripe = sparseT > 0 ? std::max(1, std::min(4, 65536 / R)) : acc_stripe();      // (the two kernels split the same stripes: a power of two)
    const int nStripes = (s->ix->d.nRanges + stripe - 1) / stripe;
    const uint64_t blocks = (uint64_t)nq * 8u * ((nStripes + 7) / 8);     // stripes rounded up to whole groups of 8 (one per XCD)
    const uint8_t* dense = nullptr;
    if (sparseT > 0) {
        if (grow(s, &s->dDense, &s->capDense, (size_t)nq * nStripes)) { s->accLayoutBad = true; return; }
        hipMemsetAsync(s->dDense, 0, (size_t)nq * nStripes, s->st);
        const size_t sw = (size_t)stripe * (R / 32);
        const int maxTl = (std::min(64, std::max(1, maxT)) + 3) & ~3;
        static const int dbgS = [] { const char* e = getenv("INFX_ACCS_SKIP"); return e ? atoi(e) : 0; }();      // kernel ablation for profiling only
        const size_t ldsS = (sw + 64 + 4) * 4 + INFX_NCLASS * 4 + WAVE * 2 + WAVE * 12 + (size_t)WAVE * maxTl + (size_t)64 * maxTl;      // padded bitmap (one pad word per lane) | class histogram | slot table | slice table | hit matrix | slice samples
#define ACCS_LAUNCH(MW_) k_accumulate_sparse<R, MW_><<<dim3((unsigned)blocks), dim3(WAVE), ldsS, s->st>>>(dev_index(s), (const DevQuery*)s->dQueries, (const DevTerm*)s->dTerms, (const int32_t*)s->dExtra, \
            (const int32_t*)s->dUDocs, (const uint32_t*)s->dURange, nq, ar, stripe, useGrp, (uint8_t*)s->dDense, (uint32_t)sparseT, nStripes, maxTl, dbgS)
        if (ar.maskWords == 4) ACCS_LAUNCH(4); else if (ar.maskWords == 2) ACCS_LAUNCH(2); else ACCS_LAUNCH(1);
#undef ACCS_LAUNCH
        dense = (const uint8_t*)s->dDense;
    }
    const size_t lds = (size_t)R + 128 + ((size_t)(R / 32) + 2) * 4 + INFX_NCLASS * 4 + ACC_CAP_DEFAULT * 2;
#define ACC_LAUNCH(MW_) k_accumulate<R, MW_><<<dim3((unsigned)blocks), dim3(WAVE), lds, s->st>>>(dev_index(s), (const DevQuery*)s->dQueries, (const DevTerm*)s->dTerms, (const int32_t*)s->dExtra, \
        (const int32_t*)s->dUDocs, (const uint32_t*)s->dURange, nq, ar, maxT, stripe, useGrp, dbgSkip, (unsigned long long*)s->dStats, dense, nStripes, \
        s->nAccHeavy != 0xFFFFFFFFu ? (const uint32_t*)s->dAccOrder : nullptr, s->nAccHeavy != 0xFFFFFFFFu ? s->nAccHeavy : 0u)
    if (ar.maskWords == 4) ACC_LAUNCH(4); else if (ar.maskWords == 2) ACC_LAUNCH(2); else ACC_LAUNCH(1);
#undef ACC_LAUNCH
    if (dbgSkip & 8) { unsigned long long h[4] = {0, 0, 0, 0}; hipStreamSynchronize(s->st); hipMemcpy(h, s->dStats, 32, hipMemcpyDeviceToHost); hipMemset(s->dStats, 0, 32);
        fprintf(stderr, "[infx] k_accumulate stats: %llu ranges with candidates (%llu blocks), %.2f rounds/range, %.1f candidates/range\n", h[0], (unsigned long long)blocks, h[0] ? (double)h[1] / h[0] : 0.0, h[0] ? (double)h[2] / h[0] : 0.0); }
}

// Longest-queries-first order for k_select's workgroups (k_select_order, stage1.hip.inc); nullptr: query order (batches beyond SEL_ORDER_MAX, INFX_SELECT_LPT=0)
static const uint32_t* select_order(infx_stream* s, uint32_t nq) {
    static const bool off = [] { const char* e = getenv("INFX_SELECT_LPT"); return e && e[0] == '0'; }();
    if (off || nq < 64 || nq > SEL_ORDER_MAX) return nullptr;
    if (grow(s, &s->dSelOrder, &s->capSelOrder, (size_t)nq * 4)) return nullptr;
    k_select_order<<<1, 1024, 0, s->st>>>((const uint32_t*)s->dBlockOutHi, nq, (uint32_t*)s->dSelOrder);
    return (const uint32_t*)s->dSelOrder;
}
#ifdef SEL_PROF
// profiling build only: per-workgroup wall_clock64() stamps (8 words per workgroup: t0 .. t5, two free words) -> span of the launch, the longest workgroups, percentiles
static void wgprof_dump(const char* name, const unsigned long long* dProf, uint32_t n, const char* const ph[5], hipStream_t st) {
    hipStreamSynchronize(st);
    std::vector<unsigned long long> h((size_t)n * 8); hipMemcpy(h.data(), dProf, h.size() * 8, hipMemcpyDeviceToHost);
    unsigned long long t0 = ~0ull, t5 = 0; for (uint32_t q = 0; q < n; q++) if (h[q * 8]) { t0 = std::min(t0, h[q * 8]); for (int k = 1; k < 6; k++) t5 = std::max(t5, h[q * 8 + k]); }
    fprintf(stderr, "[%s] span %.1f us\n", name, (t5 - t0) / 100.0);
    auto endOf = [&](uint32_t q) { unsigned long long e = h[q * 8]; for (int k = 1; k < 6; k++) e = std::max(e, h[q * 8 + k]); return e; };
    std::vector<uint32_t> ord(n); for (uint32_t q = 0; q < n; q++) ord[q] = q;
    std::sort(ord.begin(), ord.end(), [&](uint32_t a, uint32_t b) { return endOf(a) - h[a * 8] > endOf(b) - h[b * 8]; });
    auto us = [&](uint32_t q, int a, int b) { const unsigned long long x = h[q * 8 + a], y = h[q * 8 + b]; return (x && y) ? (double)(y - x) / 100.0 : -1.0; };
    auto line = [&](const char* tag, uint32_t q) { fprintf(stderr, "[%s] %s wg %u w6 %llu w7 %llu: start %.1f total %.1f | %s %.1f %s %.1f %s %.1f %s %.1f %s %.1f\n", name, tag, q, h[q * 8 + 6], h[q * 8 + 7], (h[q * 8] - t0) / 100.0,
                                                        (endOf(q) - h[q * 8]) / 100.0, ph[0], us(q, 0, 1), ph[1], us(q, 1, 2), ph[2], us(q, 2, 3), ph[3], us(q, 3, 4), ph[4], us(q, 4, 5)); };
    for (int i = 0; i < 10 && i < (int)n; i++) line("top", ord[i]);
    line("p50", ord[n / 2]); line("p90", ord[n / 10]); line("p99", ord[n / 100]);
    std::vector<unsigned long long> en(n); for (uint32_t q = 0; q < n; q++) en[q] = endOf(q) - t0; std::sort(en.begin(), en.end());
    fprintf(stderr, "[%s] ends: p10 %.1f p50 %.1f p90 %.1f p99 %.1f max %.1f us\n", name, en[n / 10] / 100.0, en[n / 2] / 100.0, en[n * 9 / 10] / 100.0, en[n * 99 / 100] / 100.0, en[n - 1] / 100.0);
}
#endif
// The largest queries of the batch swept by many workgroups in front of k_select (k_selg_hist / k_selg_gather, stage1.hip.inc).  INFX_SEL_GIANT_MIN: rows from which a
// query is one (default 65536; 0: off — k_select sweeps every query itself).  Needs the longest-first order (its first SELG_MAX entries are the candidates).
static uint32_t giant_min_rows() { static const uint32_t v = [] { const char* e = getenv("INFX_SEL_GIANT_MIN"); return e ? (uint32_t)std::max(0, atoi(e)) : 65536u; }(); return v; }
static SelGiant select_giants(infx_stream* s, Arena ar, uint32_t nq, const uint32_t* order) {
    const uint32_t minRows = giant_min_rows();
    SelGiant G{}; if (!order || !minRows || !s->nBoundGiants || s->maxQueryBound < 4ull * minRows) return G;      // (three launches + two memsets cost ~50 us: not for a batch whose largest query k_select sweeps in that time)
    const size_t head = (size_t)SELG_MAX * 2 * 4096 * 4 + (size_t)SELG_MAX * 4 * 5, total = head + (size_t)SELG_MAX * SEL_CAP * 8;
    if (grow(s, &s->dSelG, &s->capSelG, total)) return G;
    const uint32_t nSlots = std::min<uint32_t>(SELG_MAX, std::min(nq, s->nBoundGiants));
    hipMemsetAsync(s->dSelG, 0, (size_t)nSlots * 2 * 4096 * 4, s->st);                                             // the histograms of the slots in use
    hipMemsetAsync((char*)s->dSelG + (size_t)SELG_MAX * 2 * 4096 * 4, 0, (size_t)SELG_MAX * 4 * 5, s->st);       // count | left | mode | cut | shift
    G.hist = (uint32_t*)s->dSelG; G.count = G.hist + (size_t)SELG_MAX * 2 * 4096; G.left = G.count + SELG_MAX; G.mode = G.left + SELG_MAX; G.cut = G.mode + SELG_MAX; G.shift = G.cut + SELG_MAX;
    G.keys = (unsigned long long*)((char*)s->dSelG + head); G.minRows = minRows;
    // (a query holds at most its row bound: the slots and partitions that can be needed are known on the host — a batch of small queries launches a handful of workgroups)
    const dim3 grid((unsigned)std::min<uint64_t>(SELG_PARTS, (s->maxQueryBound + SELG_PART_MIN - 1) / SELG_PART_MIN), nSlots);
    k_selg_hist<<<grid, SEL_THREADS, 0, s->st>>>(ar, (const SelRule*)s->dRules, order, nq, G);
    k_selg_cut<<<grid.y, 256, 0, s->st>>>(ar, (const SelRule*)s->dRules, order, nq, G);
    k_selg_gather<<<grid, SEL_THREADS, 0, s->st>>>(ar, (const SelRule*)s->dRules, order, nq, G);
    return G;
}
// k_exact1 behind k_select: unsharded indexes only (the reference's chunking follows GLOBAL 65 536-id containers and its heap is sequential
// over the whole corpus; document shards keep k_select's deterministic (score, doc id) cut)
static bool exact_slow_only() { static const bool v = [] { const char* e = getenv("INFX_EXACT_SLOW"); return e && e[0] == '1'; }(); return v; }
// the full heap of the replay lives in registers (RHeap, exact3.hip.inc) when its entries fit the packing: internal ids below 2^30, depth <= 512;
// INFX_EX_HEAP_LDS=1 keeps the LDS heap (A/B measurements, parity tooling)
static int ex_heap_in_regs(const infx_index* ix, int depth) {
    static const bool off = [] { const char* e = getenv("INFX_EX_HEAP_LDS"); return e && e[0] == '1'; }();
    const long long total = std::max<long long>(ix->d.totalDocs, (long long)ix->d.docBase + ix->d.N);
    return (!off && depth <= EXS_MAXDEPTH && total < (1ll << 30)) ? 1 : 0;
}
// After the batch's k_select (with replay flags): a flagged query beyond two mask words (65 .. 128 reference terms) goes to the sequential replay (k_exact1 reads
// its four-word masks from the arena; the parallel replay's kernels keep two words in registers) — flag 1 -> 2, what k_ex_theta / k_ex_heap write for a query they hand over.
__global__ void k_mark_wide(uint32_t* __restrict__ flags, const uint32_t* __restrict__ list, uint32_t n) { for (uint32_t i = threadIdx.x; i < n; i += blockDim.x) if (flags[list[i]] == 1u) flags[list[i]] = 2u; }
static int32_t mark_wide_queries(infx_stream* s, int depth) {
    if (!s->nWide || exact_slow_only() || depth > EXS_MAXDEPTH) return INFX_OK;      // (no parallel replay: k_exact1 takes every flagged query as it is)
    k_mark_wide<<<1, 64, 0, s->st>>>((uint32_t*)s->dExactFlag, (const uint32_t*)s->dWideQ, s->nWide);
    HIPCHK(hipGetLastError());
    return INFX_OK;
}
static bool exact_possible(infx_stream* s) { return exact_enabled(s->ix) && s->maskWords > 0 && s->ix->nranks == 1 && s->ix->d.docBase == 0; }
// chunk table of the parallel replay: every query needs at most (containers + reserved rows / 4096 + 2) entries
static int32_t exact_chunk_tables(infx_stream* s, uint32_t nq, ExBufs& xb) {
    infx_index* ix = s->ix;
    const int rpc = 65536 / ix->d.R, nCont = (ix->d.nRanges + rpc - 1) / rpc;
    const size_t cap = (size_t)nq * (nCont + 2) + s->arBound / EX_CHUNK + 16;
    if (cap > 0x7FFFFFF0ull) return fail(INFX_ECAPACITY, "exact-replay chunk table too large; split the batch%s");
    GROW(s->exChunks, s->capExChunks, cap * sizeof(ExChunk));
    GROW(s->exTasks, s->capExTasks, cap * 3 * 4);
    GROW(s->exQueries, s->capExQueries, (size_t)nq * sizeof(ExQuery));
    GROW(s->exContEnd, s->capExContEnd, (size_t)nq * nCont * 4);
    s->exChunkCap = (uint32_t)cap;
    HIPCHK(hipMemsetAsync(s->exCounters, 0, 32, s->st));
    xb = ExBufs{s->exCand, s->exOut, s->arExc, (ExChunk*)s->exChunks, s->exChunkCap, (ExQuery*)s->exQueries, s->exCounters, (uint32_t*)s->exTasks, (uint32_t*)s->exTasks + cap,
                (uint32_t*)s->exTasks + 2 * cap, (uint32_t*)s->exContEnd, nullptr, nullptr};
    return INFX_OK;
}
// The scan and the chunk pass of the parallel replay on stream `st` (k_ex_cand, k_ex_theta, k_ex_chunk<16|4|1>, widest tasks first).  With an auxiliary stream
// (INFX_REPLAY_AUX=1) the two workgroup variants of k_ex_chunk run beside the one-wave variant (disjoint chunks; each launch ends in a tail of a few long tasks).
static int32_t launch_scan_and_chunks(infx_stream* s, uint32_t nq, Arena ar, ExBufs xb, const float* prior, bool useAux) {
    infx_index* ix = s->ix;
    const int rpc = 65536 / ix->d.R, nCont = (ix->d.nRanges + rpc - 1) / rpc;
    if (nCont > 65535) return fail(INFX_ECAPACITY, "exact replay: more than 65535 containers of 65536 documents in one shard%s");
    k_ex_walk<false><<<dim3(nq, nCont), WAVE, 0, s->st>>>(dev_index(s), ar, (const SelRule*)s->dRules, (const uint32_t*)s->dExactFlag, xb, nCont);
    k_ex_prefix<<<nq, EXS_THREADS, 0, s->st>>>((const uint32_t*)s->dExactFlag, xb, nCont);
    k_ex_walk<true><<<dim3(nq, nCont), WAVE, 0, s->st>>>(dev_index(s), ar, (const SelRule*)s->dRules, (const uint32_t*)s->dExactFlag, xb, nCont);
    k_ex_theta<<<nq, WAVE, 0, s->st>>>(ar, (const SelRule*)s->dRules, (uint32_t*)s->dExactFlag, xb, prior, nCont);
    HIPCHK(hipEventRecord(s->evXa, s->st));
    hipStream_t bigSt = s->st;
    if (useAux && s->stAux && s->st == s->stMain) { HIPCHK(hipStreamWaitEvent(s->stAux, s->evXa, 0)); bigSt = s->stAux; }
    k_ex_chunk<16><<<EXP_GRID16, 16 * WAVE, 0, bigSt>>>(dev_index(s), (const DevQuery*)s->dQueries, (const DevRefTerm*)s->dRefTerms, ar, xb, xb.tasksBig, 4, ix->avgdl);
    k_ex_chunk<4><<<EXP_GRID4, 4 * WAVE, 0, bigSt>>>(dev_index(s), (const DevQuery*)s->dQueries, (const DevRefTerm*)s->dRefTerms, ar, xb, xb.tasksMid, 2, ix->avgdl);
    if (bigSt != s->st) HIPCHK(hipEventRecord(s->evJoin, bigSt));
    k_ex_chunk<1><<<EXP_GRID1, WAVE, 0, s->st>>>(dev_index(s), (const DevQuery*)s->dQueries, (const DevRefTerm*)s->dRefTerms, ar, xb, xb.tasksSmall, 1, ix->avgdl);
    if (bigSt != s->st) HIPCHK(hipStreamWaitEvent(s->st, s->evJoin, 0));
    HIPCHK(hipGetLastError());
    return INFX_OK;
}
static int32_t exact1_lds_ready(infx_index* ix, int MW, size_t* ldsOut) {
    const int depthCap = ix->cfg.max_depth;
    const size_t lds1 = (size_t)(EX_CHUNK + EX_THREADS) * (MW <= 2 ? MW : 1) * 8 + (size_t)(EX_CHUNK + EX_THREADS) * 4 + (size_t)EX_CHUNK * 4 + (size_t)depthCap * 8 +
                        (INFX_MAX_QUERY_TERMS + 1) * 4 + 130 * 4 + 129 * 4 + 8 * 4 + (size_t)EX_CHUNK * 2 + 64;
    static std::mutex mu; static size_t attr1 = 0;
    { std::lock_guard<std::mutex> lk(mu);
      if (lds1 > attr1) { HIPCHK(hipFuncSetAttribute((const void*)k_exact1, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds1)); attr1 = lds1; } }
    *ldsOut = lds1; return INFX_OK;
}
static int32_t enqueue_exact(infx_stream* s, uint32_t nq, int stride) {
    infx_index* ix = s->ix;
    const int MW = s->maskWords, depthCap = ix->cfg.max_depth;
    static const bool slowOnly = exact_slow_only();      // parity tooling: k_exact1 for every flagged query
    size_t lds1 = 0; { int32_t rc_ = exact1_lds_ready(ix, MW, &lds1); if (rc_) return rc_; }
    Arena ar = make_arena(s);
    HIPCHK(hipMemsetAsync(s->dExactStat, 0, 16, s->st));
    HIPCHK(hipEventRecord(s->evX0, s->st));
    const bool fast = !slowOnly && depthCap <= EXS_MAXDEPTH;
    if (fast) {
        ExBufs xb; { int32_t rc_ = exact_chunk_tables(s, nq, xb); if (rc_) return rc_; }
        static const bool exProf = getenv("INFX_EXACT_PROF") != nullptr;     // per-query cycle counters of the replay kernels (profiling only)
        if (exProf) { GROW(s->dExProf, s->capExProf, ((size_t)nq * EXP_WORDS + (EXP_GRID1 + EXP_GRID4 + EXP_GRID16) * 4) * 8); HIPCHK(hipMemsetAsync(s->dExProf, 0, ((size_t)nq * EXP_WORDS + (EXP_GRID1 + EXP_GRID4 + EXP_GRID16) * 4) * 8, s->st)); }
        xb.prof = exProf ? (unsigned long long*)s->dExProf : nullptr; xb.profChunk = exProf ? (unsigned long long*)s->dExProf + (size_t)nq * EXP_WORDS : nullptr;
        { int32_t rc_ = launch_scan_and_chunks(s, nq, ar, xb, nullptr, true); if (rc_) return rc_; }
        HIPCHK(hipEventRecord(s->evXb, s->st));
        k_ex_heap<<<nq, WAVE, 0, s->st>>>(ar, (const SelRule*)s->dRules, (uint32_t*)s->dExactFlag, xb, (infx_hit*)s->dHits, (uint32_t*)s->dHitCount, stride, s->dExactStat,
                                          exProf ? (unsigned long long*)s->dExProf : nullptr, ex_heap_in_regs(ix, depthCap));
        HIPCHK(hipGetLastError());
        HIPCHK(hipEventRecord(s->evXc, s->st)); s->timedReplayParts = true;
        if (exProf) {       // profiling only: per-query counters of the replay kernels -> mean / p50 / p90 / max and the slowest queries
            hipStreamSynchronize(s->st);
            std::vector<unsigned long long> h((size_t)nq * EXP_WORDS); hipMemcpy(h.data(), s->dExProf, h.size() * 8, hipMemcpyDeviceToHost);
            uint32_t cnt[8] = {0, 0, 0, 0, 0, 0, 0, 0}; hipMemcpy(cnt, s->exCounters, 32, hipMemcpyDeviceToHost);
            static const char* names[EXP_WORDS] = {"heap.cycles", "heap.heap_cycles", "heap.rows", "heap.ops", "heap.chunks", "scan.cycles", "theta.insert_cycles", "theta.inserts", "cand.batches", "cand.rows", "cand.cands",
                                                   "theta.cycles", "-", "-", "-", "-"};
            std::vector<uint32_t> qs; for (uint32_t q = 0; q < nq; q++) if (h[(size_t)q * EXP_WORDS + 0] || h[(size_t)q * EXP_WORDS + 5]) qs.push_back(q);
            fprintf(stderr, "[infx] exact replay profile: %zu replayed queries of %u; chunk tasks 1-wave %u 4-wave %u 16-wave %u (chunk slots reserved %u)\n", qs.size(), nq, cnt[1], cnt[2], cnt[4], cnt[0]);
            if (!qs.empty()) for (int w = 0; w < 12; w++) {
                std::vector<unsigned long long> v; for (uint32_t q : qs) v.push_back(h[(size_t)q * EXP_WORDS + w]);
                std::sort(v.begin(), v.end()); double sum = 0; for (auto x : v) sum += (double)x;
                fprintf(stderr, "[infx]   %-20s mean %12.0f  p50 %12llu  p90 %12llu  p99 %12llu  max %12llu\n", names[w], sum / v.size(), v[v.size() / 2], v[v.size() * 9 / 10], v[v.size() * 99 / 100], v.back());
            }
            for (int which : {0, 5}) {
                std::sort(qs.begin(), qs.end(), [&](uint32_t a, uint32_t b) { return h[(size_t)a * EXP_WORDS + which] > h[(size_t)b * EXP_WORDS + which]; });
                for (size_t i = 0; i < std::min<size_t>(3, qs.size()); i++) { fprintf(stderr, "[infx]   slowest by %s: q %u:", names[which], qs[i]); for (int w = 0; w < 13; w++) fprintf(stderr, " %llu", h[(size_t)qs[i] * EXP_WORDS + w]); fprintf(stderr, "\n"); }
            }
            std::vector<unsigned long long> ck((EXP_GRID1 + EXP_GRID4 + EXP_GRID16) * 4); hipMemcpy(ck.data(), (char*)s->dExProf + (size_t)nq * EXP_WORDS * 8, ck.size() * 8, hipMemcpyDeviceToHost);
            const int g0[4] = {0, EXP_GRID1, EXP_GRID1 + EXP_GRID4, EXP_GRID1 + EXP_GRID4 + EXP_GRID16};
            for (int w = 0; w < 3; w++) {
                unsigned long long n = 0, cy = 0, mx = 0, tl = 0, wgMax = 0;
                for (int b = g0[w]; b < g0[w + 1]; b++) { n += ck[b * 4]; cy += ck[b * 4 + 1]; mx = std::max(mx, ck[b * 4 + 2]); tl += ck[b * 4 + 3]; wgMax = std::max(wgMax, ck[b * 4 + 1]); }
                fprintf(stderr, "[infx]   k_ex_chunk<%d>: %llu tasks, cycles per task mean %.0f max %llu, busiest workgroup %llu cycles, tiles mean %.1f\n", w == 0 ? 1 : (w == 1 ? 4 : 16), n, n ? (double)cy / n : 0.0, mx, wgMax, n ? (double)tl / n : 0.0);
            }
        }
    }
    k_exact1<<<nq, EX_THREADS, lds1, s->st>>>(dev_index(s), (const DevQuery*)s->dQueries, (const DevRefTerm*)s->dRefTerms, ar, (const SelRule*)s->dRules, (const uint32_t*)s->dExactFlag,
                                             fast ? 2u : 1u, ix->avgdl, (infx_hit*)s->dHits, (uint32_t*)s->dHitCount, stride, depthCap, s->dExactStat, nullptr, nullptr);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(s->evX1, s->st)); s->timedReplay = true;
    DOWN(s->lastExact2, s->dExactStat, 8);          // [0] replayed queries, [1] of them through the sequential k_exact1 fallback; lands at the caller's synchronisation
    DOWN(s->lastFlagWhy, s->dExactStat + 4, 16);
    return INFX_OK;
}

// An all-gather of one packed block per rank ([part 0 | part 1 | ...], `stride` bytes apart) unpacked into per-part arrays of nranks consecutive pieces:
// three exchanges of a batch (first-pass lists, their counts, the best scores left out) travel as ONE collective.
struct UnpackArgs { const uint32_t* src; uint64_t strideW; int32_t nranks, nparts; uint64_t offW[4], lenW[4]; uint32_t* dst[4]; };
__global__ void k_unpack(UnpackArgs a) {
    uint64_t per = 0; for (int p = 0; p < a.nparts; p++) per += a.lenW[p];
    const uint64_t total = per * (uint64_t)a.nranks;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t r = i / per; uint64_t w = i % per; int p = 0;
        while (w >= a.lenW[p]) { w -= a.lenW[p]; p++; }
        a.dst[p][r * a.lenW[p] + w] = a.src[r * a.strideW + a.offW[p] + w];
    }
}
// ---- RCCL (dlopen) ---------------------------------------------------------------------------------------------------------------------------
struct RcclApi {
    bool ok = false; const char* why = "";
    ncclResult_t (*getId)(ncclUniqueId*) = nullptr;
    ncclResult_t (*init)(ncclComm_t*, int, ncclUniqueId, int) = nullptr;
    ncclResult_t (*allreduce)(const void*, void*, size_t, ncclDataType_t, ncclRedOp_t, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*allgather)(const void*, void*, size_t, ncclDataType_t, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*destroy)(ncclComm_t) = nullptr;
    const char* (*errstr)(ncclResult_t) = nullptr;
};
static RcclApi& rccl_api() {
    static RcclApi a = [] {
        RcclApi r;
        // a process that already holds an RCCL (e.g. torch's) keeps using that copy
        void* h = dlopen("librccl.so", RTLD_NOW | RTLD_NOLOAD);
        if (!h) h = dlopen("librccl.so.1", RTLD_NOW | RTLD_NOLOAD);
        if (!h) h = dlopen("librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
        if (!h) h = dlopen("librccl.so", RTLD_NOW | RTLD_GLOBAL);
        if (!h) { r.why = "librccl.so not found"; return r; }
        r.getId = (decltype(r.getId))dlsym(h, "ncclGetUniqueId"); r.init = (decltype(r.init))dlsym(h, "ncclCommInitRank");
        r.allreduce = (decltype(r.allreduce))dlsym(h, "ncclAllReduce"); r.allgather = (decltype(r.allgather))dlsym(h, "ncclAllGather");
        r.destroy = (decltype(r.destroy))dlsym(h, "ncclCommDestroy"); r.errstr = (decltype(r.errstr))dlsym(h, "ncclGetErrorString");
        r.ok = r.getId && r.init && r.allreduce && r.allgather && r.destroy && r.errstr;
        if (!r.ok) r.why = "librccl.so lacks an expected symbol";
        return r;
    }();
    return a;
}
#define NCCLCHK(x) do { ncclResult_t r_ = (x); if (r_ != ncclSuccess) return fail(INFX_ENCCL, #x ": %s", rccl_api().errstr(r_)); } while (0)

static int32_t main_pool(int device, MainPool** out) {
    static std::mutex mu; static std::map<int, MainPool*> pools;
    std::lock_guard<std::mutex> lk(mu);
    auto it = pools.find(device);
    if (it == pools.end()) {
        static const int nMain = [] { const char* e = getenv("INFX_MAIN_STREAMS"); const int n = e ? atoi(e) : 4; return n < 1 ? 1 : n > 32 ? 32 : n; }();
        MainPool* mp = new MainPool();
        for (int i = 0; i < nMain; i++) {
            hipStream_t st = nullptr; const hipError_t e = hipStreamCreateWithFlags(&st, hipStreamNonBlocking);
            if (e != hipSuccess) { for (hipStream_t p : mp->st) hipStreamDestroy(p); delete mp; return fail(INFX_EHIP, "hipStreamCreateWithFlags: %s", hipGetErrorString(e)); }
            mp->st.push_back(st); mp->users.push_back(0);
        }
        it = pools.emplace(device, mp).first;
    }
    *out = it->second; return INFX_OK;
}

extern "C" {

const char* infx_last_error(void) { return g_err.c_str(); }

int32_t infx_create(const infx_config* cfg, infx_index** out) {
    if (!cfg || !out) return fail(INFX_EINVAL, "null argument%s");
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev == 0) return fail(INFX_EHIP, "no HIP device available (%s) — the GPU path is mandatory, there is no CPU fallback", hipGetErrorString(e));
    if (cfg->device < 0 || cfg->device >= ndev) return fail(INFX_EINVAL, "bad device ordinal%s");
    HIPCHK(enter_device(cfg->device));
    infx_index* ix = new infx_index();
    ix->cfg = *cfg;
    int R = cfg->range_docs ? cfg->range_docs : 1024;
    if (R != 512 && R != 1024 && R != 2048 && R != 4096 && R != 8192 && R != 16384) { delete ix; return fail(INFX_EINVAL, "range_docs must be a power of two in [512, 16384]%s"); }
    ix->d.R = R; ix->d.rshift = __builtin_ctz(R);
    if (ix->cfg.max_depth <= 0) ix->cfg.max_depth = 500;
    if (ix->cfg.max_depth > SEL_CAP / 2) { delete ix; return fail(INFX_EINVAL, "max_depth too large%s"); }
    { int32_t rc_ = main_pool(cfg->device, &ix->pool); if (rc_) { delete ix; return rc_; } }
    *out = ix;
    return INFX_OK;
}

void infx_destroy(infx_index* ix) {
    if (!ix) return;
    hipSetDevice(ix->cfg.device);
    if (ix->comm && rccl_api().ok) rccl_api().destroy(ix->comm);
    for (void* p : ix->allocs) hipFree(p);
    delete ix->lk;
    delete ix;
}

int32_t infx_set_deleted(infx_index* ix, uint32_t total, const uint8_t* deleted) {
    if (!ix) return fail(INFX_EINVAL, "null argument%s");
    if (!ix->haveDocs) return fail(INFX_EINVAL, "infx_set_deleted before infx_upload_docs%s");
    if (deleted && total != (uint32_t)ix->d.totalDocs) return fail(INFX_EINVAL, "infx_set_deleted: one flag per global internal id (total_docs) is required%s");
    HIPCHK(enter_device(ix->cfg.device));
    HIPCHK(hipDeviceSynchronize());
    if (!deleted) { ix->d.deleted = nullptr; return INFX_OK; }
    bool any = false; for (uint32_t i = 0; i < total && !any; i++) any = deleted[i] != 0;
    if (!any) { ix->d.deleted = nullptr; return INFX_OK; }           // the kernels test the pointer: no per-row gather while nothing is deleted
    if (!ix->dDeleted) HIPCHK(dalloc(ix, &ix->dDeleted, (size_t)total));
    HIPCHK(hipMemcpy(ix->dDeleted, deleted, (size_t)total, hipMemcpyHostToDevice));
    ix->d.deleted = ix->dDeleted;
    return INFX_OK;
}

// first[d] = the first live document carrying document d's key, by GLOBAL internal id (every shard holds the whole map): what a browse row's filter and
// facets look at.  Only a corpus with duplicate keys needs it; nullptr clears (keys unique: first[d] == d).  Exclusive call, as infx_set_deleted.
int32_t infx_set_post_rows(infx_index* ix, int32_t rows) {
    if (!ix) return fail(INFX_EINVAL, "null argument%s");
    if (rows < INFX_FILTER_MAX_ROWS || rows > INFX_POST_MAX_ROWS) return fail(INFX_EINVAL, "post rows lie outside [INFX_FILTER_MAX_ROWS (64), INFX_POST_MAX_ROWS (1024)]%s");
    ix->postRows = (uint32_t)rows;
    return INFX_OK;
}
int32_t infx_get_post_rows(infx_index* ix, int32_t* rows) {
    if (!ix || !rows) return fail(INFX_EINVAL, "null argument%s");
    *rows = (int32_t)ix->postRows;
    return INFX_OK;
}
int32_t infx_set_first_live(infx_index* ix, uint32_t total, const int32_t* first) {
    if (!ix) return fail(INFX_EINVAL, "null argument%s");
    if (!ix->haveDocs) return fail(INFX_EINVAL, "infx_set_first_live before infx_upload_docs%s");
    if (first && total != (uint32_t)ix->d.totalDocs) return fail(INFX_EINVAL, "infx_set_first_live: one entry per global internal id (total_docs) is required%s");
    if (first) for (uint32_t i = 0; i < total; i++) if (first[i] < 0 || (uint32_t)first[i] >= total) return fail(INFX_EINVAL, "infx_set_first_live: entry out of range%s");
    HIPCHK(enter_device(ix->cfg.device));
    HIPCHK(hipDeviceSynchronize());
    if (!first) { ix->firstLive = nullptr; return INFX_OK; }
    if (!ix->dFirstLive || ix->firstLiveCap < total) { HIPCHK(dalloc(ix, &ix->dFirstLive, (size_t)total)); ix->firstLiveCap = total; }
    HIPCHK(hipMemcpy(ix->dFirstLive, first, (size_t)total * 4, hipMemcpyHostToDevice));
    ix->firstLive = ix->dFirstLive;
    return INFX_OK;
}

int32_t infx_upload_docs(infx_index* ix, uint32_t N, const float* doc_len, float avgdl, const int64_t* doc_key, const uint8_t* deleted,
                         const uint64_t* text_offs, const uint16_t* text) {
    if (!ix || !doc_len || !doc_key) return fail(INFX_EINVAL, "null argument%s");
    if (deleted && (ix->d.docBase != 0 || (ix->d.totalDocs != 0 && ix->d.totalDocs != (int32_t)N)))
        return fail(INFX_EINVAL, "infx_upload_docs: deleted[] is for unsharded indexes; a shard takes the global flags through infx_set_deleted%s");
    HIPCHK(enter_device(ix->cfg.device));
    ix->firstLive = nullptr;       // a map of other documents is void (infx_set_first_live follows the upload)
    float *dLen = nullptr, *dNorm = nullptr; int64_t* dKey = nullptr; uint64_t* dTO = nullptr; uint16_t* dTx = nullptr;
    HIPCHK(dalloc(ix, &dNorm, N)); HIPCHK(dalloc(ix, &dKey, N)); HIPCHK(dalloc(ix, &dLen, N));
    HIPCHK(hipMemcpy(dLen, doc_len, (size_t)N * 4, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(dKey, doc_key, (size_t)N * 8, hipMemcpyHostToDevice));
    float a = avgdl > 0.f ? avgdl : 1.f;
    float bDivAvg = 0.75f / a;     // Vector256.Create(b / avgdl), Bm25Scorer.cs:390
    if (N) k_doc_norm<<<(N + 255) / 256, 256>>>(dLen, dNorm, (int)N, bDivAvg);
    HIPCHK(hipDeviceSynchronize());
    if (text_offs && text) {
        uint64_t tot = text_offs[N];
        HIPCHK(dalloc(ix, &dTO, (size_t)N + 1)); HIPCHK(dalloc(ix, &dTx, (size_t)tot));
        HIPCHK(hipMemcpy(dTO, text_offs, ((size_t)N + 1) * 8, hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(dTx, text, (size_t)tot * 2, hipMemcpyHostToDevice));
        if (tot) {      // OrdinalIgnoreCase alias characters of the corpus (stage2.hip.inc): none in most corpora — then every Stage-2 comparison is `==`
            unsigned long long* dCnt = nullptr; unsigned long long hCnt = 0;
            HIPCHK(hipMalloc((void**)&dCnt, 8)); HIPCHK(hipMemset(dCnt, 0, 8));
            k_count_alias<<<(unsigned)std::min<uint64_t>((tot + 255) / 256, 65536), 256>>>(dTx, (unsigned long long)tot, dCnt);
            HIPCHK(hipGetLastError()); HIPCHK(hipMemcpy(&hCnt, dCnt, 8, hipMemcpyDeviceToHost)); hipFree(dCnt);
            ix->hasAlias = hCnt != 0;
        }
    }
    if (ix->cfg.range_docs == 0) {   // default: wide ranges for large shards (fewer, longer per-range posting slices; measured best at 10M docs)
        int R = N >= (4u << 20) ? 8192 : N >= (1u << 20) ? 4096 : N >= (1u << 18) ? 2048 : 1024;
        ix->d.R = R; ix->d.rshift = __builtin_ctz(R);
    }
    ix->d.N = (int32_t)N; ix->d.docNorm = dNorm; ix->d.docLen = dLen; ix->d.docKey = dKey; if (!ix->d.docKeyAll) ix->d.docKeyAll = dKey; ix->d.textOff = dTO; ix->d.text = dTx;
    ix->d.nRanges = (int32_t)(((uint64_t)N + ix->d.R - 1) >> ix->d.rshift);
    if (ix->d.nRanges == 0) ix->d.nRanges = 1;
    if (ix->d.totalDocs == 0) ix->d.totalDocs = (int32_t)N;
    ix->avgdl = avgdl; ix->haveDocs = true;
    if (deleted) return infx_set_deleted(ix, N, deleted);
    return INFX_OK;
}

int32_t infx_upload_postings(infx_index* ix, uint32_t T, const uint64_t* offs, const int32_t* doc_ids, const uint8_t* tf, const int32_t* df) {
    if (!ix || !offs || !df) return fail(INFX_EINVAL, "null argument%s");
    if (!ix->haveDocs) return fail(INFX_EINVAL, "infx_upload_docs must precede infx_upload_postings (range count)%s");
    HIPCHK(enter_device(ix->cfg.device));
    uint64_t P = offs[T];
    uint64_t* dOff = nullptr; int32_t* dDoc = nullptr; uint8_t* dW = nullptr;
    // padded layout (k_pad_lists): list t lives at [off2[t], off2[t] + len_t), the rest of its 4-aligned slot holds sentinels
    std::vector<uint64_t> off2((size_t)T + 1); off2[0] = 0;
    for (uint32_t t = 0; t < T; t++) off2[t + 1] = off2[t] + ((offs[t + 1] - offs[t] + 3) & ~(uint64_t)3);
    const uint64_t P2 = off2[T];
    HIPCHK(dalloc(ix, &dOff, (size_t)T + 1)); HIPCHK(dalloc(ix, &dDoc, (size_t)P2 + 4)); HIPCHK(dalloc(ix, &dW, (size_t)P2 + 4));
    HIPCHK(hipMemcpy(dOff, off2.data(), ((size_t)T + 1) * 8, hipMemcpyHostToDevice));
    // packed postings: (doc << 8) | tf in one word — the tf of a candidate posting needs no second (gather) access and a posting costs 4 B
    // instead of 5 B of traffic; possible while shard-local doc ids stay below 2^24 - 1 (sentinel 0xFFFFFFFF decodes to doc 2^24 - 1)
    // (every doc id a range boundary can name must stay below the sentinel's doc field, so the padded range count is what matters)
    ix->d.packed = ((uint64_t)ix->d.nRanges * (uint64_t)ix->d.R <= 0xFFFFFFull && !getenv("INFX_UNPACKED")) ? 1 : 0;
    HIPCHK(hipMemset(dDoc, ix->d.packed ? 0xFF : 0x7F, ((size_t)P2 + 4) * 4)); HIPCHK(hipMemset(dW, 0, (size_t)P2 + 4));
    if (P) {
        uint64_t* tOff = nullptr; int32_t* tDoc = nullptr; uint8_t* tW = nullptr;
        HIPCHK(hipMalloc((void**)&tOff, ((size_t)T + 1) * 8)); HIPCHK(hipMalloc((void**)&tDoc, (size_t)P * 4)); HIPCHK(hipMalloc((void**)&tW, (size_t)P));
        HIPCHK(hipMemcpy(tOff, offs, ((size_t)T + 1) * 8, hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(tDoc, doc_ids, (size_t)P * 4, hipMemcpyHostToDevice)); HIPCHK(hipMemcpy(tW, tf, (size_t)P, hipMemcpyHostToDevice));
        k_pad_lists<<<(unsigned)((P + 255) / 256), 256>>>(tOff, dOff, T, P, tDoc, tW, dDoc, dW, ix->d.packed);
        HIPCHK(hipDeviceSynchronize());
        hipFree(tOff); hipFree(tDoc); hipFree(tW);
    }
    ix->hPostOff = off2; ix->hDf.assign(df, df + T);
    ix->hPostLen.resize(T); for (uint32_t t = 0; t < T; t++) ix->hPostLen[t] = offs[t + 1] - offs[t];
    // Range skip tables (nRanges+1 offsets per list): a workgroup finds a list's slice inside its doc range with one lookup
    // instead of two ~log2(df)-step binary searches whose dependent L2 round trips every (query, range) workgroup would pay.
    // HBM is plentiful, so every list of >= 64 postings gets one as long as the tables stay below 2^31 entries (8 GiB);
    // otherwise the threshold doubles until they fit.
    int nR = ix->d.nRanges;
    std::vector<uint32_t> skipIdx(T, 0xFFFFFFFFu), skipTerms;
    uint64_t per = (uint64_t)nR + 1;
    uint64_t thr = 64;
    for (;; thr *= 2) {
        uint64_t n = 0; for (uint32_t t = 0; t < T; t++) if (offs[t + 1] - offs[t] >= thr) n++;
        if (n * per <= 0x7FFFFFFFull) break;
    }
    for (uint32_t t = 0; t < T; t++) {
        uint64_t len = offs[t + 1] - offs[t];
        if (len >= thr) { skipIdx[t] = (uint32_t)(skipTerms.size() * per); skipTerms.push_back(t); }
    }
    uint32_t *dSkipIdx = nullptr, *dSkipTbl = nullptr, *dSkipTerms = nullptr;
    HIPCHK(dalloc(ix, &dSkipIdx, T)); HIPCHK(dalloc(ix, &dSkipTbl, skipTerms.size() * per));
    HIPCHK(hipMemcpy(dSkipIdx, skipIdx.data(), (size_t)T * 4, hipMemcpyHostToDevice));
    if (!skipTerms.empty()) {
        if (skipTerms.size() * per > 0xFFFFFFF0ull) return fail(INFX_EINVAL, "skip table exceeds 32-bit indexing%s");
        HIPCHK(hipMalloc((void**)&dSkipTerms, skipTerms.size() * 4));
        HIPCHK(hipMemcpy(dSkipTerms, skipTerms.data(), skipTerms.size() * 4, hipMemcpyHostToDevice));
        uint64_t tot = skipTerms.size() * per;
        k_build_skip<<<(unsigned)((tot + 255) / 256), 256>>>(dOff, dDoc, dSkipTerms, (uint32_t)skipTerms.size(), dSkipTbl, nR, ix->d.rshift, ix->d.packed);
        HIPCHK(hipDeviceSynchronize());
        hipFree(dSkipTerms);
    }
    ix->hSkipIdx = std::move(skipIdx);
    ix->d.T = (int32_t)T; ix->d.postOff = dOff; ix->d.postDoc = dDoc; ix->d.postW = dW; ix->d.skipIdx = dSkipIdx; ix->d.skipTbl = dSkipTbl;
    ix->havePostings = true;
    return INFX_OK;
}

int32_t infx_upload_prefix_docsets(infx_index* ix, uint32_t nsets, const uint64_t* offs, const int32_t* docs) {
    if (!ix || (nsets && !offs)) return fail(INFX_EINVAL, "null argument%s");
    HIPCHK(enter_device(ix->cfg.device));
    uint64_t* dOff = nullptr; int32_t* dDocs = nullptr;
    uint64_t tot = nsets ? offs[nsets] : 0;
    HIPCHK(dalloc(ix, &dOff, (size_t)nsets + 1)); HIPCHK(dalloc(ix, &dDocs, (size_t)tot));
    if (nsets) { HIPCHK(hipMemcpy(dOff, offs, ((size_t)nsets + 1) * 8, hipMemcpyHostToDevice)); }
    else { uint64_t z = 0; HIPCHK(hipMemcpy(dOff, &z, 8, hipMemcpyHostToDevice)); }
    if (tot) HIPCHK(hipMemcpy(dDocs, docs, (size_t)tot * 4, hipMemcpyHostToDevice));
    {   // range skip tables for the DocSets too (same layout as the posting lists')
        if (!ix->haveDocs) return fail(INFX_EINVAL, "infx_upload_docs must precede infx_upload_prefix_docsets (range count)%s");
        const int nR = ix->d.nRanges; const uint64_t per = (uint64_t)nR + 1;
        std::vector<uint32_t> psSkip(std::max<uint32_t>(nsets, 1), 0xFFFFFFFFu), sets;
        for (uint32_t k = 0; k < nsets; k++) if (offs[k + 1] - offs[k] >= 64 && (sets.size() + 1) * per <= 0x7FFFFFFFull) { psSkip[k] = (uint32_t)(sets.size() * per); sets.push_back(k); }
        uint32_t *dPsSkip = nullptr, *dPsTbl = nullptr, *dSets = nullptr;
        HIPCHK(dalloc(ix, &dPsSkip, psSkip.size())); HIPCHK(dalloc(ix, &dPsTbl, sets.size() * per));
        HIPCHK(hipMemcpy(dPsSkip, psSkip.data(), psSkip.size() * 4, hipMemcpyHostToDevice));
        if (!sets.empty()) {
            HIPCHK(hipMalloc((void**)&dSets, sets.size() * 4));
            HIPCHK(hipMemcpy(dSets, sets.data(), sets.size() * 4, hipMemcpyHostToDevice));
            uint64_t n = sets.size() * per;
            k_build_skip<<<(unsigned)((n + 255) / 256), 256>>>(dOff, dDocs, dSets, (uint32_t)sets.size(), dPsTbl, nR, ix->d.rshift, 0);
            HIPCHK(hipDeviceSynchronize());
            hipFree(dSets);
        }
        ix->d.psSkip = dPsSkip; ix->d.psSkipTbl = dPsTbl;
    }
    ix->d.psOff = dOff; ix->d.psDocs = dDocs; ix->d.nSets = nsets;
    if (nsets) ix->hPsOff.assign(offs, offs + nsets + 1); else ix->hPsOff.assign(1, 0);
    return INFX_OK;
}

int32_t infx_set_shard(infx_index* ix, int32_t rank, int32_t nranks, int32_t doc_base, int32_t total_docs) {
    if (!ix || nranks < 1 || rank < 0 || rank >= nranks) return fail(INFX_EINVAL, "bad shard arguments%s");
    if (ix->d.totalDocs != total_docs) ix->firstLive = nullptr;
    ix->rank = rank; ix->nranks = nranks; ix->d.docBase = doc_base; ix->d.totalDocs = total_docs;
    return INFX_OK;
}

int32_t infx_rccl_unique_id(void* id128) {
    if (!id128) return fail(INFX_EINVAL, "null argument%s");
    if (!rccl_api().ok) return fail(INFX_ENCCL, "RCCL unavailable: %s", rccl_api().why);
    ncclUniqueId id; NCCLCHK(rccl_api().getId(&id));
    static_assert(sizeof(ncclUniqueId) == INFX_RCCL_ID_BYTES, "ncclUniqueId is 128 bytes");
    std::memcpy(id128, &id, sizeof id); return INFX_OK;
}
int32_t infx_set_shard_comm(infx_index* ix, const void* id128) {
    if (!ix || !id128) return fail(INFX_EINVAL, "null argument%s");
    if (!rccl_api().ok) return fail(INFX_ENCCL, "RCCL unavailable: %s", rccl_api().why);
    if (ix->comm) return fail(INFX_EINVAL, "this index already joined a communicator%s");
    HIPCHK(enter_device(ix->cfg.device));
    ncclUniqueId id; std::memcpy(&id, id128, sizeof id);
    NCCLCHK(rccl_api().init(&ix->comm, ix->nranks, id, ix->rank));
    return INFX_OK;
}
int32_t infx_stream_comm(infx_stream* s, const void* id128) {
    if (!s || !id128) return fail(INFX_EINVAL, "null argument%s");
    if (!rccl_api().ok) return fail(INFX_ENCCL, "RCCL unavailable: %s", rccl_api().why);
    if (s->comm) return fail(INFX_EINVAL, "this stream already joined a communicator%s");
    HIPCHK(enter_device(s->ix->cfg.device));
    ncclUniqueId id; std::memcpy(&id, id128, sizeof id);
    NCCLCHK(rccl_api().init(&s->comm, s->ix->nranks, id, s->ix->rank));
    return INFX_OK;
}
int32_t infx_comm_allreduce_sum_u32(infx_stream* s, void* buf, uint64_t count) {
    if (!s || (count && !buf)) return fail(INFX_EINVAL, "null argument%s");
    ncclComm_t c = s->comm ? s->comm : s->ix->comm;
    if (!c) return fail(INFX_EINVAL, "infx_set_shard_comm / infx_stream_comm has not been called%s");
    if (!count) return INFX_OK;
    NCCLCHK(rccl_api().allreduce(buf, buf, (size_t)count, ncclUint32, ncclSum, c, s->st)); s->unsynced = true;
    return INFX_OK;
}
int32_t infx_comm_allgather(infx_stream* s, const void* send, void* recv, uint64_t bytes) {
    if (!s || (bytes && (!send || !recv))) return fail(INFX_EINVAL, "null argument%s");
    ncclComm_t c = s->comm ? s->comm : s->ix->comm;
    if (!c) return fail(INFX_EINVAL, "infx_set_shard_comm / infx_stream_comm has not been called%s");
    if (!bytes) return INFX_OK;
    NCCLCHK(rccl_api().allgather(send, recv, (size_t)bytes, ncclUint8, c, s->st)); s->unsynced = true;
    return INFX_OK;
}
int32_t infx_stream_scratch(infx_stream* s, int32_t slot, uint64_t bytes, void** out) {
    if (!s || !out || slot < 0 || slot >= 16) return fail(INFX_EINVAL, "bad scratch arguments%s");
    HIPCHK(enter_device(s->ix->cfg.device));
    if (bytes > s->capScratch[slot]) {
        if (s->unsynced) { int32_t rc_ = stream_sync(s); if (rc_) return rc_; }      // work queued on the old buffer
        GROW(s->scratch[slot], s->capScratch[slot], (size_t)bytes);
    }
    *out = s->scratch[slot]; return INFX_OK;
}
int32_t infx_stream_copy(infx_stream* s, void* dst, const void* src, uint64_t bytes) {
    if (!s || (bytes && (!dst || !src))) return fail(INFX_EINVAL, "null argument%s");
    if (!bytes) return INFX_OK;
    HIPCHK(enter_device(s->ix->cfg.device));
    const bool dd = is_device_ptr(dst), sd = is_device_ptr(src);
    if (dd && sd) { HIPCHK(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, s->st)); s->unsynced = true; return INFX_OK; }
    if (dd) return up(s, dst, src, bytes);
    if (sd) return down(s, dst, src, bytes);
    if (s->unsynced) { int32_t rc_ = stream_sync(s); if (rc_) return rc_; }
    std::memcpy(dst, src, bytes); return INFX_OK;
}
int32_t infx_stream_unpack(infx_stream* s, const void* src, uint64_t stride, int32_t nranks, int32_t nparts, const uint64_t* part_bytes, void* const* dsts) {
    if (!s || !src || nranks < 1 || nparts < 1 || nparts > 4 || !part_bytes || !dsts) return fail(INFX_EINVAL, "bad unpack arguments%s");
    uint64_t tot = 0; for (int p = 0; p < nparts; p++) { if (!dsts[p] || (part_bytes[p] & 3)) return fail(INFX_EINVAL, "unpack parts are whole 32-bit words%s"); tot += part_bytes[p]; }
    if (tot > stride || (stride & 3)) return fail(INFX_EINVAL, "unpack parts exceed the block%s");
    HIPCHK(enter_device(s->ix->cfg.device));
    if (is_device_ptr(src)) {
        UnpackArgs a{}; a.src = (const uint32_t*)src; a.strideW = stride >> 2; a.nranks = nranks; a.nparts = nparts;
        uint64_t off = 0; for (int p = 0; p < nparts; p++) { a.offW[p] = off >> 2; a.lenW[p] = part_bytes[p] >> 2; a.dst[p] = (uint32_t*)dsts[p]; off += part_bytes[p]; }
        const uint64_t words = (tot >> 2) * (uint64_t)nranks;
        const unsigned blocks = (unsigned)std::min<uint64_t>(4096, (words + 255) / 256);
        if (blocks) k_unpack<<<blocks, 256, 0, s->st>>>(a);
        HIPCHK(hipGetLastError()); s->unsynced = true;
    } else {
        uint64_t off = 0;
        for (int p = 0; p < nparts; p++) { for (int r = 0; r < nranks; r++) std::memcpy((char*)dsts[p] + (uint64_t)r * part_bytes[p], (const char*)src + (uint64_t)r * stride + off, part_bytes[p]); off += part_bytes[p]; }
    }
    return INFX_OK;
}
int32_t infx_stream_fill0(infx_stream* s, void* dev, uint64_t bytes) {
    if (!s || (bytes && !dev)) return fail(INFX_EINVAL, "null argument%s");
    if (bytes) { HIPCHK(enter_device(s->ix->cfg.device)); HIPCHK(hipMemsetAsync(dev, 0, bytes, s->st)); s->unsynced = true; }
    return INFX_OK;
}
static int32_t mask_flush(infx_stream* s);
int32_t infx_stream_wait(infx_stream* s) {
    if (!s) return fail(INFX_EINVAL, "null argument%s");
    HIPCHK(enter_device(s->ix->cfg.device));
    if (s->mkStaged) {      // a staged mask build (infx_filter_masks) that no batch has taken: built now
        { int32_t rc_ = pin_reset(s); if (rc_) return rc_; }
        { int32_t rc_ = mask_flush(s); if (rc_) return rc_; }
    }
    return stream_sync(s);
}

int32_t infx_stream_native(infx_stream* s, void** hip_stream) {
    if (!s || !hip_stream) return fail(INFX_EINVAL, "null argument%s");
    *hip_stream = (void*)s->st; return INFX_OK;
}
int32_t infx_stream_budget(infx_stream* s, int32_t* normal, int32_t* high) {
    if (!s || !normal || !high) return fail(INFX_EINVAL, "null argument%s");
    *normal = (s->stMain ? 1 : 0) + (s->stAux ? 1 : 0); *high = s->stPlan ? 1 : 0; return INFX_OK;
}

int32_t infx_stream_create(infx_index* ix, infx_stream** out) {
    if (!ix || !out) return fail(INFX_EINVAL, "null argument%s");
    HIPCHK(enter_device(ix->cfg.device));
    infx_stream* s = new infx_stream(); s->ix = ix;
    {
        static const bool noPrio = [] { const char* e = getenv("INFX_PLAN_PRIORITY"); return e && e[0] == '0'; }();
        int least = 0, greatest = 0;
        if (!noPrio && hipDeviceGetStreamPriorityRange(&least, &greatest) == hipSuccess && greatest != least &&
            hipStreamCreateWithPriority(&s->stPlan, hipStreamNonBlocking, greatest) == hipSuccess) HIPCHK(hipEventCreateWithFlags(&s->evPlan, hipEventDisableTiming));
        else { (void)hipGetLastError(); s->stPlan = nullptr; }
    }
    {
        // Opt-in (INFX_REPLAY_AUX=1), for processes with more hardware queues than streams.  The runtime serves streams from a small pool of hardware queues
        // (4 by default) and a stream beyond the pool shares a queue, idle or not: with a second normal-priority stream per session the main streams of two
        // sessions met on one queue and ran one after the other (profiles/hwqueues_default.md).  Not created unless asked for.
        static const bool aux = [] { const char* e = getenv("INFX_REPLAY_AUX"); return e && e[0] == '1'; }();
        if (aux) { HIPCHK(hipStreamCreateWithFlags(&s->stAux, hipStreamNonBlocking)); HIPCHK(hipEventCreateWithFlags(&s->evJoin, hipEventDisableTiming)); }
    }
    HIPCHK(hipEventCreateWithFlags(&s->evTurn, hipEventDisableTiming));
    hipEvent_t* ev[] = {&s->evA0, &s->evA1, &s->evS0, &s->evS1, &s->evC0, &s->evC1, &s->evP0, &s->evP1, &s->evF0, &s->evF1, &s->evX0, &s->evX1, &s->evXa, &s->evXb, &s->evXc};
    for (auto e : ev) HIPCHK(hipEventCreate(e));
    HIPCHK(hipEventCreateWithFlags(&s->evSync, hipEventBlockingSync | hipEventDisableTiming));
    HIPCHK(hipMalloc((void**)&s->dCursor, 16)); HIPCHK(hipMalloc((void**)&s->dOverflow, 4));
    HIPCHK(hipMalloc((void**)&s->dStats, 64)); HIPCHK(hipMemset(s->dStats, 0, 64));
    HIPCHK(hipMalloc((void**)&s->dExactStat, 32)); HIPCHK(hipMemset(s->dExactStat, 0, 32));      // [0..3] replay outcome counters, [4..7] k_select flag reasons
    HIPCHK(hipMalloc((void**)&s->exCounters, 32)); HIPCHK(hipMemset(s->exCounters, 0, 32));
    {   // taken last, so that a creation that fails above leaves no user count behind: the device's main stream with the fewest users (the first among equals: the engine's own session, created first and idle while sessions run, is the one shared)
        MainPool* mp = ix->pool; std::lock_guard<std::mutex> lk(mp->mu);
        int best = 0; for (int i = 1; i < (int)mp->st.size(); i++) if (mp->users[i] < mp->users[best]) best = i;
        s->st = mp->st[best]; s->mainSlot = best; mp->users[best]++;
    }
    s->stMain = s->st;
    *out = s; return INFX_OK;
}
void infx_stream_destroy(infx_stream* s) {
    if (!s) return;
    hipSetDevice(s->ix->cfg.device);
    void* ps[] = {s->dQueries, s->dTerms, s->dExtra, s->dRules, s->dHits, s->dHitCount, s->dBlockOut, s->dBlockOutHi, s->dQBytes, s->dUOffs, s->dUMem, s->dUCnt, s->dURange, s->dUBase, s->dUDocs, s->dCounts,
                  s->dCovQ, s->dCovC, s->dCovO, s->dCovF, s->arDoc, s->arScore, s->arCls, s->dCursor, s->dOverflow,
                  s->dFQ, s->dFLists, s->dFOwned, s->dFS1, s->dFMeta, s->dFQueries, s->dFKeys, s->dFScores, s->dFTies, s->dFCounts, s->dFFlags, s->dFErr, s->dFHitsAll, s->dFHcAll, s->dFPairs, s->arMask, s->dDir, s->dFDocs, s->dFacetCols, s->dFacCodes, s->dFacCounts, s->dFacN, s->dPostBlob, s->dQCount, s->dBrwBlob, s->dBrwWork, s->dFacAll, s->dRefTerms, s->dExactFlag, s->dExactStat, s->arExc, s->exCand, s->exOut, s->exChunks, s->exQueries, s->exTasks, s->exCounters, s->exContEnd, s->dExProf, s->dSelOrder,
                  s->dNext, s->dPrior, s->shBlob, s->dAllBlobs, s->dAllNext, s->dChainState, s->dChainNeed, s->dHugeWs, s->dHugeCnt, s->dLWordOff, s->dLChars, s->dLMembers, s->dLCount, s->dDense, s->dSelG, s->dAccOrder, s->dFin, s->dMaskBlob, s->dMaskCnt, s->dQDel, s->dClp, s->dHl, s->dLfCnt};
    for (void* p : s->dMask) if (p) hipFree(p);
    for (const SetKindState& K : s->kind) { if (K.ws) hipFree(K.ws); if (K.out) hipFree(K.out); }
    for (void* p : ps) if (p) hipFree(p);
    for (void* p : s->scratch) if (p) hipFree(p);
    for (void* p : s->parked) hipFree(p);
    if (s->comm && rccl_api().ok) rccl_api().destroy(s->comm);
    if (s->st) hipStreamSynchronize(s->st);
    for (auto& c : s->pins) hipHostFree(c.base);
    hipEvent_t ev[] = {s->evA0, s->evA1, s->evS0, s->evS1, s->evC0, s->evC1, s->evP0, s->evP1, s->evF0, s->evF1, s->evX0, s->evX1, s->evXa, s->evXb, s->evXc};
    for (auto e : ev) hipEventDestroy(e);
    hipEventDestroy(s->evSync);
    if (s->evPlan) hipEventDestroy(s->evPlan);
    if (s->evJoin) hipEventDestroy(s->evJoin);
    if (s->evK0) hipEventDestroy(s->evK0);
    if (s->evK1) hipEventDestroy(s->evK1);
    if (s->evH0) hipEventDestroy(s->evH0);
    if (s->evH1) hipEventDestroy(s->evH1);
    { std::lock_guard<std::mutex> lk(s->ix->turnMu); if (s->ix->turnEvent == s->evTurn) s->ix->turnEvent = nullptr; }
    if (s->evTurn) hipEventDestroy(s->evTurn);
    if (s->stAux) { hipStreamSynchronize(s->stAux); hipStreamDestroy(s->stAux); }
    if (s->stPlan) { hipStreamSynchronize(s->stPlan); hipStreamDestroy(s->stPlan); }
    if (s->mainSlot >= 0) { std::lock_guard<std::mutex> lk(s->ix->pool->mu); s->ix->pool->users[s->mainSlot]--; }
    delete s;
}

// Everything of a Stage-1 accumulate launch up to (and including) the kernel: translation of the query terms into device
// entries, arena bounds, uploads, launch.  No synchronisation.
static int32_t acc_enqueue(infx_stream* s, uint32_t nq, const infx_query* q, uint32_t nterms, const infx_term* terms,
                           uint32_t extra_n, const int32_t* extra_docs) {
    infx_index* ix = s->ix;
    if ((uint64_t)nq * ((uint64_t)ix->d.nRanges + 8) > 0x7FFFFFFFull) return fail(INFX_ECAPACITY, "nq * nRanges exceeds the grid limit; split the batch%s");
    // translate + capacity bound.  A virtual term given as a MEMBER LIST (infx_term.reserved == 1: extra_docs[extra_off..+len) are index
    // term ids) is expanded into one device entry per member, all sharing the term's idf / role / rank and a dedupe group.
    std::vector<DevQuery> dq(nq); std::vector<DevTerm> dt; dt.reserve(nterms + 64);
    std::vector<int32_t> termOfEntry; termOfEntry.reserve(nterms + 64);
    std::vector<DevRefTerm> refT(std::max<uint32_t>(1, nterms));
    for (uint32_t k = 0; k < nterms; k++) refT[k] = DevRefTerm{terms[k].idf, terms[k].max_score, terms[k].term_id, terms[k].term_id < 0 ? 1u : 0u};
    std::vector<unsigned long long> qbase((size_t)nq + 1); unsigned long long maxQb = 0;
    unsigned long long bound = 0; int maxT = 1, useGrp = 0, maxRef = 0, maxRefNarrow = 0; std::vector<uint32_t> wideQ;
    for (uint32_t i = 0; i < nq; i++) {
        const infx_query& Q = q[i];
        if (Q.num_terms > INFX_MAX_QUERY_TERMS || (uint64_t)Q.term_off + Q.num_terms > nterms) return fail(INFX_EINVAL, "bad term range%s");
        if (Q.depth <= 0 || Q.depth > ix->cfg.max_depth) return fail(INFX_EINVAL, "query depth exceeds infx_config.max_depth%s");
        if (Q.mode < INFX_MODE_PREFIX || Q.mode > INFX_MODE_AND) return fail(INFX_EINVAL, "bad query mode%s");
        if (Q.prefix_set >= (int32_t)ix->d.nSets || (Q.mode == INFX_MODE_PREFIX && Q.prefix_set < 0)) return fail(INFX_EINVAL, "bad prefix set%s");
        const uint32_t entryOff = (uint32_t)dt.size();
        unsigned long long qb = 0; int group = 0;
        for (uint32_t k = 0; k < Q.num_terms; k++) {
            const infx_term& tm = terms[Q.term_off + k];
            const bool gen = (Q.mode == INFX_MODE_AND && (tm.role & (INFX_ROLE_S1 | INFX_ROLE_S2))) ||
                             (Q.mode == INFX_MODE_DISJ && (tm.role & (INFX_ROLE_ELIGIBLE | INFX_ROLE_LOWQ)));
            DevTerm D{}; D.idf = tm.idf; D.role = tm.role; D.rank = tm.rank; D.pad = 0; D.refIdx = (uint16_t)k; D.pad2 = 0;
            if (tm.term_id >= 0) {
                if (tm.term_id >= ix->d.T) return fail(INFX_EINVAL, "term id out of range%s");
                D.begin = ix->hPostOff[tm.term_id]; D.end = D.begin + ix->hPostLen[tm.term_id]; D.isVirtual = 0;
                dt.push_back(D); termOfEntry.push_back(tm.term_id);
                if (gen) qb += D.end - D.begin;
            } else if (tm.reserved == 2) {     // union built on the device by the last infx_union_build: extra_off = its index
                if (tm.extra_off >= s->unionCount.size()) return fail(INFX_EINVAL, "virtual term refers to a union that was not built%s");
                D.begin = s->unionBase[tm.extra_off]; D.end = D.begin + s->unionCount[tm.extra_off]; D.isVirtual = 4 | 2;
                D.skip = (uint32_t)((uint64_t)tm.extra_off * (ix->d.nRanges + 1));     // k_union's per-range offsets are its skip table
                dt.push_back(D); termOfEntry.push_back(-1);
                if (gen) qb += D.end - D.begin;
            } else if (tm.reserved == 1) {
                if ((uint64_t)tm.extra_off + tm.extra_len > extra_n) return fail(INFX_EINVAL, "virtual term member list out of range%s");
                if (++group > 255) return fail(INFX_ECAPACITY, "more than 255 fuzzy virtual terms in one query%s");
                useGrp = 1;
                for (uint32_t m = 0; m < tm.extra_len; m++) {
                    int32_t mt = extra_docs[tm.extra_off + m];
                    if (mt < 0 || mt >= ix->d.T) return fail(INFX_EINVAL, "member term id out of range%s");
                    DevTerm M = D; M.begin = ix->hPostOff[mt]; M.end = M.begin + ix->hPostLen[mt]; M.isVirtual = 2; M.pad = (uint8_t)group;
                    dt.push_back(M); termOfEntry.push_back(mt);
                    if (gen) qb += M.end - M.begin;
                }
            } else {
                if ((uint64_t)tm.extra_off + tm.extra_len > extra_n) return fail(INFX_EINVAL, "virtual term slice out of range%s");
                D.begin = tm.extra_off; D.end = (uint64_t)tm.extra_off + tm.extra_len; D.isVirtual = 1; D.skip = 0xFFFFFFFFu;
                dt.push_back(D); termOfEntry.push_back(-1);
                if (gen) qb += D.end - D.begin;
            }
        }
        const uint32_t nEntries = (uint32_t)dt.size() - entryOff;
        if (nEntries > 2048) return fail(INFX_ECAPACITY, "query expands to more than 2048 posting lists (fuzzy member lists); materialise the union on the host%s");
        dq[i] = DevQuery{entryOff, nEntries, Q.mode, Q.prefix_set, Q.depth, Q.n_and, Q.term_off, Q.num_terms};
        maxT = std::max(maxT, (int)nEntries); maxRef = std::max(maxRef, (int)Q.num_terms);
        if (Q.num_terms > 64) wideQ.push_back(i); else maxRefNarrow = std::max(maxRefNarrow, (int)Q.num_terms);
        if (Q.mode == INFX_MODE_PREFIX) qb = ix->hPsOff[Q.prefix_set + 1] - ix->hPsOff[Q.prefix_set];
        qbase[i] = bound;
        bound += std::min<unsigned long long>(qb, (unsigned long long)ix->d.N);
        maxQb = std::max(maxQb, std::min<unsigned long long>(qb, (unsigned long long)ix->d.N));
    }
    qbase[nq] = bound;
    {   // k_accumulate's block order: queries by row bound, descending; "heavy" = at least INFX_ACC_HEAVY_ROWS (default 393216) candidate rows possible, at most 64 queries
        static const long long heavyRows = [] { const char* e = getenv("INFX_ACC_HEAVY_ROWS"); return e ? atoll(e) : 393216ll; }();      // 0: query order
        s->nAccHeavy = 0xFFFFFFFFu;
        if (heavyRows > 0 && nq > 1) {
            std::vector<uint32_t> ord(nq); for (uint32_t i = 0; i < nq; i++) ord[i] = i;
            std::stable_sort(ord.begin(), ord.end(), [&](uint32_t a, uint32_t b) { return qbase[a + 1] - qbase[a] > qbase[b + 1] - qbase[b]; });
            uint32_t h = 0; while (h < nq - 1 && h < 64u && qbase[ord[h] + 1] - qbase[ord[h]] >= (unsigned long long)heavyRows) h++;
            GROW(s->dAccOrder, s->capAccOrder, (size_t)nq * 4); UP(s->dAccOrder, ord.data(), (size_t)nq * 4);
            s->nAccHeavy = h;
        }
    }
    { const unsigned long long gm = giant_min_rows(); uint32_t c = 0; if (gm) for (uint32_t i = 0; i < nq; i++) if (qbase[i + 1] - qbase[i] >= gm) c++; s->nBoundGiants = c; }
    s->maxQueryBound = maxQb;      // no query of the batch can hold more rows than this (select_giants: nothing to sweep outside k_select below its threshold)
    {   // INFX_ACC_SHARE_STATS=1 (profiling): how many posting bytes do the queries of the batch share?  total = sum over (query, list) of the list length;
        // distinct = every list once; by XCD = every list once per XCD under the current block -> XCD assignment (q % 8) and under a chunked assignment of
        // the queries sorted by their longest list
        static const bool want = [] { const char* e = getenv("INFX_ACC_SHARE_STATS"); return e && e[0] == '1'; }();
        if (want) {
            unsigned long long total = 0, distinct = 0, byMod = 0, byChunk = 0;
            std::vector<std::pair<unsigned long long, uint32_t>> order(nq);       // (begin of the longest list, query)
            for (uint32_t i = 0; i < nq; i++) {
                unsigned long long bestLen = 0, bestBeg = 0;
                for (uint32_t k = 0; k < dq[i].numTerms; k++) { const DevTerm& D = dt[dq[i].termOff + k]; const unsigned long long L = D.end - D.begin; total += L; if (!D.isVirtual && L > bestLen) { bestLen = L; bestBeg = D.begin; } }
                order[i] = {bestBeg, i};
            }
            std::sort(order.begin(), order.end());
            std::vector<uint32_t> chunkOf(nq); for (uint32_t j = 0; j < nq; j++) chunkOf[order[j].second] = (uint32_t)((uint64_t)j * 8 / nq);
            std::unordered_map<unsigned long long, uint32_t> seenAll, seenMod, seenChunk;      // begin -> bitmask of XCDs that already fetch it
            for (uint32_t i = 0; i < nq; i++)
                for (uint32_t k = 0; k < dq[i].numTerms; k++) {
                    const DevTerm& D = dt[dq[i].termOff + k]; const unsigned long long L = D.end - D.begin;
                    if (D.isVirtual & 5) { distinct += L; byMod += L; byChunk += L; continue; }
                    if (!seenAll[D.begin]++) distinct += L;
                    uint32_t& m = seenMod[D.begin]; if (!(m & (1u << (i & 7)))) { m |= 1u << (i & 7); byMod += L; }
                    uint32_t& c = seenChunk[D.begin]; if (!(c & (1u << chunkOf[i]))) { c |= 1u << chunkOf[i]; byChunk += L; }
                }
            fprintf(stderr, "[infx] posting sharing of the batch (%u queries): total %.2f G postings, distinct %.2f G (x%.2f), once per XCD with q %% 8: %.2f G (x%.2f), with sorted chunks: %.2f G (x%.2f)\n",
                    nq, total * 1e-9, distinct * 1e-9, (double)total / std::max(1ull, distinct), byMod * 1e-9, (double)total / std::max(1ull, byMod), byChunk * 1e-9, (double)total / std::max(1ull, byChunk));
        }
    }
    // arena
    size_t need = (size_t)bound + 64;
    if (need > s->arCap) {
        if (need > ((size_t)1 << 31)) return fail(INFX_ECAPACITY, "candidate superset bound exceeds 2^31 entries; split the batch%s");
        if (s->arDoc) { ws_release(s, s->arDoc); ws_release(s, s->arScore); ws_release(s, s->arCls); s->arDoc = nullptr; }
        // The bound (sum of the candidate-generating lists' lengths) varies by +-30 % between 1000-query batches of one workload, and a reallocation in the
        // middle of a stream is not free even without hipFree (a multi-GB hipMalloc can wait for the device): twice the first batch's need, doubling after that.
        // ~40 B per row: 5 GB per session at 10 M documents, of 288.
        size_t n = std::max(need * 2, s->arCap * 2);
        if (getenv("INFX_DEBUG_GROW")) fprintf(stderr, "[infx] arena grow: %zu -> %zu rows (need %zu)\n", s->arCap, n, need);
        if (hipMalloc((void**)&s->arDoc, n * 4) != hipSuccess || hipMalloc((void**)&s->arScore, n * 4) != hipSuccess || hipMalloc((void**)&s->arCls, n) != hipSuccess)
            return fail(INFX_ENOMEM, "arena allocation failed%s");
        s->arCap = n;
    }
    // per-row hit masks (2 bits per reference term) for the exact Stage-1 replay, as wide as the batch's queries need: one or two 64-bit words for queries of <= 64
    // terms.  A query with more terms (a very long query: words + n-grams, up to 128 = VectorModel.cs:381's cap) takes FOUR words for the rows of its whole batch
    // (round 6; rare: the masks of such a batch cost twice the bytes) and is replayed by the sequential kernel, which reads the masks from the arena (k_mark_wide,
    // k_exact1).  Document shards keep two words and the first-pass cut for such a query (k_gflag passes it over): the sharded replay's kernels hold two words.
    const bool wideExact = !wideQ.empty() && exact_enabled(ix) && ix->nranks == 1 && ix->d.docBase == 0;
    s->maskWords = !exact_enabled(ix) || (!wideExact && wideQ.size() == nq) ? 0 : (wideExact ? 4 : (maxRefNarrow <= 32 ? 1 : 2));
    s->nWide = (uint32_t)wideQ.size();
    if (s->nWide) { GROW(s->dWideQ, s->capWideQ, wideQ.size() * 4); UP(s->dWideQ, wideQ.data(), wideQ.size() * 4); }
    if (s->maskWords && s->arCap * (size_t)s->maskWords > s->arMaskCap) {
        if (s->arMask) { ws_release(s, s->arMask); s->arMask = nullptr; s->arMaskCap = 0; }
        const size_t n = s->arCap * (size_t)s->maskWords;
        if (hipMalloc((void**)&s->arMask, n * 8) != hipSuccess) return fail(INFX_ENOMEM, "arena mask allocation failed%s");
        s->arMaskCap = n;
    }
    if (s->maskWords && s->arCap > s->exCap) {
        if (s->arExc) { ws_release(s, s->arExc); ws_release(s, s->exCand); ws_release(s, s->exOut); s->arExc = nullptr; s->exCand = nullptr; s->exOut = nullptr; s->exCap = 0; }
        if (hipMalloc((void**)&s->arExc, s->arCap * 4) != hipSuccess || hipMalloc((void**)&s->exCand, s->arCap * 4) != hipSuccess || hipMalloc((void**)&s->exOut, s->arCap * sizeof(infx_hit)) != hipSuccess)
            return fail(INFX_ENOMEM, "exact-replay workspace allocation failed%s");
        s->exCap = s->arCap;
    }
    s->arBound = (size_t)bound;
    GROW(s->dDir, s->capDir, (size_t)nq * ix->d.nRanges * sizeof(uint2));
    GROW(s->dRefTerms, s->capRefTerms, refT.size() * sizeof(DevRefTerm));
    GROW(s->dExactFlag, s->capExactFlag, (size_t)nq * 4);
    GROW(s->dQueries, s->capQueries, nq * sizeof(DevQuery));
    GROW(s->dTerms, s->capTerms, std::max<size_t>(1, dt.size()) * sizeof(DevTerm));
    GROW(s->dExtra, s->capExtra, ((size_t)extra_n + 4) * 4);
    GROW(s->dUDocs, s->capUDocs, 16); GROW(s->dURange, s->capURange, 4);
    GROW(s->dBlockOut, s->capBlockOut, ((size_t)nq + 1) * 8);      // qBase
    GROW(s->dBlockOutHi, s->capBlockOutHi, (size_t)nq * 4);        // qCursor
    GROW(s->dQBytes, s->capQBytes, (size_t)nq * 12); s->lastNqAlloc = nq;      // per query: algorithmic bytes (u64) | best emitted score bits (u32, behind the nq u64s)
    GROW(s->dCounts, s->capCounts, (size_t)nq * INFX_NCLASS * 4);
    for (size_t i = 0; i < dt.size(); i++) if (termOfEntry[i] >= 0) dt[i].skip = ix->hSkipIdx[termOfEntry[i]];

    UP(s->dQueries, dq.data(), nq * sizeof(DevQuery));
    UP(s->dTerms, dt.data(), dt.size() * sizeof(DevTerm));
    UP(s->dRefTerms, refT.data(), refT.size() * sizeof(DevRefTerm));
    HIPCHK(hipMemsetAsync(s->dExactFlag, 0, (size_t)nq * 4, s->st));
    UP(s->dExtra, extra_docs, (size_t)extra_n * 4);
    UP(s->dBlockOut, qbase.data(), ((size_t)nq + 1) * 8);
    HIPCHK(hipMemsetAsync(s->dQBytes, 0, (size_t)nq * 12, s->st));
    HIPCHK(hipMemsetAsync(s->dOverflow, 0, 4, s->st));
    HIPCHK(hipMemsetAsync(s->dCounts, 0, (size_t)nq * INFX_NCLASS * 4, s->st));
    HIPCHK(hipMemsetAsync(s->dBlockOutHi, 0, (size_t)nq * 4, s->st));
    HIPCHK(hipMemsetAsync(s->dDir, 0, (size_t)nq * ix->d.nRanges * sizeof(uint2), s->st));
    Arena ar = make_arena(s);
    HIPCHK(hipEventRecord(s->evA0, s->st));
    switch (ix->d.R) {
        case 512: launch_acc<512>(s, nq, ar, maxT, useGrp, maxRef); break;
        case 1024: launch_acc<1024>(s, nq, ar, maxT, useGrp, maxRef); break;
        case 2048: launch_acc<2048>(s, nq, ar, maxT, useGrp, maxRef); break;
        case 4096: launch_acc<4096>(s, nq, ar, maxT, useGrp, maxRef); break;
        case 8192: launch_acc<8192>(s, nq, ar, maxT, useGrp, maxRef); break;
        default: launch_acc<16384>(s, nq, ar, maxT, useGrp, maxRef); break;
    }
    if (s->accLayoutBad) return fail(INFX_EHIP, "k_accumulate was built with static LDS: its byte addressing (LDS8) is invalid%s");
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(s->evA1, s->st));
    s->timedAcc = true;
    s->lastQ.assign(q, q + nq); s->lastNq = nq; s->lastExact2[0] = s->lastExact2[1] = 0; s->msReplay = 0.f; s->timedReplay = false; s->lastFlagWhy[0] = s->lastFlagWhy[1] = s->lastFlagWhy[2] = 0;
    return INFX_OK;
}

int32_t infx_stage1_accumulate(infx_stream* s, uint32_t nq, const infx_query* q, uint32_t nterms, const infx_term* terms,
                               uint32_t extra_n, const int32_t* extra_docs, infx_counts* counts_out) {
    if (!s || !q || (nterms && !terms)) return fail(INFX_EINVAL, "null argument%s");
    infx_index* ix = s->ix;
    if (!ix->havePostings || !ix->haveDocs) return fail(INFX_EINVAL, "index not uploaded%s");
    if (nq == 0) return INFX_OK;
    HIPCHK(enter_device(ix->cfg.device));
    { int32_t rc_ = pin_reset(s); if (rc_) return rc_; }
    {   // the turnstile of infx_search_fused for the staged (document-sharded) pipeline: a batch's accumulation waits, stream-side, for the accumulation of the batch
        // submitted before it on this index — the pipeline sessions of a rank take the GPU-filling kernel one after the other instead of against each other
        static const bool turnstile = [] { const char* e = getenv("INFX_TURNSTILE"); return !(e && e[0] == '0'); }();
        std::unique_lock<std::mutex> turn(ix->turnMu, std::defer_lock);
        if (turnstile) { turn.lock(); if (ix->turnEvent && ix->turnEvent != s->evTurn) HIPCHK(hipStreamWaitEvent(s->st, ix->turnEvent, 0)); }
        { int32_t rc_ = acc_enqueue(s, nq, q, nterms, terms, extra_n, extra_docs); if (rc_) return rc_; }
        if (turnstile) { HIPCHK(hipEventRecord(s->evTurn, s->st)); ix->turnEvent = s->evTurn; }
    }
    uint32_t ovf = 0; std::vector<unsigned long long> qbytes(nq);
    if (counts_out) DOWNX(counts_out, s->dCounts, (size_t)nq * INFX_NCLASS * 4);       // host memory, or a device tensor the caller all-reduces in place
    DOWN(&ovf, s->dOverflow, 4);
    DOWN(qbytes.data(), s->dQBytes, (size_t)nq * 8);
    SYNC();
    if (ovf) return fail(INFX_ECAPACITY, "candidate arena overflow (bound violated)%s");
    s->lastAlgBytes = 0; for (auto b : qbytes) s->lastAlgBytes += b;
    s->lastQ.assign(q, q + nq); s->lastNq = nq;
    return INFX_OK;
}

int32_t infx_stage1_select(infx_stream* s, uint32_t nq, const infx_counts* counts, infx_hit* out, uint32_t* out_count) {
    if (!s || !counts || !out || !out_count) return fail(INFX_EINVAL, "null argument%s");
    if (nq == 0) return INFX_OK;
    if (nq != s->lastNq) return fail(INFX_EINVAL, "infx_stage1_select must follow infx_stage1_accumulate of the same batch%s");
    infx_index* ix = s->ix;
    HIPCHK(enter_device(ix->cfg.device));
    { int32_t rc_ = pin_reset(s); if (rc_) return rc_; }
    std::vector<SelRule> rules(nq);
    int maxDepth = 0;
    s->lastCandTotal = 0;
    for (uint32_t i = 0; i < nq; i++) { rules[i] = make_rule(s->lastQ[i], counts[i].c); maxDepth = std::max(maxDepth, rules[i].depth); s->lastCandTotal += rules[i].total; }
    GROW(s->dRules, s->capRules, nq * sizeof(SelRule));
    GROW(s->dHits, s->capHits, (size_t)nq * maxDepth * sizeof(infx_hit));
    GROW(s->dHitCount, s->capHitCount, (size_t)nq * 4);
    UP(s->dRules, rules.data(), nq * sizeof(SelRule));
    Arena ar = make_arena(s);
    HIPCHK(hipEventRecord(s->evS0, s->st));
    const bool exact = exact_possible(s);
    if (exact) HIPCHK(hipMemsetAsync(s->dExactStat + 4, 0, 16, s->st));
    const uint32_t* selOrd = select_order(s, nq);
    k_select<<<nq, SEL_THREADS, 0, s->st>>>(ar, ix->d.nRanges, (const SelRule*)s->dRules, (infx_hit*)s->dHits, (uint32_t*)s->dHitCount, maxDepth, exact ? (uint32_t*)s->dExactFlag : nullptr, exact ? s->dExactStat + 4 : nullptr, nullptr, selOrd,
                                            select_giants(s, ar, nq, selOrd));
    if (exact) { int32_t rc_ = mark_wide_queries(s, ix->cfg.max_depth); if (rc_) return rc_; }
    if (exact) { int32_t rc_ = enqueue_exact(s, nq, maxDepth); if (rc_) return rc_; }
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(s->evS1, s->st));
    s->timedSel = true;
    std::vector<infx_hit> tmp((size_t)nq * maxDepth);
    DOWN(tmp.data(), s->dHits, tmp.size() * sizeof(infx_hit));
    DOWN(out_count, s->dHitCount, (size_t)nq * 4);
    SYNC();
    // caller layout: nq * depth_i packed with the query's own depth as stride == we use max depth of the batch as stride
    for (uint32_t i = 0; i < nq; i++) memcpy(out + (size_t)i * maxDepth, tmp.data() + (size_t)i * maxDepth, (size_t)out_count[i] * sizeof(infx_hit));
    return INFX_OK;
}

int32_t infx_stage1_batch(infx_stream* s, uint32_t nq, const infx_query* q, uint32_t nterms, const infx_term* terms,
                          uint32_t extra_n, const int32_t* extra_docs, infx_hit* out, uint32_t* out_count) {
    std::vector<infx_counts> counts(nq);
    int32_t rc = infx_stage1_accumulate(s, nq, q, nterms, terms, extra_n, extra_docs, counts.data());
    if (rc) return rc;
    return infx_stage1_select(s, nq, counts.data(), out, out_count);
}

int32_t infx_stage2_long_queries(infx_stream* s, uint32_t n, const infx_cov_query_long* q) {
    if (!s || (n && !q)) return fail(INFX_EINVAL, "null argument%s");
    s->nLongQ = 0;
    if (!n) return INFX_OK;
    infx_index* ix = s->ix;
    HIPCHK(enter_device(ix->cfg.device));
    // (no pin_reset: this call sits between the phases of a batch, whose pending downloads must survive it; its own upload is staged behind theirs)
    for (uint32_t i = 0; i < n; i++) {
        if (q[i].num_tokens < 0 || q[i].num_tokens > INFX_LONGQ_TOKENS || q[i].text_len < 0 || q[i].text_len > INFX_LONGQ_CHARS || q[i].num_fusion_tokens < 0 || q[i].num_fusion_tokens > 2 * INFX_LONGQ_TOKENS)
            return fail(INFX_EUNSUPPORTED, "query exceeds the long Stage-2 envelope%s");
        // the kernel dereferences text + tok_off: a token table that points outside the text would read out of bounds on the device
        for (int32_t t = 0; t < q[i].num_tokens; t++) if ((int32_t)q[i].tok_off[t] + (int32_t)q[i].tok_len[t] > q[i].text_len) return fail(INFX_EINVAL, "long query: a token lies outside the query text%s");
        for (int32_t t = 0; t < q[i].num_fusion_tokens; t++) if ((int32_t)q[i].ftok_off[t] + (int32_t)q[i].ftok_len[t] > q[i].text_len) return fail(INFX_EINVAL, "long query: a fusion token lies outside the query text%s");
    }
    GROW(s->dCovQL, s->capCovQL, (size_t)n * sizeof(infx_cov_query_long));
    UP(s->dCovQL, q, (size_t)n * sizeof(infx_cov_query_long));
    s->longAlias = false;
    for (uint32_t i = 0; i < n && !s->longAlias; i++) for (int32_t k = 0; k < q[i].text_len; k++) if (s2_host_is_alias(q[i].text[k])) { s->longAlias = true; break; }
    s->nLongQ = n;
    return INFX_OK;
}

static const infx_stage2_setup S2_DEFAULT_SETUP = {2, 20, 2, 3, 7, 1, 1, 1, 1, 1};
static const infx_finalize_setup FIN_DEFAULT_SETUP = {1, 1, 0, 254};
int32_t infx_stream_set_coverage(infx_stream* s, const infx_stage2_setup* matchers, uint32_t nq, const infx_finalize_setup* per_query) {
    if (!s) return fail(INFX_EINVAL, "null argument%s");
    s->csOn = false; s->finOn = false;
    auto bad = [](int32_t v) { return v < 0 || v > 65535; };
    if (matchers) {
        const infx_stage2_setup& m = *matchers;
        if (bad(m.min_word_size) || bad(m.lev_max_word_size) || bad(m.num_typos) || bad(m.min_len_one_typo) || bad(m.min_len_two_typos))
            return fail(INFX_EINVAL, "coverage setup: a matcher setting lies outside [0, 65535]%s");
        infx_stage2_setup c = m;      // the switches as 0 / 1
        c.cover_whole_query = m.cover_whole_query != 0; c.cover_whole_words = m.cover_whole_words != 0; c.cover_fuzzy_words = m.cover_fuzzy_words != 0;
        c.cover_joined_words = m.cover_joined_words != 0; c.cover_prefix_suffix = m.cover_prefix_suffix != 0;
        s->cs = c; s->csOn = s2_force_custom() || std::memcmp(&c, &S2_DEFAULT_SETUP, sizeof c) != 0;
    }
    if (per_query && nq) {
        for (uint32_t i = 0; i < nq; i++) if (bad(per_query[i].min_hits_abs) || bad(per_query[i].min_hits_relative) || per_query[i].truncation_score < 0 || per_query[i].truncation_score > 255) {
            s->csOn = false; return fail(INFX_EINVAL, "coverage setup: a truncation setting lies outside its range%s");
        }
        s->finH.assign(per_query, per_query + nq); s->finOn = true;
    }
    return INFX_OK;
}

int32_t infx_stage2_batch(infx_stream* s, uint32_t nq, const infx_cov_query* q, uint32_t ncand, const infx_cov_cand* cand,
                          infx_cov_out* out, int32_t* feat_out) {
    if (!s || (ncand && (!q || !cand || !out))) return fail(INFX_EINVAL, "null argument%s");
    if (ncand == 0) return INFX_OK;
    infx_index* ix = s->ix;
    if (!ix->haveDocs || !ix->d.text) return fail(INFX_EINVAL, "document text not uploaded%s");
    HIPCHK(enter_device(ix->cfg.device));
    { int32_t rc_ = pin_reset(s); if (rc_) return rc_; }
    for (uint32_t i = 0; i < nq; i++) {
        if (q[i].reserved != 0) { if (q[i].reserved < 0 || (uint32_t)q[i].reserved > s->nLongQ) return fail(INFX_EINVAL, "query refers to a missing long-query record (infx_stage2_long_queries)%s"); continue; }
        if (q[i].num_tokens > INFX_MAX_QUERY_TOKENS || q[i].text_len > INFX_MAX_QUERY_CHARS || q[i].num_fusion_tokens > 2 * INFX_MAX_QUERY_TOKENS)
            return fail(INFX_EUNSUPPORTED, "query exceeds the Stage-2 envelope (hand it over as a long query: infx_stage2_long_queries)%s");
        if (q[i].num_tokens < 0 || q[i].text_len < 0 || q[i].num_fusion_tokens < 0) return fail(INFX_EINVAL, "negative count in a coverage query%s");
        for (int32_t t = 0; t < q[i].num_tokens; t++) if ((int32_t)q[i].tok_off[t] + (int32_t)q[i].tok_len[t] > q[i].text_len) return fail(INFX_EINVAL, "coverage query: a token lies outside the query text%s");
        for (int32_t t = 0; t < q[i].num_fusion_tokens; t++) if ((int32_t)q[i].ftok_off[t] + (int32_t)q[i].ftok_len[t] > q[i].text_len) return fail(INFX_EINVAL, "coverage query: a fusion token lies outside the query text%s");
    }
    GROW(s->dCovQ, s->capCovQ, (size_t)nq * sizeof(infx_cov_query));
    GROW(s->dCovC, s->capCovC, (size_t)ncand * sizeof(infx_cov_cand));
    GROW(s->dCovO, s->capCovO, (size_t)ncand * sizeof(infx_cov_out));
    if (feat_out) GROW(s->dCovF, s->capCovF, (size_t)ncand * INFX_NFEAT * 4);
    UP(s->dCovQ, q, (size_t)nq * sizeof(infx_cov_query));
    s->batchAlias = s->longAlias;
    for (uint32_t i = 0; i < nq && !s->batchAlias; i++) if (q[i].reserved == 0) for (int32_t k = 0; k < q[i].text_len && k < (int32_t)INFX_MAX_QUERY_CHARS; k++) if (s2_host_is_alias(q[i].text[k])) { s->batchAlias = true; break; }
    UP(s->dCovC, cand, (size_t)ncand * sizeof(infx_cov_cand));
    HIPCHK(hipEventRecord(s->evC0, s->st));
    S2_LAUNCH_FAST(dev_index(s), (const infx_cov_query*)s->dCovQ, nq,
                                                                                 (const infx_cov_cand*)s->dCovC, ncand, (infx_cov_out*)s->dCovO, feat_out ? (int32_t*)s->dCovF : nullptr, 0, 0, nullptr);
    S2_LAUNCH_SLOW(dev_index(s), (const infx_cov_query*)s->dCovQ, nq,
                                                                                 (const infx_cov_cand*)s->dCovC, ncand, (infx_cov_out*)s->dCovO, feat_out ? (int32_t*)s->dCovF : nullptr, 0, 1, nullptr);
    { int32_t rc_ = s2_huge_ready(s); if (rc_) return rc_; }
    S2_LAUNCH_HUGE(dev_index(s), (const infx_cov_query*)s->dCovQ, nq,
                                                                                 (const infx_cov_cand*)s->dCovC, ncand, (infx_cov_out*)s->dCovO, feat_out ? (int32_t*)s->dCovF : nullptr, 0, 1, nullptr);
    S2_LAUNCH_LONGQ(dev_index(s), (const infx_cov_query*)s->dCovQ, nq,
                                                                                 (const infx_cov_cand*)s->dCovC, ncand, (infx_cov_out*)s->dCovO, feat_out ? (int32_t*)s->dCovF : nullptr, 0, 1, nullptr);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(s->evC1, s->st));
    s->timedCov = true;
    DOWN(out, s->dCovO, (size_t)ncand * sizeof(infx_cov_out));
    if (feat_out) DOWN(feat_out, s->dCovF, (size_t)ncand * INFX_NFEAT * 4);
    SYNC();
    return INFX_OK;
}

int32_t infx_upload_wordmatcher(infx_index* ix, uint64_t n_exact, const int32_t* exact_docs, uint64_t n_ld1, const int32_t* ld1_docs) {
    if (!ix || (n_exact && !exact_docs) || (n_ld1 && !ld1_docs)) return fail(INFX_EINVAL, "null argument%s");
    HIPCHK(enter_device(ix->cfg.device));
    int32_t *dE = nullptr, *dL = nullptr;
    HIPCHK(dalloc(ix, &dE, (size_t)n_exact + 1)); HIPCHK(dalloc(ix, &dL, (size_t)n_ld1 + 1));
    if (n_exact) HIPCHK(hipMemcpy(dE, exact_docs, (size_t)n_exact * 4, hipMemcpyHostToDevice));
    if (n_ld1) HIPCHK(hipMemcpy(dL, ld1_docs, (size_t)n_ld1 * 4, hipMemcpyHostToDevice));
    ix->d.wmExact = dE; ix->d.wmLd1 = dL; ix->nWmExact = n_exact; ix->nWmLd1 = n_ld1; ix->haveWm = true;
    return INFX_OK;
}


// ---- dictionaries of the device-side planning lookups (lookup.hip.inc) --------------------------------------------------------------
static int32_t dict_upload(infx_index* ix, DevDict& D, uint32_t nkeys, const uint32_t* key_offs, const uint16_t* chars, const uint64_t* list_offs, uint64_t ndocs) {
    D = DevDict{};
    if (nkeys == 0) return INFX_OK;
    for (uint32_t i = 0; i < nkeys; i++) if (key_offs[i + 1] < key_offs[i] || list_offs[i + 1] < list_offs[i]) return fail(INFX_EINVAL, "dictionary offsets must ascend%s");
    if (list_offs[nkeys] > ndocs) return fail(INFX_EINVAL, "dictionary list offsets exceed the uploaded doc-id array%s");
    { int32_t rc_ = dcopy(ix, &D.keyOff, key_offs, (size_t)nkeys + 1); if (rc_) return rc_; }
    { int32_t rc_ = dcopy(ix, &D.chars, chars, (size_t)key_offs[nkeys]); if (rc_) return rc_; }
    { int32_t rc_ = dcopy(ix, &D.listOff, list_offs, (size_t)nkeys + 1); if (rc_) return rc_; }
    uint64_t cap = 1024; while (cap < (uint64_t)nkeys * 2) cap <<= 1;
    if (cap > 0x80000000ull) return fail(INFX_ECAPACITY, "dictionary too large%s");
    unsigned long long* slots = nullptr;
    HIPCHK(dalloc(ix, &slots, (size_t)cap));
    HIPCHK(hipMemset(slots, 0, (size_t)cap * 8));
    k_dict_build<<<(nkeys + 255) / 256, 256>>>(slots, (uint32_t)(cap - 1), D.keyOff, D.chars, nkeys);
    HIPCHK(hipGetLastError()); HIPCHK(hipDeviceSynchronize());
    D.slots = slots; D.mask = (uint32_t)(cap - 1);
    return INFX_OK;
}
int32_t infx_upload_wm_dictionary(infx_index* ix, uint32_t n_exact, const uint32_t* exact_key_offs, const uint16_t* exact_chars, const uint64_t* exact_list_offs,
                                  uint32_t n_ld1, const uint32_t* ld1_key_offs, const uint16_t* ld1_chars, const uint64_t* ld1_list_offs,
                                  uint32_t n_words, const uint32_t* word_offs, const uint16_t* word_chars, const int32_t* word_last_doc,
                                  uint32_t n_affix, const uint32_t* affix_fwd, const uint32_t* affix_rev, int32_t min_ld1, int32_t max_ld1) {
    if (!ix || (n_exact && (!exact_key_offs || !exact_chars || !exact_list_offs)) || (n_ld1 && (!ld1_key_offs || !ld1_chars || !ld1_list_offs)) ||
        (n_words && (!word_offs || !word_chars || !word_last_doc)) || (n_affix && (!affix_fwd || !affix_rev))) return fail(INFX_EINVAL, "null argument%s");
    if (!ix->haveWm) return fail(INFX_EINVAL, "infx_upload_wordmatcher comes first%s");
    if (ix->haveDict) return fail(INFX_EINVAL, "WordMatcher dictionary already uploaded%s");
    if (min_ld1 < 1 || max_ld1 < min_ld1 || 3 + 2 * max_ld1 > INFX_MAX_WM_LISTS) return fail(INFX_EINVAL, "bad LD1 word-length window%s");
    for (uint32_t i = 0; i < n_affix; i++) if (affix_fwd[i] >= n_words || affix_rev[i] >= n_words) return fail(INFX_EINVAL, "affix word id out of range%s");
    HIPCHK(enter_device(ix->cfg.device));
    if (!ix->lk) ix->lk = new DevLookup{};
    DevLookup& K = *ix->lk;
    { int32_t rc_ = dict_upload(ix, K.exact, n_exact, exact_key_offs, exact_chars, exact_list_offs, ix->nWmExact); if (rc_) return rc_; }
    { int32_t rc_ = dict_upload(ix, K.ld1, n_ld1, ld1_key_offs, ld1_chars, ld1_list_offs, ix->nWmLd1); if (rc_) return rc_; }
    if (n_words) {
        { int32_t rc_ = dcopy(ix, &K.wordOff, word_offs, (size_t)n_words + 1); if (rc_) return rc_; }
        { int32_t rc_ = dcopy(ix, &K.wordChars, word_chars, (size_t)word_offs[n_words]); if (rc_) return rc_; }
        { int32_t rc_ = dcopy(ix, &K.wordLastDoc, word_last_doc, (size_t)n_words); if (rc_) return rc_; }
    }
    if (n_affix) {
        { int32_t rc_ = dcopy(ix, &K.affixFwd, affix_fwd, (size_t)n_affix); if (rc_) return rc_; }
        { int32_t rc_ = dcopy(ix, &K.affixRev, affix_rev, (size_t)n_affix); if (rc_) return rc_; }
    }
    K.nAffix = n_affix; K.minLd1 = min_ld1; K.maxLd1 = max_ld1;
    ix->haveDict = true;
    return INFX_OK;
}
int32_t infx_upload_term_trie(infx_index* ix, uint32_t n_nodes, const uint32_t* edge_start, const uint16_t* edge_label, const uint32_t* edge_child, const int32_t* node_term,
                              uint32_t n_terms, const uint32_t* sorted_terms) {
    if (!ix || !n_nodes || !edge_start || !node_term || (n_terms && !sorted_terms)) return fail(INFX_EINVAL, "null argument%s");
    if (ix->haveTrie) return fail(INFX_EINVAL, "term trie already uploaded%s");
    const uint32_t ne = edge_start[n_nodes];
    if (ne && (!edge_label || !edge_child)) return fail(INFX_EINVAL, "null argument%s");
    for (uint32_t v = 0; v < n_nodes; v++) { if (edge_start[v + 1] < edge_start[v]) return fail(INFX_EINVAL, "edge offsets must ascend%s"); if (node_term[v] >= (int32_t)n_terms) return fail(INFX_EINVAL, "node term id out of range%s"); }
    for (uint32_t k = 0; k < ne; k++) if (edge_child[k] >= n_nodes) return fail(INFX_EINVAL, "edge child out of range%s");
    std::vector<uint32_t> rank(n_terms, 0xFFFFFFFFu);
    for (uint32_t i = 0; i < n_terms; i++) { if (sorted_terms[i] >= n_terms || rank[sorted_terms[i]] != 0xFFFFFFFFu) return fail(INFX_EINVAL, "sorted_terms is not a permutation%s"); rank[sorted_terms[i]] = i; }
    HIPCHK(enter_device(ix->cfg.device));
    if (!ix->lk) ix->lk = new DevLookup{};
    DevLookup& K = *ix->lk;
    { int32_t rc_ = dcopy(ix, &K.rEdgeStart, edge_start, (size_t)n_nodes + 1); if (rc_) return rc_; }
    { int32_t rc_ = dcopy(ix, &K.rEdgeLabel, edge_label, (size_t)ne); if (rc_) return rc_; }
    { int32_t rc_ = dcopy(ix, &K.rEdgeChild, edge_child, (size_t)ne); if (rc_) return rc_; }
    { int32_t rc_ = dcopy(ix, &K.rTerm, node_term, (size_t)n_nodes); if (rc_) return rc_; }
    { int32_t rc_ = dcopy(ix, &K.termRank, (const uint32_t*)rank.data(), (size_t)n_terms); if (rc_) return rc_; }
    { int32_t rc_ = dcopy(ix, &K.sortedTerms, sorted_terms, (size_t)n_terms); if (rc_) return rc_; }
    K.nTerms = n_terms; K.nNodes = n_nodes;
    ix->haveTrie = true;
    return INFX_OK;
}
int32_t infx_ld1_expand(infx_stream* s, uint32_t nwords, const uint32_t* word_offs, const uint16_t* chars, uint32_t cap, int32_t* members_out, uint32_t* counts_out, uint32_t* status_out) {
    if (!s || (nwords && (!word_offs || !members_out || !counts_out || !status_out || (word_offs[nwords] && !chars))) || cap == 0) return fail(INFX_EINVAL, "null argument%s");
    if (nwords == 0) return INFX_OK;
    infx_index* ix = s->ix;
    if (!ix->haveTrie) return fail(INFX_EINVAL, "infx_upload_term_trie has not been called%s");
    HIPCHK(enter_device(ix->cfg.device));
    { int32_t rc_ = pin_reset(s); if (rc_) return rc_; }
    PlanStream plan(s);
    const size_t nch = word_offs[nwords];
    GROW(s->dLWordOff, s->capLWordOff, ((size_t)nwords + 1) * 4);
    GROW(s->dLChars, s->capLChars, std::max<size_t>(1, nch) * 2);
    GROW(s->dLMembers, s->capLMembers, (size_t)nwords * cap * 4);
    GROW(s->dLCount, s->capLCount, (size_t)nwords * 8);
    UP(s->dLWordOff, word_offs, ((size_t)nwords + 1) * 4);
    UP(s->dLChars, chars, nch * 2);
    uint32_t* dCnt = (uint32_t*)s->dLCount; uint32_t* dSt = dCnt + nwords;
    k_ld1<<<nwords, WAVE, 0, s->st>>>(*ix->lk, (const uint32_t*)s->dLWordOff, (const uint16_t*)s->dLChars, nwords, cap, (int32_t*)s->dLMembers, dCnt, dSt, nullptr, nullptr, 0u);
    HIPCHK(hipGetLastError());
    DOWN(counts_out, dCnt, (size_t)nwords * 4);
    DOWN(status_out, dSt, (size_t)nwords * 4);
    SYNC();
    // only the members that exist travel back: one copy per word of min(count, cap) ids (a few hundred bytes each) would be many small DMAs, so
    // the rows are fetched in one strided pass up to the largest count of the batch
    uint32_t mx = 0; for (uint32_t i = 0; i < nwords; i++) if (!status_out[i]) mx = std::max(mx, std::min(counts_out[i], cap));
    if (mx) {
        void* p = pin_take(s, (size_t)nwords * mx * 4); if (!p) return fail(INFX_ENOMEM, "hipHostMalloc staging failed%s");
        HIPCHK(hipMemcpy2DAsync(p, (size_t)mx * 4, s->dLMembers, (size_t)cap * 4, (size_t)mx * 4, nwords, hipMemcpyDeviceToHost, s->st)); s->unsynced = true;
        SYNC();
        for (uint32_t i = 0; i < nwords; i++) { const uint32_t c = status_out[i] ? 0u : std::min(counts_out[i], cap); std::memcpy(members_out + (size_t)i * cap, (const int32_t*)p + (size_t)i * mx, (size_t)c * 4); }
    }
    return INFX_OK;
}

static std::string post_rows_text(const infx_index* ix) { return ix->postRows == INFX_FILTER_MAX_ROWS ? "INFX_FILTER_MAX_ROWS (64)" : std::to_string(ix->postRows); }
static uint32_t pow2_at_least(uint32_t v, uint32_t lo) { uint32_t p = lo; while (p < v) p <<= 1; return p; }

// ---- fused pipeline pieces (shared by infx_search_fused and the sharded stage API) ------------------------------------------
static uint32_t wm_words(const infx_cov_query& c) {      // words k_wm looks up: fusion tokens of at least two characters (WordMatcherLookup.cs:27-31)
    uint32_t n = 0; const int nt = std::min(c.num_fusion_tokens, 2 * INFX_MAX_QUERY_TOKENS);
    for (int t = 0; t < nt; t++) if (c.ftok_len[t] >= 2 && (int)c.ftok_off[t] + (int)c.ftok_len[t] <= c.text_len) n++;
    return n;
}
static int32_t fused_check_queries(infx_index* ix, uint32_t nd, uint32_t nq, const infx_fused_query* fq, const infx_cov_query* cq,
                                   uint32_t nlists, const infx_wm_list* lists, uint32_t owned_n, int32_t depth, int32_t max_results, uint32_t nLong) {
    if (nd > nq || max_results < 1 || depth < 1 || depth > ix->cfg.max_depth) return fail(INFX_EINVAL, "bad batch shape%s");
    bool anyWm = false;
    for (uint32_t i = 0; i < nq; i++) {
        if (fq[i].dev >= (int32_t)nd) return fail(INFX_EINVAL, "fused query refers to a missing Stage-1 query%s");
        if (fq[i].wm_count > INFX_MAX_WM_LISTS || (uint64_t)fq[i].wm_off + fq[i].wm_count > nlists) return fail(INFX_ECAPACITY, "too many WordMatcher lists for one query%s");
        if (fq[i].wm_count) anyWm = true;
        if (fq[i].flags & INFX_FQ_BROWSE) {
            if (!(fq[i].flags & INFX_FQ_SKIP) || (fq[i].flags & INFX_FQ_UNSUPPORTED)) return fail(INFX_EINVAL, "INFX_FQ_BROWSE goes with INFX_FQ_SKIP: a browse query has no text%s");
            if (fq[i].max_results > (int32_t)ix->postRows) return fail(INFX_EUNSUPPORTED, "a browse query returns at most %s rows (its facets run on them; infx_set_post_rows)", post_rows_text(ix).c_str());
        }
        if (fq[i].flags & INFX_FQ_WMDEV) {
            if (!ix->haveDict) return fail(INFX_EINVAL, "INFX_FQ_WMDEV needs infx_upload_wm_dictionary%s");
            if (fq[i].wm_count) return fail(INFX_EINVAL, "a query takes its WordMatcher lists either from the caller or from the device lookup%s");
            if ((fq[i].flags & INFX_FQ_COV) && !(fq[i].flags & INFX_FQ_SKIP) && wm_words(cq[i]) * (uint32_t)(3 + 2 * ix->lk->maxLd1) > INFX_MAX_WM_LISTS)
                return fail(INFX_ECAPACITY, "too many words for the device WordMatcher lookup (hand the lists over instead)%s");
        }
        if ((fq[i].flags & INFX_FQ_COV) && !(fq[i].flags & INFX_FQ_SKIP) && cq[i].reserved != 0) {
            if (cq[i].reserved < 0 || (uint32_t)cq[i].reserved > nLong) return fail(INFX_EINVAL, "query refers to a missing long-query record (infx_stage2_long_queries)%s");
            if (fq[i].flags & INFX_FQ_WMDEV) return fail(INFX_EINVAL, "the device WordMatcher lookup reads the words of a fast-envelope query: hand the lists of a long query over%s");
        } else if ((fq[i].flags & INFX_FQ_COV) && !(fq[i].flags & INFX_FQ_SKIP) &&
            (cq[i].num_tokens > INFX_MAX_QUERY_TOKENS || cq[i].text_len > INFX_MAX_QUERY_CHARS || cq[i].num_fusion_tokens > 2 * INFX_MAX_QUERY_TOKENS))
            return fail(INFX_EUNSUPPORTED, "query exceeds the Stage-2 envelope (hand it over as a long query: infx_stage2_long_queries)%s");
    }
    for (uint32_t l = 0; l < nlists; l++) {
        const infx_wm_list& L = lists[l];
        const uint64_t lim = L.src == 0 ? ix->nWmExact : (L.src == 1 ? ix->nWmLd1 : (L.src == 2 ? owned_n : 0));
        if (L.off + L.len > lim) return fail(INFX_EINVAL, "WordMatcher list out of range%s");
    }
    if (anyWm && !ix->haveWm) return fail(INFX_EINVAL, "infx_upload_wordmatcher has not been called%s");
    return INFX_OK;
}

// k_rules (from the class histogram in s->dCounts) + k_select -> s->dHits / s->dHitCount (stride = depth)
static int32_t fused_enqueue_select(infx_stream* s, uint32_t nd, int32_t depth, bool shardNext = false, bool markTurn = false) {
    infx_index* ix = s->ix;
    GROW(s->dRules, s->capRules, std::max<size_t>(1, nd) * sizeof(SelRule));
    GROW(s->dHits, s->capHits, std::max<size_t>(1, (size_t)nd) * depth * sizeof(infx_hit));
    GROW(s->dHitCount, s->capHitCount, std::max<size_t>(1, nd) * 4);
    GROW(s->dFQueries, s->capFQueries, std::max<size_t>(1, nd) * sizeof(infx_query));
    UP(s->dFQueries, s->lastQ.data(), (size_t)nd * sizeof(infx_query));
    HIPCHK(hipMemsetAsync(s->dHitCount, 0, std::max<size_t>(1, nd) * 4, s->st));
    Arena ar = make_arena(s);
    HIPCHK(hipEventRecord(s->evS0, s->st));
    if (nd) {
        k_rules<<<(nd + 255) / 256, 256, 0, s->st>>>((const infx_query*)s->dFQueries, (const uint32_t*)s->dCounts, (SelRule*)s->dRules, nd);
        const bool exact = !shardNext && exact_possible(s);
        if (exact) HIPCHK(hipMemsetAsync(s->dExactStat + 4, 0, 16, s->st));
        if (shardNext) GROW(s->dNext, s->capNext, (size_t)nd * 4);       // document shards: no local flags — the cut is global (k_gflag)
#ifdef SEL_PROF
        static unsigned long long* dProf = nullptr; static int profCalls = 0;
        if (getenv("INFX_SEL_PROF") && nd >= 500) { if (!dProf) { hipMalloc((void**)&dProf, 4096 * 64); hipMemcpyToSymbol(HIP_SYMBOL(g_selProf), &dProf, sizeof(dProf)); } hipMemsetAsync(dProf, 0, (size_t)nd * 64, s->st); }
#endif
        const uint32_t* selOrd = select_order(s, nd);
        const SelGiant selG = select_giants(s, ar, nd, selOrd);
        k_select<<<nd, SEL_THREADS, 0, s->st>>>(ar, ix->d.nRanges, (const SelRule*)s->dRules, (infx_hit*)s->dHits, (uint32_t*)s->dHitCount, depth, exact ? (uint32_t*)s->dExactFlag : nullptr, exact ? s->dExactStat + 4 : nullptr,
                                                shardNext ? (float*)s->dNext : nullptr, selOrd, selG);
#ifdef SEL_PROF
        if (dProf && nd >= 500 && ++profCalls == 6) { static const char* const ph[5] = {"hist1", "hist2", "gather", "sort", "write"}; wgprof_dump("selprof", dProf, nd, ph, s->st); }
#endif
        if (markTurn) { HIPCHK(hipEventRecord(s->evTurn, s->st)); markTurn = false; }      // the wide phase of this batch ends here (round 6 measured the event in FRONT of k_select — the next batch's accumulation beside this k_select's tail of giant queries: 93.7 / 94.2 k against 93.8 / 94.3 k queries/s, nothing)
        if (exact) { int32_t rc_ = mark_wide_queries(s, ix->cfg.max_depth); if (rc_) return rc_; }
        if (exact) { int32_t rc_ = enqueue_exact(s, nd, depth); if (rc_) return rc_; }
    }
    if (markTurn) HIPCHK(hipEventRecord(s->evTurn, s->st));
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(s->evS1, s->st));
    s->timedSel = true;
    return INFX_OK;
}

// uploads the per-query tables, then k_prep2 (merging W per-shard hit lists) + k_stage2 -> s->dCovC / s->dCovO / s->dFMeta / s->dFS1
static int32_t fused_enqueue_prep_stage2(infx_stream* s, int W, uint32_t nd, const infx_hit* dHitsAll, const uint32_t* dHcAll,
                                         uint32_t nq, const infx_fused_query* fq, const infx_cov_query* cq, uint32_t nlists, const infx_wm_list* lists,
                                         uint32_t owned_n, const int32_t* owned, int32_t depth, int32_t want_debug) {
    infx_index* ix = s->ix;
    const uint32_t stride = 2u * (uint32_t)depth, ncand = nq * stride;
    const uint32_t Dp = pow2_at_least((uint32_t)depth, 8);
    const uint32_t Dall = W > 1 ? pow2_at_least((uint32_t)W * (uint32_t)depth, 8) : 0;
    if (Dall > 8192) return fail(INFX_ECAPACITY, "shards x depth exceeds the in-LDS merge (8192 rows); merge hierarchically%s");
    s->browseQ.clear();
    for (uint32_t i = 0; i < nq; i++) if (fq[i].flags & INFX_FQ_BROWSE) s->browseQ.push_back({i, (uint32_t)std::max(fq[i].max_results, 0)});
    s->qpRows.clear();       // the rows each query asks for: the finalize decides with them which queries the wide post-processing kernels take
    if (ix->postRows > INFX_FILTER_MAX_ROWS) { s->qpRows.resize(nq); for (uint32_t i = 0; i < nq; i++) s->qpRows[i] = fq[i].max_results; }
    GROW(s->dFQ, s->capFQ, (size_t)nq * sizeof(infx_fused_query));
    GROW(s->dFLists, s->capFLists, std::max<size_t>(1, nlists) * sizeof(infx_wm_list));
    GROW(s->dFOwned, s->capFOwned, ((size_t)owned_n + 1) * 4);
    GROW(s->dFS1, s->capFS1, (size_t)nq * depth * sizeof(infx_hit));
    GROW(s->dFMeta, s->capFMeta, (size_t)nq * sizeof(FusedMeta));
    GROW(s->dCovQ, s->capCovQ, (size_t)nq * sizeof(infx_cov_query));
    GROW(s->dCovC, s->capCovC, (size_t)ncand * sizeof(infx_cov_cand));
    GROW(s->dCovO, s->capCovO, (size_t)ncand * sizeof(infx_cov_out));
    GROW(s->dFPairs, s->capFPairs, (size_t)ncand * 4);
    if (want_debug) GROW(s->dCovF, s->capCovF, (size_t)ncand * INFX_NFEAT * 4);
    // queries flagged INFX_FQ_WMDEV get their WordMatcher lists from k_wm: a block of INFX_MAX_WM_LISTS descriptors per query behind the caller's lists,
    // one WM_AFFIX_CAP region of `owned` per looked-up word behind the caller's ids (the regions are assigned here: `reserved` = first word slot)
    std::vector<infx_fused_query> fqDev; uint64_t wmSlots = 0;
    for (uint32_t i = 0; i < nq; i++) if (fq[i].flags & INFX_FQ_WMDEV) {
        if (fqDev.empty()) fqDev.assign(fq, fq + nq);
        fqDev[i].reserved = (int32_t)wmSlots;
        if ((fq[i].flags & INFX_FQ_COV) && !(fq[i].flags & INFX_FQ_SKIP)) wmSlots += wm_words(cq[i]);
    }
    const bool wmDev = !fqDev.empty();
    if (wmDev) {
        if (wmSlots * WM_AFFIX_CAP + owned_n > 0x7FFFFFF0ull) return fail(INFX_ECAPACITY, "device WordMatcher lookup: too many query words in one batch%s");
        GROW(s->dFLists, s->capFLists, ((size_t)nlists + (size_t)nq * INFX_MAX_WM_LISTS) * sizeof(infx_wm_list));
        GROW(s->dFOwned, s->capFOwned, ((size_t)owned_n + (size_t)wmSlots * WM_AFFIX_CAP + 1) * 4);
    }
    UP(s->dFQ, wmDev ? fqDev.data() : fq, (size_t)nq * sizeof(infx_fused_query));
    UP(s->dFLists, lists, (size_t)nlists * sizeof(infx_wm_list));
    UP(s->dFOwned, owned, (size_t)owned_n * 4);
    UP(s->dCovQ, cq, (size_t)nq * sizeof(infx_cov_query));
    s->batchAlias = s->longAlias;      // (host scan of the query texts: ~20 characters per query)
    for (uint32_t i = 0; i < nq && !s->batchAlias; i++) if (cq[i].reserved == 0) for (int32_t k = 0; k < cq[i].text_len && k < (int32_t)INFX_MAX_QUERY_CHARS; k++) if (s2_host_is_alias(cq[i].text[k])) { s->batchAlias = true; break; }
    HIPCHK(hipMemsetAsync(s->dCovO, 0, (size_t)ncand * sizeof(infx_cov_out), s->st));
    HIPCHK(hipEventRecord(s->evP0, s->st));
    if (wmDev) {
        DevLookup lk = *ix->lk; if (s->csOn && !s->cs.cover_prefix_suffix) lk.nAffix = 0;      // !CoverPrefixSuffix: no LookupAffix (WordMatcherLookup.cs:51) -> no source-2 lists
        k_wm<<<nq, WAVE, 0, s->st>>>(lk, (infx_fused_query*)s->dFQ, (const infx_cov_query*)s->dCovQ, nq, (infx_wm_list*)s->dFLists, nlists, (int32_t*)s->dFOwned, (uint64_t)owned_n);
        HIPCHK(hipGetLastError());
    }
    {
        const size_t Pp = std::max<size_t>(Dp, P2_CAP);
        const size_t lds = (size_t)Dp * 4 * 4 + Pp * 4 + (size_t)P2_CAP * 4 + (size_t)Dp * 8 + (size_t)Dp * 2 + Pp + (size_t)P2_MAXLISTS * (8 + 4 + 4 + 4) + (P2_THREADS + 2) * 4 + (size_t)Dall * 8 + 64;
        if (lds > 64 * 1024) HIPCHK(hipFuncSetAttribute((const void*)k_prep2, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
#ifdef SEL_PROF
        static unsigned long long* dP2 = nullptr; static int p2Calls = 0;
        if (getenv("INFX_SEL_PROF") && nq >= 500) { if (!dP2) { hipMalloc((void**)&dP2, 4096 * 64); hipMemcpyToSymbol(HIP_SYMBOL(g_p2Prof), &dP2, sizeof(dP2)); } hipMemsetAsync(dP2, 0, (size_t)nq * 64, s->st); }
#endif
        k_prep2<<<nq, P2_THREADS, lds, s->st>>>(dev_index(s), dHitsAll, dHcAll, depth, W, (int)nd, (int)Dall, (const infx_fused_query*)s->dFQ,
                                                 (const infx_wm_list*)s->dFLists, (const int32_t*)s->dFOwned, depth, (int)Dp,
                                                 (infx_hit*)s->dFS1, (infx_cov_cand*)s->dCovC, (int32_t*)s->dFPairs, (FusedMeta*)s->dFMeta);
#ifdef SEL_PROF
        if (dP2 && nq >= 500 && ++p2Calls == 6) { static const char* const ph[5] = {"s1sort", "topsort", "overlap", "wmrounds", "emit"}; wgprof_dump("p2prof", dP2, nq, ph, s->st); }
#endif
    }
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(s->evP1, s->st));
    HIPCHK(hipEventRecord(s->evC0, s->st));
    if (s->hlOn) {      // Query.highlight: what k_highlight needs of this Stage-2 call after it has consumed its settings — them, the alias flag, each query's word count
        s->hlCs = S2_CS ? s->cs : S2_DEFAULT_SETUP; s->hlAlias = S2_AL;
        s->hlWords.resize(nq); for (uint32_t i = 0; i < nq; i++) s->hlWords[i] = cq[i].reserved != 0 ? -1 : std::min(std::max(cq[i].num_tokens, 0), (int32_t)INFX_MAX_QUERY_TOKENS);
    }
    S2_LAUNCH_FAST(dev_index(s), (const infx_cov_query*)s->dCovQ, nq, (const infx_cov_cand*)s->dCovC, ncand,
                                                                                 (infx_cov_out*)s->dCovO, want_debug ? (int32_t*)s->dCovF : nullptr, 1, 0, (const int32_t*)s->dFPairs);
    S2_LAUNCH_SLOW(dev_index(s), (const infx_cov_query*)s->dCovQ, nq, (const infx_cov_cand*)s->dCovC, ncand,
                                                                                 (infx_cov_out*)s->dCovO, want_debug ? (int32_t*)s->dCovF : nullptr, 1, 1, (const int32_t*)s->dFPairs);
    { int32_t rc_ = s2_huge_ready(s); if (rc_) return rc_; }
    S2_LAUNCH_HUGE(dev_index(s), (const infx_cov_query*)s->dCovQ, nq, (const infx_cov_cand*)s->dCovC, ncand,
                                                                                 (infx_cov_out*)s->dCovO, want_debug ? (int32_t*)s->dCovF : nullptr, 1, 1, (const int32_t*)s->dFPairs);
    S2_LAUNCH_LONGQ(dev_index(s), (const infx_cov_query*)s->dCovQ, nq, (const infx_cov_cand*)s->dCovC, ncand,
                                                                                 (infx_cov_out*)s->dCovO, want_debug ? (int32_t*)s->dCovF : nullptr, 1, 1, (const int32_t*)s->dFPairs);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(s->evC1, s->st));
    s->timedCov = true;
    s->fusedNq = nq; s->fusedDepth = depth; s->fusedDebug = want_debug != 0;
    return INFX_OK;
}

// k_filter_count_multi over documents [docBase, docBase + n): counts[k] = the documents programs dProgs[k] accept, K programs in
// ceil(K / FCM_MAXK) launches (FCM_MAXK bounds the per-workgroup LDS counters)
#define FCM_MAXK 4096u
#define FCM_MAXGRID 2048
static int32_t count_enqueue(infx_stream* s, const DevFilter* dProgs, uint32_t K, const DevCountCols& cc, int32_t docBase, int32_t n, uint32_t* dCounts) {
    infx_index* ix = s->ix;
    { int32_t rc_ = columns_cover(ix, (int64_t)docBase + std::max(n, 0), COLS_COVER_COUNTED); if (rc_) return rc_; }
    HIPCHK(hipMemsetAsync(dCounts, 0, (size_t)K * 4, s->st));
    s->lastCountK = K; s->lastCountLaunches = 0;
    if (n <= 0 || !K) return INFX_OK;
    const DevColumns cols = dev_columns(ix);
    const int grid = (int)std::min<int64_t>(FCM_MAXGRID, ((int64_t)n + FCM_THREADS - 1) / FCM_THREADS);
    for (uint32_t k0 = 0; k0 < K; k0 += FCM_MAXK) {
        const uint32_t k = std::min(FCM_MAXK, K - k0);
        const size_t lds = ((size_t)k + (size_t)cc.nUsed * FCM_THREADS) * 4;
        HIPCHK(lds_limit((const void*)k_filter_count_multi, ix->cfg.device, lds));
        k_filter_count_multi<<<grid, FCM_THREADS, lds, s->st>>>(dProgs + k0, k, cc, cols, docBase, n, ix->d.deleted, dCounts + k0);
        HIPCHK(hipGetLastError());
        s->lastCountLaunches++;
    }
    return INFX_OK;
}

// ---- pre-filter masks (k_filter_mask_multi) ----
static int mask_slot_of(const infx_stream* s, const uint8_t* p) { for (int i = 0; i < INFX_MAX_PREFILTERS; i++) if (p && s->dMask[i] == p) return i; return -1; }
static inline size_t mask_bytes(const infx_index* ix) { return (((size_t)std::max(ix->d.totalDocs, 0) + 3) & ~(size_t)3) + 4; }
// enqueues the staged build on s->st: the programs' blob, one launch over the whole corpus, the counts' way back (they land at the next stream_sync)
static int32_t mask_flush(infx_stream* s) {
    if (!s->mkStaged) return INFX_OK;
    s->mkStaged = false;
    infx_index* ix = s->ix;
    const uint32_t K = s->mkTable.size();
    const int32_t n = ix->d.totalDocs;
    s->lastMaskBuilt = K; s->lastMaskLaunches = 0;
    if (!K) return INFX_OK;
    { int32_t rc_ = columns_cover(ix, n, COLS_COVER_CORPUS); if (rc_) return rc_; }
    for (uint32_t k = 0; k < K; k++) {      // the kernel stores whole dwords up to the padded size
        const int slot = mask_slot_of(s, s->mkOut.mask[k]);
        if (slot < 0 || s->capMask[slot] < mask_bytes(ix)) return fail(INFX_EINVAL, "a mask buffer is not a mask slot of this stream, or was made for a smaller corpus%s");
    }
    { int32_t rc_ = table_upload(s, s->mkTable, &s->dMaskBlob, &s->capMaskBlob); if (rc_) return rc_; }
    GROW(s->dMaskCnt, s->capMaskCnt, (size_t)INFX_MAX_PREFILTERS * 4);
    HIPCHK(hipMemsetAsync(s->dMaskCnt, 0, (size_t)K * 4, s->st));
    if (n > 0) {
        const DevColumns cols = dev_columns(ix);
        const DevCountCols cc = s->mkTable.columns(0, K);
        // 256 threads while four workgroups' LDS fit a CU (40 KiB each), else one wave per workgroup (64 columns: 64 KiB)
        const int threads = ((size_t)cc.nUsed * 4 * FMM_THREADS + K) * 4 <= 40 * 1024 ? FMM_THREADS : WAVE;
        const size_t lds = ((size_t)cc.nUsed * 4 * threads + K) * 4;
        const int64_t groups = ((int64_t)n + 3) / 4;
        const int grid = (int)std::min<int64_t>(FCM_MAXGRID, (groups + threads - 1) / threads);
        HIPCHK(lds_limit((const void*)k_filter_mask_multi, ix->cfg.device, lds));
        k_filter_mask_multi<<<grid, threads, lds, s->st>>>((const DevFilter*)s->dMaskBlob, K, cc, cols, n, ix->d.deleted, s->mkOut, (uint32_t*)s->dMaskCnt);
        HIPCHK(hipGetLastError());
        s->lastMaskLaunches = 1;
    }
    if (s->mkCountsOut) DOWN(s->mkCountsOut, s->dMaskCnt, (size_t)K * 4);
    return INFX_OK;
}
// the flags table of the batch being enqueued: DevIndex::qDeleted of its launches (dev_index).  Only for a batch with a pre-filtered query.
static int32_t stage_doc_masks(infx_stream* s, uint32_t nd, uint32_t nq, const infx_fused_query* fq) {
    s->qDelOn = false;
    bool any = false; for (auto m : s->docMasks) any = any || m != nullptr;
    if (!any) return INFX_OK;
    infx_index* ix = s->ix;
    std::vector<const uint8_t*> tbl((size_t)nd + nq, ix->d.deleted); std::vector<uint8_t> set(nd, 0);
    for (uint32_t i = 0; i < nq; i++) {
        const uint8_t* m = s->docMasks[i] ? s->docMasks[i] : ix->d.deleted;
        if (s->docMasks[i]) { const int slot = mask_slot_of(s, m); if (slot < 0 || s->capMask[slot] < mask_bytes(ix)) return fail(INFX_EINVAL, "a document mask is not a mask slot of this stream, or was made for a smaller corpus%s"); }
        tbl[(size_t)nd + i] = m;
        const int32_t d = fq[i].dev;
        if (d < 0 || (uint32_t)d >= nd) continue;
        if (set[d] && tbl[d] != m) return fail(INFX_EINVAL, "two queries with different document masks share one Stage-1 query%s");
        tbl[d] = m; set[d] = 1;
    }
    GROW(s->dQDel, s->capQDel, tbl.size() * sizeof(const uint8_t*));
    UP(s->dQDel, tbl.data(), tbl.size() * sizeof(const uint8_t*));
    s->qDelOn = true;
    return INFX_OK;
}

// The batch's browse queries (s->browseQ; browse.hip.inc): grouped by filter program, all groups answered by one ordered scan of the corpus, which
// also counts the ncount programs whose NumberOfDocumentsInFilter the batch needs (into s->dQCount — k_filter_count_multi is not launched for such a
// batch).  T: the batch's program table, its code at dCode; desc[q * descStride].filter = the program of query q or -1.  Enqueued after k_finalize, before k_postfilter.
#define BRW_MAXG 256u           // groups per k_browse_scan launch: at 256 programs a launch spends ~99 % of its time evaluating, so reading
                                // the codes again for the next 256 costs nothing measurable, and the per-range counts of a launch stay at 2 MB
#define BRW_MAXRANGES 2048
static int32_t browse_enqueue(infx_stream* s, const ProgTable& T, const char* dCode, const DevQPost* desc, uint32_t descStride, uint32_t ncount, int32_t max_results, bool ties) {
    infx_index* ix = s->ix;
    const int32_t n = ix->d.totalDocs;
    { int32_t rc_ = columns_cover(ix, n, COLS_COVER_CORPUS); if (rc_) return rc_; }
    static const bool earlyStop = [] { const char* e = getenv("INFX_BROWSE_EARLY_STOP"); return !(e && e[0] == '0'); }();
    const uint32_t rowStride = ix->postRows;       // rows a group can hand out: the stride of rowDocs
    std::vector<DevBrowseGroup> groups; std::vector<DevBrowseQuery> bq; std::unordered_map<int32_t, uint32_t> groupOf;
    for (auto& b : s->browseQ) {
        const int32_t prog = desc[(size_t)b.first * descStride].filter;
        auto it = groupOf.find(prog);
        if (it == groupOf.end()) { it = groupOf.emplace(prog, (uint32_t)groups.size()).first; groups.push_back(DevBrowseGroup{prog >= 0 ? T.dev((uint32_t)prog, dCode) : DevFilter{}, prog, 0u, 0u, 0u}); }
        const uint32_t rows = std::min<uint32_t>(std::min<uint32_t>(b.second, (uint32_t)max_results), rowStride);
        groups[it->second].rows = std::max(groups[it->second].rows, rows);
        bq.push_back(DevBrowseQuery{b.first, it->second, rows, 0u});
    }
    for (uint32_t k = 0; k < ncount; k++) {      // the programs to count: those no browse query uses are groups without rows
        auto it = groupOf.find((int32_t)k);
        if (it == groupOf.end()) { it = groupOf.emplace((int32_t)k, (uint32_t)groups.size()).first; groups.push_back(DevBrowseGroup{T.dev(k, dCode), (int32_t)k, 0u, 0u, 0u}); }
        groups[it->second].flags |= BRW_COUNT; groups[it->second].countIdx = k;
    }
    const uint32_t G = (uint32_t)groups.size();
    const int64_t tiles = ((int64_t)std::max(n, 1) + BRW_THREADS - 1) / BRW_THREADS;
    const uint32_t nRanges = (uint32_t)std::min<int64_t>(BRW_MAXRANGES, tiles);
    const bool dup = ix->firstLive != nullptr;
    auto al = [](size_t x) { return (x + 15) & ~(size_t)15; };
    const size_t oBq = al((size_t)G * sizeof(DevBrowseGroup)), blob = oBq + bq.size() * sizeof(DevBrowseQuery);
    const size_t oPre = al((size_t)G * nRanges * 4), oTot = oPre + oPre, oOwn = oTot + al((size_t)G * 4), oRows = oOwn + al((size_t)G * 4), work = oRows + (size_t)G * rowStride * 4;
    GROW(s->dBrwBlob, s->capBrwBlob, blob); GROW(s->dBrwWork, s->capBrwWork, work);
    std::vector<uint8_t> H(blob, 0);
    std::memcpy(H.data(), groups.data(), (size_t)G * sizeof(DevBrowseGroup)); std::memcpy(H.data() + oBq, bq.data(), bq.size() * sizeof(DevBrowseQuery));
    UP(s->dBrwBlob, H.data(), blob);
    const DevBrowseGroup* dGroups = (const DevBrowseGroup*)s->dBrwBlob; const DevBrowseQuery* dBq = (const DevBrowseQuery*)((char*)s->dBrwBlob + oBq);
    char* W = (char*)s->dBrwWork;
    uint32_t *dCnt = (uint32_t*)W, *dPre = (uint32_t*)(W + oPre), *dTot = (uint32_t*)(W + oTot), *dOwn = (uint32_t*)(W + oOwn); int32_t* dRows = (int32_t*)(W + oRows);
    if (ncount) { GROW(s->dQCount, s->capQCount, (size_t)ncount * 4); HIPCHK(hipMemsetAsync(s->dQCount, 0, (size_t)ncount * 4, s->st)); }
    if (dup) HIPCHK(hipMemsetAsync(dOwn, 0, (size_t)G * 4, s->st));
    const DevColumns cols = dev_columns(ix);
    s->lastBrowseGroups = G; s->lastBrowseLaunches = 0;
    for (uint32_t g0 = 0; g0 < G; g0 += BRW_MAXG) {
        const uint32_t g = std::min(BRW_MAXG, G - g0);
        DevCountCols cc{};
        for (uint32_t i = 0; i < g; i++) if (groups[g0 + i].prog >= 0) T.add_columns(cc, (uint32_t)groups[g0 + i].prog);
        const size_t lds = ((size_t)g * (dup ? 2 : 1) + (size_t)cc.nUsed * BRW_THREADS * (dup ? 2 : 1)) * 4;
        if (dup) {
            HIPCHK(lds_limit((const void*)k_browse_scan<true>, ix->cfg.device, lds));
            k_browse_scan<true><<<nRanges, BRW_THREADS, lds, s->st>>>(dGroups + g0, g, cc, cols, n, (uint32_t)tiles, nRanges, ix->d.deleted, ix->firstLive, earlyStop ? 1 : 0,
                                                                       dCnt + (size_t)g0 * nRanges, dOwn + g0);
        } else {
            HIPCHK(lds_limit((const void*)k_browse_scan<false>, ix->cfg.device, lds));
            k_browse_scan<false><<<nRanges, BRW_THREADS, lds, s->st>>>(dGroups + g0, g, cc, cols, n, (uint32_t)tiles, nRanges, ix->d.deleted, nullptr, earlyStop ? 1 : 0,
                                                                        dCnt + (size_t)g0 * nRanges, nullptr);
        }
        HIPCHK(hipGetLastError());
        s->lastBrowseLaunches++;
    }
    k_browse_prefix<<<G, BRW_THREADS, 0, s->st>>>(dGroups, nRanges, dCnt, dup ? dOwn : nullptr, dPre, dTot, (uint32_t*)s->dQCount);
    HIPCHK(hipGetLastError());
    if (!bq.empty()) {
        k_browse_gather<<<dim3(nRanges, std::min<uint32_t>(G, 32u)), WAVE, 0, s->st>>>(dGroups, G, cols, n, (uint32_t)tiles, nRanges, ix->d.deleted, ix->firstLive, dCnt, dPre, dRows, rowStride);
        HIPCHK(hipGetLastError());
        uint32_t mostRows = 0; for (const DevBrowseQuery& Q : bq) mostRows = std::max(mostRows, Q.rows);
        if (mostRows <= INFX_FILTER_MAX_ROWS)
            k_browse_rows<<<(uint32_t)bq.size(), WAVE, 0, s->st>>>(dBq, dGroups, dTot, dRows, rowStride, (const long long*)ix->d.docKeyAll, ix->firstLive, max_results, (long long*)s->dFKeys,
                                                                      (float*)s->dFScores, ties ? (uint8_t*)s->dFTies : nullptr, (int32_t*)s->dFDocs, (uint32_t*)s->dFCounts);
        else
            k_browse_rows_wide<<<(uint32_t)bq.size(), BRW_THREADS, 0, s->st>>>(dBq, dGroups, dTot, dRows, rowStride, (const long long*)ix->d.docKeyAll, ix->firstLive, max_results, (long long*)s->dFKeys,
                                                                                (float*)s->dFScores, ties ? (uint8_t*)s->dFTies : nullptr, (int32_t*)s->dFDocs, (uint32_t*)s->dFCounts);
        HIPCHK(hipGetLastError());
    }
    s->lastCountK = ncount; s->lastCountLaunches = 0;      // counted by the scan: no k_filter_count_multi launch
    return INFX_OK;
}

static int32_t check_group_column(const infx_index* ix, int32_t col, const char* what);
// The finalize of a batch with collapsing queries (list, in batch order): k_finalize_win — every query as k_finalize writes it, but the listed ones into their
// windows with a budget of `depth` rows — then ONE k_collapse launch of list.size() workgroups.  One blob holds the list, the slots, the windows and what
// k_collapse keeps for the host; the kept part is downloaded with the batch's other outputs (no host wait here).
static int32_t collapse_enqueue(infx_stream* s, const std::vector<DevCollapse>& list, uint32_t nq, int32_t depth, int Cp, size_t lds, int32_t max_results, bool ties) {
    const size_t k = list.size(), rows = k * (size_t)depth, out = k * (size_t)max_results;
    auto al = [](size_t x) { return (x + 63) & ~(size_t)63; };
    const size_t oList = 0, oSlot = al(oList + k * sizeof(DevCollapse)), oWK = al(oSlot + (size_t)nq * 4), oWS = al(oWK + rows * 8), oWD = al(oWS + rows * 4), oWT = al(oWD + rows * 4);
    const size_t oRD = al(oWT + rows), oRC = oRD + out * 4, oRS = oRC + out * 4, oG = oRS + out * 4, oR = oG + k * 4, oN = oR + k * 4, total = oN + k * 4;
    GROW(s->dClp, s->capClp, total);
    char* D = (char*)s->dClp;
    s->clpSlot.assign(nq, -1);
    for (size_t i = 0; i < k; i++) s->clpSlot[list[i].qi] = (int32_t)i;
    std::vector<uint8_t> H(oWK, 0);
    std::memcpy(H.data() + oList, list.data(), k * sizeof(DevCollapse)); std::memcpy(H.data() + oSlot, s->clpSlot.data(), (size_t)nq * 4);
    UP(D, H.data(), oWK);
    FinalizeWindows win{(const int32_t*)(D + oSlot), (long long*)(D + oWK), (float*)(D + oWS), (uint8_t*)(D + oWT), (int32_t*)(D + oWD)};
    k_finalize_win<<<nq, P2_THREADS, lds, s->st>>>(dev_index(s), (const infx_fused_query*)s->dFQ, (const FusedMeta*)s->dFMeta, (const infx_cov_cand*)s->dCovC,
                                                    (const infx_cov_out*)s->dCovO, (const infx_hit*)s->dFS1, depth, Cp, max_results,
                                                    (long long*)s->dFKeys, (float*)s->dFScores, ties ? (uint8_t*)s->dFTies : nullptr,
                                                    (uint32_t*)s->dFCounts, (uint32_t*)s->dFFlags, (uint32_t*)s->dFErr, (int32_t*)s->dFDocs,
                                                    (const infx_finalize_setup*)s->dFin, win);
    HIPCHK(hipGetLastError());
    if (!s->evK0) { HIPCHK(hipEventCreate(&s->evK0)); HIPCHK(hipEventCreate(&s->evK1)); }
    HIPCHK(hipEventRecord(s->evK0, s->st));
    DevCollapseIo io{};
    io.wKeys = win.keys; io.wScores = win.scores; io.wTies = win.ties; io.wDocs = win.docs; io.depth = (uint32_t)depth;
    io.keys = (long long*)s->dFKeys; io.scores = (float*)s->dFScores; io.ties = ties ? (uint8_t*)s->dFTies : nullptr; io.docs = (int32_t*)s->dFDocs;
    io.counts = (uint32_t*)s->dFCounts; io.stride = (uint32_t)max_results;
    io.rDocs = (int32_t*)(D + oRD); io.rCodes = (uint32_t*)(D + oRC); io.rSizes = (uint32_t*)(D + oRS); io.groups = (uint32_t*)(D + oG); io.ranked = (uint32_t*)(D + oR); io.returned = (uint32_t*)(D + oN);
    k_collapse<<<(uint32_t)k, CLP_THREADS, 0, s->st>>>((const DevCollapse*)(D + oList), (const infx_fused_query*)s->dFQ, io);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(s->evK1, s->st)); s->timedClp = true;
    s->clpStride = (uint32_t)max_results; s->lastClpQueries = (uint32_t)k; s->lastClpLaunches = 1;
    s->clpDocs.resize(out); s->clpCodes.resize(out); s->clpSizes.resize(out); s->clpGroups.resize(k); s->clpRanked.resize(k); s->clpReturned.resize(k);
    // (rows past a query's count are never read: infx_collapse_rows stops at the count; the blob's tail is downloaded as it is)
    DOWN(s->clpDocs.data(), D + oRD, out * 4); DOWN(s->clpCodes.data(), D + oRC, out * 4); DOWN(s->clpSizes.data(), D + oRS, out * 4);
    DOWN(s->clpGroups.data(), D + oG, k * 4); DOWN(s->clpRanked.data(), D + oR, k * 4); DOWN(s->clpReturned.data(), D + oN, k * 4);
    return INFX_OK;
}

// Query.highlight: ONE k_highlight launch over the result table as the post-processing left it, k asking queries (s->hlSlot).  One blob holds each query's
// slot and width and the rows; the rows — strided by what the batch asked: its largest word count, its largest width — come back with the batch's other
// outputs (no host wait here).
static int32_t highlight_enqueue(infx_stream* s, uint32_t nq, int32_t max_results, uint32_t k) {
    uint32_t T = 1, W = HL_MIN_CHARS;
    for (uint32_t q = 0; q < nq; q++) if (s->hlSlot[q] >= 0) { T = std::max<uint32_t>(T, (uint32_t)std::max(s->hlWords[q], 0)); W = std::max<uint32_t>(W, (uint32_t)s->hlReq[q]); }
    const size_t rowU16 = hl_row_u16(T, W), rows = (size_t)k * max_results;
    auto al = [](size_t x) { return (x + 63) & ~(size_t)63; };
    const size_t oSlot = 0, oChars = al(oSlot + (size_t)nq * 4), oRows = al(oChars + (size_t)nq * 4), total = oRows + rows * rowU16 * 2;
    GROW(s->dHl, s->capHl, total);
    char* D = (char*)s->dHl;
    std::vector<uint8_t> Hh(oRows, 0);
    std::memcpy(Hh.data() + oSlot, s->hlSlot.data(), (size_t)nq * 4); std::memcpy(Hh.data() + oChars, s->hlReq.data(), (size_t)nq * 4);
    UP(D, Hh.data(), oRows);
    DevHighlight H{};
    H.slot = (const int32_t*)(D + oSlot); H.chars = (const int32_t*)(D + oChars); H.docs = (const int32_t*)s->dFDocs; H.counts = (const uint32_t*)s->dFCounts;
    H.nq = nq; H.stride = (uint32_t)max_results; H.out = (uint16_t*)(D + oRows); H.termStride = T; H.snipStride = W; H.poolChars = s2_pool();
    if (!s->evH0) { HIPCHK(hipEventCreate(&s->evH0)); HIPCHK(hipEventCreate(&s->evH1)); }
    HIPCHK(hipEventRecord(s->evH0, s->st));
    const uint32_t grid = (uint32_t)(((size_t)nq * max_results + HL_THREADS - 1) / HL_THREADS);
    if (s->hlAlias) k_highlight<true><<<grid, HL_THREADS, (size_t)H.poolChars * 2, s->st>>>(dev_index(s), (const infx_cov_query*)s->dCovQ, H, s->hlCs);
    else k_highlight<false><<<grid, HL_THREADS, (size_t)H.poolChars * 2, s->st>>>(dev_index(s), (const infx_cov_query*)s->dCovQ, H, s->hlCs);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(s->evH1, s->st)); s->timedHl = true;
    s->hlStride = (uint32_t)max_results; s->hlTermStride = T; s->hlSnipStride = W; s->lastHlQueries = k; s->lastHlLaunches = 1; s->lastHlBytes = rows * rowU16 * 2;
    // (rows past a query's count are never read: infx_highlight_rows stops at the count)
    s->hlRows.resize(rows * rowU16); s->hlCounts.resize(nq);
    DOWN(s->hlRows.data(), D + oRows, rows * rowU16 * 2); DOWN(s->hlCounts.data(), s->dFCounts, (size_t)nq * 4);
    return INFX_OK;
}

// k_finalize over s->dCovC / s->dCovO / s->dFMeta / s->dFS1 -> result rows in s->dFKeys ...
static int32_t fused_enqueue_finalize(infx_stream* s, uint32_t nq, int32_t depth, int32_t max_results, bool ties) {
    infx_index* ix = s->ix;
    const uint32_t Cp = pow2_at_least(2u * (uint32_t)depth, 8);
    GROW(s->dFKeys, s->capFKeys, (size_t)nq * max_results * 8);
    GROW(s->dFScores, s->capFScores, (size_t)nq * max_results * 4);
    GROW(s->dFTies, s->capFTies, (size_t)nq * max_results);
    GROW(s->dFCounts, s->capFCounts, (size_t)nq * 4);
    GROW(s->dFFlags, s->capFFlags, (size_t)nq * 4);
    GROW(s->dFErr, s->capFErr, 4);
    HIPCHK(hipMemsetAsync(s->dFErr, 0, 4, s->st));
    const size_t lds = (size_t)Cp * (8 + 4 + 4 + 2 + 1 + 1) + (P2_THREADS + 1) * 4 + 64;
    // Post-processing of the rows: the per-query options of this batch (infx_stream_set_query_post, consumed here) or the session-wide post-filter /
    // facets / boosts / sort, staged as one descriptor that every query shares.  Nothing is staged or launched for a batch without either.
    const bool qp = s->qpOn;
    s->qpOn = false; s->lastCountK = 0; s->lastCountLaunches = 0;
    // Query.collapse_by: the collapsing queries of this batch, in batch order (nothing below differs from a batch without one while the list is empty)
    const bool clp = s->clpOn; s->clpOn = false;
    s->lastClpQueries = s->lastClpLaunches = 0; s->clpSlot.clear(); s->clpPosted = false; s->timedClp = false;
    std::vector<DevCollapse> clpList;
    if (clp) {
        if (s->clpReq.size() != nq) return fail(INFX_EINVAL, "the per-query collapse requests were installed for a batch of another size%s");
        for (uint32_t q = 0; q < nq; q++) {
            const infx_collapse_req& R = s->clpReq[q];
            if (R.col < 0) continue;
            { int32_t rc_ = check_group_column(ix, R.col, "collapse request"); if (rc_) return rc_; }
            if (R.keep < 1 || R.keep > (int32_t)CLP_MAX_KEEP) return fail(INFX_EINVAL, "a collapse request keeps 1 .. INFX_COLLAPSE_MAX_KEEP (16) rows per group%s");
            clpList.push_back(DevCollapse{ix->colCodes[R.col], q, (uint32_t)R.keep});
        }
        if (!clpList.empty() && depth > (int32_t)CLP_MAX_ROWS) return fail(INFX_EUNSUPPORTED, "collapsing works on a ranked list of at most 1024 rows (the depth)%s");
    }
    // Query.highlight: the asking queries of this batch get a slot each, in batch order (nothing below differs from a batch without one while hlK is 0)
    const bool hl = s->hlOn; s->hlOn = false;
    s->lastHlQueries = s->lastHlLaunches = 0; s->lastHlBytes = 0; s->hlSlot.clear(); s->timedHl = false;
    uint32_t hlK = 0;
    if (hl) {
        if (s->hlReq.size() != nq) return fail(INFX_EINVAL, "the per-query highlight requests were installed for a batch of another size%s");
        if (s->hlWords.size() != nq) return fail(INFX_EINVAL, "highlight requests need the batch's own Stage-2 call in front of its finalize (infx_search_fused)%s");
        s->hlSlot.assign(nq, -1);
        for (uint32_t q = 0; q < nq; q++) {
            if (s->hlReq[q] == 0) continue;
            if (s->hlReq[q] < HL_MIN_CHARS || s->hlReq[q] > HL_MAX_CHARS) return fail(INFX_EINVAL, "a highlight request's width is 16 .. 512 UTF-16 units%s");
            s->hlSlot[q] = (int32_t)hlK++;
        }
        if (!hlK) s->hlSlot.clear();
    }
    if (qp && s->qpNq != nq) return fail(INFX_EINVAL, "the per-query options were installed for a batch of another size%s");
    const bool post = !qp && (s->postFilter != nullptr || s->nFacet > 0);
    if (post && max_results > (int32_t)ix->postRows) return fail(INFX_EUNSUPPORTED, "post-filter / facets run on at most %s returned rows per query (infx_set_post_rows)", post_rows_text(ix).c_str());
    const bool pp = !qp && (s->nBoost > 0 || s->sortOn);         // boosts / sort-by: k_postproc after k_postfilter
    if (pp && max_results > (int32_t)ix->postRows) return fail(INFX_EUNSUPPORTED, "boosts / sort-by run on at most %s returned rows per query (infx_set_post_rows)", post_rows_text(ix).c_str());
    const bool sortKnown = !qp && s->sortOn && s->sortCol != 0xFFFFFFFFu;
    if (sortKnown && (s->sortCol >= FILT_MAXCOL || !ix->colCodes[s->sortCol] || !ix->colRankOk[s->sortCol])) return fail(INFX_EINVAL, "the sort column's rank is not uploaded%s");
    bool launchPF = post, launchPP = pp;
    // Queries whose post-processing runs on more than INFX_FILTER_MAX_ROWS rows (an index with infx_set_post_rows) are flagged QP_WIDE: the one-wave
    // kernels skip them, the *_wide kernels — launched only for a batch that has one — take them.  A query beyond the index's post rows stays unflagged
    // and is rejected by the one-wave kernels as ever.
    bool widePF = (post || pp) && max_results > INFX_FILTER_MAX_ROWS, widePP = pp && max_results > INFX_FILTER_MAX_ROWS;
    const bool wideShared = widePF;
    bool wideFacets = post && s->nFacet > 0 && max_results > INFX_FILTER_MAX_ROWS;      // a query counts facets on more than INFX_FILTER_MAX_ROWS rows
    if (qp && ix->postRows > INFX_FILTER_MAX_ROWS && s->qpRows.size() == nq) for (uint32_t q = 0; q < nq; q++) {
        DevQPost& D = s->qpDesc[q];
        const bool f = D.filter >= 0 || (D.flags & QP_FACETS), p = D.nboost > 0 || (D.flags & QP_SORT);
        if ((!f && !p) || s->qpRows[q] <= (int32_t)INFX_FILTER_MAX_ROWS || s->qpRows[q] > (int32_t)ix->postRows) continue;
        D.flags |= QP_WIDE; widePF |= f; widePP |= p; wideFacets |= (D.flags & QP_FACETS) != 0;
    }
    if (qp) for (const DevQPost& D : s->qpDesc) {
        launchPF |= D.filter >= 0 || (D.flags & QP_FACETS); launchPP |= D.nboost > 0 || (D.flags & QP_SORT);
        if ((D.flags & QP_SORT) && D.sortCol != 0xFFFFFFFFu && (D.sortCol >= FILT_MAXCOL || !ix->colCodes[D.sortCol] || !ix->colRankOk[D.sortCol]))
            return fail(INFX_EINVAL, "the sort column's rank is not uploaded%s");
    }
    const uint32_t nfacet = qp ? s->qpNFacet : s->nFacet; const uint32_t* facetCols = qp ? s->qpFacetCols : s->facetCols;
    const uint32_t ncount = qp ? s->qpNCount : 0;
    // browse queries (empty text + facets): each needs a descriptor that counts facets; their rows come from the ordered scan after k_finalize
    const bool browse = !s->browseQ.empty();
    if (browse) {
        if (!nfacet) { s->browseQ.clear(); return fail(INFX_EINVAL, "a browse query needs facet columns on the stream%s"); }
        if (qp) for (auto& b : s->browseQ) if (!(s->qpDesc[b.first].flags & QP_FACETS)) { s->browseQ.clear(); return fail(INFX_EINVAL, "a browse query needs INFX_QP_FACETS in its descriptor%s"); }
        if (!ix->d.docKeyAll) { s->browseQ.clear(); return fail(INFX_EINVAL, "index not uploaded%s"); }
    }
    if (launchPF || launchPP || !clpList.empty() || hlK) GROW(s->dFDocs, s->capFDocs, (size_t)nq * max_results * 4);
    const DevColumns cols = dev_columns(ix);
    const DevPostBatch* dPB = nullptr; const DevFilter* dProgs = nullptr; const char* dCode = nullptr;
    // the batch's program table, boost list and descriptors: the staged per-query ones, or the session-wide filters (resident entries) behind one shared descriptor
    ProgTable sprogs; std::vector<DevQBoost> sboost; std::vector<DevQPost> sdesc;
    const ProgTable& T = qp ? s->qpTable : sprogs;
    const std::vector<DevQBoost>& boosts = qp ? s->qpBoosts : sboost; const std::vector<DevQPost>& desc = qp ? s->qpDesc : sdesc;
    const uint32_t descStride = qp ? 1u : 0u;
    if (launchPF || launchPP || ncount) {       // the batch's DevPostBatch, program table, boost list and descriptors (+ the packed per-query programs): one upload
        if (!qp) {
            DevQPost D{}; D.filter = -1; D.sortCol = 0;
            if (s->postFilter) { D.filter = (int32_t)sprogs.size(); sprogs.add(s->postFilter); }
            if (s->nFacet) D.flags |= QP_FACETS;
            D.boostOff = 0; D.nboost = s->nBoost;
            for (uint32_t b = 0; b < s->nBoost; b++) { sboost.push_back(DevQBoost{(int32_t)sprogs.size(), s->boostStrength[b]}); sprogs.add(s->boosts[b]); }
            if (s->sortOn) { D.flags |= QP_SORT | (s->sortAsc ? QP_ASC : 0u); D.sortCol = s->sortCol; }
            if (wideShared) D.flags |= QP_WIDE;
            sdesc.push_back(D);
        }
        auto al = ProgTable::al16;
        const size_t oProgs = al(sizeof(DevPostBatch)), oBoosts = al(oProgs + T.table_bytes()), oDesc = al(oBoosts + boosts.size() * sizeof(DevQBoost));
        const size_t oCode = al(oDesc + desc.size() * sizeof(DevQPost)), total = oCode + T.code.size();
        GROW(s->dPostBlob, s->capPostBlob, total);
        char* D = (char*)s->dPostBlob;
        DevPostBatch pb{};
        pb.progs = (const DevFilter*)(D + oProgs); pb.boosts = (const DevQBoost*)(D + oBoosts); pb.desc = (const DevQPost*)(D + oDesc); pb.descStride = descStride;
        for (int c = 0; c < FILT_MAXCOL; c++) pb.rank[c] = ix->colRankOk[c] ? ix->colRank[c] : nullptr;
        pb.keys = (long long*)s->dFKeys; pb.scores = (float*)s->dFScores; pb.ties = ties ? (uint8_t*)s->dFTies : nullptr; pb.docs = (int32_t*)s->dFDocs;
        pb.counts = (uint32_t*)s->dFCounts; pb.flags = (uint32_t*)s->dFFlags; pb.stride = max_results;
        pb.fqs = browse ? (const infx_fused_query*)s->dFQ : nullptr;
        std::vector<uint8_t> H(total, 0);
        std::memcpy(H.data(), &pb, sizeof pb);
        T.put(H.data() + oProgs, H.data() + oCode, D + oCode);
        if (!boosts.empty()) std::memcpy(H.data() + oBoosts, boosts.data(), boosts.size() * sizeof(DevQBoost));
        if (!desc.empty()) std::memcpy(H.data() + oDesc, desc.data(), desc.size() * sizeof(DevQPost));
        UP(D, H.data(), total);
        dPB = (const DevPostBatch*)D; dProgs = (const DevFilter*)(D + oProgs); dCode = D + oCode;
    }
    if (ncount && !browse) {       // Filter.NumberOfDocumentsInFilter of the expressions this batch uses first, over the whole corpus (every shard holds the whole columns)
        GROW(s->dQCount, s->capQCount, (size_t)ncount * 4);
        { int32_t rc_ = count_enqueue(s, dProgs, ncount, T.columns(0, ncount), 0, ix->d.totalDocs, (uint32_t*)s->dQCount); if (rc_) return rc_; }
        DOWN(s->qpCountsOut, s->dQCount, (size_t)ncount * 4);
    }
    {   // the per-query truncation records (infx_stream_set_coverage, consumed here); the defaults stay on the device from one batch to the next
        const bool fin = s->finOn; s->finOn = false;
        if (fin && s->finH.size() != nq) return fail(INFX_EINVAL, "the per-query coverage setups were installed for a batch of another size%s");
        if ((size_t)nq * sizeof(infx_finalize_setup) > s->capFin) s->finDefaultN = 0;
        GROW(s->dFin, s->capFin, (size_t)nq * sizeof(infx_finalize_setup));
        if (fin) { UP(s->dFin, s->finH.data(), (size_t)nq * sizeof(infx_finalize_setup)); s->finDefaultN = 0; }
        else if (s->finDefaultN < nq) { std::vector<infx_finalize_setup> d(nq, FIN_DEFAULT_SETUP); UP(s->dFin, d.data(), (size_t)nq * sizeof(infx_finalize_setup)); s->finDefaultN = nq; }
    }
    HIPCHK(hipEventRecord(s->evF0, s->st));
    if (clpList.empty())
    k_finalize<<<nq, P2_THREADS, lds, s->st>>>(dev_index(s), (const infx_fused_query*)s->dFQ, (const FusedMeta*)s->dFMeta, (const infx_cov_cand*)s->dCovC,
                                                (const infx_cov_out*)s->dCovO, (const infx_hit*)s->dFS1, depth, (int)Cp, max_results,
                                                (long long*)s->dFKeys, (float*)s->dFScores, ties ? (uint8_t*)s->dFTies : nullptr,
                                                (uint32_t*)s->dFCounts, (uint32_t*)s->dFFlags, (uint32_t*)s->dFErr, launchPF || launchPP || hlK ? (int32_t*)s->dFDocs : nullptr,
                                                (const infx_finalize_setup*)s->dFin);
    else { int32_t rc_ = collapse_enqueue(s, clpList, nq, depth, (int)Cp, lds, max_results, ties); if (rc_) return rc_; }
    HIPCHK(hipGetLastError());
    if (browse) {
        const int32_t rc_ = browse_enqueue(s, T, dCode, desc.data(), descStride, ncount, max_results, ties);
        s->browseQ.clear();
        if (rc_) return rc_;
        if (ncount) DOWN(s->qpCountsOut, s->dQCount, (size_t)ncount * 4);
    }
    s->facetNq = 0;
    if (launchPF) {     // ResultProcessor.ApplyFilter + FacetBuilder on the rows just produced, before they leave the device
        const size_t fe = (size_t)nq * std::max<uint32_t>(1, nfacet) * ix->postRows;
        GROW(s->dFacCodes, s->capFacCodes, fe * 4); GROW(s->dFacCounts, s->capFacCounts, fe * 4); GROW(s->dFacN, s->capFacN, (size_t)nq * std::max<uint32_t>(1, nfacet) * 4);
        if (!s->dFacetCols) HIPCHK(hipMalloc(&s->dFacetCols, INFX_MAX_FACET_COLS * 4));
        UP(s->dFacetCols, facetCols, INFX_MAX_FACET_COLS * 4);
        k_postfilter<<<nq, WAVE, 0, s->st>>>(dPB, cols, (int)nfacet, (const uint32_t*)s->dFacetCols, (uint32_t*)s->dFacCodes, (uint32_t*)s->dFacCounts, (uint32_t*)s->dFacN, ix->postRows);
        if (widePF) k_postfilter_wide<<<nq, PW_THREADS, 0, s->st>>>(dPB, cols, (int)nfacet, (const uint32_t*)s->dFacetCols, (uint32_t*)s->dFacCodes, (uint32_t*)s->dFacCounts, (uint32_t*)s->dFacN, ix->postRows);
        HIPCHK(hipGetLastError());
        if (nfacet) {
            // Only the pairs that can exist travel back: INFX_FILTER_MAX_ROWS per (query, column) unless a query of the batch counts facets on more
            // rows, so a batch of narrow queries on an index with more post rows downloads what a default index does.  The host copy is packed at that width.
            const uint32_t w = wideFacets ? ix->postRows : std::min<uint32_t>(ix->postRows, INFX_FILTER_MAX_ROWS);
            const size_t slices = (size_t)nq * nfacet, feh = slices * w;
            s->hFacCodes.resize(feh); s->hFacCounts.resize(feh); s->hFacN.resize(slices); s->facetNq = nq; s->facetNFacet = nfacet; s->facetRows = w;
            if (w == ix->postRows) { DOWN(s->hFacCodes.data(), s->dFacCodes, feh * 4); DOWN(s->hFacCounts.data(), s->dFacCounts, feh * 4); }
            else for (int a = 0; a < 2; a++) {
                void* p = pin_take(s, feh * 4); if (!p) return fail(INFX_ENOMEM, "hipHostMalloc staging failed%s");
                HIPCHK(hipMemcpy2DAsync(p, (size_t)w * 4, a ? s->dFacCounts : s->dFacCodes, (size_t)ix->postRows * 4, (size_t)w * 4, slices, hipMemcpyDeviceToHost, s->st)); s->unsynced = true;
                s->pendingOut.push_back({a ? (void*)s->hFacCounts.data() : (void*)s->hFacCodes.data(), p, feh * 4});
            }
            DOWN(s->hFacN.data(), s->dFacN, slices * 4);
        }
    }
    if (launchPP) {     // ResultProcessor.ApplyBoosts + ApplySort on the kept rows (facets count rows, not their order: FacetBuilder's result is the same)
        k_postproc<<<nq, WAVE, 0, s->st>>>(dPB, cols);
        if (widePP) k_postproc_wide<<<nq, PW_THREADS, 0, s->st>>>(dPB, cols, ix->postRows);
        HIPCHK(hipGetLastError());
    }
    if (!clpList.empty()) {      // the rows as the post-processing left them: their number and, where it ran, their documents, which find each row's group again (infx_collapse_rows)
        s->clpCounts.resize(nq);
        DOWN(s->clpCounts.data(), s->dFCounts, (size_t)nq * 4);
        if (launchPF || launchPP) { s->clpFinalDocs.resize((size_t)nq * max_results); s->clpPosted = true; DOWN(s->clpFinalDocs.data(), s->dFDocs, (size_t)nq * max_results * 4); }
    }
    if (hlK) { const int32_t rc_ = highlight_enqueue(s, nq, max_results, hlK); if (rc_) return rc_; }      // on the rows as they leave
    HIPCHK(hipEventRecord(s->evF1, s->st));
    s->timedFused = true;
    return INFX_OK;
}

// result rows -> caller buffers (after the stream is synchronised); rows beyond a query's count stay untouched
struct FusedResultStage { std::vector<int64_t> k; std::vector<float> sc; std::vector<uint8_t> t; };
static int32_t fused_download_results(infx_stream* s, uint32_t nq, int32_t max_results, FusedResultStage& R, bool ties, uint32_t* out_counts, uint32_t* out_flags, uint32_t* err) {
    R.k.resize((size_t)nq * max_results); R.sc.resize((size_t)nq * max_results); R.t.resize(ties ? (size_t)nq * max_results : 0);
    DOWN(R.k.data(), s->dFKeys, (size_t)nq * max_results * 8);
    DOWN(R.sc.data(), s->dFScores, (size_t)nq * max_results * 4);
    if (ties) DOWN(R.t.data(), s->dFTies, (size_t)nq * max_results);
    DOWN(out_counts, s->dFCounts, (size_t)nq * 4);
    if (out_flags) DOWN(out_flags, s->dFFlags, (size_t)nq * 4);
    DOWN(err, s->dFErr, 4);
    return INFX_OK;
}
static void fused_scatter_results(uint32_t nq, int32_t max_results, const FusedResultStage& R, int64_t* out_keys, float* out_scores, uint8_t* out_ties, const uint32_t* out_counts) {
    for (uint32_t i = 0; i < nq; i++) {
        const size_t o = (size_t)i * max_results, c = std::min<size_t>(out_counts[i], (size_t)max_results);
        std::memcpy(out_keys + o, R.k.data() + o, c * 8); std::memcpy(out_scores + o, R.sc.data() + o, c * 4);
        if (out_ties) std::memcpy(out_ties + o, R.t.data() + o, c);
    }
}
static void fused_take_metas(infx_stream* s, const std::vector<FusedMeta>& metas) {
    s->fusedS1 = s->fusedCands = s->fusedTextBytes = 0;
    for (auto& m : metas) { s->fusedS1 += m.s1Count; s->fusedCands += m.candCount; s->fusedTextBytes += (uint64_t)m.pad0 + ((uint64_t)m.pad1 << 32); }
}

int32_t infx_wm_lookup_debug(infx_stream* s, const infx_cov_query* cq, infx_wm_list* lists_out, uint32_t* nlists_out, int32_t* owned_out, uint64_t owned_cap) {
    if (!s || !cq || !lists_out || !nlists_out || (owned_cap && !owned_out)) return fail(INFX_EINVAL, "null argument%s");
    infx_index* ix = s->ix;
    if (!ix->haveDict) return fail(INFX_EINVAL, "infx_upload_wm_dictionary has not been called%s");
    const uint32_t words = wm_words(*cq);
    if (cq->text_len > INFX_MAX_QUERY_CHARS || cq->num_fusion_tokens > 2 * INFX_MAX_QUERY_TOKENS) return fail(INFX_EUNSUPPORTED, "query exceeds the Stage-2 envelope%s");
    if (words * (uint32_t)(3 + 2 * ix->lk->maxLd1) > INFX_MAX_WM_LISTS) return fail(INFX_ECAPACITY, "too many words for the device WordMatcher lookup%s");
    if ((uint64_t)words * WM_AFFIX_CAP > owned_cap) return fail(INFX_EINVAL, "owned_out too small%s");
    HIPCHK(enter_device(ix->cfg.device));
    { int32_t rc_ = pin_reset(s); if (rc_) return rc_; }
    infx_fused_query fq{}; fq.dev = -1; fq.flags = INFX_FQ_COV | INFX_FQ_WMDEV; fq.max_results = 1; fq.reserved = 0;
    GROW(s->dFQ, s->capFQ, sizeof(infx_fused_query));
    GROW(s->dFLists, s->capFLists, (size_t)INFX_MAX_WM_LISTS * sizeof(infx_wm_list));
    GROW(s->dFOwned, s->capFOwned, ((size_t)words * WM_AFFIX_CAP + 1) * 4);
    GROW(s->dCovQ, s->capCovQ, sizeof(infx_cov_query));
    UP(s->dFQ, &fq, sizeof fq); UP(s->dCovQ, cq, sizeof *cq);
    DevLookup lk = *ix->lk; if (s->csOn && !s->cs.cover_prefix_suffix) lk.nAffix = 0;
    s->csOn = false;
    k_wm<<<1, WAVE, 0, s->st>>>(lk, (infx_fused_query*)s->dFQ, (const infx_cov_query*)s->dCovQ, 1, (infx_wm_list*)s->dFLists, 0, (int32_t*)s->dFOwned, 0ull);
    HIPCHK(hipGetLastError());
    infx_fused_query back{};
    DOWN(&back, s->dFQ, sizeof back);
    DOWN(lists_out, s->dFLists, (size_t)INFX_MAX_WM_LISTS * sizeof(infx_wm_list));
    if (words) DOWN(owned_out, s->dFOwned, (size_t)words * WM_AFFIX_CAP * 4);
    SYNC();
    *nlists_out = back.wm_count;
    return INFX_OK;
}

int32_t infx_search_fused(infx_stream* s, uint32_t nd, const infx_query* q, uint32_t nterms, const infx_term* terms,
                          uint32_t nq, const infx_fused_query* fq, const infx_cov_query* cq,
                          uint32_t nlists, const infx_wm_list* lists, uint32_t owned_n, const int32_t* owned,
                          int32_t depth, int32_t max_results, int32_t want_debug,
                          int64_t* out_keys, float* out_scores, uint8_t* out_ties, uint32_t* out_counts, uint32_t* out_flags) {
    if (!s || (nd && (!q || (nterms && !terms))) || (nq && (!fq || !cq || !out_keys || !out_scores || !out_counts)) || (nlists && !lists) || (owned_n && !owned))
        return fail(INFX_EINVAL, "null argument%s");
    infx_index* ix = s->ix;
    struct MaskUse { infx_stream* s; ~MaskUse() { s->qDelOn = false; s->docMasks.clear(); } } maskUse{s};      // the per-query flags are this batch's, whatever its outcome
    if (!ix->havePostings || !ix->haveDocs || !ix->d.text) return fail(INFX_EINVAL, "index not uploaded%s");
    if (ix->nranks > 1 || ix->d.docBase != 0) return fail(INFX_EINVAL, "infx_search_fused needs an unsharded index (sharded engines use infx_shard_*)%s");
    if (!s->docMasks.empty() && s->docMasks.size() != nq) return fail(INFX_EINVAL, "the per-query document masks were installed for a batch of another size%s");
    if (nq == 0) return INFX_OK;
    { int32_t rc_ = fused_check_queries(ix, nd, nq, fq, cq, nlists, lists, owned_n, depth, max_results, s->nLongQ); if (rc_) return rc_; }
    for (uint32_t i = 0; i < nd; i++) if (q[i].depth != depth) return fail(INFX_EINVAL, "all queries of a fused batch share one depth%s");
    HIPCHK(enter_device(ix->cfg.device));
    { int32_t rc_ = pin_reset(s); if (rc_) return rc_; }
    // Pre-filters: the masks this batch is missing are built first, on this stream (one launch, no host wait); then the table of each query's flags
    { int32_t rc_ = mask_flush(s); if (rc_) return rc_; }
    { int32_t rc_ = stage_doc_masks(s, nd, nq, fq); if (rc_) return rc_; }
    // Turnstile.  k_accumulate and k_select fill the GPU on their own; the replay, candidate assembly and Stage 2 behind them are narrow.  Sessions that
    // submit together run their wide kernels against each other and then sit in their narrow phases together — convoys that leave the GPU half empty (the
    // bench timeline showed three batches finishing within a millisecond of each other, then nothing wide to run).  Each batch's k_accumulate therefore waits
    // (stream-side, no host wait) for the k_select of the batch submitted before it on this index: wide phases queue up one behind the other, each batch's
    // narrow tail overlaps the next batch's wide phase.  INFX_TURNSTILE=0 switches it off.
    static const bool turnstile = [] { const char* e = getenv("INFX_TURNSTILE"); return !(e && e[0] == '0'); }();
    {
        std::unique_lock<std::mutex> turn(ix->turnMu, std::defer_lock);
        // (round 6 measured the wait BETWEEN k_accumulate_sparse and the streaming k_accumulate — the address-path-bound kernel of this batch beside the vector-bound
        //  kernels of the batch before: no difference, 94.7 / 94.4 k against 95.8 / 94.3 k queries/s over 200 batches; the streaming kernel's four 128-register
        //  waves per SIMD leave no room for a second kernel's waves)
        if (turnstile) { turn.lock(); if (ix->turnEvent && ix->turnEvent != s->evTurn) HIPCHK(hipStreamWaitEvent(s->st, ix->turnEvent, 0)); }
        if (nd) { int32_t rc_ = acc_enqueue(s, nd, q, nterms, terms, 0, nullptr); if (rc_) return rc_; }
        else { HIPCHK(hipEventRecord(s->evA0, s->st)); HIPCHK(hipEventRecord(s->evA1, s->st)); }
        { int32_t rc_ = fused_enqueue_select(s, nd, depth, false, turnstile); if (rc_) return rc_; }
        if (turnstile) ix->turnEvent = s->evTurn;
    }
    { int32_t rc_ = fused_enqueue_prep_stage2(s, 1, nd, (const infx_hit*)s->dHits, (const uint32_t*)s->dHitCount, nq, fq, cq, nlists, lists, owned_n, owned, depth, want_debug); if (rc_) return rc_; }
    { int32_t rc_ = fused_enqueue_finalize(s, nq, depth, max_results, out_ties != nullptr); if (rc_) return rc_; }
    uint32_t ovf = 0, err = 0; std::vector<unsigned long long> qbytes(nd); std::vector<SelRule> rules(nd); std::vector<FusedMeta> metas(nq);
    FusedResultStage R;
    DOWN(metas.data(), s->dFMeta, (size_t)nq * sizeof(FusedMeta));
    { int32_t rc_ = fused_download_results(s, nq, max_results, R, out_ties != nullptr, out_counts, out_flags, &err); if (rc_) return rc_; }
    if (nd) { DOWN(&ovf, s->dOverflow, 4); DOWN(qbytes.data(), s->dQBytes, (size_t)nd * 8); DOWN(rules.data(), s->dRules, (size_t)nd * sizeof(SelRule)); }
    SYNC();
    if (ovf) return fail(INFX_ECAPACITY, "candidate arena overflow (bound violated)%s");
    (void)err;     // candidates outside the Stage-2 envelope are skipped per query (result flag bit 3), they no longer fail the batch
    fused_scatter_results(nq, max_results, R, out_keys, out_scores, out_ties, out_counts);
    s->lastAlgBytes = 0; for (auto b : qbytes) s->lastAlgBytes += b;
    s->lastCandTotal = 0; for (auto& r : rules) s->lastCandTotal += r.total;
    fused_take_metas(s, metas);
    return INFX_OK;
}

// ---- document-sharded operation: the same device stages with the collectives of SURVEY 8(e) in between (host buffers) ----------
int32_t infx_shard_select(infx_stream* s, uint32_t nd, const infx_counts* global_counts, int32_t depth, infx_hit* hits_out, uint32_t* hitcount_out, float* next_out) {
    if (!s || (nd && (!global_counts || !hits_out || !hitcount_out))) return fail(INFX_EINVAL, "null argument%s");
    if (s) { s->shSelected = false; s->shNd = 0; s->shHead[0] = s->shHead[1] = s->shHead[2] = 0; }
    if (nd == 0) return INFX_OK;
    if (nd != s->lastNq) return fail(INFX_EINVAL, "infx_shard_select must follow infx_stage1_accumulate of the same batch%s");
    infx_index* ix = s->ix;
    HIPCHK(enter_device(ix->cfg.device));
    { int32_t rc_ = pin_reset(s); if (rc_) return rc_; }
    UPX(s->dCounts, global_counts, (size_t)nd * INFX_NCLASS * 4);         // the tier rules see the GLOBAL cardinalities (quirk Q11); host or device memory
    { int32_t rc_ = fused_enqueue_select(s, nd, depth, true); if (rc_) return rc_; }
    std::vector<SelRule> rules(nd);
    DOWNX(hits_out, s->dHits, (size_t)nd * depth * sizeof(infx_hit));
    DOWNX(hitcount_out, s->dHitCount, (size_t)nd * 4);
    if (next_out) DOWNX(next_out, s->dNext, (size_t)nd * 4);
    s->shSelected = true; s->shNd = nd; s->shDepth = depth;
    DOWN(rules.data(), s->dRules, (size_t)nd * sizeof(SelRule));
    SYNC();
    s->lastCandTotal = 0; for (auto& r : rules) s->lastCandTotal += r.total;
    return INFX_OK;
}

int32_t infx_shard_stage2(infx_stream* s, int32_t nshards, uint32_t nd, const infx_hit* all_hits, const uint32_t* all_hitcounts,
                          uint32_t nq, const infx_fused_query* fq, const infx_cov_query* cq, uint32_t nlists, const infx_wm_list* lists,
                          uint32_t owned_n, const int32_t* owned, int32_t depth, int32_t max_results, int32_t want_debug, infx_cov_out* outs_out) {
    if (!s || nshards < 1 || (nd && (!all_hits || !all_hitcounts)) || (nq && (!fq || !cq || !outs_out)) || (nlists && !lists) || (owned_n && !owned))
        return fail(INFX_EINVAL, "null argument%s");
    infx_index* ix = s->ix;
    if (!ix->haveDocs || !ix->d.text || !ix->d.docKeyAll) return fail(INFX_EINVAL, "index not uploaded%s");
    if (nq == 0) return INFX_OK;
    { int32_t rc_ = fused_check_queries(ix, nd, nq, fq, cq, nlists, lists, owned_n, depth, max_results, s->nLongQ); if (rc_) return rc_; }
    HIPCHK(enter_device(ix->cfg.device));
    { int32_t rc_ = pin_reset(s); if (rc_) return rc_; }
    const size_t nh = (size_t)nshards * std::max<size_t>(1, nd) * depth;
    GROW(s->dFHitsAll, s->capFHitsAll, nh * sizeof(infx_hit));
    GROW(s->dFHcAll, s->capFHcAll, (size_t)nshards * std::max<size_t>(1, nd) * 4);
    UPX(s->dFHitsAll, all_hits, (size_t)nshards * nd * depth * sizeof(infx_hit));
    UPX(s->dFHcAll, all_hitcounts, (size_t)nshards * nd * 4);
    { int32_t rc_ = fused_enqueue_prep_stage2(s, nshards == 1 ? 1 : nshards, nd, (const infx_hit*)s->dFHitsAll, (const uint32_t*)s->dFHcAll, nq, fq, cq, nlists, lists, owned_n, owned, depth, want_debug); if (rc_) return rc_; }
    std::vector<FusedMeta> metas(nq);
    DOWN(metas.data(), s->dFMeta, (size_t)nq * sizeof(FusedMeta));
    DOWNX(outs_out, s->dCovO, (size_t)nq * 2 * depth * sizeof(infx_cov_out));
    SYNC();
    fused_take_metas(s, metas);
    return INFX_OK;
}

int32_t infx_shard_finalize(infx_stream* s, uint32_t nq, const infx_cov_out* merged_outs, int32_t depth, int32_t max_results,
                            int64_t* out_keys, float* out_scores, uint8_t* out_ties, uint32_t* out_counts, uint32_t* out_flags) {
    if (!s || (nq && (!merged_outs || !out_keys || !out_scores || !out_counts))) return fail(INFX_EINVAL, "null argument%s");
    if (nq == 0) return INFX_OK;
    if (nq != s->fusedNq || depth != s->fusedDepth) return fail(INFX_EINVAL, "infx_shard_finalize must follow infx_shard_stage2 of the same batch%s");
    HIPCHK(enter_device(s->ix->cfg.device));
    { int32_t rc_ = pin_reset(s); if (rc_) return rc_; }
    UPX(s->dCovO, merged_outs, (size_t)nq * 2 * depth * sizeof(infx_cov_out));
    { int32_t rc_ = fused_enqueue_finalize(s, nq, depth, max_results, out_ties != nullptr); if (rc_) return rc_; }
    uint32_t err = 0; FusedResultStage R;
    { int32_t rc_ = fused_download_results(s, nq, max_results, R, out_ties != nullptr, out_counts, out_flags, &err); if (rc_) return rc_; }
    SYNC();
    (void)err;     // candidates outside the Stage-2 envelope are skipped per query (result flag bit 3), they no longer fail the batch
    fused_scatter_results(nq, max_results, R, out_keys, out_scores, out_ties, out_counts);
    return INFX_OK;
}

// ---- exact Stage-1 replay across document shards (exactsh.hip.inc) ----------------------------------------------------------------------------------
static bool shard_exact_possible(infx_stream* s) { return exact_enabled(s->ix) && s->maskWords > 0 && s->ix->cfg.max_depth <= EXS_MAXDEPTH; }

int32_t infx_shard_replay_local(infx_stream* s, int32_t nshards, uint32_t nd, const infx_hit* all_hits, const uint32_t* all_hitcounts, const float* all_next,
                                int32_t depth, uint64_t* blob_bytes) {
    if (!s || nshards < 1 || !blob_bytes || (nd && (!all_hits || !all_hitcounts || !all_next))) return fail(INFX_EINVAL, "null argument%s");
    *blob_bytes = shx_blob_bytes(nd, 0, 0);
    infx_index* ix = s->ix;
    if (nd == 0) { s->shHead[0] = 0; s->shHead[1] = s->shHead[2] = 0; return INFX_OK; }
    if (!s->shSelected || nd != s->shNd || depth != s->shDepth) return fail(INFX_EINVAL, "infx_shard_replay_local must follow infx_shard_select of the same batch%s");
    if (nshards != ix->nranks) return fail(INFX_EINVAL, "nshards differs from infx_set_shard%s");
    if (ix->nranks > 1 && (ix->d.docBase & 0xFFFF)) return fail(INFX_EINVAL, "exact replay across shards needs shard boundaries at multiples of 65536 documents (whole Roaring containers)%s");
    HIPCHK(enter_device(ix->cfg.device));
    { int32_t rc_ = pin_reset(s); if (rc_) return rc_; }
    const uint32_t Dall = pow2_at_least((uint32_t)nshards * (uint32_t)depth, 8);
    if (Dall > 16384) return fail(INFX_ECAPACITY, "shards x depth exceeds the in-LDS merge (16384 rows)%s");
    const size_t nh = (size_t)nshards * nd * depth;
    GROW(s->dFHitsAll, s->capFHitsAll, nh * sizeof(infx_hit));
    GROW(s->dFHcAll, s->capFHcAll, (size_t)nshards * nd * 4);
    GROW(s->dAllNext, s->capAllNext, (size_t)nshards * nd * 4);
    GROW(s->dPrior, s->capPrior, (size_t)nd * EXS_MAXDEPTH * 4);
    UPX(s->dFHitsAll, all_hits, nh * sizeof(infx_hit));
    UPX(s->dFHcAll, all_hitcounts, (size_t)nshards * nd * 4);
    UPX(s->dAllNext, all_next, (size_t)nshards * nd * 4);
    const bool possible = shard_exact_possible(s);
    HIPCHK(hipMemsetAsync(s->dExactStat, 0, 32, s->st));
    HIPCHK(hipEventRecord(s->evX0, s->st));
    {
        const size_t lds = (size_t)Dall * 8 + 257 * 4;
        static std::mutex mu; static size_t attr = 0;
        { std::lock_guard<std::mutex> lk(mu); if (lds > 64 * 1024 && lds > attr) { HIPCHK(hipFuncSetAttribute((const void*)k_gflag, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds)); attr = lds; } }
        k_gflag<<<nd, 256, lds, s->st>>>(dev_index(s), nshards, (int)nd, depth, (int)Dall, (const infx_hit*)s->dFHitsAll, (const uint32_t*)s->dFHcAll, (const float*)s->dAllNext,
                                        (uint32_t*)s->dExactFlag, (float*)s->dPrior, s->dExactStat + 4, possible ? 1 : 0, (const uint32_t*)s->dWideQ, s->nWide);
    }
    ExBufs xb{};
    if (possible) {
        Arena ar = make_arena(s);
        { int32_t rc_ = exact_chunk_tables(s, nd, xb); if (rc_) return rc_; }
        { int32_t rc_ = launch_scan_and_chunks(s, nd, ar, xb, ix->d.docBase > 0 ? (const float*)s->dPrior : nullptr, false); if (rc_) return rc_; }
        // worst case: every reserved row of every flagged query is emitted
        const size_t need = shx_blob_bytes(nd, s->exChunkCap, 0) + s->exCap * sizeof(infx_hit);
        GROW(s->shBlob, s->capShBlob, need);
        k_exsh_count<<<(nd + 255) / 256, 256, 0, s->st>>>(nd, (const uint32_t*)s->dExactFlag, xb, (ShQHdr*)((unsigned char*)s->shBlob + 16));
        k_exsh_scan<<<1, 256, 0, s->st>>>(nd, (ShQHdr*)((unsigned char*)s->shBlob + 16), (uint32_t*)s->shBlob);
        k_exsh_copy<<<nd, 256, 0, s->st>>>(nd, (const uint32_t*)s->dExactFlag, ar, xb, (unsigned char*)s->shBlob);
        HIPCHK(hipGetLastError());
        DOWN(s->shHead, s->shBlob, 16);
    } else {
        GROW(s->shBlob, s->capShBlob, shx_blob_bytes(nd, 0, 0));
        HIPCHK(hipMemsetAsync(s->shBlob, 0, shx_blob_bytes(nd, 0, 0), s->st));
        const uint32_t head[4] = {nd, 0, 0, 0};
        UP(s->shBlob, head, 16);
        s->shHead[0] = nd; s->shHead[1] = s->shHead[2] = s->shHead[3] = 0;
    }
    HIPCHK(hipGetLastError());
    DOWN(s->lastFlagWhy, s->dExactStat + 4, 16);
    SYNC();
    *blob_bytes = shx_blob_bytes(nd, s->shHead[1], s->shHead[2]);
    return INFX_OK;
}

int32_t infx_shard_replay_blob(infx_stream* s, void* dst, uint64_t padded_bytes) {
    if (!s || !dst) return fail(INFX_EINVAL, "null argument%s");
    const size_t have = shx_blob_bytes(s->shNd, s->shHead[1], s->shHead[2]);
    if (!s->shNd) return INFX_OK;
    if (padded_bytes < have) return fail(INFX_EINVAL, "padded size below this shard's blob%s");
    HIPCHK(enter_device(s->ix->cfg.device));
    { int32_t rc_ = pin_reset(s); if (rc_) return rc_; }
    DOWNX(dst, s->shBlob, have);       // the padding beyond `have` is never read (the header says how much is valid)
    SYNC();
    return INFX_OK;
}

int32_t infx_shard_replay_merge(infx_stream* s, int32_t nshards, uint32_t nd, const void* all_blobs, uint64_t padded_bytes, int32_t depth,
                                infx_hit* hits_out, uint32_t* hitcount_out) {
    if (!s || nshards < 1 || (nd && (!all_blobs || !hits_out || !hitcount_out))) return fail(INFX_EINVAL, "null argument%s");
    if (nd == 0) return INFX_OK;
    infx_index* ix = s->ix;
    if (!s->shSelected || nd != s->shNd || depth != s->shDepth || nshards != ix->nranks) return fail(INFX_EINVAL, "infx_shard_replay_merge must follow infx_shard_replay_local of the same batch%s");
    if (padded_bytes < shx_blob_bytes(nd, 0, 0)) return fail(INFX_EINVAL, "blob size below the header%s");
    HIPCHK(enter_device(ix->cfg.device));
    { int32_t rc_ = pin_reset(s); if (rc_) return rc_; }
    GROW(s->dAllBlobs, s->capAllBlobs, (size_t)nshards * padded_bytes);
    UPX(s->dAllBlobs, all_blobs, (size_t)nshards * padded_bytes);
    HIPCHK(hipMemsetAsync(s->dExactStat, 0, 16, s->st));
    k_ex_heap_sh<<<nd, WAVE, 0, s->st>>>(nshards, ix->rank, nd, (const unsigned char*)s->dAllBlobs, (size_t)padded_bytes, (const uint32_t*)s->dExactFlag, depth,
                                         exact_slow_only() ? 1 : 0, (infx_hit*)s->dHits, (uint32_t*)s->dHitCount, depth, s->dExactStat, ex_heap_in_regs(ix, depth));
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(s->evX1, s->st)); s->timedReplay = true;
    DOWNX(hits_out, s->dHits, (size_t)nd * depth * sizeof(infx_hit));
    DOWNX(hitcount_out, s->dHitCount, (size_t)nd * 4);
    uint32_t st4[4] = {0, 0, 0, 0};
    DOWN(st4, s->dExactStat, 16);
    SYNC();
    s->lastExact2[0] = st4[0]; s->lastExact2[1] = st4[2];       // owned queries replayed here; of the owned ones, handed to the sequential chain
    return INFX_OK;
}

int32_t infx_shard_replay_chain(infx_stream* s, uint32_t nd, const uint32_t* need, int32_t depth, void* state) {
    if (!s || (nd && (!need || !state))) return fail(INFX_EINVAL, "null argument%s");
    if (nd == 0) return INFX_OK;
    infx_index* ix = s->ix;
    if (!s->shSelected || nd != s->shNd || depth != s->shDepth) return fail(INFX_EINVAL, "infx_shard_replay_chain must follow infx_shard_select of the same batch%s");
    if (!shard_exact_possible(s)) return fail(INFX_EINVAL, "no hit masks were kept for this batch: nothing to replay%s");
    HIPCHK(enter_device(ix->cfg.device));
    { int32_t rc_ = pin_reset(s); if (rc_) return rc_; }
    const int depthCap = ix->cfg.max_depth;
    if (depth != depthCap) return fail(INFX_EINVAL, "the chained replay exchanges heaps of infx_config.max_depth entries: search with that depth%s");
    const size_t words = (size_t)nd * (2 + 2 * (size_t)depthCap);
    GROW(s->dChainState, s->capChainState, words * 4);
    GROW(s->dChainNeed, s->capChainNeed, (size_t)nd * 4);
    UPX(s->dChainState, state, words * 4);
    UPX(s->dChainNeed, need, (size_t)nd * 4);
    size_t lds1 = 0; { int32_t rc_ = exact1_lds_ready(ix, s->maskWords, &lds1); if (rc_) return rc_; }
    Arena ar = make_arena(s);
    k_exact1<<<nd, EX_THREADS, lds1, s->st>>>(dev_index(s), (const DevQuery*)s->dQueries, (const DevRefTerm*)s->dRefTerms, ar, (const SelRule*)s->dRules, (const uint32_t*)s->dExactFlag,
                                             0u, ix->avgdl, (infx_hit*)s->dHits, (uint32_t*)s->dHitCount, depth, depthCap, nullptr, (uint32_t*)s->dChainState, (const uint32_t*)s->dChainNeed);
    HIPCHK(hipGetLastError());
    DOWNX(state, s->dChainState, words * 4);
    SYNC();
    return INFX_OK;
}

int32_t infx_upload_doc_keys_all(infx_index* ix, uint32_t total_docs, const int64_t* keys) {
    if (!ix || (total_docs && !keys)) return fail(INFX_EINVAL, "null argument%s");
    HIPCHK(enter_device(ix->cfg.device));
    int64_t* d = nullptr;
    HIPCHK(dalloc(ix, &d, (size_t)total_docs + 1));
    if (total_docs) HIPCHK(hipMemcpy(d, keys, (size_t)total_docs * 8, hipMemcpyHostToDevice));
    ix->d.docKeyAll = d;
    return INFX_OK;
}

int32_t infx_fused_debug(infx_stream* s, infx_hit* s1, uint32_t* s1_counts, infx_cov_cand* cands, infx_cov_out* outs, int32_t* feat,
                         uint32_t* cand_counts, uint32_t* run_cov, int32_t* idx01) {
    if (!s || !s->fusedNq) return fail(INFX_EINVAL, "no fused batch to read back%s");
    if (feat && !s->fusedDebug) return fail(INFX_EINVAL, "the last fused batch ran without want_debug%s");
    HIPCHK(enter_device(s->ix->cfg.device));
    { int32_t rc_ = pin_reset(s); if (rc_) return rc_; }
    const uint32_t nq = s->fusedNq; const size_t depth = (size_t)s->fusedDepth, ncand = (size_t)nq * 2 * depth;
    std::vector<FusedMeta> metas(nq);
    if (s1) DOWN(s1, s->dFS1, (size_t)nq * depth * sizeof(infx_hit));
    if (cands) DOWN(cands, s->dCovC, ncand * sizeof(infx_cov_cand));
    if (outs) DOWN(outs, s->dCovO, ncand * sizeof(infx_cov_out));
    if (feat) DOWN(feat, s->dCovF, ncand * INFX_NFEAT * 4);
    DOWN(metas.data(), s->dFMeta, (size_t)nq * sizeof(FusedMeta));
    SYNC();
    for (uint32_t i = 0; i < nq; i++) {
        if (s1_counts) s1_counts[i] = metas[i].s1Count;
        if (cand_counts) cand_counts[i] = metas[i].candCount;
        if (run_cov) run_cov[i] = metas[i].runCov | (metas[i].wmAny << 1);
        if (idx01) { idx01[2 * i] = metas[i].idx0; idx01[2 * i + 1] = metas[i].idx1; }
    }
    return INFX_OK;
}

int32_t infx_last_fused_stats(infx_stream* s, uint64_t* s1_rows, uint64_t* stage2_rows, uint64_t* stage2_text_bytes) {
    if (!s) return fail(INFX_EINVAL, "null argument%s");
    if (s1_rows) *s1_rows = s->fusedS1; if (stage2_rows) *stage2_rows = s->fusedCands; if (stage2_text_bytes) *stage2_text_bytes = s->fusedTextBytes;
    return INFX_OK;
}

int32_t infx_last_fused_timings(infx_stream* s, float* ms5) {
    if (!s || !ms5) return fail(INFX_EINVAL, "null argument%s");
    if (s->timedFused) {
        hipEventElapsedTime(&s->msFused[0], s->evA0, s->evA1); hipEventElapsedTime(&s->msFused[1], s->evS0, s->evS1);
        hipEventElapsedTime(&s->msFused[2], s->evP0, s->evP1); hipEventElapsedTime(&s->msFused[3], s->evC0, s->evC1);
        hipEventElapsedTime(&s->msFused[4], s->evF0, s->evF1);
    }
    for (int i = 0; i < 5; i++) ms5[i] = s->msFused[i];
    return INFX_OK;
}

int32_t infx_last_timings(infx_stream* s, float* a, float* b, float* c) {
    if (!s) return fail(INFX_EINVAL, "null argument%s");
    if (s->timedAcc) hipEventElapsedTime(&s->msAcc, s->evA0, s->evA1);
    if (s->timedSel) hipEventElapsedTime(&s->msSel, s->evS0, s->evS1);
    if (s->timedCov) hipEventElapsedTime(&s->msCov, s->evC0, s->evC1);
    if (a) *a = s->msAcc; if (b) *b = s->msSel; if (c) *c = s->msCov;
    return INFX_OK;
}
static int32_t union_build_impl(infx_stream* s, uint32_t nv, const uint32_t* member_offs, const int32_t* members, uint32_t* counts_out,
                                const int32_t* word_of, uint32_t nwords, const uint32_t* word_offs, const uint16_t* chars, uint32_t cap,
                                int32_t* ld1_members_out, uint32_t* ld1_counts_out, uint32_t* ld1_status_out) {
    s->unionCount.clear(); s->unionBase.assign(1, 0);
    if (nv == 0) return INFX_OK;
    infx_index* ix = s->ix;
    if (!ix->havePostings || !ix->haveDocs) return fail(INFX_EINVAL, "index not uploaded%s");
    if (nwords && !ix->haveTrie) return fail(INFX_EINVAL, "infx_upload_term_trie has not been called%s");
    HIPCHK(enter_device(ix->cfg.device));
    { int32_t rc_ = pin_reset(s); if (rc_) return rc_; }
    PlanStream plan(s);
    const int nR = ix->d.nRanges;
    if ((uint64_t)nv * nR > 0x7FFFFFFFull) return fail(INFX_ECAPACITY, "nv * nRanges exceeds the grid limit%s");
    const uint32_t nm = member_offs[nv];
    for (uint32_t i = 0; i < nm; i++) if (members[i] < 0 || members[i] >= ix->d.T) return fail(INFX_EINVAL, "member term id out of range%s");
    if ((uint64_t)nm + (uint64_t)nwords * cap > 0xFFFFFFF0ull) return fail(INFX_ECAPACITY, "too many union members in one batch%s");
    // member ranges: CSR for the unions the caller listed, the word's slot of the tail (closed by k_ld1) for the others
    std::vector<uint32_t> be((size_t)nv * 2); std::vector<int32_t> uow(nwords, -1);
    for (uint32_t v = 0; v < nv; v++) {
        const int32_t w = word_of ? word_of[v] : -1;
        if (w >= 0) { if ((uint32_t)w >= nwords || uow[w] >= 0 || member_offs[v + 1] != member_offs[v]) return fail(INFX_EINVAL, "bad word reference of a union%s"); uow[w] = (int32_t)v; be[v] = nm + (uint32_t)w * cap; be[nv + v] = be[v]; }
        else { be[v] = member_offs[v]; be[nv + v] = member_offs[v + 1]; }
    }
    GROW(s->dUOffs, s->capUOffs, ((size_t)nv * 2 + 2) * 4);
    GROW(s->dUMem, s->capUMem, std::max<size_t>(1, (size_t)nm + (size_t)nwords * cap) * 4);
    GROW(s->dUCnt, s->capUCnt, (size_t)nv * 4);
    GROW(s->dURange, s->capURange, (size_t)nv * (nR + 1) * 4);
    GROW(s->dUBase, s->capUBase, ((size_t)nv + 1) * 8);
    UP(s->dUOffs, be.data(), be.size() * 4);
    UP(s->dUMem, members, (size_t)nm * 4);
    uint32_t* dBeg = (uint32_t*)s->dUOffs; uint32_t* dEnd = dBeg + nv;
    uint32_t *dCnt = nullptr, *dSt = nullptr;
    if (nwords) {
        const size_t nch = word_offs[nwords];
        GROW(s->dLWordOff, s->capLWordOff, ((size_t)nwords * 2 + 2) * 4);
        GROW(s->dLChars, s->capLChars, std::max<size_t>(1, nch) * 2);
        GROW(s->dLCount, s->capLCount, (size_t)nwords * 8);
        UP(s->dLWordOff, word_offs, ((size_t)nwords + 1) * 4);
        UP((uint32_t*)s->dLWordOff + nwords + 1, uow.data(), (size_t)nwords * 4);
        UP(s->dLChars, chars, nch * 2);
        dCnt = (uint32_t*)s->dLCount; dSt = dCnt + nwords;
        k_ld1<<<nwords, WAVE, 0, s->st>>>(*ix->lk, (const uint32_t*)s->dLWordOff, (const uint16_t*)s->dLChars, nwords, cap, (int32_t*)s->dUMem + nm, dCnt, dSt,
                                          dEnd, (const int32_t*)((uint32_t*)s->dLWordOff + nwords + 1), nm);
        HIPCHK(hipGetLastError());
    }
    launch_union_any(s, nv, dBeg, dEnd, (const int32_t*)s->dUMem, (uint32_t*)s->dURange, nullptr, nullptr);
    k_union_scan<<<nv, 256, 0, s->st>>>((uint32_t*)s->dURange, nR, (uint32_t*)s->dUCnt);
    HIPCHK(hipGetLastError());
    DOWN(counts_out, s->dUCnt, (size_t)nv * 4);
    // the expansions travel back with the counts (nwords x cap ids: a few MB at most) — one wait; fetching only the filled part of each row would need the counts
    // first, i.e. a second wait, and that one would sit behind the write pass below
    if (nwords) { DOWN(ld1_counts_out, dCnt, (size_t)nwords * 4); DOWN(ld1_status_out, dSt, (size_t)nwords * 4); DOWN(ld1_members_out, (const int32_t*)s->dUMem + nm, (size_t)nwords * cap * 4); }
    SYNC();
    s->unionCount.assign(counts_out, counts_out + nv);
    s->unionBase.assign((size_t)nv + 1, 0);
    for (uint32_t v = 0; v < nv; v++) s->unionBase[v + 1] = s->unionBase[v] + ((counts_out[v] + 3u) & ~3u);     // 16-byte aligned, sentinel-padded like the index lists
    GROW(s->dUDocs, s->capUDocs, ((size_t)s->unionBase[nv] + 4) * 4);
    HIPCHK(hipMemsetAsync(s->dUDocs, 0x7F, ((size_t)s->unionBase[nv] + 4) * 4, s->st));
    UP(s->dUBase, s->unionBase.data(), ((size_t)nv + 1) * 8);
    launch_union_any(s, nv, dBeg, dEnd, (const int32_t*)s->dUMem, (uint32_t*)s->dURange, (const unsigned long long*)s->dUBase, (int32_t*)s->dUDocs);
    HIPCHK(hipGetLastError());
    return plan.leave();     // the write pass stays queued (planning stream); the main stream — infx_stage1_accumulate — is ordered behind it
}
int32_t infx_union_build(infx_stream* s, uint32_t nv, const uint32_t* member_offs, const int32_t* members, uint32_t* counts_out) {
    if (!s || (nv && (!member_offs || !counts_out || (member_offs[nv] && !members)))) return fail(INFX_EINVAL, "null argument%s");
    return union_build_impl(s, nv, member_offs, members, counts_out, nullptr, 0, nullptr, nullptr, 1, nullptr, nullptr, nullptr);
}
int32_t infx_union_build_ld1(infx_stream* s, uint32_t nv, const uint32_t* member_offs, const int32_t* members, const int32_t* word_of,
                             uint32_t nwords, const uint32_t* word_offs, const uint16_t* chars, uint32_t cap,
                             uint32_t* counts_out, int32_t* ld1_members_out, uint32_t* ld1_counts_out, uint32_t* ld1_status_out) {
    if (!s || (nv && (!member_offs || !counts_out || (member_offs[nv] && !members))) || (nwords && (!word_of || !word_offs || !ld1_members_out || !ld1_counts_out || !ld1_status_out || (word_offs[nwords] && !chars))) || cap == 0)
        return fail(INFX_EINVAL, "null argument%s");
    return union_build_impl(s, nv, member_offs, members, counts_out, nwords ? word_of : nullptr, nwords, word_offs, chars, cap, ld1_members_out, ld1_counts_out, ld1_status_out);
}
int32_t infx_last_replay_stats(infx_stream* s, float* ms, uint32_t* why3) {
    if (!s) return fail(INFX_EINVAL, "null argument%s");
    if (s->timedReplay) { hipEventElapsedTime(&s->msReplay, s->evX0, s->evX1); s->timedReplay = false; }
    if (ms) *ms = s->msReplay;
    if (why3) { why3[0] = s->lastFlagWhy[0]; why3[1] = s->lastFlagWhy[1]; why3[2] = s->lastFlagWhy[2]; }
    return INFX_OK;
}
int32_t infx_last_replay_breakdown(infx_stream* s, float* ms4) {      // scan (k_ex_walk x2 + k_ex_prefix + k_ex_theta), k_ex_chunk (three launches), k_ex_heap, k_exact1 of the last batch
    if (!s || !ms4) return fail(INFX_EINVAL, "null argument%s");
    if (s->timedReplayParts) {
        hipEventElapsedTime(&s->msReplayParts[0], s->evX0, s->evXa); hipEventElapsedTime(&s->msReplayParts[1], s->evXa, s->evXb);
        hipEventElapsedTime(&s->msReplayParts[2], s->evXb, s->evXc); hipEventElapsedTime(&s->msReplayParts[3], s->evXc, s->evX1);
        s->timedReplayParts = false;
    }
    for (int i = 0; i < 4; i++) ms4[i] = s->msReplayParts[i];
    return INFX_OK;
}
int32_t infx_last_exact_replays(infx_stream* s, uint32_t* n) {
    if (!s || !n) return fail(INFX_EINVAL, "null argument%s");
    *n = s->lastExact2[0] + s->lastExact2[1]; return INFX_OK;
}
int32_t infx_last_exact_fallbacks(infx_stream* s, uint32_t* n) {
    if (!s || !n) return fail(INFX_EINVAL, "null argument%s");
    *n = s->lastExact2[1]; return INFX_OK;
}
int32_t infx_last_candidates(infx_stream* s, uint64_t* n) {
    if (!s || !n) return fail(INFX_EINVAL, "null argument%s");
    *n = s->lastCandTotal; return INFX_OK;
}
int32_t infx_last_alg_bytes(infx_stream* s, uint64_t* bytes) {
    if (!s || !bytes) return fail(INFX_EINVAL, "null argument%s");
    *bytes = s->lastAlgBytes; return INFX_OK;
}


// ---- Infiscript post-filter + facets (config 5) --------------------------------------------------------------------------------------
int32_t infx_upload_column(infx_index* ix, uint32_t col, uint32_t total_docs, const uint32_t* codes, uint32_t num_values) {
    if (!ix || col >= FILT_MAXCOL || (total_docs && !codes)) return fail(INFX_EINVAL, "bad column arguments%s");
    HIPCHK(enter_device(ix->cfg.device));
    if (ix->haveDocs && (uint64_t)total_docs < (uint64_t)ix->d.docBase + (uint64_t)ix->d.N) return fail(INFX_EINVAL, "a column needs one code per GLOBAL internal id covering this shard%s");
    HIPCHK(hipDeviceSynchronize());                      // exclusive call (the reference's write lock): no search is in flight
    uint32_t* d = const_cast<uint32_t*>(ix->colCodes[col]);
    if (!d || ix->colCap[col] < total_docs) { HIPCHK(dalloc(ix, &d, (size_t)total_docs + 1)); ix->colCap[col] = total_docs; }     // a re-upload reuses the column's buffer
    if (total_docs) HIPCHK(hipMemcpy(d, codes, (size_t)total_docs * 4, hipMemcpyHostToDevice));
    ix->colCodes[col] = d; ix->colValues[col] = num_values; ix->colDocs[col] = total_docs; ix->colRankOk[col] = false; ix->colBitsOk[col] = false; ix->colTieOk[col] = false;
    return INFX_OK;
}
// a program must be a well-formed postfix expression whose stack fits the kernels' 32 slots, over uploaded columns, with its leaf tables in range
static int32_t check_filter_prog(infx_index* ix, uint32_t nops, const infx_filter_op* ops, uint32_t nleaves, const infx_filter_leaf* leaves, uint32_t ntable_words) {
    if (nops > INFX_FILTER_MAX_OPS) return fail(INFX_ECAPACITY, "filter program too long%s");
    int depth = 0, maxDepth = 0;
    for (uint32_t i = 0; i < nops; i++) {
        const uint32_t o = ops[i].op;
        if (o == INFX_FOP_LEAF) { if (ops[i].arg >= nleaves) return fail(INFX_EINVAL, "filter leaf index out of range%s"); depth++; }
        else if (o == INFX_FOP_LIT) depth++;
        else if (o == INFX_FOP_NOT) { if (depth < 1) return fail(INFX_EINVAL, "malformed filter program%s"); }
        else if (o == INFX_FOP_AND || o == INFX_FOP_OR) { if (depth < 2) return fail(INFX_EINVAL, "malformed filter program%s"); depth--; }
        else if (o == INFX_FOP_TERN) { if (depth < 3) return fail(INFX_EINVAL, "malformed filter program%s"); depth -= 2; }
        else return fail(INFX_EINVAL, "unknown filter opcode%s");
        maxDepth = std::max(maxDepth, depth);
    }
    if (depth != 1 || maxDepth > 32) return fail(INFX_EINVAL, "malformed or too deeply nested filter program%s");
    for (uint32_t l = 0; l < nleaves; l++) {
        const infx_filter_leaf& L = leaves[l];
        if (L.col != 0xFFFFFFFFu && (L.col >= FILT_MAXCOL || !ix->colCodes[L.col])) return fail(INFX_EINVAL, "filter refers to a column that was not uploaded%s");
        if ((uint64_t)L.table_off + (L.num_values + 31) / 32 > ntable_words) return fail(INFX_EINVAL, "filter leaf table out of range%s");
    }
    return INFX_OK;
}
int32_t infx_filter_check(infx_index* ix, uint32_t nops, const infx_filter_op* ops, uint32_t nleaves, const infx_filter_leaf* leaves, uint32_t ntable_words) {
    if (!ix || !nops || !ops || (nleaves && !leaves)) return fail(INFX_EINVAL, "null argument%s");
    return check_filter_prog(ix, nops, ops, nleaves, leaves, ntable_words);
}
int32_t infx_filter_create(infx_index* ix, uint32_t nops, const infx_filter_op* ops, uint32_t nleaves, const infx_filter_leaf* leaves,
                           uint32_t ntable_words, const uint32_t* tables, infx_filter** out) {
    if (!ix || !out || !nops || !ops || (nleaves && (!leaves || !tables))) return fail(INFX_EINVAL, "null argument%s");
    { int32_t rc_ = check_filter_prog(ix, nops, ops, nleaves, leaves, ntable_words); if (rc_) return rc_; }
    HIPCHK(enter_device(ix->cfg.device));
    infx_filter* f = new infx_filter(); f->ix = ix; f->nops = nops; f->nleaves = nleaves; f->hLeaves.assign(leaves, leaves + nleaves);
    auto bail = [&](int32_t rc) { infx_filter_destroy(f); return rc; };
    if (hipMalloc(&f->dOps, nops * sizeof(infx_filter_op)) != hipSuccess || hipMalloc(&f->dLeaves, std::max<size_t>(1, nleaves) * sizeof(infx_filter_leaf)) != hipSuccess ||
        hipMalloc(&f->dTables, std::max<size_t>(1, ntable_words) * 4) != hipSuccess) return bail(fail(INFX_ENOMEM, "filter allocation failed%s"));
    if (hipMemcpy(f->dOps, ops, nops * sizeof(infx_filter_op), hipMemcpyHostToDevice) != hipSuccess) return bail(fail(INFX_EHIP, "filter upload failed%s"));
    if (nleaves && (hipMemcpy(f->dLeaves, leaves, nleaves * sizeof(infx_filter_leaf), hipMemcpyHostToDevice) != hipSuccess ||
                    hipMemcpy(f->dTables, tables, (size_t)ntable_words * 4, hipMemcpyHostToDevice) != hipSuccess)) return bail(fail(INFX_EHIP, "filter upload failed%s"));
    f->d = DevFilter{(const infx_filter_op*)f->dOps, nops, (const infx_filter_leaf*)f->dLeaves, nleaves, (const uint32_t*)f->dTables};
    *out = f; return INFX_OK;
}
void infx_filter_destroy(infx_filter* f) {
    if (!f) return;
    hipSetDevice(f->ix->cfg.device);
    if (f->dOps) hipFree(f->dOps); if (f->dLeaves) hipFree(f->dLeaves); if (f->dTables) hipFree(f->dTables);
    delete f;
}
int32_t infx_filter_count(infx_stream* s, infx_filter* f, uint32_t* count) {
    if (!s || !f || !count || f->ix != s->ix) return fail(INFX_EINVAL, "bad filter arguments%s");
    infx_index* ix = s->ix;
    if (!ix->haveDocs) return fail(INFX_EINVAL, "index not uploaded%s");
    HIPCHK(enter_device(ix->cfg.device));
    { int32_t rc_ = pin_reset(s); if (rc_) return rc_; }
    // k_filter_count_multi with a one-entry program table (the filter's device copy) over this shard's documents
    ProgTable T; T.add(f);
    { int32_t rc_ = table_upload(s, T, &s->dPostBlob, &s->capPostBlob); if (rc_) return rc_; }
    GROW(s->dQCount, s->capQCount, 4);
    { int32_t rc_ = count_enqueue(s, (const DevFilter*)s->dPostBlob, 1, T.columns(0, 1), ix->d.docBase, ix->d.N, (uint32_t*)s->dQCount); if (rc_) return rc_; }
    DOWN(count, s->dQCount, 4);
    SYNC();
    return INFX_OK;
}
int32_t infx_stream_set_postfilter(infx_stream* s, infx_filter* f, uint32_t nfacet, const uint32_t* facet_cols) {
    if (!s || nfacet > INFX_MAX_FACET_COLS || (nfacet && !facet_cols) || (f && f->ix != s->ix)) return fail(INFX_EINVAL, "bad post-filter arguments%s");
    for (uint32_t c = 0; c < nfacet; c++) if (facet_cols[c] >= FILT_MAXCOL || !s->ix->colCodes[facet_cols[c]]) return fail(INFX_EINVAL, "facet column was not uploaded%s");
    { int32_t rc_ = columns_cover(s->ix, s->ix->d.totalDocs, COLS_COVER_CORPUS); if (rc_) return rc_; }      // rows carry GLOBAL internal ids
    if (s->qpOn && (f || nfacet)) return fail(INFX_EINVAL, "per-query options are installed on this stream%s");
    s->postFilter = f; s->nFacet = nfacet;
    for (uint32_t c = 0; c < INFX_MAX_FACET_COLS; c++) s->facetCols[c] = c < nfacet ? facet_cols[c] : 0;
    return INFX_OK;
}
// ---- Query.Boosts + Query.SortBy (k_postproc) ----------------------------------------------------------------------------------------
int32_t infx_upload_sort_rank(infx_index* ix, uint32_t col, uint32_t num_values, const uint32_t* rank) {
    if (!ix || col >= FILT_MAXCOL || (num_values && !rank)) return fail(INFX_EINVAL, "bad sort-rank arguments%s");
    if (!ix->colCodes[col] || num_values != ix->colValues[col]) return fail(INFX_EINVAL, "a sort rank needs one entry per distinct value of an uploaded column%s");
    HIPCHK(enter_device(ix->cfg.device));
    HIPCHK(hipDeviceSynchronize());                      // exclusive call, as infx_upload_column: no search is reading a rank that is rewritten
    uint32_t* d = const_cast<uint32_t*>(ix->colRank[col]);
    if (!d || ix->colRankCap[col] < num_values) { HIPCHK(dalloc(ix, &d, (size_t)num_values)); ix->colRankCap[col] = num_values; }
    if (num_values) HIPCHK(hipMemcpy(d, rank, (size_t)num_values * 4, hipMemcpyHostToDevice));
    ix->colRank[col] = d; ix->colRankOk[col] = true;
    return INFX_OK;
}
// the facet tie order of a column's codes — a permutation of them — for infx_top_groups
int32_t infx_upload_group_rank(infx_index* ix, uint32_t col, uint32_t num_values, const uint32_t* rank) {
    if (!ix || col >= FILT_MAXCOL || (num_values && !rank)) return fail(INFX_EINVAL, "bad group-rank arguments%s");
    if (!ix->colCodes[col] || num_values != ix->colValues[col]) return fail(INFX_EINVAL, "a group rank needs one entry per distinct value of an uploaded column%s");
    {   // the select relies on distinct composites: every rank below num_values, none twice
        std::vector<uint8_t> seen(num_values, 0);
        for (uint32_t i = 0; i < num_values; i++) { if (rank[i] >= num_values || seen[rank[i]]) return fail(INFX_EINVAL, "a group rank is a permutation of the column's codes%s"); seen[rank[i]] = 1; }
    }
    HIPCHK(enter_device(ix->cfg.device));
    HIPCHK(hipDeviceSynchronize());                      // exclusive call, as infx_upload_column
    uint32_t* d = const_cast<uint32_t*>(ix->colTie[col]);
    if (!d || ix->colTieCap[col] < num_values) { HIPCHK(dalloc(ix, &d, (size_t)num_values)); ix->colTieCap[col] = num_values; }
    if (num_values) HIPCHK(hipMemcpy(d, rank, (size_t)num_values * 4, hipMemcpyHostToDevice));
    ix->colTie[col] = d; ix->colTieOk[col] = true;
    return INFX_OK;
}
// the raw values of a column's codes for infx_field_stats, with the scale and width the caller found for them (exact_sum.h)
int32_t infx_upload_column_values(infx_index* ix, uint32_t col, uint32_t num_values, const uint64_t* bits, int32_t kind, int32_t scale_exp, uint32_t nlimbs) {
    if (!ix || col >= FILT_MAXCOL || (num_values && !bits)) return fail(INFX_EINVAL, "bad column-value arguments%s");
    if (!ix->colCodes[col] || num_values != ix->colValues[col]) return fail(INFX_EINVAL, "a value table needs one entry per distinct value of an uploaded column%s");
    if ((kind != XS_KIND_INT && kind != XS_KIND_DOUBLE) || nlimbs < 1 || nlimbs > (kind == XS_KIND_INT ? 2u : (uint32_t)XS_MAX_LIMBS) || (kind == XS_KIND_INT && scale_exp != 0) || scale_exp < -1074 || scale_exp > 1023)
        return fail(INFX_EINVAL, "a value table is int64 (kind 1, scale 0, 1 .. 2 limbs) or double (kind 2, scale -1074 .. 1023, 1 .. 4 limbs)%s");
    {   // the scale and width must be the table's own: the kernel relies on no value shifting a set bit out of nlimbs limbs
        XsScale sc; const bool ok = xs_column_scale(bits, num_values, kind, &sc);
        if (!ok || sc.scale != scale_exp || sc.nlimbs != nlimbs) return fail(INFX_EINVAL, "scale_exp and nlimbs are not the scale and width of the values%s");
    }
    HIPCHK(enter_device(ix->cfg.device));
    HIPCHK(hipDeviceSynchronize());                      // exclusive call, as infx_upload_column
    uint64_t* d = const_cast<uint64_t*>(ix->colBits[col]);
    if (!d || ix->colBitsCap[col] < num_values) { HIPCHK(dalloc(ix, &d, (size_t)num_values)); ix->colBitsCap[col] = num_values; }
    if (num_values) HIPCHK(hipMemcpy(d, bits, (size_t)num_values * 8, hipMemcpyHostToDevice));
    ix->colBits[col] = d; ix->colKind[col] = kind; ix->colScale[col] = scale_exp; ix->colLimbs[col] = nlimbs; ix->colBitsOk[col] = true;
    return INFX_OK;
}
int32_t infx_stream_set_boosts(infx_stream* s, uint32_t n, infx_filter* const* f, const int32_t* strengths) {
    if (!s || (n && (!f || !strengths))) return fail(INFX_EINVAL, "bad boost arguments%s");
    uint32_t m = 0;
    for (uint32_t i = 0; i < n; i++) if (f[i]) { if (f[i]->ix != s->ix) return fail(INFX_EINVAL, "a boost filter belongs to another index%s"); m++; }
    if (m > INFX_MAX_BOOSTS) return fail(INFX_ECAPACITY, "more than INFX_MAX_BOOSTS boosts with a filter%s");
    if (m) { int32_t rc_ = columns_cover(s->ix, s->ix->d.totalDocs, COLS_COVER_CORPUS); if (rc_) return rc_; }      // rows carry GLOBAL internal ids
    if (s->qpOn && m) return fail(INFX_EINVAL, "per-query options are installed on this stream%s");
    s->nBoost = 0;
    for (uint32_t i = 0; i < n; i++) if (f[i]) { s->boosts[s->nBoost] = f[i]; s->boostStrength[s->nBoost] = strengths[i]; s->nBoost++; }
    for (uint32_t i = s->nBoost; i < INFX_MAX_BOOSTS; i++) { s->boosts[i] = nullptr; s->boostStrength[i] = 0; }
    return INFX_OK;
}
int32_t infx_stream_set_sort(infx_stream* s, uint32_t col, int32_t ascending, int32_t enabled) {
    if (!s) return fail(INFX_EINVAL, "null argument%s");
    if (enabled && col != 0xFFFFFFFFu) {
        if (col >= FILT_MAXCOL || !s->ix->colCodes[col] || !s->ix->colRankOk[col]) return fail(INFX_EINVAL, "sort column or its rank was not uploaded%s");
        { int32_t rc_ = columns_cover(s->ix, s->ix->d.totalDocs, COLS_COVER_CORPUS, (int)col); if (rc_) return rc_; }
    }
    if (s->qpOn && enabled) return fail(INFX_EINVAL, "per-query options are installed on this stream%s");
    s->sortOn = enabled != 0; s->sortCol = enabled ? col : 0; s->sortAsc = enabled && ascending != 0;
    return INFX_OK;
}
// ---- per-query post-processing (k_postfilter / k_postproc with one descriptor per query) + k_filter_count_multi ----------------------------------
int32_t infx_stream_set_query_post(infx_stream* s, uint32_t nq, uint32_t nprog, const infx_filter_prog* progs, uint32_t nboost, const infx_query_boost* boosts,
                                   const infx_query_post* post, uint32_t nfacet, const uint32_t* facet_cols, uint32_t ncount, uint32_t* counts_out) {
    if (!s) return fail(INFX_EINVAL, "null argument%s");
    s->qpOn = false; s->lastCountK = 0; s->lastCountLaunches = 0;      // the count stats are set again only by the finalize that consumes these options
    if (nq == 0) return INFX_OK;
    if (!post || (nprog && !progs) || (nboost && !boosts) || nfacet > INFX_MAX_FACET_COLS || (nfacet && !facet_cols) || ncount > nprog || (ncount && !counts_out))
        return fail(INFX_EINVAL, "bad per-query post-processing arguments%s");
    if (s->postFilter || s->nFacet || s->nBoost || s->sortOn) return fail(INFX_EINVAL, "per-query options and a session-wide post-filter, facets, boosts or sort exclude each other%s");
    infx_index* ix = s->ix;
    for (uint32_t c = 0; c < nfacet; c++) if (facet_cols[c] >= FILT_MAXCOL || !ix->colCodes[facet_cols[c]]) return fail(INFX_EINVAL, "facet column was not uploaded%s");
    { int32_t rc_ = columns_cover(ix, ix->d.totalDocs, COLS_COVER_CORPUS); if (rc_) return rc_; }      // rows carry GLOBAL internal ids and the counts run over the whole corpus
    for (uint32_t b = 0; b < nboost; b++) if (boosts[b].prog < 0 || (uint32_t)boosts[b].prog >= nprog) return fail(INFX_EINVAL, "boost program index out of range%s");
    for (uint32_t q = 0; q < nq; q++) {
        const infx_query_post& D = post[q];
        if (D.filter >= 0 && (uint32_t)D.filter >= nprog) return fail(INFX_EINVAL, "filter program index out of range%s");
        if (D.nboost > INFX_MAX_BOOSTS || (uint64_t)D.boost_off + D.nboost > nboost) return fail(INFX_EINVAL, "boost list out of range%s");
        if ((D.flags & INFX_QP_SORT) && D.sort_col != 0xFFFFFFFFu && (D.sort_col >= FILT_MAXCOL || !ix->colCodes[D.sort_col] || !ix->colRankOk[D.sort_col]))
            return fail(INFX_EINVAL, "sort column or its rank was not uploaded%s");
        if (D.flags & ~(uint32_t)(INFX_QP_FACETS | INFX_QP_SORT | INFX_QP_ASC)) return fail(INFX_EINVAL, "unknown per-query flag%s");
    }
    { int32_t rc_ = s->qpTable.pack(ix, nprog, progs); if (rc_) return rc_; }
    s->qpBoosts.resize(nboost); for (uint32_t b = 0; b < nboost; b++) s->qpBoosts[b] = DevQBoost{boosts[b].prog, boosts[b].strength};
    s->qpDesc.resize(nq);
    for (uint32_t q = 0; q < nq; q++) {
        const infx_query_post& D = post[q]; DevQPost& E = s->qpDesc[q];
        E = DevQPost{}; E.filter = D.filter < 0 ? -1 : D.filter; E.flags = D.flags; E.sortCol = (D.flags & INFX_QP_SORT) ? D.sort_col : 0u; E.boostOff = D.boost_off; E.nboost = D.nboost;
    }
    s->qpNq = nq; s->qpNFacet = nfacet; s->qpNCount = ncount; s->qpCountsOut = counts_out;
    for (uint32_t c = 0; c < INFX_MAX_FACET_COLS; c++) s->qpFacetCols[c] = c < nfacet ? facet_cols[c] : 0;
    s->qpOn = true;
    return INFX_OK;
}
int32_t infx_filter_count_progs(infx_stream* s, uint32_t k, const infx_filter_prog* progs, int32_t whole_corpus, uint32_t* counts) {
    if (!s || (k && (!progs || !counts))) return fail(INFX_EINVAL, "null argument%s");
    infx_index* ix = s->ix;
    if (!ix->haveDocs) return fail(INFX_EINVAL, "index not uploaded%s");
    if (!k) return INFX_OK;
    HIPCHK(enter_device(ix->cfg.device));
    { int32_t rc_ = pin_reset(s); if (rc_) return rc_; }
    ProgTable T;
    { int32_t rc_ = T.pack(ix, k, progs); if (rc_) return rc_; }
    { int32_t rc_ = table_upload(s, T, &s->dPostBlob, &s->capPostBlob); if (rc_) return rc_; }
    GROW(s->dQCount, s->capQCount, (size_t)k * 4);
    const int32_t base = whole_corpus ? 0 : ix->d.docBase, n = whole_corpus ? ix->d.totalDocs : ix->d.N;
    { int32_t rc_ = count_enqueue(s, (const DevFilter*)s->dPostBlob, k, T.columns(0, k), base, n, (uint32_t*)s->dQCount); if (rc_) return rc_; }
    DOWN(counts, s->dQCount, (size_t)k * 4);
    SYNC();
    return INFX_OK;
}
// ---- Query.collapse_by (k_collapse) --------------------------------------------------------------------------------------------------------------------
int32_t infx_stream_set_query_collapse(infx_stream* s, uint32_t nq, const infx_collapse_req* reqs) {
    if (!s || (nq && !reqs)) return fail(INFX_EINVAL, "null argument%s");
    s->clpOn = nq > 0; s->clpReq.assign(reqs, reqs + nq);
    return INFX_OK;
}
int32_t infx_last_collapse(infx_stream* s, uint32_t nq, uint32_t* total_groups, uint32_t* total_ranked) {
    if (!s || (nq && (!total_groups || !total_ranked))) return fail(INFX_EINVAL, "null argument%s");
    if (nq != s->clpSlot.size()) return fail(INFX_EINVAL, "no batch of this size with a collapsing query on the stream%s");
    for (uint32_t q = 0; q < nq; q++) { const int32_t k = s->clpSlot[q]; total_groups[q] = k < 0 ? 0 : s->clpGroups[k]; total_ranked[q] = k < 0 ? 0 : s->clpRanked[k]; }
    return INFX_OK;
}
// The rows of query qi as the batch returned them: each row's group code and the size of its group in the ranked list; returns the rows written, -1 on error.
// k_postfilter only drops rows and k_postproc only reorders them, and the documents of a consolidated list are distinct: a returned row is the row k_collapse
// wrote with the same document.
int32_t infx_collapse_rows(infx_stream* s, uint32_t qi, uint32_t* codes, uint32_t* sizes, int32_t cap) {
    if (!s || qi >= s->clpSlot.size() || s->clpSlot[qi] < 0 || cap < 0 || (cap && (!codes || !sizes))) { fail(INFX_EINVAL, "no collapsing query of this index in the stream's last batch%s"); return -1; }
    const size_t r = (size_t)s->clpSlot[qi] * s->clpStride, o = (size_t)qi * s->clpStride;
    const uint32_t n = std::min(std::min(s->clpCounts[qi], s->clpStride), (uint32_t)cap);
    if (!s->clpPosted) { for (uint32_t i = 0; i < n; i++) { codes[i] = s->clpCodes[r + i]; sizes[i] = s->clpSizes[r + i]; } return (int32_t)n; }
    const uint32_t wrote = std::min(s->clpReturned[s->clpSlot[qi]], s->clpStride);
    std::vector<std::pair<int32_t, uint32_t>> byDoc(wrote);      // (document, row k_collapse wrote)
    for (uint32_t i = 0; i < wrote; i++) byDoc[i] = {s->clpDocs[r + i], i};
    std::sort(byDoc.begin(), byDoc.end());
    for (uint32_t i = 0; i < n; i++) {
        const int32_t d = s->clpFinalDocs[o + i];
        auto it = std::lower_bound(byDoc.begin(), byDoc.end(), std::make_pair(d, 0u));
        if (it == byDoc.end() || it->first != d) { fail(INFX_EINVAL, "a returned row is not one the collapse step wrote%s"); return -1; }
        codes[i] = s->clpCodes[r + it->second]; sizes[i] = s->clpSizes[r + it->second];
    }
    return (int32_t)n;
}
int32_t infx_last_collapse_stats(infx_stream* s, uint32_t* queries, uint32_t* launches) {
    if (!s) return fail(INFX_EINVAL, "null argument%s");
    if (queries) *queries = s->lastClpQueries; if (launches) *launches = s->lastClpLaunches;
    return INFX_OK;
}
int32_t infx_last_collapse_timings(infx_stream* s, float* ms2) {
    if (!s || !ms2) return fail(INFX_EINVAL, "null argument%s");
    ms2[0] = ms2[1] = 0.f;
    if (s->timedClp) { hipEventElapsedTime(&ms2[0], s->evF0, s->evK0); hipEventElapsedTime(&ms2[1], s->evK0, s->evK1); }
    return INFX_OK;
}
// ---- Query.highlight (k_highlight) -----------------------------------------------------------------------------------------------------------------------
int32_t infx_stream_set_query_highlight(infx_stream* s, uint32_t nq, const int32_t* chars) {
    if (!s || (nq && !chars)) return fail(INFX_EINVAL, "null argument%s");
    s->hlOn = nq > 0; s->hlReq.assign(chars, chars + nq); s->hlWords.clear();
    return INFX_OK;
}
int32_t infx_highlight_layout(infx_stream* s, uint32_t qi, int32_t* rows, int32_t* term_stride, int32_t* snippet_stride) {
    if (!s || qi >= s->hlSlot.size() || s->hlSlot[qi] < 0) return fail(INFX_EINVAL, "no highlighting query of this index in the stream's last batch%s");
    if (rows) *rows = (int32_t)std::min(s->hlCounts[qi], s->hlStride);
    if (term_stride) *term_stride = (int32_t)s->hlTermStride;
    if (snippet_stride) *snippet_stride = (int32_t)s->hlSnipStride;
    return INFX_OK;
}
// Query qi's rows as the batch returned them, hl_row_u16(term stride, snippet stride) uint16 each (csrc/highlight.h); returns the rows written, -1 on error
int32_t infx_highlight_rows(infx_stream* s, uint32_t qi, uint16_t* out, int64_t cap_u16) {
    if (!s || qi >= s->hlSlot.size() || s->hlSlot[qi] < 0 || cap_u16 < 0 || (cap_u16 && !out)) { fail(INFX_EINVAL, "no highlighting query of this index in the stream's last batch%s"); return -1; }
    const size_t rowU16 = hl_row_u16(s->hlTermStride, s->hlSnipStride);
    const uint32_t n = (uint32_t)std::min<uint64_t>(std::min(s->hlCounts[qi], s->hlStride), (uint64_t)cap_u16 / rowU16);
    const uint16_t* src = s->hlRows.data() + (size_t)s->hlSlot[qi] * s->hlStride * rowU16;
    for (uint32_t r = 0; r < n; r++) if (src[(size_t)r * rowU16] == HL_BAD_ROW) { fail(INFX_EINVAL, "a returned row's document is not one of the index%s"); return -1; }
    std::memcpy(out, src, (size_t)n * rowU16 * 2);
    return (int32_t)n;
}
int32_t infx_last_highlight_stats(infx_stream* s, uint32_t* queries, uint32_t* launches) {
    if (!s) return fail(INFX_EINVAL, "null argument%s");
    if (queries) *queries = s->lastHlQueries; if (launches) *launches = s->lastHlLaunches;
    return INFX_OK;
}
int32_t infx_last_highlight_timings(infx_stream* s, float* ms, uint64_t* bytes) {
    if (!s || !ms) return fail(INFX_EINVAL, "null argument%s");
    *ms = 0.f; if (bytes) *bytes = s->lastHlBytes;
    if (s->timedHl) hipEventElapsedTime(ms, s->evH0, s->evH1);
    return INFX_OK;
}
int32_t infx_last_browse_stats(infx_stream* s, uint32_t* groups, uint32_t* launches) {
    if (!s) return fail(INFX_EINVAL, "null argument%s");
    if (groups) *groups = s->lastBrowseGroups;
    if (launches) *launches = s->lastBrowseLaunches;
    return INFX_OK;
}
// FacetBuilder.BuildFacetsFromAllDocuments: counts_out = for each of the ncol columns in turn, one count per distinct value (the column's num_values)
int32_t infx_facets_all(infx_stream* s, uint32_t ncol, const uint32_t* cols, uint32_t* counts_out) {
    if (!s || ncol > INFX_MAX_FACET_COLS || (ncol && (!cols || !counts_out))) return fail(INFX_EINVAL, "bad facet arguments%s");
    infx_index* ix = s->ix;
    if (!ix->haveDocs) return fail(INFX_EINVAL, "index not uploaded%s");
    if (!ncol) return INFX_OK;
    const int32_t n = ix->d.totalDocs;
    DevFacetAll F{}; size_t total = 0; uint32_t ldsWords = 0;
    for (uint32_t c = 0; c < ncol; c++) {
        if (cols[c] >= FILT_MAXCOL || !ix->colCodes[cols[c]]) return fail(INFX_EINVAL, "facet column was not uploaded%s");
        { int32_t rc_ = columns_cover(ix, n, COLS_COVER_CORPUS, (int)cols[c]); if (rc_) return rc_; }
        total += ix->colValues[cols[c]];
    }
    HIPCHK(enter_device(ix->cfg.device));
    { int32_t rc_ = pin_reset(s); if (rc_) return rc_; }
    GROW(s->dFacAll, s->capFacAll, std::max<size_t>(total, 1) * 4);
    HIPCHK(hipMemsetAsync(s->dFacAll, 0, std::max<size_t>(total, 1) * 4, s->st));
    size_t o = 0;
    for (uint32_t c = 0; c < ncol; c++) {
        const uint32_t nv = ix->colValues[cols[c]];
        F.codes[c] = ix->colCodes[cols[c]]; F.out[c] = (uint32_t*)s->dFacAll + o; F.nvals[c] = nv; o += nv;
        // LDS counters for the small dictionaries, within 64 KiB per workgroup in all (two workgroups per CU stay resident)
        if (nv <= FALL_LDS_VALUES && ldsWords + nv <= 16384u) { F.ldsOff[c] = ldsWords; ldsWords += nv; } else F.ldsOff[c] = 0xFFFFFFFFu;
    }
    if (n > 0) {
        const int grid = (int)std::min<int64_t>(2048, ((int64_t)n + FALL_THREADS - 1) / FALL_THREADS);
        k_facets_all<<<grid, FALL_THREADS, (size_t)ldsWords * 4, s->st>>>(F, (int)ncol, ldsWords, n, ix->d.deleted);
        HIPCHK(hipGetLastError());
    }
    if (total) DOWN(counts_out, s->dFacAll, total * 4);
    SYNC();
    return INFX_OK;
}
// ---- facets of the documents a filter accepts (k_facets_filtered) ----
// Where the counters of one launch live.  The LDS budget is k_facets_all's: FFL_LDS_WORDS words per workgroup, and a column of more than FALL_LDS_VALUES
// values always counts in global memory.  Contention decides the rest: the fewer values a column has, the more adds meet on one counter, so
//   1. a column of at most FFL_HOT_VALUES values is ALWAYS counted in LDS: the programs of a call are spread evenly over as many launches as it takes
//      for (programs of a launch) x (words of those columns) to fit (8 such columns hold at most 2048 words: a launch always takes 8 programs or more);
//   2. the other columns of at most FALL_LDS_VALUES values get LDS counters in ascending order of their size while (programs of the launch) x words
//      still fits, and global counters after that.
#define FFL_LDS_WORDS 16384u
#define FFL_HOT_VALUES 256u
#define FFL_CU_LDS ((size_t)160 * 1024)      // LDS of a CU (gfx950)
static uint32_t ffl_programs_per_launch(uint32_t K, uint32_t ncol, const uint32_t* nv) {
    uint32_t hot = 0; for (uint32_t c = 0; c < ncol; c++) if (nv[c] <= FFL_HOT_VALUES) hot += nv[c];
    const uint32_t fit = hot ? std::max(1u, FFL_LDS_WORDS / hot) : K;
    if (!K || fit >= K) return K;
    const uint32_t launches = (K + fit - 1) / fit;
    return (K + launches - 1) / launches;
}
static uint32_t ffl_place(uint32_t k, uint32_t ncol, const uint32_t* nv, uint32_t* ldsOff) {      // returns the LDS words of the facet counters
    uint32_t order[INFX_MAX_FACET_COLS]; for (uint32_t c = 0; c < ncol; c++) order[c] = c;
    std::stable_sort(order, order + ncol, [&](uint32_t a, uint32_t b) { return nv[a] < nv[b]; });
    uint32_t words = 0;
    for (uint32_t i = 0; i < ncol; i++) {
        const uint32_t c = order[i]; const uint64_t w = (uint64_t)k * nv[c];
        if (nv[c] && nv[c] <= FALL_LDS_VALUES && words + w <= FFL_LDS_WORDS) { ldsOff[c] = words; words += (uint32_t)w; } else ldsOff[c] = 0xFFFFFFFFu;
    }
    return words;
}
int32_t infx_facets_filtered(infx_stream* s, uint32_t k, const infx_filter_prog* progs, uint32_t ncol, const uint32_t* cols, uint32_t* counts_out, uint32_t* totals_out) {
    if (!s || ncol > INFX_MAX_FACET_COLS || (ncol && !cols) || (k && (!progs || !totals_out))) return fail(INFX_EINVAL, "bad filtered-facet arguments%s");
    s->lastFfProgs = 0; s->lastFfLaunches = 0;
    if (!k) return INFX_OK;
    if (k > INFX_MAX_PREFILTERS) return fail(INFX_ECAPACITY, "more than INFX_MAX_PREFILTERS (16) programs in one call%s");
    infx_index* ix = s->ix;
    if (!ix->haveDocs) return fail(INFX_EINVAL, "index not uploaded%s");
    const int32_t n = ix->d.totalDocs;
    uint64_t total = 0; uint32_t nv[INFX_MAX_FACET_COLS] = {};
    for (uint32_t c = 0; c < ncol; c++) {
        if (cols[c] >= FILT_MAXCOL || !ix->colCodes[cols[c]]) return fail(INFX_EINVAL, "facet column was not uploaded%s");
        nv[c] = ix->colValues[cols[c]]; total += nv[c];
    }
    { int32_t rc_ = columns_cover(ix, n, COLS_COVER_CORPUS); if (rc_) return rc_; }      // the programs may read any uploaded column
    if (total && !counts_out) return fail(INFX_EINVAL, "bad filtered-facet arguments%s");
    if (total > 0xFFFFFFFFull / INFX_MAX_PREFILTERS) return fail(INFX_ECAPACITY, "the facet columns hold too many distinct values%s");
    HIPCHK(enter_device(ix->cfg.device));
    { int32_t rc_ = pin_reset(s); if (rc_) return rc_; }
    ProgTable T;
    { int32_t rc_ = T.pack(ix, k, progs); if (rc_) return rc_; }      // (validates every program against the uploaded columns)
    const size_t words = (size_t)k * (size_t)total + k;                                  // counters [k][total], then totals [k]
    { int32_t rc_ = table_upload(s, T, &s->dFfBlob, &s->capFfBlob); if (rc_) return rc_; }
    GROW(s->dFfCnt, s->capFfCnt, words * 4);
    HIPCHK(hipMemsetAsync(s->dFfCnt, 0, words * 4, s->st));
    uint32_t* dOut = (uint32_t*)s->dFfCnt; uint32_t* dTot = dOut + (size_t)k * (size_t)total;
    s->lastFfProgs = k;
    if (n > 0) {
        const DevColumns dc = dev_columns(ix);
        const uint32_t per = ffl_programs_per_launch(k, ncol, nv);
        for (uint32_t k0 = 0; k0 < k; k0 += per) {
            const uint32_t kk = std::min(per, k - k0);
            const DevCountCols cc = T.columns(k0, kk);
            DevFacetFilt F{}; uint32_t o = 0;
            const uint32_t ldsWords = ffl_place(kk, ncol, nv, F.ldsOff);
            for (uint32_t c = 0; c < ncol; c++) {
                F.codes[c] = ix->colCodes[cols[c]]; F.nvals[c] = nv[c]; F.outOff[c] = o; o += nv[c];
                F.slot[c] = 0xFFu; for (uint32_t u = 0; u < cc.nUsed; u++) if (cc.col[u] == cols[c]) F.slot[c] = (uint8_t)u;
            }
            // 256 threads while the codes of a workgroup stay within 16 KiB, else one wave per workgroup.  Counters beyond 16 KiB change the shape (measured,
            // profiles/filtered_facets.md: at 80 KiB per workgroup two 256-thread workgroups fit a CU, 2 waves per SIMD, and each of 2048 workgroups merges its
            // counters into global memory): then one workgroup of FFL_BIG_THREADS threads per CU-sized share of LDS and only as many workgroups as are resident
            const bool big = (size_t)ldsWords * 4 > 16 * 1024 && ((size_t)cc.nUsed * 4 * FFL_BIG_THREADS + kk + ldsWords) * 4 <= FFL_CU_LDS;
            const int threads = big ? FFL_BIG_THREADS : (size_t)cc.nUsed * 4 * FMM_THREADS * 4 <= 16 * 1024 ? FMM_THREADS : WAVE;
            const size_t lds = ((size_t)cc.nUsed * 4 * threads + kk + ldsWords) * 4;
            const int64_t groups = ((int64_t)n + 3) / 4;
            int64_t maxGrid = FCM_MAXGRID;
            if (big) { int cus = 0; HIPCHK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, ix->cfg.device)); maxGrid = std::max<int64_t>(1, (int64_t)cus * (int64_t)(FFL_CU_LDS / lds)); }
            const int grid = (int)std::min<int64_t>(maxGrid, (groups + threads - 1) / threads);
            HIPCHK(lds_limit((const void*)k_facets_filtered, ix->cfg.device, lds));
            k_facets_filtered<<<grid, threads, lds, s->st>>>((const DevFilter*)s->dFfBlob + k0, kk, cc, dc, n, ix->d.deleted, F, (int)ncol, ldsWords, (uint32_t)total,
                                                            dOut + (size_t)k0 * (size_t)total, dTot + k0);
            HIPCHK(hipGetLastError());
            s->lastFfLaunches++;
        }
    }
    if (total) DOWN(counts_out, dOut, (size_t)k * (size_t)total * 4);
    DOWN(totals_out, dTot, (size_t)k * 4);
    SYNC();
    return INFX_OK;
}
int32_t infx_last_facets_filtered_stats(infx_stream* s, uint32_t* programs, uint32_t* launches) {
    if (!s) return fail(INFX_EINVAL, "null argument%s");
    if (programs) *programs = s->lastFfProgs;
    if (launches) *launches = s->lastFfLaunches;
    return INFX_OK;
}
// ---- list columns (list_columns.hip.inc) ----
int32_t infx_upload_list_column(infx_index* ix, uint32_t lcol, uint32_t total_docs, const uint32_t* elem_off, const uint32_t* elem_codes, uint32_t num_values) {
    if (!ix || lcol >= INFX_MAX_LIST_COLS || (total_docs && !elem_off)) return fail(INFX_EINVAL, "bad list-column arguments%s");
    if (ix->nranks > 1) return fail(INFX_EUNSUPPORTED, "list columns need an index that is not sharded%s");
    HIPCHK(enter_device(ix->cfg.device));
    HIPCHK(hipDeviceSynchronize());                      // exclusive call, as infx_upload_column
    if (!total_docs) { ix->listDocs[lcol] = 0; ix->listValues[lcol] = 0; return INFX_OK; }      // dropped (its buffers are kept for the next upload)
    if (ix->haveDocs && (uint64_t)total_docs != (uint64_t)ix->d.totalDocs) return fail(INFX_EINVAL, "a list column needs one list per document%s");
    if (elem_off[0] != 0) return fail(INFX_EINVAL, "a list column's offsets start at 0%s");
    for (uint32_t d = 0; d < total_docs; d++) if (elem_off[d + 1] < elem_off[d]) return fail(INFX_EINVAL, "a list column's offsets must ascend%s");
    const size_t total = elem_off[total_docs];
    if (total && !elem_codes) return fail(INFX_EINVAL, "bad list-column arguments%s");
    for (size_t i = 0; i < total; i++) if (elem_codes[i] >= num_values) return fail(INFX_EINVAL, "a list column's element code is out of range%s");
    uint32_t* dOff = const_cast<uint32_t*>(ix->listOff[lcol]); uint32_t* dCode = const_cast<uint32_t*>(ix->listCode[lcol]);
    ix->listDocs[lcol] = 0;                              // (not uploaded while a step below can fail)
    if (!dOff || ix->listOffCap[lcol] < (size_t)total_docs + 1) { HIPCHK(dalloc(ix, &dOff, (size_t)total_docs + 1)); ix->listOff[lcol] = dOff; ix->listOffCap[lcol] = (size_t)total_docs + 1; }
    if (!dCode || ix->listCodeCap[lcol] < total) { HIPCHK(dalloc(ix, &dCode, total)); ix->listCode[lcol] = dCode; ix->listCodeCap[lcol] = std::max<size_t>(total, 1); }
    HIPCHK(hipMemcpy(dOff, elem_off, ((size_t)total_docs + 1) * 4, hipMemcpyHostToDevice));
    if (total) HIPCHK(hipMemcpy(dCode, elem_codes, total * 4, hipMemcpyHostToDevice));
    ix->listDocs[lcol] = total_docs; ix->listValues[lcol] = num_values;
    return INFX_OK;
}
int32_t infx_list_leaf_build(infx_index* ix, uint32_t lcol, uint32_t k, const uint32_t* slots, const uint32_t* maps, uint32_t empty_bits) {
    if (!ix || lcol >= INFX_MAX_LIST_COLS || !k || k > INFX_LIST_LEAF_MAX || !slots || !maps) return fail(INFX_EINVAL, "bad list-leaf arguments%s");
    const uint32_t n = ix->listDocs[lcol], nv = ix->listValues[lcol];
    if (!n || !ix->haveDocs || (int64_t)n != (int64_t)ix->d.totalDocs) return fail(INFX_EINVAL, "the list column was not uploaded%s");
    for (uint32_t i = 0; i < k; i++) {
        if (slots[i] >= FILT_MAXCOL) return fail(INFX_EINVAL, "a derived column's slot is out of range%s");
        for (uint32_t j = 0; j < i; j++) if (slots[j] == slots[i]) return fail(INFX_EINVAL, "two derived columns share a slot%s");
    }
    HIPCHK(enter_device(ix->cfg.device));
    HIPCHK(hipDeviceSynchronize());                      // nothing in flight reads a slot that is rewritten
    const size_t mapWords = (size_t)((nv + 31u) / 32u) * k;
    if (!ix->listMaps || ix->listMapsCap < mapWords) { uint32_t* m = nullptr; HIPCHK(dalloc(ix, &m, mapWords)); ix->listMaps = m; ix->listMapsCap = std::max<size_t>(mapWords, 1); }
    if (mapWords) HIPCHK(hipMemcpy(ix->listMaps, maps, mapWords * 4, hipMemcpyHostToDevice));
    DevListLeaf A{}; A.elemOff = ix->listOff[lcol]; A.elemCode = ix->listCode[lcol]; A.maps = ix->listMaps;
    A.K = k; A.nvals = nv; A.emptyBits = empty_bits; A.mapsInLds = mapWords <= INFX_LIST_LEAF_LDS_WORDS ? 1u : 0u; A.n = (int32_t)n;
    // Other sessions read the column table (columns_cover, dev_columns) without a lock while this runs: a slot is never published half built.  A slot
    // that already holds a buffer of n rows keeps its table entries and only gets new contents (its callers made sure no program in use reads it); a
    // slot without one gets its buffer here and enters the table only after the kernel has completed, the pointer last.
    uint32_t* fresh[INFX_LIST_LEAF_MAX] = {};
    for (uint32_t i = 0; i < k; i++) {
        const uint32_t c = slots[i];
        uint32_t* d = const_cast<uint32_t*>(ix->colCodes[c]);
        if (!d || ix->colCap[c] < n || ix->colDocs[c] != n) { d = nullptr; HIPCHK(dalloc(ix, &d, (size_t)n + 1)); fresh[i] = d; }      // (a failure leaves the table as it was; the buffer is the index's to free)
        A.out[i] = d;
    }
    const int grid = (int)std::min<int64_t>(LL_MAXGRID, ((int64_t)n + LL_DOCS - 1) / LL_DOCS);
    k_list_leaf<<<grid, LL_THREADS, 0, 0>>>(A);
    HIPCHK(hipGetLastError());
    HIPCHK(hipDeviceSynchronize());
    for (uint32_t i = 0; i < k; i++) {
        const uint32_t c = slots[i];
        if (ix->colRankOk[c]) ix->colRankOk[c] = false; if (ix->colBitsOk[c]) ix->colBitsOk[c] = false; if (ix->colTieOk[c]) ix->colTieOk[c] = false;
        if (ix->colValues[c] != 2) ix->colValues[c] = 2;
        if (fresh[i]) {
            ix->colCap[c] = n; ix->colDocs[c] = n;
            __atomic_thread_fence(__ATOMIC_RELEASE);
            ix->colCodes[c] = fresh[i];
        }
    }
    return INFX_OK;
}
int32_t infx_list_facets(infx_stream* s, uint32_t lcol, uint32_t k, const uint8_t* const* masks, uint32_t* counts_out) {
    if (!s || lcol >= INFX_MAX_LIST_COLS || !k || k > INFX_MAX_PREFILTERS || !masks) return fail(INFX_EINVAL, "bad list-facet arguments%s");
    infx_index* ix = s->ix;
    const uint32_t n = ix->listDocs[lcol], nv = ix->listValues[lcol];
    if (!n || !ix->haveDocs || (int64_t)n != (int64_t)ix->d.totalDocs) return fail(INFX_EINVAL, "the list column was not uploaded%s");
    if (nv && !counts_out) return fail(INFX_EINVAL, "bad list-facet arguments%s");
    if ((uint64_t)nv * k > 0xFFFFFFFFull / 4) return fail(INFX_ECAPACITY, "the list column holds too many distinct values%s");
    for (uint32_t i = 0; i < k; i++) if (masks[i]) { const int slot = mask_slot_of(s, masks[i]); if (slot < 0 || s->capMask[slot] < mask_bytes(ix)) return fail(INFX_EINVAL, "a list-facet mask is not a mask slot of this stream%s"); }
    if (!nv) return INFX_OK;
    HIPCHK(enter_device(ix->cfg.device));
    { int32_t rc_ = pin_reset(s); if (rc_) return rc_; }
    const size_t words = (size_t)k * nv;
    GROW(s->dLfCnt, s->capLfCnt, words * 4);
    HIPCHK(hipMemsetAsync(s->dLfCnt, 0, words * 4, s->st));
    DevListFacets A{}; A.elemOff = ix->listOff[lcol]; A.elemCode = ix->listCode[lcol]; A.out = (uint32_t*)s->dLfCnt;
    A.K = k; A.nvals = nv; A.inLds = words <= FFL_LDS_WORDS ? 1u : 0u; A.n = (int32_t)n;
    for (uint32_t i = 0; i < k; i++) A.mask[i] = masks[i] ? masks[i] : ix->d.deleted;
    const size_t lds = ((size_t)2 * LL_DOCS + 1 + (A.inLds ? words : 0)) * 4;
    // counters beyond 16 KiB: fewer, longer-lived workgroups (each merges its counters once), two per CU's share of LDS
    const int64_t maxGrid = lds > 16 * 1024 ? 512 : LL_MAXGRID;
    const int grid = (int)std::min<int64_t>(maxGrid, ((int64_t)n + LL_DOCS - 1) / LL_DOCS);
    HIPCHK(lds_limit((const void*)k_list_facets, ix->cfg.device, lds));
    k_list_facets<<<grid, LL_THREADS, lds, s->st>>>(A);
    HIPCHK(hipGetLastError());
    DOWN(counts_out, s->dLfCnt, words * 4);
    SYNC();
    return INFX_OK;
}
// ---- requests over document sets: a mask (null: every live document) and a column read through its sort rank ----
// What infx_list_ordered and infx_range_counts ask of one request before anything is enqueued: the column uploaded with its sort rank and covering the corpus
// (col < 0, a set in document order, only where !needCol), the mask a slot of this stream and large enough.  `what` names the request in the messages.
static int32_t check_set_request(const infx_stream* s, const uint8_t* mask, int32_t col, bool needCol, const char* what) {
    const infx_index* ix = s->ix;
    if (col >= 0 || needCol) {
        if (col < 0 || col >= FILT_MAXCOL || !ix->colCodes[col] || !ix->colRankOk[col]) return fail(INFX_EINVAL, "the %s's column or its sort rank was not uploaded", what);
        int32_t rc_ = columns_cover(ix, ix->d.totalDocs, COLS_COVER_CORPUS, col); if (rc_) return rc_;
    }
    if (mask) { const int slot = mask_slot_of(s, mask); if (slot < 0 || s->capMask[slot] < mask_bytes(ix)) return fail(INFX_EINVAL, "a %s's mask is not a mask slot of this stream, or was made for a smaller corpus", what); }
    return INFX_OK;
}
// a group column (field_stats, list_groups): uploaded and covering the corpus
static int32_t check_group_column(const infx_index* ix, int32_t col, const char* what) {
    if (col < 0 || col >= FILT_MAXCOL || !ix->colCodes[col]) return fail(INFX_EINVAL, "the %s's group column was not uploaded", what);
    return columns_cover(ix, ix->d.totalDocs, COLS_COVER_CORPUS, col);
}
// the group column of a call that keeps one slot per group: as above, with at most STS_MAX_GROUPS values
static int32_t check_group_slots(const infx_index* ix, int32_t col, const char* what) {
    { int32_t rc_ = check_group_column(ix, col, what); if (rc_) return rc_; }
    if (ix->colValues[col] > STS_MAX_GROUPS) return fail(INFX_EINVAL, "a group column has at most INFX_STATS_MAX_GROUPS (4096) values%s");
    return INFX_OK;
}
struct SetKey { const uint8_t* mask; int32_t col, gcol; };      // what the device's order of a call's requests looks at (gcol: -1 throughout a call without groups)
// order[]: the requests so that the ones that share a mask follow one another, among them the ones that share a value column, among those the ones that share
// a group column — the walk keeps what the request before loaded — and the others in the caller's order
static void set_order(uint32_t nreq, const SetKey* key, uint32_t* order) {
    for (uint32_t i = 0; i < nreq; i++) order[i] = i;
    std::stable_sort(order, order + nreq, [&](uint32_t a, uint32_t b) {
        const SetKey &A = key[a], &B = key[b];
        return A.mask != B.mask ? std::less<const uint8_t*>()(A.mask, B.mask) : A.col != B.col ? A.col < B.col : A.gcol < B.gcol; });
}
// what request Q keeps of B, the one before it in that order: 1 the mask's flags, 3 the value column's ranks as well
static uint32_t set_reuse(const SetKey& B, const SetKey& Q) { return B.mask == Q.mask ? (B.col == Q.col ? 3u : 1u) : 0u; }
// The frame of a set call.  What the nine kinds' starts differ in: the two refusals' words; whether the rows need the documents' keys (the listings); where
// info[] counts requests and launches (-1: not at all; the mask build is the first launch of a kind that counts them); whether the device takes the requests
// in set_order's order (infx_list_grouped and infx_list_group_members keep one of their own, infx_list_ordered the caller's).
struct SetKindSpec { const char *badArgs, *tooMany; bool needKeys; int requestsAt, launchesAt; bool ordered; };
static const SetKindSpec SET_KINDS[SK_KINDS] = {
    {"bad listing arguments%s", "more than INFX_MAX_PREFILTERS (16) listing requests in one call%s", true, -1, 1, false},
    {"bad range arguments%s", "more than 16 range requests in one call%s", false, 0, -1, true},
    {"bad field-stats arguments%s", "more than 16 field-stats requests in one call%s", false, 0, -1, true},
    {"bad field-quantiles arguments%s", "more than 16 field-quantiles requests in one call%s", false, 0, 2, true},
    {"bad grouped-listing arguments%s", "more than INFX_MAX_PREFILTERS (16) grouped-listing requests in one call%s", true, -1, 2, false},
    {"bad top-groups arguments%s", "more than 16 top-groups requests in one call%s", false, 0, 3, true},
    {"bad field-distinct arguments%s", "more than 16 field-distinct requests in one call%s", false, 0, 1, true},
    {"bad group-members arguments%s", "more than INFX_MAX_PREFILTERS (16) group-members requests in one call%s", true, -1, 3, false},
    {"bad bucket-stats arguments%s", "more than 16 bucket-stats requests in one call%s", false, 0, -1, true},
};
static_assert(RB_MAX_REQS == INFX_MAX_PREFILTERS && STS_MAX_REQS == INFX_MAX_PREFILTERS && QNT_MAX_REQS == INFX_MAX_PREFILTERS && TOP_MAX_REQS == INFX_MAX_PREFILTERS &&
              DST_MAX_REQS == INFX_MAX_PREFILTERS && BKS_MAX_REQS == INFX_MAX_PREFILTERS, "every set call takes as many requests as a mask build takes filters");
struct SetCall {
    infx_stream* s; infx_index* ix; SetKindState* K; const SetKindSpec* spec;
    int32_t n; uint32_t nreq;                                            // the corpus (never negative), the call's requests
    SetKey key[INFX_MAX_PREFILTERS]; uint32_t order[INFX_MAX_PREFILTERS];      // key[i]: request i's, filled by the checks of an ordered kind; order[k]: the k-th request of the device
};
// The start of a set call, in front of its per-request checks: null arguments refused (badArgs: what the entry point found of its own), the kind's counters
// reset, then too many requests and an index without documents refused.  Nothing is consumed or enqueued.
static int32_t set_call_open(SetCall* c, infx_stream* s, SetKind kind, bool badArgs, uint32_t nreq) {
    const SetKindSpec& spec = SET_KINDS[kind];
    if (!s || badArgs) return fail(INFX_EINVAL, spec.badArgs);
    c->s = s; c->ix = s->ix; c->K = &s->kind[kind]; c->spec = &spec; c->nreq = nreq;
    std::fill(c->K->info, c->K->info + 7, 0u);
    if (nreq > INFX_MAX_PREFILTERS) return fail(INFX_ECAPACITY, spec.tooMany);
    if (!c->ix->haveDocs || (spec.needKeys && !c->ix->d.docKeyAll)) return fail(INFX_EINVAL, "index not uploaded%s");
    c->n = std::max(c->ix->d.totalDocs, 0);
    return INFX_OK;
}
// The rest of the start, the requests checked: the device, the staging of the call before consumed, the masks the call is missing built (infx_filter_masks:
// one launch in front of the rest; a kind that counts its launches starts from it), the requests counted and put into the device's order.  A call without
// requests ends here, synchronised.
static int32_t set_call_begin(SetCall* c) {
    infx_stream* s = c->s;
    HIPCHK(enter_device(c->ix->cfg.device));
    { int32_t rc_ = pin_reset(s); if (rc_) return rc_; }
    const uint32_t builds = s->mkStaged && s->mkTable.size() && c->n > 0 ? 1u : 0u;
    { int32_t rc_ = mask_flush(s); if (rc_) return rc_; }
    if (c->spec->launchesAt >= 0) c->K->info[c->spec->launchesAt] = builds;
    if (!c->nreq && s->unsynced) SYNC();
    if (c->spec->requestsAt >= 0) c->K->info[c->spec->requestsAt] = c->nreq;
    if (c->spec->ordered) set_order(c->nreq, c->key, c->order);
    return INFX_OK;
}
// the flags a request's set is read from: its mask, or every live document
static const uint8_t* set_flags(const infx_index* ix, const uint8_t* mask) { return mask ? mask : ix->d.deleted; }
extern "C++" {      // (the two templates of this section)
// a value column as a device request (DevListReq, DevRangeReq, DevStatsReq, DevQuantReq) reads it: codes, sort rank, number of values
template <class Dev> static void put_column(const infx_index* ix, int32_t col, Dev* D) { D->codes = ix->colCodes[col]; D->rank = ix->colRank[col]; D->nvals = ix->colValues[col]; }
// Runs of requests that share a spec, in the device's order: the position behind the run that starts at k0 (same: of two requests, by the caller's numbering)
template <class Same> static uint32_t run_end(const uint32_t* order, uint32_t k0, uint32_t nreq, Same same) {
    uint32_t k1 = k0 + 1;
    while (k1 < nreq && same(order[k0], order[k1])) k1++;
    return k1;
}
}
// k_field_stats' request: the set, the summed column with its value table, the group column (gcol < 0: none) with `slots` slots at out, their smallest ranks at lo
static DevStatsReq stats_dev_req(const infx_index* ix, const uint8_t* mask, int32_t col, int32_t gcol, uint32_t slots, uint32_t* out, uint32_t* lo, uint32_t ldsOff) {
    DevStatsReq D{};
    D.mask = set_flags(ix, mask); put_column(ix, col, &D);
    D.bits = ix->colBits[col]; D.kind = ix->colKind[col]; D.scale = ix->colScale[col]; D.nlimbs = ix->colLimbs[col];
    D.gcodes = gcol >= 0 ? ix->colCodes[gcol] : nullptr; D.gvals = slots; D.out = out; D.lo = lo; D.ldsOff = ldsOff;
    return D;
}
// a slot as k_field_stats leaves it (w: five counters and ranks, then limbs from STS_HEAD), its first nl limbs read and the others zero, with its smallest rank
static infx_stats_slot stats_slot(const uint32_t* w, uint32_t nl, uint32_t minRank) {
    infx_stats_slot S{};
    S.finite = w[0]; S.nan = w[1]; S.pinf = w[2]; S.ninf = w[3]; S.max_rank = w[4]; S.min_rank = minRank;
    for (uint32_t i = 0; i < nl; i++) std::memcpy(&S.sum[i], w + STS_HEAD + 2 * i, 8);
    return S;
}
// whether a placement may take the whole LDS of a CU (one workgroup of 1024 threads): not with INFX_STATS_NO_BIG_LDS=1, for measurements
static bool stats_big_lds() { static const bool noBig = [] { const char* v = getenv("INFX_STATS_NO_BIG_LDS"); return v && v[0] == '1'; }(); return !noBig; }
// the kind's output, `words` words of it, copied to its raw host copy: the call's last download and its synchronisation
static int32_t set_fetch_raw(const SetCall& c, size_t words) {
    infx_stream* s = c.s;
    c.K->raw.assign(words, 0u);
    DOWN(c.K->raw.data(), c.K->out, words * 4);
    SYNC();
    return INFX_OK;
}
// one reader behind the nine infx_last_*: out[i] (where not null) takes counter i of the kind's last call
static int32_t put_info(const infx_stream* s, SetKind kind, std::initializer_list<uint32_t*> out) {
    if (!s) return fail(INFX_EINVAL, "null argument%s");
    const uint32_t* v = s->kind[kind].info;
    for (uint32_t* p : out) { if (p) *p = *v; v++; }
    return INFX_OK;
}
// Threads and grid of a set walk (set_walk.h: 16 documents per thread and step) whose workgroups keep ldsWords words of LDS and merge them once at the end:
// STS_THREADS while the words fit STS_LDS_WORDS, else one workgroup of STS_BIG_THREADS per CU (the same sixteen waves); no more workgroups than are resident
// (LDS of a CU: FFL_CU_LDS; 2048 threads), at least one.
static int32_t merge_once_shape(const infx_index* ix, int32_t n, uint32_t ldsWords, int* threads, int* grid) {
    int cus = 0; HIPCHK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, ix->cfg.device));
    const int64_t groups = ((int64_t)n + SW_GROUP - 1) / SW_GROUP, T = ldsWords <= STS_LDS_WORDS ? STS_THREADS : STS_BIG_THREADS;
    const int64_t perCu = std::min<int64_t>(2048 / T, (int64_t)(FFL_CU_LDS / std::max<size_t>((size_t)ldsWords * 4, 1)));      // (at least one: ldsWords <= STS_BIG_LDS_WORDS)
    *threads = (int)T; *grid = (int)std::max<int64_t>(1, std::min<int64_t>((int64_t)std::max(cus, 1) * perCu, (groups + T - 1) / T));
    return INFX_OK;
}
// ---- list_documents: a page of the documents a filter accepts, in the order of a column (listing.hip.inc) ----
// The enqueue part of a listing call, shared by infx_list_ordered and infx_list_grouped.  Where the nreq requests of a call lie in the stream's listing
// workspace W ([states | histograms] zeroed, [page composites] all ones, range counts and prefixes [nreq][2][3][nRanges]) and in its rows O
// ([keys | docs | codes | counts | totals], INFX_POST_MAX_ROWS rows per request).
struct ListLayout {
    int32_t n; uint32_t nreq, tiles, nRanges;
    size_t stBytes, oHist, oPairs, oRange, oDocs, oCodes, oCnt, oTot, histOff[INFX_MAX_PREFILTERS];
    char *W, *O;
    int32_t* docs(uint32_t i) const { return (int32_t*)(O + oDocs) + (size_t)i * INFX_POST_MAX_ROWS; }
    uint32_t* count(uint32_t i) const { return (uint32_t*)(O + oCnt) + i; }
    uint32_t* total(uint32_t i) const { return (uint32_t*)(O + oTot) + i; }
};
// what a request reads of the index: the set (mask or the Deleted flags), the ordered column with its sort rank, the passes of its select
static DevListReq list_dev_req(const infx_index* ix, const uint8_t* mask, int32_t col, bool ascending, uint32_t offset, uint32_t limit, uint32_t digitBits) {
    DevListReq D{};
    D.mask = set_flags(ix, mask);
    if (col >= 0) put_column(ix, col, &D); else D.nvals = 1;
    D.ascending = ascending ? 1u : 0u; D.offset = offset; D.limit = limit; D.digitBits = digitBits; D.passes = ls_passes(D.nvals, digitBits);
    return D;
}
// the workspace of nreq requests, grown and initialised on the stream
static int32_t list_prepare(infx_stream* s, int32_t n, uint32_t nreq, const DevListReq* D, ListLayout* L) {
    L->n = n; L->nreq = nreq;
    size_t histWords = 0;
    for (uint32_t i = 0; i < nreq; i++) { L->histOff[i] = histWords; histWords += (size_t)D[i].passes * 2u << D[i].digitBits; }
    L->tiles = (uint32_t)(((int64_t)n + LST_TILE - 1) / LST_TILE); L->nRanges = std::max(1u, std::min(LST_MAXRANGES, L->tiles));
    L->stBytes = (sizeof(DevListState) + 63) & ~(size_t)63;
    L->oHist = (size_t)nreq * L->stBytes; L->oPairs = (L->oHist + histWords * 4 + 63) & ~(size_t)63; L->oRange = L->oPairs + (size_t)nreq * INFX_POST_MAX_ROWS * 8;
    const size_t wsBytes = L->oRange + (size_t)nreq * 6 * L->nRanges * 4;
    const size_t R = INFX_POST_MAX_ROWS;
    L->oDocs = (size_t)nreq * R * 8; L->oCodes = L->oDocs + (size_t)nreq * R * 4; L->oCnt = L->oCodes + (size_t)nreq * R * 4; L->oTot = L->oCnt + (size_t)nreq * 4;
    SetKindState& K = s->kind[SK_LIST];
    GROW(K.ws, K.capWs, wsBytes);
    GROW(K.out, K.capOut, L->oTot + (size_t)nreq * 4);
    L->W = (char*)K.ws; L->O = (char*)K.out;
    HIPCHK(hipMemsetAsync(L->W, 0, L->oPairs, s->st));
    HIPCHK(hipMemsetAsync(L->W + L->oPairs, 0xFF, (size_t)nreq * INFX_POST_MAX_ROWS * 8, s->st));
    s->unsynced = true;
    return INFX_OK;
}
// request i of the layout: select, count, prefix, gather and sort on the stream, and its rows' way back to the caller's keys / docs / codes (the request's own
// rows: D.limit of each; an array that is null is not fetched).  *histPasses / *launches grow by what was enqueued.
static int32_t list_enqueue(infx_stream* s, const ListLayout& L, uint32_t i, const DevListReq& D, int64_t* keys_out, int32_t* docs_out, uint32_t* codes_out,
                            uint32_t* histPasses, uint32_t* launches) {
    const int32_t n = L.n; const uint32_t nRanges = L.nRanges, tiles = L.tiles; const size_t R = INFX_POST_MAX_ROWS;
    char* W = L.W; char* O = L.O;
    DevListState* st = (DevListState*)(W + (size_t)i * L.stBytes);
    uint32_t* hist = (uint32_t*)(W + L.oHist) + L.histOff[i];
    unsigned long long* pairs = (unsigned long long*)(W + L.oPairs) + (size_t)i * INFX_POST_MAX_ROWS;
    uint32_t* rangeCnt = (uint32_t*)(W + L.oRange) + (size_t)i * 6 * nRanges; uint32_t* rangePre = rangeCnt + 3 * (size_t)nRanges;
    if (n > 0) {
        const size_t nb = (size_t)1 << D.digitBits;
        const int64_t groups = ((int64_t)n + LST_GROUP - 1) / LST_GROUP;
        const int grid = (int)std::min<int64_t>(FCM_MAXGRID, (groups + LST_THREADS - 1) / LST_THREADS);
        for (uint32_t p = 0; p < D.passes; p++) {
            k_list_hist<<<grid, LST_THREADS, 2 * nb * 4, s->st>>>(D, n, p, st, hist + (size_t)p * 2 * nb);
            k_list_pick<<<1, LST_THREADS, 0, s->st>>>(D, p, st, hist + (size_t)p * 2 * nb);
        }
        k_list_count<<<nRanges, LST_THREADS, 0, s->st>>>(D, n, tiles, nRanges, st, rangeCnt);
        k_list_prefix<<<3, LST_THREADS, 0, s->st>>>(nRanges, st, rangeCnt, rangePre);
        k_list_gather<<<nRanges, WAVE, 0, s->st>>>(D, n, tiles, nRanges, st, rangeCnt, rangePre, pairs);
        *histPasses += D.passes; *launches += 2 * D.passes + 3;
    }
    k_list_sort<<<1, LST_SORT_THREADS, 0, s->st>>>(D, n, st, pairs, (const long long*)s->ix->d.docKeyAll, (long long*)O + (size_t)i * R, L.docs(i),
                                                 (uint32_t*)(O + L.oCodes) + (size_t)i * R, L.count(i), L.total(i));
    HIPCHK(hipGetLastError());
    ++*launches;
    if (keys_out) DOWN(keys_out, (long long*)O + (size_t)i * R, (size_t)D.limit * 8);
    if (docs_out) DOWN(docs_out, L.docs(i), (size_t)D.limit * 4);
    if (codes_out) DOWN(codes_out, (uint32_t*)(O + L.oCodes) + (size_t)i * R, (size_t)D.limit * 4);
    return INFX_OK;
}
// a request's page: limit, offset and digit width in range
static int32_t check_page_request(uint32_t limit, uint32_t offset, uint32_t digitBits) {
    if (limit < 1 || limit > INFX_POST_MAX_ROWS) return fail(INFX_EINVAL, "a listing's limit is 1 .. INFX_POST_MAX_ROWS (1024)%s");
    if (offset >= 0x80000000u) return fail(INFX_EINVAL, "a listing's offset is below 2^31%s");
    if (digitBits < LS_MIN_DIGIT_BITS || digitBits > LS_MAX_DIGIT_BITS) return fail(INFX_EINVAL, "a listing's digit width is 4 .. 11 bits%s");
    return INFX_OK;
}
int32_t infx_list_ordered(infx_stream* s, uint32_t nreq, const infx_list_req* reqs, int64_t* keys_out, int32_t* docs_out, uint32_t* codes_out, uint32_t* counts_out, uint32_t* totals_out) {
    SetCall c;
    { int32_t rc_ = set_call_open(&c, s, SK_LIST, nreq && (!reqs || !keys_out || !docs_out || !codes_out || !counts_out || !totals_out), nreq); if (rc_) return rc_; }
    infx_index* ix = c.ix; const int32_t n = c.n; uint32_t* info = c.K->info;
    DevListReq D[INFX_MAX_PREFILTERS];
    for (uint32_t i = 0; i < nreq; i++) {
        const infx_list_req& Q = reqs[i];
        { int32_t rc_ = check_page_request(Q.limit, Q.offset, Q.digit_bits); if (rc_) return rc_; }
        { int32_t rc_ = check_set_request(s, Q.mask, Q.col, false, "listing"); if (rc_) return rc_; }
        D[i] = list_dev_req(ix, Q.mask, Q.col, Q.ascending != 0, Q.offset, Q.limit, Q.digit_bits);
    }
    { int32_t rc_ = set_call_begin(&c); if (rc_) return rc_; }
    if (!nreq) return INFX_OK;
    ListLayout L;
    { int32_t rc_ = list_prepare(s, n, nreq, D, &L); if (rc_) return rc_; }
    for (uint32_t i = 0; i < nreq; i++) {
        const size_t at = (size_t)i * INFX_POST_MAX_ROWS;
        int32_t rc_ = list_enqueue(s, L, i, D[i], keys_out + at, docs_out + at, codes_out + at, &info[0], &info[1]); if (rc_) return rc_;
    }
    DOWN(counts_out, L.count(0), (size_t)nreq * 4);
    DOWN(totals_out, L.total(0), (size_t)nreq * 4);
    SYNC();
    return INFX_OK;
}
int32_t infx_last_list_stats(infx_stream* s, uint32_t* hist_passes, uint32_t* launches) {
    return put_info(s, SK_LIST, {hist_passes, launches});
}
// ---- range_facets: bucket counts and the extreme sort ranks of a numeric column over a document set (ranges.hip.inc) ----
int32_t infx_range_counts(infx_stream* s, uint32_t nreq, const infx_range_req* reqs, uint32_t* counts_out, uint32_t* min_rank_out, uint32_t* max_rank_out) {
    SetCall c;
    { int32_t rc_ = set_call_open(&c, s, SK_RANGE, nreq && (!reqs || !counts_out || !min_rank_out || !max_rank_out), nreq); if (rc_) return rc_; }
    infx_index* ix = c.ix; SetKindState& K = *c.K; const int32_t n = c.n; const SetKey* key = c.key; const uint32_t* order = c.order;
    size_t thrWords = 0;
    for (uint32_t i = 0; i < nreq; i++) {
        const infx_range_req& Q = reqs[i];
        if (Q.nedges < RB_MIN_EDGES || Q.nedges > RB_MAX_EDGES || !Q.thr) return fail(INFX_EINVAL, "a range request has 2 .. INFX_RANGE_MAX_EDGES (257) thresholds%s");
        { int32_t rc_ = check_set_request(s, Q.mask, Q.col, true, "range request"); if (rc_) return rc_; }
        if (Q.nan_ranks > 1u) return fail(INFX_EINVAL, "nan_ranks is 0 or 1%s");
        for (uint32_t j = 0; j < Q.nedges; j++)
            if (Q.thr[j] < Q.nan_ranks || Q.thr[j] > ix->colValues[Q.col] || (j && Q.thr[j] < Q.thr[j - 1])) return fail(INFX_EINVAL, "a range request's thresholds are non-decreasing, from nan_ranks to the column's number of values%s");
        thrWords += Q.nedges; c.key[i] = SetKey{Q.mask, Q.col, -1};
    }
    { int32_t rc_ = set_call_begin(&c); if (rc_) return rc_; }
    if (!nreq) return INFX_OK;
    const size_t oHi = (size_t)nreq * RNG_OUT_STRIDE * 4, oLo = oHi + (size_t)nreq * 4;
    GROW(K.ws, K.capWs, thrWords * 4);
    GROW(K.out, K.capOut, oLo + (size_t)nreq * 4);
    char* O = (char*)K.out;
    std::vector<uint32_t> thr; thr.reserve(thrWords);
    DevRangeCall P{}; P.nreq = nreq;
    uint32_t ldsWords = 0;
    for (uint32_t k = 0; k < nreq; k++) {
        const infx_range_req& Q = reqs[order[k]];
        DevRangeReq& D = P.r[k];
        D.mask = set_flags(ix, Q.mask); put_column(ix, Q.col, &D);
        D.thr = (const uint32_t*)K.ws + thr.size(); thr.insert(thr.end(), Q.thr, Q.thr + Q.nedges);
        D.nedges = Q.nedges; D.nanRanks = Q.nan_ranks; D.ldsOff = ldsWords; ldsWords += rb_lds_words(Q.nedges);
        if (k) D.reuse = set_reuse(key[order[k - 1]], key[order[k]]);
    }
    UP(K.ws, thr.data(), thrWords * 4);
    HIPCHK(hipMemsetAsync(O, 0, oLo, s->st));
    HIPCHK(hipMemsetAsync(O + oLo, 0xFF, (size_t)nreq * 4, s->st));
    s->unsynced = true;
    if (n > 0) {
        const int64_t groups = ((int64_t)n + LST_GROUP - 1) / LST_GROUP;
        const int grid = (int)std::min<int64_t>(RNG_MAXGRID, (groups + RNG_THREADS - 1) / RNG_THREADS);
        k_range_counts<<<grid, RNG_THREADS, (size_t)ldsWords * 4, s->st>>>(P, n, (uint32_t*)O, (uint32_t*)(O + oHi), (uint32_t*)(O + oLo));
        HIPCHK(hipGetLastError());
        K.info[1] = 1;
    }
    for (uint32_t k = 0; k < nreq; k++) {
        const uint32_t i = order[k];
        DOWN(counts_out + (size_t)i * INFX_RANGE_SLOTS, (uint32_t*)O + (size_t)k * RNG_OUT_STRIDE, (size_t)rb_slots(reqs[i].nedges) * 4);
        DOWN(max_rank_out + i, (uint32_t*)(O + oHi) + k, 4);
        DOWN(min_rank_out + i, (uint32_t*)(O + oLo) + k, 4);
    }
    SYNC();
    return INFX_OK;
}
int32_t infx_last_range_stats(infx_stream* s, uint32_t* requests, uint32_t* launches) {
    return put_info(s, SK_RANGE, {requests, launches});
}
// ---- field_stats: counts, extreme sort ranks and exact limb sums of a numeric column over a document set, whole or per group (stats.hip.inc) ----
// Where the slots of a call's requests live: in ascending size (slots x words) while they fit `budget` words of LDS per workgroup, the others in global
// memory.  words[k] = request k's slots x stride; ldsOff[k] = its first LDS word or STS_GLOBAL; *inGlobal the requests left out.  Returns the LDS words in use.
static uint32_t sts_place(uint32_t nreq, const uint32_t* words, uint32_t budget, uint32_t* ldsOff, uint32_t* inGlobal) {
    uint32_t by[2 * STS_MAX_REQS], used = 0; *inGlobal = 0;      // (nreq <= 2 x STS_MAX_REQS: infx_field_quantiles places two sets of rows per request)
    for (uint32_t k = 0; k < nreq; k++) by[k] = k;
    std::stable_sort(by, by + nreq, [&](uint32_t a, uint32_t b) { return words[a] < words[b]; });
    for (uint32_t j = 0; j < nreq; j++) {
        const uint32_t k = by[j];
        if (used + words[k] <= budget) { ldsOff[k] = used; used += words[k]; } else { ldsOff[k] = STS_GLOBAL; ++*inGlobal; }
    }
    return used;
}
// sts_place under the two budgets: k_facets_all's (STS_LDS_WORDS, 256 threads); where that leaves requests in global memory and the whole LDS of a CU would
// hold more of them, that (STS_BIG_LDS_WORDS, if `big` allows it): merge_once_shape then takes one workgroup of 1024 threads per CU, LDS atomics for global ones
// `reserve`: words of both budgets the caller keeps for itself (infx_bucket_stats: the thresholds), at most STS_LDS_WORDS
static uint32_t sts_place_best(uint32_t nreq, const uint32_t* words, bool big, uint32_t* ldsOff, uint32_t reserve = 0) {
    uint32_t inGlobal = 0, ldsWords = sts_place(nreq, words, STS_LDS_WORDS - reserve, ldsOff, &inGlobal);
    if (inGlobal && big) {
        uint32_t bigOff[2 * STS_MAX_REQS], bigGlobal = 0; const uint32_t bigWords = sts_place(nreq, words, STS_BIG_LDS_WORDS - reserve, bigOff, &bigGlobal);
        if (bigGlobal < inGlobal) { std::copy(bigOff, bigOff + nreq, ldsOff); ldsWords = bigWords; }
    }
    return ldsWords;
}
int32_t infx_field_stats(infx_stream* s, uint32_t nreq, const infx_stats_req* reqs, infx_stats_slot* slots_out) {
    SetCall c;
    { int32_t rc_ = set_call_open(&c, s, SK_STATS, nreq && (!reqs || !slots_out), nreq); if (rc_) return rc_; }
    infx_index* ix = c.ix; SetKindState& K = *c.K; const int32_t n = c.n; const SetKey* key = c.key; const uint32_t* order = c.order;
    for (uint32_t i = 0; i < nreq; i++) {
        const infx_stats_req& Q = reqs[i];
        { int32_t rc_ = check_set_request(s, Q.mask, Q.col, true, "field-stats request"); if (rc_) return rc_; }
        if (!ix->colBitsOk[Q.col]) return fail(INFX_EINVAL, "the field-stats request's value table was not uploaded%s");
        if (Q.group_col >= 0) { int32_t rc_ = check_group_slots(ix, Q.group_col, "field-stats request"); if (rc_) return rc_; }
        c.key[i] = SetKey{Q.mask, Q.col, Q.group_col};
    }
    { int32_t rc_ = set_call_begin(&c); if (rc_) return rc_; }
    if (!nreq) return INFX_OK;
    // a request's slots: one per value of its group column (at least one), one without; in the caller's order request i's follow request i - 1's, at at[i]
    uint32_t slotsOf[STS_MAX_REQS]; size_t at[STS_MAX_REQS], totalSlots = 0;
    for (uint32_t i = 0; i < nreq; i++) { const int32_t g = reqs[i].group_col; slotsOf[i] = g >= 0 ? std::max(ix->colValues[g], 1u) : 1u; at[i] = totalSlots; totalSlots += slotsOf[i]; }
    // the output: per request (in device order) its slots, then every request's smallest ranks
    uint32_t words[STS_MAX_REQS], ldsOff[STS_MAX_REQS]; size_t off[STS_MAX_REQS], loOff[STS_MAX_REQS], outWords = 0, loSlots = 0;
    for (uint32_t k = 0; k < nreq; k++) {
        const infx_stats_req& Q = reqs[order[k]];
        words[k] = slotsOf[order[k]] * sts_stride(ix->colLimbs[Q.col]);
        off[k] = outWords; outWords += words[k]; loOff[k] = loSlots; loSlots += slotsOf[order[k]];
    }
    const uint32_t ldsWords = sts_place_best(nreq, words, stats_big_lds(), ldsOff);
    GROW(K.out, K.capOut, (outWords + totalSlots) * 4);
    uint32_t* O = (uint32_t*)K.out;
    DevStatsCall P{}; P.nreq = nreq;
    for (uint32_t k = 0; k < nreq; k++) {
        const infx_stats_req& Q = reqs[order[k]];
        P.r[k] = stats_dev_req(ix, Q.mask, Q.col, Q.group_col, slotsOf[order[k]], O + off[k], O + outWords + loOff[k], ldsOff[k]);
        if (k) P.r[k].reuse = set_reuse(key[order[k - 1]], key[order[k]]);
    }
    HIPCHK(hipMemsetAsync(O, 0, outWords * 4, s->st));
    HIPCHK(hipMemsetAsync(O + outWords, 0xFF, totalSlots * 4, s->st));
    s->unsynced = true;
    if (n > 0) {
        int threads, grid; { int32_t rc_ = merge_once_shape(ix, n, ldsWords, &threads, &grid); if (rc_) return rc_; }
        HIPCHK(lds_limit((const void*)k_field_stats, ix->cfg.device, (size_t)ldsWords * 4));
        k_field_stats<<<grid, threads, (size_t)ldsWords * 4, s->st>>>(P, n);
        HIPCHK(hipGetLastError());
        K.info[1] = 1;
    }
    { int32_t rc_ = set_fetch_raw(c, outWords + totalSlots); if (rc_) return rc_; }
    for (uint32_t k = 0; k < nreq; k++) {
        const uint32_t nl = ix->colLimbs[reqs[order[k]].col], W = sts_stride(nl);
        for (uint32_t g = 0; g < slotsOf[order[k]]; g++)
            slots_out[at[order[k]] + g] = stats_slot(K.raw.data() + off[k] + (size_t)g * W, nl, K.raw[outWords + loOff[k] + g]);
    }
    return INFX_OK;
}
int32_t infx_last_field_stats_info(infx_stream* s, uint32_t* requests, uint32_t* launches) {
    return put_info(s, SK_STATS, {requests, launches});
}
// ---- bucket_stats: field_stats' slots per range bucket of a second numeric column over a document set (bucket_stats.hip.inc) ----
static_assert(BKS_MAX_THR_WORDS <= STS_LDS_WORDS && INFX_RANGE_MAX_EDGES == RB_MAX_EDGES, "a call's thresholds fit the small budget");
int32_t infx_bucket_stats(infx_stream* s, uint32_t nreq, const infx_bucket_stats_req* reqs, infx_stats_slot* slots_out) {
    SetCall c;
    { int32_t rc_ = set_call_open(&c, s, SK_BUCKETS, nreq && (!reqs || !slots_out), nreq); if (rc_) return rc_; }
    infx_index* ix = c.ix; SetKindState& K = *c.K; const int32_t n = c.n; const SetKey* key = c.key; const uint32_t* order = c.order;
    for (uint32_t i = 0; i < nreq; i++) {
        const infx_bucket_stats_req& Q = reqs[i];
        if (Q.nedges < RB_MIN_EDGES || Q.nedges > RB_MAX_EDGES || !Q.thr) return fail(INFX_EINVAL, "a bucket-stats request has 2 .. INFX_RANGE_MAX_EDGES (257) thresholds%s");
        { int32_t rc_ = check_set_request(s, Q.mask, Q.col, true, "bucket-stats request"); if (rc_) return rc_; }
        if (!ix->colBitsOk[Q.col]) return fail(INFX_EINVAL, "the bucket-stats request's value table was not uploaded%s");
        { int32_t rc_ = check_set_request(s, Q.mask, Q.bucket_col, true, "bucket-stats request"); if (rc_) return rc_; }
        if (Q.nan_ranks > 1u) return fail(INFX_EINVAL, "nan_ranks is 0 or 1%s");
        for (uint32_t j = 0; j < Q.nedges; j++)
            if (Q.thr[j] < Q.nan_ranks || Q.thr[j] > ix->colValues[Q.bucket_col] || (j && Q.thr[j] < Q.thr[j - 1]))
                return fail(INFX_EINVAL, "a bucket-stats request's thresholds are non-decreasing, from nan_ranks to the bucket column's number of values%s");
        c.key[i] = SetKey{Q.mask, Q.col, Q.bucket_col};
    }
    { int32_t rc_ = set_call_begin(&c); if (rc_) return rc_; }
    if (!nreq) return INFX_OK;
    // a request's slots: B + 3, in rb_slot's order; in the caller's order request i's follow request i - 1's, at at[i]
    size_t at[BKS_MAX_REQS], totalSlots = 0;
    for (uint32_t i = 0; i < nreq; i++) { at[i] = totalSlots; totalSlots += bks_slots(reqs[i].nedges); }
    // the output: per request (in device order) its slots, then every request's smallest ranks; LDS: every request's thresholds, then the slots placed there
    uint32_t words[BKS_MAX_REQS], ldsOff[BKS_MAX_REQS], thrOff[BKS_MAX_REQS], thrWords = 0; size_t off[BKS_MAX_REQS], loOff[BKS_MAX_REQS], outWords = 0, loSlots = 0;
    for (uint32_t k = 0; k < nreq; k++) {
        const infx_bucket_stats_req& Q = reqs[order[k]];
        words[k] = bks_slot_words(Q.nedges, ix->colLimbs[Q.col]);
        off[k] = outWords; outWords += words[k]; loOff[k] = loSlots; loSlots += bks_slots(Q.nedges);
        thrOff[k] = thrWords; thrWords += bks_thr_words(Q.nedges);
    }
    const uint32_t slotWords = sts_place_best(nreq, words, stats_big_lds(), ldsOff, thrWords), ldsWords = thrWords + slotWords;
    uint32_t* info = K.info;
    for (uint32_t k = 0; k < nreq; k++) {
        if (ldsOff[k] == STS_GLOBAL) info[4]++;
        else { ldsOff[k] += thrWords; info[ldsWords <= STS_LDS_WORDS ? 2 : 3]++; }
    }
    GROW(K.ws, K.capWs, (size_t)thrWords * 4);
    GROW(K.out, K.capOut, (outWords + totalSlots) * 4);
    uint32_t* O = (uint32_t*)K.out;
    std::vector<uint32_t> thr(thrWords, 0u);
    DevBucketCall P{}; P.nreq = nreq;
    for (uint32_t k = 0; k < nreq; k++) {
        const infx_bucket_stats_req& Q = reqs[order[k]];
        DevBucketReq& D = P.r[k];
        D.s = stats_dev_req(ix, Q.mask, Q.col, Q.bucket_col, bks_slots(Q.nedges), O + off[k], O + outWords + loOff[k], ldsOff[k]);
        if (k) D.s.reuse = set_reuse(key[order[k - 1]], key[order[k]]);
        D.brank = ix->colRank[Q.bucket_col]; D.bvals = ix->colValues[Q.bucket_col];
        D.thr = (const uint32_t*)K.ws + thrOff[k]; std::copy(Q.thr, Q.thr + Q.nedges, thr.begin() + thrOff[k]);
        D.nedges = Q.nedges; D.nanRanks = Q.nan_ranks; D.thrOff = thrOff[k];
    }
    UP(K.ws, thr.data(), (size_t)thrWords * 4);
    HIPCHK(hipMemsetAsync(O, 0, outWords * 4, s->st));
    HIPCHK(hipMemsetAsync(O + outWords, 0xFF, totalSlots * 4, s->st));
    s->unsynced = true;
    if (n > 0) {
        int threads, grid; { int32_t rc_ = merge_once_shape(ix, n, ldsWords, &threads, &grid); if (rc_) return rc_; }
        HIPCHK(lds_limit((const void*)k_bucket_stats, ix->cfg.device, (size_t)ldsWords * 4));
        k_bucket_stats<<<grid, threads, (size_t)ldsWords * 4, s->st>>>(P, n);
        HIPCHK(hipGetLastError());
        info[1] = 1;
    }
    { int32_t rc_ = set_fetch_raw(c, outWords + totalSlots); if (rc_) return rc_; }
    for (uint32_t k = 0; k < nreq; k++) {
        const uint32_t nl = ix->colLimbs[reqs[order[k]].col], W = sts_stride(nl);
        for (uint32_t g = 0; g < bks_slots(reqs[order[k]].nedges); g++)
            slots_out[at[order[k]] + g] = stats_slot(K.raw.data() + off[k] + (size_t)g * W, nl, K.raw[outWords + loOff[k] + g]);
    }
    return INFX_OK;
}
int32_t infx_last_bucket_stats_info(infx_stream* s, uint32_t* requests, uint32_t* launches, uint32_t* small_lds, uint32_t* big_lds, uint32_t* in_global) {
    return put_info(s, SK_BUCKETS, {requests, launches, small_lds, big_lds, in_global});
}
// ---- field_quantiles: the sort ranks at the quantiles' positions of a numeric column over a document set, whole and per group (quantiles.hip.inc) ----
// The digit width of request Q under the call's cap: its own digit_bits (never above the cap), else the narrowest width that takes no more passes than the cap
static uint32_t qnt_width(const infx_quant_req& Q, uint32_t nvals, uint32_t cap) { return Q.digit_bits ? std::min(Q.digit_bits, cap) : qs_narrow(nvals, cap); }
int32_t infx_field_quantiles(infx_stream* s, uint32_t nreq, const infx_quant_req* reqs, infx_quant_slot* slots_out, uint32_t* ranks_out) {
    SetCall c;
    { int32_t rc_ = set_call_open(&c, s, SK_QUANT, nreq && (!reqs || !slots_out || !ranks_out), nreq); if (rc_) return rc_; }
    infx_index* ix = c.ix; SetKindState& K = *c.K; const int32_t n = c.n; const SetKey* key = c.key; const uint32_t* order = c.order;
    for (uint32_t i = 0; i < nreq; i++) {
        const infx_quant_req& Q = reqs[i];
        { int32_t rc_ = check_set_request(s, Q.mask, Q.col, true, "field-quantiles request"); if (rc_) return rc_; }
        if (Q.group_col >= 0) { int32_t rc_ = check_group_slots(ix, Q.group_col, "field-quantiles request"); if (rc_) return rc_; }
        c.key[i] = SetKey{Q.mask, Q.col, Q.group_col};
        if (Q.nq < 1 || Q.nq > QS_MAX_Q) return fail(INFX_EINVAL, "a field-quantiles request has 1 .. INFX_QUANT_MAX (16) quantiles%s");
        for (uint32_t t = 0; t < Q.nq; t++) if (!(Q.q[t] >= 0.0 && Q.q[t] <= 1.0)) return fail(INFX_EINVAL, "a quantile is a number in [0, 1]%s");
        if (Q.nan_ranks > 1u) return fail(INFX_EINVAL, "nan_ranks is 0 or 1%s");
        if (Q.digit_bits && (Q.digit_bits < LS_MIN_DIGIT_BITS || Q.digit_bits > LS_MAX_DIGIT_BITS)) return fail(INFX_EINVAL, "a field-quantiles request's digit width is 0 (chosen by the call) or 4 .. 11 bits%s");
    }
    { int32_t rc_ = set_call_begin(&c); if (rc_) return rc_; }
    if (!nreq) return INFX_OK;
    // a request's slots: one per value of its group column, then the whole set's; in the caller's order request i's slots and ranks follow request i - 1's
    uint32_t slotsOf[QNT_MAX_REQS]; size_t atSlot[QNT_MAX_REQS], atTgt[QNT_MAX_REQS], ns = 0, nt = 0;
    for (uint32_t i = 0; i < nreq; i++) {
        slotsOf[i] = reqs[i].group_col >= 0 ? ix->colValues[reqs[i].group_col] + 1u : 1u;
        atSlot[i] = ns; atTgt[i] = nt; ns += slotsOf[i]; nt += (size_t)slotsOf[i] * reqs[i].nq;
    }
    uint32_t slots[QNT_MAX_REQS], width[QNT_MAX_REQS], passes[QNT_MAX_REQS]; size_t slot0[QNT_MAX_REQS], tgt0[QNT_MAX_REQS], q0[QNT_MAX_REQS], totalSlots = 0, totalTgts = 0, totalQ = 0;
    for (uint32_t k = 0; k < nreq; k++) {
        const infx_quant_req& Q = reqs[order[k]];
        slots[k] = slotsOf[order[k]];
        slot0[k] = totalSlots; tgt0[k] = totalTgts; q0[k] = totalQ;
        totalSlots += slots[k]; totalTgts += (size_t)slots[k] * Q.nq; totalQ += Q.nq;
    }
    // The digit width: the widest (fewest passes) at which the rows of one pass of the whole call stay inside QNT_SCRATCH_WORDS.  At 4 bits they always do:
    // 16 requests x 4097 slots x 16 quantiles x 16 bins.
    uint32_t cap = LS_MAX_DIGIT_BITS; size_t tabWords = 0;
    for (;; cap--) {
        size_t first = 0, later = 0;
        for (uint32_t k = 0; k < nreq; k++) {
            const infx_quant_req& Q = reqs[order[k]];
            width[k] = qnt_width(Q, ix->colValues[Q.col], cap); passes[k] = ls_passes(ix->colValues[Q.col], width[k]);
            first += (size_t)slots[k] * qs_slot_words(0, Q.nq, width[k]);
            if (passes[k] > 1) later += (size_t)slots[k] * qs_slot_words(1, Q.nq, width[k]);
        }
        tabWords = std::max(first, later);
        if (tabWords <= QNT_SCRATCH_WORDS || cap == LS_MIN_DIGIT_BITS) break;
    }
    K.info[3] = cap;
    const size_t oTgt = (totalQ * 8 + 63) & ~(size_t)63, oTab = (oTgt + totalTgts * sizeof(ls_target) + 63) & ~(size_t)63;
    GROW(K.ws, K.capWs, oTab + tabWords * 4);
    GROW(K.out, K.capOut, (2 * totalSlots + totalTgts) * 4);
    char* W = (char*)K.ws; uint32_t* O = (uint32_t*)K.out;
    {
        std::vector<double> qs; qs.reserve(totalQ);
        for (uint32_t k = 0; k < nreq; k++) qs.insert(qs.end(), reqs[order[k]].q, reqs[order[k]].q + reqs[order[k]].nq);
        UP(W, qs.data(), totalQ * 8);
    }
    // without a pass (an empty corpus) every slot reads count 0 and every target no rank
    HIPCHK(hipMemsetAsync(O, 0, 2 * totalSlots * 4, s->st));
    HIPCHK(hipMemsetAsync(O + 2 * totalSlots, 0xFF, totalTgts * 4, s->st));
    s->unsynced = true;
    const uint32_t maxPasses = *std::max_element(passes, passes + nreq);
    for (uint32_t p = 0; n > 0 && p < maxPasses; p++) {
        // the requests that still have a pass to go, in the call's order: what one keeps of the one before it holds among them
        // words / ldsOff: per request its groups' rows (none without a group column), then the whole set's
        DevQuantCall P{}; uint32_t words[2 * QNT_MAX_REQS], ldsOff[2 * QNT_MAX_REQS]; size_t used = 0; int32_t before = -1;
        for (uint32_t k = 0; k < nreq; k++) {
            if (passes[k] <= p) continue;
            const infx_quant_req& Q = reqs[order[k]];
            DevQuantReq& D = P.r[P.nreq];
            D.mask = set_flags(ix, Q.mask); put_column(ix, Q.col, &D);
            D.gcodes = Q.group_col >= 0 ? ix->colCodes[Q.group_col] : nullptr; D.gvals = slots[k] - 1u; D.slots = slots[k]; D.nq = Q.nq;
            D.q = (const double*)W + q0[k]; D.tgt = (ls_target*)(W + oTgt) + tgt0[k]; D.tab = (uint32_t*)(W + oTab) + used;
            D.slotOut = O + 2 * slot0[k]; D.rankOut = O + 2 * totalSlots + tgt0[k];
            D.digitBits = width[k]; D.passes = passes[k]; D.nanRanks = Q.nan_ranks; D.slot0 = P.slots;
            if (before >= 0) D.reuse = set_reuse(key[order[before]], key[order[k]]);
            words[2 * P.nreq + 1] = qs_slot_words(p, Q.nq, width[k]); words[2 * P.nreq] = D.gvals * words[2 * P.nreq + 1];
            used += (size_t)slots[k] * words[2 * P.nreq + 1]; P.slots += slots[k]; P.nreq++; before = (int32_t)k;
        }
        const uint32_t ldsWords = sts_place_best(2 * P.nreq, words, true, ldsOff);      // the rows' places: k_field_stats' rule and its two launch shapes
        for (uint32_t k = 0; k < P.nreq; k++) {
            P.r[k].ldsOff = ldsOff[2 * k]; P.r[k].ldsOffWhole = ldsOff[2 * k + 1];
            // counted by where the rows that make the request large lie: its groups', the whole set's without a group column
            const bool inLds = (P.r[k].gvals ? P.r[k].ldsOff : P.r[k].ldsOffWhole) != STS_GLOBAL;
            K.info[inLds ? 4 : 5]++;
        }
        HIPCHK(hipMemsetAsync(W + oTab, 0, used * 4, s->st));
        int threads, grid; { int32_t rc_ = merge_once_shape(ix, n, ldsWords, &threads, &grid); if (rc_) return rc_; }
        HIPCHK(lds_limit((const void*)k_quant_hist, ix->cfg.device, (size_t)ldsWords * 4));
        k_quant_hist<<<grid, threads, (size_t)ldsWords * 4, s->st>>>(P, n, p);
        const uint32_t perBlock = QNT_PICK_THREADS / WAVE;
        k_quant_pick<<<(P.slots + perBlock - 1) / perBlock, QNT_PICK_THREADS, 0, s->st>>>(P, p);
        HIPCHK(hipGetLastError());
        K.info[1]++; K.info[2] += 2;
    }
    { int32_t rc_ = set_fetch_raw(c, 2 * totalSlots + totalTgts); if (rc_) return rc_; }
    for (uint32_t k = 0; k < nreq; k++) {
        const uint32_t i = order[k];
        for (uint32_t g = 0; g < slots[k]; g++) { slots_out[atSlot[i] + g].count = K.raw[2 * (slot0[k] + g)]; slots_out[atSlot[i] + g].nan = K.raw[2 * (slot0[k] + g) + 1]; }
        std::copy(K.raw.begin() + 2 * totalSlots + tgt0[k], K.raw.begin() + 2 * totalSlots + tgt0[k] + (size_t)slots[k] * reqs[i].nq, ranks_out + atTgt[i]);
    }
    return INFX_OK;
}
int32_t infx_last_field_quantiles_info(infx_stream* s, uint32_t* requests, uint32_t* hist_passes, uint32_t* launches, uint32_t* digit_bits, uint32_t* lds_rows, uint32_t* global_rows) {
    return put_info(s, SK_QUANT, {requests, hist_passes, launches, digit_bits, lds_rows, global_rows});
}
// ---- list_groups: a page of the heads of a document set's groups, in the order of a column, with the groups' sizes (groups.hip.inc) ----
// The part infx_list_grouped and infx_list_group_members share: everything but the walk that follows a spec's pages.  What that walk finds enqueued on the
// stream, for the requests [k0, k1) of one spec in the device's order (request k is the caller's order[k]):
struct GroupPages {
    DevGroupSpec G;                         // the spec: its set, columns and head table
    uint32_t k0, k1; const uint32_t* order; const DevListReq* D; const ListLayout* L;      // D[k]: the page as a listing over the heads mask; L->count(k): its rows
    uint32_t *sorted, *perm, *sizes;        // at [k * INFX_POST_MAX_ROWS ..]: the page's group codes ascending, the row of each, the rows' sizes (zeroed)
};
extern "C++" {
// Req: infx_group_list_req, or a struct that begins with its fields.  The requests are checked and the call begun (c); info[]: where the call counts its head
// passes, histogram passes and kernel launches.  Per spec: head pass, heads mask, the pages (their rows to keys_out / docs_out / codes_out, each skipped
// where null), k_group_page, then walk(P) — which fills P.sizes and enqueues what else the call returns — and the way back of the group codes, the sizes and
// the totals.  Not synchronised.
template <class Req, class Walk>
static int32_t grouped_pages(SetCall& c, const Req* reqs, uint32_t* heads, uint32_t* histPasses, uint32_t* launches, int64_t* keys_out, int32_t* docs_out, uint32_t* codes_out,
                             uint32_t* gcodes_out, uint32_t* sizes_out, uint32_t* counts_out, uint32_t* group_totals_out, uint32_t* totals_out, Walk walk) {
    infx_stream* s = c.s; infx_index* ix = c.ix; SetKindState& K = *c.K; const int32_t n = c.n; const uint32_t nreq = c.nreq; uint32_t* order = c.order;
    uint32_t gvMax = 1;
    for (uint32_t i = 0; i < nreq; i++) gvMax = std::max(gvMax, ix->colValues[reqs[i].group_col]);
    // requests of one spec — (mask, group column, order column, direction) — follow one another: they share the head pass, the heads mask and the size walk
    for (uint32_t i = 0; i < nreq; i++) order[i] = i;
    auto same_spec = [&](uint32_t a, uint32_t b) { const Req &A = reqs[a], &B = reqs[b]; return A.mask == B.mask && A.group_col == B.group_col && A.col == B.col && (A.ascending != 0) == (B.ascending != 0); };
    std::stable_sort(order, order + nreq, [&](uint32_t a, uint32_t b) {
        const Req &A = reqs[a], &B = reqs[b];
        if (A.mask != B.mask) return std::less<const uint8_t*>()(A.mask, B.mask);
        if (A.group_col != B.group_col) return A.group_col < B.group_col;
        return A.col != B.col ? A.col < B.col : (A.ascending != 0) < (B.ascending != 0); });
    // workspace, one spec at a time: [head table | heads mask (whole groups of 16 bytes)]; then per spec its set's size, per request [sorted codes | rows | group codes | sizes]
    const size_t R = INFX_POST_MAX_ROWS, groups16 = ((size_t)n + LST_GROUP - 1) / LST_GROUP;
    const size_t oHeads = ((size_t)gvMax * 8 + 63) & ~(size_t)63, oTot = (oHeads + groups16 * LST_GROUP + 63) & ~(size_t)63, oSorted = oTot + INFX_MAX_PREFILTERS * 4;
    const size_t oPerm = oSorted + (size_t)nreq * R * 4, oGc = oPerm + (size_t)nreq * R * 4, oSizes = oGc + (size_t)nreq * R * 4;
    GROW(K.ws, K.capWs, oSizes + (size_t)nreq * R * 4);
    char* G0 = (char*)K.ws;
    uint32_t* dTot = (uint32_t*)(G0 + oTot); uint32_t* dSorted = (uint32_t*)(G0 + oSorted); uint32_t* dPerm = (uint32_t*)(G0 + oPerm);
    uint32_t* dGc = (uint32_t*)(G0 + oGc); uint32_t* dSizes = (uint32_t*)(G0 + oSizes);
    HIPCHK(hipMemsetAsync(dTot, 0, INFX_MAX_PREFILTERS * 4, s->st));
    s->unsynced = true;
    // the pages are listings over the heads mask
    DevListReq D[INFX_MAX_PREFILTERS];
    for (uint32_t k = 0; k < nreq; k++) {
        const Req& Q = reqs[order[k]];
        D[k] = list_dev_req(ix, (const uint8_t*)(G0 + oHeads), Q.col, Q.ascending != 0, Q.offset, Q.limit, Q.digit_bits);
    }
    ListLayout L;
    { int32_t rc_ = list_prepare(s, n, nreq, D, &L); if (rc_) return rc_; }
    const int64_t groups = (int64_t)groups16;
    uint32_t spec = 0;
    for (uint32_t k0 = 0, k1; k0 < nreq; k0 = k1, spec++) {
        k1 = run_end(order, k0, nreq, same_spec);
        const Req& Q = reqs[order[k0]];
        DevGroupSpec G{};
        G.mask = set_flags(ix, Q.mask); G.gcodes = ix->colCodes[Q.group_col]; G.gvals = ix->colValues[Q.group_col];
        G.ocodes = D[k0].codes; G.orank = D[k0].rank; G.onvals = D[k0].nvals; G.ascending = D[k0].ascending;
        G.table = (unsigned long long*)G0; G.heads = (uint8_t*)(G0 + oHeads); G.total = dTot + spec;
        if (n > 0) {
            HIPCHK(hipMemsetAsync(G.table, 0xFF, (size_t)std::max(G.gvals, 1u) * 8, s->st));
            // the table and the workgroup's member counter (two words) in LDS while they fit one of the two budgets
            const uint32_t words = 2u * G.gvals + 2u;
            G.inLds = words <= GRP_BIG_LDS_WORDS ? 1u : 0u;
            int threads, grid; { int32_t rc_ = merge_once_shape(ix, n, G.inLds ? words : 2u, &threads, &grid); if (rc_) return rc_; }
            const size_t lds = (size_t)(G.inLds ? words : 2u) * 4;
            HIPCHK(lds_limit((const void*)k_group_heads, ix->cfg.device, lds));
            k_group_heads<<<grid, threads, lds, s->st>>>(G, n);
            k_group_heads_mask<<<(int)std::min<int64_t>(FCM_MAXGRID, (groups + GRP_THREADS - 1) / GRP_THREADS), GRP_THREADS, 0, s->st>>>(G, n);
            HIPCHK(hipGetLastError());
            ++*heads; *launches += 2;
        }
        for (uint32_t k = k0; k < k1; k++) {
            const size_t at = (size_t)order[k] * R;
            int32_t rc_ = list_enqueue(s, L, k, D[k], keys_out ? keys_out + at : nullptr, docs_out ? docs_out + at : nullptr, codes_out ? codes_out + at : nullptr, histPasses, launches);
            if (rc_) return rc_;
        }
        k_group_page<<<k1 - k0, LST_SORT_THREADS, 0, s->st>>>(G.gcodes, n, L.docs(k0), L.count(k0), dGc + (size_t)k0 * R, dSorted + (size_t)k0 * R, dPerm + (size_t)k0 * R, dSizes + (size_t)k0 * R);
        HIPCHK(hipGetLastError());
        ++*launches;
        { const GroupPages P{G, k0, k1, order, D, &L, dSorted, dPerm, dSizes}; int32_t rc_ = walk(P); if (rc_) return rc_; }
        for (uint32_t k = k0; k < k1; k++) {
            const uint32_t i = order[k];
            DOWN(gcodes_out + (size_t)i * R, dGc + (size_t)k * R, (size_t)D[k].limit * 4);
            DOWN(sizes_out + (size_t)i * R, dSizes + (size_t)k * R, (size_t)D[k].limit * 4);
            DOWN(counts_out + i, L.count(k), 4);
            DOWN(group_totals_out + i, L.total(k), 4);
            DOWN(totals_out + i, dTot + spec, 4);
        }
    }
    return INFX_OK;
}
}
int32_t infx_list_grouped(infx_stream* s, uint32_t nreq, const infx_group_list_req* reqs, int64_t* keys_out, int32_t* docs_out, uint32_t* codes_out, uint32_t* gcodes_out,
                          uint32_t* sizes_out, uint32_t* counts_out, uint32_t* group_totals_out, uint32_t* totals_out) {
    SetCall c;
    const bool badArgs = nreq && (!reqs || !keys_out || !docs_out || !codes_out || !gcodes_out || !sizes_out || !counts_out || !group_totals_out || !totals_out);
    { int32_t rc_ = set_call_open(&c, s, SK_GROUPED, badArgs, nreq); if (rc_) return rc_; }
    infx_index* ix = c.ix; SetKindState& K = *c.K; const int32_t n = c.n;
    for (uint32_t i = 0; i < nreq; i++) {
        const infx_group_list_req& Q = reqs[i];
        { int32_t rc_ = check_page_request(Q.limit, Q.offset, Q.digit_bits); if (rc_) return rc_; }
        { int32_t rc_ = check_set_request(s, Q.mask, Q.col, false, "grouped listing"); if (rc_) return rc_; }
        { int32_t rc_ = check_group_column(ix, Q.group_col, "grouped listing"); if (rc_) return rc_; }
    }
    { int32_t rc_ = set_call_begin(&c); if (rc_) return rc_; }
    if (!nreq) return INFX_OK;
    // the walk behind a spec's pages: the sizes of the listed groups
    auto sizes_walk = [&](const GroupPages& P) -> int32_t {
        if (n <= 0) return INFX_OK;
        const size_t R = INFX_POST_MAX_ROWS;
        DevGroupSizes Z{};
        Z.mask = P.G.mask; Z.gcodes = P.G.gcodes; Z.nreq = P.k1 - P.k0;
        uint32_t words = 0;
        for (uint32_t k = P.k0; k < P.k1; k++) {
            const uint32_t q = k - P.k0;
            Z.cnt[q] = P.L->count(k); Z.sorted[q] = P.sorted + (size_t)k * R; Z.perm[q] = P.perm + (size_t)k * R; Z.sizes[q] = P.sizes + (size_t)k * R;
            Z.ldsOff[q] = words; Z.limit[q] = P.D[k].limit; words += 2u * P.D[k].limit;
        }
        int threads, grid; { int32_t rc_ = merge_once_shape(ix, n, words, &threads, &grid); if (rc_) return rc_; }
        HIPCHK(lds_limit((const void*)k_group_sizes, ix->cfg.device, (size_t)words * 4));
        k_group_sizes<<<grid, threads, (size_t)words * 4, s->st>>>(Z, n);
        HIPCHK(hipGetLastError());
        K.info[2]++;
        return INFX_OK;
    };
    { int32_t rc_ = grouped_pages(c, reqs, &K.info[0], &K.info[1], &K.info[2], keys_out, docs_out, codes_out, gcodes_out, sizes_out, counts_out, group_totals_out, totals_out, sizes_walk);
      if (rc_) return rc_; }
    SYNC();
    return INFX_OK;
}
int32_t infx_last_group_list_stats(infx_stream* s, uint32_t* head_passes, uint32_t* hist_passes, uint32_t* launches) {
    return put_info(s, SK_GROUPED, {head_passes, hist_passes, launches});
}
// ---- list_group_members: list_groups' page with the first per_group members of every listed group (group_members.hip.inc) ----
static_assert(GM_MAX_PER_GROUP == INFX_GROUP_MEMBERS_MAX_PER_GROUP && GM_MAX_SLOTS == INFX_GROUP_MEMBERS_MAX && GH_MAX_CODES == INFX_POST_MAX_ROWS, "group_members.h's limits are the interface's");
static_assert(gm_lds_words(INFX_POST_MAX_ROWS, INFX_GROUP_MEMBERS_MAX / INFX_POST_MAX_ROWS) <= STS_LDS_WORDS && gm_lds_words(INFX_GROUP_MEMBERS_MAX / INFX_GROUP_MEMBERS_MAX_PER_GROUP, INFX_GROUP_MEMBERS_MAX_PER_GROUP) <= STS_LDS_WORDS,
              "one request always fits a workgroup's LDS");
int32_t infx_list_group_members(infx_stream* s, uint32_t nreq, const infx_group_members_req* reqs, int32_t* rows_out, uint32_t* gcodes_out, uint32_t* sizes_out,
                                uint32_t* member_counts_out, int64_t* member_keys_out, int32_t* member_docs_out, uint32_t* member_codes_out,
                                uint32_t* counts_out, uint32_t* group_totals_out, uint32_t* totals_out) {
    SetCall c;
    const bool badArgs = nreq && (!reqs || !rows_out || !gcodes_out || !sizes_out || !member_counts_out || !member_keys_out || !member_docs_out || !member_codes_out ||
                                  !counts_out || !group_totals_out || !totals_out);
    { int32_t rc_ = set_call_open(&c, s, SK_MEMBERS, badArgs, nreq); if (rc_) return rc_; }
    infx_index* ix = c.ix; SetKindState& K = *c.K; const int32_t n = c.n;
    for (uint32_t i = 0; i < nreq; i++) {
        const infx_group_members_req& Q = reqs[i];
        { int32_t rc_ = check_page_request(Q.limit, Q.offset, Q.digit_bits); if (rc_) return rc_; }
        if (Q.per_group < 1 || Q.per_group > INFX_GROUP_MEMBERS_MAX_PER_GROUP) return fail(INFX_EINVAL, "a group-members request keeps 1 .. INFX_GROUP_MEMBERS_MAX_PER_GROUP (16) members per group%s");
        if (Q.limit * Q.per_group > INFX_GROUP_MEMBERS_MAX) return fail(INFX_EINVAL, "a group-members request's limit * per_group is at most INFX_GROUP_MEMBERS_MAX (4096)%s");
        { int32_t rc_ = check_set_request(s, Q.mask, Q.col, false, "group-members request"); if (rc_) return rc_; }
        { int32_t rc_ = check_group_column(ix, Q.group_col, "group-members request"); if (rc_) return rc_; }
    }
    { int32_t rc_ = set_call_begin(&c); if (rc_) return rc_; }
    if (!nreq) return INFX_OK;
    // output, request k of the device's order at [k * M ..]: [slots (all ones) | member keys | member documents | member codes], then R member counts each
    const size_t R = INFX_POST_MAX_ROWS, M = INFX_GROUP_MEMBERS_MAX;
    const size_t oKeys = (size_t)nreq * M * 8, oDocs = oKeys + (size_t)nreq * M * 8, oCodes = oDocs + (size_t)nreq * M * 4, oHeld = oCodes + (size_t)nreq * M * 4;
    GROW(K.out, K.capOut, oHeld + (size_t)nreq * R * 4);
    char* O = (char*)K.out;
    unsigned long long* dSlots = (unsigned long long*)O; long long* dKeys = (long long*)(O + oKeys); int32_t* dDocs = (int32_t*)(O + oDocs);
    uint32_t* dCodes = (uint32_t*)(O + oCodes); uint32_t* dHeld = (uint32_t*)(O + oHeld);
    HIPCHK(hipMemsetAsync(dSlots, 0xFF, (size_t)nreq * M * 8, s->st));
    s->unsynced = true;
    // the walk behind a spec's pages: the sizes of the listed groups and their first members, for as many consecutive requests per launch as the LDS of a CU holds
    auto members_walk = [&](const GroupPages& P) -> int32_t {
        DevMemberRows W{};
        for (uint32_t k0 = P.k0, k1; k0 < P.k1; k0 = k1) {
            DevGroupMembers Z{};
            Z.mask = P.G.mask; Z.gcodes = P.G.gcodes; Z.gvals = P.G.gvals; Z.ocodes = P.G.ocodes; Z.orank = P.G.orank; Z.onvals = P.G.onvals; Z.ascending = P.G.ascending;
            uint32_t words = 0;
            for (k1 = k0; k1 < P.k1; k1++) {
                const infx_group_members_req& Q = reqs[P.order[k1]];
                const uint32_t w = gm_lds_words(Q.limit, Q.per_group), q = k1 - k0;
                if (q && words + w > GM_PACK_LDS_WORDS) break;
                Z.cnt[q] = P.L->count(k1); Z.sorted[q] = P.sorted + (size_t)k1 * R; Z.perm[q] = P.perm + (size_t)k1 * R; Z.sizes[q] = P.sizes + (size_t)k1 * R;
                Z.slots[q] = dSlots + (size_t)k1 * M; Z.ldsOff[q] = words; Z.limit[q] = Q.limit; Z.perGroup[q] = Q.per_group; words += w;
                W.limit[k1 - P.k0] = Q.limit; W.perGroup[k1 - P.k0] = Q.per_group;
            }
            Z.nreq = k1 - k0;
            if (n <= 0) continue;
            int threads, grid; { int32_t rc_ = merge_once_shape(ix, n, words + GM_STATIC_LDS_WORDS, &threads, &grid); if (rc_) return rc_; }
            HIPCHK(lds_limit((const void*)k_group_members, ix->cfg.device, (size_t)words * 4));
            k_group_members<<<grid, threads, (size_t)words * 4, s->st>>>(Z, n);
            HIPCHK(hipGetLastError());
            K.info[2]++; K.info[3]++;
        }
        k_group_member_rows<<<P.k1 - P.k0, LST_SORT_THREADS, 0, s->st>>>(dSlots + (size_t)P.k0 * M, W, P.G.ocodes, n, (const long long*)ix->d.docKeyAll, dKeys + (size_t)P.k0 * M,
                                                                        dDocs + (size_t)P.k0 * M, dCodes + (size_t)P.k0 * M, dHeld + (size_t)P.k0 * R);
        HIPCHK(hipGetLastError());
        K.info[3]++;
        for (uint32_t k = P.k0; k < P.k1; k++) {
            const uint32_t i = P.order[k]; const size_t places = (size_t)reqs[i].limit * reqs[i].per_group;
            DOWN(member_keys_out + (size_t)i * M, dKeys + (size_t)k * M, places * 8);
            DOWN(member_docs_out + (size_t)i * M, dDocs + (size_t)k * M, places * 4);
            DOWN(member_codes_out + (size_t)i * M, dCodes + (size_t)k * M, places * 4);
            DOWN(member_counts_out + (size_t)i * R, dHeld + (size_t)k * R, (size_t)reqs[i].limit * 4);
        }
        return INFX_OK;
    };
    { int32_t rc_ = grouped_pages(c, reqs, &K.info[0], &K.info[1], &K.info[3], nullptr, rows_out, nullptr, gcodes_out, sizes_out, counts_out, group_totals_out, totals_out, members_walk);
      if (rc_) return rc_; }
    SYNC();
    return INFX_OK;
}
int32_t infx_last_group_members_stats(infx_stream* s, uint32_t* head_passes, uint32_t* hist_passes, uint32_t* member_walks, uint32_t* launches) {
    return put_info(s, SK_MEMBERS, {head_passes, hist_passes, member_walks, launches});
}
// ---- top_groups: a page of a document set's groups, ranked by a figure of the group (top_groups.hip.inc) ----
int32_t infx_top_groups(infx_stream* s, uint32_t nreq, const infx_top_req* reqs, uint32_t* codes_out, infx_stats_slot* slots_out, uint32_t* counts_out, uint32_t* group_totals_out, uint32_t* totals_out) {
    SetCall c;
    { int32_t rc_ = set_call_open(&c, s, SK_TOP, nreq && (!reqs || !codes_out || !slots_out || !counts_out || !group_totals_out || !totals_out), nreq); if (rc_) return rc_; }
    infx_index* ix = c.ix; SetKindState& K = *c.K; const int32_t n = c.n; const SetKey* key = c.key; const uint32_t* order = c.order;
    for (uint32_t i = 0; i < nreq; i++) {
        const infx_top_req& Q = reqs[i];
        { int32_t rc_ = check_page_request(Q.limit, Q.offset, Q.digit_bits); if (rc_) return rc_; }
        { int32_t rc_ = check_set_request(s, Q.mask, Q.col, false, "top-groups request"); if (rc_) return rc_; }
        { int32_t rc_ = check_group_column(ix, Q.group_col, "top-groups request"); if (rc_) return rc_; }
        if (!ix->colTieOk[Q.group_col]) return fail(INFX_EINVAL, "the top-groups request's group rank was not uploaded%s");
        if (Q.by >= TS_BYS) return fail(INFX_EINVAL, "a top-groups request ranks by size, count, min, max, sum or mean (0 .. 5)%s");
        if (Q.col < 0 && Q.by != TS_BY_SIZE) return fail(INFX_EINVAL, "without a value column a top-groups request ranks by size%s");
        if (Q.col >= 0 && !ix->colBitsOk[Q.col]) return fail(INFX_EINVAL, "the top-groups request's value table was not uploaded%s");
        c.key[i] = SetKey{Q.mask, Q.col, Q.group_col};
    }
    { int32_t rc_ = set_call_begin(&c); if (rc_) return rc_; }
    if (!nreq) return INFX_OK;
    auto same_table = [&](uint32_t a, uint32_t b) { return key[a].mask == key[b].mask && key[a].col == key[b].col && key[a].gcol == key[b].gcol; };
    // per request (device order) what its select needs; per table the words of its slots and smallest ranks and of its requests' composites
    uint32_t figWords[TOP_MAX_REQS], passes[TOP_MAX_REQS]; size_t keyOff[TOP_MAX_REQS], tabWords = 0, keyWords = 0;
    for (uint32_t k0 = 0, k1; k0 < nreq; k0 = k1) {
        k1 = run_end(order, k0, nreq, same_table);
        const infx_top_req& Q = reqs[order[k0]];
        const size_t gv = ix->colValues[Q.group_col];
        tabWords = std::max(tabWords, Q.col >= 0 ? gv * (sts_stride(ix->colLimbs[Q.col]) + 1u) : gv);
        size_t kw = 0;
        for (uint32_t k = k0; k < k1; k++) {
            const infx_top_req& R = reqs[order[k]];
            figWords[k] = ts_fig_words(R.by, R.col >= 0 ? ix->colKind[R.col] : XS_KIND_INT); passes[k] = ts_passes(figWords[k], R.digit_bits);
            keyOff[k] = kw; kw += gv * ts_key_words(figWords[k]);
        }
        keyWords = std::max(keyWords, kw);
    }
    const size_t stBytes = (sizeof(DevTopState) + 63) & ~(size_t)63;
    const size_t oKeys = (tabWords * 4 + 63) & ~(size_t)63, oHist = (oKeys + keyWords * 4 + 63) & ~(size_t)63, oState = oHist + (size_t)nreq * 2 * LS_MAX_BINS * 4;
    GROW(K.ws, K.capWs, oState + nreq * stBytes);
    GROW(K.out, K.capOut, (size_t)nreq * TOP_OUT_WORDS * 4);
    char* W = (char*)K.ws; uint32_t* O = (uint32_t*)K.out;
    HIPCHK(hipMemsetAsync(W + oHist, 0, oState + nreq * stBytes - oHist, s->st));
    HIPCHK(hipMemsetAsync(O, 0, (size_t)nreq * TOP_OUT_WORDS * 4, s->st));
    s->unsynced = true;
    for (uint32_t k0 = 0, k1; k0 < nreq; k0 = k1) {
        k1 = run_end(order, k0, nreq, same_table);
        const infx_top_req& Q = reqs[order[k0]];
        const uint32_t gv = ix->colValues[Q.group_col], nl = Q.col >= 0 ? ix->colLimbs[Q.col] : 0u, stride = Q.col >= 0 ? sts_stride(nl) : 1u;
        uint32_t* slots = (uint32_t*)W; uint32_t* lo = slots + (size_t)gv * stride;
        // 1. accumulate: the table's slots, placed as field_stats places one request's
        if (gv) HIPCHK(hipMemsetAsync(slots, 0, (size_t)gv * stride * 4, s->st));
        if (gv && Q.col >= 0) HIPCHK(hipMemsetAsync(lo, 0xFF, (size_t)gv * 4, s->st));
        if (n > 0 && gv) {
            const uint32_t words = gv * stride; uint32_t ldsOff = 0;
            const uint32_t ldsWords = (uint64_t)gv * stride > STS_BIG_LDS_WORDS ? (ldsOff = STS_GLOBAL, 0u) : sts_place_best(1, &words, stats_big_lds(), &ldsOff);
            int threads, grid; { int32_t rc_ = merge_once_shape(ix, n, ldsWords, &threads, &grid); if (rc_) return rc_; }
            if (Q.col >= 0) {
                DevStatsCall P{}; P.nreq = 1;
                P.r[0] = stats_dev_req(ix, Q.mask, Q.col, Q.group_col, gv, slots, lo, ldsOff);
                HIPCHK(lds_limit((const void*)k_field_stats, ix->cfg.device, (size_t)ldsWords * 4));
                k_field_stats<<<grid, threads, (size_t)ldsWords * 4, s->st>>>(P, n);
            } else {
                HIPCHK(lds_limit((const void*)k_top_sizes, ix->cfg.device, (size_t)ldsWords * 4));
                k_top_sizes<<<grid, threads, (size_t)ldsWords * 4, s->st>>>(set_flags(ix, Q.mask), ix->colCodes[Q.group_col], gv, slots, ldsOff != STS_GLOBAL ? 1u : 0u, n);
            }
            HIPCHK(hipGetLastError());
            K.info[1]++; K.info[3]++;
            K.info[ldsOff == STS_GLOBAL ? 6 : ldsWords <= STS_LDS_WORDS ? 4 : 5]++;
        }
        // 2. keys; 3. select: the requests that still have a pass, in one launch each for histogram and pick; 4. the pages
        DevTopCall P{}; P.nreq = k1 - k0;
        uint32_t maxPasses = 0;
        for (uint32_t k = k0; k < k1; k++) {
            const infx_top_req& R = reqs[order[k]];
            DevTopReq& D = P.r[k - k0];
            D.slots = slots; D.lo = Q.col >= 0 ? lo : nullptr; D.tie = ix->colTie[Q.group_col];
            D.keys = (uint32_t*)(W + oKeys) + keyOff[k]; D.hist = (uint32_t*)(W + oHist) + (size_t)k * 2 * LS_MAX_BINS; D.st = (DevTopState*)(W + oState + k * stBytes);
            D.out = O + (size_t)k * TOP_OUT_WORDS;
            D.gvals = gv; D.stride = stride; D.nlimbs = nl; D.by = R.by; D.kind = Q.col >= 0 ? ix->colKind[Q.col] : XS_KIND_INT; D.scale = Q.col >= 0 ? ix->colScale[Q.col] : 0;
            D.ascending = R.ascending ? 1u : 0u; D.offset = R.offset; D.limit = R.limit; D.digitBits = R.digit_bits; D.figWords = figWords[k]; D.passes = passes[k];
            maxPasses = std::max(maxPasses, passes[k]);
        }
        const int blocks = (int)std::max<int64_t>(1, std::min<int64_t>(FCM_MAXGRID, ((int64_t)gv + TOP_THREADS - 1) / TOP_THREADS));
        k_top_keys<<<dim3(blocks, P.nreq), TOP_THREADS, 0, s->st>>>(P);
        K.info[3]++;
        for (uint32_t p = 0; p < maxPasses; p++) {
            DevTopCall A{}; uint32_t bits = LS_MIN_DIGIT_BITS;
            for (uint32_t q = 0; q < P.nreq; q++) if (P.r[q].passes > p) { A.r[A.nreq++] = P.r[q]; bits = std::max(bits, P.r[q].digitBits); }
            k_top_hist<<<dim3(blocks, A.nreq), TOP_THREADS, ((size_t)2 << bits) * 4, s->st>>>(A, p);
            k_top_pick<<<A.nreq, TOP_THREADS, 0, s->st>>>(A, p);
            K.info[2]++; K.info[3] += 2;
        }
        k_top_gather<<<dim3(blocks, P.nreq), TOP_THREADS, 0, s->st>>>(P);
        k_top_page<<<P.nreq, LST_SORT_THREADS, 0, s->st>>>(P);
        HIPCHK(hipGetLastError());
        K.info[3] += 2;
    }
    { int32_t rc_ = set_fetch_raw(c, (size_t)nreq * TOP_OUT_WORDS); if (rc_) return rc_; }
    for (uint32_t k = 0; k < nreq; k++) {
        const uint32_t i = order[k]; const uint32_t* w = K.raw.data() + (size_t)k * TOP_OUT_WORDS;
        const uint32_t rows = std::min<uint32_t>(w[0], INFX_POST_MAX_ROWS);
        counts_out[i] = rows; group_totals_out[i] = w[1]; totals_out[i] = w[2];
        for (uint32_t r = 0; r < rows; r++) {
            codes_out[(size_t)i * INFX_POST_MAX_ROWS + r] = w[TOP_OUT_HEAD + r];
            const uint32_t* v = w + TOP_OUT_HEAD + INFX_POST_MAX_ROWS + (size_t)r * TOP_SLOT_WORDS;
            slots_out[(size_t)i * INFX_POST_MAX_ROWS + r] = stats_slot(v, INFX_STATS_MAX_LIMBS, v[5]);      // (a page's slot: every limb, the smallest rank in word 5)
        }
    }
    return INFX_OK;
}
int32_t infx_last_top_groups_info(infx_stream* s, uint32_t* requests, uint32_t* accumulate_passes, uint32_t* select_passes, uint32_t* launches, uint32_t* small_lds, uint32_t* big_lds, uint32_t* in_global) {
    return put_info(s, SK_TOP, {requests, accumulate_passes, select_passes, launches, small_lds, big_lds, in_global});
}
// ---- field_distinct: the distinct values of a column over a document set, whole and per group (distinct.hip.inc) ----
// Where a spec's pairs are marked (DST_PLACE_*) under `mode`, and — for LDS — the words of the workgroup: k_field_stats' two budgets decide whether the rows
// and their size counters fit; between the global bitmap and the hash set the smaller workspace wins (profiles/field_distinct.md).  A forced placement that
// does not fit falls to the next larger one.
static uint32_t dst_place(uint32_t mode, uint32_t gv, uint32_t fv, uint64_t docs, bool big, uint32_t* ldsWords) {
    const uint64_t rows = ds_bitmap_words(gv, fv);
    *ldsWords = 0;
    if (mode <= DST_PLACE_LDS && rows + gv <= STS_BIG_LDS_WORDS) {
        const uint32_t words = (uint32_t)rows + gv; uint32_t off = 0;
        const uint32_t used = sts_place_best(1, &words, big, &off);
        if (off != STS_GLOBAL) { *ldsWords = used; return DST_PLACE_LDS; }
    }
    if (mode == DST_PLACE_HASH || !ds_bitmap_fits(gv, fv)) return DST_PLACE_HASH;
    if (mode != DST_PLACE_AUTO) return DST_PLACE_BITMAP;
    return (rows + (gv > 1 ? ds_row_words(fv) : 0u)) * 4u <= ds_capacity(ds_max_pairs(docs, gv, fv)) * 8u ? DST_PLACE_BITMAP : DST_PLACE_HASH;
}
static int dst_count_grid(uint32_t words) { return (int)std::max<int64_t>(1, std::min<int64_t>(DST_COUNT_GRID, ((int64_t)words + DST_COUNT_THREADS - 1) / DST_COUNT_THREADS)); }
int32_t infx_field_distinct(infx_stream* s, uint32_t nreq, const infx_distinct_req* reqs, uint32_t* distinct_out, uint32_t* totals_out, uint32_t* group_sizes_out, uint32_t* group_distinct_out) {
    SetCall c;
    { int32_t rc_ = set_call_open(&c, s, SK_DISTINCT, nreq && (!reqs || !distinct_out || !totals_out || !group_sizes_out || !group_distinct_out), nreq); if (rc_) return rc_; }
    infx_index* ix = c.ix; SetKindState& K = *c.K; const int32_t n = c.n; const SetKey* key = c.key; const uint32_t* order = c.order;
    for (uint32_t i = 0; i < nreq; i++) {
        const infx_distinct_req& Q = reqs[i];
        { int32_t rc_ = check_set_request(s, Q.mask, -1, false, "field-distinct request"); if (rc_) return rc_; }
        if (Q.col < 0 || Q.col >= FILT_MAXCOL || !ix->colCodes[Q.col]) return fail(INFX_EINVAL, "the field-distinct request's column was not uploaded%s");
        { int32_t rc_ = columns_cover(ix, ix->d.totalDocs, COLS_COVER_CORPUS, Q.col); if (rc_) return rc_; }
        if (Q.group_col >= 0) { int32_t rc_ = check_group_slots(ix, Q.group_col, "field-distinct request"); if (rc_) return rc_; }
        if (Q.placement > DST_PLACE_HASH) return fail(INFX_EINVAL, "a field-distinct request's placement is 0 (automatic), 1 (LDS), 2 (global bitmap) or 3 (hash set)%s");
        c.key[i] = SetKey{Q.mask, Q.col, Q.group_col >= 0 ? Q.group_col : -1};
    }
    { int32_t rc_ = set_call_begin(&c); if (rc_) return rc_; }
    if (!nreq) return INFX_OK;
    auto same_spec = [&](uint32_t a, uint32_t b) { return key[a].mask == key[b].mask && key[a].col == key[b].col && key[a].gcol == key[b].gcol && reqs[a].placement == reqs[b].placement; };
    // per spec (device order): its placement, its words of LDS, its bytes of workspace and where its counters lie in the output
    uint32_t place[DST_MAX_REQS] = {}, ldsWords[DST_MAX_REQS] = {}; size_t outOff[DST_MAX_REQS] = {}, wsBytes = 64, outWords = 0;
    for (uint32_t k0 = 0; k0 < nreq; k0 = run_end(order, k0, nreq, same_spec)) {
        const infx_distinct_req& Q = reqs[order[k0]];
        const uint32_t gv = Q.group_col >= 0 ? ix->colValues[Q.group_col] : 1u, fv = ix->colValues[Q.col], row = ds_row_words(fv);
        place[k0] = dst_place(Q.placement, gv, fv, (uint64_t)n, stats_big_lds(), &ldsWords[k0]);
        wsBytes = std::max(wsBytes, place[k0] == DST_PLACE_HASH ? (size_t)ds_capacity(ds_max_pairs((uint64_t)n, gv, fv)) * 8 + (size_t)row * 4
                                                                : ((size_t)ds_bitmap_words(gv, fv) + row) * 4);
        outOff[k0] = outWords; outWords += 2 * (size_t)gv + 2;
    }
    GROW(K.ws, K.capWs, wsBytes);
    GROW(K.out, K.capOut, outWords * 4);
    uint32_t* O = (uint32_t*)K.out;
    HIPCHK(hipMemsetAsync(O, 0, outWords * 4, s->st));
    s->unsynced = true;
    for (uint32_t k0 = 0; k0 < nreq; k0 = run_end(order, k0, nreq, same_spec)) {
        const infx_distinct_req& Q = reqs[order[k0]];
        const bool grouped = Q.group_col >= 0;
        const uint32_t gv = grouped ? ix->colValues[Q.group_col] : 1u, fv = ix->colValues[Q.col], row = ds_row_words(fv);
        if (n > 0 && gv && fv) {
            DevDistinct D{};
            D.mask = set_flags(ix, Q.mask); D.fcodes = ix->colCodes[Q.col]; D.gcodes = grouped ? ix->colCodes[Q.group_col] : nullptr;
            D.gvals = gv; D.fvals = fv; D.rowWords = row;
            D.sizes = O + outOff[k0]; D.distinct = D.sizes + gv; uint32_t* whole = D.distinct + gv; D.overflow = whole + 1;
            const uint32_t rows = gv * row;                    // (placements 1 and 2: below 2^27)
            uint32_t* uni = nullptr;                           // the row whose bits are the whole set's values, where it is not the spec's one row
            int threads, grid;
            if (place[k0] == DST_PLACE_HASH) {
                D.capacity = ds_capacity(ds_max_pairs((uint64_t)n, gv, fv)); D.table = (unsigned long long*)K.ws;
                if (gv > 1) D.side = uni = (uint32_t*)(D.table + D.capacity);
                HIPCHK(hipMemsetAsync(D.table, 0, (size_t)D.capacity * 8 + (gv > 1 ? (size_t)row * 4 : 0), s->st));
                { int32_t rc_ = merge_once_shape(ix, n, 2u * gv, &threads, &grid); if (rc_) return rc_; }
                k_distinct_hash<<<grid, threads, (size_t)2 * gv * 4, s->st>>>(D, n);
            } else {
                D.bits = (uint32_t*)K.ws;
                if (gv > 1) uni = D.bits + rows;
                HIPCHK(hipMemsetAsync(D.bits, 0, ((size_t)rows + (gv > 1 ? row : 0u)) * 4, s->st));
                if (place[k0] == DST_PLACE_LDS) {
                    { int32_t rc_ = merge_once_shape(ix, n, ldsWords[k0], &threads, &grid); if (rc_) return rc_; }
                    HIPCHK(lds_limit((const void*)k_distinct_lds, ix->cfg.device, (size_t)ldsWords[k0] * 4));
                    k_distinct_lds<<<grid, threads, (size_t)ldsWords[k0] * 4, s->st>>>(D, n);
                } else {
                    { int32_t rc_ = merge_once_shape(ix, n, gv, &threads, &grid); if (rc_) return rc_; }
                    k_distinct_bitmap<<<grid, threads, (size_t)gv * 4, s->st>>>(D, n);
                }
                k_distinct_count<<<dst_count_grid(rows), DST_COUNT_THREADS, 0, s->st>>>(D.bits, rows, row, D.distinct);
                K.info[1]++;
                if (uni) {
                    const dim3 ug((unsigned)std::min<int64_t>(FCM_MAXGRID, ((int64_t)row + DST_COUNT_THREADS - 1) / DST_COUNT_THREADS), (gv + DST_UNION_ROWS - 1) / DST_UNION_ROWS);
                    k_distinct_union<<<ug, DST_COUNT_THREADS, 0, s->st>>>(D.bits, gv, row, DST_UNION_ROWS, uni);
                    K.info[1]++;
                }
            }
            // the whole set's figure: the bits of the union (side) row; with one row the host takes that row's counter
            if (uni) { k_distinct_count<<<dst_count_grid(row), DST_COUNT_THREADS, 0, s->st>>>(uni, row, row, whole); K.info[1]++; }
            HIPCHK(hipGetLastError());
            K.info[1]++; K.info[1 + place[k0]]++;
        }
    }
    { int32_t rc_ = set_fetch_raw(c, outWords); if (rc_) return rc_; }
    for (uint32_t k0 = 0, k1; k0 < nreq; k0 = k1) {
        k1 = run_end(order, k0, nreq, same_spec);
        const infx_distinct_req& Q = reqs[order[k0]];
        const bool grouped = Q.group_col >= 0;
        const uint32_t gv = grouped ? ix->colValues[Q.group_col] : 1u;
        const uint32_t *sizes = K.raw.data() + outOff[k0], *distinct = sizes + gv;
        if (distinct[gv + 1]) return fail(INFX_ECAPACITY, "field-distinct: the hash set of a request overflowed%s");      // (sized never to: a broken table, not a large request)
        uint32_t total = 0; for (uint32_t g = 0; g < gv; g++) total += sizes[g];
        for (uint32_t k = k0; k < k1; k++) {
            const uint32_t i = order[k];
            distinct_out[i] = gv > 1 ? distinct[gv] : (gv ? distinct[0] : 0u); totals_out[i] = total;      // (one row: that row is the whole)
            if (grouped && gv) {
                std::memcpy(group_sizes_out + (size_t)i * INFX_STATS_MAX_GROUPS, sizes, (size_t)gv * 4);
                std::memcpy(group_distinct_out + (size_t)i * INFX_STATS_MAX_GROUPS, distinct, (size_t)gv * 4);
            }
        }
    }
    return INFX_OK;
}
int32_t infx_last_field_distinct_info(infx_stream* s, uint32_t* requests, uint32_t* launches, uint32_t* lds_passes, uint32_t* bitmap_passes, uint32_t* hash_passes) {
    return put_info(s, SK_DISTINCT, {requests, launches, lds_passes, bitmap_passes, hash_passes});
}
int32_t infx_stream_mask_slot(infx_stream* s, uint32_t slot, uint8_t** out) {
    if (!s || !out || slot >= INFX_MAX_PREFILTERS) return fail(INFX_EINVAL, "bad mask slot%s");
    infx_index* ix = s->ix;
    if (!ix->haveDocs) return fail(INFX_EINVAL, "index not uploaded%s");
    const size_t need = mask_bytes(ix);
    if (s->capMask[slot] < need) {
        HIPCHK(enter_device(ix->cfg.device));
        if (s->unsynced) { int32_t rc_ = stream_sync(s); if (rc_) return rc_; }      // work queued on the old buffer
        if (s->dMask[slot]) ws_release(s, s->dMask[slot]);
        s->dMask[slot] = nullptr; s->capMask[slot] = 0;
        void* p = nullptr;
        if (hipMalloc(&p, need) != hipSuccess) return fail(INFX_ENOMEM, "hipMalloc of a document mask failed%s");
        s->dMask[slot] = (uint8_t*)p; s->capMask[slot] = need;
    }
    *out = s->dMask[slot];
    return INFX_OK;
}
int32_t infx_filter_masks(infx_stream* s, uint32_t k, const infx_filter_prog* progs, uint8_t* const* masks, uint32_t* counts) {
    if (!s || (k && (!progs || !masks))) return fail(INFX_EINVAL, "null argument%s");
    s->mkStaged = false; s->mkTable.clear(); s->mkCountsOut = nullptr;
    if (!k) return INFX_OK;
    if (k > INFX_MAX_PREFILTERS) return fail(INFX_ECAPACITY, "more than INFX_MAX_PREFILTERS (16) masks in one build%s");
    infx_index* ix = s->ix;
    if (!ix->haveDocs) return fail(INFX_EINVAL, "index not uploaded%s");
    for (uint32_t i = 0; i < k; i++) {
        if (mask_slot_of(s, masks[i]) < 0) return fail(INFX_EINVAL, "a mask buffer is not a mask slot of this stream%s");
        for (uint32_t j = 0; j < i; j++) if (masks[j] == masks[i]) return fail(INFX_EINVAL, "two masks of one build share a slot%s");
    }
    { int32_t rc_ = s->mkTable.pack(ix, k, progs); if (rc_) { s->mkTable.clear(); return rc_; } }
    s->mkOut = DevMaskOut{}; for (uint32_t i = 0; i < k; i++) s->mkOut.mask[i] = masks[i];
    s->mkCountsOut = counts; s->mkStaged = true;
    return INFX_OK;
}
int32_t infx_stream_set_doc_masks(infx_stream* s, uint32_t nq, const uint8_t* const* masks) {
    if (!s || (nq && !masks)) return fail(INFX_EINVAL, "null argument%s");
    s->docMasks.clear();
    // the masks hold one byte per GLOBAL internal id (a sharded index may build them, for infx_list_ordered); a shard's queries read flags by shard-local id
    for (uint32_t i = 0; i < nq; i++) if (masks[i] && (s->ix->nranks > 1 || s->ix->d.docBase != 0)) return fail(INFX_EUNSUPPORTED, "document masks need an unsharded index%s");
    for (uint32_t i = 0; i < nq; i++) if (masks[i] && mask_slot_of(s, masks[i]) < 0) return fail(INFX_EINVAL, "a document mask is not a mask slot of this stream%s");
    s->docMasks.assign(masks, masks + nq);
    return INFX_OK;
}
int32_t infx_last_filter_mask_stats(infx_stream* s, uint32_t* built, uint32_t* launches) {
    if (!s) return fail(INFX_EINVAL, "null argument%s");
    if (built) *built = s->lastMaskBuilt;
    if (launches) *launches = s->lastMaskLaunches;
    return INFX_OK;
}
int32_t infx_last_filter_count_stats(infx_stream* s, uint32_t* counted, uint32_t* launches) {
    if (!s) return fail(INFX_EINVAL, "null argument%s");
    if (counted) *counted = s->lastCountK;
    if (launches) *launches = s->lastCountLaunches;
    return INFX_OK;
}
int32_t infx_last_facets(infx_stream* s, uint32_t nq, uint32_t* codes_out, uint32_t* counts_out, uint32_t* n_out) {
    if (!s || !codes_out || !counts_out || !n_out) return fail(INFX_EINVAL, "null argument%s");
    if (nq != s->facetNq || !s->facetNFacet) return fail(INFX_EINVAL, "no facets of a batch of this size on the stream%s");
    const size_t rows = s->ix->postRows, w = s->facetRows, slices = (size_t)nq * s->facetNFacet;      // the caller's stride: the index's post rows
    if (w == rows) { std::memcpy(codes_out, s->hFacCodes.data(), s->hFacCodes.size() * 4); std::memcpy(counts_out, s->hFacCounts.data(), s->hFacCounts.size() * 4); }
    else for (size_t i = 0; i < slices; i++) { std::memcpy(codes_out + i * rows, s->hFacCodes.data() + i * w, w * 4); std::memcpy(counts_out + i * rows, s->hFacCounts.data() + i * w, w * 4); }
    std::memcpy(n_out, s->hFacN.data(), s->hFacN.size() * 4);
    return INFX_OK;
}

int32_t infx_last_facets_of(infx_stream* s, uint32_t nq, uint32_t q, uint32_t k, uint32_t* codes_out, uint32_t* counts_out, uint32_t* n_out) {
    if (!s || !codes_out || !counts_out || !n_out) return fail(INFX_EINVAL, "null argument%s");
    if (nq != s->facetNq || !s->facetNFacet || q >= nq || k >= s->facetNFacet) return fail(INFX_EINVAL, "no facets of a batch of this size on the stream%s");
    const size_t i = (size_t)q * s->facetNFacet + k, rows = s->facetRows;
    const uint32_t n = std::min<uint32_t>(s->hFacN[i], (uint32_t)rows);
    std::memcpy(codes_out, s->hFacCodes.data() + i * rows, (size_t)n * 4); std::memcpy(counts_out, s->hFacCounts.data() + i * rows, (size_t)n * 4);
    *n_out = n;
    return INFX_OK;
}
} // extern "C"
