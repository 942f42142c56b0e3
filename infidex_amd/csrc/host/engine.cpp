// Host engine of the product: the C++ stand-in for the reference's C# SearchEngine (no .NET toolchain in the image).
// Same surface for the hot path — CreateDefault/CreateMinimal, IndexDocuments, Search(Query) — with the two accelerated
// seams delegated to the HIP kernels through the C ABI of include/infidex_hip.h. There is NO CPU scoring path here: without
// a GPU Search fails with INFX_EHIP.
//   SearchEngine.Search / IndexDocuments     src/Infidex/SearchEngine.cs:96-192, 256-319
//   SearchPipeline.Execute                   src/Infidex/Scoring/SearchPipeline.cs:49-206 (gates), :298-447 (coverage stage)
//   ResultProcessor.CalculateTruncationIndex src/Infidex/Scoring/ResultProcessor.cs:146-178
//   TopKHeap / ScoreEntry / ConsolidateSegments  Core/TopKHeap.cs, Core/ScoreEntry.cs:25-36, Scoring/SegmentProcessor.cs:15-37
#include "query.h"
#include "filter.h"
#include "list_columns.h"
#include "infdx2.h"
#include "infdx2_verify.h"
#include "infs.h"
#include "hostcache.h"
#include <array>
#include <mutex>
#include <condition_variable>
#include "../../../include/infidex_engine.h"
#define XS_FN static inline
#include "../exact_sum.h"
#define TS_BYS 6                            // the figures infx_top_groups ranks by (INFX_TOP_BY_*), in the order of their names
#include <chrono>
#include <map>
#include <list>
#include <unordered_map>
#include <unordered_set>
#include <cstdio>
#include <cstdlib>

using namespace infx;

namespace {
thread_local std::string g_eerr;
int32_t efail(int32_t code, const std::string& m) { g_eerr = m; return code; }
double now_ms() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

struct Entry { float score; int64_t key; uint8_t tie; };
inline int cmp_entry(const Entry& a, const Entry& b) {    // ScoreEntry.CompareTo
    if (a.score != b.score) return a.score < b.score ? -1 : 1;
    if (a.tie != b.tie) return a.tie < b.tie ? -1 : 1;
    return b.key < a.key ? -1 : (b.key > a.key ? 1 : 0);
}
}

// One in-flight batch: its own HIP stream + scratch. Several sessions on one engine let the host preparation of one batch
// overlap the GPU stages of another (SearchEngine.Search is callable from many threads concurrently, SearchEngine.cs:258).
struct FusedIn;
struct PerQ {
    std::vector<Entry> stage1;          // consolidated Stage-1 (score desc, key asc)
    std::vector<int32_t> stage1Doc;     // global internal ids
    bool runCov = false, wmAny = false, done = false, envelope = false;   // envelope: the query exceeds the Stage-2 query envelope -> answered as unsupported
    uint32_t candOff = 0, candCount = 0; int covIndex = -1;
    int32_t idx0 = -1, idx1 = -1;       // docs with docIndex 0 / 1
};
struct Batch {
    uint32_t nq = 0, nd = 0; int depth = 0, maxResults = 0;
    std::vector<infx_query> dq; std::vector<infx_term> dterms; std::vector<int32_t> extra; std::vector<uint32_t> qmap; std::vector<int> devOf;
    std::vector<infx_counts> counts;
    std::vector<PerQ> pq;
    std::vector<uint32_t> localIdx;     // local Stage-2 candidates -> position in lastCands
    std::vector<std::shared_ptr<FuzzyUnion>> pending; std::vector<uint32_t> pendingCounts; std::unordered_map<const FuzzyUnion*, uint32_t> unionIdx;   // unions whose df this batch counts
    double t0 = 0, t1 = 0, t2 = 0, t3 = 0, t4 = 0, tPlanPar = 0, tTok = 0, tUnion = 0;
    double tLd1Dev = 0, tUnionDev = 0;      // of the planning time: spent inside infx_ld1_expand / infx_union_build (device work + the wait for it)
    std::shared_ptr<FusedIn> pre;      // sharded phases: per-query device-pipeline inputs prepared in phase 0 (off the collective path)
};

// What the four per-query parts of the session's next batch share ("One frame behind the per-query parts"): whether the part is installed and for
// how many queries, and per query whether the part refuses it, with which status and why
struct QueryPart {
    bool on = false, bound = false; uint32_t nq = 0;      // bound: a sharded phase 0 took the part for its batch (a second phase 0 finds it stale)
    std::vector<uint8_t> reject; std::vector<int32_t> status; std::vector<std::string> err;
    void open(uint32_t n) { nq = n; reject.assign(n, 0); status.assign(n, INFX_OK); err.assign(n, std::string()); }
    void refuse(uint32_t i, int32_t rc, const std::string& why) { reject[i] = 1; status[i] = rc; err[i] = why; }
};
// The parts in their fixed order: a query that several refuse reports the first one's message
enum { QP_OPTIONS, QP_COVERAGE, QP_PREFILTERS, QP_COLLAPSE, QP_HIGHLIGHT, QP_PARTS };
static const char* const QUERY_PART_NAMES[QP_PARTS] = {"options", "coverage setups", "pre-filters", "collapse requests", "highlight requests"};
// Per-query options of the session's next batch (infx_engine_set_query_options): consumed by that batch, whichever search path runs it
struct QueryOpts : QueryPart {
    std::vector<int32_t> maxResults; std::vector<uint8_t> cov, facets;      // facets: the query counts facets (a blank text then browses)
    std::vector<std::string> filterExpr;       // per query: its filter ("" = none), for NumberOfDocumentsInFilter after the batch
    std::vector<std::string> pinned;           // cache entries the batch holds (filters and boosts)
    std::vector<std::string> countExprs; std::vector<uint32_t> counts;      // expressions the batch counts first (programs [0, n) of its table) + the device's counts
};
// Per-query CoverageSetup of the session's next batch (infx_engine_set_query_coverage): consumed by that batch like QueryOpts, with or without them.
// fin / qLimit / relativeq: the six members SearchPipeline reads, already resolved against the engine-wide setup for a query without one of its own.
struct QueryCov : QueryPart { std::vector<infx_finalize_setup> fin; std::vector<int32_t> qLimit; std::vector<double> relativeq; };
// Pre-filters of the session's next batch (infx_engine_set_query_prefilters): consumed by that batch like QueryCov, with or without QueryOpts.
struct QueryPre : QueryPart {
    std::vector<std::string> expr;             // per query: its pre-filter ("" = none, or refused)
    std::vector<uint8_t> has;                  // the query asked for one
    std::vector<std::string> pinned;           // cache entries the batch holds
};
// Query.collapse_by of the session's next batch (infx_engine_set_query_collapse): consumed by that batch like QueryPre, with or without QueryOpts.
struct QueryClp : QueryPart {
    std::vector<int32_t> col, keep;            // per query: its column (-1: none, or refused) and the rows kept per group
    std::vector<uint8_t> has;                  // the query asked for it
};
// Query.highlight of the session's next batch (infx_engine_set_query_highlight): consumed by that batch like QueryClp, with or without QueryOpts.
struct QueryHl : QueryPart {
    std::vector<int32_t> chars;                // per query: its snippet width (0: none, or refused)
    std::vector<uint8_t> has;                  // the query asked for it
    bool asks(uint32_t i) const { return on && i < nq && has[i] && !reject[i]; }
};
// A highlighted query of the session's last batch: its Stage-2 words (the text they are slices of, their offsets and lengths, in Stage 2's order)
struct HlQuery { std::vector<uint16_t> text, off, len; bool longQuery = false; };
// One mask of the session's cache (mask slot i of its stream): the expression it was built from, the engine's mask epoch at that time, the live documents
// it accepts, when it was last used (least recently used first out)
struct PreMask { std::string expr; uint64_t epoch = 0, lastUse = 0; uint32_t count = 0; bool valid = false; };
// The facets of one Infiscript expression (infx_engine_facets_filtered), as the engine caches them: per facet column the ordered (code, count) list, cut to 100,
// and the number of live documents the expression accepts; valid for the mask epoch it was counted in
struct FfEntry { uint64_t epoch = 0; uint32_t total = 0; std::vector<std::vector<std::pair<uint32_t, uint32_t>>> lists, listLists; std::list<std::string>::iterator lru; };      // listLists: the facetable list columns, after the scalar ones
// What the answer to one request of a per-request call begins with: its status and message (why it was refused) and the size of its set (0 when refused)
struct Answer { int32_t status = INFX_OK; std::string err; uint32_t total = 0; };
// answer `which` of a session's last per-request call (null: no session, or no such answer)
template <class A> static const A* answer_at(const std::vector<A>* v, uint32_t which) { return v && which < v->size() ? &(*v)[which] : nullptr; }
struct FfAnswer : Answer { std::shared_ptr<const FfEntry> r; };
// One request of the session's last infx_engine_list_documents: its status and message, the size of its set, its page
struct ListAnswer : Answer { std::vector<int64_t> keys; std::vector<int32_t> docs; std::vector<uint32_t> codes; };
// One request of the session's last infx_engine_range_facets: its status and message, its counters, the extremes as values (kind 0: none, 1 int64, 2 double)
struct RangeAnswer : Answer { uint32_t below = 0, above = 0, nan = 0; std::vector<uint32_t> counts;
                     int32_t kind = 0; int64_t loI = 0, hiI = 0; double loD = 0, hiD = 0; };
// One request of the session's last infx_engine_field_stats (F: infx_stats_figures) or infx_engine_field_quantiles (infx_quantile_figures): its status and
// message, the whole's figures, the group column (-1: none) and the groups that have a member, in the contract's order
template <class F> struct FiguresAnswer : Answer { F whole = {}; int32_t groupCol = -1; std::vector<uint32_t> codes; std::vector<F> groups; };
typedef FiguresAnswer<infx_stats_figures> StatsAnswer;
typedef FiguresAnswer<infx_quantile_figures> QuantAnswer;
typedef FiguresAnswer<infx_distinct_figures> DistinctAnswer;      // (whole: the set's size and the field's values in it)
// One request of the session's last infx_engine_list_groups: its status and message, the size of its set (total), the groups with a member, its page: per
// row what a ListAnswer holds, the group's code and its size
struct GroupListAnswer : ListAnswer { uint32_t totalGroups = 0; std::vector<uint32_t> gcodes, sizes; };
// One request of the session's last infx_engine_list_group_members: its status and message, both totals, per row of its page the group's code, its size and
// the number of members it carries; keys / docs / codes: the members of all rows, row after row (what a ListAnswer holds of a row, per member)
struct GroupMembersAnswer : ListAnswer { uint32_t totalGroups = 0; std::vector<uint32_t> gcodes, sizes, held; };
// One request of the session's last infx_engine_top_groups: its status and message, the size of its set (total), the groups with a member, the group column,
// whether it had a field, its page: per row the group's code, its members and — with a field — its figures
struct TopAnswer : Answer { uint32_t totalGroups = 0; int32_t groupCol = -1; bool hasField = false; std::vector<uint32_t> codes, sizes; std::vector<infx_stats_figures> figures; };
// One request of the session's last infx_engine_bucket_stats: its status and message, the size of its set, per slot [below | B buckets | above | nan] the
// members and the figures of the field over them, the figures over the whole set
struct BucketAnswer : Answer { std::vector<uint32_t> sizes; std::vector<infx_stats_figures> rows; infx_stats_figures whole = {}; };
struct MaskUse { uint32_t built = 0, reused = 0; };      // masks a call built / found in the session's cache
template <class A> struct LastCall { typedef A answer; std::vector<A> ans; MaskUse masks; };
struct infx_session {
    QueryOpts qo; QueryCov qc; QueryPre qp; QueryClp qk; QueryHl qh;
    QueryPart* const parts[QP_PARTS] = {&qo, &qc, &qp, &qk, &qh};      // (indexed by QP_*)
    std::vector<int32_t> lastClpCol;      // per query of the last batch the column it was collapsed by (-1: it was not)
    std::vector<int32_t> lastHlChars; std::vector<HlQuery> lastHlQuery;      // per query of the last batch the width it was highlighted with (0: it was not) and its words
    PreMask preMask[INFX_MAX_PREFILTERS]; uint64_t preTick = 0; uint32_t preCountBuf[INFX_MAX_PREFILTERS] = {};      // preCountBuf: where a build's counts land
    std::vector<uint32_t> lastInPre; uint32_t preBuilt = 0, preReused = 0, preLaunches = 0;      // of the last batch (or infx_engine_prefilter_mask)
    std::vector<uint32_t> facetCols;      // engine column indices whose facets the session's stream counts
    std::vector<std::string> swPinFilter, swPinBoosts;      // cache entries the session-wide filter / boosts hold
    bool swFilter = false, swBoost = false, swSort = false;      // session-wide options installed (infx_engine_set_filter / _set_boosts / _set_sort)
    std::vector<uint32_t> facAllListCols, ffListCols; std::vector<std::vector<std::pair<uint32_t, uint32_t>>> facAllList;      // the facetable list columns of the last infx_engine_facets_all / _facets_filtered, and the former's lists
    std::vector<uint32_t> facAllCols; std::vector<std::vector<std::pair<uint32_t, uint32_t>>> facAll;      // infx_engine_facets_all: columns and their ordered (code, count) lists
    // infx_engine_facets_filtered: the facet columns of the session's last call, one answer per expression of it (its entry of the engine's cache, or why it
    // was refused), and what the call cost: expressions counted on the device, expressions taken from the cache, k_facets_filtered launches
    std::vector<uint32_t> ffCols; std::vector<FfAnswer> ff; uint32_t ffCounted = 0, ffCached = 0, ffLaunches = 0;
    // What the session keeps of its last call of each per-request kind (set_call): one answer per request, the masks built / reused, what else the call cost
    // infx_engine_list_documents: histogram passes, kernel launches; lstDigitBits: the digit width
    struct Lst : LastCall<ListAnswer> { uint32_t passes = 0, launches = 0; } lst; int32_t lstDigitBits = 11;
    struct Rng : LastCall<RangeAnswer> { uint32_t launches = 0; } rng;      // infx_engine_range_facets: k_range_counts launches
    struct Sts : LastCall<StatsAnswer> { uint32_t launches = 0; } sts;      // infx_engine_field_stats: k_field_stats launches
    // infx_engine_field_quantiles: histogram passes, kernel launches; place: the call's digit width, (request, pass) pairs with bins in LDS / in global memory;
    // qntDigitBits: the digit width asked for (0: chosen per call)
    struct Qnt : LastCall<QuantAnswer> { uint32_t passes = 0, launches = 0, place[3] = {0, 0, 0}; } qnt; int32_t qntDigitBits = 0;
    // infx_engine_list_groups: head passes, histogram passes, kernel launches (the digit width is lstDigitBits)
    struct Grp : LastCall<GroupListAnswer> { uint32_t heads = 0, passes = 0, launches = 0; } grp;
    // infx_engine_list_group_members: head passes, histogram passes, member walks, kernel launches (the digit width is lstDigitBits)
    struct Mem : LastCall<GroupMembersAnswer> { uint32_t heads = 0, passes = 0, walks = 0, launches = 0; } mem;
    // infx_engine_top_groups: accumulate passes, select passes, kernel launches, tables accumulated in a workgroup's LDS / a CU's whole LDS / global memory
    // (the digit width is lstDigitBits)
    struct Top : LastCall<TopAnswer> { uint32_t accumulates = 0, passes = 0, launches = 0, place[3] = {0, 0, 0}; } top;
    // infx_engine_field_distinct: kernel launches, passes that marked in LDS / in a global bitmap / in a hash set; dstPlacement: the placement asked of the device
    struct Dst : LastCall<DistinctAnswer> { uint32_t launches = 0, place[3] = {0, 0, 0}; } dst; int32_t dstPlacement = 0;
    // infx_engine_bucket_stats: k_bucket_stats launches, requests whose slots lay in a workgroup's LDS / a CU's whole LDS / global memory
    struct Bks : LastCall<BucketAnswer> { uint32_t launches = 0, place[3] = {0, 0, 0}; } bks;
    std::vector<uint32_t> lastInFilter; std::vector<std::string> lastErr; uint32_t lastCounted = 0, lastCountLaunches = 0;     // of the last per-query batch
    infx_engine* e = nullptr;
    Batch* batch = nullptr;
    infx_stream* stream = nullptr;
    double tPrep1 = 0, tStage1 = 0, tPrep2 = 0, tStage2 = 0, tPost = 0;
    bool kernelTimesPending = false; float msReplayParts[4] = {0, 0, 0, 0};
    uint64_t collCalls[2] = {0, 0}, collBytes[2] = {0, 0};      // all-reduce / all-gather calls and payload bytes this session issued (sharded driver), cumulative
    float msAcc = 0, msSel = 0, msCov = 0, msPrep2 = 0, msFin = 0, msReplay = 0; uint32_t flagWhy[3] = {0, 0, 0}; uint64_t algBytes = 0; uint64_t s2Candidates = 0, s2TextBytes = 0, streamedBytes = 0, s1Candidates = 0; uint32_t exactReplays = 0;
    // last-batch introspection for parity tests
    std::vector<QueryPlan> lastPlans;
    std::vector<infx_hit> lastHits; std::vector<uint32_t> lastHitCount; int lastStride = 0;
    std::vector<infx_cov_cand> lastCands; std::vector<infx_cov_out> lastOuts; std::vector<int32_t> lastFeat;
    // sharded planning (infx_session_prefetch_*): WordMatcher descriptors of the coming batch computed by peer ranks, keyed by the search text;
    // this rank's own share, serialised for the exchange
    struct WmPre { std::vector<infx_wm_list> lists; std::vector<int32_t> owned; };
    std::unordered_map<std::u16string, WmPre> wmPre;
    std::vector<uint8_t> prefetchBlob;
    // plan exchange: per query of the COMING batch, the token-level plan (plan_tokens_text) and the coverage query context (prepare_cov_query) computed by
    // the rank whose slice holds the query — this rank's own slice included; consumed by the next phase 0 (ph_plan, build_fused_inputs)
    // Own slice: parsed (plan, cq filled in by the collect).  A peer's: `rec` points at the query's record inside the retained blob (PlanSlab) and is parsed where
    // the plan is needed — on the planner threads of phase 0, straight into the batch's plan / coverage-query arrays — so the import itself costs a checksum.
    struct OwnPlan { QueryPlan plan; infx_cov_query cq; std::unique_ptr<infx_cov_query_long> cql; };
    struct PlanPre { uint64_t rawHash = 0; int32_t depth = 0, covErr = 0; bool hasCov = false, longCov = false, planTaken = false;      /* planTaken: own->plan was moved into a batch */ const uint8_t* rec = nullptr; uint32_t recLen = 0, covOff = 0; std::unique_ptr<OwnPlan> own; };
    struct PlanSlab { std::vector<uint8_t> bytes; std::vector<PlanPre> pre; };
    std::vector<std::shared_ptr<PlanPre>> planPre;
    uint32_t planFromExchange = 0, planFromPeers = 0;      // last phase 0: queries planned from planPre / of them imported from another rank
    std::vector<uint8_t> planPeer;                          // planPre[i] came from a peer
};

// One Infiscript expression of the engine's filter cache: its host program (a per-query batch packs it), its device copy (compiled on first use by a
// session-wide setter), Filter.NumberOfDocumentsInFilter of this shard (infx_engine_set_filter) and of the whole corpus (per-query options; the same
// number when the engine is not sharded)
struct CompiledFilter {
    std::vector<infx_filter_op> ops; std::vector<infx_filter_leaf> leaves; std::vector<uint32_t> tables;
    infx_filter* dev = nullptr;
    uint32_t inFilter = 0, inAll = 0; bool counted = false, countedAll = false;
    uint32_t pins = 0;                      // installs that hold the entry: it is not evicted while > 0
    std::vector<std::pair<int, std::string>> derived;      // the derived leaf columns its program reads (list column, list_leaf_key): each holds one reference
    std::list<std::string>::iterator lru;
};
// the program of anything that holds ops, leaves and tables (a CompiledFilter, a copy taken out of the filter cache), as the device library takes it
template <class F> static infx_filter_prog prog_of(const F& cf) {
    infx_filter_prog P{};
    P.ops = cf.ops.data(); P.leaves = cf.leaves.data(); P.tables = cf.tables.data();
    P.nops = (uint32_t)cf.ops.size(); P.nleaves = (uint32_t)cf.leaves.size(); P.ntable_words = (uint32_t)cf.tables.size();
    return P;
}
// per-query options of the session's batch (infx_engine_set_query_options): query i's MaxNumberOfRecordsToReturn (never above the call's row stride)
// and EnableCoverage; the call's values for a session without options
static inline int32_t qo_max(const infx_session* S, size_t i, int32_t mr) {
    return S->qo.on && i < S->qo.nq && S->qo.maxResults[i] >= 1 ? std::min(S->qo.maxResults[i], mr) : mr;
}
// A blank text with EnableFacets is a browse query (SearchEngine.cs:292-293, HandleEmptyQueryWithFacets): per query with its options, or for every
// query of the batch while the session-wide facets are installed.  (The facets need a facetable column; without one a blank query stays empty.)
static inline bool qo_browse(const infx_session* S, size_t i) {
    if (S->qo.on) return i < S->qo.nq && S->qo.facets[i] && !S->qo.reject[i];
    return S->swFilter && !S->facetCols.empty();
}
static inline bool qo_cov(const infx_session* S, size_t i, bool cov) { return cov && (!S->qo.on || i >= S->qo.nq || S->qo.cov[i]); }
static bool host_phases() { static const bool on = getenv("INFX_PHASED") != nullptr; return on; }      // the host-driven phases (the sharded code path) on one GPU
static int32_t query_parts_check(infx_session* S, uint32_t nq, int32_t max_results);
static int32_t query_parts_finish(infx_session* S, uint32_t* out_counts, uint32_t* out_flags, bool ok);
static void query_parts_unbind(infx_session* S);
static void query_parts_bind(infx_session* S);
static int32_t stage_collapse(infx_session* S, uint32_t nq, std::vector<infx_fused_query>& fq);
static int32_t stage_highlight(infx_session* S, uint32_t nq, std::vector<infx_fused_query>& fq, const FusedIn& FI);
// The filter and mask part of one call over the documents that filters accept: a batch with pre-filters, infx_engine_prefilter_mask, _list_documents,
// _range_facets, _field_stats.  Request i's filter is interned (one cache lookup and one mask per distinct expression), acquire() finds or stages the masks of the call in
// the session's mask cache, mask(i) is request i's; the device call that follows ends in failed(rc) or done().  (Defined with the mask cache, below.)
struct MaskCall {
    infx_session* S; MaskUse* use;                // use: where the call's kind keeps its masks built / reused, beside the session's pre* counters
    std::vector<std::string> exprs; std::unordered_map<std::string, int> idx; std::vector<int> of;      // the distinct filters; request i's among them (-1: none)
    std::vector<uint8_t*> masks; std::vector<int> built;      // exprs[k]'s device flags; the slots the call builds
    MaskCall(infx_session* S, uint32_t nreq, MaskUse* use = nullptr) : S(S), use(use), of(nreq, -1) {}
    void add(uint32_t i, const std::string& expr);      // request i has filter expr, which is known to compile
    int32_t intern(uint32_t i, const char* expr);        // request i has filter expr: compiled on first sight, a failure (message in g_eerr) is the request's.  Caller holds filterMu
    int32_t acquire();                                   // once per call, nothing holding filterMu; without a filter only zeroes the pre* counters
    uint8_t* mask(uint32_t i) const { return of[i] >= 0 ? masks[of[i]] : nullptr; }
    int32_t failed(int32_t rc);                          // the device call failed: its message is kept, nothing stays staged
    void done(uint32_t nq = 0);                          // it succeeded: the built masks' counts, the statistics (nq: the batch whose queries' counts to take)
    // The filters whose masks the call builds stay pinned in the filter cache until the device has run the build (done / failed): a cached filter holds the
    // derived columns of its list-column leaves, so no other compile can hand their slots to another leaf in between.
    std::vector<std::string> pinned; bool locked = false;      // locked: acquire() holds filterMu
    void release();
    ~MaskCall() { release(); }
    MaskCall(const MaskCall&) = delete; MaskCall& operator=(const MaskCall&) = delete;
};
static int32_t stage_prefilters(infx_session* S, uint32_t nq, std::vector<infx_fused_query>& fq, MaskCall& pre);
static int32_t stage_coverage_setup(infx_session* S, uint32_t nq, bool deviceFinalize);
static inline int32_t qc_tolerance(const infx_session* S, size_t i, int len);
static inline infx_finalize_setup qc_finalize(const infx_session* S, size_t i);
// Order of the collectives of a rank's pipeline sessions.  Every session has a communicator and a HIP stream of its own, and its host thread enqueues the
// collectives of its batch when it gets there — left alone, the relative order of DIFFERENT communicators' kernels on a device depends on thread timing and
// differs from rank to rank, the classic multi-communicator hang (two collective kernels each holding the CUs the other's peer needs).  The ring makes the
// order a function of the batch schedule alone: the sessions of a stream take turns, one collective per turn, in ring order; a session whose last batch is
// done leaves the ring (infx_session_coll_retire).  Batch i runs on session i mod K on every rank and a batch issues the same collectives everywhere, so every
// rank enqueues every communicator's kernels in the same global order.
struct CollSeq {
    std::mutex m; std::condition_variable cv;
    std::vector<infx_session*> ring; std::vector<uint8_t> active; size_t cur = 0;
    int index_of(const infx_session* S) const { for (size_t i = 0; i < ring.size(); i++) if (ring[i] == S) return (int)i; return -1; }
    void advance_from(size_t i) {                       // next active member after i (stays on i when it is the only one)
        for (size_t k = 1; k <= ring.size(); k++) { const size_t j = (i + k) % ring.size(); if (active[j]) { cur = j; return; } }
        cur = i;
    }
    void set_ring(infx_session* const* ss, uint32_t n) { std::lock_guard<std::mutex> lk(m); ring.assign(ss, ss + n); active.assign(n, 1); cur = 0; cv.notify_all(); }
    bool enter(const infx_session* S) {                 // blocks until it is S's turn; false: S is not (or no longer) in the ring -> unordered
        std::unique_lock<std::mutex> lk(m);
        const int i = index_of(S);
        if (i < 0 || !active[i]) return false;
        cv.wait(lk, [&] { return cur == (size_t)i || !active[i]; });
        return active[i] != 0;
    }
    void leave(const infx_session* S) { std::lock_guard<std::mutex> lk(m); const int i = index_of(S); if (i >= 0 && cur == (size_t)i) { advance_from((size_t)i); cv.notify_all(); } }
    void retire(const infx_session* S) {
        std::lock_guard<std::mutex> lk(m); const int i = index_of(S); if (i < 0 || !active[i]) return;
        active[i] = 0; if (cur == (size_t)i) advance_from((size_t)i); cv.notify_all();
    }
};
// Host planning of concurrent sessions goes through a FIFO gate of `limit` planners at a time.  Each planner fans out over the whole worker pool; with
// six sessions planning at once (the start of a stream, or any moment their phases line up) every one of them takes six times as long and the GPU
// waits for all of them — gated, the first batches reach the device after one planning time and the pipeline fills in order.
struct PlanGate {
    std::mutex m; std::condition_variable cv; int inUse = 0, limit = 0; uint64_t next = 0, serving = 0;
    void enter() { if (limit <= 0) return; std::unique_lock<std::mutex> lk(m); const uint64_t t = next++; cv.wait(lk, [&] { return t == serving && inUse < limit; }); serving++; inUse++; cv.notify_all(); }
    void leave() { if (limit <= 0) return; { std::lock_guard<std::mutex> lk(m); inUse--; } cv.notify_all(); }
};
static thread_local PlanGate* tl_gate = nullptr;      // the gate this thread holds, if any
struct PlanGateHold { PlanGate& g; explicit PlanGateHold(PlanGate& x) : g(x) { g.enter(); tl_gate = &g; } ~PlanGateHold() { tl_gate = nullptr; g.leave(); } };
// A planner that waits for the device (LD1 expansion, union cardinalities) gives its place at the gate to the next planner and queues again afterwards: the
// gate rations CPU time, and a thread blocked on a HIP event uses none (held across the wait it capped the pipeline at `limit` / wait batches per second).
struct PlanGatePause { PlanGate* g; PlanGatePause() : g(tl_gate) { if (g) g->leave(); } ~PlanGatePause() { if (g) g->enter(); } };
struct infx_engine {
    // non-indexed document fields (DocumentFields) as dictionary-encoded columns + compiled Infiscript filters (config 5)
    std::vector<filt::Column> columns; std::mutex filterMu; std::unordered_map<std::string, CompiledFilter> filters;
    std::vector<infx_filter*> retiredFilters;     // compiled against an older column set (a session's stream may still point at one): freed with the engine
    std::vector<uint8_t> tieRanked;               // per column: its facet tie order (Column.rank) is on the device (infx_engine_top_groups, uploaded on first use)
    std::vector<uint8_t> sortRanked;              // per column: its sort rank is on the device (infx_engine_set_sort, built on first use)
    // per column, for infx_engine_range_facets (built on first use, under filterMu): the lowest code of every sort rank, in rank order, and whether rank 0 is a NaN
    struct RangeIndex { bool ok = false; uint32_t nanRanks = 0; std::vector<uint32_t> codeOfRank; };
    std::vector<RangeIndex> rangeIndex;
    // per column, for infx_engine_field_stats (built on first use, under filterMu; dropped with the column): the raw values of its codes, the scale and width
    // they are summed at (exact_sum.h), whether they can be summed exactly, and whether the table is on the device
    struct StatsIndex { bool ok = false, summable = false, uploaded = false; int32_t kind = 0; XsScale sc = {0, 1, 1}; std::vector<uint64_t> bits; };
    std::vector<StatsIndex> statsIndex;
    // NumberOfDocumentsInFilter is cached per expression; a Filter parsed after a mutation counts again (the reference keeps the count on the Filter instance)
    void invalidate_filter_counts() { std::lock_guard<std::mutex> lk(filterMu); for (auto& kv : filters) kv.second.counted = kv.second.countedAll = false; }
    void retire_filters() { std::lock_guard<std::mutex> lk(filterMu); for (auto& kv : filters) if (kv.second.dev) retiredFilters.push_back(kv.second.dev); filters.clear(); filterLru.clear(); derived.clear(); }
    // List columns (infx_engine_add_list_column): their own INFX_ENGINE_MAX_LIST_COLS slots, outside `columns`; a slot whose name is empty is free.
    // Derived leaf columns: a filter leaf over a list column is lowered to a one-bit scalar column on the device (k_list_leaf) that takes a free slot among
    // the 64 scalar slots, from the top down, above `columns`.  They are cached by (list column, operator, constants), reference-counted by the compiled
    // filters of the cache, at most INFX_ENGINE_MAX_DERIVED, least recently used first out among those no cached filter uses; whatever retires the compiled
    // filters (a new or replaced column of either kind) drops them all.  Guarded by filterMu.
    std::vector<filt::ListColumn> listCols;
    struct DerivedCol { int lcol; std::string key; uint32_t slot; uint32_t refs; uint64_t lastUse; };
    std::vector<DerivedCol> derived; uint64_t derivedTick = 0;
    uint32_t llBuilt = 0, llLaunches = 0; uint64_t llBuiltAll = 0, llLaunchesAll = 0;      // infx_engine_last_list_leaf_stats: the last expression compiled; all compiles of the engine
    void release_derived(const CompiledFilter& cf) {
        for (auto& k : cf.derived) for (auto& D : derived) if (D.lcol == k.first && D.key == k.second && D.refs) { D.refs--; break; }
    }
    // The cache is bounded (per-user expressions would grow it without limit): least recently used first, never an entry an install holds.  An evicted
    // expression is parsed and counted again on its next use.  Its device copy is parked with the retired ones (hipFree would wait for the whole device).
    std::list<std::string> filterLru; size_t filterCacheLimit = 4096;
    void evict_filters() {
        for (auto it = filterLru.end(); filters.size() > filterCacheLimit && it != filterLru.begin();) {
            --it;
            auto f = filters.find(*it);
            if (f == filters.end() || f->second.pins) continue;
            if (f->second.dev) retiredFilters.push_back(f->second.dev);
            release_derived(f->second);
            filters.erase(f); it = filterLru.erase(it);
        }
    }
    infx_coverage_setup cs = {2, 20, 2, 3, 7, 1, 0, 5, 0.2, 1, 1, 1, 1, 1, 1, 0, 254};      // the engine-wide CoverageSetup (infx_engine_set_coverage_setup)
    // Pre-filter masks (one byte per document, cached per session) are valid for one epoch: whatever changes a document's Deleted flag or what a compiled
    // filter accepts — a deletion, a restore, a new column, a (re-)index — starts the next one
    std::atomic<uint64_t> maskEpoch{1};
    // Facets of the documents a filter accepts, per expression (infx_engine_facets_filtered): shared by the sessions, least recently used first out, an entry
    // of an earlier mask epoch is counted again on its next use
    std::mutex ffMu; std::unordered_map<std::string, std::shared_ptr<FfEntry>> ffCache; std::list<std::string> ffLru; size_t ffCacheLimit = 256;
    HostIndex ix;
    PlanGate gate;
    CollSeq collSeq;
    infx_engine_config cfg{};
    infx_index* dev = nullptr;
    bool indexed = false;
    int32_t postRows = INFX_FILTER_MAX_ROWS;      // rows per query that filter / facets / boosts / sort-by / browse accept (infx_engine_set_post_rows, before the first search)
    std::atomic<bool> searched{false};            // a search has begun on this engine
    FuzzyCache fuzzy;
    std::unordered_map<int64_t, int32_t> keyToFirst;
    bool keysAreIds = false;
    std::vector<uint8_t> deleted;     // Document.Deleted per global internal id; empty = nothing deleted
    std::atomic<long long> ld1OnHost{0}, ld1OnDevice{0}, wmOnHost{0}, wmOnDevice{0};      // where the planning lookups ran (introspection)
    bool devLookups = false;          // WordMatcher dictionaries + term trie uploaded: the LD1 / WordMatcher lookups of planning can run on the GPU (f3)
    // Both sides can answer a batch's lookups with identical results (tests/test_gpu_lookups.py).
    // WordMatcher: always the device once the dictionaries are uploaded — k_wm rides inside the batch's pipeline (0.12 ms, no extra wait), while the host's cost
    // depends on the sizes of the affix ranges (config 3: 37 ms of 16 threads per batch; a word-count model sent it to the host and halved the rate).
    // LD1 expansion: by cost.  The host walk is predictable (~21 us of one core per unknown word, spread over the planner threads); k_ld1 is one latency-bound wave
    // per word whose result the host WAITS for, and behind five other batches' streaming kernels that wait is ~15 ms (0.2 ms on an idle GPU): with cores to spare
    // the host is faster for a few hundred words (config 4, ~220 unknown words per batch, 10 M documents, 16 CPUs: 74.8 k against 68.7 k queries/s); the device takes
    // the batch when the estimated host time exceeds a tenth of the planner threads' time in a 10-ms batch interval — two threads per rank on an 8-GPU node, or about
    // a thousand unknown words: config 3 (every query misspelt, ~960 words per batch) runs 68.0 k against 65.7 k queries/s with the expansion on the device (fused into
    // the union build: one wait) at four sessions, 43.5 k against 39.7 k at one (round 5, profiles/r05_bench_cfg3_device_ld1_*.json; the threshold was 2.5 x before and
    // sent config 3 to the host).  INFX_DEVICE_LOOKUPS=1 pins the device (the GPU test suite does), INFX_HOST_LOOKUPS=1 keeps everything on the host (no upload).
    bool ld1Pinned = false;
    bool ld1_on_device(double estThreadMs) const { return devLookups && (ld1Pinned || estThreadMs > 1.0 * (double)std::max(1, threads)); }
    bool lookups_on_device(double) const { return devLookups; }
    int threads = 1;
    int buildThreads = 0;             // > 0: threads of the index build only (infx_engine_set_build_threads)
    infx_session* def = nullptr;      // default session (single-caller API)
    // document sharding: this engine's GPU holds internal ids [shardBase, shardBase + shardN) of the corpus
    int rank = 0, nranks = 1; int32_t shardBase = 0, shardN = 0;
    std::vector<uint64_t> shardOff;   // sharded: per-term slice lengths prefix (T+1) of the uploaded CSR
    uint64_t shardTermLen(int32_t t) const { return nranks > 1 ? shardOff[t + 1] - shardOff[t] : ix.terms.len((uint32_t)t); }
};

// byte-blob writer / reader of the sharded-planning exchange (infx_session_prefetch_*)
namespace {
// what a peer's descriptors index into: sizes of the host index (FNV-1a over the counts; every rank builds the same index from the same corpus)
uint64_t index_fingerprint(const HostIndex& ix) {
    const uint64_t v[6] = {(uint64_t)ix.N, (uint64_t)ix.terms.K(), (uint64_t)ix.terms.doc.size(), (uint64_t)ix.wmExact.doc.size(), (uint64_t)ix.wmLd1.doc.size(), (uint64_t)ix.text.size()};
    uint64_t h = 1469598103934665603ull;
    for (uint64_t x : v) for (int b = 0; b < 8; b++) { h ^= (x >> (8 * b)) & 0xFFu; h *= 1099511628211ull; }
    return h;
}
struct BlobW { std::vector<uint8_t>& b; template <class T> void put(const T& v) { const uint8_t* p = (const uint8_t*)&v; b.insert(b.end(), p, p + sizeof(T)); }
               void bytes(const void* p, size_t n) { const uint8_t* q = (const uint8_t*)p; b.insert(b.end(), q, q + n); } };
uint64_t raw_hash(const uint16_t* p, size_t n) {      // FNV-1a over the raw query text: ties an exchanged plan to the query it was made for
    uint64_t h = 1469598103934665603ull ^ (uint64_t)n;
    for (size_t i = 0; i < n; i++) { h ^= p[i]; h *= 1099511628211ull; }
    return h;
}
uint64_t bytes_hash(const uint8_t* p, size_t n) {      // checksum of a blob section: eight bytes per step
    uint64_t h = 0x9E3779B97F4A7C15ull ^ (uint64_t)n; size_t i = 0;
    for (; i + 8 <= n; i += 8) { uint64_t w; std::memcpy(&w, p + i, 8); h = (h ^ w) * 0xFF51AFD7ED558CCDull; h ^= h >> 32; }
    for (; i < n; i++) { h = (h ^ p[i]) * 1099511628211ull; }
    return h ^ (h >> 29);
}
struct BlobR { const uint8_t* p; const uint8_t* e; bool ok = true;
               template <class T> T get() { T v{}; if ((size_t)(e - p) < sizeof(T)) { ok = false; return v; } std::memcpy(&v, p, sizeof(T)); p += sizeof(T); return v; }
               const uint8_t* take(size_t n) { if ((size_t)(e - p) < n) { ok = false; return nullptr; } const uint8_t* r = p; p += n; return r; } };
// CoverageEngine.PrepareQuery into the fast record, or — beyond its envelope — into a long record (then `lq` is set and q is left zeroed: its `reserved` member
// gets 1 + the record's index in the batch's long-query table when that is assembled).  INFX_EUNSUPPORTED: beyond the long envelope too.
int32_t prepare_cov_any(const HostIndex& ix, uview st, infx_cov_query& q, std::unique_ptr<infx_cov_query_long>& lq) {
    lq.reset();
    int32_t rc = prepare_cov_query(ix, st, q);
    if (rc != INFX_EUNSUPPORTED) return rc;
    lq.reset(new infx_cov_query_long);
    rc = prepare_cov_query_long(ix, st, *lq);
    if (rc) lq.reset(); else std::memset(&q, 0, sizeof q);
    return rc;
}
// One query's record of the plan exchange (layout: infx_session_prefetch_collect).  parse_plan_record fills the token-level plan and reports where the
// coverage query sits; parse_cov_record rebuilds the infx_cov_query exactly as prepare_cov_query wrote it (its text is the plan's searchText).
// Everything that reaches the device is range-checked.  nullptr = fine, else what is wrong.
const char* parse_plan_record(const HostIndex& ix, const uint8_t* rec, uint32_t len, int depth, QueryPlan& P, bool& hasCov, int32_t& covErr, uint32_t& covOff, bool& longCov) {
    BlobR R{rec, rec + len};
    auto str = [&](ustr& t) { const uint32_t l = R.get<uint32_t>(); const uint8_t* p = R.take((size_t)l * 2); if (!R.ok) return; t.resize(l); if (l) std::memcpy(&t[0], p, (size_t)l * 2); };
    P = QueryPlan(); P.depth = depth;
    R.get<uint64_t>(); const uint8_t fl = R.get<uint8_t>();
    P.blank = (fl & 1) != 0; P.unsupported = (fl & 2) != 0; hasCov = (fl & 16) != 0; covErr = 0; longCov = (fl & 64) != 0;
    str(P.qtext); if (fl & 4) P.searchText = P.qtext; else str(P.searchText); if (fl & 8) P.tfidfQuery = P.searchText; else str(P.tfidfQuery);
    const uint16_t nraw = R.get<uint16_t>();
    if (!R.ok) return "record truncated";
    if (nraw > 128) return "more than 128 raw tokens";
    const int64_t nTerms = (int64_t)ix.terms.K();
    P.rawTok.resize(nraw);
    for (uint16_t k = 0; k < nraw && R.ok; k++) {
        auto& r = P.rawTok[k]; r.id = R.get<int32_t>();
        if (r.id < 0) { r.id = -1; str(r.text); } else if ((int64_t)r.id >= nTerms) return "term id out of range (ranks must hold the same index)";
    }
    if (!R.ok) return "record truncated";
    covOff = (uint32_t)(R.p - rec);
    if (hasCov && (fl & 32)) { covErr = R.get<int32_t>(); if (!R.ok || covErr == 0) return "inconsistent coverage-query status"; }
    return nullptr;
}
template <class QT, int MAXCHARS, int MAXTOK>
const char* parse_cov_record_t(const ustr& searchText, const uint8_t* rec, uint32_t len, uint32_t covOff, QT& C) {
    if (covOff > len) return "record truncated";
    BlobR R{rec + covOff, rec + len};
    std::memset(&C, 0, sizeof C);
    const size_t tl = searchText.size();
    if (tl > (size_t)MAXCHARS) return "coverage query longer than the envelope";
    std::memcpy(C.text, searchText.data(), tl * 2); C.text_len = (int32_t)tl;
    C.num_tokens = R.get<int32_t>();
    if (!R.ok || C.num_tokens < 0 || C.num_tokens > MAXTOK) return "coverage query token count out of range";
    const size_t nt = (size_t)C.num_tokens; const uint8_t* p;
    if ((p = R.take(nt * 2))) std::memcpy(C.tok_off, p, nt * 2);
    if ((p = R.take(nt * 2))) std::memcpy(C.tok_len, p, nt * 2);
    if ((p = R.take(nt * 4))) std::memcpy(C.term_idf, p, nt * 4);
    if ((p = R.take(nt * 4))) std::memcpy(C.word_idf, p, nt * 4);
    C.has_word_idf = R.get<int32_t>(); C.num_fusion_tokens = R.get<int32_t>();
    if (!R.ok || C.num_fusion_tokens < 0 || C.num_fusion_tokens > 2 * MAXTOK) return "coverage query token count out of range";
    const size_t nf = (size_t)C.num_fusion_tokens;
    if ((p = R.take(nf * 2))) std::memcpy(C.ftok_off, p, nf * 2);
    if ((p = R.take(nf * 2))) std::memcpy(C.ftok_len, p, nf * 2);
    C.lcs_tolerance = R.get<int32_t>();
    if (!R.ok) return "record truncated";
    for (size_t k = 0; k < nt; k++) if ((size_t)C.tok_off[k] + C.tok_len[k] > tl) return "coverage token outside its text";      // the token tables go to the device
    for (size_t k = 0; k < nf; k++) if ((size_t)C.ftok_off[k] + C.ftok_len[k] > tl) return "coverage token outside its text";
    return nullptr;
}
const char* parse_cov_record(const ustr& st, const uint8_t* rec, uint32_t len, uint32_t covOff, infx_cov_query& C) { return parse_cov_record_t<infx_cov_query, INFX_MAX_QUERY_CHARS, INFX_MAX_QUERY_TOKENS>(st, rec, len, covOff, C); }
const char* parse_cov_record_long(const ustr& st, const uint8_t* rec, uint32_t len, uint32_t covOff, infx_cov_query_long& C) { return parse_cov_record_t<infx_cov_query_long, INFX_LONGQ_CHARS, INFX_LONGQ_TOKENS>(st, rec, len, covOff, C); }
}

extern "C" {

const char* infx_engine_last_error(void) { return g_eerr.empty() ? infx_last_error() : g_eerr.c_str(); }

int32_t infx_engine_create(const infx_engine_config* cfg, infx_engine** out) {
    if (!cfg || !out) return efail(INFX_EINVAL, "null argument");
    infx_engine* e = new infx_engine();
    e->cfg = *cfg;
    HostConfig& h = e->ix.cfg;
    h.enableCoverage = cfg->enable_coverage != 0; h.wordMatcher = cfg->word_matcher != 0;
    if (cfg->stop_term_limit > 0) h.stopTermLimit = cfg->stop_term_limit;
    h.maxDepth = cfg->max_depth > 0 ? cfg->max_depth : 500;
    h.threads = cfg->threads;
    e->threads = cfg->threads > 0 ? cfg->threads : effective_cpus();
    { const char* g = getenv("INFX_PLAN_GATE"); e->gate.limit = g ? atoi(g) : std::max(1, e->threads / 8); }      // 0 = no gate
    if (cfg->device >= 0) {
        infx_config dc{}; dc.device = cfg->device; dc.range_docs = cfg->range_docs; dc.max_depth = h.maxDepth; dc.flags = cfg->no_exact_replay ? INFX_CFG_NO_EXACT_REPLAY : 0;
        int32_t rc = infx_create(&dc, &e->dev);
        if (rc) { g_eerr = infx_last_error(); delete e; return rc; }
    }
    e->def = new infx_session(); e->def->e = e; e->def->batch = new Batch();
    *out = e; return INFX_OK;
}

void infx_engine_destroy(infx_engine* e) {
    if (!e) return;
    infx_session* S = e->def;
    if (S && S->stream) infx_stream_destroy(S->stream);
    if (S) delete S->batch;
    delete S;
    for (auto& kv : e->filters) if (kv.second.dev) infx_filter_destroy(kv.second.dev);
    for (auto* f : e->retiredFilters) infx_filter_destroy(f);
    if (e->dev) infx_destroy(e->dev);
    delete e;
}

static int32_t finish_index(infx_engine* e);
// SearchEngine.IndexDocuments: n documents x field_count fields (UTF-16 arena + offsets), keys may be null (key = index)
int32_t infx_engine_index_documents(infx_engine* e, int64_t n, const int64_t* keys, const uint16_t* arena, const uint64_t* offs,
                                    int32_t field_count, const int32_t* field_weights) {
    if (!e || n < 0 || (n && (!arena || !offs)) || field_count < 1 || !field_weights) return efail(INFX_EINVAL, "bad arguments");
    if (e->indexed) return efail(INFX_EINVAL, "this engine instance is already indexed (re-indexing: create a new engine)");
    if (n > 0x7FFFFFF0ll) return efail(INFX_EINVAL, "too many documents");
    for (int64_t i = 0, m = n * field_count; i < m; i++) if (offs[i + 1] < offs[i]) return efail(INFX_EINVAL, "field offsets must be ascending (offs[n * field_count] = the arena's length)");
    DocSource src{n, field_count, field_weights, keys, (const u16*)arena, offs};
    {
        const int planThreads = e->ix.cfg.threads;
        if (e->buildThreads > 0) e->ix.cfg.threads = e->buildThreads;      // a node's leader rank builds with every core while the other ranks wait for its cache
        build_index(src, e->ix);
        e->ix.cfg.threads = planThreads;
    }
    e->keysAreIds = (keys == nullptr);
    return finish_index(e);
}
// An engine populated from FLUSHED SEGMENTS + a live tail (VectorModel.Flush, VectorModel.cs:804-815): segment i holds the postings of documents
// [doc_bases[i], doc_bases[i] + its document count), the segments cover the documents from 0 without gaps, the documents behind them are the live tail.  The
// posting lists of the flushed ranges are taken from the files (read and validated by host/infs.h) — only the tail's postings are accumulated from the texts;
// term ids, document lengths, the WordMatcher dictionaries, prefix sets and the Stage-2 texts need the documents, so all n documents are supplied.  The engine
// then searches the whole corpus as ONE index.  (The reference answers a mixed index segment by segment, every segment with its own tier decisions and its own
// top-k heap, merged afterwards — VectorModel.cs:572-584: an index-lifecycle artefact this does not imitate; an unflushed index of the same documents is what
// it equals, and what tests/test_infs.py checks against the oracle.)
int32_t infx_engine_index_from_segments(infx_engine* e, int64_t n, const int64_t* keys, const uint16_t* arena, const uint64_t* offs, int32_t field_count, const int32_t* field_weights,
                                        int32_t n_segments, const char* const* paths, const int32_t* doc_bases) {
    if (!e || n < 0 || (n && (!arena || !offs)) || field_count < 1 || !field_weights || n_segments < 0 || (n_segments && (!paths || !doc_bases))) return efail(INFX_EINVAL, "bad arguments");
    if (e->indexed) return efail(INFX_EINVAL, "this engine instance is already indexed (re-indexing: create a new engine)");
    if (n > 0x7FFFFFF0ll) return efail(INFX_EINVAL, "too many documents");
    for (int64_t i = 0, m = n * field_count; i < m; i++) if (offs[i + 1] < offs[i]) return efail(INFX_EINVAL, "field offsets must be ascending (offs[n * field_count] = the arena's length)");
    std::vector<infs::Segment> files((size_t)n_segments); std::vector<SegmentPostings> segs((size_t)n_segments);
    for (int32_t i = 0; i < n_segments; i++) {
        if (!paths[i]) return efail(INFX_EINVAL, "null segment path");
        if (!infs::read_file(paths[i], files[i])) return efail(INFX_EINVAL, "INFS segment: " + files[i].error);
        segs[i].docBase = doc_bases[i]; segs[i].docCount = files[i].docCount; segs[i].terms = &files[i].terms; segs[i].off = &files[i].off; segs[i].doc = &files[i].doc; segs[i].w = &files[i].w;
    }
    DocSource src{n, field_count, field_weights, keys, (const u16*)arena, offs};
    const int planThreads = e->ix.cfg.threads;
    if (e->buildThreads > 0) e->ix.cfg.threads = e->buildThreads;
    const char* err = build_index(src, e->ix, &segs);
    e->ix.cfg.threads = planThreads;
    if (err) { const HostConfig cfg = e->ix.cfg; e->ix = HostIndex(); e->ix.cfg = cfg; return efail(INFX_EUNSUPPORTED, std::string("index from segments: ") + err); }      // the engine stays unindexed and reusable
    e->keysAreIds = (keys == nullptr);
    return finish_index(e);
}


// The dictionaries of the planning lookups go to the device next to the lists they resolve to (include/infidex_hip.h "Dictionary lookups"): WordMatcher
// exact / symmetric-delete keys, the word list with its affix orders, the reversed-term trie.  INFX_HOST_LOOKUPS=1 keeps the lookups on the host.
static void key_arena(const KeyTable& K, std::vector<uint32_t>& offs, std::vector<u16>& repack, const u16*& chars) {
    const size_t n = K.size();
    offs.resize(n + 1);
    bool contiguous = true; uint32_t run = n ? K.keyOff[0] : 0;
    for (size_t i = 0; i < n; i++) { if (K.keyOff[i] != run) { contiguous = false; break; } run += K.keyLen[i]; }
    if (contiguous && (n == 0 || K.keyOff[0] == 0)) { for (size_t i = 0; i < n; i++) offs[i] = K.keyOff[i]; offs[n] = run; chars = K.arena.data(); return; }
    repack.clear(); for (size_t i = 0; i < n; i++) { offs[i] = (uint32_t)repack.size(); repack.insert(repack.end(), K.arena.begin() + K.keyOff[i], K.arena.begin() + K.keyOff[i] + K.keyLen[i]); }
    offs[n] = (uint32_t)repack.size(); chars = repack.data();
}
static int32_t upload_lookups(infx_engine* e) {
    const HostIndex& ix = e->ix;
    { const char* h = getenv("INFX_HOST_LOOKUPS"); if (h && h[0] == '1') return INFX_OK; }
    if (ix.rEdgeStart.size() < 2) return INFX_OK;
    int32_t rc = infx_upload_term_trie(e->dev, (uint32_t)ix.rTerm.size(), ix.rEdgeStart.data(), (const uint16_t*)ix.rEdgeLabel.data(), ix.rEdgeChild.data(), ix.rTerm.data(),
                                       (uint32_t)ix.sortedTerms.size(), ix.sortedTerms.data());
    if (rc) return rc;
    if (ix.cfg.wordMatcher) {
        std::vector<uint32_t> eo, lo, wo; std::vector<u16> er, lr, wr; const u16 *ec = nullptr, *lc = nullptr, *wc = nullptr;
        key_arena(ix.wmExact.keys, eo, er, ec); key_arena(ix.wmLd1.keys, lo, lr, lc); key_arena(ix.words, wo, wr, wc);
        rc = infx_upload_wm_dictionary(e->dev, (uint32_t)ix.wmExact.K(), eo.data(), (const uint16_t*)ec, ix.wmExact.off.data(),
                                       (uint32_t)ix.wmLd1.K(), lo.data(), (const uint16_t*)lc, ix.wmLd1.off.data(),
                                       (uint32_t)ix.words.size(), wo.data(), (const uint16_t*)wc, ix.wordLastDoc.data(),
                                       (uint32_t)ix.affixFwd.size(), ix.affixFwd.data(), ix.affixRev.data(), ix.cfg.wmMinLD1, ix.cfg.wmMaxLD1);
        if (rc) return rc;
    }
    e->devLookups = true;
    { const char* d = getenv("INFX_DEVICE_LOOKUPS"); e->ld1Pinned = d && d[0] == '1'; }
    return INFX_OK;
}

static int32_t refresh_first_live(infx_engine* e);
// After the host index exists (built here or read from a node-local cache): key map, shard bounds, upload of this rank's slice
static int32_t finish_index(infx_engine* e) {
    if (!e->keysAreIds) { const int64_t n = e->ix.N; e->keyToFirst.reserve((size_t)n * 2); for (int64_t d = 0; d < n; d++) e->keyToFirst.emplace(e->ix.docKey[d], (int32_t)d); }
    {
        // contiguous doc-range shards of whole 65 536-id Roaring containers: the reference scores its candidates in chunks that never span a
        // container (Bm25Scorer.cs:195-280), so with boundaries at container multiples its sequential walk is the shards' walks one after the other and
        // the exact Stage-1 replay stays shard-local (exactsh.hip.inc).  Rank r owns containers [nCont*r/W, nCont*(r+1)/W) — an empty shard if W > nCont.
        const int64_t N = e->ix.N, W = e->nranks, r = e->rank, C = 65536, nCont = (N + C - 1) / C;
        auto bound = [&](int64_t k) { return std::min<int64_t>(N, C * (nCont * k / W)); };
        e->shardBase = (int32_t)bound(r); e->shardN = (int32_t)(bound(r + 1) - bound(r));
    }
    if (e->dev) {
        HostIndex& ix = e->ix;
        int32_t rc;
        if (e->nranks == 1) {
            rc = infx_upload_docs(e->dev, (uint32_t)ix.N, ix.docLen.data(), ix.avgdl, ix.docKey.data(), nullptr, ix.textOff.data(), (const uint16_t*)ix.text.data());
            if (!rc) rc = infx_upload_postings(e->dev, (uint32_t)ix.terms.K(), ix.terms.off.data(), ix.terms.doc.data(), ix.terms.w.data(), ix.df.data());
            if (!rc) rc = infx_upload_prefix_docsets(e->dev, (uint32_t)(ix.psOff.size() - 1), ix.psOff.data(), ix.psDocs.data());
            if (!rc && ix.cfg.wordMatcher) rc = infx_upload_wordmatcher(e->dev, ix.wmExact.doc.size(), ix.wmExact.doc.data(), ix.wmLd1.doc.size(), ix.wmLd1.doc.data());
        } else {
            // global statistics (df, avgdl, N, prefix populations, word IDF) stay on the host; the GPU gets this shard's slices, rebased
            const int32_t sb = e->shardBase, sn = e->shardN, se = sb + sn;
            std::vector<uint64_t> to((size_t)sn + 1);
            for (int32_t d = 0; d <= sn; d++) to[d] = ix.textOff[sb + d] - ix.textOff[sb];
            rc = infx_upload_docs(e->dev, (uint32_t)sn, ix.docLen.data() + sb, ix.avgdl, ix.docKey.data() + sb, nullptr, to.data(), (const uint16_t*)ix.text.data() + ix.textOff[sb]);
            size_t T = ix.terms.K();
            std::vector<uint64_t> lo(T), hi(T); e->shardOff.assign(T + 1, 0);
            parallel_for((int64_t)T, e->threads, [&](int64_t b, int64_t en, int) {
                for (int64_t t = b; t < en; t++) {
                    const int32_t* p = ix.terms.doc.data(); uint64_t a = ix.terms.off[t], z = ix.terms.off[t + 1];
                    lo[t] = std::lower_bound(p + a, p + z, sb) - p; hi[t] = std::lower_bound(p + lo[t], p + z, se) - p;
                }
            });
            for (size_t t = 0; t < T; t++) e->shardOff[t + 1] = e->shardOff[t] + (hi[t] - lo[t]);
            std::vector<int32_t> sd(e->shardOff[T]); std::vector<uint8_t> sw(e->shardOff[T]);
            parallel_for((int64_t)T, e->threads, [&](int64_t b, int64_t en, int) {
                for (int64_t t = b; t < en; t++) { uint64_t o = e->shardOff[t]; for (uint64_t i = lo[t]; i < hi[t]; i++, o++) { sd[o] = ix.terms.doc[i] - sb; sw[o] = ix.terms.w[i]; } }
            });
            if (!rc) rc = infx_upload_postings(e->dev, (uint32_t)T, e->shardOff.data(), sd.data(), sw.data(), ix.df.data());
            size_t ns = ix.psOff.size() - 1;
            std::vector<uint64_t> po(ns + 1, 0); std::vector<int32_t> pd;
            for (size_t k = 0; k < ns; k++) {
                auto a = std::lower_bound(ix.psDocs.begin() + ix.psOff[k], ix.psDocs.begin() + ix.psOff[k + 1], sb);
                auto z = std::lower_bound(a, ix.psDocs.begin() + ix.psOff[k + 1], se);
                for (auto it = a; it != z; ++it) pd.push_back(*it - sb);
                po[k + 1] = pd.size();
            }
            if (!rc) rc = infx_upload_prefix_docsets(e->dev, (uint32_t)ns, po.data(), pd.data());
            if (!rc) rc = infx_set_shard(e->dev, e->rank, e->nranks, sb, ix.N);
            if (!rc && ix.cfg.wordMatcher) rc = infx_upload_wordmatcher(e->dev, ix.wmExact.doc.size(), ix.wmExact.doc.data(), ix.wmLd1.doc.size(), ix.wmLd1.doc.data());
            if (!rc) rc = infx_upload_doc_keys_all(e->dev, (uint32_t)ix.N, ix.docKey.data());
        }
        if (!rc) rc = upload_lookups(e);
        if (!rc) rc = infx_stream_create(e->dev, &e->def->stream);
        if (rc) { g_eerr = infx_last_error(); return rc; }
        rc = refresh_first_live(e); if (rc) return rc;
    }
    e->indexed = true;
    e->maskEpoch++;
    return INFX_OK;
}

// The device's map "first live document of each document's key" (browse rows look a row up by key: include/infidex_hip.h, infx_set_first_live).
// Only a corpus with duplicate keys has one; rebuilt whenever Deleted flags change.
static int32_t refresh_first_live(infx_engine* e) {
    if (!e->dev) return INFX_OK;
    const int64_t N = e->ix.N;
    if (e->keysAreIds || (int64_t)e->keyToFirst.size() == N) return INFX_OK;      // unique keys: no map (as deleted[] is absent while nothing is deleted)
    std::vector<int32_t> first((size_t)N); std::unordered_map<int64_t, int32_t> live; live.reserve(e->keyToFirst.size() * 2);
    for (int64_t d = 0; d < N; d++) {
        if (!e->deleted.empty() && e->deleted[(size_t)d]) { first[(size_t)d] = (int32_t)d; continue; }
        first[(size_t)d] = live.emplace(e->ix.docKey[(size_t)d], (int32_t)d).first->second;
    }
    int32_t rc = infx_set_first_live(e->dev, (uint32_t)N, first.data());
    if (rc) g_eerr = infx_last_error();
    return rc;
}
static int32_t key_to_id(infx_engine* e, int64_t key) {
    if (e->keysAreIds) return (key >= 0 && key < e->ix.N) ? (int32_t)key : -1;
    auto it = e->keyToFirst.find(key); return it == e->keyToFirst.end() ? -1 : it->second;
}

// SearchEngine.Search for a batch of queries (each = one reference Search call; results are independent of batching).
// out_* are nq x max_results; out_flags: bit0 unsupported (short-query path), bit1 coverage stage ran, bit2 fell back to Stage 1
// ------------------------------------------------------------------------------------------------------------------------
// One batch = four phases.  Unsharded: they run back to back (search_batch_impl).  Document-sharded: the caller
// (infidex_amd/sharded.py) interleaves the collectives — all-reduce of the class histograms after phase 1, all-gather of the
// per-shard top-`depth` after phase 2, all-reduce of the disjoint Stage-2 records after phase 3.

// FstIndex.MatchWithinEditDistance1 for the distinct unknown words of a batch that the expansion cache does not hold: one infx_ld1_expand call; the few
// words the kernel hands back (work lists outgrown, longer than 64 characters) are expanded by the host walk.  Results enter the LRU cache as before.
// Words of the batch that wait for the device expansion fused into the union build (infx_union_build_ld1): placeholders until the members are back
struct DevLd1 { std::vector<ustr> words; std::vector<std::shared_ptr<FuzzyUnion>> fz; };
static int32_t expand_pending(infx_engine* e, infx_session* S, std::vector<QueryPlan>& plans, DevLd1* dev) {
    const HostIndex& ix = e->ix;
    std::vector<const ustr*> words; std::unordered_map<std::u16string, uint32_t> idx;
    for (auto& P : plans) for (auto& r : P.rawTok) if (r.pending && idx.emplace(r.text, (uint32_t)words.size()).second) words.push_back(&r.text);
    if (words.empty()) return INFX_OK;
    const uint32_t nw = (uint32_t)words.size(), cap = 1024;
    static const bool fusedOff = [] { const char* v = getenv("INFX_LD1_FUSED"); return v && v[0] == '0'; }();
    if (dev && !fusedOff && e->ld1_on_device(0.021 * (double)nw)) {
        // the device expands these words inside the union build (one wait for the device instead of two): every occurrence gets the word's placeholder union
        dev->words.resize(nw); dev->fz.resize(nw);
        for (uint32_t i = 0; i < nw; i++) { dev->words[i] = *words[i]; dev->fz[i] = std::make_shared<FuzzyUnion>(); }
        for (auto& P : plans) for (auto& r : P.rawTok) if (r.pending) { r.fz = dev->fz[idx.at(r.text)]; r.pending = false; }
        return INFX_OK;
    }
    std::vector<std::shared_ptr<FuzzyUnion>> made(nw);
    std::vector<uint32_t> offs(nw + 1, 0), counts(nw, 0), status(nw, 2); std::vector<u16> chars; std::vector<int32_t> members((size_t)nw * cap);
    for (uint32_t i = 0; i < nw; i++) { if (words[i]->size() <= 64) chars.insert(chars.end(), words[i]->begin(), words[i]->end()); offs[i + 1] = (uint32_t)chars.size(); }     // longer words: empty -> status 2
    auto t0 = std::chrono::steady_clock::now();
    if (e->ld1_on_device(0.021 * (double)nw)) {
        int32_t rc;
        { PlanGatePause pause; rc = infx_ld1_expand(S->stream, nw, offs.data(), (const uint16_t*)chars.data(), cap, members.data(), counts.data(), status.data()); }
        if (rc) { g_eerr = infx_last_error(); return rc; }
        S->batch->tLd1Dev = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    }      // else: status stays 2 for every word -> the host walk below, spread over the planner threads
    std::vector<uint32_t> onHost;
    for (uint32_t i = 0; i < nw; i++) {
        if (status[i] == 0) made[i] = union_of_matches(ix, members.data() + (size_t)i * cap, std::min(counts[i], cap));
        else onHost.push_back(i);
    }
    if (!onHost.empty())
        parallel_dyn((int64_t)onHost.size(), e->threads, 1, [&](int64_t b, int64_t en, int) {
            std::vector<int> m;
            for (int64_t k = b; k < en; k++) { const uint32_t i = onHost[k]; match_ld1(ix, *words[i], m, (int)cap); made[i] = union_of_matches(ix, m.data(), m.size()); }
        });
    e->fuzzy.ld1Ns += std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - t0).count();
    e->fuzzy.fuzzyCalls += nw; e->ld1OnHost += (long long)onHost.size(); e->ld1OnDevice += (long long)(nw - onHost.size());
    for (uint32_t i = 0; i < nw; i++) made[i] = e->fuzzy.put(*words[i], made[i]);
    for (auto& P : plans) for (auto& r : P.rawTok) if (r.pending) { r.fz = made[idx.at(r.text)]; r.pending = false; }
    return INFX_OK;
}
static int32_t ph_plan(infx_engine* e, infx_session* S, uint32_t nq, const uint16_t* q_arena, const uint64_t* q_offs, int32_t depth) {
    if (!e || (nq && (!q_arena || !q_offs))) return efail(INFX_EINVAL, "bad arguments");
    e->searched.store(true, std::memory_order_relaxed);
    if (!e->dev || !S || !S->stream) return efail(INFX_EHIP, "no GPU: the scoring hot path has no CPU fallback");
    if (depth <= 0 || depth > e->ix.cfg.maxDepth) return efail(INFX_EINVAL, "CoverageDepth exceeds the engine's max_depth");
    const HostIndex& ix = e->ix; const int threads = e->threads;
    Batch& B = *S->batch; B = Batch(); B.nq = nq; B.depth = depth;
    g_eerr.clear();
    B.t0 = now_ms();
    std::vector<QueryPlan>& plans = S->lastPlans; plans.assign(nq, QueryPlan());
    const bool devLd1 = e->devLookups;      // unknown words are collected per batch; who expands them is decided once their number is known
    // plan exchange (document shards): the token-level plan of a query may have been made by the rank whose slice holds it (infx_session_prefetch_*);
    // it is used when it was made for exactly this text and depth, and only the cache / expansion pass runs here
    const bool havePre = S->planPre.size() == nq;
    std::atomic<uint32_t> nPre{0}, nPeer{0}; std::atomic<const char*> badRec{nullptr};
    parallel_dyn(nq, threads, devLd1 ? 8 : 1, [&](int64_t b, int64_t en, int) {
        for (int64_t i = b; i < en; i++) {
            const u16* rp = (const u16*)q_arena + q_offs[i]; const size_t rl = (size_t)(q_offs[i + 1] - q_offs[i]);
            infx_session::PlanPre* pre = havePre ? S->planPre[i].get() : nullptr;
            if (pre && !pre->planTaken && pre->depth == depth && pre->rawHash == raw_hash((const uint16_t*)rp, rl)) {
                // (the entry keeps its coverage query — parsed, or where it sits in the record — for build_fused_inputs)
                if (pre->rec) { const char* why = parse_plan_record(ix, pre->rec, pre->recLen, depth, plans[i], pre->hasCov, pre->covErr, pre->covOff, pre->longCov); if (why) badRec.store(why); }
                else { plans[i] = std::move(pre->own->plan); pre->planTaken = true; }      // a second phase 0 on the same entries (INFX_PHASED, an empty batch: build_fused_inputs did not clear them) plans afresh instead of taking the moved-from plan
                nPre++; if (S->planPeer[i]) nPeer++;
            } else {
                if (havePre) S->planPre[i] = nullptr;      // not this query's: build_fused_inputs must not take its coverage query either
                plan_tokens_text(ix, uview(rp, rl), depth, plans[i]);
            }
            plan_tokens_expand(ix, e->fuzzy, plans[i], false, devLd1);
        }
    });
    S->planFromExchange = nPre.load(); S->planFromPeers = nPeer.load();
    if (badRec.load()) { S->planPre.clear(); S->planPeer.clear(); return efail(INFX_EINVAL, std::string("exchanged plan record: ") + badRec.load()); }
    DevLd1 dl;
    if (devLd1) { int32_t rc = expand_pending(e, S, plans, &dl); if (rc) return rc; }
    B.tTok = now_ms() - B.t0;
    {   // every fuzzy union this batch uses is materialised on the device (this shard's slice); |union| = its df (sharded:
        // summed over the shards by the caller)
        // One union per distinct misspelt WORD of the batch, in first-occurrence order: the list must be the same on every rank (the counts are
        // all-reduced position by position), so it may not depend on the state of the expansion cache — two queries of a batch can hold two
        // FuzzyUnion objects for one word when the LRU cache evicted it in between (the objects have the same members: LD1 is a function of the word).
        B.pending.clear(); B.unionIdx.clear();
        std::unordered_map<std::u16string, uint32_t> byWord;
        for (auto& P : plans) for (auto& r : P.rawTok) if (r.fz && !r.fz->materialised) {
            auto it = byWord.find(r.text);
            uint32_t v;
            if (it == byWord.end()) { v = (uint32_t)B.pending.size(); byWord.emplace(r.text, v); B.pending.push_back(r.fz); } else v = it->second;
            B.unionIdx.emplace(r.fz.get(), v);
        }
        B.pendingCounts.assign(B.pending.size(), 0);
        std::vector<uint32_t> mo(B.pending.size() + 1, 0); std::vector<int32_t> mm;
        for (size_t v = 0; v < B.pending.size(); v++) { mm.insert(mm.end(), B.pending[v]->members.begin(), B.pending[v]->members.end()); mo[v + 1] = (uint32_t)mm.size(); }
        const double tu0 = now_ms();
        int32_t rc;
        if (dl.words.empty()) { PlanGatePause pause; rc = infx_union_build(S->stream, (uint32_t)B.pending.size(), mo.data(), mm.data(), B.pendingCounts.data()); }
        else {
            // k_ld1 for the placeholders' words, k_union for every union of the batch, one wait (infx_union_build_ld1)
            const uint32_t nw = (uint32_t)dl.words.size(), cap = 1024;
            std::unordered_map<const FuzzyUnion*, int32_t> wordOfFz; for (uint32_t w = 0; w < nw; w++) wordOfFz.emplace(dl.fz[w].get(), (int32_t)w);
            std::vector<int32_t> wordOf(B.pending.size(), -1);
            for (size_t v = 0; v < B.pending.size(); v++) { auto it = wordOfFz.find(B.pending[v].get()); if (it != wordOfFz.end()) wordOf[v] = it->second; }
            std::vector<uint32_t> wo(nw + 1, 0), lc(nw, 0), ls(nw, 2); std::vector<u16> wc; std::vector<int32_t> lm((size_t)nw * cap);
            for (uint32_t w = 0; w < nw; w++) { if (dl.words[w].size() <= 64) wc.insert(wc.end(), dl.words[w].begin(), dl.words[w].end()); wo[w + 1] = (uint32_t)wc.size(); }      // longer words: empty -> status 2
            { PlanGatePause pause; rc = infx_union_build_ld1(S->stream, (uint32_t)B.pending.size(), mo.data(), mm.data(), wordOf.data(), nw, wo.data(), (const uint16_t*)wc.data(), cap,
                                                            B.pendingCounts.data(), lm.data(), lc.data(), ls.data()); }
            if (rc) { g_eerr = infx_last_error(); return rc; }
            B.tLd1Dev = now_ms() - tu0;
            std::vector<uint32_t> onHost;
            for (uint32_t w = 0; w < nw; w++) {
                if (ls[w] == 0) { auto u = union_of_matches(ix, lm.data() + (size_t)w * cap, std::min(lc[w], cap)); dl.fz[w]->members.swap(u->members); }
                else onHost.push_back(w);
            }
            e->ld1OnDevice += (long long)(nw - onHost.size()); e->ld1OnHost += (long long)onHost.size(); e->fuzzy.fuzzyCalls += nw;
            if (!onHost.empty()) {
                // the few words the kernel handed back: host walk, then the unions once more with every member list known
                parallel_dyn((int64_t)onHost.size(), threads, 1, [&](int64_t b, int64_t en, int) {
                    std::vector<int> m;
                    for (int64_t k = b; k < en; k++) { const uint32_t w = onHost[k]; match_ld1(ix, dl.words[w], m, (int)cap); auto u = union_of_matches(ix, m.data(), m.size()); dl.fz[w]->members.swap(u->members); }
                });
                mm.clear();
                for (size_t v = 0; v < B.pending.size(); v++) { mm.insert(mm.end(), B.pending[v]->members.begin(), B.pending[v]->members.end()); mo[v + 1] = (uint32_t)mm.size(); }
                { PlanGatePause pause; rc = infx_union_build(S->stream, (uint32_t)B.pending.size(), mo.data(), mm.data(), B.pendingCounts.data()); }
                if (rc) { g_eerr = infx_last_error(); return rc; }
            }
            for (uint32_t w = 0; w < nw; w++) e->fuzzy.put(dl.words[w], dl.fz[w]);      // into the expansion cache (LRU 1000, as the reference's)
        }
        if (rc) { g_eerr = infx_last_error(); return rc; }
        B.tUnionDev = now_ms() - tu0;
    }
    B.tUnion = now_ms() - B.t0;
    return INFX_OK;
}

// second half of planning: global df of the pending unions known
static int32_t ph_plan_finish(infx_engine* e, infx_session* S, const uint32_t* globalUnionCounts) {
    const HostIndex& ix = e->ix; const int threads = e->threads;
    Batch& B = *S->batch; const uint32_t nq = B.nq;
    std::vector<QueryPlan>& plans = S->lastPlans;
    for (size_t v = 0; v < B.pending.size(); v++) B.pending[v]->df.store((int)globalUnionCounts[v]);
    for (auto& kv : B.unionIdx) const_cast<FuzzyUnion*>(kv.first)->df.store((int)globalUnionCounts[kv.second]);      // every object of the word, not only the first
    parallel_dyn(nq, threads, 8, [&](int64_t b, int64_t en, int) { for (int64_t i = b; i < en; i++) plan_finish(ix, plans[i]); });
    B.tPlanPar = now_ms() - B.t0;
    const int32_t sb = e->shardBase, se = e->shardBase + e->shardN;
    const bool sharded = e->nranks > 1;
    auto shard_slice = [&](const std::vector<int32_t>& d, size_t& lo, size_t& hi) {
        if (!sharded) { lo = 0; hi = d.size(); return; }
        lo = std::lower_bound(d.begin(), d.end(), sb) - d.begin(); hi = std::lower_bound(d.begin(), d.end(), se) - d.begin();
    };
    size_t nterm = 0, nextra = 0;
    std::vector<size_t> termBase(nq), extraBase(nq);
    B.devOf.assign(nq, -1);
    for (uint32_t i = 0; i < nq; i++) {
        QueryPlan& P = plans[i];
        termBase[i] = nterm; extraBase[i] = nextra;
        if (P.blank || P.unsupported || P.noTerms) continue;
        P.q.term_off = (uint32_t)nterm; nterm += P.terms.size();
        for (size_t k = 0; k < P.terms.size(); k++) if (P.terms[k].term_id < 0) {
            if (P.terms[k].reserved == 1) continue;
            else { size_t lo, hi; shard_slice(P.fuzzy[k]->docs, lo, hi); nextra += hi - lo; }
        }
        B.devOf[i] = (int)B.dq.size(); B.dq.push_back(P.q); B.qmap.push_back(i);
    }
    if (nextra > 0xFFFFFFF0ull) return efail(INFX_ECAPACITY, "fuzzy unions of this batch exceed 2^32 postings; split the batch");
    B.dterms.resize(nterm); B.extra.resize(nextra);
    parallel_dyn(nq, threads, 8, [&](int64_t b, int64_t en, int) {
        for (int64_t i = b; i < en; i++) {
            QueryPlan& P = plans[i];
            if (P.blank || P.unsupported || P.noTerms) continue;
            size_t xo = extraBase[i];
            for (size_t k = 0; k < P.terms.size(); k++) {
                infx_term t = P.terms[k];
                if (t.term_id < 0 && t.reserved == 1) {     // union materialised on the device by ph_plan
                    const uint32_t v = B.unionIdx.at(P.fuzzy[k].get());
                    t.reserved = 2; t.extra_off = v; t.extra_len = B.pendingCounts[v];
                } else if (t.term_id < 0) {     // host-built union: global ids -> this shard's slice, rebased (its df / idf stay global)
                    const auto& d = P.fuzzy[k]->docs; size_t lo, hi; shard_slice(d, lo, hi);
                    t.extra_off = (uint32_t)xo; t.extra_len = (uint32_t)(hi - lo);
                    for (size_t z = lo; z < hi; z++) B.extra[xo + (z - lo)] = d[z] - sb;
                    xo += hi - lo;
                }
                B.dterms[termBase[i] + k] = t;
            }
        }
    });
    B.nd = (uint32_t)B.dq.size();
    B.t1 = now_ms();
    return INFX_OK;
}

static int32_t ph_accumulate(infx_engine* e, infx_session* S) {
    Batch& B = *S->batch;
    B.counts.assign(B.nd, infx_counts{});
    S->msAcc = S->msSel = S->msCov = S->msPrep2 = S->msFin = 0; S->algBytes = 0;
    if (B.nd) {
        int32_t rc = infx_stage1_accumulate(S->stream, B.nd, B.dq.data(), (uint32_t)B.dterms.size(), B.dterms.data(), (uint32_t)B.extra.size(), B.extra.data(), B.counts.data());
        if (rc) { g_eerr = infx_last_error(); return rc; }
    }
    return INFX_OK;
}

static int32_t ph_select(infx_engine* e, infx_session* S, const infx_counts* globalCounts) {
    Batch& B = *S->batch; const HostIndex& ix = e->ix;
    std::vector<infx_hit>& hits = S->lastHits; std::vector<uint32_t>& hitCount = S->lastHitCount;
    hits.assign((size_t)B.nd * B.depth, infx_hit{0, 0.f}); hitCount.assign(B.nd, 0); S->lastStride = B.depth;
    if (B.nd) {
        int32_t rc = infx_stage1_select(S->stream, B.nd, globalCounts, hits.data(), hitCount.data());
        if (rc) { g_eerr = infx_last_error(); return rc; }
        infx_last_timings(S->stream, &S->msAcc, &S->msSel, nullptr);
        infx_last_alg_bytes(S->stream, &S->streamedBytes);
        infx_last_candidates(S->stream, &S->s1Candidates); infx_last_exact_replays(S->stream, &S->exactReplays);
        // B_alg(q) = sum_t df_t * 5 B (4 B for fuzzy virtual terms) + card(C_q) * 4 B + depth * 12 B   (this shard's slices)
        uint64_t ab = 0;
        for (auto& t : B.dterms) {
            if (t.term_id >= 0) ab += (uint64_t)e->shardTermLen(t.term_id) * 5ull;
            else ab += (uint64_t)t.extra_len * 4ull;
        }
        uint64_t nh = 0; for (uint32_t c : hitCount) nh += c;
        S->algBytes = ab + S->s1Candidates * 4ull + nh * 12ull;
    }
    (void)ix;
    B.t2 = now_ms();
    return INFX_OK;
}

// allHits: W x nd x depth (global internal ids), allCounts: W x nd.  Runs the local part of Stage 2.
static int32_t ph_stage2(infx_engine* e, infx_session* S, int W, const infx_hit* allHits, const uint32_t* allCounts, int32_t max_results, int32_t enable_coverage) {
    Batch& B = *S->batch; const HostIndex& ix = e->ix; const int threads = e->threads;
    const uint32_t nq = B.nq, nd = B.nd; const int depth = B.depth;
    B.maxResults = max_results;
    std::vector<QueryPlan>& plans = S->lastPlans;
    B.pq.assign(nq, PerQ());
    std::vector<std::vector<infx_cov_cand>> candLocal(nq);
    std::vector<infx_cov_query> covQ(nq); std::vector<std::unique_ptr<infx_cov_query_long>> covL(nq);      // covL: queries beyond the fast Stage-2 envelope
    std::vector<int32_t> covErr(nq, 0);
    const bool covEnabled = ix.cfg.enableCoverage && enable_coverage;
    static const bool dbg = getenv("INFX_DEBUG") != nullptr;
    std::atomic<long long> nsMerge{0}, nsWm{0}, nsSel{0}, nsCovQ{0}, nsPush{0}, nsSelMax{0};
    auto tick = [] { return std::chrono::steady_clock::now(); };
    auto since = [](std::chrono::steady_clock::time_point t) { return (long long)std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - t).count(); };
    parallel_dyn(nq, threads, 4, [&](int64_t b, int64_t en, int) {
        WmResult wm; std::vector<int32_t> sortedTop, overlap, uniq; std::vector<infx_hit> merged; std::vector<uint8_t> hitFlag; std::vector<uint32_t> sbase;
        for (int64_t i = b; i < en; i++) {
            QueryPlan& P = plans[i]; PerQ& Sq = B.pq[i];
            auto tA = tick();
            if (P.blank || P.unsupported) { Sq.done = true; continue; }
            int j = B.devOf[i];
            if (j >= 0) {
                // global top-`depth` = best `depth` of the union of the per-shard top-`depth` lists, device order (score desc, id asc)
                merged.clear();
                for (int w = 0; w < W; w++) { uint32_t c = allCounts[(size_t)w * nd + j]; const infx_hit* H = allHits + ((size_t)w * nd + j) * depth; merged.insert(merged.end(), H, H + c); }
                if (W > 1) {
                    std::sort(merged.begin(), merged.end(), [](const infx_hit& x, const infx_hit& y) { if (x.score != y.score) return x.score > y.score; return x.doc < y.doc; });
                    if ((int)merged.size() > depth) merged.resize(depth);
                }
                uint32_t c = (uint32_t)merged.size();
                Sq.stage1.resize(c); Sq.stage1Doc.resize(c);
                // TopKHeap -> ConsolidateSegments: (score desc, key asc)
                std::sort(merged.begin(), merged.end(), [&](const infx_hit& x, const infx_hit& y) { if (x.score != y.score) return x.score > y.score; return ix.docKey[x.doc] < ix.docKey[y.doc]; });
                for (uint32_t k = 0; k < c; k++) { Sq.stage1[k] = Entry{merged[k].score, ix.docKey[merged[k].doc], 0}; Sq.stage1Doc[k] = merged[k].doc; }
            }
            const ustr& st = P.searchText;
            bool isShort = !st.empty() && st.size() <= 3;
            if (isShort) for (u16 ch : st) if (is_delim(ch)) { isShort = false; break; }
            if (isShort && (int)Sq.stage1.size() >= qo_max(S, i, max_results)) { Sq.done = true; continue; }     // SearchPipeline.cs:114-120
            int shortCount = 0;
            if (isShort) { int64_t pk = ix.prefixKeys.find(st); shortCount = pk >= 0 ? (int)ix.prefixPop[pk] : 0; }
            bool skipCov = isShort && shortCount > 500;
            if (!qo_cov(S, i, covEnabled) || skipCov) { Sq.done = true; continue; }
            Sq.runCov = true;
            if (dbg) nsMerge += since(tA);
            auto tB = tick();
            // ---- ExecuteCoverageStage preparation ----
            wm_collect(ix, st, ix.cfg.coverPrefixSuffix, wm);
            Sq.wmAny = wm.any;
            if (dbg) nsWm += since(tB);
            auto tC = tick();
            size_t ntop = std::min<size_t>(Sq.stage1.size(), (size_t)depth);
            sortedTop.assign(Sq.stage1Doc.begin(), Sq.stage1Doc.begin() + ntop);
            std::sort(sortedTop.begin(), sortedTop.end());
            overlap.clear();
            if (wm.any) { wm_contains_batch(wm, sortedTop.data(), (int)sortedTop.size(), hitFlag, sbase); for (size_t z = 0; z < sortedTop.size(); z++) if (hitFlag[z]) overlap.push_back(sortedTop[z]); }   // ascending
            size_t wmLimit = (size_t)std::max(0, depth - (int)overlap.size());
            size_t need = std::max<size_t>(wmLimit, 2);
            const uint8_t* del = e->deleted.empty() ? nullptr : e->deleted.data();     // Document.Deleted per global internal id
            int32_t live[2] = {-1, -1};
            wm_first_unique(wm, sortedTop, need, uniq, del, (int)std::max<int64_t>(0, 2 - (int64_t)ntop), live);
            // docIndex 0/1 = first two keys in insertion order: Stage-1 docs, then the (live) WordMatcher-only ids ascending
            int32_t first2[2] = {-1, -1}; int nf = 0;
            for (size_t k = 0; k < ntop && nf < 2; k++) first2[nf++] = Sq.stage1Doc[k];
            if (!del) { for (size_t k = 0; k < uniq.size() && nf < 2; k++) first2[nf++] = uniq[k]; }
            else for (int k = 0; k < 2 && nf < 2; k++) if (live[k] >= 0) first2[nf++] = live[k];
            Sq.idx0 = first2[0]; Sq.idx1 = first2[1];
            if (dbg) { long long d = since(tC); nsSel += d; long long cur = nsSelMax.load(); while (d > cur && !nsSelMax.compare_exchange_weak(cur, d)) {} }
            auto tD = tick();
            covErr[i] = prepare_cov_any(ix, st, covQ[i], covL[i]);
            if (!covErr[i]) { if (covL[i]) covL[i]->lcs_tolerance = qc_tolerance(S, (size_t)i, covL[i]->text_len); else covQ[i].lcs_tolerance = qc_tolerance(S, (size_t)i, covQ[i].text_len); }
            if (dbg) nsCovQ += since(tD);
            if (covErr[i]) continue;
            auto tE = tick();
            auto& CL = candLocal[i];
            auto push = [&](int32_t doc, float base) { infx_cov_cand c{}; c.query = 0; c.doc = doc; c.base_score = base; c.want_lcs = (doc == first2[0] || doc == first2[1]) ? 1 : 0; CL.push_back(c); };
            for (int32_t d : overlap) push(d, 0.f);
            for (size_t k = 0; k < uniq.size() && k < wmLimit; k++) if (!(del && del[uniq[k]])) push(uniq[k], 0.f);     // a deleted id still uses up its wmLimit slot
            float maxT = ntop ? Sq.stage1[0].score : 1.f;
            for (size_t k = 0; k < ntop; k++) {
                push(Sq.stage1Doc[k], maxT > 0 ? Sq.stage1[k].score / maxT : 0.f);
                // a document already evaluated as an overlap row: its LCS is read back from the byte span (infx_cov_cand.want_lcs = 2)
                if (CL.back().want_lcs && std::binary_search(overlap.begin(), overlap.end(), Sq.stage1Doc[k])) CL.back().want_lcs = 2;
            }
            if (dbg) nsPush += since(tE);
        }
    });
    if (dbg) fprintf(stderr, "[infx] prep2 cpu-ms: merge %.1f wm %.1f select %.1f (max %.2f) covq %.1f push %.1f | wall %.1f\n", nsMerge / 1e6, nsWm / 1e6, nsSel / 1e6, nsSelMax / 1e6, nsCovQ / 1e6, nsPush / 1e6, now_ms() - B.t2);
    // a query outside the Stage-2 envelope is answered as "unsupported" (empty result, flag bit 0); the rest of the batch is unaffected
    for (uint32_t i = 0; i < nq; i++) if (covErr[i]) { B.pq[i].runCov = false; B.pq[i].stage1.clear(); B.pq[i].stage1Doc.clear(); B.pq[i].envelope = true; candLocal[i].clear(); }
    std::vector<infx_cov_query> covBatch; std::vector<infx_cov_query_long> covBatchL; std::vector<infx_cov_cand>& cands = S->lastCands;
    size_t ncand = 0;
    for (uint32_t i = 0; i < nq; i++) {
        PerQ& Sq = B.pq[i];
        if (!Sq.runCov) continue;
        Sq.covIndex = (int)covBatch.size(); covBatch.push_back(covQ[i]);
        if (covL[i]) { covBatch.back().reserved = 1 + (int32_t)covBatchL.size(); covBatchL.push_back(*covL[i]); }
        Sq.candOff = (uint32_t)ncand; Sq.candCount = (uint32_t)candLocal[i].size(); ncand += candLocal[i].size();
    }
    cands.resize(ncand);
    const int32_t sb = e->shardBase, se = e->shardBase + e->shardN;
    const bool sharded = e->nranks > 1;
    std::vector<uint64_t> tbytes(nq, 0);
    parallel_dyn(nq, threads, 8, [&](int64_t b, int64_t en, int) {
        for (int64_t i = b; i < en; i++) {
            PerQ& Sq = B.pq[i]; if (!Sq.runCov) continue;
            infx_cov_cand* dst = cands.data() + Sq.candOff; uint64_t tb = 0;
            for (size_t k = 0; k < candLocal[i].size(); k++) {
                infx_cov_cand c = candLocal[i][k]; c.query = (uint32_t)Sq.covIndex; dst[k] = c;
                if (c.doc >= sb && c.doc < se) tb += 2 * (ix.textOff[c.doc + 1] - ix.textOff[c.doc]);
            }
            tbytes[i] = tb;
        }
    });
    S->s2TextBytes = 0; for (uint64_t x : tbytes) S->s2TextBytes += x;
    B.t3 = now_ms();
    // ---------------- Stage 2 on the GPU: the candidates whose text this shard holds ----------------
    std::vector<infx_cov_out>& outs = S->lastOuts; outs.resize(cands.size());
    const bool wantF = e->cfg.want_features != 0;
    if (wantF) S->lastFeat.assign(cands.size() * INFX_NFEAT, 0);
    B.localIdx.clear();
    if (!sharded) {     // every candidate is local: score in place
        S->s2Candidates = cands.size();
        if (!cands.empty()) {
            int32_t rc = covBatchL.empty() ? INFX_OK : infx_stage2_long_queries(S->stream, (uint32_t)covBatchL.size(), covBatchL.data());
            if (!rc) rc = stage_coverage_setup(S, nq, false);
            if (!rc) rc = infx_stage2_batch(S->stream, (uint32_t)covBatch.size(), covBatch.data(), (uint32_t)cands.size(), cands.data(), outs.data(), wantF ? S->lastFeat.data() : nullptr);
            if (rc) { g_eerr = infx_last_error(); return rc; }
            infx_last_timings(S->stream, nullptr, nullptr, &S->msCov);
        }
    } else {
        std::fill(outs.begin(), outs.end(), infx_cov_out{});
        std::vector<infx_cov_cand> local;
        for (size_t i = 0; i < cands.size(); i++) {
            const infx_cov_cand& c = cands[i];
            if (c.doc < sb || c.doc >= se) continue;
            infx_cov_cand l = c; l.doc = c.doc - sb; local.push_back(l); B.localIdx.push_back((uint32_t)i);
        }
        S->s2Candidates = local.size();
        std::vector<infx_cov_out> lout(local.size());
        std::vector<int32_t> lfeat;
        if (wantF) lfeat.assign(local.size() * INFX_NFEAT, 0);
        if (!local.empty()) {
            int32_t rc = covBatchL.empty() ? INFX_OK : infx_stage2_long_queries(S->stream, (uint32_t)covBatchL.size(), covBatchL.data());
            if (!rc) rc = stage_coverage_setup(S, nq, false);
            if (!rc) rc = infx_stage2_batch(S->stream, (uint32_t)covBatch.size(), covBatch.data(), (uint32_t)local.size(), local.data(), lout.data(), wantF ? lfeat.data() : nullptr);
            if (rc) { g_eerr = infx_last_error(); return rc; }
            infx_last_timings(S->stream, nullptr, nullptr, &S->msCov);
            for (size_t i = 0; i < local.size(); i++) {
                outs[B.localIdx[i]] = lout[i];
                if (wantF) std::memcpy(S->lastFeat.data() + (size_t)B.localIdx[i] * INFX_NFEAT, lfeat.data() + i * INFX_NFEAT, INFX_NFEAT * 4);
            }
        }
    }
    {   std::atomic<int> bad{0};
        parallel_for((int64_t)outs.size(), threads, [&](int64_t b, int64_t en, int) { for (int64_t i = b; i < en; i++) if (outs[i].status) { bad.store(1); break; } });
        (void)bad;     // rows with a non-zero status are skipped per query in ph_finalize (result flag bit 3)
    }
    B.t4 = now_ms();
    return INFX_OK;
}

static int32_t ph_finalize(infx_engine* e, infx_session* S, const infx_cov_out* outs, int64_t* out_keys, float* out_scores, uint8_t* out_ties,
                           uint32_t* out_counts, uint32_t* out_flags) {
    Batch& B = *S->batch; const HostIndex& ix = e->ix; const int threads = e->threads;
    const uint32_t nq = B.nq; const int depth = B.depth, stride = B.maxResults;
    std::vector<QueryPlan>& plans = S->lastPlans; std::vector<infx_cov_cand>& cands = S->lastCands;
    parallel_dyn(nq, threads, 8, [&](int64_t b, int64_t en, int) {
        std::vector<Entry> fin, cons;
        for (int64_t i = b; i < en; i++) {
            PerQ& Sq = B.pq[i]; const QueryPlan& P = plans[i];
            const int max_results = qo_max(S, i, B.maxResults);
            uint32_t flags = 0; const std::vector<Entry>* res = &Sq.stage1;
            if (P.unsupported || Sq.envelope) flags |= 1;
            if (Sq.runCov) {
                flags |= 2;
                int maxWordHits = 0; uint8_t hits01[2] = {0, 0}, lcs01[2] = {0, 0};
                fin.clear();
                for (uint32_t k = 0; k < Sq.candCount; k++) {
                    const infx_cov_cand& c = cands[Sq.candOff + k]; const infx_cov_out& o = outs[Sq.candOff + k];
                    if (o.status) { flags |= 8; continue; }          // outside the Stage-2 envelope: left out of this query's ranking
                    maxWordHits = std::max(maxWordHits, o.word_hits_full);
                    for (int z = 0; z < 2; z++) { int32_t dz = z == 0 ? Sq.idx0 : Sq.idx1; if (dz >= 0 && c.doc == dz) { if (hits01[z] == 0) hits01[z] = o.word_hits; if (lcs01[z] == 0) lcs01[z] = o.lcs; } }
                    fin.push_back(Entry{o.score, ix.docKey[c.doc], o.tiebreaker});
                }
                if (maxWordHits == 0 && !Sq.wmAny) { cons.clear(); }
                else {
                    // TopKHeap(depth): best `depth` by the total order, then ConsolidateSegments (best per key, descending)
                    std::sort(fin.begin(), fin.end(), [](const Entry& a, const Entry& c) { return cmp_entry(a, c) > 0; });
                    if ((int)fin.size() > depth) fin.resize(depth);
                    cons.clear();
                    std::unordered_map<int64_t, char> seen; seen.reserve(fin.size() * 2);
                    for (auto& x : fin) if (seen.emplace(x.key, 1).second) cons.push_back(x);
                    int truncIdx = -1;
                    const infx_finalize_setup FS = qc_finalize(S, (size_t)i);      // the values k_finalize reads from its per-query record
                    int minHits = std::max(FS.min_hits_abs, maxWordHits - FS.min_hits_relative);
                    int64_t k0 = Sq.idx0 >= 0 ? ix.docKey[Sq.idx0] : INT64_MIN, k1 = Sq.idx1 >= 0 ? ix.docKey[Sq.idx1] : INT64_MIN;
                    for (int r = (int)cons.size() - 1; r >= 0 && FS.truncate; r--) {
                        uint8_t wh = 0, lc = 0;
                        if (Sq.idx0 >= 0 && cons[r].key == k0) { wh = hits01[0]; lc = lcs01[0]; }
                        else if (Sq.idx1 >= 0 && cons[r].key == k1) { wh = hits01[1]; lc = lcs01[1]; }
                        if (wh >= minHits || lc > 0 || cons[r].score >= (float)FS.truncation_score) { truncIdx = r; break; }
                    }
                    int resultCount = truncIdx == -1 ? max_results : std::min(std::max(0, truncIdx) + 1, max_results);
                    if ((int)cons.size() > resultCount) cons.resize(resultCount);
                }
                if (cons.empty() && !Sq.stage1.empty()) { flags |= 4; res = &Sq.stage1; } else res = &cons;
            }
            uint32_t cnt = (uint32_t)std::min<size_t>(res->size(), (size_t)max_results);
            out_counts[i] = cnt;
            for (uint32_t k = 0; k < cnt; k++) {
                out_keys[(size_t)i * stride + k] = (*res)[k].key; out_scores[(size_t)i * stride + k] = (*res)[k].score;
                if (out_ties) out_ties[(size_t)i * stride + k] = (*res)[k].tie;
            }
            if (out_flags) out_flags[i] = flags;
        }
    });
    double t5 = now_ms();
    if (getenv("INFX_DEBUG")) {
        int nm[4] = {0, 0, 0, 0}; unsigned long long dfsum[4] = {0, 0, 0, 0}; size_t maxT = 0;
        for (auto& P : plans) { if (P.blank || P.unsupported || P.noTerms) continue; nm[P.q.mode]++; maxT = std::max(maxT, P.terms.size());
            for (auto& t : P.terms) dfsum[P.q.mode] += t.term_id >= 0 ? (unsigned long long)ix.terms.len((uint32_t)t.term_id) : t.extra_len; }
        fprintf(stderr, "[infx] modes: prefix=%d disj=%d and=%d | postings per mode: %llu %llu %llu | maxT=%zu\n", nm[1], nm[2], nm[3], dfsum[1], dfsum[2], dfsum[3], maxT);
        fprintf(stderr, "[infx] nq=%u dev=%u terms=%zu extra=%zu cands=%zu | plan %.1f (tokens %.1f unions[%zu] %.1f finish %.1f) s1 %.1f prep2 %.1f s2 %.1f post %.1f ms | fuzzy calls=%lld %.1f ms-cpu (ld1 %.1f) docs=%lld\n",
                nq, B.nd, B.dterms.size(), B.extra.size(), cands.size(), B.t1 - B.t0, B.tTok, B.pending.size(), B.tUnion - B.tTok, B.tPlanPar - B.tUnion, B.t2 - B.t1, B.t3 - B.t2, B.t4 - B.t3, t5 - B.t4,
                (long long)e->fuzzy.fuzzyCalls.exchange(0), e->fuzzy.fuzzyNs.exchange(0) / 1e6, e->fuzzy.ld1Ns.exchange(0) / 1e6, (long long)e->fuzzy.fuzzyDocs.exchange(0));
    }
    S->tPrep1 = B.t1 - B.t0; S->tStage1 = B.t2 - B.t1; S->tPrep2 = B.t3 - B.t2; S->tStage2 = B.t4 - B.t3; S->tPost = t5 - B.t4;
    return INFX_OK;
}

// Per-query inputs of the device pipeline that need the host dictionaries: flags, WordMatcher list descriptors (WordMatcher.Lookup,
// WordMatcher.cs:95-186; affix hits are copied into `owned`), CoverageEngine.PrepareQuery.
// The WordMatcher lists of one search text as device descriptors: (src 0 exact / 1 symmetric-delete dictionary, offset, length) into the uploaded
// doc-id arrays, affix hits (src 2) copied into `owned`.  A pure function of (index, text): document shards compute it for a slice of the batch each
// and exchange the results (infx_session_prefetch_*).
static void wm_descriptors(const HostIndex& ix, const ustr& st, WmResult& wm, std::vector<infx_wm_list>& lists, std::vector<int32_t>& owned) {
    const int32_t* exB = ix.wmExact.doc.data(); const int32_t* exE = exB + ix.wmExact.doc.size();
    const int32_t* l1B = ix.wmLd1.doc.data(); const int32_t* l1E = l1B + ix.wmLd1.doc.size();
    lists.clear(); owned.clear();
    wm_collect(ix, st, ix.cfg.coverPrefixSuffix, wm);
    for (auto& l : wm.lists) {
        if (!l.n) continue;
        infx_wm_list L{}; L.len = (uint32_t)l.n;
        if (l.p >= exB && l.p < exE) { L.src = 0; L.off = (uint64_t)(l.p - exB); }
        else if (l.p >= l1B && l.p < l1E) { L.src = 1; L.off = (uint64_t)(l.p - l1B); }
        else { L.src = 2; L.off = owned.size(); owned.insert(owned.end(), l.p, l.p + l.n); }
        lists.push_back(L);
    }
    if (lists.size() > INFX_MAX_WM_LISTS) {
        // very long queries: the device probes at most INFX_MAX_WM_LISTS lists per query, so the lists are merged here into ONE
        // ascending list (membership in any list / first-unique over the union are unchanged by the merge)
        std::vector<int32_t> all;
        for (auto& l : wm.lists) all.insert(all.end(), l.p, l.p + l.n);
        std::sort(all.begin(), all.end()); all.erase(std::unique(all.begin(), all.end()), all.end());
        owned.swap(all);
        infx_wm_list L{}; L.src = 2; L.off = 0; L.len = (uint32_t)owned.size();
        lists.assign(1, L);
    }
}

// May k_wm look this query's words up?  It reads them from the coverage query text as they stand, where WordMatcherLookup normalises each word again
// (lower + Normalize, WordMatcherLookup.cs:27-31) — the identity on an already prepared search text, checked here; and a query may hold at most
// INFX_MAX_WM_LISTS lists (each word: <= 2 + 2*maxLd1 dictionary hits + 1 affix list).
static bool wm_on_device(const HostIndex& ix, const ustr& st) {
    const auto& T = tables();
    int words = 0; bool same = true;
    for_each_word(st, [&](int off, int len) {
        if (len < 2) return;
        words++;
        for (int i = 0; i < len; i++) { const u16 c = st[off + i]; const u16 n = T.norm[T.lower[c]]; if (n != c || n == u' ') same = false; }
    });
    return same && words * (3 + 2 * ix.cfg.wmMaxLD1) <= INFX_MAX_WM_LISTS;
}
struct FusedIn { std::vector<infx_fused_query> fq; std::vector<infx_cov_query> cq; std::vector<infx_wm_list> lists; std::vector<int32_t> owned;
                 std::vector<infx_cov_query_long> cql; };      // cql: the batch's long-query table (queries beyond the fast Stage-2 envelope; cq[i].reserved = 1 + index)
// the long-query table goes to the stream in front of the Stage-2 call that consumes it (infx_search_fused / infx_shard_stage2)
static int32_t stage_long_queries(infx_session* S, const FusedIn& F) {
    if (F.cql.empty()) return INFX_OK;
    int32_t rc = infx_stage2_long_queries(S->stream, (uint32_t)F.cql.size(), F.cql.data());
    if (rc) g_eerr = infx_last_error();
    return rc;
}
static int32_t build_fused_inputs(infx_engine* e, infx_session* S, int32_t max_results, int32_t enable_coverage, FusedIn& F) {
    Batch& B = *S->batch; const HostIndex& ix = e->ix; const int threads = e->threads; const uint32_t nq = B.nq;
    std::vector<QueryPlan>& plans = S->lastPlans;
    auto& fq = F.fq; auto& cq = F.cq; auto& lists = F.lists; auto& owned = F.owned;
    const bool covEnabled = ix.cfg.enableCoverage && enable_coverage;
    fq.assign(nq, infx_fused_query{}); cq.assign(nq, infx_cov_query{});
    std::vector<std::vector<infx_wm_list>> qLists(nq); std::vector<std::vector<int32_t>> qOwned(nq);
    std::vector<int32_t> covErr(nq, 0);
    std::vector<std::unique_ptr<infx_cov_query_long>> qLong(nq);      // queries beyond the fast envelope
    F.cql.clear();
    bool devWm = e->devLookups && ix.cfg.wordMatcher;
    if (devWm) {      // ~2.5 looked-up words per query: estimated from the batch's text volume (one word per ~7 characters), 7 us of one core each
        size_t chars = 0; for (uint32_t i = 0; i < nq; i++) chars += plans[i].searchText.size();
        devWm = e->lookups_on_device(0.007 * (double)chars / 7.0);
    }
    std::atomic<long long> nDev{0}, nHost{0}; std::atomic<const char*> badRec{nullptr};
    parallel_dyn(nq, threads, 4, [&](int64_t b, int64_t en, int) {
        WmResult wm;
        for (int64_t i = b; i < en; i++) {
            const QueryPlan& P = plans[i]; infx_fused_query& F = fq[i];
            F = infx_fused_query{}; F.dev = -1; F.max_results = qo_max(S, i, max_results);
            if (P.blank || P.unsupported) { F.flags = INFX_FQ_SKIP | (P.unsupported ? INFX_FQ_UNSUPPORTED : 0u) | (P.blank && !P.unsupported && qo_browse(S, i) ? INFX_FQ_BROWSE : 0u); continue; }
            F.dev = B.devOf.empty() ? -1 : B.devOf[i];      // (pre-built in phase 0: filled in by fused_inputs_for_phase3)
            const ustr& st = P.searchText;
            bool isShort = !st.empty() && st.size() <= 3;
            if (isShort) for (u16 ch : st) if (is_delim(ch)) { isShort = false; break; }
            if (isShort) { F.flags |= INFX_FQ_SHORT; int64_t pk = ix.prefixKeys.find(st); int shortCount = pk >= 0 ? (int)ix.prefixPop[pk] : 0; if (shortCount > 500) F.flags |= INFX_FQ_SHORTSKIP; }
            if (!qo_cov(S, i, covEnabled) || (F.flags & INFX_FQ_SHORTSKIP)) {
                // Query.highlight without coverage: k_highlight still reads the query's Stage-2 words from cq[i] (Stage 2 itself ignores the record: no
                // INFX_FQ_COV).  A query beyond the fast envelope is marked (reserved = -1, no record in the long-query table): its rows report "long_query".
                if (S->qh.asks((uint32_t)i)) {
                    std::unique_ptr<infx_cov_query_long> lq;
                    if (prepare_cov_any(ix, st, cq[i], lq) || lq) { std::memset(&cq[i], 0, sizeof cq[i]); cq[i].reserved = -1; }
                }
                continue;
            }
            F.flags |= INFX_FQ_COV;
            const infx_session::PlanPre* pp = S->planPre.size() == nq ? S->planPre[i].get() : nullptr;      // (ph_plan dropped the entries that were not made for this batch)
            if (pp && pp->hasCov) {
                covErr[i] = pp->covErr;
                if (!covErr[i] && pp->longCov) {
                    qLong[i].reset(new infx_cov_query_long);
                    if (pp->rec) { if (const char* why = parse_cov_record_long(st, pp->rec, pp->recLen, pp->covOff, *qLong[i])) badRec.store(why); }
                    else if (pp->own->cql) *qLong[i] = *pp->own->cql; else badRec.store("long coverage query missing");
                }
                else if (!covErr[i] && pp->rec) { if (const char* why = parse_cov_record(st, pp->rec, pp->recLen, pp->covOff, cq[i])) badRec.store(why); }
                else if (!covErr[i]) cq[i] = pp->own->cq;
            } else covErr[i] = prepare_cov_any(ix, st, cq[i], qLong[i]);
            // the LCS tolerance follows the QUERY's CoverageSetup (SearchPipeline.cs:498-499), whoever prepared the record: this rank, or the slice's owner in the plan exchange
            if (!covErr[i]) { if (qLong[i]) qLong[i]->lcs_tolerance = qc_tolerance(S, (size_t)i, qLong[i]->text_len); else cq[i].lcs_tolerance = qc_tolerance(S, (size_t)i, cq[i].text_len); }
            if (devWm && !covErr[i] && !qLong[i] && wm_on_device(ix, st)) { F.flags |= INFX_FQ_WMDEV; nDev++; continue; }      // k_wm resolves the words of cq[i] (lookup.hip.inc; fast-envelope queries)
            auto pre = S->wmPre.find(st);            // computed by a peer rank (sharded planning): same index, same text, same descriptors
            if (pre != S->wmPre.end()) { qLists[i] = pre->second.lists; qOwned[i] = pre->second.owned; }
            else wm_descriptors(ix, st, wm, qLists[i], qOwned[i]);
            nHost++;
        }
    });
    if (badRec.load()) { S->planPre.clear(); S->planPeer.clear(); return efail(INFX_EINVAL, std::string("exchanged plan record: ") + badRec.load()); }
    // a query outside the Stage-2 envelope (INFX_MAX_QUERY_TOKENS / INFX_MAX_QUERY_CHARS / token length) is answered as "unsupported" (empty result,
    // flag bit 0) — it does not fail the other queries of the batch
    for (uint32_t i = 0; i < nq; i++) if (covErr[i]) { fq[i].flags = INFX_FQ_SKIP | INFX_FQ_UNSUPPORTED; qLists[i].clear(); qOwned[i].clear(); }
    e->wmOnDevice += nDev.load(); e->wmOnHost += nHost.load();
    for (uint32_t i = 0; i < nq; i++) if (qLong[i] && !covErr[i]) { std::memset(&cq[i], 0, sizeof cq[i]); cq[i].reserved = 1 + (int32_t)F.cql.size(); F.cql.push_back(*qLong[i]); }
    lists.clear(); owned.clear();
    for (uint32_t i = 0; i < nq; i++) {
        fq[i].wm_off = (uint32_t)lists.size(); fq[i].wm_count = (uint32_t)qLists[i].size();
        if (qLists[i].size() > INFX_MAX_WM_LISTS) return efail(INFX_ECAPACITY, "a query needs more than INFX_MAX_WM_LISTS WordMatcher lists");
        for (auto L : qLists[i]) { if (L.src == 2) L.off += owned.size(); lists.push_back(L); }
        owned.insert(owned.end(), qOwned[i].begin(), qOwned[i].end());
    }
    if (owned.size() > 0xFFFFFFF0ull) return efail(INFX_ECAPACITY, "affix matches of this batch exceed 2^32 ids; split the batch");
    S->wmPre.clear(); S->planPre.clear(); S->planPeer.clear();
    return INFX_OK;
}

// Sharded phases: phase 0 (which may run on a planner thread while another batch is in its collective phases) prepares the inputs;
// phase 3 only fills in what it learns later (the Stage-1 query index, max_results, the caller's coverage switch).
static int32_t fused_inputs_for_phase3(infx_engine* e, infx_session* S, int32_t max_results, int32_t enable_coverage, std::shared_ptr<FusedIn>& out) {
    Batch& B = *S->batch;
    if (!B.pre) { B.pre = std::make_shared<FusedIn>(); int32_t rc = build_fused_inputs(e, S, max_results, 1, *B.pre); if (rc) return rc; }
    FusedIn& F = *B.pre;
    const bool cov = e->ix.cfg.enableCoverage && enable_coverage;
    for (uint32_t i = 0; i < B.nq; i++) {
        infx_fused_query& q = F.fq[i];
        q.max_results = qo_max(S, i, max_results);
        if (!(q.flags & INFX_FQ_SKIP)) q.dev = B.devOf.empty() ? -1 : B.devOf[i];
        else if (!(q.flags & INFX_FQ_UNSUPPORTED)) /* skipped and not unsupported: a blank text */ q.flags = (q.flags & ~INFX_FQ_BROWSE) | (qo_browse(S, i) ? INFX_FQ_BROWSE : 0u);      // (the options the batch runs with)
        if (!qo_cov(S, i, cov)) { q.flags &= ~(INFX_FQ_COV | INFX_FQ_WMDEV); q.wm_count = 0; }
    }
    out = B.pre;
    return INFX_OK;
}

// Unsharded engines: the whole batch on the device with one synchronisation (infx_search_fused).  The host keeps what needs
// its dictionaries: text preparation, term lookup, LD1 expansion, idf / roles (ph_plan*), and per query the WordMatcher list
// descriptors (WordMatcher.Lookup, WordMatcher.cs:95-186) + CoverageEngine.PrepareQuery.
static void resolve_kernel_times(infx_session* S) {
    if (!S->kernelTimesPending || !S->stream) return;
    S->kernelTimesPending = false;
    float ms5[5] = {0, 0, 0, 0, 0}; infx_last_fused_timings(S->stream, ms5);
    S->msAcc = ms5[0]; S->msSel = ms5[1]; S->msPrep2 = ms5[2]; S->msCov = ms5[3]; S->msFin = ms5[4];
    infx_last_replay_stats(S->stream, &S->msReplay, S->flagWhy);
    infx_last_replay_breakdown(S->stream, S->msReplayParts);
}
static int32_t search_batch_fused(infx_engine* e, infx_session* S, uint32_t nq, const uint16_t* q_arena, const uint64_t* q_offs, int32_t max_results,
                                  int32_t depth, int32_t enable_coverage, int64_t* out_keys, float* out_scores, uint8_t* out_ties,
                                  uint32_t* out_counts, uint32_t* out_flags) {
    int32_t rc; FusedIn FI;
    {   PlanGateHold hold(e->gate);
        rc = ph_plan(e, S, nq, q_arena, q_offs, depth); if (rc) return rc;
        rc = ph_plan_finish(e, S, S->batch->pendingCounts.data()); if (rc) return rc;
        rc = build_fused_inputs(e, S, max_results, enable_coverage, FI); if (rc) return rc;
    }
    Batch& B = *S->batch; const HostIndex& ix = e->ix;
    auto& fq = FI.fq; auto& cq = FI.cq; auto& lists = FI.lists; auto& owned = FI.owned;
    B.t2 = now_ms();
    const bool dbg = e->cfg.want_features != 0;
    rc = stage_long_queries(S, FI); if (rc) return rc;
    rc = stage_coverage_setup(S, nq, true); if (rc) return rc;
    // Pre-filters: the masks the batch is missing are staged on the session's stream (one launch in front of the batch, no host wait), each query's flags installed
    MaskCall pre(S, nq);
    rc = stage_prefilters(S, nq, fq, pre); if (rc) return rc;
    rc = stage_collapse(S, nq, fq); if (rc) return pre.failed(rc);
    rc = stage_highlight(S, nq, fq, FI); if (rc) { if (S->qk.on) infx_stream_set_query_collapse(S->stream, 0, nullptr); return pre.failed(rc); }
    rc = infx_search_fused(S->stream, B.nd, B.dq.data(), (uint32_t)B.dterms.size(), B.dterms.data(), nq, fq.data(), cq.data(),
                           (uint32_t)lists.size(), lists.data(), (uint32_t)owned.size(), owned.data(), depth, max_results, dbg ? 1 : 0,
                           out_keys, out_scores, out_ties, out_counts, out_flags);
    if (rc) { if (S->qk.on) infx_stream_set_query_collapse(S->stream, 0, nullptr); if (S->qh.on) infx_stream_set_query_highlight(S->stream, 0, nullptr); return pre.failed(rc); }
    pre.done(nq);
    B.t3 = now_ms();
    // Kernel durations are resolved when somebody asks (infx_engine_session_last_timings): every hipEventElapsedTime is a HIP API call that queues behind the
    // launches of the other sessions (measured: 2.8-3.3 ms of "post" time per batch on two of three boxes with six sessions).
    S->kernelTimesPending = true;
    float ms5[5] = {0, 0, 0, 0, 0};
    static const bool dbgTimes = getenv("INFX_DEBUG") != nullptr;
    if (dbgTimes) { resolve_kernel_times(S); ms5[0] = S->msAcc; ms5[1] = S->msSel; ms5[2] = S->msPrep2; ms5[3] = S->msCov; ms5[4] = S->msFin; }
    uint64_t s1rows = 0; infx_last_fused_stats(S->stream, &s1rows, &S->s2Candidates, &S->s2TextBytes);
    infx_last_alg_bytes(S->stream, &S->streamedBytes); infx_last_candidates(S->stream, &S->s1Candidates); infx_last_exact_replays(S->stream, &S->exactReplays);
    {   // B_alg(q) = sum_t df_t * 5 B (4 B for fuzzy virtual terms) + card(C_q) * 4 B + depth * 12 B
        uint64_t ab = 0;
        for (auto& t : B.dterms) ab += t.term_id >= 0 ? (uint64_t)e->shardTermLen(t.term_id) * 5ull : (uint64_t)t.extra_len * 4ull;
        S->algBytes = B.nd ? ab + S->s1Candidates * 4ull + s1rows * 12ull : 0;
    }
    if (dbg) {   // parity tests: pull the intermediate device tables into the session's introspection buffers
        const size_t stride = 2 * (size_t)depth;
        std::vector<infx_hit> s1((size_t)nq * depth); std::vector<uint32_t> s1c(nq), cc(nq), rcv(nq);
        std::vector<infx_cov_cand> cands(nq * stride); std::vector<infx_cov_out> outs(nq * stride); std::vector<int32_t> feat(nq * stride * INFX_NFEAT);
        rc = infx_fused_debug(S->stream, s1.data(), s1c.data(), cands.data(), outs.data(), feat.data(), cc.data(), rcv.data(), nullptr);
        if (rc) { g_eerr = infx_last_error(); return rc; }
        S->lastHits.assign((size_t)B.nd * depth, infx_hit{0, 0.f}); S->lastHitCount.assign(B.nd, 0); S->lastStride = depth;
        S->lastCands.clear(); S->lastOuts.clear(); S->lastFeat.clear();
        uint32_t covIndex = 0;
        for (uint32_t i = 0; i < nq; i++) {
            const int j = B.devOf.empty() ? -1 : B.devOf[i];
            if (j >= 0) { S->lastHitCount[j] = s1c[i]; std::memcpy(S->lastHits.data() + (size_t)j * depth, s1.data() + (size_t)i * depth, (size_t)s1c[i] * sizeof(infx_hit)); }
            if (!(rcv[i] & 1)) continue;
            for (uint32_t k = 0; k < cc[i]; k++) {
                infx_cov_cand c = cands[i * stride + k]; c.query = covIndex;
                S->lastCands.push_back(c); S->lastOuts.push_back(outs[i * stride + k]);
                S->lastFeat.insert(S->lastFeat.end(), feat.begin() + (i * stride + k) * INFX_NFEAT, feat.begin() + (i * stride + k + 1) * INFX_NFEAT);
            }
            covIndex++;
        }
    }
    double t5 = now_ms();
    if (getenv("INFX_DEBUG"))
        fprintf(stderr, "[infx] fused nq=%u dev=%u terms=%zu lists=%zu owned=%zu cands=%llu | plan %.1f (tokens %.1f unions[%zu] %.1f finish %.1f) wm-prep %.1f gpu %.1f (acc %.2f sel %.2f prep2 %.2f s2 %.2f fin %.2f) post %.1f ms | fuzzy calls=%lld %.1f ms-cpu\n",
                nq, B.nd, B.dterms.size(), lists.size(), owned.size(), (unsigned long long)S->s2Candidates, B.t1 - B.t0, B.tTok, B.pending.size(), B.tUnion - B.tTok, B.tPlanPar - B.tUnion,
                B.t2 - B.t1, B.t3 - B.t2, ms5[0], ms5[1], ms5[2], ms5[3], ms5[4], t5 - B.t3, (long long)e->fuzzy.fuzzyCalls.exchange(0), e->fuzzy.fuzzyNs.exchange(0) / 1e6);
    S->tPrep1 = B.t1 - B.t0; S->tStage1 = 0; S->tPrep2 = B.t2 - B.t1; S->tStage2 = B.t3 - B.t2; S->tPost = t5 - B.t3;
    return INFX_OK;
}

static int32_t search_batch_run(infx_engine* e, infx_session* S, uint32_t nq, const uint16_t* q_arena, const uint64_t* q_offs, int32_t max_results,
                                int32_t depth, int32_t enable_coverage, int64_t* out_keys, float* out_scores, uint8_t* out_ties,
                                uint32_t* out_counts, uint32_t* out_flags);
// a search call on a session: per-query options installed on it apply to this batch (and are cleared after it, whatever its outcome)
static int32_t search_batch_impl(infx_engine* e, infx_session* S, uint32_t nq, const uint16_t* q_arena, const uint64_t* q_offs, int32_t max_results,
                                 int32_t depth, int32_t enable_coverage, int64_t* out_keys, float* out_scores, uint8_t* out_ties,
                                 uint32_t* out_counts, uint32_t* out_flags) {
    if (!e || !S || (nq && (!q_arena || !q_offs || !out_keys || !out_scores || !out_counts)) || max_results < 1) return efail(INFX_EINVAL, "bad arguments");
    { int32_t rc = query_parts_check(S, nq, max_results); if (rc) return rc; }
    e->searched.store(true, std::memory_order_relaxed);
    S->lastInPre.assign(nq, 0); S->lastHlChars.clear(); S->lastHlQuery.clear();
    int32_t rc = search_batch_run(e, S, nq, q_arena, q_offs, max_results, depth, enable_coverage, out_keys, out_scores, out_ties, out_counts, out_flags);
    const int32_t rc2 = query_parts_finish(S, out_counts, out_flags, rc == INFX_OK && e->indexed);
    return rc ? rc : rc2;
}
static int32_t search_batch_run(infx_engine* e, infx_session* S, uint32_t nq, const uint16_t* q_arena, const uint64_t* q_offs, int32_t max_results,
                                int32_t depth, int32_t enable_coverage, int64_t* out_keys, float* out_scores, uint8_t* out_ties,
                                uint32_t* out_counts, uint32_t* out_flags) {
    if (!e->indexed) { for (uint32_t i = 0; i < nq; i++) out_counts[i] = 0; return INFX_OK; }   // Result.MakeEmptyResult(), SearchEngine.cs:261-262
    if (e->nranks > 1) return efail(INFX_EINVAL, "sharded engine: drive the phase API (infx_session_phase1..4) with the collectives in between");
    if (!host_phases()) return search_batch_fused(e, S, nq, q_arena, q_offs, max_results, depth, enable_coverage, out_keys, out_scores, out_ties, out_counts, out_flags);
    int32_t rc = ph_plan(e, S, nq, q_arena, q_offs, depth); if (rc) return rc;
    rc = ph_plan_finish(e, S, S->batch->pendingCounts.data()); if (rc) return rc;
    rc = ph_accumulate(e, S); if (rc) return rc;
    rc = ph_select(e, S, S->batch->counts.data()); if (rc) return rc;
    rc = ph_stage2(e, S, 1, S->lastHits.data(), S->lastHitCount.data(), max_results, enable_coverage); if (rc) return rc;
    return ph_finalize(e, S, S->lastOuts.data(), out_keys, out_scores, out_ties, out_counts, out_flags);
}

int32_t infx_engine_search_batch(infx_engine* e, uint32_t nq, const uint16_t* q_arena, const uint64_t* q_offs, int32_t max_results,
                                 int32_t depth, int32_t enable_coverage, int64_t* out_keys, float* out_scores, uint8_t* out_ties,
                                 uint32_t* out_counts, uint32_t* out_flags) {
    if (!e) return efail(INFX_EINVAL, "null engine");
    return search_batch_impl(e, e->def, nq, q_arena, q_offs, max_results, depth, enable_coverage, out_keys, out_scores, out_ties, out_counts, out_flags);
}
int32_t infx_engine_session_create(infx_engine* e, infx_session** out) {
    if (!e || !out) return efail(INFX_EINVAL, "null");
    if (!e->indexed || !e->dev) return efail(INFX_EINVAL, "sessions need an indexed engine with a GPU");
    infx_session* S = new infx_session(); S->e = e; S->batch = new Batch();
    int32_t rc = infx_stream_create(e->dev, &S->stream);
    if (rc) { g_eerr = infx_last_error(); delete S->batch; delete S; return rc; }
    *out = S; return INFX_OK;
}
void infx_engine_session_destroy(infx_session* S) { if (!S) return; if (S->stream) infx_stream_destroy(S->stream); delete S->batch; delete S; }
int32_t infx_engine_session_stream_native(infx_session* S, void** hip_stream) {
    if (!S || !S->stream) return efail(INFX_EINVAL, "null");
    int32_t rc = infx_stream_native(S->stream, hip_stream);
    if (rc) g_eerr = infx_last_error();
    return rc;
}
int32_t infx_engine_stream_native(infx_engine* e, void** hip_stream) {
    if (!e || !e->def || !e->def->stream) return efail(INFX_EINVAL, "the engine has no GPU stream (not indexed, or no device)");
    int32_t rc = infx_stream_native(e->def->stream, hip_stream);
    if (rc) g_eerr = infx_last_error();
    return rc;
}
int32_t infx_engine_session_stream_budget(infx_session* S, int32_t* normal, int32_t* high) {
    if (!S || !S->stream) return efail(INFX_EINVAL, "null");
    int32_t rc = infx_stream_budget(S->stream, normal, high);
    if (rc) g_eerr = infx_last_error();
    return rc;
}
int32_t infx_engine_session_search_batch(infx_session* S, uint32_t nq, const uint16_t* q_arena, const uint64_t* q_offs, int32_t max_results,
                                         int32_t depth, int32_t enable_coverage, int64_t* out_keys, float* out_scores, uint8_t* out_ties,
                                         uint32_t* out_counts, uint32_t* out_flags) {
    if (!S) return efail(INFX_EINVAL, "null session");
    return search_batch_impl(S->e, S, nq, q_arena, q_offs, max_results, depth, enable_coverage, out_keys, out_scores, out_ties, out_counts, out_flags);
}
// ---- sharded operation: phases with the collectives in between (infidex_amd/sharded.py) ----
int32_t infx_engine_add_synonym(infx_engine* e, const uint16_t* a, int32_t la, const uint16_t* b, int32_t lb) {
    if (!e || !a || !b || la < 0 || lb < 0) return efail(INFX_EINVAL, "bad arguments");
    if (e->indexed) return efail(INFX_EINVAL, "synonyms must be added before IndexDocuments");
    e->ix.cfg.syn.add(uview((const u16*)a, (size_t)la), uview((const u16*)b, (size_t)lb));
    return INFX_OK;
}
int32_t infx_engine_set_shard(infx_engine* e, int32_t rank, int32_t nranks) {
    if (!e || nranks < 1 || rank < 0 || rank >= nranks) return efail(INFX_EINVAL, "bad shard arguments");
    if (e->indexed) return efail(INFX_EINVAL, "set the shard before IndexDocuments");
    e->rank = rank; e->nranks = nranks; return INFX_OK;
}
int32_t infx_engine_shard_info(infx_engine* e, int32_t* base, int32_t* n) { if (!e) return INFX_EINVAL; if (base) *base = e->shardBase; if (n) *n = e->shardN; return INFX_OK; }
int32_t infx_session_phase0(infx_session* S, uint32_t nq, const uint16_t* q_arena, const uint64_t* q_offs, int32_t depth, uint32_t* nunions) {
    if (!S) return efail(INFX_EINVAL, "null session");
    // the exact cut across shards falls back to a chained sequential replay whose exchanged state is laid out for max_depth entries (infx_shard_replay_chain)
    if (S->e && S->e->nranks > 1 && depth != S->e->ix.cfg.maxDepth) return efail(INFX_EINVAL, "document shards search with CoverageDepth == the engine's max_depth");
    query_parts_unbind(S);        // what a sharded batch left that failed between its phase 0 and phase 4
    { int32_t rc = query_parts_check(S, nq, 0); if (rc) return rc; }
    query_parts_bind(S); S->lastInPre.assign(nq, 0);
    PlanGateHold hold(S->e->gate);
    int32_t rc = ph_plan(S->e, S, nq, q_arena, q_offs, depth); if (rc) return rc;
    if (nunions) *nunions = (uint32_t)S->batch->pending.size();
    if (!host_phases() && nq) {     // WordMatcher descriptors + PrepareQuery now: phase 0 is off the collective path (sharded.py search_stream)
        S->batch->pre = std::make_shared<FusedIn>();
        rc = build_fused_inputs(S->e, S, 1, 1, *S->batch->pre); if (rc) return rc;
    }
    return INFX_OK;
}
// ---- sharded planning: the two expensive, index-wide host lookups of a batch — the LD1 expansion of unknown words (plan_tokens) and the
// WordMatcher dictionary / affix lookups (wm_collect), together ~85 % of the host time per query at 10 M documents — are pure functions of
// (index, text) and every rank holds the whole host index.  Rank r therefore computes them for queries [begin, end) of the coming batch only,
// the ranks all-gather the serialised results and import each other's share before phase 0, which then finds every LD1 expansion in the fuzzy
// cache and every descriptor list in the session (infidex_amd/sharded.py: ShardedSearcher._prefetch, on its own process group).
// Blob: u32 nLd1 { u16 len, u16 chars[len], u32 n, i32 members[n] }*  u32 nWm { u16 len, u16 chars[len], u32 nl, {u32 src, u32 len, u64 off}[nl], u32 no, i32 owned[no] }*
int64_t infx_session_prefetch_collect(infx_session* S, uint32_t nq, const uint16_t* q_arena, const uint64_t* q_offs, uint32_t begin, uint32_t end, int32_t depth) {
    if (!S || (nq && (!q_arena || !q_offs)) || begin > end || end > nq) { efail(INFX_EINVAL, "bad arguments"); return -1; }
    infx_engine* e = S->e; const HostIndex& ix = e->ix; const uint32_t n = end - begin;
    // With the dictionaries on the device the two lookups are kernels on every rank's own GPU and sections 1-2 stay empty; section 3 — the
    // plan exchange — is always there: the host work that is left (text preparation, term lookups, the coverage query context) for this rank's slice only.
    const bool hostLookups = !e->devLookups;
    std::vector<std::shared_ptr<infx_session::PlanPre>> pres(n);
    std::vector<std::vector<infx_wm_list>> qL(n); std::vector<std::vector<int32_t>> qO(n);
    parallel_dyn(n, e->threads, 1, [&](int64_t b, int64_t en, int) {
        WmResult wm;
        for (int64_t i = b; i < en; i++) {
            const uint32_t q = begin + (uint32_t)i;
            pres[i] = std::make_shared<infx_session::PlanPre>(); pres[i]->own.reset(new infx_session::OwnPlan); pres[i]->depth = depth;
            infx_session::PlanPre& R = *pres[i]; QueryPlan& P = R.own->plan;
            const u16* rp = (const u16*)q_arena + q_offs[q]; const size_t rl = (size_t)(q_offs[q + 1] - q_offs[q]);
            R.rawHash = raw_hash((const uint16_t*)rp, rl);
            plan_tokens_text(ix, uview(rp, rl), depth, P);
            if (hostLookups) plan_tokens_expand(ix, e->fuzzy, P, false);
            if (!P.blank && !P.unsupported && ix.cfg.enableCoverage) {
                if (hostLookups) wm_descriptors(ix, P.searchText, wm, qL[i], qO[i]);
                R.hasCov = true; R.covErr = prepare_cov_any(ix, P.searchText, R.own->cq, R.own->cql); R.longCov = (bool)R.own->cql;
            }
        }
    });
    std::vector<uint8_t>& blob = S->prefetchBlob; blob.clear(); BlobW W{blob};
    W.put<uint64_t>(index_fingerprint(ix));
    std::map<std::u16string, const FuzzyUnion*> words;          // ordered: the blob is a deterministic function of (index, slice)
    for (auto& R : pres) for (auto& r : R->own->plan.rawTok) if (r.fz) words.emplace(r.text, r.fz.get());
    W.put<uint32_t>((uint32_t)words.size());
    for (auto& kv : words) {
        W.put<uint16_t>((uint16_t)kv.first.size()); W.bytes(kv.first.data(), kv.first.size() * 2);
        W.put<uint32_t>((uint32_t)kv.second->members.size()); W.bytes(kv.second->members.data(), kv.second->members.size() * 4);
    }
    std::map<std::u16string, uint32_t> texts;
    if (hostLookups)
        for (uint32_t i = 0; i < n; i++) { const QueryPlan& P = pres[i]->own->plan; if (!P.blank && !P.unsupported && ix.cfg.enableCoverage && P.searchText.size() <= 0xFFFF) texts.emplace(P.searchText, i); }
    W.put<uint32_t>((uint32_t)texts.size());
    for (auto& kv : texts) {
        const uint32_t i = kv.second;
        W.put<uint16_t>((uint16_t)kv.first.size()); W.bytes(kv.first.data(), kv.first.size() * 2);
        W.put<uint32_t>((uint32_t)qL[i].size());
        for (auto& L : qL[i]) { W.put<uint32_t>(L.src); W.put<uint32_t>(L.len); W.put<uint64_t>(L.off); }
        W.put<uint32_t>((uint32_t)qO[i].size()); W.bytes(qO[i].data(), qO[i].size() * 4);
    }
    // section 3, the plan exchange: u32 begin, end, nq; i32 depth; per query of the slice
    //   (table of n + 1 u32 record offsets first, so that an importer can find a record without parsing the ones before it)
    //   u64 hash of the raw text; u8 flags (1 blank, 2 unsupported, 4 searchText == qtext, 8 tfidfQuery == searchText, 16 coverage query present, 32 .. outside the envelope,
    //   64 .. in the long envelope: infx_cov_query_long)
    //   str qtext; [str searchText]; [str tfidfQuery]; u16 nraw { i32 id; [str text] }*       (str = u32 length + UTF-16 units; unknown words drop their expansion:
    //   the importer looks them up in ITS cache / expands them with the batch, as for its own queries)
    //   coverage query (its text is searchText): i32 status | i32 num_tokens, u16 tok_off[], u16 tok_len[], f32 term_idf[], f32 word_idf[], i32 has_word_idf,
    //   i32 num_fusion_tokens, u16 ftok_off[], u16 ftok_len[], i32 lcs_tolerance
    auto str = [&](const ustr& t) { W.put<uint32_t>((uint32_t)t.size()); W.bytes(t.data(), t.size() * 2); };
    const size_t sec3 = blob.size();
    W.put<uint32_t>(begin); W.put<uint32_t>(end); W.put<uint32_t>(nq); W.put<int32_t>(depth);
    const size_t tab = blob.size(); blob.resize(tab + ((size_t)n + 1) * 4);      // u32 record offsets (n + 1), relative to the first record
    const size_t rec0 = blob.size();
    auto tabput = [&](uint32_t k) { const uint32_t o = (uint32_t)(blob.size() - rec0); std::memcpy(blob.data() + tab + (size_t)k * 4, &o, 4); };
    for (uint32_t i = 0; i < n; i++) {
        tabput(i);
        const infx_session::PlanPre& R = *pres[i]; const QueryPlan& P = R.own->plan;
        const bool sameST = P.searchText == P.qtext, sameTQ = P.tfidfQuery == P.searchText;
        W.put<uint64_t>(R.rawHash);
        W.put<uint8_t>((uint8_t)((P.blank ? 1 : 0) | (P.unsupported ? 2 : 0) | (sameST ? 4 : 0) | (sameTQ ? 8 : 0) | (R.hasCov ? 16 : 0) | (R.covErr ? 32 : 0) | (R.longCov ? 64 : 0)));
        str(P.qtext); if (!sameST) str(P.searchText); if (!sameTQ) str(P.tfidfQuery);
        W.put<uint16_t>((uint16_t)P.rawTok.size());
        for (auto& r : P.rawTok) { W.put<int32_t>(r.id); if (r.id < 0) str(r.text); }
        if (R.hasCov && R.covErr) W.put<int32_t>(R.covErr);
        else if (R.hasCov) {
            auto putcov = [&](const auto& C) {
                const size_t nt = (size_t)C.num_tokens, nf = (size_t)C.num_fusion_tokens;
                W.put<int32_t>(C.num_tokens); W.bytes(C.tok_off, nt * 2); W.bytes(C.tok_len, nt * 2); W.bytes(C.term_idf, nt * 4); W.bytes(C.word_idf, nt * 4);
                W.put<int32_t>(C.has_word_idf); W.put<int32_t>(C.num_fusion_tokens); W.bytes(C.ftok_off, nf * 2); W.bytes(C.ftok_len, nf * 2); W.put<int32_t>(C.lcs_tolerance);
            };
            if (R.longCov) putcov(*R.own->cql); else putcov(R.own->cq);
        }
    }
    tabput(n);
    W.put<uint64_t>(bytes_hash(blob.data() + sec3, blob.size() - sec3));      // the section's checksum: plans steer kernels, a damaged one must not be believed
    // this rank's own slice needs no round trip
    S->planPre.assign(nq, nullptr); S->planPeer.assign(nq, 0);
    for (uint32_t i = 0; i < n; i++) {
        for (auto& r : pres[i]->own->plan.rawTok) { r.fz = nullptr; r.pending = false; }      // phase 0 resolves them against the cache as it stands then
        S->planPre[begin + i] = std::move(pres[i]);
    }
    return (int64_t)blob.size();
}
int64_t infx_session_prefetch_pending(infx_session* S) { return S ? (int64_t)S->wmPre.size() : -1; }
int32_t infx_session_prefetch_blob(infx_session* S, uint8_t* out, int64_t cap) {
    if (!S || !out || cap < (int64_t)S->prefetchBlob.size()) return efail(INFX_EINVAL, "bad arguments");
    std::memcpy(out, S->prefetchBlob.data(), S->prefetchBlob.size()); return INFX_OK;
}
int32_t infx_session_prefetch_import(infx_session* S, const uint8_t* blob, int64_t len) {
    if (!S || !blob || len < 16) return efail(INFX_EINVAL, "bad arguments");
    infx_engine* e = S->e; const HostIndex& ix = e->ix;
    BlobR R{blob, blob + len};
    if (R.get<uint64_t>() != index_fingerprint(ix)) return efail(INFX_EINVAL, "prefetch blob comes from a different index (ranks must index the same corpus with the same build)");
    const uint32_t nw = R.get<uint32_t>();
    for (uint32_t k = 0; k < nw && R.ok; k++) {
        const uint16_t wl = R.get<uint16_t>(); const uint8_t* wp = R.take((size_t)wl * 2);
        const uint32_t nm = R.get<uint32_t>(); const uint8_t* mp = R.take((size_t)nm * 4);
        if (!R.ok) break;
        std::u16string word((size_t)wl, u'\0'); std::memcpy(&word[0], wp, (size_t)wl * 2);
        if (e->fuzzy.get(word)) continue;
        auto nf = std::make_shared<FuzzyUnion>(); nf->members.resize(nm); if (nm) std::memcpy(nf->members.data(), mp, (size_t)nm * 4);
        for (int32_t id : nf->members) if (id < 0 || (size_t)id >= ix.df.size()) return efail(INFX_EINVAL, "prefetch blob: term id out of range (ranks must hold the same index)");
        if (nf->members.empty()) nf->df.store(0);
        e->fuzzy.put(word, nf);
    }
    const uint32_t nt = R.ok ? R.get<uint32_t>() : 0;
    for (uint32_t k = 0; k < nt && R.ok; k++) {
        const uint16_t tl = R.get<uint16_t>(); const uint8_t* tp = R.take((size_t)tl * 2);
        const uint32_t nl = R.get<uint32_t>();
        infx_session::WmPre pre; pre.lists.resize(nl);
        for (uint32_t j = 0; j < nl && R.ok; j++) { pre.lists[j] = infx_wm_list{}; pre.lists[j].src = R.get<uint32_t>(); pre.lists[j].len = R.get<uint32_t>(); pre.lists[j].off = R.get<uint64_t>(); }
        const uint32_t no = R.get<uint32_t>(); const uint8_t* op = R.take((size_t)no * 4);
        if (!R.ok) break;
        pre.owned.resize(no); if (no) std::memcpy(pre.owned.data(), op, (size_t)no * 4);
        for (auto& L : pre.lists) {          // descriptors go straight to the device: reject anything outside the arrays they index
            const uint64_t lim = L.src == 0 ? ix.wmExact.doc.size() : (L.src == 1 ? ix.wmLd1.doc.size() : (L.src == 2 ? (uint64_t)no : 0));
            if (L.src > 2 || L.off > lim || (uint64_t)L.len > lim - L.off) return efail(INFX_EINVAL, "prefetch blob: WordMatcher descriptor out of range");
        }
        for (int32_t id : pre.owned) if (id < 0 || id >= ix.N) return efail(INFX_EINVAL, "prefetch blob: affix document id out of range");
        std::u16string text((size_t)tl, u'\0'); std::memcpy(&text[0], tp, (size_t)tl * 2);
        S->wmPre.emplace(std::move(text), std::move(pre));
    }
    if (!R.ok) return efail(INFX_EINVAL, "prefetch blob truncated");
    // section 3: the peer's slice of the batch's plans
    if ((size_t)(R.e - R.p) < 24 || [&] { uint64_t want; std::memcpy(&want, R.e - 8, 8); return want != bytes_hash(R.p, (size_t)(R.e - R.p) - 8); }())
        return efail(INFX_EINVAL, "prefetch blob: plan section damaged (checksum)");
    R.e -= 8;
    const uint32_t begin = R.get<uint32_t>(), end = R.get<uint32_t>(), bnq = R.get<uint32_t>(); const int32_t depth = R.get<int32_t>();
    if (!R.ok || begin > end || end > bnq) return efail(INFX_EINVAL, "prefetch blob: plan section truncated or its slice is out of range");
    const uint32_t n = end - begin;
    const uint8_t* offp = R.take(((size_t)n + 1) * 4);
    if (!offp) return efail(INFX_EINVAL, "prefetch blob truncated");
    // the records stay in a copy of the section; each query's entry points at its record, which phase 0 parses on its planner threads
    auto slab = std::make_shared<infx_session::PlanSlab>();
    slab->bytes.assign(R.p, R.e); slab->pre.resize(n);
    const size_t total = slab->bytes.size();
    std::vector<uint32_t> offs((size_t)n + 1); std::memcpy(offs.data(), offp, ((size_t)n + 1) * 4);
    if (offs[0] != 0 || offs[n] != total) return efail(INFX_EINVAL, "prefetch blob: plan record table does not match the section");
    for (uint32_t k = 0; k < n; k++) {
        if (offs[k + 1] < offs[k] || offs[k + 1] > total || offs[k + 1] - offs[k] < 9) return efail(INFX_EINVAL, "prefetch blob: plan record table does not match the section");
        infx_session::PlanPre& E = slab->pre[k];
        E.rec = slab->bytes.data() + offs[k]; E.recLen = offs[k + 1] - offs[k]; E.depth = depth;
        std::memcpy(&E.rawHash, E.rec, 8);
    }
    if (S->planPre.size() != bnq) { S->planPre.assign(bnq, nullptr); S->planPeer.assign(bnq, 0); }
    for (uint32_t k = 0; k < n; k++) { S->planPre[begin + k] = std::shared_ptr<infx_session::PlanPre>(slab, &slab->pre[k]); S->planPeer[begin + k] = 1; }
    return INFX_OK;
}
// Plan exchange, observed: out2 = {queries of the last phase 0 whose token-level plan came through infx_session_prefetch_* (own slice + imported), of them imported from peers}
int32_t infx_session_plan_exchange_stats(infx_session* S, uint32_t* out2) {
    if (!S || !out2) return efail(INFX_EINVAL, "null");
    out2[0] = S->planFromExchange; out2[1] = S->planFromPeers; return INFX_OK;
}
// Parity tooling (no device needed): one 64-bit digest per query of everything the plan exchange carries — flags, the three texts, the raw tokens, the coverage
// query context byte for byte — taken from the session's pending exchange entries where they exist and match the text, computed here otherwise; *from_exchange
// counts the former.  Equal digests with and without an exchange = the exchange changes nothing.  Does not consume the entries.
int32_t infx_session_plan_digest(infx_session* S, uint32_t nq, const uint16_t* q_arena, const uint64_t* q_offs, int32_t depth, uint64_t* out, uint32_t* from_exchange) {
    if (!S || !out || (nq && (!q_arena || !q_offs))) return efail(INFX_EINVAL, "bad arguments");
    const HostIndex& ix = S->e->ix; uint32_t used = 0;
    for (uint32_t i = 0; i < nq; i++) {
        const u16* rp = (const u16*)q_arena + q_offs[i]; const size_t rl = (size_t)(q_offs[i + 1] - q_offs[i]);
        infx_session::PlanPre local; local.own.reset(new infx_session::OwnPlan); const infx_session::PlanPre* R = S->planPre.size() == nq ? S->planPre[i].get() : nullptr;
        if (R && R->depth == depth && R->rawHash == raw_hash((const uint16_t*)rp, rl)) {
            used++;
            if (R->rec) {      // a peer's record: parsed here as phase 0 would
                const char* why = parse_plan_record(ix, R->rec, R->recLen, depth, local.own->plan, local.hasCov, local.covErr, local.covOff, local.longCov);
                if (!why && local.hasCov && !local.covErr && local.longCov) { local.own->cql.reset(new infx_cov_query_long); why = parse_cov_record_long(local.own->plan.searchText, R->rec, R->recLen, local.covOff, *local.own->cql); }
                else if (!why && local.hasCov && !local.covErr) why = parse_cov_record(local.own->plan.searchText, R->rec, R->recLen, local.covOff, local.own->cq);
                if (why) return efail(INFX_EINVAL, std::string("exchanged plan record: ") + why);
                R = &local;
            }
        } else {
            plan_tokens_text(ix, uview(rp, rl), depth, local.own->plan);
            if (!local.own->plan.blank && !local.own->plan.unsupported && ix.cfg.enableCoverage) { local.hasCov = true; local.covErr = prepare_cov_any(ix, local.own->plan.searchText, local.own->cq, local.own->cql); local.longCov = (bool)local.own->cql; }
            R = &local;
        }
        uint64_t h = 1469598103934665603ull;
        auto mix = [&](const void* p, size_t n) { const uint8_t* b = (const uint8_t*)p; for (size_t k = 0; k < n; k++) { h ^= b[k]; h *= 1099511628211ull; } const uint64_t nn = n; for (int k = 0; k < 8; k++) { h ^= (nn >> (8 * k)) & 0xFF; h *= 1099511628211ull; } };
        const QueryPlan& P = R->own->plan; const uint8_t fl = (uint8_t)((P.blank ? 1 : 0) | (P.unsupported ? 2 : 0) | (R->hasCov ? 4 : 0)); const int32_t d = P.depth;
        mix(&fl, 1); mix(&d, 4); mix(P.qtext.data(), P.qtext.size() * 2); mix(P.searchText.data(), P.searchText.size() * 2); mix(P.tfidfQuery.data(), P.tfidfQuery.size() * 2);
        for (auto& r : P.rawTok) { mix(&r.id, 4); mix(r.text.data(), r.text.size() * 2); }
        if (R->hasCov) { mix(&R->covErr, 4); const uint8_t lg = R->longCov ? 1 : 0; mix(&lg, 1); if (!R->covErr && R->longCov) mix(R->own->cql.get(), sizeof(infx_cov_query_long)); else if (!R->covErr) mix(&R->own->cq, sizeof R->own->cq); }
        out[i] = h;
    }
    if (from_exchange) *from_exchange = used;
    return INFX_OK;
}
int32_t infx_session_union_counts(infx_session* S, uint32_t* counts) {   // this shard's |union| of every pending fuzzy virtual term
    if (!S || !counts) return efail(INFX_EINVAL, "null");
    std::memcpy(counts, S->batch->pendingCounts.data(), S->batch->pendingCounts.size() * 4); return INFX_OK;
}
int32_t infx_session_phase1(infx_session* S, const uint32_t* global_union_counts, uint32_t* ndev) {
    if (!S) return efail(INFX_EINVAL, "null session");
    static const uint32_t zero = 0;
    int32_t rc = ph_plan_finish(S->e, S, global_union_counts ? global_union_counts : &zero); if (rc) return rc;
    rc = ph_accumulate(S->e, S); if (rc) return rc;
    if (ndev) *ndev = S->batch->nd;
    return INFX_OK;
}
// phase 1 with the class histograms written straight into caller memory on the host OR the device (nq x INFX_NCLASS uint32, the first ndev rows
// are used): with a device tensor the count all-reduce (Exchange 1) runs in place on it and infx_session_phase2x reads it back from HBM.
int32_t infx_session_phase1x(infx_session* S, const uint32_t* global_union_counts, void* counts, uint32_t* ndev) {
    if (!S || !counts) return efail(INFX_EINVAL, "null");
    static const uint32_t zero = 0;
    int32_t rc = ph_plan_finish(S->e, S, global_union_counts ? global_union_counts : &zero); if (rc) return rc;
    Batch& B = *S->batch;
    S->msAcc = S->msSel = S->msCov = S->msPrep2 = S->msFin = 0; S->algBytes = 0;
    if (B.nd) {
        rc = infx_stage1_accumulate(S->stream, B.nd, B.dq.data(), (uint32_t)B.dterms.size(), B.dterms.data(), (uint32_t)B.extra.size(), B.extra.data(), (infx_counts*)counts);
        if (rc) { g_eerr = infx_last_error(); return rc; }
    }
    if (ndev) *ndev = B.nd;
    return INFX_OK;
}
int32_t infx_session_counts(infx_session* S, uint32_t* counts) {   // nd x INFX_NCLASS, this shard
    if (!S || !counts) return efail(INFX_EINVAL, "null");
    std::memcpy(counts, S->batch->counts.data(), S->batch->counts.size() * sizeof(infx_counts)); return INFX_OK;
}
int32_t infx_session_phase2(infx_session* S, const uint32_t* global_counts, infx_hit* hits, uint32_t* hitcounts) {
    if (!S || !global_counts) return efail(INFX_EINVAL, "null");
    if (host_phases()) {      // the original host-side candidate assembly / final ordering
        int32_t rc = ph_select(S->e, S, (const infx_counts*)global_counts); if (rc) return rc;
        if (hits) std::memcpy(hits, S->lastHits.data(), S->lastHits.size() * sizeof(infx_hit));
        if (hitcounts) std::memcpy(hitcounts, S->lastHitCount.data(), S->lastHitCount.size() * 4);
        return INFX_OK;
    }
    Batch& B = *S->batch;
    S->lastHits.assign((size_t)B.nd * B.depth, infx_hit{0, 0.f}); S->lastHitCount.assign(B.nd, 0); S->lastStride = B.depth;
    if (B.nd) {
        int32_t rc = infx_shard_select(S->stream, B.nd, (const infx_counts*)global_counts, B.depth, S->lastHits.data(), S->lastHitCount.data(), nullptr);
        if (rc) { g_eerr = infx_last_error(); return rc; }
        infx_last_timings(S->stream, &S->msAcc, &S->msSel, nullptr);
        infx_last_alg_bytes(S->stream, &S->streamedBytes); infx_last_candidates(S->stream, &S->s1Candidates); infx_last_exact_replays(S->stream, &S->exactReplays); infx_last_replay_stats(S->stream, &S->msReplay, S->flagWhy);
        uint64_t ab = 0, nh = 0;
        for (auto& t : B.dterms) ab += t.term_id >= 0 ? (uint64_t)S->e->shardTermLen(t.term_id) * 5ull : (uint64_t)t.extra_len * 4ull;
        for (uint32_t c : S->lastHitCount) nh += c;
        S->algBytes = ab + S->s1Candidates * 4ull + nh * 12ull;
    }
    if (hits) std::memcpy(hits, S->lastHits.data(), S->lastHits.size() * sizeof(infx_hit));
    if (hitcounts) std::memcpy(hitcounts, S->lastHitCount.data(), S->lastHitCount.size() * 4);
    B.t2 = now_ms();
    return INFX_OK;
}
// ---- phase 2 with the exact cut across shards (infx_shard_replay_*) ----
static void take_stage1_stats(infx_session* S, bool withHits) {
    Batch& B = *S->batch;
    infx_last_timings(S->stream, &S->msAcc, &S->msSel, nullptr);
    infx_last_alg_bytes(S->stream, &S->streamedBytes); infx_last_candidates(S->stream, &S->s1Candidates);
    uint64_t ab = 0;
    for (auto& t : B.dterms) ab += t.term_id >= 0 ? (uint64_t)S->e->shardTermLen(t.term_id) * 5ull : (uint64_t)t.extra_len * 4ull;
    S->algBytes = ab + S->s1Candidates * 4ull + (withHits ? (uint64_t)B.nd * B.depth * 12ull : 0ull);
}
int32_t infx_session_phase2a(infx_session* S, const void* global_counts, void* hits, void* hitcounts, void* next) {
    if (!S || !global_counts || !hits || !hitcounts || !next) return efail(INFX_EINVAL, "null");
    Batch& B = *S->batch;
    int32_t rc = infx_shard_select(S->stream, B.nd, (const infx_counts*)global_counts, B.depth, (infx_hit*)hits, (uint32_t*)hitcounts, (float*)next);     // nd == 0: resets the replay state
    if (rc) { g_eerr = infx_last_error(); return rc; }
    if (B.nd) take_stage1_stats(S, true);
    return INFX_OK;
}
int32_t infx_session_phase2b(infx_session* S, int32_t W, const void* all_hits, const void* all_hitcounts, const void* all_next, uint64_t* blob_bytes) {
    if (!S || W < 1 || !blob_bytes) return efail(INFX_EINVAL, "null");
    Batch& B = *S->batch;
    int32_t rc = infx_shard_replay_local(S->stream, W, B.nd, (const infx_hit*)all_hits, (const uint32_t*)all_hitcounts, (const float*)all_next, B.depth, blob_bytes);
    if (rc) { g_eerr = infx_last_error(); return rc; }
    return INFX_OK;
}
int32_t infx_session_phase2b_blob(infx_session* S, void* dst, uint64_t padded) {
    if (!S || !dst) return efail(INFX_EINVAL, "null");
    int32_t rc = infx_shard_replay_blob(S->stream, dst, padded);
    if (rc) { g_eerr = infx_last_error(); return rc; }
    return INFX_OK;
}
int32_t infx_session_phase2c(infx_session* S, int32_t W, const void* all_blobs, uint64_t padded, void* hits, void* hitcounts) {
    if (!S || W < 1 || !hits || !hitcounts) return efail(INFX_EINVAL, "null");
    Batch& B = *S->batch;
    if (B.nd) {
        int32_t rc = infx_shard_replay_merge(S->stream, W, B.nd, all_blobs, padded, B.depth, (infx_hit*)hits, (uint32_t*)hitcounts);
        if (rc) { g_eerr = infx_last_error(); return rc; }
        infx_last_exact_replays(S->stream, &S->exactReplays); infx_last_replay_stats(S->stream, &S->msReplay, S->flagWhy);
    }
    B.t2 = now_ms();
    return INFX_OK;
}
int32_t infx_session_phase2d(infx_session* S, const uint32_t* need, void* state) {
    if (!S || !need || !state) return efail(INFX_EINVAL, "null");
    Batch& B = *S->batch;
    int32_t rc = infx_shard_replay_chain(S->stream, B.nd, need, B.depth, state);
    if (rc) { g_eerr = infx_last_error(); return rc; }
    return INFX_OK;
}
// ---- native driver of the sharded phases (infidex_engine.h) ---------------------------------------------------------------------------------------------
namespace {
int32_t rccl_allreduce(void* ctx, void* buf, uint64_t count, void* /*stream*/) { return infx_comm_allreduce_sum_u32((infx_stream*)ctx, buf, count); }
int32_t rccl_allgather(void* ctx, const void* send, void* recv, uint64_t bytes, void* /*stream*/) { return infx_comm_allgather((infx_stream*)ctx, send, recv, bytes); }
// exchange buffers of one batch: HBM scratch of the session's stream (RCCL) or host vectors (other transports)
struct XBufs {
    infx_session* S; bool dev; std::vector<std::vector<uint8_t>> host; int slot = 0;
    XBufs(infx_session* s, bool d) : S(s), dev(d) { host.reserve(16); }
    int32_t get(size_t bytes, void** out, bool zero) {
        bytes = std::max<size_t>(bytes, 16);
        if (dev) { int32_t rc = infx_stream_scratch(S->stream, slot++, bytes, out); if (rc) return rc; return zero ? infx_stream_fill0(S->stream, *out, bytes) : INFX_OK; }
        host.emplace_back(bytes, (uint8_t)0); *out = host.back().data(); return INFX_OK;
    }
};
}
int32_t infx_engine_rccl_unique_id(void* id128) { int32_t rc = infx_rccl_unique_id(id128); if (rc) g_eerr = infx_last_error(); return rc; }
int32_t infx_engine_comm_rccl(infx_engine* e, const void* id128, infx_comm* out) {
    if (!e || !id128 || !out) return efail(INFX_EINVAL, "null argument");
    if (!e->dev || !e->indexed) return efail(INFX_EINVAL, "the RCCL communicator is created on an indexed engine with a GPU");
    int32_t rc = infx_set_shard_comm(e->dev, id128);
    if (rc) { g_eerr = infx_last_error(); return rc; }
    std::memset(out, 0, sizeof *out);
    out->ctx = nullptr;                      // the session's stream is supplied per call (the collective runs on ITS HIP stream)
    out->rank = e->rank; out->nranks = e->nranks; out->device_buffers = 1;
    out->allreduce_sum_u32 = rccl_allreduce; out->allgather = rccl_allgather;
    return INFX_OK;
}
int32_t infx_session_comm_rccl(infx_session* S, const void* id128, infx_comm* out) {
    if (!S || !id128 || !out) return efail(INFX_EINVAL, "null argument");
    if (!S->stream) return efail(INFX_EINVAL, "the session has no GPU stream");
    int32_t rc = infx_stream_comm(S->stream, id128);
    if (rc) { g_eerr = infx_last_error(); return rc; }
    std::memset(out, 0, sizeof *out);
    out->rank = S->e->rank; out->nranks = S->e->nranks; out->device_buffers = 1;
    out->allreduce_sum_u32 = rccl_allreduce; out->allgather = rccl_allgather;
    return INFX_OK;
}
int32_t infx_session_sharded_finish(infx_session* S, const infx_comm* comm, int32_t max_results, int32_t enable_coverage,
                                    int64_t* out_keys, float* out_scores, uint8_t* out_ties, uint32_t* out_counts, uint32_t* out_flags) {
    if (!S || !comm || !comm->allreduce_sum_u32 || !comm->allgather || !out_keys || !out_scores || !out_counts || max_results < 1) return efail(INFX_EINVAL, "bad arguments");
    infx_engine* e = S->e; Batch& B = *S->batch;
    if (comm->nranks != e->nranks || comm->rank != e->rank) return efail(INFX_EINVAL, "communicator and engine disagree about the shard layout");
    const int W = comm->nranks; const bool dev = comm->device_buffers != 0;
    void* const cctx = comm->ctx ? comm->ctx : (void*)S->stream;       // the in-library RCCL ops run on the session's stream
    void* hs = nullptr;                                                // what a caller-supplied op with device buffers orders itself on: the session's hipStream_t
    if (dev && infx_stream_native(S->stream, &hs) != INFX_OK) return efail(INFX_EINVAL, "device exchange buffers need a session with a GPU stream");
    auto chk = [&](int32_t rc) { if (rc && g_eerr.empty()) g_eerr = infx_last_error(); return rc; };
    // An error return leaves the rank's collective ring: a session that stays a member but issues no further collective would block every peer
    // session of this rank in CollSeq::enter() for ever.  (The peer RANKS then see this session's collectives missing and time out: INFX_COMM_TIMEOUT_S.)
    struct RetireOnError { infx_engine* e; infx_session* S; bool armed = true; ~RetireOnError() { if (armed) e->collSeq.retire(S); } } onError{e, S};
#define XCHK(x) do { int32_t rc_ = chk(x); if (rc_) return rc_; } while (0)
    // one turn of the rank's collective ring per collective (CollSeq above); INFX_COLL_ORDER=0 switches the ordering off
    static const bool orderedEnv = [] { const char* v = getenv("INFX_COLL_ORDER"); return !(v && v[0] == '0'); }();
    const bool ordered = orderedEnv && comm->nranks > 1;      // a single rank has no peer to fall out of step with (measured cost of the lock-step at W = 1: 12 %)
    struct Turn { CollSeq& q; const infx_session* S; bool in; Turn(CollSeq& x, const infx_session* s_, bool on) : q(x), S(s_), in(on && x.enter(s_)) {} ~Turn() { if (in) q.leave(S); } };
    auto all_reduce = [&](void* buf, uint64_t count) { Turn t(e->collSeq, S, ordered); S->collCalls[0]++; S->collBytes[0] += count * 4; return comm->allreduce_sum_u32(cctx, buf, count, hs); };
    auto all_gather = [&](const void* send, void* recv, uint64_t bytes) { Turn t(e->collSeq, S, ordered); S->collCalls[1]++; S->collBytes[1] += bytes; return comm->allgather(cctx, send, recv, bytes, hs); };
    const uint32_t nq = B.nq; const int depth = B.depth;
    if (W > 1 && depth != e->ix.cfg.maxDepth) return efail(INFX_EINVAL, "document shards search with CoverageDepth == the engine's max_depth (the chained replay exchanges heaps of max_depth entries)");
    XBufs X(S, dev);
    // Exchange 1b: global df of the batch's new fuzzy unions (the host needs the values: idf is computed there with the reference's logf)
    std::vector<uint32_t> guc(B.pendingCounts);
    if (!guc.empty()) {
        if (dev) {
            void* d = nullptr; XCHK(X.get(guc.size() * 4, &d, false));
            XCHK(infx_stream_copy(S->stream, d, guc.data(), guc.size() * 4));
            XCHK(all_reduce(d, guc.size()));
            XCHK(infx_stream_copy(S->stream, guc.data(), d, guc.size() * 4)); XCHK(infx_stream_wait(S->stream));
        } else XCHK(all_reduce(guc.data(), guc.size()));
    }
    static const uint32_t zero = 0;
    // phase 1 + Exchange 1: class histograms (tier decisions need GLOBAL cardinalities, Q11)
    void* counts = nullptr; XCHK(X.get((size_t)std::max<uint32_t>(nq, 1) * INFX_NCLASS * 4, &counts, true));
    uint32_t nd = 0; XCHK(infx_session_phase1x(S, guc.empty() ? &zero : guc.data(), counts, &nd));
    XCHK(all_reduce(counts, (uint64_t)std::max<uint32_t>(nq, 1) * INFX_NCLASS));
    // phase 2a + Exchange 2a: first-pass lists, counts, best score left out
    const size_t ndp = std::max<uint32_t>(nd, 1), hitB = ndp * depth * sizeof(infx_hit);
    // the three pieces a rank contributes (lists | counts | best scores left out) are one packed block: ONE all-gather, unpacked into the per-piece arrays
    void *pack = nullptr, *apack = nullptr, *ah = nullptr, *ac = nullptr, *an = nullptr;
    const size_t packB = hitB + 2 * ndp * 4;
    XCHK(X.get(packB, &pack, true)); XCHK(X.get(packB * W, &apack, false));
    void* hits = pack; void* hc = (char*)pack + hitB; void* nxt = (char*)pack + hitB + ndp * 4;
    XCHK(X.get(hitB * W, &ah, false)); XCHK(X.get(ndp * 4 * W, &ac, false)); XCHK(X.get(ndp * 4 * W, &an, false));
    XCHK(infx_session_phase2a(S, counts, hits, hc, nxt));
    XCHK(all_gather(pack, apack, packB));
    { const uint64_t pb[3] = {hitB, ndp * 4, ndp * 4}; void* const ds3[3] = {ah, ac, an}; XCHK(infx_stream_unpack(S->stream, apack, packB, W, 3, pb, ds3)); }
    // phase 2b + Exchange 2c: this shard's part of the exact replay, packed; padded to the largest blob of the world
    uint64_t blobBytes = 0; XCHK(infx_session_phase2b(S, W, ah, ac, an, &blobBytes));
    uint64_t pad = blobBytes;
    {   // max over ranks through the sum-all-reduce the communicator has: one slot per rank
        std::vector<uint32_t> sz((size_t)W, 0u); sz[comm->rank] = (uint32_t)((blobBytes + 15) >> 4);
        if (dev) {
            void* d = nullptr; XCHK(X.get(sz.size() * 4, &d, false));
            XCHK(infx_stream_copy(S->stream, d, sz.data(), sz.size() * 4));
            XCHK(all_reduce(d, sz.size()));
            XCHK(infx_stream_copy(S->stream, sz.data(), d, sz.size() * 4)); XCHK(infx_stream_wait(S->stream));
        } else XCHK(all_reduce(sz.data(), sz.size()));
        pad = 16ull * *std::max_element(sz.begin(), sz.end());
    }
    void *blob = nullptr, *ab = nullptr; XCHK(X.get(pad, &blob, false)); XCHK(X.get(pad * W, &ab, false));
    XCHK(infx_session_phase2b_blob(S, blob, pad));
    XCHK(all_gather(blob, ab, pad));
    // phase 2c + Exchange 2b: owner-side heap; the all-gather of the per-rank final lists
    XCHK(infx_session_phase2c(S, W, ab, pad, hits, hc));
    XCHK(all_gather(pack, apack, hitB + ndp * 4));      // lists | counts, one collective
    { const uint64_t pb[2] = {hitB, ndp * 4}; void* const ds2[2] = {ah, ac}; XCHK(infx_stream_unpack(S->stream, apack, hitB + ndp * 4, W, 2, pb, ds2)); }
    // queries the parallel replay could not certify (rare): the literal sequential replay, shard after shard
    std::vector<uint32_t> fc((size_t)W * ndp);
    XCHK(infx_stream_copy(S->stream, fc.data(), ac, fc.size() * 4)); XCHK(infx_stream_wait(S->stream));
    std::vector<uint32_t> need(ndp, 0u); bool anyNeed = false;
    for (int w = 0; w < W; w++) for (uint32_t q = 0; q < nd; q++) if (fc[(size_t)w * ndp + q] == 0xFFFFFFFFu) { need[q] = 1; anyNeed = true; }
    if (anyNeed) {
        const size_t words = ndp * (2 + 2 * (size_t)depth);
        std::vector<uint32_t> state(words, 0u), all(words * W);
        void *ds = nullptr, *da = nullptr;
        if (dev) { XCHK(X.get(words * 4, &ds, false)); XCHK(X.get(words * 4 * W, &da, false)); }
        for (int r = 0; r < W; r++) {
            if (r == comm->rank) XCHK(infx_session_phase2d(S, need.data(), state.data()));
            if (dev) {
                XCHK(infx_stream_copy(S->stream, ds, state.data(), words * 4)); XCHK(all_gather(ds, da, words * 4));
                XCHK(infx_stream_copy(S->stream, all.data(), da, words * 4 * W)); XCHK(infx_stream_wait(S->stream));
            } else XCHK(all_gather(state.data(), all.data(), words * 4));
            std::memcpy(state.data(), all.data() + (size_t)r * words, words * 4);          // rank r's continuation is the state of record
        }
        std::vector<infx_hit> fh((size_t)W * ndp * depth);
        XCHK(infx_stream_copy(S->stream, fh.data(), ah, fh.size() * sizeof(infx_hit))); XCHK(infx_stream_wait(S->stream));
        for (uint32_t q = 0; q < nd; q++) if (need[q]) {
            const uint32_t* st = state.data() + (size_t)q * (2 + 2 * (size_t)depth); const uint32_t n = st[0];
            for (int w = 0; w < W; w++) { fc[(size_t)w * ndp + q] = 0; std::memset(fh.data() + ((size_t)w * ndp + q) * depth, 0, (size_t)depth * sizeof(infx_hit)); }
            for (uint32_t i = 0; i < n; i++) { infx_hit h; h.doc = (int32_t)st[2 + i]; std::memcpy(&h.score, &st[2 + depth + i], 4); fh[(size_t)q * depth + i] = h; }
            fc[q] = n;
        }
        XCHK(infx_stream_copy(S->stream, ah, fh.data(), fh.size() * sizeof(infx_hit))); XCHK(infx_stream_copy(S->stream, ac, fc.data(), fc.size() * 4));
        if (dev) XCHK(infx_stream_wait(S->stream));
    }
    // phase 3 + the all-reduce of the disjoint Stage-2 rows + phase 4
    void* outs = nullptr; XCHK(X.get((size_t)std::max<uint32_t>(nq, 1) * 2 * depth * sizeof(infx_cov_out), &outs, true));
    XCHK(infx_session_phase3x(S, W, ah, ac, max_results, enable_coverage, outs));
    XCHK(all_reduce(outs, (uint64_t)std::max<uint32_t>(nq, 1) * 2 * depth * 3));
    XCHK(infx_session_phase4(S, (const int32_t*)outs, out_keys, out_scores, out_ties, out_counts, out_flags));
#undef XCHK
    onError.armed = false;
    return INFX_OK;
}

int32_t infx_engine_coll_ring(infx_engine* e, uint32_t n, infx_session* const* sessions) {
    if (!e || (n && !sessions)) return efail(INFX_EINVAL, "null argument");
    for (uint32_t i = 0; i < n; i++) if (!sessions[i] || sessions[i]->e != e) return efail(INFX_EINVAL, "a ring session belongs to another engine");
    e->collSeq.set_ring(sessions, n);
    return INFX_OK;
}
int32_t infx_session_coll_retire(infx_session* S) { if (!S || !S->e) return efail(INFX_EINVAL, "null session"); S->e->collSeq.retire(S); return INFX_OK; }
int32_t infx_session_coll_stats(infx_session* S, uint64_t* out4) {      // all-reduce calls, all-gather calls, all-reduce bytes, all-gather bytes (cumulative)
    if (!S || !out4) return efail(INFX_EINVAL, "null argument");
    out4[0] = S->collCalls[0]; out4[1] = S->collCalls[1]; out4[2] = S->collBytes[0]; out4[3] = S->collBytes[1];
    return INFX_OK;
}
int32_t infx_session_phase3(infx_session* S, int32_t W, const infx_hit* all_hits, const uint32_t* all_counts, int32_t max_results, int32_t enable_coverage, uint64_t* ncand) {
    if (!S || W < 1 || max_results < 1) return efail(INFX_EINVAL, "bad arguments");
    { int32_t rc = query_parts_check(S, S->batch->nq, max_results); if (rc) return rc; }
    if (host_phases()) {
        int32_t rc = ph_stage2(S->e, S, W, all_hits, all_counts, max_results, enable_coverage); if (rc) return rc;
        if (ncand) *ncand = S->lastCands.size();
        return INFX_OK;
    }
    infx_engine* e = S->e; Batch& B = *S->batch;
    B.maxResults = max_results;
    std::shared_ptr<FusedIn> FIp; int32_t rc = fused_inputs_for_phase3(e, S, max_results, enable_coverage, FIp); if (rc) return rc;
    FusedIn& FI = *FIp;
    B.t3 = now_ms();
    S->lastOuts.assign((size_t)B.nq * 2 * B.depth, infx_cov_out{});
    if (B.nq) {
        rc = stage_long_queries(S, FI); if (rc) return rc;
        rc = stage_coverage_setup(S, B.nq, true); if (rc) return rc;
        rc = infx_shard_stage2(S->stream, W, B.nd, all_hits, all_counts, B.nq, FI.fq.data(), FI.cq.data(), (uint32_t)FI.lists.size(), FI.lists.data(),
                               (uint32_t)FI.owned.size(), FI.owned.data(), B.depth, max_results, 0, S->lastOuts.data());
        if (rc) { g_eerr = infx_last_error(); return rc; }
        float ms5[5] = {0, 0, 0, 0, 0}; infx_last_fused_timings(S->stream, ms5); S->msPrep2 = ms5[2]; S->msCov = ms5[3];
        infx_last_fused_stats(S->stream, nullptr, &S->s2Candidates, &S->s2TextBytes);
    }
    if (ncand) *ncand = S->lastOuts.size();
    B.t4 = now_ms();
    return INFX_OK;
}
// Variants whose exchange buffers are caller memory on the host OR the device (e.g. the tensors an RCCL collective works on):
// nothing is staged through the session's host vectors.
int32_t infx_session_phase2x(infx_session* S, const uint32_t* global_counts, void* hits, void* hitcounts) {
    if (!S || !global_counts || !hits || !hitcounts) return efail(INFX_EINVAL, "null");
    Batch& B = *S->batch;
    if (B.nd) {
        int32_t rc = infx_shard_select(S->stream, B.nd, (const infx_counts*)global_counts, B.depth, (infx_hit*)hits, (uint32_t*)hitcounts, nullptr);
        if (rc) { g_eerr = infx_last_error(); return rc; }
        infx_last_timings(S->stream, &S->msAcc, &S->msSel, nullptr);
        infx_last_alg_bytes(S->stream, &S->streamedBytes); infx_last_candidates(S->stream, &S->s1Candidates); infx_last_exact_replays(S->stream, &S->exactReplays); infx_last_replay_stats(S->stream, &S->msReplay, S->flagWhy);
        uint64_t ab = 0;
        for (auto& t : B.dterms) ab += t.term_id >= 0 ? (uint64_t)S->e->shardTermLen(t.term_id) * 5ull : (uint64_t)t.extra_len * 4ull;
        S->algBytes = ab + S->s1Candidates * 4ull + (uint64_t)B.nd * B.depth * 12ull;
    }
    B.t2 = now_ms();
    return INFX_OK;
}
int32_t infx_session_phase3x(infx_session* S, int32_t W, const void* all_hits, const void* all_counts, int32_t max_results, int32_t enable_coverage, void* outs) {
    if (!S || W < 1 || max_results < 1 || !outs) return efail(INFX_EINVAL, "bad arguments");
    { int32_t rc = query_parts_check(S, S->batch->nq, max_results); if (rc) return rc; }
    infx_engine* e = S->e; Batch& B = *S->batch;
    B.maxResults = max_results;
    std::shared_ptr<FusedIn> FIp; int32_t rc = fused_inputs_for_phase3(e, S, max_results, enable_coverage, FIp); if (rc) return rc;
    FusedIn& FI = *FIp;
    B.t3 = now_ms();
    if (B.nq) {
        rc = stage_long_queries(S, FI); if (rc) return rc;
        rc = stage_coverage_setup(S, B.nq, true); if (rc) return rc;
        rc = infx_shard_stage2(S->stream, W, B.nd, (const infx_hit*)all_hits, (const uint32_t*)all_counts, B.nq, FI.fq.data(), FI.cq.data(), (uint32_t)FI.lists.size(), FI.lists.data(),
                               (uint32_t)FI.owned.size(), FI.owned.data(), B.depth, max_results, 0, (infx_cov_out*)outs);
        if (rc) { g_eerr = infx_last_error(); return rc; }
        float ms5[5] = {0, 0, 0, 0, 0}; infx_last_fused_timings(S->stream, ms5); S->msPrep2 = ms5[2]; S->msCov = ms5[3];
        infx_last_fused_stats(S->stream, nullptr, &S->s2Candidates, &S->s2TextBytes);
    }
    B.t4 = now_ms();
    return INFX_OK;
}
int32_t infx_session_outs(infx_session* S, int32_t* outs3) {   // ncand x 3 int32 words; zeros for candidates another shard owns
    if (!S || !outs3) return efail(INFX_EINVAL, "null");
    static_assert(sizeof(infx_cov_out) == 12, "infx_cov_out is exchanged as 3 int32 words");
    std::memcpy(outs3, S->lastOuts.data(), S->lastOuts.size() * sizeof(infx_cov_out)); return INFX_OK;
}
int32_t infx_session_phase4(infx_session* S, const int32_t* merged_outs3, int64_t* out_keys, float* out_scores, uint8_t* out_ties, uint32_t* out_counts, uint32_t* out_flags) {
    if (!S || !merged_outs3 || !out_keys || !out_scores || !out_counts) return efail(INFX_EINVAL, "null");
    if (host_phases()) {
        int32_t rc = ph_finalize(S->e, S, (const infx_cov_out*)merged_outs3, out_keys, out_scores, out_ties, out_counts, out_flags);
        const int32_t rc2 = query_parts_finish(S, out_counts, out_flags, rc == INFX_OK);
        return rc ? rc : rc2;
    }
    Batch& B = *S->batch;
    if (B.nq) {
        int32_t rc = infx_shard_finalize(S->stream, B.nq, (const infx_cov_out*)merged_outs3, B.depth, B.maxResults, out_keys, out_scores, out_ties, out_counts, out_flags);
        if (rc) g_eerr = infx_last_error();
        const int32_t rc2 = query_parts_finish(S, out_counts, out_flags, rc == INFX_OK);
        if (rc || rc2) return rc ? rc : rc2;
        float ms5[5] = {0, 0, 0, 0, 0}; infx_last_fused_timings(S->stream, ms5); S->msFin = ms5[4];
    }
    double t5 = now_ms();
    S->tPrep1 = B.t1 - B.t0; S->tStage1 = B.t2 - B.t1; S->tPrep2 = B.t3 - B.t2; S->tStage2 = B.t4 - B.t3; S->tPost = t5 - B.t4;
    return INFX_OK;
}
int32_t infx_engine_default_session(infx_engine* e, infx_session** out) { if (!e || !out) return INFX_EINVAL; *out = e->def; return INFX_OK; }

int32_t infx_engine_session_last_timings(infx_session* S, double* host_ms5, float* kernel_ms3, uint64_t* alg_bytes3) {
    if (!S) return efail(INFX_EINVAL, "null");
    if (host_ms5) { host_ms5[0] = S->tPrep1; host_ms5[1] = S->tStage1; host_ms5[2] = S->tPrep2; host_ms5[3] = S->tStage2; host_ms5[4] = S->tPost; }
    if (kernel_ms3) resolve_kernel_times(S);
    if (kernel_ms3) { kernel_ms3[0] = S->msAcc; kernel_ms3[1] = S->msSel; kernel_ms3[2] = S->msCov; kernel_ms3[3] = S->msPrep2; kernel_ms3[4] = S->msFin; }
    if (alg_bytes3) { alg_bytes3[0] = S->algBytes; alg_bytes3[1] = S->s2Candidates; alg_bytes3[2] = S->s2TextBytes; alg_bytes3[3] = S->streamedBytes; alg_bytes3[4] = S->s1Candidates; alg_bytes3[5] = S->exactReplays; }
    return INFX_OK;
}

int32_t infx_engine_session_replay_breakdown(infx_session* S, float* ms4) {      // k_ex_scan, k_ex_chunk, k_ex_heap, k_exact1 of the last batch (ms)
    if (!S || !ms4) return INFX_EINVAL;
    resolve_kernel_times(S);
    for (int i = 0; i < 4; i++) ms4[i] = S->msReplayParts[i];
    return INFX_OK;
}
int32_t infx_engine_session_plan_breakdown(infx_session* S, double* out4) {      // of the last batch's plan_ms: tokens + term lookups (incl. the LD1 call), of that inside infx_ld1_expand, inside infx_union_build, idf / roles
    if (!S || !out4 || !S->batch) return INFX_EINVAL;
    const Batch& B = *S->batch;
    out4[0] = B.tTok; out4[1] = B.tLd1Dev; out4[2] = B.tUnionDev; out4[3] = B.t1 - B.t0 - B.tUnion;
    return INFX_OK;
}
int32_t infx_engine_session_last_replay(infx_session* S, float* ms, uint32_t* why3) {
    if (!S) return efail(INFX_EINVAL, "null");
    resolve_kernel_times(S);
    if (ms) *ms = S->msReplay; if (why3) { why3[0] = S->flagWhy[0]; why3[1] = S->flagWhy[1]; why3[2] = S->flagWhy[2]; }
    return INFX_OK;
}

int32_t infx_engine_last_timings(infx_engine* e, double* host_ms5, float* kernel_ms3, uint64_t* alg_bytes3) {
    if (!e) return efail(INFX_EINVAL, "null");
    infx_session* S = e->def;
    if (host_ms5) { host_ms5[0] = S->tPrep1; host_ms5[1] = S->tStage1; host_ms5[2] = S->tPrep2; host_ms5[3] = S->tStage2; host_ms5[4] = S->tPost; }
    if (kernel_ms3) { kernel_ms3[0] = S->msAcc; kernel_ms3[1] = S->msSel; kernel_ms3[2] = S->msCov; kernel_ms3[3] = S->msPrep2; kernel_ms3[4] = S->msFin; }
    if (alg_bytes3) { alg_bytes3[0] = S->algBytes; alg_bytes3[1] = S->s2Candidates; alg_bytes3[2] = S->s2TextBytes; alg_bytes3[3] = S->streamedBytes; alg_bytes3[4] = S->s1Candidates; alg_bytes3[5] = S->exactReplays; }
    return INFX_OK;
}

// ---- introspection for parity tests (host logic is testable without a GPU) ------------------------------------------------
int32_t infx_engine_index_stats(infx_engine* e, int64_t* n_docs, int64_t* n_terms, int64_t* n_postings, float* avgdl) {
    if (!e) return efail(INFX_EINVAL, "null");
    if (n_docs) *n_docs = e->ix.N; if (n_terms) *n_terms = (int64_t)e->ix.terms.K();
    if (n_postings) *n_postings = (int64_t)e->ix.terms.doc.size(); if (avgdl) *avgdl = e->ix.avgdl;
    return INFX_OK;
}
int32_t infx_engine_export_index(infx_engine* e, int32_t* df, uint64_t* post_off, int32_t* post_doc, uint8_t* post_w, float* doc_len) {
    if (!e) return efail(INFX_EINVAL, "null");
    const HostIndex& ix = e->ix; size_t T = ix.terms.K();
    if (df) std::memcpy(df, ix.df.data(), T * 4);
    if (post_off) std::memcpy(post_off, ix.terms.off.data(), (T + 1) * 8);
    if (post_doc) std::memcpy(post_doc, ix.terms.doc.data(), ix.terms.doc.size() * 4);
    if (post_w) std::memcpy(post_w, ix.terms.w.data(), ix.terms.w.size());
    if (doc_len) std::memcpy(doc_len, ix.docLen.data(), (size_t)ix.N * 4);
    return INFX_OK;
}
int32_t infx_engine_term_text(infx_engine* e, int32_t t, uint16_t* out, int32_t cap) {
    if (!e || t < 0 || t >= (int32_t)e->ix.terms.K()) return -1;
    uview s = e->ix.terms.keys.key((uint32_t)t);
    std::memcpy(out, s.data(), (size_t)std::min<int>(cap, (int)s.size()) * 2);
    return (int32_t)s.size();
}
int32_t infx_engine_match_ld1(infx_engine* e, const uint16_t* q, int32_t len, int32_t* out, int32_t cap) {
    if (!e || len < 0 || (len && !q) || (cap > 0 && !out)) return -1;
    std::vector<int> m; int c = match_ld1(e->ix, uview((const u16*)q, len), m, cap);
    for (size_t i = 0; i < m.size(); i++) out[i] = m[i];
    return c;
}
// Stage-1 plan of one query (no GPU needed): returns number of terms; mode/prefix_set/n_and/df_s1/df_s2 in meta[5]
int32_t infx_engine_match_ld1_forward(infx_engine* e, const uint16_t* q, int32_t len, int32_t* out, int32_t cap) {   // the literal trie walk (test cross-check)
    if (!e) return -1;
    std::vector<int> m; int c = match_ld1_forward(e->ix, uview((const u16*)q, (size_t)len), m, cap);
    for (size_t i = 0; i < m.size() && (int32_t)i < cap; i++) out[i] = m[i];
    return c;
}
int32_t infx_engine_plan(infx_engine* e, const uint16_t* q, int32_t len, int32_t depth, int32_t* term_ids, int32_t* dfs, float* idfs,
                         uint8_t* roles, uint8_t* ranks, int32_t cap, int32_t* meta, int32_t* flags) {
    if (!e) return -1;
    QueryPlan P; plan_stage1(e->ix, e->fuzzy, uview((const u16*)q, len), depth, P);
    if (flags) *flags = (P.blank ? 1 : 0) | (P.unsupported ? 2 : 0) | (P.noTerms ? 4 : 0);
    int n = (int)P.terms.size();
    for (int i = 0; i < n && i < cap; i++) {
        term_ids[i] = P.terms[i].term_id; idfs[i] = P.terms[i].idf; roles[i] = P.terms[i].role; ranks[i] = P.terms[i].rank;
        dfs[i] = P.terms[i].term_id >= 0 ? e->ix.df[P.terms[i].term_id] : (int32_t)P.terms[i].extra_len;
    }
    if (meta) { meta[0] = P.q.mode; meta[1] = P.q.prefix_set; meta[2] = P.q.n_and; meta[3] = P.q.df_s1; meta[4] = P.q.df_s2; }
    return n;
}
// Host planning profile (measurement hook, no device needed): the per-query host work of a batch, single-threaded, by stage, in microseconds
// per query: [0] plan_tokens (text preparation, term lookups, LD1 expansion), [1] of that: LD1 walks, [2] plan_finish (idf, roles, modes),
// [3] wm_collect (WordMatcher descriptors), [4] prepare_cov_query, [5] plan_tokens_text (the share of [0] that the plan exchange moves to the slice's owner),
// [6] import of the batch's exchanged plans (with host lookups also the LD1 member lists and WordMatcher descriptors), [7] parsing the imported records in
// phase 0 (what an imported query costs there instead of [5] + [4]).  Pending fuzzy unions get a stand-in df.
int32_t infx_engine_host_plan_profile(infx_engine* e, uint32_t nq, const uint16_t* q_arena, const uint64_t* q_offs, int32_t depth, double* out_us) {
    if (!e || !out_us || (nq && (!q_arena || !q_offs))) return efail(INFX_EINVAL, "null argument");
    const HostIndex& ix = e->ix; FuzzyCache fc;
    std::vector<QueryPlan> plans(nq);
    auto t0 = std::chrono::steady_clock::now();
    for (uint32_t i = 0; i < nq; i++) plan_tokens(ix, fc, uview((const u16*)q_arena + q_offs[i], (size_t)(q_offs[i + 1] - q_offs[i])), depth, plans[i], false);
    auto t1 = std::chrono::steady_clock::now();
    for (auto& P : plans) for (auto& r : P.rawTok) if (r.fz && r.fz->df.load() < 0) r.fz->df.store((int)std::max<size_t>(1, r.fz->members.size()));
    auto t2 = std::chrono::steady_clock::now();
    for (uint32_t i = 0; i < nq; i++) plan_finish(ix, plans[i]);
    auto t3 = std::chrono::steady_clock::now();
    WmResult wm; size_t sink = 0;
    for (uint32_t i = 0; i < nq; i++) { const QueryPlan& P = plans[i]; if (P.blank || P.unsupported) continue; wm_collect(ix, P.searchText, ix.cfg.coverPrefixSuffix, wm); sink += wm.lists.size(); }
    auto t4 = std::chrono::steady_clock::now();
    infx_cov_query cq;
    for (uint32_t i = 0; i < nq; i++) { const QueryPlan& P = plans[i]; if (P.blank || P.unsupported) continue; sink += (size_t)prepare_cov_query(ix, P.searchText, cq); }
    auto t5 = std::chrono::steady_clock::now();
    // the plan exchange: [5] the part of plan_tokens a peer can do (plan_tokens_text: no cache, no expansion), [6] importing a peer's plans (the whole batch as one slice)
    { QueryPlan tmp; for (uint32_t i = 0; i < nq; i++) { plan_tokens_text(ix, uview((const u16*)q_arena + q_offs[i], (size_t)(q_offs[i + 1] - q_offs[i])), depth, tmp); sink += tmp.rawTok.size(); } }
    auto t6 = std::chrono::steady_clock::now();
    auto t7 = t6, t8 = t6, t9 = t6;
    const bool dl = e->devLookups; e->devLookups = true;      // the blob of the deployment this hook is about: dictionaries on the device, the plan section only
    const int64_t blobBytes = e->def ? infx_session_prefetch_collect(e->def, nq, q_arena, q_offs, 0, nq, depth) : -1;
    e->devLookups = dl;
    if (blobBytes >= 0) {
        std::vector<uint8_t> blob = e->def->prefetchBlob;
        e->def->planPre.clear(); e->def->planPeer.clear();      // (a peer's slice never overlaps the own one)
        t7 = std::chrono::steady_clock::now();
        const int32_t rc = infx_session_prefetch_import(e->def, blob.data(), (int64_t)blob.size());
        t8 = std::chrono::steady_clock::now();
        if (!rc) {      // [7]: what phase 0 then pays per imported query instead of [5] + [4]: parsing the record into the plan and the coverage query
            QueryPlan tmp; infx_cov_query tc; bool hc, lg; int32_t ce; uint32_t co;
            for (auto& pp : e->def->planPre) if (pp && pp->rec && !parse_plan_record(ix, pp->rec, pp->recLen, depth, tmp, hc, ce, co, lg) && hc && !ce && !lg) sink += parse_cov_record(tmp.searchText, pp->rec, pp->recLen, co, tc) ? 1 : 0;
        }
        t9 = std::chrono::steady_clock::now();
        e->def->planPre.clear(); e->def->planPeer.clear(); e->def->wmPre.clear();
        if (rc) return rc;
    }
    auto us = [&](auto a, auto b) { return std::chrono::duration_cast<std::chrono::nanoseconds>(b - a).count() / 1e3 / std::max<uint32_t>(1, nq); };
    out_us[5] = us(t5, t6); out_us[6] = us(t7, t8); out_us[7] = us(t8, t9);
    out_us[0] = us(t0, t1); out_us[1] = fc.ld1Ns.load() / 1e3 / std::max<uint32_t>(1, nq); out_us[2] = us(t2, t3); out_us[3] = us(t3, t4); out_us[4] = us(t4, t5) + (sink == (size_t)-1 ? 1 : 0);
    return INFX_OK;
}
// WordMatcherLookup.Execute, fully enumerated (tests only): sorted unique ids
int64_t infx_engine_wordmatcher(infx_engine* e, const uint16_t* q, int32_t len, int32_t* out, int64_t cap) {
    if (!e || len < 0 || (len && !q) || (cap > 0 && !out)) return -1;
    WmResult wm; ustr t = normalize(uview((const u16*)q, len)); lower_inplace(t);
    wm_collect(e->ix, t, e->ix.cfg.coverPrefixSuffix, wm);
    std::vector<int32_t> all;
    for (auto& l : wm.lists) all.insert(all.end(), l.p, l.p + l.n);
    std::sort(all.begin(), all.end()); all.erase(std::unique(all.begin(), all.end()), all.end());
    for (size_t i = 0; i < all.size() && (int64_t)i < cap; i++) out[i] = all[i];
    return (int64_t)all.size();
}
// ---- the planning lookups as the DEVICE answers them (parity tests: tests/test_gpu_lookups.py) ----
int32_t infx_engine_device_lookups(infx_engine* e) { return !e ? -1 : (e->devLookups ? 1 : 0); }
int32_t infx_engine_lookup_stats(infx_engine* e, int64_t* out4) {      // words expanded on the device / on the host, queries whose WordMatcher lists came from the device / the host
    if (!e || !out4) return INFX_EINVAL;
    out4[0] = e->ld1OnDevice.load(); out4[1] = e->ld1OnHost.load(); out4[2] = e->wmOnDevice.load(); out4[3] = e->wmOnHost.load();
    return INFX_OK;
}
int32_t infx_engine_match_ld1_device(infx_engine* e, const uint16_t* q, int32_t len, int32_t* out, int32_t cap) {      // like infx_engine_match_ld1; -1 / -2: the kernel handed the word back (status 1 / 2)
    if (!e || len < 0 || (len && !q) || cap < 1 || !out) return -100;
    if (!e->devLookups || !e->def || !e->def->stream) { g_eerr = "no device dictionaries"; return -100; }
    uint32_t offs[2] = {0, (uint32_t)len}, count = 0, status = 0;
    std::vector<int32_t> mem((size_t)cap);
    int32_t rc = infx_ld1_expand(e->def->stream, 1, offs, q, (uint32_t)cap, mem.data(), &count, &status);
    if (rc) { g_eerr = infx_last_error(); return -100 - rc; }
    if (status) return -(int32_t)status;
    for (uint32_t k = 0; k < count && k < (uint32_t)cap; k++) out[k] = mem[k];
    return (int32_t)count;
}
int64_t infx_engine_wordmatcher_device(infx_engine* e, const uint16_t* q, int32_t len, int32_t* out, int64_t cap) {      // like infx_engine_wordmatcher, lists resolved by k_wm
    if (!e || len < 0 || (len && !q)) return -1;
    if (!e->devLookups || !e->ix.cfg.wordMatcher || !e->def || !e->def->stream) { g_eerr = "no device dictionaries"; return -1; }
    const HostIndex& ix = e->ix;
    ustr st((const u16*)q, (size_t)len);
    if (!wm_on_device(ix, st)) { g_eerr = "query not admissible for the device lookup"; return -2; }
    infx_cov_query cq; if (prepare_cov_query(ix, st, cq)) { g_eerr = "query exceeds the Stage-2 envelope"; return -2; }
    size_t words = 0; for_each_word(st, [&](int, int l) { if (l >= 2) words++; });
    std::vector<infx_wm_list> lists(INFX_MAX_WM_LISTS); std::vector<int32_t> owned(words * 4096 + 1); uint32_t nl = 0;
    int32_t rc = stage_coverage_setup(e->def, 0, false);      // (CoverPrefixSuffix off: no affix walk)
    if (!rc) rc = infx_wm_lookup_debug(e->def->stream, &cq, lists.data(), &nl, owned.data(), (uint64_t)words * 4096);
    if (rc) { g_eerr = infx_last_error(); return -1; }
    std::vector<int32_t> all;
    for (uint32_t l = 0; l < nl; l++) {
        const infx_wm_list& L = lists[l];
        const int32_t* p = L.src == 0 ? ix.wmExact.doc.data() : (L.src == 1 ? ix.wmLd1.doc.data() : owned.data());
        const uint64_t lim = L.src == 0 ? ix.wmExact.doc.size() : (L.src == 1 ? ix.wmLd1.doc.size() : owned.size());
        if (L.off + L.len > lim) { g_eerr = "device list out of range"; return -3; }
        for (uint32_t i = 1; i < L.len; i++) if (p[L.off + i] <= p[L.off + i - 1]) { g_eerr = "device list not ascending"; return -4; }
        all.insert(all.end(), p + L.off, p + L.off + L.len);
    }
    std::sort(all.begin(), all.end()); all.erase(std::unique(all.begin(), all.end()), all.end());
    for (size_t i = 0; i < all.size() && (int64_t)i < cap; i++) out[i] = all[i];
    return (int64_t)all.size();
}
int32_t infx_engine_prefix_pop(infx_engine* e, const uint16_t* p, int32_t len) {
    if (!e || len < 0 || (len && !p)) return -1;
    int64_t k = e->ix.prefixKeys.find(uview((const u16*)p, len)); return k < 0 ? 0 : (int32_t)e->ix.prefixPop[k];
}
// last batch: Stage-1 hits of query i (device order re-sorted to the reference's) and the Stage-2 records
int32_t infx_engine_last_stage1(infx_engine* e, uint32_t qi, int64_t* keys, float* scores, int32_t cap) {
    if (!e) return -1;
    infx_session* S = e->def;
    if (qi >= S->lastPlans.size()) return -1;
    // recompute the device index of query qi
    uint32_t j = 0; bool found = false;
    for (uint32_t i = 0; i < S->lastPlans.size(); i++) { const QueryPlan& P = S->lastPlans[i]; if (P.blank || P.unsupported || P.noTerms) { if (i == qi) break; continue; } if (i == qi) { found = true; break; } j++; }
    if (!found) return 0;
    uint32_t c = S->lastHitCount[j]; const infx_hit* H = S->lastHits.data() + (size_t)j * S->lastStride;
    std::vector<uint32_t> o(c); for (uint32_t k = 0; k < c; k++) o[k] = k;
    std::sort(o.begin(), o.end(), [&](uint32_t x, uint32_t y) { if (H[x].score != H[y].score) return H[x].score > H[y].score; return e->ix.docKey[H[x].doc] < e->ix.docKey[H[y].doc]; });
    for (uint32_t k = 0; k < c && (int32_t)k < cap; k++) { keys[k] = e->ix.docKey[H[o[k]].doc]; scores[k] = H[o[k]].score; }
    return (int32_t)c;
}
int64_t infx_engine_last_stage2(infx_engine* e, uint32_t* query_of, int32_t* docs, float* base, float* scores, uint8_t* ties, int32_t* feat, int64_t cap) {
    if (!e) return -1;
    infx_session* S = e->def;
    int64_t n = (int64_t)S->lastCands.size();
    // map cov index -> query index
    for (int64_t i = 0; i < n && i < cap; i++) {
        const infx_cov_cand& c = S->lastCands[i]; const infx_cov_out& o = S->lastOuts[i];
        if (query_of) query_of[i] = c.query; if (docs) docs[i] = c.doc; if (base) base[i] = c.base_score;
        if (scores) scores[i] = o.score; if (ties) ties[i] = o.tiebreaker;
        if (feat) { if (S->lastFeat.size() >= (size_t)(i + 1) * INFX_NFEAT) std::memcpy(feat + (size_t)i * INFX_NFEAT, S->lastFeat.data() + (size_t)i * INFX_NFEAT, INFX_NFEAT * 4); else std::memset(feat + (size_t)i * INFX_NFEAT, 0, INFX_NFEAT * 4); }
    }
    return n;
}
// CoverageEngine.PrepareQuery for one raw query text, exactly as the engine prepares it for infx_stage2_batch / infx_search_fused (a C# host
// would build the same struct from its CoverageQueryContext).  Returns INFX_OK, or the status prepare_cov_query reports (envelope).
int32_t infx_engine_prepare_cov_query(infx_engine* e, const uint16_t* q, int32_t len, infx_cov_query* out) {
    if (!e || !q || !out || len < 0) return efail(INFX_EINVAL, "bad arguments");
    QueryPlan P; plan_tokens(e->ix, e->fuzzy, uview((const u16*)q, (size_t)len), 500, P, true);
    if (P.blank || P.unsupported) return efail(INFX_EINVAL, "blank or unsupported query");
    std::memset(out, 0, sizeof *out);
    return prepare_cov_query(e->ix, P.searchText, *out);
}
int32_t infx_sizeof_cov_query(void) { return (int32_t)sizeof(infx_cov_query); }
// the same for a query beyond the fast envelope: the record of the long-query table (infx_stage2_long_queries)
int32_t infx_engine_prepare_cov_query_long(infx_engine* e, const uint16_t* q, int32_t len, infx_cov_query_long* out) {
    if (!e || !out || (len && !q)) return efail(INFX_EINVAL, "null argument");
    QueryPlan P; plan_tokens_text(e->ix, uview((const u16*)q, (size_t)len), 500, P);
    if (P.blank || P.unsupported) return efail(INFX_EINVAL, "blank or unsupported query");
    return prepare_cov_query_long(e->ix, P.searchText, *out);
}
int32_t infx_sizeof_cov_query_long(void) { return (int32_t)sizeof(infx_cov_query_long); }
int32_t infx_engine_effective_cpus(void) { return effective_cpus(); }
// parity tooling: switch the introspection downloads (Stage-1 rows, Stage-2 candidates / features of the last batch) on or off at run time
int32_t infx_engine_set_introspection(infx_engine* e, int32_t on) { if (!e) return INFX_EINVAL; e->cfg.want_features = on ? 1 : 0; return INFX_OK; }

int32_t infx_engine_normalize(const uint16_t* s, int32_t len, int32_t lower, uint16_t* out, int32_t cap) {
    ustr r = normalize(uview((const u16*)s, len)); if (lower) lower_inplace(r);
    std::memcpy(out, r.data(), (size_t)std::min<int>(cap, (int)r.size()) * 2);
    return (int32_t)r.size();
}
// raw access for bench.py (HBM-resident inputs are the engine's; these expose the flat host arrays for oracle adoption)
int32_t infx_engine_device_handles(infx_engine* e, infx_index** idx, infx_stream** st) { if (!e) return INFX_EINVAL; if (idx) *idx = e->dev; if (st) *st = e->def->stream; return INFX_OK; }


// ---- INFDX2 index files (host/infdx2.h) -------------------------------------------------------------------------------------------------------
// SearchEngine.Load (SearchEngine.cs:399-441) for files whose documents were indexed as single Med-weight fields: the documents are read and indexed
// (which uploads the shard as infx_engine_index_documents does), Deleted flags are applied, and every stored term is compared with the index just
// built.  *checked3 = {documents, stored terms compared, stored postings compared}.  INFX_EUNSUPPORTED: the stored postings are not what this
// builder produces for the stored texts (multi-field weights, other tokenizer settings); INFX_EINVAL: not an INFDX2 file / corrupted.
// ---- node-local cache of the host index (host/hostcache.h): one build per node instead of one per rank ------------------------------------
static uint64_t syn_hash(const SynMap& m) {
    uint64_t h = 1469598103934665603ull;
    for (auto& pr : m.parent) for (const ustr* t : {&pr.first, &pr.second}) { for (u16 c : *t) { h ^= c; h *= 1099511628211ull; } h ^= 0xFFFFu; h *= 1099511628211ull; }
    return h;
}
int64_t infx_engine_fuzzy_cache_size(infx_engine* e) { return e ? (int64_t)e->fuzzy.size() : -1; }
int32_t infx_engine_set_build_threads(infx_engine* e, int32_t threads) {
    if (!e || threads < 0) return efail(INFX_EINVAL, "bad arguments");
    e->buildThreads = threads; return INFX_OK;
}
int32_t infx_engine_save_host_index(infx_engine* e, const char* path) {
    if (!e || !path) return efail(INFX_EINVAL, "null argument");
    if (!e->indexed) return efail(INFX_EINVAL, "index the documents first");
    const std::string err = hostcache::save(path, e->ix, e->keysAreIds, hostcache::config_signature(e->ix.cfg, syn_hash(e->ix.cfg.syn)), index_fingerprint(e->ix));
    if (!err.empty()) return efail(INFX_EINVAL, err.c_str());
    return INFX_OK;
}
int32_t infx_engine_index_from_host_cache(infx_engine* e, const char* path) {
    if (!e || !path) return efail(INFX_EINVAL, "null argument");
    if (e->indexed) return efail(INFX_EINVAL, "this engine instance is already indexed (re-indexing: create a new engine)");
    bool keysAreIds = true;
    const std::string err = hostcache::load(path, e->ix, keysAreIds, hostcache::config_signature(e->ix.cfg, syn_hash(e->ix.cfg.syn)), &index_fingerprint);
    if (!err.empty()) return efail(INFX_EINVAL, err.c_str());
    e->keysAreIds = keysAreIds;
    return finish_index(e);
}

int32_t infx_engine_load_index(infx_engine* e, const char* path, int64_t* checked3) {
    if (!e || !path) return efail(INFX_EINVAL, "null argument");
    if (e->indexed) return efail(INFX_EINVAL, "this engine instance is already indexed");
    infdx2::File F;
    if (!infdx2::read_file(path, F)) return efail(INFX_EINVAL, F.error);
    const int64_t n = (int64_t)F.docs.size();
    std::vector<int64_t> keys((size_t)n); std::vector<uint64_t> offs((size_t)n + 1, 0); std::vector<uint16_t> arena;
    for (int64_t d = 0; d < n; d++) {
        if (F.docs[d].id != (int32_t)d) return efail(INFX_EUNSUPPORTED, "document ids of the file are not 0..n-1 in order (written after deletions): the stored postings refer to ids Load does not restore");
        keys[d] = F.docs[d].key; arena.insert(arena.end(), F.docs[d].text.begin(), F.docs[d].text.end()); offs[d + 1] = arena.size();
    }
    if (arena.empty()) arena.push_back(0);
    const int32_t w = 1;      // Weight.Med: ReadDocuments adds the text as the single field "content" with Weight.Med (IndexPersistence.cs:338-339)
    if (n > 0x7FFFFFF0ll) return efail(INFX_EINVAL, "too many documents");
    // build the host index, CHECK it against the file, and only then commit (upload, key map): a refused file leaves the engine unindexed and reusable
    {
        DocSource src{n, 1, &w, keys.data(), (const u16*)arena.data(), offs.data()};
        const int planThreads = e->ix.cfg.threads;
        if (e->buildThreads > 0) e->ix.cfg.threads = e->buildThreads;
        build_index(src, e->ix);
        e->ix.cfg.threads = planThreads;
    }
    const HostIndex& ix = e->ix;
    int64_t nterms = 0, npost = 0;
    const char* bad = nullptr;
    infdx2::LossyMatcher termOf(ix.terms.keys);          // the same text, or the lossy UTF-8 image of a term that holds half a surrogate pair (infdx2.h)
    for (auto& t : F.terms) {
        const int64_t id = termOf.match(t.text, [&](uint32_t k) { return ix.df[k] > 0; });
        if (id < 0) { bad = "a stored term does not exist in the index built from the stored documents"; break; }
        const uint64_t b = ix.terms.off[id], len = ix.terms.off[id + 1] - b;
        if (ix.df[id] != t.df || len != t.docs.size()) { bad = "a stored term's document frequency / posting count differs from the rebuilt index"; break; }
        for (size_t i = 0; i < t.docs.size() && !bad; i++)
            if (ix.terms.doc[b + i] != t.docs[i] || ix.terms.w[b + i] != t.w[i]) bad = "a stored posting (document, weight) differs from the rebuilt index: the file was not written from single Med-weight fields";
        if (bad) break;
        nterms++; npost += (int64_t)t.docs.size();
    }
    if (!bad) {   // ... and the other direction: the rebuilt index may not hold non-stop terms the file lacks (e.g. a file written with another stop-term limit)
        int64_t built = 0; for (size_t id = 0; id < ix.terms.K(); id++) if (ix.df[id] > 0) built++;
        if (built != nterms) bad = "the index rebuilt from the stored documents holds another number of non-stop terms than the file";
    }
    if (!bad) bad = infdx2::check_derived(F, ix);
    if (bad) { const HostConfig keep = e->ix.cfg; e->ix = HostIndex{}; e->ix.cfg = keep; return efail(INFX_EUNSUPPORTED, bad); }
    e->keysAreIds = false;
    int32_t rc = finish_index(e);
    if (rc) return rc;
    std::vector<int64_t> gone; for (auto& d : F.docs) if (d.deleted) gone.push_back(d.key);
    if (!gone.empty()) { rc = infx_engine_delete_documents(e, gone.data(), (int64_t)gone.size(), nullptr); if (rc) return rc; }
    if (checked3) { checked3[0] = n; checked3[1] = nterms; checked3[2] = npost; }
    return INFX_OK;
}

// ---- INFS segment files (host/infs.h): SearchEngine.Flush's on-disk segments -------------------------------------------------------------------
struct infx_segment { infs::Segment S; };
int32_t infx_segment_open(const char* path, infx_segment** out) {
    if (!path || !out) return efail(INFX_EINVAL, "null argument");
    infx_segment* g = new infx_segment();
    if (!infs::read_file(path, g->S)) { const std::string m = g->S.error; delete g; return efail(INFX_EINVAL, "INFS segment: " + m); }
    *out = g; return INFX_OK;
}
void infx_segment_close(infx_segment* g) { delete g; }
int32_t infx_segment_info(infx_segment* g, int32_t* doc_count, int32_t* num_terms, int64_t* num_postings, int64_t* term_chars) {
    if (!g) return efail(INFX_EINVAL, "null segment");
    if (doc_count) *doc_count = g->S.docCount; if (num_terms) *num_terms = (int32_t)g->S.terms.size(); if (num_postings) *num_postings = (int64_t)g->S.doc.size();
    if (term_chars) { int64_t c = 0; for (auto& t : g->S.terms) c += (int64_t)t.size(); *term_chars = c; }
    return INFX_OK;
}
int32_t infx_segment_export(infx_segment* g, uint32_t* term_offs, uint16_t* term_chars, uint64_t* post_offs, int32_t* doc_ids, uint8_t* weights) {
    if (!g) return efail(INFX_EINVAL, "null segment");
    const infs::Segment& S = g->S; const size_t T = S.terms.size();
    if (term_offs) { uint32_t o = 0; for (size_t t = 0; t < T; t++) { term_offs[t] = o; if (term_chars) std::memcpy(term_chars + o, S.terms[t].data(), S.terms[t].size() * 2); o += (uint32_t)S.terms[t].size(); } term_offs[T] = o; }
    if (post_offs) std::memcpy(post_offs, S.off.data(), (T + 1) * 8);
    if (doc_ids && !S.doc.empty()) std::memcpy(doc_ids, S.doc.data(), S.doc.size() * 4);
    if (weights && !S.w.empty()) std::memcpy(weights, S.w.data(), S.w.size());
    return INFX_OK;
}
int32_t infx_engine_verify_segment(infx_engine* e, const char* path, int32_t doc_base, int64_t* checked3) {
    if (!e || !path || doc_base < 0) return efail(INFX_EINVAL, "bad arguments");
    if (!e->indexed) return efail(INFX_EINVAL, "index the documents first: a segment holds postings, not documents");
    infs::Segment S;
    if (!infs::read_file(path, S)) return efail(INFX_EINVAL, "INFS segment: " + S.error);
    const HostIndex& ix = e->ix;
    if ((int64_t)doc_base + S.docCount > ix.N) return efail(INFX_EUNSUPPORTED, "the segment's documents [doc_base, doc_base + docCount) lie outside the indexed corpus");
    const int32_t lo = doc_base, hi = doc_base + S.docCount;
    int64_t npost = 0;
    for (size_t t = 0; t < S.terms.size(); t++) {
        const int64_t id = ix.terms.keys.find(uview((const u16*)S.terms[t].data(), S.terms[t].size()));
        if (id < 0) return efail(INFX_EUNSUPPORTED, "a term of the segment does not exist in the index built from the documents");
        const int32_t* p = ix.terms.doc.data(); const uint64_t b = ix.terms.off[id], z = ix.terms.off[id + 1];
        const uint64_t a = std::lower_bound(p + b, p + z, lo) - p, c = std::lower_bound(p + a, p + z, hi) - p;
        const uint64_t n = S.off[t + 1] - S.off[t];
        if (c - a != n) return efail(INFX_EUNSUPPORTED, "a term's posting count inside the segment's document range differs from the index");
        for (uint64_t i = 0; i < n; i++)
            if (p[a + i] != S.doc[S.off[t] + i] + doc_base || ix.terms.w[a + i] != S.w[S.off[t] + i]) return efail(INFX_EUNSUPPORTED, "a posting (document, weight) of the segment differs from the index");
        npost += (int64_t)n;
    }
    // the other direction: every index term with postings in the range must be in the segment (SegmentWriter keeps the terms with DocumentFrequency > 0)
    int64_t present = 0;
    for (size_t id = 0; id < ix.terms.K(); id++) {
        if (ix.df[id] <= 0) continue;
        const int32_t* p = ix.terms.doc.data(); const uint64_t b = ix.terms.off[id], z = ix.terms.off[id + 1];
        const uint64_t a = std::lower_bound(p + b, p + z, lo) - p;
        if (a < z && p[a] < hi) present++;
    }
    if (present != (int64_t)S.terms.size()) return efail(INFX_EUNSUPPORTED, "the index holds terms with postings in the segment's document range that the segment lacks");
    if (checked3) { checked3[0] = S.docCount; checked3[1] = (int64_t)S.terms.size(); checked3[2] = npost; }
    return INFX_OK;
}

// ---- Document.Deleted -----------------------------------------------------------------------------------------------------------------
// DocumentCollection.DeleteDocumentsByKey (Core/DocumentCollection.cs:200-212): every document (alias / segment) with one of the keys is marked
// deleted.  The index itself is not touched — like the reference between a deletion and the next re-index, df / doc lengths / avgdl still
// include the document; the query path skips it (include/infidex_hip.h, infx_set_deleted).  Exclusive: no search may be in flight.
int32_t infx_engine_delete_documents(infx_engine* e, const int64_t* keys, int64_t n, int64_t* out_marked) {
    if (!e || (n > 0 && !keys)) return efail(INFX_EINVAL, "null argument");
    if (!e->indexed) return efail(INFX_EINVAL, "delete before index_documents");
    const int64_t N = e->ix.N; int64_t marked = 0;
    if (e->deleted.empty()) e->deleted.assign((size_t)N, 0);
    if (e->keysAreIds) { for (int64_t i = 0; i < n; i++) if (keys[i] >= 0 && keys[i] < N && !e->deleted[(size_t)keys[i]]) { e->deleted[(size_t)keys[i]] = 1; marked++; } }
    else {
        std::unordered_set<int64_t> ks(keys, keys + n);
        for (int64_t d = 0; d < N; d++) if (!e->deleted[(size_t)d] && ks.count(e->ix.docKey[(size_t)d])) { e->deleted[(size_t)d] = 1; marked++; }
    }
    if (out_marked) *out_marked = marked;
    if (e->dev) { int32_t rc = infx_set_deleted(e->dev, (uint32_t)N, e->deleted.data()); if (rc) { g_eerr = infx_last_error(); return rc; } }
    e->invalidate_filter_counts(); e->maskEpoch++;
    return refresh_first_live(e);
}
// Document.Deleted = true on single documents, by internal id (indexing order): the documents of one key need not share the flag (a persisted index
// restores it per document, Indexing/IndexPersistence.cs:334).  Exclusive, as infx_engine_delete_documents.
int32_t infx_engine_delete_document_ids(infx_engine* e, const int64_t* ids, int64_t n, int64_t* out_marked) {
    if (!e || (n > 0 && !ids)) return efail(INFX_EINVAL, "null argument");
    if (!e->indexed) return efail(INFX_EINVAL, "delete before index_documents");
    const int64_t N = e->ix.N; int64_t marked = 0;
    if (e->deleted.empty()) e->deleted.assign((size_t)N, 0);
    for (int64_t i = 0; i < n; i++) if (ids[i] >= 0 && ids[i] < N && !e->deleted[(size_t)ids[i]]) { e->deleted[(size_t)ids[i]] = 1; marked++; }
    if (out_marked) *out_marked = marked;
    if (e->dev) { int32_t rc = infx_set_deleted(e->dev, (uint32_t)N, e->deleted.data()); if (rc) { g_eerr = infx_last_error(); return rc; } }
    e->invalidate_filter_counts(); e->maskEpoch++;
    return refresh_first_live(e);
}
// Clears every Deleted flag (what a reload of the undeleted documents would give).
int32_t infx_engine_restore_documents(infx_engine* e) {
    if (!e) return efail(INFX_EINVAL, "null argument");
    e->deleted.clear();
    if (e->dev && e->indexed) { int32_t rc = infx_set_deleted(e->dev, 0, nullptr); if (rc) { g_eerr = infx_last_error(); return rc; } }
    e->invalidate_filter_counts(); e->maskEpoch++;
    return e->indexed ? refresh_first_live(e) : INFX_OK;
}

// the facet columns: the first INFX_MAX_FACET_COLS facetable columns of the engine; *total_values = the sum of their dictionaries' sizes
static std::vector<uint32_t> facet_columns(const infx_engine* e, size_t* total_values = nullptr) {
    std::vector<uint32_t> cols; size_t total = 0;
    for (size_t c = 0; c < e->columns.size() && cols.size() < INFX_MAX_FACET_COLS; c++) if (e->columns[c].facetable) { cols.push_back((uint32_t)c); total += e->columns[c].dict.size(); }
    if (total_values) *total_values = total;
    return cols;
}
typedef std::vector<std::pair<uint32_t, uint32_t>> FacetPairs;      // (code, count)
// A column's (code, count) pairs as FacetBuilder lists them: empty strings are not facet values (FacetBuilder.cs:95-99, :170-174), count descending, then value
// ascending (the column's rank), cut to 100
static void order_facets(const filt::Column& C, FacetPairs& v) {
    v.erase(std::remove_if(v.begin(), v.end(), [&](auto& x) { return x.first >= C.text.size() || C.text[x.first].empty(); }), v.end());
    std::sort(v.begin(), v.end(), [&](auto& a, auto& b) { if (a.second != b.second) return a.second > b.second; return C.rank[a.first] < C.rank[b.first]; });
    if (v.size() > 100) v.resize(100);
}
// the readers' copies: up to cap pairs into codes / counts (returns their number); a message into out, cap (returns its length)
static int32_t copy_pairs(const FacetPairs& v, uint32_t* codes, uint32_t* counts, int32_t cap) {
    int32_t m = 0; for (auto& x : v) { if (m >= cap) break; codes[m] = x.first; counts[m] = x.second; m++; }
    return m;
}
static int32_t copy_message(const std::string& t, char* out, int32_t cap) {
    if (out && cap > 0) snprintf(out, (size_t)cap, "%s", t.c_str());
    return (int32_t)t.size();
}
// The readers of a per-request call, over answer_at(): the answer's message (its length; -1 without an answer), the size of its set with its status
// (INFX_EINVAL and `none` without an answer)
static int32_t answer_error(const Answer* a, char* out, int32_t cap) { return a ? copy_message(a->err, out, cap) : -1; }
static int32_t answer_total(const Answer* a, uint32_t* total, const char* none) {
    if (!a || !total) return efail(INFX_EINVAL, none);
    *total = a->total;
    return a->status;
}
// the getters of a call's counters: each value to its destination, where one was given
static int32_t put_stats(std::initializer_list<std::pair<uint32_t*, uint32_t>> to) { for (auto& p : to) if (p.first) *p.first = p.second; return INFX_OK; }
// the engine's column of a field name, -1: none (case sensitive, as the filter's fields)
static int32_t column_named(const infx_engine* e, const char* name) {
    int32_t col = -1;
    for (size_t c = 0; c < e->columns.size(); c++) if (e->columns[c].name == name) col = (int32_t)c;
    return col;
}

// ---- Infiscript post-filter + facets (config 5): Query.Filter / Query.EnableFacets (SearchEngine.cs:298-316) ------------------------------
// One non-indexed document field for all documents (DocumentFields / Field.Value), by internal id: kind 1 int64, 2 double, 3 UTF-8 strings
// (arena + n+1 offsets).  facetable = Field.Facetable.  After infx_engine_index_documents.
static int32_t install_column(infx_engine* e, size_t at, filt::Column&& c);
static void drop_list_column_named(infx_engine* e, const char* name);
int32_t infx_engine_add_column(infx_engine* e, const char* name, int32_t kind, int32_t facetable, int64_t n, const int64_t* vi, const double* vd,
                               const char* arena, const uint64_t* offs) {
    if (!e || !name || n < 0 || (kind == 1 && !vi) || (kind == 2 && !vd) || (kind == 3 && (!arena || !offs)) || kind < 1 || kind > 3) return efail(INFX_EINVAL, "bad column arguments");
    if (!e->indexed || n != e->ix.N) return efail(INFX_EINVAL, "a column needs one value per indexed document");
    // a name the engine already holds: the column is REPLACED in its slot (new values, possibly of another kind); everything derived from it goes
    if (!name[0]) return efail(INFX_EINVAL, "a column needs a name");
    size_t at = e->columns.size();
    for (size_t i = 0; i < e->columns.size(); i++) if (e->columns[i].name == name) at = i;
    if (at == e->columns.size()) for (size_t i = 0; i < e->columns.size(); i++) if (e->columns[i].name.empty()) { at = i; break; }      // the slot a list column took a scalar column's name from
    if (at == e->columns.size() && e->columns.size() >= 64) return efail(INFX_ECAPACITY, "too many columns");
    filt::Column c; c.name = name; c.facetable = facetable != 0;
    if (kind == 1) filt::encode_column(c, (size_t)n, [&](size_t d) { filt::Boxed b; b.kind = 1; b.i = vi[d]; return b; }, (long long)0);
    else if (kind == 2) filt::encode_column(c, (size_t)n, [&](size_t d) { filt::Boxed b; b.kind = 2; b.d = vd[d]; return b; }, (uint64_t)0);
    else filt::encode_column(c, (size_t)n, [&](size_t d) { filt::Boxed b; b.kind = 3; b.s.assign(arena + offs[d], arena + offs[d + 1]); return b; }, std::string());
    { int32_t rc = install_column(e, at, std::move(c)); if (rc) return rc; }
    drop_list_column_named(e, name);      // one namespace: a list column of this name is replaced by the scalar column
    return INFX_OK;
}
// Puts column c into slot `at` (a new slot at the end, or a replaced one: everything derived from the old column goes) and invalidates what was compiled or counted
static int32_t install_column(infx_engine* e, size_t at, filt::Column&& c) {
    const size_t n = c.codes.size();
    if (e->dev) {
        int32_t rc = infx_upload_column(e->dev, (uint32_t)at, (uint32_t)n, c.codes.data(), (uint32_t)c.dict.size());      // (a re-upload voids the column's sort rank on the device)
        if (rc) { g_eerr = infx_last_error(); return rc; }
    }
    if (at < e->columns.size()) {
        std::lock_guard<std::mutex> lk(e->filterMu);
        e->columns[at] = std::move(c);
        if (at < e->sortRanked.size()) e->sortRanked[at] = 0;
        if (at < e->tieRanked.size()) e->tieRanked[at] = 0;
        if (at < e->rangeIndex.size()) e->rangeIndex[at] = infx_engine::RangeIndex();
        if (at < e->statsIndex.size()) e->statsIndex[at] = infx_engine::StatsIndex();
    } else e->columns.push_back(std::move(c));
    e->invalidate_filter_counts();
    e->maskEpoch++;
    e->retire_filters();      // leaf tables of filters compiled before this field existed treat it as null: compile again on next use
    return INFX_OK;
}
int32_t infx_engine_column_count(infx_engine* e) { return e ? (int32_t)e->columns.size() : -1; }
int32_t infx_engine_column_info(infx_engine* e, int32_t col, char* name, int32_t cap, int32_t* facetable, int32_t* num_values) {
    if (!e || col < 0 || col >= (int32_t)e->columns.size()) return INFX_EINVAL;
    const filt::Column& c = e->columns[col];
    if (name && cap > 0) snprintf(name, (size_t)cap, "%s", c.name.c_str());
    if (facetable) *facetable = c.facetable ? 1 : 0; if (num_values) *num_values = (int32_t)c.dict.size();
    return INFX_OK;
}
int32_t infx_engine_column_value(infx_engine* e, int32_t col, uint32_t code, char* out, int32_t cap) {      // ToString() of a distinct value (facet key)
    if (!e || col < 0 || col >= (int32_t)e->columns.size() || code >= e->columns[col].text.size()) return -1;
    const std::string& t = e->columns[col].text[code];
    if (out && cap > 0) snprintf(out, (size_t)cap, "%s", t.c_str());
    return (int32_t)t.size();
}
// ---- list columns: a field that holds a list of values per document (Field.IsArray), in filters and filtered / whole-corpus facets ---------------------
static int32_t list_column_named(const infx_engine* e, const char* name) {
    for (size_t c = 0; c < e->listCols.size(); c++) if (e->listCols[c].live() && e->listCols[c].name == name) return (int32_t)c;
    return -1;
}
static void drop_list_column_named(infx_engine* e, const char* name) {
    const int32_t lc = list_column_named(e, name);
    if (lc < 0) return;
    { std::lock_guard<std::mutex> lk(e->filterMu); e->listCols[lc] = filt::ListColumn(); }
    if (e->dev) infx_upload_list_column(e->dev, (uint32_t)lc, 0, nullptr, nullptr, 0);
}
// the facetable list columns: the first INFX_ENGINE_MAX_LIST_FACETS of them
static std::vector<uint32_t> list_facet_columns(const infx_engine* e) {
    std::vector<uint32_t> cols;
    for (size_t c = 0; c < e->listCols.size() && cols.size() < INFX_ENGINE_MAX_LIST_FACETS; c++) if (e->listCols[c].live() && e->listCols[c].facetable) cols.push_back((uint32_t)c);
    return cols;
}
// One list of values per indexed document, by internal id: doc_offs[n + 1] (ascending from 0) delimits document d's elements in vals_i / vals_d / the
// strings arena + offs (element j: arena[offs[j] .. offs[j + 1])).  See include/infidex_engine.h.
int32_t infx_engine_add_list_column(infx_engine* e, const char* name, int32_t kind, int32_t facetable, int64_t n, const uint64_t* doc_offs, const int64_t* vi, const double* vd,
                                    const char* arena, const uint64_t* offs) {
    if (!e || !name || !name[0] || n < 0 || !doc_offs || kind < 1 || kind > 3) return efail(INFX_EINVAL, "bad list-column arguments");
    if (e->nranks > 1) return efail(INFX_EUNSUPPORTED, "list columns need an engine that is not sharded");
    if (!e->indexed || n != e->ix.N) return efail(INFX_EINVAL, "a list column needs one list per indexed document");
    if (doc_offs[0] != 0) return efail(INFX_EINVAL, "a list column's offsets start at 0");
    for (int64_t d = 0; d < n; d++) if (doc_offs[d + 1] < doc_offs[d]) return efail(INFX_EINVAL, "a list column's offsets must ascend");
    const uint64_t total = doc_offs[n];
    if (total > 0xFFFFFFFFull) return efail(INFX_ECAPACITY, "a list column holds fewer than 2^32 elements");
    if (total && ((kind == 1 && !vi) || (kind == 2 && !vd) || (kind == 3 && (!arena || !offs)))) return efail(INFX_EINVAL, "bad list-column arguments");
    int32_t at = list_column_named(e, name);
    if (at < 0) {
        size_t live = 0, facets = 0; for (auto& L : e->listCols) { live += L.live(); facets += L.live() && L.facetable; }
        if (live >= INFX_ENGINE_MAX_LIST_COLS) return efail(INFX_ECAPACITY, "more than INFX_ENGINE_MAX_LIST_COLS (8) list columns");
        if (facetable && facets >= INFX_ENGINE_MAX_LIST_FACETS) return efail(INFX_ECAPACITY, "more than INFX_ENGINE_MAX_LIST_FACETS (4) facetable list columns");
        for (size_t c = 0; c < e->listCols.size() && at < 0; c++) if (!e->listCols[c].live()) at = (int32_t)c;
        if (at < 0) { std::lock_guard<std::mutex> lk(e->filterMu); at = (int32_t)e->listCols.size(); e->listCols.emplace_back(); }
    } else if (facetable && !e->listCols[at].facetable) {
        size_t facets = 0; for (auto& L : e->listCols) facets += L.live() && L.facetable;
        if (facets >= INFX_ENGINE_MAX_LIST_FACETS) return efail(INFX_ECAPACITY, "more than INFX_ENGINE_MAX_LIST_FACETS (4) facetable list columns");
    }
    filt::ListColumn c; c.name = name; c.facetable = facetable != 0; c.kind = kind;
    if (kind == 1) filt::encode_column(c.dict, (size_t)total, [&](size_t j) { filt::Boxed b; b.kind = 1; b.i = vi[j]; return b; }, (long long)0);
    else if (kind == 2) filt::encode_column(c.dict, (size_t)total, [&](size_t j) { filt::Boxed b; b.kind = 2; b.d = vd[j]; return b; }, (uint64_t)0);
    else filt::encode_column(c.dict, (size_t)total, [&](size_t j) { filt::Boxed b; b.kind = 3; b.s.assign(arena + offs[j], arena + offs[j + 1]); return b; }, std::string());
    c.off.resize((size_t)n + 1); for (int64_t d = 0; d <= n; d++) c.off[(size_t)d] = (uint32_t)doc_offs[d];
    if (e->dev) {
        int32_t rc = infx_upload_list_column(e->dev, (uint32_t)at, (uint32_t)n, c.off.data(), c.dict.codes.data(), (uint32_t)c.dict.dict.size());
        if (rc) { g_eerr = infx_last_error(); return rc; }
    }
    { std::lock_guard<std::mutex> lk(e->filterMu); e->listCols[(size_t)at] = std::move(c); }
    // one namespace: a scalar column of this name is replaced.  Its slot stays (the slots above it keep their indices) as a nameless column of one null
    // value that no field name reaches, until infx_engine_add_column reuses it.
    const int32_t sc = column_named(e, name);
    if (sc >= 0) {
        filt::Column t; t.dict.push_back(filt::Boxed()); t.text.push_back(std::string()); t.rank.push_back(0u); t.codes.assign((size_t)n, 0u);
        return install_column(e, (size_t)sc, std::move(t));      // (invalidates, as below)
    }
    e->invalidate_filter_counts();
    e->maskEpoch++;
    e->retire_filters();      // with them go the derived leaf columns
    return INFX_OK;
}
int32_t infx_engine_list_column_count(infx_engine* e) { return e ? (int32_t)e->listCols.size() : -1; }
// list column slot lcol (a free slot has an empty name): its name, whether it is facetable, its number of distinct element values, the kind of its elements
int32_t infx_engine_list_column_info(infx_engine* e, int32_t lcol, char* name, int32_t cap, int32_t* facetable, int32_t* num_values, int32_t* kind) {
    if (!e || lcol < 0 || lcol >= (int32_t)e->listCols.size()) return INFX_EINVAL;
    const filt::ListColumn& c = e->listCols[(size_t)lcol];
    if (name && cap > 0) snprintf(name, (size_t)cap, "%s", c.name.c_str());
    if (facetable) *facetable = c.facetable ? 1 : 0; if (num_values) *num_values = (int32_t)c.dict.dict.size(); if (kind) *kind = c.kind;
    return INFX_OK;
}
int32_t infx_engine_list_column_value(infx_engine* e, int32_t lcol, uint32_t code, char* out, int32_t cap) {      // ToString() of a distinct element value
    if (!e || lcol < 0 || lcol >= (int32_t)e->listCols.size() || code >= e->listCols[(size_t)lcol].dict.text.size()) return -1;
    return copy_message(e->listCols[(size_t)lcol].dict.text[code], out, cap);
}
// the stored list of one document: up to cap element codes into codes; returns the list's length, -1 on error
int64_t infx_engine_list_column_document(infx_engine* e, int32_t lcol, int64_t document_index, uint32_t* codes, int64_t cap) {
    if (!e || lcol < 0 || lcol >= (int32_t)e->listCols.size() || !e->listCols[(size_t)lcol].live()) { efail(INFX_EINVAL, "no such list column"); return -1; }
    const filt::ListColumn& c = e->listCols[(size_t)lcol];
    if (document_index < 0 || document_index >= (int64_t)c.docs()) { efail(INFX_EINVAL, "no document of this index"); return -1; }
    const uint32_t b = c.off[(size_t)document_index], m = c.off[(size_t)document_index + 1] - b;
    for (uint32_t j = 0; j < m && (int64_t)j < cap && codes; j++) codes[j] = c.dict.codes[b + j];
    return (int64_t)m;
}
int32_t infx_engine_last_list_leaf_stats(infx_engine* e, uint32_t* built, uint32_t* launches) {
    if (!e) return efail(INFX_EINVAL, "null argument");
    std::lock_guard<std::mutex> lk(e->filterMu);
    return put_stats({{built, e->llBuilt}, {launches, e->llLaunches}});
}
int32_t infx_engine_list_leaf_totals(infx_engine* e, uint64_t* built, uint64_t* launches) {
    if (!e) return efail(INFX_EINVAL, "null argument");
    std::lock_guard<std::mutex> lk(e->filterMu);
    if (built) *built = e->llBuiltAll; if (launches) *launches = e->llLaunchesAll;
    return INFX_OK;
}
// The leaves of program P over list columns, lowered: for each such leaf its derived column's slot in slotOf[leaf index] (leaves over other fields: -1), the
// missing derived columns built — one k_list_leaf launch per list column — and cached, and the (list column, key) references of the program in refs.
// INFX_ECAPACITY when no cache entry or no scalar slot is free: the expression is refused alone.  Caller holds e->filterMu.
static int32_t lower_list_leaves(infx_engine* e, const filt::Program& P, std::vector<int>& slotOf, std::vector<std::pair<int, std::string>>& refs) {
    slotOf.assign(P.leaves.size(), -1); refs.clear();
    struct Pending { int lcol; std::string key; std::vector<uint32_t> words; bool empty; uint32_t slot; };
    std::vector<Pending> pend;
    auto undo = [&](int32_t rc, const char* msg) {      // the entries this compile added are not built: they go
        for (auto& p : pend) for (size_t i = 0; i < e->derived.size(); i++) if (e->derived[i].lcol == p.lcol && e->derived[i].key == p.key) { e->derived.erase(e->derived.begin() + (long)i); break; }
        return efail(rc, msg);
    };
    // every derived column the expression reads is kept while room is made for the ones it is missing
    std::vector<int> lcOf(P.leaves.size(), -1); std::vector<std::string> keyOf(P.leaves.size());
    for (size_t l = 0; l < P.leaves.size(); l++) {
        const filt::Leaf& L = P.leaves[l];
        if (column_named(e, L.field.c_str()) >= 0) continue;
        lcOf[l] = list_column_named(e, L.field.c_str());
        if (lcOf[l] >= 0) keyOf[l] = filt::list_leaf_key(L);
    }
    for (size_t l = 0; l < P.leaves.size(); l++) {
        const filt::Leaf& L = P.leaves[l];
        const int32_t lc = lcOf[l];
        if (lc < 0) continue;
        const std::string& key = keyOf[l];
        const uint64_t tick = ++e->derivedTick;
        infx_engine::DerivedCol* D = nullptr;
        for (auto& x : e->derived) if (x.lcol == lc && x.key == key) D = &x;
        if (!D) {
            auto pinned = [&](const infx_engine::DerivedCol& x) {      // in use by a cached filter, or by this very expression
                if (x.refs) return true;
                for (size_t j = 0; j < lcOf.size(); j++) if (lcOf[j] == x.lcol && keyOf[j] == x.key) return true;
                return false;
            };
            if (e->derived.size() >= INFX_ENGINE_MAX_DERIVED) {
                int victim = -1;
                for (size_t i = 0; i < e->derived.size(); i++) if (!pinned(e->derived[i]) && (victim < 0 || e->derived[i].lastUse < e->derived[(size_t)victim].lastUse)) victim = (int)i;
                if (victim < 0) return undo(INFX_ECAPACITY, "no derived leaf column is free: INFX_ENGINE_MAX_DERIVED (16) list-column leaves are in use by cached filters");
                e->derived.erase(e->derived.begin() + victim);
            }
            int slot = -1;
            for (int c = 63; c >= (int)e->columns.size() && slot < 0; c--) { bool used = false; for (auto& x : e->derived) used |= x.slot == (uint32_t)c; if (!used) slot = c; }
            if (slot < 0) return undo(INFX_ECAPACITY, "no scalar column slot is free for a list-column leaf");
            Pending p; p.lcol = lc; p.key = key; p.slot = (uint32_t)slot;
            p.empty = filt::list_leaf_table(L, e->listCols[(size_t)lc], p.words);
            pend.push_back(std::move(p));
            e->derived.push_back(infx_engine::DerivedCol{lc, key, (uint32_t)slot, 0u, tick});
            D = &e->derived.back();
        }
        D->lastUse = tick;
        slotOf[l] = (int)D->slot;
        bool seen = false; for (auto& r : refs) seen |= r.first == lc && r.second == key;
        if (!seen) refs.push_back({lc, key});
    }
    e->llBuilt = 0; e->llLaunches = 0;
    if (e->dev) for (size_t c = 0; c < e->listCols.size(); c++) {
        std::vector<std::vector<uint32_t>> tables; std::vector<uint32_t> slots; uint32_t emptyBits = 0;
        for (auto& p : pend) if (p.lcol == (int)c) { if (p.empty) emptyBits |= 1u << tables.size(); tables.push_back(p.words); slots.push_back(p.slot); }
        if (tables.empty()) continue;
        std::vector<uint32_t> maps; filt::list_leaf_maps(tables, (e->listCols[c].dict.dict.size() + 31) / 32, maps);
        if (maps.empty()) maps.push_back(0u);
        const int32_t rc = infx_list_leaf_build(e->dev, (uint32_t)c, (uint32_t)tables.size(), slots.data(), maps.data(), emptyBits);
        if (rc) { const std::string m = infx_last_error(); return undo(rc, m.c_str()); }
        e->llBuilt += (uint32_t)tables.size(); e->llLaunches++; e->llBuiltAll += tables.size(); e->llLaunchesAll++;
    }
    return INFX_OK;
}
// The compiled program of an Infiscript expression, from the engine's cache (parsed on first use; its device copy made on the first use that needs it:
// dev = true).  Caller holds e->filterMu.  Marks the entry most recently used; may evict others.
static int32_t compile_filter(infx_engine* e, const char* expr, CompiledFilter** out, bool dev) {
    auto it = e->filters.find(expr);
    if (it == e->filters.end()) {
        filt::Program P;
        try { P = filt::parse(expr); }
        catch (const filt::Unsupported& x) { return efail(INFX_EUNSUPPORTED, x.what()); }
        catch (const filt::SyntaxError& x) { return efail(INFX_EINVAL, std::string("filter syntax error: ") + x.what()); }
        CompiledFilter cf; std::vector<uint32_t> w;
        std::vector<int> derivedSlot;
        { int32_t rc = lower_list_leaves(e, P, derivedSlot, cf.derived); if (rc) return rc; }
        for (auto& in : P.code) cf.ops.push_back(infx_filter_op{in.op, in.arg});
        for (auto& L : P.leaves) {
            const int ds = derivedSlot[(size_t)(&L - P.leaves.data())];
            if (ds >= 0) {      // a list-column leaf: an ordinary leaf over its derived one-bit column, true for code 1
                cf.leaves.push_back(infx_filter_leaf{(uint32_t)ds, (uint32_t)cf.tables.size(), 2u, 0});
                cf.tables.push_back(2u);
                continue;
            }
            int ci = -1; for (size_t c = 0; c < e->columns.size(); c++) if (e->columns[c].name == L.field) ci = (int)c;      // field names are case sensitive (Dictionary<string, Field>)
            filt::leaf_table(L, ci >= 0 ? &e->columns[ci] : nullptr, w);
            cf.leaves.push_back(infx_filter_leaf{ci >= 0 ? (uint32_t)ci : 0xFFFFFFFFu, (uint32_t)cf.tables.size(), ci >= 0 ? (uint32_t)e->columns[ci].dict.size() : 1u, 0});
            cf.tables.insert(cf.tables.end(), w.begin(), w.end());
        }
        // what the device cannot run (more than INFX_FILTER_MAX_OPS ops, a stack deeper than 32) is refused here, for this expression alone — as a syntax
        // error is — on every path; checked only later, by the batch's program table or mask build, it would fail the whole batch
        if (e->dev) {
            int32_t rc = infx_filter_check(e->dev, (uint32_t)cf.ops.size(), cf.ops.data(), (uint32_t)cf.leaves.size(), cf.leaves.data(), (uint32_t)cf.tables.size());
            if (rc) { g_eerr = infx_last_error(); return rc; }
        }
        for (auto& k : cf.derived) for (auto& D : e->derived) if (D.lcol == k.first && D.key == k.second) D.refs++;
        e->filterLru.push_front(expr);
        it = e->filters.emplace(expr, std::move(cf)).first;
        it->second.lru = e->filterLru.begin();
        it->second.pins++;                // (held while the cache makes room)
        e->evict_filters();
        it->second.pins--;
    } else e->filterLru.splice(e->filterLru.begin(), e->filterLru, it->second.lru);
    CompiledFilter& cf = it->second;
    if (dev && !cf.dev) {
        int32_t rc = infx_filter_create(e->dev, (uint32_t)cf.ops.size(), cf.ops.data(), (uint32_t)cf.leaves.size(), cf.leaves.data(), (uint32_t)cf.tables.size(), cf.tables.data(), &cf.dev);
        if (rc) { g_eerr = infx_last_error(); return rc; }
    }
    *out = &cf;
    return INFX_OK;
}
static bool engine_sharded(const infx_engine* e) { return e->nranks > 1; }
// pins / unpins cache entries by expression (an entry evicted meanwhile — after retire_filters — is simply gone).  Caller holds e->filterMu.
static void pin_filters(infx_engine* e, const std::vector<std::string>& keys, int d) {
    for (auto& k : keys) { auto it = e->filters.find(k); if (it != e->filters.end()) it->second.pins = (uint32_t)std::max<int64_t>(0, (int64_t)it->second.pins + d); }
}
static void set_session_pins(infx_session* S, std::vector<std::string>& slot, std::vector<std::string> keys) {      // caller holds e->filterMu
    pin_filters(S->e, keys, +1); pin_filters(S->e, slot, -1); slot = std::move(keys); S->e->evict_filters();
}
// Installs Query.Filter (expr, UTF-8; NULL = none) and Query.EnableFacets on the session: every following search on it post-filters its rows
// on the device and counts the facetable fields.  n_in_filter = Filter.NumberOfDocumentsInFilter (this shard's share when sharded),
// counted on the device the first time the expression is used.  Status: INFX_EINVAL + message for a syntax error (FilterParseException),
// INFX_EUNSUPPORTED for MATCHES.
int32_t infx_engine_set_filter(infx_session* S, const char* expr, int32_t enable_facets, uint32_t* n_in_filter) {
    if (!S) return efail(INFX_EINVAL, "null session");
    infx_engine* e = S->e;
    if (!e->dev || !S->stream) return efail(INFX_EHIP, "no GPU: the post-filter runs on the device");
    if (S->qo.on && (expr || enable_facets)) return efail(INFX_EINVAL, "per-query options are installed on this session: a session-wide filter would conflict");
    if (S->qo.on) { if (n_in_filter) *n_in_filter = 0; return INFX_OK; }      // nothing session-wide is installed: clearing changes nothing (the batch's facet columns stay)
    infx_filter* dev = nullptr; uint32_t cnt = 0;
    std::vector<std::string> keep;
    {
        std::lock_guard<std::mutex> lk(e->filterMu);
        if (expr) {
            CompiledFilter* cf = nullptr;
            { int32_t rc = compile_filter(e, expr, &cf, true); if (rc) return rc; }
            if (!cf->counted) {       // ResultProcessor.cs:39-54: first use runs the filter over every document
                int32_t rc = infx_filter_count(S->stream, cf->dev, &cf->inFilter);
                if (rc) { g_eerr = infx_last_error(); return rc; }
                cf->counted = true;
                if (!engine_sharded(e)) { cf->inAll = cf->inFilter; cf->countedAll = true; }
            }
            dev = cf->dev; cnt = cf->inFilter;
            keep.push_back(expr);
        }
    }
    S->facetCols.clear();
    if (enable_facets) S->facetCols = facet_columns(e);
    int32_t rc = infx_stream_set_postfilter(S->stream, dev, (uint32_t)S->facetCols.size(), S->facetCols.data());
    if (rc) { g_eerr = infx_last_error(); return rc; }
    S->swFilter = expr != nullptr || enable_facets;
    { std::lock_guard<std::mutex> lk(e->filterMu); set_session_pins(S, S->swPinFilter, keep); }
    if (n_in_filter) *n_in_filter = cnt;
    return INFX_OK;
}
// Facets of query qi of the session's last search: for the k-th facetable column (engine column index in *col), up to cap (code, count) pairs ordered
// as FacetBuilder does (count descending, value ascending), at most 100.  Returns the number of pairs, -1 on error.
int32_t infx_engine_last_facets(infx_session* S, uint32_t nq, uint32_t qi, uint32_t k, int32_t* col, uint32_t* codes, uint32_t* counts, int32_t cap) {
    if (!S || !S->stream || qi >= nq || k >= S->facetCols.size()) return -1;
    std::vector<uint32_t> cd((size_t)S->e->postRows), ct(cd.size()); uint32_t n = 0;      // one (query, column) slice: at most the engine's post rows pairs
    if (infx_last_facets_of(S->stream, nq, qi, k, cd.data(), ct.data(), &n)) { g_eerr = infx_last_error(); return -1; }
    const filt::Column& C = S->e->columns[S->facetCols[k]];
    FacetPairs v;
    for (uint32_t i = 0; i < n; i++) v.push_back({cd[i], ct[i]});
    order_facets(C, v);
    if (col) *col = (int32_t)S->facetCols[k];
    return copy_pairs(v, codes, counts, cap);
}
int32_t infx_engine_facet_column_count(infx_session* S) { return S ? (int32_t)S->facetCols.size() : -1; }
// One column's value counts (one word per distinct value) as a facet list: the values that occur, ordered as the row facets are
static FacetPairs facet_list(const filt::Column& C, const uint32_t* counts) {
    FacetPairs v;
    for (uint32_t code = 0; code < C.dict.size(); code++) if (counts[code]) v.push_back({code, counts[code]});
    order_facets(C, v);
    return v;
}
// FacetBuilder.BuildFacetsFromAllDocuments (Core/FacetBuilder.cs:110-181): value counts of every facetable column over all documents that are not
// Deleted, one device pass for all columns (infx_facets_all); per column the values ordered count descending, value ascending, cut to 100, null and
// empty values left out — as infx_engine_last_facets orders the row facets.  *ncols = facetable columns; their lists: infx_engine_facets_all_column.
int32_t infx_engine_facets_all(infx_session* S, int32_t* ncols) {
    if (!S) return efail(INFX_EINVAL, "null session");
    infx_engine* e = S->e;
    if (!e->dev || !S->stream) return efail(INFX_EHIP, "no GPU: the facet counts run on the device");
    if (!e->indexed) return efail(INFX_EINVAL, "facets before index_documents");
    S->facAllCols.clear(); S->facAll.clear(); S->facAllListCols.clear(); S->facAllList.clear();
    size_t total = 0;
    S->facAllCols = facet_columns(e, &total);
    if (ncols) *ncols = (int32_t)S->facAllCols.size();
    // the facetable list columns: element occurrences among the documents that are not Deleted, one k_list_facets launch per column
    for (uint32_t lc : list_facet_columns(e)) {
        const filt::ListColumn& C = e->listCols[lc];
        std::vector<uint32_t> cnt(std::max<size_t>(C.dict.dict.size(), 1)); const uint8_t* all = nullptr;
        int32_t rc = infx_list_facets(S->stream, lc, 1, &all, cnt.data());
        if (rc) { g_eerr = infx_last_error(); S->facAllListCols.clear(); S->facAllList.clear(); return rc; }
        S->facAllListCols.push_back(lc); S->facAllList.push_back(facet_list(C.dict, cnt.data()));
    }
    if (S->facAllCols.empty()) return INFX_OK;
    std::vector<uint32_t> counts(std::max<size_t>(total, 1));
    int32_t rc = infx_facets_all(S->stream, (uint32_t)S->facAllCols.size(), S->facAllCols.data(), counts.data());
    if (rc) { g_eerr = infx_last_error(); S->facAllCols.clear(); return rc; }
    size_t o = 0;
    for (uint32_t col : S->facAllCols) {
        const filt::Column& C = e->columns[col];
        S->facAll.push_back(facet_list(C, counts.data() + o));
        o += C.dict.size();
    }
    return INFX_OK;
}
// The k-th facetable column of the session's last infx_engine_facets_all: engine column index in *col, up to cap (code, count) pairs; returns their
// number, -1 on error.
int32_t infx_engine_facets_all_column(infx_session* S, uint32_t k, int32_t* col, uint32_t* codes, uint32_t* counts, int32_t cap) {
    if (!S || k >= S->facAll.size() || (cap > 0 && (!codes || !counts))) return -1;
    if (col) *col = (int32_t)S->facAllCols[k];
    return copy_pairs(S->facAll[k], codes, counts, cap);
}

// The facetable list columns of the session's last infx_engine_facets_all (their number; -1: no session), and the k-th of them as infx_engine_facets_all_column
// gives a scalar column: list column index in *lcol, (element code, occurrences) pairs.
int32_t infx_engine_facets_all_list_column_count(infx_session* S) { return S ? (int32_t)S->facAllList.size() : -1; }
int32_t infx_engine_facets_all_list_column(infx_session* S, uint32_t k, int32_t* lcol, uint32_t* codes, uint32_t* counts, int32_t cap) {
    if (!S || k >= S->facAllList.size() || (cap > 0 && (!codes || !counts))) return -1;
    if (lcol) *lcol = (int32_t)S->facAllListCols[k];
    return copy_pairs(S->facAllList[k], codes, counts, cap);
}

// ---- Query.Boosts / Query.SortBy (SearchEngine.cs:355-359): ResultProcessor.ApplyBoosts / ApplySort on the device after the post-filter -------------
int32_t infx_engine_set_boosts(infx_session* S, uint32_t n, const char* const* exprs, const int32_t* strengths, int32_t enable) {
    if (!S || (enable && n && (!exprs || !strengths))) return efail(INFX_EINVAL, "bad boost arguments");
    infx_engine* e = S->e;
    if (!e->dev || !S->stream) return efail(INFX_EHIP, "no GPU: boosts run on the device");
    std::vector<infx_filter*> devs; std::vector<int32_t> st; std::vector<std::string> keep;
    if (S->qo.on && enable && n) return efail(INFX_EINVAL, "per-query options are installed on this session: session-wide boosts would conflict");
    if (enable) {       // SearchEngine.cs:355: only with EnableBoost; a Boost whose Filter is null is dropped (ResultProcessor.cs:84-85)
        uint32_t withFilter = 0;
        for (uint32_t i = 0; i < n; i++) withFilter += exprs[i] != nullptr;
        if (withFilter > INFX_MAX_BOOSTS) return efail(INFX_ECAPACITY, "more than INFX_MAX_BOOSTS (8) boosts with a filter");
        std::lock_guard<std::mutex> lk(e->filterMu);
        for (uint32_t i = 0; i < n; i++) {
            if (!exprs[i]) continue;
            CompiledFilter* cf = nullptr;
            int32_t rc = compile_filter(e, exprs[i], &cf, true);      // ApplyBoosts never counts NumberOfDocumentsInFilter
            if (rc) return rc;
            devs.push_back(cf->dev); st.push_back(strengths[i]); keep.push_back(exprs[i]);
        }
    }
    int32_t rc = infx_stream_set_boosts(S->stream, (uint32_t)devs.size(), devs.data(), st.data());
    if (rc) { g_eerr = infx_last_error(); return rc; }
    S->swBoost = !devs.empty();
    { std::lock_guard<std::mutex> lk(e->filterMu); set_session_pins(S, S->swPinBoosts, keep); }
    return INFX_OK;
}
// Column col's sort rank is on the device: built and uploaded on its first use, which leaves the rank in *built where the caller asks for it.
// Caller holds e->filterMu.
static int32_t sort_rank_on_device(infx_engine* e, uint32_t col, std::vector<uint32_t>* built = nullptr) {
    if (e->sortRanked.size() < e->columns.size()) e->sortRanked.resize(e->columns.size(), 0);
    if (e->sortRanked[col]) return INFX_OK;
    std::vector<uint32_t> rank; filt::sort_rank(e->columns[col], rank);
    int32_t rc = infx_upload_sort_rank(e->dev, col, (uint32_t)rank.size(), rank.data());
    if (rc) { g_eerr = infx_last_error(); return rc; }
    e->sortRanked[col] = 1;
    if (built) built->swap(rank);
    return INFX_OK;
}
// the column of a SortBy field (0xFFFFFFFF: no such field), its sort rank on the device.  Caller holds e->filterMu.
static int32_t sort_column(infx_engine* e, const char* field, uint32_t* out) {
    *out = (uint32_t)column_named(e, field);
    if (*out == 0xFFFFFFFFu && list_column_named(e, field) >= 0) return efail(INFX_EINVAL, std::string("sort_by: no scalar field named '") + field + "': it is a list column");
    return *out != 0xFFFFFFFFu ? sort_rank_on_device(e, *out) : INFX_OK;
}
int32_t infx_engine_set_sort(infx_session* S, const char* field, int32_t ascending) {
    if (!S) return efail(INFX_EINVAL, "null session");
    infx_engine* e = S->e;
    if (!e->dev || !S->stream) return efail(INFX_EHIP, "no GPU: sort-by runs on the device");
    if (S->qo.on && field) return efail(INFX_EINVAL, "per-query options are installed on this session: a session-wide sort would conflict");
    uint32_t col = 0xFFFFFFFFu;
    if (field) {
        std::lock_guard<std::mutex> lk(e->filterMu);
        int32_t rc = sort_column(e, field, &col); if (rc) return rc;
    }
    int32_t rc = infx_stream_set_sort(S->stream, col, ascending, field != nullptr);
    if (rc) { g_eerr = infx_last_error(); return rc; }
    S->swSort = field != nullptr;
    return INFX_OK;
}

// ---- per-query options (Search(Query) for a batch of Query objects, each with its own options) ---------------------------------------------------
// ---- the frame of the four per-query parts ("One frame behind the per-query parts") ----
// Part k is dropped: what it holds in the filter cache and on the stream is released
static void query_part_clear(infx_session* S, int k) {
    if (!S->parts[k]->on) return;
    auto unpin = [&](const std::vector<std::string>& pinned) { std::lock_guard<std::mutex> lk(S->e->filterMu); pin_filters(S->e, pinned, -1); S->e->evict_filters(); };
    switch (k) {
    case QP_OPTIONS:
        unpin(S->qo.pinned);
        if (S->stream) infx_stream_set_query_post(S->stream, 0, 0, nullptr, 0, nullptr, nullptr, 0, nullptr, 0, nullptr);
        S->qo = QueryOpts(); break;
    case QP_COVERAGE: S->qc = QueryCov(); break;
    case QP_PREFILTERS: unpin(S->qp.pinned); S->qp = QueryPre(); break;
    case QP_COLLAPSE: S->qk = QueryClp(); break;
    case QP_HIGHLIGHT: S->qh = QueryHl(); break;
    }
}
// The messages infx_engine_query_error reads, for a batch of nq queries: per query the first one among the parts installed for nq queries, in their fixed order
static void query_parts_publish(infx_session* S, uint32_t nq) {
    S->lastErr.assign(nq, std::string());
    for (const QueryPart* P : S->parts) if (P->on && P->nq == nq)
        for (uint32_t i = 0; i < nq; i++) if (S->lastErr[i].empty() && !P->err[i].empty()) S->lastErr[i] = P->err[i];
}
// The end of an installer: part k as the call leaves it (installed, or cleared: the messages keep their number) is published, its statuses are copied out
static int32_t query_part_installed(infx_session* S, int k, int32_t* out_status) {
    const QueryPart& P = *S->parts[k];
    query_parts_publish(S, P.on ? P.nq : (uint32_t)S->lastErr.size());
    if (P.on && out_status) std::copy(P.status.begin(), P.status.end(), out_status);
    return INFX_OK;
}
// A batch of nq queries is about to run on the session: every installed part must be for nq queries (one that is not is cleared, it alone), and the options'
// max_results must fit the call's row stride
static int32_t query_parts_check(infx_session* S, uint32_t nq, int32_t max_results) {
    for (int k = 0; k < QP_PARTS; k++) {
        if (!S->parts[k]->on) continue;
        if (S->parts[k]->nq != nq) { query_part_clear(S, k); return efail(INFX_EINVAL, std::string("the per-query ") + QUERY_PART_NAMES[k] + " were installed for a batch of another size"); }
        if (k == QP_OPTIONS && max_results > 0) for (uint32_t i = 0; i < nq; i++) if (!S->qo.reject[i] && S->qo.maxResults[i] > max_results) {
            query_part_clear(S, k); return efail(INFX_EINVAL, "a query's max_results exceeds the call's (the row stride)");
        }
    }
    return INFX_OK;
}
static void query_parts_unbind(infx_session* S) { for (int k = 0; k < QP_PARTS; k++) if (S->parts[k]->bound) query_part_clear(S, k); }
static void query_parts_bind(infx_session* S) { for (QueryPart* P : S->parts) P->bound = P->on; }
// The batch is done (ok: it succeeded): the expressions the options counted enter the cache, a query that a part refuses comes back empty with result flag bit 4,
// which queries were collapsed by which column, the messages of the batch; every part is consumed.  Returns the options' status.
static int32_t query_parts_finish(infx_session* S, uint32_t* out_counts, uint32_t* out_flags, bool ok) {
    S->lastClpCol.clear();
    if (!S->qh.on) { S->lastHlChars.clear(); S->lastHlQuery.clear(); }
    if (!S->qo.on && !S->qc.on && !S->qp.on && !S->qk.on && !S->qh.on) return INFX_OK;
    infx_engine* e = S->e;
    int32_t rc = INFX_OK;
    if (S->qo.on) {
        QueryOpts& Q = S->qo;
        S->lastInFilter.assign(Q.nq, 0); S->lastCounted = 0; S->lastCountLaunches = 0;
        if (ok) {
            // The counts come from the batch's own finalize: infx_stream_set_query_post resets the stream's count stats and only the finalize that consumes
            // the options sets them.  (The host phases refuse every query with a filter, so such a batch counts nothing.)
            uint32_t counted = 0, launches = 0;
            infx_last_filter_count_stats(S->stream, &counted, &launches);
            if (counted != Q.countExprs.size()) rc = efail(INFX_EINVAL, "the batch's NumberOfDocumentsInFilter counts did not come back with it");
            if (!rc) {
                S->lastCounted = counted; S->lastCountLaunches = launches;
                std::lock_guard<std::mutex> lk(e->filterMu);
                for (size_t k = 0; k < Q.countExprs.size(); k++) {
                    auto it = e->filters.find(Q.countExprs[k]);
                    if (it == e->filters.end()) continue;
                    it->second.inAll = Q.counts[k]; it->second.countedAll = true;
                    if (!engine_sharded(e)) { it->second.inFilter = Q.counts[k]; it->second.counted = true; }
                }
                for (uint32_t i = 0; i < Q.nq; i++) if (!Q.filterExpr[i].empty() && !Q.reject[i]) {
                    auto it = e->filters.find(Q.filterExpr[i]);
                    if (it != e->filters.end() && it->second.countedAll) S->lastInFilter[i] = it->second.inAll;
                }
            }
        }
    }
    uint32_t nq = 0;
    for (const QueryPart* P : S->parts) {
        if (!P->on) continue;
        if (!nq) nq = P->nq;
        if (ok) for (uint32_t i = 0; i < P->nq; i++) if (P->reject[i]) { if (out_counts) out_counts[i] = 0; if (out_flags) out_flags[i] |= INFX_RESULT_REJECTED; }
        if (P == &S->qo) ok = ok && rc == INFX_OK;      // a batch whose options fail counts as failed for the parts after them
    }
    if (S->qk.on) {      // (after the loop: a query any part refused was not collapsed)
        const QueryClp& Q = S->qk;
        S->lastClpCol.assign(Q.nq, -1);
        for (uint32_t i = 0; i < Q.nq; i++) if (ok && Q.has[i] && !Q.reject[i] && !(out_flags && (out_flags[i] & INFX_RESULT_REJECTED))) S->lastClpCol[i] = Q.col[i];
    }
    if (S->qh.on) {      // (likewise: lastHlChars holds what stage_highlight installed; a query any part refused, or a failed batch, has no highlights)
        const QueryHl& Q = S->qh;
        S->lastHlChars.resize(Q.nq, 0); S->lastHlQuery.resize(Q.nq);
        for (uint32_t i = 0; i < Q.nq; i++) if (!ok || !Q.asks(i) || (out_flags && (out_flags[i] & INFX_RESULT_REJECTED))) S->lastHlChars[i] = 0;
    }
    query_parts_publish(S, nq);
    for (int k = 0; k < QP_PARTS; k++) query_part_clear(S, k);
    return rc;
}
int32_t infx_engine_set_query_options(infx_session* S, uint32_t nq, const infx_query_options* opts, int32_t* out_status) {
    if (!S || (nq && !opts)) return efail(INFX_EINVAL, "null argument");
    infx_engine* e = S->e;
    query_part_clear(S, QP_OPTIONS);
    if (nq == 0) return query_part_installed(S, QP_OPTIONS, nullptr);
    if (!e->dev || !S->stream) return efail(INFX_EHIP, "no GPU: the per-query options run on the device");
    if (S->swFilter || S->swBoost || S->swSort) return efail(INFX_EINVAL, "a session-wide filter, facets, boosts or sort is installed on this session: per-query options would conflict");
    QueryOpts Q; Q.open(nq);
    Q.maxResults.assign(nq, 0); Q.cov.assign(nq, 0); Q.facets.assign(nq, 0); Q.filterExpr.assign(nq, std::string());
    std::vector<infx_query_post> post(nq); std::vector<infx_query_boost> boosts;
    std::vector<const CompiledFilter*> progs; std::unordered_map<std::string, int32_t> progIdx;
    std::vector<uint32_t> facetCols = facet_columns(e);
    bool anyFacets = false;
    std::lock_guard<std::mutex> lk(e->filterMu);
    // per query: compile what it uses (a failure rejects that query alone); the table's programs to count come first
    struct QUse { std::string filter; std::vector<std::pair<std::string, int32_t>> boosts; uint32_t sortCol = 0xFFFFFFFFu; bool sort = false; };
    std::vector<QUse> use(nq);
    std::vector<std::string> toCount; std::unordered_set<std::string> toCountSet, all;
    auto hold = [&](const char* x) { if (all.insert(x).second) { Q.pinned.push_back(x); pin_filters(e, {std::string(x)}, +1); } };      // pinned as compiled: a small cache bound cannot evict the batch's own
    for (uint32_t i = 0; i < nq; i++) {
        const infx_query_options& O = opts[i]; QUse& U = use[i];
        Q.maxResults[i] = O.max_results; Q.cov[i] = O.enable_coverage ? 1 : 0;
        if (O.max_results < 1) { Q.refuse(i, INFX_EINVAL, "MaxNumberOfRecordsToReturn must be at least 1"); continue; }
        int32_t rc = INFX_OK;
        if (O.filter) { CompiledFilter* cf = nullptr; rc = compile_filter(e, O.filter, &cf, false); if (!rc) { U.filter = O.filter; hold(O.filter); } }
        if (!rc && O.enable_boost && O.nboosts) {
            uint32_t withFilter = 0;
            for (uint32_t b = 0; b < O.nboosts; b++) withFilter += O.boost_filters && O.boost_filters[b] != nullptr;
            if (!O.boost_filters || !O.boost_strengths) rc = efail(INFX_EINVAL, "bad boost arguments");
            else if (withFilter > INFX_MAX_BOOSTS) rc = efail(INFX_ECAPACITY, "more than INFX_MAX_BOOSTS (8) boosts with a filter");
            for (uint32_t b = 0; !rc && b < O.nboosts; b++) {
                if (!O.boost_filters[b]) continue;          // a Boost whose Filter is null is dropped (ResultProcessor.cs:84-85)
                CompiledFilter* cf = nullptr; rc = compile_filter(e, O.boost_filters[b], &cf, false);
                if (!rc) { U.boosts.push_back({O.boost_filters[b], O.boost_strengths[b]}); hold(O.boost_filters[b]); }
            }
        }
        if (!rc && O.sort_by) { U.sort = true; rc = sort_column(e, O.sort_by, &U.sortCol); }
        if (rc) { Q.refuse(i, rc, g_eerr); U = QUse(); continue; }
        const bool pp = O.filter || (O.enable_facets && !facetCols.empty()) || !U.boosts.empty() || U.sort;      // (facets without a facetable field: {} as the session path)
        if (pp && host_phases()) { Q.refuse(i, INFX_EUNSUPPORTED, "filter / facets / boosts / sort-by run in the device finalize: the host phases (INFX_PHASED) do not post-process rows"); U = QUse(); continue; }
        if (pp && O.max_results > e->postRows) {
            Q.refuse(i, INFX_EUNSUPPORTED, e->postRows == INFX_FILTER_MAX_ROWS ? std::string("filter / facets / boosts / sort-by run on at most INFX_FILTER_MAX_ROWS (64) returned rows per query")
                                                                               : "filter / facets / boosts / sort-by run on at most " + std::to_string(e->postRows) + " returned rows per query (the engine's post rows)");
            U = QUse(); continue;
        }
        if (O.enable_facets && !facetCols.empty()) anyFacets = true;
        if (!U.filter.empty()) {
            Q.filterExpr[i] = U.filter;
            const CompiledFilter& cf = e->filters.at(U.filter);
            if (!cf.countedAll && toCountSet.insert(U.filter).second) toCount.push_back(U.filter);      // ResultProcessor.cs:39-54: first use counts
        }
    }
    // the program table: the expressions to count, then every other one the batch uses; each entry pinned until the batch is done
    for (auto& x : toCount) { progIdx[x] = (int32_t)progs.size(); progs.push_back(&e->filters.at(x)); }
    for (auto& x : Q.pinned) if (!progIdx.count(x)) { progIdx[x] = (int32_t)progs.size(); progs.push_back(&e->filters.at(x)); }
    for (uint32_t i = 0; i < nq; i++) {
        const QUse& U = use[i]; infx_query_post& D = post[i];
        D = infx_query_post{}; D.filter = U.filter.empty() ? -1 : progIdx.at(U.filter);
        if (!Q.reject[i] && opts[i].enable_facets && anyFacets) { D.flags |= INFX_QP_FACETS; Q.facets[i] = 1; }
        D.boost_off = (uint32_t)boosts.size(); D.nboost = (uint32_t)U.boosts.size();
        for (auto& b : U.boosts) boosts.push_back(infx_query_boost{progIdx.at(b.first), b.second});
        if (U.sort) { D.flags |= INFX_QP_SORT | (opts[i].sort_ascending ? INFX_QP_ASC : 0u); D.sort_col = U.sortCol; }
    }
    std::vector<infx_filter_prog> P(progs.size());
    for (size_t k = 0; k < progs.size(); k++) P[k] = prog_of(*progs[k]);
    Q.countExprs = toCount; Q.counts.assign(toCount.size(), 0u);
    if (!anyFacets) facetCols.clear();
    int32_t rc = infx_stream_set_query_post(S->stream, nq, (uint32_t)P.size(), P.data(), (uint32_t)boosts.size(), boosts.data(), post.data(),
                                            (uint32_t)facetCols.size(), facetCols.data(), (uint32_t)toCount.size(), Q.counts.data());
    if (rc) { g_eerr = infx_last_error(); pin_filters(e, Q.pinned, -1); return rc; }
    S->facetCols = facetCols;
    Q.on = true;
    S->qo = std::move(Q);
    return query_part_installed(S, QP_OPTIONS, out_status);
}
int32_t infx_engine_last_in_filter(infx_session* S, uint32_t nq, uint32_t* out) {
    if (!S || (nq && !out)) return efail(INFX_EINVAL, "null argument");
    if (nq != S->lastInFilter.size()) return efail(INFX_EINVAL, "no per-query batch of this size on the session");
    std::memcpy(out, S->lastInFilter.data(), (size_t)nq * 4);
    return INFX_OK;
}
int32_t infx_engine_last_count_stats(infx_session* S, uint32_t* counted, uint32_t* launches) {
    if (!S) return efail(INFX_EINVAL, "null session");
    return put_stats({{counted, S->lastCounted}, {launches, S->lastCountLaunches}});
}
int32_t infx_engine_last_browse_stats(infx_session* S, uint32_t* groups, uint32_t* launches) {
    if (!S) return efail(INFX_EINVAL, "null session");
    if (!S->stream) return efail(INFX_EHIP, "no GPU: browse queries run on the device");
    int32_t rc = infx_last_browse_stats(S->stream, groups, launches);
    if (rc) g_eerr = infx_last_error();
    return rc;
}
int32_t infx_engine_query_error(infx_session* S, uint32_t qi, char* out, int32_t cap) {
    if (!S || qi >= S->lastErr.size()) return -1;
    return copy_message(S->lastErr[qi], out, cap);
}
// ---- CoverageSetup: engine-wide (SearchEngine's coverageSetup: argument) and per query (Query.CoverageSetup) -----------------------------------------
static const infx_coverage_setup COVERAGE_SETUP_DEFAULT = {2, 20, 2, 3, 7, 1, 0, 5, 0.2, 1, 1, 1, 1, 1, 1, 0, 254};
// nullptr = acceptable; else what is wrong.  *status: INFX_EINVAL, or INFX_EUNSUPPORTED for the lexical pre-screen.
static const char* coverage_setup_problem(const infx_coverage_setup& c, int32_t* status) {
    *status = INFX_EINVAL;
    const int32_t ints[8] = {c.min_word_size, c.levenshtein_max_word_size, c.num_typos, c.min_length_one_typo, c.min_length_two_typos,
                             c.coverage_min_word_hits_abs, c.coverage_min_word_hits_relative, c.coverage_q_limit_for_error_tolerance};
    for (int32_t v : ints) if (v < 0 || v > 65535) return "CoverageSetup: an integer member lies outside [0, 65535]";
    if (c.truncation_score < 0 || c.truncation_score > 255) return "CoverageSetup: TruncationScore lies outside [0, 255]";
    if (!std::isfinite(c.coverage_lcs_error_tolerance_relativeq) || c.coverage_lcs_error_tolerance_relativeq < 0.0) return "CoverageSetup: CoverageLcsErrorToleranceRelativeq must be finite and not negative";
    if (c.enable_lexical_prescreen) { *status = INFX_EUNSUPPORTED; return "CoverageSetup.EnableLexicalPrescreen is not implemented"; }
    return nullptr;
}
int32_t infx_coverage_setup_default(infx_coverage_setup* out) { if (!out) return efail(INFX_EINVAL, "null argument"); *out = COVERAGE_SETUP_DEFAULT; return INFX_OK; }
int32_t infx_sizeof_coverage_setup(void) { return (int32_t)sizeof(infx_coverage_setup); }
int32_t infx_engine_set_coverage_setup(infx_engine* e, const infx_coverage_setup* setup) {
    if (!e) return efail(INFX_EINVAL, "null engine");
    const infx_coverage_setup c = setup ? *setup : COVERAGE_SETUP_DEFAULT;
    int32_t st = INFX_OK;
    if (const char* why = coverage_setup_problem(c, &st)) return efail(st, why);
    e->cs = c;
    HostConfig& h = e->ix.cfg;
    h.covMinWordSize = c.min_word_size; h.coverPrefixSuffix = c.cover_prefix_suffix != 0;
    h.covQLimit = c.coverage_q_limit_for_error_tolerance; h.covRelativeq = c.coverage_lcs_error_tolerance_relativeq;
    return INFX_OK;
}
// Post rows: how many returned rows per query filter / facets / boosts / sort-by / browse accept.  Fixed once a search has begun: sessions size their
// facet readout by it.
int32_t infx_engine_set_post_rows(infx_engine* e, int32_t rows) {
    if (!e) return efail(INFX_EINVAL, "null engine");
    if (rows < INFX_FILTER_MAX_ROWS || rows > INFX_POST_MAX_ROWS) return efail(INFX_EINVAL, "post rows lie outside [64, 1024]");
    if (e->searched.load(std::memory_order_relaxed)) return efail(INFX_EINVAL, "the post rows are set between create and the first search");
    if (e->dev) { int32_t rc = infx_set_post_rows(e->dev, rows); if (rc) { g_eerr = infx_last_error(); return rc; } }
    e->postRows = rows;
    return INFX_OK;
}
int32_t infx_engine_get_post_rows(infx_engine* e, int32_t* out) { if (!e || !out) return efail(INFX_EINVAL, "null argument"); *out = e->postRows; return INFX_OK; }
int32_t infx_engine_get_coverage_setup(infx_engine* e, infx_coverage_setup* out) { if (!e || !out) return efail(INFX_EINVAL, "null argument"); *out = e->cs; return INFX_OK; }
static infx_finalize_setup finalize_of(const infx_coverage_setup& c) {
    infx_finalize_setup f; f.truncate = c.truncate != 0; f.min_hits_abs = c.coverage_min_word_hits_abs; f.min_hits_relative = c.coverage_min_word_hits_relative; f.truncation_score = c.truncation_score;
    return f;
}
static inline infx_finalize_setup qc_finalize(const infx_session* S, size_t i) { return S->qc.on && i < S->qc.nq ? S->qc.fin[i] : finalize_of(S->e->cs); }
static inline int32_t qc_tolerance(const infx_session* S, size_t i, int len) {
    const HostConfig& h = S->e->ix.cfg;
    return S->qc.on && i < S->qc.nq ? cov_lcs_tolerance(len, S->qc.qLimit[i], S->qc.relativeq[i]) : cov_lcs_tolerance(len, h.covQLimit, h.covRelativeq);
}
int32_t infx_engine_set_query_coverage(infx_session* S, uint32_t nq, const infx_coverage_setup* const* setups, int32_t* out_status) {
    if (!S || (nq && !setups)) return efail(INFX_EINVAL, "null argument");
    query_part_clear(S, QP_COVERAGE);
    if (nq == 0) return query_part_installed(S, QP_COVERAGE, nullptr);
    QueryCov Q; Q.open(nq);
    Q.fin.assign(nq, finalize_of(S->e->cs)); Q.qLimit.assign(nq, S->e->ix.cfg.covQLimit); Q.relativeq.assign(nq, S->e->ix.cfg.covRelativeq);
    for (uint32_t i = 0; i < nq; i++) {
        if (!setups[i]) continue;
        const infx_coverage_setup& c = *setups[i];
        int32_t st = INFX_OK;
        if (const char* why = coverage_setup_problem(c, &st)) { Q.refuse(i, st, why); continue; }
        // Only what SearchPipeline reads; the matcher members stay the engine's (quirk Q19)
        Q.fin[i] = finalize_of(c); Q.qLimit[i] = c.coverage_q_limit_for_error_tolerance; Q.relativeq[i] = c.coverage_lcs_error_tolerance_relativeq;
    }
    Q.on = true;
    S->qc = std::move(Q);
    return query_part_installed(S, QP_COVERAGE, out_status);
}
// The stream's next Stage-2 call gets the engine-wide matcher settings, its next finalize the per-query truncation records (deviceFinalize: the batch is
// finalized by k_finalize; the host phases apply the same values in ph_finalize).  Defaults everywhere: nothing is staged.
static int32_t stage_coverage_setup(infx_session* S, uint32_t nq, bool deviceFinalize) {
    if (!S->stream) return INFX_OK;
    const infx_coverage_setup& c = S->e->cs;
    infx_stage2_setup m;
    m.min_word_size = c.min_word_size; m.lev_max_word_size = c.levenshtein_max_word_size; m.num_typos = c.num_typos;
    m.min_len_one_typo = c.min_length_one_typo; m.min_len_two_typos = c.min_length_two_typos;
    m.cover_whole_query = c.cover_whole_query; m.cover_whole_words = c.cover_whole_words; m.cover_fuzzy_words = c.cover_fuzzy_words;
    m.cover_joined_words = c.cover_joined_words; m.cover_prefix_suffix = c.cover_prefix_suffix;
    const infx_finalize_setup engineFin = finalize_of(c);
    static const infx_finalize_setup defFin = finalize_of(COVERAGE_SETUP_DEFAULT);
    std::vector<infx_finalize_setup> fin;
    if (deviceFinalize && nq) {
        if (S->qc.on && S->qc.nq == nq) fin = S->qc.fin;
        else if (std::memcmp(&engineFin, &defFin, sizeof defFin) != 0) fin.assign(nq, engineFin);
    }
    int32_t rc = infx_stream_set_coverage(S->stream, &m, (uint32_t)fin.size(), fin.empty() ? nullptr : fin.data());
    if (rc) g_eerr = infx_last_error();
    return rc;
}

// ---- Query.pre_filter: rank only the documents a filter accepts -----------------------------------------------------------------------------------------
// A query with a pre-filter P returns what it would return if every document P does not accept carried Document.Deleted (include/infidex_hip.h, "pre-filter
// masks").  The masks live per session, in the mask slots of its stream: at most INFX_MAX_PREFILTERS, keyed by the expression, least recently used first out,
// valid for one mask epoch of the engine.
int32_t infx_engine_set_query_prefilters(infx_session* S, uint32_t nq, const char* const* exprs, int32_t* out_status) {
    if (!S || (nq && !exprs)) return efail(INFX_EINVAL, "null argument");
    infx_engine* e = S->e;
    query_part_clear(S, QP_PREFILTERS);
    if (nq == 0) return query_part_installed(S, QP_PREFILTERS, nullptr);
    if (!e->dev || !S->stream) return efail(INFX_EHIP, "no GPU: the pre-filter masks are built on the device");
    QueryPre Q; Q.open(nq);
    Q.expr.assign(nq, std::string()); Q.has.assign(nq, 0);
    {
        std::lock_guard<std::mutex> lk(e->filterMu);
        std::unordered_set<std::string> distinct;
        for (uint32_t i = 0; i < nq; i++) {
            if (!exprs[i]) continue;
            Q.has[i] = 1;
            if (engine_sharded(e)) { Q.refuse(i, INFX_EUNSUPPORTED, "a pre-filter needs an engine that is not sharded: the masks cover one device's documents"); continue; }
            if (host_phases()) { Q.refuse(i, INFX_EUNSUPPORTED, "a pre-filter runs in the device pipeline: the host phases (INFX_PHASED) do not read the masks"); continue; }
            CompiledFilter* cf = nullptr;
            const int32_t rc = compile_filter(e, exprs[i], &cf, false);      // syntax error: INFX_EINVAL; MATCHES: INFX_EUNSUPPORTED
            if (rc) { Q.refuse(i, rc, g_eerr); continue; }
            if (!distinct.count(exprs[i])) {
                if (distinct.size() >= INFX_MAX_PREFILTERS) { Q.refuse(i, INFX_ECAPACITY, "more than INFX_MAX_PREFILTERS (16) distinct pre-filters in one batch; split the batch"); continue; }
                distinct.insert(exprs[i]); Q.pinned.push_back(exprs[i]); pin_filters(e, {std::string(exprs[i])}, +1);
            }
            Q.expr[i] = exprs[i];
        }
    }
    Q.on = true;
    S->qp = std::move(Q);
    return query_part_installed(S, QP_PREFILTERS, out_status);
}
// ---- Query.collapse_by: at most collapse_keep ranked rows per group ------------------------------------------------------------------------------------
// (include/infidex_engine.h, "collapse_by"; the step itself is the device library's: include/infidex_hip.h, "collapsing")
int32_t infx_engine_set_query_collapse(infx_session* S, uint32_t nq, const char* const* fields, const int32_t* keeps, int32_t* out_status) {
    if (!S || (nq && fields && !keeps)) return efail(INFX_EINVAL, "null argument");
    infx_engine* e = S->e;
    query_part_clear(S, QP_COLLAPSE);
    if (nq == 0 || !fields) return query_part_installed(S, QP_COLLAPSE, nullptr);
    QueryClp Q; Q.open(nq);
    Q.col.assign(nq, -1); Q.keep.assign(nq, 1); Q.has.assign(nq, 0);
    {
        std::lock_guard<std::mutex> lk(e->filterMu);
        for (uint32_t i = 0; i < nq; i++) {
            if (!fields[i]) continue;
            Q.has[i] = 1;
            const int32_t col = column_named(e, fields[i]);
            if (col < 0) { Q.refuse(i, INFX_EINVAL, std::string("collapse_by: no field named '") + fields[i] + "'"); continue; }
            if (keeps[i] < 1 || keeps[i] > INFX_COLLAPSE_MAX_KEEP) { Q.refuse(i, INFX_EINVAL, "collapse_keep is 1 .. 16 rows per group"); continue; }
            if (engine_sharded(e)) { Q.refuse(i, INFX_EUNSUPPORTED, "collapse_by needs an engine that is not sharded: the ranked list is folded on one device"); continue; }
            if (host_phases()) { Q.refuse(i, INFX_EUNSUPPORTED, "collapse_by runs in the device pipeline: the host phases (INFX_PHASED) do not fold the ranked list"); continue; }
            if (!e->dev || !S->stream) { Q.refuse(i, INFX_EHIP, "no GPU: the ranked list is folded on the device"); continue; }
            Q.col[i] = col; Q.keep[i] = keeps[i];
        }
    }
    Q.on = true;
    S->qk = std::move(Q);
    return query_part_installed(S, QP_COLLAPSE, out_status);
}
// Before the batch's infx_search_fused: refuses collapse_by on a browse query, installs each query's request on the stream
static int32_t stage_collapse(infx_session* S, uint32_t nq, std::vector<infx_fused_query>& fq) {
    QueryClp& Q = S->qk;
    if (!Q.on || Q.nq != nq) return INFX_OK;
    std::vector<infx_collapse_req> reqs(nq, infx_collapse_req{-1, 1}); bool any = false;
    for (uint32_t i = 0; i < nq; i++) {
        if (!Q.has[i] || Q.reject[i]) continue;
        if (fq[i].flags & INFX_FQ_BROWSE) {      // empty text + EnableFacets: nothing is ranked
            Q.refuse(i, INFX_EUNSUPPORTED, "collapse_by does not apply to a browse query (empty text with EnableFacets): nothing is ranked; list_groups lists one row per group");
            fq[i].flags &= ~INFX_FQ_BROWSE;
            continue;
        }
        reqs[i] = infx_collapse_req{Q.col[i], Q.keep[i]}; any = true;
    }
    if (!any) return INFX_OK;
    const int32_t rc = infx_stream_set_query_collapse(S->stream, nq, reqs.data());
    if (rc) g_eerr = infx_last_error();
    return rc;
}
int32_t infx_engine_last_collapse(infx_session* S, uint32_t nq, uint32_t* total_groups, uint32_t* total_ranked) {
    if (!S || (nq && (!total_groups || !total_ranked))) return efail(INFX_EINVAL, "null argument");
    if (nq != S->lastClpCol.size()) return efail(INFX_EINVAL, "no batch of this size with collapse requests on the session");
    bool any = false; for (int32_t c : S->lastClpCol) any |= c >= 0;
    if (any) { const int32_t rc = infx_last_collapse(S->stream, nq, total_groups, total_ranked); if (rc) { g_eerr = infx_last_error(); return rc; } }
    for (uint32_t i = 0; i < nq; i++) if (S->lastClpCol[i] < 0) total_groups[i] = total_ranked[i] = 0;
    return INFX_OK;
}
int32_t infx_engine_collapse_rows(infx_session* S, uint32_t qi, int32_t* col, uint32_t* codes, uint32_t* sizes, int32_t cap) {
    if (!S || qi >= S->lastClpCol.size() || S->lastClpCol[qi] < 0 || !S->stream) { efail(INFX_EINVAL, "no collapsed query of this index in the session's last batch"); return -1; }
    if (col) *col = S->lastClpCol[qi];
    const int32_t n = infx_collapse_rows(S->stream, qi, codes, sizes, cap);
    if (n < 0) g_eerr = infx_last_error();
    return n;
}
int32_t infx_engine_last_collapse_stats(infx_session* S, uint32_t* queries, uint32_t* launches) {
    if (!S) return efail(INFX_EINVAL, "null session");
    if (!S->stream) return put_stats({{queries, 0u}, {launches, 0u}});
    const int32_t rc = infx_last_collapse_stats(S->stream, queries, launches);
    if (rc) g_eerr = infx_last_error();
    return rc;
}
int32_t infx_engine_last_collapse_timings(infx_session* S, float* ms2) {
    if (!S || !ms2) return efail(INFX_EINVAL, "null argument");
    ms2[0] = ms2[1] = 0.f;
    if (!S->stream) return INFX_OK;
    const int32_t rc = infx_last_collapse_timings(S->stream, ms2);
    if (rc) g_eerr = infx_last_error();
    return rc;
}
// ---- Query.highlight: match spans and a snippet for every returned row ---------------------------------------------------------------------------------
// (include/infidex_engine.h, "highlight"; the step itself is the device library's: include/infidex_hip.h, "highlighting")
int32_t infx_engine_set_query_highlight(infx_session* S, uint32_t nq, const int32_t* chars, int32_t* out_status) {
    if (!S) return efail(INFX_EINVAL, "null argument");
    infx_engine* e = S->e;
    query_part_clear(S, QP_HIGHLIGHT);
    if (nq == 0 || !chars) return query_part_installed(S, QP_HIGHLIGHT, nullptr);
    QueryHl Q; Q.open(nq);
    Q.chars.assign(nq, 0); Q.has.assign(nq, 0);
    for (uint32_t i = 0; i < nq; i++) {
        if (chars[i] == 0) continue;
        Q.has[i] = 1;
        if (chars[i] < INFX_HIGHLIGHT_MIN_CHARS || chars[i] > INFX_HIGHLIGHT_MAX_CHARS) { Q.refuse(i, INFX_EINVAL, "highlight_chars is 16 .. 512 UTF-16 units"); continue; }
        if (engine_sharded(e)) { Q.refuse(i, INFX_EUNSUPPORTED, "highlight needs an engine that is not sharded: the returned rows are highlighted on one device"); continue; }
        if (host_phases()) { Q.refuse(i, INFX_EUNSUPPORTED, "highlight runs in the device pipeline: the host phases (INFX_PHASED) do not highlight the returned rows"); continue; }
        if (!e->dev || !S->stream) { Q.refuse(i, INFX_EHIP, "no GPU: the returned rows are highlighted on the device"); continue; }
        Q.chars[i] = chars[i];
    }
    Q.on = true;
    S->qh = std::move(Q);
    return query_part_installed(S, QP_HIGHLIGHT, out_status);
}
// Before the batch's infx_search_fused: refuses highlight on a browse query, installs each query's width on the stream, keeps each asking query's words
static int32_t stage_highlight(infx_session* S, uint32_t nq, std::vector<infx_fused_query>& fq, const FusedIn& FI) {
    QueryHl& Q = S->qh;
    S->lastHlChars.assign(nq, 0); S->lastHlQuery.assign(nq, HlQuery());
    if (!Q.on || Q.nq != nq) return INFX_OK;
    bool any = false;
    for (uint32_t i = 0; i < nq; i++) {
        if (!Q.asks(i)) continue;
        if (fq[i].flags & INFX_FQ_BROWSE) {      // empty text + EnableFacets: nothing was matched
            Q.refuse(i, INFX_EUNSUPPORTED, "highlight does not apply to a browse query (empty text with EnableFacets): nothing was matched");
            fq[i].flags &= ~INFX_FQ_BROWSE;
            continue;
        }
        S->lastHlChars[i] = Q.chars[i]; any = true;
        const infx_cov_query& c = FI.cq[i]; HlQuery& H = S->lastHlQuery[i];
        H.longQuery = c.reserved != 0;
        if (!H.longQuery) {
            const int32_t n = std::min(std::max(c.num_tokens, 0), (int32_t)INFX_MAX_QUERY_TOKENS);
            H.text.assign(c.text, c.text + std::min(std::max(c.text_len, 0), (int32_t)INFX_MAX_QUERY_CHARS));
            H.off.assign(c.tok_off, c.tok_off + n); H.len.assign(c.tok_len, c.tok_len + n);
        }
    }
    if (!any) return INFX_OK;
    const int32_t rc = infx_stream_set_query_highlight(S->stream, nq, S->lastHlChars.data());
    if (rc) g_eerr = infx_last_error();
    return rc;
}
static const HlQuery* highlighted(infx_session* S, uint32_t qi) {
    if (!S || qi >= S->lastHlChars.size() || S->lastHlChars[qi] == 0 || qi >= S->lastHlQuery.size() || !S->stream) { efail(INFX_EINVAL, "no highlighted query of this index in the session's last batch"); return nullptr; }
    return &S->lastHlQuery[qi];
}
int32_t infx_engine_highlight_query(infx_session* S, uint32_t qi, int32_t* rows, int32_t* term_stride, int32_t* snippet_stride, int32_t* long_query,
                                    uint16_t* text, int32_t* text_len, uint16_t* word_off, uint16_t* word_len, int32_t* words) {
    const HlQuery* H = highlighted(S, qi);
    if (!H) return INFX_EINVAL;
    const int32_t rc = infx_highlight_layout(S->stream, qi, rows, term_stride, snippet_stride);
    if (rc) { g_eerr = infx_last_error(); return rc; }
    if (long_query) *long_query = H->longQuery ? 1 : 0;
    if (text) std::copy(H->text.begin(), H->text.end(), text);
    if (text_len) *text_len = (int32_t)H->text.size();
    if (word_off) std::copy(H->off.begin(), H->off.end(), word_off);
    if (word_len) std::copy(H->len.begin(), H->len.end(), word_len);
    if (words) *words = (int32_t)H->off.size();
    return INFX_OK;
}
int32_t infx_engine_highlight_rows(infx_session* S, uint32_t qi, uint16_t* out, int64_t cap_u16) {
    if (!highlighted(S, qi)) return -1;
    const int32_t n = infx_highlight_rows(S->stream, qi, out, cap_u16);
    if (n < 0) g_eerr = infx_last_error();
    return n;
}
int32_t infx_engine_last_highlight_stats(infx_session* S, uint32_t* queries, uint32_t* launches) {
    if (!S) return efail(INFX_EINVAL, "null session");
    if (!S->stream) return put_stats({{queries, 0u}, {launches, 0u}});
    const int32_t rc = infx_last_highlight_stats(S->stream, queries, launches);
    if (rc) g_eerr = infx_last_error();
    return rc;
}
int32_t infx_engine_last_highlight_timings(infx_session* S, float* ms, uint64_t* bytes) {
    if (!S || !ms) return efail(INFX_EINVAL, "null argument");
    *ms = 0.f; if (bytes) *bytes = 0;
    if (!S->stream) return INFX_OK;
    const int32_t rc = infx_last_highlight_timings(S->stream, ms, bytes);
    if (rc) g_eerr = infx_last_error();
    return rc;
}
// The host's copy of what Stage 2 reads of document `document_index` (an internal index): lower(normalize(IndexedText)), UTF-16.  Returns its length in units
// (copies at most cap of them), -1 on error.
int64_t infx_engine_document_text(infx_engine* e, int64_t document_index, uint16_t* out, int64_t cap) {
    if (!e || cap < 0 || (cap && !out)) { efail(INFX_EINVAL, "null argument"); return -1; }
    const HostIndex& ix = e->ix;
    if (!e->indexed || document_index < 0 || document_index >= (int64_t)ix.N || ix.textOff.size() != (size_t)ix.N + 1) { efail(INFX_EINVAL, "no document of this index"); return -1; }
    const uint64_t b = ix.textOff[document_index], n = ix.textOff[document_index + 1] - b;
    std::copy(ix.text.begin() + b, ix.text.begin() + b + std::min<uint64_t>(n, (uint64_t)cap), out);
    return (int64_t)n;
}
static void unstage_prefilters(infx_session* S, const std::vector<int>& builtSlots) {
    for (int b : builtSlots) S->preMask[b].valid = false;
    if (S->stream) { infx_filter_masks(S->stream, 0, nullptr, nullptr, nullptr); infx_stream_set_doc_masks(S->stream, 0, nullptr); }
}
void MaskCall::add(uint32_t i, const std::string& expr) {
    auto it = idx.find(expr);
    if (it == idx.end()) { it = idx.emplace(expr, (int)exprs.size()).first; exprs.push_back(expr); }
    of[i] = it->second;
}
int32_t MaskCall::intern(uint32_t i, const char* expr) {
    CompiledFilter* cf = nullptr;
    if (!idx.count(expr)) { const int32_t rc = compile_filter(S->e, expr, &cf, false); if (rc) return rc; }      // syntax error: INFX_EINVAL; MATCHES: INFX_EUNSUPPORTED
    add(i, expr);
    return INFX_OK;
}
int32_t MaskCall::failed(int32_t rc) {
    g_eerr = infx_last_error(); unstage_prefilters(S, built); built.clear(); release();
    return rc;
}
void MaskCall::release() {
    if (pinned.empty()) return;
    infx_engine* e = S->e;
    if (locked) { pin_filters(e, pinned, -1); e->evict_filters(); }
    else { std::lock_guard<std::mutex> lk(e->filterMu); pin_filters(e, pinned, -1); e->evict_filters(); }
    pinned.clear();
}
// The masks of exprs (distinct, at most INFX_MAX_PREFILTERS) in the session's cache: masks[k] = the device flags of exprs[k]'s slot; the ones that have to be built
// are staged on the stream as ONE build (infx_filter_masks) and listed in `built` — their counts land in S->preCountBuf, in that order, when the stream is next
// waited for.  A failure leaves nothing staged.
int32_t MaskCall::acquire() {
    infx_engine* e = S->e;
    S->preBuilt = S->preReused = S->preLaunches = 0;
    if (exprs.empty()) return INFX_OK;
    const uint64_t ep = e->maskEpoch.load(); const uint64_t tick = ++S->preTick;
    std::vector<int> slots(exprs.size(), -1);
    masks.assign(exprs.size(), nullptr); built.clear();
    auto bail = [&](int32_t rc) { unstage_prefilters(S, built); built.clear(); release(); return rc; };
    for (size_t k = 0; k < exprs.size(); k++)
        for (int i = 0; i < INFX_MAX_PREFILTERS; i++) { PreMask& M = S->preMask[i]; if (M.valid && M.epoch == ep && M.expr == exprs[k]) { slots[k] = i; M.lastUse = tick; S->preReused++; break; } }
    std::vector<infx_filter_prog> progs; std::vector<uint8_t*> ptrs;
    std::lock_guard<std::mutex> lk(e->filterMu);
    struct Held { bool& f; explicit Held(bool& x) : f(x) { f = true; } ~Held() { f = false; } } held(locked);
    for (size_t k = 0; k < exprs.size(); k++) {
        if (slots[k] >= 0) { int32_t rc = infx_stream_mask_slot(S->stream, (uint32_t)slots[k], &masks[k]); if (rc) return failed(rc); continue; }
        int best = -1;      // a slot of an earlier epoch or an empty one first, else the least recently used that this batch does not use
        for (int i = 0; i < INFX_MAX_PREFILTERS; i++) {
            PreMask& M = S->preMask[i];
            if (M.valid && M.epoch == ep && M.lastUse == tick) continue;
            const bool stale = !M.valid || M.epoch != ep;
            if (best < 0) { best = i; continue; }
            const PreMask& Bm = S->preMask[best]; const bool bestStale = !Bm.valid || Bm.epoch != ep;
            if (stale != bestStale ? stale : (!stale && M.lastUse < Bm.lastUse)) best = i;
        }
        if (best < 0) return bail(efail(INFX_ECAPACITY, "more than INFX_MAX_PREFILTERS (16) distinct pre-filters in one batch"));
        CompiledFilter* cf = nullptr;
        { int32_t rc = compile_filter(e, exprs[k].c_str(), &cf, false); if (rc) return bail(rc); }
        pin_filters(e, {exprs[k]}, +1); pinned.push_back(exprs[k]);
        { int32_t rc = infx_stream_mask_slot(S->stream, (uint32_t)best, &masks[k]); if (rc) return failed(rc); }
        PreMask& M = S->preMask[best]; M.expr = exprs[k]; M.epoch = ep; M.lastUse = tick; M.count = 0; M.valid = true;
        built.push_back(best); progs.push_back(prog_of(*cf)); ptrs.push_back(masks[k]);
    }
    if (!built.empty()) {
        int32_t rc = infx_filter_masks(S->stream, (uint32_t)progs.size(), progs.data(), ptrs.data(), S->preCountBuf);
        if (rc) return failed(rc);
        S->preBuilt = (uint32_t)built.size();
    }
    return INFX_OK;
}
// Before the batch's infx_search_fused: refuses a pre-filter on a browse query, finds or stages the masks, installs each query's flags on the stream
static int32_t stage_prefilters(infx_session* S, uint32_t nq, std::vector<infx_fused_query>& fq, MaskCall& pre) {
    S->lastInPre.assign(nq, 0);
    QueryPre& Q = S->qp;
    const uint32_t n = Q.on && Q.nq == nq ? nq : 0;      // (the pre-filters were installed for this batch)
    for (uint32_t i = 0; i < n; i++) {
        if (!Q.has[i] || Q.reject[i]) continue;
        if (fq[i].flags & INFX_FQ_BROWSE) {      // empty text + EnableFacets: Filter already restricts the scan
            Q.refuse(i, INFX_EUNSUPPORTED, "a pre-filter does not apply to a browse query (empty text with EnableFacets): its Filter already restricts the scan");
            fq[i].flags &= ~INFX_FQ_BROWSE;
            continue;
        }
        pre.add(i, Q.expr[i]);      // (compiled by infx_engine_set_query_prefilters)
    }
    { int32_t rc = pre.acquire(); if (rc) return rc; }
    if (pre.exprs.empty()) return INFX_OK;
    std::vector<const uint8_t*> masks(nq, nullptr);
    for (uint32_t i = 0; i < nq; i++) masks[i] = pre.mask(i);
    int32_t rc = infx_stream_set_doc_masks(S->stream, nq, masks.data());
    return rc ? pre.failed(rc) : INFX_OK;
}
// After the call: the counts of the masks it built have landed; what it built and reused; each pre-filtered query's count
void MaskCall::done(uint32_t nq) {
    release();
    for (size_t k = 0; k < built.size(); k++) S->preMask[built[k]].count = S->preCountBuf[k];
    if (!built.empty()) { uint32_t b = 0, l = 0; infx_last_filter_mask_stats(S->stream, &b, &l); S->preLaunches = l; }
    if (use) *use = MaskUse{S->preBuilt, S->preReused};
    if (!S->qp.on || S->qp.nq != nq) return;
    const uint64_t ep = S->e->maskEpoch.load();
    for (uint32_t i = 0; i < nq; i++) {
        if (!S->qp.has[i] || S->qp.reject[i]) continue;
        for (const PreMask& M : S->preMask) if (M.valid && M.epoch == ep && M.expr == S->qp.expr[i]) { S->lastInPre[i] = M.count; break; }
    }
}
int32_t infx_engine_last_in_prefilter(infx_session* S, uint32_t nq, uint32_t* out) {
    if (!S || (nq && !out)) return efail(INFX_EINVAL, "null argument");
    if (nq != S->lastInPre.size()) return efail(INFX_EINVAL, "no batch of this size on the session");
    if (nq) std::memcpy(out, S->lastInPre.data(), (size_t)nq * 4);
    return INFX_OK;
}
int32_t infx_engine_last_prefilter_stats(infx_session* S, uint32_t* built, uint32_t* reused, uint32_t* launches) {
    if (!S) return efail(INFX_EINVAL, "null session");
    return put_stats({{built, S->preBuilt}, {reused, S->preReused}, {launches, S->preLaunches}});
}
int32_t infx_engine_prefilter_mask(infx_session* S, const char* expr, uint8_t* out_bytes, uint64_t cap) {
    if (!S || !expr || !out_bytes) return efail(INFX_EINVAL, "null argument");
    infx_engine* e = S->e;
    if (!e->dev || !S->stream || !e->indexed) return efail(INFX_EHIP, "no GPU: the pre-filter masks are built on the device");
    if (engine_sharded(e)) return efail(INFX_EUNSUPPORTED, "a pre-filter needs an engine that is not sharded");
    const uint64_t N = (uint64_t)e->ix.N;
    if (cap < N) return efail(INFX_EINVAL, "the mask holds one byte per indexed document");
    MaskCall mc(S, 1);
    { std::lock_guard<std::mutex> lk(e->filterMu); int32_t rc = mc.intern(0, expr); if (rc) return rc; }
    { int32_t rc = mc.acquire(); if (rc) return rc; }
    int32_t rc = infx_stream_wait(S->stream);      // builds what was staged
    if (rc) return mc.failed(rc);
    mc.done();
    if (N) rc = infx_stream_copy(S->stream, out_bytes, mc.mask(0), N);
    if (!rc) rc = infx_stream_wait(S->stream);
    if (rc) { g_eerr = infx_last_error(); return rc; }
    return INFX_OK;
}

// ---- facets of the documents a filter accepts (not in the reference: the facet side of Query.pre_filter) -----------------------------------------------
// For each expression: the value counts of every facetable column (the first INFX_MAX_FACET_COLS) over the documents that are not Deleted and whose OWN fields the
// expression accepts, ordered and cut as infx_engine_facets_all does, and the number of those documents.  Answers are cached per expression in the engine for
// one mask epoch; the expressions a call is missing go to the device INFX_MAX_PREFILTERS at a time, each time one pass over the columns (infx_facets_filtered).
// An expression is refused on its own (its status in out_status[i], its message from infx_engine_facets_filtered_error): INFX_EINVAL for a syntax error,
// INFX_EUNSUPPORTED for MATCHES.
int32_t infx_engine_facets_filtered(infx_session* S, uint32_t k, const char* const* exprs, int32_t* out_status) {
    if (!S || (k && !exprs)) return efail(INFX_EINVAL, "null argument");
    infx_engine* e = S->e;
    S->ff.clear(); S->ffCols.clear(); S->ffListCols.clear(); S->ffCounted = S->ffCached = S->ffLaunches = 0;
    if (!e->dev || !S->stream) return efail(INFX_EHIP, "no GPU: the filtered facet counts run on the device");
    if (!e->indexed) return efail(INFX_EINVAL, "facets before index_documents");
    S->ff.assign(k, FfAnswer());
    size_t total = 0;
    S->ffCols = facet_columns(e, &total);
    S->ffListCols = list_facet_columns(e);
    const uint64_t ep = e->maskEpoch.load();
    // the call's distinct expressions: from the cache, refused, or missing (compiled here; the programs are copied out of the filter cache, which other
    // sessions may evict from while the device counts)
    struct Missing { std::string expr; std::vector<infx_filter_op> ops; std::vector<infx_filter_leaf> leaves; std::vector<uint32_t> tables; };
    // ... and their cache entries stay pinned until the device has counted: an entry holds the derived columns of its list-column leaves, whose slots a later
    // compile (of this call or of another session) could otherwise hand to another leaf while a copy here still reads them
    struct Held { infx_engine* e; std::vector<std::string> keys;
                  ~Held() { if (keys.empty()) return; std::lock_guard<std::mutex> lk(e->filterMu); pin_filters(e, keys, -1); e->evict_filters(); } } held{e, {}};
    std::unordered_map<std::string, FfAnswer> answer; std::vector<Missing> miss;
    for (uint32_t i = 0; i < k; i++) {
        if (!exprs[i]) { S->ff[i].status = INFX_EINVAL; S->ff[i].err = "null expression"; continue; }
        if (answer.count(exprs[i])) continue;
        FfAnswer A;
        {
            std::lock_guard<std::mutex> lk(e->ffMu);
            auto it = e->ffCache.find(exprs[i]);
            if (it != e->ffCache.end() && it->second->epoch == ep) { e->ffLru.splice(e->ffLru.begin(), e->ffLru, it->second->lru); A.r = it->second; S->ffCached++; }
        }
        if (!A.r) {
            std::lock_guard<std::mutex> lk(e->filterMu);
            CompiledFilter* cf = nullptr;
            const int32_t rc = compile_filter(e, exprs[i], &cf, false);      // syntax error: INFX_EINVAL; MATCHES: INFX_EUNSUPPORTED
            if (rc) { A.status = rc; A.err = g_eerr; }
            else { miss.push_back(Missing{exprs[i], cf->ops, cf->leaves, cf->tables}); pin_filters(e, {exprs[i]}, +1); held.keys.push_back(exprs[i]); }
        }
        answer.emplace(exprs[i], std::move(A));
    }
    std::vector<uint32_t> counts, totals(INFX_MAX_PREFILTERS);
    for (size_t m0 = 0; m0 < miss.size(); m0 += INFX_MAX_PREFILTERS) {
        const uint32_t kk = (uint32_t)std::min<size_t>(INFX_MAX_PREFILTERS, miss.size() - m0);
        std::vector<infx_filter_prog> progs(kk);
        for (uint32_t j = 0; j < kk; j++) progs[j] = prog_of(miss[m0 + j]);
        counts.resize(std::max<size_t>((size_t)kk * total, 1));
        int32_t rc = infx_facets_filtered(S->stream, kk, progs.data(), (uint32_t)S->ffCols.size(), S->ffCols.data(), counts.data(), totals.data());
        if (rc) { g_eerr = infx_last_error(); S->ff.clear(); S->ffCols.clear(); S->ffListCols.clear(); return rc; }
        uint32_t np = 0, nl = 0; infx_last_facets_filtered_stats(S->stream, &np, &nl);
        S->ffCounted += kk; S->ffLaunches += nl;
        // the facetable list columns: the accept sets are the session's pre-filter masks of these expressions (built through the 16-mask cache, or reused),
        // one k_list_facets launch per column for all kk of them
        std::vector<std::vector<uint32_t>> listCounts(S->ffListCols.size());
        if (!S->ffListCols.empty()) {
            auto bail0 = [&](int32_t r) { S->ff.clear(); S->ffCols.clear(); S->ffListCols.clear(); return r; };
            const uint32_t pre[3] = {S->preBuilt, S->preReused, S->preLaunches};      // (the session's last_prefilter_stats are the last search's, not this call's)
            auto bail = [&](int32_t r) { S->preBuilt = pre[0]; S->preReused = pre[1]; S->preLaunches = pre[2]; return bail0(r); };
            MaskCall mc(S, kk);
            for (uint32_t j = 0; j < kk; j++) mc.add(j, miss[m0 + j].expr);
            { int32_t r = mc.acquire(); if (r) return bail(r); }
            { int32_t r = infx_stream_wait(S->stream); if (r) return bail(mc.failed(r)); }      // builds what was staged
            mc.done();
            std::vector<const uint8_t*> masks(kk); for (uint32_t j = 0; j < kk; j++) masks[j] = mc.mask(j);
            for (size_t c = 0; c < S->ffListCols.size(); c++) {
                const filt::ListColumn& C = e->listCols[S->ffListCols[c]];
                listCounts[c].assign(std::max<size_t>((size_t)kk * C.dict.dict.size(), 1), 0u);
                int32_t r = infx_list_facets(S->stream, S->ffListCols[c], kk, masks.data(), listCounts[c].data());
                if (r) { g_eerr = infx_last_error(); return bail(r); }
            }
            S->preBuilt = pre[0]; S->preReused = pre[1]; S->preLaunches = pre[2];
        }
        for (uint32_t j = 0; j < kk; j++) {
            auto E = std::make_shared<FfEntry>(); E->epoch = ep; E->total = totals[j];
            size_t o = (size_t)j * total;
            for (uint32_t col : S->ffCols) { const filt::Column& C = e->columns[col]; E->lists.push_back(facet_list(C, counts.data() + o)); o += C.dict.size(); }
            for (size_t c = 0; c < S->ffListCols.size(); c++) { const filt::Column& C = e->listCols[S->ffListCols[c]].dict; E->listLists.push_back(facet_list(C, listCounts[c].data() + (size_t)j * C.dict.size())); }
            answer[miss[m0 + j].expr].r = E;
            std::lock_guard<std::mutex> lk(e->ffMu);
            auto it = e->ffCache.find(miss[m0 + j].expr);
            if (it != e->ffCache.end()) { e->ffLru.erase(it->second->lru); e->ffCache.erase(it); }
            e->ffLru.push_front(miss[m0 + j].expr); E->lru = e->ffLru.begin();
            e->ffCache.emplace(miss[m0 + j].expr, E);
            while (e->ffCache.size() > e->ffCacheLimit) { e->ffCache.erase(e->ffLru.back()); e->ffLru.pop_back(); }
        }
    }
    for (uint32_t i = 0; i < k; i++) if (exprs[i]) { S->ff[i] = answer[exprs[i]]; if (S->ff[i].r) S->ff[i].total = S->ff[i].r->total; }
    if (out_status) for (uint32_t i = 0; i < k; i++) out_status[i] = S->ff[i].status;
    return INFX_OK;
}
int32_t infx_engine_facets_filtered_column_count(infx_session* S) { return S ? (int32_t)S->ffCols.size() : -1; }
// Expression `which` of the session's last infx_engine_facets_filtered, its k-th facet column: engine column index in *col, up to cap (code, count) pairs; returns
// their number, -1 on error (also for an expression that was refused).
int32_t infx_engine_facets_filtered_column(infx_session* S, uint32_t which, uint32_t k, int32_t* col, uint32_t* codes, uint32_t* counts, int32_t cap) {
    if (!S || which >= S->ff.size() || !S->ff[which].r || k >= S->ff[which].r->lists.size() || k >= S->ffCols.size() || (cap > 0 && (!codes || !counts))) return -1;
    if (col) *col = (int32_t)S->ffCols[k];
    return copy_pairs(S->ff[which].r->lists[k], codes, counts, cap);
}
// the facetable list columns of the session's last infx_engine_facets_filtered, and expression `which`'s k-th: list column index in *lcol, (element code, occurrences)
int32_t infx_engine_facets_filtered_list_column_count(infx_session* S) { return S ? (int32_t)S->ffListCols.size() : -1; }
int32_t infx_engine_facets_filtered_list_column(infx_session* S, uint32_t which, uint32_t k, int32_t* lcol, uint32_t* codes, uint32_t* counts, int32_t cap) {
    if (!S || which >= S->ff.size() || !S->ff[which].r || k >= S->ff[which].r->listLists.size() || k >= S->ffListCols.size() || (cap > 0 && (!codes || !counts))) return -1;
    if (lcol) *lcol = (int32_t)S->ffListCols[k];
    return copy_pairs(S->ff[which].r->listLists[k], codes, counts, cap);
}
// the live documents expression `which` accepts (0 for a refused one, whose status is returned)
int32_t infx_engine_facets_filtered_total(infx_session* S, uint32_t which, uint32_t* total) {
    return answer_total(answer_at(S ? &S->ff : nullptr, which), total, "no such expression in the session's last filtered-facet call");
}
// the message of expression `which`'s refusal ("" if it was counted); returns its length, -1 out of range
int32_t infx_engine_facets_filtered_error(infx_session* S, uint32_t which, char* out, int32_t cap) { return answer_error(answer_at(S ? &S->ff : nullptr, which), out, cap); }
int32_t infx_engine_last_facets_filtered_stats(infx_session* S, uint32_t* counted, uint32_t* cached, uint32_t* launches) {
    if (!S) return efail(INFX_EINVAL, "null session");
    return put_stats({{counted, S->ffCounted}, {cached, S->ffCached}, {launches, S->ffLaunches}});
}

// ---- requests over the documents a filter accepts: infx_engine_list_documents, _range_facets, _field_stats, _field_quantiles and _list_groups -----------
// Each takes up to INFX_MAX_PREFILTERS requests, answer each on its own (a refusal is the request's: its status in out_status[i], its message with the answer)
// and leave the answers on the session for the readers.  A call that fails as a whole leaves no answers behind — the readers refuse — while the statuses
// already written to out_status stay.  The filters and their masks are a MaskCall's.
// what such a call needs of the engine (`what` names the call in the message)
static int32_t need_indexed_device(const infx_session* S, const char* what) {
    if (!S->e->dev || !S->stream) return efail(INFX_EHIP, std::string("no GPU: ") + what + " runs on the device");
    if (!S->e->indexed) return efail(INFX_EINVAL, std::string(what) + " before index_documents");
    return INFX_OK;
}
extern "C++" {
// One such call while it runs, as its kind's steps see it: `last` is where the session keeps the kind's answers, who[j] the request behind the j-th live one
template <class K> struct SetCall {
    infx_session* S; K& last; int32_t* out; MaskCall mc; std::vector<uint32_t> who;
    void refuse(uint32_t i, int32_t rc, const std::string& msg) { last.ans[i].status = rc; last.ans[i].err = msg; if (out) out[i] = rc; }
    // request i's filter (null: none) through the filter cache; false: refused.  Caller holds filterMu
    bool filter(uint32_t i, const char* expr) { const int32_t rc = expr ? mc.intern(i, expr) : INFX_OK; if (rc) refuse(i, rc, g_eerr); return !rc; }
    template <class Fn> void each(bool locked, Fn fn) {      // fn(*this, i) for every request not refused so far, under filterMu if `locked`
        std::unique_lock<std::mutex> lk(S->e->filterMu, std::defer_lock);
        if (locked) lk.lock();
        for (uint32_t i = 0; i < last.ans.size(); i++) if (!last.ans[i].status) fn(*this, i);
    }
    int32_t fail(int32_t rc, bool staged) { last.ans.clear(); return staged ? mc.failed(rc) : rc; }      // the call fails as a whole (staged: a build may be)
};
// The frame of every such call.  `kind` is what the session keeps of the kind's last call (reset here), `name` the call's name and `plural` its requests in
// the messages.  The kind's own steps: check(F, i) looks at what of request i needs no device (under filterMu where lockedCheck), resolve(F, i) at its columns
// and its filter under filterMu — both refuse on the request's behalf and see only requests not refused so far; run(F) packs the live requests F.who, makes
// the device call and returns its status; unpack(F) fetches the device's counters and fills the answers of F.who.
template <class K, class Q, class Check, class Resolve, class Run, class Unpack>
static int32_t set_call(infx_session* S, K infx_session::*kind, const char* name, const char* plural, bool lockedCheck, uint32_t nreq, const Q* reqs,
                        int32_t* out_status, Check check, Resolve resolve, Run run, Unpack unpack) {
    if (!S || (nreq && !reqs)) return efail(INFX_EINVAL, "null argument");
    S->*kind = K();
    if (nreq > INFX_MAX_PREFILTERS) return efail(INFX_ECAPACITY, std::string("more than INFX_MAX_PREFILTERS (16) ") + plural + " in one call");
    SetCall<K> F{S, S->*kind, out_status, MaskCall(S, nreq, &(S->*kind).masks), {}};
    F.last.ans.assign(nreq, typename K::answer());
    if (out_status) std::fill(out_status, out_status + nreq, (int32_t)INFX_OK);
    F.each(lockedCheck, check);
    { const int32_t rc = need_indexed_device(S, name); if (rc) return F.fail(rc, false); }
    F.each(true, resolve);
    { const int32_t rc = F.mc.acquire(); if (rc) return F.fail(rc, false); }
    for (uint32_t i = 0; i < nreq; i++) if (!F.last.ans[i].status) F.who.push_back(i);
    { const int32_t rc = run(F); if (rc) return F.fail(rc, true); }
    F.mc.done();
    unpack(F);
    return INFX_OK;
}
// The groups of G that have a member — members(g) of them — in the contract's order: members descending, then the group column's rank ascending
template <class M> static std::vector<uint32_t> groups_in_order(const filt::Column& G, M members) {
    std::vector<uint32_t> ord;
    for (uint32_t g = 0; g < G.dict.size(); g++) if (members(g)) ord.push_back(g);
    std::sort(ord.begin(), ord.end(), [&](uint32_t a, uint32_t b) { return members(a) != members(b) ? members(a) > members(b) : G.rank[a] < G.rank[b]; });
    return ord;
}
// page j of a listing call's rows (INFX_POST_MAX_ROWS per request), its first c
template <class T> static void page_of(std::vector<T>& to, const std::vector<T>& rows, size_t j, size_t c) {
    to.assign(rows.begin() + j * INFX_POST_MAX_ROWS, rows.begin() + j * INFX_POST_MAX_ROWS + c);
}
// The two readers of a FiguresAnswer (null: no such answer).  The whole's figures: returns the request's status, INFX_EINVAL (message `none`) without an answer
template <class F> static int32_t figures_whole(const FiguresAnswer<F>* A, F* out, const char* none) {
    if (!A || !out) return efail(INFX_EINVAL, none);
    *out = A->whole;
    return A->status;
}
// its groups, in the contract's order: up to cap codes (of column *group_col, -1 without group_by) and figures; returns the number of groups, -1 on error
// (also for a refused request)
template <class F> static int32_t figures_groups(const FiguresAnswer<F>* A, int32_t* group_col, uint32_t* codes, F* figures, int32_t cap) {
    if (!A || A->status || (cap > 0 && (!codes || !figures))) return -1;
    const size_t c = std::min<size_t>(A->groups.size(), (size_t)std::max(cap, 0));
    if (c) { std::memcpy(codes, A->codes.data(), c * 4); std::memcpy(figures, A->groups.data(), c * sizeof(F)); }
    if (group_col) *group_col = A->groupCol;
    return (int32_t)A->groups.size();
}
} // extern "C++"

// ---- list_documents: a filter's documents in the order of a field, by page (not in the reference) ------------------------------------------------------
// Per request: the filter goes through the filter cache (refusals are the request's own), its mask through the session's mask cache (the slots, the LRU
// rule and the statistics of a batch's pre-filters; the missing ones staged as ONE build), the field to its column, whose sort rank is built on first use.
// infx_list_ordered then selects, gathers and sorts every page on the device; the answers stay on the session for the readers.
// what is wrong with a page's limit or offset (null: nothing)
static const char* page_problem(uint32_t limit, uint32_t offset) {
    if (limit < 1 || limit > INFX_POST_MAX_ROWS) return "a listing's limit is 1 .. 1024";
    return offset >= 0x80000000u ? "a listing's offset is below 2^31" : nullptr;
}
// order_by (null: document order, *col stays -1) to its column, whose sort rank is built on first use; a failure is the request's: its status, the text in
// *why (`what` names the call).  Caller holds e->filterMu.
static int32_t order_column(infx_engine* e, const char* what, const char* order_by, int32_t* col, std::string* why) {
    if (!order_by) return INFX_OK;
    uint32_t c = 0xFFFFFFFFu;
    const int32_t rc = sort_column(e, order_by, &c);
    if (rc) { *why = g_eerr; return rc; }
    if (c == 0xFFFFFFFFu) { *why = std::string(what) + ": no field named '" + order_by + "'"; return INFX_EINVAL; }
    *col = (int32_t)c;
    return INFX_OK;
}
// The pages of a listing call's m live requests as the device library writes them: INFX_POST_MAX_ROWS rows per request, its page's row count, its set's size
struct PageRows {
    std::vector<int64_t> keys; std::vector<int32_t> docs; std::vector<uint32_t> codes, counts, totals;
    void pages(size_t m) {
        const size_t rows = std::max<size_t>(m, 1) * INFX_POST_MAX_ROWS;
        keys.resize(rows); docs.resize(rows); codes.resize(rows); counts.assign(std::max<size_t>(m, 1), 0); totals.assign(std::max<size_t>(m, 1), 0);
    }
    // answer A takes page j, cut to the request's limit, and the size of the set; returns the page's rows
    size_t take(ListAnswer& A, size_t j, uint32_t limit) const {
        const size_t c = std::min<size_t>(counts[j], limit);
        A.total = totals[j]; page_of(A.keys, keys, j, c); page_of(A.docs, docs, j, c); page_of(A.codes, codes, j, c);
        return c;
    }
};
int32_t infx_engine_list_documents(infx_session* S, uint32_t nreq, const infx_list_request* reqs, int32_t* out_status) {
    std::array<int32_t, INFX_MAX_PREFILTERS> col; col.fill(-1); std::vector<infx_list_req> dr; PageRows P;
    return set_call(S, &infx_session::lst, "list_documents", "listing requests", false, nreq, reqs, out_status,
        [&](auto& F, uint32_t i) { if (const char* bad = page_problem(reqs[i].limit, reqs[i].offset)) F.refuse(i, INFX_EINVAL, bad); },
        [&](auto& F, uint32_t i) {
            std::string why;
            const int32_t rc = order_column(S->e, "list_documents", reqs[i].order_by, &col[i], &why);
            if (rc) F.refuse(i, rc, why); else F.filter(i, reqs[i].filter);
        },
        [&](auto& F) {
            for (uint32_t i : F.who) {
                infx_list_req R{};
                R.mask = F.mc.mask(i); R.col = col[i]; R.ascending = reqs[i].ascending ? 1 : 0; R.offset = reqs[i].offset; R.limit = reqs[i].limit;
                R.digit_bits = (uint32_t)S->lstDigitBits;
                dr.push_back(R);
            }
            P.pages(dr.size());
            return infx_list_ordered(S->stream, (uint32_t)dr.size(), dr.data(), P.keys.data(), P.docs.data(), P.codes.data(), P.counts.data(), P.totals.data());
        },
        [&](auto& F) {
            infx_last_list_stats(S->stream, &S->lst.passes, &S->lst.launches);
            for (size_t j = 0; j < dr.size(); j++) P.take(S->lst.ans[F.who[j]], j, dr[j].limit);
        });
}
// The rows reader of a page: up to cap rows; returns the page's row count (*copied: how many it copied), -1 on error (also for a refused request).  A reader
// with further arrays passes whether they are there in `more`.
static int32_t page_rows(const ListAnswer* A, int64_t* keys, int32_t* docs, uint32_t* codes, int32_t cap, bool more = true, size_t* copied = nullptr) {
    if (!A || A->status || (cap > 0 && (!keys || !docs || !codes || !more))) return -1;
    const size_t c = std::min<size_t>(A->keys.size(), (size_t)std::max(cap, 0));
    if (c) { std::memcpy(keys, A->keys.data(), c * 8); std::memcpy(docs, A->docs.data(), c * 4); std::memcpy(codes, A->codes.data(), c * 4); }
    if (copied) *copied = c;
    return (int32_t)A->keys.size();
}
// request `which` of the session's last infx_engine_list_documents: its page, as page_rows
int32_t infx_engine_list_rows(infx_session* S, uint32_t which, int64_t* keys, int32_t* docs, uint32_t* codes, int32_t cap) {
    return page_rows(answer_at(S ? &S->lst.ans : nullptr, which), keys, docs, codes, cap);
}
// the size of request `which`'s set (0 for a refused one, whose status is returned)
int32_t infx_engine_list_total(infx_session* S, uint32_t which, uint32_t* total) {
    return answer_total(answer_at(S ? &S->lst.ans : nullptr, which), total, "no such request in the session's last list_documents call");
}
int32_t infx_engine_list_error(infx_session* S, uint32_t which, char* out, int32_t cap) { return answer_error(answer_at(S ? &S->lst.ans : nullptr, which), out, cap); }
int32_t infx_engine_last_list_stats(infx_session* S, uint32_t* masks_built, uint32_t* masks_reused, uint32_t* hist_passes, uint32_t* launches) {
    if (!S) return efail(INFX_EINVAL, "null session");
    return put_stats({{masks_built, S->lst.masks.built}, {masks_reused, S->lst.masks.reused}, {hist_passes, S->lst.passes}, {launches, S->lst.launches}});
}
int32_t infx_engine_set_list_digit_bits(infx_session* S, int32_t bits) {
    if (!S || bits < 4 || bits > 11) return efail(INFX_EINVAL, "the digit width of list_documents is 4 .. 11 bits");
    S->lstDigitBits = bits;
    return INFX_OK;
}

// ---- range_facets: bucket counts and min / max of a numeric field over the documents a filter accepts (not in the reference) --------------------------
// Per request: the field to its column (int64 or double), the edges to thresholds over the column's dense sort rank — thr[i] = the number of distinct ranks
// whose value compares < e_i under filt::sort_cmp, found by bisection over the ranks' values — the filter through the filter cache and its mask through the
// session's mask cache, as infx_engine_list_documents.  infx_range_counts then counts every request in one pass; the extreme ranks come back as values.
// The column's rank order (lowest code of every rank; built with the sort rank's first use).  Caller holds e->filterMu.
static int32_t range_index(infx_engine* e, uint32_t col, const infx_engine::RangeIndex** out) {
    if (e->rangeIndex.size() < e->columns.size()) e->rangeIndex.resize(e->columns.size());
    infx_engine::RangeIndex& X = e->rangeIndex[col];
    std::vector<uint32_t> rank;
    { const int32_t rc = sort_rank_on_device(e, col, &rank); if (rc) return rc; }
    if (!X.ok) {
        const filt::Column& c = e->columns[col];
        if (rank.empty()) filt::sort_rank(c, rank);
        uint32_t nr = 0; for (uint32_t r : rank) nr = std::max(nr, r + 1u);
        X.codeOfRank.assign(nr, 0xFFFFFFFFu);
        for (size_t code = 0; code < rank.size(); code++) if (X.codeOfRank[rank[code]] == 0xFFFFFFFFu) X.codeOfRank[rank[code]] = (uint32_t)code;      // codes ascend: the lowest wins
        X.nanRanks = nr && c.dict[X.codeOfRank[0]].kind == 2 && std::isnan(c.dict[X.codeOfRank[0]].d) ? 1u : 0u;
        X.ok = true;
    }
    *out = &X;
    return INFX_OK;
}
// the value of a rank of column C: its lowest code's (null: no such rank, as the ranks of an empty set)
static const filt::Boxed* value_of_rank(const filt::Column& C, const infx_engine::RangeIndex& X, uint32_t rank) {
    return rank < X.codeOfRank.size() ? &C.dict[X.codeOfRank[rank]] : nullptr;
}
static int column_kind(const filt::Column& c) { return c.dict.empty() ? 0 : c.dict[0].kind; }
// What is wrong with request Q before anything of it is looked at on the device — the field, its kind, the edges, in this order — as the request's status, the
// text in *why; INFX_OK with the field's column and the kind of the edges (1 int64, 2 double).  `what` names the call and `role` the field in the messages
// (infx_engine_bucket_stats: its bucket_by).  Caller holds e->filterMu.
static int32_t range_request_check(const infx_engine* e, const infx_range_request& Q, int32_t* col, int* kind, std::string* why, const std::string& what = "range_facets",
                                   const std::string& role = "field") {
    auto bad = [&](const std::string& msg) { *why = msg; return (int32_t)INFX_EINVAL; };
    if (!Q.field) return bad(what + " needs a " + role);
    if ((*col = column_named(e, Q.field)) < 0) return bad(what + ": no " + role + " named '" + Q.field + "'");
    int k = column_kind(e->columns[*col]);
    if (k == 3) return bad(what + ": " + role + " '" + Q.field + "' is a string column; ranges need an int64 or a double column");
    if (k == 0) k = Q.edges_i ? 1 : 2;                              // (a column without a value)
    *kind = k;
    if (Q.nedges < 2 || Q.nedges > INFX_RANGE_MAX_EDGES) return bad(what + " takes 2 to 257 edges (1 to 256 buckets)");
    if (k == 1) {
        if (!Q.edges_i) return bad("integer column needs integer edges");
        for (uint32_t j = 1; j < Q.nedges; j++) if (!(Q.edges_i[j - 1] < Q.edges_i[j])) return bad("the edges of " + what + " are strictly increasing");
    } else {
        if (!Q.edges_d) return bad("double column needs double edges");
        for (uint32_t j = 0; j < Q.nedges; j++) {
            if (std::isnan(Q.edges_d[j])) return bad("an edge of " + what + " is not a NaN");
            if (j && !(Q.edges_d[j - 1] < Q.edges_d[j])) return bad("the edges of " + what + " are strictly increasing (-0.0 and 0.0 compare equal)");
        }
    }
    return INFX_OK;
}
// The edges of Q as thresholds over column c's ranks: the ranks' values ascend under sort_cmp, thr[j] = the first rank whose value is not below edge j
static std::vector<uint32_t> range_thresholds(const filt::Column& c, const infx_engine::RangeIndex& X, const infx_range_request& Q, int kind) {
    std::vector<uint32_t> thr(Q.nedges);
    for (uint32_t j = 0; j < Q.nedges; j++) {
        filt::Boxed edge; edge.kind = kind; if (kind == 1) edge.i = Q.edges_i[j]; else edge.d = Q.edges_d[j];
        thr[j] = (uint32_t)(std::partition_point(X.codeOfRank.begin(), X.codeOfRank.end(), [&](uint32_t code) { return filt::sort_cmp(c.dict[code], edge) < 0; }) - X.codeOfRank.begin());
    }
    return thr;
}
int32_t infx_engine_range_facets(infx_session* S, uint32_t nreq, const infx_range_request* reqs, int32_t* out_status) {
    struct Req { int32_t col = -1; int kind = 0; uint32_t nanRanks = 0; std::vector<uint32_t> thr; } rq[INFX_MAX_PREFILTERS];
    std::vector<infx_range_req> dr; std::vector<uint32_t> counts, lo, hi;
    return set_call(S, &infx_session::rng, "range_facets", "range requests", true, nreq, reqs, out_status,
        [&](auto& F, uint32_t i) {
            std::string why;
            const int32_t rc = range_request_check(S->e, reqs[i], &rq[i].col, &rq[i].kind, &why);
            if (rc) F.refuse(i, rc, why);
        },
        [&](auto& F, uint32_t i) {
            const infx_engine::RangeIndex* X = nullptr;
            const int32_t rc = range_index(S->e, (uint32_t)rq[i].col, &X);
            if (rc) return F.refuse(i, rc, g_eerr);
            if (!F.filter(i, reqs[i].filter)) return;
            rq[i].nanRanks = X->nanRanks;
            rq[i].thr = range_thresholds(S->e->columns[rq[i].col], *X, reqs[i], rq[i].kind);
        },
        [&](auto& F) {
            for (uint32_t i : F.who) {
                infx_range_req R{};
                R.mask = F.mc.mask(i); R.col = rq[i].col; R.nedges = reqs[i].nedges; R.nan_ranks = rq[i].nanRanks; R.thr = rq[i].thr.data();
                dr.push_back(R);
            }
            const size_t m = std::max<size_t>(dr.size(), 1);
            counts.assign(m * INFX_RANGE_SLOTS, 0); lo.assign(m, 0xFFFFFFFFu); hi.assign(m, 0);
            return infx_range_counts(S->stream, (uint32_t)dr.size(), dr.data(), counts.data(), lo.data(), hi.data());
        },
        [&](auto& F) {
            infx_engine* e = S->e;
            infx_last_range_stats(S->stream, nullptr, &S->rng.launches);
            std::lock_guard<std::mutex> lk(e->filterMu);
            for (size_t j = 0; j < dr.size(); j++) {
                RangeAnswer& A = S->rng.ans[F.who[j]];
                const uint32_t ne = dr[j].nedges; const uint32_t* c = counts.data() + j * INFX_RANGE_SLOTS;
                A.below = c[0]; A.counts.assign(c + 1, c + ne); A.above = c[ne]; A.nan = c[ne + 1];
                uint64_t t = 0; for (uint32_t k = 0; k < ne + 2; k++) t += c[k];
                A.total = (uint32_t)t;
                const filt::Column& C = e->columns[dr[j].col]; const infx_engine::RangeIndex& X = e->rangeIndex[dr[j].col];
                const filt::Boxed *a = value_of_rank(C, X, lo[j]), *b = value_of_rank(C, X, hi[j]);
                if (!a || !b) continue;
                A.kind = a->kind == 1 ? 1 : 2;
                if (A.kind == 1) { A.loI = a->i; A.hiI = b->i; } else { A.loD = a->d; A.hiD = b->d; }
            }
        });
}
// request `which` of the session's last infx_engine_range_facets: up to cap bucket counts; returns the number of buckets, -1 on error (also for a refused request)
int32_t infx_engine_range_counts(infx_session* S, uint32_t which, uint32_t* counts, int32_t cap, uint32_t* below, uint32_t* above, uint32_t* nan) {
    const RangeAnswer* A = answer_at(S ? &S->rng.ans : nullptr, which);
    if (!A || A->status || (cap > 0 && !counts)) return -1;
    const size_t c = std::min<size_t>(A->counts.size(), (size_t)std::max(cap, 0));
    if (c) std::memcpy(counts, A->counts.data(), c * 4);
    if (below) *below = A->below; if (above) *above = A->above; if (nan) *nan = A->nan;
    return (int32_t)A->counts.size();
}
// the size of request `which`'s set (0 for a refused one, whose status is returned)
int32_t infx_engine_range_total(infx_session* S, uint32_t which, uint32_t* total) {
    return answer_total(answer_at(S ? &S->rng.ans : nullptr, which), total, "no such request in the session's last range_facets call");
}
// the smallest and largest non-NaN value of request `which`'s set: *kind 1 -> lo_i / hi_i, 2 -> lo_d / hi_d, 0 -> there is none
int32_t infx_engine_range_minmax(infx_session* S, uint32_t which, int32_t* kind, int64_t* lo_i, int64_t* hi_i, double* lo_d, double* hi_d) {
    if (!S || !kind || which >= S->rng.ans.size()) return efail(INFX_EINVAL, "no such request in the session's last range_facets call");
    const RangeAnswer& A = S->rng.ans[which];
    *kind = A.kind;
    if (lo_i) *lo_i = A.loI; if (hi_i) *hi_i = A.hiI; if (lo_d) *lo_d = A.loD; if (hi_d) *hi_d = A.hiD;
    return A.status;
}
int32_t infx_engine_range_error(infx_session* S, uint32_t which, char* out, int32_t cap) { return answer_error(answer_at(S ? &S->rng.ans : nullptr, which), out, cap); }
int32_t infx_engine_last_range_stats(infx_session* S, uint32_t* masks_built, uint32_t* masks_reused, uint32_t* launches) {
    if (!S) return efail(INFX_EINVAL, "null session");
    return put_stats({{masks_built, S->rng.masks.built}, {masks_reused, S->rng.masks.reused}, {launches, S->rng.launches}});
}

// ---- field_stats: counts, min / max and the exact sum and mean of a numeric field over the documents a filter accepts, whole or per group (not in the reference) ----
// Per request: the field to its column (int64 or double) and the column to its value table — the raw values of its codes with the power-of-two scale at which
// every finite one is an integer (exact_sum.h; a double column that spans more than 128 binary digits is refused) — group_by to any column of at most 4096
// values, the filter through the filter cache and its mask through the session's mask cache, as infx_engine_range_facets.  infx_field_stats then adds integers
// only, one slot per group code; the engine recombines the limb sums and rounds ONCE, for the sum and for the mean (exact_sum.h).
// The value table of a column (host part).  Caller holds e->filterMu.
static infx_engine::StatsIndex& stats_index(infx_engine* e, uint32_t col) {
    if (e->statsIndex.size() < e->columns.size()) e->statsIndex.resize(e->columns.size());
    infx_engine::StatsIndex& X = e->statsIndex[col];
    if (!X.ok) {
        const filt::Column& c = e->columns[col];
        X.kind = c.dict.empty() || c.dict[0].kind == 1 ? XS_KIND_INT : XS_KIND_DOUBLE;
        X.bits.resize(c.dict.size());
        for (size_t v = 0; v < c.dict.size(); v++) { if (X.kind == XS_KIND_INT) X.bits[v] = (uint64_t)c.dict[v].i; else std::memcpy(&X.bits[v], &c.dict[v].d, 8); }
        X.summable = xs_column_scale(X.bits.data(), X.bits.size(), X.kind, &X.sc);
        X.uploaded = false; X.ok = true;
    }
    return X;
}
// What is wrong with the group_by of a request of `what` (null: none, *gcol = -1): an unknown column or one of more than INFX_STATS_MAX_GROUPS values.
// Caller holds e->filterMu.
static int32_t group_by_check(const infx_engine* e, const std::string& what, const char* group_by, int32_t* gcol, std::string* why) {
    auto bad = [&](const std::string& msg) { *why = what + msg; return (int32_t)INFX_EINVAL; };
    *gcol = -1;
    if (group_by) {
        if ((*gcol = column_named(e, group_by)) < 0) return bad(std::string(": no group_by field named '") + group_by + "'");
        if (e->columns[*gcol].dict.size() > INFX_STATS_MAX_GROUPS) return bad(std::string(": group_by field '") + group_by + "' has more than 4096 distinct values");
    }
    return INFX_OK;
}
// What is wrong with the field and the group_by of a field_stats or field_quantiles request (`what`; its `figures` need a numeric column) before anything of
// it is looked at on the device — the field, its kind, group_by, in this order — as the request's status, the text in *why; INFX_OK with the columns (gcol -1:
// no group_by).  Caller holds e->filterMu.
static int32_t numeric_field_check(const infx_engine* e, const std::string& what, const char* figures, const char* field, const char* group_by, int32_t* col,
                                   int32_t* gcol, std::string* why) {
    auto bad = [&](const std::string& msg) { *why = what + msg; return (int32_t)INFX_EINVAL; };
    *gcol = -1;
    if (!field) return bad(" needs a field");
    if ((*col = column_named(e, field)) < 0) return bad(std::string(": no field named '") + field + "'");
    if (column_kind(e->columns[*col]) == 3) return bad(std::string(": field '") + field + "' is a string column; " + figures + " need an int64 or a double column");
    return group_by_check(e, what, group_by, gcol, why);
}
// The figures of one slot (a group, or the whole): counts, the extremes as values through the rank's lowest code, the limb sums recombined and rounded once
static infx_stats_figures stats_figures(const infx_stats_slot& S, const infx_engine::StatsIndex& V, const filt::Column& C, const infx_engine::RangeIndex& X) {
    infx_stats_figures F = {};
    F.count = S.finite + S.pinf + S.ninf; F.nan = S.nan; F.kind = V.kind;
    const XsWide W = xs_recombine(S.sum, V.sc.nlimbs);
    const uint64_t sb = xs_sum_bits(W, V.sc.scale, S.pinf, S.ninf); std::memcpy(&F.sum_d, &sb, 8);
    if (V.kind == XS_KIND_INT) xs_sum_int128(W, &F.sum_lo, &F.sum_hi);
    if (F.count) {
        const uint64_t mb = xs_mean_bits(W, V.sc.scale, F.count, S.pinf, S.ninf); std::memcpy(&F.mean, &mb, 8);
        const filt::Boxed *a = value_of_rank(C, X, S.min_rank), *b = value_of_rank(C, X, S.max_rank);
        if (a && b) { if (V.kind == XS_KIND_INT) { F.min_i = a->i; F.max_i = b->i; } else { F.min_d = a->d; F.max_d = b->d; } }
    }
    return F;
}
int32_t infx_engine_field_stats(infx_session* S, uint32_t nreq, const infx_stats_request* reqs, int32_t* out_status) {
    std::array<int32_t, INFX_MAX_PREFILTERS> col, gcol; std::vector<infx_stats_req> dr; std::vector<size_t> at; std::vector<infx_stats_slot> slots;
    return set_call(S, &infx_session::sts, "field_stats", "field_stats requests", true, nreq, reqs, out_status,
        [&](auto& F, uint32_t i) {
            std::string why;
            int32_t rc = numeric_field_check(S->e, "field_stats", "sums", reqs[i].field, reqs[i].group_by, &col[i], &gcol[i], &why);
            if (!rc && !stats_index(S->e, (uint32_t)col[i]).summable) {
                rc = INFX_EINVAL;
                why = std::string("field_stats: the finite values of field '") + reqs[i].field + "' span more than 128 binary digits; they cannot be summed exactly";
            }
            if (rc) F.refuse(i, rc, why);
        },
        [&](auto& F, uint32_t i) {
            infx_engine* e = S->e;
            const infx_engine::RangeIndex* X = nullptr;
            { const int32_t rc = range_index(e, (uint32_t)col[i], &X); if (rc) return F.refuse(i, rc, g_eerr); }      // (the sort rank, for min / max)
            infx_engine::StatsIndex& V = stats_index(e, (uint32_t)col[i]);
            if (!V.uploaded) {
                const int32_t rc = infx_upload_column_values(e->dev, (uint32_t)col[i], (uint32_t)V.bits.size(), V.bits.data(), V.kind, V.sc.scale, V.sc.nlimbs);
                if (rc) return F.refuse(i, rc, infx_last_error());
                V.uploaded = true;
            }
            F.filter(i, reqs[i].filter);
        },
        [&](auto& F) {
            size_t nslots = 0;
            for (uint32_t i : F.who) {
                infx_stats_req R{};
                R.mask = F.mc.mask(i); R.col = col[i]; R.group_col = gcol[i];
                dr.push_back(R); at.push_back(nslots);
                nslots += gcol[i] >= 0 ? std::max<size_t>(S->e->columns[gcol[i]].dict.size(), 1) : 1;
            }
            slots.resize(std::max<size_t>(nslots, 1));
            return infx_field_stats(S->stream, (uint32_t)dr.size(), dr.data(), slots.data());
        },
        [&](auto& F) {
            infx_engine* e = S->e;
            infx_last_field_stats_info(S->stream, nullptr, &S->sts.launches);
            std::lock_guard<std::mutex> lk(e->filterMu);
            for (size_t j = 0; j < dr.size(); j++) {
                StatsAnswer& A = S->sts.ans[F.who[j]];
                const filt::Column& C = e->columns[dr[j].col]; const infx_engine::RangeIndex& X = e->rangeIndex[dr[j].col]; const infx_engine::StatsIndex& V = e->statsIndex[dr[j].col];
                const infx_stats_slot* sl = slots.data() + at[j];
                A.groupCol = dr[j].group_col;
                if (A.groupCol < 0) A.whole = stats_figures(sl[0], V, C, X);
                else {
                    infx_stats_slot all = {}; all.min_rank = 0xFFFFFFFFu;
                    A.codes = groups_in_order(e->columns[A.groupCol], [&](uint32_t g) { return (uint64_t)sl[g].finite + sl[g].nan + sl[g].pinf + sl[g].ninf; });
                    for (uint32_t g : A.codes) {
                        const infx_stats_slot& s1 = sl[g];
                        all.finite += s1.finite; all.nan += s1.nan; all.pinf += s1.pinf; all.ninf += s1.ninf;
                        if (s1.min_rank != 0xFFFFFFFFu) { all.min_rank = std::min(all.min_rank, s1.min_rank); all.max_rank = std::max(all.max_rank, s1.max_rank); }
                        for (int k = 0; k < INFX_STATS_MAX_LIMBS; k++) all.sum[k] += s1.sum[k];      // (fewer than 2^31 members in all: no limb sum overflows)
                        A.groups.push_back(stats_figures(s1, V, C, X));
                    }
                    A.whole = stats_figures(all, V, C, X);
                }
                A.total = A.whole.count + A.whole.nan;
            }
        });
}
// request `which` of the session's last infx_engine_field_stats: the whole's figures and the groups', as figures_whole and figures_groups
int32_t infx_engine_field_stats_whole(infx_session* S, uint32_t which, infx_stats_figures* out) {
    return figures_whole(answer_at(S ? &S->sts.ans : nullptr, which), out, "no such request in the session's last field_stats call");
}
int32_t infx_engine_field_stats_groups(infx_session* S, uint32_t which, int32_t* group_col, uint32_t* codes, infx_stats_figures* figures, int32_t cap) {
    return figures_groups(answer_at(S ? &S->sts.ans : nullptr, which), group_col, codes, figures, cap);
}
// the size of request `which`'s set (0 for a refused one, whose status is returned)
int32_t infx_engine_field_stats_total(infx_session* S, uint32_t which, uint32_t* total) {
    return answer_total(answer_at(S ? &S->sts.ans : nullptr, which), total, "no such request in the session's last field_stats call");
}
int32_t infx_engine_field_stats_error(infx_session* S, uint32_t which, char* out, int32_t cap) { return answer_error(answer_at(S ? &S->sts.ans : nullptr, which), out, cap); }
int32_t infx_engine_last_field_stats_stats(infx_session* S, uint32_t* masks_built, uint32_t* masks_reused, uint32_t* launches) {
    if (!S) return efail(INFX_EINVAL, "null session");
    return put_stats({{masks_built, S->sts.masks.built}, {masks_reused, S->sts.masks.reused}, {launches, S->sts.launches}});
}

// ---- bucket_stats: field_stats' figures of a numeric field per range bucket of a second numeric field over the documents a filter accepts (not in the reference) ----
// Per request: `field` as infx_engine_field_stats resolves it (numeric_field_check, the value table, summable or refused), `bucket_by` and the edges as
// infx_engine_range_facets resolves its field and edges (range_request_check, range_thresholds over the column's dense sort rank), the filter through the
// filter cache and its mask through the session's mask cache.  infx_bucket_stats then adds integers only, one slot per bucket; the engine turns every slot
// into figures with stats_figures and adds the slots as integers for the whole, as a grouped field_stats does.
int32_t infx_engine_bucket_stats(infx_session* S, uint32_t nreq, const infx_bucket_stats_request* reqs, int32_t* out_status) {
    struct Req { int32_t col = -1, bcol = -1; int kind = 0; uint32_t nanRanks = 0; std::vector<uint32_t> thr; } rq[INFX_MAX_PREFILTERS];
    std::vector<infx_bucket_stats_req> dr; std::vector<size_t> at; std::vector<infx_stats_slot> slots;
    auto as_range = [&](uint32_t i) { return infx_range_request{reqs[i].filter, reqs[i].bucket_by, reqs[i].nedges, reqs[i].edges_i, reqs[i].edges_d}; };
    return set_call(S, &infx_session::bks, "bucket_stats", "bucket_stats requests", true, nreq, reqs, out_status,
        [&](auto& F, uint32_t i) {
            std::string why; int32_t g = -1;
            int32_t rc = numeric_field_check(S->e, "bucket_stats", "sums", reqs[i].field, nullptr, &rq[i].col, &g, &why);
            if (!rc && !stats_index(S->e, (uint32_t)rq[i].col).summable) {
                rc = INFX_EINVAL;
                why = std::string("bucket_stats: the finite values of field '") + reqs[i].field + "' span more than 128 binary digits; they cannot be summed exactly";
            }
            if (!rc) {
                rc = range_request_check(S->e, as_range(i), &rq[i].bcol, &rq[i].kind, &why, "bucket_stats", "bucket_by field");
                if (rc && why.compare(0, 12, "bucket_stats")) why = "bucket_stats: " + why;
            }
            if (rc) F.refuse(i, rc, why);
        },
        [&](auto& F, uint32_t i) {
            infx_engine* e = S->e;
            const infx_engine::RangeIndex *X = nullptr, *B = nullptr;
            { const int32_t rc = range_index(e, (uint32_t)rq[i].col, &X); if (rc) return F.refuse(i, rc, g_eerr); }      // (the sort rank, for min / max)
            { const int32_t rc = range_index(e, (uint32_t)rq[i].bcol, &B); if (rc) return F.refuse(i, rc, g_eerr); }
            infx_engine::StatsIndex& V = stats_index(e, (uint32_t)rq[i].col);
            if (!V.uploaded) {
                const int32_t rc = infx_upload_column_values(e->dev, (uint32_t)rq[i].col, (uint32_t)V.bits.size(), V.bits.data(), V.kind, V.sc.scale, V.sc.nlimbs);
                if (rc) return F.refuse(i, rc, infx_last_error());
                V.uploaded = true;
            }
            if (!F.filter(i, reqs[i].filter)) return;
            rq[i].nanRanks = B->nanRanks;
            rq[i].thr = range_thresholds(e->columns[rq[i].bcol], *B, as_range(i), rq[i].kind);
        },
        [&](auto& F) {
            size_t nslots = 0;
            for (uint32_t i : F.who) {
                infx_bucket_stats_req R{};
                R.mask = F.mc.mask(i); R.col = rq[i].col; R.bucket_col = rq[i].bcol; R.nedges = reqs[i].nedges; R.nan_ranks = rq[i].nanRanks; R.thr = rq[i].thr.data();
                dr.push_back(R); at.push_back(nslots);
                nslots += (size_t)reqs[i].nedges + 2;
            }
            slots.resize(std::max<size_t>(nslots, 1));
            return infx_bucket_stats(S->stream, (uint32_t)dr.size(), dr.data(), slots.data());
        },
        [&](auto& F) {
            infx_engine* e = S->e;
            infx_last_bucket_stats_info(S->stream, nullptr, &S->bks.launches, &S->bks.place[0], &S->bks.place[1], &S->bks.place[2]);
            std::lock_guard<std::mutex> lk(e->filterMu);
            for (size_t j = 0; j < dr.size(); j++) {
                BucketAnswer& A = S->bks.ans[F.who[j]];
                const filt::Column& C = e->columns[dr[j].col]; const infx_engine::RangeIndex& X = e->rangeIndex[dr[j].col]; const infx_engine::StatsIndex& V = e->statsIndex[dr[j].col];
                const infx_stats_slot* sl = slots.data() + at[j];
                infx_stats_slot all = {}; all.min_rank = 0xFFFFFFFFu;
                for (uint32_t g = 0; g < dr[j].nedges + 2; g++) {
                    const infx_stats_slot& s1 = sl[g];
                    all.finite += s1.finite; all.nan += s1.nan; all.pinf += s1.pinf; all.ninf += s1.ninf;
                    if (s1.min_rank != 0xFFFFFFFFu) { all.min_rank = std::min(all.min_rank, s1.min_rank); all.max_rank = std::max(all.max_rank, s1.max_rank); }
                    for (int k = 0; k < INFX_STATS_MAX_LIMBS; k++) all.sum[k] += s1.sum[k];      // (fewer than 2^31 members in all: no limb sum overflows)
                    A.sizes.push_back(s1.finite + s1.nan + s1.pinf + s1.ninf);
                    A.rows.push_back(stats_figures(s1, V, C, X));
                }
                A.whole = stats_figures(all, V, C, X);
                A.total = A.whole.count + A.whole.nan;
            }
        });
}
// request `which` of the session's last infx_engine_bucket_stats: up to cap rows in slot order [below | B buckets | above | nan] — sizes[k] the members of row k,
// figures[k] the field's figures over them; returns the number of rows (B + 3), -1 on error (also for a refused request)
int32_t infx_engine_bucket_stats_rows(infx_session* S, uint32_t which, uint32_t* sizes, infx_stats_figures* figures, int32_t cap) {
    const BucketAnswer* A = answer_at(S ? &S->bks.ans : nullptr, which);
    if (!A || A->status || (cap > 0 && (!sizes || !figures))) return -1;
    const size_t c = std::min<size_t>(A->rows.size(), (size_t)std::max(cap, 0));
    if (c) { std::memcpy(sizes, A->sizes.data(), c * 4); std::memcpy(figures, A->rows.data(), c * sizeof(infx_stats_figures)); }
    return (int32_t)A->rows.size();
}
// the figures over the whole set (returning the request's status)
int32_t infx_engine_bucket_stats_whole(infx_session* S, uint32_t which, infx_stats_figures* out) {
    const BucketAnswer* A = answer_at(S ? &S->bks.ans : nullptr, which);
    if (!A || !out) return efail(INFX_EINVAL, "no such request in the session's last bucket_stats call");
    *out = A->whole;
    return A->status;
}
// the size of request `which`'s set (0 for a refused one, whose status is returned)
int32_t infx_engine_bucket_stats_total(infx_session* S, uint32_t which, uint32_t* total) {
    return answer_total(answer_at(S ? &S->bks.ans : nullptr, which), total, "no such request in the session's last bucket_stats call");
}
int32_t infx_engine_bucket_stats_error(infx_session* S, uint32_t which, char* out, int32_t cap) { return answer_error(answer_at(S ? &S->bks.ans : nullptr, which), out, cap); }
int32_t infx_engine_last_bucket_stats_stats(infx_session* S, uint32_t* masks_built, uint32_t* masks_reused, uint32_t* launches) {
    if (!S) return efail(INFX_EINVAL, "null session");
    return put_stats({{masks_built, S->bks.masks.built}, {masks_reused, S->bks.masks.reused}, {launches, S->bks.launches}});
}
int32_t infx_engine_last_bucket_stats_placement(infx_session* S, uint32_t* small_lds, uint32_t* big_lds, uint32_t* in_global) {
    if (!S) return efail(INFX_EINVAL, "null session");
    return put_stats({{small_lds, S->bks.place[0]}, {big_lds, S->bks.place[1]}, {in_global, S->bks.place[2]}});
}

// ---- field_quantiles: the values at the quantiles' positions of a numeric field over the documents a filter accepts, whole and per group (not in the reference) ----
// Per request: the field to its column (int64 or double) and the column to its sort rank, group_by to any column of at most 4096 values, the filter through
// the filter cache and its mask through the session's mask cache, as infx_engine_field_stats.  infx_field_quantiles then selects every (slot, quantile) of the
// call on sort ranks; the engine maps each answered rank to a value through the rank's lowest code, as stats_figures does for min / max.
// What is wrong with request Q before anything of it is looked at on the device — field and group_by as numeric_field_check, then the quantiles — as the
// request's status, the text in *why; INFX_OK with the columns (gcol -1: no group_by).  Caller holds e->filterMu.
static int32_t quant_request_check(const infx_engine* e, const infx_quantile_request& Q, int32_t* col, int32_t* gcol, std::string* why) {
    auto bad = [&](const char* msg) { *why = msg; return (int32_t)INFX_EINVAL; };
    { const int32_t rc = numeric_field_check(e, "field_quantiles", "quantiles", Q.field, Q.group_by, col, gcol, why); if (rc) return rc; }
    if (!Q.nq || !Q.q) return bad("field_quantiles needs at least one quantile");
    if (Q.nq > INFX_QUANT_MAX) return bad("field_quantiles: more than 16 quantiles in one request");
    for (uint32_t t = 0; t < Q.nq; t++) if (!(Q.q[t] >= 0.0 && Q.q[t] <= 1.0)) return bad("field_quantiles: every quantile is a number in [0, 1]");
    return INFX_OK;
}
// The figures of one slot: its counts and the values of its nq answered ranks through the rank's lowest code
static infx_quantile_figures quant_figures(const infx_quant_slot& S, const uint32_t* ranks, uint32_t nq, const filt::Column& C, const infx_engine::RangeIndex& X) {
    infx_quantile_figures F = {};
    F.count = S.count; F.nan = S.nan; F.kind = C.dict.empty() || C.dict[0].kind == 1 ? 1 : 2; F.nq = nq;
    for (uint32_t t = 0; t < nq && S.count; t++)
        if (const filt::Boxed* v = value_of_rank(C, X, ranks[t])) { if (F.kind == 1) F.v_i[t] = v->i; else F.v_d[t] = v->d; }
    return F;
}
int32_t infx_engine_field_quantiles(infx_session* S, uint32_t nreq, const infx_quantile_request* reqs, int32_t* out_status) {
    std::array<int32_t, INFX_MAX_PREFILTERS> col, gcol; std::array<uint32_t, INFX_MAX_PREFILTERS> nanRanks;
    std::vector<infx_quant_req> dr; std::vector<size_t> atSlot, atRank; std::vector<infx_quant_slot> slots; std::vector<uint32_t> ranks;
    return set_call(S, &infx_session::qnt, "field_quantiles", "field_quantiles requests", true, nreq, reqs, out_status,
        [&](auto& F, uint32_t i) {
            std::string why;
            const int32_t rc = quant_request_check(S->e, reqs[i], &col[i], &gcol[i], &why);
            if (rc) F.refuse(i, rc, why);
        },
        [&](auto& F, uint32_t i) {
            const infx_engine::RangeIndex* X = nullptr;
            const int32_t rc = range_index(S->e, (uint32_t)col[i], &X);
            if (rc) return F.refuse(i, rc, g_eerr);
            nanRanks[i] = X->nanRanks;
            F.filter(i, reqs[i].filter);
        },
        [&](auto& F) {
            size_t nslots = 0, nranks = 0;
            for (uint32_t i : F.who) {
                infx_quant_req R{};
                R.mask = F.mc.mask(i); R.col = col[i]; R.group_col = gcol[i]; R.digit_bits = (uint32_t)S->qntDigitBits; R.nan_ranks = nanRanks[i];
                R.nq = reqs[i].nq; std::copy(reqs[i].q, reqs[i].q + reqs[i].nq, R.q);
                dr.push_back(R); atSlot.push_back(nslots); atRank.push_back(nranks);
                const size_t sl = gcol[i] >= 0 ? S->e->columns[gcol[i]].dict.size() + 1 : 1;
                nslots += sl; nranks += sl * reqs[i].nq;
            }
            slots.resize(std::max<size_t>(nslots, 1)); ranks.resize(std::max<size_t>(nranks, 1));
            return infx_field_quantiles(S->stream, (uint32_t)dr.size(), dr.data(), slots.data(), ranks.data());
        },
        [&](auto& F) {
            infx_engine* e = S->e;
            infx_last_field_quantiles_info(S->stream, nullptr, &S->qnt.passes, &S->qnt.launches, &S->qnt.place[0], &S->qnt.place[1], &S->qnt.place[2]);
            std::lock_guard<std::mutex> lk(e->filterMu);
            for (size_t j = 0; j < dr.size(); j++) {
                QuantAnswer& A = S->qnt.ans[F.who[j]];
                const filt::Column& C = e->columns[dr[j].col]; const infx_engine::RangeIndex& X = e->rangeIndex[dr[j].col];
                const infx_quant_slot* sl = slots.data() + atSlot[j]; const uint32_t* rk = ranks.data() + atRank[j]; const uint32_t nq = dr[j].nq;
                A.groupCol = dr[j].group_col;
                const size_t ng = A.groupCol >= 0 ? e->columns[A.groupCol].dict.size() : 0;      // (the whole set's slot lies behind the groups')
                A.whole = quant_figures(sl[ng], rk + ng * nq, nq, C, X);
                if (A.groupCol >= 0) {
                    A.codes = groups_in_order(e->columns[A.groupCol], [&](uint32_t g) { return (uint64_t)sl[g].count + sl[g].nan; });
                    for (uint32_t g : A.codes) A.groups.push_back(quant_figures(sl[g], rk + (size_t)g * nq, nq, C, X));
                }
                A.total = A.whole.count + A.whole.nan;
            }
        });
}
// request `which` of the session's last infx_engine_field_quantiles: the whole's figures and the groups', as figures_whole and figures_groups
int32_t infx_engine_field_quantiles_whole(infx_session* S, uint32_t which, infx_quantile_figures* out) {
    return figures_whole(answer_at(S ? &S->qnt.ans : nullptr, which), out, "no such request in the session's last field_quantiles call");
}
int32_t infx_engine_field_quantiles_groups(infx_session* S, uint32_t which, int32_t* group_col, uint32_t* codes, infx_quantile_figures* figures, int32_t cap) {
    return figures_groups(answer_at(S ? &S->qnt.ans : nullptr, which), group_col, codes, figures, cap);
}
int32_t infx_engine_field_quantiles_total(infx_session* S, uint32_t which, uint32_t* total) {
    return answer_total(answer_at(S ? &S->qnt.ans : nullptr, which), total, "no such request in the session's last field_quantiles call");
}
int32_t infx_engine_field_quantiles_error(infx_session* S, uint32_t which, char* out, int32_t cap) { return answer_error(answer_at(S ? &S->qnt.ans : nullptr, which), out, cap); }
int32_t infx_engine_last_field_quantiles_stats(infx_session* S, uint32_t* masks_built, uint32_t* masks_reused, uint32_t* hist_passes, uint32_t* launches) {
    if (!S) return efail(INFX_EINVAL, "null session");
    return put_stats({{masks_built, S->qnt.masks.built}, {masks_reused, S->qnt.masks.reused}, {hist_passes, S->qnt.passes}, {launches, S->qnt.launches}});
}
int32_t infx_engine_last_field_quantiles_placement(infx_session* S, uint32_t* digit_bits, uint32_t* lds_rows, uint32_t* global_rows) {
    if (!S) return efail(INFX_EINVAL, "null session");
    return put_stats({{digit_bits, S->qnt.place[0]}, {lds_rows, S->qnt.place[1]}, {global_rows, S->qnt.place[2]}});
}
int32_t infx_engine_set_quantile_digit_bits(infx_session* S, int32_t bits) {
    if (!S || (bits != 0 && (bits < 4 || bits > 11))) return efail(INFX_EINVAL, "the digit width of field_quantiles is 4 .. 11 bits, or 0: chosen per call");
    S->qntDigitBits = bits;
    return INFX_OK;
}

// ---- list_groups: one row per value of a field — the group's first document in the order of a field — by page (not in the reference) ---------------------
// Per request, as infx_engine_list_documents: the filter through the filter cache, its mask through the session's mask cache, order_by to its column, whose
// sort rank is built on first use; group_by to its column (any kind: the group is the dictionary code).  infx_list_grouped then finds the heads of every
// (mask, group column, order column, direction) once and pages over them; the answers stay on the session for the readers.
extern "C++" {
// The two per-request steps list_groups and list_group_members (`name`) share, for a request R with their common fields.  What needs no device — the page,
// group_by, order_by — wrong: the refusal's message, else "".  Caller holds e->filterMu.
template <class Q> static std::string group_request_problem(infx_engine* e, const char* name, const Q& R) {
    if (const char* bad = page_problem(R.limit, R.offset)) return bad;
    if (!R.group_by) return std::string(name) + " needs a group_by field";
    if (column_named(e, R.group_by) < 0) return std::string(name) + ": no group_by field named '" + R.group_by + "'";
    if (R.order_by && column_named(e, R.order_by) < 0) return std::string(name) + ": no field named '" + R.order_by + "'";
    return "";
}
// its columns and its filter: group_by to *gcol, order_by to *col (its sort rank built on first use), the filter through the filter cache; refusals are F's
template <class F, class Q> static void group_request_resolve(F& call, const char* name, uint32_t i, const Q& R, int32_t* col, int32_t* gcol) {
    std::string why;
    if ((*gcol = column_named(call.S->e, R.group_by)) < 0) return call.refuse(i, INFX_EINVAL, std::string(name) + ": no group_by field named '" + R.group_by + "'");
    const int32_t rc = order_column(call.S->e, name, R.order_by, col, &why);
    if (rc) call.refuse(i, rc, why); else call.filter(i, R.filter);
}
}
int32_t infx_engine_list_groups(infx_session* S, uint32_t nreq, const infx_group_list_request* reqs, int32_t* out_status) {
    std::array<int32_t, INFX_MAX_PREFILTERS> col, gcol; col.fill(-1);
    std::vector<infx_group_list_req> dr; PageRows P; std::vector<uint32_t> gcodes, sizes, groups;
    return set_call(S, &infx_session::grp, "list_groups", "list_groups requests", true, nreq, reqs, out_status,
        [&](auto& F, uint32_t i) { const std::string bad = group_request_problem(S->e, "list_groups", reqs[i]); if (!bad.empty()) F.refuse(i, INFX_EINVAL, bad); },
        [&](auto& F, uint32_t i) { group_request_resolve(F, "list_groups", i, reqs[i], &col[i], &gcol[i]); },
        [&](auto& F) {
            for (uint32_t i : F.who) {
                infx_group_list_req R{};
                R.mask = F.mc.mask(i); R.col = col[i]; R.group_col = gcol[i]; R.ascending = reqs[i].ascending ? 1 : 0; R.offset = reqs[i].offset;
                R.limit = reqs[i].limit; R.digit_bits = (uint32_t)S->lstDigitBits;
                dr.push_back(R);
            }
            P.pages(dr.size());
            gcodes.resize(P.codes.size()); sizes.resize(P.codes.size()); groups.assign(P.counts.size(), 0);
            return infx_list_grouped(S->stream, (uint32_t)dr.size(), dr.data(), P.keys.data(), P.docs.data(), P.codes.data(), gcodes.data(), sizes.data(),
                                     P.counts.data(), groups.data(), P.totals.data());
        },
        [&](auto& F) {
            infx_last_group_list_stats(S->stream, &S->grp.heads, &S->grp.passes, &S->grp.launches);
            for (size_t j = 0; j < dr.size(); j++) {
                GroupListAnswer& A = S->grp.ans[F.who[j]];
                const size_t c = P.take(A, j, dr[j].limit);
                A.totalGroups = groups[j]; page_of(A.gcodes, gcodes, j, c); page_of(A.sizes, sizes, j, c);
            }
        });
}
// request `which` of the session's last infx_engine_list_groups: its page as page_rows, with every row's group code and group size
int32_t infx_engine_group_list_rows(infx_session* S, uint32_t which, int64_t* keys, int32_t* docs, uint32_t* codes, uint32_t* group_codes, uint32_t* sizes, int32_t cap) {
    const GroupListAnswer* A = answer_at(S ? &S->grp.ans : nullptr, which);
    size_t c = 0;
    const int32_t n = page_rows(A, keys, docs, codes, cap, group_codes && sizes, &c);
    if (c) { std::memcpy(group_codes, A->gcodes.data(), c * 4); std::memcpy(sizes, A->sizes.data(), c * 4); }
    return n;
}
// the number of groups with a member and the size of request `which`'s set (0 for a refused one, whose status is returned)
int32_t infx_engine_group_list_totals(infx_session* S, uint32_t which, uint32_t* total_groups, uint32_t* total) {
    const GroupListAnswer* A = answer_at(S ? &S->grp.ans : nullptr, which);
    if (A && total_groups) *total_groups = A->totalGroups;
    return answer_total(total_groups ? A : nullptr, total, "no such request in the session's last list_groups call");
}
int32_t infx_engine_group_list_error(infx_session* S, uint32_t which, char* out, int32_t cap) { return answer_error(answer_at(S ? &S->grp.ans : nullptr, which), out, cap); }
int32_t infx_engine_last_group_list_stats(infx_session* S, uint32_t* masks_built, uint32_t* masks_reused, uint32_t* head_passes, uint32_t* hist_passes, uint32_t* launches) {
    if (!S) return efail(INFX_EINVAL, "null session");
    return put_stats({{masks_built, S->grp.masks.built}, {masks_reused, S->grp.masks.reused}, {head_passes, S->grp.heads}, {hist_passes, S->grp.passes}, {launches, S->grp.launches}});
}

// ---- list_group_members: list_groups' rows, each with the first per_group members of its group (not in the reference) -----------------------------------
// Per request as infx_engine_list_groups, through the same two steps; per_group is checked with the page.  infx_list_group_members then returns every page
// with its rows' members; the answers stay on the session for the readers, the members of a page row after row.
int32_t infx_engine_list_group_members(infx_session* S, uint32_t nreq, const infx_group_members_request* reqs, int32_t* out_status) {
    std::array<int32_t, INFX_MAX_PREFILTERS> col, gcol; col.fill(-1);
    std::vector<infx_group_members_req> dr;
    std::vector<int32_t> rows, mdocs; std::vector<int64_t> mkeys; std::vector<uint32_t> gcodes, sizes, held, mcodes, counts, groups, totals;
    const size_t R = INFX_POST_MAX_ROWS, M = INFX_GROUP_MEMBERS_MAX;
    return set_call(S, &infx_session::mem, "list_group_members", "list_group_members requests", true, nreq, reqs, out_status,
        [&](auto& F, uint32_t i) {
            const std::string bad = group_request_problem(S->e, "list_group_members", reqs[i]);
            if (!bad.empty()) F.refuse(i, INFX_EINVAL, bad);
            else if (reqs[i].per_group < 1 || reqs[i].per_group > INFX_GROUP_MEMBERS_MAX_PER_GROUP) F.refuse(i, INFX_EINVAL, "list_group_members: per_group is 1 .. 16");
            else if ((uint64_t)reqs[i].limit * reqs[i].per_group > INFX_GROUP_MEMBERS_MAX) F.refuse(i, INFX_EINVAL, "list_group_members: limit * per_group is at most 4096");
        },
        [&](auto& F, uint32_t i) { group_request_resolve(F, "list_group_members", i, reqs[i], &col[i], &gcol[i]); },
        [&](auto& F) {
            for (uint32_t i : F.who) {
                infx_group_members_req Q{};
                Q.mask = F.mc.mask(i); Q.col = col[i]; Q.group_col = gcol[i]; Q.ascending = reqs[i].ascending ? 1 : 0; Q.offset = reqs[i].offset;
                Q.limit = reqs[i].limit; Q.digit_bits = (uint32_t)S->lstDigitBits; Q.per_group = reqs[i].per_group;
                dr.push_back(Q);
            }
            const size_t m = std::max<size_t>(dr.size(), 1);
            rows.resize(m * R); gcodes.resize(m * R); sizes.resize(m * R); held.resize(m * R); mkeys.resize(m * M); mdocs.resize(m * M); mcodes.resize(m * M);
            counts.assign(m, 0); groups.assign(m, 0); totals.assign(m, 0);
            return infx_list_group_members(S->stream, (uint32_t)dr.size(), dr.data(), rows.data(), gcodes.data(), sizes.data(), held.data(), mkeys.data(), mdocs.data(),
                                           mcodes.data(), counts.data(), groups.data(), totals.data());
        },
        [&](auto& F) {
            infx_last_group_members_stats(S->stream, &S->mem.heads, &S->mem.passes, &S->mem.walks, &S->mem.launches);
            for (size_t j = 0; j < dr.size(); j++) {
                GroupMembersAnswer& A = S->mem.ans[F.who[j]];
                const size_t c = std::min<size_t>(counts[j], dr[j].limit), pg = dr[j].per_group;
                A.total = totals[j]; A.totalGroups = groups[j]; page_of(A.gcodes, gcodes, j, c); page_of(A.sizes, sizes, j, c); page_of(A.held, held, j, c);
                for (size_t r = 0; r < c; r++) {
                    const size_t at = j * M + r * pg, h = std::min<size_t>(A.held[r], pg);
                    A.keys.insert(A.keys.end(), mkeys.begin() + at, mkeys.begin() + at + h); A.docs.insert(A.docs.end(), mdocs.begin() + at, mdocs.begin() + at + h);
                    A.codes.insert(A.codes.end(), mcodes.begin() + at, mcodes.begin() + at + h);
                }
            }
        });
}
// request `which` of the session's last infx_engine_list_group_members: per row of its page the group's code, its size and the members it carries; returns
// the page's row count, -1 on error (also for a refused request)
int32_t infx_engine_group_members_rows(infx_session* S, uint32_t which, uint32_t* group_codes, uint32_t* sizes, uint32_t* member_counts, int32_t cap) {
    const GroupMembersAnswer* A = answer_at(S ? &S->mem.ans : nullptr, which);
    if (!A || A->status || (cap > 0 && (!group_codes || !sizes || !member_counts))) return -1;
    const size_t c = std::min<size_t>(A->gcodes.size(), (size_t)std::max(cap, 0));
    if (c) { std::memcpy(group_codes, A->gcodes.data(), c * 4); std::memcpy(sizes, A->sizes.data(), c * 4); std::memcpy(member_counts, A->held.data(), c * 4); }
    return (int32_t)A->gcodes.size();
}
// the members of all its rows, row after row, as page_rows: returns the page's member count
int32_t infx_engine_group_members_members(infx_session* S, uint32_t which, int64_t* keys, int32_t* docs, uint32_t* codes, int32_t cap) {
    return page_rows(answer_at(S ? &S->mem.ans : nullptr, which), keys, docs, codes, cap);
}
int32_t infx_engine_group_members_totals(infx_session* S, uint32_t which, uint32_t* total_groups, uint32_t* total) {
    const GroupMembersAnswer* A = answer_at(S ? &S->mem.ans : nullptr, which);
    if (A && total_groups) *total_groups = A->totalGroups;
    return answer_total(total_groups ? A : nullptr, total, "no such request in the session's last list_group_members call");
}
int32_t infx_engine_group_members_error(infx_session* S, uint32_t which, char* out, int32_t cap) { return answer_error(answer_at(S ? &S->mem.ans : nullptr, which), out, cap); }
int32_t infx_engine_last_group_members_stats(infx_session* S, uint32_t* masks_built, uint32_t* masks_reused, uint32_t* head_passes, uint32_t* hist_passes, uint32_t* member_walks, uint32_t* launches) {
    if (!S) return efail(INFX_EINVAL, "null session");
    return put_stats({{masks_built, S->mem.masks.built}, {masks_reused, S->mem.masks.reused}, {head_passes, S->mem.heads}, {hist_passes, S->mem.passes}, {member_walks, S->mem.walks},
                      {launches, S->mem.launches}});
}

// ---- top_groups: the groups of a field ranked by their size or by the count, min, max, sum or mean of a second field, by page (not in the reference) --------
// Per request, as infx_engine_field_stats: the field (if any) to its column, its sort rank and its value table; group_by to its column — any kind, any number
// of values — whose facet tie order (Column.rank) is uploaded on first use; the filter through the filter cache and its mask through the session's mask cache.
// infx_top_groups then accumulates one slot per group code, ranks the slots by order-preserving composites and selects the page; the engine turns the page's
// slots into figures with stats_figures, the reader of infx_engine_field_stats.
static const char* const TOP_BY_NAMES[TS_BYS] = {"size", "count", "min", "max", "sum", "mean"};
// Column col's facet tie order is on the device.  Caller holds e->filterMu.
static int32_t group_rank_on_device(infx_engine* e, uint32_t col) {
    if (e->tieRanked.size() < e->columns.size()) e->tieRanked.resize(e->columns.size(), 0);
    if (e->tieRanked[col]) return INFX_OK;
    const filt::Column& c = e->columns[col];
    int32_t rc = infx_upload_group_rank(e->dev, col, (uint32_t)c.rank.size(), c.rank.data());
    if (rc) { g_eerr = infx_last_error(); return rc; }
    e->tieRanked[col] = 1;
    return INFX_OK;
}
int32_t infx_engine_top_groups(infx_session* S, uint32_t nreq, const infx_top_request* reqs, int32_t* out_status) {
    std::array<int32_t, INFX_MAX_PREFILTERS> col, gcol, by; col.fill(-1); gcol.fill(-1); by.fill(-1);
    std::vector<infx_top_req> dr; std::vector<uint32_t> codes, counts, groups, totals; std::vector<infx_stats_slot> slots;
    return set_call(S, &infx_session::top, "top_groups", "top_groups requests", true, nreq, reqs, out_status,
        [&](auto& F, uint32_t i) {
            const infx_top_request& Q = reqs[i];
            if (const char* bad = page_problem(Q.limit, Q.offset)) return F.refuse(i, INFX_EINVAL, bad);
            if (!Q.group_by) return F.refuse(i, INFX_EINVAL, "top_groups needs a group_by field");
            if ((gcol[i] = column_named(S->e, Q.group_by)) < 0) return F.refuse(i, INFX_EINVAL, std::string("top_groups: no group_by field named '") + Q.group_by + "'");
            for (int b = 0; Q.by && b < TS_BYS; b++) if (!std::strcmp(Q.by, TOP_BY_NAMES[b])) by[i] = b;
            if (by[i] < 0) return F.refuse(i, INFX_EINVAL, std::string("top_groups: by is one of size, count, min, max, sum, mean, not '") + (Q.by ? Q.by : "") + "'");
            if (!Q.field) {
                if (by[i] != INFX_TOP_BY_SIZE) F.refuse(i, INFX_EINVAL, std::string("top_groups: by = '") + Q.by + "' needs a field");
                return;
            }
            std::string why; int32_t g = -1;
            int32_t rc = numeric_field_check(S->e, "top_groups", "figures", Q.field, nullptr, &col[i], &g, &why);
            if (!rc && !stats_index(S->e, (uint32_t)col[i]).summable) {
                rc = INFX_EINVAL;
                why = std::string("top_groups: the finite values of field '") + Q.field + "' span more than 128 binary digits; they cannot be summed exactly";
            }
            if (rc) F.refuse(i, rc, why);
        },
        [&](auto& F, uint32_t i) {
            infx_engine* e = S->e;
            if (col[i] >= 0) {
                const infx_engine::RangeIndex* X = nullptr;
                { const int32_t rc = range_index(e, (uint32_t)col[i], &X); if (rc) return F.refuse(i, rc, g_eerr); }      // (the sort rank, for min / max)
                infx_engine::StatsIndex& V = stats_index(e, (uint32_t)col[i]);
                if (!V.uploaded) {
                    const int32_t rc = infx_upload_column_values(e->dev, (uint32_t)col[i], (uint32_t)V.bits.size(), V.bits.data(), V.kind, V.sc.scale, V.sc.nlimbs);
                    if (rc) return F.refuse(i, rc, infx_last_error());
                    V.uploaded = true;
                }
            }
            { const int32_t rc = group_rank_on_device(e, (uint32_t)gcol[i]); if (rc) return F.refuse(i, rc, g_eerr); }
            F.filter(i, reqs[i].filter);
        },
        [&](auto& F) {
            for (uint32_t i : F.who) {
                infx_top_req R{};
                R.mask = F.mc.mask(i); R.col = col[i]; R.group_col = gcol[i]; R.by = (uint32_t)by[i]; R.ascending = reqs[i].ascending ? 1 : 0;
                R.offset = reqs[i].offset; R.limit = reqs[i].limit; R.digit_bits = (uint32_t)S->lstDigitBits;
                dr.push_back(R);
            }
            const size_t m = std::max<size_t>(dr.size(), 1);
            codes.assign(m * INFX_POST_MAX_ROWS, 0); slots.assign(m * INFX_POST_MAX_ROWS, infx_stats_slot()); counts.assign(m, 0); groups.assign(m, 0); totals.assign(m, 0);
            return infx_top_groups(S->stream, (uint32_t)dr.size(), dr.data(), codes.data(), slots.data(), counts.data(), groups.data(), totals.data());
        },
        [&](auto& F) {
            infx_engine* e = S->e;
            infx_last_top_groups_info(S->stream, nullptr, &S->top.accumulates, &S->top.passes, &S->top.launches, &S->top.place[0], &S->top.place[1], &S->top.place[2]);
            std::lock_guard<std::mutex> lk(e->filterMu);
            for (size_t j = 0; j < dr.size(); j++) {
                TopAnswer& A = S->top.ans[F.who[j]];
                const size_t c = std::min<size_t>(counts[j], dr[j].limit), at = j * INFX_POST_MAX_ROWS;
                A.total = totals[j]; A.totalGroups = groups[j]; A.groupCol = dr[j].group_col; A.hasField = dr[j].col >= 0;
                A.codes.assign(codes.begin() + at, codes.begin() + at + c);
                for (size_t r = 0; r < c; r++) {
                    const infx_stats_slot& sl = slots[at + r];
                    A.sizes.push_back(sl.finite + sl.nan + sl.pinf + sl.ninf);
                    A.figures.push_back(A.hasField ? stats_figures(sl, e->statsIndex[dr[j].col], e->columns[dr[j].col], e->rangeIndex[dr[j].col]) : infx_stats_figures());
                }
            }
        });
}
// request `which` of the session's last infx_engine_top_groups: up to cap rows — the group's code in column *group_col, its members, its figures (kind 0
// throughout a request without a field); returns the page's row count, -1 on error (also for a refused request)
int32_t infx_engine_top_groups_rows(infx_session* S, uint32_t which, int32_t* group_col, uint32_t* codes, uint32_t* sizes, infx_stats_figures* figures, int32_t cap) {
    const TopAnswer* A = answer_at(S ? &S->top.ans : nullptr, which);
    if (!A || A->status || (cap > 0 && (!codes || !sizes || !figures))) return -1;
    const size_t c = std::min<size_t>(A->codes.size(), (size_t)std::max(cap, 0));
    if (c) { std::memcpy(codes, A->codes.data(), c * 4); std::memcpy(sizes, A->sizes.data(), c * 4); std::memcpy(figures, A->figures.data(), c * sizeof(infx_stats_figures)); }
    if (group_col) *group_col = A->groupCol;
    return (int32_t)A->codes.size();
}
// the number of groups with a member and the size of request `which`'s set (0 for a refused one, whose status is returned)
int32_t infx_engine_top_groups_totals(infx_session* S, uint32_t which, uint32_t* total_groups, uint32_t* total) {
    const TopAnswer* A = answer_at(S ? &S->top.ans : nullptr, which);
    if (A && total_groups) *total_groups = A->totalGroups;
    return answer_total(total_groups ? A : nullptr, total, "no such request in the session's last top_groups call");
}
int32_t infx_engine_top_groups_error(infx_session* S, uint32_t which, char* out, int32_t cap) { return answer_error(answer_at(S ? &S->top.ans : nullptr, which), out, cap); }
int32_t infx_engine_last_top_groups_stats(infx_session* S, uint32_t* masks_built, uint32_t* masks_reused, uint32_t* accumulate_passes, uint32_t* select_passes, uint32_t* launches) {
    if (!S) return efail(INFX_EINVAL, "null session");
    return put_stats({{masks_built, S->top.masks.built}, {masks_reused, S->top.masks.reused}, {accumulate_passes, S->top.accumulates}, {select_passes, S->top.passes}, {launches, S->top.launches}});
}
int32_t infx_engine_last_top_groups_placement(infx_session* S, uint32_t* small_lds, uint32_t* big_lds, uint32_t* in_global) {
    if (!S) return efail(INFX_EINVAL, "null session");
    return put_stats({{small_lds, S->top.place[0]}, {big_lds, S->top.place[1]}, {in_global, S->top.place[2]}});
}

// ---- field_distinct: the exact number of distinct values of a field over the documents a filter accepts, whole and per group (not in the reference) --------
// Per request: the field to its column — any kind, any number of values; nothing of it but its codes is needed — group_by as infx_engine_field_stats checks
// it, the filter through the filter cache and its mask through the session's mask cache.  infx_field_distinct marks the (group code, field code) pairs of the
// set and counts them; the engine orders the groups with a member as field_stats does.
int32_t infx_engine_field_distinct(infx_session* S, uint32_t nreq, const infx_distinct_request* reqs, int32_t* out_status) {
    std::array<int32_t, INFX_MAX_PREFILTERS> col, gcol; col.fill(-1); gcol.fill(-1);
    std::vector<infx_distinct_req> dr; std::vector<uint32_t> distinct, totals, gsizes, gdistinct;
    return set_call(S, &infx_session::dst, "field_distinct", "field_distinct requests", true, nreq, reqs, out_status,
        [&](auto& F, uint32_t i) {
            const infx_distinct_request& Q = reqs[i];
            if (!Q.field) return F.refuse(i, INFX_EINVAL, "field_distinct needs a field");
            if ((col[i] = column_named(S->e, Q.field)) < 0) return F.refuse(i, INFX_EINVAL, std::string("field_distinct: no field named '") + Q.field + "'");
            std::string why;
            const int32_t rc = group_by_check(S->e, "field_distinct", Q.group_by, &gcol[i], &why);
            if (rc) F.refuse(i, rc, why);
        },
        [&](auto& F, uint32_t i) { F.filter(i, reqs[i].filter); },
        [&](auto& F) {
            for (uint32_t i : F.who) {
                infx_distinct_req R{};
                R.mask = F.mc.mask(i); R.col = col[i]; R.group_col = gcol[i]; R.placement = (uint32_t)S->dstPlacement;
                dr.push_back(R);
            }
            const size_t m = std::max<size_t>(dr.size(), 1);
            distinct.assign(m, 0); totals.assign(m, 0); gsizes.assign(m * INFX_STATS_MAX_GROUPS, 0); gdistinct.assign(m * INFX_STATS_MAX_GROUPS, 0);
            return infx_field_distinct(S->stream, (uint32_t)dr.size(), dr.data(), distinct.data(), totals.data(), gsizes.data(), gdistinct.data());
        },
        [&](auto& F) {
            infx_engine* e = S->e;
            infx_last_field_distinct_info(S->stream, nullptr, &S->dst.launches, &S->dst.place[0], &S->dst.place[1], &S->dst.place[2]);
            std::lock_guard<std::mutex> lk(e->filterMu);
            for (size_t j = 0; j < dr.size(); j++) {
                DistinctAnswer& A = S->dst.ans[F.who[j]];
                A.groupCol = dr[j].group_col; A.total = totals[j]; A.whole.size = totals[j]; A.whole.distinct = distinct[j];
                if (A.groupCol < 0) continue;
                const uint32_t *sz = gsizes.data() + j * INFX_STATS_MAX_GROUPS, *dc = gdistinct.data() + j * INFX_STATS_MAX_GROUPS;
                A.codes = groups_in_order(e->columns[A.groupCol], [&](uint32_t g) { return (uint64_t)sz[g]; });
                for (uint32_t g : A.codes) A.groups.push_back(infx_distinct_figures{sz[g], dc[g]});
            }
        });
}
// request `which` of the session's last infx_engine_field_distinct: the whole's figures and the groups', as figures_whole and figures_groups
int32_t infx_engine_field_distinct_whole(infx_session* S, uint32_t which, infx_distinct_figures* out) {
    return figures_whole(answer_at(S ? &S->dst.ans : nullptr, which), out, "no such request in the session's last field_distinct call");
}
int32_t infx_engine_field_distinct_groups(infx_session* S, uint32_t which, int32_t* group_col, uint32_t* codes, infx_distinct_figures* figures, int32_t cap) {
    return figures_groups(answer_at(S ? &S->dst.ans : nullptr, which), group_col, codes, figures, cap);
}
// the size of request `which`'s set (0 for a refused one, whose status is returned)
int32_t infx_engine_field_distinct_total(infx_session* S, uint32_t which, uint32_t* total) {
    return answer_total(answer_at(S ? &S->dst.ans : nullptr, which), total, "no such request in the session's last field_distinct call");
}
int32_t infx_engine_field_distinct_error(infx_session* S, uint32_t which, char* out, int32_t cap) { return answer_error(answer_at(S ? &S->dst.ans : nullptr, which), out, cap); }
int32_t infx_engine_last_field_distinct_stats(infx_session* S, uint32_t* masks_built, uint32_t* masks_reused, uint32_t* lds_passes, uint32_t* bitmap_passes, uint32_t* hash_passes, uint32_t* launches) {
    if (!S) return efail(INFX_EINVAL, "null session");
    return put_stats({{masks_built, S->dst.masks.built}, {masks_reused, S->dst.masks.reused}, {lds_passes, S->dst.place[0]}, {bitmap_passes, S->dst.place[1]}, {hash_passes, S->dst.place[2]}, {launches, S->dst.launches}});
}
int32_t infx_engine_set_distinct_placement(infx_session* S, int32_t mode) {
    if (!S || mode < 0 || mode > 3) return efail(INFX_EINVAL, "a distinct placement is 0 (automatic), 1 (LDS), 2 (global bitmap) or 3 (hash set)");
    S->dstPlacement = mode;
    return INFX_OK;
}

int32_t infx_engine_set_filter_cache_limit(infx_engine* e, uint64_t limit) {
    if (!e || limit < 1) return efail(INFX_EINVAL, "bad arguments");
    std::lock_guard<std::mutex> lk(e->filterMu);
    e->filterCacheLimit = (size_t)limit; e->evict_filters();
    return INFX_OK;
}
int64_t infx_engine_filter_cache_size(infx_engine* e) { if (!e) return -1; std::lock_guard<std::mutex> lk(e->filterMu); return (int64_t)e->filters.size(); }

} // extern "C"
